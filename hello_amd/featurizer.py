"""Pileup-tensor producer on the GPU.

The reference turns the reads supporting each allele of a site into ``uint8 [reads, L, 6|7]`` colour
tensors in C++ (``AlleleSearcherLite.computeFeatures`` -> ``libCallability``'s
``computeFeaturesColoredSimple``, reference python/AlleleSearcherLite.py:232-251,
c++/src/AlleleSearcherLiteFiltered.cpp:1031-1180), one allele at a time on one CPU thread.  Here every read
of every allele of every site of a batch is encoded in ONE launch (``hello_engine_featurize``) straight
into the packed ``[sum R, L, C]`` buffer + reads-per-allele / alleles-per-site counts the scoring engine
consumes, so featurisation and scoring can stay on the device.

Read collection (BAM access, allele assembly, read -> allele support) remains the caller's job; this
module takes what ``AlleleSearcherLite`` holds per read: bases, base qualities, CIGAR tuples, reference
start, mapping quality, orientation, haplotag (python/AlleleSearcherLite.py:159-174).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .engine import HELLO_IN_DEVICE, HELLO_OUT_DEVICE, Engine, _check


@dataclass
class AlignedRead:
    bases: str
    quals: Sequence[int]
    cigar: Sequence[Tuple[int, int]]          # pysam-style (operation, length) tuples
    ref_start: int
    mapq: int = 40
    orientation: int = 1                      # > 0 forward strand
    hp: int = 0                               # haplotag 0 | 1 | 2


@dataclass
class SiteReads:
    reference: str                            # reference window
    window_start: int                         # genome position of reference[0]
    assembly_start: int                       # allele span [start, stop) in genome coordinates
    assembly_stop: int
    alleles: List[Tuple[str, List[AlignedRead]]] = field(default_factory=list)   # (allele, supporting reads)


def pack_sites(sites: Sequence[SiteReads]):
    """Flatten sites -> the arrays of hello_engine_featurize + the batch's count arrays.  An allele without
    supporting reads contributes one read with an empty CIGAR: the all-zero dummy row of the reference
    (AlleleSearcherLiteFiltered.cpp:1037-1043)."""
    bases, quals, cigars = [], [], []
    read_off, cigar_off = [0], [0]
    ref_start, mapq, orient, hp, site_of_read = [], [], [], [], []
    ref, ref_off, wstart, a0, a1 = [], [0], [], [], []
    reads_per_allele, alleles_per_site = [], []
    for s, site in enumerate(sites):
        ref.append(site.reference.encode("ascii"))
        ref_off.append(ref_off[-1] + len(site.reference))
        wstart.append(site.window_start)
        a0.append(site.assembly_start)
        a1.append(site.assembly_stop)
        alleles_per_site.append(len(site.alleles))
        for _, reads in site.alleles:
            group = reads if reads else [AlignedRead("", [], [], 0)]
            reads_per_allele.append(len(group))
            for rd in group:
                assert len(rd.bases) == len(rd.quals)
                bases.append(rd.bases.encode("ascii"))
                quals.append(bytes(bytearray(int(q) & 0xFF for q in rd.quals)))
                read_off.append(read_off[-1] + len(rd.bases))
                for op, length in rd.cigar:
                    cigars.append((int(length) << 4) | int(op))
                cigar_off.append(cigar_off[-1] + len(rd.cigar))
                ref_start.append(rd.ref_start)
                mapq.append(min(int(rd.mapq), 255))
                orient.append(1 if rd.orientation > 0 else -1)
                hp.append(int(rd.hp))
                site_of_read.append(s)
    u8 = lambda b: np.frombuffer(b"".join(b) + b"\0", dtype=np.uint8).copy()      # noqa: E731 (never empty)
    return dict(
        bases=u8(bases), quals=u8(quals), read_off=np.asarray(read_off, np.int64),
        cigars=np.asarray(cigars + [0], np.uint32), cigar_off=np.asarray(cigar_off, np.int64),
        ref_start=np.asarray(ref_start, np.int64), mapq=np.asarray(mapq, np.uint8),
        orientation=np.asarray(orient, np.int8), hp=np.asarray(hp, np.uint8),
        site_of_read=np.asarray(site_of_read, np.int32), ref=u8(ref), ref_off=np.asarray(ref_off, np.int64),
        window_start=np.asarray(wstart, np.int64), asm_start=np.asarray(a0, np.int64),
        asm_stop=np.asarray(a1, np.int64),
        reads_per_allele=np.asarray(reads_per_allele, np.int32),
        alleles_per_site=np.asarray(alleles_per_site, np.int32))


def featurize(engine: Engine, sites: Sequence[SiteReads], feature_length: int = 150, include_hp: bool = False,
              device_output: bool = False):
    """-> (pileups uint8 [sum R, L, C], reads_per_allele int32 [A], alleles_per_site int32 [S]).  With
    ``device_output`` the pileups are a torch CUDA tensor that can go straight into ``Engine.forward``."""
    # ``sites``: SiteReads objects, or the already flat arrays of ``pack_sites`` (shards.PackedShard.featurizer_arrays)
    p = sites if isinstance(sites, dict) else pack_sites(sites)
    n_reads, n_sites = int(p["site_of_read"].shape[0]), int(p["alleles_per_site"].shape[0])
    channels = 7 if include_hp else 6
    flags = 0
    if device_output:
        import torch
        out = torch.empty((n_reads, feature_length, channels), dtype=torch.uint8, device=f"cuda:{engine.device}")
        out_ptr, stream = out.data_ptr(), None
        flags |= HELLO_OUT_DEVICE
    else:
        out = np.empty((n_reads, feature_length, channels), dtype=np.uint8)
        out_ptr, stream = out.ctypes.data, None
    fn = engine.lib.hello_engine_featurize
    fn.restype = C.c_int
    vp = C.c_void_p
    fn.argtypes = [vp] * 16 + [C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, vp]
    ptr = lambda k: p[k].ctypes.data                                              # noqa: E731
    def launch(handle):
        _check(fn(engine.handle, ptr("bases"), ptr("quals"), ptr("read_off"), ptr("cigars"), ptr("cigar_off"),
                  ptr("ref_start"), ptr("mapq"), ptr("orientation"), ptr("hp"), ptr("site_of_read"), ptr("ref"),
                  ptr("ref_off"), ptr("window_start"), ptr("asm_start"), ptr("asm_stop"),
                  n_reads, n_sites, feature_length, channels, out_ptr, flags, handle))
    if device_output:
        with engine.on_stream(out.device) as handle:      # ordered with the caller's current torch stream
            launch(handle)
    else:
        launch(None)
    return out, p["reads_per_allele"], p["alleles_per_site"]


FEATURIZE_ARRAYS = ("bases", "quals", "read_off", "cigars", "cigar_off", "ref_start", "mapq", "orientation", "hp", "site_of_read",
                    "ref", "ref_off", "window_start", "asm_start", "asm_stop")          # hello_engine_featurize's order


def featurize_device(engine: Engine, pointers: dict, n_reads: int, n_sites: int, feature_length: int, channels: int,
                     out_pointer: int, stream: int):
    """``hello_engine_featurize`` on arrays ALREADY in device memory (``pointers``: name of FEATURIZE_ARRAYS -> device
    address), asynchronous on ``stream`` -- the staged form the shard pipeline uses (one H2D copy per launch carries all
    fifteen arrays)."""
    fn = engine.lib.hello_engine_featurize
    fn.restype = C.c_int
    vp = C.c_void_p
    fn.argtypes = [vp] * 16 + [C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, vp]
    _check(fn(engine.handle, *[pointers[k] for k in FEATURIZE_ARRAYS], n_reads, n_sites, feature_length, channels,
              out_pointer, HELLO_IN_DEVICE | HELLO_OUT_DEVICE, stream))


# ---------------------------------------------------------------------------------------------------------------------
# per-allele read support (hello_engine_allele_support, hello_amd/csrc/support.hip)
# ---------------------------------------------------------------------------------------------------------------------
SUPPORT_ARRAYS = ("cigar_off", "mapq", "orientation", "allele_off")                   # hello_engine_allele_support's order
SUPPORT_DTYPES = dict(cigar_off=np.int64, mapq=np.uint8, orientation=np.int8, allele_off=np.int64)


def _support_fn(engine: Engine):
    fn = getattr(engine.lib, "hello_engine_allele_support", None)
    if fn is None:
        raise RuntimeError("this libhello_mi355x.so has no hello_engine_allele_support: rebuild it (`make -C hello_amd/csrc`)")
    return fn


def allele_offsets(reads_per_allele) -> np.ndarray:
    """int64 [A + 1]: the exclusive scan of the ``reads_per_allele`` the engine receives (dummy reads count as 1)."""
    off = np.zeros(int(np.shape(reads_per_allele)[0]) + 1, np.int64)
    np.cumsum(reads_per_allele, dtype=np.int64, out=off[1:])
    return off


def allele_support(engine: Engine, cigar_off, mapq, orientation, allele_off, device: bool = False):
    """Per allele, over its reads with at least one CIGAR operation: [reads, forward reads, sum mapq, sum mapq^2], int64 [A, 4].
    Host form: NumPy arrays in, a NumPy array out (staged through device memory, synchronous).  ``device``: the four arrays
    are copied to the engine's GPU first and the call takes device pointers, ordered with the caller's current torch stream;
    -> a torch CUDA tensor."""
    fn = _support_fn(engine)
    given = dict(cigar_off=cigar_off, mapq=mapq, orientation=orientation, allele_off=allele_off)
    host = {k: np.ascontiguousarray(given[k], dtype=SUPPORT_DTYPES[k]) for k in SUPPORT_ARRAYS}
    n_reads, n_alleles = int(host["mapq"].shape[0]), int(host["allele_off"].shape[0]) - 1
    if host["cigar_off"].shape[0] != n_reads + 1 or host["orientation"].shape[0] != n_reads or n_alleles < 0:
        raise ValueError("cigar_off [R + 1], mapq [R], orientation [R] and allele_off [A + 1] do not fit each other")
    pad = lambda a: a if a.shape[0] else np.zeros(1, a.dtype)                           # noqa: E731 (a pointer is taken of each)
    if not device:
        out = np.zeros(4 * max(n_alleles, 1), np.int64)
        held = {k: pad(v) for k, v in host.items()}
        _check(fn(engine.handle, *[held[k].ctypes.data for k in SUPPORT_ARRAYS], n_reads, n_alleles, out.ctypes.data, 0, None))
        return out[:4 * n_alleles].reshape(n_alleles, 4)
    import torch
    where = torch.device(f"cuda:{engine.device}")
    dev = {k: torch.from_numpy(pad(v)).to(where) for k, v in host.items()}
    out = torch.zeros(4 * max(n_alleles, 1), dtype=torch.int64, device=where)
    with engine.on_stream(where) as handle:
        allele_support_device(engine, {k: dev[k].data_ptr() for k in SUPPORT_ARRAYS}, n_reads, n_alleles, out.data_ptr(), handle)
    return out[:4 * n_alleles].view(n_alleles, 4)


def allele_support_device(engine: Engine, pointers: dict, n_reads: int, n_alleles: int, out_pointer: int, stream):
    """``hello_engine_allele_support`` on arrays ALREADY in device memory (``pointers``: name of SUPPORT_ARRAYS -> device
    address), asynchronous on ``stream``: what the shard pipeline launches behind each technology's featurizer."""
    _check(_support_fn(engine)(engine.handle, *[pointers[k] for k in SUPPORT_ARRAYS], n_reads, n_alleles, out_pointer,
                               HELLO_IN_DEVICE | HELLO_OUT_DEVICE, stream))


# ---------------------------------------------------------------------------------------------------------------------
# per-allele base-level read evidence (hello_engine_allele_evidence, hello_amd/csrc/evidence.hip)
# ---------------------------------------------------------------------------------------------------------------------
EVIDENCE_ARRAYS = ("quals", "read_off", "cigars", "cigar_off", "ref_start", "hp", "site_of_read", "asm_start", "asm_stop",
                   "allele_off")                                                        # hello_engine_allele_evidence's order
EVIDENCE_DTYPES = dict(quals=np.uint8, read_off=np.int64, cigars=np.uint32, cigar_off=np.int64, ref_start=np.int64, hp=np.uint8,
                       site_of_read=np.int32, asm_start=np.int64, asm_stop=np.int64, allele_off=np.int64)


def _evidence_fn(engine: Engine):
    fn = getattr(engine.lib, "hello_engine_allele_evidence", None)
    if fn is None:
        raise RuntimeError("this libhello_mi355x.so has no hello_engine_allele_evidence: rebuild it (`make -C hello_amd/csrc`)")
    return fn


def allele_evidence(engine: Engine, arrays: dict, allele_off=None, device: bool = False):
    """Per allele, over its reads with at least one CIGAR operation: [reads with a base inside the site's span, sum of their
    lowest such quality, sum of their distance to the nearer read end, reads with hp == 1, reads with hp == 2, reads stopped
    by the guard], int64 [A, 6] (include/hello_mi355x.h states the walk).  ``arrays``: the featurizer's arrays by name
    (``pack_sites``) with ``allele_off`` among them or given.  Host form: NumPy in, NumPy out (staged, synchronous);
    ``device``: the arrays are copied to the engine's GPU first and the call takes device pointers, ordered with the caller's
    current torch stream; -> a torch CUDA tensor."""
    fn = _evidence_fn(engine)
    given = dict(arrays)
    if allele_off is not None:
        given["allele_off"] = allele_off
    host = {k: np.ascontiguousarray(given[k], dtype=EVIDENCE_DTYPES[k]) for k in EVIDENCE_ARRAYS}
    n_reads, n_sites, n_alleles = int(host["ref_start"].shape[0]), int(host["asm_start"].shape[0]), int(host["allele_off"].shape[0]) - 1
    if (host["read_off"].shape[0] != n_reads + 1 or host["cigar_off"].shape[0] != n_reads + 1 or host["hp"].shape[0] != n_reads
            or host["site_of_read"].shape[0] != n_reads or host["asm_stop"].shape[0] != n_sites or n_alleles < 0
            or host["quals"].shape[0] < int(host["read_off"][-1]) or host["cigars"].shape[0] < int(host["cigar_off"][-1])):
        raise ValueError("the per-read arrays [R] / [R + 1], the site arrays [S], allele_off [A + 1], quals and cigars do not fit "
                         "each other")
    pad = lambda a: a if a.shape[0] else np.zeros(1, a.dtype)                           # noqa: E731 (a pointer is taken of each)
    if not device:
        out = np.zeros(6 * max(n_alleles, 1), np.int64)
        held = {k: pad(v) for k, v in host.items()}
        _check(fn(engine.handle, *[held[k].ctypes.data for k in EVIDENCE_ARRAYS], n_reads, n_sites, n_alleles, out.ctypes.data, 0,
                  None))
        return out[:6 * n_alleles].reshape(n_alleles, 6)
    import torch
    where = torch.device(f"cuda:{engine.device}")
    dev = {k: torch.from_numpy(pad(v)).to(where) for k, v in host.items()}
    out = torch.zeros(6 * max(n_alleles, 1), dtype=torch.int64, device=where)
    with engine.on_stream(where) as handle:
        allele_evidence_device(engine, {k: dev[k].data_ptr() for k in EVIDENCE_ARRAYS}, n_reads, n_sites, n_alleles, out.data_ptr(),
                               handle)
    return out[:6 * n_alleles].view(n_alleles, 6)


def allele_evidence_device(engine: Engine, pointers: dict, n_reads: int, n_sites: int, n_alleles: int, out_pointer: int, stream):
    """``hello_engine_allele_evidence`` on arrays ALREADY in device memory (``pointers``: name of EVIDENCE_ARRAYS -> device
    address), asynchronous on ``stream``: what the shard pipeline launches behind each technology's support kernel."""
    _check(_evidence_fn(engine)(engine.handle, *[pointers[k] for k in EVIDENCE_ARRAYS], n_reads, n_sites, n_alleles, out_pointer,
                                HELLO_IN_DEVICE | HELLO_OUT_DEVICE, stream))
