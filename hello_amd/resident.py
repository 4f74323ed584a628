"""Candidate sites whose reads stay on the GPU: the hand-over from the candidate stage to the scoring loop without shard files.

``candidates.find_sites(..., resident=True)`` (and ``find_candidates``, ``pacbio.find_pacbio_candidates``,
``hybrid.find_hybrid_candidates``) call the library with ``HELLO_CANDIDATES_RESIDENT`` and return a ``ResidentShard``: the
site-level arrays of a ``PackedShard`` on the host (what the record stage and the launch's small staging arrays need), the
per-allele read counts, and the live ``hello_candidates`` handle that owns the pass-2 reads and the gather tables in device
memory.  ``shard_pipeline.ShardScorer.submit`` lays a launch's block out on the device from ``featurizer_counts`` and has
``gather`` (``hello_candidates_gather``: one launch of ``gather_reads_kernel``) write every per-read array where a file
shard's arrays would have been copied to; the handle is released when the launch that read it has finished.
include/hello_mi355x.h states the contract, DESIGN.md 7c the measurements.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from ._abi import bind, check, i32, i64, vp
from .shards import SiteShard

HELLO_CANDIDATES_RESIDENT = 64
GATHER_ARRAYS = ("bases", "quals", "read_off", "cigars", "cigar_off", "ref_start", "mapq", "orientation", "hp", "site_of_read")
NOT_WRITABLE = ("a resident shard keeps its reads on the GPU and cannot be written as a .hshard file or read as host arrays: build "
                "the candidates without resident=True for that")

_PROTOTYPES = (
    ("hello_candidates_featurizer_counts", [vp, i32] + [C.POINTER(i64)] * 3),
    ("hello_candidates_gather", [vp, i32] + [vp] * 10 + [i64] * 4 + [vp]),
    ("hello_candidates_gather_table", [vp, i64, vp, vp, i64, vp, vp, vp, C.POINTER(i64)]),
    ("hello_candidates_free", [vp], None),
)


def _lib():
    return bind(_PROTOTYPES)


def gather_table(reads_per_allele: Sequence[int], read_off: Sequence[int], cigar_off: Sequence[int]) -> Dict[str, np.ndarray]:
    """The host half of the library's gather table (``hello_candidates_gather_table``) for one technology's counts and the
    offsets of its supporting reads: ``source`` (per featurizer read the supporting read, -1 = the dummy read of an allele
    without reads) and the exclusive scans ``read_off`` / ``cigar_off`` of the featurizer reads' base and CIGAR counts."""
    lib = _lib()
    counts = np.ascontiguousarray(reads_per_allele, np.int32)
    read_off, cigar_off = np.ascontiguousarray(read_off, np.int64), np.ascontiguousarray(cigar_off, np.int64)
    real = int(np.maximum(counts, 0).sum())
    if read_off.shape[0] != real + 1 or cigar_off.shape[0] != real + 1:
        raise ValueError(f"read_off and cigar_off must hold {real + 1} offsets for {real} supporting reads")
    n = C.c_int64()
    check(lib.hello_candidates_gather_table(counts.ctypes.data, counts.shape[0], read_off.ctypes.data, cigar_off.ctypes.data, 0,
                                            None, None, None, C.byref(n)), value_error_on_arg=True)
    k = int(n.value)
    source, out_read, out_cigar = np.zeros(k, np.int64), np.zeros(k + 1, np.int64), np.zeros(k + 1, np.int64)
    check(lib.hello_candidates_gather_table(counts.ctypes.data, counts.shape[0], read_off.ctypes.data, cigar_off.ctypes.data, k,
                                            source.ctypes.data, out_read.ctypes.data, out_cigar.ctypes.data, C.byref(n)),
          value_error_on_arg=True)
    return dict(source=source, read_off=out_read, cigar_off=out_cigar)


class ResidentShard(SiteShard):
    """The sites of one candidate call with the reads left on the GPU.  ``arrays``: the site arrays and chromosome table of a
    ``PackedShard`` plus ``reads_per_allele<t>`` per technology.  Owns ``handle`` until ``close()`` (also a context manager)."""

    def __init__(self, handle: int, arrays: dict, feature_length: int = 150, hybrid: bool = False):
        self._lib = _lib()
        self.handle: Optional[int] = handle
        self.hybrid = bool(hybrid)
        try:
            self._init_sites(arrays, feature_length)
            self.validate_sites(feature_length)
            self.counts = [self.validate_counts(arrays[f"reads_per_allele{t}"], t) for t in ((0, 1) if hybrid else (0,))]
            self._sizes = [self._featurizer_counts(t) for t in range(len(self.counts))]
            for t, counts in enumerate(self.counts):
                if self._sizes[t][0] != int(np.maximum(counts, 1).sum()):
                    self._bad(f"the library counts {self._sizes[t][0]} reads of technology {t}, reads_per_allele{t} "
                              f"{int(np.maximum(counts, 1).sum())}")
        except BaseException:
            self.close()
            raise

    # -- what a PackedShard answers -------------------------------------------------------------------------------
    @property
    def z(self):
        raise ValueError(NOT_WRITABLE)

    def has_reads(self, tech: int) -> bool:
        return tech < len(self.counts)

    def n_reads(self, tech: int = 0) -> int:
        """Reads the featurizer will write for technology ``tech`` (dummy reads of unsupported alleles included)."""
        return self._sizes[tech][0] if self.has_reads(tech) else 0

    def reads_per_allele(self, tech: int) -> np.ndarray:
        """The counts as the engine wants them: max(count, 1), int32."""
        return np.maximum(self.counts[tech], 1).astype(np.int32)

    def featurizer_counts(self, tech: int) -> Tuple[int, int, int]:
        """(reads, bases, CIGAR words) of technology ``tech``'s featurizer input, dummy reads included."""
        return self._sizes[tech]

    def _featurizer_counts(self, tech: int) -> Tuple[int, int, int]:
        n = [C.c_int64(), C.c_int64(), C.c_int64()]
        check(self._lib.hello_candidates_featurizer_counts(self.handle, tech, *[C.byref(x) for x in n]), value_error_on_arg=True)
        return tuple(int(x.value) for x in n)

    # -- the device side --------------------------------------------------------------------------------------------
    def gather(self, tech: int, pointers: Dict[str, int], read_shift: int = 0, base_shift: int = 0, cigar_shift: int = 0,
               site_shift: int = 0, stream: int = 0) -> None:
        """Enqueue the gather of technology ``tech`` on ``stream`` into the device arrays ``pointers`` (name of GATHER_ARRAYS ->
        address).  The shard must stay open until the stream has passed the launch."""
        if self.handle is None:
            raise ValueError("this resident shard is closed: its device memory was released")
        check(self._lib.hello_candidates_gather(self.handle, tech, *[pointers[k] for k in GATHER_ARRAYS], int(read_shift),
                                                int(base_shift), int(cigar_shift), int(site_shift), stream or None),
              value_error_on_arg=True)

    def close(self) -> None:
        if getattr(self, "handle", None) is not None:
            self._lib.hello_candidates_free(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:                                   # noqa: BLE001 -- interpreter shutdown
            pass
