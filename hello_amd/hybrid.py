"""Candidate sites of an Illumina BAM and a PacBio BAM together on the GPU: the hybrid caller's stage between
``hello_amd.hotspots`` (two BAMs, ``--hybrid_hotspot``) and the scoring driver with a two-technology model.

``python -m hello_amd.hybrid --bam I,P --ref F --activity shardN.txt --outputPrefix P [--hybrid_hotspot] [--reconcilement_size N]``
does what the reference's python/caller_calling.py does up to its featurizer (:784-843) when it is given both BAMs, and writes
``P.hshard`` with both technologies (``has_second`` = 1, also when the PacBio BAM contributed nothing).  Both passes, the
coverage gate, the reassembly of PacBio reads onto Illumina alleles and the allele stage run in
``hello_candidates_find_hybrid`` (hello_amd/csrc/candidates.hip); include/hello_mi355x.h and DESIGN.md "Two BAMs" state the
rules, among them the two this project defines (the coverage rule and the tie rule).  Technology 1's reads in the shard are
the clipped copies of pass 2.
"""
from __future__ import annotations

import argparse
import ctypes as C
import logging
import os
import sys
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import candidates as cd
from . import shards
from .bam import BamFile, Reads
from ._abi import ARRAY_GETTER, READS, STATS_GETTER, bind, check, handle_array, handle_stats, i32, i64, vp
from .hotspots import HOTSPOTS_HYBRID

DEFAULT_REASSEMBLY_SIZE = 10       # call.py: --reconcilement_size
N_STATS = 29
STAT_NAMES = cd.STAT_NAMES + ("clusters_gate_passed", "clusters_reassembled", "pacbio_reads_eligible", "pacbio_reads_reassigned",
                              "pacbio_reads_reassigned_by_tie", "illumina_sites", "reassembly_ms")
_SITE_ARRAYS = tuple(a for a in cd._ARRAYS if a[1] < 8)                       # start ... allele_text_off
_READ_ARRAYS = tuple(a for a in cd._ARRAYS if 8 <= a[1] <= 18)                # reads_per_allele0 ... hp0, read_index
_REGION_ARRAYS = tuple(a for a in cd._ARRAYS if a[1] > 18)
_READ_SET = READS + [i64]
_PROTOTYPES = (
    ("hello_candidates_find_hybrid", _READ_SET + _READ_SET + [vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    ("hello_candidates_array", ARRAY_GETTER),
    ("hello_candidates_array_tech", [vp, i32] + ARRAY_GETTER[1:]),
    ("hello_candidates_hybrid_stats", STATS_GETTER),
    ("hello_candidates_free", [vp], None),
)


def _lib():
    return bind(_PROTOTYPES)


def find_sites(illumina: Reads, pacbio: Reads, reference: str, positions: Sequence[int], chromosome: str = "chr",
               hybrid_hotspot: bool = False, reassembly_size: int = DEFAULT_REASSEMBLY_SIZE, feature_length: int = 150,
               q_threshold: int = cd.DEFAULT_Q_THRESHOLD, mapq_threshold: int = cd.DEFAULT_MIN_MAPQ,
               device: int = 0, resident: bool = False) -> Tuple[shards.PackedShard, Dict[str, float], Dict[str, np.ndarray]]:
    """One call over already decoded reads -> (validated hybrid shard, statistics, {read_index0, read_index1, regions_pass1,
    regions_pass2}).  ``resident``: the reads of both technologies stay on the GPU and the shard is a
    ``resident.ResidentShard``; the extra arrays then also hold read_off<t> and cigar_off<t>."""
    from . import resident as rs
    ref = np.frombuffer(reference.encode("latin-1"), np.uint8)
    pos = np.ascontiguousarray(positions, dtype=np.int64)
    lib = _lib()
    h = C.c_void_p()
    sets = illumina.pointers(illumina.hp) + [int(illumina.n_reads)] + pacbio.pointers(pacbio.hp) + [int(pacbio.n_reads)]
    check(lib.hello_candidates_find_hybrid(*sets, ref.ctypes.data, int(ref.shape[0]), pos.ctypes.data, int(pos.shape[0]),
                                           (HOTSPOTS_HYBRID if hybrid_hotspot else 0) | (rs.HELLO_CANDIDATES_RESIDENT if resident else 0),
                                           int(reassembly_size), int(feature_length),
                                           int(q_threshold), int(mapq_threshold), int(device), C.byref(h)), value_error_on_arg=True)

    def array(tech, which, dtype):
        return handle_array(lib.hello_candidates_array_tech, h, which, dtype, tech)
    keep = False
    try:
        got = {name: array(0, which, dtype) for name, which, dtype in _SITE_ARRAYS}
        extra = {name: array(0, which, dtype) for name, which, dtype in _REGION_ARRAYS}
        for tech in (0, 1):
            for name, which, dtype in _READ_ARRAYS:
                if name == "read_index":
                    extra[f"read_index{tech}"] = array(tech, which, dtype)
                else:
                    got[name[:-1] + str(tech)] = array(tech, which, dtype)
        st = handle_stats(lib.hello_candidates_hybrid_stats, h, STAT_NAMES)
        got.update(cd.chromosome_table(chromosome, got["start"].shape[0]), has_second=np.array(1))
        if resident:
            extra.update({f"{k}{t}": got[f"{k}{t}"] for k in ("read_off", "cigar_off") for t in (0, 1)})
            shard = rs.ResidentShard(h.value, got, feature_length, hybrid=True)     # owns the handle from here on
            keep = True
        else:
            shard = shards.PackedShard(got, feature_length)
    finally:
        if not keep:
            lib.hello_candidates_free(h)
    return shard, st, extra


def split_bams(bam) -> Tuple[str, str]:
    """``[ibam, pbam]`` or ``"ibam,pbam"`` -> (ibam, pbam); anything else is refused."""
    paths = bam.split(",") if isinstance(bam, str) else list(bam)
    if len(paths) != 2 or not all(paths):
        raise ValueError("hybrid candidate sites are built from two BAMs: the Illumina BAM, then the PacBio BAM (one BAM goes through "
                         "hello_amd.candidates or hello_amd.pacbio)")
    return paths[0], paths[1]


def find_hybrid_candidates(bams, fasta: Optional[str], chromosome: str, positions: Sequence[int], hybrid_hotspot: bool = False,
                           reassembly_size: int = DEFAULT_REASSEMBLY_SIZE, q_threshold: int = cd.DEFAULT_Q_THRESHOLD,
                           mapq_threshold: int = cd.DEFAULT_MIN_MAPQ, device: int = 0, feature_length: int = 150,
                           reference: Optional[str] = None, stats: Optional[dict] = None,
                           resident: bool = False, tagger=None) -> shards.PackedShard:
    """The candidate sites of the sorted hotspot ``positions`` of ``chromosome`` from ``bams`` = [Illumina BAM, PacBio BAM] as a
    validated hybrid ``PackedShard``: alleles in the order of ``candidates.find_candidates``, every allele's supporting reads
    per technology in file order, the PacBio reads clipped.  ``stats``: filled with the statistics of the call.  ``resident``: a
    ``resident.ResidentShard`` whose reads of both technologies stay on the GPU.  ``tagger``: a ``haplotag.Haplotagger``; the reads
    fetched from each BAM get its haplotags in place of the BAM's HP tags, on the full alignments, before any clipping or
    reconciliation."""
    ibam, pbam = split_bams(bams)
    if reference is None:
        from .hotspots import _read_reference
        reference = _read_reference(fasta, chromosome)
    positions = np.asarray(positions, np.int64)
    if positions.shape[0] == 0:
        lo = hi = 0
    else:       # the interval of candidates.find_candidates
        lo = max(0, int(positions.min()) - cd.MIN_DISTANCE // 2 - cd.FLANKING_BASES)
        hi = int(positions.max()) + cd.MIN_DISTANCE // 2 + cd.FLANKING_BASES
    with BamFile(ibam) as b:
        illumina = b.fetch(chromosome, lo, max(hi, lo))
    with BamFile(pbam) as b:
        pacbio = b.fetch(chromosome, lo, max(hi, lo))
    if tagger is not None:
        illumina, pacbio = tagger.retag(chromosome, illumina), tagger.retag(chromosome, pacbio)
    shard, st, extra = find_sites(illumina, pacbio, reference, positions, chromosome, hybrid_hotspot, reassembly_size, feature_length,
                                  q_threshold, mapq_threshold, device, resident=resident)
    if stats is not None:
        stats.update(st)
        stats.update(extra)
    return shard


_TECH1_ARRAYS = ("reads_per_allele1", "bases1", "quals1", "cigars1", "ref_start1", "mapq1", "orientation1", "hp1")
_TECH1_OFFSETS = ("read_off1", "cigar_off1")


def concat_payloads(parts: Sequence[shards.PackedShard]) -> dict:
    """``candidates.concat_payloads`` for hybrid shards: technology 1's arrays too, ``has_second`` = 1."""
    out = cd.concat_payloads(parts)
    for k in _TECH1_ARRAYS:
        out[k] = np.concatenate([np.asarray(p.z[k]) for p in parts])
    for k in _TECH1_OFFSETS:
        chunks, base = [np.zeros(1, np.int64)], 0
        for p in parts:
            o = np.asarray(p.z[k], np.int64)
            chunks.append(o[1:] + base)
            base += int(o[-1])
        out[k] = np.concatenate(chunks)
    out["has_second"] = np.array(1)
    return out


def run_activity(bams, fasta: str, activity: str, output_prefix: str, hybrid_hotspot: bool = False,
                 reassembly_size: int = DEFAULT_REASSEMBLY_SIZE, feature_length: int = 150, q_threshold: int = cd.DEFAULT_Q_THRESHOLD,
                 mapq_threshold: int = cd.DEFAULT_MIN_MAPQ, device: int = 0, genome: Optional[Dict[str, str]] = None,
                 find=None) -> Tuple[str, Dict[str, float]]:
    """One activity file -> ``<output_prefix>.hshard`` (both technologies) and the summed statistics.  ``find``: the function with
    ``find_hybrid_candidates``' signature that builds one chromosome's shard (default: ``find_hybrid_candidates``)."""
    find = find or find_hybrid_candidates
    from .call import read_fasta
    by_chromosome = cd.read_positions(activity)
    if genome is None:
        genome = read_fasta(fasta, list(by_chromosome))
    parts, total = [], {}
    for chromosome, positions in by_chromosome.items():
        if chromosome not in genome:
            raise ValueError(f"{fasta}: no sequence named {chromosome!r}")
        st: dict = {}
        parts.append(find(bams, fasta, chromosome, positions, hybrid_hotspot, reassembly_size, q_threshold, mapq_threshold, device,
                          feature_length, reference=genome[chromosome], stats=st))
        for k in STAT_NAMES:
            total[k] = total.get(k, 0.0) + st[k]
    path = output_prefix + ".hshard"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    shards.write_flat(path, concat_payloads(parts))
    return path, total


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Candidate sites of a hotspot shard from an Illumina and a PacBio BAM on the GPU")
    p.add_argument("--bam", required=True, help="The Illumina BAM and the PacBio BAM, comma-separated, in this order")
    p.add_argument("--ref", required=True, help="Reference FASTA")
    p.add_argument("--activity", required=True, help="Hotspot / shard file: one {'chromosome', 'position'} line per position")
    p.add_argument("--outputPrefix", required=True, help="The shard is written to <outputPrefix>.hshard")
    p.add_argument("--hybrid_hotspot", action="store_true", default=False, help="Differing regions by the hybrid rule (as the hotspot stage's flag)")
    p.add_argument("--reconcilement_size", type=int, default=DEFAULT_REASSEMBLY_SIZE,
                   help="Clusters with at least this many differing regions are not reassembled")
    p.add_argument("--featureLength", type=int, default=150, help="Length of the feature window")
    p.add_argument("--q_threshold", type=int, default=cd.DEFAULT_Q_THRESHOLD, help="Quality score threshold")
    p.add_argument("--mapq_threshold", type=int, default=cd.DEFAULT_MIN_MAPQ, help="Mapping quality threshold")
    p.add_argument("--include_hp", action="store_true", default=False, help="Accepted for the reference's command line: the reads' HP tags are always stored")
    p.add_argument("--debug", action="store_true", default=False, help="Display debug messages")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def main(argv=None) -> str:
    args = parser().parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if args.debug else logging.INFO, format="%(asctime)-15s %(message)s")
    bams = split_bams(args.bam)
    logging.info("Started script")
    path, st = run_activity(bams, args.ref, args.activity, args.outputPrefix, args.hybrid_hotspot, args.reconcilement_size,
                            args.featureLength, args.q_threshold, args.mapq_threshold, args.device)
    logging.info("%d active regions -> %d sites, %d alleles, %d reads in %s (%d clusters reassembled, %d PacBio reads reassigned, %d by "
                 "the tie rule)", st.get("active_regions", 0), st.get("sites", 0), st.get("alleles", 0), st.get("reads_gathered", 0), path,
                 st.get("clusters_reassembled", 0), st.get("pacbio_reads_reassigned", 0), st.get("pacbio_reads_reassigned_by_tie", 0))
    for key in ("regions_at_read_cap", "clusters_at_read_cap"):
        if st.get(key):
            logging.warning("%d %s: their first reads in file order were kept", st[key], key.replace("_", " "))
    logging.info("Completed running the script")
    return path


if __name__ == "__main__":
    main(sys.argv[1:])
