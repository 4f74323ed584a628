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
import sys
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import candidates as cd
from . import shards
from .bam import Reads
from ._abi import ARRAY_GETTER, READS, STATS_GETTER, bind, check, i32, i64, vp
from .hotspots import HOTSPOTS_HYBRID

DEFAULT_REASSEMBLY_SIZE = 10       # call.py: --reconcilement_size
N_STATS = 29
STAT_NAMES = cd.STAT_NAMES + ("clusters_gate_passed", "clusters_reassembled", "pacbio_reads_eligible", "pacbio_reads_reassigned",
                              "pacbio_reads_reassigned_by_tie", "illumina_sites", "reassembly_ms")
_READ_SET = READS + [i64]
_PROTOTYPES = (
    ("hello_candidates_find_hybrid", _READ_SET + _READ_SET + [vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]),
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
    return cd.read_handle(lib, h, 2, lib.hello_candidates_hybrid_stats, STAT_NAMES, chromosome, feature_length, resident)


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
    return cd.find_from_bams(split_bams(bams), fasta, chromosome, positions, q_threshold, mapq_threshold, device, feature_length,
                             reference, stats, resident, tagger, hybrid_hotspot=hybrid_hotspot, reassembly_size=reassembly_size)


def parser() -> argparse.ArgumentParser:
    return cd.stage_parser(
        "Candidate sites of a hotspot shard from an Illumina and a PacBio BAM on the GPU",
        "The Illumina BAM and the PacBio BAM, comma-separated, in this order",
        after_output=(("--hybrid_hotspot", dict(cd.FLAG, help="Differing regions by the hybrid rule (as the hotspot stage's flag)")),
                      ("--reconcilement_size", dict(type=int, default=DEFAULT_REASSEMBLY_SIZE,
                                                    help="Clusters with at least this many differing regions are not reassembled"))))


def main(argv=None) -> str:
    args = cd.start_main(parser(), argv)
    bams = split_bams(args.bam)
    logging.info("Started script")
    path, st = cd.run_activity(bams, args.ref, args.activity, args.outputPrefix, args.featureLength, args.q_threshold,
                               args.mapq_threshold, args.device, find=find_hybrid_candidates, hybrid_hotspot=args.hybrid_hotspot,
                               reassembly_size=args.reconcilement_size)
    return cd.finish_main(path, st, " (%d clusters reassembled, %d PacBio reads reassigned, %d by the tie rule)" % (
        st.get("clusters_reassembled", 0), st.get("pacbio_reads_reassigned", 0), st.get("pacbio_reads_reassigned_by_tie", 0)))


if __name__ == "__main__":
    main(sys.argv[1:])
