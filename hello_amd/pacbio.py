"""Candidate sites of ONE PacBio BAM on the GPU: ``hello_amd.candidates`` for long reads.

``python -m hello_amd.pacbio --bam B --ref F --activity shardN.txt --outputPrefix P`` does what the reference's
python/caller_calling.py does up to its featurizer (:784-843) when it is given one PacBio BAM (``pacbio = pbam and not ibam``,
python/call.py:90-109): one read sampler with READ_RATE_PACBIO = (100, 100), strict read clipping with a flank of 200 and no
reassembly.  It writes ``P.hshard`` like ``hello_amd.candidates``.  The stages are those of ``hello_candidates_find`` with
``HELLO_HOTSPOTS_PACBIO`` (hello_amd/csrc/candidates.hip; include/hello_mi355x.h and DESIGN.md "Candidate sites" state the cap
and the clipping rules): the reads of a shard are the clipped copies of pass 2.  Two BAMs, ``--hybrid_hotspot``, ``--clr``
and ``--noClip`` are not supported here; an Illumina and a PacBio BAM together go through ``hello_amd.hybrid``.
"""
from __future__ import annotations

import argparse
import logging
import sys
from typing import Optional, Sequence

from . import candidates as cd
from . import shards
from .hotspots import HOTSPOTS_PACBIO


def find_pacbio_candidates(bam, fasta: Optional[str], chromosome: str, positions: Sequence[int],
                           q_threshold: int = cd.DEFAULT_Q_THRESHOLD, mapq_threshold: int = cd.DEFAULT_MIN_MAPQ, device: int = 0,
                           feature_length: int = 150, reference: Optional[str] = None,
                           stats: Optional[dict] = None, resident: bool = False, tagger=None) -> shards.PackedShard:
    """The candidate sites of the sorted hotspot ``positions`` of ``chromosome`` from one PacBio BAM as a validated
    ``PackedShard``; alleles and supporting reads in the orders of ``candidates.find_candidates``, the reads clipped.  ``bam``:
    one path.  ``stats``: filled with the statistics of the call.  ``resident``: a ``resident.ResidentShard`` whose reads (the
    clipped copies) stay on the GPU where the clip kernel wrote them.  ``tagger``: a ``haplotag.Haplotagger``; the reads fetched
    get its haplotags in place of the BAM's HP tags, on the full alignments, before anything is clipped."""
    paths = [bam] if isinstance(bam, str) else list(bam)
    if len(paths) != 1 or "," in paths[0]:
        raise ValueError(cd.REFUSAL)
    return cd.find_from_bams(paths, fasta, chromosome, positions, q_threshold, mapq_threshold, device, feature_length, reference, stats,
                             resident, tagger, options=HOTSPOTS_PACBIO)


def parser() -> argparse.ArgumentParser:
    return cd.stage_parser("Candidate sites of a hotspot shard from one PacBio BAM on the GPU", "The PacBio BAM file (one file)")


def main(argv=None) -> str:
    args = cd.start_main(parser(), argv)
    if len(args.bam.split(",")) != 1:
        raise ValueError(cd.REFUSAL)
    logging.info("Started script")
    path, st = cd.run_activity(args.bam, args.ref, args.activity, args.outputPrefix, args.featureLength, args.q_threshold,
                               args.mapq_threshold, args.device, find=find_pacbio_candidates)
    return cd.finish_main(path, st, " (%d reads clipped)" % st.get("reads_clipped", 0))


if __name__ == "__main__":
    main(sys.argv[1:])
