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

import numpy as np

from . import candidates as cd
from . import shards
from .bam import BamFile
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
    if reference is None:
        from .hotspots import _read_reference
        reference = _read_reference(fasta, chromosome)
    positions = np.asarray(positions, np.int64)
    if positions.shape[0] == 0:
        lo = hi = 0
    else:       # the interval of find_candidates: long reads reach far outside it
        lo = max(0, int(positions.min()) - cd.MIN_DISTANCE // 2 - cd.FLANKING_BASES)
        hi = int(positions.max()) + cd.MIN_DISTANCE // 2 + cd.FLANKING_BASES
    with BamFile(paths[0]) as b:
        reads = b.fetch(chromosome, lo, max(hi, lo))
    if tagger is not None:
        reads = tagger.retag(chromosome, reads)
    shard, st, extra = cd.find_sites(reads, reference, positions, chromosome, feature_length, q_threshold, mapq_threshold, device,
                                     options=HOTSPOTS_PACBIO, resident=resident)
    if stats is not None:
        stats.update(st)
        stats.update(extra)
    return shard


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Candidate sites of a hotspot shard from one PacBio BAM on the GPU")
    p.add_argument("--bam", required=True, help="The PacBio BAM file (one file)")
    p.add_argument("--ref", required=True, help="Reference FASTA")
    p.add_argument("--activity", required=True, help="Hotspot / shard file: one {'chromosome', 'position'} line per position")
    p.add_argument("--outputPrefix", required=True, help="The shard is written to <outputPrefix>.hshard")
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
    if len(args.bam.split(",")) != 1:
        raise ValueError(cd.REFUSAL)
    logging.info("Started script")
    path, st = cd.run_activity(args.bam, args.ref, args.activity, args.outputPrefix, args.featureLength, args.q_threshold,
                               args.mapq_threshold, args.device, find=find_pacbio_candidates)
    logging.info("%d active regions -> %d sites, %d alleles, %d reads in %s (%d reads clipped)", st.get("active_regions", 0),
                 st.get("sites", 0), st.get("alleles", 0), st.get("reads_gathered", 0), path, st.get("reads_clipped", 0))
    for key in ("regions_at_read_cap", "clusters_at_read_cap"):
        if st.get(key):
            logging.warning("%d %s: their first reads in file order were kept", st[key], key.replace("_", " "))
    logging.info("Completed running the script")
    return path


if __name__ == "__main__":
    main(sys.argv[1:])
