"""The BAM route of a ``hello_amd.call`` command line: which BAM(s) its stages read, and with which options and thresholds.

Three routes exist: ``--from_bam`` with one Illumina BAM, ``--from_bam`` with one PacBio BAM, and ``--from_bams`` with an Illumina
and a PacBio BAM.  ``Route.from_args`` is the one place that knows their rule -- ``--from_bam`` runs every stage at the default
thresholds and ignores ``--q_threshold``, ``--mapq_threshold``, ``--hybrid_hotspot`` and ``--reconcilement_size``; ``--from_bams``
passes them on, as the reference's python/call.py does -- and every stage of the driver (hotspots, candidate sites, ``--gvcf``,
``--phase``, ``--haplotag_vcf``) reads its BAM(s), thresholds, chromosomes and device off the route it returns.
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import Dict, List, Optional, Tuple

from . import candidates as cd


def chromosome_list(text: Optional[str]) -> Optional[List[str]]:
    """``--chromosomes``: the comma-separated names, or None for every chromosome."""
    return text.split(",") if text else None


def from_bam_route(ibam: Optional[str], pbam: Optional[str]):
    """python/call.py:90-109 for --from_bam: one Illumina BAM, or one PacBio BAM (``pacbio = pbam and not ibam``).  -> (the BAM,
    pacbio, the function that builds a chromosome's candidate sites).  Both BAMs and comma lists are refused."""
    if (ibam and pbam) or not (ibam or pbam) or "," in (ibam or pbam):
        raise ValueError(cd.REFUSAL)
    if pbam:
        from .pacbio import find_pacbio_candidates
        return pbam, True, find_pacbio_candidates
    return ibam, False, cd.find_candidates


@dataclasses.dataclass(frozen=True)
class Route:
    bams: Tuple[str, ...]                      # one BAM, or the Illumina BAM and then the PacBio BAM
    pacbio: bool                               # the single BAM is a PacBio BAM
    hybrid_hotspot: bool
    reassembly_size: int
    q_threshold: int
    mapq_threshold: int
    chromosomes: Optional[Tuple[str, ...]]     # None: every chromosome of the FASTA
    device: int
    ref: Optional[str]

    @classmethod
    def from_args(cls, args, two_bams: Optional[bool] = None, need_ref: bool = True) -> "Route":
        """The route of the driver's parsed arguments; ``two_bams``: ``--from_bams`` (default: as the arguments say).  A wrong
        number of BAMs is refused first, then (``need_ref``: the stages that read the FASTA follow) a missing ``--ref``."""
        if getattr(args, "from_bams", False) if two_bams is None else two_bams:
            if not (args.ibam and args.pbam) or "," in args.ibam or "," in args.pbam:
                raise ValueError("--from_bams needs one --ibam and one --pbam (one BAM: --from_bam)")
            flag, bams, pacbio = "--from_bams", (args.ibam, args.pbam), False
            options = (args.hybrid_hotspot, args.reconcilement_size, args.q_threshold, args.mapq_threshold)
        else:
            bam, pacbio, _ = from_bam_route(args.ibam, args.pbam)
            flag, bams = "--from_bam", (bam,)
            options = (False, 0, cd.DEFAULT_Q_THRESHOLD, cd.DEFAULT_MIN_MAPQ)      # no reassembly with one BAM
        if need_ref and not args.ref:
            raise SystemExit(f"{flag} needs --ref")
        chromosomes = chromosome_list(args.chromosomes)
        return cls(bams, pacbio, *options, tuple(chromosomes) if chromosomes else None, args.device, args.ref)

    def hotspot_args(self, workdir: str, genome: Dict[str, str]) -> argparse.Namespace:
        """What ``hotspots.run_workdir`` takes; ``genome``: the FASTA's sequences, whose names are the chromosomes when none was given."""
        return argparse.Namespace(bam=",".join(self.bams), ref=self.ref, pacbio=self.pacbio, hybrid_hotspot=self.hybrid_hotspot,
                                  workdir=workdir, chromosomes=",".join(self.chromosomes or list(genome)), q_threshold=self.q_threshold,
                                  mapq_threshold=self.mapq_threshold, device=self.device)

    def finder(self, tagger=None):
        """-> (the function that builds one chromosome's candidate sites from ``list(bams)``, its keyword arguments);
        ``tagger``: a ``haplotag.Haplotagger`` for the reads it fetches."""
        kw = dict(q_threshold=self.q_threshold, mapq_threshold=self.mapq_threshold, device=self.device)
        if tagger is not None:
            kw["tagger"] = tagger
        if len(self.bams) == 2:
            from .hybrid import find_hybrid_candidates
            return find_hybrid_candidates, dict(kw, hybrid_hotspot=self.hybrid_hotspot, reassembly_size=self.reassembly_size)
        ibam, pbam = (None, self.bams[0]) if self.pacbio else (self.bams[0], None)
        return from_bam_route(ibam, pbam)[2], kw
