"""Candidate variant positions from BAM files on the GPU: a drop-in for the reference's hotspot stage.

``python -m hello_amd.hotspots`` takes the command line of python/HotspotDetectorDVFiltered.py (:263-330) and writes the
same file: one ``str({'chromosome': c, 'position': p})`` line per position, sorted.  ``--workdir`` runs stage 1 of
python/call.py (:111-160) for whole chromosomes: ``get_chunks(length, 500)`` regions, one ``job_chromosome<c>_job<i>.txt``
per region and their concatenation ``hotspots.txt`` in ``get_workdir(ibam, pbam, chrom, "hotspots")``; the regions of a
chromosome go to the GPU in a few launches instead of a 500-job CPU pool.

The counting and flagging run in ``hello_hotspots_find`` (hello_amd/csrc/hotspots.hip); DESIGN.md "Candidate positions"
states the rules.  Sharding (``shardHotspots``) stays upstream.
"""
from __future__ import annotations

import argparse
import ctypes as C
import logging
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .bam import BamFile, Reads
from ._abi import READS, STATS_GETTER, bind, check, handle_array, handle_stats, i32, i64, vp

CHUNK_SIZE_ILLUMINA = 400          # HotspotDetectorDVFiltered.py:14-17
CHUNK_SIZE_PACBIO = 10000
MAX_NUM_READS_ILLUMINA = 10000
MAX_NUM_READS_PACBIO = 1000
DEFAULT_Q_THRESHOLD = 10
DEFAULT_MIN_MAPQ = 10
HOTSPOTS_PACBIO, HOTSPOTS_HYBRID, HOTSPOTS_TWO_BAMS = 1, 2, 4
N_STATS = 10
STAT_NAMES = ("chunks", "chunks_without_reads", "chunks_out_of_bounds", "chunks_at_read_cap", "reads_counted", "tiles",
              "event_capacity", "kernel_ms", "plan_ms", "total_ms")
MAX_LAUNCH_BASES = 16_000_000      # --workdir: regions of at most this many positions share a launch

_log = logging.getLogger(__name__)
_PROTOTYPES = (
    ("hello_hotspots_find", READS + [i64, vp, i64, vp, vp, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    ("hello_hotspots_positions", [vp, C.POINTER(vp), C.POINTER(i64)]),
    ("hello_hotspots_stats", STATS_GETTER),
    ("hello_hotspots_free", [vp], None),
)


def _lib():
    return bind(_PROTOTYPES)


def get_chunks(length: int, n_jobs: int) -> List[Tuple[int, int]]:
    """python/call.py:52-62."""
    split = length // n_jobs
    ranges = [(i * split, min((i + 1) * split, length)) for i in range(n_jobs)]
    if n_jobs * split < length:
        ranges.append((n_jobs * split, length))
    return ranges


def get_bam_string(bam: str) -> str:
    """python/call.py:33-38."""
    bam = os.path.abspath(bam)
    name0 = os.path.split(bam)[-1]
    name1 = os.path.split(os.path.split(bam)[0])[-1]
    return (name1.replace("/", "__") + "___" + name0.replace("/", "__")).replace(".", "__")


def get_workdir(ibam: Optional[str], pbam: Optional[str], chrom: Optional[str] = None, string: str = "features") -> str:
    """python/call.py:41-49."""
    prefix = string
    if chrom:
        prefix = "%s_%s" % (prefix, chrom)
    if ibam:
        prefix += "_" + get_bam_string(ibam)
    if pbam:
        prefix += "_" + get_bam_string(pbam)
    return prefix


def chunk_plan(start: int, stop: int, two_bams: bool, pacbio: bool) -> List[Tuple[int, int]]:
    """The chunks one region is cut into (HotspotDetectorDVFiltered.py:110-116,149-154)."""
    size = CHUNK_SIZE_PACBIO if (two_bams or pacbio) else CHUNK_SIZE_ILLUMINA
    return [(b, min(b + size, stop)) for b in range(start, stop, size)]


def find_positions(reads: Sequence[Reads], reference: str, regions: Sequence[Tuple[int, int]], pacbio: bool = False,
                   hybrid_hotspot: bool = False, q_threshold: int = DEFAULT_Q_THRESHOLD,
                   mapq_threshold: int = DEFAULT_MIN_MAPQ, device: int = 0) -> Tuple[np.ndarray, Dict[str, float]]:
    """One launch over already decoded read sets (one per BAM, at most two) -> (sorted int64 positions, statistics)."""
    if not 1 <= len(reads) <= 2:
        raise ValueError("one or two read sets (BAM files)")
    if pacbio and len(reads) == 2:
        raise ValueError("pacbio describes a single BAM; two BAMs are Illumina, then PacBio")
    r, source = Reads.concat(list(reads))
    ref = np.frombuffer(reference.encode("latin-1"), np.uint8)
    starts = np.array([a for a, _ in regions], np.int64)
    stops = np.array([b for _, b in regions], np.int64)
    lib = _lib()
    h = C.c_void_p()
    ptr = lambda a: a.ctypes.data  # noqa: E731
    check(lib.hello_hotspots_find(*r.pointers(source), int(r.n_reads), ptr(ref), int(ref.shape[0]), ptr(starts), ptr(stops),
                                  int(starts.shape[0]),
                                  (HOTSPOTS_PACBIO if pacbio else 0) | (HOTSPOTS_HYBRID if hybrid_hotspot else 0)
                                  | (HOTSPOTS_TWO_BAMS if len(reads) == 2 else 0),    # even when the second set is empty
                                  int(q_threshold), int(mapq_threshold), int(device), C.byref(h)))
    try:
        positions = handle_array(lambda h_, _, p, n: lib.hello_hotspots_positions(h_, p, n), h, 0, np.int64)   # one array, no selector
        return positions, handle_stats(lib.hello_hotspots_stats, h, STAT_NAMES)
    finally:
        lib.hello_hotspots_free(h)


def _read_reference(fasta: str, chromosome: str) -> str:
    from .call import read_fasta
    seq = read_fasta(fasta, [chromosome]).get(chromosome)
    if seq is None:
        raise ValueError(f"{fasta}: no sequence named {chromosome!r}")
    return seq


def find_hotspots(bams, fasta: str, chromosome: str, start: int, stop: int, pacbio: bool = False,
                  hybrid_hotspot: bool = False, q_threshold: int = DEFAULT_Q_THRESHOLD, mapq_threshold: int = DEFAULT_MIN_MAPQ,
                  device: int = 0, reference: Optional[str] = None, stats: Optional[dict] = None) -> np.ndarray:
    """Sorted candidate positions of [start, stop) on `chromosome`: what HotspotDetectorDVFiltered.main writes.
    ``bams``: a path, or a list of one or two (Illumina, PacBio).  ``reference``: the chromosome's text, if already read."""
    paths = [bams] if isinstance(bams, str) else list(bams)
    if reference is None:
        reference = _read_reference(fasta, chromosome)
    # reads overlapping any chunk of [start, stop): pysam fetch per chunk sees a subset of these, in the same order
    sets = []
    for path in paths:
        with BamFile(path) as b:
            sets.append(b.fetch(chromosome, start, stop))
    positions, st = find_positions(sets, reference, [(start, stop)], pacbio, hybrid_hotspot, q_threshold, mapq_threshold,
                                   device)
    if stats is not None:
        stats.update(st)
    return positions


def write_positions(path: str, chromosome: str, positions) -> None:
    """HotspotDetectorDVFiltered.py:256-262: one ``str(dict)`` line per position."""
    with open(path, "w") as fh:
        for p in positions:
            fh.write(str({'chromosome': chromosome, 'position': int(p)}) + '\n')


def run_workdir(args) -> List[str]:
    """python/call.py:111-160 without sharding: per chromosome, one job file per get_chunks(len, 500) region and hotspots.txt."""
    bams = args.bam.split(",")
    ibam = bams[0] if (len(bams) == 2 or not args.pacbio) else None
    pbam = bams[1] if len(bams) == 2 else (bams[0] if args.pacbio else None)
    from .call import read_fasta
    chromosomes = args.chromosomes.split(",") if args.chromosomes else None
    genome = read_fasta(args.ref, chromosomes)
    out = []
    for chrom in (chromosomes or list(genome)):
        seq = genome[chrom]
        output_dir = os.path.join(args.workdir, get_workdir(ibam, pbam, chrom=chrom, string="hotspots"))
        os.makedirs(output_dir, exist_ok=True)
        regions = get_chunks(len(seq), 500)
        found: List[np.ndarray] = []
        group: List[Tuple[int, int]] = []
        handles = [BamFile(p) for p in bams]
        try:
            def flush():
                if not group:
                    return
                sets = [h.fetch(chrom, group[0][0], group[-1][1]) for h in handles]
                pos, st = find_positions(sets, seq, group, args.pacbio and len(bams) == 1, args.hybrid_hotspot,
                                         args.q_threshold, args.mapq_threshold, args.device)
                _log.info("chromosome %s [%d, %d): %d positions, kernel %.1f ms", chrom, group[0][0], group[-1][1], len(pos),
                          st["kernel_ms"])
                found.append(pos)
                group.clear()
            for reg in regions:
                if group and reg[1] - group[0][0] > MAX_LAUNCH_BASES:
                    flush()
                group.append(reg)
            flush()
        finally:
            for h in handles:
                h.close()
        allpos = np.concatenate(found) if found else np.zeros(0, np.int64)
        names = []
        for i, (a, b) in enumerate(regions):
            name = os.path.join(output_dir, "job_chromosome%s_job%d.txt" % (chrom, i))
            lo, hi = np.searchsorted(allpos, a), np.searchsorted(allpos, b)
            write_positions(name, chrom, allpos[lo:hi])
            names.append(name)
        hotspot_name = os.path.join(output_dir, "hotspots.txt")
        with open(hotspot_name, "w") as fh:
            for name in names:
                with open(name) as part:
                    fh.write(part.read())
        _log.info("chromosome %s: %d hotspots in %s", chrom, len(allpos), hotspot_name)
        out.append(hotspot_name)
    return out


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Hotspot detection on the GPU (HotspotDetectorDVFiltered.py's command line)")
    p.add_argument("--bam", required=True, help="Comma-separated list of BAM files from which to call hotspots")
    p.add_argument("--ref", required=True, help="Reference FASTA")
    p.add_argument("--region", help="Chromosome,start,stop or simply Chromosome")
    p.add_argument("--pacbio", action="store_true", default=False, help="Indicate that we are using PacBio reads (for a single file)")
    p.add_argument("--output", help="Path to the output file")
    p.add_argument("--debug", action="store_true", default=False, help="Display debug messages")
    p.add_argument("--hybrid_hotspot", action="store_true", default=False, help="Enable hybrid hotspot detection")
    p.add_argument("--q_threshold", type=int, default=DEFAULT_Q_THRESHOLD, help="Quality score threshold")
    p.add_argument("--mapq_threshold", type=int, default=DEFAULT_MIN_MAPQ, help="Mapping quality threshold")
    p.add_argument("--workdir", help="Whole-genome mode (python/call.py stage 1): job files and hotspots.txt under this directory")
    p.add_argument("--chromosomes", help="--workdir: comma-separated chromosomes (default: every FASTA record)")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    p = parser()
    args = p.parse_args(argv)
    if args.workdir is None and (args.region is None or args.output is None):
        p.error("--region and --output are required (or --workdir for whole chromosomes)")
    if len(args.bam.split(",")) > 2:
        p.error("--bam takes one or two files")
    return args


def main(argv=None) -> Optional[str]:
    args = parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if args.debug else logging.INFO, format="%(asctime)-15s %(message)s")
    logging.info("Started script")
    if args.workdir is not None:
        run_workdir(args)
        logging.info("Completed running the script")
        return args.workdir
    fields = args.region.split(",")
    reference = None
    if len(fields) == 1:
        chromosome = fields[0]
        reference = _read_reference(args.ref, chromosome)
        start, stop = 0, len(reference)
    elif len(fields) == 3:
        chromosome, start, stop = fields[0], int(fields[1]), int(fields[2])
    else:
        raise SystemExit("--region: chromosome or chromosome,start,stop")
    bams = args.bam.split(",")
    stats: dict = {}
    positions = find_hotspots(bams if len(bams) > 1 else bams[0], args.ref, chromosome, start, stop,
                              pacbio=args.pacbio and len(bams) == 1, hybrid_hotspot=args.hybrid_hotspot,
                              q_threshold=args.q_threshold, mapq_threshold=args.mapq_threshold, device=args.device,
                              reference=reference, stats=stats)
    logging.debug("statistics: %s", stats)
    if stats.get("chunks_at_read_cap"):
        logging.warning("%d chunks reached the read cap: their first reads in file order were kept", stats["chunks_at_read_cap"])
    write_positions(args.output, chromosome, positions)
    logging.info("Completed running the script")
    return args.output


if __name__ == "__main__":
    main(sys.argv[1:])
