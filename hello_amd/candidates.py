"""Candidate sites from hotspot positions on the GPU: the stage between ``hello_amd.hotspots`` and ``hello_amd.call``.

``python -m hello_amd.candidates --bam B --ref F --activity shardN.txt --outputPrefix P`` does what the reference's
python/caller_calling.py does up to its featurizer (:784-843) for ONE Illumina BAM, and writes ``P.hshard``
(hello_amd/shards.py) instead of calling a network: the positions of a hotspot / shard file become active regions, their
strict differing regions (pass 1), clusters of those, the clusters' own strict differing regions (pass 2, the sites), and per
site the alleles the reads spell there with every allele's supporting reads.  Both passes and the allele stage run in
``hello_candidates_find`` (hello_amd/csrc/candidates.hip); DESIGN.md "Candidate sites" states the rules.  ``shard_positions``
is the reference's python/shardHotspots.py.  Two BAMs and ``--hybrid_hotspot`` are refused here: they go through
``hello_amd.hybrid`` (``hello_candidates_find_hybrid``).
One PacBio BAM has its own entry points in ``hello_amd.pacbio``; ``pacbio=True`` / ``--pacbio`` here are refused with a pointer
to them.
"""
from __future__ import annotations

import argparse
import ast
import ctypes as C
import logging
import math
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import shards
from .bam import BamFile, Reads
from ._abi import ARRAY_GETTER, READS, STATS_GETTER, bind, check, handle_array, handle_stats, i32, i64, vp

DEFAULT_Q_THRESHOLD = 10
DEFAULT_MIN_MAPQ = 10
MIN_DISTANCE = 30                  # PileupDataTools.py:21
FLANKING_BASES = 75                # :24
N_STATS = 22
STAT_NAMES = ("active_regions", "regions_without_reads", "regions_out_of_bounds", "regions_at_read_cap", "differing_regions_pass1",
              "clusters", "clusters_without_reads", "clusters_out_of_bounds", "clusters_at_read_cap", "differing_regions_pass2",
              "sites", "sites_out_of_bounds", "alleles", "reads_gathered", "record_slots", "pass1_kernel_ms", "pass2_kernel_ms",
              "allele_kernel_ms", "gather_ms", "total_ms", "clip_kernel_ms", "reads_clipped")
_ARRAYS = (  # (name, hello_candidates_array_tech selector, dtype; the read arrays carry technology 0's name)
    ("start", 0, np.int64), ("stop", 1, np.int64), ("window_start", 2, np.int64), ("ref_off", 3, np.int64), ("ref", 4, np.uint8),
    ("alleles_per_site", 5, np.int32), ("allele_text", 6, np.uint8), ("allele_text_off", 7, np.int64),
    ("reads_per_allele0", 8, np.int32), ("bases0", 9, np.uint8), ("quals0", 10, np.uint8), ("read_off0", 11, np.int64),
    ("cigars0", 12, np.uint32), ("cigar_off0", 13, np.int64), ("ref_start0", 14, np.int64), ("mapq0", 15, np.uint8),
    ("orientation0", 16, np.int8), ("hp0", 17, np.uint8), ("read_index", 18, np.int64), ("regions_pass1", 19, np.int64),
    ("regions_pass2", 20, np.int64),
)
REFUSAL = ("candidate sites are built from one Illumina BAM: two BAMs and --hybrid_hotspot need the two-BAM reassembly, which "
           "hello_amd does not have; one PacBio BAM goes through hello_amd.pacbio (python -m hello_amd.pacbio)")

_log = logging.getLogger(__name__)
_PROTOTYPES = (
    ("hello_candidates_find", READS + [i64, vp, i64, vp, i64, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    ("hello_candidates_array_tech", [vp, i32] + ARRAY_GETTER[1:]),
    ("hello_candidates_stats", STATS_GETTER),
    ("hello_candidates_free", [vp], None),
)


def _lib():
    return bind(_PROTOTYPES)


def read_positions(path: str) -> Dict[str, List[int]]:
    """A hotspot / shard file (one ``str({'chromosome': c, 'position': p})`` line per position) -> positions per chromosome, in
    file order."""
    out: Dict[str, List[int]] = {}
    with open(path) as fh:
        for line in fh:
            if line.strip():
                point = ast.literal_eval(line)
                out.setdefault(str(point['chromosome']), []).append(int(point['position']))
    return out


def shard_positions(positions: Sequence[int], max_shards: int = 500, min_separation: int = 25) -> List[List[int]]:
    """python/shardHotspots.py: runs of adjacent positions are items; a shard closes once it holds ceil(items / max_shards)
    items and the next item starts at least ``min_separation`` behind its last position."""
    items: List[List[int]] = []
    for p in positions:
        if items and p - items[-1][-1] == 1:
            items[-1].append(int(p))
        else:
            items.append([int(p)])
    min_items = math.ceil(len(items) / max_shards)
    out: List[List[int]] = []
    cluster: List[List[int]] = []
    for item in items:
        if len(cluster) < min_items or item[0] - cluster[-1][-1] < min_separation:
            cluster.append(item)
        else:
            out.append([p for it in cluster for p in it])
            cluster = [item]
    if cluster:
        out.append([p for it in cluster for p in it])
    return out


def find_sites(reads: Reads, reference: str, positions: Sequence[int], chromosome: str = "chr", feature_length: int = 150,
               q_threshold: int = DEFAULT_Q_THRESHOLD, mapq_threshold: int = DEFAULT_MIN_MAPQ, device: int = 0,
               options: int = 0, resident: bool = False) -> Tuple[shards.PackedShard, Dict[str, float], Dict[str, np.ndarray]]:
    """One call over already decoded reads -> (validated shard, statistics, {read_index, regions_pass1, regions_pass2}).
    ``resident``: the reads stay on the GPU and the shard is a ``resident.ResidentShard`` (close it, or hand it to
    ``ShardScorer.submit``, which does); the extra arrays then also hold read_off0 and cigar_off0."""
    from . import resident as rs
    ref = np.frombuffer(reference.encode("latin-1"), np.uint8)
    pos = np.ascontiguousarray(positions, dtype=np.int64)
    lib = _lib()
    h = C.c_void_p()
    check(lib.hello_candidates_find(*reads.pointers(reads.hp), int(reads.n_reads), ref.ctypes.data, int(ref.shape[0]),
                                    pos.ctypes.data, int(pos.shape[0]),
                                    int(options) | (rs.HELLO_CANDIDATES_RESIDENT if resident else 0),
                                    int(feature_length), int(q_threshold), int(mapq_threshold), int(device), C.byref(h)),
          value_error_on_arg=True)
    return read_handle(lib, h, 1, lib.hello_candidates_stats, STAT_NAMES, chromosome, feature_length, resident)


def read_handle(lib, h, technologies: int, stats_getter, stat_names, chromosome: str, feature_length: int, resident: bool):
    """The arrays and statistics of the ``hello_candidates`` handle ``h`` of one or two technologies -> (``PackedShard``, or a
    ``ResidentShard`` that owns the handle from here on, also when it raises; statistics; the extra arrays).  The read index is
    ``read_index`` for one technology and ``read_index0`` / ``read_index1`` for two.  The handle is freed unless the shard owns it."""
    from . import resident as rs
    try:
        got, extra = {}, {}
        for name, which, dtype in _ARRAYS:
            if which < 8:                                   # start ... allele_text_off: the sites
                got[name] = handle_array(lib.hello_candidates_array_tech, h, which, dtype, 0)
            elif which > 18:                                # regions_pass1, regions_pass2
                extra[name] = handle_array(lib.hello_candidates_array_tech, h, which, dtype, 0)
            else:                                           # reads_per_allele0 ... hp0, read_index: per technology
                for tech in range(technologies):
                    a = handle_array(lib.hello_candidates_array_tech, h, which, dtype, tech)
                    if name == "read_index":
                        extra[name + (str(tech) if technologies == 2 else "")] = a
                    else:
                        got[name[:-1] + str(tech)] = a
        st = handle_stats(stats_getter, h, stat_names)
        got.update(chromosome_table(chromosome, got["start"].shape[0]), has_second=np.array(technologies - 1))
        if resident:
            extra.update({f"{k}{t}": got[f"{k}{t}"] for k in ("read_off", "cigar_off") for t in range(technologies)})
            owned, h = h, None
            return rs.ResidentShard(owned.value, got, feature_length, hybrid=technologies == 2), st, extra
        return shards.PackedShard(got, feature_length), st, extra
    finally:
        if h is not None:
            lib.hello_candidates_free(h)


def chromosome_table(chromosome: str, n_sites: int) -> Dict[str, np.ndarray]:
    """The chromosome arrays of a shard whose ``n_sites`` sites all lie on ``chromosome``."""
    name = np.frombuffer(chromosome.encode("ascii"), np.uint8)
    return dict(chromosome_text=name if n_sites else np.zeros(0, np.uint8),
                chromosome_text_off=np.array([0, name.shape[0]] if n_sites else [0], np.int64),
                chromosome_of_site=np.zeros(n_sites, np.int32))


def fetch_interval(positions: np.ndarray) -> Tuple[int, int]:
    """The interval whose reads the candidate stage needs: pass 1 fetches [start - 75, stop + 75) around [first - 15, last + 15]
    (long reads reach far outside it)."""
    if positions.shape[0] == 0:
        return 0, 0
    lo = max(0, int(positions.min()) - MIN_DISTANCE // 2 - FLANKING_BASES)
    return lo, max(int(positions.max()) + MIN_DISTANCE // 2 + FLANKING_BASES, lo)


def find_from_bams(paths: Sequence[str], fasta: Optional[str], chromosome: str, positions: Sequence[int], q_threshold: int,
                   mapq_threshold: int, device: int, feature_length: int, reference: Optional[str], stats: Optional[dict],
                   resident: bool, tagger, options: int = 0, hybrid_hotspot: bool = False, reassembly_size: int = 0) -> shards.PackedShard:
    """What the three finders share: the reads of ``fetch_interval`` from every BAM of ``paths``, retagged by ``tagger`` if there
    is one, through ``find_sites`` with ``options`` (one BAM) or ``hybrid.find_sites`` (two: Illumina, PacBio); ``stats`` is filled
    with the statistics and the extra arrays of the call."""
    if reference is None:
        from .hotspots import _read_reference
        reference = _read_reference(fasta, chromosome)
    positions = np.asarray(positions, np.int64)
    lo, hi = fetch_interval(positions)
    sets = []
    for path in paths:
        with BamFile(path) as b:
            sets.append(b.fetch(chromosome, lo, hi))
    if tagger is not None:
        sets = [tagger.retag(chromosome, reads) for reads in sets]
    if len(sets) == 2:
        from . import hybrid
        shard, st, extra = hybrid.find_sites(sets[0], sets[1], reference, positions, chromosome, hybrid_hotspot, reassembly_size,
                                             feature_length, q_threshold, mapq_threshold, device, resident=resident)
    else:
        shard, st, extra = find_sites(sets[0], reference, positions, chromosome, feature_length, q_threshold, mapq_threshold, device,
                                      options=options, resident=resident)
    if stats is not None:
        stats.update(st)
        stats.update(extra)
    return shard


def find_candidates(bam, fasta: Optional[str], chromosome: str, positions: Sequence[int], q_threshold: int = DEFAULT_Q_THRESHOLD,
                    mapq_threshold: int = DEFAULT_MIN_MAPQ, device: int = 0, feature_length: int = 150, pacbio: bool = False,
                    hybrid_hotspot: bool = False, reference: Optional[str] = None,
                    stats: Optional[dict] = None, resident: bool = False, tagger=None) -> shards.PackedShard:
    """The candidate sites of the sorted hotspot ``positions`` of ``chromosome`` as a validated ``PackedShard``: sites, alleles
    (reference allele first, then ascending byte order) and every allele's supporting reads (file order).  ``bam``: one path
    (a list of two, ``pacbio`` and ``hybrid_hotspot`` are refused).  ``stats``: filled with the statistics of the call.
    ``resident``: a ``resident.ResidentShard`` whose reads stay on the GPU.  ``tagger``: a ``haplotag.Haplotagger``; the reads
    fetched get its haplotags in place of the BAM's HP tags before the sites are looked for."""
    paths = [bam] if isinstance(bam, str) else list(bam)
    if len(paths) != 1 or pacbio or hybrid_hotspot:
        raise ValueError(REFUSAL)
    return find_from_bams(paths, fasta, chromosome, positions, q_threshold, mapq_threshold, device, feature_length, reference, stats,
                          resident, tagger)


def write_packed(path: str, shard: shards.PackedShard) -> str:
    """A ``PackedShard`` as a ``.hshard`` file, array for array (a resident shard is refused: its reads are on the GPU)."""
    return shards.write_flat(path, {k: np.asarray(v) for k, v in shard.z.items()})


def concat_payloads(parts: Sequence[shards.PackedShard]) -> dict:
    """The arrays of several single-chromosome shards as one shard's arrays (a shard file may span chromosomes); technology 1's
    arrays too, and ``has_second`` = 1, when the parts are hybrid shards."""
    def cat(name):
        return np.concatenate([np.asarray(p.z[name]) for p in parts])

    def offsets(name):
        out, base = [np.zeros(1, np.int64)], 0
        for p in parts:
            o = np.asarray(p.z[name], np.int64)
            out.append(o[1:] + base)
            base += int(o[-1])
        return np.concatenate(out)
    per_read = ("reads_per_allele", "bases", "quals", "cigars", "ref_start", "mapq", "orientation", "hp")
    names = [p.chromosome_names[0] for p in parts if p.n_sites]
    out = {k: cat(k) for k in ("start", "stop", "window_start", "ref", "alleles_per_site", "allele_text") + tuple(k + "0" for k in per_read)}
    for k in ("ref_off", "allele_text_off", "read_off0", "cigar_off0"):
        out[k] = offsets(k)
    out["chromosome_text"], out["chromosome_text_off"] = shards.text_table(np.array(names, dtype="U")) if names else (
        np.zeros(0, np.uint8), np.zeros(1, np.int64))
    out["chromosome_of_site"] = np.concatenate([np.full(p.n_sites, i, np.int32) for i, p in enumerate(q for q in parts if q.n_sites)]
                                               + [np.zeros(0, np.int32)])
    second = all(p.hybrid for p in parts)
    out["has_second"] = np.array(int(second))
    if second:
        out.update({k + "1": cat(k + "1") for k in per_read})
        out.update({k: offsets(k) for k in ("read_off1", "cigar_off1")})
    return out


FLAG = dict(action="store_true", default=False)
HP_HELP = "Accepted for the reference's command line: the reads' HP tags are always stored"


def stage_parser(description: str, bam_help: str, hp_help: str = HP_HELP, after_output=(), after_hp=()) -> argparse.ArgumentParser:
    """The command line the three candidate modules share; ``after_output`` / ``after_hp``: a module's own (flag, keywords) at the
    two places where the modules' lists differ."""
    p = argparse.ArgumentParser(description=description)
    for name, kw in (("--bam", dict(required=True, help=bam_help)),
                     ("--ref", dict(required=True, help="Reference FASTA")),
                     ("--activity", dict(required=True, help="Hotspot / shard file: one {'chromosome', 'position'} line per position")),
                     ("--outputPrefix", dict(required=True, help="The shard is written to <outputPrefix>.hshard")),
                     *after_output,
                     ("--featureLength", dict(type=int, default=150, help="Length of the feature window")),
                     ("--q_threshold", dict(type=int, default=DEFAULT_Q_THRESHOLD, help="Quality score threshold")),
                     ("--mapq_threshold", dict(type=int, default=DEFAULT_MIN_MAPQ, help="Mapping quality threshold")),
                     ("--include_hp", dict(FLAG, help=hp_help)),
                     *after_hp,
                     ("--debug", dict(FLAG, help="Display debug messages")),
                     ("--device", dict(type=int, default=0, help="GPU index"))):
        p.add_argument(name, **kw)
    return p


def parser() -> argparse.ArgumentParser:
    return stage_parser("Candidate sites of a hotspot shard on the GPU (caller_calling.py's flags where they apply)",
                        "The Illumina BAM file (one file)",
                        HP_HELP + "; the scoring driver's --include_hp decides whether they are used",
                        after_hp=(("--pacbio", dict(FLAG, help="Refused: use python -m hello_amd.pacbio for one PacBio BAM")),
                                  ("--hybrid_hotspot", dict(FLAG, help="Refused: needs two BAMs"))))


def activity_shards(bam, fasta: str, activity: str, genome: Optional[Dict[str, str]] = None, find=None, total: Optional[dict] = None,
                    **kw):
    """One shard per chromosome of the activity file, in file order.  ``find``: ``find_candidates`` (default),
    ``pacbio.find_pacbio_candidates`` or ``hybrid.find_hybrid_candidates``; ``kw``: its thresholds and options (``resident``
    among them); ``total``: the statistics are summed into it."""
    find = find or find_candidates
    from .call import read_fasta
    by_chromosome = read_positions(activity)
    if genome is None:
        genome = read_fasta(fasta, list(by_chromosome))
    for chromosome, positions in by_chromosome.items():
        if chromosome not in genome:
            raise ValueError(f"{fasta}: no sequence named {chromosome!r}")
        st: dict = {}
        shard = find(bam, fasta, chromosome, positions, reference=genome[chromosome], stats=st, **kw)
        if total is not None:
            for k, v in st.items():
                if not isinstance(v, np.ndarray):
                    total[k] = total.get(k, 0.0) + v
        yield shard


def run_activity(bam, fasta: str, activity: str, output_prefix: str, feature_length: int = 150,
                 q_threshold: int = DEFAULT_Q_THRESHOLD, mapq_threshold: int = DEFAULT_MIN_MAPQ, device: int = 0, genome: Optional[Dict[str, str]] = None,
                 find=None, **kw) -> Tuple[str, Dict[str, float]]:
    """One activity file -> ``<output_prefix>.hshard`` and the summed statistics.  ``bam``, ``find`` and ``kw`` (a hybrid
    finder's ``hybrid_hotspot`` and ``reassembly_size``, a ``tagger``) as for ``activity_shards``."""
    total: dict = {}
    parts = list(activity_shards(bam, fasta, activity, genome, find, total, q_threshold=q_threshold, mapq_threshold=mapq_threshold,
                                 device=device, feature_length=feature_length, **kw))
    path = output_prefix + ".hshard"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    shards.write_flat(path, concat_payloads(parts))
    return path, total


def resident_activity(bam, fasta: str, activity: str, genome: Optional[Dict[str, str]] = None, find=None, total: Optional[dict] = None,
                      **kw):
    """``run_activity`` without the file: yields one ``ResidentShard`` per chromosome of the activity file, each naming the file
    (the caller closes them or hands them to ``ShardScorer.submit``)."""
    for shard in activity_shards(bam, fasta, activity, genome, find, total, resident=True, **kw):
        shard.path = activity
        yield shard


def start_main(parser: argparse.ArgumentParser, argv) -> argparse.Namespace:
    args = parser.parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if args.debug else logging.INFO, format="%(asctime)-15s %(message)s")
    return args


def finish_main(path: str, st: Dict[str, float], detail: str = "") -> str:
    """The summary line of a module's command line (``detail``: what the module adds in brackets), the read-cap warnings and the
    sentinel."""
    logging.info("%d active regions -> %d sites, %d alleles, %d reads in %s%s", st.get("active_regions", 0), st.get("sites", 0),
                 st.get("alleles", 0), st.get("reads_gathered", 0), path, detail)
    for key in ("regions_at_read_cap", "clusters_at_read_cap"):
        if st.get(key):
            logging.warning("%d %s: their first reads in file order were kept", st[key], key.replace("_", " "))
    logging.info("Completed running the script")
    return path


def main(argv=None) -> str:
    args = start_main(parser(), argv)
    if args.pacbio or args.hybrid_hotspot or len(args.bam.split(",")) != 1:
        raise ValueError(REFUSAL)
    logging.info("Started script")
    path, st = run_activity(args.bam, args.ref, args.activity, args.outputPrefix, args.featureLength, args.q_threshold,
                            args.mapq_threshold, args.device)
    return finish_main(path, st)


if __name__ == "__main__":
    main(sys.argv[1:])
