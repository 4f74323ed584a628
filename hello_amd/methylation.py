"""CpG methylation per haplotype from the MM / ML tags of a sorted PacBio BAM, counted on the GPU.

    python -m hello_amd.call --from_bam --pbam P | --from_bams [--resident] ... --methylation [--phase | --haplotag_vcf V]
    python -m hello_amd.methylation --bam B --ref F --output_prefix P [--phased_vcf V] [--chromosomes a,b]
                                    [--mapq_threshold 10] [--device N]

Not in the reference; DESIGN.md section 7m defines the rules.  ``parse_mm``, ``listed``, ``observations_of``, ``tables_of`` and
``restated`` restate them in plain Python / NumPy without a GPU; ``Counter`` binds ``hello_meth_*``
(hello_amd/csrc/methylation.hip), which equal the restatement integer for integer.  ``measure`` is the pass over one BAM: per
chromosome one batch of reads per span of at most ``hotspots.MAX_LAUNCH_BASES`` positions -- a read belongs to the span that holds
its start, so no table depends on the spans.  A read's haplotype is its ``hp``: the BAM's own HP tag, or what a
``haplotag.Haplotagger`` gives it from a phased VCF.  Its result, ``Methylation``, holds SITES and COUNTS per chromosome.
"""
from __future__ import annotations

import argparse
import ctypes as C
import logging
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._abi import ARRAY_GETTER, READS, STATS_GETTER, bind, check, i32, i64, vp
from .bam import Mods, Reads
from .gvcf import _bytes_of, counted
from .spans import Handle, measure_spans, save_tables

NONE, USABLE, BAD = 0, 1, 2                                # a read's modification state
MODIFIED, UNMODIFIED, ML_SUM = range(3)                    # the counters of COUNTS [n_sites, 3, 3]; the classes: all, hap 1, hap 2
THRESHOLD = 128
STATUS_NAMES = ("not_counted", "counting", "bad_mods", "no_mods", "hard_clipped")       # STATUS of the last add, per read
COUNT_NAMES = ("reads_given", "belonging", "counting", "reads_no_mods", "reads_bad_mods", "reads_hard_clipped", "observations",
               "n_sites")
STAT_NAMES = COUNT_NAMES + ("sites_ms", "reads_ms")
METRIC_STATS = COUNT_NAMES[1:]                             # what does not depend on the spans
MAX_COUNTING_READS = (1 << 31) // 255
BED_NAMES = ("combined", "hap1", "hap2")
BED_HEADER = "#chrom\tstart\tend\tpercent_modified\tcoverage\tmodified\tunmodified\tmean_probability\n"

_log = logging.getLogger(__name__)


# ------------------------------------------------------------------------------------------------
# the rules, restated
# ------------------------------------------------------------------------------------------------
def _bad():
    return np.zeros(0, np.int32), np.zeros(0, np.uint8), 0, BAD


def parse_mm(mm: Optional[bytes], ml=None) -> Tuple[np.ndarray, np.ndarray, int, int]:
    """(deltas int32, probabilities uint8, mode, state) of one record: ``mm`` the text of MM:Z (None: the record has none), ``ml``
    the bytes of ML when it is of type B:C (else None).  The group used is ``C+`` with letter codes containing ``m``; every other
    group is skipped and still takes its bytes of ML."""
    if mm is None:
        return np.zeros(0, np.int32), np.zeros(0, np.uint8), 0, NONE
    mm = bytes(mm)
    i, total, found = 0, 0, None
    while i < len(mm):
        base = mm[i:i + 1]
        i += 1
        if base not in (b"A", b"C", b"G", b"T", b"U", b"N") or mm[i:i + 1] not in (b"+", b"-"):
            return _bad()
        strand = mm[i:i + 1]
        i += 1
        j = i
        if mm[j:j + 1].isdigit():
            while mm[j:j + 1].isdigit():
                j += 1
            codes, letters = 1, b""
        else:
            while b"a" <= mm[j:j + 1] <= b"z":
                j += 1
            codes, letters = j - i, mm[i:j]
        if codes == 0:
            return _bad()
        i, mode = j, 0
        if mm[i:i + 1] in (b".", b"?"):
            mode = int(mm[i:i + 1] == b"?")
            i += 1
        mine = base == b"C" and strand == b"+" and b"m" in letters
        if mine and found is not None:
            return _bad()
        deltas = []
        while mm[i:i + 1] == b",":
            j = i + 1
            while mm[j:j + 1].isdigit():
                j += 1
            if j == i + 1 or int(mm[i + 1:j]) > 0x7FFFFFFF:
                return _bad()
            deltas.append(int(mm[i + 1:j]))
            i = j
        if mm[i:i + 1] != b";":
            return _bad()
        i += 1
        if mine:
            found = (deltas, total, codes, letters.index(b"m"), mode)
        total += len(deltas) * codes
    if found is None:
        return np.zeros(0, np.int32), np.zeros(0, np.uint8), 0, NONE
    if ml is None or len(ml) != total:
        return _bad()
    deltas, offset, codes, at, mode = found
    ml = np.frombuffer(bytes(ml), np.uint8) if not isinstance(ml, np.ndarray) else ml.astype(np.uint8)
    return np.array(deltas, np.int32), ml[offset + at:offset + len(deltas) * codes:codes].copy(), mode, USABLE


def listed(bases: np.ndarray, reverse: bool, deltas) -> Optional[np.ndarray]:
    """The stored indices of the listed bases of a read, entry by entry, or None when the last one does not exist.  The candidates
    are the stored ``C`` from the left, or for a reverse read the stored ``G`` from the right; entry k names candidate
    k + delta_0 + .. + delta_k."""
    at = np.flatnonzero(np.asarray(bases) == (ord("G") if reverse else ord("C")))
    if reverse:
        at = at[::-1]
    t = np.arange(len(deltas), dtype=np.int64) + np.cumsum(np.asarray(deltas, np.int64))
    if t.shape[0] and t[-1] >= at.shape[0]:
        return None
    return at[t]


def sites_of(reference) -> np.ndarray:
    """int64: the positions p with C at p and G at p + 1, either case."""
    ref = _bytes_of(reference) & 0xDF
    return np.flatnonzero((ref[:-1] == ord("C")) & (ref[1:] == ord("G"))).astype(np.int64) if ref.shape[0] > 1 else np.zeros(0, np.int64)


def _no_hard_clip(rd: Reads, r: int) -> bool:
    return not any(int(c) & 15 == 5 for c in rd.cigars[int(rd.cigar_offsets[r]):int(rd.cigar_offsets[r + 1])])


def observations_of(rd: Reads, mods: Mods, r: int, is_site: np.ndarray) -> Optional[List[Tuple[int, int]]]:
    """[(site position, value)] of read ``r`` whose state is 1, in stored order, or None when its last listed base does not exist.
    ``is_site``: bool per position of the chromosome."""
    b0, b1 = int(rd.read_offsets[r]), int(rd.read_offsets[r + 1])
    bases, reverse = rd.bases[b0:b1], bool(int(rd.flags[r]) & 0x10)
    m0, m1 = int(mods.offsets[r]), int(mods.offsets[r + 1])
    where = listed(bases, reverse, mods.deltas[m0:m1])
    if where is None:
        return None
    value = {int(i): int(v) for i, v in zip(where, mods.probs[m0:m1])}
    ops = [(int(c) & 15, int(c) >> 4) for c in rd.cigars[int(rd.cigar_offsets[r]):int(rd.cigar_offsets[r + 1])]]
    if any(op > 8 for op, _ in ops) or sum(k for op, k in ops if op in (0, 1, 4, 7, 8)) != b1 - b0:
        raise ValueError(f"read {r}: its CIGAR does not consume exactly its {b1 - b0} bases")
    candidate, shift = (ord("G"), 1) if reverse else (ord("C"), 0)
    out, pos, i = [], int(rd.ref_starts[r]), 0
    for op, k in ops:
        if op in (0, 7, 8):
            for j in range(k):
                p = pos + j - shift
                if bases[i + j] == candidate and pos + j < is_site.shape[0] and p >= 0 and is_site[p]:
                    if i + j in value:
                        out.append((p, value[i + j]))
                    elif int(mods.mode[r]) == 0:
                        out.append((p, 0))
            pos, i = pos + k, i + k
        elif op in (1, 4):
            i += k
        elif op in (2, 3):
            pos += k
    return out


def tables_of(reads: Reads, mods: Mods, reference, lo: int, hi: int, mapq_threshold: int = 10) -> Dict[str, object]:
    """One span [lo, hi) of the chromosome ``reference`` and the reads overlapping it with their modifications -> SITES, COUNTS,
    ``counts`` (COUNT_NAMES) and ``status`` (uint8 per read, STATUS_NAMES)."""
    ref = _bytes_of(reference)
    if not 0 <= lo < hi <= ref.shape[0]:
        raise ValueError("a span that leaves the reference")
    sites = sites_of(ref)
    is_site = np.zeros(ref.shape[0], bool)
    is_site[sites] = True
    table = np.zeros((sites.shape[0], 3, 3), np.int64)
    status = np.zeros(reads.n_reads, np.uint8)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    counts.update(reads_given=reads.n_reads, n_sites=int(sites.shape[0]))
    for r in range(reads.n_reads):
        if int(reads.ref_starts[r]) < lo:
            continue
        counts["belonging"] += 1
        if not counted(int(reads.flags[r]), int(reads.mapq[r]), mapq_threshold):
            continue
        state = int(mods.state[r])
        seen = observations_of(reads, mods, r, is_site) if _no_hard_clip(reads, r) and state == USABLE else None
        if not _no_hard_clip(reads, r):
            status[r], key = 4, "reads_hard_clipped"
        elif state == NONE:
            status[r], key = 3, "reads_no_mods"
        elif state == BAD or seen is None:
            status[r], key = 2, "reads_bad_mods"
        else:
            status[r], key = 1, "counting"
        counts[key] += 1
        if status[r] != 1:
            continue
        counts["observations"] += len(seen)
        hp = int(reads.hp[r])
        for p, v in seen:
            s = int(np.searchsorted(sites, p))
            for cls in (0, hp) if hp in (1, 2) else (0,):
                table[s, cls, MODIFIED if v >= THRESHOLD else UNMODIFIED] += 1
                table[s, cls, ML_SUM] += v
    return dict(SITES=sites, COUNTS=table, counts=counts, status=status)


def restated(spans: Sequence[Tuple[Reads, Mods, int, int]], reference, mapq_threshold: int = 10) -> Tuple[Dict[str, np.ndarray], Dict[str, int]]:
    """({SITES, COUNTS}, the counts) of one chromosome given as (reads, mods, lo, hi) span after span, from the restatement."""
    ref = _bytes_of(reference)
    sites = sites_of(ref)
    total = dict(SITES=sites, COUNTS=np.zeros((sites.shape[0], 3, 3), np.int64))
    counts = dict.fromkeys(COUNT_NAMES, 0)
    counts["n_sites"] = int(sites.shape[0])
    for reads, mods, lo, hi in spans:
        part = tables_of(reads, mods, ref, lo, hi, mapq_threshold)
        total["COUNTS"] += part["COUNTS"]
        for k, v in part["counts"].items():
            if k != "n_sites":
                counts[k] += v
    return total, counts


# ------------------------------------------------------------------------------------------------
# the GPU
# ------------------------------------------------------------------------------------------------
_PROTOTYPES = (
    ("hello_meth_create", [vp, i64, i32, i32, C.POINTER(vp)]),
    ("hello_meth_add", [vp] + READS + [i64, vp, i64, vp, i64, vp, vp, vp, i64, i64]),
    ("hello_meth_array", ARRAY_GETTER),
    ("hello_meth_stats", STATS_GETTER),
    ("hello_meth_free", [vp], None),
)


def _lib():
    return bind(_PROTOTYPES)


class Counter(Handle):
    """One (BAM, chromosome)'s ``hello_meth`` handle: creating it flags the CpG sites of ``reference`` on the device, ``add`` takes
    the reads overlapping a span with their modifications, ``arrays`` gives SITES, COUNTS and the STATUS of the last ``add``."""
    NAME, STAT_NAMES, TIMES = "meth", STAT_NAMES, STAT_NAMES[len(COUNT_NAMES):]
    ARRAYS = (("SITES", 0, np.int64, None), ("COUNTS", 1, np.int64, (-1, 3, 3)), ("STATUS", 2, np.uint8, None))

    def __init__(self, reference, mapq_threshold: int = 10, device: int = 0):
        ref = np.ascontiguousarray(_bytes_of(reference))
        super().__init__(_lib())
        check(self._lib.hello_meth_create(ref.ctypes.data, int(ref.shape[0]), int(mapq_threshold), int(device), C.byref(self._h)))

    def add(self, reads: Reads, mods: Mods, lo: int, hi: int) -> None:
        check(self._lib.hello_meth_add(self._h, *reads.pointers(reads.hp), int(reads.n_reads), mods.deltas.ctypes.data,
                                       int(mods.deltas.shape[0]), mods.probs.ctypes.data, int(mods.probs.shape[0]),
                                       mods.offsets.ctypes.data, mods.mode.ctypes.data, mods.state.ctypes.data, int(lo), int(hi)))


def counted_on_gpu(spans: Sequence[Tuple[Reads, Mods, int, int]], reference, mapq_threshold: int = 10,
                   device: int = 0) -> Tuple[Dict[str, np.ndarray], Dict[str, float]]:
    """``restated`` on the GPU: ({SITES, COUNTS, STATUS of the last span}, the statistics of ``hello_meth_stats``)."""
    with Counter(reference, mapq_threshold, device) as counter:
        for reads, mods, lo, hi in spans:
            counter.add(reads, mods, lo, hi)
        return counter.arrays(), counter.stats()


# ------------------------------------------------------------------------------------------------
# the methylation of one BAM
# ------------------------------------------------------------------------------------------------
def _bed_line(chromosome: str, p: int, row) -> str:
    modified, unmodified, ml_sum = (int(x) for x in row)
    coverage = modified + unmodified
    return "%s\t%d\t%d\t%.1f\t%d\t%d\t%d\t%.4f\n" % (chromosome, p, p + 2, 100 * modified / coverage, coverage, modified, unmodified,
                                                     (ml_sum + coverage / 2) / (256 * coverage))


class Methylation:
    """``tables[chromosome]``: SITES int64 [n], COUNTS int64 [n, 3, 3] (class: all, haplotype 1, haplotype 2; counter: modified,
    unmodified, ml_sum) and STATS (int64, METRIC_STATS)."""

    def __init__(self):
        self.tables: Dict[str, Dict[str, np.ndarray]] = {}

    def set(self, chromosome: str, tables: Dict[str, np.ndarray], counts: Dict[str, float]) -> None:
        self.tables[chromosome] = dict(SITES=np.asarray(tables["SITES"], np.int64), COUNTS=np.asarray(tables["COUNTS"], np.int64),
                                       STATS=np.array([int(counts[k]) for k in METRIC_STATS], np.int64))

    def total(self) -> Dict[str, int]:
        return {k: sum(int(t["STATS"][i]) for t in self.tables.values()) for i, k in enumerate(METRIC_STATS)}

    def save(self, path: str) -> str:
        names = list(self.tables)
        out = dict(chromosomes=np.array(names, dtype=np.str_))
        for i, c in enumerate(names):
            for name, a in self.tables[c].items():
                out["%s_%d" % (name, i)] = a
        return save_tables(path, out)

    @classmethod
    def load(cls, path: str) -> "Methylation":
        with np.load(path, allow_pickle=False) as z:
            out = cls()
            for i, c in enumerate(str(c) for c in z["chromosomes"]):
                out.tables[c] = {name: z["%s_%d" % (name, i)] for name in ("SITES", "COUNTS", "STATS")}
        return out

    def write_bed(self, prefix: str) -> List[str]:
        """``<prefix>.combined.bed``, ``.hap1.bed`` and ``.hap2.bed``: a header line, then per site with coverage in the class
        ``chrom p p+2 percent_modified coverage modified unmodified mean_probability``."""
        written = []
        for cls, name in enumerate(BED_NAMES):
            path = "%s.%s.bed" % (prefix, name)
            with open(path, "w") as fh:
                fh.write(BED_HEADER)
                for c, t in self.tables.items():
                    rows = t["COUNTS"][:, cls]
                    for s in np.flatnonzero(rows[:, MODIFIED] + rows[:, UNMODIFIED]):
                        fh.write(_bed_line(c, int(t["SITES"][s]), rows[s]))
            written.append(path)
        return written


def measure(bam: str, fasta, chromosomes: Optional[Sequence[str]] = None, haplotagger=None, mapq_threshold: int = 10,
            max_span: Optional[int] = None, device: int = 0, restatement: bool = False, stats: Optional[dict] = None) -> Methylation:
    """The methylation of one BAM, chromosome after chromosome (default: every sequence of the FASTA).  ``fasta``: a path, or
    {chromosome: sequence}; ``haplotagger``: its ``retag(chromosome, reads)`` replaces the BAM's own HP; ``restatement``: from the
    plain-Python rules instead of the GPU.  ``stats``: the library's kernel times and the seconds of decoding (``decode_s``), of
    the library's calls (``device_s``) and of the whole pass (``total_s``) are added."""
    out = Methylation()
    measure_spans(bam, fasta, chromosomes, max_span, stats, restatement,
                  open_handle=lambda c, ref: Counter(ref, mapq_threshold, device),
                  restated=lambda c, ref, spans: restated(spans, ref, mapq_threshold),
                  done=lambda c, ref, tables, counts: out.set(c, tables, counts),
                  with_mods=True, retag=haplotagger.retag if haplotagger is not None else None)
    return out


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="CpG methylation per haplotype from the MM / ML tags of a coordinate-sorted BAM, counted on the GPU")
    p.add_argument("--bam", required=True, help="The BAM (with its .bai, or scanned)")
    p.add_argument("--ref", required=True, help="Reference FASTA")
    p.add_argument("--output_prefix", required=True, help="Writes <prefix>.combined.bed, .hap1.bed, .hap2.bed and <prefix>.npz")
    p.add_argument("--phased_vcf", help="A phased VCF (a|b records with PS): the reads' haplotypes come from it, not from the HP tags")
    p.add_argument("--chromosomes", help="Comma-separated chromosomes (default: every sequence of the FASTA)")
    p.add_argument("--mapq_threshold", type=int, default=10, help="A read below it does not count")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def main(argv=None) -> List[str]:
    args = parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)-15s %(message)s")
    chromosomes = args.chromosomes.split(",") if args.chromosomes else None
    tagger = None
    if args.phased_vcf:
        from .haplotag import Haplotagger
        tagger = Haplotagger(args.phased_vcf, chromosomes, 10, args.mapq_threshold, args.device)
    stats: dict = {}
    try:
        found = measure(args.bam, args.ref, chromosomes, tagger, args.mapq_threshold, device=args.device, stats=stats)
    finally:
        if tagger is not None:
            tagger.close()
    total = found.total()
    _log.info("%d sites, %d reads counting, %d observations (kernels %.1f ms)", total["n_sites"], total["counting"],
              total["observations"], stats.get("sites_ms", 0.0) + stats.get("reads_ms", 0.0))
    return found.write_bed(args.output_prefix) + [found.save(args.output_prefix + ".npz")]


if __name__ == "__main__":
    main(sys.argv[1:])
