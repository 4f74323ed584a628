"""Alignment, coverage and insert-size metrics of a sorted BAM, counted on the GPU: what went into a run.

    python -m hello_amd.call --from_bam | --from_bams [--resident] ... --qc [--qc_regions BED] [--qc_window 1000]
    python -m hello_amd.qc --bam B --ref F --output_prefix P [--regions BED] [--window N] [--chromosomes a,b]
                           [--mapq_threshold 10] [--device N]

Not in the reference; DESIGN.md section 7k defines the rules.  ``measured``, ``cycle_of``, ``read_tables``, ``depth_of``,
``insert_of`` and ``tables_of`` restate them in plain Python / NumPy without a GPU; ``Meter`` binds ``hello_qc_*``
(hello_amd/csrc/qc.hip), which equal the restatement integer for integer.  ``measure`` is the pass over one BAM: per chromosome one
batch of reads per span of at most ``hotspots.MAX_LAUNCH_BASES`` positions -- a read belongs to the span that holds its start, the
depth counts the span's positions from every read that overlaps it, so no table depends on the spans -- and the mate join
chromosome-wide.  Its result, ``Metrics``, holds the integer tables per chromosome; ``summary`` derives every ratio from them.
"""
from __future__ import annotations

import argparse
import ctypes as C
import logging
import math
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._abi import ARRAY_GETTER, READS, STATS_GETTER, bind, check, i32, i64, vp
from .bam import Reads
from .gvcf import _bytes_of, counted
from .phase import join_mates
from .spans import Handle, measure_spans, save_tables

NOT_MEASURED = 0x4 | 0x100 | 0x800 | 0x400 | 0x200      # unmapped, secondary, supplementary, duplicate, QC-fail
FLAG_NAMES = ("reads", "unmapped", "secondary", "supplementary", "duplicate", "qc_fail", "paired", "proper_pair", "read1", "read2",
              "mate_unmapped", "reverse", "mapq0")
CYCLE_FIELDS = ("bases", "quality_sum", "aligned", "mismatches", "inserted", "soft_clipped", "deletions")
BASES, QUALITY_SUM, ALIGNED, MISMATCHES, INSERTED, SOFT_CLIPPED, DELETIONS = range(7)
ORIENTATIONS = ("FR", "RF", "TANDEM")
LAST_CYCLE, LAST_LENGTH, LAST_DEPTH, LAST_INSERT = 512, 65535, 1023, 4095
TABLE_NAMES = ("FLAGS", "MAPQ", "LENGTH", "CYCLE", "QUALITY", "DEPTH_HIST", "WINDOW_SUM", "TARGET_DEPTH_HIST", "TARGET_SUM",
               "TARGET_COVERED", "INSERT")                  # in the order of HELLO_QC_*
SHAPES = dict(FLAGS=(13,), MAPQ=(256,), LENGTH=(LAST_LENGTH + 1,), CYCLE=(2, LAST_CYCLE + 1, 7), QUALITY=(256, 2),
              DEPTH_HIST=(LAST_DEPTH + 1,), TARGET_DEPTH_HIST=(LAST_DEPTH + 1,), INSERT=(3, LAST_INSERT + 1))
COUNT_NAMES = ("reads_given", "belonging", "measured", "counted", "reads_past_reference", "positions_excluded", "pairs",
               "groups_refused")
STAT_NAMES = COUNT_NAMES + ("reads_ms", "depth_ms", "pair_ms", "insert_ms")
METRIC_STATS = COUNT_NAMES[2:]                              # what does not depend on the spans: written beside FLAGS
DEPTH_LEVELS = (1, 5, 10, 15, 20, 30, 50)
DEFAULT_WINDOW = 1000

Targets = Sequence[Tuple[int, int]]
_log = logging.getLogger(__name__)
_ACGT = np.zeros(256, bool)
_ACGT[list(b"ACGT")] = True


# ------------------------------------------------------------------------------------------------
# the rules, restated
# ------------------------------------------------------------------------------------------------
def measured(flags) -> np.ndarray:
    """bool [reads]: mapped, primary, not supplementary, not a duplicate, not QC-fail; mapq and the pairing flags do not matter."""
    return (np.asarray(flags).astype(np.int64) & NOT_MEASURED) == 0


def cycle_of(i, length: int, reverse: bool):
    """The cycle of stored base ``i`` of a read of ``length`` stored bases: its index in sequencing order, clamped to 512."""
    return np.minimum(length - 1 - i if reverse else i, LAST_CYCLE)


def flag_row(flag: int, mapq: int) -> List[int]:
    """One read's contribution to FLAGS."""
    return [1, int(bool(flag & 0x4)), int(bool(flag & 0x100)), int(bool(flag & 0x800)), int(bool(flag & 0x400)),
            int(bool(flag & 0x200)), int(bool(flag & 0x1)), int(flag & 0x3 == 0x3), int(bool(flag & 0x40)), int(bool(flag & 0x80)),
            int(flag & 0x9 == 0x9), int(bool(flag & 0x10)), int(not flag & 0x4 and mapq == 0)]


def empty_tables(reference_length: int, n_targets: int = 0, window: int = DEFAULT_WINDOW) -> Dict[str, np.ndarray]:
    out = {name: np.zeros(shape, np.int64) for name, shape in SHAPES.items()}
    out["WINDOW_SUM"] = np.zeros(-(-reference_length // window), np.int64)
    out["TARGET_SUM"], out["TARGET_COVERED"] = np.zeros(n_targets, np.int64), np.zeros(n_targets, np.int64)
    return out


def read_tables(rd: Reads, r: int, reference: np.ndarray, out: Dict[str, np.ndarray]) -> bool:
    """Adds measured read ``r`` into MAPQ, LENGTH, CYCLE and QUALITY of ``out`` -> whether an aligned base lies at or behind the
    reference's end (such a base counts in ``bases`` and ``quality_sum`` only)."""
    b0, b1 = int(rd.read_offsets[r]), int(rd.read_offsets[r + 1])
    n, flag = b1 - b0, int(rd.flags[r])
    ops = [(int(c) & 15, int(c) >> 4) for c in rd.cigars[int(rd.cigar_offsets[r]):int(rd.cigar_offsets[r + 1])]]
    if any(op > 8 for op, _ in ops) or sum(k for op, k in ops if op in (0, 1, 4, 7, 8)) != n:
        raise ValueError(f"read {r}: its CIGAR does not consume exactly its {n} bases")
    out["MAPQ"][int(rd.mapq[r])] += 1
    out["LENGTH"][min(n, LAST_LENGTH)] += 1
    table, quality = out["CYCLE"][1 if flag & 0x80 else 0], out["QUALITY"]
    cycle = cycle_of(np.arange(n), n, bool(flag & 0x10))
    q = rd.quals[b0:b1].astype(np.int64)
    np.add.at(table[:, BASES], cycle, 1)
    np.add.at(table[:, QUALITY_SUM], cycle, q)
    p, i, past = int(rd.ref_starts[r]), 0, False
    for op, k in ops:
        if op in (0, 7, 8):
            inside = max(0, min(k, reference.shape[0] - p))             # the bases that have a reference position
            past = past or inside < k
            if inside:
                u, v = rd.bases[b0 + i:b0 + i + inside] & 0xDF, reference[p:p + inside] & 0xDF
                aligned = _ACGT[u] & _ACGT[v]
                wrong = aligned & (u != v)
                np.add.at(table[:, ALIGNED], cycle[i:i + inside][aligned], 1)
                np.add.at(table[:, MISMATCHES], cycle[i:i + inside][wrong], 1)
                np.add.at(quality[:, 0], q[i:i + inside][aligned], 1)
                np.add.at(quality[:, 1], q[i:i + inside][wrong], 1)
            p, i = p + k, i + k
        elif op in (1, 4):
            np.add.at(table[:, INSERTED if op == 1 else SOFT_CLIPPED], cycle[i:i + k], 1)
            i += k
        elif op == 2:
            if n:
                table[cycle[min(i, n - 1)], DELETIONS] += 1
            p += k
        elif op == 3:
            p += k
    return past


def depth_of(rd: Reads, lo: int, hi: int, mapq_threshold: int = 10) -> np.ndarray:
    """int64 [hi - lo]: the counted reads with an M / = / X / D operation over each position of [lo, hi)."""
    depth = np.zeros(hi - lo + 1, np.int64)
    for r in range(rd.n_reads):
        if not counted(int(rd.flags[r]), int(rd.mapq[r]), mapq_threshold):
            continue
        p = int(rd.ref_starts[r])
        for c in rd.cigars[int(rd.cigar_offsets[r]):int(rd.cigar_offsets[r + 1])]:
            op, k = int(c) & 15, int(c) >> 4
            if op in (0, 2, 7, 8):
                a, b = max(p, lo), min(p + k, hi)
                if b > a:
                    depth[a - lo] += 1
                    depth[b - lo] -= 1
            if op in (0, 2, 3, 7, 8):
                p += k
    return np.cumsum(depth)[:-1]


def insert_of(name_hash, flags, ref_starts, ref_ends) -> Tuple[np.ndarray, Dict[str, int]]:
    """(INSERT int64 [3, 4096], {pairs, groups_refused}) over the belonging measured reads of one chromosome: the mate join of
    section 7i, every pair once; insert = max(ref_end) - min(ref_start); TANDEM when both mates have one strand, else FR when the
    forward mate starts below the reverse mate's end, else RF."""
    n = len(flags)
    mate, counts = join_mates(name_hash, flags, np.zeros(n, np.uint8), np.ones(n, bool))
    table = np.zeros(SHAPES["INSERT"], np.int64)
    for c in range(n):
        m = int(mate[c])
        if m <= c:
            continue
        insert = max(int(ref_ends[c]), int(ref_ends[m])) - min(int(ref_starts[c]), int(ref_starts[m]))
        r0, r1 = bool(int(flags[c]) & 0x10), bool(int(flags[m]) & 0x10)
        if r0 == r1:
            orientation = 2
        else:
            forward, reverse = (m, c) if r0 else (c, m)
            orientation = 0 if int(ref_starts[forward]) < int(ref_ends[reverse]) else 1
        table[orientation, min(insert, LAST_INSERT)] += 1
    return table, counts


def check_targets(targets: Targets) -> np.ndarray:
    """int64 [n, 2]: sorted intervals with 0 <= start < stop that do not overlap (they may touch)."""
    t = np.asarray(list(targets), np.int64).reshape(-1, 2)
    for i in range(t.shape[0]):
        if t[i, 0] < 0 or t[i, 0] >= t[i, 1] or (i and t[i, 0] < t[i - 1, 1]):
            raise ValueError(f"target {i}: [{t[i, 0]}, {t[i, 1]}) is empty, or not sorted behind its predecessor")
    return t


def tables_of(reads: Reads, reference, lo: int, hi: int, targets: Targets = (), window: int = DEFAULT_WINDOW,
              mapq_threshold: int = 10) -> Dict[str, object]:
    """One span [lo, hi) of the chromosome ``reference`` and the reads overlapping it -> every table but INSERT, ``counts``
    (COUNT_NAMES without the pairs) and ``pairing``: name_hash, flags, ref_starts, ref_ends of the belonging measured reads."""
    ref, t = _bytes_of(reference), check_targets(targets)
    if window < 1 or not 0 <= lo < hi <= ref.shape[0]:
        raise ValueError("window below 1, or a span that leaves the reference")
    out = empty_tables(ref.shape[0], t.shape[0], window)
    belongs = reads.ref_starts >= lo
    is_measured = measured(reads.flags)
    past = 0
    for r in np.flatnonzero(belongs):
        out["FLAGS"] += flag_row(int(reads.flags[r]), int(reads.mapq[r]))
        if is_measured[r]:
            past += read_tables(reads, int(r), ref, out)
    depth = depth_of(reads, lo, hi, mapq_threshold)
    acgt = _ACGT[ref[lo:hi] & 0xDF]
    bins = np.minimum(depth, LAST_DEPTH)
    np.add.at(out["DEPTH_HIST"], bins[acgt], 1)
    np.add.at(out["WINDOW_SUM"], np.arange(lo, hi) // window, depth)
    for k in range(t.shape[0]):
        a, b = max(int(t[k, 0]), lo), min(int(t[k, 1]), hi)
        if b > a:
            inside = depth[a - lo:b - lo]
            np.add.at(out["TARGET_DEPTH_HIST"], bins[a - lo:b - lo][acgt[a - lo:b - lo]], 1)
            out["TARGET_SUM"][k] += int(inside.sum())
            out["TARGET_COVERED"][k] += int((inside >= 1).sum())
    mine = np.flatnonzero(belongs & is_measured)
    is_counted = np.array([counted(int(f), int(q), mapq_threshold) for f, q in zip(reads.flags, reads.mapq)], bool)
    out["counts"] = dict(reads_given=reads.n_reads, belonging=int(belongs.sum()), measured=int(mine.shape[0]),
                         counted=int((belongs & is_counted).sum()), reads_past_reference=past, positions_excluded=int((~acgt).sum()))
    out["pairing"] = (reads.name_hash[mine], reads.flags[mine], reads.ref_starts[mine], reads.ref_ends[mine])
    return out


def restated(spans: Sequence[Tuple[Reads, int, int]], reference, targets: Targets = (), window: int = DEFAULT_WINDOW,
             mapq_threshold: int = 10) -> Tuple[Dict[str, np.ndarray], Dict[str, int]]:
    """(the eleven tables, the eight counts) of one chromosome given as (reads, lo, hi) span after span, from the restatement."""
    ref = _bytes_of(reference)
    total = empty_tables(ref.shape[0], len(list(targets)), window)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    pairing: List[tuple] = []
    for reads, lo, hi in spans:
        part = tables_of(reads, ref, lo, hi, targets, window, mapq_threshold)
        for name in total:
            if name != "INSERT":
                total[name] += part[name]
        for k, v in part["counts"].items():
            counts[k] += v
        pairing.append(part["pairing"])
    joined = [np.concatenate([p[i] for p in pairing]) if pairing else np.zeros(0, np.int64) for i in range(4)]
    total["INSERT"], pairs = insert_of(*joined)
    counts.update(pairs)
    return total, counts


# ------------------------------------------------------------------------------------------------
# the GPU
# ------------------------------------------------------------------------------------------------
_PROTOTYPES = (
    ("hello_qc_add", READS + [i64, vp, i64, i64, i64, vp, vp, i64, i32, i64, i32, C.POINTER(vp)]),
    ("hello_qc_finish", [vp]),
    ("hello_qc_array", ARRAY_GETTER),
    ("hello_qc_stats", STATS_GETTER),
    ("hello_qc_free", [vp], None),
)


def _lib():
    return bind(_PROTOTYPES)


class Meter(Handle):
    """One (BAM, chromosome)'s ``hello_qc`` handle: ``add`` takes the reads overlapping a span, ``finish`` (once, after the last
    ``add``) joins the mates and fills INSERT, ``arrays`` gives the tables by name."""
    NAME, STAT_NAMES, TIMES = "qc", STAT_NAMES, STAT_NAMES[len(COUNT_NAMES):]
    ARRAYS = tuple((name, which, np.int64, SHAPES.get(name)) for which, name in enumerate(TABLE_NAMES))

    def __init__(self, reference, targets: Targets = (), window: int = DEFAULT_WINDOW, mapq_threshold: int = 10, device: int = 0):
        self._ref = np.ascontiguousarray(_bytes_of(reference))
        t = np.asarray(list(targets), np.int64).reshape(-1, 2)               # the library refuses what check_targets would
        self._starts, self._stops = np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])
        self._window, self._threshold, self._device = int(window), int(mapq_threshold), int(device)
        super().__init__(_lib())
        self._finished = False

    def add(self, reads: Reads, lo: int, hi: int) -> None:
        check(self._lib.hello_qc_add(*reads.pointers(reads.hp)[:10], None, int(reads.n_reads), self._ref.ctypes.data,
                                     int(self._ref.shape[0]), int(lo), int(hi), self._starts.ctypes.data, self._stops.ctypes.data,
                                     int(self._starts.shape[0]), self._threshold, self._window, self._device, C.byref(self._h)))

    def finish(self) -> None:
        check(self._lib.hello_qc_finish(self._h))
        self._finished = True

    def _has(self, name: str) -> bool:
        return name != "INSERT" or self._finished

    def results(self):
        self.finish()
        return super().results()


def metered(spans: Sequence[Tuple[Reads, int, int]], reference, targets: Targets = (), window: int = DEFAULT_WINDOW,
            mapq_threshold: int = 10, device: int = 0) -> Tuple[Dict[str, np.ndarray], Dict[str, float]]:
    """``restated`` on the GPU: (the eleven tables, the statistics of ``hello_qc_stats``).  At least one span."""
    with Meter(reference, targets, window, mapq_threshold, device) as meter:
        for reads, lo, hi in spans:
            meter.add(reads, lo, hi)
        return meter.results()


# ------------------------------------------------------------------------------------------------
# the summary: float64 from the integer tables alone
# ------------------------------------------------------------------------------------------------
def _ratio(a, b) -> float:
    return float(a) / float(b) if b else 0.0


def histogram_median(hist) -> int:
    """The smallest value whose cumulative count reaches half of the histogram's total; 0 for an empty histogram."""
    hist = np.asarray(hist, np.int64)
    total = int(hist.sum())
    if total == 0:
        return 0
    return int(np.argmax(2 * np.cumsum(hist) >= total))


def _depth_summary(prefix: str, hist) -> List[Tuple[str, float]]:
    hist = np.asarray(hist, np.int64)
    total = int(hist.sum())
    out = [(prefix + "mean_depth", _ratio(int((hist * np.arange(hist.shape[0])).sum()), total)),
           (prefix + "median_depth", float(histogram_median(hist)))]
    return out + [(prefix + "depth_ge_%d" % level, _ratio(int(hist[level:].sum()), total)) for level in DEPTH_LEVELS]


def summary(tables: Dict[str, np.ndarray], with_targets: bool = False) -> Dict[str, float]:
    """Every derived figure, in the order it is written.  Fractions are of FLAGS' reads; the depth figures of the positions with an
    ACGT reference base (the last bin counts as 1 023); the empirical quality of reported quality q is -10 log10((mismatches + 1) /
    (aligned + 2)); the insert median and MAD are of the FR pairs below the last bin."""
    flags = dict(zip(FLAG_NAMES, (int(v) for v in tables["FLAGS"])))
    out: List[Tuple[str, float]] = [("mapped_fraction", _ratio(flags["reads"] - flags["unmapped"], flags["reads"])),
                                    ("duplicate_fraction", _ratio(flags["duplicate"], flags["reads"])),
                                    ("proper_pair_fraction", _ratio(flags["proper_pair"], flags["reads"]))]
    out += _depth_summary("", tables["DEPTH_HIST"])
    if with_targets:
        out += _depth_summary("target_", tables["TARGET_DEPTH_HIST"])
    cycle = np.asarray(tables["CYCLE"], np.int64)
    out.append(("mismatch_rate", _ratio(int(cycle[:, :, MISMATCHES].sum()), int(cycle[:, :, ALIGNED].sum()))))
    for end in range(2):
        for c in np.flatnonzero(cycle[end, :, BASES]):
            out.append(("read%d.cycle%d.mean_quality" % (end + 1, c), _ratio(int(cycle[end, c, QUALITY_SUM]), int(cycle[end, c, BASES]))))
    quality = np.asarray(tables["QUALITY"], np.int64)
    for q in np.flatnonzero(quality[:, 0]):
        out.append(("quality%d.empirical" % q, -10.0 * math.log10((int(quality[q, 1]) + 1) / (int(quality[q, 0]) + 2))))
    insert = np.asarray(tables["INSERT"], np.int64)
    fr = insert[0, :LAST_INSERT]
    median = histogram_median(fr)
    deviation = np.zeros(LAST_INSERT, np.int64)
    np.add.at(deviation, np.abs(np.arange(LAST_INSERT) - median), fr)
    pairs = int(insert.sum())
    out += [("insert_median", float(median)), ("insert_mad", float(histogram_median(deviation)))]
    out += [("%s_fraction" % name.lower(), _ratio(int(insert[k].sum()), pairs)) for k, name in enumerate(ORIENTATIONS)]
    return dict(out)


# ------------------------------------------------------------------------------------------------
# the metrics of one BAM
# ------------------------------------------------------------------------------------------------
class Metrics:
    """The tables of one BAM: ``tables[chromosome][name]`` for TABLE_NAMES and ``STATS`` (int64, METRIC_STATS), with the
    chromosomes' ``lengths``, the ``window`` and the ``targets`` (int64 [n, 2] per chromosome) they were counted with."""

    def __init__(self, window: int = DEFAULT_WINDOW, has_targets: bool = False):
        self.window, self.has_targets = int(window), bool(has_targets)      # has_targets: target intervals were asked for
        self.tables: Dict[str, Dict[str, np.ndarray]] = {}
        self.lengths: Dict[str, int] = {}
        self.targets: Dict[str, np.ndarray] = {}

    def set(self, chromosome: str, length: int, tables: Dict[str, np.ndarray], counts: Dict[str, float], targets: Targets = ()) -> None:
        self.tables[chromosome] = dict({k: np.asarray(tables[k], np.int64) for k in TABLE_NAMES},
                                       STATS=np.array([int(counts[k]) for k in METRIC_STATS], np.int64))
        self.lengths[chromosome] = int(length)
        self.targets[chromosome] = np.asarray(list(targets), np.int64).reshape(-1, 2)

    def total(self) -> Dict[str, np.ndarray]:
        """The tables summed over the chromosomes; WINDOW_SUM, TARGET_SUM and TARGET_COVERED one chromosome after the other."""
        out = dict({name: np.zeros(shape, np.int64) for name, shape in SHAPES.items()}, STATS=np.zeros(len(METRIC_STATS), np.int64))
        for t in self.tables.values():
            for name in out:
                out[name] = out[name] + t[name]
        for name in ("WINDOW_SUM", "TARGET_SUM", "TARGET_COVERED"):
            out[name] = np.concatenate([np.zeros(0, np.int64)] + [t[name] for t in self.tables.values()])
        return out

    def summary(self) -> Dict[str, float]:
        return summary(self.total(), self.has_targets)

    def save(self, path: str) -> str:
        names = list(self.tables)
        out = dict(chromosomes=np.array(names, dtype=np.str_), lengths=np.array([self.lengths[c] for c in names], np.int64),
                   window=np.array([self.window, int(self.has_targets)], np.int64))
        for i, c in enumerate(names):
            out["targets_%d" % i] = self.targets[c]
            for name, a in self.tables[c].items():
                out["%s_%d" % (name, i)] = a
        return save_tables(path, out)

    @classmethod
    def load(cls, path: str) -> "Metrics":
        with np.load(path, allow_pickle=False) as z:
            metrics = cls(int(z["window"][0]), bool(z["window"][1]))
            for i, c in enumerate(str(c) for c in z["chromosomes"]):
                metrics.tables[c] = {name: z["%s_%d" % (name, i)] for name in TABLE_NAMES + ("STATS",)}
                metrics.lengths[c] = int(z["lengths"][i])
                metrics.targets[c] = z["targets_%d" % i]
        return metrics

    def write_metrics(self, path: str) -> str:
        """``name<TAB>value`` lines: the integers of FLAGS and METRIC_STATS per chromosome (``<chromosome>.<name>``) and in total
        (``total.<name>``), then the summary (``summary.<name>``, ``%.4f``)."""
        with open(path, "w") as fh:
            for c, t in list(self.tables.items()) + [("total", self.total())]:
                for k, v in list(zip(FLAG_NAMES, t["FLAGS"])) + list(zip(METRIC_STATS, t["STATS"])):
                    fh.write("%s.%s\t%d\n" % (c, k, int(v)))
            for k, v in self.summary().items():
                fh.write("summary.%s\t%.4f\n" % (k, v))
        return path

    def write_windows(self, path: str) -> str:
        """bedGraph: ``chrom start end mean_depth`` per window, the last one ending at the chromosome's end."""
        with open(path, "w") as fh:
            for c, t in self.tables.items():
                for w, total in enumerate(t["WINDOW_SUM"].tolist()):
                    a, b = w * self.window, min((w + 1) * self.window, self.lengths[c])
                    fh.write("%s\t%d\t%d\t%.4f\n" % (c, a, b, _ratio(total, b - a)))
        return path

    def write_targets(self, path: str) -> str:
        """``chrom start end mean_depth covered_fraction`` per target, the target clipped to the chromosome."""
        with open(path, "w") as fh:
            for c, t in self.tables.items():
                for (a, b), total, covered in zip(self.targets[c].tolist(), t["TARGET_SUM"].tolist(), t["TARGET_COVERED"].tolist()):
                    a, b = min(a, self.lengths[c]), min(b, self.lengths[c])
                    fh.write("%s\t%d\t%d\t%.4f\t%.4f\n" % (c, a, b, _ratio(total, b - a), _ratio(covered, b - a)))
        return path

    def write_all(self, prefix: str) -> List[str]:
        """``<prefix>.metrics.txt``, ``.tables.npz``, ``.windows.bedgraph`` and, with targets, ``.targets.tsv``."""
        out = [self.write_metrics(prefix + ".metrics.txt"), self.save(prefix + ".tables.npz"), self.write_windows(prefix + ".windows.bedgraph")]
        if self.has_targets:
            out.append(self.write_targets(prefix + ".targets.tsv"))
        return out


def read_bed(path: str) -> Dict[str, List[Tuple[int, int]]]:
    """chromosome -> sorted (start, stop) of a BED file's first three columns; intervals that overlap are merged, touching ones stay
    apart.  ``#``, ``track`` and ``browser`` lines are skipped; an empty or negative interval is refused."""
    found: Dict[str, List[Tuple[int, int]]] = {}
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            f = line.split()
            if not f or f[0].startswith("#") or f[0] in ("track", "browser"):
                continue
            if len(f) < 3 or not (f[1].isdigit() and f[2].isdigit()) or int(f[1]) >= int(f[2]):
                raise ValueError(f"{path}:{n}: not a BED interval with 0 <= start < end")
            found.setdefault(f[0], []).append((int(f[1]), int(f[2])))
    out = {}
    for c, intervals in found.items():
        merged: List[Tuple[int, int]] = []
        for a, b in sorted(intervals):
            if merged and a < merged[-1][1]:
                merged[-1] = (merged[-1][0], max(merged[-1][1], b))
            else:
                merged.append((a, b))
        out[c] = merged
    return out


def measure(bam: str, fasta, chromosomes: Optional[Sequence[str]] = None, targets: Optional[Dict[str, Targets]] = None,
            window: int = DEFAULT_WINDOW, mapq_threshold: int = 10, max_span: Optional[int] = None, device: int = 0,
            restatement: bool = False, stats: Optional[dict] = None) -> Metrics:
    """The metrics of one BAM, chromosome after chromosome (default: every sequence of the FASTA).  ``fasta``: a path, or
    {chromosome: sequence}; ``targets``: {chromosome: intervals} as ``read_bed`` gives them; ``restatement``: from the plain-Python
    rules instead of the GPU.  ``stats``: the library's kernel times and the seconds of decoding (``decode_s``), of the library's
    calls (``device_s``) and of the whole pass (``total_s``) are added."""
    if window < 1:
        raise ValueError("window: at least 1")
    metrics = Metrics(window, targets is not None)
    mine = lambda c: check_targets((targets or {}).get(c, ()))      # noqa: E731
    measure_spans(bam, fasta, chromosomes, max_span, stats, restatement,       # a chromosome without positions has no add: restated
                  open_handle=lambda c, ref: Meter(ref, mine(c), window, mapq_threshold, device) if ref.shape[0] else None,
                  restated=lambda c, ref, spans: restated(spans, ref, mine(c), window, mapq_threshold),
                  done=lambda c, ref, tables, counts: metrics.set(c, ref.shape[0], tables, counts, mine(c)))
    return metrics


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Alignment, coverage and insert-size metrics of a coordinate-sorted BAM, counted on the GPU")
    p.add_argument("--bam", required=True, help="The BAM (with its .bai, or scanned)")
    p.add_argument("--ref", required=True, help="Reference FASTA")
    p.add_argument("--output_prefix", required=True, help="Writes <prefix>.metrics.txt, .tables.npz, .windows.bedgraph and, with "
                                                          "--regions, .targets.tsv")
    p.add_argument("--regions", help="BED file of target intervals: depth on target and per target")
    p.add_argument("--window", type=int, default=DEFAULT_WINDOW, help="Width of the depth windows (at least 1)")
    p.add_argument("--chromosomes", help="Comma-separated chromosomes (default: every sequence of the FASTA)")
    p.add_argument("--mapq_threshold", type=int, default=10, help="A read below it leaves the depth (it is still measured)")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def main(argv=None) -> List[str]:
    args = parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)-15s %(message)s")
    if args.window < 1:
        raise SystemExit("--window is the width of a depth window: give 1 or more")
    stats: dict = {}
    metrics = measure(args.bam, args.ref, args.chromosomes.split(",") if args.chromosomes else None,
                      read_bed(args.regions) if args.regions else None, args.window, args.mapq_threshold, device=args.device, stats=stats)
    total = metrics.total()
    _log.info("%d reads, %d measured, %d pairs (kernels %.1f ms)", int(total["FLAGS"][0]), int(total["STATS"][0]),
              int(total["STATS"][4]), sum(stats.get(k, 0.0) for k in STAT_NAMES[len(COUNT_NAMES):]))
    return metrics.write_all(args.output_prefix)


if __name__ == "__main__":
    main(sys.argv[1:])
