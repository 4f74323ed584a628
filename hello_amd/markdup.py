"""PCR duplicates: which reads of a sorted BAM are copies of one fragment, found on the GPU before anything counts them.

    python -m hello_amd.call --from_bam | --from_bams [--resident] ... --mark_duplicates
    python -m hello_amd.markdup --bam illumina.bam --output marks.npz [--chromosomes a,b] [--metrics F] [--device N]

Not in the reference; DESIGN.md section 7j defines the rules.  ``eligible``, ``end5_of``, ``score_of``, ``kinds_of`` and
``duplicates_of`` restate them in plain Python / NumPy without a GPU, built on ``phase.join_mates``; ``Deduper`` binds
``hello_markdup_*`` (hello_amd/csrc/markdup.hip), which equal the restatement integer for integer.  ``find_duplicates`` is the pass
over one BAM: per chromosome one batch of reads per span of at most ``hotspots.MAX_LAUNCH_BASES`` positions (a read belongs to the
span that holds its start), the join and the keys chromosome-wide.  Its result, ``Marks``, names every duplicate by
``(name_hash, flag & 0xC0, ref_start)`` within its chromosome; inside ``applied({bam: marks})`` every ``BamFile.fetch`` of that BAM
returns its reads with flag 0x400 set on the marked ones, and every stage's read filter drops them.
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import logging
import os
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import bam as _bam
from ._abi import ARRAY_GETTER, READS, STATS_GETTER, bind, check, i32, i64, vp
from .bam import BamFile, Reads
from .phase import _from, join_mates
from .spans import Handle, adder, span_step

NOT_ELIGIBLE = 0x4 | 0x100 | 0x800 | 0x400          # unmapped, secondary, supplementary, a duplicate already
DUPLICATE = 0x400
MIN_QUALITY = 15
MAX_SCORE = 2 ** 30 - 1
NOT_ELIGIBLE_KIND, PAIR, SINGLE, UNRESOLVED = range(4)
E, SCORE, MATE, KIND, DUP = range(5)                # HELLO_MARKDUP_*
COUNT_NAMES = ("reads", "eligible", "pairs", "singles", "unresolved", "groups_refused", "duplicate_pairs", "duplicate_singles")
STAT_NAMES = COUNT_NAMES + ("ends_ms", "pair_ms", "key_ms", "mark_ms")
METRIC_NAMES = COUNT_NAMES + ("duplicate_reads",)

_log = logging.getLogger(__name__)


# ------------------------------------------------------------------------------------------------
# the rules, restated
# ------------------------------------------------------------------------------------------------
def eligible(flags) -> np.ndarray:
    """bool [reads]: mapped, primary, not supplementary, not a duplicate already; mapq and QC-fail do not matter."""
    return (np.asarray(flags).astype(np.int64) & NOT_ELIGIBLE) == 0


def end5_of(rd: Reads, r: int) -> int:
    """The reference position of the read's 5' base as the fragment had it, soft and hard clips counted back in: a forward read's
    ``ref_start`` minus its leading run of S / H, a reverse read's ``ref_end - 1`` plus its trailing run.  May be negative."""
    ops = [(int(c) & 15, int(c) >> 4) for c in rd.cigars[int(rd.cigar_offsets[r]):int(rd.cigar_offsets[r + 1])]]
    if int(rd.flags[r]) & 0x10:
        ops.reverse()
    clip = 0
    for op, n in ops:
        if op not in (4, 5):
            break
        clip += n
    return int(rd.ref_ends[r]) - 1 + clip if int(rd.flags[r]) & 0x10 else int(rd.ref_starts[r]) - clip


def packed_end(rd: Reads, r: int) -> int:
    """e = 2 end5 + strand."""
    return 2 * end5_of(rd, r) + (1 if int(rd.flags[r]) & 0x10 else 0)


def score_of(rd: Reads, r: int) -> int:
    """The sum of the read's base qualities that are at least 15, saturated at 2^30 - 1."""
    q = rd.quals[int(rd.read_offsets[r]):int(rd.read_offsets[r + 1])].astype(np.int64)
    return min(int(q[q >= MIN_QUALITY].sum()), MAX_SCORE)


def kinds_of(flags, mate, is_eligible) -> np.ndarray:
    """uint8 [reads]: 0 not eligible, 1 pair (joined by ``phase.join_mates``, whatever its 0x8 says), 2 single (flag 0x1 unset, or
    0x1 and 0x8: the mate is unmapped), 3 unresolved (every other eligible read)."""
    kind = np.zeros(len(flags), np.uint8)
    for r in range(len(flags)):
        if is_eligible[r]:
            f = int(flags[r])
            kind[r] = PAIR if mate[r] >= 0 else SINGLE if not f & 0x1 or f & 0x8 else UNRESOLVED
    return kind


def duplicates_of(rd: Reads) -> Tuple[np.ndarray, dict]:
    """(duplicate uint8 [reads], details) over the reads of ONE chromosome of ONE BAM.  ``details``: e int64, score int32, mate
    int64, kind uint8, all aligned with the reads (0, 0, -1, 0 for a read that is not eligible), and the eight counts."""
    n = rd.n_reads
    ok = eligible(rd.flags)
    e, score = np.zeros(n, np.int64), np.zeros(n, np.int32)
    for r in np.flatnonzero(ok):
        e[r], score[r] = packed_end(rd, r), score_of(rd, r)
    mate, counts = join_mates(rd.name_hash, rd.flags, np.zeros(n, np.uint8), ok)
    kind = kinds_of(rd.flags, mate, ok)
    duplicate = np.zeros(n, np.uint8)
    pairs: Dict[Tuple[int, int], List[int]] = {}            # (lo, hi) -> the smaller read index of every pair
    singles: Dict[int, List[int]] = {}
    pair_ends = set()
    for r in range(n):
        if kind[r] == PAIR:
            pair_ends.add(int(e[r]))
            if r < mate[r]:
                a, b = int(e[r]), int(e[mate[r]])
                pairs.setdefault((min(a, b), max(a, b)), []).append(r)
        elif kind[r] == SINGLE:
            singles.setdefault(int(e[r]), []).append(r)
    duplicate_pairs = duplicate_singles = 0
    for members in pairs.values():                          # the largest summed score survives, ties to the smallest index
        best = min(members, key=lambda r: (-(int(score[r]) + int(score[mate[r]])), r))
        for r in members:
            if r != best:
                duplicate[r] = duplicate[mate[r]] = 1
                duplicate_pairs += 1
    for end, members in singles.items():
        best = None if end in pair_ends else min(members, key=lambda r: (-int(score[r]), r))
        for r in members:
            if r != best:
                duplicate[r] = 1
                duplicate_singles += 1
    counts = dict(reads=n, eligible=int(ok.sum()), pairs=counts["pairs"], singles=int((kind == SINGLE).sum()),
                  unresolved=int((kind == UNRESOLVED).sum()), groups_refused=counts["groups_refused"],
                  duplicate_pairs=duplicate_pairs, duplicate_singles=duplicate_singles)
    return duplicate, dict(e=e, score=score, mate=mate, kind=kind, duplicate=duplicate, counts=counts)


def key_table_size(n_inserts: int) -> int:
    """Slots of the key kernel's open-addressing table: the power of two that is at least twice the inserts (and 2); the inserts
    are three per pair (an END entry per mate, a PAIR entry) and one per single."""
    size = 2
    while size < 2 * n_inserts:
        size <<= 1
    return size


def key_table_slot(a, b, pair, size: int) -> np.ndarray:
    """uint32: the first slot the key kernel probes in a table of ``size`` slots (markdup.hip: key_slot) for END(e) -- ``a`` = e,
    ``b`` = 0, ``pair`` = 0 -- or PAIR(lo, hi) -- ``a`` = lo, ``b`` = hi, ``pair`` = 1."""
    u = np.uint64
    x = np.atleast_1d(np.asarray(a, np.int64)).astype(u)
    y = np.atleast_1d(np.asarray(b, np.int64)).astype(u) + np.atleast_1d(np.asarray(pair)).astype(u)
    x = x ^ (x >> u(29))
    x = x * u(0xBF58476D1CE4E5B9)
    x = x ^ (x >> u(32))
    x = x + y
    x = x ^ (x >> u(29))
    x = x * u(0x94D049BB133111EB)
    x = x ^ (x >> u(32))
    return ((x & u(0xFFFFFFFF)) & u(size - 1)).astype(np.uint32)


# ------------------------------------------------------------------------------------------------
# the GPU
# ------------------------------------------------------------------------------------------------
_PROTOTYPES = (
    ("hello_markdup_add", READS + [i64, i32, C.POINTER(vp)]),
    ("hello_markdup_find", [vp]),
    ("hello_markdup_array", ARRAY_GETTER),
    ("hello_markdup_stats", STATS_GETTER),
    ("hello_markdup_free", [vp], None),
)


def _lib():
    return bind(_PROTOTYPES)


class Deduper(Handle):
    """One (BAM, chromosome)'s ``hello_markdup`` handle: ``add`` takes the reads of a span, ``find`` (once, after the last ``add``)
    joins the mates and marks, ``arrays`` gives e, score, mate, kind and duplicate of every read given, in the order given."""
    NAME, STAT_NAMES = "markdup", STAT_NAMES
    ARRAYS = (("e", E, np.int64, None), ("score", SCORE, np.int32, None), ("mate", MATE, np.int64, None),
              ("kind", KIND, np.uint8, None), ("duplicate", DUP, np.uint8, None))

    def __init__(self, device: int = 0):
        super().__init__(_lib())
        self._device = int(device)
        self._found = False

    def add(self, reads: Reads) -> None:
        check(self._lib.hello_markdup_add(*reads.pointers(reads.hp)[:10], None, int(reads.n_reads), self._device, C.byref(self._h)))

    def find(self) -> None:
        check(self._lib.hello_markdup_find(self._h))
        self._found = True

    def _has(self, name: str) -> bool:
        return name in ("e", "score") or self._found


def find_arrays(reads: Reads, device: int = 0) -> Tuple[Dict[str, np.ndarray], Dict[str, float]]:
    """One ``add`` and ``find`` over an already decoded read set -> (the five arrays, statistics)."""
    with Deduper(device) as d:
        d.add(reads)
        d.find()
        return d.arrays(), d.stats()


# ------------------------------------------------------------------------------------------------
# the marks of one BAM
# ------------------------------------------------------------------------------------------------
class Marks:
    """The duplicates of one BAM: per chromosome ``identities[c]`` = (name_hash uint64, flag & 0xC0 as uint16, ref_start int64),
    sorted by the three in that order, and ``metrics[c]`` = {METRIC_NAMES: int}."""

    def __init__(self):
        self.identities: Dict[str, Tuple[np.ndarray, np.ndarray, np.ndarray]] = {}
        self.metrics: Dict[str, Dict[str, int]] = {}
        self._sets: Dict[str, set] = {}

    def set(self, chromosome: str, name_hash, flags, ref_starts, metrics: Dict[str, int]) -> None:
        """The identities of the duplicates of ``chromosome`` (one entry per marked read) and its metrics."""
        name = np.asarray(name_hash, np.uint64)
        mates = (np.asarray(flags).astype(np.uint16) & np.uint16(0xC0)).astype(np.uint16)
        start = np.asarray(ref_starts, np.int64)
        order = np.lexsort((start, mates, name))
        self.identities[chromosome] = (name[order], mates[order], start[order])
        self.metrics[chromosome] = {k: int(metrics[k]) for k in METRIC_NAMES}
        self._sets.pop(chromosome, None)

    def total(self) -> Dict[str, int]:
        return {k: sum(m[k] for m in self.metrics.values()) for k in METRIC_NAMES}

    def apply(self, chromosome: str, reads: Reads) -> int:
        """ORs 0x400 into ``reads.flags`` where (name_hash, flag & 0xC0, ref_start) is a mark of ``chromosome`` -> reads marked."""
        if chromosome not in self.identities or reads.n_reads == 0:
            return 0
        name, mates, start = self.identities[chromosome]
        if name.shape[0] == 0:
            return 0
        if chromosome not in self._sets:
            self._sets[chromosome] = set(zip(name.tolist(), mates.tolist(), start.tolist()))
        marked = self._sets[chromosome]
        at = np.searchsorted(name, reads.name_hash)                       # the names that are marked at all, then the exact triple
        maybe = np.flatnonzero(name[np.minimum(at, name.shape[0] - 1)] == reads.name_hash)
        hit = [r for r in maybe.tolist()
               if (int(reads.name_hash[r]), int(reads.flags[r]) & 0xC0, int(reads.ref_starts[r])) in marked]
        reads.flags[np.array(hit, np.int64)] |= np.uint16(DUPLICATE)
        return len(hit)

    def save(self, path: str) -> str:
        names = list(self.identities)
        out = dict(chromosomes=np.array(names, dtype=np.str_), metric_names=np.array(METRIC_NAMES, dtype=np.str_),
                   metrics=np.array([[self.metrics[c][k] for k in METRIC_NAMES] for c in names], np.int64).reshape(len(names), len(METRIC_NAMES)))
        for i, c in enumerate(names):
            out["name_hash_%d" % i], out["mates_%d" % i], out["ref_start_%d" % i] = self.identities[c]
        with open(path, "wb") as fh:
            np.savez(fh, **out)
        return path

    @classmethod
    def load(cls, path: str) -> "Marks":
        marks = cls()
        with np.load(path, allow_pickle=False) as z:
            keys = [str(k) for k in z["metric_names"]]
            for i, c in enumerate(str(c) for c in z["chromosomes"]):
                marks.identities[c] = (z["name_hash_%d" % i], z["mates_%d" % i], z["ref_start_%d" % i])
                marks.metrics[c] = dict(zip(keys, (int(v) for v in z["metrics"][i])))
        return marks

    def write_metrics(self, path: str) -> str:
        """One ``name<TAB>value`` line per statistic, per chromosome (``<chromosome>.<name>``) and in total (``total.<name>``)."""
        with open(path, "w") as fh:
            for c, metrics in list(self.metrics.items()) + [("total", self.total())]:
                for k in METRIC_NAMES:
                    fh.write("%s.%s\t%d\n" % (c, k, metrics[k]))
        return path


@contextlib.contextmanager
def applied(marks_by_bam: Dict[str, Marks]):
    """Inside: every ``BamFile.fetch`` of a BAM of ``marks_by_bam`` (by ``os.path.abspath``) returns its reads with the marks
    applied.  The registry is the process's; it is left as it was found."""
    mine = {os.path.abspath(p): m for p, m in marks_by_bam.items()}
    before = {p: _bam.MARKS.get(p) for p in mine}
    _bam.MARKS.update(mine)
    try:
        yield
    finally:
        for p, m in before.items():
            if m is None:
                _bam.MARKS.pop(p, None)
            else:
                _bam.MARKS[p] = m


def find_duplicates(bam: str, chromosomes: Optional[Sequence[str]] = None, max_span: Optional[int] = None, device: int = 0,
                    restatement: bool = False, stats: Optional[dict] = None) -> Marks:
    """The duplicates of one BAM, chromosome after chromosome (default: every sequence of its header).  ``restatement``: from the
    plain-Python rules instead of the GPU.  ``stats``: the library's statistics and the seconds of decoding (``decode_s``), of the
    kernels' calls (``device_s``), of the host's gather of the identities (``gather_s``) and of the whole pass (``total_s``) are added."""
    step, add = span_step(max_span), adder(stats)
    marks = Marks()
    t_all = time.perf_counter()
    with BamFile(bam) as handle:
        lengths = dict(handle.references)
        for c in (chromosomes or [name for name, _ in handle.references]):
            if c not in lengths:
                raise ValueError(f"no sequence named {c!r} in the BAM header")
            names, flags, starts, spans = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint16)], [np.zeros(0, np.int64)], []
            dd = None if restatement else Deduper(device)
            try:
                for lo in range(0, lengths[c], step):
                    t0 = time.perf_counter()
                    rd = _from(handle.fetch(c, lo, min(lo + step, lengths[c])), lo)
                    t1 = time.perf_counter()
                    names.append(rd.name_hash)
                    flags.append(rd.flags)
                    starts.append(rd.ref_starts)
                    if restatement:
                        spans.append(rd)
                    else:
                        dd.add(rd)
                    add("decode_s", t1 - t0)
                    add("device_s", time.perf_counter() - t1)
                t0 = time.perf_counter()
                if restatement:
                    got = duplicates_of(Reads.concat(spans)[0]) if spans else (np.zeros(0, np.uint8), dict(counts=dict.fromkeys(COUNT_NAMES, 0)))
                    duplicate, counts = got[0], got[1]["counts"]
                else:
                    dd.find()
                    duplicate, counts = dd.arrays()["duplicate"], dd.stats()
                    for k in STAT_NAMES[len(COUNT_NAMES):]:
                        add(k, counts[k])
                add("device_s", time.perf_counter() - t0)
            finally:
                if dd is not None:
                    dd.close()
            t0 = time.perf_counter()
            which = np.flatnonzero(duplicate)
            metrics = dict({k: int(counts[k]) for k in COUNT_NAMES}, duplicate_reads=int(which.shape[0]))
            marks.set(c, np.concatenate(names)[which], np.concatenate(flags)[which], np.concatenate(starts)[which], metrics)
            add("gather_s", time.perf_counter() - t0)
    add("total_s", time.perf_counter() - t_all)
    return marks


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Find the PCR duplicates of a coordinate-sorted BAM on the GPU and save their marks")
    p.add_argument("--bam", required=True, help="The BAM (with its .bai, or scanned)")
    p.add_argument("--output", required=True, help="Path of the marks (.npz; hello_amd.markdup.Marks.load reads it)")
    p.add_argument("--chromosomes", help="Comma-separated chromosomes (default: every sequence of the BAM header)")
    p.add_argument("--metrics", help="Also write the counts as name<TAB>value lines, per chromosome and in total")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def main(argv=None) -> str:
    args = parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)-15s %(message)s")
    stats: dict = {}
    marks = find_duplicates(args.bam, args.chromosomes.split(",") if args.chromosomes else None, device=args.device, stats=stats)
    total = marks.total()
    _log.info("%d reads, %d pairs, %d duplicate reads (kernels %.1f ms)", total["reads"], total["pairs"], total["duplicate_reads"],
              sum(stats.get(k, 0.0) for k in ("ends_ms", "pair_ms", "key_ms", "mark_ms")))
    if args.metrics:
        marks.write_metrics(args.metrics)
    return marks.save(args.output)


if __name__ == "__main__":
    main(sys.argv[1:])
