"""A seeded corpus over the whole CIGAR and flag grammar for the BAM-side stages (DESIGN.md sections 7f - 7k, 7l), the census of
what it really contains, and an oracle that is no third copy of the kernels.

``corpus(seed, profile)`` -> (reference, rows, records): rows in the format of tests/qc_cases.py, records heterozygous
``phase.Record``s, reads sampled from two haplotypes built from the records and then spoiled.  ``census`` counts the situations
tests/test_read_fuzz.py asserts.  ``alignment_table`` expands the rows into one line per base of every operation and does nothing
else; ``Oracle`` derives every quantity from that table with NumPy group-bys -- no cursor walks a CIGAR there -- and ``Rules``
switches each rule off, so that a test can show the corpus reaches it.
"""
from __future__ import annotations

import functools
from collections import Counter
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

from hello_amd import gvcf, haplotag, markdup, phase, qc
from tests import qc_cases
from tests.gvcf_cases import D, EQ, H, I, M, N, P, S, X

LENGTH = 2600
TILE = 1024                                  # kRbTile of refblocks.hip, the tile of qc.hip
SPAN = 700                                   # the cut spans: no divisor of the tile
TILE_EDGES = (TILE, 2 * TILE)
CUTS = (SPAN, 2 * SPAN, 3 * SPAN)
SEEDS = range(32)
PROFILES = ("short", "long")
RUN_LENGTHS = (1, 2, 7, 63, 64, 65, 130, 150)
QUALITIES = (0, 2, 9, 10, 14, 15, 30, 41, 93)
MAPQS = (0, 5, 10, 60, 255)
FILTERS = (0x4, 0x100, 0x200, 0x400, 0x800)
NOISE = "ACGTNacgt"
REV = 0x10
ALIGNED = (M, EQ, X)
Q_THRESHOLD = MAPQ_THRESHOLD = 10
WINDOW = 50


# ------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------
def _pick(rng, values, p=None):
    return values[int(rng.choice(len(values), p=p))]


def _other(rng, base: str, but: str = "") -> str:
    return _pick(rng, [b for b in "ACGT" if b != base and b not in but])


def _reference(rng) -> str:
    """2 600 bases: two runs of N (one over the first cut, one over the second tile edge) and a lower-case stretch."""
    s = "".join(rng.choice(list("ACGT"), size=LENGTH))
    s = s[:690] + "N" * 25 + s[715:]
    s = s[:2040] + "N" * 12 + s[2052:]
    return s[:1500] + s[1500:1580].lower() + s[1580:]


def _records(rng, reference: str) -> Tuple[List[phase.Record], List[Tuple[str, str]]]:
    """Heterozygous records every 7 - 40 bases and, per record, the allele strings of haplotype 0 and 1."""
    records, alleles = [], []
    p = int(rng.integers(3, 12))
    while p < LENGTH - 8:
        kind = _pick(rng, ("snv", "mnp", "ins", "del", "two"), [0.34, 0.14, 0.2, 0.2, 0.12])
        n_ref = dict(snv=1, mnp=2, ins=1, two=1)[kind] if kind != "del" else int(rng.integers(2, 6))
        ref = reference[p:p + n_ref].upper()
        if set(ref) <= set("ACGT"):
            tail = "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 4))))
            a, b, al_a = 0, 1, ref
            if kind == "snv":
                al_b = _other(rng, ref)
            elif kind == "mnp":
                al_b = _other(rng, ref[0]) + _other(rng, ref[1])
            elif kind == "ins":
                al_b = ref + tail
            elif kind == "del":
                al_b = ref[0]
            else:                                                        # 1/2: both alleles are ALT
                a, b = 1, 2
                if rng.random() < 0.5:
                    al_a = _other(rng, ref)
                    al_b = _other(rng, ref, al_a)
                else:
                    al_a, al_b = ref + tail, ref + tail + _other(rng, tail[-1])
            records.append(phase.Record(p, p + n_ref, a, b, al_a.encode(), al_b.encode()))
            alleles.append((al_a, al_b) if rng.random() < 0.5 else (al_b, al_a))
        p += int(min(rng.integers(7, 41), rng.integers(7, 41)))
    return records, alleles


def _between(rng) -> List[Tuple[int, int]]:
    kind = int(rng.choice(7, p=[0.24, 0.1, 0.1, 0.2, 0.12, 0.12, 0.12]))
    i, d, n = lambda: _pick(rng, (1, 3, 70)), lambda: _pick(rng, (1, 5, 90)), lambda: _pick(rng, (3, 300))   # noqa: E731
    pad = lambda: (P, int(rng.integers(1, 4)))                                                            # noqa: E731
    return ([(I, i())], [(I, i()), pad(), (I, i())], [pad(), (I, i())], [(D, d())], [(N, n())], [(D, d()), (I, i())], [])[kind]


def _cigar(rng, profile: str) -> List[Tuple[int, int]]:
    """One CIGAR of the grammar; its query length is 1 - 160 (short) or 600 - 1 500 with at most 30 operations (long).  A quarter
    of the long ones have 512 - 575 bases between two soft clips of a wave or more, so that a soft clip holds cycle 511."""
    lo, hi = (1, 160) if profile == "short" else (600, 1500)
    clipped = profile == "long" and rng.random() < 0.25
    if clipped:
        lo, hi = 512, 575
    while True:
        if profile == "short":
            runs = int(rng.choice(6, p=[0.3, 0.3, 0.2, 0.1, 0.05, 0.05])) + 1
            lengths, weights = RUN_LENGTHS, None
        else:
            runs = int(rng.integers(2, 5)) if clipped else int(rng.integers(5, 13))
            lengths, weights = RUN_LENGTHS, [0.04, 0.04, 0.04, 0.1, 0.1, 0.1, 0.29, 0.29]
        clip = lambda: _pick(rng, (64, 65, 66, 80) if clipped else (1, 3, 20, 64, 65, 66, 80))           # noqa: E731
        ops: List[Tuple[int, int]] = []
        if rng.random() < 0.15:
            ops.append((H, int(rng.integers(1, 30))))
        if clipped or rng.random() < 0.3:
            ops.append((S, clip()))
        lead = rng.random()
        if lead < 0.08:
            ops.append((I, _pick(rng, (1, 3, 70))))
        elif lead < 0.13:
            ops.append((D, _pick(rng, (1, 5, 90))))
        for k in range(runs):
            if k:
                ops += _between(rng)
            ops.append((_pick(rng, (M, M, M, M, EQ, X)), _pick(rng, lengths, weights)))
        tail = rng.random()
        if tail < 0.08:
            ops.append((I, _pick(rng, (1, 3, 70))))
        elif tail < 0.13:
            ops.append((D, _pick(rng, (1, 5, 90))))
        if clipped or rng.random() < 0.3:
            ops.append((S, clip()))
        if rng.random() < 0.15:
            ops.append((H, int(rng.integers(1, 30))))
        merged: List[Tuple[int, int]] = []
        for op, n in ops:                                                # two equal neighbours are one operation
            if merged and merged[-1][0] == op:
                merged[-1] = (op, merged[-1][1] + n)
            else:
                merged.append((op, n))
        qlen = sum(n for op, n in merged if op in (M, I, S, EQ, X))
        if lo <= qlen <= hi and len(merged) <= 30:
            return merged


def _ref_len(cigar) -> int:
    return sum(n for op, n in cigar if op in (M, D, N, EQ, X))


def _place(rng, cigar, profile: str) -> Tuple[int, bool]:
    """-> (position, whether an operation boundary was put on an edge: such a read gets no planted indel that would move it)."""
    span = _ref_len(cigar)
    mode = rng.random()
    edge = _pick(rng, (1000,) + TILE_EDGES + (2000,) + CUTS)
    if mode < 0.2:                                                       # an operation begins exactly at a tile edge or a cut
        offsets, p = [], 0
        for k, (op, n) in enumerate(cigar):
            if k and op in (I, D, N) and p > 0:
                offsets.append(p)
            p += n if op in (M, D, N, EQ, X) else 0
        if offsets and edge - (off := _pick(rng, offsets)) >= 0:
            return edge - off, True
    if mode < 0.3 and span > 1:                                          # straddles an edge
        return max(0, edge - int(rng.integers(1, span))), False
    if mode < 0.36:
        return 0, False
    if mode < 0.46:                                                      # runs past the reference's end
        return max(0, LENGTH - int(rng.integers(1, max(2, span)))), False
    return int(rng.integers(0, max(1, LENGTH - (span if profile == "long" else 0)))), False


def _realize(rng, reference: str, planted: Dict[int, Tuple[phase.Record, str]], cigar, pos: int, plant: bool):
    """The CIGAR with the haplotype's insertions and deletions planted into its aligned runs, and the read's bases."""
    out: List[Tuple[int, int]] = []
    bases: List[str] = []
    budget = 40 - len(cigar)
    p = pos

    def base_at(q: int) -> str:
        b = reference[q].upper() if q < LENGTH else "N"
        return b if b in "ACGT" else "ACGT"[int(rng.integers(4))]
    for op, n in cigar:
        if op in ALIGNED:
            j = seg = 0
            while j < n:
                hit = planted.get(p + j)
                if hit is not None:
                    rec, allele = hit
                    width = rec.end - rec.start
                    if len(allele) == width:                             # a substitution, or the reference allele
                        k = min(width, n - j)
                        bases.append(allele[:k])
                        j, seg = j + k, seg + k
                        continue
                    if plant and budget >= 2 and j + 1 < n:
                        bases.append(allele[0])
                        out.append((op, seg + 1))
                        budget -= 2
                        if width == 1:
                            out.append((I, len(allele) - 1))
                            bases.append(allele[1:])
                        else:
                            out.append((D, width - 1))
                            p += width - 1
                        j, seg = j + 1, 0
                        continue
                bases.append(base_at(p + j))
                j, seg = j + 1, seg + 1
            if seg:
                out.append((op, seg))
            p += n
        else:
            if op in (I, S):
                bases.append("".join(rng.choice(list("ACGT"), size=n)))
            elif op in (D, N):
                p += n
            out.append((op, n))
    text = list("".join(bases))
    for k in np.flatnonzero(rng.random(len(text)) < 0.08):
        text[k] = NOISE[int(rng.integers(len(NOISE)))]
    return out, "".join(text)


def _quals(rng, n: int) -> List[int]:
    if rng.random() < 0.04:
        return [0xFF] * n                                                # QUAL absent
    main = _pick(rng, (10, 14, 15, 30, 41, 93), [0.05, 0.05, 0.1, 0.4, 0.3, 0.1])
    q = np.where(rng.random(n) < 0.12, rng.choice(QUALITIES, size=n), main)
    return [int(v) for v in q]


def _mapq(rng) -> int:
    return _pick(rng, MAPQS, [0.04, 0.04, 0.1, 0.72, 0.1])


@functools.lru_cache(maxsize=None)
def corpus(seed: int, profile: str = "short", acgt_only: bool = False, reference_of: str = None):
    """-> (reference, rows sorted by position, records).  ``acgt_only``: the variant whose read bases are all upper-case ACGT.
    ``reference_of``: the profile whose generator draws the reference and the records; the reads stay the profile's own, so the
    long and the short reads of one seed can share a chromosome (tests/candidate_fuzz.py, the two-BAM route)."""
    rng = np.random.default_rng([seed, PROFILES.index(profile), 20261020])
    source = rng if reference_of is None else np.random.default_rng([seed, PROFILES.index(reference_of), 20261020])
    reference = _reference(source)
    records, alleles = _records(source, reference)
    planted = [{rec.start: (rec, al[h]) for rec, al in zip(records, alleles)} for h in range(2)]
    units: List[List[tuple]] = []
    name = [0]

    def read(flag: int, near: int = -1, hap: int = 0) -> tuple:
        cigar = _cigar(rng, profile)
        pos, fixed = _place(rng, cigar, profile)
        if near >= 0:
            pos = min(LENGTH - 1, near + int(rng.integers(0, 300)))
        cigar, bases = _realize(rng, reference, planted[hap], cigar, pos, not fixed)
        if acgt_only:
            bases = "".join(b if b in "ACGT" else "ACGT"[k % 4] for k, b in enumerate(bases.upper()))
        return (name[0], flag, pos, cigar, bases, _quals(rng, len(bases)), _mapq(rng))

    def unit(kind: str) -> List[tuple]:
        name[0] += 1
        hap = int(rng.integers(2))
        s = [REV * int(rng.integers(2)) for _ in range(3)]
        if kind == "single":
            return [read(s[0], hap=hap)]
        if kind == "pair":
            f1, f2 = _pick(rng, ((0x63, 0x93), (0x53, 0xA3), (0xA3, 0x53), (0x93, 0x63)))
            first = read(f1, hap=hap)
            return [first, read(f2, first[2], hap)]
        if kind == "improper":
            first = read(0x41 | s[0], hap=hap)
            return [first, read(0x81 | s[1], first[2], hap)]
        if kind == "mate_unmapped":
            return [read(0x49 | s[0], hap=hap)]
        if kind == "three":
            first = read(0x63, hap=hap)
            return [first, read(0x93, first[2], hap), read(0x93 if rng.random() < 0.5 else 0, first[2], hap)]
        first = read(0x63, hap=hap)                                       # two first mates
        return [first, read(0x63 | s[1], first[2], hap)]

    def copy_of(old: List[tuple]) -> List[tuple]:
        """A PCR copy: the same alignments under a new name, with the same qualities (a tie) or new ones; or one mate as a single."""
        name[0] += 1
        if len(old) > 1 and rng.random() < 0.3:
            r = old[int(rng.integers(len(old)))]
            return [(name[0], r[1] & REV, r[2], r[3], r[4], _quals(rng, len(r[4])), r[6])]
        fresh = rng.random() < 0.5
        return [(name[0], r[1], r[2], r[3], r[4], _quals(rng, len(r[4])) if fresh else r[5], r[6]) for r in old]
    if profile == "short":
        kinds, weights, n_reads = ("single", "pair", "improper", "mate_unmapped", "three", "two_first"), [0.4, 0.36, 0.08, 0.06, 0.05, 0.05], 140
    else:
        kinds, weights, n_reads = ("single", "pair"), [0.5, 0.5], 12
    while sum(len(u) for u in units) < n_reads:
        if units and profile == "short" and rng.random() < 0.15:
            units.append(copy_of(units[int(rng.integers(len(units)))]))
        else:
            units.append(unit(_pick(rng, kinds, weights)))
    rows = [r for u in units for r in u]
    for bit in FILTERS:                                                  # each filter flag on a few reads
        for k in rng.choice(len(rows), size=3 if profile == "short" else 1, replace=False):
            rows[k] = rows[k][:1] + (rows[k][1] | bit,) + rows[k][2:]
    name[0] += 1
    rows.append((name[0], 0, int(rng.integers(0, LENGTH)), [], "", [], 60))          # mapped, no CIGAR, no bases
    rows.sort(key=lambda row: row[2])
    return reference, rows, records


def saturating():
    """-> (reference, rows) with one read whose qualities of 15 and more sum above 2^30 - 1: what no read of the grammar reaches,
    4 210 753 bases of quality 255 at the least.  Beside it two short reads at the same 5' end."""
    reference = _reference(np.random.default_rng(7))
    n = (markdup.MAX_SCORE + 1) // 255 + 3
    return reference, [(1, 0, 100, [(M, 10), (S, n - 10)], "A" * n, [0xFF] * n, 60), (2, 0, 100, [(M, 10)], "A" * 10, [30] * 10, 60),
                       (3, 0, 100, [(M, 10)], "A" * 10, [41] * 10, 60)]


def bam_rows(rows):
    """The rows as a BAM can hold them: its 4-bit base codes have no case, and ``hello_bam_fetch`` refuses a read without stored
    qualities (QUAL 0xFF), so a read that has none gets quality 30."""
    return [r[:4] + (r[4].upper(), [30] * len(r[5]) if r[5] and r[5][0] == 0xFF else r[5], r[6]) for r in rows]


def bam_reads(rows):
    """tests.bam_writer records of ``bam_rows(rows)``, named by their name hash."""
    from tests.bam_writer import Read
    return [Read("n%d" % r[0], r[2], r[3], r[4], r[5], r[1], r[6]) for r in bam_rows(rows)]


def fnv1a(name: str) -> int:
    h = 1469598103934665603
    for c in name.encode():
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


# ------------------------------------------------------------------------------------------------
# the alignment table
# ------------------------------------------------------------------------------------------------
@dataclass
class Table:
    """One line per base of every operation: read, operation index, query index or -1, reference position or -1, operation."""
    read: np.ndarray
    opi: np.ndarray
    q: np.ndarray
    p: np.ndarray
    op: np.ndarray


_IS_QUERY = np.isin(np.arange(16), (M, I, S, EQ, X))
_IS_REF = np.isin(np.arange(16), (M, D, N, EQ, X))


def alignment_table(rows) -> Table:
    read = np.array([r for r, row in enumerate(rows) for _ in row[3]], np.int64)
    opi = np.array([k for row in rows for k in range(len(row[3]))], np.int64)
    op = np.array([o for row in rows for o, _ in row[3]], np.int64)
    n = np.array([k for row in rows for _, k in row[3]], np.int64)
    pos = np.array([row[2] for row in rows], np.int64)
    first = opi == 0

    def starts(consumed):                                                # per operation: what the read's earlier ones consumed
        total = np.cumsum(consumed) - consumed
        return total - np.maximum.accumulate(np.where(first, total, 0)) if total.size else total
    q0, p0 = starts(n * _IS_QUERY[op]), starts(n * _IS_REF[op]) + (pos[read] if read.size else 0)
    line = np.repeat(np.arange(op.shape[0]), n)
    within = np.arange(line.shape[0]) - np.repeat(np.cumsum(n) - n, n)
    o = op[line]
    return Table(read[line], opi[line], np.where(_IS_QUERY[o], q0[line] + within, -1), np.where(_IS_REF[o], p0[line] + within, -1), o)


# ------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Rules:
    """Every rule of sections 7f - 7k the oracle knows, each of which can be switched off."""
    eqx_aligned: bool = True          # = and X count as M
    d_in_depth: bool = True           # a deleted position is covered
    n_skipped: bool = True            # a skipped one is not
    anchor: bool = True               # the base an insertion is anchored at does not support the reference
    p_transparent: bool = True        # ... also with a P between the two
    reverse_mirrored: bool = True     # a reverse read's cycles run from its last stored base
    cycle_clamped: bool = True        # ... and stop at 512
    deletion_once: bool = True        # a D counts once, not per base
    h_in_end5: bool = True            # hard clips count back into the 5' end
    case_folded: bool = True          # a lower-case base is its upper-case one
    qc_fail_dropped: bool = True      # a QC-fail read is not counted
    improper_dropped: bool = True     # nor a paired read that is no proper pair
    insertion_left: bool = True       # an insertion belongs to the reference position on its left
    n_overlap: bool = True            # an N over a record: no observation
    end_strict: bool = True           # B < ref_end
    quality_over_all: bool = True     # the smallest quality is over inserted bases too
    score_saturated: bool = True      # 2^30 - 1
    ties_smallest: bool = True        # ties go to the smallest index


def _next(flag_rows: np.ndarray, read: np.ndarray) -> np.ndarray:
    """Per line: the index of the read's next line with ``flag_rows`` set, or -1."""
    n = read.shape[0]
    if n == 0:
        return np.zeros(0, np.int64)
    behind = np.minimum.accumulate(np.where(flag_rows, np.arange(n), n)[::-1])[::-1]
    nxt = np.concatenate([behind[1:], [n]])
    ok = nxt < n
    nxt = np.where(ok, nxt, 0)
    return np.where(ok & (read[nxt] == read), nxt, -1)


def _previous(flag_rows: np.ndarray, read: np.ndarray) -> np.ndarray:
    n = read.shape[0]
    last = np.maximum.accumulate(np.where(flag_rows, np.arange(n), -1))
    prev = np.concatenate([[-1], last[:-1]]).astype(np.int64) if n else last
    return np.where((prev >= 0) & (read[np.maximum(prev, 0)] == read), prev, -1)


def _pairs(name, flags, ok) -> Tuple[np.ndarray, int, int]:
    """(mate, pairs, groups refused): sections 7i's join by grouping, the reads of ``ok`` only."""
    mate = np.full(name.shape[0], -1, np.int64)
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return mate, 0, 0
    _, inverse, size = np.unique(name[idx], return_inverse=True, return_counts=True)
    kind = np.where(flags[idx] & 1, flags[idx] & 0xC0, 0)
    firsts = np.bincount(inverse, kind == 0x40, size.shape[0])
    seconds = np.bincount(inverse, kind == 0x80, size.shape[0])
    is_pair = (size == 2) & (firsts == 1) & (seconds == 1)
    member = idx[is_pair[inverse]]
    order = member[np.argsort(inverse[is_pair[inverse]], kind="stable")].reshape(-1, 2)
    mate[order[:, 0]], mate[order[:, 1]] = order[:, 1], order[:, 0]
    return mate, int(is_pair.sum()), int(((size >= 2) & ~is_pair).sum())


class Oracle:
    def __init__(self, reference: str, rows, rules: Rules = Rules()):
        self.rules, self.rows, self.n = rules, rows, len(rows)
        self.ref = np.frombuffer(reference.encode(), np.uint8)
        self.t = t = alignment_table(rows)
        self.name = np.array([r[0] for r in rows], np.uint64)
        self.flag = np.array([r[1] for r in rows], np.int64)
        self.pos = np.array([r[2] for r in rows], np.int64)
        self.mapq = np.array([r[6] for r in rows], np.int64)
        self.length = np.array([len(r[4]) for r in rows], np.int64)
        off = np.cumsum(self.length) - self.length
        bases = np.frombuffer("".join(r[4] for r in rows).encode(), np.uint8)
        quals = np.array([v for r in rows for v in r[5]], np.int64)
        has_q = t.q >= 0
        at = np.where(has_q, off[t.read] + t.q, 0) if t.read.size else t.q
        self.raw = np.where(has_q, bases[at], 0).astype(np.int64) if bases.size else np.zeros(t.q.shape[0], np.int64)
        self.base = self.raw & 0xDF if rules.case_folded else self.raw
        self.qual = np.where(has_q, quals[at], 0) if quals.size else np.zeros(t.q.shape[0], np.int64)
        self.aligned = np.isin(t.op, ALIGNED if rules.eqx_aligned else (M,))
        f = self.flag
        self.eligible = (f & markdup.NOT_ELIGIBLE) == 0
        self.measured = (f & qc.NOT_MEASURED) == 0
        proper = ((f & 1) == 0) | ((f & 2) != 0) if rules.improper_dropped else np.ones(self.n, bool)
        fail = (f & 0x200) != 0 if rules.qc_fail_dropped else np.zeros(self.n, bool)
        self.counted = self.eligible & proper & ~fail & (self.mapq > 0) & (self.mapq >= MAPQ_THRESHOLD)
        on_ref = t.p >= 0
        self.ref_end = self.pos + np.bincount(t.read[on_ref], minlength=self.n)             # 7g's: the start plus what is consumed
        self.acgt = np.isin(np.arange(256), list(b"ACGT"))
        with np.errstate(invalid="ignore"):
            inside = on_ref & (t.p < LENGTH)
        self.refbase = np.where(inside, self.ref[np.where(inside, t.p, 0)], 0).astype(np.int64)
        self.refbase = self.refbase & 0xDF if rules.case_folded else self.refbase

    # ---- depth, 7k and 7f ------------------------------------------------------------------------
    def depth(self) -> np.ndarray:
        t = self.t
        covers = self.aligned | ((t.op == D) & self.rules.d_in_depth) | ((t.op == N) & (not self.rules.n_skipped))
        rows = covers & self.counted[t.read] & (t.p >= 0) & (t.p < LENGTH)
        return np.bincount(t.p[rows], minlength=LENGTH)

    def counts(self) -> Tuple[np.ndarray, np.ndarray]:
        """(n_ref, n_total) of ``gvcf.count_positions`` over the whole chromosome."""
        t, r = self.t, self.rules
        good = self.aligned & (self.qual >= Q_THRESHOLD) & self.acgt[self.base & 0xFF] & self.counted[t.read] & (t.p < LENGTH)
        total = np.bincount(t.p[good], minlength=LENGTH) + np.bincount(t.p[(t.op == D) & self.counted[t.read] & (t.p < LENGTH)],
                                                                       minlength=LENGTH)
        follower = _next(np.ones(t.op.shape[0], bool) if not r.p_transparent else (t.q >= 0) | (t.p >= 0), t.read)
        anchor = (follower >= 0) & (t.op[np.maximum(follower, 0)] == I) & r.anchor
        same = good & (self.base == self.refbase) & ~anchor
        return np.bincount(t.p[same], minlength=LENGTH).astype(np.int32), total.astype(np.int32)

    # ---- the quality metrics, 7k -----------------------------------------------------------------
    def tables(self, targets=(), window: int = WINDOW) -> Tuple[Dict[str, np.ndarray], Dict[str, int]]:
        t, r, n = self.t, self.rules, self.n
        out = qc.empty_tables(LENGTH, len(targets), window)
        f = self.flag
        out["FLAGS"][:] = [n, (f & 4 != 0).sum(), (f & 0x100 != 0).sum(), (f & 0x800 != 0).sum(), (f & 0x400 != 0).sum(),
                           (f & 0x200 != 0).sum(), (f & 1 != 0).sum(), (f & 3 == 3).sum(), (f & 0x40 != 0).sum(), (f & 0x80 != 0).sum(),
                           (f & 9 == 9).sum(), (f & 0x10 != 0).sum(), ((f & 4 == 0) & (self.mapq == 0)).sum()]
        me = self.measured
        out["MAPQ"] += np.bincount(self.mapq[me], minlength=256)
        out["LENGTH"] += np.bincount(np.minimum(self.length[me], qc.LAST_LENGTH), minlength=qc.LAST_LENGTH + 1)
        reverse = (f & REV != 0) & r.reverse_mirrored
        stored = lambda q, rd: np.where(reverse[rd], self.length[rd] - 1 - q, q)            # noqa: E731
        limit = qc.LAST_CYCLE if r.cycle_clamped else 1 << 20
        end = (f & 0x80 != 0).astype(np.int64)
        has_q = (t.q >= 0) & me[t.read]
        cycle = np.minimum(stored(t.q, t.read), limit)

        def add(field, rows, cycles=cycle, weight=None):                 # without the clamp a cycle behind the last bin is nobody's
            rows = rows & (cycles <= qc.LAST_CYCLE)
            np.add.at(out["CYCLE"][:, :, field], (end[t.read[rows]], cycles[rows]), 1 if weight is None else weight[rows])
        add(qc.BASES, has_q)
        add(qc.QUALITY_SUM, has_q, weight=self.qual)
        hit = has_q & self.aligned & (t.p < LENGTH) & self.acgt[self.base & 0xFF] & self.acgt[self.refbase & 0xFF]
        wrong = hit & (self.base != self.refbase)
        add(qc.ALIGNED, hit)
        add(qc.MISMATCHES, wrong)
        add(qc.INSERTED, has_q & (t.op == I))
        add(qc.SOFT_CLIPPED, has_q & (t.op == S))
        deleted = (t.op == D) & me[t.read] & (self.length[t.read] > 0)
        if r.deletion_once:                                              # the first line of every D operation
            key = t.read * 65536 + t.opi
            deleted &= np.concatenate([[True], key[1:] != key[:-1]]) if key.size else deleted
        nxt = _next(t.q >= 0, t.read)
        at = np.where(nxt >= 0, t.q[np.maximum(nxt, 0)], self.length[t.read] - 1)           # the next query base, or the last
        add(qc.DELETIONS, deleted, cycles=np.minimum(stored(at, t.read), limit))
        out["QUALITY"][:, 0] += np.bincount(self.qual[hit], minlength=256)
        out["QUALITY"][:, 1] += np.bincount(self.qual[wrong], minlength=256)
        past = np.unique(t.read[self.aligned & me[t.read] & (t.p >= LENGTH)]).shape[0]
        depth = self.depth()
        acgt = self.acgt[self.ref & 0xDF]
        bins = np.minimum(depth, qc.LAST_DEPTH)
        out["DEPTH_HIST"] += np.bincount(bins[acgt], minlength=qc.LAST_DEPTH + 1)
        out["WINDOW_SUM"] += np.bincount(np.arange(LENGTH) // window, depth, out["WINDOW_SUM"].shape[0]).astype(np.int64)
        if len(targets):
            tg = np.asarray(targets, np.int64)
            which = np.searchsorted(tg[:, 0], np.arange(LENGTH), "right") - 1
            on = (which >= 0) & (np.arange(LENGTH) < tg[np.maximum(which, 0), 1])
            out["TARGET_DEPTH_HIST"] += np.bincount(bins[on & acgt], minlength=qc.LAST_DEPTH + 1)
            out["TARGET_SUM"] += np.bincount(which[on], depth[on], tg.shape[0]).astype(np.int64)
            out["TARGET_COVERED"] += np.bincount(which[on], depth[on] >= 1, tg.shape[0]).astype(np.int64)
        mate, pairs, refused = _pairs(self.name, f, me)
        c = np.flatnonzero(mate > np.arange(n))
        m = mate[c]
        ends = self.pos + np.maximum(self.ref_end - self.pos, 1)
        insert = np.maximum(ends[c], ends[m]) - np.minimum(self.pos[c], self.pos[m])
        rc, rm = f[c] & REV != 0, f[m] & REV != 0
        forward, backward = np.where(rc, m, c), np.where(rc, c, m)
        orientation = np.where(rc == rm, 2, np.where(self.pos[forward] < ends[backward], 0, 1))
        np.add.at(out["INSERT"], (orientation, np.minimum(insert, qc.LAST_INSERT)), 1)
        stats = dict(measured=int(me.sum()), counted=int(self.counted.sum()), reads_past_reference=int(past),
                     positions_excluded=int((~acgt).sum()), pairs=pairs, groups_refused=refused)
        return out, stats

    # ---- duplicates, 7j --------------------------------------------------------------------------
    def duplicates(self) -> Dict[str, object]:
        t, r, n = self.t, self.rules, self.n
        clip = np.isin(t.op, (S, H))
        body = ~clip
        counts = clip if r.h_in_end5 else t.op == S
        leading = counts & (_previous(body, t.read) < 0)                   # no line of the read's body in front of it
        trailing = counts & (_next(body, t.read) < 0)
        reverse = self.flag & REV != 0
        ends = self.pos + np.maximum(self.ref_end - self.pos, 1)
        end5 = np.where(reverse, ends - 1 + np.bincount(t.read[trailing], minlength=n), self.pos - np.bincount(t.read[leading], minlength=n))
        ok = self.eligible
        e = np.where(ok, 2 * end5 + reverse, 0)
        sums = np.bincount(t.read[(t.q >= 0) & (self.qual >= markdup.MIN_QUALITY)], self.qual[(t.q >= 0) & (self.qual >= markdup.MIN_QUALITY)],
                           n).astype(np.int64)
        score = np.where(ok, np.minimum(sums, markdup.MAX_SCORE) if r.score_saturated else sums, 0)
        mate, pairs, refused = _pairs(self.name, self.flag, ok)
        kind = np.where(~ok, 0, np.where(mate >= 0, markdup.PAIR, np.where((self.flag & 1 == 0) | (self.flag & 8 != 0), markdup.SINGLE,
                                                                           markdup.UNRESOLVED)))
        duplicate = np.zeros(n, np.uint8)
        tie = 1 if r.ties_smallest else -1
        c = np.flatnonzero((kind == markdup.PAIR) & (mate > np.arange(n)))
        m = mate[c]
        lo, hi = np.minimum(e[c], e[m]), np.maximum(e[c], e[m])
        order = np.lexsort((tie * c, -(score[c] + score[m]), hi, lo))
        first = np.concatenate([[True], (lo[order][1:] != lo[order][:-1]) | (hi[order][1:] != hi[order][:-1])]) if c.size else np.zeros(0, bool)
        lost = order[~first]
        duplicate[c[lost]] = duplicate[m[lost]] = 1
        s = np.flatnonzero(kind == markdup.SINGLE)
        order = np.lexsort((tie * s, -score[s], e[s]))
        first = np.concatenate([[True], e[s][order][1:] != e[s][order][:-1]]) if s.size else np.zeros(0, bool)
        held = np.isin(e[s], e[kind == markdup.PAIR])                     # a single whose end a pair holds loses
        single_lost = ~first[np.argsort(order)] | held if s.size else np.zeros(0, bool)
        duplicate[s[single_lost]] = 1
        counts = dict(reads=n, eligible=int(ok.sum()), pairs=pairs, singles=int(s.shape[0]), unresolved=int((kind == markdup.UNRESOLVED).sum()),
                      groups_refused=refused, duplicate_pairs=int(lost.shape[0]), duplicate_singles=int(single_lost.sum()))
        return dict(e=e, score=score, mate=mate, kind=kind, duplicate=duplicate, counts=counts)

    # ---- observations, 7g ------------------------------------------------------------------------
    def record_lines(self, records):
        """Per line: the record (index, or -1) it speaks about -- an aligned line by its position, an inserted one by the
        reference position beside it, a skipped one by its position -- and whether it is part of the string."""
        t, r = self.t, self.rules
        starts = np.array([rec.start for rec in records], np.int64)
        stops = np.array([rec.end for rec in records], np.int64)
        on_ref = t.p >= 0
        if r.insertion_left:
            beside = _previous(on_ref, t.read)
            key_i = np.where(beside >= 0, t.p[np.maximum(beside, 0)], self.pos[t.read] - 1)
        else:
            beside = _next(on_ref, t.read)
            key_i = np.where(beside >= 0, t.p[np.maximum(beside, 0)], -1)
        text = self.aligned | (t.op == I)
        key = np.where(self.aligned | (t.op == N), t.p, np.where(t.op == I, key_i, -1))
        rec = np.searchsorted(starts, key, "right") - 1
        rec = np.where((rec >= 0) & (key >= 0) & (key < stops[np.maximum(rec, 0)]), rec, -1) if len(records) else np.full(key.shape, -1)
        return rec, text

    def slots(self, records) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(slots, slot_offsets, first) of ``phase.slots_of``."""
        t, r = self.t, self.rules
        starts = np.array([rec.start for rec in records], np.int64)
        first = np.where(self.counted, np.searchsorted(starts, self.pos, "left"), 0)
        count = np.where(self.counted, np.maximum(np.searchsorted(starts, self.ref_end, "left") - first, 0), 0)
        offsets = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
        rec, text = self.record_lines(records)
        use = (rec >= 0) & self.counted[t.read] & (text | (t.op == N))
        lines = np.flatnonzero(use)
        group = t.read[lines] * len(records) + rec[lines]
        order = np.argsort(group, kind="stable")                         # within a group the lines stay in query order
        lines, group = lines[order], group[order]
        cut = np.flatnonzero(np.concatenate([[True], group[1:] != group[:-1]])) if group.size else np.zeros(0, np.int64)
        seen = {}
        for a, b in zip(cut, np.concatenate([cut[1:], [group.shape[0]]])):
            mine = lines[a:b]
            is_text = text[mine]
            string = bytes(self.base[mine][is_text].astype(np.uint8))
            qual_of = is_text if r.quality_over_all else is_text & self.aligned[mine]
            seen[int(group[a])] = (string, int(self.qual[mine][qual_of].min(initial=255)), bool((t.op[mine] == N).any()))
        slots = np.full(int(offsets[-1]), phase.NONE, np.int8)
        for rd in np.flatnonzero(count):
            for k in range(int(count[rd])):
                rec_t = records[int(first[rd]) + k]
                string, low, skipped = seen.get(int(rd) * len(records) + int(first[rd]) + k, (b"", 255, False))
                behind = rec_t.end < self.ref_end[rd] if r.end_strict else rec_t.end <= self.ref_end[rd]
                if not behind or (skipped and r.n_overlap) or low < Q_THRESHOLD:
                    continue
                if string == rec_t.allele_a:
                    slots[offsets[rd] + k] = 0
                elif string == rec_t.allele_b:
                    slots[offsets[rd] + k] = 1
        return slots, offsets, first.astype(np.int64)


def tags_of(slots, offsets, first, ps_of, flip) -> Tuple[np.ndarray, np.ndarray]:
    """7h over given observations at ``phase.Record``s with phase set ``ps_of`` (0: unphased, no record of the phased file) and
    ``flip``: a read's set is the PS of its first observation; n1 / n2 count ``o xor flip`` over its observations in that set."""
    n = first.shape[0]
    hp, ps = np.zeros(n, np.uint8), np.zeros(n, np.int64)
    for r in range(n):
        o = slots[offsets[r]:offsets[r + 1]].astype(np.int64)
        s = ps_of[first[r]:first[r] + o.shape[0]]
        seen = (o >= 0) & (s > 0)
        if seen.any():
            ps[r] = s[seen][0]
            h = o ^ flip[first[r]:first[r] + o.shape[0]]
            n1, n2 = int((seen & (h == 0) & (s == ps[r])).sum()), int((seen & (h == 1) & (s == ps[r])).sum())
            hp[r] = 1 if n1 > n2 else 2 if n2 > n1 else 0
    return hp, ps


def chained(records, slots, offsets, first, window: int = phase.DEFAULT_WINDOW) -> Tuple[np.ndarray, np.ndarray]:
    """(PS per record, 0 where unphased; flip per record) of the restated links and chain over given observations."""
    sets, flip = phase.chain(phase.links_of(slots, offsets, first, len(records), window), window, 2)
    return phase.set_positions(sets, [rec.pos for rec in records]), flip.astype(np.int64)


def phased_records(records, ps_of, flip) -> List[haplotag.PhasedRecord]:
    """The phased records as a phased VCF gives them back: haplotype 1's allele first, so a flipped record with its alleles swapped."""
    return [haplotag.PhasedRecord(rec.start, rec.end, rec.a, rec.b, rec.allele_b if f else rec.allele_a, rec.allele_a if f else rec.allele_b,
                                  int(s)) for rec, f, s in zip(records, flip.tolist(), ps_of.tolist()) if s]


# ------------------------------------------------------------------------------------------------
# the restatements of one corpus, and where the oracle differs
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated(seed: int, profile: str) -> Dict[str, object]:
    reference, rows, records = corpus(seed, profile)
    reads = qc_cases.read_set(rows)
    tables, counts = qc.restated([(reads, 0, LENGTH)], reference, TARGETS, WINDOW, MAPQ_THRESHOLD)
    n_ref, n_total = gvcf.count_positions([reads], reference, 0, LENGTH, Q_THRESHOLD, MAPQ_THRESHOLD)
    slots = phase.slots_of([reads], records, Q_THRESHOLD, MAPQ_THRESHOLD)
    ps_of, flip = chained(records, *slots)
    back = phased_records(records, ps_of, flip)
    return dict(reads=reads, tables=tables, stats={k: int(counts[k]) for k in qc.METRIC_STATS}, n_ref=n_ref, n_total=n_total,
                duplicates=markdup.duplicates_of(reads)[1], slots=slots, phased=back, ps_of=ps_of, flip=flip,
                tags=haplotag.haplotags_restated(reads, back, Q_THRESHOLD, MAPQ_THRESHOLD))


TARGETS = [(0, 40), (690, 700), (700, 720), (1000, 1100), (2040, 2050), (2590, 2700)]


def disagreements(seed: int, profile: str, rules: Rules = Rules()) -> List[str]:
    """The names of what the oracle under ``rules`` and the restatements give differently on one corpus."""
    reference, rows, records = corpus(seed, profile)
    want, oracle = restated(seed, profile), Oracle(reference, rows, rules)
    out = []
    tables, stats = oracle.tables(TARGETS, WINDOW)
    out += ["qc." + k for k in qc.TABLE_NAMES if not np.array_equal(tables[k], want["tables"][k])]
    out += ["qc." + k for k in qc.METRIC_STATS if stats[k] != want["stats"][k]]
    n_ref, n_total = oracle.counts()
    out += [k for k, a, b in (("n_ref", n_ref, want["n_ref"]), ("n_total", n_total, want["n_total"])) if not np.array_equal(a, b)]
    dup = oracle.duplicates()
    out += ["markdup." + k for k in ("e", "score", "mate", "kind", "duplicate") if not np.array_equal(dup[k], want["duplicates"][k])]
    out += ["markdup.counts"] if dup["counts"] != want["duplicates"]["counts"] else []
    slots = oracle.slots(records)
    out += ["phase." + k for k, a, b in zip(("slots", "slot_offsets", "first"), slots, want["slots"]) if not np.array_equal(a, b)]
    tags = tags_of(*slots, want["ps_of"], want["flip"])                  # the oracle's observations, the restatement's phase sets
    out += ["haplotag." + k for k, a, b in zip(("hp", "ps"), tags, want["tags"]) if not np.array_equal(a, b)]
    return out


# ------------------------------------------------------------------------------------------------
# the census
# ------------------------------------------------------------------------------------------------
def census(corpora) -> Counter:
    """How often each situation of DESIGN.md section 7l occurs in ``corpora`` ((reference, rows, records) each), from the rows and
    records alone; the two shares of 14 and the causes of 15 from ``phase.observe_why``."""
    c: Counter = Counter()
    for reference, rows, records in corpora:
        o = Oracle(reference, rows)
        t = o.t
        c["name_groups_of_three"] += sum(1 for v in Counter(r[0] for r in rows).values() if v >= 3)
        for r, (_, flag, pos, cigar, bases, _, _) in enumerate(rows):
            strand, end, n = "reverse" if flag & REV else "forward", "second" if flag & 0x80 else "first", len(bases)
            body = [k for k, (op, _) in enumerate(cigar) if op not in (S, H)]
            for op, _ in cigar:
                c["op_%s" % "MIDNSHP=X"[op]] += 1
            if o.eligible[r]:
                lead = sum(k for op, k in cigar[:body[0]]) if body else 0
                c["negative_end5"] += bool(not flag & REV and pos - lead < 0)
                c["H_S_on_a_reverse_5prime"] += bool(flag & REV and [op for op, _ in cigar[-2:]] == [S, H])
            if not o.measured[r]:
                continue
            c["D_behind_a_leading_clip"] += bool(body and body[0] > 0 and cigar[body[0]][0] == D)
            c["D_behind_the_last_base"] += bool(body and cigar[body[-1]][0] == D)
            i, p = 0, pos
            target = (511 if not flag & REV else n - 1 - 511) if n >= 512 else -1
            past = set()
            for k, (op, length) in enumerate(cigar):
                kind = "M" if op in ALIGNED else "MIDNSHP"[op]
                if op in (I, S) and length >= 65:
                    c["%s_of_65_%s" % (kind, strand)] += 1
                if op in (M, I, S, EQ, X) and i <= target < i + length:
                    c["cycle511_%s_%s" % (kind, strand)] += 1
                    c["cycle511_%s_%s" % (strand, end)] += 1
                if op in ALIGNED and p + length > LENGTH:
                    stored = np.arange(i + max(LENGTH - p, 0), i + length)
                    cycles = n - 1 - stored if flag & REV else stored
                    past |= {"past_the_end_cycle_%s511" % ("ge" if v else "lt") for v in np.unique(cycles >= 511)}
                if o.counted[r] and op in ALIGNED + (D, N):
                    for name, edges in (("tile", TILE_EDGES), ("cut", CUTS)):
                        c["%s_across_a_%s" % (kind, name)] += any(p < e < p + length for e in edges)
                    follower = [x for x, _ in cigar[k + 1:] if x != P]
                    if op in ALIGNED and follower and follower[0] == I:
                        how = "direct" if cigar[k + 1][0] == I else "through_P"
                        c["anchor_%s_last_of_a_tile" % how] += p + length in TILE_EDGES
                        c["anchor_%s_last_of_a_cut" % how] += p + length in CUTS
                i += length if op in (M, I, S, EQ, X) else 0
                p += length if op in ALIGNED + (D, N) else 0
            c.update(past)
        if not records:
            continue
        reads = qc_cases.read_set(rows)
        starts = np.array([rec.start for rec in records], np.int64)
        stops = np.array([rec.end for rec in records], np.int64)
        rec, text = o.record_lines(records)
        under = np.searchsorted(starts, t.p, "right") - 1
        under = np.where((t.p >= 0) & (under >= 0) & (t.p < stops[np.maximum(under, 0)]), under, -1)
        pairs = lambda lines, which: np.unique(t.read[lines] * len(records) + which[lines]).shape[0]      # noqa: E731
        mine = o.counted[t.read]
        c["record_inside_a_D"] += pairs(mine & (t.op == D) & (under >= 0), under)
        c["record_under_an_N"] += pairs(mine & (t.op == N) & (under >= 0), under)
        c["record_with_an_insertion"] += pairs(mine & (t.op == I) & (rec >= 0), rec)
        c["record_with_a_low_quality_base"] += pairs(mine & text & (rec >= 0) & (o.qual < Q_THRESHOLD), rec)
        c["record_with_a_lower_case_or_N_base"] += pairs(mine & text & (rec >= 0) & ~o.acgt[o.raw & 0xFF], rec)
        _, offsets, first = o.slots(records)
        for r in np.flatnonzero(np.diff(offsets)):
            k = int(offsets[r + 1] - offsets[r])
            c["more_than_64_candidates"] += k > 64
            last = [op for op, _ in rows[r][3] if op in ALIGNED + (D, N)][-1]
            for rec_t in records[int(first[r]):int(first[r]) + k]:
                c["record_ends_on_the_last_aligned_base"] += rec_t.end == o.ref_end[r] and last in ALIGNED
                got, why = phase.observe_why(reads, int(r), rec_t, Q_THRESHOLD)
                c["slots"] += 1
                c["observes_%s" % ("a" if got == 0 else "b" if got == 1 else "nothing_" + why)] += 1
    return c


CENSUS_AT_LEAST_5 = tuple("op_" + x for x in "MIDNSHP=X") + tuple(
    "%s_%s" % (a, b) for a in ("I_of_65", "S_of_65", "cycle511_I", "cycle511_S", "cycle511_M") for b in ("forward", "reverse")) + tuple(
    "cycle511_%s_%s" % (a, b) for a in ("forward", "reverse") for b in ("first", "second")) + (
    "past_the_end_cycle_ge511", "past_the_end_cycle_lt511", "anchor_direct_last_of_a_tile", "anchor_through_P_last_of_a_tile",
    "anchor_direct_last_of_a_cut", "anchor_through_P_last_of_a_cut", "D_across_a_tile", "N_across_a_tile", "M_across_a_tile",
    "D_across_a_cut", "N_across_a_cut", "M_across_a_cut", "D_behind_a_leading_clip", "D_behind_the_last_base", "negative_end5",
    "H_S_on_a_reverse_5prime", "record_ends_on_the_last_aligned_base", "record_inside_a_D", "record_under_an_N",
    "record_with_an_insertion", "record_with_a_low_quality_base", "record_with_a_lower_case_or_N_base", "more_than_64_candidates",
    "name_groups_of_three")
CENSUS_CAUSES = ("observes_nothing_end", "observes_nothing_N", "observes_nothing_neither", "observes_nothing_quality")
