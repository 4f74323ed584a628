"""Inputs of the tests of the read pairs and clipped ends (tests/test_sv_pairs.py on the CPU, tests/test_gpu_sv_pairs.py on the GPU):
cases worked by hand, one per rule of DESIGN.md section 7s, at min_size 5, flank 3, clip_min 4 and the library (10, 4, 16) on a
chromosome of 2 600 positions; a stress over the kernel's edges; and a seeded fuzz of single, proper and discordant reads.

A row is a row of tests/sv_split_cases.py with the mate's chromosome and position behind it: (name_hash, flag, position, CIGAR,
bases, qualities, mapq, hp, tag, mate_tid, mate_pos).  The hand cases' expected rows were worked out from the rules, not from the
code.  The fuzz draws its own reads: the generators of tests/read_fuzz.py place reads for phasing and know no mate fields."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from hello_amd import sv
from hello_amd.bam import Mates
from tests import sv_cases as sc, sv_split_cases as ss
from tests.sv_cases import D, H, M, N, REV, S  # noqa: F401

DEL, INS, DUP, INV3, INV5, BND = sv.DEL, sv.INS, sv.DUP, sv.INV3, sv.INV5, sv.BND
PAIRED, PROPER, MATE_UNMAPPED, MREV, FIRST, SECOND, QC_FAIL, DUPLICATE = 0x1, 0x2, 0x8, 0x20, 0x40, 0x80, 0x200, 0x400
CONTIGS, OWN = ss.CONTIGS, ss.OWN                     # chr1 (own), chr2, chrUn_1
LENGTH = 2600
LIBRARY = (10, 4, 16)
HAND = dict(min_size=5, flank=3, mapq_threshold=10, cluster_gap=10, len_ratio_percent=70, min_support=3, clip_min=4)
OP = sv.PAIR_OP


def _reference(length: int, seed: int, differ=()) -> str:
    """Random bases; ``differ``: pairs of positions whose bases differ, so that no deletion between them moves to the left."""
    rng = np.random.default_rng(seed)
    ref = list("".join(rng.choice(list("ACGT"), size=length)))
    for a, b in differ:
        ref[a], ref[b] = "A", "C"
    return "".join(ref)


REFERENCE = _reference(LENGTH, 43, [(499, 539), (814, 864)])


def mated(row: tuple, mt: int = -1, ms: int = -1, tag: bytes = b"") -> tuple:
    return tuple(row[:8]) + (bytes(tag), int(mt), int(ms))


def read(name, pos, cigar, flag=0, mt=-1, ms=-1, mapq=60, hp=0, tag=b"", reference=REFERENCE) -> tuple:
    return mated(sc.row(name, reference, pos, cigar, flag, mapq, hp), mt, ms, tag)


def fr_pair(name, s, ms, n=10, extra=0, reference=REFERENCE) -> List[tuple]:
    """A forward read of n bases at s (first of the pair) and its reverse mate at ms, both on chr1."""
    return [read(name, s, [(M, n)], PAIRED | MREV | FIRST | extra, OWN, ms, reference=reference),
            read(name + 1000, ms, [(M, n)], PAIRED | REV | SECOND | extra, OWN, s, reference=reference)]


def pair_set(rows):
    """Rows -> (Reads, Splits, Mates) as ``fetch_pairs`` would give them."""
    reads, splits = ss.split_set([r[:9] for r in rows])
    return reads, splits, Mates(np.array([r[9] for r in rows], np.int32), np.array([r[10] for r in rows], np.int64),
                                np.zeros(len(rows), np.int32))


def spans_of(rows, length: int, cuts=()):
    """[(reads, splits, mates, lo, hi)]: the chromosome whole, or cut at ``cuts``, each span with the rows a fetch of it returns."""
    rows = sorted(rows, key=lambda r: r[2])
    edges = [0] + list(cuts) + [length]
    return [pair_set(sc.overlapping(rows, lo, hi)) + (lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]


@dataclass
class Case:
    name: str
    rows: List[tuple]
    signatures: List[Tuple[int, ...]]                 # every row of sv.SIGNATURE_COLUMNS, sorted
    clusters: List[Tuple[int, ...]]                   # (type, pos, len, DV, SR, PR, IMPRECISE, CE, DP, DR, END_MIN, END_MAX)
    pair_status: List[int]                            # per row in coordinate order
    counts: Dict[str, int] = field(default_factory=dict)      # of sv.PAIR_COUNT_NAMES, what is not 0
    params: Dict[str, int] = field(default_factory=dict)      # what differs from HAND
    reference: str = REFERENCE

    def __post_init__(self):
        self.rows = sorted(self.rows, key=lambda r: r[2])
        self.signatures = sorted(self.signatures)

    def kw(self) -> Dict[str, int]:
        return dict(HAND, **self.params)

    def cut(self) -> int:
        return self.rows[len(self.rows) // 2][2] + 1

    def want_counts(self) -> Dict[str, int]:
        return dict(dict.fromkeys(sv.PAIR_COUNT_NAMES, 0), **self.counts)


# ---- the hand cases ------------------------------------------------------------------------------------------------------------------
_40D = [(M, 20), (D, 40), (M, 20)]                    # at 480: the deletion of 500 .. 539, which cannot move (REFERENCE differs there)
_CARRIERS = [read(k, 480, _40D) for k in (1, 2, 3)]
_D_ROWS = [(DEL, 500, 40, 0, k, 1, 0, 0) for k in range(3)]
# four pairs around it: (a, b) = (read end, mate start); (b - a) - 40 = 15, 14, 14, 13, inside [4, 16]
_AB = [(488, 542), (490, 545), (492, 546), (495, 548)]


def _straddling(ab, extra=0):
    return [r for k, (a, b) in enumerate(ab) for r in fr_pair(10 + k, a - 10, b, extra=extra)]


def _pair_rows(ab, first_ordinal=0, step=1):
    """The DEL rows of left records that end at a with mates at b: len = (b - a) - median."""
    return [(DEL, a, b - a - 10, b, first_ordinal + step * k, OP, 0, 0) for k, (a, b) in enumerate(ab)]


_FIVE = [(998, 1099), (1000, 1100), (1001, 1102), (1002, 1101), (1004, 1103)]         # lens 91, 90, 91, 89, 89: the lower median 90

HAND_TABLE: List[Case] = [
    # in coordinate order: the left read at 478, the three carriers and the left read at 480, the lefts at 482 and 485, the four
    # rights.  The lefts are pair ordinals 0 .. 3, the carriers counting ordinals 0 .. 2 (with 0x2 on the pairs, below: 1 .. 3).  No
    # pair read has 0x2, so none is among the counting reads: DP at 500 is the three carriers', DR = max(0, 3 - 3) = 0
    Case("a 40D of three reads takes the four pairs that straddle it", _CARRIERS + _straddling(_AB),
         _D_ROWS + _pair_rows(_AB), [(DEL, 500, 40, 3, 0, 4, 0, 0, 3, 0, 540, 540)],
         [7, 0, 0, 0, 7, 7, 7, 2, 2, 2, 2], dict(pair_reads=8, pairs_left=4, pairs_right=4, pair_signatures=4, pairs_assigned=4)),
    # (547 - 490) - 40 = 17 is above hi: the pair stays a row and joins nothing; alone it is below min_support
    Case("a pair whose inner distance less the deletion is 17 is not assigned", _CARRIERS + _straddling([(488, 542), (490, 547), (492, 546), (495, 548)]),
         _D_ROWS + _pair_rows([(488, 542), (490, 547), (492, 546), (495, 548)]), [(DEL, 500, 40, 3, 0, 3, 0, 0, 3, 0, 540, 540)],
         [7, 0, 0, 0, 7, 7, 7, 2, 2, 2, 2], dict(pair_reads=8, pairs_left=4, pairs_right=4, pair_signatures=4, pairs_assigned=3)),
    # with 0x2 the same pair reads count: each left read covers its 483 .. 492 at most, each mate begins behind 540, so the depth at
    # 500 is still the carriers' three -- pair supporters are not in DP
    Case("flag 0x2 on a discordant pair: still a row, and pair supporters are not in DP", _CARRIERS + _straddling(_AB, PROPER),
         [(DEL, 500, 40, 0, k, 1, 0, 0) for k in (1, 2, 3)] + _pair_rows(_AB),
         [(DEL, 500, 40, 3, 0, 4, 0, 0, 3, 0, 540, 540)], [7, 0, 0, 0, 7, 7, 7, 2, 2, 2, 2],
         dict(pair_reads=8, pairs_left=4, pairs_right=4, pair_signatures=4, pairs_assigned=4)),
    # a proper pair 486 .. 496 / 508 .. 518 (inner distance 12) spans the deletion as a fragment; neither read covers 500 with its
    # flanks, and the pair is counted nowhere: DP, DR and the genotype are those of the first case
    Case("a normal pair that spans the event is no reference support", _CARRIERS + _straddling(_AB) + fr_pair(30, 486, 508, extra=PROPER),
         _D_ROWS + _pair_rows(_AB),
         [(DEL, 500, 40, 3, 0, 4, 0, 0, 3, 0, 540, 540)], [7, 0, 0, 0, 7, 7, 7, 3, 2, 2, 2, 2, 2],
         dict(pair_reads=10, pairs_left=5, pairs_right=5, pairs_normal=1, pair_signatures=4, pairs_assigned=4)),
    # five pairs and nothing else: POS = max a = 1004, END = min b = 1099, LEN the lower median of (b - a) - 10
    Case("five pairs alone are an imprecise deletion", _straddling(_FIVE), _pair_rows(_FIVE),
         [(DEL, 1004, 90, 0, 0, 5, 1, 0, 0, 0, 1099, 1103)], [7] * 5 + [2] * 5,
         dict(pair_reads=10, pairs_left=5, pairs_right=5, pair_signatures=5, pair_candidates=1), dict(min_support=5)),
    Case("four pairs are below min_support 5", _straddling(_FIVE[:4]), _pair_rows(_FIVE[:4]), [], [7] * 4 + [2] * 4,
         dict(pair_reads=8, pairs_left=4, pairs_right=4, pair_signatures=4), dict(min_support=5)),
    # the left record is reverse, its mate forward: the read at 1500 .. 1510 with its mate at 1560 is a duplication of 60; the pair
    # whose mate begins at 1705, inside the read 1700 .. 1710, is a read-through
    Case("an RF pair is a duplication, a read-through pair is none",
         [read(1, 1500, [(M, 10)], PAIRED | REV | FIRST, OWN, 1560), read(2, 1700, [(M, 10)], PAIRED | REV | FIRST, OWN, 1705)],
         [(DUP, 1500, 60, 1560, 0, OP, 1, 0)], [], [7, 5], dict(pair_reads=2, pairs_left=2, pairs_small=1, pair_signatures=1)),
    Case("FF and RR pairs are inversion junctions",
         [read(1, 1700, [(M, 10)], PAIRED | FIRST, OWN, 1800, hp=1), read(2, 1900, [(M, 10)], PAIRED | REV | MREV | FIRST, OWN, 2000)],
         [(INV3, 1710, 90, 1800, 0, OP, 0, 1), (INV5, 1900, 100, 2000, 1, OP, 1, 0)], [], [7, 7],
         dict(pair_reads=2, pairs_left=2, pair_signatures=2)),
    # a forward read leaves at its end, a reverse read at its start; chr7 is not in the header, nor is -1
    Case("a mate on another chromosome is a BND; one outside the header is unplaced",
         [read(1, 2000, [(M, 10)], PAIRED | FIRST, 1, 300), read(2, 2020, [(M, 10)], PAIRED | REV | FIRST, 2, 7),
          read(3, 2040, [(M, 10)], PAIRED | FIRST, 7, 5), read(4, 2060, [(M, 10)], PAIRED | FIRST, -1, 5)],
         [(BND, 2010, 1, 300, 0, OP, 0, 0), (BND, 2020, 2, 7, 1, OP, 1, 0)], [], [8, 8, 6, 6],
         dict(pair_reads=4, pairs_unplaced=2, pair_signatures=2)),
    # both records start at 2100: the one with 0x40 is the left one (FR, inner distance -10: short), the other the right one
    Case("mates at one position: 0x40 decides",
         [read(1, 2100, [(M, 10)], PAIRED | MREV | FIRST, OWN, 2100), read(2, 2100, [(M, 10)], PAIRED | REV | SECOND, OWN, 2100)],
         [], [], [4, 2], dict(pair_reads=2, pairs_left=1, pairs_right=1, pairs_short=1)),
    Case("mate unmapped, QC-fail, duplicate and mapq 9 are not pair-counted",
         [read(1, 2200, [(M, 10)], PAIRED | MREV | FIRST | MATE_UNMAPPED, OWN, 2400), read(2, 2201, [(M, 10)], PAIRED | MREV | FIRST | QC_FAIL, OWN, 2400),
          read(3, 2202, [(M, 10)], PAIRED | MREV | FIRST | DUPLICATE, OWN, 2400), read(4, 2203, [(M, 10)], PAIRED | MREV | FIRST, OWN, 2400, mapq=9),
          read(5, 2204, [(M, 10)], MREV, OWN, 2400)],
         [], [], [0] * 5),
    # -1 and 2601 on the own chromosome and 2^31 anywhere are BAD_MATE; 2600 = length is valid: a deletion row that ends there
    Case("mate positions at the edges",
         [read(1, 2300, [(M, 10)], PAIRED | MREV | FIRST, OWN, -1), read(2, 2301, [(M, 10)], PAIRED | MREV | FIRST, OWN, LENGTH),
          read(3, 2302, [(M, 10)], PAIRED | MREV | FIRST, OWN, LENGTH + 1), read(4, 2303, [(M, 10)], PAIRED | MREV | FIRST, 1, 1 << 31),
          read(5, 2304, [(M, 10)], PAIRED | MREV | FIRST, 1, (1 << 31) - 1)],
         [(DEL, 2311, 279, LENGTH, 1, OP, 0, 0), (BND, 2314, 1, (1 << 31) - 1, 4, OP, 0, 0)], [], [1, 7, 1, 1, 8],
         dict(pair_reads=5, pairs_left=1, bad_mate=3, pair_signatures=2)),
    # 3S is too short; 4S counts where the aligned part starts (CLIP_RIGHT[100]); 5S .. 6S counts on both sides (CLIP_RIGHT[120],
    # CLIP_LEFT[130]); H is no clip, an S behind an H is one (CLIP_RIGHT[160]); a read with an SA tag is 7q's business
    Case("clipped ends",
         [read(1, 80, [(S, 3), (M, 10)]), read(2, 100, [(S, 4), (M, 10)]), read(3, 120, [(S, 5), (M, 10), (S, 6)]), read(4, 140, [(H, 5), (M, 10)]),
          read(5, 160, [(H, 2), (S, 4), (M, 10)]), read(6, 180, [(S, 8), (M, 10)], tag=ss.sa("chr2", 50, "+", "8M10S"))],
         [(BND, 180, 1, 58, 5, -1, 0, 0)], [], [0] * 6, dict(clipped_reads=3)),
    # one read shows the deletion 815 .. 864 twice: as a split alignment (15M at 800, the rest at 865) and as a pair (its mate at
    # 880: 65 - 50 = 15).  Both count: SR 1 and PR 1, SUPPORT 2.  Its cover ends at 812, so DP = 0
    Case("a read with a split row and a pair row counts in SR and in PR",
         [read(1, 800, [(M, 15), (S, 15)], PAIRED | PROPER | MREV | FIRST, OWN, 880, tag=ss.sa("chr1", 865, "+", "15S15M"))],
         [(DEL, 815, 50, 0, 0, -1, 0, 0), (DEL, 815, 55, 880, 0, OP, 0, 0)], [(DEL, 815, 50, 1, 1, 1, 0, 0, 0, 0, 865, 865)], [7],
         dict(pair_reads=1, pairs_left=1, pair_signatures=1, pairs_assigned=1), dict(min_support=1)),
    # 2595 .. 2605 ends beyond the chromosome of 2 600: as a pair-counted read it is BAD_MATE whatever its mate fields say, as a
    # clipped read it counts nowhere (CLIP_LEFT has length + 1 entries).  The reads that end exactly at 2 600 are inside: the 4S
    # before 2590 counts at CLIP_RIGHT[2590], the 4S behind 2600 at CLIP_LEFT[2600], the last entry
    Case("reads that end at and beyond the end of the chromosome",
         [read(1, 2590, [(S, 4), (M, 10)]), read(2, 2590, [(M, 10), (S, 4)]), read(3, 2595, [(M, 10)], PAIRED | MREV | FIRST, OWN, 2598),
          read(4, 2595, [(S, 4), (M, 10), (S, 4)]), read(5, 2596, [(M, 4)], PAIRED | MREV | FIRST, OWN, 2600)],
         [], [], [0, 0, 1, 0, 4], dict(pair_reads=2, pairs_left=1, pairs_short=1, bad_mate=1, clipped_reads=2)),
]
END_CASE = HAND_TABLE[-1]
END_CLIPS = dict(CLIP_LEFT={LENGTH: 1}, CLIP_RIGHT={2590: 1})
CLIP_CASE = [c for c in HAND_TABLE if c.name == "clipped ends"][0]
CLIPS = dict(CLIP_LEFT={130: 1}, CLIP_RIGHT={100: 1, 120: 1, 160: 1})


# ---- the stress: the kernel's edges ---------------------------------------------------------------------------------------------------
STRESS_LENGTH = 6000
STRESS = dict(min_size=10, flank=5, mapq_threshold=10, cluster_gap=20, len_ratio_percent=70, min_support=2, clip_min=4)
STRESS_LIBRARY = (200, 100, 300)
STRESS_REFERENCE = _reference(STRESS_LENGTH, 47)


def _s(name, pos, cigar, flag=0, mt=-1, ms=-1, **kw):
    return read(name, pos, cigar, flag, mt, ms, reference=STRESS_REFERENCE, **kw)


def rows_emitting(n: int) -> List[tuple]:
    """n reads with a BND row each, every third behind a read that emits none: the ballot's lanes are not all set."""
    rows = []
    for k in range(n):
        rows.append(_s(2 * k, 100 + 3 * k, [(M, 12)], PAIRED | FIRST | (REV if k % 5 == 0 else 0), 1 + k % 2, 40 + k, hp=k % 3))
        if k % 3 == 0:
            rows.append(_s(2 * k + 1, 100 + 3 * k, [(M, 12)], 0))
    return rows


EMITTING = (63, 64, 65, 257)
INNER_EDGES = (-1025, -1024, 3071, 3072)


def inner_edge_rows() -> List[tuple]:
    """Left FR records whose inner distances are the edges of INNER: a negative one needs a read that spans more than it."""
    rows = []
    for k, g in enumerate(INNER_EDGES):
        cigar = [(M, 10), (N, 1100), (M, 10)] if g < 0 else [(M, 20)]
        e = 300 + 10 * k + sum(n for _, n in cigar)
        rows.append(_s(k, 300 + 10 * k, cigar, PAIRED | MREV | FIRST, OWN, e + g))
    return rows


def one_bin_rows(n: int = 300) -> List[tuple]:
    """n pairs, all of inner distance 200: one LDS counter takes every add of two workgroups."""
    return [r for k in range(n) for r in fr_pair(k, 500 + 2 * k, 500 + 2 * k + 20 + 200, n=20, reference=STRESS_REFERENCE)]


def across_rows() -> List[tuple]:
    """A discordant pair whose mates lie in two spans of 700, six of them (an imprecise deletion), and clipped reads at the cut."""
    rows = [r for k in range(6) for r in fr_pair(k, 600 + 3 * k, 1500 + 2 * k, n=20, reference=STRESS_REFERENCE)]
    rows += [_s(100 + k, 695 + k, [(S, 6), (M, 20), (S, 4)]) for k in range(10)]
    rows += [_s(120 + k, 613 + k, [(M, 20), (S, 6)]) for k in range(4)]       # ends clipped at the left breakpoint, 633 .. 636
    rows += [_s(130 + k, 1498 + k, [(S, 6), (M, 20)]) for k in range(3)]      # and at the right one
    return rows


STRESS_SETS = dict([("emitting%d" % n, rows_emitting(n)) for n in EMITTING]
                   + [("inner_edges", inner_edge_rows()), ("one_bin", one_bin_rows()), ("across", across_rows()),
                      ("no_pairs", [_s(k, 200 + 7 * k, [(M, 30)]) for k in range(20)])])
STRESS_CUTS = tuple(range(sc.SPAN, STRESS_LENGTH, sc.SPAN))


# ---- the fuzz ------------------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = tuple(range(700, 732))
FUZZ_LENGTH = 3000
FUZZ = dict(min_size=8, flank=4, mapq_threshold=10, cluster_gap=30, len_ratio_percent=70, min_support=2, clip_min=5)
FUZZ_LIBRARY = (60, 20, 100)


def fuzz(seed: int) -> Tuple[str, List[tuple]]:
    """(reference, rows): single reads, proper pairs and discordant pairs of every orientation around a few planted events, with
    clips, deletions, SA tags, bad flags and bad mate fields mixed in."""
    rng = np.random.default_rng(seed)
    reference = _reference(FUZZ_LENGTH, seed + 1)
    rows: List[tuple] = []
    events = [(int(rng.integers(200, 2500)), int(rng.integers(30, 300))) for _ in range(4)]
    name = 0

    def body(n):
        kind = rng.integers(0, 8)
        if kind == 0:
            return [(S, int(rng.integers(1, 9))), (M, n)]
        if kind == 1:
            return [(M, n), (S, int(rng.integers(1, 9)))]
        if kind == 2:
            return [(H, 3), (S, int(rng.integers(3, 8))), (M, n), (S, int(rng.integers(3, 8)))]
        if kind == 3:
            return [(M, n // 2), (D, int(rng.integers(6, 40))), (M, n - n // 2)]
        return [(M, n)]

    for at, size in events:                                                  # the event as a D operation of a few single reads
        for _ in range(int(rng.integers(0, 4))):
            name += 2
            rows.append(read(name, at - 15, [(M, 15), (D, size), (M, 15)], REV if rng.random() < 0.5 else 0, reference=reference))
    for _ in range(int(rng.integers(150, 260))):
        n = int(rng.integers(20, 40))
        what = rng.integers(0, 10)
        mapq = int(rng.choice([60, 60, 60, 30, 9, 0]))
        hp = int(rng.integers(0, 3))
        flag = 0
        for bit, p in ((QC_FAIL, 0.02), (DUPLICATE, 0.02), (0x100, 0.02), (0x800, 0.02), (0x4, 0.01), (MATE_UNMAPPED, 0.03)):
            flag |= bit if rng.random() < p else 0
        tag = b""
        if rng.random() < 0.08:
            tag = ss.sa(str(rng.choice(["chr1", "chr2", "chrX"])), int(rng.integers(0, FUZZ_LENGTH - 100)), str(rng.choice(["+", "-"])),
                        "%dS%dM" % (5, n)) if rng.random() < 0.8 else b"garbage;"
        name += 2
        if what < 2:                                                         # a single read
            rows.append(read(name, int(rng.integers(0, FUZZ_LENGTH - 120)), body(n), flag | (REV if rng.random() < 0.5 else 0), mapq=mapq,
                             hp=hp, tag=tag, reference=reference))
            continue
        if what < 5:                                                         # a proper pair near the library's median
            s = int(rng.integers(0, FUZZ_LENGTH - 400))
            ms = s + n + int(rng.integers(10, 120))
            own_rev, mate_rev = False, True
        else:                                                                # a discordant pair around an event
            at, size = events[int(rng.integers(0, len(events)))]
            s = max(0, at - n - int(rng.integers(0, 40)))
            ms = min(FUZZ_LENGTH - 60, at + size + int(rng.integers(0, 40)))
            own_rev, mate_rev = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
            if rng.random() < 0.15:                                          # mates that overlap or lie a few bases apart
                ms = s + int(rng.integers(0, n + 6))
        mt = OWN
        if rng.random() < 0.08:
            mt = int(rng.choice([1, 2, 3, -1, 9]))
        bad = rng.random()
        left_ms = -1 if bad < 0.02 else FUZZ_LENGTH + 1 if bad < 0.04 else 1 << 31 if bad < 0.05 else ms
        pairing = PAIRED | (PROPER if rng.random() < 0.5 else 0)
        rows.append(read(name, s, body(n), flag | pairing | FIRST | (REV if own_rev else 0) | (MREV if mate_rev else 0), mt, left_ms,
                         mapq, hp, tag, reference))
        if mt == OWN and rng.random() < 0.9:
            rows.append(read(name + 1, ms, [(M, n)], pairing | SECOND | (REV if mate_rev else 0) | (MREV if own_rev else 0), OWN, s, mapq,
                             hp, reference=reference))
    for k in range(int(rng.integers(2, 6))):                                 # reads that end at and beyond the end of the chromosome
        name += 2
        n = int(rng.integers(20, 40))
        s = FUZZ_LENGTH - n + int(rng.integers(-3, 12))
        flag = int(rng.choice([0, PAIRED | MREV | FIRST, PAIRED | PROPER | MREV | FIRST, PAIRED | REV | FIRST]))
        rows.append(read(name, s, body(n), flag, OWN, int(rng.integers(s, FUZZ_LENGTH + 1)), reference=reference))
    return reference, sorted(rows, key=lambda r: r[2])
