"""Inputs of the quality-metrics tests (tests/test_qc.py on the CPU, tests/test_gpu_qc.py on the GPU): tables worked by hand, one
case per rule of DESIGN.md section 7k, and the edge stress on one 6 kb chromosome.

A hand row is (name_hash, flag, position, CIGAR, bases, qualities, mapq) on a reference of 200 bases, ``ACGT`` fifty times unless
the case changes it; ``seq(p, n)`` are the reference's own bases.  Windows are 50 wide, the mapq threshold is 10.  The expected
tables are written sparsely -- what is not named is 0 -- and were worked out from the rules, not from the code."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from hello_amd import qc
from hello_amd.bam import Reads
from tests.gvcf_cases import D, H, I, M, N, S, reads_of

REF = "ACGT" * 50
REV = 0x10
WINDOW = 50


def seq(pos: int, n: int, reference: str = REF) -> str:
    return (reference[pos:pos + n].upper() + "A" * n)[:n]


def q(n: int, value: int = 30) -> List[int]:
    return [value] * n


def read_set(rows) -> Reads:
    """Rows -> the arrays ``hello_bam_fetch`` would give."""
    made = [(pos, cigar, bases, quals, flag, mapq) for _, flag, pos, cigar, bases, quals, mapq in rows]
    return dataclasses.replace(reads_of(made), name_hash=np.array([row[0] for row in rows], np.uint64))


def overlapping(rows, lo: int, hi: int):
    """The rows a fetch of [lo, hi) returns: those whose reference span overlaps it."""
    def end(row):
        return row[2] + max(1, sum(k for op, k in row[3] if op in (M, D, N, 7, 8)))
    return [row for row in rows if end(row) > lo and row[2] < hi]


def cyc(bases=0, quality_sum=0, aligned=0, mismatches=0, inserted=0, soft_clipped=0, deletions=0) -> List[int]:
    return [bases, quality_sum, aligned, mismatches, inserted, soft_clipped, deletions]


@dataclass
class Case:
    name: str
    rows: List[tuple]
    flags: Dict[str, int]
    mapq: Dict[int, int]
    length: Dict[int, int]
    cycle: Dict[Tuple[int, int], List[int]]          # (end, cycle) -> the seven fields
    quality: Dict[int, Tuple[int, int]]              # reported quality -> (aligned, mismatches)
    depth_hist: Dict[int, int]
    window_sum: List[int]
    counts: Dict[str, int]                           # of qc.METRIC_STATS, what is not 0
    insert: Dict[Tuple[int, int], int] = field(default_factory=dict)     # (orientation, insert) -> pairs
    reference: str = REF
    targets: List[Tuple[int, int]] = field(default_factory=list)
    target_hist: Dict[int, int] = field(default_factory=dict)
    target_sum: List[int] = field(default_factory=list)
    target_covered: List[int] = field(default_factory=list)

    def reads(self) -> Reads:
        return read_set(self.rows)

    def cut(self) -> int:
        """Where the two-span run cuts the chromosome: through the middle of the first read that has a middle."""
        for row in self.rows:
            if sum(k for op, k in row[3] if op in (M, D, N)) >= 3:
                return row[2] + 2
        return 100

    def expected(self) -> Dict[str, np.ndarray]:
        out = qc.empty_tables(len(self.reference), len(self.targets), WINDOW)
        for name, v in self.flags.items():
            out["FLAGS"][qc.FLAG_NAMES.index(name)] = v
        for table, sparse in (("MAPQ", self.mapq), ("LENGTH", self.length), ("DEPTH_HIST", self.depth_hist),
                              ("TARGET_DEPTH_HIST", self.target_hist), ("CYCLE", self.cycle), ("QUALITY", self.quality),
                              ("INSERT", self.insert)):
            for k, v in sparse.items():
                out[table][k] = v
        out["WINDOW_SUM"][:] = self.window_sum
        out["TARGET_SUM"][:] = self.target_sum
        out["TARGET_COVERED"][:] = self.target_covered
        return out

    def want_counts(self) -> Dict[str, int]:
        return dict(dict.fromkeys(qc.METRIC_STATS, 0), **self.counts)


def _replace(reference: str, at: int, text: str) -> str:
    return reference[:at] + text + reference[at + len(text):]


M4 = [(M, 4)]
_ONE = {(0, c): cyc(1, 30, 1) for c in range(4)}             # one forward read of 4 matching bases at quality 30
F1, R2, R1, F2 = 0x63, 0x93, 0x53, 0xA3

HAND_TABLE: List[Case] = [
    # the reverse read's stored bases 0..3 are cycles 3..0; its stored base 0 (quality 11) differs from the reference
    Case("forward and reverse cycles",
         [(1, 0, 10, M4, seq(10, 4), [10, 20, 30, 40], 60), (2, REV, 20, M4, "C" + seq(21, 3), [11, 21, 31, 41], 60)],
         dict(reads=2, reverse=1), {60: 2}, {4: 2},
         {(0, 0): cyc(2, 51, 2), (0, 1): cyc(2, 51, 2), (0, 2): cyc(2, 51, 2), (0, 3): cyc(2, 51, 2, 1)},
         {10: (1, 0), 20: (1, 0), 30: (1, 0), 40: (1, 0), 11: (1, 1), 21: (1, 0), 31: (1, 0), 41: (1, 0)},
         {0: 192, 1: 8}, [8, 0, 0, 0], dict(measured=2, counted=2)),
    Case("read 2 into the second half", [(1, 0x83, 10, [(M, 3)], seq(10, 3), q(3), 60)],
         dict(reads=1, paired=1, proper_pair=1, read2=1), {60: 1}, {3: 1}, {(1, c): cyc(1, 30, 1) for c in range(3)}, {30: (3, 0)},
         {0: 197, 1: 3}, [3, 0, 0, 0], dict(measured=1, counted=1)),
    # forward 2I3M: cycles 0, 1 inserted; reverse 3M2I: the insertion is stored last and sequenced first, cycles 1, 0
    Case("an insertion as first and as last operation",
         [(1, 0, 10, [(I, 2), (M, 3)], "TT" + seq(10, 3), q(5), 60), (2, REV, 20, [(M, 3), (I, 2)], seq(20, 3) + "TT", q(5), 60)],
         dict(reads=2, reverse=1), {60: 2}, {5: 2},
         {(0, 0): cyc(2, 60, inserted=2), (0, 1): cyc(2, 60, inserted=2), (0, 2): cyc(2, 60, 2), (0, 3): cyc(2, 60, 2),
          (0, 4): cyc(2, 60, 2)}, {30: (6, 0)}, {0: 194, 1: 6}, [6, 0, 0, 0], dict(measured=2, counted=2)),
    # 2M3D2M: two bases before the D, cycle 2.  2D3M: none before it, stored base 0.  Reverse 3M1D: all three before it, the
    # last stored base (2), which a reverse read sequenced first: cycle 0.  Depth: 7 + 5 + 4 positions
    Case("a deletion's cycle, including a D before any base",
         [(1, 0, 10, [(M, 2), (D, 3), (M, 2)], seq(10, 2) + seq(15, 2), q(4), 60), (2, 0, 30, [(D, 2), (M, 3)], seq(32, 3), q(3), 60),
          (3, REV, 50, [(M, 3), (D, 1)], seq(50, 3), q(3), 60)],
         dict(reads=3, reverse=1), {60: 3}, {4: 1, 3: 2},
         {(0, 0): cyc(3, 90, 3, deletions=2), (0, 1): cyc(3, 90, 3), (0, 2): cyc(3, 90, 3, deletions=1), (0, 3): cyc(1, 30, 1)},
         {30: (10, 0)}, {0: 184, 1: 16}, [12, 4, 0, 0], dict(measured=3, counted=3)),
    # 2H2S3M1S3H: six stored bases, the hard clips are none
    Case("soft and hard clips", [(1, 0, 10, [(H, 2), (S, 2), (M, 3), (S, 1), (H, 3)], "GG" + seq(10, 3) + "G", q(6), 60)],
         dict(reads=1), {60: 1}, {6: 1},
         {(0, 0): cyc(1, 30, soft_clipped=1), (0, 1): cyc(1, 30, soft_clipped=1), (0, 2): cyc(1, 30, 1), (0, 3): cyc(1, 30, 1),
          (0, 4): cyc(1, 30, 1), (0, 5): cyc(1, 30, soft_clipped=1)}, {30: (3, 0)}, {0: 197, 1: 3}, [3, 0, 0, 0],
         dict(measured=1, counted=1)),
    Case("an N skip leaving the depth alone", [(1, 0, 10, [(M, 2), (N, 5), (M, 2)], seq(10, 2) + seq(17, 2), q(4), 60)],
         dict(reads=1), {60: 1}, {4: 1}, _ONE, {30: (4, 0)}, {0: 196, 1: 4}, [4, 0, 0, 0], dict(measured=1, counted=1)),
    # reference 10..13 is "gtac"; the read says G, A (a mismatch), a (lower case, equal), C
    Case("lower-case reference", [(1, 0, 10, M4, "GAaC", q(4), 60)], dict(reads=1), {60: 1}, {4: 1},
         {(0, 0): cyc(1, 30, 1), (0, 1): cyc(1, 30, 1, 1), (0, 2): cyc(1, 30, 1), (0, 3): cyc(1, 30, 1)}, {30: (4, 1)},
         {0: 196, 1: 4}, [4, 0, 0, 0], dict(measured=1, counted=1), reference=_replace(REF, 10, "gtac")),
    # position 11 is N: not aligned, not in the histogram (199 positions), but in the window sum
    Case("N in the reference", [(1, 0, 10, M4, seq(10, 4), q(4), 60)], dict(reads=1), {60: 1}, {4: 1},
         {(0, 0): cyc(1, 30, 1), (0, 1): cyc(1, 30), (0, 2): cyc(1, 30, 1), (0, 3): cyc(1, 30, 1)}, {30: (3, 0)},
         {0: 196, 1: 3}, [4, 0, 0, 0], dict(measured=1, counted=1, positions_excluded=1), reference=_replace(REF, 11, "N")),
    Case("N in a read", [(1, 0, 10, M4, "GTNC", q(4), 60)], dict(reads=1), {60: 1}, {4: 1},
         {(0, 0): cyc(1, 30, 1), (0, 1): cyc(1, 30, 1), (0, 2): cyc(1, 30), (0, 3): cyc(1, 30, 1)}, {30: (3, 0)},
         {0: 196, 1: 4}, [4, 0, 0, 0], dict(measured=1, counted=1)),
    # none is measured, none is counted; the unmapped read's mapq 0 is not a mapped read's
    Case("a QC-fail / duplicate / secondary read in FLAGS only",
         [(1, 0x200, 10, M4, seq(10, 4), q(4), 60), (2, 0x400, 11, M4, seq(11, 4), q(4), 60), (3, 0x100, 12, M4, seq(12, 4), q(4), 60),
          (4, 0x4, 13, M4, seq(13, 4), q(4), 0), (5, 0x800, 14, M4, seq(14, 4), q(4), 60)],
         dict(reads=5, unmapped=1, secondary=1, supplementary=1, duplicate=1, qc_fail=1), {}, {}, {}, {}, {0: 200}, [0, 0, 0, 0], {}),
    Case("a read with mapq below the threshold that is measured but not counted",
         [(1, 0, 10, M4, seq(10, 4), q(4), 9), (2, 0, 20, M4, seq(20, 4), q(4), 0)],
         dict(reads=2, mapq0=1), {9: 1, 0: 1}, {4: 2}, {(0, c): cyc(2, 60, 2) for c in range(4)}, {30: (8, 0)}, {0: 200},
         [0, 0, 0, 0], dict(measured=2)),
    # 0x41 and 0x81 of one name: joined (both forward: TANDEM, 34 - 10), measured, but paired without 0x2: not counted
    Case("an improper pair that is measured but not counted",
         [(1, 0x41, 10, M4, seq(10, 4), q(4), 60), (1, 0x81, 30, M4, seq(30, 4), q(4), 60)],
         dict(reads=2, paired=2, read1=1, read2=1), {60: 2}, {4: 2},
         dict(list(_ONE.items()) + [((1, c), cyc(1, 30, 1)) for c in range(4)]), {30: (8, 0)}, {0: 200}, [0, 0, 0, 0],
         dict(measured=2, pairs=1), insert={(2, 24): 1}),
    # 5M at 197: three bases on the reference, two behind its end
    Case("a read running past the reference's end", [(1, 0, 197, [(M, 5)], seq(197, 5), q(5), 60)],
         dict(reads=1), {60: 1}, {5: 1},
         {(0, 0): cyc(1, 30, 1), (0, 1): cyc(1, 30, 1), (0, 2): cyc(1, 30, 1), (0, 3): cyc(1, 30), (0, 4): cyc(1, 30)}, {30: (3, 0)},
         {0: 197, 1: 3}, [0, 0, 0, 3], dict(measured=1, counted=1, reads_past_reference=1)),
    # name 1: forward at 10, reverse over [40, 44): FR, 34.  name 2: reverse over [20, 24), forward at 60: RF, 44.  name 3: both
    # forward, 30 and [70, 74): TANDEM, 44.  name 4: three reads, left apart.  name 5: unpaired
    Case("FR, RF and TANDEM pairs, a refused group, and a single",
         [(1, F1, 10, M4, seq(10, 4), q(4), 60), (2, R1, 20, M4, seq(20, 4), q(4), 60), (3, 0x43, 30, M4, seq(30, 4), q(4), 60),
          (1, R2, 40, M4, seq(40, 4), q(4), 60), (2, F2, 60, M4, seq(60, 4), q(4), 60), (3, 0x83, 70, M4, seq(70, 4), q(4), 60),
          (4, F1, 80, M4, seq(80, 4), q(4), 60), (4, R2, 90, M4, seq(90, 4), q(4), 60), (4, R2, 100, M4, seq(100, 4), q(4), 60),
          (5, 0, 110, M4, seq(110, 4), q(4), 60)],
         dict(reads=10, paired=9, proper_pair=9, read1=4, read2=5, reverse=4), {60: 10}, {4: 10},
         {(e, c): cyc(5, 150, 5) for e in range(2) for c in range(4)}, {30: (40, 0)}, {0: 160, 1: 40}, [16, 16, 8, 0],
         dict(measured=10, counted=10, pairs=3, groups_refused=1), insert={(0, 34): 1, (1, 44): 1, (2, 44): 1}),
    # depth 2 over [12, 16), 1 over [16, 18) and [195, 200).  [10, 14): 2 + 2; [14, 20): 2 + 2 + 1 + 1; [190, 260) ends at 200
    Case("touching targets, and a target clipped at the chromosome end",
         [(1, 0, 12, [(M, 6)], seq(12, 6), q(6), 60), (2, 0, 12, M4, seq(12, 4), q(4), 60), (3, 0, 195, [(M, 5)], seq(195, 5), q(5), 60)],
         dict(reads=3), {60: 3}, {6: 1, 4: 1, 5: 1},
         {(0, 0): cyc(3, 90, 3), (0, 1): cyc(3, 90, 3), (0, 2): cyc(3, 90, 3), (0, 3): cyc(3, 90, 3), (0, 4): cyc(2, 60, 2),
          (0, 5): cyc(1, 30, 1)}, {30: (15, 0)}, {0: 189, 1: 7, 2: 4}, [10, 0, 0, 5], dict(measured=3, counted=3),
         targets=[(10, 14), (14, 20), (190, 260)], target_hist={0: 9, 1: 7, 2: 4}, target_sum=[4, 6, 5], target_covered=[2, 4, 5]),
    Case("an empty read set", [], {}, {}, {}, {}, {}, {0: 200}, [0, 0, 0, 0], {}),
]


# ---- the edge stress: one 6 kb chromosome ---------------------------------------------------------------------------------------
LENGTH = 6000
TILE = 1024
SPAN = 1000                                        # max_span of the run in several spans: no multiple of the tile
STRESS_TARGETS = [(1000, 1030), (1030, 1100), (1990, 2010), (2040, 2060), (3050, 3080), (5900, 6100)]


def stress(seed: int = 11):
    """-> (reference, rows sorted by position): what tests/test_gpu_qc.py's edge stress asserts really occurs."""
    rng = np.random.default_rng(seed)
    reference = "".join(rng.choice(list("ACGT"), size=LENGTH))
    reference = _replace(reference, 2500, "N" * 40)
    reference = _replace(reference, 4000, reference[4000:4100].lower())
    rows: List[tuple] = []

    def add(name, flag, pos, cigar, mapq=60, quals=None, mismatch_every=0):
        n = sum(k for op, k in cigar if op in (M, I, S))
        bases, p = [], pos
        for op, k in cigar:
            if op == M:
                bases.append(reference[p:p + k].upper())
                p += k
            elif op in (I, S):
                bases.append("T" * k)
            elif op in (D, N):
                p += k
        text = list("".join(bases))
        for i in range(mismatch_every, len(text), mismatch_every) if mismatch_every else ():
            text[i] = "ACGT"[("ACGT".index(text[i]) + 1) % 4] if text[i] in "ACGT" else text[i]
        rows.append((name, flag, pos, cigar, "".join(text), quals if quals is not None else [int(x) for x in rng.integers(2, 42, size=n)], mapq))
    name = 1
    for pos in range(20, LENGTH - 160, 37):                               # background: 150-base reads, every third reverse
        add(name, REV if name % 3 == 0 else 0, pos, [(M, 150)], mismatch_every=17 if name % 2 else 0)
        name += 1
    for edge in (TILE, 2 * TILE, 3 * TILE, 5 * TILE, SPAN, 2 * SPAN, 3 * SPAN):     # a read and a deletion across every edge
        add(name, 0, edge - 70, [(M, 60), (D, 20), (M, 60)])
        add(name + 1, REV, edge - 5, [(S, 4), (M, 30), (I, 2), (M, 30)])
        name += 2
    add(name, 0, 300, [(M, 700)])                                          # cycles past 512, forward and reverse
    add(name + 1, REV, 1400, [(M, 700)], mismatch_every=13)
    add(name + 2, 0, 3100, [(M, 1500)])                                    # the global LENGTH path
    name += 3
    for _ in range(1100):                                                  # the last depth bin
        rows.append((name, 0, 4500, [(M, 20)], reference[4500:4520].upper(), q(20, 37), 60))
        name += 1
    rows.append((name, F1, 200, [(M, 100)], reference[200:300], q(100, 33), 60))             # a pair 5 000 apart: the last insert bin
    rows.append((name, R2, 5100, [(M, 100)], reference[5100:5200], q(100, 33), 60))
    name += 1
    add(name, 0, 5300, [(M, 64)], quals=q(64, 25))                         # a wave's worth of one quality
    add(name + 1, 0, 5400, [(M, 64)], quals=list(range(2, 66)), mismatch_every=5)     # and of 64 different ones
    rows.sort(key=lambda row: row[2])
    return reference, rows
