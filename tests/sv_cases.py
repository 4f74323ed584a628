"""Inputs of the tests of the large deletions and insertions (tests/test_sv.py on the CPU, tests/test_gpu_sv.py on the GPU): cases
worked by hand, one per rule of DESIGN.md section 7p, and the edge stress on one chromosome of 2 600 positions.

A row is (name_hash, flag, position, CIGAR, bases, qualities, mapq, hp) -- the format of tests/qc_cases.py with the haplotype behind
it.  The hand cases run with min_size 5, flank 3, cluster_gap 10, len_ratio 70 % and min_support 2 on references of their own, short
enough to follow every comparison of the move to the left with a finger; their expected signatures and candidates were worked out
from the rules, not from the code."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from hello_amd import sv
from hello_amd.bam import Reads
from tests.gvcf_cases import D, H, I, M, N, S, reads_of
from tests.qc_cases import overlapping  # noqa: F401  (the tests take it from here)

REV = 0x10
DEL, INS = sv.DEL, sv.INS


def q(n: int, value: int = 30) -> List[int]:
    return [value] * n


def read_set(rows) -> Reads:
    """Rows -> the arrays ``hello_bam_fetch`` would give, the haplotypes in ``hp``."""
    made = [(pos, cigar, bases, quals, flag, mapq) for _, flag, pos, cigar, bases, quals, mapq, _ in rows]
    return dataclasses.replace(reads_of(made), name_hash=np.array([row[0] for row in rows], np.uint64),
                               hp=np.array([row[7] for row in rows], np.uint8))


def realize(reference: str, pos: int, cigar, inserted: Dict[int, str] = None, fill: str = "A") -> str:
    """The bases of a read that follows the reference: M takes its bases (``fill`` past its end), I and S take ``inserted[operation
    index]`` (default: ``fill``)."""
    out, p = [], pos
    for k, (op, n) in enumerate(cigar):
        if op in (M, 7, 8):
            out.append((reference[p:p + n] + fill * n)[:n])
        elif op in (I, S):
            out.append((inserted or {}).get(k, fill * n))
            assert len(out[-1]) == n
        if op in (M, D, N, 7, 8):
            p += n
    return "".join(out)


def row(name: int, reference: str, pos: int, cigar, flag: int = 0, mapq: int = 60, hp: int = 0, inserted: Dict[int, str] = None) -> tuple:
    bases = realize(reference, pos, cigar, inserted)
    return (name, flag, pos, list(cigar), bases, q(len(bases)), mapq, hp)


# ---- the hand cases --------------------------------------------------------------------------------------------------------------
HAND = dict(min_size=5, flank=3, mapq_threshold=10, cluster_gap=10, len_ratio_percent=70, min_support=2)


@dataclass
class Case:
    name: str
    reference: str
    rows: List[tuple]
    signatures: List[Tuple[int, ...]]                # rows of sv.SIGNATURE_COLUMNS, sorted
    candidates: List[Tuple[int, ...]]                # rows of sv.CANDIDATE_COLUMNS, sorted
    counts: Dict[str, int]                           # of sv.METRIC_STATS, what is not 0 (belonging is filled in)
    status: List[int] = field(default_factory=list)

    def cut(self) -> int:
        """Where the two-span run cuts the chromosome: through the first read, two bases behind its start."""
        return self.rows[0][2] + 2

    def want_counts(self) -> Dict[str, int]:
        return dict(dict.fromkeys(sv.METRIC_STATS, 0), belonging=len(self.rows), signatures=len(self.signatures),
                    candidates=len(self.candidates), **self.counts)


#            0         1         2
#            0123456789012345678901234
UNIQUE =    "TCAGACCCCCGGGGGTTTTTCAGAT"        # deleting GGGGG (10 .. 14): the base before it is C, the last deleted one is G
TANDEM =    "TCAGTCCGTACCGTAGTTCAGATCA"        # CCGTA at 5 and at 10, T before them: the second copy moves left by five and stops
INSERTED =  "TCAGACCCCCTTTTTCAGATCAGAT"        # GGGGG inserted at 10 moves nowhere
#            TCAGT ACACACAC GTTCAGATCAGA: ACACAC inserted at 13 moves over itself (six) and two bases of the reference's own repeat
WRAPPED =   "TCAGTACACACACGTTCAGATCAGA"

_DEL8 = [(M, 8), (D, 5), (M, 8)]
# three reads with the deletion (one reverse; haplotypes 1, 2 and none) and two that span it without: five reads cover 5 .. 20, so
# DP 5, DV 3, DR 2.  log10 L = 3 log10 .05 + 2 log10 .95 = -3.94764, 5 log10 .5 = -1.50515, 3 log10 .95 + 2 log10 .05 = -2.66889:
# 0/1, PL round(24.42) = 24, 0, round(11.64) = 12, GQ 12
_GENOTYPED = [row(1, UNIQUE, 2, _DEL8, hp=1), row(2, UNIQUE, 2, _DEL8, REV, hp=2), row(3, UNIQUE, 2, _DEL8),
              row(4, UNIQUE, 2, [(M, 21)]), row(5, UNIQUE, 2, [(M, 21)], REV)]

HAND_TABLE: List[Case] = [
    Case("a deletion in unique sequence does not move", UNIQUE, [row(1, UNIQUE, 2, _DEL8)],
         [(DEL, 10, 5, 0, 0, 1, 0, 0)], [], dict(counting=1, walked=1, reads_with_a_signature=1), [3]),
    # j = 0 .. 4 compare the first copy with the second; j = 5 compares T at 4 with A at 9.  The read at 7 has three bases before the
    # deletion: it may move by three.  The read at 8 has two, fewer than the flank
    Case("a deletion of the second copy moves to the first, or to the read's start", TANDEM,
         [row(1, TANDEM, 2, _DEL8), row(2, TANDEM, 7, [(M, 3), (D, 5), (M, 8)], REV, hp=2), row(3, TANDEM, 8, [(M, 2), (D, 5), (M, 8)])],
         [(DEL, 5, 5, 5, 0, 1, 0, 0), (DEL, 7, 5, 3, 1, 1, 1, 2)],
         [(DEL, 5, 5, 2, 1, 1, 1, 0, 1, 5, 7, 5, 5, 1, 0, 2, 6, 26, 6, 0)],
         dict(counting=3, walked=3, reads_with_a_signature=2), [3, 3, 2]),
    Case("an insertion that matches nothing does not move; lower case in the read folds", INSERTED,
         [row(1, INSERTED, 2, [(M, 8), (I, 5), (M, 8)], inserted={1: "GGGGG"}),
          row(2, INSERTED, 2, [(M, 8), (I, 5), (M, 8)], inserted={1: "ggggc"})],       # c against C at 9, then g against C at 8
         [(INS, 9, 5, 1, 1, 1, 0, 0), (INS, 10, 5, 0, 0, 1, 0, 0)],
         [(INS, 9, 5, 2, 2, 0, 2, 0, 0, 9, 10, 5, 5, 2, 0, 2, 6, 26, 6, 0)],
         dict(counting=2, walked=2, reads_with_a_signature=2), [3, 3]),
    # j = 0 .. 5: C A C A C A at 12 .. 7 against the inserted bases from their end; j = 6, 7: C A at 6, 5 against C A at 12, 11;
    # j = 8: T at 4 against C at 10
    Case("an insertion moves over itself into the reference's own repeat", WRAPPED,
         [row(1, WRAPPED, 2, [(M, 11), (I, 6), (M, 8)], inserted={1: "ACACAC"})],
         [(INS, 5, 6, 8, 0, 1, 0, 0)], [], dict(counting=1, walked=1, reads_with_a_signature=1), [3]),
    Case("three reads with a deletion and two without", UNIQUE, _GENOTYPED,
         [(DEL, 10, 5, 0, 0, 1, 0, 1), (DEL, 10, 5, 0, 1, 1, 1, 2), (DEL, 10, 5, 0, 2, 1, 0, 0)],
         [(DEL, 10, 5, 3, 2, 1, 1, 1, 1, 10, 10, 5, 5, 5, 2, 1, 12, 24, 0, 12)],
         dict(counting=5, walked=3, reads_with_a_signature=3), [3, 3, 3, 1, 1]),
    # four bases, under min_size; N of five; the flank missed by one on either side; a leading and a trailing operation; and reads
    # that do not count: mapq 9, a duplicate
    Case("what is no signature", UNIQUE,
         [row(1, UNIQUE, 2, [(M, 8), (D, 4), (M, 8)]), row(2, UNIQUE, 2, [(M, 8), (N, 5), (M, 8)]),
          row(3, UNIQUE, 2, [(M, 2), (D, 5), (M, 8)]), row(4, UNIQUE, 2, [(M, 8), (D, 5), (M, 2)]),
          row(5, UNIQUE, 2, [(D, 5), (M, 8)]), row(6, UNIQUE, 2, [(M, 8), (I, 5)]), row(7, UNIQUE, 2, _DEL8, mapq=9),
          row(8, UNIQUE, 2, _DEL8, 0x400)],
         [], [], dict(counting=6, walked=4), [1, 1, 2, 2, 2, 2, 0, 0]),
]
GENOTYPED_VCF = ("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=25>\n" + sv.VCF_HEADER
                 + "chr1\t10\t.\tC\t<DEL>\t.\tPASS\tSVTYPE=DEL;SVLEN=-5;END=15;SUPPORT=3;CIPOS=0,0;CILEN=0,0;STRANDS=2,1\t"
                   "GT:GQ:DR:DV:PL:HPS\t0/1:12:2:3:24,0,12:1,1,1\n")

# clusters worked by hand, at cluster_gap 10, len_ratio 70 % and min_support 2: (signatures, candidates' cluster columns)
CLUSTER_TABLE = [
    ("a gap of exactly cluster_gap joins, one more parts",
     [(DEL, 100, 20, 0, 0, 1, 0, 0), (DEL, 110, 20, 0, 1, 1, 1, 1), (DEL, 121, 20, 0, 2, 1, 0, 0), (DEL, 121, 20, 0, 3, 1, 0, 2)],
     [(DEL, 100, 20, 2, 1, 1, 1, 1, 0, 100, 110, 20, 20), (DEL, 121, 20, 2, 2, 0, 1, 0, 1, 121, 121, 20, 20)]),
    ("a ratio exactly at the threshold joins (100 x 14 = 70 x 20), just under parts (100 x 20 < 70 x 29)",
     [(INS, 50, 14, 0, 0, 1, 0, 0), (INS, 50, 20, 0, 1, 1, 0, 0), (INS, 50, 29, 0, 2, 1, 0, 0), (INS, 50, 29, 0, 3, 1, 0, 0)],
     [(INS, 50, 14, 2, 2, 0, 2, 0, 0, 50, 50, 14, 20), (INS, 50, 29, 2, 2, 0, 2, 0, 0, 50, 50, 29, 29)]),
    ("one read twice in a group counts once; its group of one read is no candidate",
     [(DEL, 10, 8, 0, 7, 1, 1, 2), (DEL, 15, 8, 0, 7, 3, 1, 2)], []),
    ("a deletion and an insertion at one position; the lower medians of three",
     [(INS, 30, 9, 0, 0, 1, 0, 1), (INS, 30, 9, 0, 1, 1, 0, 1), (DEL, 30, 9, 0, 0, 3, 0, 1), (DEL, 31, 10, 0, 1, 3, 0, 1),
      (DEL, 29, 11, 0, 2, 1, 1, 3)],
     [(DEL, 30, 10, 3, 2, 1, 1, 2, 0, 29, 31, 9, 11), (INS, 30, 9, 2, 2, 0, 0, 2, 0, 30, 30, 9, 9)]),
]


# ---- the edge stress: one chromosome of 2 600 positions -----------------------------------------------------------------------------
LENGTH = 2600
SPAN = 700                                         # the cut spans: no divisor of the tile of 1 024
STRESS = dict(min_size=10, flank=5, mapq_threshold=10, cluster_gap=20, len_ratio_percent=70, min_support=2)
SHIFTS = (0, 63, 64, 65)
SHIFT_AT = {0: 200, 63: 330, 64: 470, 65: 610}     # where the deletion of each shift begins
LONG_AT, LONG_SPECIAL = 30, {63: (D, 12), 64: (I, 11), 127: (I, 10), 128: (D, 13)}
STOPPED_AT, WRAP_AT, N_AT = 760, 860, 960          # a move the reads' start stops; an insertion that wraps; an N in the repeat
TILE_EDGE = (1023, 1024, 1025)
GAP_AT, GAP_MORE_AT, RATIO_AT, RATIO_UNDER_AT, TWICE_AT, BOTH_AT = 1200, 1300, 1400, 1500, 1600, 1700
FLANK_AT, CLIP_AT, SHORT_AT = 1800, 1950, 2100


def _other(base: str) -> str:
    return "ACGT"[("ACGT".index(base.upper()) + 1) % 4] if base.upper() in "ACGT" else "A"


def stress(seed: int = 29):
    """-> (reference, rows sorted by position, named): ``named[situation]`` are the name hashes of the rows that stage it."""
    rng = np.random.default_rng(seed)
    ref = list("".join(rng.choice(list("ACGT"), size=LENGTH)))
    rows: List[tuple] = []
    named: Dict[str, List[int]] = {}
    pending = []                                   # the rows are realized once the reference is final

    def add(situation: str, pos: int, cigar, flag: int = 0, mapq: int = 60, hp: int = 0, inserted=None):
        name = len(pending) + 1
        pending.append((name, pos, list(cigar), flag, mapq, hp, inserted))
        named.setdefault(situation, []).append(name)
        return name

    def periodic(start: int, stop: int, unit: str):
        """[start, stop) holds ``unit`` with its period; the base before it breaks the period."""
        for p in range(start, stop):
            ref[p] = unit[p % len(unit)]
        ref[start - 1] = _other(unit[(start - 1) % len(unit)])

    def unmoved(p: int, n: int):
        """A deletion of n bases at p moves nowhere."""
        ref[p - 1] = _other(ref[p - 1 + n])

    # a read of 130 operations with signatures at operations 63, 64, 127 and 128
    cigar = [LONG_SPECIAL[i] if i in LONG_SPECIAL else (M, 20) if i in (65, 129) else (M, 3) if i % 2 == 0 else ((I, 1), (D, 1))[i // 2 % 2]
             for i in range(130)]
    add("long", LONG_AT, cigar, hp=1)
    # shifts of 0, 63, 64 and 65: a deletion of 12 at the end of a stretch of period 12 that is k + 12 long
    unit = "GATTCAGCCTAC"
    for k in SHIFTS:
        p = SHIFT_AT[k]
        periodic(p - k, p + 12, unit)
        add("shift%d" % k, p - k - 10, [(M, k + 10), (D, 12), (M, 20)], REV * (k % 2))
    # the read's start stops the move: 40 bases before a deletion inside a stretch that would let it move by 65
    periodic(STOPPED_AT - 65, STOPPED_AT + 12, unit)
    add("stopped", STOPPED_AT - 40, [(M, 40), (D, 12), (M, 20)])
    add("stopped", STOPPED_AT - 40, [(M, 40), (D, 12), (M, 21)], REV)
    # an insertion of 10 that continues a stretch of period 10 and 25 long: it moves by 25, over itself and on; the stretch is
    # partly lower case, and so are the inserted bases
    unit10 = "ACCGTTGACA"
    periodic(WRAP_AT - 25, WRAP_AT, unit10)
    ref[WRAP_AT] = _other(unit10[WRAP_AT % 10])
    for p in range(WRAP_AT - 25, WRAP_AT, 2):
        ref[p] = ref[p].lower()
    add("wrap", WRAP_AT - 35, [(M, 35), (I, 10), (M, 20)], inserted={1: "".join(unit10[(WRAP_AT + i) % 10] for i in range(10)).lower()})
    # an N in the repeat: the stretch of period 12 holds an N and an n, and the deletion moves across both
    unit_n = "GATNCAGCCTAC"
    periodic(N_AT - 30, N_AT + 12, unit_n)
    ref[N_AT - 9] = "n"
    assert unit_n[(N_AT - 9) % 12] == "N"
    add("n_in_repeat", N_AT - 40, [(M, 40), (D, 12), (M, 20)])
    # candidates at 1 023, 1 024 and 1 025 (lengths 12, 12 and 40, so that nothing joins them) and at length - 1, two reads each;
    # beside them reads without an event whose cover begins or ends exactly there, or one off
    unmoved(1025, 40)
    unmoved(1023, 12)
    for name, p, op, n in (("tile1023", 1023, D, 12), ("tile1024", 1024, I, 12), ("tile1025", 1025, D, 40)):
        for k in range(2):
            add(name, p - 30 - k, [(M, 30 + k), (op, n), (M, 25)], REV * k, hp=1 + k,
                inserted={1: "C" * 11 + _other(ref[1023])} if op == I else None)
    for k in range(2):                             # 20M 12I 6M at length - 21: the insertion begins at length - 1, the read ends past it
        add("last", LENGTH - 21 - k, [(M, 20 + k), (I, 12), (M, 6)], inserted={1: "G" * 11 + _other(ref[LENGTH - 2])})
    for s_plus, e_minus in ((1023, 1100), (1024, 1100), (900, 1025), (900, 1024)):
        add("cover_edge", s_plus - 5, [(M, e_minus + 5 - (s_plus - 5))])
    # a deletion that ends exactly at length (the read runs six bases past it: the clamp of the cover), and one that ends past it
    add("ends_at_length", LENGTH - 30, [(M, 18), (D, 12), (M, 6)])
    add("ends_past_length", LENGTH - 29, [(M, 18), (D, 12), (M, 6)])
    # a gap of exactly cluster_gap, and of one more; a ratio exactly at the threshold, and just under: two reads per signature
    for name, at, second, n1, n2 in (("gap", GAP_AT, 20, 12, 12), ("gap_more", GAP_MORE_AT, 21, 12, 12),
                                     ("ratio", RATIO_AT, 0, 14, 20), ("ratio_under", RATIO_UNDER_AT, 0, 20, 29)):
        unmoved(at, n1)
        if second:
            unmoved(at + second, n2)
        elif ref[at - 1 + n2].upper() == ref[at - 1].upper():
            ref[at - 1 + n2] = _other(ref[at - 1])                  # the longer deletion at the same place moves nowhere either
        for k in range(2):
            add(name, at - 40 - k, [(M, 40 + k), (D, n1), (M, 60)], REV * k)
            add(name, at + second - 40 - k, [(M, 40 + k), (D, n2), (M, 60)], hp=2)
    # one read with two deletions of one group, and one other read with the first: two reads, three signatures
    unmoved(TWICE_AT, 12)
    unmoved(TWICE_AT + 20, 12)
    add("twice", TWICE_AT - 30, [(M, 30), (D, 12), (M, 8), (D, 12), (M, 30)], hp=1)
    add("twice", TWICE_AT - 25, [(M, 25), (D, 12), (M, 30)], REV)
    # a deletion and an insertion at one position, two reads each
    unmoved(BOTH_AT, 12)
    for k in range(2):
        add("both", BOTH_AT - 30 - k, [(M, 30 + k), (D, 12), (M, 30)])
        add("both", BOTH_AT - 33 - k, [(M, 33 + k), (I, 12), (M, 30)], REV, inserted={1: "T" * 11 + _other(ref[BOTH_AT - 1])})
    # the flank met exactly and missed by one, on each side; a leading and a trailing operation of either kind
    add("flank_met", FLANK_AT, [(M, 5), (D, 12), (M, 30)])
    add("flank_missed", FLANK_AT + 1, [(M, 4), (D, 12), (M, 30)])
    add("flank_met", FLANK_AT + 2, [(M, 30), (I, 12), (M, 5)])
    add("flank_missed", FLANK_AT + 3, [(M, 30), (I, 12), (M, 4)])
    for cigar in ([(I, 12), (M, 30)], [(D, 12), (M, 30)], [(M, 30), (I, 12)], [(M, 30), (D, 12)]):
        add("outermost", FLANK_AT + 60, cigar)
    # straight after H and S: as the first aligned operation it is a leading one; behind eight aligned bases it is operation 3
    add("outermost", CLIP_AT, [(H, 2), (S, 3), (D, 12), (M, 30)])
    add("after_clips", CLIP_AT + 1, [(H, 2), (S, 3), (M, 8), (D, 12), (M, 30)])
    # shorter than two flanks, and exactly two flanks long
    add("short", SHORT_AT, [(M, 9)])
    add("two_flanks", SHORT_AT + 20, [(M, 10)])
    # reads that do not count carry events too
    add("not_counting", GAP_AT - 40, [(M, 40), (D, 12), (M, 60)], mapq=5)
    add("not_counting", GAP_AT - 40, [(M, 40), (D, 12), (M, 60)], 0x400)
    # plain reads over everything but 450 .. 950, so that the depths are not all alike
    for s in range(0, LENGTH - 150, 37):
        if not 450 <= s < 800:
            add("plain", s, [(M, 150)], REV * (s % 2))

    reference = "".join(ref)
    for name, pos, cigar, flag, mapq, hp, inserted in pending:
        rows.append(row(name, reference, pos, cigar, flag, mapq, hp, inserted))
    rows.sort(key=lambda r: r[2])
    return reference, rows, named
