"""Inputs of the duplicate-marking tests (tests/test_markdup.py on the CPU, tests/test_gpu_markdup.py on the GPU): tables worked by
hand, one case per rule of DESIGN.md section 7j, the key-table stress and the 6 kb chromosome.

A hand row is (name_hash, flag, position, CIGAR, qualities); every base is ``A``.  ``M10`` at quality 30 scores 300.  A forward
read at position p has e = 2 p; a reverse read over [p, p + 10) has end5 = p + 9 and e = 2 (p + 9) + 1, so the second mate at 300
has e = 619.  Expected values were worked out from the rules, not from the code."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

from hello_amd.bam import Reads
from tests.bam_writer import Read
from tests.gvcf_cases import D, H, I, M, S, reads_of

REV = 0x10
F1, R2 = 0x63, 0x93            # a pair in the usual orientation: first mate forward, second mate reverse
R1, F2 = 0x53, 0xA3            # the other way round: first mate reverse, second mate forward
M10 = [(M, 10)]


def q(n: int = 10, value: int = 30) -> List[int]:
    return [value] * n


def read_set(rows: Sequence[tuple]) -> Reads:
    """Rows -> the arrays ``hello_bam_fetch`` would give."""
    made = []
    for _, flag, pos, cigar, quals in rows:
        n = sum(k for op, k in cigar if op in (M, I, S))
        assert len(quals) == n
        made.append((pos, cigar, "A" * n, quals, flag, 60))
    return dataclasses.replace(reads_of(made), name_hash=np.array([row[0] for row in rows], np.uint64))


@dataclass
class Case:
    name: str
    rows: List[tuple]
    e: List[int]
    score: List[int]
    mate: List[int]
    kind: List[int]              # 0 not eligible, 1 pair, 2 single, 3 unresolved
    duplicate: List[int]
    counts: Tuple[int, ...]      # eligible, pairs, singles, unresolved, groups_refused, duplicate_pairs, duplicate_singles

    def reads(self) -> Reads:
        return read_set(self.rows)

    def want_counts(self) -> dict:
        names = ("eligible", "pairs", "singles", "unresolved", "groups_refused", "duplicate_pairs", "duplicate_singles")
        return dict(zip(names, self.counts), reads=len(self.rows))


def _pair(name, at=100, mate_at=300, quality=30):
    return [(name, F1, at, M10, q(10, quality)), (name, R2, mate_at, M10, q(10, quality))]


HAND_TABLE: List[Case] = [
    # 3S7M at 100: the fragment began at 97, where the unclipped copy starts
    Case("a forward read with S", [(1, 0, 100, [(S, 3), (M, 7)], q()), (2, 0, 97, M10, q())],
         [194, 194], [300, 300], [-1, -1], [2, 2], [0, 1], (2, 0, 2, 0, 0, 0, 1)),
    # 2H3S7M: both clips count, the hard clip has no bases (10 qualities)
    Case("a forward read with H then S", [(1, 0, 100, [(H, 2), (S, 3), (M, 7)], q()), (2, 0, 95, M10, q())],
         [190, 190], [300, 300], [-1, -1], [2, 2], [0, 1], (2, 0, 2, 0, 0, 0, 1)),
    # 7M3S at 100: ref_end 107, end5 = 106 + 3 = 109, as 10M at 100 (ref_end 110)
    Case("a reverse read with a trailing S", [(1, REV, 100, [(M, 7), (S, 3)], q()), (2, REV, 100, M10, q())],
         [219, 219], [300, 300], [-1, -1], [2, 2], [0, 1], (2, 0, 2, 0, 0, 0, 1)),
    # 7M2D3S at 100: the D is reference (ref_end 109) and ends the run: end5 = 108 + 3 = 111, as 10M at 102; 7M3S is 109
    Case("a reverse read with a trailing D ... S",
         [(1, REV, 100, [(M, 7), (D, 2), (S, 3)], q()), (2, REV, 102, M10, q()), (3, REV, 100, [(M, 7), (S, 3)], q())],
         [223, 223, 219], [300, 300, 300], [-1, -1, -1], [2, 2, 2], [0, 1, 0], (3, 0, 3, 0, 0, 0, 1)),
    Case("qualities 14 and 15 on either side of the threshold",
         [(1, 0, 100, M10, q(10, 14)), (2, 0, 100, M10, q(5, 14) + q(5, 15)), (3, 0, 100, M10, q(4, 15) + q(6, 14))],
         [200, 200, 200], [0, 75, 60], [-1, -1, -1], [2, 2, 2], [1, 0, 1], (3, 0, 3, 0, 0, 0, 2)),
    Case("two pairs with one key and different scores",
         [_pair(10)[0], _pair(11, quality=20)[0], _pair(10)[1], _pair(11, quality=20)[1]],
         [200, 200, 619, 619], [300, 200, 300, 200], [2, 3, 0, 1], [1, 1, 1, 1], [0, 1, 0, 1], (4, 2, 0, 0, 0, 1, 0)),
    # pair 11 holds read 0, pair 10 begins at read 1: equal scores, the pair with the smaller smaller index survives
    Case("a score tie resolved by index", [_pair(11)[1], _pair(10)[0], _pair(10)[1], _pair(11)[0]],
         [619, 200, 619, 200], [300, 300, 300, 300], [3, 2, 1, 0], [1, 1, 1, 1], [0, 1, 1, 0], (4, 2, 0, 0, 0, 1, 0)),
    Case("three pairs with one key",
         [_pair(10)[0], _pair(11, quality=40)[0], _pair(12, quality=35)[0], _pair(10)[1], _pair(11, quality=40)[1],
          _pair(12, quality=35)[1]],
         [200, 200, 200, 619, 619, 619], [300, 400, 350, 300, 400, 350], [3, 4, 5, 0, 1, 2], [1] * 6, [1, 0, 1, 1, 0, 1],
         (6, 3, 0, 0, 0, 2, 0)),
    # the first mate of pair 11 is a REVERSE read over [91, 101): end5 100 as pair 10's forward mate, but e = 201
    Case("pairs with equal end5 but different strands", _pair(10) + [(11, R1, 91, M10, q()), (11, R2, 300, M10, q())],
         [200, 619, 201, 619], [300] * 4, [1, 0, 3, 2], [1] * 4, [0, 0, 0, 0], (4, 2, 0, 0, 0, 0, 0)),
    # pair 11 reaches (200, 619) with its SECOND mate forward at 100 and its first mate reverse at 300
    Case("the same two ends with first and second mate swapped", _pair(10) + [(11, F2, 100, M10, q()), (11, R1, 300, M10, q())],
         [200, 619, 200, 619], [300] * 4, [1, 0, 3, 2], [1] * 4, [0, 0, 1, 1], (4, 2, 0, 0, 0, 1, 0)),
    # an unpaired read at 100 and a read whose mate is unmapped (0x1 | 0x8) at the reverse end: both duplicates, whatever they
    # score; the unpaired read at 150 is the only one of its key
    Case("a single at a pair's end",
         _pair(10, quality=20) + [(20, 0, 100, M10, q(10, 40)), (21, 0x59, 300, M10, q(10, 40)), (22, 0, 150, M10, q())],
         [200, 619, 200, 619, 300], [200, 200, 400, 400, 300], [1, 0, -1, -1, -1], [1, 1, 2, 2, 2], [0, 0, 1, 1, 0],
         (5, 1, 3, 0, 0, 0, 2)),
    Case("a single at a pair's end5 but the other strand", _pair(10) + [(20, REV, 91, M10, q())],
         [200, 619, 201], [300] * 3, [1, 0, -1], [1, 1, 2], [0, 0, 0], (3, 1, 1, 0, 0, 0, 0)),
    # quality 10 is below 15: score 0, and the only read of its key survives with it
    Case("singles among themselves",
         [(1, 0, 100, M10, q(10, 20)), (2, 0, 100, M10, q()), (3, 0, 100, M10, q()), (4, 0, 200, M10, q(10, 10))],
         [200, 200, 200, 400], [200, 300, 300, 0], [-1] * 4, [2] * 4, [1, 0, 1, 0], (4, 0, 4, 0, 0, 0, 2)),
    # three reads of one name are unresolved; pair 11 has their ends and a lower score and is no duplicate, nor are they
    Case("a group of three names", [(10, F1, 100, M10, q()), (10, R2, 300, M10, q()), (10, R2, 300, M10, q())] + _pair(11, quality=20),
         [200, 619, 619, 200, 619], [300, 300, 300, 200, 200], [-1, -1, -1, 4, 3], [3, 3, 3, 1, 1], [0] * 5, (5, 1, 0, 3, 1, 0, 0)),
    # read 0 is unresolved and shields nothing: the singles at its end decide among themselves
    Case("a paired read whose mate is absent", [(10, F1, 100, M10, q()), (20, 0, 100, M10, q(10, 20)), (21, 0, 100, M10, q(10, 25))],
         [200, 200, 200], [300, 200, 250], [-1] * 3, [3, 2, 2], [0, 1, 0], (3, 0, 2, 1, 0, 0, 1)),
    Case("an input 0x400, an unmapped, a secondary and a supplementary read",
         [(1, 0x400, 100, M10, q()), (2, 0x4, 100, M10, q()), (3, 0x100, 100, M10, q()), (4, 0x800, 100, M10, q()), (5, 0, 100, M10, q())],
         [0, 0, 0, 0, 200], [0, 0, 0, 0, 300], [-1] * 5, [0, 0, 0, 0, 2], [0] * 5, (1, 0, 1, 0, 0, 0, 0)),
    # 5S5M at 2: end5 = -3, e = -6
    Case("a clip that reaches before the first position", [(1, 0, 2, [(S, 5), (M, 5)], q()), (2, 0, 2, [(S, 5), (M, 5)], q(10, 20))],
         [-6, -6], [300, 200], [-1, -1], [2, 2], [0, 1], (2, 0, 2, 0, 0, 0, 1)),
    Case("an empty read set", [], [], [], [], [], [], (0, 0, 0, 0, 0, 0, 0)),
]


# ---- the key-table stress -----------------------------------------------------------------------------------------------------
def _forward(name, end5, quality):
    return (name, F1, end5, M10, q(10, quality))


def _reverse(name, end5, quality, flag=R2):
    return (name, flag, end5 - 9, M10, q(10, quality))


def stress(key_table_size, key_table_slot):
    """-> (rows in shuffled order, table size, the twelve wrapping ends): 4 096 pairs in 512 pair keys (8 pairs each) and 1 024
    singles, 256 of them on pair ends.  Key k is (lo, hi) = (2 a, 2 b + 1) of a forward mate at a and a reverse mate with end5
    b.  128 keys have forward ends that differ only above bit 40, 128 only in their low 7 bits; 12 keys have a forward end whose
    END entry first probes three slots before the table's end -- twelve entries on three slots, so the probe wraps; the rest are
    random."""
    rng = np.random.default_rng(23)
    inserts = 3 * 4096 + 1024
    size = key_table_size(inserts)
    tried = rng.integers(1000, 2 ** 40, size=2_000_000, dtype=np.int64)
    wrapping = tried[key_table_slot(2 * tried, 0, 0, size) == size - 3][:12]
    assert wrapping.shape[0] == 12
    starts = [(i << 40) + 5000 for i in range(1, 129)] + [(1 << 33) + i for i in range(128)] + wrapping.tolist()
    starts += rng.integers(10 ** 6, 2 ** 38, size=512 - len(starts), dtype=np.int64).tolist()
    assert len(set(starts)) == 512
    rows, name = [], 1
    for a in starts:
        b = a + 400
        for _ in range(8):
            quality = int(rng.integers(15, 41))
            rows += [_forward(name, a, quality), _reverse(name, b, quality)]
            name += 1
    for k in range(1024):
        a = starts[2 * k] if k < 256 else 2 ** 41 + (k % 96)                # the other 768 share 96 keys among themselves
        rows.append((name, 0, a, M10, q(10, int(rng.integers(15, 41)))))
        name += 1
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return rows, size, wrapping


# ---- the 6 kb chromosome --------------------------------------------------------------------------------------------------------
LENGTH = 6000
SITES = list(range(100, LENGTH - 100, 200))              # heterozygous SNVs: the ALT allele is on haplotype 1


def _other(base: str) -> str:
    return "ACGT"[("ACGT".index(base) + 1) % 4]


def chromosome(seed: int = 7):
    """-> (reference, reads sorted by position): about 30x of 150-base pairs 300 - 600 bp from end to end, half of them with the
    first mate on the reverse strand; about 15 % of the fragments have 2 - 5 copies of other qualities, some with a soft clip at
    the 5' end of either mate (the same fragment end) or at a 3' end (which does not matter); 40 single-end reads, eight of them
    on a pair's forward end and eight copies of other singles; five single-end reads with long CIGARs.  No base differs from
    its haplotype."""
    rng = np.random.default_rng(seed)
    ref = "".join(rng.choice(list("ACGT"), size=LENGTH))
    hap1 = list(ref)
    for p in SITES:
        hap1[p] = _other(ref[p])
    haps = (ref, "".join(hap1))
    reads: List[Read] = []

    def mate(name, which, start, flag, clip5=0, clip3=0):
        """The 150 bases of haplotype ``which`` from ``start``; clip5 / clip3: bases soft-clipped at the read's 5' / 3' end."""
        left, right = (clip3, clip5) if flag & REV else (clip5, clip3)
        cigar = ([(S, left)] if left else []) + [(M, 150 - left - right)] + ([(S, right)] if right else [])
        quals = [int(x) for x in rng.integers(12, 41, size=150)]
        return Read(name, start + left, cigar, haps[which][start:start + 150], quals, flag, 60)

    forward_ends = []
    for j in range(600):
        length = int(rng.integers(300, 601))
        start = int(rng.integers(0, LENGTH - length))
        which = int(rng.integers(2))
        flags = (F1, R2) if j % 2 == 0 else (F2, R1)
        copies = int(rng.integers(2, 6)) if rng.random() < 0.15 else 0
        forward_ends.append(start)
        for c in range(1 + copies):
            name = "f%d" % j if c == 0 else "f%d_c%d" % (j, c)
            clip = [0, 0, 0, 0]                                               # 5' and 3' of the left mate, 5' and 3' of the right
            if c and rng.random() < 0.4:
                clip[int(rng.integers(4))] = int(rng.integers(1, 9))
            reads.append(mate(name, which, start, flags[0], clip[0], clip[1]))
            reads.append(mate(name, which, start + length - 150, flags[1], clip[2], clip[3]))
    singles = []
    for j in range(40):
        if j < 8:
            start, flag = forward_ends[j * 7], 0                              # on a pair's forward end
        elif j < 16:
            start, flag = singles[j - 8]                                      # a copy of another single
        else:
            start, flag = int(rng.integers(0, LENGTH - 150)), REV * int(rng.integers(2))
        singles.append((start, flag))
        reads.append(mate("s%d" % j, int(rng.integers(2)), start, flag))
    for j in range(5):
        start = int(rng.integers(0, LENGTH - 200))
        seq = ref[start - 0:start + 30] + "A" + ref[start + 30:start + 70] + ref[start + 72:start + 122]
        cigar = [(S, 2), (M, 28), (I, 1), (M, 40), (D, 2), (M, 47), (S, 3)]
        reads.append(Read("l%d" % j, start + 2, cigar, seq, [int(x) for x in rng.integers(12, 41, size=len(seq))], REV * (j % 2), 60))
    reads.sort(key=lambda r: r.pos)
    return ref, reads
