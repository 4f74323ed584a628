"""Inputs of the haplotag tests (tests/test_haplotag.py on the CPU, tests/test_gpu_haplotag.py on the GPU), beside
tests/phase_cases.py: the parser table, one line per clause of DESIGN.md section 7h; the reads worked by hand; and the "rounds"
case, one 300-base read over a record every 2 bp, where the cross-lane reduction of the kernel can go wrong.  Every expected value
was worked out by hand from the rule, not taken from the code."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

from hello_amd.haplotag import PhasedRecord
from tests.phase_cases import D, I, M, N, _q  # noqa: F401


def rec(start, ref, hap1, hap2, ps, a=0, b=1):
    return PhasedRecord(start, start + len(ref), a, b, hap1.encode(), hap2.encode(), ps)


def line(pos, ref, alt, fmt, sample, chrom="chr1"):
    return ("%s\t%d\t.\t%s\t%s\t30\t.\tHELLO\t%s\t%s\n" % (chrom, pos, ref, alt, fmt, sample)).encode()


# ---- the parser: (name, line, the record or None, counted as "a|b without PS") ------------------------------------------------
PARSER_TABLE: List[Tuple[str, bytes, Optional[PhasedRecord], bool]] = [
    ("0|1 with PS", line(5, "G", "T", "GT:PS", "0|1:5"), rec(4, "G", "G", "T", 5), False),
    ("0|1 with fields between GT and PS", line(5, "G", "T", "GT:GQ:DP:PS", "0|1:30:12:3"), rec(4, "G", "G", "T", 3), False),
    ("1|0: the alternate allele is haplotype 1", line(5, "G", "T", "GT:PS", "1|0:5"), rec(4, "G", "T", "G", 5, 1, 0), False),
    ("1|2", line(5, "G", "T,C", "GT:PS", "1|2:5"), rec(4, "G", "T", "C", 5, 1, 2), False),
    ("lower-case alleles are upper-cased", line(5, "g", "gtt", "GT:PS", "0|1:5"), rec(4, "G", "G", "GTT", 5), False),
    ("a deletion: the span is that of REF", line(5, "GCA", "G", "GT:PS", "0|1:2"), rec(4, "GCA", "GCA", "G", 2), False),
    ("PS not last in FORMAT", line(5, "G", "T", "GT:PS:GQ", "0|1:7:30"), rec(4, "G", "G", "T", 7), False),
    ("0/1 is not phased", line(5, "G", "T", "GT:PS", "0/1:5"), None, False),
    ("1|1 names one allele", line(5, "G", "T", "GT:PS", "1|1:5"), None, False),
    ("0|2 names an allele the line does not have", line(5, "G", "T", "GT:PS", "0|2:5"), None, False),
    (".|1 is not two integers", line(5, "G", "T", "GT:PS", ".|1:5"), None, False),
    ("0|1 without PS", line(5, "G", "T", "GT", "0|1"), None, True),
    ("0|1 with FORMAT PS but a short sample column", line(5, "G", "T", "GT:GQ:PS", "0|1:30"), None, True),
    ("PS of .", line(5, "G", "T", "GT:PS", "0|1:."), None, True),
    ("PS of 0", line(5, "G", "T", "GT:PS", "0|1:0"), None, True),
    ("a negative PS", line(5, "G", "T", "GT:PS", "0|1:-4"), None, True),
    ("a non-ACGT allele", line(5, "N", "T", "GT:PS", "0|1:5"), None, False),
    ("a symbolic allele", line(5, "G", "<NON_REF>", "GT:PS", "0|1:5"), None, False),
    ("fewer than ten columns", b"chr1\t5\t.\tG\tT\t30\t.\tHELLO\tGT:PS\n", None, False),
    ("an empty line", b"\n", None, False),
]


# ---- reads worked by hand -------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """reads: (pos, cigar, bases, qualities, flag, mapq); want: (hp, ps) per read; why: per read, the cause ``phase.observe_why``
    names for a NONE at the read's FIRST candidate record (only where given)."""
    name: str
    records: List[PhasedRecord]
    reads: List[tuple]
    want: List[Tuple[int, int]]
    why: List[str] = field(default_factory=list)


# sets 3 and 6 interleave: records at 2 (set 3), 5 and 7 (set 6), 9 (set 3)
INTERLEAVED = [rec(2, "A", "A", "C", 3), rec(5, "G", "G", "T", 6), rec(7, "A", "A", "G", 6), rec(9, "A", "A", "T", 3)]
# a SNP at 4 in set 5 and one at 8 in set 9: the set of a read comes from the record at 8 when it shows nothing at 4
LATER = [rec(4, "G", "G", "T", 5), rec(8, "A", "A", "C", 9)]
G_T = rec(4, "G", "G", "T", 5)

READ_TABLE: List[Case] = [
    # the first read shows A at 2 (haplotype 1 of set 3), T at 5 and G at 7 (haplotype 2, but of set 6) and A at 9 (haplotype 1 of
    # set 3): n1 = 2, n2 = 0 from set 3 alone -- counting every set would tie at 2 : 2.  The second read starts at 4: its first
    # observation is at 5, its set is 6, and the record of set 3 at 9 does not count
    Case("interleaved sets", INTERLEAVED,
         [(0, [(M, 12)], "AAAAATAGAAAA", _q(12), 0, 60), (4, [(M, 8)], "ATAGAAAA", _q(8), 0, 60)],
         [(1, 3), (2, 6)]),
    Case("a tie keeps the set and says 0", [rec(2, "A", "A", "C", 3), rec(5, "G", "G", "T", 3)],
         [(0, [(M, 10)], "AAAAATAAAA", _q(10), 0, 60)], [(0, 3)]),
    # C at 4 is neither allele; T at 4 with quality 5; an N over [3, 6).  All three show C at 8: haplotype 2 of set 9
    Case("nothing at the first candidate: neither, quality, N", LATER,
         [(0, [(M, 12)], "ACGTCCATCAAA", _q(12), 0, 60),
          (0, [(M, 12)], "ACGTTCATCAAA", [30, 30, 30, 30, 5] + _q(7), 0, 60),
          (0, [(M, 3), (N, 3), (M, 6)], "ACGATCAAA", _q(9), 0, 60)],
         [(2, 9), (2, 9), (2, 9)], ["neither", "quality", "N"]),
    # REF GCATCAAA -> G spans [4, 12) and the read ends at 12: no aligned base behind the span.  The SNP at 8 lies inside it
    Case("nothing at the first candidate: end", [rec(4, "GCATCAAA", "GCATCAAA", "G", 5), rec(8, "A", "A", "C", 9)],
         [(0, [(M, 12)], "ACGTGCATCAAA", _q(12), 0, 60)], [(2, 9)], ["end"]),
    Case("a 1|0 record: the alternate allele is haplotype 1", [rec(4, "G", "T", "G", 5, 1, 0)],
         [(0, [(M, 8)], "ACGTTCAT", _q(8), 0, 60), (0, [(M, 8)], "ACGTGCAT", _q(8), 0, 60)], [(1, 5), (2, 5)]),
    Case("a 1|2 record: the reference base is neither haplotype", [rec(4, "G", "T", "C", 5, 1, 2)],
         [(0, [(M, 8)], "ACGTTCAT", _q(8), 0, 60), (0, [(M, 8)], "ACGTCCAT", _q(8), 0, 60), (0, [(M, 8)], "ACGTGCAT", _q(8), 0, 60)],
         [(1, 5), (2, 5), (0, 0)]),
    # REF GCA -> G on haplotype 2: the D removes C and A; REF G -> GTT at 12 on haplotype 1: the I joins the base on its left
    Case("indel records", [rec(4, "GCA", "GCA", "G", 5), rec(12, "G", "GTT", "G", 5)],
         [(0, [(M, 5), (D, 2), (M, 3)], "ACGTGTAC", _q(8), 0, 60), (0, [(M, 10)], "ACGTGCATAC", _q(10), 0, 60),
          (8, [(M, 5), (I, 2), (M, 3)], "ACATGTTCAT", _q(10), 0, 60), (8, [(M, 8)], "ACATGCAT", _q(8), 0, 60),
          (0, [(M, 5), (D, 2), (M, 6), (I, 2), (M, 3)], "ACGTGTACATGTTCAT", _q(16), 0, 60)],
         [(2, 5), (1, 5), (1, 5), (2, 5), (0, 5)]),
    Case("uncounted reads", [G_T],
         [(0, [(M, 8)], "ACGTTCAT", _q(8), 0x400, 60), (0, [(M, 8)], "ACGTTCAT", _q(8), 0, 9), (0, [(M, 8)], "ACGTTCAT", _q(8), 0x200, 60),
          (0, [(M, 8)], "ACGTTCAT", _q(8), 0, 10)],
         [(0, 0), (0, 0), (0, 0), (2, 5)]),
    # candidates are the records with ref_start <= start < ref_end: none of a read that starts behind the record or ends on it
    Case("reads without a candidate", [G_T],
         [(5, [(M, 8)], "CATAATAG", _q(8), 0, 60), (0, [(M, 4)], "ACGT", _q(4), 0, 60)], [(0, 0), (0, 0)]),
    Case("an empty table", [], [(0, [(M, 8)], "ACGTTCAT", _q(8), 0, 60)], [(0, 0)]),
]


# ---- the rounds case -------------------------------------------------------------------------------------------------------------
ROUNDS_RECORDS = 140                        # at 10, 12, ..., 288: 64 + 64 + 12 candidates of a read over all of them
SET_X, SET_Y = 11, 13                       # even records are in X, odd ones in Y: the two sets interleave all along
FIRST_SEEN = 70                             # the first record a long read shows anything at: in round 2, an even one


def rounds_records() -> List[PhasedRecord]:
    """REF A every 2 bp; haplotype 1 is C and haplotype 2 is G."""
    return [rec(10 + 2 * k, "A", "C", "G", SET_X if k % 2 == 0 else SET_Y) for k in range(ROUNDS_RECORDS)]


def _long(x_round2: str, x_round3: str, y: str):
    """A 300-base read at 0: T (neither allele) at the records 0 .. 63, the right base at low quality at 64 .. 69, then
    ``x_round2`` at the even records up to 126, ``x_round3`` at the even records from 128 on, and ``y`` at the odd ones."""
    bases, quals = ["A"] * 300, [30] * 300
    for k in range(ROUNDS_RECORDS):
        p = 10 + 2 * k
        if k < 64:
            bases[p] = "T"
        elif k < FIRST_SEEN:
            bases[p], quals[p] = "C", 5
        elif k % 2:
            bases[p] = y
        else:
            bases[p] = x_round2 if k < 128 else x_round3
    return (0, [(M, 300)], "".join(bases), quals, 0, 60)


def _short(n: int):
    """A read at 0 with exactly ``n`` candidate records, all observed: C at records 0, 3, 6, ..., G at the others."""
    length = 2 * n + 10                     # the record n - 1 ends at 2 n + 9, the record n starts at 2 n + 10
    bases = ["A"] * length
    for k in range(n):
        bases[10 + 2 * k] = "C" if k % 3 == 0 else "G"
    return (0, [(M, length)], "".join(bases), [30] * length, 0, 60)


def rounds_reads():
    """-> (reads, the (hp, ps) worked by hand).  Set X is chosen in round 2 (record 70) by both long reads.
    Long read 1: X shows haplotype 1 at its 29 records of round 2 (70 .. 126) and haplotype 2 at its 6 of round 3 (128 .. 138);
    Y shows haplotype 2 at all 35: n1 = 29, n2 = 6 -> hp 1.  Round 3 alone would say 2; counting Y too would say 2.
    Long read 2: X shows 2 at round 2 and 1 at round 3, Y shows 1: n1 = 6, n2 = 29 -> hp 2.
    Short reads with n = 1, 63, 64, 65 candidates: the set is X (record 0); of X's records k = 0, 2, 4, ... below n, those with
    k % 3 == 0 (k = 0, 6, 12, ...) show haplotype 1, the others haplotype 2."""
    reads = [_long("C", "G", "G"), _long("G", "C", "C")]
    want = [(1, SET_X), (2, SET_X)]
    for n in (1, 63, 64, 65):
        reads.append(_short(n))
        n1 = len([k for k in range(0, n, 2) if k % 3 == 0])
        n2 = len([k for k in range(0, n, 2) if k % 3 != 0])
        want.append((1 if n1 > n2 else 2 if n2 > n1 else 0, SET_X))
    return reads, want
