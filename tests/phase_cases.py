"""Inputs of the phasing tests (tests/test_phase.py on the CPU, tests/test_gpu_phase.py on the GPU): the table of cases worked by
hand, one per rule of DESIGN.md section 7g, and the synthetic chromosome of the GPU tests.  No case needs a reference text: a
record carries its own alleles."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Sequence

import numpy as np

from hello_amd.phase import Record
from tests.bam_writer import Read
from tests.gvcf_cases import D, EQ, H, I, M, N, P, S, X, reads_of  # noqa: F401

NONE = -1


def _q(n, q=30):
    return [q] * n


def snp(start, ref, alt, a=0, b=1, alts=None):
    alleles = [ref] + (alts or [alt])
    return Record(start, start + len(ref), a, b, alleles[a].encode(), alleles[b].encode())


@dataclass
class Case:
    """reads: (pos, cigar, bases, qualities, flag, mapq); slots: per read, one value per candidate record in record order."""
    name: str
    records: List[Record]
    reads: List[tuple]
    slots: List[List[int]]
    why: List[str] = field(default_factory=list)       # per read, the cause of a NONE at its first candidate (only where given)


G_T = snp(4, "G", "T")                       # chr:5 G>T, span [4, 5)
# q_threshold 10, mapq_threshold 10 throughout; every expected slot was worked out by hand from the rules
OBSERVE_TABLE: List[Case] = [
    Case("SNP seen as a, as b, as neither", [G_T],
         [(0, [(M, 8)], "ACGTGCAT", _q(8), 0, 60), (0, [(M, 8)], "ACGTTCAT", _q(8), 0, 60), (0, [(M, 8)], "ACGTCCAT", _q(8), 0, 60)],
         [[0], [1], [NONE]], ["", "", "neither"]),
    Case("= and X operations read like M", [G_T], [(0, [(EQ, 4), (X, 1), (EQ, 3)], "ACGTTCAT", _q(8), 0, 60)], [[1]]),
    # REF GCA -> G: the D removes C and A, the base at 4 is all the read shows over [4, 7)
    Case("deletion record matched by a D", [snp(4, "GCA", "G")],
         [(0, [(M, 5), (D, 2), (M, 3)], "ACGTGTAC", _q(8), 0, 60), (0, [(M, 10)], "ACGTGCATAC", _q(10), 0, 60),
          (0, [(M, 5), (D, 1), (M, 4)], "ACGTGATAC", _q(9), 0, 60)],
         [[1], [0], [NONE]], ["", "", "neither"]),
    # REF G -> GTT: the I behind the base at 4 joins it
    Case("insertion record matched by an I joined on its left", [snp(4, "G", "GTT")],
         [(0, [(M, 5), (I, 2), (M, 3)], "ACGTGTTCAT", _q(10), 0, 60), (0, [(M, 8)], "ACGTGCAT", _q(8), 0, 60),
          (0, [(M, 5), (I, 3), (M, 3)], "ACGTGTTTCAT", _q(11), 0, 60)],
         [[1], [0], [NONE]], ["", "", "neither"]),
    # REF TG -> TGA, span [3, 5): the I sits behind B - 1 = 4.  Counted while an aligned base follows (ref_end 8 > B); a read that
    # ends at B shows nothing, with the I or without it
    Case("I anchored at B - 1, counted and not counted", [snp(3, "TG", "TGA")],
         [(0, [(M, 5), (I, 1), (M, 3)], "ACGTGACAT", _q(9), 0, 60), (0, [(M, 5), (I, 1)], "ACGTGA", _q(6), 0, 60),
          (0, [(M, 5)], "ACGTG", _q(5), 0, 60), (0, [(M, 6)], "ACGTGC", _q(6), 0, 60)],
         [[1], [NONE], [NONE], [0]], ["", "end", "end", ""]),
    Case("I anchored at A - 1 is ignored", [G_T], [(0, [(M, 4), (I, 2), (M, 4)], "ACGTCCGCAT", _q(10), 0, 60)], [[0]]),
    # REF TGC, span [3, 6): T at 3, the D removes 4 and 5, the I behind it has position 5 on its left -> "TAA"
    Case("D followed by I", [snp(3, "TGC", "TAA")], [(0, [(M, 4), (D, 2), (I, 2), (M, 3)], "ACGTAAATA", _q(9), 0, 60)], [[1]]),
    Case("N over the span, and N beside it", [G_T],
         [(0, [(M, 3), (N, 3), (M, 3)], "ACGCAT", _q(6), 0, 60), (0, [(M, 5), (N, 2), (M, 2)], "ACGTGAC", _q(7), 0, 60)],
         [[NONE], [0]], ["N", ""]),
    Case("soft and hard clips in front", [G_T],
         [(2, [(S, 3), (M, 6)], "NNNGTTCAT", _q(9), 0, 60), (2, [(H, 2), (S, 3), (M, 6), (H, 1)], "NNNGTGCAT", _q(9), 0, 60),
          (2, [(S, 1), (P, 1), (M, 6)], "NGTTCAT", _q(7), 0, 60)],
         [[1], [0], [1]]),
    Case("lower-case read bases", [G_T], [(0, [(M, 8)], "acgttcat", _q(8), 0, 60)], [[1]]),
    Case("low quality inside the span and outside it", [G_T, snp(6, "A", "ACC")],
         [(0, [(M, 8)], "ACGTTCAT", [30, 30, 30, 30, 9, 30, 30, 30], 0, 60), (0, [(M, 8)], "ACGTTCAT", [2, 2, 2, 2, 10, 2, 30, 2], 0, 60),
          (0, [(M, 7), (I, 2), (M, 1)], "ACGTTCACCT", [30] * 8 + [9, 30], 0, 60)],
         [[NONE, 0], [1, 0], [1, NONE]], ["quality", "", ""]),
    # 1/2 at a site with ALT T,C: a is T, b is C, the reference base is neither
    Case("a 1/2 record", [snp(4, "G", None, 1, 2, ["T", "C"])],
         [(0, [(M, 8)], "ACGTTCAT", _q(8), 0, 60), (0, [(M, 8)], "ACGTCCAT", _q(8), 0, 60), (0, [(M, 8)], "ACGTGCAT", _q(8), 0, 60)],
         [[0], [1], [NONE]], ["", "", "neither"]),
    Case("uncounted reads have no slot", [G_T],
         [(0, [(M, 8)], "ACGTTCAT", _q(8), 0x400, 60), (0, [(M, 8)], "ACGTTCAT", _q(8), 0, 9), (0, [(M, 8)], "ACGTTCAT", _q(8), 0x200, 60),
          (0, [(M, 8)], "ACGTTCAT", _q(8), 0, 10)],
         [[], [], [], [1]]),
    # candidates are the records with ref_start <= A < ref_end: the record at 4 is none of the read at 5, and the one at 12 none of a
    # read that ends at 12
    Case("candidate records", [G_T, snp(8, "A", "C"), snp(12, "T", "A")],
         [(0, [(M, 12)], "ACGTTCATGATA", _q(12), 0, 60), (5, [(M, 9)], "CATAATAGA", _q(9), 0, 60)],
         [[1, NONE], [0, NONE]], ["", ""]),
]

# ---- links: SNPs at 2 (A/C), 5 (G/T), 8 (A/T), 11 (C/G), window 2.  The first read shows (a, a, b, b), the second (b, -, b, -)
LINK_RECORDS = [snp(2, "A", "C"), snp(5, "G", "T"), snp(8, "A", "T"), snp(11, "C", "G")]
LINK_READS = [(0, [(M, 14)], "AAAAAGAATAAGAA", _q(14), 0, 60), (0, [(M, 14)], "AACAAAAATAAAAA", _q(14), 0, 60)]
LINK_SLOTS = [[0, 0, 1, 1], [1, NONE, 1, NONE]]
LINK_WINDOW = 2
# link[t][k - 1] = [cis, trans]: t = 1 with 0 cis; t = 2 with 1 trans, with 0 trans (read 1) and cis (read 2); t = 3 with 2 cis, with 1
# trans; record 3 is not linked to record 0 (k = 3 > window)
LINKS = [[[0, 0], [0, 0]], [[1, 0], [0, 0]], [[0, 1], [1, 1]], [[1, 0], [0, 1]]]


@dataclass
class ChainCase:
    name: str
    link: list                         # [n][window][2]
    sets: List[int]
    flip: List[int]
    window: int = 2
    min_margin: int = 2
    chromosome: Sequence[int] = ()


Z = [0, 0]
CHAIN_TABLE: List[ChainCase] = [
    ChainCase("join", [[Z, Z], [[3, 0], Z]], [0, 0], [0, 0]),
    # record 1 is trans to 0: flipped; record 2 is cis to the flipped 1: its counts swap, so it is flipped too
    ChainCase("flip", [[Z, Z], [[0, 3], Z], [[3, 0], Z]], [0, 0, 0], [0, 1, 1]),
    # records 0 and 1 are two sets; record 2 has margin 2 to both: the set of k = 1 wins
    ChainCase("a tie goes to the nearest set", [[Z, Z], [Z, Z], [[2, 0], [0, 2]]], [0, 1, 1], [0, 0, 0]),
    ChainCase("the larger margin wins over the nearer set", [[Z, Z], [Z, Z], [[2, 0], [0, 3]]], [0, 1, 0], [0, 0, 1]),
    ChainCase("margin one short opens a new set", [[Z, Z], [[2, 1], Z]], [0, 1], [0, 0]),
    ChainCase("margin at the threshold joins", [[Z, Z], [[3, 1], Z]], [0, 0], [0, 0]),
    ChainCase("a lone record", [[Z, Z]], [0], [0]),
    # {0, 1} and {2, 3}: record 3 is linked to both sets (margin 2 to record 1, 3 to record 2), joins one, and the sets stay two
    ChainCase("two sets are never merged", [[Z, Z], [[3, 0], Z], [Z, Z], [[3, 0], [2, 0]]], [0, 0, 2, 2], [0, 0, 0, 0]),
    ChainCase("the counts of one set add up over k", [[Z, Z], [[3, 0], Z], [[1, 0], [1, 0]]], [0, 0, 0], [0, 0, 0]),
    ChainCase("a record of another chromosome is not linked", [[Z, Z], [[5, 0], Z]], [0, 1], [0, 0], chromosome=[0, 1]),
]

# ---- haplotags: records 0 and 1 are one set (record 1 flipped), 2 and 3 another, 4 is alone
TAG_SETS, TAG_FLIP, TAG_POSITIONS = [0, 0, 2, 2, 4], [0, 1, 0, 0, 0], [10, 20, 30, 40, 50]
TAG_SET_POSITIONS = [10, 10, 30, 30, 0]
# (first record, slots) per read, and the expected (hp, ps)
TAG_READS = [
    (0, [0, 1, 1, 1], (1, 10)),        # its first observation is in the set of 10: a at 0 and b at the flipped 1 are both haplotype 1
    (1, [NONE, 1, 1], (2, 30)),        # nothing at 1: its set is that of 30, b twice
    (0, [0, 0], (0, 10)),              # a at 0 is haplotype 1, a at the flipped 1 is haplotype 2: a tie keeps the set and says 0
    (0, [NONE, NONE], (0, 0)),
    (4, [0], (0, 0)),                  # an observation at an unphased record only
    (3, [1, 0], (2, 30)),              # the lone record 4 does not count
    (0, [], (0, 0)),
]

# ---- file lines: (input, record, flip, ps, expected)
LINE_TABLE = [
    (b"chr1\t5\t.\tG\tT\t30\t.\tHELLO\tGT\t0/1\n", G_T, 0, 5, b"chr1\t5\t.\tG\tT\t30\t.\tHELLO\tGT:PS\t0|1:5\n"),
    (b"chr1\t5\t.\tG\tT\t30\t.\tHELLO\tGT\t0/1\n", G_T, 1, 3, b"chr1\t5\t.\tG\tT\t30\t.\tHELLO\tGT:PS\t1|0:3\n"),
    (b"chr1\t5\t.\tG\tT,C\t30\t.\tHELLO\tGT\t1/2", snp(4, "G", None, 1, 2, ["T", "C"]), 1, 5, b"chr1\t5\t.\tG\tT,C\t30\t.\tHELLO\tGT:PS\t2|1:5"),
    # the FORMAT of --annotate_evidence with --include_hp
    (b"chr1\t10\t.\tA\tC\t120.3\tPASS\tHELLO;MQ=60.00;MBQ=30,31;MPOS=3,4\tGT:GQ:DP:AD:ADF:ADR:PL:ADI:ADP:AH1:AH2\t"
     b"0/1:30:10:5,5:3,1:2,4:13,0,13:4,2:1,3:2,3:2,2\r\n", snp(9, "A", "C"), 0, 10,
     b"chr1\t10\t.\tA\tC\t120.3\tPASS\tHELLO;MQ=60.00;MBQ=30,31;MPOS=3,4\tGT:GQ:DP:AD:ADF:ADR:PL:ADI:ADP:AH1:AH2:PS\t"
     b"0|1:30:10:5,5:3,1:2,4:13,0,13:4,2:1,3:2,3:2,2:10\r\n"),
]

# lines that pass through: not a/b, equal alleles, a symbolic or N allele, already phased, an allele the line does not have
NOT_PHASABLE = [b"chr1\t5\t.\tG\tT\t30\t.\tHELLO\tGT\t1/1\n", b"chr1\t5\t.\tG\tT\t30\t.\tHELLO\tGT\t./.\n",
                b"chr1\t5\t.\tG\t<NON_REF>\t.\t.\tEND=9\tGT:GQ\t0/1:3\n", b"chr1\t5\t.\tN\tT\t30\t.\tHELLO\tGT\t0/1\n",
                b"chr1\t5\t.\tG\tT\t30\t.\tHELLO\tGT:PS\t0|1:5\n", b"chr1\t5\t.\tG\tT\t30\t.\tHELLO\tGT\t0/2\n",
                b"chr1\t5\t.\tG\tT\t30\t.\tHELLO\n", b"\n"]


# ---- the synthetic chromosome of the GPU tests ----------------------------------------------------------------------------------
LENGTH = 6000
DENSE = (2000, 3000)                         # a record every 8 bp: a long read holds more than 64 candidate records
GAP = (3400, 3800)                           # no record: longer than any short read
WINDOW = 8


def _other(base: str, k: int = 1) -> str:
    return "ACGT"[("ACGT".index(base) + k) % 4]


def synthetic(seed: int = 1):
    """-> (reference, VCF data lines, short reads, long reads).  Two planted haplotypes; the records' a allele lies on haplotype 1
    except where ``swap`` says otherwise (those records come out flipped).  Short reads: 150 b at ~20x; long reads: 1 - 4 kb at ~15x
    with ~1 % indel noise; one long read of more than 300 operations; a short read inside GAP without any candidate record; reads
    with an N operation, with low qualities and ending right behind a record."""
    rng = np.random.default_rng(seed)
    ref = "".join(rng.choice(list("ACGT"), size=LENGTH))
    sites = sorted(set(range(60, DENSE[0] - 20, 100)) | set(range(DENSE[0], DENSE[1], 8)) | set(range(DENSE[1] + 40, GAP[0] - 10, 80))
                   | set(range(GAP[1] + 10, LENGTH - 60, 120)))
    lines, variants = [], []                 # variants: (start, ref allele, hap1 allele, hap2 allele)
    for n, p in enumerate(sites):
        kind = "snp" if DENSE[0] <= p < DENSE[1] else ("snp", "snp", "del", "ins", "snp")[n % 5]
        if kind == "snp":
            r, alts = ref[p], [_other(ref[p])]
        elif kind == "del":
            r, alts = ref[p:p + 3], [ref[p]]
        else:
            r, alts = ref[p], [ref[p] + _other(ref[p + 1], 2) + _other(ref[p + 1], 2)]
        a, b = 0, 1
        if p == sites[7]:                    # the 1/2 record
            r, alts, a, b = ref[p], [_other(ref[p]), _other(ref[p], 2)], 1, 2
        alleles = [r] + alts
        swap = bool(rng.random() < 0.4)
        h1, h2 = (alleles[b], alleles[a]) if swap else (alleles[a], alleles[b])
        variants.append((p, r, h1, h2))
        lines.append(("chr1\t%d\t.\t%s\t%s\t30\t.\tHELLO\tGT\t%d/%d\n" % (p + 1, r, ",".join(alts), a, b)).encode())
    # a homozygous record, which passes through, and a 1/2 record whose alleles no read carries, which stays unphased
    x = sites[10] + 2
    lines.insert(11, ("chr1\t%d\t.\t%s\t%s,%s\t30\t.\tHELLO\tGT\t1/2\n" % (x + 1, ref[x], _other(ref[x]), _other(ref[x], 2))).encode())
    lines.insert(5, ("chr1\t%d\t.\t%s\t%s\t30\t.\tHELLO\tGT\t1/1\n" % (sites[4] + 3, ref[sites[4] + 2], _other(ref[sites[4] + 2]))).encode())

    def read(name, start, stop, hap, noise=0.0, low=0.0):
        """The read of haplotype ``hap`` over [start, stop) of the reference, with every planted variant inside it."""
        cigar, seq = [], []

        def push(op, n, text=""):
            if n == 0:
                return
            if cigar and cigar[-1][0] == op:
                cigar[-1] = (op, cigar[-1][1] + n)
            else:
                cigar.append((op, n))
            seq.append(text)
        p = start
        for v, r, h1, h2 in variants:
            if v < p or v + len(r) >= stop:
                continue
            allele = (h1, h2)[hap]
            while p < v:                     # reference bases up to the variant, with indel noise
                if noise and rng.random() < noise and p + 2 < v:
                    if rng.random() < 0.5:
                        push(D, 1)
                        p += 1
                    else:
                        push(I, 1, "ACGT"[int(rng.integers(4))])
                        push(M, 1, ref[p])
                        p += 1
                else:
                    push(M, 1, ref[p])
                    p += 1
            push(M, 1, allele[0])
            if len(allele) > len(r):
                push(I, len(allele) - len(r), allele[1:])
            elif len(r) > len(allele):
                push(D, len(r) - len(allele))
            p = v + len(r)
        push(M, stop - p, ref[p:stop])
        text = "".join(seq)
        qual = [int(q) for q in np.where(rng.random(len(text)) < low, 5, 30)]
        return Read(name, start, cigar, text, qual, 0, 60)

    short, long = [], []
    for i in range(int(20 * LENGTH / 150)):
        start = int(rng.integers(0, LENGTH - 150))
        r = read("s%d" % i, start, start + 150, int(rng.integers(2)), low=0.02)
        if i % 50 == 0:
            r.flag = 0x400                   # a duplicate: not counted
        short.append(r)
    for i in range(int(15 * LENGTH / 2500)):
        n = int(rng.integers(1000, 4001))
        start = int(rng.integers(0, LENGTH - n))
        long.append(read("l%d" % i, start, start + n, i % 2, noise=0.01, low=0.01))
    # the read of more than 300 operations: = / X runs over the dense stretch and beyond
    base = read("many", DENSE[0] - 300, DENSE[1] + 300, 0)
    ops, at = [], 0
    for op, n in base.cigar:
        if op == M:
            for j in range(n):
                ops.append((X if (at + j) % 4 == 0 else EQ, 1))
            at += n
        else:
            ops.append((op, n))
            at += n if op == I else 0
    merged = []
    for op, n in ops:
        if merged and merged[-1][0] == op:
            merged[-1] = (op, merged[-1][1] + n)
        else:
            merged.append((op, n))
    long.append(Read("many", base.pos, merged, base.seq, base.qual, 0, 60))
    # a read with an N over records, one that ends right behind a record's span, and one inside the gap
    v = variants[3]
    spliced = read("n", v[0] - 40, v[0] + 110, 0)
    left = v[0] - 40
    spliced = Read("n", left, [(M, 38), (N, 6), (M, 106)], spliced.seq[:38] + ref[v[0] + 4:v[0] + 110], [30] * 144, 0, 60)
    w = variants[12]
    ends = read("e", w[0] - 100, w[0] + len(w[1]) + 1, 0)
    last = [(M, ends.cigar[-1][1] - 1)] if ends.cigar[-1][1] > 1 else []
    ends = Read("e", ends.pos, ends.cigar[:-1] + last, ends.seq[:-1], ends.qual[:-1], 0, 60)
    short += [spliced, ends, read("gap", GAP[0] + 100, GAP[0] + 250, 0)]
    short.sort(key=lambda r: r.pos)
    long.sort(key=lambda r: r.pos)
    return ref, lines, short, long
