"""Inputs of the contamination tests (tests/test_contamination.py on the CPU, tests/test_gpu_contamination.py on the GPU): pileups
worked by hand, one case per rule of DESIGN.md section 7n, the edge stress on one 6 kb chromosome, and planted mixtures.

A hand row is (name_hash, flag, position, CIGAR, bases, qualities, mapq), the format of tests/qc_cases.py, on a reference of 200
bases, ``ACGT`` fifty times: position p holds ``"ACGT"[p % 4]``.  The sites are 0, 10, 11, 20, 63, 64, 100, 150 and 199; q_threshold
and mapq_threshold are 10.  The expected COUNTS are written sparsely -- {(site position, strand, bin): value}, what is not named is
0 -- and were worked out from the rules, not from the code."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from hello_amd import contamination as cn
from tests.gvcf_cases import D, EQ, I, M, N, S, X
from tests.qc_cases import overlapping, read_set  # noqa: F401  (the tests take them from here)

A, C, G, T, OTHER, DEL, LOWQ = range(7)
FWD, REVS = 0, 1
REV = 0x10
REF = "ACGT" * 50
SITES = [0, 10, 11, 20, 63, 64, 100, 150, 199]


def q(n: int, value: int = 30) -> List[int]:
    return [value] * n


@dataclass
class Case:
    name: str
    rows: List[tuple]
    counts_at: Dict[Tuple[int, int, int], int]       # (site position, strand, bin) -> value
    counts: Dict[str, int]                           # of cn.METRIC_STATS, what is not 0 (belonging and n_sites are filled in)
    reference: str = REF
    sites: List[int] = field(default_factory=lambda: list(SITES))

    def cut(self) -> int:
        """Where the two-span run cuts the chromosome: through the first read, two bases behind its start."""
        return self.rows[0][2] + 2 if self.rows else 100

    def expected(self) -> np.ndarray:
        out = np.zeros((len(self.sites), 2, 7), np.int64)
        for (p, strand, which), v in self.counts_at.items():
            out[self.sites.index(p), strand, which] = v
        return out

    def want_counts(self) -> Dict[str, int]:
        return dict(dict.fromkeys(cn.METRIC_STATS, 0), belonging=len(self.rows), n_sites=len(self.sites), **self.counts)


M4 = [(M, 4)]


def at18(bases: str, flag: int = 0, quals=None, mapq: int = 60, cigar=None) -> tuple:
    """A read of four bases over 18 .. 21: its third base lies on the site at 20."""
    return (1, flag, 18, cigar or M4, bases, quals or q(len(bases)), mapq)


HAND_TABLE: List[Case] = [
    Case("each base on each strand", [at18("GT" + b + "C", flag) for flag in (0, REV) for b in "ACGT"],
         {(20, s, b): 1 for s in (FWD, REVS) for b in (A, C, G, T)}, dict(counting=8, reads_on_a_site=8, observations=8)),
    Case("quality at q_threshold - 1 and at q_threshold", [at18("GTGC", quals=[30, 30, 9, 30]), at18("GTGC", quals=[30, 30, 10, 30])],
         {(20, FWD, LOWQ): 1, (20, FWD, G): 1}, dict(counting=2, reads_on_a_site=2, observations=2)),
    Case("mapq at the threshold and below", [at18("GTGC", mapq=10), at18("GTGC", mapq=9)],
         {(20, FWD, G): 1}, dict(counting=1, reads_on_a_site=1, observations=1)),
    # unmapped, secondary, supplementary, duplicate, QC-fail, paired but no proper pair, mapq 0; a proper pair's mate counts
    Case("each filter flag of counted",
         [at18("GTGC", f) for f in (0x4, 0x100, 0x800, 0x400, 0x200, 0x1)] + [at18("GTGC", mapq=0), at18("GTGC", 0x3)],
         {(20, FWD, G): 1}, dict(counting=1, reads_on_a_site=1, observations=1)),
    # 2M 3I 4M at 16: the bases are 16 17 | inserted | 18 19 20 21, so the site's base is stored at index 7, not at 4
    Case("an insertion before a site, so the site shifts",
         [(1, 0, 16, [(M, 2), (I, 3), (M, 4)], "AC" + "TTT" + "GTCC", q(9), 60)],
         {(20, FWD, C): 1}, dict(counting=1, reads_on_a_site=1, observations=1)),
    # 2M 4D 2M at 16 deletes 18 .. 21; 2M 4N 2M skips them; 4S 4M at 22 and 4M 6S at 12 would reach 20 with their clips
    Case("D over a site, N over a site and a soft clip where a site would be",
         [(1, 0, 12, [(M, 4), (S, 6)], "ACGT" + "TTTTTT", q(10), 60), (2, REV, 16, [(M, 2), (D, 4), (M, 2)], "ACGT", q(4, 2), 60),
          (3, 0, 16, [(M, 2), (N, 4), (M, 2)], "ACGT", q(4), 60), (4, 0, 22, [(S, 4), (M, 4)], "TTTT" + "GTAC", q(8), 60)],
         {(20, REVS, DEL): 1}, dict(counting=4, reads_on_a_site=1, observations=1)),
    Case("= and X operations", [at18("GTCC", cigar=[(EQ, 2), (X, 1), (EQ, 1)])],
         {(20, FWD, C): 1}, dict(counting=1, reads_on_a_site=1, observations=1)),
    Case("a lower-case and a non-ACGT byte in the arrays", [at18("GTaC"), at18("GTNC"), at18("GTnC"), at18("GT=C"), at18("gttc", REV)],
         {(20, FWD, A): 1, (20, FWD, OTHER): 3, (20, REVS, T): 1}, dict(counting=5, reads_on_a_site=5, observations=5)),
    # 4M 2S at 17 ends on 20; 2S 4M at 20 begins on it
    Case("a site on a read's first and last aligned base",
         [(1, 0, 17, [(M, 4), (S, 2)], "CGTT" + "AA", q(6), 60), (2, 0, 20, [(S, 2), (M, 4)], "GG" + "CCGT", q(6), 60)],
         {(20, FWD, T): 1, (20, FWD, C): 1}, dict(counting=2, reads_on_a_site=2, observations=2)),
    # the read without a CIGAR lies on the site at 20 with no base to show; the read beside it shows its fifth
    Case("a read without a CIGAR", [(1, 0, 16, [(M, 8)], "CCCCACCC", q(8), 60), (2, 0, 20, [], "", [], 60)],
         {(20, FWD, A): 1}, dict(counting=2, reads_on_a_site=1, observations=1)),
    Case("sites at positions 0 and 199", [(1, 0, 0, M4, "TCGT", q(4), 60), (2, REV, 196, M4, "ACGG", q(4), 60)],
         {(0, FWD, T): 1, (199, REVS, G): 1}, dict(counting=2, reads_on_a_site=2, observations=2)),
    Case("sites at bit 63 of a word and at bit 0 of the next", [(1, 0, 60, [(M, 8)], "ACGCGCGT", q(8), 60)],
         {(63, FWD, C): 1, (64, FWD, G): 1}, dict(counting=1, reads_on_a_site=1, observations=2)),
    Case("two adjacent sites", [(1, 0, 8, [(M, 6)], "ACGTAC", q(6), 60), (2, REV, 11, M4, "CCCC", q(4), 60)],
         {(10, FWD, G): 1, (11, FWD, T): 1, (11, REVS, C): 1}, dict(counting=2, reads_on_a_site=2, observations=3)),
    # 20M at 90 covers 90 .. 109; the two-span run cuts at 92, so the read belongs to the first span and its site lies in the second
    Case("a read that starts in one span and observes a site in the next", [(1, 0, 90, [(M, 20)], "A" * 10 + "C" + "A" * 9, q(20), 60)],
         {(100, FWD, C): 1}, dict(counting=1, reads_on_a_site=1, observations=1)),
]


# ---- the edge stress: one 6 kb chromosome ---------------------------------------------------------------------------------------
LENGTH = 6000                                      # 93 words and 48 positions
SPAN = 1000
DENSE_AT, DENSE_END, DENSE_STEP = 300, 1800, 7     # a site every 7 positions: the 1 500-base read at 300 meets 215 of them
EMPTY_AT = 2000                                    # no site in 1 801 .. 5 054: the 1 500-base read at 2 000 meets none
WORDS_AT, WORDS = 55 * 64, 24                      # a read over exactly the words 55 .. 78, whose only site is the last bit of the last
PILE_AT, PILE = 5500, 300                          # 300 copies of a 20-base read on the site at 5 509
SHARE = 1024                                       # kPileShare of pileup.hip: the most counting reads of a workgroup, asked for here
SURVIVORS = (0, 1, 255, 256, 257)


def stress_sites() -> np.ndarray:
    return np.array(sorted(set([0] + list(range(DENSE_AT, DENSE_END, DENSE_STEP)) + [WORDS_AT + WORDS * 64 - 1, PILE_AT + 9, LENGTH - 1])),
                    np.int64)


def stress(seed: int = 17):
    """-> (reference, sites, rows sorted by position): what tests/test_gpu_contamination.py's edge stress asserts really occurs."""
    rng = np.random.default_rng(seed)
    reference = "".join(rng.choice(list("ACGT"), size=LENGTH))
    rows: List[tuple] = []

    def add(flag, pos, cigar):
        bases, p = [], pos
        for op, k in cigar:
            if op in (M, EQ, X):
                bases.append("".join(b if rng.random() > 0.05 else "ACGTNa"[int(rng.integers(6))] for b in reference[p:p + k]))
                p += k
            elif op in (I, S):
                bases.append("".join(rng.choice(list("ACGT"), size=k)))
            elif op in (D, N):
                p += k
        stored = "".join(bases)
        quals = [int(v) for v in np.where(rng.random(len(stored)) < 0.1, 5, 30)]
        rows.append((len(rows) + 1, flag, pos, cigar, stored, quals, 60))
    for n, pos in enumerate(range(0, LENGTH - 150, 41)):                  # background: 150-base reads, every second reverse
        add(REV if n % 2 else 0, pos, [(M, 150)])
    add(0, LENGTH - 20, [(M, 20)])                                         # the last site of the chromosome (the first: the read at 0)
    add(0, DENSE_AT, [(M, 1500)])
    add(REV, DENSE_AT + 3, [(M, 700), (D, 30), (M, 300), (I, 5), (M, 400), (N, 40), (M, 30)])
    add(0, EMPTY_AT, [(M, 1500)])
    add(REV, WORDS_AT, [(M, WORDS * 64)])
    for edge in (SPAN, 2 * SPAN, 1024):                                    # clips, insertions and deletions across the edges
        add(0, edge - 70, [(S, 5), (M, 60), (D, 20), (M, 30), (I, 6), (M, 60)])
        add(REV, edge - 40, [(S, 4), (M, 30), (I, 2), (M, 30), (S, 3)])
    for n in range(PILE):
        add(REV if n % 3 == 0 else 0, PILE_AT, [(M, 20)])
    rows.sort(key=lambda r: r[2])
    return reference, stress_sites(), rows


def survivor_launch(k: int, tail: int = 100) -> List[tuple]:
    """``SHARE + tail`` counting reads of 20 bases, sorted: the first workgroup's share holds exactly ``k`` that cover a site (in the
    dense stretch, where every read of 20 bases covers two or three) and ``SHARE - k`` that cover none; the second workgroup's is
    partly empty and all of it covers the site of the pile."""
    hits = [(i + 1, 0, DENSE_AT + 10 + (i * 1100) // max(k, 1), [(M, 20)], "ACGT" * 5, q(20), 60) for i in range(k)]
    misses = [(2000 + i, REV * (i % 2), EMPTY_AT + i, [(M, 20)], "TGCA" * 5, q(20), 60) for i in range(SHARE - k)]
    rest = [(9000 + i, 0, PILE_AT, [(M, 20)], "GGGGG" * 4, q(20), 60) for i in range(tail)]
    return hits + misses + rest


# ---- the scan's carry: a chromosome of three rounds of the site scan ------------------------------------------------------------
CARRY_LENGTH = 2 * 65536 + 48                      # 2 049 words: two full rounds of 1 024 words and a third of one word
CARRY_SPAN = 50000
CARRY_NAMED = (0, 65535, 65536, 131071, 131072, CARRY_LENGTH - 1)      # the last and first bit of a round, and both ends


def carry(seed: int = 23):
    """-> (reference, sites, rows sorted by position): the named sites and 40 at seeded positions, a read of 20 to 150 bases over
    every site on alternating strands, and one read across each of the two round edges."""
    rng = np.random.default_rng(seed)
    reference = "".join(rng.choice(list("ACGT"), size=CARRY_LENGTH))
    sites = np.array(sorted(set(CARRY_NAMED) | set(int(p) for p in rng.integers(1, CARRY_LENGTH - 1, size=40))), np.int64)
    rows: List[tuple] = []

    def add(flag, pos, n):
        rows.append((len(rows) + 1, flag, pos, [(M, n)], reference[pos:pos + n], q(n), 60))
    for k, p in enumerate(int(p) for p in sites):
        n = int(rng.integers(20, 151))
        add(REV if k % 2 else 0, max(0, min(p - int(rng.integers(0, n)), CARRY_LENGTH - n)), n)
    add(0, 65536 - 50, 100)
    add(REV, 131072 - 40, 70)
    rows.sort(key=lambda r: r[2])
    return reference, sites, rows


# ---- the driver's BAMs: people with genotypes at known sites ---------------------------------------------------------------------
DRIVER_LENGTH = 20000


def population(seed: int = 5, length: int = DRIVER_LENGTH, step: int = 80):
    """-> (reference, POS, ALT letters, AF): a SNV site every ``step`` positions with an allele frequency of 0.1 .. 0.9."""
    rng = np.random.default_rng([seed, 11])
    reference = "".join(rng.choice(list("ACGT"), size=length))
    pos = np.arange(200, length - 200, step)
    alt = ["ACGT"[("ACGT".index(reference[p]) + 1 + int(rng.integers(3))) % 4] for p in pos]
    return reference, pos, alt, rng.uniform(0.1, 0.9, size=pos.shape[0])


def person(seed: int, af: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """-> (ALT copies per site drawn from Hardy-Weinberg, the haplotype that carries the ALT of a heterozygous site)."""
    rng = np.random.default_rng([seed, 12])
    return rng.binomial(2, af), rng.integers(0, 2, size=af.shape[0])


def reads_of_person(seed: int, reference: str, pos, alt, who, read_len: int, depth: float, prefix: str, copies: int = 0):
    """tests.bam_writer records, sorted: error-free reads of ``read_len`` bases of one of the person's two haplotypes each, about
    ``depth`` over every position; ``copies``: as many reads are written twice, the copy with lower qualities (a PCR duplicate)."""
    from tests.bam_writer import Read
    rng = np.random.default_rng([seed, 13])
    genotype, carrier = who
    starts = np.sort(rng.integers(0, len(reference) - read_len + 1, size=int(depth * len(reference) / read_len)))
    reads = []
    for n, s in enumerate(starts.tolist()):
        hap, seq = int(rng.integers(2)), list(reference[s:s + read_len])
        for k in range(int(np.searchsorted(pos, s)), int(np.searchsorted(pos, s + read_len))):
            if genotype[k] == 2 or (genotype[k] == 1 and carrier[k] == hap):
                seq[int(pos[k]) - s] = alt[k]
        reads.append(Read("%s%d" % (prefix, n), s, [(M, read_len)], "".join(seq), [30] * read_len, REV * int(rng.integers(2)), 60))
        if n < 4 * copies and n % 4 == 0:
            reads.append(Read("%sc%d" % (prefix, n), s, [(M, read_len)], "".join(seq), [20] * read_len, reads[-1].flag, 60))
    return reads


def sites_vcf(reference: str, pos, alt, af, chromosome: str = "chr1") -> str:
    """The text of a sites file for ``population``, its records in descending order of position (they need not be sorted)."""
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    lines += ["%s\t%d\t.\t%s\t%s\t.\t.\tAF=%r" % (chromosome, int(p) + 1, reference[int(p)], b, float(f)) for p, b, f in zip(pos, alt, af)][::-1]
    return "\n".join(lines) + "\n"


# ---- planted mixtures -----------------------------------------------------------------------------------------------------------
def planted(seed: int, alpha: float, n_sites: int = 200, depth: float = 30.0, error: float = 0.004, genotypes=None):
    """-> (r, a, o, af, genotypes): counts of a sample mixed with a fraction ``alpha`` of an unrelated one, both drawn from
    Hardy-Weinberg at af uniform in 0.05 .. 0.95 (``genotypes``: the sample's own, given instead of drawn)."""
    rng = np.random.default_rng([seed, 7])
    af = rng.uniform(0.05, 0.95, size=n_sites)
    g1 = rng.binomial(2, af) if genotypes is None else np.asarray(genotypes)
    g2 = rng.binomial(2, af)
    share = (1 - alpha) * g1 / 2 + alpha * g2 / 2                          # of the reads that carry ALT
    n = rng.poisson(depth, size=n_sites)
    p_alt = share * (1 - error) + (1 - share) * error / 3
    p_ref = (1 - share) * (1 - error) + share * error / 3
    counts = np.array([rng.multinomial(int(k), [pr, pa, max(0.0, 1 - pr - pa)]) for k, pr, pa in zip(n, p_ref, p_alt)], np.int64)
    return counts[:, 0], counts[:, 1], counts[:, 2], af, g1
