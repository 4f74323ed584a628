"""Inputs of the fragment tests (tests/test_phase_fragments.py on the CPU, tests/test_gpu_phase_fragments.py on the GPU): tables
worked by hand, one case per clause of DESIGN.md section 7i, and the paired chromosomes of the two files.

Every hand case uses the records of ``RECORDS``: SNPs A/C at 10, 20, 30, 40, 50 and 60 (indices 0..5).  A read is all ``A`` (allele
a, observation 0) except where its row says otherwise: ``C`` is allele b (1), ``G`` is neither (none).  A read over [s, s + n)
has the records with s <= position < s + n as candidates.  A counted paired read needs flag 0x2 as well (``gvcf.usable``), so the
first mate of the tables is 0x43 and the second 0x83.  Expected tags are those under ``phase.chain(links, window, min_margin=1)``."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

import numpy as np

from hello_amd.bam import Reads
from hello_amd.phase import Record
from tests.bam_writer import Read
from tests.gvcf_cases import M, reads_of

NONE = -1
FIRST, SECOND = 0x43, 0x83
RECORDS = [Record(p, p + 1, 0, 1, b"A", b"C") for p in (10, 20, 30, 40, 50, 60)]
TOP = 2 ** 64 - 1


def read_set(rows: Sequence[tuple]) -> Reads:
    """(name_hash, flag, mapq, start, length, {position: base}) per read -> the arrays ``hello_bam_fetch`` would give."""
    made = []
    for _, flag, mapq, start, length, bases in rows:
        text = "".join(bases.get(p, "A") for p in range(start, start + length))
        made.append((start, [(M, length)], text, [30] * length, flag, mapq))
    return dataclasses.replace(reads_of(made), name_hash=np.array([row[0] for row in rows], np.uint64))


@dataclass
class Case:
    name: str
    reads: List[tuple]                                   # source 0
    mate: List[int]                                      # over source 0's reads, then source 1's
    links: Dict[Tuple[int, int, int], int]               # {(t, k, 0 cis | 1 trans): count}; every other counter is 0
    hp: List[int]
    ps: List[int]
    window: int = 2
    pairs: int = 0
    refused: int = 0
    reads1: List[tuple] = field(default_factory=list)    # source 1
    records: List[Record] = field(default_factory=lambda: RECORDS)

    def sets(self) -> List[Reads]:
        return [read_set(self.reads)] + ([read_set(self.reads1)] if self.reads1 else [])

    def dense_links(self) -> np.ndarray:
        link = np.zeros((len(self.records), self.window, 2), np.int32)
        for (t, k, trans), count in self.links.items():
            link[t, k - 1, trans] = count
        return link


LEFT = (5, 20, {})                           # records 0 and 1: a, a
RIGHT = (45, 20, {50: "C", 60: "C"})         # records 4 and 5: b, b
# the links of LEFT and RIGHT as one fragment at window 3: 1 - 0 cis, 5 - 4 cis and, across the gap, 4 - 1 (k = 3) trans; 4 - 0 and
# 5 - 1 are k = 4.  Chained at margin 1: set 0 holds 0, 1, 4, 5 with 4 and 5 flipped, records 2 and 3 are alone.
JOINED = {(1, 1, 0): 1, (5, 1, 0): 1, (4, 3, 1): 1}
APART = {(1, 1, 0): 1, (5, 1, 0): 1}        # two sets, {0, 1} (POS 11) and {4, 5} (POS 51): RIGHT alone is b, b there -> hp 2

HAND_TABLE: List[Case] = [
    # F = (a, a, -, -, b, b); o xor flip is 0 at all four observed records
    Case("a gap whose cross-gap records are within the window", [(7, FIRST, 60, *LEFT), (7, SECOND, 60, *RIGHT)],
         [1, 0], JOINED, [1, 1], [11, 11], window=3, pairs=1),
    # window 2: no link crosses the gap, two sets; the fragment's first observation is in the set of 11, so BOTH mates get it, and
    # the observations at 4 and 5 are in another set and do not count (alone, the second mate would be hp 2 in the set of 51)
    Case("a gap whose cross-gap records are beyond the window", [(7, FIRST, 60, *LEFT), (7, SECOND, 60, *RIGHT)],
         [1, 0], APART, [1, 1], [11, 11], window=2, pairs=1),
    # first mate over records 0, 1, 2: a, b, a; second over 1, 2, 3: b, a, b.  F = (a, b, a, b); every link once -- per read,
    # 2 - 1 would be counted twice.  Chain: flips (0, 1, 0, 1), one set
    Case("overlapping mates that agree are counted once",
         [(7, FIRST, 60, 5, 30, {20: "C"}), (7, SECOND, 60, 15, 30, {20: "C", 40: "C"})],
         [1, 0], {(1, 1, 1): 1, (2, 1, 1): 1, (2, 2, 0): 1, (3, 1, 1): 1, (3, 2, 0): 1}, [1, 1], [11, 11], pairs=1),
    # record 1: a in the first mate, b in the second -> none; F = (a, -, a, a): 2 - 0 at k = 2, 3 - 2 at k = 1, nothing through 1
    Case("overlapping mates that disagree leave the record out",
         [(7, FIRST, 60, 5, 30, {}), (7, SECOND, 60, 15, 30, {20: "C"})],
         [1, 0], {(2, 2, 0): 1, (3, 1, 0): 1}, [1, 1], [11, 11], pairs=1),
    # record 1: b in the first mate, G (neither allele) in the second -> b; F = (a, b, a, a).  Chain: flips (0, 1, 0, 0)
    Case("a shared record that one mate observes and the other does not",
         [(7, FIRST, 60, 5, 30, {20: "C"}), (7, SECOND, 60, 15, 30, {20: "G"})],
         [1, 0], {(1, 1, 1): 1, (2, 1, 1): 1, (2, 2, 0): 1, (3, 1, 0): 1, (3, 2, 1): 1}, [1, 1], [11, 11], pairs=1),
    # the second mate has mapq 5: not counted, no slot, no group of two
    Case("a mate that is not counted", [(7, FIRST, 60, 5, 20, {20: "C"}), (7, SECOND, 5, 25, 20, {})],
         [-1, -1], {(1, 1, 1): 1}, [1, 0], [11, 0]),
    Case("a group of three", [(7, FIRST, 60, 5, 20, {}), (7, SECOND, 60, 15, 20, {}), (7, SECOND, 60, 25, 20, {})],
         [-1, -1, -1], {(1, 1, 0): 1, (2, 1, 0): 1, (3, 1, 0): 1}, [1, 1, 1], [11, 11, 11], refused=1),
    Case("two first mates", [(7, FIRST, 60, *LEFT), (7, FIRST, 60, *RIGHT)], [-1, -1], APART, [1, 2], [11, 51], window=3, refused=1),
    Case("flag 0x1 unset", [(7, 0x40, 60, *LEFT), (7, 0x80, 60, *RIGHT)], [-1, -1], APART, [1, 2], [11, 51], window=3, refused=1),
    Case("the same name in source 0 and source 1", [(7, FIRST, 60, *LEFT)], [-1, -1], APART, [1, 2], [11, 51], window=3,
         reads1=[(7, SECOND, 60, *RIGHT)]),
    Case("the second mate before the first in file order", [(7, SECOND, 60, *LEFT), (7, FIRST, 60, *RIGHT)],
         [1, 0], JOINED, [1, 1], [11, 11], window=3, pairs=1),
    Case("a read whose mate is absent", [(7, FIRST, 60, *LEFT)], [-1], {(1, 1, 0): 1}, [1], [11]),
    # two pairs, name 0 and name 2^64 - 1, the second with the alleles the other way round: F = (b, b, -, -, a, a) -> hp 2
    Case("name_hash 0 and 2^64 - 1",
         [(0, FIRST, 60, *LEFT), (TOP, FIRST, 60, 5, 20, {10: "C", 20: "C"}), (0, SECOND, 60, *RIGHT), (TOP, SECOND, 60, 45, 20, {})],
         [2, 3, 0, 1], {key: 2 for key in JOINED}, [1, 2, 1, 2], [11] * 4, window=3, pairs=2),
    Case("an empty read set", [], [], {}, [], []),
    Case("an empty record table", [(7, FIRST, 60, *LEFT), (7, SECOND, 60, *RIGHT)], [1, 0], {}, [0, 0], [0, 0], pairs=1, records=[]),
]


# ---- the chromosomes ----------------------------------------------------------------------------------------------------------
LENGTH = 6000


def _other(base: str) -> str:
    return "ACGT"[("ACGT".index(base) + 1) % 4]


def _planted(seed: int, sites: Sequence[int]):
    """-> (reference, VCF data lines GT 0/1, hap: per site the allele index (0 REF, 1 ALT) on haplotype 1)."""
    rng = np.random.default_rng(seed)
    ref = "".join(rng.choice(list("ACGT"), size=LENGTH))
    hap = [int(x) for x in rng.integers(0, 2, size=len(sites))]
    lines = [("chr1\t%d\t.\t%s\t%s\t30\t.\tHELLO\tGT\t0/1\n" % (p + 1, ref[p], _other(ref[p]))).encode() for p in sites]
    return ref, lines, hap


def _read(name, ref, sites, hap, which, start, stop, flag) -> Read:
    """The noise-free read of haplotype ``which`` (0 or 1) over [start, stop)."""
    text = list(ref[start:stop])
    for p, h in zip(sites, hap):
        if start <= p < stop and (h ^ which) == 1:
            text[p - start] = _other(ref[p])
    return Read(name, start, [(M, stop - start)], "".join(text), [30] * (stop - start), flag, 60)


def illumina_pairs(seed: int = 3):
    """What the feature is for -> (VCF lines, hap, reads sorted by position): 20 heterozygous SNVs 300 bp apart; 600 pairs (30x) of
    150-base mates whose starts lie 300 bp apart, so that no read holds two records and every pair whose first mate holds a
    record holds the next one with its second; flags 0x63 / 0x93 (0x41 / 0x81, proper pair, the strand bits); no noise."""
    sites = list(range(150, LENGTH, 300))
    ref, lines, hap = _planted(seed, sites)
    reads = []
    for j in range(600):
        start = (j * (LENGTH - 450)) // 600
        reads.append(_read("p%d" % j, ref, sites, hap, j % 2, start, start + 150, 0x63))
        reads.append(_read("p%d" % j, ref, sites, hap, j % 2, start + 300, start + 450, 0x93))
    reads.sort(key=lambda r: r.pos)
    return lines, hap, reads


def two_sources(seed: int = 5):
    """The 6 kb two-source chromosome of the GPU tests -> (VCF lines, short reads, long reads), each sorted by position: a record
    every 100 bp; 400 pairs (20x) of 150-base mates with inserts of 300 - 600 bp and, every fifth pair, of 160 - 290 bp
    (overlapping mates, some sharing two records), 2 % of the bases at quality 5, ten second mates at mapq 5; 36 unpaired reads of 1 - 4 kb (15x) in the second source."""
    rng = np.random.default_rng(seed)
    sites = list(range(50, LENGTH - 50, 100))
    ref, lines, hap = _planted(seed, sites)
    short, long = [], []
    for j in range(400):
        insert = int(rng.integers(160, 291)) if j % 5 == 0 else int(rng.integers(300, 601))
        start = int(rng.integers(0, LENGTH - insert))
        which = int(rng.integers(2))
        for k, (at, flag) in enumerate(((start, 0x63), (start + insert - 150, 0x93))):
            r = _read("s%d" % j, ref, sites, hap, which, at, at + 150, flag)
            r.qual = [int(q) for q in np.where(rng.random(150) < 0.02, 5, 30)]
            if j % 40 == 7 and k == 1:
                r.mapq = 5                                   # the second mate is not counted
            short.append(r)
    for j in range(36):
        n = int(rng.integers(1000, 4001))
        start = int(rng.integers(0, LENGTH - n))
        long.append(_read("l%d" % j, ref, sites, hap, j % 2, start, start + n, 0))
    short.sort(key=lambda r: r.pos)
    long.sort(key=lambda r: r.pos)
    return lines, short, long
