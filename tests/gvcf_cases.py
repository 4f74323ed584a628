"""Inputs of the gVCF tests (tests/test_gvcf.py on the CPU, tests/test_gpu_refblocks.py on the GPU): the table of counting cases
worked by hand, one per rule of DESIGN.md section 7f, and the synthetic span of the tile tests."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

from hello_amd.bam import Reads
from tests import hotspot_synth as synth
from tests.bam_writer import Read

M, I, D, N, S, H, P, EQ, X = range(9)
TILE = 1024                                  # kRbTile of hello_amd/csrc/refblocks.hip


def reads_of(records: Sequence[tuple]) -> Reads:
    """(pos, [(op, length)], bases, qualities, flag, mapq) per read -> the arrays ``hello_bam_fetch`` would give."""
    bases, quals, cigars, read_off, cigar_off = [], [], [], [0], [0]
    starts, ends, mapq, flags = [], [], [], []
    for pos, cigar, seq, qual, flag, mq in records:
        bases.append(np.frombuffer(seq.encode(), np.uint8))
        quals.append(np.asarray(qual, np.uint8))
        assert len(seq) == len(qual)
        cigars += [(n << 4) | op for op, n in cigar]
        read_off.append(read_off[-1] + len(seq))
        cigar_off.append(cigar_off[-1] + len(cigar))
        starts.append(pos)
        ends.append(pos + max(1, sum(n for op, n in cigar if op in (M, D, N, EQ, X))))
        mapq.append(mq)
        flags.append(flag)
    n = len(records)
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)   # noqa: E731
    return Reads(bases=cat(bases, np.uint8), quals=cat(quals, np.uint8), read_offsets=np.array(read_off, np.int64),
                 cigars=np.array(cigars, np.uint32), cigar_offsets=np.array(cigar_off, np.int64), ref_starts=np.array(starts, np.int64),
                 ref_ends=np.array(ends, np.int64), mapq=np.array(mapq, np.uint8), flags=np.array(flags, np.uint16),
                 name_hash=np.arange(n, dtype=np.uint64), strand=np.zeros(n, np.uint8), hp=np.zeros(n, np.uint8))


def reads_of_bam_records(reads: Sequence[Read]) -> Reads:
    """tests.bam_writer records -> the same arrays, without a file."""
    return reads_of([(r.pos, r.cigar, r.seq, list(r.qual), r.flag, r.mapq) for r in reads])


@dataclass
class Case:
    name: str
    reference: str
    reads: List[tuple]
    n_ref: List[int]
    n_total: List[int]
    lo: int = 0
    hi: int = -1

    def span(self) -> Tuple[int, int]:
        return self.lo, len(self.reference) if self.hi < 0 else self.hi


def _q(n, q=30):
    return [q] * n


def _flag_case(name, flag, mapq, depth):
    return Case(name, "ACGT", [(0, [(M, 4)], "ACGT", _q(4), flag, mapq)], [depth] * 4, [depth] * 4)


# q_threshold 10, mapq_threshold 10 throughout; every expected counter was worked out by hand from the rules
HAND_TABLE: List[Case] = [
    Case("match / mismatch", "ACGTACGT", [(0, [(M, 8)], "ACTTACGT", _q(8), 0, 60)], [1, 1, 0, 1, 1, 1, 1, 1], [1] * 8),
    Case("= and X operations count like M", "ACGTACGT", [(0, [(EQ, 2), (X, 1), (EQ, 5)], "ACTTACGT", _q(8), 0, 60)],
         [1, 1, 0, 1, 1, 1, 1, 1], [1] * 8),
    Case("low-quality base", "ACGT", [(0, [(M, 4)], "ACGT", [30, 9, 10, 30], 0, 60)], [1, 0, 1, 1], [1, 0, 1, 1]),
    Case("lower-case reference base that matches", "acgT", [(0, [(M, 4)], "ACGA", _q(4), 0, 60)], [1, 1, 1, 0], [1] * 4),
    Case("lower-case read base", "ACGT", [(0, [(M, 4)], "acgt", _q(4), 0, 60)], [1] * 4, [1] * 4),
    Case("N read base", "ACGT", [(0, [(M, 4)], "ANGT", _q(4), 0, 60)], [1, 0, 1, 1], [1, 0, 1, 1]),
    Case("N reference base", "ANGT", [(0, [(M, 4)], "ACGT", _q(4), 0, 60)], [1, 0, 1, 1], [1] * 4),
    Case("D counted without a quality", "ACGTACGT", [(0, [(M, 2), (D, 3), (M, 2)], "ACCG", [30, 30, 2, 30], 0, 60)],
         [1, 1, 0, 0, 0, 0, 1, 0], [1, 1, 1, 1, 1, 0, 1, 0]),
    Case("N skipped", "ACGTACGT", [(0, [(M, 2), (N, 3), (M, 2)], "ACCG", _q(4), 0, 60)], [1, 1, 0, 0, 0, 1, 1, 0], [1, 1, 0, 0, 0, 1, 1, 0]),
    Case("last M base before I", "ACGTAC", [(0, [(M, 3), (I, 2), (M, 3)], "ACGTTTAC", _q(8), 0, 60)], [1, 1, 0, 1, 1, 1], [1] * 6),
    Case("last M base before P and I", "ACGTAC", [(0, [(M, 3), (P, 1), (I, 2), (M, 3)], "ACGTTTAC", _q(8), 0, 60)],
         [1, 1, 0, 1, 1, 1], [1] * 6),
    Case("last M base before I, of low quality", "ACGTAC", [(0, [(M, 3), (I, 2), (M, 3)], "ACGTTTAC", [30, 30, 5, 30, 30, 30, 30, 30], 0, 60)],
         [1, 1, 0, 1, 1, 1], [1, 1, 0, 1, 1, 1]),
    Case("I as first operation", "ACGTAC", [(1, [(I, 2), (M, 4)], "TTCGTA", _q(6), 0, 60)], [0, 1, 1, 1, 1, 0], [0, 1, 1, 1, 1, 0]),
    Case("S / H", "ACGTAC", [(2, [(H, 2), (S, 2), (M, 3), (S, 1), (H, 3)], "TTGTAC", _q(6), 0, 60)], [0, 0, 1, 1, 1, 0], [0, 0, 1, 1, 1, 0]),
    Case("both mates count where they overlap", "ACGTAC", [(0, [(M, 4)], "ACGT", _q(4), 0x63, 60), (2, [(M, 4)], "GTAC", _q(4), 0x93, 60)],
         [1, 1, 2, 2, 1, 1], [1, 1, 2, 2, 1, 1]),
    _flag_case("flag: unmapped", 0x4, 60, 0),
    _flag_case("flag: secondary", 0x100, 60, 0),
    _flag_case("flag: supplementary", 0x800, 60, 0),
    _flag_case("flag: duplicate", 0x400, 60, 0),
    _flag_case("flag: paired, not a proper pair", 0x1, 60, 0),
    _flag_case("flag: proper pair", 0x3, 60, 1),
    _flag_case("flag: QC fail", 0x200, 60, 0),
    _flag_case("flag: reverse strand", 0x10, 60, 1),
    _flag_case("mapq 0", 0, 0, 0),
    _flag_case("mapq below the threshold", 0, 9, 0),
    _flag_case("mapq at the threshold", 0, 10, 1),
    Case("a read crossing lo and one crossing hi", "ACGTACGTACGT",
         [(2, [(M, 4)], "GTAC", _q(4), 0, 60), (6, [(M, 4)], "GAAC", _q(4), 0, 60), (7, [(D, 3), (M, 1)], "T", _q(1), 0, 60)],
         [1, 1, 1, 0], [1, 1, 1, 2], lo=4, hi=8),
    Case("a read that ends at lo and one that starts at hi", "ACGTACGTACGT",
         [(0, [(M, 4)], "ACGT", _q(4), 0, 60), (8, [(M, 4)], "ACGT", _q(4), 0, 60)], [0] * 4, [0] * 4, lo=4, hi=8),
]


# ---- the tile test's span ---------------------------------------------------------------------------------------------------
SPAN_LO = 389                                # not aligned to a tile
SPAN = 3 * TILE + 17
GAP = (SPAN_LO + TILE - 90, SPAN_LO + 2 * TILE + 130)     # no read touches it: wider than a tile, both edges inside tiles
EXCLUDED = [(SPAN_LO, SPAN_LO + 2), (SPAN_LO + 500, SPAN_LO + 503), (SPAN_LO + 503, SPAN_LO + 504),
            (SPAN_LO + 2 * TILE + 300, SPAN_LO + 2 * TILE + 301), (SPAN_LO + 3 * TILE - 3, SPAN_LO + 3 * TILE + 4),
            (SPAN_LO + SPAN - 1, SPAN_LO + SPAN)]


def tile_input(seed: int = 5):
    """-> (reference, Illumina-like reads, PacBio-like reads): a reference of SPAN_LO + SPAN + 400 bases with a soft-masked stretch;
    ~8x of 150-base reads from tests.hotspot_synth over the span outside GAP, reads placed across every tile edge that has coverage,
    and one read of more than 64 operations that spans all tiles (written with = / X runs)."""
    rng = np.random.default_rng(seed)
    length = SPAN_LO + SPAN + 400
    chars = list(synth.random_reference(rng, length))
    for i in range(SPAN_LO + 200, SPAN_LO + 420):                            # soft-masked
        chars[i] = chars[i].lower()
    for i in range(SPAN_LO + 2 * TILE + 200, SPAN_LO + 2 * TILE + 260):
        chars[i] = chars[i].lower()
    reference = "".join(chars)
    sampled = synth.sample_reads(rng, reference, 8, 150, snv_rate=0.01, indel_rate=0.004, prefix="s")
    reads = [r for r in sampled if r.ref_end <= GAP[0] or r.pos >= GAP[1]]
    exact = lambda name, pos, n: Read(name, pos, [(M, n)], reference[pos:pos + n].upper(), [30] * n, 0, 60)   # noqa: E731
    reads += [exact("lo", SPAN_LO - 70, 150), exact("edge1", SPAN_LO + TILE - 140, 50), exact("edge3", SPAN_LO + 3 * TILE - 75, 150),
              exact("hi", SPAN_LO + SPAN - 60, 150), exact("edge2", GAP[1], 150)]
    # a thinly covered stretch: depth 1 to 3 gives low bands beside the deep ones
    reads = [r for r in reads if r.ref_end <= SPAN_LO + 2 * TILE + 400 or r.pos >= SPAN_LO + 2 * TILE + 700]
    reads += [exact(f"thin{i}", SPAN_LO + 2 * TILE + 400 + 60 * i, 100 + 40 * (i % 3)) for i in range(5)]
    reads.sort(key=lambda r: r.pos)
    # the long read: = / X runs of 1 to 40 bases from before the span to behind it; its bases over the gap are of quality 5, so it
    # crosses the tile edges inside the gap without covering them
    other = lambda b: "ACGT"[("ACGT".index(b.upper()) + 1) % 4]             # noqa: E731
    pos, cigar, seq = SPAN_LO - 30, [], []
    p, k = pos, 0
    while p < SPAN_LO + SPAN + 20:
        n = min(int(rng.integers(1, 41)), SPAN_LO + SPAN + 20 - p)
        if k % 2:
            cigar.append((X, 1))
            seq.append(other(reference[p]))
            p += 1
        else:
            cigar.append((EQ, n))
            seq.append(reference[p:p + n].upper())
            p += n
        k += 1
    text = "".join(seq)
    qual = [int(q) for q in rng.integers(8, 41, size=len(text))]
    for i in range(GAP[0] - 10 - pos, GAP[1] + 10 - pos):
        qual[i] = 5
    long_read = Read("long", pos, cigar, text, qual, 0, 60)
    return reference, reads, [long_read]
