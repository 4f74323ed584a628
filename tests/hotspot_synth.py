"""Synthetic genomes and reads for the hotspot tests and tools/hotspot_bench.py: a donor with SNVs and indels, reads sampled
from it with their exact CIGARs against the reference, plus sequencing errors, clips, N bases, low qualities, filtered flags,
low mapping qualities and repeated names."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from tests.bam_writer import Read

BASES = "ACGT"


def random_reference(rng: np.random.Generator, length: int, masked_fraction: float = 0.0) -> str:
    ref = "".join(rng.choice(list(BASES), size=length))
    if masked_fraction > 0:                                   # soft-masked stretches (lower case, kept by the FASTA reader)
        chars = list(ref)
        for _ in range(max(1, int(length * masked_fraction / 50))):
            a = int(rng.integers(0, max(1, length - 50)))
            for i in range(a, min(length, a + 50)):
                chars[i] = chars[i].lower()
        ref = "".join(chars)
    return ref


def donor(rng, reference: str, snv_rate: float, indel_rate: float) -> Tuple[str, List[int]]:
    """-> (donor sequence, reference position of every donor base or -1 for inserted bases)."""
    seq, where = [], []
    p = 0
    n = len(reference)
    while p < n:
        u = rng.random()
        if u < indel_rate / 2 and p > 0:                      # deletion of 1-6 bases
            p += int(rng.integers(1, 7))
            continue
        if u < indel_rate:                                    # insertion of 1-6 bases before p
            for _ in range(int(rng.integers(1, 7))):
                seq.append(BASES[int(rng.integers(0, 4))])
                where.append(-1)
        b = reference[p].upper()
        if rng.random() < snv_rate:
            b = BASES[(BASES.index(b) + int(rng.integers(1, 4))) % 4] if b in BASES else "A"
        seq.append(b)
        where.append(p)
        p += 1
    return "".join(seq), where


def cigar_of(where: List[int]) -> Tuple[int, List[Tuple[int, int]]]:
    """Alignment of donor bases (ref position or -1) -> (leftmost reference position, CIGAR)."""
    ops: List[Tuple[int, int]] = []

    def push(op, n):
        if ops and ops[-1][0] == op:
            ops[-1] = (op, ops[-1][1] + n)
        else:
            ops.append((op, n))
    first = next((w for w in where if w >= 0), None)
    last = None
    for w in where:
        if w < 0:
            push(1, 1)
            continue
        if last is not None and w > last + 1:
            push(2, w - last - 1)
        push(0, 1)
        last = w
    if first is None:
        return 0, ops
    # a read that starts with inserted bases is placed at the first aligned base (a leading insertion: a left partial)
    return first, ops


def sample_reads(rng, reference: str, coverage: float, read_len: int, snv_rate=0.01, indel_rate=0.001, pacbio=False,
                 error_rate=0.002, prefix="r", hard=True, noisy=True) -> List[Read]:
    dseq, where = donor(rng, reference, snv_rate, indel_rate)
    n_reads = int(coverage * len(dseq) / read_len)
    starts = np.sort(rng.integers(0, max(1, len(dseq) - read_len), size=n_reads))
    reads = []
    for i, s in enumerate(starts):
        s = int(s)
        L = read_len if not pacbio else int(rng.integers(read_len // 2, read_len * 3 // 2))
        seg, wseg = list(dseq[s:s + L]), where[s:s + L]
        if not any(w >= 0 for w in wseg):
            continue
        if pacbio:                                            # PacBio-like: extra single-base insertion / deletion errors
            seg, wseg = _pacbio_noise(rng, seg, wseg)
        qual = [int(q) for q in rng.integers(20, 41, size=len(seg))]
        for j in range(len(seg)):
            if rng.random() < error_rate:
                seg[j] = BASES[int(rng.integers(0, 4))]
            if noisy and rng.random() < 0.002:
                seg[j] = "N"
            if noisy and rng.random() < 0.01:
                qual[j] = int(rng.integers(2, 10))
        pos, cigar = cigar_of(wseg)
        if noisy and cigar and cigar[0][0] == 0 and cigar[0][1] > 10 and rng.random() < 0.1:
            k = int(rng.integers(1, 6))                       # soft clip: the first k aligned bases
            cigar = [(4, k), (0, cigar[0][1] - k)] + cigar[1:]
            pos += k
        if hard and noisy and rng.random() < 0.05:
            cigar = [(5, int(rng.integers(1, 20)))] + cigar
        flag = 16 if rng.random() < 0.5 else 0
        mapq = 60
        if noisy:
            u = rng.random()
            if u < 0.01:
                flag |= 0x400
            elif u < 0.02:
                flag |= 0x100
            elif u < 0.03:
                flag |= 0x1                                   # paired, not proper
            elif u < 0.04:
                flag |= 0x3                                   # proper pair
            elif u < 0.05:
                flag |= 0x200                                 # QC fail: kept
            u = rng.random()
            if u < 0.02:
                mapq = 0
            elif u < 0.06:
                mapq = int(rng.integers(1, 10))
        name = f"{prefix}{i}"
        if noisy and i > 0 and rng.random() < 0.01:
            name = f"{prefix}{i - 1}"                          # a repeated name (same or other strand)
        reads.append(Read(name, pos, cigar, "".join(seg), qual, flag, mapq))
    reads.sort(key=lambda r: r.pos)
    return reads


def _pacbio_noise(rng, seg, wseg, rate=0.01):
    out, wout = [], []
    for b, w in zip(seg, wseg):
        u = rng.random()
        if u < rate and out:                                  # drop the base: a deletion in the CIGAR
            continue
        if u < 2 * rate:                                      # a random base before it: an insertion
            out.append(BASES[int(rng.integers(0, 4))])
            wout.append(-1)
        out.append(b)
        wout.append(w)
    return out, wout
