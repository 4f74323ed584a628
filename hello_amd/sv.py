"""Large deletions and insertions of sorted BAMs from the reads' own CIGARs, found on the GPU.

    python -m hello_amd.call --from_bam | --from_bams [--resident] ... --sv [--sv_min_size 50] [--sv_min_support 3] [--sv_flank 20]
                             [--sv_cluster_gap 100] [--sv_len_ratio 0.7] [--sv_split]
    python -m hello_amd.sv --bam B[,P] --ref F --output_prefix P [--phased_vcf V] [--chromosomes a,b] [--mapq_threshold 10]
                           [--sv_min_size 50] ... [--split] [--device N]

Not in the reference; DESIGN.md section 7p defines the rules.  By default intra-alignment events only: an ``I`` or ``D`` operation of
at least ``min_size`` bases inside one alignment record.  With ``--sv_split`` / ``--split`` (section 7q) the ``SA`` tags are read too and
every junction between two segments of a split alignment is a row as well (DEL, INS, DUP, INV, BND): ``segments_of``, ``junctions_of``
and ``split_rows_of`` restate those rules.  Clipped ends and discordant pairs are not looked at, so this is no complete
structural-variant caller.  ``signatures_of``, ``restated``, ``clustered`` and ``genotyped`` restate the rules in plain
Python / NumPy without a GPU; ``Caller`` binds ``hello_sv_*`` (hello_amd/csrc/sv.hip, sv.h), whose arrays equal the restatement
integer for integer, and ``clustered_native`` / ``genotyped_native`` run the host rules of the library alone.  ``measure`` is the pass
over one BAM (``spans.measure_spans``); its result, ``Events``, writes the VCF and the ``.npz``.
"""
from __future__ import annotations

import argparse
import ctypes as C
import logging
import math
import os
import re
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._abi import ARRAY_GETTER, READS, STATS_GETTER, bind, check, i32, i64, vp
from .bam import Reads, Splits
from .gvcf import _bytes_of, counted
from .spans import Handle, measure_spans, save_tables

DEL, INS = 0, 1
TYPE_NAMES = ("DEL", "INS")
SIGNATURE_COLUMNS = ("TYPE", "POS", "LEN", "SHIFT", "ORDINAL", "OP", "STRAND", "HP")
CANDIDATE_COLUMNS = ("TYPE", "POS", "LEN", "DV", "DV_FWD", "DV_REV", "HP0", "HP1", "HP2", "POS_MIN", "POS_MAX", "LEN_MIN", "LEN_MAX",
                     "DP", "DR", "GT", "GQ", "PL0", "PL1", "PL2")
CLUSTER_COLUMNS = CANDIDATE_COLUMNS[:13]                    # what the clusters alone give; the rest needs the cover
STATUS_NAMES = ("not_counted", "counting", "walked", "with_a_signature")     # STATUS of the last add, per read
COUNT_NAMES = ("reads_given", "belonging", "counting", "walked", "reads_with_a_signature", "signatures", "candidates")
# split alignments: the types of their rows, SPLIT_STATUS of the last add per read, and their statistics
DUP, INV3, INV5, BND = 2, 3, 4, 5
SPLIT_TYPE_NAMES = ("DEL", "INS", "DUP", "INV", "INV", "BND")
SPLIT_STATUS_NAMES = ("no_tag", "parsed", "with_a_row", "bad_sa", "too_many")
NO_TAG, PARSED, WITH_A_ROW, BAD_SA, TOO_MANY = range(5)
SPLIT_COUNT_NAMES = ("split_reads", "bad_sa", "too_many", "junctions", "junctions_dropped", "junctions_small", "junctions_unplaced",
                     "split_signatures")
TIME_NAMES = ("cover_ms", "reads_ms", "finish_ms", "split_ms")
STAT_NAMES = COUNT_NAMES + TIME_NAMES[:3] + SPLIT_COUNT_NAMES + TIME_NAMES[3:]
METRIC_STATS = COUNT_NAMES[1:]                              # what does not depend on the spans
SPLIT_METRIC_STATS = METRIC_STATS + SPLIT_COUNT_NAMES       # what a run with split alignments keeps
MAX_SEGMENTS = 8                                            # the primary and at most 7 entries of its SA tag
SA_MAX_POS, SA_MAX_COUNT = (1 << 31) - 1, (1 << 28) - 1
MIN_SIZE, FLANK, CLUSTER_GAP, LEN_RATIO, MIN_SUPPORT = 50, 20, 100, 0.7, 3
EPSILON = 0.05
GT_TEXT = ("0/0", "0/1", "1/1")
MAX_COUNTING_READS = (1 << 31) - 1

_log = logging.getLogger(__name__)


def percent_of(len_ratio: float) -> int:
    """``--sv_len_ratio`` as the integer the rules compare with."""
    return int(round(float(len_ratio) * 100))


# ------------------------------------------------------------------------------------------------
# the rules, restated: signatures and cover
# ------------------------------------------------------------------------------------------------
def _fold(b: int) -> int:
    return int(b) & 0xDF


def left_shift(ref: np.ndarray, bases: np.ndarray, kind: int, p: int, q: int, n: int, s: int) -> int:
    """k: the greatest value with cond(j) true for all j < k, over j < p - s only."""
    k = 0
    while k < p - s:
        left = _fold(ref[p - 1 - k])
        right = _fold(bases[q + n - 1 - k]) if kind == INS and k < n else _fold(ref[p - 1 - k + n])
        if left != right:
            break
        k += 1
    return k


# ------------------------------------------------------------------------------------------------
# the rules of the split alignments, restated: segments and junctions
# ------------------------------------------------------------------------------------------------
_SA_ENTRY = re.compile(rb"([^,]+),([0-9]{1,10}),([+-]),((?:[0-9]{1,10}[MIDNSHP=X])+),([0-9]{1,10}),([0-9]{1,10})", re.DOTALL)
_SA_OP = re.compile(rb"([0-9]+)([MIDNSHP=X])")


def _segment(tid: int, strand: int, s: int, ops: Sequence[Tuple[str, int]], mapq: int) -> Optional[Tuple[int, ...]]:
    """(tid, strand, s, a, m, b, r, mapq) of a CIGAR of (letter, count), or None: S and H lie in the leading and trailing runs
    alone, and the alignment has a query base and a reference base."""
    i, j = 0, len(ops)
    while i < j and ops[i][0] in "SH":
        i += 1
    while j > i and ops[j - 1][0] in "SH":
        j -= 1
    if any(op in "SH" for op, _ in ops[i:j]):
        return None
    a, b = sum(n for _, n in ops[:i]), sum(n for _, n in ops[j:])
    m, r = sum(n for op, n in ops[i:j] if op in "MI=X"), sum(n for op, n in ops[i:j] if op in "MDN=X")
    if m < 1 or r < 1:
        return None
    return (tid, strand, s, a, m, b, r, mapq)


def segments_of(primary: Tuple[int, int, Sequence[Tuple[int, int]], int], tag: bytes, contigs: Sequence[str], own: int,
                length: int) -> Tuple[int, List[Tuple[int, ...]]]:
    """``primary`` (ref_start, flag, [(BAM op, count)], mapq) and the read's SA text -> (PARSED, BAD_SA or TOO_MANY, the segments
    (tid, strand, s, a, m, b, r, mapq) in the order they appear, the primary first; none unless PARSED)."""
    tag = bytes(tag)
    if tag.count(b";") >= MAX_SEGMENTS:
        return TOO_MANY, []
    if not tag.endswith(b";"):
        return BAD_SA, []
    s, flag, ops, mapq = primary
    first = _segment(own, int(bool(flag & 0x10)), s, [("MIDNSHP=X"[op], n) for op, n in ops], mapq)
    if first is None or first[2] + first[6] > length:
        return BAD_SA, []
    total = first[3] + first[4] + first[5]
    names = {name.encode(): i for i, name in enumerate(contigs)}
    out = [first]
    for text in tag[:-1].split(b";"):
        found = _SA_ENTRY.fullmatch(text)
        if found is None:
            return BAD_SA, []
        rname, pos, strand, cigar, mq, _ = found.groups()
        ops = [(op.decode(), int(n)) for n, op in _SA_OP.findall(cigar)]
        if not 1 <= int(pos) <= SA_MAX_POS or int(mq) > 255 or any(not 1 <= n <= SA_MAX_COUNT for _, n in ops):
            return BAD_SA, []
        seg = _segment(names.get(rname, -1), int(strand == b"-"), int(pos) - 1, ops, int(mq))
        if seg is None or seg[3] + seg[4] + seg[5] != total or seg[2] + seg[6] > SA_MAX_POS or (seg[0] == own and seg[2] + seg[6] > length):
            return BAD_SA, []
        out.append(seg)
    return PARSED, out


def junctions_of(segments: Sequence[Tuple[int, ...]], own: int, length: int, min_size: int, flank: int,
                 mapq_threshold: int) -> List[Tuple]:
    """The segments of one read in their order of appearance -> per pair of neighbours on the read, in the read's order, one of
    ("dropped",), ("unplaced",), ("small",) and ("row", type, pos, len, shift, bound): ``bound`` > 0 marks a DEL that is still to
    move to the left, over j < bound; a BND carries the mate's tid as len and its breakpoint as shift."""
    def on_read(g):
        qs = g[5] if g[1] else g[3]
        return qs, qs + g[4]
    order = sorted(range(len(segments)), key=lambda i: on_read(segments[i]) + (i,))
    out: List[Tuple] = []
    for ia, ib in zip(order[:-1], order[1:]):
        A, B = segments[ia], segments[ib]
        g = on_read(B)[0] - on_read(A)[1]
        overlap = max(0, -g)
        if A[7] < mapq_threshold or B[7] < mapq_threshold or A[4] < flank or B[4] - overlap < flank:
            out.append(("dropped",))
            continue
        if A[0] != own and B[0] != own:
            out.append(("unplaced",))
            continue
        x = A[2] if A[1] else A[2] + A[6]                       # A's exit
        y = B[2] + B[6] if B[1] else B[2]                       # B's entry
        if (A[0] == own) != (B[0] == own):
            out.append(("row", BND, x, B[0], y, 0) if A[0] == own else ("row", BND, y, A[0], x, 0))
        elif A[1] != B[1]:
            n = abs(x - y)
            out.append(("row", INV5 if A[1] else INV3, min(x, y), n, 0, 0) if n >= min_size else ("small",))
        else:
            forward = not A[1]
            if overlap:                                         # trimmed from B: its entry moves on, the bases counted as matches
                y += overlap if forward else -overlap
                g = 0
                if not 0 <= y <= length:
                    out.append(("dropped",))
                    continue
            d = y - x if forward else x - y
            net, lower = d - g, min(x, y)
            if d <= -min_size:
                out.append(("row", DUP, lower, -d, 0, 0))
            elif net >= min_size:
                left = A if forward else B
                out.append(("row", DEL, lower, net, 0, max(0, lower - left[2]) if g == 0 else 0))
            elif net <= -min_size:
                out.append(("row", INS, lower, -net, 0, 0) if -net <= SA_MAX_POS else ("dropped",))
            else:
                out.append(("small",))
    return out


def split_rows_of(primary, tag: bytes, contigs: Sequence[str], own: int, ref: np.ndarray, min_size: int, flank: int, mapq_threshold: int,
                  ordinal: int, hp: int) -> Tuple[int, List[Tuple[int, ...]], Dict[str, int]]:
    """One counting read with a tag -> (its SPLIT_STATUS, its rows of SIGNATURE_COLUMNS, its junction counts)."""
    counts = dict.fromkeys(SPLIT_COUNT_NAMES[3:], 0)
    status, segments = segments_of(primary, tag, contigs, own, int(ref.shape[0]))
    rows: List[Tuple[int, ...]] = []
    if status != PARSED:
        return status, rows, counts
    strand = int(bool(primary[1] & 0x10))
    for k, found in enumerate(junctions_of(segments, own, int(ref.shape[0]), min_size, flank, mapq_threshold)):
        counts["junctions"] += 1
        if found[0] != "row":
            counts["junctions_" + found[0]] += 1
            continue
        _, kind, pos, n, shift, bound = found
        if bound > 0:
            shift = left_shift(ref, None, DEL, pos, 0, n, pos - bound)
            pos -= shift
        rows.append((kind, pos, n, shift, ordinal, -(k + 1), strand, hp))
    counts["split_signatures"] = len(rows)
    return (WITH_A_ROW if rows else PARSED), rows, counts


def signatures_of(reads: Reads, ref, lo: int, hi: int, min_size: int = MIN_SIZE, flank: int = FLANK, mapq_threshold: int = 10,
                  counting_given: int = 0, splits: Optional[Splits] = None, contigs: Optional[Sequence[str]] = None,
                  own: Optional[int] = None) -> Dict[str, object]:
    """One span [lo, hi) with the reads overlapping it -> ``signatures`` (rows of SIGNATURE_COLUMNS in the order the reads and their
    operations come), ``cover`` ([(position, +1 or -1)] of the difference array), ``counts`` (COUNT_NAMES but the candidates) and
    ``status`` (uint8 per read, STATUS_NAMES).  With ``splits`` (and ``contigs``, ``own``) the rows of the split alignments follow a
    read's own, ``counts`` holds SPLIT_COUNT_NAMES too and ``split_status`` is SPLIT_STATUS per read."""
    ref = _bytes_of(ref)
    length = int(ref.shape[0])
    if not 0 <= lo < hi <= length:
        raise ValueError("a span that leaves the reference")
    if min_size < 1 or flank < 1:
        raise ValueError("min_size and flank are 1 at the least")
    rows: List[Tuple[int, ...]] = []
    cover: List[Tuple[int, int]] = []
    status = np.zeros(reads.n_reads, np.uint8)
    split_status = np.zeros(reads.n_reads, np.uint8)
    counts = dict.fromkeys(COUNT_NAMES[:-1] + SPLIT_COUNT_NAMES, 0)
    counts["reads_given"] = reads.n_reads
    if splits is not None and (contigs is None or own is None or not 0 <= own < len(contigs)):
        raise ValueError("split alignments need the contig names and the chromosome's index among them")
    ordinal = counting_given
    for r in range(reads.n_reads):
        s = int(reads.ref_starts[r])
        if s < lo:
            continue
        counts["belonging"] += 1
        if not counted(int(reads.flags[r]), int(reads.mapq[r]), mapq_threshold):
            continue
        counts["counting"] += 1
        b0, b1 = int(reads.read_offsets[r]), int(reads.read_offsets[r + 1])
        ops = [(int(c) & 15, int(c) >> 4) for c in reads.cigars[int(reads.cigar_offsets[r]):int(reads.cigar_offsets[r + 1])]]
        if any(op > 8 for op, _ in ops) or sum(n for op, n in ops if op in (0, 1, 4, 7, 8)) != b1 - b0:
            raise ValueError(f"read {r}: its CIGAR does not consume exactly its {b1 - b0} bases")
        e = s + sum(n for op, n in ops if op in (0, 2, 3, 7, 8))
        if e - s >= 2 * flank and s + flank < length:
            cover += [(s + flank, 1), (min(e - flank, length - 1) + 1, -1)]
        status[r] = 1
        if any(op in (1, 2) and n >= min_size for op, n in ops):
            counts["walked"] += 1
            status[r] = 2
            p, q, found = s, 0, 0
            for index, (op, n) in enumerate(ops):
                if op in (1, 2) and n >= min_size:
                    pe = p + n if op == 2 else p
                    if p - s >= flank and e - pe >= flank and pe <= length:
                        kind = DEL if op == 2 else INS
                        k = left_shift(ref, reads.bases[b0:b1], kind, p, q, n, s)
                        hp = int(reads.hp[r])
                        rows.append((kind, p - k, n, k, ordinal, index, int(bool(int(reads.flags[r]) & 0x10)), hp))
                        found += 1
                if op in (0, 2, 3, 7, 8):
                    p += n
                if op in (0, 1, 4, 7, 8):
                    q += n
            if found:
                status[r] = 3
                counts["reads_with_a_signature"] += 1
                counts["signatures"] += found
        if splits is not None and splits.offsets[r + 1] > splits.offsets[r]:
            tag = splits.bytes[int(splits.offsets[r]):int(splits.offsets[r + 1])].tobytes()
            bam_ops = [(op, n) for op, n in ops]
            split_status[r], more, of_read = split_rows_of((s, int(reads.flags[r]), bam_ops, int(reads.mapq[r])), tag, contigs, own, ref,
                                                           min_size, flank, mapq_threshold, ordinal, int(reads.hp[r]))
            rows += more
            counts["split_reads"] += 1
            counts["bad_sa"] += int(split_status[r] == BAD_SA)
            counts["too_many"] += int(split_status[r] == TOO_MANY)
            for k, v in of_read.items():
                counts[k] += v
        ordinal += 1
    return dict(signatures=rows, cover=cover, counts=counts, status=status, split_status=split_status)


def _columns(rows: Sequence[Sequence[int]], names: Sequence[str], prefix: str) -> Dict[str, np.ndarray]:
    table = np.array(rows, np.int64).reshape(-1, len(names))
    return {prefix + name: table[:, i].copy() for i, name in enumerate(names)}


# ------------------------------------------------------------------------------------------------
# the rules, restated: clusters, depth and genotype
# ------------------------------------------------------------------------------------------------
def clustered(signatures: Sequence[Sequence[int]], cluster_gap: int = CLUSTER_GAP, len_ratio_percent: int = percent_of(LEN_RATIO),
              min_support: int = MIN_SUPPORT, with_sr: bool = False) -> List[Tuple[int, ...]]:
    """Rows of SIGNATURE_COLUMNS, in any order -> rows of CLUSTER_COLUMNS sorted by (pos, type, len); ``with_sr``: and SR behind
    them, the distinct reads of the group with a row of a split alignment.  BND rows are never clustered."""
    sigs = sorted((tuple(int(v) for v in row) for row in signatures if int(row[0]) < BND), key=lambda g: (g[0], g[1], g[2], g[4], g[5]))
    out = []
    i = 0
    while i < len(sigs):
        j = i + 1
        while j < len(sigs) and sigs[j][0] == sigs[i][0] and sigs[j][1] - sigs[j - 1][1] <= cluster_gap:
            j += 1
        run = sorted(sigs[i:j], key=lambda g: (g[2], g[1], g[4], g[5]))
        start = 0
        for k in range(len(run)):
            if k + 1 == len(run) or 100 * run[k][2] < len_ratio_percent * run[k + 1][2]:
                group = run[start:k + 1]
                start = k + 1
                who = {g[4]: (g[6], g[7] if g[7] in (1, 2) else 0) for g in reversed(group)}
                if len(who) < min_support:
                    continue
                m = len(group)
                pos, lens = sorted(g[1] for g in group), [g[2] for g in group]
                by_hp = [sum(1 for _, hp in who.values() if hp == x) for x in (0, 1, 2)]
                rev = sum(strand for strand, _ in who.values())
                sr = (len({g[4] for g in group if g[5] < 0}),) if with_sr else ()
                out.append((group[0][0], pos[(m - 1) // 2], lens[(m - 1) // 2], len(who), len(who) - rev, rev, *by_hp, pos[0], pos[-1],
                            lens[0], lens[-1]) + sr)
        i = j
    return sorted(out, key=lambda c: (c[1], c[0], c[2]))


def genotype_of(dv: int, dr: int) -> Tuple[int, int, int, int, int]:
    """(GT index, GQ, PL 0/0, PL 0/1, PL 1/1)."""
    like = [dv * math.log10(f) + dr * math.log10(1.0 - f) for f in (EPSILON, 0.5, 1.0 - EPSILON)]
    best = max(range(3), key=lambda g: (like[g], -g))           # the first greatest
    pl = [int(math.floor(-10.0 * (x - like[best]) + 0.5)) for x in like]
    return (best, min(sorted(pl)[1], 99), *pl)


def genotyped(clusters: Sequence[Sequence[int]], diff: np.ndarray) -> List[Tuple[int, ...]]:
    """Rows of CLUSTER_COLUMNS and the cover's difference array [length + 1] -> rows of CANDIDATE_COLUMNS; rows with SR behind
    them keep it behind them.  A supporter with a split row ends at the breakpoint and is not among the spanning reads."""
    spanning = np.cumsum(np.asarray(diff, np.int64))
    out = []
    for c in clusters:
        c, sr = tuple(c[:len(CLUSTER_COLUMNS)]), tuple(c[len(CLUSTER_COLUMNS):])
        dp = int(spanning[c[1]])
        dr = max(0, dp - (c[3] - sum(sr)))
        out.append(c + (dp, dr) + genotype_of(c[3], dr) + sr)
    return out


def restated(spans: Sequence[tuple], ref, min_size: int = MIN_SIZE, flank: int = FLANK, mapq_threshold: int = 10,
             cluster_gap: int = CLUSTER_GAP, len_ratio_percent: int = percent_of(LEN_RATIO), min_support: int = MIN_SUPPORT,
             contigs: Optional[Sequence[str]] = None, own: Optional[int] = None) -> Tuple[Dict[str, np.ndarray], Dict[str, int]]:
    """({SIGNATURES_*, CANDIDATES_*, STATUS and SPLIT_STATUS of the last span, DIFF}, the counts) of one chromosome given as
    (reads, lo, hi) or, with split alignments, (reads, splits, lo, hi) span after span, from the restatement."""
    ref = _bytes_of(ref)
    diff = np.zeros(ref.shape[0] + 1, np.int64)
    counts = dict.fromkeys(COUNT_NAMES + SPLIT_COUNT_NAMES, 0)
    rows: List[Tuple[int, ...]] = []
    status = split_status = np.zeros(0, np.uint8)
    for reads, *splits, lo, hi in spans:
        part = signatures_of(reads, ref, lo, hi, min_size, flank, mapq_threshold, counts["counting"], splits[0] if splits else None,
                             contigs, own)
        split_status = part["split_status"]
        rows += part["signatures"]
        for at, by in part["cover"]:
            diff[at] += by
        for k, v in part["counts"].items():
            counts[k] += v
        status = part["status"]
    rows.sort(key=lambda g: (g[0], g[1], g[2], g[4], g[5]))
    found = genotyped(clustered(rows, cluster_gap, len_ratio_percent, min_support, with_sr=True), diff)
    counts["candidates"] = len(found)
    tables = dict(_columns(rows, SIGNATURE_COLUMNS, "SIGNATURES_"), **_columns(found, CANDIDATE_COLUMNS + ("SR",), "CANDIDATES_"))
    tables.update(STATUS=status, SPLIT_STATUS=split_status, DIFF=diff)
    return tables, counts


# ------------------------------------------------------------------------------------------------
# the library
# ------------------------------------------------------------------------------------------------
_PROTOTYPES = (
    ("hello_sv_create", [vp, i64, i32, i32, i32, i32, C.POINTER(vp)]),
    ("hello_sv_add", [vp] + READS + [i64, i64, i64]),
    ("hello_sv_finish", [vp, i64, i32, i32]),
    ("hello_sv_array", ARRAY_GETTER),
    ("hello_sv_stats", STATS_GETTER),
    ("hello_sv_free", [vp], None),
    ("hello_sv_genotype", [vp, vp, i64, vp]),
    ("hello_sv_cluster", [vp, i64, i64, i32, i32, vp, C.POINTER(i64)]),
    ("hello_sv_cluster_split", [vp, i64, i64, i32, i32, vp, C.POINTER(i64)]),
    ("hello_sv_contigs", [vp, C.POINTER(C.c_char_p), i64, i64]),
    ("hello_sv_add_split", [vp] + READS + [vp, vp, i64, i64, i64, i64]),
)


def _lib():
    return bind(_PROTOTYPES)


def genotyped_native(dv, dr) -> np.ndarray:
    """int64 [n, 5] (GT index, GQ, PL 0/0, PL 0/1, PL 1/1) from ``hello_sv_genotype`` (host only: no device is opened)."""
    dv, dr = np.ascontiguousarray(dv, np.int64), np.ascontiguousarray(dr, np.int64)
    out = np.zeros((dv.shape[0], 5), np.int64)
    check(_lib().hello_sv_genotype(dv.ctypes.data, dr.ctypes.data, int(dv.shape[0]), out.ctypes.data))
    return out


class Caller(Handle):
    """One (BAM, chromosome)'s ``hello_sv`` handle: ``add`` takes the reads overlapping a span, ``finish`` clusters and genotypes,
    ``arrays`` gives the SIGNATURES columns, after ``finish`` the CANDIDATES columns, and the STATUS of the last ``add``; once
    ``set_contigs`` was called also CANDIDATES_SR and the SPLIT_STATUS of the last ``add``."""
    NAME, STAT_NAMES, TIMES = "sv", STAT_NAMES, TIME_NAMES
    ARRAYS = (tuple(("SIGNATURES_" + name, i, np.int64, None) for i, name in enumerate(SIGNATURE_COLUMNS))
              + tuple(("CANDIDATES_" + name, 8 + i, np.int64, None) for i, name in enumerate(CANDIDATE_COLUMNS))
              + (("STATUS", 28, np.uint8, None), ("CANDIDATES_SR", 29, np.int64, None), ("SPLIT_STATUS", 30, np.uint8, None)))

    def __init__(self, ref, min_size: int = MIN_SIZE, flank: int = FLANK, mapq_threshold: int = 10, device: int = 0,
                 cluster_gap: int = CLUSTER_GAP, len_ratio_percent: int = percent_of(LEN_RATIO), min_support: int = MIN_SUPPORT):
        ref = np.ascontiguousarray(_bytes_of(ref))
        super().__init__(_lib())
        self.finished = self.split = False
        self.clustering = (int(cluster_gap), int(len_ratio_percent), int(min_support))
        check(self._lib.hello_sv_create(ref.ctypes.data, int(ref.shape[0]), int(min_size), int(flank), int(mapq_threshold), int(device),
                                        C.byref(self._h)))

    def set_contigs(self, names: Sequence[str], own: int) -> None:
        """The names of the BAM header's sequences and the index of this chromosome among them: once, before the first add with
        ``splits``."""
        table = (C.c_char_p * len(names))(*[name.encode() for name in names])
        check(self._lib.hello_sv_contigs(self._h, table, len(names), int(own)))
        self.split = True

    def add(self, reads: Reads, *span, splits: Optional[Splits] = None) -> None:
        """``add(reads, lo, hi)``, ``add(reads, lo, hi, splits=...)`` or, as ``measure_spans`` calls it, ``add(reads, splits, lo, hi)``."""
        if len(span) == 3:
            splits, span = span[0], span[1:]
        lo, hi = span
        if splits is None:
            check(self._lib.hello_sv_add(self._h, *reads.pointers(reads.hp), int(reads.n_reads), int(lo), int(hi)))
            return
        text, offsets = np.ascontiguousarray(splits.bytes, np.uint8), np.ascontiguousarray(splits.offsets, np.int64)
        if offsets.shape[0] != reads.n_reads + 1:
            raise ValueError(f"{offsets.shape[0]} SA offsets for {reads.n_reads} reads")
        check(self._lib.hello_sv_add_split(self._h, *reads.pointers(reads.hp), text.ctypes.data, offsets.ctypes.data, int(text.shape[0]),
                                           int(reads.n_reads), int(lo), int(hi)))

    def finish(self, cluster_gap: Optional[int] = None, len_ratio_percent: Optional[int] = None, min_support: Optional[int] = None) -> None:
        given = (cluster_gap, len_ratio_percent, min_support)
        check(self._lib.hello_sv_finish(self._h, *[int(d if g is None else g) for g, d in zip(given, self.clustering)]))
        self.finished = True

    def _has(self, name: str) -> bool:
        """The CANDIDATES columns exist after ``finish``; SR and SPLIT_STATUS are handed out once ``set_contigs`` was called."""
        if name in ("CANDIDATES_SR", "SPLIT_STATUS") and not self.split:
            return False
        return self.finished or not name.startswith("CANDIDATES_")

    def results(self):
        """After the last add: finishes with the handle's own clustering values where nobody has yet."""
        if not self.finished:
            self.finish()
        return self.arrays(), self.stats()


def found_on_gpu(spans: Sequence[tuple], ref, min_size: int = MIN_SIZE, flank: int = FLANK, mapq_threshold: int = 10,
                 cluster_gap: int = CLUSTER_GAP, len_ratio_percent: int = percent_of(LEN_RATIO), min_support: int = MIN_SUPPORT,
                 device: int = 0, contigs: Optional[Sequence[str]] = None, own: Optional[int] = None) -> Tuple[Dict[str, np.ndarray], Dict[str, float]]:
    """``restated`` on the GPU: ({SIGNATURES_*, CANDIDATES_*, STATUS and SPLIT_STATUS of the last span}, the statistics of
    ``hello_sv_stats``)."""
    with Caller(ref, min_size, flank, mapq_threshold, device, cluster_gap, len_ratio_percent, min_support) as caller:
        if contigs is not None:
            caller.set_contigs(contigs, own)
        for span in spans:
            caller.add(*span)
        return caller.results()


def clustered_native(signatures: Sequence[Sequence[int]], cluster_gap: int = CLUSTER_GAP,
                     len_ratio_percent: int = percent_of(LEN_RATIO), min_support: int = MIN_SUPPORT) -> List[Tuple[int, ...]]:
    """``clustered`` from ``hello_sv_cluster``, the host rules ``hello_sv_finish`` runs (csrc/sv.h; host only: no device is opened)."""
    rows = np.ascontiguousarray(np.array(signatures, np.int64).reshape(-1, len(SIGNATURE_COLUMNS)))
    out, n = np.zeros((rows.shape[0], len(CLUSTER_COLUMNS)), np.int64), C.c_int64()
    check(_lib().hello_sv_cluster(rows.ctypes.data, int(rows.shape[0]), int(cluster_gap), int(len_ratio_percent), int(min_support),
                                  out.ctypes.data, C.byref(n)))
    return [tuple(int(v) for v in row) for row in out[:n.value]]


def clustered_split_native(signatures: Sequence[Sequence[int]], cluster_gap: int = CLUSTER_GAP,
                           len_ratio_percent: int = percent_of(LEN_RATIO), min_support: int = MIN_SUPPORT) -> List[Tuple[int, ...]]:
    """``clustered(..., with_sr=True)`` over rows of the types 0 to 4 from ``hello_sv_cluster_split`` (host only)."""
    rows = np.ascontiguousarray(np.array(signatures, np.int64).reshape(-1, len(SIGNATURE_COLUMNS)))
    out, n = np.zeros((rows.shape[0], len(CLUSTER_COLUMNS) + 1), np.int64), C.c_int64()
    check(_lib().hello_sv_cluster_split(rows.ctypes.data, int(rows.shape[0]), int(cluster_gap), int(len_ratio_percent), int(min_support),
                                        out.ctypes.data, C.byref(n)))
    return [tuple(int(v) for v in row) for row in out[:n.value]]


# ------------------------------------------------------------------------------------------------
# the events of one BAM
# ------------------------------------------------------------------------------------------------
VCF_HEADER = (
    '##ALT=<ID=DEL,Description="Deletion inside one alignment record">\n'
    '##ALT=<ID=INS,Description="Insertion inside one alignment record">\n'
    '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of the event">\n'
    '##INFO=<ID=SVLEN,Number=1,Type=Integer,Description="Length of the event, negative for a deletion">\n'
    '##INFO=<ID=END,Number=1,Type=Integer,Description="Last reference base of the event">\n'
    '##INFO=<ID=SUPPORT,Number=1,Type=Integer,Description="Distinct reads that show the event">\n'
    '##INFO=<ID=CIPOS,Number=2,Type=Integer,Description="Least and greatest position of the supporting signatures, relative to POS">\n'
    '##INFO=<ID=CILEN,Number=2,Type=Integer,Description="Least and greatest length of the supporting signatures, relative to SVLEN">\n'
    '##INFO=<ID=STRANDS,Number=2,Type=Integer,Description="Supporting reads on the forward and on the reverse strand">\n'
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
    '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">\n'
    '##FORMAT=<ID=DR,Number=1,Type=Integer,Description="Spanning reads without the event">\n'
    '##FORMAT=<ID=DV,Number=1,Type=Integer,Description="Reads that show the event">\n'
    '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods">\n'
    '##FORMAT=<ID=HPS,Number=3,Type=Integer,Description="Supporting reads without a haplotype, of haplotype 1 and of haplotype 2">\n'
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE1\n")


SPLIT_VCF_HEADER = VCF_HEADER.replace(
    '##INFO=<ID=SVTYPE', '##ALT=<ID=DUP,Description="Tandem duplication, from split alignments">\n'
                         '##ALT=<ID=INV,Description="Inversion junction, from split alignments">\n##INFO=<ID=SVTYPE').replace(
    '##FORMAT=<ID=GT', '##INFO=<ID=SR,Number=1,Type=Integer,Description="Supporting reads that show the event as a split alignment">\n'
                       '##INFO=<ID=JUNCTION,Number=1,Type=String,Description="The ends an inversion junction joins: 3to3 or 5to5">\n'
                       '##FORMAT=<ID=GT').replace(
    "inside one alignment record", "inside one alignment record or between the segments of a split alignment")


def vcf_line(chromosome: str, ref: np.ndarray, c: Dict[str, int], split: bool = False) -> str:
    """One candidate (a dict over CANDIDATE_COLUMNS; ``split``: and SR).  POS is ``pos``, the 1-based base before the event; an
    event at position 0 has none and is written at POS 0 with REF N."""
    pos, n, kind = c["POS"], c["LEN"], c["TYPE"]
    base = chr(int(ref[pos - 1])) if pos >= 1 else "N"
    info = "SVTYPE=%s;SVLEN=%d;END=%d;SUPPORT=%d;CIPOS=%d,%d;CILEN=%d,%d;STRANDS=%d,%d" % (
        SPLIT_TYPE_NAMES[kind], -n if kind == DEL else n, pos if kind == INS else pos + n, c["DV"], c["POS_MIN"] - pos, c["POS_MAX"] - pos,
        c["LEN_MIN"] - n, c["LEN_MAX"] - n, c["DV_FWD"], c["DV_REV"])
    if split:
        info += ";SR=%d" % c["SR"] + (";JUNCTION=%s" % ("3to3" if kind == INV3 else "5to5") if kind in (INV3, INV5) else "")
    sample = "%s:%d:%d:%d:%d,%d,%d:%d,%d,%d" % (GT_TEXT[c["GT"]], c["GQ"], c["DR"], c["DV"], c["PL0"], c["PL1"], c["PL2"], c["HP0"],
                                                 c["HP1"], c["HP2"])
    return "%s\t%d\t.\t%s\t<%s>\t.\tPASS\t%s\tGT:GQ:DR:DV:PL:HPS\t%s\n" % (chromosome, pos, base, SPLIT_TYPE_NAMES[kind], info, sample)


class Events:
    """``tables[chromosome]``: the SIGNATURES_* and CANDIDATES_* columns (int64) and STATS (int64, METRIC_STATS); ``refs``: the
    chromosomes' texts, ``lengths`` their lengths.  ``split``: of a run with split alignments -- CANDIDATES_SR is kept, STATS is
    SPLIT_METRIC_STATS and the VCF has the lines of section 7q."""

    def __init__(self, split: bool = False):
        self.split = bool(split)
        self.stat_names = SPLIT_METRIC_STATS if split else METRIC_STATS
        self.candidate_columns = CANDIDATE_COLUMNS + (("SR",) if split else ())
        self.tables: Dict[str, Dict[str, np.ndarray]] = {}
        self.refs: Dict[str, np.ndarray] = {}

    def set(self, chromosome: str, ref: np.ndarray, tables: Dict[str, np.ndarray], counts: Dict[str, float]) -> None:
        names = ["SIGNATURES_" + c for c in SIGNATURE_COLUMNS] + ["CANDIDATES_" + c for c in self.candidate_columns]
        kept = {k: np.asarray(tables[k], np.int64) for k in names}
        kept["STATS"] = np.array([int(counts[k]) for k in self.stat_names], np.int64)
        self.tables[chromosome], self.refs[chromosome] = kept, ref

    def total(self) -> Dict[str, int]:
        return {k: sum(int(t["STATS"][i]) for t in self.tables.values()) for i, k in enumerate(self.stat_names)}

    def candidates(self, chromosome: str) -> List[Dict[str, int]]:
        t = self.tables[chromosome]
        return [{name: int(t["CANDIDATES_" + name][i]) for name in self.candidate_columns} for i in range(t["CANDIDATES_POS"].shape[0])]

    def vcf_text(self) -> str:
        out = ["##fileformat=VCFv4.2\n"] + ["##contig=<ID=%s,length=%d>\n" % (c, self.refs[c].shape[0]) for c in self.tables]
        out.append(SPLIT_VCF_HEADER if self.split else VCF_HEADER)
        for c in self.tables:
            out += [vcf_line(c, self.refs[c], row, self.split) for row in self.candidates(c)]
        return "".join(out)

    def save(self, path: str) -> str:
        names = list(self.tables)
        out = dict(chromosomes=np.array(names, dtype=np.str_))
        for i, c in enumerate(names):
            for name, a in self.tables[c].items():
                out["%s_%d" % (name, i)] = a
        return save_tables(path, out)

    def write_all(self, prefix: str) -> List[str]:
        """``<prefix>.vcf`` and ``<prefix>.npz``."""
        with open(prefix + ".vcf", "w") as fh:
            fh.write(self.vcf_text())
        return [prefix + ".vcf", self.save(prefix + ".npz")]


def measure(bam: str, fasta, chromosomes: Optional[Sequence[str]] = None, haplotagger=None, min_size: int = MIN_SIZE, flank: int = FLANK,
            mapq_threshold: int = 10, cluster_gap: int = CLUSTER_GAP, len_ratio_percent: int = percent_of(LEN_RATIO),
            min_support: int = MIN_SUPPORT, max_span: Optional[int] = None, device: int = 0, restatement: bool = False,
            stats: Optional[dict] = None, split: bool = False) -> Events:
    """The events of one BAM, chromosome after chromosome (default: every sequence of the FASTA).  ``fasta``: a path, or
    {chromosome: sequence}; ``haplotagger``: its ``retag(chromosome, reads)`` replaces the BAM's own HP; ``restatement``: from the
    plain-Python rules instead of the GPU.  ``stats``: the library's kernel times and the seconds of decoding (``decode_s``), of
    the library's calls (``device_s``) and of the whole pass (``total_s``) are added.  ``split``: the reads come with their SA tags
    (``fetch_with_sa``) and the junctions of the split alignments are rows too; the contigs are the BAM header's sequences."""
    out = Events(split)
    contigs: Optional[List[str]] = None
    if split:
        from .bam import BamFile
        with BamFile(bam) as source:
            contigs = [name for name, _ in source.references]

    def open_handle(c, ref):
        caller = Caller(ref, min_size, flank, mapq_threshold, device, cluster_gap, len_ratio_percent, min_support)
        if split:
            try:
                caller.set_contigs(contigs, contigs.index(c))
            except Exception:
                caller.close()
                raise
        return caller

    measure_spans(bam, fasta, chromosomes, max_span, stats, restatement, open_handle=open_handle,
                  restated=lambda c, ref, spans: restated(spans, ref, min_size, flank, mapq_threshold, cluster_gap, len_ratio_percent,
                                                          min_support, contigs, contigs.index(c) if split else None),
                  done=lambda c, ref, tables, counts: out.set(c, ref, tables, counts),
                  retag=haplotagger.retag if haplotagger is not None else None, with_sa=split)
    return out


def add_options(p: argparse.ArgumentParser, given_or_none: bool = False) -> None:
    """The ``--sv_*`` options; ``given_or_none``: an absent option is None, for a caller that must tell it from a given one."""
    pick = lambda v: None if given_or_none else v                   # noqa: E731
    p.add_argument("--sv_min_size", type=int, default=pick(MIN_SIZE), help="--sv: the fewest bases of an I or D operation (default %d)" % MIN_SIZE)
    p.add_argument("--sv_min_support", type=int, default=pick(MIN_SUPPORT), help="--sv: the fewest distinct reads of an event (default %d)" % MIN_SUPPORT)
    p.add_argument("--sv_flank", type=int, default=pick(FLANK),
                   help="--sv: the reference bases of the read an operation keeps on both sides (default %d)" % FLANK)
    p.add_argument("--sv_cluster_gap", type=int, default=pick(CLUSTER_GAP),
                   help="--sv: signatures whose positions lie farther apart start a new run (default %d)" % CLUSTER_GAP)
    p.add_argument("--sv_len_ratio", type=float, default=pick(LEN_RATIO),
                   help="--sv: the least ratio of two neighbouring lengths of one event (default %.1f)" % LEN_RATIO)


def check_options(min_size, min_support, flank, cluster_gap, len_ratio) -> None:
    """The refusals of the ``--sv_*`` values, each naming the fix."""
    if min_size < 1:
        raise SystemExit("--sv_min_size is the fewest bases of an event: give 1 or more")
    if min_support < 1:
        raise SystemExit("--sv_min_support is the fewest distinct reads of an event: give 1 or more")
    if flank < 1:
        raise SystemExit("--sv_flank is the reference bases a read keeps on both sides of an event: give 1 or more")
    if cluster_gap < 0:
        raise SystemExit("--sv_cluster_gap is a distance between positions: give 0 or more")
    if not 1 <= percent_of(len_ratio) <= 100:
        raise SystemExit("--sv_len_ratio is the least ratio of two lengths of one event: give 0.01 to 1")


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Large deletions and insertions of coordinate-sorted BAMs from the reads' CIGARs, found on the GPU")
    p.add_argument("--bam", required=True, help="The BAM (with its .bai, or scanned); B,P: two BAMs, each with files of its own")
    p.add_argument("--ref", required=True, help="Reference FASTA")
    p.add_argument("--output_prefix", required=True, help="Writes <prefix>.vcf and <prefix>.npz; with two BAMs <prefix>.1.* and <prefix>.2.*")
    p.add_argument("--phased_vcf", help="A phased VCF (a|b records with PS): the reads' haplotypes come from it, not from the HP tags")
    p.add_argument("--chromosomes", help="Comma-separated chromosomes (default: every sequence of the FASTA)")
    p.add_argument("--mapq_threshold", type=int, default=10, help="A read below it does not count")
    add_options(p)
    p.add_argument("--split", action="store_true", default=False,
                   help="Also call deletions, insertions, duplications and inversions from split alignments (the SA tags; DESIGN.md 7q)")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def main(argv=None) -> List[str]:
    from .call import read_fasta
    args = parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)-15s %(message)s")
    check_options(args.sv_min_size, args.sv_min_support, args.sv_flank, args.sv_cluster_gap, args.sv_len_ratio)
    chromosomes = args.chromosomes.split(",") if args.chromosomes else None
    genome = read_fasta(args.ref, chromosomes)
    bams = args.bam.split(",")
    if not 1 <= len(bams) <= 2:
        raise SystemExit("--bam takes one BAM, or two separated by a comma")
    tagger = None
    if args.phased_vcf:
        from .haplotag import Haplotagger
        tagger = Haplotagger(args.phased_vcf, chromosomes, 10, args.mapq_threshold, args.device)
    written: List[str] = []
    try:
        for n, bam in enumerate(bams):
            stats: dict = {}
            found = measure(bam, genome, chromosomes, tagger, args.sv_min_size, args.sv_flank, args.mapq_threshold, args.sv_cluster_gap,
                            percent_of(args.sv_len_ratio), args.sv_min_support, device=args.device, stats=stats, split=args.split)
            written += found.write_all(args.output_prefix + (".%d" % (n + 1) if len(bams) > 1 else ""))
            total = found.total()
            _log.info("%s: %d reads counting, %d walked, %d signatures, %d events (kernels %.1f ms)", os.path.basename(bam),
                      total["counting"], total["walked"], total["signatures"], total["candidates"],
                      sum(stats.get(k, 0.0) for k in TIME_NAMES))
    finally:
        if tagger is not None:
            tagger.close()
    return written


if __name__ == "__main__":
    main(sys.argv[1:])
