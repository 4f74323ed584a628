"""Large deletions and insertions of sorted BAMs from the reads' own CIGARs, found on the GPU.

    python -m hello_amd.call --from_bam | --from_bams [--resident] ... --sv [--sv_min_size 50] [--sv_min_support 3] [--sv_flank 20]
                             [--sv_cluster_gap 100] [--sv_len_ratio 0.7] [--sv_split]
                             [--sv_pairs [--sv_pairs_library M,LO,HI] [--sv_pairs_k 8] [--sv_clip_min 20]]
    python -m hello_amd.sv --bam B[,P] --ref F --output_prefix P [--phased_vcf V] [--chromosomes a,b] [--mapq_threshold 10]
                           [--sv_min_size 50] ... [--split] [--pairs [--pairs_library M,LO,HI] [--pairs_k 8] [--clip_min 20]]
                           [--device N]

Not in the reference; DESIGN.md section 7p defines the rules.  By default intra-alignment events only: an ``I`` or ``D`` operation of
at least ``min_size`` bases inside one alignment record.  With ``--sv_split`` / ``--split`` (section 7q) the ``SA`` tags are read too and
every junction between two segments of a split alignment is a row as well (DEL, INS, DUP, INV, BND): ``segments_of``, ``junctions_of``
and ``split_rows_of`` restate those rules.  With ``--sv_pairs`` / ``--pairs`` (section 7s) the mate fields are read as well: a pair
whose mates lie too far apart, face the wrong way or sit on two chromosomes is a row (DEL, DUP, INV, BND), pair rows support the
clusters of the other rows or form imprecise clusters of their own, and soft-clipped ends near a candidate are counted
(``pair_counted``, ``pair_rows_of``, ``library_of``, ``assigned``, ``clustered_pairs``).  Still not looked at: the mate's mapping
quality, pairs that support the reference, insertions from short inserts, pairing the two BNDs of a translocation, assembly and
joint calls over two BAMs.  ``signatures_of``, ``restated``, ``clustered`` and ``genotyped`` restate the rules in plain
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

from ._abi import ARRAY_GETTER, READS, STATS_GETTER, bind, check, handle_array, handle_stats, i32, i64, vp
from .bam import Mates, Reads, Splits
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

# discordant pairs and clipped ends
PAIR_OP = -16                                               # the OP column of a pair row
INNER_BINS, INNER_ZERO = 4096, 1024
MATE_MAX_POS = (1 << 31) - 1
UNSET_LIBRARY = (0, -(1 << 31), (1 << 31) - 1)
PAIRS_K, CLIP_MIN, LIBRARY_MIN_PAIRS, LIBRARY_SAMPLE = 8, 20, 100, 10000
PAIR_STATUS_NAMES = ("not_pair_counted", "bad_mate", "right", "normal", "short", "small", "unplaced", "with_a_row", "with_a_bnd_row")
NOT_PAIR, BAD_MATE, RIGHT, NORMAL, SHORT, SMALL, UNPLACED, PAIR_ROW, PAIR_BND_ROW = range(9)
PAIR_COUNT_NAMES = ("pair_reads", "pairs_left", "pairs_right", "pairs_normal", "pairs_short", "pairs_small", "pairs_unplaced", "bad_mate",
                    "pair_signatures", "clipped_reads", "pairs_assigned", "pair_candidates")
PAIR_STAT_NAMES = PAIR_COUNT_NAMES + ("pairs_ms",)
PAIR_METRIC_STATS = SPLIT_METRIC_STATS + PAIR_COUNT_NAMES
PAIR_CANDIDATE_COLUMNS = ("PR", "CE", "END_MIN", "END_MAX", "IMPRECISE")
CLUSTER_PAIRS_COLUMNS = CLUSTER_COLUMNS + ("SR",) + ("PR", "END_MIN", "END_MAX", "IMPRECISE")

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
# the rules of the read pairs and the clipped ends, restated
# ------------------------------------------------------------------------------------------------
def pair_counted(flag: int, mapq: int, mapq_threshold: int) -> bool:
    """Paired, mapped with a mapped mate, primary, no duplicate, not QC-fail, at the threshold; flag 0x2 is not consulted."""
    return bool(flag & 0x1) and not flag & (0x4 | 0x8 | 0x100 | 0x800 | 0x400 | 0x200) and mapq >= mapq_threshold


def clips_of(ops: Sequence[Tuple[int, int]], clip_min: int) -> int:
    """Bit 0: the leading soft clip (the first operation, or the second behind an H) has ``clip_min`` bases; bit 1: the trailing."""
    if not ops:
        return 0
    i = 1 if ops[0][0] == 5 else 0
    j = len(ops) - 2 if ops[-1][0] == 5 else len(ops) - 1
    found = 1 if i < len(ops) and ops[i][0] == 4 and ops[i][1] >= clip_min else 0
    return found | (2 if j > i and ops[j][0] == 4 and ops[j][1] >= clip_min else 0)


def pair_outcome(flag: int, s: int, e: int, own: int, mt: int, ms: int, n_contigs: int, library: Tuple[int, int, int],
                 min_size: int) -> Tuple[int, Optional[int], Optional[Tuple[int, int, int, int]]]:
    """One belonging, pair-counted record with valid mate fields -> (PAIR_STATUS, its INNER bin or None, (type, pos, len, shift) of
    its row or None)."""
    median, lo, hi = library
    rev, mrev = bool(flag & 0x10), bool(flag & 0x20)
    if mt != own:
        if not 0 <= mt < n_contigs:
            return UNPLACED, None, None
        return PAIR_BND_ROW, None, (BND, s if rev else e, mt, ms)
    if not (s < ms or (s == ms and flag & 0x40)):
        return RIGHT, None, None
    at = None
    if not rev and mrev:
        g = ms - e
        at = min(max(g + INNER_ZERO, 0), INNER_BINS - 1)
        if g <= hi:
            return (SHORT if g < lo else NORMAL), at, None
        row = (DEL, e, g - median, ms)
    elif rev and not mrev:
        if ms < e:
            return SMALL, None, None
        row = (DUP, s, ms - s, ms)
    else:
        pos = s if rev else e
        row = (INV5 if rev else INV3, pos, abs(ms - pos), ms)
    return (PAIR_ROW, at, row) if min_size <= row[2] <= MATE_MAX_POS else (SMALL, at, None)


def pair_rows_of(reads: Reads, splits: Splits, mates: "Mates", lo: int, own: int, n_contigs: int, length: int, min_size: int,
                 mapq_threshold: int, library: Tuple[int, int, int], clip_min: int = CLIP_MIN, pairs_given: int = 0) -> Dict[str, object]:
    """One span that begins at ``lo`` with the reads overlapping it -> ``rows`` (of SIGNATURE_COLUMNS, OP = PAIR_OP, in the reads'
    order), ``inner`` ([bin] per left FR record), ``clip_left`` / ``clip_right`` ([position] per counting clip), ``status``
    (PAIR_STATUS per read) and ``counts`` (PAIR_COUNT_NAMES but the two of finish)."""
    rows: List[Tuple[int, ...]] = []
    inner: List[int] = []
    clip_left: List[int] = []
    clip_right: List[int] = []
    status = np.zeros(reads.n_reads, np.uint8)
    counts = dict.fromkeys(PAIR_COUNT_NAMES, 0)
    ordinal = pairs_given
    for r in range(reads.n_reads):
        s, e = int(reads.ref_starts[r]), int(reads.ref_ends[r])
        if s < lo:
            continue
        flag, mapq = int(reads.flags[r]), int(reads.mapq[r])
        if pair_counted(flag, mapq, mapq_threshold):
            counts["pair_reads"] += 1
            mt, ms = int(mates.tid[r]), int(mates.pos[r])
            if not (0 <= ms <= MATE_MAX_POS and (mt != own or ms <= length) and e <= length):
                status[r] = BAD_MATE
                counts["bad_mate"] += 1
            else:
                status[r], at, row = pair_outcome(flag, s, e, own, mt, ms, n_contigs, library, min_size)
                if at is not None:
                    inner.append(at)
                if row is not None:
                    rows.append(row[:2] + (row[2], row[3], ordinal, PAIR_OP, int(bool(flag & 0x10)), int(reads.hp[r])))
                key = {RIGHT: "pairs_right", NORMAL: "pairs_normal", SHORT: "pairs_short", SMALL: "pairs_small", UNPLACED: "pairs_unplaced"}
                if int(status[r]) in key:
                    counts[key[int(status[r])]] += 1
                counts["pairs_left"] += int(status[r]) in (NORMAL, SHORT, SMALL, PAIR_ROW)
            ordinal += 1
        if counted(flag, mapq, mapq_threshold) and splits.offsets[r + 1] == splits.offsets[r] and e <= length:
            ops = [(int(c) & 15, int(c) >> 4) for c in reads.cigars[int(reads.cigar_offsets[r]):int(reads.cigar_offsets[r + 1])]]
            found = clips_of(ops, clip_min)
            if found & 1:
                clip_right.append(s)
            if found & 2:
                clip_left.append(e)
            counts["clipped_reads"] += found != 0
    counts["pair_signatures"] = len(rows)
    return dict(rows=rows, inner=inner, clip_left=clip_left, clip_right=clip_right, status=status, counts=counts)


def _histogram_median(h: np.ndarray) -> int:
    """The lower median of the values a histogram counts."""
    total = int(h.sum())
    return int(np.searchsorted(np.cumsum(h), (total - 1) // 2 + 1))


def library_of(histogram, k: int = PAIRS_K) -> Tuple[int, int, int]:
    """INNER -> (median, lo, hi): the lower median, and k max(mad, 1) to either side, where mad is the lower median of the absolute
    deviations over the histogram without its two clamped bins.  Integer arithmetic throughout."""
    h = np.asarray(histogram, np.int64)
    if h.shape != (INNER_BINS,) or h.sum() == 0:
        raise ValueError("an empty histogram has no library")
    at = _histogram_median(h)
    dev = np.zeros(INNER_BINS, np.int64)
    for v in range(1, INNER_BINS - 1):
        dev[abs(v - at)] += h[v]
    mad = max(_histogram_median(dev), 1) if dev.sum() else 1
    return at - INNER_ZERO, at - INNER_ZERO - k * mad, at - INNER_ZERO + k * mad


def _cluster_end(c: Sequence[int]) -> int:
    return c[1] if c[0] == INS else c[1] + c[2]


def assigned(clusters: Sequence[Sequence[int]], pair_rows: Sequence[Sequence[int]], library: Tuple[int, int, int],
             flank: int) -> Tuple[List[int], List[Tuple[int, ...]]]:
    """Clusters (rows that begin with TYPE, POS, LEN) in (pos, type, len) order and pair rows sorted by (type, pos, len, ordinal) ->
    (PR per cluster, the pair rows no cluster took).  The first cluster that accepts a row takes it; a BND is never taken nor left."""
    _, lo, hi = library
    pr, left = [0] * len(clusters), []
    for g in pair_rows:
        kind, a, b = int(g[0]), int(g[1]), int(g[3])
        if kind >= BND:
            continue
        for i, c in enumerate(clusters):
            P, L = int(c[1]), int(c[2])
            if int(c[0]) != kind:
                continue
            if (a - flank <= P and P + L <= b + flank and lo <= (b - a) - L <= hi) if kind == DEL else (abs(a - P) <= hi and abs(b - (P + L)) <= hi):
                pr[i] += 1
                break
        else:
            left.append(tuple(int(v) for v in g))
    return pr, left


def clustered_pairs(rows: Sequence[Sequence[int]], library: Tuple[int, int, int], min_support: int = MIN_SUPPORT) -> List[Tuple[int, ...]]:
    """The pair rows no cluster took -> rows of CLUSTER_PAIRS_COLUMNS, in the order (type, first a) they are found."""
    _, lo, hi = library
    left = sorted((tuple(int(v) for v in g) for g in rows), key=lambda g: (g[0], g[1], g[3], g[4]))
    out, group, top, bottom = [], [], 0, 0

    def close():
        if len(group) < min_support:
            return
        a, b, n = sorted(g[1] for g in group), sorted(g[3] for g in group), sorted(g[2] for g in group)
        m = (len(group) - 1) // 2
        kind = group[0][0]
        out.append((kind, a[-1] if kind == DEL else a[m], n[m], 0, 0, 0, 0, 0, 0, a[0], a[-1], n[0], n[-1], 0, len(group), b[0], b[-1], 1))

    for g in left:
        x, y = min(g[1], g[3]), max(g[1], g[3])
        if group and not (g[0] == group[-1][0] and g[1] - group[-1][1] <= hi - lo and x <= bottom and y >= top):
            close()
            group = []
        top, bottom = (max(top, x), min(bottom, y)) if group else (x, y)
        group.append(g)
    close()
    return out


def clustered_with_pairs(signatures: Sequence[Sequence[int]], library: Tuple[int, int, int], flank: int, cluster_gap: int = CLUSTER_GAP,
                         len_ratio_percent: int = percent_of(LEN_RATIO), min_support: int = MIN_SUPPORT) -> Tuple[List[Tuple[int, ...]], int]:
    """Rows of SIGNATURE_COLUMNS of all kinds -> (rows of CLUSTER_PAIRS_COLUMNS sorted by (pos, type, len, imprecise), the pair rows a
    cluster took): what ``hello_sv_cluster_pairs`` computes."""
    rows = sorted((tuple(int(v) for v in g) for g in signatures), key=lambda g: (g[0], g[1], g[2], g[4], g[5]))
    plain, pairs = [g for g in rows if g[5] != PAIR_OP], [g for g in rows if g[5] == PAIR_OP]
    clusters = clustered(plain, cluster_gap, len_ratio_percent, min_support, with_sr=True)
    pr, left = assigned(clusters, pairs, library, flank)
    out = [c + (n, _cluster_end(c), _cluster_end(c), 0) for c, n in zip(clusters, pr)] + clustered_pairs(left, library, min_support)
    return sorted(out, key=lambda c: (c[1], c[0], c[2], c[17])), sum(pr)


def clip_sum(clip_left: np.ndarray, clip_right: np.ndarray, pos: int, end: int, flank: int) -> int:
    """CE: CLIP_LEFT + CLIP_RIGHT over [pos - flank, pos + flank] and what [end - flank, end + flank] adds to it, inside the arrays."""
    length = clip_left.shape[0] - 1
    lo1, hi1 = max(pos - flank, 0), min(pos + flank, length)
    lo2, hi2 = max(end - flank, 0, hi1 + 1), min(end + flank, length)
    both = np.asarray(clip_left, np.int64) + np.asarray(clip_right, np.int64)
    return int(both[lo1:hi1 + 1].sum()) + (int(both[lo2:hi2 + 1].sum()) if lo2 <= hi2 else 0)


def restated_pairs(spans: Sequence[tuple], ref, library: Tuple[int, int, int], contigs: Sequence[str], own: int, min_size: int = MIN_SIZE,
                   flank: int = FLANK, mapq_threshold: int = 10, cluster_gap: int = CLUSTER_GAP,
                   len_ratio_percent: int = percent_of(LEN_RATIO), min_support: int = MIN_SUPPORT,
                   clip_min: int = CLIP_MIN) -> Tuple[Dict[str, np.ndarray], Dict[str, int]]:
    """``restated`` for spans (reads, splits, mates, lo, hi): the tables of a handle whose every add is ``hello_sv_add_pairs`` -- and
    INNER, CLIP_LEFT, CLIP_RIGHT, PAIR_STATUS of the last span, CANDIDATES_PR .. CANDIDATES_IMPRECISE -- and the counts of both
    getters."""
    ref = _bytes_of(ref)
    length = int(ref.shape[0])
    diff = np.zeros(length + 1, np.int64)
    counts = dict.fromkeys(COUNT_NAMES + SPLIT_COUNT_NAMES + PAIR_COUNT_NAMES, 0)
    inner = np.zeros(INNER_BINS, np.int64)
    clip_left, clip_right = np.zeros(length + 1, np.int32), np.zeros(length + 1, np.int32)
    rows: List[Tuple[int, ...]] = []
    status = split_status = pair_status = np.zeros(0, np.uint8)
    for reads, splits, mates, lo, hi in spans:
        part = signatures_of(reads, ref, lo, hi, min_size, flank, mapq_threshold, counts["counting"], splits, contigs, own)
        more = pair_rows_of(reads, splits, mates, lo, own, len(contigs), length, min_size, mapq_threshold, library, clip_min,
                            counts["pair_reads"])
        rows += part["signatures"] + more["rows"]
        for at, by in part["cover"]:
            diff[at] += by
        np.add.at(inner, np.array(more["inner"], np.int64), 1)
        np.add.at(clip_left, np.array(more["clip_left"], np.int64), 1)
        np.add.at(clip_right, np.array(more["clip_right"], np.int64), 1)
        for k, v in list(part["counts"].items()) + list(more["counts"].items()):
            counts[k] += v
        status, split_status, pair_status = part["status"], part["split_status"], more["status"]
    rows.sort(key=lambda g: (g[0], g[1], g[2], g[4], g[5]))
    clusters, counts["pairs_assigned"] = clustered_with_pairs(rows, library, flank, cluster_gap, len_ratio_percent, min_support)
    spanning = np.cumsum(diff)
    found = []
    for c in clusters:
        dp = int(spanning[c[1]])
        dr = max(0, dp - (c[3] - c[13]))
        end = c[15] if c[17] and c[0] == DEL else _cluster_end(c)
        found.append(c[:13] + (dp, dr) + genotype_of(c[3] + c[14], dr) + (c[13], c[14], clip_sum(clip_left, clip_right, c[1], end, flank))
                     + c[15:])
    counts["candidates"] = len(found)
    counts["pair_candidates"] = sum(c[17] for c in clusters)
    tables = dict(_columns(rows, SIGNATURE_COLUMNS, "SIGNATURES_"),
                  **_columns(found, CANDIDATE_COLUMNS + ("SR",) + PAIR_CANDIDATE_COLUMNS, "CANDIDATES_"))
    tables.update(STATUS=status, SPLIT_STATUS=split_status, PAIR_STATUS=pair_status, DIFF=diff, INNER=inner, CLIP_LEFT=clip_left,
                  CLIP_RIGHT=clip_right)
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
    ("hello_sv_library", [vp, i32, i32, i32]),
    ("hello_sv_clip_min", [vp, i32]),
    ("hello_sv_add_pairs", [vp] + READS + [vp, vp, i64, vp, vp, i64, i64, i64]),
    ("hello_sv_pairs_array", ARRAY_GETTER),
    ("hello_sv_pairs_stats", STATS_GETTER),
    ("hello_sv_cluster_pairs", [vp, i64, i64, i32, i32, i32, i32, i32, i32, vp, C.POINTER(i64)]),
    ("hello_sv_library_of", [vp, i64, vp]),
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
    PAIR_ARRAYS = ((("INNER", 0, np.int64), ("CLIP_LEFT", 1, np.int32), ("CLIP_RIGHT", 2, np.int32), ("PAIR_STATUS", 3, np.uint8))
                   + tuple(("CANDIDATES_" + name, 4 + i, np.int64) for i, name in enumerate(PAIR_CANDIDATE_COLUMNS)))

    def __init__(self, ref, min_size: int = MIN_SIZE, flank: int = FLANK, mapq_threshold: int = 10, device: int = 0,
                 cluster_gap: int = CLUSTER_GAP, len_ratio_percent: int = percent_of(LEN_RATIO), min_support: int = MIN_SUPPORT):
        ref = np.ascontiguousarray(_bytes_of(ref))
        super().__init__(_lib())
        self.finished = self.split = self.pairs = False
        self.clustering = (int(cluster_gap), int(len_ratio_percent), int(min_support))
        check(self._lib.hello_sv_create(ref.ctypes.data, int(ref.shape[0]), int(min_size), int(flank), int(mapq_threshold), int(device),
                                        C.byref(self._h)))

    def set_contigs(self, names: Sequence[str], own: int) -> None:
        """The names of the BAM header's sequences and the index of this chromosome among them: once, before the first add with
        ``splits``."""
        table = (C.c_char_p * len(names))(*[name.encode() for name in names])
        check(self._lib.hello_sv_contigs(self._h, table, len(names), int(own)))
        self.split = True

    def set_library(self, median: int, lo: int, hi: int, clip_min: Optional[int] = None) -> None:
        """The library's inner distances, or ``UNSET_LIBRARY``: once, before the first add with ``mates``."""
        check(self._lib.hello_sv_library(self._h, int(median), int(lo), int(hi)))
        if clip_min is not None:
            check(self._lib.hello_sv_clip_min(self._h, int(clip_min)))
        self.pairs = True

    def add(self, reads: Reads, *span, splits: Optional[Splits] = None, mates: Optional[Mates] = None) -> None:
        """``add(reads, lo, hi)``, ``add(reads, lo, hi, splits=...[, mates=...])`` or, as ``measure_spans`` calls it,
        ``add(reads, splits, lo, hi)`` and ``add(reads, splits, mates, lo, hi)``."""
        if len(span) == 4:
            splits, mates, span = span[0], span[1], span[2:]
        elif len(span) == 3:
            splits, span = span[0], span[1:]
        lo, hi = span
        if mates is not None:
            text, offsets = np.ascontiguousarray(splits.bytes, np.uint8), np.ascontiguousarray(splits.offsets, np.int64)
            tid, pos = np.ascontiguousarray(mates.tid, np.int32), np.ascontiguousarray(mates.pos, np.int64)
            if offsets.shape[0] != reads.n_reads + 1 or tid.shape[0] != reads.n_reads or pos.shape[0] != reads.n_reads:
                raise ValueError(f"{offsets.shape[0]} SA offsets, {tid.shape[0]} and {pos.shape[0]} mate fields for {reads.n_reads} reads")
            check(self._lib.hello_sv_add_pairs(self._h, *reads.pointers(reads.hp), text.ctypes.data, offsets.ctypes.data, int(text.shape[0]),
                                               tid.ctypes.data, pos.ctypes.data, int(reads.n_reads), int(lo), int(hi)))
            return
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

    def arrays(self) -> Dict[str, np.ndarray]:
        out = super().arrays()
        if self.pairs:
            out.update({name: handle_array(self._lib.hello_sv_pairs_array, self._h, which, dtype)
                        for name, which, dtype in self.PAIR_ARRAYS if self._has(name)})
        return out

    def stats(self) -> Dict[str, float]:
        out = super().stats()
        if self.pairs:
            out.update(handle_stats(self._lib.hello_sv_pairs_stats, self._h, PAIR_STAT_NAMES))
        return out

    def results(self):
        """After the last add: finishes with the handle's own clustering values where nobody has yet."""
        if not self.finished:
            self.finish()
        return self.arrays(), self.stats()


def found_on_gpu(spans: Sequence[tuple], ref, min_size: int = MIN_SIZE, flank: int = FLANK, mapq_threshold: int = 10,
                 cluster_gap: int = CLUSTER_GAP, len_ratio_percent: int = percent_of(LEN_RATIO), min_support: int = MIN_SUPPORT,
                 device: int = 0, contigs: Optional[Sequence[str]] = None, own: Optional[int] = None,
                 library: Optional[Tuple[int, int, int]] = None, clip_min: Optional[int] = None) -> Tuple[Dict[str, np.ndarray], Dict[str, float]]:
    """``restated`` on the GPU: ({SIGNATURES_*, CANDIDATES_*, STATUS and SPLIT_STATUS of the last span}, the statistics of
    ``hello_sv_stats``)."""
    with Caller(ref, min_size, flank, mapq_threshold, device, cluster_gap, len_ratio_percent, min_support) as caller:
        if contigs is not None:
            caller.set_contigs(contigs, own)
        if library is not None:
            caller.set_library(*library, clip_min=clip_min)
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


def clustered_pairs_native(signatures: Sequence[Sequence[int]], library: Tuple[int, int, int], flank: int, cluster_gap: int = CLUSTER_GAP,
                           len_ratio_percent: int = percent_of(LEN_RATIO), min_support: int = MIN_SUPPORT) -> List[Tuple[int, ...]]:
    """``clustered_with_pairs(...)[0]`` from ``hello_sv_cluster_pairs`` (host only)."""
    rows = np.ascontiguousarray(np.array(signatures, np.int64).reshape(-1, len(SIGNATURE_COLUMNS)))
    out, n = np.zeros((rows.shape[0], len(CLUSTER_PAIRS_COLUMNS)), np.int64), C.c_int64()
    check(_lib().hello_sv_cluster_pairs(rows.ctypes.data, int(rows.shape[0]), int(cluster_gap), int(len_ratio_percent), int(min_support),
                                        int(library[0]), int(library[1]), int(library[2]), int(flank), out.ctypes.data, C.byref(n)))
    return [tuple(int(v) for v in row) for row in out[:n.value]]


def library_of_native(histogram, k: int = PAIRS_K) -> Tuple[int, int, int]:
    """``library_of`` from ``hello_sv_library_of`` (host only)."""
    h, out = np.ascontiguousarray(histogram, np.int64), np.zeros(3, np.int64)
    if h.shape != (INNER_BINS,):
        raise ValueError(f"a histogram of {INNER_BINS} bins")
    check(_lib().hello_sv_library_of(h.ctypes.data, int(k), out.ctypes.data))
    return tuple(int(v) for v in out)


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


PAIRS_VCF_HEADER = SPLIT_VCF_HEADER.replace(
    '##FORMAT=<ID=GT', '##INFO=<ID=PR,Number=1,Type=Integer,Description="Supporting read pairs whose mates lie too far apart or face the wrong way">\n'
                       '##INFO=<ID=CE,Number=1,Type=Integer,Description="Soft-clipped read ends within the flank of the two ends of the event">\n'
                       '##INFO=<ID=IMPRECISE,Number=0,Type=Flag,Description="Called from read pairs alone: POS and END bound the breakpoints">\n'
                       '##INFO=<ID=CIEND,Number=2,Type=Integer,Description="Least and greatest mate position of the supporting pairs, relative to END">\n'
                       '##FORMAT=<ID=GT').replace(
    "Distinct reads that show the event", "Distinct reads (DV) and read pairs (PR) that show the event").replace(
    "from split alignments", "from split alignments or read pairs")


def vcf_line(chromosome: str, ref: np.ndarray, c: Dict[str, int], split: bool = False, pairs: bool = False) -> str:
    """One candidate (a dict over CANDIDATE_COLUMNS; ``split``: and SR; ``pairs``: and PAIR_CANDIDATE_COLUMNS).  POS is ``pos``, the
    1-based base before the event; an event at position 0 has none and is written at POS 0 with REF N."""
    pos, n, kind = c["POS"], c["LEN"], c["TYPE"]
    base = chr(int(ref[pos - 1])) if pos >= 1 else "N"
    only = pairs and c["IMPRECISE"]
    end = c["END_MIN"] if only and kind == DEL else pos if kind == INS else pos + n
    info = "SVTYPE=%s;SVLEN=%d;END=%d;SUPPORT=%d;CIPOS=%d,%d;CILEN=%d,%d;STRANDS=%d,%d" % (
        SPLIT_TYPE_NAMES[kind], -n if kind == DEL else n, end, c["DV"] + (c["PR"] if pairs else 0), c["POS_MIN"] - pos, c["POS_MAX"] - pos,
        c["LEN_MIN"] - n, c["LEN_MAX"] - n, c["DV_FWD"], c["DV_REV"])
    if split:
        info += ";SR=%d" % c["SR"] + (";JUNCTION=%s" % ("3to3" if kind == INV3 else "5to5") if kind in (INV3, INV5) else "")
    if pairs:
        info += ";PR=%d;CE=%d" % (c["PR"], c["CE"]) + (";IMPRECISE;CIEND=%d,%d" % (c["END_MIN"] - end, c["END_MAX"] - end) if only else "")
    sample = "%s:%d:%d:%d:%d,%d,%d:%d,%d,%d" % (GT_TEXT[c["GT"]], c["GQ"], c["DR"], c["DV"], c["PL0"], c["PL1"], c["PL2"], c["HP0"],
                                                 c["HP1"], c["HP2"])
    return "%s\t%d\t.\t%s\t<%s>\t.\tPASS\t%s\tGT:GQ:DR:DV:PL:HPS\t%s\n" % (chromosome, pos, base, SPLIT_TYPE_NAMES[kind], info, sample)


class Events:
    """``tables[chromosome]``: the SIGNATURES_* and CANDIDATES_* columns (int64) and STATS (int64, METRIC_STATS); ``refs``: the
    chromosomes' texts, ``lengths`` their lengths.  ``split``: of a run with split alignments -- CANDIDATES_SR is kept, STATS is
    SPLIT_METRIC_STATS and the VCF has the lines of section 7q."""

    def __init__(self, split: bool = False, pairs: bool = False):
        self.pairs = bool(pairs)                     # a run with read pairs (section 7s) is one with split alignments too
        self.split = bool(split) or self.pairs
        self.library: Optional[Tuple[int, int, int]] = None      # of a pairs run, and how it was obtained
        self.library_source = ""
        self.stat_names = PAIR_METRIC_STATS if pairs else SPLIT_METRIC_STATS if split else METRIC_STATS
        self.candidate_columns = CANDIDATE_COLUMNS + (("SR",) if self.split else ()) + (PAIR_CANDIDATE_COLUMNS if pairs else ())
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
        out.append(PAIRS_VCF_HEADER if self.pairs else SPLIT_VCF_HEADER if self.split else VCF_HEADER)
        for c in self.tables:
            out += [vcf_line(c, self.refs[c], row, self.split, self.pairs) for row in self.candidates(c)]
        return "".join(out)

    def save(self, path: str) -> str:
        names = list(self.tables)
        out = dict(chromosomes=np.array(names, dtype=np.str_))
        if self.pairs:
            out.update(library=np.array(self.library, np.int64), library_source=np.array(self.library_source, dtype=np.str_))
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
            stats: Optional[dict] = None, split: bool = False, pairs: bool = False, library: Optional[Tuple[int, int, int]] = None,
            k: int = PAIRS_K, clip_min: int = CLIP_MIN) -> Events:
    """The events of one BAM, chromosome after chromosome (default: every sequence of the FASTA).  ``fasta``: a path, or
    {chromosome: sequence}; ``haplotagger``: its ``retag(chromosome, reads)`` replaces the BAM's own HP; ``restatement``: from the
    plain-Python rules instead of the GPU.  ``stats``: the library's kernel times and the seconds of decoding (``decode_s``), of
    the library's calls (``device_s``) and of the whole pass (``total_s``) are added.  ``split``: the reads come with their SA tags
    (``fetch_with_sa``) and the junctions of the split alignments are rows too; the contigs are the BAM header's sequences.
    ``pairs``: the reads come with their mate fields as well (``fetch_pairs``) and the rules of section 7s apply; ``library``:
    (median, lo, hi) of the inner distances, or None to sample it (``sampled_library``) with ``k``."""
    out = Events(split, pairs)
    contigs: Optional[List[str]] = None
    if pairs:
        if library is None:
            out.library = sampled_library(bam, fasta, chromosomes, min_size, flank, mapq_threshold, max_span, device, restatement, k)
            out.library_source = "sampled with k = %d" % k if out.library != UNSET_LIBRARY else "unset: the BAM has no paired reads"
        else:
            out.library, out.library_source = tuple(int(v) for v in library), "given"
        _log.info("%s: inner distances of the library: median %d, normal from %d to %d (%s)", os.path.basename(bam), *out.library,
                  out.library_source)
    if split or pairs:
        from .bam import BamFile
        with BamFile(bam) as source:
            contigs = [name for name, _ in source.references]

    def open_handle(c, ref):
        caller = Caller(ref, min_size, flank, mapq_threshold, device, cluster_gap, len_ratio_percent, min_support)
        if split or pairs:
            try:
                caller.set_contigs(contigs, contigs.index(c))
                if pairs:
                    caller.set_library(*out.library, clip_min=clip_min)
            except Exception:
                caller.close()
                raise
        return caller

    def restate(c, ref, spans):
        if pairs:
            return restated_pairs(spans, ref, out.library, contigs, contigs.index(c), min_size, flank, mapq_threshold, cluster_gap,
                                  len_ratio_percent, min_support, clip_min)
        return restated(spans, ref, min_size, flank, mapq_threshold, cluster_gap, len_ratio_percent, min_support, contigs,
                        contigs.index(c) if split else None)

    measure_spans(bam, fasta, chromosomes, max_span, stats, restatement, open_handle=open_handle, restated=restate,
                  done=lambda c, ref, tables, counts: out.set(c, ref, tables, counts),
                  retag=haplotagger.retag if haplotagger is not None else None, with_sa=split, with_pairs=pairs)
    return out


class LibraryError(ValueError):
    """A BAM with paired reads but too few forward-reverse pairs to sample a library from; the message names the fix."""


class _Sampled(Exception):
    """Ends the sampling pass once INNER holds enough pairs."""


def sampled_library(bam: str, fasta, chromosomes: Optional[Sequence[str]] = None, min_size: int = MIN_SIZE, flank: int = FLANK,
                    mapq_threshold: int = 10, max_span: Optional[int] = None, device: int = 0, restatement: bool = False,
                    k: int = PAIRS_K) -> Tuple[int, int, int]:
    """(median, lo, hi) of the BAM's own inner distances: the leading spans of the chromosomes in order go through a throw-away handle
    with the unset triple (under ``restatement`` through ``pair_rows_of``) until INNER holds LIBRARY_SAMPLE pairs or the BAM ends.
    A BAM without a single pair-counted read (PacBio) has no library and needs none: ``UNSET_LIBRARY``, under which it yields no
    pair row.  Paired reads but fewer than LIBRARY_MIN_PAIRS forward-reverse pairs: ``LibraryError``."""
    from .bam import BamFile
    with BamFile(bam) as source:
        contigs = [name for name, _ in source.references]
    inner = np.zeros(INNER_BINS, np.int64)
    pair_reads = [0]

    class Sampler:
        """What ``measure_spans`` takes for a handle; ``caller`` is the library's, or None under ``restatement``."""
        TIMES = ()

        def __init__(self, c, ref):
            self.own, self.length, self.given, self.base, self.seen = contigs.index(c), int(ref.shape[0]), 0, inner.copy(), pair_reads[0]
            self.caller = None
            if not restatement:
                self.caller = Caller(ref, min_size, flank, mapq_threshold, device)
                try:
                    self.caller.set_contigs(contigs, self.own)
                    self.caller.set_library(*UNSET_LIBRARY)
                except Exception:
                    self.caller.close()
                    raise

        def add(self, reads, splits, mates, lo, hi):
            if self.caller is not None:
                self.caller.add(reads, splits, mates, lo, hi)
                inner[:] = self.base + handle_array(self.caller._lib.hello_sv_pairs_array, self.caller._h, 0, np.int64)
                pair_reads[0] = self.seen + int(self.caller.stats()["pair_reads"])
            else:
                part = pair_rows_of(reads, splits, mates, lo, self.own, len(contigs), self.length, min_size, mapq_threshold, UNSET_LIBRARY,
                                    CLIP_MIN, self.given)
                self.given += part["counts"]["pair_reads"]
                pair_reads[0] = self.seen + self.given
                np.add.at(inner, np.array(part["inner"], np.int64), 1)
            if inner.sum() >= LIBRARY_SAMPLE:
                raise _Sampled()

        def results(self):
            return {}, {}

        def close(self):
            if self.caller is not None:
                self.caller.close()

    try:
        measure_spans(bam, fasta, chromosomes, max_span, None, False, open_handle=Sampler, restated=None, done=lambda *a: None,
                      with_pairs=True)
    except _Sampled:
        pass
    if pair_reads[0] == 0:
        return UNSET_LIBRARY
    if inner.sum() < LIBRARY_MIN_PAIRS:
        raise LibraryError("%s: %d forward-reverse pairs on one chromosome, too few for a library (at least %d): give the inner distances "
                         "with --sv_pairs_library MEDIAN,LO,HI (--pairs_library of hello_amd.sv)" % (bam, int(inner.sum()), LIBRARY_MIN_PAIRS))
    return library_of(inner, k)


def add_pairs_options(p: argparse.ArgumentParser, prefix: str, given_or_none: bool = False) -> None:
    """``--<prefix>pairs_library``, ``--<prefix>pairs_k`` and ``--[sv_]clip_min`` (prefix: "sv_" for hello_amd.call, "" here)."""
    pick = lambda v: None if given_or_none else v                   # noqa: E731
    p.add_argument("--%spairs_library" % prefix, default=None, metavar="M,LO,HI",
                   help="with pairs: the library's inner distance (mate start minus read end) as median and the least and greatest "
                        "normal value, instead of sampling them from the BAM")
    p.add_argument("--%spairs_k" % prefix, type=int, default=pick(PAIRS_K),
                   help="with pairs: a sampled library calls normal what lies within k median absolute deviations (default %d)" % PAIRS_K)
    p.add_argument("--%sclip_min" % prefix, type=int, default=pick(CLIP_MIN),
                   help="with pairs: the fewest bases of a soft clip that counts as a clipped end (default %d)" % CLIP_MIN)


def library_option(text: Optional[str], name: str) -> Optional[Tuple[int, int, int]]:
    """``M,LO,HI`` -> the triple, refused with the fix where it is none."""
    if text is None:
        return None
    try:
        median, lo, hi = (int(v) for v in text.split(","))
    except ValueError:
        raise SystemExit(f"--{name} takes three integers MEDIAN,LO,HI: give for instance --{name} 200,40,360") from None
    if not -(1 << 31) <= lo <= median <= hi < (1 << 31):
        raise SystemExit(f"--{name} is MEDIAN,LO,HI with LO <= MEDIAN <= HI: give for instance --{name} 200,40,360")
    return median, lo, hi


def check_pairs_options(k: int, clip_min: int, prefix: str) -> None:
    if k < 1:
        raise SystemExit(f"--{prefix}pairs_k is a number of median absolute deviations: give 1 or more")
    if clip_min < 1:
        raise SystemExit(f"--{prefix}clip_min is the fewest bases of a soft clip that counts: give 1 or more")


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
    p.add_argument("--pairs", action="store_true", default=False,
                   help="Also call deletions, duplications, inversions and translocation ends from discordant read pairs, and count "
                        "the clipped ends near every event (DESIGN.md 7s)")
    add_pairs_options(p, "", given_or_none=True)
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def main(argv=None) -> List[str]:
    from .call import read_fasta
    args = parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)-15s %(message)s")
    check_options(args.sv_min_size, args.sv_min_support, args.sv_flank, args.sv_cluster_gap, args.sv_len_ratio)
    if not args.pairs:
        for flag in ("pairs_library", "pairs_k", "clip_min"):
            if getattr(args, flag) is not None:
                raise SystemExit(f"--{flag} is an option of the read pairs and this run looks at none: add --pairs, or drop --{flag}")
    library = library_option(args.pairs_library, "pairs_library")
    pairs_k, clip_min = PAIRS_K if args.pairs_k is None else args.pairs_k, CLIP_MIN if args.clip_min is None else args.clip_min
    check_pairs_options(pairs_k, clip_min, "")
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
            try:
                found = measure(bam, genome, chromosomes, tagger, args.sv_min_size, args.sv_flank, args.mapq_threshold, args.sv_cluster_gap,
                                percent_of(args.sv_len_ratio), args.sv_min_support, device=args.device, stats=stats, split=args.split,
                                pairs=args.pairs, library=library, k=pairs_k, clip_min=clip_min)
            except LibraryError as refused:
                raise SystemExit(str(refused)) from None
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
