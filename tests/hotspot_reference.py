"""Plain-Python restatement of the reference's hotspot stage, the yardstick of hello_amd/csrc/hotspots.hip.

Each function cites the reference lines it restates (python/ and c++/ of the reference).  The reference's own C++ needs
Boost.Python and cannot run here, so this restatement is pinned by hand-derived cases in tests/test_hotspots.py.  Reads are
tests.bam_writer.Read records; the reference is the chromosome's text, case kept.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Set, Tuple

import numpy as np

CHUNK_SIZE_ILLUMINA, CHUNK_SIZE_PACBIO = 400, 10000          # HotspotDetectorDVFiltered.py:14-15
MAX_NUM_READS_ILLUMINA, MAX_NUM_READS_PACBIO = 10000, 1000   # :16-17
F32 = np.float32
SNV_THRESHOLD = INDEL_THRESHOLD = F32(0.12)                  # AlleleSearcherLiteFiltered.cpp:385-386, float members (.h:131-132)
MIN_COUNT = 2                                                # :387
MAX_ALLELE_SIZE = 100                                        # :389


def is_usable(r) -> bool:
    """python/PileupContainer.py:33-41 (QC-fail reads are kept: 'Missing: failed_vendor_quality_checks')."""
    f = r.flag
    if f & 0x4 or f & 0x100 or f & 0x800 or f & 0x400:
        return False
    if (f & 0x1) and not (f & 0x2):
        return False
    return r.mapq > 0


def chunk_reads(reads: Sequence, begin: int, end: int, cap: int) -> Tuple[List, bool]:
    """python/PileupContainerLite.py:526-570: fetch (pos < end, bam_endpos > begin) in file order, usable reads only, the
    first of each (name, strand); the reservoir (:545-567) is replaced by keeping the first `cap` reads.  -> (reads, capped)."""
    seen, out, capped = set(), [], False
    for r in reads:
        if not (r.pos < end and r.ref_end > begin) or not is_usable(r):
            continue
        key = (r.name, r.is_reverse)
        if key in seen:
            continue
        seen.add(key)
        if len(out) >= cap:
            capped = True
            continue
        out.append(r)
    return out, capped


class AlleleCounts:
    """AlleleSearcherLiteFiltered.h:65-73."""
    __slots__ = ("total", "alt", "left", "right")

    def __init__(self):
        self.total = 0            # float in the reference; integer sums below 2**24 are exact
        self.alt: Dict[Tuple[str, str], int] = {}
        self.left: Dict[Tuple[str, str], int] = {}
        self.right: Dict[Tuple[str, str], int] = {}


def update_counts(counts: Dict[int, AlleleCounts], read, reference: str, q_threshold: int, pacbio: bool) -> None:
    """AlleleSearcherLiteFiltered.cpp:121-317 for one read (the mapq test :134-136 is the caller's).  `counts` is keyed by
    genome position; `reference` is the chromosome, so reference[p] is the window's base at p."""
    seq, qual, cigar = read.seq, read.qual, read.cigar
    rf, rd = read.pos, 0
    inc = 1 if pacbio else 2

    def at(p):
        c = counts.get(p)
        if c is None:
            c = counts[p] = AlleleCounts()
        return c

    def add(count, ref_allele, alt_allele, rd0, rdlen, partial=False, left=False):      # :141-173
        if "N" in ref_allele or "N" in alt_allele:
            return
        if rd0 >= 0 and min(qual[rd0:rd0 + rdlen]) < q_threshold:
            return
        table = (count.left if left else count.right) if partial else count.alt
        table[(ref_allele, alt_allele)] = table.get((ref_allele, alt_allele), 0) + inc

    for ci, (op, length) in enumerate(cigar):
        if op in (0, 7, 8):                                                                # :184-216
            for j in range(length):
                c = at(rf + j)
                if seq[rd + j] != reference[rf + j]:
                    if qual[rd + j] >= q_threshold and seq[rd + j] != "N" and reference[rf + j] != "N":
                        c.alt[(reference[rf + j], seq[rd + j])] = c.alt.get((reference[rf + j], seq[rd + j]), 0) + 1
                c.total += 1
            rf += length
            rd += length
        elif op == 2:                                                                      # :218-238, then :239-243
            c = at(rf - 1)
            ref_allele = reference[rf - 1:rf + length]
            alt = seq[rd - 1] if rd > 0 else reference[rf - 1]
            add(c, ref_allele, alt, rd - 1, 1)
            rf += length
        elif op == 3:                                                                      # :239-243
            rf += length
        elif op == 1:                                                                      # :245-304, then :305-309
            c = at(rf - 1)
            ref_allele = reference[rf - 1]
            if ci == 0:
                add(c, ref_allele, seq[rd:rd + length], rd, length, True, True)
                c.total += 1                                                               # :267
            elif ci == len(cigar) - 1 and rd > 0:
                add(c, ref_allele, seq[rd - 1:rd + length], rd - 1, length + 1, True, False)
            elif rd > 0:
                add(c, ref_allele, seq[rd - 1:rd + length], rd - 1, length + 1)
            else:
                add(c, ref_allele, ref_allele + seq[rd:rd + length], rd, length)
            rd += length
        elif op == 4:                                                                      # :305-309
            rd += length
        # H (5) and P (6): no case in the switch; cigarcount still advances (:312)


def resolve_partials(c: AlleleCounts) -> None:
    """AlleleCounts::resolvePartials (AlleleSearcherLiteFiltered.cpp:19-100): a partial whose alt is a suffix (left) or a
    prefix (right) of exactly one key's alt adds its count there; otherwise it is dropped (a key enters the tracker only on a
    match, so the keys.size() == 0 branch never runs)."""
    for partials, left in ((c.left, True), (c.right, False)):
        adds = {}
        for (_, palt), n in partials.items():
            hits = [k for k in c.alt if len(k[1]) >= len(palt) and (k[1].endswith(palt) if left else k[1].startswith(palt))]
            if len(hits) == 1:
                adds[hits[0]] = adds.get(hits[0], 0) + n
        for k, n in adds.items():
            c.alt[k] += n
    c.left, c.right = {}, {}


def flag_single(counts: Dict[int, AlleleCounts], min_indel: int, out: Set[int]) -> None:
    """determine_differing_regions_helper (:834-890); the float32 expressions of the reference."""
    for pos, item in counts.items():
        if item.total == 0:
            continue
        total = F32(item.total)
        for (ref, alt), n in item.alt.items():
            value = F32(n)
            if len(ref) == 1 and len(alt) == 1:
                if value / total >= SNV_THRESHOLD and value >= MIN_COUNT:
                    out.add(pos)
            else:
                if max(len(ref), len(alt)) > MAX_ALLELE_SIZE:
                    continue
                if value / total >= INDEL_THRESHOLD and value >= min_indel:
                    out.update(range(pos, pos + len(ref) + 1))


def flag_hybrid(counts_i: Dict[int, AlleleCounts], counts_p: Dict[int, AlleleCounts], out: Set[int]) -> None:
    """determine_differing_regions_hybrid_helper (:550-609): keys from counts_i only (the loop at :559-565 reads count_i
    twice), totals summed, no allele size limit, an indel flags [pos, pos + |ref|)."""
    for pos, ci in counts_i.items():
        cp = counts_p.get(pos)
        total = F32(ci.total) + F32(cp.total if cp else 0)
        if total == 0:
            continue
        for key in ci.alt:
            vi = F32(ci.alt[key])
            vp = F32(cp.alt.get(key, 0) if cp else 0)
            ref, alt = key
            if len(ref) == 1 and len(alt) == 1:
                if (vi + vp) / total >= SNV_THRESHOLD and vi + vp >= MIN_COUNT:
                    out.add(pos)
            else:
                if (vi + vp) / total >= INDEL_THRESHOLD and vi / F32(2) + vp >= MIN_COUNT:
                    out.update(range(pos, pos + len(ref)))


def do_chunk(read_sets: Sequence[Sequence], tables: Sequence[int], caps: Sequence[int], reference: str, begin: int, end: int,
             hybrid_hotspot: bool, q_threshold: int, mapq_threshold: int, stats: dict = None) -> Set[int]:
    """HotspotDetectorDVFiltered.doOneChunk (:31-101) with AlleleSearcherLite (python/AlleleSearcherLite.py:112-190):
    read sets, the window bounds that skip a chunk, counting, partials, flagging (:611-646, under the num_*_reads quirk:
    both tables flagged and unioned), clipped to [begin, end)."""
    kept = []
    for reads, cap in zip(read_sets, caps):
        rs, capped = chunk_reads(reads, begin, end, cap)
        kept.append(rs)
        if stats is not None and capped:
            stats["capped"] = stats.get("capped", 0) + 1
    if all(len(k) == 0 for k in kept):
        return set()
    window_start = min([r.pos for k in kept for r in k] + [begin]) - 10
    window_end = max(r.ref_end for k in kept for r in k)
    if window_start < 0 or window_end > len(reference):
        return set()
    counts = ({}, {})
    for k, table in zip(kept, tables):
        for r in k:
            if r.mapq < mapq_threshold:
                continue
            update_counts(counts[table], r, reference, q_threshold, pacbio=table == 1)
    for t in counts:
        for c in t.values():
            resolve_partials(c)
    found: Set[int] = set()
    if hybrid_hotspot:
        flag_hybrid(counts[0], counts[1], found)
    else:
        flag_single(counts[0], 2 * MIN_COUNT, found)
        flag_single(counts[1], MIN_COUNT, found)
    return {p for p in found if begin <= p < end}


def find_hotspots(read_sets: Sequence[Sequence], reference: str, start: int, stop: int, pacbio: bool = False,
                  hybrid_hotspot: bool = False, q_threshold: int = 10, mapq_threshold: int = 10, stats: dict = None) -> List[int]:
    """hotspotGeneratorSingle / hotspotGeneratorHybrid (HotspotDetectorDVFiltered.py:104-165, main :168-262)."""
    if len(read_sets) == 2:
        size, tables, caps = CHUNK_SIZE_PACBIO, (0, 1), (MAX_NUM_READS_ILLUMINA, MAX_NUM_READS_PACBIO)
    elif pacbio:
        size, tables, caps = CHUNK_SIZE_PACBIO, (1,), (MAX_NUM_READS_PACBIO,)
    else:
        size, tables, caps = CHUNK_SIZE_ILLUMINA, (0,), (MAX_NUM_READS_ILLUMINA,)
    positions: Set[int] = set()
    for i in range(math.ceil((stop - start) / size)):
        b = start + size * i
        positions |= do_chunk(read_sets, tables, caps, reference, b, min(b + size, stop), hybrid_hotspot, q_threshold,
                              mapq_threshold, stats)
    return sorted(positions)
