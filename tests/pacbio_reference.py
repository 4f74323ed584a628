"""Plain-Python restatement of the reference's candidate stage for one PacBio BAM, the yardstick of the PacBio path of
hello_amd/csrc/candidates.hip: tests/candidate_reference.py with the PacBio read cap, the PacBio counting table and thresholds,
and strictly clipped reads.

``strict_clip_fn`` / ``strict_clip`` restate python/PileupContainerLite.py:255-468 (strictClipFn, strictClipRead); they are pinned
by the reference's own functions through tests/golden/pacbio_clip_cases.json (tests/golden/make_pacbio_clip_fixture.py).
``clip_read`` is what PileupContainerLite.__get_reads (:554-573) does to every kept read of a container: a copy, clipped on the
left at the container's position and then on the right at position + span, the right clip seeing the left clip's result.

Read selection (fetch overlap, usable, first of (name, strand), cap) looks at the original alignment; everything after it -- window
tests, counting, alleles, supports, the reads of a site -- at the clipped reads.  The deviations are those of
tests/candidate_reference.py.
"""
from __future__ import annotations

from dataclasses import replace
from typing import Dict, List, Optional, Sequence, Set, Tuple

from tests import candidate_reference as cr
from tests import hotspot_reference as hr

READ_RATE_PACBIO = (100, 100)          # PileupDataTools.py:18
CLIP_FLANK = 200                       # caller_calling.py:795-843 (clipFlank)
QUERY_OPS = (0, 1, 4, 7, 8)            # M I S = X: read bases
REF_OPS = (0, 2, 3, 7, 8)              # M D N = X: reference bases


def read_cap(start: int, stop: int) -> float:
    """ReadSampler.__call__ (PileupDataTools.py:139-146) with READ_RATE_PACBIO: a float."""
    if stop - start > READ_RATE_PACBIO[1]:
        return READ_RATE_PACBIO[0] / READ_RATE_PACBIO[1] * (stop - start)
    return READ_RATE_PACBIO[0]


def strict_clip_fn(cigars: Sequence[Tuple[int, int]], limit: int, left: bool):
    """strictClipFn (:255-363): walk away from the split (backwards for the left half), keep operations until the one in which
    the read-base count passes `limit`, of which ``limit - count + 1`` are kept; an outermost kept I becomes S.
    -> (kept operations, read bases discarded, reference bases discarded)."""
    ops = list(reversed(cigars)) if left else list(cigars)
    keep: List[Tuple[int, int]] = []
    discard: List[Tuple[int, int]] = []
    count = 0
    for i, (op, n) in enumerate(ops):
        after = count + (n if op in QUERY_OPS else 0)
        if count <= limit < after:
            k = limit - count + 1
            if k > 0:
                keep.append((op, k))
            if n - k > 0:
                discard.append((op, n - k))
            discard.extend(ops[i + 1:])
            break
        keep.append((op, n))
        count = after
    if left:
        keep.reverse()
    edge = 0 if left else -1
    if keep[edge][0] == 1:
        keep[edge] = (4, keep[edge][1])
    pruned_query = sum(n for op, n in discard if op in QUERY_OPS)
    pruned_ref = sum(n for op, n in discard if op in REF_OPS)
    return keep, pruned_query, pruned_ref


def strict_clip(pos: int, end: int, cigar: Sequence[Tuple[int, int]], seq, qual, position: int, left: bool, flank: int = CLIP_FLANK):
    """strictClipRead (:366-468) on (reference_start, reference_end, cigartuples, query_sequence, query_qualities) -> the same
    five, changed or not."""
    cigar = [tuple(c) for c in cigar]
    if not (pos <= position < end):
        return pos, end, cigar, seq, qual
    counter = pos
    left_ops: List[Tuple[int, int]] = []
    right_ops: List[Tuple[int, int]] = []
    for i, (op, n) in enumerate(cigar):
        after = counter + (n if op in REF_OPS else 0)
        if counter <= position < after:
            k = position - counter + 1
            if k > 0:
                left_ops.append((op, k))
            if n - k > 0:
                right_ops.append((op, n - k))
            right_ops.extend(cigar[i + 1:])
            break
        left_ops.append((op, n))
        counter = after
    if left and left_ops:
        left_keep, pruned_query, pruned_ref = strict_clip_fn(left_ops, flank, True)
        pos += pruned_ref
        seq, qual = seq[pruned_query:], qual[pruned_query:]
        right_keep = right_ops
    elif right_ops:
        right_keep, pruned_query, pruned_ref = strict_clip_fn(right_ops, flank, False)
        end -= pruned_ref
        if pruned_query > 0:
            seq, qual = seq[:-pruned_query], qual[:-pruned_query]
        left_keep = left_ops
    else:
        return pos, end, cigar, seq, qual
    if left_keep and right_keep:
        centre = [left_keep[-1], right_keep[0]]
        if centre[0][0] == centre[1][0]:
            centre = [(centre[0][0], centre[0][1] + centre[1][1])]
    else:
        centre = []
        if left_keep:
            centre = [left_keep[-1]]
        if right_keep:
            centre = [right_keep[0]]
    return pos, end, left_keep[:-1] + centre + right_keep[1:], seq, qual


def clip_read(read, position: int, span: int, flank: int = CLIP_FLANK):
    """PileupContainerLite.__get_reads (:554-573): a copy of the read, clipped left at `position`, then right at
    `position + span`."""
    state = (read.pos, read.ref_end, read.cigar, read.seq, list(read.qual))
    state = strict_clip(*state, position, True, flank)
    pos, end, cigar, seq, qual = strict_clip(*state, position + span, False, flank)
    out = replace(read, pos=pos, cigar=[tuple(c) for c in cigar], seq=seq, qual=list(qual))
    assert len(out.seq) == sum(n for op, n in out.cigar if op in QUERY_OPS)
    assert out.ref_end == end or not any(op in REF_OPS for op, _ in out.cigar)
    return out


class Searcher:
    """candidate_reference.Searcher for one set of PacBio reads (AlleleSearcherLite.__init__ with pacbio = True, clipped reads,
    no reassembly: one container): selection on the original alignments, everything else on the clipped copies; every read
    counts in counts_p with increment 1 and indels need minCount reads (AlleleSearcherLiteFiltered.cpp:621-624)."""

    def __init__(self, reads: Sequence, reference: str, start: int, stop: int, fetch_start: int, fetch_stop: int,
                 q_threshold: int, mapq_threshold: int):
        self.start, self.stop = start, stop
        kept, self.capped = hr.chunk_reads(reads, fetch_start, fetch_stop, read_cap(fetch_start, fetch_stop))
        self.originals = kept
        self.reads = [clip_read(r, fetch_start, fetch_stop - fetch_start) for r in kept]
        self.regions: List[Tuple[int, int]] = []
        self.status = "ok"
        if not self.reads:
            self.status = "no_reads"
            return
        window_start = min([r.pos for r in self.reads] + [start]) - 10
        window_end = max(r.ref_end for r in self.reads)
        if window_start < 0 or window_end > len(reference):
            self.status = "out_of_bounds"
            return
        counts: Dict[int, hr.AlleleCounts] = {}
        for r in self.reads:
            if r.mapq >= mapq_threshold:
                hr.update_counts(counts, r, reference, q_threshold, pacbio=True)
        for c in counts.values():
            hr.resolve_partials(c)
        flagged: Set[int] = set()
        hr.flag_single(counts, hr.MIN_COUNT, flagged)
        self.regions = cr.strict_runs(flagged, start, stop)


def pass1(reads: Sequence, reference: str, positions: Sequence[int], q_threshold: int, mapq_threshold: int,
          stats: dict) -> List[Tuple[int, int]]:
    """candidate_reference.pass1 with the PacBio searcher."""
    out: List[Tuple[int, int]] = []
    for start, stop in cr.active_regions(positions):
        stats["active_regions"] += 1
        s = Searcher(reads, reference, start, stop, max(0, start - cr.FLANKING_BASES), stop + cr.FLANKING_BASES, q_threshold,
                     mapq_threshold)
        if s.status == "no_reads":
            stats["regions_without_reads"] += 1
        elif s.status == "out_of_bounds":
            stats["regions_out_of_bounds"] += 1
        else:
            stats["regions_at_read_cap"] += int(s.capped)
        out += s.regions
    out.sort()
    for a, b in zip(out, out[1:]):
        assert a[1] < b[0], "differing regions of different active regions overlap or touch"
    return out


def find_candidates(reads: Sequence, reference: str, positions: Sequence[int], q_threshold: int = 10, mapq_threshold: int = 10,
                    feature_length: int = 150, stats: Optional[dict] = None) -> List[cr.Site]:
    """candidate_reference.find_candidates for one PacBio BAM.  A site's ``reads`` are the cluster's clipped reads (a fresh
    fetch from the original reads, trainDataTools.py:1059-1065, not a re-clip of pass 1's copies)."""
    st = {k: 0 for k in cr.STAT_KEYS}
    locations = pass1(reads, reference, positions, q_threshold, mapq_threshold, st)
    st["differing_regions_pass1"] = len(locations)
    st["regions_pass1"] = list(locations)
    st["regions_pass2"] = []
    sites: List[cr.Site] = []
    for cluster in cr.cluster_locations(locations):
        st["clusters"] += 1
        start = cluster[0][0] - cr.MIN_DISTANCE // 2
        stop = cluster[-1][1] + cr.MIN_DISTANCE // 2 - 1
        s = Searcher(reads, reference, start, stop, start, stop, q_threshold, mapq_threshold)
        if s.status == "no_reads":
            st["clusters_without_reads"] += 1
        elif s.status == "out_of_bounds":
            st["clusters_out_of_bounds"] += 1
        else:
            st["clusters_at_read_cap"] += int(s.capped)
        st["differing_regions_pass2"] += len(s.regions)
        st["regions_pass2"] += s.regions
        sites += cr.sites_of_cluster(s, reference, q_threshold, mapq_threshold, feature_length, st)
    st["sites"] = len(sites)
    st["alleles"] = sum(len(s.alleles) for s in sites)
    st["reads_gathered"] = sum(len(r) for s in sites for _, r in s.alleles)
    if stats is not None:
        stats.update(st)
    return sites
