"""Plain-Python restatement of the reference's candidate stage for one Illumina BAM, the yardstick of
hello_amd/csrc/candidates.hip: hotspot positions -> active regions -> strict differing regions (pass 1) -> clusters -> the
clusters' own strict differing regions (pass 2, the sites) -> alleles and their supporting reads.

One function per cited block of the reference (python/ and c++/).  Counting, partial resolution and the thresholds are those of
tests/hotspot_reference.py.  The reference's own C++ needs Boost.Python and cannot run here, so this restatement is pinned by
hand-derived cases in tests/test_candidates.py.  Reads are tests.bam_writer.Read records in file order; the reference is the
chromosome's text, case kept.

Defined where the reference leaves it open: alternative alleles in ascending byte order after the reference allele, supporting
reads in file order.  Deviations: the first reads are kept at the read cap (the reference samples a reservoir, unseeded); a
cluster whose window leaves the chromosome is skipped and counted (the reference lets LocationOutOfBounds end the job); a site
whose feature window leaves the chromosome is dropped and counted (a shard needs that window).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Set, Tuple

from tests import hotspot_reference as hr

MIN_DISTANCE = 30                      # PileupDataTools.py:21
FLANKING_BASES = 75                    # :24
READ_RATE_ILLUMINA = (1000, 30)        # :17
MAX_ITEMS_PER_GROUP = 1024             # caller_calling.py:859
MAX_ALLELE_LENGTH = 80                 # trainDataTools.createTensors / clusterLocations
SUCCESS, LEFT_PARTIAL, RIGHT_PARTIAL, FAIL = "Success", "LeftPartial", "RightPartial", "Fail"


def active_regions(positions: Sequence[int], distance: int = MIN_DISTANCE) -> List[Tuple[int, int]]:
    """hotspotsReader (PileupDataTools.py:207-244): consecutive points with 0 <= d <= distance form [first - 15, last + 15]."""
    out, cluster = [], []
    for p in positions:
        if not cluster or 0 <= p - cluster[-1] <= distance:
            cluster.append(p)
        else:
            out.append((cluster[0] - distance // 2, cluster[-1] + distance // 2))
            cluster = [p]
    if cluster:
        out.append((cluster[0] - distance // 2, cluster[-1] + distance // 2))
    return out


def read_cap(start: int, stop: int) -> float:
    """ReadSampler.__call__ (PileupDataTools.py:139-146): a float."""
    if stop - start > READ_RATE_ILLUMINA[1]:
        return READ_RATE_ILLUMINA[0] / READ_RATE_ILLUMINA[1] * (stop - start)
    return READ_RATE_ILLUMINA[0]


def strict_runs(flagged: Set[int], start: int, stop: int) -> List[Tuple[int, int]]:
    """cluster_differing_regions_helper + pushRegions(strict = True) (AlleleSearcherLiteFiltered.cpp:495-547): maximal runs
    [a, b + 1); a run with a < start or b + 1 > stop is dropped whole."""
    out, run = [], []

    def push():
        a, b = run[0], run[-1] + 1
        if not (a < start or b > stop):
            out.append((a, b))
    for p in sorted(flagged):
        if run and run[-1] != p - 1:
            push()
            run = []
        run.append(p)
    if run:
        push()
    return out


class Searcher:
    """AlleleSearcherLite.__init__ (python/AlleleSearcherLite.py:92-184) for one read set of Illumina reads: the reads fetched
    over [fetch_start, fetch_stop) under the cap, the window bounds, and determineDifferingRegions(strict = True)
    (AlleleSearcherLiteFiltered.cpp:611-646: num_illumina_reads == num_pacbio_reads == 0, so the union branch; the PacBio table
    is empty).  ``status``: "ok", "no_reads" or "out_of_bounds"."""

    def __init__(self, reads: Sequence, reference: str, start: int, stop: int, fetch_start: int, fetch_stop: int,
                 q_threshold: int, mapq_threshold: int):
        self.start, self.stop = start, stop
        self.reads, self.capped = hr.chunk_reads(reads, fetch_start, fetch_stop, read_cap(fetch_start, fetch_stop))
        self.regions: List[Tuple[int, int]] = []
        self.status = "ok"
        if not self.reads:
            self.status = "no_reads"
            return
        window_start = min([r.pos for r in self.reads] + [start]) - 10
        window_end = max(r.ref_end for r in self.reads)
        if window_start < 0 or window_end > len(reference):        # LocationOutOfBounds (:142-149)
            self.status = "out_of_bounds"
            return
        counts: Dict[int, hr.AlleleCounts] = {}
        for r in self.reads:
            if r.mapq >= mapq_threshold:
                hr.update_counts(counts, r, reference, q_threshold, pacbio=False)
        for c in counts.values():
            hr.resolve_partials(c)
        flagged: Set[int] = set()
        hr.flag_single(counts, 2 * hr.MIN_COUNT, flagged)
        self.regions = strict_runs(flagged, start, stop)


def pass1(reads: Sequence, reference: str, positions: Sequence[int], q_threshold: int, mapq_threshold: int,
          stats: dict) -> List[Tuple[int, int]]:
    """candidateReader (PileupDataTools.py:302-384): one strict searcher per active region over the reads of
    [max(0, start - 75), stop + 75); its regions, sorted.  merge_overlaps has nothing to merge (asserted)."""
    out: List[Tuple[int, int]] = []
    for start, stop in active_regions(positions):
        stats["active_regions"] += 1
        s = Searcher(reads, reference, start, stop, max(0, start - FLANKING_BASES), stop + FLANKING_BASES, q_threshold, mapq_threshold)
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


def cluster_locations(locations: Sequence[Tuple[int, int]], distance: int = MIN_DISTANCE,
                      max_allele_length: int = MAX_ALLELE_LENGTH) -> List[List[Tuple[int, int]]]:
    """clusterLocations (trainDataTools.py:477-514), its quirk kept: a location longer than max_allele_length closes and emits
    a non-empty cluster and is itself dropped; with an empty cluster it falls through and is appended."""
    out, cluster = [], []
    for location in locations:
        if location[1] - location[0] > max_allele_length:
            if len(cluster) > 0:
                out.append(cluster)
                cluster = []
                continue
        if len(cluster) == 0:
            cluster.append(location)
        elif location[0] - cluster[-1][1] < distance and len(cluster) < MAX_ITEMS_PER_GROUP:
            cluster.append(location)
        else:
            out.append(cluster)
            cluster = [location]
    if cluster:
        out.append(cluster)
    return out


def split_clusters(cluster: Sequence[Tuple[int, int]], reference: str):
    """split_clusters (trainDataTools.py:517-554): (regions, reference segment, segment start) groups of at most
    MAX_ITEMS_PER_GROUP regions.  Only the segment the reference allele is cut from changes; the allele is the same text."""
    cluster = list(cluster)
    if len(cluster) <= MAX_ITEMS_PER_GROUP:
        a, b = cluster[0][0] - MIN_DISTANCE // 2, cluster[-1][-1] + MIN_DISTANCE // 2
        yield cluster, reference[max(a, 0):b], max(a, 0)
        return
    last = None
    indices = list(range(0, len(cluster), MAX_ITEMS_PER_GROUP))
    for i, index in enumerate(indices):
        nxt = indices[i + 1] if i + 1 < len(indices) else -1
        current = cluster[index:index + MAX_ITEMS_PER_GROUP]
        following = cluster[nxt:nxt + MAX_ITEMS_PER_GROUP] if nxt >= 0 else None
        a = max(current[0][0] - MIN_DISTANCE // 2, last[-1][-1] if last else -math.inf)
        b = min(current[-1][-1] + MIN_DISTANCE // 2, following[0][0] if following else math.inf)
        a = max(int(a), 0)
        yield current, reference[a:int(b)], a
        last = current


class ReadMap:
    """Read::_get_read_mapping (Read.cpp:4-77), literally: aligned_pairs / aligned_qualities keyed by reference position."""

    def __init__(self, read):
        self.pairs: Dict[int, str] = {}
        self.quals: Dict[int, int] = {}
        self.reference_start = read.pos
        self.last_position = -1
        self.partial_start = self.partial_stop = False
        ref_ptr, rd_ptr = read.pos, 0
        for count, (op, length) in enumerate(read.cigar):
            if op in (0, 7, 8):
                for i in range(length):
                    self.pairs[ref_ptr + i] = read.seq[rd_ptr + i]
                    self.quals[ref_ptr + i] = read.qual[rd_ptr + i]
                    self.last_position = ref_ptr + i
                rd_ptr += length
                ref_ptr += length
            elif op == 2:
                for i in range(length):
                    self.pairs[ref_ptr + i] = ""
                    self.quals[ref_ptr + i] = 60
                    self.last_position = ref_ptr + i
                ref_ptr += length
            elif op == 3:
                ref_ptr += length
            elif op == 1:
                text = read.seq[rd_ptr:rd_ptr + length]
                if ref_ptr - 1 not in self.pairs:
                    self.pairs[ref_ptr - 1] = text
                    self.partial_start = True
                else:
                    self.pairs[ref_ptr - 1] += text
                    if count == len(read.cigar) - 1:
                        self.partial_stop = True
                q = min(read.qual[rd_ptr:rd_ptr + length])
                self.quals[ref_ptr - 1] = min(self.quals[ref_ptr - 1], q) if ref_ptr - 1 in self.quals else q
                rd_ptr += length
            elif op == 4:
                rd_ptr += length

    def aligned_bases(self, start: int, stop: int) -> Tuple[str, str, int]:
        """Read::get_aligned_bases (Read.cpp:79-137) -> (allele, status, min_q)."""
        if not (start <= self.last_position and self.reference_start < stop) or self.last_position == -1:
            return "", FAIL, 10000
        if start not in self.pairs:
            status = LEFT_PARTIAL
        elif start - 1 not in self.pairs:
            status = LEFT_PARTIAL if self.partial_start else SUCCESS
        elif stop - 1 not in self.pairs:
            status = RIGHT_PARTIAL
        elif stop not in self.pairs:
            status = RIGHT_PARTIAL if self.partial_stop else SUCCESS
        else:
            status = SUCCESS
        if start in self.pairs and len(self.pairs[start]) == 0:
            status = FAIL
        if stop - 1 in self.pairs and len(self.pairs[stop - 1]) == 0:
            status = FAIL
        allele, min_q = "", 10000
        for i in range(start, stop):
            if i in self.pairs:
                allele += self.pairs[i]
            if i in self.quals:
                min_q = min(min_q, self.quals[i])
        return allele, status, min_q


def extract_alleles(read, regions: Sequence[Tuple[int, int]]):
    """Read::extract_alleles (Read.cpp:139-172) -> (Success records, last left partial or None, last right partial or None);
    a record is (allele, start, stop, min_q)."""
    m = ReadMap(read)
    alleles, left, right = [], None, None
    for start, stop in regions:
        allele, status, min_q = m.aligned_bases(start, stop)
        record = (allele, start, stop, min_q)
        if status == SUCCESS:
            alleles.append(record)
        elif status == LEFT_PARTIAL:
            left = record
        elif status == RIGHT_PARTIAL:
            right = record
    return alleles, left, right


def supports(reads: Sequence, regions: Sequence[Tuple[int, int]], q_threshold: int, mapq_threshold: int):
    """assemble_alleles_from_reads without reassembly (AlleleSearcherLiteFiltered.cpp:740-831) ->
    (alleles_in_regions {(start, stop): strings without N}, supports_in_region {(start, stop): {string: set of read indices}})."""
    extracted = [extract_alleles(r, regions) for r in reads]
    candidates: Dict[Tuple[int, int], Set[str]] = {}
    support: Dict[Tuple[int, int], Dict[str, Set[int]]] = {}
    for i, (r, (alleles, _, _)) in enumerate(zip(reads, extracted)):
        for allele, start, stop, min_q in alleles:
            if min_q >= q_threshold and r.mapq >= mapq_threshold:
                if "N" not in allele:                                      # get_alleles_from_reads (:648-666)
                    candidates.setdefault((start, stop), set()).add(allele)
                support.setdefault((start, stop), {}).setdefault(allele, set()).add(i)
    for i, (_, left, right) in enumerate(extracted):
        partial, is_left = (left, True) if left is not None else (right, False)
        if partial is None:
            continue
        allele, start, stop, _ = partial
        at = support.get((start, stop), {})
        hits = [full for full in at if len(full) >= len(allele) and (full.endswith(allele) if is_left else full.startswith(allele))]
        if len(hits) == 1:
            at[hits[0]].add(i)
    return candidates, support


@dataclass
class Site:
    start: int
    stop: int
    window_start: int
    reference: str
    alleles: List[Tuple[str, List[int]]] = field(default_factory=list)     # (string, indices into `reads`, ascending)
    reads: Optional[Sequence] = None                                       # the cluster's read list the indices refer to


def sites_of_cluster(searcher: Searcher, reference: str, q_threshold: int, mapq_threshold: int, feature_length: int,
                     stats: dict) -> List[Site]:
    """get_labeled_candidates + createTensors (trainDataTools.py:557-640,880-977) with the orders this project defines."""
    regions = searcher.regions                                                    # searcher.cluster, not the input cluster
    if not regions:
        return []
    candidates, support = supports(searcher.reads, regions, q_threshold, mapq_threshold)
    out = []
    for group, segment, seg_start in split_clusters(regions, reference):
        for start, stop in group:
            ref_allele = segment[start - seg_start:stop - seg_start]
            alts = sorted(a for a in candidates.get((start, stop), set()) if a != ref_allele)
            kept = []
            for allele in [ref_allele] + alts:
                reads = sorted(support.get((start, stop), {}).get(allele, ()))
                if len(reads) == 0 or len(allele) > MAX_ALLELE_LENGTH:
                    continue
                kept.append((allele, reads))
            if not kept:                                                          # caller_calling.py:876
                continue
            lo = (start + stop) // 2 - feature_length // 2
            ws, we = min(lo, start - 1), max(lo + feature_length, stop)
            if ws < 0 or we > len(reference):
                stats["sites_out_of_bounds"] += 1
                continue
            out.append(Site(start, stop, ws, reference[ws:we], kept, searcher.reads))
    return out


STAT_KEYS = ("active_regions", "regions_without_reads", "regions_out_of_bounds", "regions_at_read_cap", "differing_regions_pass1",
             "clusters", "clusters_without_reads", "clusters_out_of_bounds", "clusters_at_read_cap", "differing_regions_pass2",
             "sites", "sites_out_of_bounds", "alleles", "reads_gathered")


def find_candidates(reads: Sequence, reference: str, positions: Sequence[int], q_threshold: int = 10, mapq_threshold: int = 10,
                    feature_length: int = 150, stats: Optional[dict] = None) -> List[Site]:
    """caller_calling.main (:784-893) up to the featurizer: pass 1, clustering, pass 2, alleles and supports."""
    st = {k: 0 for k in STAT_KEYS}
    locations = pass1(reads, reference, positions, q_threshold, mapq_threshold, st)
    st["differing_regions_pass1"] = len(locations)
    st["regions_pass1"] = list(locations)
    st["regions_pass2"] = []
    sites: List[Site] = []
    for cluster in cluster_locations(locations):
        st["clusters"] += 1
        start = cluster[0][0] - MIN_DISTANCE // 2                                 # trainDataTools.py:1047-1048
        stop = cluster[-1][1] + MIN_DISTANCE // 2 - 1
        s = Searcher(reads, reference, start, stop, start, stop, q_threshold, mapq_threshold)
        if s.status == "no_reads":
            st["clusters_without_reads"] += 1
        elif s.status == "out_of_bounds":
            st["clusters_out_of_bounds"] += 1
        else:
            st["clusters_at_read_cap"] += int(s.capped)
        st["differing_regions_pass2"] += len(s.regions)
        st["regions_pass2"] += s.regions
        sites += sites_of_cluster(s, reference, q_threshold, mapq_threshold, feature_length, st)
    st["sites"] = len(sites)
    st["alleles"] = sum(len(s.alleles) for s in sites)
    st["reads_gathered"] = sum(len(r) for s in sites for _, r in s.alleles)
    if stats is not None:
        stats.update(st)
    return sites


def candidate_sites(sites: Sequence[Site], chromosome: str):
    """The sites as hello_amd.shards.CandidateSite objects (what write_shard and the featurizer take)."""
    from hello_amd.featurizer import AlignedRead
    from hello_amd.shards import CandidateSite
    out = []
    for s in sites:
        alleles = []
        for text, idx in s.alleles:
            reads = [AlignedRead(r.seq, list(r.qual), list(r.cigar), r.pos, r.mapq, -1 if r.is_reverse else 1, getattr(r, "hp", 0))
                     for r in (s.reads[i] for i in idx)]
            alleles.append((text, reads, None))
        out.append(CandidateSite(chromosome, s.start, s.stop, s.reference, s.window_start, alleles))
    return out
