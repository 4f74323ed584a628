"""Plain-Python restatement of the reference's candidate stage for an Illumina and a PacBio BAM together, the yardstick of
hello_candidates_find_hybrid (hello_amd/csrc/candidates.hip): tests/candidate_reference.py and tests/pacbio_reference.py joined
(two containers per searcher), the coverage gate this project defines, and the reconcilement of PacBio reads onto Illumina
alleles (c++/src/AlleleSearcherLiteFiltered.cpp:668-738, c++/src/Read.cpp:174-323), written as the reference does it: the full
product of the Illumina sites' alleles is enumerated.

Defined here where the reference leaves it open (DESIGN.md "Two BAMs"): the coverage rule (``coverage_gate``; the reference asks
a pysam pileup) and the tie rule (when several choices of alleles spell a read's haplotype, every site's strings are ordered by
bytes and the choice with the smallest tuple of indices wins; the reference lets hash order decide).  Not reproduced: the
reference hands the C++ searcher the ``hp`` list of the last container only (python/AlleleSearcherLite.py:125); here every read
keeps its own tag.  The reads of a searcher are the Illumina reads in file order, then the clipped PacBio reads in file order.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Set, Tuple

from tests import candidate_reference as cr
from tests import hotspot_reference as hr
from tests import pacbio_reference as pr

BAND_MARGIN = 6                        # AlleleSearcherLiteFiltered: band_margin
MIN_COVERAGE = 14                      # AlleleSearcherLite.assemble_region: average_coverage > 14
MIN_COVERAGE_MAPQ = 10
MIN_COVERAGE_BASEQ = 13
REASSIGNED_MIN_Q = 60                  # enumerate_all_haplotypes: AllelicRecord(allele, start, stop, 60)

HYBRID_KEYS = ("clusters_gate_passed", "clusters_reassembled", "pacbio_reads_eligible", "pacbio_reads_reassigned",
               "pacbio_reads_reassigned_by_tie", "illumina_sites")
STAT_KEYS = cr.STAT_KEYS + HYBRID_KEYS


def coverage_gate(reads: Sequence, lo: int, hi: int) -> Tuple[int, int]:
    """The project's coverage rule over the fetch interval [lo, hi) of a cluster -> (sum of counts, columns); the gate is
    ``sum > 14 * columns``.  Reads: those of BAM 0 that overlap the interval and are mapped, primary (neither secondary nor
    supplementary), not QC-fail, not duplicate and a proper pair if paired -- before de-duplication and the cap.  A column is
    every reference position one of them covers with M/=/X/D/N, outside the interval too.  A read counts at a column when
    its mapq >= 10 and its base quality there >= 13; on a D/N column the quality is that of its last read base before the
    operation (none: it does not count)."""
    columns: Set[int] = set()
    total = 0
    for r in reads:
        if not (r.pos < hi and r.ref_end > lo):
            continue
        f = r.flag
        if f & (0x4 | 0x100 | 0x800 | 0x200 | 0x400) or ((f & 0x1) and not (f & 0x2)):
            continue
        rf, rd = r.pos, 0
        for op, n in r.cigar:
            if op in (0, 7, 8):
                for j in range(n):
                    columns.add(rf + j)
                    total += int(r.mapq >= MIN_COVERAGE_MAPQ and r.qual[rd + j] >= MIN_COVERAGE_BASEQ)
                rf += n
                rd += n
            elif op in (2, 3):
                columns.update(range(rf, rf + n))
                if rd > 0 and r.mapq >= MIN_COVERAGE_MAPQ and r.qual[rd - 1] >= MIN_COVERAGE_BASEQ:
                    total += n
                rf += n
            elif op in (1, 4):
                rd += n
    return total, len(columns)


class Searcher:
    """AlleleSearcherLite.__init__ (python/AlleleSearcherLite.py:100-206) with two containers: container 0 the Illumina reads
    under the Illumina cap, container 1 the PacBio reads under the PacBio cap, every kept one strictly clipped.  ``reads`` are
    both, Illumina first; ``tech`` their technology."""

    def __init__(self, illumina: Sequence, pacbio: Sequence, reference: str, start: int, stop: int, fetch_start: int, fetch_stop: int,
                 q_threshold: int, mapq_threshold: int, hybrid_hotspot: bool):
        self.start, self.stop = start, stop
        self.fetch = (fetch_start, fetch_stop)
        kept_i, capped_i = hr.chunk_reads(illumina, fetch_start, fetch_stop, cr.read_cap(fetch_start, fetch_stop))
        kept_p, capped_p = hr.chunk_reads(pacbio, fetch_start, fetch_stop, pr.read_cap(fetch_start, fetch_stop))
        self.capped = capped_i or capped_p
        self.reads0 = kept_i
        self.originals1 = kept_p
        self.reads1 = [pr.clip_read(r, fetch_start, fetch_stop - fetch_start) for r in kept_p]
        self.reads = list(self.reads0) + list(self.reads1)
        self.tech = [0] * len(self.reads0) + [1] * len(self.reads1)
        self.regions: List[Tuple[int, int]] = []
        self.status = "ok"
        if not self.reads:                                                   # all(self.noReads)
            self.status = "no_reads"
            return
        window_start = min([r.pos for r in self.reads] + [start]) - 10       # :135
        window_end = max(r.ref_end for r in self.reads)                      # :138-140, the non-empty containers
        if window_start < 0 or window_end > len(reference):
            self.status = "out_of_bounds"
            return
        counts: Tuple[Dict[int, hr.AlleleCounts], Dict[int, hr.AlleleCounts]] = ({}, {})
        for r, t in zip(self.reads, self.tech):
            if r.mapq >= mapq_threshold:
                hr.update_counts(counts[t], r, reference, q_threshold, pacbio=t == 1)
        for table in counts:
            for c in table.values():
                hr.resolve_partials(c)
        flagged: Set[int] = set()
        if hybrid_hotspot:                                                   # AlleleSearcherLiteFiltered.cpp:638-640
            hr.flag_hybrid(counts[0], counts[1], flagged)
        else:                                                                # :619-637: both tables flagged and unioned
            hr.flag_single(counts[0], 2 * hr.MIN_COUNT, flagged)
            hr.flag_single(counts[1], hr.MIN_COUNT, flagged)
        self.regions = cr.strict_runs(flagged, start, stop)


def enumerate_haplotypes(sites: Sequence[Tuple[Tuple[int, int], List[str]]], reference: str, start: int, stop: int):
    """enumerate_all_haplotypes (Read.cpp:239-323): every choice of one allele per site -> its haplotype over [start, stop).
    -> {haplotype: (first choice in lexicographic order of the index tuples, number of choices spelling it)}; the strings
    of a site are in ascending byte order.  Without sites: {"": ((), 1)}, which no read's haplotype equals."""
    if not sites:
        return {"": ((), 1)}
    out: Dict[str, Tuple[Tuple[int, ...], int]] = {}
    for choice in itertools.product(*[range(len(strings)) for _, strings in sites]):
        text, previous = "", start
        for ((a, b), strings), k in zip(sites, choice):
            text += reference[previous:a] + strings[k]
            previous = b
        text += reference[previous:stop]
        if text in out:
            out[text] = (out[text][0], out[text][1] + 1)
        else:
            out[text] = (choice, 1)
    return out


def haplotype_string(alleles, reference: str, start: int, stop: int) -> str:
    """Read::get_haplotype_string (Read.cpp:174-203): the reference over [start, stop) with every Success record's region
    replaced by the record's string."""
    if not alleles:
        return reference[start:stop]
    text, previous = "", start
    for allele, a, b, _ in alleles:
        text += reference[previous:a] + allele
        previous = b
    return text + reference[previous:stop]


def reassemble(reads: Sequence, tech: Sequence[int], extracted: list, regions: Sequence[Tuple[int, int]], reference: str,
               q_threshold: int, mapq_threshold: int, stats: dict) -> None:
    """The reassembly branch of assemble_alleles_from_reads (:695-738): ``extracted`` is changed in place."""
    start, stop = regions[0][0] - BAND_MARGIN, regions[-1][1] + BAND_MARGIN
    i_alleles: Dict[Tuple[int, int], Set[str]] = {}
    for r, t, (alleles, _, _) in zip(reads, tech, extracted):
        if t == 0 and r.mapq >= mapq_threshold:
            for allele, a, b, min_q in alleles:
                if min_q >= q_threshold and "N" not in allele:               # get_alleles_from_reads (:648-666)
                    i_alleles.setdefault((a, b), set()).add(allele)
    sites = [(key, sorted(strings, key=lambda s: s.encode("latin-1"))) for key, strings in sorted(i_alleles.items())]
    stats["illumina_sites"] += len(sites)
    table = enumerate_haplotypes(sites, reference, start, stop)
    for i, (r, t) in enumerate(zip(reads, tech)):
        if t != 1:
            continue
        m = cr.ReadMap(r)
        # Read::update_allelic_records (:211-214) "if the read doesn't span the full start to stop segment, then do not
        # continue".  Its first test is written `start > reference_start`, which lets through the reads that begin at or after
        # start; the spanning test its comment states is what this project implements (DESIGN.md "Two BAMs").
        if m.reference_start > start or m.last_position < stop:
            continue
        stats["pacbio_reads_eligible"] += 1
        hit = table.get(haplotype_string(extracted[i][0], reference, start, stop))
        if hit is None:
            continue
        choice, n_choices = hit
        new = [(strings[k], a, b, REASSIGNED_MIN_Q) for ((a, b), strings), k in zip(sites, choice)]
        extracted[i] = (new, extracted[i][1], extracted[i][2])
        stats["pacbio_reads_reassigned"] += 1
        stats["pacbio_reads_reassigned_by_tie"] += int(n_choices > 1)


def supports(searcher: Searcher, reference: str, q_threshold: int, mapq_threshold: int, reassembly: bool, stats: dict):
    """assemble_alleles_from_reads (:668-832) -> (alleles_in_regions, supports_in_region) as candidate_reference.supports."""
    reads, regions = searcher.reads, searcher.regions
    extracted = [cr.extract_alleles(r, regions) for r in reads]
    if reassembly:
        reassemble(reads, searcher.tech, extracted, regions, reference, q_threshold, mapq_threshold, stats)
    candidates: Dict[Tuple[int, int], Set[str]] = {}
    support: Dict[Tuple[int, int], Dict[str, Set[int]]] = {}
    for i, (r, (alleles, _, _)) in enumerate(zip(reads, extracted)):
        for allele, a, b, min_q in alleles:
            if min_q >= q_threshold and r.mapq >= mapq_threshold:
                if "N" not in allele:
                    candidates.setdefault((a, b), set()).add(allele)
                support.setdefault((a, b), {}).setdefault(allele, set()).add(i)
    for i, (_, left, right) in enumerate(extracted):
        partial, is_left = (left, True) if left is not None else (right, False)
        if partial is None:
            continue
        allele, a, b, _ = partial
        at = support.get((a, b), {})
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
    alleles: List[Tuple[str, List[int], List[int]]] = field(default_factory=list)   # (string, indices into reads0, into reads1)
    reads0: Optional[Sequence] = None          # the cluster's Illumina reads
    reads1: Optional[Sequence] = None          # the cluster's clipped PacBio reads
    originals1: Optional[Sequence] = None      # the PacBio reads they were clipped from


def sites_of_cluster(searcher: Searcher, illumina: Sequence, reference: str, q_threshold: int, mapq_threshold: int,
                     feature_length: int, reassembly_size: int, stats: dict) -> List[Site]:
    """assemble_region (python/AlleleSearcherLite.py:257-268), get_labeled_candidates and createTensors
    (trainDataTools.py:557-640,880-977) for a searcher that ran."""
    total, columns = coverage_gate(illumina, *searcher.fetch)
    gate = total > MIN_COVERAGE * columns
    stats["clusters_gate_passed"] += int(gate)
    regions = searcher.regions
    if not regions:                                                               # :678
        return []
    reassembly = gate and len(regions) < reassembly_size                          # :695
    stats["clusters_reassembled"] += int(reassembly)
    candidates, support = supports(searcher, reference, q_threshold, mapq_threshold, reassembly, stats)
    n0 = len(searcher.reads0)
    out = []
    for group, segment, seg_start in cr.split_clusters(regions, reference):
        for start, stop in group:
            ref_allele = segment[start - seg_start:stop - seg_start]
            alts = sorted((a for a in candidates.get((start, stop), set()) if a != ref_allele), key=lambda s: s.encode("latin-1"))
            kept = []
            for allele in [ref_allele] + alts:
                reads = sorted(support.get((start, stop), {}).get(allele, ()))
                if len(reads) == 0 or len(allele) > cr.MAX_ALLELE_LENGTH:         # createTensors:926-937, both technologies summed
                    continue
                kept.append((allele, [i for i in reads if i < n0], [i - n0 for i in reads if i >= n0]))
            if not kept:
                continue
            lo = (start + stop) // 2 - feature_length // 2
            ws, we = min(lo, start - 1), max(lo + feature_length, stop)
            if ws < 0 or we > len(reference):
                stats["sites_out_of_bounds"] += 1
                continue
            out.append(Site(start, stop, ws, reference[ws:we], kept, searcher.reads0, searcher.reads1, searcher.originals1))
    return out


def find_candidates(illumina_reads: Sequence, pacbio_reads: Sequence, reference: str, positions: Sequence[int],
                    hybrid_hotspot: bool = False, reassembly_size: int = 10, q_threshold: int = 10, mapq_threshold: int = 10,
                    feature_length: int = 150, stats: Optional[dict] = None) -> List[Site]:
    """caller_calling.main (:784-893) up to the featurizer with two BAMs."""
    st = {k: 0 for k in STAT_KEYS}
    locations: List[Tuple[int, int]] = []
    for start, stop in cr.active_regions(positions):
        st["active_regions"] += 1
        s = Searcher(illumina_reads, pacbio_reads, reference, start, stop, max(0, start - cr.FLANKING_BASES), stop + cr.FLANKING_BASES,
                     q_threshold, mapq_threshold, hybrid_hotspot)
        if s.status == "no_reads":
            st["regions_without_reads"] += 1
        elif s.status == "out_of_bounds":
            st["regions_out_of_bounds"] += 1
        else:
            st["regions_at_read_cap"] += int(s.capped)
        locations += s.regions
    locations.sort()
    for a, b in zip(locations, locations[1:]):
        assert a[1] < b[0], "differing regions of different active regions overlap or touch"
    st["differing_regions_pass1"] = len(locations)
    st["regions_pass1"] = list(locations)
    st["regions_pass2"] = []
    st["clusters_skipped_for_size"] = 0                     # gate open, regions >= reassembly_size (not a statistic of the library)
    sites: List[Site] = []
    for cluster in cr.cluster_locations(locations):
        st["clusters"] += 1
        start = cluster[0][0] - cr.MIN_DISTANCE // 2
        stop = cluster[-1][1] + cr.MIN_DISTANCE // 2 - 1
        s = Searcher(illumina_reads, pacbio_reads, reference, start, stop, start, stop, q_threshold, mapq_threshold, hybrid_hotspot)
        if s.status == "no_reads":
            st["clusters_without_reads"] += 1
            continue
        if s.status == "out_of_bounds":
            st["clusters_out_of_bounds"] += 1
            continue
        st["clusters_at_read_cap"] += int(s.capped)
        st["differing_regions_pass2"] += len(s.regions)
        st["regions_pass2"] += s.regions
        before = st["clusters_gate_passed"], st["clusters_reassembled"]
        sites += sites_of_cluster(s, illumina_reads, reference, q_threshold, mapq_threshold, feature_length, reassembly_size, st)
        if st["clusters_gate_passed"] > before[0] and st["clusters_reassembled"] == before[1] and len(s.regions) >= reassembly_size:
            st["clusters_skipped_for_size"] += 1
    st["sites"] = len(sites)
    st["alleles"] = sum(len(s.alleles) for s in sites)
    st["reads_gathered"] = sum(len(r0) + len(r1) for s in sites for _, r0, r1 in s.alleles)
    if stats is not None:
        stats.update(st)
    return sites


def candidate_sites(sites: Sequence[Site], chromosome: str):
    """The sites as hello_amd.shards.CandidateSite objects with both technologies (an empty list, not None, for a technology
    without support: has_second is set)."""
    from hello_amd.featurizer import AlignedRead
    from hello_amd.shards import CandidateSite

    def aligned(r):                    # every read's own HP tag (here: a leading HP:C tag of the test reads), whatever its container
        hp = r.tags[3] if r.tags[:3] == b"HPC" else getattr(r, "hp", 0)
        return AlignedRead(r.seq, list(r.qual), list(r.cigar), r.pos, r.mapq, -1 if r.is_reverse else 1, hp)
    out = []
    for s in sites:
        alleles = [(text, [aligned(s.reads0[i]) for i in i0], [aligned(s.reads1[i]) for i in i1]) for text, i0, i1 in s.alleles]
        out.append(CandidateSite(chromosome, s.start, s.stop, s.reference, s.window_start, alleles))
    return out
