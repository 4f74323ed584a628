"""CPU tests of the two-BAM candidate stage: the hand-derived cases that pin tests/hybrid_reference.py (expected sites, alleles
and per-technology supports written out), the coverage rule, the command lines and the new symbols of the C ABI."""
import ctypes
import os
import re

import pytest

from tests import hybrid_reference as hy
from tests.bam_writer import Read
from tests.test_candidates import REF, _match, _names, _snv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# REF with C TTTTTTTT put in front of position 300: RUN[300] = C, RUN[301:309] = T * 8, RUN[309] = G = REF[300]; RUN[299] = A
RUN = REF[:300] + "C" + "T" * 8 + REF[300:]
assert RUN[298:311] == "CACTTTTTTTTGA"


def _plain(name, pos, length, ref=RUN, edits=(), q=30, **kw):
    """A read of `ref` without indels; `edits`: (position, base, quality) substitutions."""
    seq, qual = list(ref[pos:pos + length]), [q] * length
    for at, base, bq in edits:
        seq[at - pos], qual[at - pos] = base, bq
    return Read(name, pos, [(0, length)], "".join(seq), qual, **kw)


def _del1(name, pos, length, at, ref=RUN, edits=(), **kw):
    """A read of `ref` with the one base at `at` deleted."""
    r = _plain(name, pos, length, ref, edits)
    k = at - pos
    return Read(name, pos, [(0, k), (2, 1), (0, length - k - 1)], r.seq[:k] + r.seq[k + 1:], r.qual[:k] + r.qual[k + 1:], **kw)


def repeat_reads(n_illumina_ref=8, edits_i=(), edits_left=(), edits_p_del=(), edits_p_ref=(), extra_pacbio=()):
    """One T of the run RUN[301:309] is missing in the donor.  The Illumina reads that carry it delete the first T (301: planted
    at 300 with reference allele CT, it flags 300..302), the PacBio reads the last (308: planted at 307 with TT, flags 307..309):
    two regions, (300, 303) and (307, 310).  There the Illumina reads spell CT | TTG (deletion) and CTT | TTG, the PacBio reads
    CTT | TG (deletion) and CTT | TTG.  Over [294, 316) the PacBio deletion reads' haplotype is C TTTTTTT G -- what the Illumina
    choice CT + TTG spells."""
    illumina = [_plain(f"r{i}", 250, 100, edits=edits_i) for i in range(n_illumina_ref)]
    illumina += [_del1(f"d{i}", 250, 100, 301, edits=tuple(edits_i) + tuple(edits_left)) for i in range(7)]
    pacbio = [_plain(f"pr{i}", 30, 540, edits=edits_p_ref) for i in range(3)] + [_del1(f"pd{i}", 30, 540, 308, edits=edits_p_del) for i in range(3)]
    return illumina, sorted(pacbio + list(extra_pacbio), key=lambda r: r.pos)


def hybrid_hand_cases():
    """(name, Illumina reads, PacBio reads, reference, positions, keyword arguments,
    expected [(start, stop, [(allele, [Illumina read names], [PacBio read names])])], expected statistics)."""
    cases = []
    refs, alts = [_match(f"r{i}", 250, 100) for i in range(6)], [_snv(f"t{i}", 250, 100, 300, "T") for i in range(6)]
    prefs, palts = [_match(f"pr{i}", 30, 540) for i in range(4)], [_snv(f"pt{i}", 30, 540, 300, "T") for i in range(4)]
    # an SNV G>T at 300 in both read sets: 6 of 12 Illumina reads, 4 of 8 PacBio reads.  12 Illumina reads: the gate is closed.
    cases.append(("snv in both sets", refs + alts, prefs + palts, REF, [300], {},
                  [(300, 301, [("G", _names("r", 6), _names("pr", 4)), ("T", _names("t", 6), _names("pt", 4))])],
                  dict(clusters=1, clusters_gate_passed=0, clusters_reassembled=0, pacbio_reads_eligible=0)))
    # the same with HP tags: Illumina T reads HP 1, PacBio G reads HP 1, PacBio T reads HP 2 -- every read keeps its own tag
    cases.append(("snv in both sets, HP tags", refs + [_snv(f"t{i}", 250, 100, 300, "T", tags=b"HPC\x01") for i in range(6)],
                  [_match(f"pr{i}", 30, 540, tags=b"HPC\x01") for i in range(4)] + [_snv(f"pt{i}", 30, 540, 300, "T", tags=b"HPC\x02") for i in range(4)],
                  REF, [300], {}, [(300, 301, [("G", _names("r", 6), _names("pr", 4)), ("T", _names("t", 6), _names("pt", 4))])], {}))
    # only the Illumina reads carry T: the allele is kept with no PacBio read ...
    cases.append(("an Illumina-only allele", refs + alts, prefs, REF, [300], {},
                  [(300, 301, [("G", _names("r", 6), _names("pr", 4)), ("T", _names("t", 6), [])])], {}))
    # ... only the PacBio reads carry it (4 of 8 in table 1): kept with no Illumina read
    cases.append(("a PacBio-only allele", refs + [_match(f"s{i}", 250, 100) for i in range(6)], prefs + palts, REF, [300], {},
                  [(300, 301, [("G", _names("r", 6) + _names("s", 6), _names("pr", 4)), ("T", [], _names("pt", 4))])], {}))
    # the repeat, 15 Illumina reads (15 > 14: the gate is open): the PacBio deletion reads take CT | TTG
    il, pb = repeat_reads(8)
    open_sites = [(300, 303, [("CTT", _names("r", 8), _names("pr", 3)), ("CT", _names("d", 7), _names("pd", 3))]),
                  (307, 310, [("TTG", _names("r", 8) + _names("d", 7), _names("pr", 3) + _names("pd", 3))])]
    cases.append(("reconciliation, 15 Illumina reads", il, pb, RUN, [301, 308], {}, open_sites,
                  dict(clusters=1, clusters_gate_passed=1, clusters_reassembled=1, pacbio_reads_eligible=6, pacbio_reads_reassigned=6,
                       pacbio_reads_reassigned_by_tie=0, illumina_sites=2, differing_regions_pass2=2)))
    # 14 Illumina reads: 14 > 14 is false, the gate is closed and the PacBio reads keep CTT | TG
    il, pb = repeat_reads(7)
    closed_sites = [(300, 303, [("CTT", _names("r", 7), _names("pr", 3) + _names("pd", 3)), ("CT", _names("d", 7), [])]),
                    (307, 310, [("TTG", _names("r", 7) + _names("d", 7), _names("pr", 3)), ("TG", [], _names("pd", 3))])]
    cases.append(("reconciliation, 14 Illumina reads", il, pb, RUN, [301, 308], {}, closed_sites,
                  dict(clusters_gate_passed=0, clusters_reassembled=0, pacbio_reads_eligible=0, pacbio_reads_reassigned=0)))
    # eligibility: [start, stop) = [294, 316).  "late" starts at 295 > 294, "early" ends at 315 (last_position 315 < 316): both
    # carry the PacBio deletion and keep TG; the others are reassigned
    late, early = _del1("late", 295, 300, 308), _del1("early", 30, 286, 308)
    il, pb = repeat_reads(8, extra_pacbio=[late, early])
    cases.append(("eligibility", il, pb, RUN, [301, 308], {},
                  [(300, 303, [("CTT", _names("r", 8), _names("pr", 3) + ["early", "late"]), ("CT", _names("d", 7), _names("pd", 3))]),
                   (307, 310, [("TTG", _names("r", 8) + _names("d", 7), _names("pr", 3) + _names("pd", 3)), ("TG", [], ["early", "late"])])],
                  dict(pacbio_reads_eligible=6, pacbio_reads_reassigned=6)))
    # reassembly size: the Illumina deletion reads and the PacBio deletion reads also carry SNVs to A at 314 (C), 317 (G), 320 (T),
    # 324 (G), 327 (C), 330 (T), 333 (C) and 336 (G).  The first 7 of them: 9 regions < 10, reassembled; all 8: 10 regions, not
    # reassembled -- unless the reassembly size is 11
    snv_at = [314, 317, 320, 324, 327, 330, 333, 336]
    assert "".join(RUN[p] for p in snv_at) == "CGTGCTCG"
    for n_snv, size_kw in ((7, {}), (8, {}), (8, dict(reassembly_size=11))):
        at = snv_at[:n_snv]
        edits = tuple((p, "A", 30) for p in at)
        il, pb = repeat_reads(8, edits_left=edits, edits_p_del=edits)
        reassembled = n_snv + 2 < size_kw.get("reassembly_size", 10)
        sites = list(open_sites if reassembled else
                     [(300, 303, [("CTT", _names("r", 8), _names("pr", 3) + _names("pd", 3)), ("CT", _names("d", 7), [])]),
                      (307, 310, [("TTG", _names("r", 8) + _names("d", 7), _names("pr", 3)), ("TG", [], _names("pd", 3))])])
        sites += [(p, p + 1, [(RUN[p], _names("r", 8), _names("pr", 3)), ("A", _names("d", 7), _names("pd", 3))]) for p in at]
        cases.append((f"{n_snv + 2} regions, reassembly size {size_kw.get('reassembly_size', 10)}", il, pb, RUN, [301, 308] + at, size_kw, sites,
                      dict(clusters=1, clusters_gate_passed=1, clusters_reassembled=int(reassembled),
                           pacbio_reads_reassigned=6 if reassembled else 0, differing_regions_pass2=n_snv + 2)))
    # the tie rule: Illumina reads delete the first T (5 reads: CT | TTG) or the last (5 reads: CTT | TG); one PacBio read lacks a
    # T.  Its haplotype C TTTTTTT G is spelled by CT + TTG and by CTT + TG.  Ascending bytes: (CT, CTT) and (TG, TTG); the index
    # tuples are (0, 1) and (1, 0); (0, 1) is smaller: CT | TTG.  The PacBio reference reads spell C TTTTTTTT G: CTT + TTG only.
    il = ([_plain(f"r{i}", 250, 100) for i in range(6)] + [_del1(f"d{i}", 250, 100, 301) for i in range(5)]
          + [_del1(f"e{i}", 250, 100, 308) for i in range(5)])
    pb = [_plain(f"pr{i}", 30, 540) for i in range(3)] + [_del1("pd0", 30, 540, 308)]
    cases.append(("the tie rule", il, pb, RUN, [301, 308], {},
                  [(300, 303, [("CTT", _names("r", 6) + _names("e", 5), _names("pr", 3)), ("CT", _names("d", 5), ["pd0"])]),
                   (307, 310, [("TTG", _names("r", 6) + _names("d", 5), _names("pr", 3) + ["pd0"]), ("TG", _names("e", 5), [])])],
                  dict(clusters_reassembled=1, pacbio_reads_eligible=4, pacbio_reads_reassigned=4, pacbio_reads_reassigned_by_tie=1,
                       illumina_sites=2)))
    # a region that is no Illumina site: at 330 (RUN[330] = T) every Illumina base has quality 5 (no passing record); three PacBio
    # reads "ps" carry A there (3 of 6 in table 1).  The reassigned deletion reads lose their record T at 330: the reference
    # allele is left without support.  "ps" spell A at 330, which no choice of Illumina alleles does: eligible, not reassigned.
    assert RUN[330] == "T"
    il, pb = repeat_reads(8, edits_i=((330, "T", 5),), edits_p_ref=((330, "A", 30),))
    pb = [Read(r.name.replace("pr", "ps"), r.pos, r.cigar, r.seq, r.qual) for r in pb]
    cases.append(("a region without a passing Illumina record", il, pb, RUN, [301, 308, 330], {},
                  [(300, 303, [("CTT", _names("r", 8), _names("ps", 3)), ("CT", _names("d", 7), _names("pd", 3))]),
                   (307, 310, [("TTG", _names("r", 8) + _names("d", 7), _names("ps", 3) + _names("pd", 3))]),
                   (330, 331, [("A", [], _names("ps", 3))])],
                  dict(differing_regions_pass2=3, illumina_sites=2, pacbio_reads_eligible=6, pacbio_reads_reassigned=3)))
    # an empty PacBio BAM: the regions of the Illumina-only path, no PacBio read anywhere; both BAMs empty: no regions
    cases.append(("an empty PacBio BAM", refs + alts, [], REF, [300], {},
                  [(300, 301, [("G", _names("r", 6), []), ("T", _names("t", 6), [])])], dict(regions_without_reads=0)))
    cases.append(("both BAMs empty", [], [], REF, [300], {}, [], dict(active_regions=1, regions_without_reads=1, clusters=0)))
    # --hybrid_hotspot, the hotspot stage's hand case: one Illumina read and one PacBio read carry T.  Without it table 0 counts
    # 1 < 2 and table 1 counts 1 < 2: nothing.  With it vi + vp = 2 >= 2 of a total of 6: {300}.
    il, pb = refs[:2] + alts[:1], prefs[:2] + palts[:1]
    cases.append(("one read each, without hybrid_hotspot", il, pb, REF, [300], {}, [], dict(differing_regions_pass1=0)))
    cases.append(("one read each, with hybrid_hotspot", il, pb, REF, [300], dict(hybrid_hotspot=True),
                  [(300, 301, [("G", _names("r", 2), _names("pr", 2)), ("T", ["t0"], ["pt0"])])], dict(differing_regions_pass1=1)))
    return [(n, sorted(i, key=lambda r: r.pos), sorted(p, key=lambda r: r.pos), ref, pos, kw, want, st) for n, i, p, ref, pos, kw, want, st in cases]


def site_names(sites):
    return [(s.start, s.stop, [(a, [s.reads0[i].name for i in i0], [s.reads1[i].name for i in i1]) for a, i0, i1 in s.alleles]) for s in sites]


@pytest.mark.parametrize("case", hybrid_hand_cases(), ids=lambda c: c[0])
def test_restatement_hand_cases(case):
    name, illumina, pacbio, reference, positions, kw, expected, expected_stats = case
    st = {}
    sites = hy.find_candidates(illumina, pacbio, reference, positions, stats=st, **kw)
    assert site_names(sites) == expected, name
    assert {k: st[k] for k in expected_stats} == expected_stats, name
    for s in sites:                                   # technology 1's reads are the clipped copies (flank 200 around the cluster)
        for r, original in zip(s.reads1, s.originals1):
            assert r.name == original.name and (len(original.seq) < 539 or len(r.seq) < 500)


def test_has_second_is_set_and_the_shard_holds_both_technologies():
    from hello_amd import shards
    name, illumina, pacbio, reference, positions, kw, expected, _ = hybrid_hand_cases()[2]
    assert name == "an Illumina-only allele"
    sites = hy.find_candidates(illumina, pacbio, reference, positions)
    payload = shards._payload(hy.candidate_sites(sites, "chr1"))
    assert int(payload["has_second"]) == 1
    assert payload["reads_per_allele0"].tolist() == [6, 6] and payload["reads_per_allele1"].tolist() == [4, 0]
    shard = shards.PackedShard(payload)
    assert shard.hybrid and len(payload["read_off1"]) - 1 == 4 and shard.n_reads(1) == 5      # 4 reads and one dummy read


def test_every_read_keeps_its_own_hp_tag():
    """The reference hands its searcher the last container's hp list for all reads (python/AlleleSearcherLite.py:125); here the
    Illumina reads of the shard carry the Illumina BAM's tags and the PacBio reads the PacBio BAM's."""
    from hello_amd import shards
    name, illumina, pacbio, reference, positions, kw, expected, _ = hybrid_hand_cases()[1]
    assert name == "snv in both sets, HP tags"
    payload = shards._payload(hy.candidate_sites(hy.find_candidates(illumina, pacbio, reference, positions), "chr1"))
    assert payload["hp0"].tolist() == [0] * 6 + [1] * 6                 # G: r0-5 untagged; T: t0-5 HP 1
    assert payload["hp1"].tolist() == [1] * 4 + [2] * 4                 # G: pr0-3 HP 1; T: pt0-3 HP 2


def test_coverage_rule():
    def read(name, pos, cigar, quals, mapq=60, flag=0):
        n = sum(k for op, k in cigar if op in (0, 1, 4, 7, 8))
        return Read(name, pos, cigar, "A" * n, quals if isinstance(quals, list) else [quals] * n, flag, mapq)
    # mapq 9 against 10: the columns of a low-mapq read exist, it counts at none
    assert hy.coverage_gate([read("a", 100, [(0, 10)], 30, mapq=10)], 100, 110) == (10, 10)
    assert hy.coverage_gate([read("a", 100, [(0, 10)], 30, mapq=9)], 100, 110) == (0, 10)
    # base quality 12 against 13
    assert hy.coverage_gate([read("a", 100, [(0, 4)], [13, 12, 13, 12])], 100, 110) == (2, 4)
    # a deletion: its 3 columns count with the quality of the read base before it (13: yes, 12: no); an N skip likewise; an
    # insertion and a soft clip add no column
    assert hy.coverage_gate([read("a", 100, [(0, 2), (2, 3), (0, 2)], [30, 13, 30, 30])], 100, 110) == (7, 7)
    assert hy.coverage_gate([read("a", 100, [(0, 2), (2, 3), (0, 2)], [30, 12, 30, 30])], 100, 110) == (3, 7)
    assert hy.coverage_gate([read("a", 100, [(4, 1), (0, 2), (3, 3), (1, 2), (0, 2)], 30)], 100, 110) == (7, 7)
    assert hy.coverage_gate([read("a", 100, [(2, 3), (0, 2)], 30)], 100, 110) == (2, 5)          # no read base before: no count
    # columns outside the interval count: the read overlaps [100, 110) by one base and has 50 columns
    assert hy.coverage_gate([read("a", 60, [(0, 50)], 30)], 109, 120) == (50, 50)
    assert hy.coverage_gate([read("a", 60, [(0, 50)], 30)], 110, 120) == (0, 0)                  # ends at 110: no overlap
    # the read filter: unmapped, secondary, supplementary, QC-fail, duplicate, paired but not proper are out; a proper pair and
    # mapq 0 (columns only) are in; the same read twice counts twice (before de-duplication)
    for flag in (0x4, 0x100, 0x800, 0x200, 0x400, 0x1):
        assert hy.coverage_gate([read("a", 100, [(0, 10)], 30, flag=flag)], 100, 110) == (0, 0), flag
    assert hy.coverage_gate([read("a", 100, [(0, 10)], 30, flag=0x3), read("a", 100, [(0, 10)], 30, flag=0x3)], 100, 110) == (20, 10)
    assert hy.coverage_gate([read("a", 100, [(0, 10)], 30, mapq=0)], 100, 110) == (0, 10)
    # the gate is strict: 14 reads over the same 10 columns give 140 > 140: closed; 15 give 150: open
    fourteen = [read(f"r{i}", 100, [(0, 10)], 30) for i in range(14)]
    total, columns = hy.coverage_gate(fourteen, 100, 110)
    assert (total, columns) == (140, 10) and not total > hy.MIN_COVERAGE * columns
    total, columns = hy.coverage_gate(fourteen + [read("x", 100, [(0, 10)], 30)], 100, 110)
    assert total > hy.MIN_COVERAGE * columns


def test_haplotype_enumeration_and_tie_rule():
    ref = "ACGTACGTAC"
    # sites (2, 3) {G, T} and (6, 7) {G}: over [0, 10) four ... two haplotypes
    table = hy.enumerate_haplotypes([((2, 3), ["G", "T"]), ((6, 7), ["G"])], ref, 0, 10)
    assert table == {"ACGTACGTAC": ((0, 0), 1), "ACTTACGTAC": ((1, 0), 1)}
    # two sites inside AAAA: (1, 3) {A, AA} and (3, 5) {A, AA}: A + AA and AA + A spell the same text; (0, 1) < (1, 0)
    table = hy.enumerate_haplotypes([((1, 3), ["A", "AA"]), ((3, 5), ["A", "AA"])], "CAAAAC", 0, 6)
    assert table == {"CAAC": ((0, 0), 1), "CAAAC": ((0, 1), 2), "CAAAAC": ((1, 1), 1)}
    assert hy.enumerate_haplotypes([], ref, 0, 10) == {"": ((), 1)}
    assert hy.haplotype_string([], ref, 2, 8) == "GTACGT"
    assert hy.haplotype_string([("", 3, 4, 60), ("GGG", 6, 7, 30)], ref, 2, 8) == "G" + "" + "AC" + "GGG" + "T"


def test_parsers():
    from hello_amd import call, hybrid
    a = hybrid.parser().parse_args(["--bam", "i.bam,p.bam", "--ref", "g.fa", "--activity", "shard0.txt", "--outputPrefix", "out/shard0"])
    assert (a.hybrid_hotspot, a.reconcilement_size, a.featureLength, a.q_threshold, a.mapq_threshold, a.device) == (False, 10, 150, 10, 10, 0)
    a = hybrid.parser().parse_args(["--bam", "i.bam,p.bam", "--ref", "g.fa", "--activity", "s.txt", "--outputPrefix", "o", "--hybrid_hotspot",
                                    "--reconcilement_size", "4"])
    assert (a.hybrid_hotspot, a.reconcilement_size) == (True, 4)
    assert hybrid.split_bams("i.bam,p.bam") == ("i.bam", "p.bam") and hybrid.split_bams(["i.bam", "p.bam"]) == ("i.bam", "p.bam")
    for bad in ("i.bam", "a,b,c", ["i.bam"], "i.bam,"):
        with pytest.raises(ValueError, match="two BAMs"):
            hybrid.split_bams(bad)
    with pytest.raises(SystemExit):
        hybrid.parser().parse_args(["--bam", "i.bam,p.bam", "--ref", "g.fa"])
    base = ["--workdir", "w", "--network", "m.npz"]
    a = call.parser().parse_args(base + ["--from_bams", "--ibam", "i.bam", "--pbam", "p.bam", "--ref", "g.fa", "--hybrid_hotspot",
                                         "--reconcilement_size", "7"])
    assert a.from_bams and not a.from_bam and (a.hybrid_hotspot, a.reconcilement_size) == (True, 7)
    assert not call.parser().parse_args(base).from_bams
    assert "--from_bams" in call._argv_of(a)
    with pytest.raises(ValueError, match="--from_bams needs one --ibam and one --pbam"):
        call.shards_from_bams(call.parser().parse_args(base + ["--from_bams", "--ibam", "i.bam", "--ref", "g.fa"]))
    with pytest.raises(SystemExit, match="exclude each other"):
        call.main(call.parser().parse_args(base + ["--from_bams", "--from_bam", "--ibam", "i.bam", "--pbam", "p.bam", "--ref", "g.fa"]))
    with pytest.raises(SystemExit, match="--from_bams needs --ref"):
        call.main(call.parser().parse_args(base + ["--from_bams", "--ibam", "i.bam", "--pbam", "p.bam"]))


def test_abi_symbols_are_declared_exported_and_mirrored():
    from hello_amd import hybrid
    from hello_amd.engine import load_library
    header = open(os.path.join(ROOT, "include", "hello_mi355x.h")).read()
    lib = load_library()
    for symbol in ("hello_candidates_find_hybrid", "hello_candidates_array_tech", "hello_candidates_hybrid_stats"):
        assert re.search(r"\bint %s\(" % symbol, header), symbol
        assert hasattr(lib, symbol), symbol
    assert int(re.search(r"#define HELLO_CANDIDATES_HYBRID_STATS (\d+)", header).group(1)) == hybrid.N_STATS == len(hybrid.STAT_NAMES) == 29
    assert int(re.search(r"#define HELLO_CANDIDATES_STATS (\d+)", header).group(1)) == 22           # unchanged
    bound = hybrid._lib()
    assert len(bound.hello_candidates_find_hybrid.argtypes) == 2 * 12 + 11
    # the entry points that need no GPU: NULL handles are refused with HELLO_ERR_ARG
    data, count = ctypes.c_void_p(), ctypes.c_int64()
    assert bound.hello_candidates_array_tech(None, 1, 8, ctypes.byref(data), ctypes.byref(count)) == -1
    assert bound.hello_candidates_hybrid_stats(None, (ctypes.c_double * 29)()) == -1
    out = ctypes.c_void_p()
    args = [None] * 11 + [0] + [None] * 11 + [0] + [None, 0, None, 0, 0, 10, 150, 10, 10, 0, ctypes.byref(out)]
    assert bound.hello_candidates_find_hybrid(*args) == -1 and b"NULL" in bound.hello_last_error()
