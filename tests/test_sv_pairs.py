"""The read pairs and clipped ends on the CPU: the restatement of hello_amd/sv.py against the cases worked by
hand (tests/sv_pairs_cases.py), whole and cut into spans; ``hello_sv_cluster_pairs`` against ``assigned`` / ``clustered_pairs``;
``library_of`` against a computation over the sorted values; ``fetch_pairs`` through BAMs written by tests/mate_writer.py; the
refusals that need no device; the VCF text; ``--sv_pairs`` on the command lines; and csrc/sv_pairs.h as a stand-alone program under
AddressSanitizer and UBSan (tests/abi/sv_pairs_check.cpp) over the hand cases, the stress and the fuzz, against the restatement."""
import argparse
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

from hello_amd import call, sv
from hello_amd.bam import BamFile, Mates, Splits
from tests import sv_cases as sc, sv_pairs_cases as pc, sv_split_cases as ss
from tests.test_sv import rows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLUSTER_NAMES = ("TYPE", "POS", "LEN", "DV", "SR", "PR", "IMPRECISE", "CE", "DP", "DR", "END_MIN", "END_MAX")
_made: dict = {}


def restated(rows, reference, library, params, cuts=()):
    kw = dict(params)
    clip_min = kw.pop("clip_min")
    return sv.restated_pairs(pc.spans_of(rows, len(reference), cuts), reference, library, pc.CONTIGS, pc.OWN, clip_min=clip_min, **kw)


def stress_restated(name: str):
    if name not in _made:
        _made[name] = restated(pc.STRESS_SETS[name], pc.STRESS_REFERENCE, pc.STRESS_LIBRARY, pc.STRESS)
    return _made[name]


def fuzz_restated(seed: int):
    if seed not in _made:
        reference, rows = pc.fuzz(seed)
        _made[seed] = (reference, rows) + restated(rows, reference, pc.FUZZ_LIBRARY, pc.FUZZ)
    return _made[seed]


def clusters_of(tables):
    return rows_of(tables, "CANDIDATES_", CLUSTER_NAMES)


# ---- the restatement against the hand cases -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.HAND_TABLE, ids=[c.name for c in pc.HAND_TABLE])
def test_restatement_equals_the_hand_cases_whole_and_cut(case):
    for cuts in ((), (case.cut(),)):
        tables, counts = restated(case.rows, case.reference, pc.LIBRARY, case.kw(), cuts)
        assert rows_of(tables, "SIGNATURES_", sv.SIGNATURE_COLUMNS) == case.signatures
        assert clusters_of(tables) == case.clusters
        assert {k: counts[k] for k in sv.PAIR_COUNT_NAMES} == case.want_counts()
        for c in clusters_of(tables):                                        # genotype_of(DV + PR, DR)
            row = [r for r in rows_of(tables, "CANDIDATES_", sv.CANDIDATE_COLUMNS) if r[:3] == c[:3]][0]
            assert row[15:] == sv.genotype_of(c[3] + c[5], c[9])
        if not cuts:
            assert tables["PAIR_STATUS"].tolist() == case.pair_status
    assert pc.LENGTH == len(case.reference) == sc.LENGTH


def test_the_three_conventions_are_pinned():
    by_name = {c.name: c for c in pc.HAND_TABLE}
    first = by_name["a 40D of three reads takes the four pairs that straddle it"]
    proper = by_name["flag 0x2 on a discordant pair: still a row, and pair supporters are not in DP"]
    spanned = by_name["a normal pair that spans the event is no reference support"]
    both = by_name["a read with a split row and a pair row counts in SR and in PR"]
    assert first.clusters == proper.clusters == spanned.clusters            # DP 3, DR 0 whether the pairs count as reads or not
    assert sv.genotype_of(7, 0)[0] == 2
    (cluster,) = both.clusters
    assert cluster[3:6] == (1, 1, 1) and len({g[4] for g in both.signatures}) == 1      # one read: DV 1, SR 1 and PR 1


def test_clip_arrays_of_the_hand_case_and_the_filter():
    tables, counts = restated(pc.CLIP_CASE.rows, pc.REFERENCE, pc.LIBRARY, pc.HAND)
    for name, want in pc.CLIPS.items():
        assert tables[name].dtype == np.int32 and tables[name].shape == (pc.LENGTH + 1,)
        assert {int(i): int(tables[name][i]) for i in np.flatnonzero(tables[name])} == want
    assert sv.clip_sum(tables["CLIP_LEFT"], tables["CLIP_RIGHT"], 118, 131, 3) == 2 and sv.clip_sum(tables["CLIP_LEFT"], tables["CLIP_RIGHT"], 120, 122, 3) == 1
    assert sv.clip_sum(tables["CLIP_LEFT"], tables["CLIP_RIGHT"], 0, pc.LENGTH, 3) == 0
    assert sv.pair_counted(0x1, 10, 10) and sv.pair_counted(0x1 | 0x2, 60, 10) and not sv.pair_counted(0x2, 60, 10)
    for bit in (0x4, 0x8, 0x100, 0x800, 0x400, 0x200):
        assert not sv.pair_counted(0x1 | bit, 60, 10)
    assert not sv.pair_counted(0x1, 9, 10)


def test_reads_beyond_the_end_of_the_chromosome_touch_no_array():
    case = pc.END_CASE
    tables, counts = restated(case.rows, case.reference, pc.LIBRARY, case.kw())
    for name, want in pc.END_CLIPS.items():
        assert {int(i): int(tables[name][i]) for i in np.flatnonzero(tables[name])} == want
    assert {int(i): int(tables["INNER"][i]) for i in np.flatnonzero(tables["INNER"])} == {1024: 1}       # of the read that ends at 2 600 alone
    reads, splits, mates = pc.pair_set(case.rows)
    assert reads.ref_ends.tolist() == [2600, 2600, 2605, 2605, 2600] and pc.LENGTH == 2600
    beyond = [r for seed in pc.FUZZ_SEEDS for r in pc.fuzz(seed)[1] if r[2] + sum(n for op, n in r[3] if op in (0, 2, 3, 7, 8)) > pc.FUZZ_LENGTH]
    assert len(beyond) > 32 and any(r[1] & 1 for r in beyond) and any(r[3][-1][0] == sc.S for r in beyond)


def test_stress_each_situation_occurs_in_the_restatement():
    for n in pc.EMITTING:
        tables, counts = stress_restated("emitting%d" % n)
        assert counts["pair_signatures"] == n == int((tables["SIGNATURES_TYPE"] == sv.BND).sum()) and counts["pair_reads"] == n
    tables, counts = stress_restated("inner_edges")
    assert {int(i): int(tables["INNER"][i]) for i in np.flatnonzero(tables["INNER"])} == {0: 2, 4095: 2}
    assert sv.pair_outcome(0x61, 0, 2000, 0, 0, 2000 - 1023, 3, sv.UNSET_LIBRARY, 5)[1] == 1
    assert sv.pair_outcome(0x61, 0, 20, 0, 0, 20 + 3070, 3, sv.UNSET_LIBRARY, 5)[1] == 4094
    tables, counts = stress_restated("one_bin")
    assert int(tables["INNER"][1024 + 200]) == 300 == int(tables["INNER"].sum()) and counts["pairs_normal"] == 300
    tables, counts = stress_restated("across")
    # a = 620 .. 635, b = 1500 .. 1510, lens 680 .. 675: the lower median 677; four clipped ends at 633 .. 636, three at 1498 .. 1500
    assert clusters_of(tables) == [(sv.DEL, 635, 677, 0, 0, 6, 1, 7, 0, 0, 1500, 1510)] and counts["clipped_reads"] == 17
    tables, counts = stress_restated("no_pairs")
    assert all(counts[k] == 0 for k in sv.PAIR_COUNT_NAMES) and not tables["INNER"].any() and not tables["CLIP_LEFT"].any()
    for name, rows in pc.STRESS_SETS.items():                                # whole and cut give the same tables
        tables, counts = stress_restated(name)
        cut, cut_counts = restated(rows, pc.STRESS_REFERENCE, pc.STRESS_LIBRARY, pc.STRESS, pc.STRESS_CUTS)
        for k in tables:
            if k not in ("STATUS", "SPLIT_STATUS", "PAIR_STATUS"):
                assert np.array_equal(tables[k], cut[k]), (name, k)
        assert {k: counts[k] for k in sv.PAIR_METRIC_STATS} == {k: cut_counts[k] for k in sv.PAIR_METRIC_STATS}


def test_fuzz_has_what_it_is_run_for():
    seen = dict.fromkeys(sv.PAIR_COUNT_NAMES, 0)
    types = set()
    for seed in pc.FUZZ_SEEDS[:8]:
        _, _, tables, counts = fuzz_restated(seed)
        for k in seen:
            seen[k] += counts[k]
        types |= {(int(t), int(op) == sv.PAIR_OP) for t, op in zip(tables["SIGNATURES_TYPE"], tables["SIGNATURES_OP"])}
    assert all(v > 0 for v in seen.values()), seen
    assert {(t, True) for t in (sv.DEL, sv.DUP, sv.INV3, sv.INV5, sv.BND)} <= types and (sv.DEL, False) in types, types


# ---- the clusters and the library: the library's host rules against the restatement ----------------------------------------------------
def test_cluster_pairs_native_equals_assigned_and_clustered_pairs():
    sets = [(rows_of(fuzz_restated(seed)[2], "SIGNATURES_", sv.SIGNATURE_COLUMNS), pc.FUZZ_LIBRARY, pc.FUZZ) for seed in pc.FUZZ_SEEDS[:8]]
    sets += [(case.signatures, pc.LIBRARY, case.kw()) for case in pc.HAND_TABLE]
    sets += [(rows_of(stress_restated("across")[0], "SIGNATURES_", sv.SIGNATURE_COLUMNS), pc.STRESS_LIBRARY, pc.STRESS), ([], pc.LIBRARY, pc.HAND)]
    some = 0
    for rows, library, p in sets:
        for gap, percent, support in ((p["cluster_gap"], p["len_ratio_percent"], p["min_support"]), (0, 100, 1), (100, 70, 3)):
            want, n_assigned = sv.clustered_with_pairs(rows, library, p["flank"], gap, percent, support)
            assert sv.clustered_pairs_native(rows, library, p["flank"], gap, percent, support) == want
            assert sv.clustered_pairs_native(rows[::-1], library, p["flank"], gap, percent, support) == want
            plain = [g for g in rows if g[5] != sv.PAIR_OP and g[0] != sv.BND]           # 7p / 7q's clusters are formed as before
            assert [c[:14] for c in want if not c[17]] == sv.clustered(plain, gap, percent, support, with_sr=True)
            some += n_assigned + sum(c[17] for c in want)
    assert some > 20
    # assigned / clustered_pairs by hand: the first cluster in (pos, type, len) order that accepts a row takes it
    clusters = [(sv.DEL, 100, 50), (sv.DEL, 102, 50), (sv.DUP, 100, 50)]
    rows = [(sv.DEL, 99, 55, 164, 0, sv.PAIR_OP, 0, 0), (sv.DEL, 106, 55, 160, 1, sv.PAIR_OP, 0, 0), (sv.DUP, 110, 45, 155, 2, sv.PAIR_OP, 1, 0),
            (sv.DUP, 120, 45, 155, 3, sv.PAIR_OP, 1, 0), (sv.BND, 100, 1, 5, 4, sv.PAIR_OP, 0, 0)]
    pr, left = sv.assigned(clusters, rows, pc.LIBRARY, 3)
    assert pr == [1, 0, 1] and left == [rows[1], rows[3]]                    # 106 - 3 > 100 and 102; |120 - 100| > 16
    with pytest.raises(RuntimeError, match=r"library \(10, 11, 16\)"):
        sv.clustered_pairs_native([], (10, 11, 16), 3)
    with pytest.raises(RuntimeError, match="signature 0: type 6"):
        sv.clustered_pairs_native([(6, 5, 9, 0, 0, sv.PAIR_OP, 0, 0)], pc.LIBRARY, 3)


def test_library_of_equals_a_sorted_array_computation():
    rng = np.random.default_rng(5)
    for trial in range(40):
        n = int(rng.integers(1, 400))
        values = np.round(rng.normal(rng.integers(-900, 2900), rng.integers(1, 200), n)).astype(np.int64)
        if trial % 4 == 0:
            values[: n // 3] = rng.integers(-3000, 6000, n // 3)             # outliers that land in the clamped bins
        bins = np.clip(values + 1024, 0, 4095)
        histogram = np.bincount(bins, minlength=4096).astype(np.int64)
        ordered = np.sort(bins)
        median = int(ordered[(n - 1) // 2])
        inside = ordered[(ordered > 0) & (ordered < 4095)]
        mad = int(np.sort(np.abs(inside - median))[(inside.shape[0] - 1) // 2]) if inside.shape[0] else 1
        k = int(rng.integers(1, 12))
        want = (median - 1024, median - 1024 - k * max(mad, 1), median - 1024 + k * max(mad, 1))
        assert sv.library_of(histogram, k) == want == sv.library_of_native(histogram, k)
    with pytest.raises(ValueError, match="empty histogram"):
        sv.library_of(np.zeros(4096, np.int64))
    with pytest.raises(RuntimeError, match="empty histogram"):
        sv.library_of_native(np.zeros(4096, np.int64))


# ---- the BAM reader -------------------------------------------------------------------------------------------------------------
def _mated_reads(rows, reference):
    from tests.mate_writer import MatedRead
    out = []
    for k, r in enumerate(rows):
        tags = (b"SAZ" + r[8] + b"\0" if r[8] else b"") + (b"HPC" + bytes([r[7]]) if r[7] else b"")
        out.append(MatedRead("r%d" % k, r[2], r[3], r[4], r[5], flag=r[1], mapq=r[6], tags=tags, next_ref_id=r[9], next_pos=r[10],
                             tlen=(-1) ** k * (100 + k)))
    return out


def test_fetch_pairs_round_trips_the_mate_fields(tmp_path):
    from tests.mate_writer import write_bam
    case = pc.HAND_TABLE[0]
    rows = case.rows + [r for r in pc.HAND_TABLE[8].rows] + pc.HAND_TABLE[13].rows
    rows = sorted(rows, key=lambda r: r[2])
    path = str(tmp_path / "pairs.bam")
    write_bam(path, [("chr1", pc.LENGTH), ("chr2", 1000), ("chrUn_1", 500)], _mated_reads(rows, pc.REFERENCE))
    with BamFile(path) as bam:
        got, splits, mates = bam.fetch_pairs("chr1")
        assert isinstance(splits, Splits) and isinstance(mates, Mates)
        assert mates.tid.dtype == np.int32 and mates.pos.dtype == np.int64 and mates.tlen.dtype == np.int32
        assert mates.tid.tolist() == [r[9] for r in rows] and mates.pos.tolist() == [r[10] for r in rows]
        assert mates.tlen.tolist() == [(-1) ** k * (100 + k) for k in range(len(rows))]
        with_sa, sa = bam.fetch_with_sa("chr1")
        assert np.array_equal(splits.bytes, sa.bytes) and np.array_equal(splits.offsets, sa.offsets) and sa.bytes.shape[0] > 0
        for f in dataclasses.fields(with_sa):
            a, b = getattr(got, f.name), getattr(with_sa, f.name)
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, f.name
        part, _, part_mates = bam.fetch_pairs("chr1", 0, 481)
        assert part.n_reads == 5 and part_mates.pos.tolist() == [r[10] for r in rows[:5]]
        from hello_amd._abi import handle_array
        for entry in (bam._lib.hello_bam_fetch, bam._lib.hello_bam_fetch_mods, bam._lib.hello_bam_fetch_sa):
            r = C.c_void_p()
            assert entry(bam._h, b"chr1", 0, 300, -1, C.byref(r)) == 0
            try:
                for which in (19, 20, 21):
                    with pytest.raises(RuntimeError, match="no read array %d: hello_bam_fetch_pairs alone fills it" % which):
                        handle_array(bam._lib.hello_bam_reads_array, r, which, np.uint8)
            finally:
                bam._lib.hello_bam_reads_free(r)
    # a record without mate fields holds -1, -1, 0, as tests/bam_writer.py writes them
    from tests.bam_writer import Read, write_bam as write_plain
    plain = str(tmp_path / "plain.bam")
    write_plain(plain, [("chr1", pc.LENGTH)], [Read("a", 5, [(sc.M, 10)], pc.REFERENCE[5:15], [30] * 10)])
    with BamFile(plain) as bam:
        _, _, mates = bam.fetch_pairs("chr1")
        assert (mates.tid.tolist(), mates.pos.tolist(), mates.tlen.tolist()) == ([-1], [-1], [0])
    # the restatement reads what the reader gives
    tables, counts = sv.restated_pairs([(got, splits, mates_of(rows), 0, pc.LENGTH)], pc.REFERENCE, pc.LIBRARY, pc.CONTIGS, pc.OWN,
                                       **{k: v for k, v in pc.HAND.items()})
    assert counts["pair_signatures"] == 7 and counts["pairs_assigned"] == 4


def mates_of(rows) -> Mates:
    return pc.pair_set(rows)[2]


# ---- the files ------------------------------------------------------------------------------------------------------------------
def test_vcf_text(tmp_path):
    ref = np.frombuffer(pc.REFERENCE.encode(), np.uint8)
    found = sv.Events(pairs=True)
    found.library, found.library_source = pc.LIBRARY, "given"
    case = pc.HAND_TABLE[0]
    tables, counts = restated(case.rows, case.reference, pc.LIBRARY, case.kw())
    found.set("chr1", ref, tables, counts)
    genotype = sv.genotype_of(7, 0)
    line = ("chr1\t500\t.\t%s\t<DEL>\t.\tPASS\tSVTYPE=DEL;SVLEN=-40;END=540;SUPPORT=7;CIPOS=0,0;CILEN=0,0;STRANDS=3,0;SR=0;PR=4;CE=0\t"
            "GT:GQ:DR:DV:PL:HPS\t%s:%d:0:3:%d,%d,%d:3,0,0\n" % ((pc.REFERENCE[499], sv.GT_TEXT[genotype[0]]) + genotype[1:]))
    assert found.vcf_text() == "##fileformat=VCFv4.2\n##contig=<ID=chr1,length=2600>\n" + sv.PAIRS_VCF_HEADER + line
    for needed in ("##INFO=<ID=PR,", "##INFO=<ID=CE,", "##INFO=<ID=IMPRECISE,", "##INFO=<ID=CIEND,"):
        assert needed in sv.PAIRS_VCF_HEADER and needed not in sv.SPLIT_VCF_HEADER and needed not in sv.VCF_HEADER
    case = [c for c in pc.HAND_TABLE if c.name == "five pairs alone are an imprecise deletion"][0]
    tables, counts = restated(case.rows, case.reference, pc.LIBRARY, case.kw())
    alone = sv.Events(pairs=True)
    alone.library, alone.library_source = pc.LIBRARY, "given"
    alone.set("chr1", ref, tables, counts)
    assert ("chr1\t1004\t.\t%s\t<DEL>\t.\tPASS\tSVTYPE=DEL;SVLEN=-90;END=1099;SUPPORT=5;CIPOS=-6,0;CILEN=-1,1;STRANDS=0,0;SR=0;PR=5;CE=0;"
            "IMPRECISE;CIEND=0,4\tGT:GQ:DR:DV:PL:HPS\t1/1:" % pc.REFERENCE[1003]) in alone.vcf_text()
    assert alone.tables["chr1"]["STATS"].tolist() == [counts[k] for k in sv.PAIR_METRIC_STATS]
    first, again = alone.write_all(str(tmp_path / "a")), alone.write_all(str(tmp_path / "b"))
    assert open(first[1], "rb").read() == open(again[1], "rb").read()
    with np.load(first[1]) as z:
        assert z["library"].tolist() == list(pc.LIBRARY) and str(z["library_source"]) == "given"
        assert z["CANDIDATES_PR_0"].tolist() == [5] and z["CANDIDATES_IMPRECISE_0"].tolist() == [1] and z["CANDIDATES_END_MAX_0"].tolist() == [1103]
        assert set(z["SIGNATURES_OP_0"].tolist()) == {sv.PAIR_OP}
    # without pairs the writers give what they gave: no new header line, no new field, no new array
    split = sv.Events(split=True)
    split.set("chr1", ref, tables, counts)
    assert sv.SPLIT_VCF_HEADER in split.vcf_text() and ";PR=" not in split.vcf_text() and "CANDIDATES_PR" not in split.tables["chr1"]
    assert split.tables["chr1"]["STATS"].shape == (len(sv.SPLIT_METRIC_STATS),)


# ---- the refusals that need no device -------------------------------------------------------------------------------------------------
def test_host_side_refusals():
    case = pc.HAND_TABLE[0]
    reads, splits, mates = pc.pair_set(case.rows)
    with sv.Caller(case.reference, 5, 3) as caller:
        caller.set_contigs(pc.CONTIGS, pc.OWN)
        with pytest.raises(RuntimeError, match="hello_sv_add_pairs before hello_sv_library"):
            caller.add(reads, splits, mates, 0, pc.LENGTH)
        for triple, said in (((10, 11, 16), r"library \(10, 11, 16\): lo <= median <= hi"), ((17, 4, 16), r"library \(17, 4, 16\)")):
            with pytest.raises(RuntimeError, match=said):
                caller.set_library(*triple)
        with pytest.raises(RuntimeError, match="clip_min 0: at least 1"):
            sv.check(caller._lib.hello_sv_clip_min(caller._h, 0))
        caller.set_library(*pc.LIBRARY, clip_min=4)
        with pytest.raises(RuntimeError, match="hello_sv_library twice"):
            caller.set_library(*pc.LIBRARY)
        with pytest.raises(ValueError, match="mate fields for 11 reads"):
            caller.add(reads, splits, Mates(mates.tid[:3], mates.pos, mates.tlen), 0, pc.LENGTH)
        with pytest.raises(RuntimeError, match=r"span \[0, 2601\) of a reference of 2600 bases"):
            caller.add(reads, splits, mates, 0, pc.LENGTH + 1)
        with pytest.raises(RuntimeError, match="SA offsets end at"):
            caller.add(reads, Splits(splits.bytes, splits.offsets + 1), mates, 0, pc.LENGTH)
        stats, arrays = caller.stats(), caller.arrays()
        assert all(v == 0 for v in stats.values()) and set(sv.PAIR_STAT_NAMES) < set(stats)
        assert arrays["INNER"].shape == (4096,) and not arrays["INNER"].any() and arrays["CLIP_LEFT"].shape == (pc.LENGTH + 1,)
        assert arrays["PAIR_STATUS"].shape == (0,) and "CANDIDATES_PR" not in arrays
        with pytest.raises(RuntimeError, match="before hello_sv_finish"):
            sv.handle_array(caller._lib.hello_sv_pairs_array, caller._h, 4, np.int64)
        with pytest.raises(RuntimeError, match="array selector 9"):
            sv.handle_array(caller._lib.hello_sv_pairs_array, caller._h, 9, np.int64)
        caller.finish()
        assert caller.arrays()["CANDIDATES_PR"].shape == (0,)
        with pytest.raises(RuntimeError, match="hello_sv_add_pairs after hello_sv_finish"):
            caller.add(reads, splits, mates, 0, pc.LENGTH)
    with sv.Caller(case.reference, 5, 3) as caller:                          # the unset triple is a library too; contigs are needed
        caller.set_library(*sv.UNSET_LIBRARY)
        with pytest.raises(RuntimeError, match="hello_sv_add_pairs before hello_sv_contigs"):
            caller.add(reads, splits, mates, 0, pc.LENGTH)
    with sv.Caller(case.reference, 5, 3) as caller:                          # the old getters of a handle without pairs are what they were
        assert set(caller.stats()) == set(sv.STAT_NAMES) and "INNER" not in caller.arrays()


def _args(**kw):
    base = dict(sv=False, sv_split=False, sv_pairs=False, shards=None, from_bam=False, from_bams=False, gpus=1, ibam=None, pbam=None)
    base.update(dict.fromkeys(call.SV_OPTIONS + call.SV_PAIRS_OPTIONS))
    base.update(kw)
    return argparse.Namespace(**base)


def test_check_sv_refuses_the_pairs_options_without_their_pass_and_names_the_fix(monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    call.check_sv(_args())
    call.check_sv(_args(sv=True, sv_pairs=True, from_bam=True, ibam="i.bam", sv_pairs_library="200,40,360", sv_pairs_k=6, sv_clip_min=10))
    with pytest.raises(SystemExit, match="--sv_pairs adds the discordant read pairs .* add --sv, or drop --sv_pairs"):
        call.check_sv(_args(sv_pairs=True, from_bam=True))
    for flag, value in (("sv_pairs_library", "1,2,3"), ("sv_pairs_k", 8), ("sv_clip_min", 20)):
        with pytest.raises(SystemExit, match=f"--{flag} is an option of the pass .* add --sv, or drop --{flag}"):
            call.check_sv(_args(from_bam=True, **{flag: value}))
        with pytest.raises(SystemExit, match=f"--{flag} is an option of the read pairs .* add --sv_pairs, or drop --{flag}"):
            call.check_sv(_args(sv=True, from_bam=True, ibam="i.bam", **{flag: value}))
    for text in ("200,40", "a,b,c", "200,300,400", "200,40,100"):
        with pytest.raises(SystemExit, match="--sv_pairs_library .* give for instance --sv_pairs_library 200,40,360"):
            call.check_sv(_args(sv=True, sv_pairs=True, from_bam=True, ibam="i.bam", sv_pairs_library=text))
    with pytest.raises(SystemExit, match="--sv_pairs_k is a number of median absolute deviations: give 1 or more"):
        call.check_sv(_args(sv=True, sv_pairs=True, from_bam=True, ibam="i.bam", sv_pairs_k=0))
    with pytest.raises(SystemExit, match="--sv_clip_min is the fewest bases of a soft clip that counts: give 1 or more"):
        call.check_sv(_args(sv=True, sv_pairs=True, from_bam=True, ibam="i.bam", sv_clip_min=0))
    args = call.parser().parse_args(["--workdir", "w", "--network", "n"])
    assert args.sv_pairs is False and args.sv_pairs_library is None and args.sv_pairs_k is None and args.sv_clip_min is None
    args = call.parser().parse_args(["--workdir", "w", "--network", "n", "--sv", "--sv_pairs", "--sv_pairs_library", "200,40,360"])
    assert args.sv and args.sv_pairs and sv.library_option(args.sv_pairs_library, "sv_pairs_library") == (200, 40, 360)
    own = sv.parser().parse_args(["--bam", "b", "--ref", "r", "--output_prefix", "p", "--pairs", "--pairs_k", "5", "--clip_min", "9"])
    assert own.pairs and own.pairs_k == 5 and own.clip_min == 9 and own.pairs_library is None
    with pytest.raises(SystemExit, match="--pairs_k is an option of the read pairs .* add --pairs, or drop --pairs_k"):
        sv.main(["--bam", "b", "--ref", "r", "--output_prefix", "p", "--pairs_k", "5"])


def test_pass_1_of_haplotag_runs_without_sv_pairs(monkeypatch):
    seen = []
    monkeypatch.setattr(call, "main", lambda ns: seen.append(ns) or os.path.join(ns.workdir, "results.output.vcf"))
    args = call.parser().parse_args(["--workdir", "w", "--network", "n", "--from_bam", "--pbam", "p.bam", "--include_hp", "--haplotag", "--sv",
                                     "--sv_pairs", "--sv_pairs_k", "6"])
    call.haplotag_passes(args)
    first, second = seen
    assert first.sv is False and first.sv_pairs is False and first.sv_pairs_k is None and second.sv_pairs is True and second.sv_pairs_k == 6
    call.check_sv(first)


def test_sampling_a_library_by_the_restatement(tmp_path):
    from tests.mate_writer import write_bam
    rng = np.random.default_rng(9)
    rows = []
    for k in range(120):
        s = 20 + 20 * k
        rows += pc.fr_pair(2 * k, s, s + 10 + int(rng.integers(5, 16)), extra=pc.PROPER)
    rows = sorted(rows, key=lambda r: r[2])
    path = str(tmp_path / "library.bam")
    write_bam(path, [("chr1", pc.LENGTH)], _mated_reads(rows, pc.REFERENCE))
    inner = np.bincount([r[10] - (r[2] + 10) + 1024 for r in rows if r[1] & pc.FIRST], minlength=4096)
    assert sv.sampled_library(path, {"chr1": pc.REFERENCE}, restatement=True) == sv.library_of(inner, 8)
    assert sv.sampled_library(path, {"chr1": pc.REFERENCE}, restatement=True, k=3, max_span=700) == sv.library_of(inner, 3)
    few = str(tmp_path / "few.bam")
    write_bam(few, [("chr1", pc.LENGTH)], _mated_reads(rows[:40], pc.REFERENCE))
    with pytest.raises(sv.LibraryError, match="too few for a library .* --sv_pairs_library"):
        sv.sampled_library(few, {"chr1": pc.REFERENCE}, restatement=True)


def test_an_unpaired_bam_goes_through_the_pairs_path_and_yields_no_pair_row(tmp_path):
    from tests.bam_writer import Read, write_bam
    rows = [r for r in pc.HAND_TABLE[0].rows if not r[1] & pc.PAIRED] + pc.CLIP_CASE.rows[:5]          # the three 40D reads, five clipped
    rows = sorted(rows, key=lambda r: r[2])
    path = str(tmp_path / "unpaired.bam")
    write_bam(path, [("chr1", pc.LENGTH)], [Read("r%d" % k, r[2], r[3], r[4], r[5], flag=r[1], mapq=r[6]) for k, r in enumerate(rows)])
    genome = {"chr1": pc.REFERENCE}
    assert sv.sampled_library(path, genome, restatement=True) == sv.UNSET_LIBRARY
    kw = dict(min_size=5, flank=3, cluster_gap=10, len_ratio_percent=70, min_support=3, restatement=True)
    found = sv.measure(path, genome, pairs=True, clip_min=4, **kw)
    assert found.library == sv.UNSET_LIBRARY and found.library_source == "unset: the BAM has no paired reads"
    total = found.total()
    assert total["pair_reads"] == 0 and total["pair_signatures"] == 0 and total["clipped_reads"] == 3 and total["candidates"] == 1
    split = sv.measure(path, genome, split=True, **kw)
    for name in sv.SIGNATURE_COLUMNS:
        assert np.array_equal(found.tables["chr1"]["SIGNATURES_" + name], split.tables["chr1"]["SIGNATURES_" + name])
    for name in split.candidate_columns:
        assert np.array_equal(found.tables["chr1"]["CANDIDATES_" + name], split.tables["chr1"]["CANDIDATES_" + name])
    (event,) = found.candidates("chr1")
    assert (event["PR"], event["CE"], event["IMPRECISE"], event["DV"]) == (0, 0, 0, 3)


# ---- csrc/sv_pairs.h under the sanitizers, against the restatement ----------------------------------------------------------------------
def _block(lines, want, reference, rows, library, p, plain_rows):
    """One block of the program's input, and what the restatement says it prints."""
    length = len(reference)
    lines.append("P %d %d %d %d %d %d %d %d %d %d %d %d %d" % (length, pc.OWN, len(pc.CONTIGS), p["min_size"], p["flank"], p["mapq_threshold"],
                                                             p["cluster_gap"], p["len_ratio_percent"], p["min_support"], p["clip_min"], *library))
    reads, splits, mates = pc.pair_set(rows)
    part = sv.pair_rows_of(reads, splits, mates, 0, pc.OWN, len(pc.CONTIGS), length,
                           p["min_size"], p["mapq_threshold"], library, p["clip_min"])
    made = {g[4]: g for g in part["rows"]}
    ordinal, inner = 0, np.zeros(4096, np.int64)
    for k, r in enumerate(rows):
        e = int(reads.ref_ends[k])
        cigar = "".join("%d%s" % (n, "MIDNSHP=X"[op]) for op, n in r[3])
        lines.append("R %d %d %d %d %d %d %d %s" % (r[2], r[1], r[6], r[7], r[9], r[10], 1 if r[8] else 0, cigar))
        status, at = int(part["status"][k]), -1
        if status not in (sv.NOT_PAIR, sv.BAD_MATE):
            at = sv.pair_outcome(r[1], r[2], e, pc.OWN, r[9], r[10], len(pc.CONTIGS), library, p["min_size"])[1]
            at = -1 if at is None else at
        clips = sv.clips_of(r[3], p["clip_min"]) if sv.counted(r[1], r[6], p["mapq_threshold"]) and e <= length and not r[8] else 0
        want.append("S %d %d %d" % (status, at, clips))
        if sv.pair_counted(r[1], r[6], p["mapq_threshold"]):
            if ordinal in made:
                want.append("G " + " ".join(str(v) for v in made[ordinal]))
            ordinal += 1
        if at >= 0:
            inner[at] += 1
    lines += ["X " + " ".join(str(v) for v in g) for g in plain_rows]
    lines.append("E")
    want.append("H %d %d %d" % sv.library_of(inner, 8) if inner.any() else "H none")
    found, n_assigned = sv.clustered_with_pairs(list(part["rows"]) + list(plain_rows), library, p["flank"], p["cluster_gap"],
                                                p["len_ratio_percent"], p["min_support"])
    want += ["K " + " ".join(str(v) for v in c) for c in found]
    want.append("E %d" % n_assigned)


def test_pair_rules_are_clean_under_sanitizers_and_equal_the_restatement(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler on this box"
    exe = str(tmp_path / "sv_pairs_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                            os.path.join(ROOT, "tests", "abi", "sv_pairs_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    lines, want = [], []
    for case in pc.HAND_TABLE:
        _block(lines, want, case.reference, case.rows, pc.LIBRARY, case.kw(), [g for g in case.signatures if g[5] != sv.PAIR_OP])
    for name, rows in pc.STRESS_SETS.items():
        _block(lines, want, pc.STRESS_REFERENCE, sorted(rows, key=lambda r: r[2]), pc.STRESS_LIBRARY, pc.STRESS, [])
    for seed in pc.FUZZ_SEEDS:
        reference, rows, tables, _ = fuzz_restated(seed)
        plain = [g for g in rows_of(tables, "SIGNATURES_", sv.SIGNATURE_COLUMNS) if g[5] != sv.PAIR_OP]
        _block(lines, want, reference, rows, pc.FUZZ_LIBRARY, pc.FUZZ, plain)
        _block(lines, want, reference, rows, sv.UNSET_LIBRARY, pc.FUZZ, [])
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "sv_pairs_check: ok" in run.stdout, (run.returncode, run.stdout[-500:], run.stderr[-3000:])
    got = run.stdout.splitlines()[:-1]
    assert len(got) == len(want) and len([x for x in got if x.startswith("G")]) > 2000
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a, b)
