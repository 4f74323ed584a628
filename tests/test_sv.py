"""The large deletions and insertions on the CPU: the restatement of hello_amd/sv.py against the cases
worked by hand (tests/sv_cases.py), the library's host rules -- clusters and genotype, which need no device -- against it, the VCF
text of one hand case byte for byte, the situations of the edge stress in the restatement's own output, the refusals of ``check_sv``
and of the entry points before they look for a device, and csrc/sv.h with ``sv_walk`` as a stand-alone program under AddressSanitizer
and UBSan (tests/abi/sv_check.cpp)."""
import argparse
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

from hello_amd import call, sv
from tests import read_fuzz as rf, sv_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_stress: dict = {}


def spans_of(rows, length: int, cuts=()):
    """[(reads, lo, hi)]: the chromosome whole, or cut at ``cuts``, each span with the rows a fetch of it returns."""
    edges = [0] + list(cuts) + [length]
    return [(sc.read_set(sc.overlapping(rows, lo, hi)), lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]


def rows_of(tables, prefix: str, names):
    return [tuple(int(tables[prefix + name][i]) for name in names) for i in range(tables[prefix + names[0]].shape[0])]


def same_tables(got, want):
    """Every SIGNATURES and CANDIDATES column, integer for integer."""
    for prefix, names in (("SIGNATURES_", sv.SIGNATURE_COLUMNS), ("CANDIDATES_", sv.CANDIDATE_COLUMNS)):
        for name in names:
            assert got[prefix + name].dtype == np.int64 and np.array_equal(got[prefix + name], want[prefix + name]), prefix + name


def stress_restated():
    """The edge stress and its restatement, made once: (reference, rows, named, tables, counts)."""
    if not _stress:
        reference, rows, named = sc.stress()
        tables, counts = sv.restated(spans_of(rows, sc.LENGTH), reference, **sc.STRESS)
        _stress.update(value=(reference, rows, named, tables, counts))
    return _stress["value"]


# ---- the restatement against the hand tables ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.HAND_TABLE, ids=[c.name for c in sc.HAND_TABLE])
def test_restatement_equals_the_hand_table(case):
    length = len(case.reference)
    for cuts in ((), (case.cut(),)):
        tables, counts = sv.restated(spans_of(case.rows, length, cuts), case.reference, **sc.HAND)
        assert rows_of(tables, "SIGNATURES_", sv.SIGNATURE_COLUMNS) == case.signatures
        assert rows_of(tables, "CANDIDATES_", sv.CANDIDATE_COLUMNS) == case.candidates
        assert {k: counts[k] for k in sv.METRIC_STATS} == case.want_counts()
    whole = sv.signatures_of(sc.read_set(case.rows), case.reference, 0, length, sc.HAND["min_size"], sc.HAND["flank"])
    assert whole["status"].tolist() == case.status


def test_a_read_belongs_to_the_span_that_holds_its_start_and_keeps_its_ordinal():
    case = next(c for c in sc.HAND_TABLE if c.name.startswith("three reads"))
    second = sc.read_set(case.rows[1:])                                     # as if the first read lay in an earlier span
    part = sv.signatures_of(second, case.reference, 2, 25, sc.HAND["min_size"], sc.HAND["flank"], counting_given=7)
    assert [g[4] for g in part["signatures"]] == [7, 8] and part["counts"]["counting"] == 4
    early = sv.signatures_of(second, case.reference, 3, 25, sc.HAND["min_size"], sc.HAND["flank"])
    assert early["signatures"] == [] and early["counts"]["belonging"] == 0 and early["cover"] == []


# ---- clusters and genotype: the library's host rules against the restatement ----------------------------------------------------
@pytest.mark.parametrize("name,signatures,want", sc.CLUSTER_TABLE, ids=[c[0][:40] for c in sc.CLUSTER_TABLE])
def test_clusters_worked_by_hand_restated_and_native(name, signatures, want):
    assert sv.clustered(signatures, 10, 70, 2) == want
    assert sv.clustered_native(signatures, 10, 70, 2) == want
    assert sv.clustered_native(signatures[::-1], 10, 70, 2) == want         # the order given does not matter


def test_clusters_native_equal_restated_on_the_stress_and_on_random_signatures():
    _, _, _, tables, _ = stress_restated()
    stress = rows_of(tables, "SIGNATURES_", sv.SIGNATURE_COLUMNS)
    assert len(stress) > 40
    rng = np.random.default_rng(11)
    sets = [stress]
    for n in (0, 1, 2, 50, 400):
        sets.append([(int(rng.integers(2)), int(rng.integers(0, 3000)), int(rng.integers(10, 200)), int(rng.integers(0, 9)),
                      int(rng.integers(0, max(1, n // 3))), int(rng.integers(0, 5)), k % 2, k % 4) for k in range(n)])
        # a read has one strand and one haplotype: make them functions of the ordinal
        sets[-1] = list({(g[4], g[5], g[0]): g[:6] + (g[4] % 2, g[4] % 4) for g in sets[-1]}.values())
    for signatures in sets:
        for gap, percent, support in ((20, 70, 2), (0, 100, 1), (100, 70, 3), (5, 1, 2), (1000, 50, 1)):
            assert sv.clustered_native(signatures, gap, percent, support) == sv.clustered(signatures, gap, percent, support)


def test_genotype_native_equals_restated():
    counts = [(dv, dr) for dv in list(range(0, 40)) + [100, 999, 12345] for dr in list(range(0, 40)) + [100, 999, 54321]]
    native = sv.genotyped_native([c[0] for c in counts], [c[1] for c in counts])
    for (dv, dr), got in zip(counts, native.tolist()):
        want = sv.genotype_of(dv, dr)
        assert got[0] == want[0], (dv, dr)                                 # GT
        assert all(abs(a - b) <= 1 for a, b in zip(got[1:], want[1:])), (dv, dr, got, want)      # GQ and PL: the last rounding
        assert min(got[2:]) == 0 and got[2 + got[0]] == 0 and 0 <= got[1] <= 99
    assert sv.genotype_of(3, 2) == (1, 12, 24, 0, 12) and sv.genotype_of(2, 0) == (2, 6, 26, 6, 0) and sv.genotype_of(0, 0) == (0, 0, 0, 0, 0)


# ---- the files ------------------------------------------------------------------------------------------------------------------
def test_vcf_text_of_a_hand_case_byte_for_byte(tmp_path):
    case = next(c for c in sc.HAND_TABLE if c.name.startswith("three reads"))
    tables, counts = sv.restated(spans_of(case.rows, 25), case.reference, **sc.HAND)
    found = sv.Events()
    found.set("chr1", np.frombuffer(case.reference.encode(), np.uint8), tables, counts)
    assert found.vcf_text() == sc.GENOTYPED_VCF
    first = found.write_all(str(tmp_path / "a"))
    again = found.write_all(str(tmp_path / "b"))
    assert [os.path.basename(p) for p in first] == ["a.vcf", "a.npz"] and open(first[0]).read() == sc.GENOTYPED_VCF
    assert open(first[1], "rb").read() == open(again[1], "rb").read()
    with np.load(first[1]) as z:
        assert z["chromosomes"].tolist() == ["chr1"] and z["CANDIDATES_POS_0"].tolist() == [10] and z["SIGNATURES_ORDINAL_0"].tolist() == [0, 1, 2]
        assert z["STATS_0"].tolist() == [5, 5, 3, 3, 3, 1]
    # an event at position 0 has no base before it
    line = sv.vcf_line("c", np.frombuffer(b"ACGT", np.uint8), dict(dict.fromkeys(sv.CANDIDATE_COLUMNS, 0), TYPE=sv.INS, LEN=7, DV=2, GT=2))
    assert line.startswith("c\t0\t.\tN\t<INS>\t.\tPASS\tSVTYPE=INS;SVLEN=7;END=0;SUPPORT=2;")


# ---- the edge stress: each situation really occurs --------------------------------------------------------------------------------
def assert_situations(reference, rows, named, tables, counts):
    p = sc.STRESS
    flank, gap = p["flank"], p["cluster_gap"]
    reads = sc.read_set(rows)
    whole = sv.signatures_of(reads, reference, 0, sc.LENGTH, p["min_size"], p["flank"], p["mapq_threshold"])
    status = {r[0]: int(s) for r, s in zip(rows, whole["status"])}
    ordinal, k = {}, 0
    for r, s in zip(rows, whole["status"]):
        if s:
            ordinal[r[0]] = k
            k += 1
    by_name = {r[0]: r for r in rows}
    sigs = rows_of(tables, "SIGNATURES_", sv.SIGNATURE_COLUMNS)
    cands = rows_of(tables, "CANDIDATES_", sv.CANDIDATE_COLUMNS)
    of = lambda situation: [g for g in sigs if g[4] in [ordinal[n] for n in named[situation] if n in ordinal]]      # noqa: E731
    at = lambda kind, pos: [c for c in cands if c[0] == kind and c[1] == pos]                                      # noqa: E731
    # a read of more than 128 operations with signatures at 63, 64, 127 and 128
    assert len(by_name[named["long"][0]][3]) == 130 and sorted(g[5] for g in of("long")) == [63, 64, 127, 128]
    assert {g[5]: (g[0], g[2]) for g in of("long")} == {63: (sv.DEL, 12), 64: (sv.INS, 11), 127: (sv.INS, 10), 128: (sv.DEL, 13)}
    # straight after H and S; the outermost operations and the missed flanks are walked and give nothing
    assert [(g[5], g[0]) for g in of("after_clips")] == [(3, sv.DEL)] and by_name[named["after_clips"][0]][3][:2] == [(sc.H, 2), (sc.S, 3)]
    assert len(named["outermost"]) == 5 and all(status[n] == 2 for n in named["outermost"]) and of("outermost") == []
    assert len(of("flank_met")) == 2 and {g[0] for g in of("flank_met")} == {sv.DEL, sv.INS}
    assert [status[n] for n in named["flank_missed"]] == [2, 2] and [status[n] for n in named["flank_met"]] == [3, 3]
    # the shifts
    for shift in sc.SHIFTS:
        assert [(g[3], g[1]) for g in of("shift%d" % shift)] == [(shift, sc.SHIFT_AT[shift] - shift)]
    stopped = by_name[named["stopped"][0]]
    assert [(g[3], g[1]) for g in of("stopped")] == [(40, stopped[2])] * 2              # it stops on the reads' first base
    wrap = of("wrap")
    assert [(g[0], g[2], g[3]) for g in wrap] == [(sv.INS, 10, 25)] and wrap[0][3] > wrap[0][2]
    assert any(b.islower() for b in reference[wrap[0][1]:sc.WRAP_AT]) and any(b.islower() for b in by_name[named["wrap"][0]][4])
    n_repeat = of("n_in_repeat")
    assert [g[3] for g in n_repeat] == [30] and {"N", "n"} <= set(reference[n_repeat[0][1]:sc.N_AT + 12])
    # the chromosome's end
    assert [(g[1] + g[3] + g[2]) for g in of("ends_at_length")] == [sc.LENGTH] and of("ends_past_length") == []
    assert status[named["ends_past_length"][0]] == 2
    end_read = by_name[named["ends_at_length"][0]]
    assert end_read[2] + 36 - flank >= sc.LENGTH                                       # the clamp of the cover
    assert tables["DIFF"][sc.LENGTH] < 0 and tables["DIFF"].sum() == 0 and np.cumsum(tables["DIFF"]).min() == 0
    # a read overlaps two spans and has a signature; a short read leaves the cover alone
    starts = {n: by_name[n][2] for n in ordinal}
    ends = {n: by_name[n][2] + sum(k for op, k in by_name[n][3] if op in (sc.M, sc.D, sc.N)) for n in ordinal}
    assert any(status[n] == 3 and starts[n] < cut < ends[n] for n in ordinal for cut in range(sc.SPAN, sc.LENGTH, sc.SPAN))
    short, two = by_name[named["short"][0]], by_name[named["two_flanks"][0]]
    assert ends[short[0]] - short[2] == 2 * flank - 1 and ends[two[0]] - two[2] == 2 * flank
    assert (two[2] + flank, 1) in whole["cover"] and (two[2] + flank + 1, -1) in whole["cover"]
    assert len(whole["cover"]) == 2 * sum(ends[n] - starts[n] >= 2 * flank for n in ordinal) and (short[2] + flank, 1) not in whole["cover"]
    # candidates on both sides of a tile's edge and on the last position, with the cover's own edges on them
    for pos, kind in zip(sc.TILE_EDGE, (sv.DEL, sv.INS, sv.DEL)):
        assert len(at(kind, pos)) == 1 and at(kind, pos)[0][3] == 2
    assert len(at(sv.INS, sc.LENGTH - 1)) == 1 and at(sv.INS, sc.LENGTH - 1)[0][13] >= 2
    begins, stops = {starts[n] + flank for n in ordinal}, {ends[n] - flank for n in ordinal}
    assert {1023, 1024} <= begins and {1024, 1025} <= stops
    for c in cands:                                                                    # spanning, counted read by read
        assert c[13] == sum(starts[n] + flank <= c[1] <= min(ends[n] - flank, sc.LENGTH - 1) for n in ordinal if ends[n] - starts[n] >= 2 * flank)
    # the gap and the ratio at their thresholds; a read twice; the support at its threshold; both types at one place
    assert [c[3] for c in at(sv.DEL, sc.GAP_AT)] == [4] and at(sv.DEL, sc.GAP_AT)[0][9:11] == (sc.GAP_AT, sc.GAP_AT + gap)
    assert [c[3] for c in at(sv.DEL, sc.GAP_MORE_AT)] == [2] and [c[3] for c in at(sv.DEL, sc.GAP_MORE_AT + gap + 1)] == [2]
    assert [(c[2], c[3], c[11], c[12]) for c in at(sv.DEL, sc.RATIO_AT)] == [(14, 4, 14, 20)]
    assert [(c[2], c[3]) for c in at(sv.DEL, sc.RATIO_UNDER_AT)] == [(20, 2), (29, 2)]
    twice = at(sv.DEL, sc.TWICE_AT)
    assert [c[3] for c in twice] == [2] and len(of("twice")) == 3 and twice[0][10] == sc.TWICE_AT + 20
    assert min(c[3] for c in cands) == p["min_support"] and len(of("flank_met")) == 2 and not at(sv.DEL, sc.FLANK_AT + 5)
    assert [c[0] for c in cands if c[1] == sc.BOTH_AT] == [sv.DEL, sv.INS]
    assert of("not_counting") == [] and all(n not in ordinal for n in named["not_counting"])
    assert {c[15] for c in cands} >= {1, 2} and {g[6] for g in sigs} == {0, 1} and {g[7] for g in sigs} == {0, 1, 2}
    # the clamp of DR: the two reads whose start stopped the move support a position their own cover does not reach
    assert [(c[3], c[13], c[14], c[15]) for c in at(sv.DEL, stopped[2])] == [(2, 0, 0, 2)]


def test_edge_stress_each_situation_occurs_in_the_restatement():
    reference, rows, named, tables, counts = stress_restated()
    assert_situations(reference, rows, named, tables, counts)
    cut, cut_counts = sv.restated(spans_of(rows, sc.LENGTH, range(sc.SPAN, sc.LENGTH, sc.SPAN)), reference, **sc.STRESS)
    same_tables(cut, tables)
    assert np.array_equal(cut["DIFF"], tables["DIFF"])
    assert {k: cut_counts[k] for k in sv.METRIC_STATS} == {k: counts[k] for k in sv.METRIC_STATS}


# ---- the fuzz corpus of tests/read_fuzz.py ---------------------------------------------------------------------------------------
FUZZ = dict(min_size=3, flank=1, mapq_threshold=rf.MAPQ_THRESHOLD, cluster_gap=20, len_ratio_percent=70, min_support=2)


def _fold(a):
    return np.asarray(a, np.uint8) & 0xDF


def independent(reference, rows):
    """(signatures sorted, spanning per position) from the alignment table of tests/read_fuzz.py: an event is a run of inserted or
    deleted lines of one operation, its shift the common suffix of two strings; spanning is counted position by position.  No cursor
    walks a CIGAR."""
    o = rf.Oracle(reference, rows)
    t, L, flank = o.t, rf.LENGTH, FUZZ["flank"]
    ref = np.frombuffer(reference.encode(), np.uint8)
    counting = np.flatnonzero(o.counted)
    ordinal = {int(r): k for k, r in enumerate(counting)}
    spanning = np.zeros(L + 1, np.int64)
    for r in counting:
        s, e = int(o.pos[r]), int(o.ref_end[r])
        if e - s >= 2 * flank:
            inside = np.arange(s + flank, min(e - flank, L - 1) + 1)
            spanning[inside] += 1
    sigs = []
    event = np.isin(t.op, (rf.I, rf.D)) & o.counted[t.read]
    key = t.read[event] * (1 << 20) + t.opi[event]
    for k in np.unique(key):
        lines = np.flatnonzero(event)[key == k]
        r, opi, n, op = int(t.read[lines[0]]), int(t.opi[lines[0]]), int(lines.shape[0]), int(t.op[lines[0]])
        if n < FUZZ["min_size"]:
            continue
        mine = t.read == r
        before = mine & (np.arange(t.read.shape[0]) < lines[0])
        s, e = int(o.pos[r]), int(o.ref_end[r])
        p = s + int((before & (t.p >= 0)).sum())
        pe = p + n if op == rf.D else p
        if not (p - s >= flank and e - pe >= flank and pe <= L):
            continue
        if op == rf.D:
            other = ref[s + n:p + n]
        else:
            inserted = np.frombuffer(rows[r][4].encode(), np.uint8)[t.q[lines]]
            other = np.concatenate([ref[:p], inserted])[s + n:p + n]
        match = (_fold(ref[s:p]) == _fold(other))[::-1]
        shift = int(match.shape[0] if match.all() else np.argmin(match))
        sigs.append((sv.DEL if op == rf.D else sv.INS, p - shift, n, shift, ordinal[r], opi, int(bool(rows[r][1] & rf.REV)), 0))
    return sorted(sigs, key=lambda g: (g[0], g[1], g[2], g[4], g[5])), spanning


def with_hp(rows):
    return [tuple(r) + (0,) for r in rows]


def test_fuzz_corpus_has_what_it_is_run_for():
    """The restatement equals the derivation from the alignment table, and over the seeds there are signatures of both types, moved ones, candidates, and reads that run past the chromosome's end."""
    seen = dict(signatures=0, ins=0, moved=0, candidates=0, past_end=0)
    for seed in list(rf.SEEDS)[:8]:
        for profile in rf.PROFILES:
            reference, rows, _ = rf.corpus(seed, profile)
            want, counts = sv.restated(spans_of(with_hp(rows), rf.LENGTH), reference, **FUZZ)
            signatures, spanning = independent(reference, rows)
            assert rows_of(want, "SIGNATURES_", sv.SIGNATURE_COLUMNS) == signatures and np.array_equal(np.cumsum(want["DIFF"]), spanning)
            seen["signatures"] += counts["signatures"]
            seen["ins"] += int((want["SIGNATURES_TYPE"] == sv.INS).sum())
            seen["moved"] += int((want["SIGNATURES_SHIFT"] > 0).sum())
            seen["candidates"] += counts["candidates"]
            seen["past_end"] += sum(r[2] + sum(k for op, k in r[3] if op in (rf.M, rf.D, rf.N, rf.EQ, rf.X)) > rf.LENGTH for r in rows)
    assert seen["signatures"] > 100 and 0 < seen["ins"] < seen["signatures"] and seen["moved"] > 10 and seen["past_end"] > 0, seen


# ---- the refusals that need no device ---------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_they_look_for_a_device():
    case = next(c for c in sc.HAND_TABLE if c.name.startswith("three reads"))
    reads = sc.read_set(case.rows)
    decreasing = reads.read_offsets.copy()
    decreasing[3] -= 18
    for kw, said in ((dict(min_size=0), "min_size 0: at least 1"), (dict(flank=0), "flank 0: at least 1")):
        with pytest.raises(RuntimeError, match=said):
            sv.Caller(case.reference, **kw)
    with sv.Caller(case.reference, 5, 3) as caller:
        with pytest.raises(RuntimeError, match="offsets decrease"):
            caller.add(dataclasses.replace(reads, read_offsets=decreasing), 0, 25)
        with pytest.raises(RuntimeError, match="CIGAR query length 17, 16 bases"):
            caller.add(dataclasses.replace(reads, cigars=reads.cigars + np.array([16] + [0] * 10, np.uint32)), 0, 25)
        with pytest.raises(RuntimeError, match="ref_end does not match"):
            caller.add(dataclasses.replace(reads, ref_ends=reads.ref_ends + 1), 0, 25)
        with pytest.raises(RuntimeError, match=r"span \[0, 26\) of a reference of 25 bases"):
            caller.add(reads, 0, 26)
        for gap, percent, support, said in ((-1, 70, 2, "cluster_gap -1"), (10, 0, 2, "len_ratio_percent 0"), (10, 101, 2, "len_ratio_percent 101"),
                                            (10, 70, 0, "min_support 0")):
            with pytest.raises(RuntimeError, match=said):
                caller.finish(gap, percent, support)
        with pytest.raises(RuntimeError, match="before hello_sv_finish"):
            caller._array(9, np.int64)
        assert all(v == 0 for v in caller.stats().values()) and caller.arrays()["SIGNATURES_POS"].shape == (0,)
        caller.finish()                                                    # nothing was added: no device is needed
        assert caller.arrays()["CANDIDATES_POS"].shape == (0,) and caller.stats()["candidates"] == 0
        with pytest.raises(RuntimeError, match="hello_sv_finish twice"):
            caller.finish()
        with pytest.raises(RuntimeError, match="hello_sv_add after hello_sv_finish"):
            caller.add(reads, 0, 25)
    with pytest.raises(RuntimeError, match="count -1"):
        sv.genotyped_native([1, -1], [0, 0])
    with pytest.raises(RuntimeError, match="signature 0: type 2"):
        sv.clustered_native([(2, 5, 9, 0, 0, 1, 0, 0)])
    with pytest.raises(RuntimeError, match="min_support 0"):
        sv.clustered_native([], min_support=0)


def _args(**kw):
    base = dict(sv=False, shards=None, from_bam=False, from_bams=False, gpus=1, ibam=None, pbam=None)
    base.update(dict.fromkeys(call.SV_OPTIONS))
    base.update(kw)
    return argparse.Namespace(**base)


def test_check_sv_names_the_fix(monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    call.check_sv(_args())
    call.check_sv(_args(sv=True, from_bam=True, ibam="i.bam"))
    call.check_sv(_args(sv=True, from_bams=True, sv_min_size=30, sv_len_ratio=1.0, sv_cluster_gap=0))
    with pytest.raises(SystemExit, match="drop --shards and start from the BAM"):
        call.check_sv(_args(sv=True, shards="s/*.npz", from_bam=True))
    with pytest.raises(SystemExit, match="no BAM on its path: add --from_bam"):
        call.check_sv(_args(sv=True))
    with pytest.raises(SystemExit, match="run it with --gpus 1 as a plain command"):
        call.check_sv(_args(sv=True, from_bam=True, gpus=2))
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process on one GPU"):
        call.check_sv(_args(sv=True, from_bam=True))
    monkeypatch.delenv("RANK")
    monkeypatch.delenv("WORLD_SIZE")
    for flag, value in zip(call.SV_OPTIONS, (50, 3, 20, 100, 0.7)):
        with pytest.raises(SystemExit, match=f"--{flag} is an option of the pass .* add --sv, or drop --{flag}"):
            call.check_sv(_args(**{flag: value}))
    for kw, said in ((dict(sv_min_size=0), "--sv_min_size"), (dict(sv_min_support=0), "--sv_min_support"), (dict(sv_flank=0), "--sv_flank"),
                     (dict(sv_cluster_gap=-1), "--sv_cluster_gap"), (dict(sv_len_ratio=1.5), "--sv_len_ratio"),
                     (dict(sv_len_ratio=0.0), "--sv_len_ratio")):
        with pytest.raises(SystemExit, match=said + " is "):
            call.check_sv(_args(sv=True, from_bam=True, **kw))


def test_the_command_lines_know_the_options():
    args = call.parser().parse_args(["--workdir", "w", "--network", "n"])
    assert args.sv is False and all(getattr(args, flag) is None for flag in call.SV_OPTIONS)
    args = call.parser().parse_args(["--workdir", "w", "--network", "n", "--sv", "--sv_min_size", "30", "--sv_len_ratio", "0.5"])
    assert args.sv and call._sv_values(args) == (30, sv.MIN_SUPPORT, sv.FLANK, sv.CLUSTER_GAP, 0.5)
    own = sv.parser().parse_args(["--bam", "b", "--ref", "r", "--output_prefix", "p"])
    assert (own.sv_min_size, own.sv_min_support, own.sv_flank, own.sv_cluster_gap, own.sv_len_ratio) == (50, 3, 20, 100, 0.7)
    assert sv.percent_of(0.7) == 70 and sv.percent_of(0.29) == 29 and sv.percent_of(1) == 100


def test_pass_1_of_haplotag_runs_without_sv(monkeypatch):
    seen = []
    monkeypatch.setattr(call, "main", lambda ns: seen.append(ns) or os.path.join(ns.workdir, "results.output.vcf"))
    args = call.parser().parse_args(["--workdir", "w", "--network", "n", "--from_bam", "--pbam", "p.bam", "--include_hp", "--haplotag", "--sv",
                                     "--sv_min_size", "30"])
    call.haplotag_passes(args)
    first, second = seen
    assert first.sv is False and all(getattr(first, flag) is None for flag in call.SV_OPTIONS) and first.phase is True
    assert second.sv is True and second.sv_min_size == 30 and second.haplotag_vcf.endswith("results.output.phased.vcf")
    call.check_sv(first)


# ---- csrc/sv.h and sv_walk under the sanitizers -------------------------------------------------------------------------------------
def test_host_rules_are_clean_under_sanitizers(tmp_path):
    """sv.h and cigar.h need no HIP: the host compiler alone builds them, without a ROCm include path."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler on this box"
    exe = str(tmp_path / "sv_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                            os.path.join(ROOT, "tests", "abi", "sv_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "sv_check: ok" in run.stdout, (run.returncode, run.stdout, run.stderr[-3000:])
