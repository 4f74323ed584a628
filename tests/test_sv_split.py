"""The split alignments on the CPU: the restatement of hello_amd/sv.py against the cases worked by hand
(tests/sv_split_cases.py), whole and cut into spans; the library's clustering with its SR column against the restatement, and the
clustering of 7p unchanged; ``fetch_with_sa`` through BAMs written by tests/bam_writer.py; the VCF text byte for byte; the refusals
that need no device; ``--sv_split`` on the command lines; and csrc/sv_split.h as a stand-alone program under AddressSanitizer and
UBSan (tests/abi/sv_split_check.cpp) over the hand cases, the stress and the fuzz, against the restatement."""
import argparse
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

from hello_amd import call, sv
from hello_amd.bam import BamFile, Splits
from tests import sv_cases as sc, sv_split_cases as ss
from tests.test_sv import rows_of, same_tables, spans_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(contigs=ss.CONTIGS, own=ss.OWN)
_made: dict = {}


def clusters_of(tables):
    names = ("TYPE", "POS", "LEN", "DV", "SR", "DP", "DR")
    return [tuple(int(tables["CANDIDATES_" + n][i]) for n in names) for i in range(tables["CANDIDATES_POS"].shape[0])]


def stress_restated():
    """(reference, rows, named, tables, counts) of the stress, made once."""
    if "stress" not in _made:
        reference, rows, named = ss.stress()
        tables, counts = sv.restated(ss.spans_of(rows, ss.LENGTH), reference, **ss.STRESS, **KW)
        _made["stress"] = (reference, rows, named, tables, counts)
    return _made["stress"]


def fuzz_restated(seed: int):
    if ("fuzz", seed) not in _made:
        reference, rows = ss.fuzz(seed)
        _made["fuzz", seed] = (reference, rows) + sv.restated(ss.spans_of(rows, ss.FUZZ_LENGTH), reference, **ss.FUZZ, **KW)
    return _made["fuzz", seed]


def same_split_tables(got, want):
    same_tables(got, want)
    assert got["CANDIDATES_SR"].dtype == np.int64 and np.array_equal(got["CANDIDATES_SR"], want["CANDIDATES_SR"])


# ---- the restatement against the hand cases -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ss.HAND_TABLE, ids=[c.name for c in ss.HAND_TABLE])
def test_restatement_equals_the_hand_cases_whole_and_cut(case):
    length = len(case.reference)
    for cuts in ((), (case.cut(),)):
        tables, counts = sv.restated(ss.spans_of(case.rows, length, cuts), case.reference, **ss.HAND, **KW)
        assert rows_of(tables, "SIGNATURES_", sv.SIGNATURE_COLUMNS) == case.signatures
        assert clusters_of(tables) == case.clusters
        assert {k: counts[k] for k in sv.SPLIT_COUNT_NAMES} == case.want_counts()
        for c in clusters_of(tables):                                      # the genotype is 7p's of (DV, DR)
            row = [r for r in rows_of(tables, "CANDIDATES_", sv.CANDIDATE_COLUMNS) if r[:3] == c[:3]][0]
            assert row[15:] == sv.genotype_of(c[3], c[6])
    reads, splits = ss.split_set(case.rows)
    whole = sv.signatures_of(reads, case.reference, 0, length, ss.HAND["min_size"], ss.HAND["flank"], splits=splits, **KW)
    assert whole["split_status"].tolist() == case.split_status


def test_without_splits_the_restatement_is_what_it_was():
    reference, rows, _, tables, _ = stress_restated()
    plain, counts = sv.restated(spans_of([r[:8] for r in rows], ss.LENGTH), reference, **ss.STRESS)
    assert not plain["CANDIDATES_SR"].any() and not plain["SPLIT_STATUS"].any() and all(counts[k] == 0 for k in sv.SPLIT_COUNT_NAMES)
    assert (plain["SIGNATURES_OP"] >= 0).all() and set(plain["SIGNATURES_TYPE"].tolist()) == {sv.DEL, sv.INS}
    own = tables["SIGNATURES_OP"] >= 0                                       # the tags change no row of a CIGAR operation
    for name in sv.SIGNATURE_COLUMNS:
        assert np.array_equal(tables["SIGNATURES_" + name][own], plain["SIGNATURES_" + name])
    with pytest.raises(ValueError, match="contig names"):
        sv.restated(ss.spans_of(rows, ss.LENGTH), reference, **ss.STRESS)


def test_stress_each_situation_occurs_in_the_restatement():
    reference, rows, named, tables, counts = stress_restated()
    reads, splits = ss.split_set(rows)
    p = ss.STRESS
    whole = sv.signatures_of(reads, reference, 0, ss.LENGTH, p["min_size"], p["flank"], p["mapq_threshold"], splits=splits, **KW)
    status = {r[0]: int(s) for r, s in zip(rows, whole["split_status"])}
    ordinal, k = {}, 0
    for r, s in zip(rows, whole["status"]):
        if s:
            ordinal[r[0]] = k
            k += 1
    sigs = rows_of(tables, "SIGNATURES_", sv.SIGNATURE_COLUMNS)
    of = lambda what: [g for g in sigs if g[5] < 0 and g[4] in [ordinal[n] for n in named[what] if n in ordinal]]      # noqa: E731
    by_name = {r[0]: r for r in rows}
    for shift in ss.SHIFTS:                                                # a split deletion lands where the 12D of the event does
        assert [(g[0], g[1], g[2], g[3]) for g in of("split_shift%d" % shift)] == [(sv.DEL, ss.SHIFT_AT[shift] - shift, 12, shift)]
        cluster = [c for c in clusters_of(tables) if c[:3] == (sv.DEL, ss.SHIFT_AT[shift] - shift, 12)]
        assert len(cluster) == 1 and cluster[0][3] >= 2 and cluster[0][4] == 1              # with the 12D read(s) of sv_cases
    assert [(g[1], g[3]) for g in of("split_stopped")] == [(sc.STOPPED_AT - 40, 40)]
    assert [g[3] for g in of("split_n_in_repeat")] == [30]
    for total in (63, 64, 65, 129):
        assert len(by_name[named["bytes%d" % total][0]][8]) == total and [(g[0], g[2]) for g in of("bytes%d" % total)] == [(sv.BND, -1)]
    for what, first in (("number_straddles", 58), ("entry_straddles", 60), ("semicolon_at_63", 64), ("semicolon_at_64", 65)):
        tag = by_name[named[what][0]][8]
        assert tag.index(b";") == first - 1 and len(tag) > 64 and [g[0] for g in of(what)] == [sv.BND, sv.BND]
    assert by_name[named["number_straddles"][0]][8][63:67] == b"2101"
    assert sorted(g[5] for g in of("seven_entries")) == list(range(-7, 0)) and {g[0] for g in of("seven_entries")} == {sv.DEL}
    assert status[named["eight_entries"][0]] == sv.TOO_MANY and by_name[named["eight_entries"][0]][8].count(b";") == 8
    assert status[named["pos_max"][0]] == sv.PARSED and status[named["pos_eleven"][0]] == sv.BAD_SA
    at_end = of("ends_at_length")
    assert len(at_end) == 1 and at_end[0][1] + at_end[0][2] + at_end[0][3] == ss.LENGTH - 20
    assert status[[n for n in named["ends_past_length"] if by_name[n][8]][0]] == sv.BAD_SA
    assert [g[0] for g in of("unknown_rname")] == [sv.BND] and of("unknown_rname")[0][2] == -1
    assert all(status[n] == sv.NO_TAG for n in named["not_counting"])
    both = [g for g in sigs if g[4] == ordinal[named["both_kinds"][0]]]
    assert sorted(g[5] for g in both) == [-1, 1]
    for cause in ss.BAD_CAUSES:
        assert status[named["bad: " + cause][0]] == sv.BAD_SA, cause
    assert counts["bad_sa"] == len(ss.BAD_CAUSES) + 2 and counts["too_many"] == 1
    assert counts["junctions"] == counts["junctions_dropped"] + counts["junctions_small"] + counts["junctions_unplaced"] + counts["split_signatures"]
    cut, cut_counts = sv.restated(ss.spans_of(rows, ss.LENGTH, range(sc.SPAN, ss.LENGTH, sc.SPAN)), reference, **p, **KW)
    same_split_tables(cut, tables)
    assert {k: cut_counts[k] for k in sv.SPLIT_METRIC_STATS} == {k: counts[k] for k in sv.SPLIT_METRIC_STATS}
    over = by_name[named["over_two_spans"][0]]
    assert over[2] < 2 * sc.SPAN < over[2] + 40 and status[over[0]] == sv.WITH_A_ROW


def test_fuzz_has_what_it_is_run_for():
    seen = dict.fromkeys(sv.SPLIT_COUNT_NAMES, 0)
    types = set()
    for seed in ss.FUZZ_SEEDS[:8]:
        _, _, tables, counts = fuzz_restated(seed)
        for k in seen:
            seen[k] += counts[k]
        types |= set(tables["SIGNATURES_TYPE"].tolist())
        assert (tables["SIGNATURES_SHIFT"][tables["SIGNATURES_TYPE"] == sv.DEL] >= 0).all()
    assert all(seen[k] > 0 for k in seen if k != "too_many") and {sv.DEL, sv.DUP, sv.INV3, sv.INV5, sv.BND} <= types, (seen, types)


# ---- the clusters: the library's host rules against the restatement ------------------------------------------------------------------
def test_cluster_split_native_equals_restated_and_the_old_clustering_is_unchanged():
    sets = [rows_of(stress_restated()[3], "SIGNATURES_", sv.SIGNATURE_COLUMNS)]
    sets += [rows_of(fuzz_restated(seed)[2], "SIGNATURES_", sv.SIGNATURE_COLUMNS) for seed in ss.FUZZ_SEEDS[:6]]
    sets += [case.signatures for case in ss.HAND_TABLE] + [[]]
    for rows in sets:
        rows = [g for g in rows if g[0] != sv.BND]
        for gap, percent, support in ((20, 70, 2), (0, 100, 1), (100, 70, 3), (1000, 50, 1)):
            want = sv.clustered(rows, gap, percent, support, with_sr=True)
            assert sv.clustered_split_native(rows, gap, percent, support) == want
            assert sv.clustered_split_native(rows[::-1], gap, percent, support) == want
            assert [c[:13] for c in want] == sv.clustered(rows, gap, percent, support)
    assert any(c[13] for c in sv.clustered(sets[0], 20, 70, 2, with_sr=True))
    for _, signatures, want in sc.CLUSTER_TABLE:                             # 7p's entry point and its hand table
        assert sv.clustered_native(signatures, 10, 70, 2) == want
        assert [c[:13] for c in sv.clustered_split_native(signatures, 10, 70, 2)] == want
        assert all(c[13] == 0 for c in sv.clustered_split_native(signatures, 10, 70, 2))
    with pytest.raises(RuntimeError, match="signature 0: type 2"):
        sv.clustered_native([(2, 5, 9, 0, 0, -1, 0, 0)])
    with pytest.raises(RuntimeError, match="signature 0: type 5"):
        sv.clustered_split_native([(5, 5, 9, 0, 0, -1, 0, 0)])
    assert sv.clustered([(5, 5, 1, 7, 0, -1, 0, 0), (5, 5, 1, 7, 1, -1, 0, 0)], 10, 70, 1, with_sr=True) == []     # a BND is never clustered


# ---- the BAM reader -------------------------------------------------------------------------------------------------------------
def test_fetch_with_sa_round_trips_the_tags(tmp_path):
    from tests.bam_writer import Read, write_bam
    reference = ss.PLAIN
    long_tag = ss.sa("chr2", 7, "-", "10S20M") * 40
    tags = [b"SAZ" + ss.sa("chr1", 130, "+", "15S15M") + b"\0",
            b"",                                                             # no tag at all
            b"NMC\x03SAZ" + long_tag + b"\0HPC\x02",                         # between other fields
            b"SAi" + (7).to_bytes(4, "little"),                              # SA of another type: an empty range
            b"XZZ" + b"SA:not this one\0",                                   # the letters SA inside another field's text
            b"MLBC" + (3).to_bytes(4, "little") + b"\1\2\3" + b"SAZ;\0"]
    want = [ss.sa("chr1", 130, "+", "15S15M"), b"", long_tag, b"", b"", b";"]
    reads = [Read("r%d" % i, 100 + i, [(sc.M, 15), (sc.S, 15)], reference[100 + i:130 + i], [30] * 30, tags=t) for i, t in enumerate(tags)]
    path = str(tmp_path / "sa.bam")
    write_bam(path, [("chr1", len(reference)), ("chr2", 1000)], reads)
    with BamFile(path) as bam:
        got, splits = bam.fetch_with_sa("chr1")
        plain = bam.fetch("chr1")
        assert isinstance(splits, Splits) and splits.bytes.dtype == np.uint8 and splits.offsets.dtype == np.int64
        assert splits.offsets.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in want])]).tolist()
        assert splits.bytes.tobytes() == b"".join(want) and got.hp.tolist() == [0, 0, 2, 0, 0, 0]
        for f in dataclasses.fields(plain):
            a, b = getattr(got, f.name), getattr(plain, f.name)
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, f.name
        part, part_splits = bam.fetch_with_sa("chr1", 0, 103)                # a region: the reads that start below 103
        assert part.n_reads == 3 and part_splits.bytes.tobytes() == want[0] + want[2]
        # after the other two fetches there are no such arrays: the selectors are refused, as tests/test_methylation.py has it of 17
        from hello_amd._abi import handle_array
        import ctypes as C
        for entry in (bam._lib.hello_bam_fetch, bam._lib.hello_bam_fetch_mods):
            r = C.c_void_p()
            assert entry(bam._h, b"chr1", 0, 300, -1, C.byref(r)) == 0
            try:
                for which in (17, 18):
                    with pytest.raises(RuntimeError, match="no read array %d: hello_bam_fetch_sa alone fills it" % which):
                        handle_array(bam._lib.hello_bam_reads_array, r, which, np.uint8)
            finally:
                bam._lib.hello_bam_reads_free(r)
    # the restatement reads what the reader gives: the first record is a split read of the hand cases
    tables, counts = sv.restated([(got, splits, 0, len(reference))], reference, **ss.HAND, contigs=["chr1", "chr2"], own=0)
    assert counts["split_reads"] == 3 and counts["bad_sa"] == 1 and counts["too_many"] == 1
    assert (sv.DEL, 115, 15, 0, 0, -1, 0, 0) in rows_of(tables, "SIGNATURES_", sv.SIGNATURE_COLUMNS)


# ---- the files ------------------------------------------------------------------------------------------------------------------
def test_vcf_text_byte_for_byte(tmp_path):
    case = ss.HAND_TABLE[0]
    tables, counts = sv.restated(ss.spans_of(case.rows, 25), case.reference, **ss.HAND, **KW)
    found = sv.Events(split=True)
    found.set("chr1", np.frombuffer(case.reference.encode(), np.uint8), tables, counts)
    genotype = sv.genotype_of(2, 1)
    line = ss.HAND_VCF_LINES % ((sv.GT_TEXT[genotype[0]],) + genotype[1:])
    assert found.vcf_text() == "##fileformat=VCFv4.2\n##contig=<ID=chr1,length=25>\n" + sv.SPLIT_VCF_HEADER + line
    for needed in ("##ALT=<ID=DUP,", "##ALT=<ID=INV,", "##INFO=<ID=SR,", "##INFO=<ID=JUNCTION,"):
        assert needed in sv.SPLIT_VCF_HEADER and needed not in sv.VCF_HEADER
    plain = sv.Events()                                                      # without --sv_split the same tables write 7p's text
    plain.set("chr1", np.frombuffer(case.reference.encode(), np.uint8), tables, counts)
    assert ";SR=" not in plain.vcf_text() and sv.VCF_HEADER in plain.vcf_text() and "STATS" in plain.tables["chr1"]
    assert plain.tables["chr1"]["STATS"].shape == (len(sv.METRIC_STATS),) and "CANDIDATES_SR" not in plain.tables["chr1"]
    assert found.tables["chr1"]["STATS"].tolist() == [counts[k] for k in sv.SPLIT_METRIC_STATS]
    first, again = found.write_all(str(tmp_path / "a")), found.write_all(str(tmp_path / "b"))
    assert open(first[1], "rb").read() == open(again[1], "rb").read()
    with np.load(first[1]) as z:
        assert z["CANDIDATES_SR_0"].tolist() == [1] and z["SIGNATURES_OP_0"].tolist() == [1, -1]
    ref = np.frombuffer(ss.PLAIN.encode(), np.uint8)
    row = dict(dict.fromkeys(sv.CANDIDATE_COLUMNS + ("SR",), 0), POS=100, LEN=40, DV=2, SR=2, GT=1)
    dup = sv.vcf_line("c", ref, dict(row, TYPE=sv.DUP), split=True)
    assert dup.startswith("c\t100\t.\t%s\t<DUP>\t.\tPASS\tSVTYPE=DUP;SVLEN=40;END=140;SUPPORT=2;" % ss.PLAIN[99]) and ";SR=2\t" in dup
    assert ";SR=2;JUNCTION=3to3\t" in sv.vcf_line("c", ref, dict(row, TYPE=sv.INV3), split=True)
    inv = sv.vcf_line("c", ref, dict(row, TYPE=sv.INV5), split=True)
    assert "\t<INV>\t" in inv and "SVTYPE=INV;SVLEN=40;END=140;" in inv and ";SR=2;JUNCTION=5to5\t" in inv


# ---- the refusals that need no device -------------------------------------------------------------------------------------------------
def test_host_side_refusals():
    case = ss.HAND_TABLE[0]
    reads, splits = ss.split_set(case.rows)
    with sv.Caller(case.reference, 5, 3) as caller:
        with pytest.raises(RuntimeError, match="hello_sv_add_split before hello_sv_contigs"):
            caller.add(reads, 0, 25, splits=splits)
        for names, own, said in (([], 0, "0 contigs"), (["a"], 1, "own contig 1 of 1"), (["a"], -1, "own contig -1"),
                                 (["a", "b", "a"], 0, "contig 'a' twice")):
            with pytest.raises(RuntimeError, match=said):
                caller.set_contigs(names, own)
        caller.set_contigs(ss.CONTIGS, ss.OWN)
        with pytest.raises(RuntimeError, match="hello_sv_contigs twice"):
            caller.set_contigs(ss.CONTIGS, ss.OWN)
        decreasing = splits.offsets.copy()
        decreasing[1] = 5
        decreasing[2] = 4
        for bad, said in ((Splits(splits.bytes, decreasing), "read 1: SA offsets decrease"),
                          (Splits(splits.bytes[:-1], splits.offsets), "SA offsets end at 20, 19 SA bytes"),
                          (Splits(splits.bytes, splits.offsets - 1), "SA offsets begin at -1")):
            with pytest.raises(RuntimeError, match=said):
                caller.add(reads, 0, 25, splits=bad)
        with pytest.raises(ValueError, match="2 SA offsets for 2 reads"):
            caller.add(reads, 0, 25, splits=Splits(splits.bytes, splits.offsets[:2]))
        with pytest.raises(RuntimeError, match=r"span \[0, 26\) of a reference of 25 bases"):
            caller.add(reads, 0, 26, splits=splits)
        assert all(v == 0 for v in caller.stats().values()) and set(sv.SPLIT_COUNT_NAMES) < set(caller.stats())
        arrays = caller.arrays()
        assert arrays["SIGNATURES_POS"].shape == (0,) and arrays["SPLIT_STATUS"].shape == (0,) and "CANDIDATES_SR" not in arrays
        with pytest.raises(RuntimeError, match="before hello_sv_finish"):
            caller._array(29, np.int64)
        caller.finish()
        assert caller.arrays()["CANDIDATES_SR"].shape == (0,)
        with pytest.raises(RuntimeError, match="hello_sv_add_split after hello_sv_finish"):
            caller.add(reads, 0, 25, splits=splits)


def _args(**kw):
    base = dict(sv=False, sv_split=False, shards=None, from_bam=False, from_bams=False, gpus=1, ibam=None, pbam=None)
    base.update(dict.fromkeys(call.SV_OPTIONS))
    base.update(kw)
    return argparse.Namespace(**base)


def test_check_sv_refuses_sv_split_without_sv_and_names_the_fix(monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    call.check_sv(_args())
    call.check_sv(_args(sv=True, sv_split=True, from_bam=True, pbam="p.bam"))
    with pytest.raises(SystemExit, match="--sv_split adds the split alignments .* add --sv, or drop --sv_split"):
        call.check_sv(_args(sv_split=True, from_bam=True))
    args = call.parser().parse_args(["--workdir", "w", "--network", "n"])
    assert args.sv_split is False
    args = call.parser().parse_args(["--workdir", "w", "--network", "n", "--sv", "--sv_split"])
    assert args.sv and args.sv_split
    assert sv.parser().parse_args(["--bam", "b", "--ref", "r", "--output_prefix", "p", "--split"]).split is True
    assert sv.parser().parse_args(["--bam", "b", "--ref", "r", "--output_prefix", "p"]).split is False


def test_pass_1_of_haplotag_runs_without_sv_split(monkeypatch):
    seen = []
    monkeypatch.setattr(call, "main", lambda ns: seen.append(ns) or os.path.join(ns.workdir, "results.output.vcf"))
    args = call.parser().parse_args(["--workdir", "w", "--network", "n", "--from_bam", "--pbam", "p.bam", "--include_hp", "--haplotag", "--sv",
                                     "--sv_split"])
    call.haplotag_passes(args)
    first, second = seen
    assert first.sv is False and first.sv_split is False and second.sv is True and second.sv_split is True
    call.check_sv(first)


# ---- csrc/sv_split.h under the sanitizers, against the restatement ----------------------------------------------------------------------
def _block(lines, want, reference, rows, p):
    """One block of the program's input, and what the restatement says it prints."""
    lines.append("P %d %d %d %d %d %d %d %d" % (len(reference), ss.OWN, p["min_size"], p["flank"], p["mapq_threshold"], p["cluster_gap"],
                                                p["len_ratio_percent"], p["min_support"]))
    lines += ["C " + name for name in ss.CONTIGS] + ["F " + reference]
    ref = np.frombuffer(reference.encode(), np.uint8)
    ordinal, found = 0, []
    for r in rows:
        if not sv.counted(r[1], r[6], p["mapq_threshold"]):
            continue
        if r[8]:
            cigar = "".join("%d%s" % (n, "MIDNSHP=X"[op]) for op, n in r[3])
            lines.append("R %d %d %d %d %d %s %s" % (r[2], r[1], r[6], r[7], ordinal, cigar, r[8].hex()))
            status, made, counts = sv.split_rows_of((r[2], r[1], r[3], r[6]), r[8], ss.CONTIGS, ss.OWN, ref, p["min_size"], p["flank"],
                                                    p["mapq_threshold"], ordinal, r[7])
            want.append("S %d %d %d %d %d" % (status, counts["junctions"], counts["junctions_dropped"], counts["junctions_small"],
                                              counts["junctions_unplaced"]))
            want += ["G " + " ".join(str(v) for v in g) for g in made]
            found += made
        ordinal += 1
    lines.append("E")
    want += ["K " + " ".join(str(v) for v in c) for c in sv.clustered(found, p["cluster_gap"], p["len_ratio_percent"], p["min_support"], with_sr=True)]
    want.append("E")


def test_split_rules_are_clean_under_sanitizers_and_equal_the_restatement(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler on this box"
    exe = str(tmp_path / "sv_split_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                            os.path.join(ROOT, "tests", "abi", "sv_split_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    lines, want = [], []
    for case in ss.HAND_TABLE:
        _block(lines, want, case.reference, case.rows, ss.HAND)
    reference, rows, _, _, _ = stress_restated()
    _block(lines, want, reference, rows, ss.STRESS)
    for seed in ss.FUZZ_SEEDS:
        reference, rows = ss.fuzz(seed)
        _block(lines, want, reference, rows, ss.FUZZ)
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "sv_split_check: ok" in run.stdout, (run.returncode, run.stdout[-500:], run.stderr[-3000:])
    got = run.stdout.splitlines()[:-1]
    assert len(got) == len(want) and len([x for x in got if x.startswith("G")]) > 500
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a, b)
