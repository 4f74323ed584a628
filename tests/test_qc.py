"""Quality metrics without a GPU (hello_amd/qc.py): the plain-Python restatement against the tables worked by
hand (tests/qc_cases.py), the summary on tables small enough to check by hand, ``read_bed``, the files' exact text, the spans, the
refusals of ``call --qc`` and the C ABI -- declarations, exports and the host-side validation, which needs no device."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hello_amd import call, qc
from tests import qc_cases as cc
from tests.bam_writer import Read, write_bam
from tests.test_stage_host import one_read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def same_tables(got, want, names=qc.TABLE_NAMES):
    for name in names:
        assert got[name].dtype == np.int64 and got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name]), (name, np.argwhere(got[name] != want[name])[:5].tolist())


def spans_of(case, cuts):
    edges = [0] + list(cuts) + [len(case.reference)]
    return [(cc.read_set(cc.overlapping(case.rows, lo, hi)), lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.HAND_TABLE, ids=[c.name for c in cc.HAND_TABLE])
def test_restatement_equals_the_hand_table(case):
    want = case.expected()
    for cuts in ((), (case.cut(),)):                                            # whole, and cut through the middle of a read
        got, counts = qc.restated(spans_of(case, cuts), case.reference, case.targets, cc.WINDOW)
        same_tables(got, want)
        assert {k: counts[k] for k in qc.METRIC_STATS} == case.want_counts()
        assert counts["belonging"] == len(case.rows) == int(got["FLAGS"][0])
    assert counts["reads_given"] >= len(case.rows)                             # the read that was cut is given twice


def test_the_hand_table_names_every_rule():
    names = " / ".join(c.name for c in cc.HAND_TABLE)
    for rule in ("forward and reverse", "read 2", "insertion as first and as last", "D before any base", "soft and hard", "N skip",
                 "lower-case reference", "N in the reference", "N in a read", "FLAGS only", "below the threshold", "improper pair",
                 "past the reference", "FR, RF and TANDEM", "refused group", "single", "touching targets", "clipped", "empty read set"):
        assert rule in names, rule
    assert len(cc.REF) == 200 and all(len(c.reference) == 200 for c in cc.HAND_TABLE)


def test_the_parts_of_the_restatement():
    assert qc.measured(np.array([0, 0x4, 0x100, 0x800, 0x400, 0x200, 0x63, 0x41], np.uint16)).tolist() == [1, 0, 0, 0, 0, 0, 1, 1]
    assert [int(qc.cycle_of(i, 700, False)) for i in (0, 511, 512, 699)] == [0, 511, 512, 512]
    assert [int(qc.cycle_of(i, 700, True)) for i in (0, 187, 188, 699)] == [512, 512, 511, 0]
    assert qc.flag_row(0x63, 0) == [1, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1]
    assert qc.flag_row(0x9 | 0x10 | 0x80, 7) == [1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 1, 0]
    assert qc.flag_row(0x4, 0)[12] == 0                                         # an unmapped read's mapq 0 is no mapq0
    rd = cc.read_set([(1, 0, 10, [(cc.M, 2), (cc.D, 3), (cc.N, 4), (cc.M, 2)], "ACGT", [30] * 4, 60)])
    assert qc.depth_of(rd, 8, 22).tolist() == [0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0]
    assert qc.depth_of(rd, 11, 13, 61).tolist() == [0, 0]
    table, counts = qc.insert_of([7, 7], [0x63, 0x93], [100, 5000], [250, 5150])
    assert table[0, 4095] == 1 and table.sum() == 1 and counts == dict(pairs=1, groups_refused=0)
    with pytest.raises(ValueError, match="not sorted behind"):
        qc.check_targets([(10, 20), (19, 30)])
    with pytest.raises(ValueError, match="is empty"):
        qc.check_targets([(10, 10)])
    assert qc.check_targets([(10, 20), (20, 30)]).tolist() == [[10, 20], [20, 30]]
    with pytest.raises(ValueError, match="does not consume exactly"):
        qc.tables_of(one_read([(0, 5)], 4), cc.REF, 0, 200)


# ---- the summary ----------------------------------------------------------------------------------------------------------------
def test_summary_on_tables_checked_by_hand():
    t = qc.empty_tables(200)
    empty = qc.summary(t)
    assert set(empty.values()) == {0.0} and not any("cycle" in k or "empirical" in k for k in empty)      # nothing divides by 0
    assert qc.histogram_median(np.zeros(5, np.int64)) == 0
    # medians at ties: the smallest value whose cumulative count reaches half
    assert qc.histogram_median([2, 0, 0, 1, 1]) == 0 and qc.histogram_median([1, 0, 0, 1, 1]) == 3
    assert qc.histogram_median([0, 1, 1]) == 1 and qc.histogram_median([0, 1, 2]) == 2
    t["FLAGS"][[0, 1, 4, 7]] = [8, 2, 1, 4]
    t["DEPTH_HIST"][[0, 3, 10]] = [2, 1, 1]
    t["TARGET_DEPTH_HIST"][[3, 10]] = [1, 1]
    t["CYCLE"][0, 0] = [2, 61, 2, 1, 0, 0, 0]
    t["CYCLE"][1, 5] = [4, 100, 2, 0, 0, 0, 0]
    t["QUALITY"][30] = [98, 0]
    t["QUALITY"][20] = [8, 1]
    t["INSERT"][0, [100, 200, 300, 4095]] = [1, 1, 2, 1]
    t["INSERT"][1, 50] = 1
    s = qc.summary(t, with_targets=True)
    want = {"mapped_fraction": 0.75, "duplicate_fraction": 0.125, "proper_pair_fraction": 0.5, "mean_depth": 3.25, "median_depth": 0.0,
            "depth_ge_1": 0.5, "depth_ge_5": 0.25, "depth_ge_10": 0.25, "depth_ge_15": 0.0, "depth_ge_50": 0.0,
            "target_mean_depth": 6.5, "target_median_depth": 3.0, "target_depth_ge_5": 0.5, "mismatch_rate": 0.25,
            "read1.cycle0.mean_quality": 30.5, "read2.cycle5.mean_quality": 25.0, "quality30.empirical": 20.0,
            "insert_median": 200.0, "insert_mad": 100.0, "fr_fraction": 5 / 6, "rf_fraction": 1 / 6, "tandem_fraction": 0.0}
    for k, v in want.items():
        assert s[k] == pytest.approx(v, abs=1e-12), k
    assert "%.4f" % s["quality20.empirical"] == "6.9897"                       # -10 log10(2 / 10)
    assert [k for k in s if "cycle" in k] == ["read1.cycle0.mean_quality", "read2.cycle5.mean_quality"]
    assert "target_mean_depth" not in qc.summary(t)


# ---- files ----------------------------------------------------------------------------------------------------------------------
def test_read_bed_sorts_merges_overlaps_and_keeps_touching_apart(tmp_path):
    path = tmp_path / "t.bed"
    path.write_text("# a comment\ntrack name=x\nchr2\t5\t9\textra\nchr1\t30\t40\nchr1\t10\t20\nchr1\t20\t25\nchr1\t35\t50\nchr1 38 39\n\n")
    assert qc.read_bed(str(path)) == {"chr2": [(5, 9)], "chr1": [(10, 20), (20, 25), (30, 50)]}
    for bad in ("chr1\t9\t9\n", "chr1\t-1\t5\n", "chr1\t7\n"):
        path.write_text(bad)
        with pytest.raises(ValueError, match="t.bed:1"):
            qc.read_bed(str(path))


def small_metrics():
    m = qc.Metrics(50, True)
    t = qc.empty_tables(120, 2, 50)
    t["FLAGS"][[0, 4]] = [4, 1]
    t["WINDOW_SUM"][:] = [100, 25, 10]
    t["TARGET_SUM"][:] = [15, 5]
    t["TARGET_COVERED"][:] = [10, 5]
    t["DEPTH_HIST"][[0, 2]] = [60, 60]
    m.set("chr1", 120, t, dict(dict.fromkeys(qc.COUNT_NAMES, 0), measured=3, pairs=1), [(10, 20), (110, 150)])
    return m


def test_save_load_and_the_exact_text_of_the_files(tmp_path):
    m = small_metrics()
    files = m.write_all(str(tmp_path / "qc.illumina"))
    assert [os.path.basename(f) for f in files] == ["qc.illumina.metrics.txt", "qc.illumina.tables.npz", "qc.illumina.windows.bedgraph",
                                                    "qc.illumina.targets.tsv"]
    assert open(files[2]).read() == "chr1\t0\t50\t2.0000\nchr1\t50\t100\t0.5000\nchr1\t100\t120\t0.5000\n"
    assert open(files[3]).read() == "chr1\t10\t20\t1.5000\t1.0000\nchr1\t110\t120\t0.5000\t0.5000\n"
    lines = open(files[0]).read().splitlines()
    n = len(qc.FLAG_NAMES) + len(qc.METRIC_STATS)
    assert lines[:2] == ["chr1.reads\t4", "chr1.unmapped\t0"] and lines[4] == "chr1.duplicate\t1" and lines[13] == "chr1.measured\t3"
    assert lines[n] == "total.reads\t4" and lines[n + 17] == "total.pairs\t1" and lines[2 * n - 1] == "total.groups_refused\t0"
    assert lines[2 * n:2 * n + 5] == ["summary.mapped_fraction\t1.0000", "summary.duplicate_fraction\t0.2500",
                                      "summary.proper_pair_fraction\t0.0000", "summary.mean_depth\t1.0000", "summary.median_depth\t0.0000"]
    assert all(re.fullmatch(r"(chr1|total)\.[a-z0-9_]+\t\d+|summary\.[a-z0-9_.]+\t-?\d+\.\d{4}", x) for x in lines)
    assert "summary.target_mean_depth\t0.0000" in lines and lines[-1] == "summary.tandem_fraction\t0.0000"
    loaded = qc.Metrics.load(files[1])
    assert (loaded.window, loaded.has_targets, loaded.lengths) == (50, True, {"chr1": 120}) and list(loaded.tables) == ["chr1"]
    same_tables(loaded.tables["chr1"], m.tables["chr1"], qc.TABLE_NAMES + ("STATS",))
    assert loaded.targets["chr1"].tolist() == [[10, 20], [110, 150]] and loaded.summary() == m.summary()
    again = loaded.write_all(str(tmp_path / "again"))
    for a, b in zip(files, again):
        if not a.endswith(".npz"):
            assert open(a, "rb").read() == open(b, "rb").read()
    plain = qc.Metrics(50)                                                      # without targets: three files, no target lines
    plain.set("chr1", 120, m.tables["chr1"], dict.fromkeys(qc.COUNT_NAMES, 0))
    assert len(plain.write_all(str(tmp_path / "plain"))) == 3 and "target" not in open(tmp_path / "plain.metrics.txt").read()


# ---- the spans ------------------------------------------------------------------------------------------------------------------
_made: dict = {}


def stress_bam(tmp_path_factory):
    """The edge-stress chromosome as a BAM and a FASTA-like dictionary -- made once, for this file and tests/test_gpu_qc.py."""
    if not _made:
        tmp = tmp_path_factory.mktemp("qc")
        reference, rows = cc.stress()
        reads = [Read("n%d" % name, pos, cigar, bases.upper(), quals, flag, mapq) for name, flag, pos, cigar, bases, quals, mapq in rows]
        path = str(tmp / "s.bam")
        write_bam(path, [("chr1", cc.LENGTH)], reads, index=True, block_bytes=20000)
        targets = {"chr1": cc.STRESS_TARGETS}
        _made.update(path=path, genome={"chr1": reference}, rows=rows, targets=targets,
                     whole=qc.measure(path, {"chr1": reference}, targets=targets, window=7, restatement=True))
    return _made


def test_tables_of_the_restatement_do_not_depend_on_the_spans(tmp_path_factory):
    s = stress_bam(tmp_path_factory)
    small = qc.measure(s["path"], s["genome"], ["chr1"], s["targets"], window=7, max_span=cc.SPAN, restatement=True)
    same_tables(small.tables["chr1"], s["whole"].tables["chr1"], qc.TABLE_NAMES + ("STATS",))
    # and they equal the rows, without a BAM in between (the names hash differently, the pairs are the same)
    direct, counts = qc.restated([(cc.read_set(s["rows"]), 0, cc.LENGTH)], s["genome"]["chr1"], cc.STRESS_TARGETS, 7)
    same_tables(s["whole"].tables["chr1"], direct)
    assert s["whole"].tables["chr1"]["STATS"].tolist() == [counts[k] for k in qc.METRIC_STATS]
    with pytest.raises(ValueError, match="no sequence named"):
        qc.measure(s["path"], s["genome"], ["chr9"], restatement=True)
    with pytest.raises(ValueError, match="in the BAM header"):
        qc.measure(s["path"], {"chr1": s["genome"]["chr1"][:-1]}, restatement=True)


# ---- the refusals and the flags -------------------------------------------------------------------------------------------------
def _args(*extra):
    return call.parser().parse_args(["--workdir", "w", "--network", "m.npz"] + list(extra))


def test_refusals_of_qc_name_the_fix(monkeypatch):
    bam = ["--ibam", "x.bam", "--ref", "g.fa"]
    with pytest.raises(SystemExit, match="add --from_bam .*or --from_bams"):
        call.check_qc(_args("--qc", *bam))
    with pytest.raises(SystemExit, match="drop --shards"):
        call.check_qc(_args("--qc", "--from_bam", "--shards", "s", *bam))
    with pytest.raises(SystemExit, match="--gpus 1"):
        call.check_qc(_args("--qc", "--from_bam", "--gpus", "2", *bam))
    with pytest.raises(SystemExit, match="add --qc, or drop --qc_regions"):
        call.check_qc(_args("--from_bam", "--qc_regions", "t.bed", *bam))
    with pytest.raises(SystemExit, match="add --qc, or drop --qc_window"):
        call.check_qc(_args("--from_bam", "--qc_window", "500", *bam))
    with pytest.raises(SystemExit, match="give 1 or more"):
        call.check_qc(_args("--qc", "--from_bam", "--qc_window", "0", *bam))
    with pytest.raises(SystemExit, match="--qc"):
        call.main(_args("--qc", "--shards", "s"))
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="plain command"):
        call.check_qc(_args("--qc", "--from_bam", *bam))
    monkeypatch.delenv("RANK")
    call.check_qc(_args("--qc", "--from_bam", "--qc_regions", "t.bed", "--qc_window", "1", *bam))
    call.check_qc(_args("--qc", "--from_bams", "--resident", "--pbam", "p.bam", *bam))
    call.check_qc(_args("--shards", "s"))
    plain = _args("--shards", "s")
    assert (plain.qc, plain.qc_regions, plain.qc_window) == (False, None, None) and call.qc_pass(plain, {}) == []
    argv = call._argv_of(_args("--qc", "--qc_window", "7"))
    assert "--qc" in argv and argv[argv.index("--qc_window") + 1] == "7" and "--qc_regions" not in argv
    args = qc.parser().parse_args(["--bam", "b.bam", "--ref", "g.fa", "--output_prefix", "p", "--regions", "t.bed", "--window", "5",
                                   "--chromosomes", "a,b", "--mapq_threshold", "3", "--device", "1"])
    assert (args.bam, args.ref, args.output_prefix, args.regions, args.window, args.chromosomes, args.mapq_threshold, args.device) == \
        ("b.bam", "g.fa", "p", "t.bed", 5, "a,b", 3, 1)


def test_qc_is_cleared_for_pass_1_of_haplotag(monkeypatch, tmp_path):
    seen = []
    monkeypatch.setattr(call, "main", lambda args: seen.append(args) or os.path.join(args.workdir, "results.output.vcf"))
    args = _args("--from_bam", "--ibam", "x.bam", "--ref", "g.fa", "--include_hp", "--haplotag", "--qc", "--qc_regions", "t.bed",
                 "--qc_window", "500")
    call.haplotag_passes(args)
    first, second = seen
    assert (first.qc, first.qc_regions, first.qc_window, first.phase) == (False, None, None, True)
    assert (second.qc, second.qc_regions, second.qc_window, second.haplotag) == (True, "t.bed", 500, False)
    assert args.qc is True and args.haplotag is True                            # the caller's arguments are left as they were


def test_the_route_names_the_files_and_passes_its_threshold(monkeypatch, tmp_path):
    calls = []

    def measure(bam, genome, chromosomes, targets, window, mapq_threshold, **kw):
        calls.append((bam, tuple(chromosomes), targets, window, mapq_threshold))
        return small_metrics()
    monkeypatch.setattr(qc, "measure", measure)
    bed = tmp_path / "t.bed"
    bed.write_text("chr1\t10\t20\n")
    work = str(tmp_path / "w")
    os.makedirs(work)
    args = call.parser().parse_args(["--workdir", work, "--network", "m.npz", "--from_bams", "--ibam", "i.bam", "--pbam", "p.bam",
                                     "--ref", "g.fa", "--qc", "--qc_regions", str(bed), "--mapq_threshold", "3"])
    written = call.qc_pass(args, {"chr1": "ACGT"})
    assert calls == [("i.bam", ("chr1",), {"chr1": [(10, 20)]}, 1000, 3), ("p.bam", ("chr1",), {"chr1": [(10, 20)]}, 1000, 3)]
    assert sorted(os.listdir(work)) == sorted("qc.%s.%s" % (t, s) for t in ("illumina", "pacbio")
                                              for s in ("metrics.txt", "tables.npz", "windows.bedgraph", "targets.tsv"))
    assert len(written) == 8
    calls.clear()
    one = call.parser().parse_args(["--workdir", work, "--network", "m.npz", "--from_bam", "--pbam", "p.bam", "--ref", "g.fa", "--qc",
                                    "--qc_window", "9", "--mapq_threshold", "3", "--chromosomes", "chr1"])
    assert [os.path.basename(f) for f in call.qc_pass(one, {"chr1": "ACGT"})][0] == "qc.pacbio.metrics.txt"
    assert calls == [("p.bam", ("chr1",), None, 9, 10)]                         # --from_bam runs at the default thresholds


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("hello_qc_add", "hello_qc_finish", "hello_qc_array", "hello_qc_stats")


def test_abi_symbols_are_declared_exported_and_mirrored():
    from hello_amd.engine import load_library
    header = open(os.path.join(ROOT, "include", "hello_mi355x.h")).read()
    lib = load_library()
    for symbol in SYMBOLS:
        assert re.search(r"^int %s\(" % symbol, header, flags=re.M), symbol
        assert hasattr(lib, symbol), symbol
    assert re.search(r"^void hello_qc_free\(", header, flags=re.M) and hasattr(lib, "hello_qc_free")
    assert int(re.search(r"#define HELLO_QC_STATS (\d+)", header).group(1)) == len(qc.STAT_NAMES) == 12
    for which, name in enumerate(qc.TABLE_NAMES):
        assert int(re.search(r"HELLO_QC_%s = (\d+)" % name, header).group(1)) == which
    define = lambda name: int(re.search(r"#define HELLO_QC_%s (\d+)" % name, header).group(1))      # noqa: E731
    assert (define("FLAG_FIELDS"), define("CYCLES"), define("CYCLE_FIELDS"), define("LENGTHS"), define("DEPTHS"), define("INSERTS")) == \
        (len(qc.FLAG_NAMES), qc.LAST_CYCLE + 1, len(qc.CYCLE_FIELDS), qc.LAST_LENGTH + 1, qc.LAST_DEPTH + 1, qc.LAST_INSERT + 1)
    assert re.search(r"#define HELLO_ABI_VERSION 2\b", header)
    bound = qc._lib()
    assert len(bound.hello_qc_add.argtypes) == 23 and bound.hello_qc_free.restype is None
    text = open(os.path.join(ROOT, "hello_amd", "csrc", "qc.hip")).read()      # one copy of the join
    assert '#include "phase_pair.h"' in text and "pair_probe" not in text and "pair_insert_kernel" not in text


def test_the_host_walk_is_clean_under_sanitizers(tmp_path):
    """cigar.h: qc_walk as a stand-alone host program under AddressSanitizer and UBSan (tests/abi/qc_check.cpp)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler on this box"
    exe = str(tmp_path / "qc_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                            os.path.join(ROOT, "tests", "abi", "qc_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "qc_check: ok" in run.stdout, (run.returncode, run.stdout, run.stderr[-3000:])


REFERENCE = np.frombuffer(b"ACGT" * 50, np.uint8)


def call_qc(rd, lo=0, hi=200, targets=(), window=50, reference_length=200):
    lib, h = qc._lib(), C.c_void_p()
    t = np.asarray(list(targets), np.int64).reshape(-1, 2)
    starts, stops = np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])
    rc = lib.hello_qc_add(*rd.pointers(rd.hp)[:10], None, rd.n_reads, REFERENCE.ctypes.data, reference_length, lo, hi,
                          starts.ctypes.data, stops.ctypes.data, t.shape[0], 10, window, 0, C.byref(h))
    return rc, lib.hello_last_error().decode(), h


def two_reads():
    return cc.read_set([(1, 0, 10, cc.M4, "ACGT", [30] * 4, 60), (2, 0, 12, cc.M4, "ACGT", [30] * 4, 60)])


# (what is wrong, the message): every one is HELLO_ERR_ARG, before the device is looked for
REFUSALS = [
    (dict(read=dict(cigar=[(0, 5)], n_bases=4)), "read 0: CIGAR query length 5, 4 bases"),
    (dict(read=dict(cigar=[(0, 5)], n_bases=6)), "read 0: CIGAR query length 5, 6 bases"),
    (dict(read=dict(cigar=[(0, 5)], n_bases=4, mapq=0)), "read 0: CIGAR query length 5, 4 bases"),            # measured, not counted
    (dict(read=dict(cigar=[(0, 3), (9, 2)], n_bases=5)), "read 0: CIGAR operation 9"),
    (dict(read=dict(cigar=[(0, 5)], n_bases=5, ref_end=11)), "read 0: ref_end does not match its CIGAR"),
    (dict(read=dict(cigar=[(0, 5)], n_bases=5, ref_start=-1)), "read 0: ref_start -1"),
    (dict(change=dict(read_offsets=np.array([0, 4, 3], np.int64))), "read 1: offsets decrease"),
    (dict(change=dict(cigar_offsets=np.array([1, 2, 3], np.int64))), "offsets do not start at 0"),
    (dict(change=dict(ref_starts=np.array([12, 10], np.int64), ref_ends=np.array([16, 14], np.int64))), "read 1: reads are not coordinate-sorted (the BAM must be)"),
    (dict(lo=50, hi=50), "span [50, 50) of a reference of 200 bases"),
    (dict(lo=60, hi=50), "span [60, 50) of a reference of 200 bases"),
    (dict(lo=-1, hi=50), "span [-1, 50) of a reference of 200 bases"),
    (dict(hi=201), "span [0, 201) of a reference of 200 bases"),
    (dict(window=0), "window 0: at least 1"),
    (dict(targets=[(30, 40), (10, 20)]), "target 1: [10, 20) is empty, or not sorted behind its predecessor"),
    (dict(targets=[(10, 20), (19, 30)]), "target 1: [19, 30) is empty, or not sorted behind its predecessor"),
    (dict(targets=[(10, 10)]), "target 0: [10, 10) is empty, or not sorted behind its predecessor"),
    (dict(reference_length=-1), "negative count"),
]


@pytest.mark.parametrize("wrong,message", REFUSALS, ids=[r[1][:34].strip() + ("-%d" % i) for i, r in enumerate(REFUSALS)])
def test_add_refuses_before_it_looks_for_a_device(wrong, message):
    wrong = dict(wrong)
    rd = one_read(**wrong.pop("read")) if "read" in wrong else dataclasses.replace(two_reads(), **wrong.pop("change", {}))
    rc, said, handle = call_qc(rd, **wrong)
    assert (rc, said) == (ERR_ARG, message)
    assert not handle.value


def test_host_side_validation_needs_no_device():
    lib = qc._lib()
    error = lambda: lib.hello_last_error().decode()      # noqa: E731
    assert lib.hello_qc_add(*([None] * 11), 0, None, 0, 0, 0, None, None, 0, 10, 50, 0, None) == ERR_ARG and "NULL pointer" in error()
    assert lib.hello_qc_finish(None) == ERR_ARG and "NULL pointer" in error()
    assert lib.hello_qc_stats(None, (C.c_double * 12)()) == ERR_ARG and "NULL pointer" in error()
    p, n = C.c_void_p(), C.c_int64()
    assert lib.hello_qc_array(None, 0, C.byref(p), C.byref(n)) == ERR_ARG and "NULL pointer" in error()
    # a read that is not measured is not looked at: what the call answers then needs a device or needs none
    rc, said, handle = call_qc(one_read([(0, 5)], 4, flag=0x200))
    assert rc in (0, -5) and "read 0" not in said
    if handle:
        lib.hello_qc_free(handle)
