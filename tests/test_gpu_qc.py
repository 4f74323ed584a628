"""Quality metrics on the GPU (hello_qc_*; hello_amd/csrc/qc.hip): every table equals the restatement of hello_amd/qc.py integer for
integer -- on the tables worked by hand (tests/qc_cases.py), on an edge stress whose reads, deletions and targets cross the tile and
span edges, on the 6 kb paired chromosome of the duplicate-marking tests, and through the driver, where ``--qc`` writes the files
the restatement writes and leaves the VCF alone."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from hello_amd import _abi, call, markdup, qc
from hello_amd.phase import join_mates
from tests import markdup_cases as mc
from tests import qc_cases as cc
from tests.test_markdup import chromosome
from tests.test_qc import same_tables, spans_of, stress_bam

pytestmark = pytest.mark.gpu
MODEL_SEED = 1
ALL = qc.TABLE_NAMES + ("STATS",)


def same_bytes(a, b):
    for name in qc.TABLE_NAMES:
        assert a[name].tobytes() == b[name].tobytes(), name


# ---- (1) the hand tables through the kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.HAND_TABLE, ids=[c.name for c in cc.HAND_TABLE])
def test_hand_table_through_the_kernels(case):
    want = case.expected()
    runs = []
    for cuts in ((), (case.cut(),), (), (case.cut(),)):                        # whole and cut through a read, each twice
        spans = spans_of(case, cuts)
        got, stats = qc.metered(spans, case.reference, case.targets, cc.WINDOW)
        same_tables(got, want)
        same_tables(got, qc.restated(spans, case.reference, case.targets, cc.WINDOW)[0])
        assert {k: int(stats[k]) for k in qc.METRIC_STATS} == case.want_counts()
        assert int(stats["belonging"]) == len(case.rows) and int(stats["reads_given"]) == sum(rd.n_reads for rd, _, _ in spans)
        runs.append(got)
    same_bytes(runs[0], runs[2])
    same_bytes(runs[1], runs[3])
    same_bytes(runs[0], runs[1])


# ---- (2) the refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points():
    case = next(c for c in cc.HAND_TABLE if c.name.startswith("FR, RF"))
    rd = case.reads()
    with qc.Meter(case.reference, case.targets, cc.WINDOW) as m:
        m.add(cc.read_set(cc.overlapping(case.rows, 0, 100)), 0, 100)
        before, stats = m.arrays(), m.stats()
        assert "INSERT" not in before
        p, n = C.c_void_p(), C.c_int64()
        assert m._lib.hello_qc_array(m._h, qc.TABLE_NAMES.index("INSERT"), C.byref(p), C.byref(n)) == -1
        with pytest.raises(RuntimeError, match="exist after hello_qc_finish"):
            _abi.check(-1)
        rest = cc.read_set(cc.overlapping(case.rows, 100, 200))
        with pytest.raises(RuntimeError, match="offsets decrease"):
            m.add(dataclasses.replace(rd, read_offsets=np.array([0, 4, 8, 6] + [12] * 7, np.int64)), 100, 200)
        with pytest.raises(RuntimeError, match="CIGAR query length"):
            m.add(dataclasses.replace(rest, cigars=rest.cigars + np.uint32(16)), 100, 200)
        with pytest.raises(RuntimeError, match=r"begins below 100, where the previous one ended"):
            m.add(rest, 99, 200)
        with pytest.raises(RuntimeError, match=r"span \[100, 201\)"):
            m.add(rest, 100, 201)
        with pytest.raises(RuntimeError, match=r"span \[100, 100\)"):
            m.add(rest, 100, 100)
        for name, other, message in (("_window", 7, "differ from the first call's"), ("_threshold", 11, "differ from the first call's"),
                                     ("_stops", np.array([5], np.int64), "differ from the first call's"),
                                     ("_ref", np.frombuffer(b"ACGT" * 49, np.uint8), r"span \[100, 200\) of a reference of 196"),
                                     ("_window", 0, "window 0"), ("_device", 99, "names another device")):
            kept = getattr(m, name)
            setattr(m, name, other)
            if name == "_stops":
                m._starts = np.array([1], np.int64)
            with pytest.raises(RuntimeError, match=message):
                m.add(rest, 100, 200)
            setattr(m, name, kept)
            if name == "_stops":
                m._starts = np.zeros(0, np.int64)
        after = m.arrays()
        assert sorted(after) == sorted(before) and all(after[k].tobytes() == before[k].tobytes() for k in before)
        assert m.stats() == stats                                               # a refused add left nothing behind
        m.add(rest, 100, 200)
        m.finish()
        same_tables(m.arrays(), case.expected())
        with pytest.raises(RuntimeError, match="called once"):
            m.finish()
        with pytest.raises(RuntimeError, match="cannot be added after hello_qc_finish"):
            m.add(rest, 100, 200)
        same_tables(m.arrays(), case.expected())
    with qc.Meter(case.reference) as m:
        with pytest.raises(RuntimeError, match="NULL pointer"):
            m.finish()
    with pytest.raises(RuntimeError, match="device 99"):
        qc.metered([(rd, 0, 200)], case.reference, device=99)
    with pytest.raises(RuntimeError, match="not sorted behind"):
        qc.metered([(rd, 0, 200)], case.reference, [(10, 20), (15, 30)])


# ---- (3) the edge stress --------------------------------------------------------------------------------------------------------
def test_edge_stress_on_one_chromosome(tmp_path_factory):
    s = stress_bam(tmp_path_factory)
    rows, reference = s["rows"], s["genome"]["chr1"]
    ends = [(pos, pos + sum(k for op, k in cigar if op in (cc.M, cc.D, cc.N))) for _, _, pos, cigar, _, _, _ in rows]
    edges = [cc.TILE * k for k in range(1, 6)] + [cc.SPAN * k for k in range(1, 6)]
    # each situation really occurs
    for edge in edges:
        assert any(a < edge < b for a, b in ends), edge
    for edge in (cc.TILE, 2 * cc.TILE, 3 * cc.TILE, cc.SPAN, 2 * cc.SPAN):
        assert any(pos + 60 < edge < pos + 80 for _, _, pos, cigar, _, _, _ in rows if cigar[1:2] == [(cc.D, 20)]), edge
    assert sum(a < cc.TILE < b or a < 2 * cc.TILE < b or a < 3 * cc.TILE < b for a, b in cc.STRESS_TARGETS) >= 3
    assert any(a < 2 * cc.SPAN < b for a, b in cc.STRESS_TARGETS) and cc.STRESS_TARGETS[-1][1] > cc.LENGTH and cc.SPAN % cc.TILE
    assert sorted((flag & 0x10, len(bases)) for _, flag, _, _, bases, _, _ in rows if len(bases) == 700) == [(0, 700), (0x10, 700)]
    whole = s["whole"].tables["chr1"]
    assert whole["CYCLE"][0, 512, qc.BASES] == 2 * 188 + 988 and whole["LENGTH"][1500] == 1 and whole["LENGTH"][:1024].sum() == len(rows) - 1
    assert whole["DEPTH_HIST"][1023] >= 20 and whole["INSERT"][0, 4095] == 1 and whole["STATS"][qc.METRIC_STATS.index("positions_excluded")] == 40
    assert whole["QUALITY"][25, 0] >= 64 and (whole["QUALITY"][2:66, 0] >= 1).all() and whole["QUALITY"][2:66, 1].sum() > 0
    assert whole["TARGET_COVERED"].tolist()[-1] > 0 and (whole["TARGET_SUM"] > 0).all()
    # max_span 1 000 and unset: equal arrays, equal to the restatement; twice for equal bytes
    runs = [qc.measure(s["path"], s["genome"], ["chr1"], s["targets"], window=7, max_span=span) for span in (cc.SPAN, None, cc.SPAN, None)]
    for got in runs:
        same_tables(got.tables["chr1"], whole, ALL)
        same_bytes(got.tables["chr1"], runs[0].tables["chr1"])
    # window 1 000, straight from the rows: one span and six
    reads = cc.read_set(rows)
    want, counts = qc.restated([(reads, 0, cc.LENGTH)], reference, cc.STRESS_TARGETS, 1000)
    assert want["WINDOW_SUM"].shape == (6,) and whole["WINDOW_SUM"].shape == (858,) and want["WINDOW_SUM"].sum() == whole["WINDOW_SUM"].sum()
    cuts = [(lo, min(lo + cc.SPAN, cc.LENGTH)) for lo in range(0, cc.LENGTH, cc.SPAN)]
    for spans in ([(reads, 0, cc.LENGTH)], [(cc.read_set(cc.overlapping(rows, lo, hi)), lo, hi) for lo, hi in cuts]):
        got, stats = qc.metered(spans, reference, cc.STRESS_TARGETS, 1000)
        same_tables(got, want)
        assert {k: int(stats[k]) for k in qc.METRIC_STATS} == {k: counts[k] for k in qc.METRIC_STATS}
        assert all(stats[k] > 0 for k in ("reads_ms", "depth_ms", "pair_ms", "insert_ms"))


# ---- (4) the 6 kb paired chromosome ---------------------------------------------------------------------------------------------
def test_paired_chromosome_equals_the_restatement(tmp_path_factory):
    c = chromosome(tmp_path_factory)
    genome = {"chr1": c["reference"]}
    targets = {"chr1": [(500, 1500), (1500, 1600), (5900, 6000)]}
    want = qc.measure(c["path"], genome, targets=targets, restatement=True)
    stats: dict = {}
    for max_span in (None, 1000):
        got = qc.measure(c["path"], genome, targets=targets, max_span=max_span, stats=stats)
        same_tables(got.tables["chr1"], want.tables["chr1"], ALL)
        assert got.summary() == want.summary()
    assert stats["reads_ms"] > 0 and stats["decode_s"] > 0
    # INSERT counts exactly the pairs the join reports
    whole = c["whole"]
    is_measured = qc.measured(whole.flags)
    _, joined = join_mates(whole.name_hash, whole.flags, np.zeros(whole.n_reads, np.uint8), is_measured)
    table = want.tables["chr1"]
    pairs = int(table["STATS"][qc.METRIC_STATS.index("pairs")])
    assert pairs == joined["pairs"] == int(table["INSERT"].sum()) > 700 and table["INSERT"][0].sum() == pairs
    assert 300 <= want.summary()["insert_median"] <= 600


# ---- (5) the driver -------------------------------------------------------------------------------------------------------------
QC_FILES = ("qc.illumina.metrics.txt", "qc.illumina.tables.npz", "qc.illumina.windows.bedgraph", "qc.illumina.targets.tsv")
_driver: dict = {}


def _run(argv):
    return call.main(call.parser().parse_args(argv))


def _read(*parts):
    return open(os.path.join(*parts), "rb").read()


def driver_input(tmp_path_factory):
    if not _driver:
        from hello_amd import loader, netspec as ns, weights
        from tests.test_gpu_candidates import _fasta
        c = chromosome(tmp_path_factory)
        tmp = tmp_path_factory.mktemp("qc_driver")
        model = str(tmp / "m.hello.npz")
        loader.save_native(model, "single_tech", weights.synth_state(ns.build("single_tech"), seed=MODEL_SEED))
        bed = tmp / "targets.bed"
        bed.write_text("chr1\t1000\t1100\nchr1\t1100\t2100\nchr1\t5950\t6500\nchr2\t5\t9\n")
        _driver.update(tmp=tmp, bam=c["path"], bed=str(bed), genome={"chr1": c["reference"]},
                       tail=["--ibam", c["path"], "--ref", _fasta(tmp, "chr1", c["reference"]), "--network", model, "--from_bam"])
    return _driver


@pytest.mark.parametrize("resident", [False, True], ids=["shards", "resident"])
def test_the_driver_writes_the_files_of_the_restatement_and_leaves_the_vcf_alone(resident, tmp_path_factory):
    d = driver_input(tmp_path_factory)
    c = chromosome(tmp_path_factory)
    tail = d["tail"] + (["--resident"] if resident else [])
    work = {name: str(d["tmp"] / ("%s_%d" % (name, resident))) for name in ("qc", "plain", "marked", "want", "want_marked")}
    _run(["--workdir", work["qc"], "--qc", "--qc_regions", d["bed"], "--qc_window", "300"] + tail)
    _run(["--workdir", work["plain"]] + tail)
    assert _read(work["qc"], "results.output.vcf") == _read(work["plain"], "results.output.vcf")
    assert not [f for f in os.listdir(work["plain"]) if f.startswith("qc.")]
    targets = qc.read_bed(d["bed"])
    os.makedirs(work["want"])
    want = qc.measure(d["bam"], d["genome"], ["chr1"], targets, 300, restatement=True)
    want.write_all(os.path.join(work["want"], "qc.illumina"))
    for name in QC_FILES:
        assert _read(work["qc"], name) == _read(work["want"], name), name
    assert not os.path.exists(os.path.join(work["qc"], "qc.pacbio.metrics.txt"))
    # under --mark_duplicates the marked reads count as duplicates and leave the depth
    _run(["--workdir", work["marked"], "--mark_duplicates", "--qc", "--qc_window", "300"] + tail)
    metrics = dict(line.split("\t") for line in _read(work["marked"], "qc.illumina.metrics.txt").decode().splitlines())
    duplicates = dict(line.split("\t") for line in _read(work["marked"], "duplicates.metrics.txt").decode().splitlines())
    assert int(metrics["total.duplicate"]) == int(duplicates["total.duplicate_reads"]) == int(c["duplicate"].sum()) > 300
    assert not os.path.exists(os.path.join(work["marked"], "qc.illumina.targets.tsv"))
    with markdup.applied({d["bam"]: c["marks"]}):
        os.makedirs(work["want_marked"])
        qc.measure(d["bam"], d["genome"], ["chr1"], None, 300, restatement=True).write_all(os.path.join(work["want_marked"], "qc.illumina"))
    for name in QC_FILES[:3]:
        assert _read(work["marked"], name) == _read(work["want_marked"], name), name
    marked = qc.Metrics.load(os.path.join(work["marked"], "qc.illumina.tables.npz")).tables["chr1"]
    unmarked = want.tables["chr1"]
    assert not np.array_equal(marked["DEPTH_HIST"], unmarked["DEPTH_HIST"]) and marked["DEPTH_HIST"].sum() == unmarked["DEPTH_HIST"].sum()
    # the depth falls by exactly the duplicates' aligned positions, window for window
    whole = c["whole"]
    only = dataclasses.replace(whole, flags=np.where(c["duplicate"] > 0, whole.flags, 0x4).astype(np.uint16))
    lost = np.add.reduceat(qc.depth_of(only, 0, mc.LENGTH), np.arange(0, mc.LENGTH, 300))
    assert np.array_equal(unmarked["WINDOW_SUM"] - marked["WINDOW_SUM"], lost) and (lost > 0).sum() > 10
