"""Duplicate marking on the GPU (hello_markdup_*; hello_amd/csrc/markdup.hip): ``e``, ``score``, ``mate``, ``kind``, ``duplicate`` and
the counts equal the restatement of hello_amd/markdup.py integer for integer -- on the tables worked by hand
(tests/markdup_cases.py), on a key-table stress whose probes collide and wrap at the table's end, on a 6 kb chromosome with mates
in different spans, and through the driver, where ``--mark_duplicates`` gives the files of a BAM that carries 0x400 itself."""
import dataclasses
import os

import numpy as np
import pytest

from hello_amd import call, markdup
from tests import markdup_cases as mc
from tests.bam_writer import write_bam
from tests.test_markdup import ARRAYS, check_case, chromosome

pytestmark = pytest.mark.gpu
MODEL_SEED = 1


def same(got, want):
    for name, dtype in ARRAYS:
        assert got[name].dtype == want[name].dtype == dtype and np.array_equal(got[name], want[name]), name


# ---- (1) the hand tables through the kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.HAND_TABLE, ids=[c.name for c in mc.HAND_TABLE])
def test_hand_table_through_the_kernels(case):
    rd = case.reads()
    got, stats = markdup.find_arrays(rd)
    check_case(case, got, stats)
    same(got, markdup.duplicates_of(rd)[1])
    if rd.n_reads:                                                              # in two spans: the same answer
        with markdup.Deduper() as d:
            half = rd.n_reads // 2
            keep = np.arange(rd.n_reads)
            for part in (keep[:half], keep[half:]):
                d.add(mc.read_set([case.rows[i] for i in part]))
            only_ends = d.arrays()
            d.find()
            same(d.arrays(), got)
            assert sorted(only_ends) == ["e", "score"] and np.array_equal(only_ends["e"], got["e"])


# ---- (2) the refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points():
    rd = mc.HAND_TABLE[5].reads()
    with markdup.Deduper() as d:
        d.add(rd)
        with pytest.raises(RuntimeError, match="offsets decrease"):
            d.add(dataclasses.replace(rd, read_offsets=np.array([0, 10, 20, 15, 40], np.int64)))
        with pytest.raises(RuntimeError, match="CIGAR query length"):
            d.add(dataclasses.replace(rd, cigars=rd.cigars + np.uint32(16)))
        d.find()
        assert d.stats()["reads"] == 4 and d.arrays()["duplicate"].tolist() == [0, 1, 0, 1]      # a refused add left nothing behind
        with pytest.raises(RuntimeError, match="called once"):
            d.find()
        with pytest.raises(RuntimeError, match="cannot be added after hello_markdup_find"):
            d.add(rd)
    with markdup.Deduper() as d:
        with pytest.raises(RuntimeError, match="NULL pointer"):
            d.find()
    with pytest.raises(RuntimeError, match="device 99"):
        markdup.find_arrays(rd, device=99)


# ---- (3) the key-table stress -----------------------------------------------------------------------------------------------------
def test_key_table_stress_collisions_and_a_probe_that_wraps():
    rows, size, wrapping = mc.stress(markdup.key_table_size, markdup.key_table_slot)
    rd = mc.read_set(rows)
    want, details = markdup.duplicates_of(rd)
    counts = details["counts"]
    assert (counts["pairs"], counts["singles"], counts["unresolved"]) == (4096, 1024, 0) and size == 32768
    assert counts["duplicate_pairs"] == 4096 - 512 and counts["duplicate_singles"] == 256 + (768 - 96)
    # the wrap and the collisions really occur: twelve END entries begin three slots before the end, and the entries' first
    # probes land on fewer slots than there are entries
    e, mate, kind = details["e"], details["mate"], details["kind"]
    ends = np.unique(e[kind > 0])
    first = np.flatnonzero((kind == 1) & (np.arange(rd.n_reads) < mate))
    lo, hi = np.minimum(e[first], e[mate[first]]), np.maximum(e[first], e[mate[first]])
    pair_keys = np.unique(np.stack([lo, hi], 1), axis=0)
    assert pair_keys.shape[0] == 512 and np.isin(2 * wrapping, ends).all()
    end_slots = markdup.key_table_slot(ends, 0, 0, size)
    assert (end_slots == size - 3).sum() >= 12
    slots = np.concatenate([end_slots, markdup.key_table_slot(pair_keys[:, 0], pair_keys[:, 1], 1, size)])
    assert np.unique(slots).shape[0] < slots.shape[0] and slots.shape[0] <= 3 * 4096 + 1024
    got, stats = markdup.find_arrays(rd)
    again, _ = markdup.find_arrays(rd)
    same(got, details)
    for name, _ in ARRAYS:
        assert got[name].tobytes() == again[name].tobytes(), name
    assert np.array_equal(got["duplicate"], want) and {k: int(stats[k]) for k in counts} == counts
    assert all(stats[k] > 0 for k in ("ends_ms", "pair_ms", "key_ms", "mark_ms"))


# ---- (4) the 6 kb chromosome ------------------------------------------------------------------------------------------------------
def identity_bytes(marks):
    return b"".join(a.tobytes() for a in marks.identities["chr1"])


def test_chromosome_equals_the_restatement_whatever_the_spans(tmp_path_factory):
    c = chromosome(tmp_path_factory)
    want = c["marks"]
    runs = []
    for max_span in (1000, None, 1000, None):
        stats = {}
        runs.append(markdup.find_duplicates(c["path"], ["chr1"], max_span=max_span, stats=stats))
        assert stats["ends_ms"] > 0 and stats["decode_s"] > 0
    for got in runs:
        assert identity_bytes(got) == identity_bytes(want) and got.metrics == want.metrics
        for a, b in zip(got.identities["chr1"], want.identities["chr1"]):
            assert a.dtype == b.dtype
    # worth something: mates in different spans of 1 000, and duplicates strictly between none and all
    whole, mate = c["whole"], c["details"]["mate"]
    paired = np.flatnonzero(mate >= 0)
    assert (whole.ref_starts[paired] // 1000 != whole.ref_starts[mate[paired]] // 1000).sum() >= 100
    total = want.total()
    assert 0 < total["duplicate_reads"] < total["eligible"] and total["duplicate_reads"] == 2 * total["duplicate_pairs"] + total["duplicate_singles"]
    # the whole chromosome in one add: every array, not only the marks
    got, _ = markdup.find_arrays(whole)
    same(got, c["details"])
    # the module's command line saves the same marks
    tmp = tmp_path_factory.mktemp("markdup_cli")
    saved = markdup.main(["--bam", c["path"], "--output", str(tmp / "m.npz"), "--metrics", str(tmp / "m.txt"), "--chromosomes", "chr1"])
    loaded = markdup.Marks.load(saved)
    assert identity_bytes(loaded) == identity_bytes(want) and loaded.metrics == want.metrics
    assert "total.duplicate_reads\t%d" % total["duplicate_reads"] in open(tmp / "m.txt").read().splitlines()


# ---- (5) the driver ---------------------------------------------------------------------------------------------------------------
OUTPUTS = ("results.output.vcf", "results.output.g.vcf", "results.output.phased.vcf")
_driver: dict = {}


def _run(argv):
    return call.main(call.parser().parse_args(argv))


def _read(*parts):
    return open(os.path.join(*parts), "rb").read()


def driver_input(tmp_path_factory):
    """The 6 kb BAM, the same reads with 0x400 in the file exactly where the restatement marks them, and the runs on both
    without ``--mark_duplicates`` (made once: both driver tests compare with them)."""
    if not _driver:
        from hello_amd import loader, netspec as ns, weights
        from tests.test_gpu_candidates import _fasta
        c = chromosome(tmp_path_factory)
        tmp = tmp_path_factory.mktemp("markdup_driver")
        marked = [dataclasses.replace(r, flag=r.flag | (0x400 if d else 0)) for r, d in zip(c["reads"], c["duplicate"].tolist())]
        path = str(tmp / "marked.bam")
        write_bam(path, [("chr1", mc.LENGTH)], marked, index=True, block_bytes=20000)
        model = str(tmp / "m.hello.npz")
        loader.save_native(model, "single_tech", weights.synth_state(ns.build("single_tech"), seed=MODEL_SEED))
        _driver.update(tmp=tmp, plain=c["path"], marked=path, tail=["--ref", _fasta(tmp, "chr1", c["reference"]), "--network", model,
                                                                      "--from_bam", "--annotate", "--gvcf", "--phase"])
    return _driver


def fields(vcf_bytes, name):
    """{(chromosome, position): the sample column's field ``name``} of the record lines."""
    out = {}
    for line in vcf_bytes.decode().splitlines():
        if not line.startswith("#"):
            f = line.split("\t")
            out[(f[0], int(f[1]))] = dict(zip(f[8].split(":"), f[9].split(":"))).get(name)
    return out


@pytest.mark.parametrize("resident", [False, True], ids=["shards", "resident"])
def test_the_driver_gives_the_files_of_a_marked_bam(resident, tmp_path_factory):
    d = driver_input(tmp_path_factory)
    tail = d["tail"] + (["--resident"] if resident else [])
    work = {name: str(d["tmp"] / ("%s_%d" % (name, resident))) for name in ("flag", "marked", "plain")}
    _run(["--ibam", d["plain"], "--workdir", work["flag"], "--mark_duplicates"] + tail)
    _run(["--ibam", d["marked"], "--workdir", work["marked"]] + tail)
    for name in OUTPUTS:
        assert _read(work["flag"], name) == _read(work["marked"], name), name
    assert not os.path.exists(os.path.join(work["marked"], "duplicates.metrics.txt"))
    metrics = dict(line.split("\t") for line in _read(work["flag"], "duplicates.metrics.txt").decode().splitlines())
    want = markdup.find_duplicates(d["plain"], restatement=True).total()
    assert {k: int(metrics["total." + k]) for k in want} == want and metrics["chr1.pairs"] == metrics["total.pairs"]
    if not resident:                                                            # without the flag the copies count
        _run(["--ibam", d["plain"], "--workdir", work["plain"]] + tail)
        assert not os.path.exists(os.path.join(work["plain"], "duplicates.metrics.txt"))
        for name in OUTPUTS:
            assert _read(work["plain"], name) != _read(work["flag"], name), name
        with_copies, without = fields(_read(work["plain"], OUTPUTS[0]), "AD"), fields(_read(work["flag"], OUTPUTS[0]), "AD")
        shared = [k for k in without if k in with_copies]
        assert shared and any(with_copies[k] != without[k] for k in shared)
        assert any(k[1] - 1 in mc.SITES for k in shared if with_copies[k] != without[k])         # at a planted heterozygous site
