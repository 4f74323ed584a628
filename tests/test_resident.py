"""Resident candidate sites, host side (no GPU): the three library entry points and the gather table exist and refuse what
include/hello_mi355x.h says they refuse; the gather table equals what ``PackedShard.featurizer_core`` derives from the same
counts; ``python -m hello_amd.call --resident`` parses and names its refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from hello_amd import call, candidates as cd, hybrid, resident as rs, shards
from hello_amd.bam import Reads
from hello_amd.engine import load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "ACGT" * 200


def no_reads() -> Reads:
    z = lambda dtype, n=0: np.zeros(n, dtype)      # noqa: E731
    return Reads(z(np.uint8), z(np.uint8), z(np.int64, 1), z(np.uint32), z(np.int64, 1), z(np.int64), z(np.int64), z(np.uint8),
                 z(np.uint16), z(np.uint64), z(np.uint8), z(np.uint8))


def test_the_new_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "hello_mi355x.h")).read()
    lib = load_library()
    for name in ("hello_candidates_featurizer_counts", "hello_candidates_gather", "hello_candidates_gather_table"):
        assert f"int {name}(" in header, name
        assert getattr(lib, name) is not None
    assert f"#define HELLO_CANDIDATES_RESIDENT {rs.HELLO_CANDIDATES_RESIDENT}" in header
    from hello_amd import hotspots as hs
    assert rs.HELLO_CANDIDATES_RESIDENT not in (hs.HOTSPOTS_PACBIO, hs.HOTSPOTS_HYBRID, hs.HOTSPOTS_TWO_BAMS)
    assert rs.HELLO_CANDIDATES_RESIDENT & (hs.HOTSPOTS_PACBIO | hs.HOTSPOTS_HYBRID | hs.HOTSPOTS_TWO_BAMS) == 0


def _find_handle(options):
    """hello_candidates_find over zero reads (no GPU needed) -> the raw handle."""
    cd._lib()
    lib = rs._lib()
    r = no_reads()
    ref = np.frombuffer(REFERENCE.encode(), np.uint8)
    pos = np.array([300, 301], np.int64)
    h = C.c_void_p()
    p = lambda a: a.ctypes.data      # noqa: E731
    rc = lib.hello_candidates_find(p(r.bases), p(r.quals), p(r.read_offsets), p(r.cigars), p(r.cigar_offsets), p(r.ref_starts),
                                   p(r.ref_ends), p(r.mapq), p(r.flags), p(r.name_hash), p(r.hp), 0, p(ref), ref.shape[0], p(pos), 2,
                                   options, 150, 10, 10, 0, C.byref(h))
    assert rc == 0, lib.hello_last_error()
    return lib, h


def test_gather_refuses_candidates_that_are_not_resident():
    lib, h = _find_handle(0)
    try:
        rc = lib.hello_candidates_gather(h, 0, *([None] * 10), 0, 0, 0, 0, None)
        assert rc == -1
        assert b"HELLO_CANDIDATES_RESIDENT" in lib.hello_last_error()
        n = [C.c_int64(7), C.c_int64(7), C.c_int64(7)]
        assert lib.hello_candidates_featurizer_counts(h, 0, *[C.byref(x) for x in n]) == 0       # valid for both kinds
        assert [x.value for x in n] == [0, 0, 0]
    finally:
        lib.hello_candidates_free(h)


def test_resident_candidates_without_reads_hold_nothing_and_gather_nothing():
    lib, h = _find_handle(rs.HELLO_CANDIDATES_RESIDENT)
    try:
        n = [C.c_int64(7), C.c_int64(7), C.c_int64(7)]
        assert lib.hello_candidates_featurizer_counts(h, 0, *[C.byref(x) for x in n]) == 0
        assert [x.value for x in n] == [0, 0, 0]
        assert lib.hello_candidates_gather(h, 0, *([None] * 10), 0, 0, 0, 0, None) == 0          # n_reads == 0: nothing launched
        assert lib.hello_candidates_gather(h, 0, *([None] * 10), 0, -1, 0, 0, None) == -1
        assert b"shift" in lib.hello_last_error()
        assert lib.hello_candidates_gather(h, 1, *([None] * 10), 0, 0, 0, 0, None) == -1         # one technology only
        assert b"technology 1" in lib.hello_last_error()
        assert lib.hello_candidates_featurizer_counts(h, 1, *[C.byref(x) for x in n]) == -1
    finally:
        lib.hello_candidates_free(h)


def test_find_sites_resident_without_reads_is_a_closed_book():
    shard, st, extra = cd.find_sites(no_reads(), REFERENCE, [300, 301], resident=True)
    with shard:
        assert isinstance(shard, rs.ResidentShard) and shard.n_sites == 0 and shard.n_alleles == 0 and not shard.hybrid
        assert shard.n_reads(0) == 0 and shard.featurizer_counts(0) == (0, 0, 0) and shard.reads_per_allele(0).shape == (0,)
        assert st["gather_ms"] == 0 and st["active_regions"] == 1
        assert extra["read_off0"].tolist() == [0] and extra["cigar_off0"].tolist() == [0]
        with pytest.raises(ValueError, match="without resident=True"):
            cd.write_packed("/nonexistent/x.hshard", shard)
    assert shard.handle is None
    shard.close()                                                                              # closing twice is harmless
    with pytest.raises(ValueError, match="closed"):
        shard.gather(0, {k: 0 for k in rs.GATHER_ARRAYS})
    plain, st0, _ = cd.find_sites(no_reads(), REFERENCE, [300, 301])
    assert isinstance(plain, shards.PackedShard)
    assert {k: v for k, v in st.items() if not k.endswith("_ms")} == {k: v for k, v in st0.items() if not k.endswith("_ms")}
    both, st2, extra2 = hybrid.find_sites(no_reads(), no_reads(), REFERENCE, [300], resident=True)
    with both:
        assert both.hybrid and both.has_reads(1) and both.n_reads(1) == 0 and extra2["read_off1"].tolist() == [0]


def test_resident_activity_yields_a_shard_per_chromosome(tmp_path):
    """An activity file over two chromosomes becomes two resident shards in file order, each naming the file (BAMs without
    reads: nothing here needs a GPU)."""
    from tests.bam_writer import write_bam
    bam, fa, activity = str(tmp_path / "e.bam"), str(tmp_path / "g.fa"), str(tmp_path / "shard0.txt")
    write_bam(bam, [("chr1", len(REFERENCE)), ("chr2", len(REFERENCE))], [], index=True)
    with open(fa, "w") as fh:
        fh.write(f">chr1\n{REFERENCE}\n>chr2\n{REFERENCE}\n")
    with open(activity, "w") as fh:
        fh.write("".join(str({"chromosome": c, "position": p}) + "\n" for c, p in (("chr2", 300), ("chr2", 301), ("chr1", 420))))
    total: dict = {}
    found = list(cd.resident_activity(bam, fa, activity, total=total))
    try:
        assert [type(sh) for sh in found] == [rs.ResidentShard] * 2 and [sh.path for sh in found] == [activity] * 2
        assert [sh.n_sites for sh in found] == [0, 0] and total["active_regions"] == 2 and total["gather_ms"] == 0
    finally:
        for sh in found:
            sh.close()
    both = list(cd.resident_activity([bam, bam], fa, activity, find=hybrid.find_hybrid_candidates, reassembly_size=4))
    assert [sh.hybrid for sh in both] == [True, True]
    with pytest.raises(ValueError, match="no sequence named"):
        list(cd.resident_activity(bam, fa, activity, genome={"chr2": REFERENCE}))


def _packed(counts, rng):
    """A shard of one site per allele group with the given reads_per_allele0 and random read and CIGAR lengths."""
    counts = np.asarray(counts, np.int32)
    R, A = int(counts.sum()), counts.shape[0]
    lengths = rng.integers(1, 40, R)
    ops = rng.integers(1, 4, R)
    cigars = np.concatenate([np.array([(int(n - k + 1) << 4) | 0] + [(1 << 4) | 0] * int(k - 1), np.uint32) if k <= n else
                             np.array([(int(n) << 4) | 0] + [(1 << 4) | 2] * int(k - 1), np.uint32)
                             for n, k in zip(lengths, ops)] + [np.zeros(0, np.uint32)])
    arrays = dict(
        chromosome_text=np.frombuffer(b"c", np.uint8), chromosome_text_off=np.array([0, 1], np.int64) if A else np.array([0], np.int64),
        chromosome_of_site=np.zeros(1 if A else 0, np.int32), start=np.full(1 if A else 0, 300, np.int64),
        stop=np.full(1 if A else 0, 301, np.int64), window_start=np.full(1 if A else 0, 200, np.int64),
        ref=np.frombuffer((REFERENCE[:300] if A else "").encode(), np.uint8), ref_off=np.array([0, 300] if A else [0], np.int64),
        alleles_per_site=np.array([A] if A else [], np.int32), allele_text=np.frombuffer(b"A" * A, np.uint8),
        allele_text_off=np.arange(A + 1, dtype=np.int64), has_second=np.array(0),
        reads_per_allele0=counts, bases0=np.full(int(lengths.sum()), 65, np.uint8), quals0=np.full(int(lengths.sum()), 30, np.uint8),
        read_off0=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), cigars0=cigars,
        cigar_off0=np.concatenate([[0], np.cumsum(ops)]).astype(np.int64), ref_start0=np.full(R, 250, np.int64),
        mapq0=np.full(R, 60, np.uint8), orientation0=np.ones(R, np.int8), hp0=np.zeros(R, np.uint8))
    if not A:
        arrays["chromosome_text"] = np.zeros(0, np.uint8)
    return shards.PackedShard(arrays)


@pytest.mark.parametrize("counts", [[0], [0, 0, 3], [2, 0, 1], [1, 4, 2, 1], [], [3], [0, 0], [5, 0, 0, 1, 0]])
def test_the_gather_table_is_what_featurizer_core_derives(counts):
    rng = np.random.default_rng(len(counts) + sum(counts))
    shard = _packed(counts, rng)
    core = shard.featurizer_core(0)
    z = shard.z
    table = rs.gather_table(counts, z["read_off0"], z["cigar_off0"])
    n = int(np.maximum(np.asarray(counts, np.int64), 1).sum()) if counts else 0
    assert table["source"].shape == (n,) and n == int(core["site_of_read"].shape[0])
    # featurizer_core's own source index: the dummy reads are where an allele has no read
    want = []
    at = 0
    for c in counts:
        want += list(range(at, at + c)) if c else [-1]
        at += c
    assert table["source"].tolist() == want
    assert np.array_equal(table["read_off"], np.asarray(core["read_off"], np.int64))
    assert np.array_equal(table["cigar_off"], np.asarray(core["cigar_off"], np.int64))
    real = table["source"] >= 0
    for name, default in (("ref_start", 0), ("mapq", 40), ("orientation", 1), ("hp", 0)):          # the dummy's defaults
        col = np.asarray(z[f"{name}0"])
        picked = np.where(real, col[np.where(real, table["source"], 0)] if col.shape[0] else default, default)
        assert np.array_equal(picked, core[name]), name
    assert core["reads_per_allele"].tolist() == [max(c, 1) for c in counts]


def test_the_gather_table_refuses_inconsistent_input():
    with pytest.raises(ValueError, match="offsets"):
        rs.gather_table([2], [0, 5], [0, 1, 2])
    with pytest.raises(ValueError, match="negative"):
        rs.gather_table([-1], [0], [0])


def _args(*argv):
    return call.parser().parse_args(["--workdir", "w", "--network", "n"] + list(argv))


def test_resident_parses_with_both_bam_routes():
    assert _args("--from_bam", "--resident", "--ibam", "i.bam", "--ref", "g.fa").resident
    assert _args("--from_bams", "--resident", "--ibam", "i.bam", "--pbam", "p.bam", "--ref", "g.fa").resident
    assert not _args("--from_bam").resident
    call.check_resident(_args("--from_bam", "--resident"))
    call.check_resident(_args("--from_bams", "--resident"))
    call.check_resident(_args("--shards", "x", "--gpus", "4"))                    # without --resident nothing is refused here


def test_resident_refusals_name_the_fix(monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for argv, message in ((["--resident"], "add --from_bam"),
                          (["--resident", "--shards", "x"], "add --from_bam"),
                          (["--resident", "--from_bam", "--shards", "x"], "drop --shards"),
                          (["--resident", "--from_bams", "--shards", "x"], "drop --shards"),
                          (["--resident", "--from_bam", "--gpus", "2"], "--gpus 1"),
                          (["--resident", "--from_bams", "--gpus", "8"], "--gpus 1"),
                          (["--resident", "--from_bam", "--from_bams"], "exclude each other")):
        for entry in (call.check_resident, call.main):
            with pytest.raises(SystemExit, match=message):
                entry(_args(*argv))
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="plain command"):
        call.main(_args("--resident", "--from_bam"))


def test_a_launch_does_not_mix_file_and_resident_shards():
    """The scorer's refusal is decided before anything touches the GPU."""
    from hello_amd import shard_pipeline as sp
    plain = _packed([1, 2], np.random.default_rng(1))
    res = object.__new__(rs.ResidentShard)
    res.n_sites, res.handle = 1, None
    scorer = object.__new__(sp.ShardScorer)
    scorer.slots, scorer.count = [sp._Slot(), sp._Slot()], 0
    with pytest.raises(ValueError, match="not both"):
        scorer.submit([plain, res])
