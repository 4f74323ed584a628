"""Duplicate marking without a GPU (hello_amd/markdup.py): the plain-Python restatement against the tables
worked by hand (tests/markdup_cases.py), the marks (apply, save / load, the fetch hook), the spans, the refusals of
``call --mark_duplicates`` and the C ABI -- declarations, exports and the host-side validation, which needs no device."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from hello_amd import call, markdup
from hello_amd.bam import BamFile, Reads
from tests import markdup_cases as mc
from tests.bam_writer import write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = (("e", np.int64), ("score", np.int32), ("mate", np.int64), ("kind", np.uint8), ("duplicate", np.uint8))


def check_case(case, got, counts):
    """``got``: the five arrays; dtype and value equal the hand table."""
    for name, dtype in ARRAYS:
        assert got[name].dtype == dtype, name
        assert got[name].tolist() == getattr(case, name), name
    assert {k: int(counts[k]) for k in case.want_counts()} == case.want_counts()


@pytest.mark.parametrize("case", mc.HAND_TABLE, ids=[c.name for c in mc.HAND_TABLE])
def test_restatement_equals_the_hand_table(case):
    duplicate, details = markdup.duplicates_of(case.reads())
    assert duplicate is details["duplicate"] or np.array_equal(duplicate, details["duplicate"])
    check_case(case, details, details["counts"])


def test_the_parts_of_the_restatement():
    rd = mc.HAND_TABLE[3].reads()                                               # 7M2D3S, 10M and 7M3S, all reverse
    assert [markdup.end5_of(rd, r) for r in range(3)] == [111, 111, 109]
    assert markdup.eligible(np.array([0, 0x4, 0x100, 0x800, 0x400, 0x200, 0x63], np.uint16)).tolist() == [1, 0, 0, 0, 0, 1, 1]
    big = mc.read_set([(1, 0, 0, [(mc.M, 5)], [255] * 5)])
    assert markdup.score_of(big, 0) == 1275
    huge = dataclasses.replace(big, quals=np.full(5_000_000, 255, np.uint8), read_offsets=np.array([0, 5_000_000], np.int64))
    assert markdup.score_of(huge, 0) == 2 ** 30 - 1                             # 1 275 000 000 saturates
    assert markdup.kinds_of([0x63, 0x63, 0, 0x49, 0x400], [1, -1, -1, -1, -1], [1, 1, 1, 1, 0]).tolist() == [1, 3, 2, 2, 0]


def test_key_table_size_and_slot():
    assert [markdup.key_table_size(n) for n in (0, 1, 2, 3, 1000, 13312)] == [2, 2, 4, 8, 2048, 32768]
    ends = np.array([-6, 0, 1, 2 ** 40, 2 ** 62], np.int64)
    slots = markdup.key_table_slot(ends, 0, 0, 1 << 20)
    assert slots.dtype == np.uint32 and (slots < (1 << 20)).all() and len(set(slots.tolist())) == 5
    # an END entry and the PAIR entries that begin with its end start elsewhere; the order of lo and hi matters
    assert markdup.key_table_slot(200, 0, 0, 1 << 20) != markdup.key_table_slot(200, 0, 1, 1 << 20)
    assert markdup.key_table_slot(200, 619, 1, 1 << 20) != markdup.key_table_slot(619, 200, 1, 1 << 20)
    # every bit of either end reaches the slot
    for bit in (0, 1, 31, 32, 47, 62):
        assert markdup.key_table_slot(200 ^ (1 << bit), 619, 1, 1 << 20) != markdup.key_table_slot(200, 619, 1, 1 << 20), bit
        assert markdup.key_table_slot(200, 619 ^ (1 << bit), 1, 1 << 20) != markdup.key_table_slot(200, 619, 1, 1 << 20), bit


# ---- the marks ------------------------------------------------------------------------------------------------------------------
_made: dict = {}


def chromosome(tmp_path_factory):
    """The 6 kb BAM, what a whole-chromosome fetch gives, and the restatement's marks -- made once."""
    if not _made:
        tmp = tmp_path_factory.mktemp("markdup")
        reference, reads = mc.chromosome()
        path = str(tmp / "d.bam")
        write_bam(path, [("chr1", mc.LENGTH)], reads, index=True, block_bytes=20000)
        with BamFile(path) as b:
            whole = b.fetch("chr1")
        duplicate, details = markdup.duplicates_of(whole)
        _made.update(path=path, reference=reference, reads=reads, whole=whole, duplicate=duplicate, details=details,
                     marks=markdup.find_duplicates(path, restatement=True))
    return _made


def test_the_fixture_is_worth_something(tmp_path_factory):
    c = chromosome(tmp_path_factory)
    counts, kind, dup = c["details"]["counts"], c["details"]["kind"], c["duplicate"]
    assert counts["eligible"] == counts["reads"] == len(c["reads"]) and 0 < dup.sum() < counts["eligible"]
    assert counts["pairs"] > 700 and counts["duplicate_pairs"] > 150 and counts["singles"] == 45 and counts["duplicate_singles"] >= 16
    assert counts["unresolved"] == 0 and counts["groups_refused"] == 0
    # copies with a soft clip at a 5' end are found; every fragment keeps exactly one of its copies
    clipped = np.flatnonzero((c["whole"].cigars[c["whole"].cigar_offsets[:-1]] & 15) == mc.S)
    assert dup[clipped].sum() > 20
    kept = {}
    for r, read in enumerate(c["reads"]):
        if read.name.startswith("f"):
            kept.setdefault(read.name.split("_")[0], []).append(int(dup[r]))
    assert all(flags.count(0) == 2 for flags in kept.values()) and max(len(v) for v in kept.values()) == 12
    assert set(np.unique(kind).tolist()) == {1, 2}


def test_marks_equal_the_whole_chromosome_whatever_the_spans(tmp_path_factory):
    c = chromosome(tmp_path_factory)
    name, mates, start = c["marks"].identities["chr1"]
    which = np.flatnonzero(c["duplicate"])
    want = sorted(zip(c["whole"].name_hash[which].tolist(), (c["whole"].flags[which] & 0xC0).tolist(), c["whole"].ref_starts[which].tolist()))
    assert list(zip(name.tolist(), mates.tolist(), start.tolist())) == want and len(set(want)) == len(want)
    assert c["marks"].metrics["chr1"] == dict(c["details"]["counts"], duplicate_reads=len(want))
    small = markdup.find_duplicates(c["path"], ["chr1"], max_span=1000, restatement=True)
    for a, b in zip(small.identities["chr1"], c["marks"].identities["chr1"]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert small.metrics == c["marks"].metrics
    # mates lie in different spans of 1 000
    mate = c["details"]["mate"]
    paired = np.flatnonzero(mate >= 0)
    assert (c["whole"].ref_starts[paired] // 1000 != c["whole"].ref_starts[mate[paired]] // 1000).sum() >= 100
    with pytest.raises(ValueError, match="no sequence named"):
        markdup.find_duplicates(c["path"], ["chr9"], restatement=True)


def test_apply_and_the_round_trip_through_a_file(tmp_path, tmp_path_factory):
    c = chromosome(tmp_path_factory)
    path = c["marks"].save(str(tmp_path / "marks.npz"))
    loaded = markdup.Marks.load(path)
    assert list(loaded.identities) == ["chr1"] and loaded.metrics == c["marks"].metrics and loaded.total() == c["marks"].metrics["chr1"]
    for a, b in zip(loaded.identities["chr1"], c["marks"].identities["chr1"]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    for marks in (c["marks"], loaded):
        with BamFile(c["path"]) as b:
            rd = b.fetch("chr1", 1500, 4200)
        before = rd.flags.copy()
        assert marks.apply("chr1", rd) == int((rd.flags != before).sum()) > 0 and marks.apply("chr2", rd) == 0
        inside = (c["whole"].ref_ends > 1500) & (c["whole"].ref_starts < 4200)
        assert np.array_equal(rd.flags, before | (c["duplicate"][inside].astype(np.uint16) << 10))
    # all three fields must match
    one = markdup.Marks()
    one.set("chr1", [7, 7], [0x40, 0x80], [100, 300], dict.fromkeys(markdup.METRIC_NAMES, 0))
    rd = mc.read_set([(7, mc.F1, 100, mc.M10, mc.q()), (7, mc.R2, 100, mc.M10, mc.q()), (7, mc.R2, 300, mc.M10, mc.q()),
                      (8, mc.F1, 100, mc.M10, mc.q()), (7, mc.F1, 300, mc.M10, mc.q())])
    assert one.apply("chr1", rd) == 2 and (rd.flags & 0x400).tolist() == [0x400, 0, 0x400, 0, 0]
    metrics = c["marks"].write_metrics(str(tmp_path / "m.txt"))
    lines = open(metrics).read().splitlines()
    assert len(lines) == 2 * len(markdup.METRIC_NAMES) and all(re.fullmatch(r"(chr1|total)\.[a-z_]+\t\d+", x) for x in lines)
    assert "chr1.duplicate_reads\t%d" % c["duplicate"].sum() in lines and "total.pairs\t%d" % c["details"]["counts"]["pairs"] in lines


def test_fetch_applies_the_marks_inside_applied_and_only_there(tmp_path_factory):
    from hello_amd import bam
    c = chromosome(tmp_path_factory)
    fields = [f for f, _, _ in bam._ARRAYS]

    def fetch(path=c["path"]):
        with BamFile(path) as b:
            return b.fetch("chr1")
    before = c["whole"]
    assert not bam.MARKS
    with markdup.applied({c["path"]: c["marks"]}):
        assert list(bam.MARKS) == [os.path.abspath(c["path"])]
        inside = fetch()
        relative = fetch(os.path.relpath(c["path"]))                            # the registry knows the BAM by its absolute path
        other = str(tmp_path_factory.mktemp("other") / "e.bam")
        write_bam(other, [("chr1", mc.LENGTH)], c["reads"], index=True)
        untouched = fetch(other)                                                # another BAM with the same reads is left alone
    assert not bam.MARKS
    after = fetch()
    for f in fields:
        assert np.array_equal(getattr(after, f), getattr(before, f)), f
        assert np.array_equal(getattr(untouched, f), getattr(before, f)), f
        if f != "flags":
            assert np.array_equal(getattr(inside, f), getattr(before, f)), f
    want = before.flags | (c["duplicate"].astype(np.uint16) << 10)
    assert np.array_equal(inside.flags, want) and np.array_equal(relative.flags, want) and (want != before.flags).sum() > 300
    with pytest.raises(RuntimeError):                                           # the registry is emptied on every way out
        with markdup.applied({c["path"]: c["marks"]}):
            raise RuntimeError("x")
    assert not bam.MARKS


def test_every_stage_filter_drops_a_marked_read():
    """gvcf.usable / gvcf.counted are the Python statement of the filter every BAM-side stage applies (cigar.h: usable)."""
    from hello_amd import gvcf
    for flag in (0, 0x63, 0x93):
        assert gvcf.usable(flag, 60) and not gvcf.usable(flag | 0x400, 60)
        assert gvcf.counted(flag, 60, 10) and not gvcf.counted(flag | 0x400, 60, 10)
    text = open(os.path.join(ROOT, "hello_amd", "csrc", "cigar.h")).read()
    assert re.search(r"flag & \(0x4 \| 0x100 \| 0x800 \| 0x400\)\) return false", text)


# ---- the refusals and the flags -----------------------------------------------------------------------------------------------
def _args(*extra):
    return call.parser().parse_args(["--workdir", "w", "--network", "m.npz"] + list(extra))


def test_refusals_of_mark_duplicates_name_the_fix(monkeypatch):
    bam = ["--ibam", "x.bam", "--ref", "g.fa"]
    with pytest.raises(SystemExit, match="add --from_bam .*or --from_bams"):
        call.check_mark_duplicates(_args("--mark_duplicates", *bam))
    with pytest.raises(SystemExit, match="drop --shards"):
        call.check_mark_duplicates(_args("--mark_duplicates", "--from_bam", "--shards", "s", *bam))
    with pytest.raises(SystemExit, match="--gpus 1"):
        call.check_mark_duplicates(_args("--mark_duplicates", "--from_bam", "--gpus", "2", *bam))
    with pytest.raises(SystemExit, match="give the Illumina BAM as --ibam"):
        call.check_mark_duplicates(_args("--mark_duplicates", "--from_bam", "--pbam", "p.bam", "--ref", "g.fa"))
    with pytest.raises(SystemExit, match="--mark_duplicates"):
        call.main(_args("--mark_duplicates", "--shards", "s"))
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="plain command"):
        call.check_mark_duplicates(_args("--mark_duplicates", "--from_bam", *bam))
    monkeypatch.delenv("RANK")
    call.check_mark_duplicates(_args("--mark_duplicates", "--from_bam", *bam))
    call.check_mark_duplicates(_args("--mark_duplicates", "--from_bam", "--resident", *bam))
    call.check_mark_duplicates(_args("--mark_duplicates", "--from_bams", "--pbam", "p.bam", *bam))
    call.check_mark_duplicates(_args("--shards", "s"))
    assert _args("--shards", "s").mark_duplicates is False and "--mark_duplicates" in call._argv_of(_args("--mark_duplicates"))
    args = markdup.parser().parse_args(["--bam", "b.bam", "--output", "m.npz", "--chromosomes", "a,b", "--metrics", "f", "--device", "1"])
    assert (args.bam, args.output, args.chromosomes, args.metrics, args.device) == ("b.bam", "m.npz", "a,b", "f", 1)


def test_the_marks_are_computed_once_and_serve_both_passes_of_haplotag(monkeypatch, tmp_path):
    from hello_amd import bam
    marks = markdup.Marks()
    marks.set("chr1", [7], [0x40], [100], dict.fromkeys(markdup.METRIC_NAMES, 3))
    calls, seen = [], []
    monkeypatch.setattr(markdup, "find_duplicates", lambda path, chromosomes, **kw: calls.append((path, chromosomes)) or marks)

    def passes(args):                                                           # stands in for the two passes: what do they see?
        seen.append((args.mark_duplicates, args.haplotag, dict(bam.MARKS)))
        return "done"
    monkeypatch.setattr(call, "haplotag_passes", passes)
    work = str(tmp_path / "w")
    args = call.parser().parse_args(["--workdir", work, "--network", "m.npz", "--from_bam", "--ibam", "x.bam", "--ref", "g.fa",
                                     "--include_hp", "--haplotag", "--mark_duplicates", "--chromosomes", "chr1"])
    assert call.main(args) == "done"
    assert calls == [("x.bam", ("chr1",))] and seen == [(False, True, {os.path.abspath("x.bam"): marks})]
    assert not bam.MARKS and args.mark_duplicates is True                       # the caller's arguments are left as they were
    assert open(os.path.join(work, "duplicates.metrics.txt")).read().splitlines()[0] == "chr1.reads\t3"


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
SYMBOLS = ("hello_markdup_add", "hello_markdup_find", "hello_markdup_array", "hello_markdup_stats")


def test_abi_symbols_are_declared_exported_and_mirrored():
    from hello_amd.engine import load_library
    header = open(os.path.join(ROOT, "include", "hello_mi355x.h")).read()
    lib = load_library()
    for symbol in SYMBOLS:
        assert re.search(r"^int %s\(" % symbol, header, flags=re.M), symbol
        assert hasattr(lib, symbol), symbol
    assert re.search(r"^void hello_markdup_free\(", header, flags=re.M) and hasattr(lib, "hello_markdup_free")
    assert int(re.search(r"#define HELLO_MARKDUP_STATS (\d+)", header).group(1)) == len(markdup.STAT_NAMES) == 12
    for name in ("E", "SCORE", "MATE", "KIND"):
        assert int(re.search(r"HELLO_MARKDUP_%s = (\d+)" % name, header).group(1)) == getattr(markdup, name)
    assert int(re.search(r"HELLO_MARKDUP_DUPLICATE = (\d+)", header).group(1)) == markdup.DUP
    bound = markdup._lib()
    assert len(bound.hello_markdup_add.argtypes) == 14 and bound.hello_markdup_free.restype is None
    # one copy of the join: the pair kernels live in the header both stages include
    for name in ("phase.hip", "markdup.hip"):
        text = open(os.path.join(ROOT, "hello_amd", "csrc", name)).read()
        assert '#include "phase_pair.h"' in text and "pair_probe" not in text and "pair_insert_kernel" not in text, name


def test_the_host_walk_is_clean_under_sanitizers(tmp_path):
    """cigar.h: markdup_walk as a stand-alone host program under AddressSanitizer and UBSan (tests/abi/markdup_check.cpp)."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler on this box"
    exe = str(tmp_path / "markdup_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                            os.path.join(ROOT, "tests", "abi", "markdup_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "markdup_check: ok" in run.stdout, (run.returncode, run.stdout, run.stderr[-3000:])


def _add(lib, rd, handle):
    return lib.hello_markdup_add(*rd.pointers(rd.hp)[:10], None, rd.n_reads, 0, C.byref(handle))


def test_host_side_validation_needs_no_device():
    """What ``hello_markdup_add`` refuses, it refuses before it looks for a device: HELLO_ERR_ARG here, GPU or not."""
    lib = markdup._lib()
    error = lambda: lib.hello_last_error().decode()      # noqa: E731
    h = C.c_void_p()
    assert lib.hello_markdup_add(*([None] * 11), 0, 0, None) == -1 and "NULL pointer" in error()
    assert lib.hello_markdup_find(None) == -1 and "NULL pointer" in error()
    assert lib.hello_markdup_stats(None, (C.c_double * 12)()) == -1 and "NULL pointer" in error()
    good = mc.HAND_TABLE[0].reads()
    bad = Reads(**good.__dict__)
    bad.read_offsets = np.array([0, 10, 5], np.int64)
    assert _add(lib, bad, h) == -1 and "read 1: offsets decrease" in error()
    bad = Reads(**good.__dict__)
    bad.cigar_offsets = np.array([1, 2, 3], np.int64)
    assert _add(lib, bad, h) == -1 and "do not start at 0" in error()
    bad = Reads(**good.__dict__)
    bad.cigars = good.cigars.copy()
    bad.cigars[2] = (10 << 4) | 9
    assert _add(lib, bad, h) == -1 and "read 1: CIGAR operation 9" in error()
    bad = Reads(**good.__dict__)
    bad.cigars = good.cigars.copy()
    bad.cigars[2] = (11 << 4) | mc.M
    assert _add(lib, bad, h) == -1 and "read 1: CIGAR query length 11, 10 bases" in error()
    bad = Reads(**good.__dict__)
    bad.ref_ends = good.ref_ends + 1
    assert _add(lib, bad, h) == -1 and "read 0: ref_end does not match its CIGAR" in error()
    bad.flags = np.full(2, 0x400, np.uint16)                                    # a read that takes no part is not looked at
    assert _add(lib, bad, h) in (0, -5)                                         # HELLO_ERR_NOGPU where there is none
    if h:
        lib.hello_markdup_free(h)
