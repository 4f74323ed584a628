"""CpG methylation without a GPU (hello_amd/methylation.py): the plain-Python restatement against the tables
worked by hand (tests/methylation_cases.py), the spans, the MM / ML parser through ``fetch_with_mods`` on written BAMs, the files'
exact text, the refusals of ``call --methylation`` and the C ABI -- declarations, exports and the host-side validation, which needs
no device."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hello_amd import call, methylation as me
from hello_amd.bam import BamFile, Mods
from tests import methylation_cases as mc
from tests.bam_writer import write_bam
from tests.test_stage_host import one_read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def same_tables(got, want):
    for name in ("SITES", "COUNTS"):
        assert got[name].dtype == np.int64 and got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name]), (name, np.argwhere(got[name] != want[name])[:5].tolist())


def spans_of(case, cuts):
    edges = [0] + list(cuts) + [len(case.reference)]
    return [mc.read_set(mc.overlapping(case.rows, lo, hi)) + (lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]


def same_mods(got: Mods, want: Mods):
    for f in dataclasses.fields(Mods):
        a, b = getattr(got, f.name), getattr(want, f.name)
        assert a.dtype == b.dtype and np.array_equal(a, b), f.name


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.HAND_TABLE, ids=[c.name for c in mc.HAND_TABLE])
def test_restatement_equals_the_hand_table(case):
    want = dict(SITES=np.array(case.sites, np.int64), COUNTS=case.expected())
    for cuts in ((), (case.cut(),)):                                            # whole, and cut through the middle of a read
        got, counts = me.restated(spans_of(case, cuts), case.reference)
        same_tables(got, want)
        assert {k: counts[k] for k in me.METRIC_STATS} == case.want_counts()
    assert counts["reads_given"] > len(case.rows)                              # the read that was cut is given twice


def test_the_hand_table_names_every_rule():
    names = " / ".join(c.name for c in mc.HAND_TABLE)
    for rule in ("forward and reverse", "a deletion, an insertion and a soft clip", "non-CpG position", "mismatching base",
                 "127 against 128", "mode '.', mode '?' and absent", "empty group", "C+mh and C+hm", "C+h before C+m", "G-m group",
                 "numeric code", "HP 0, 1, 2 and 3", "last two bases", "very last base", "bad-modification", "hard-clipped", "uncounted"):
        assert rule in names, rule
    assert len(mc.REF) == 200 and all(len(c.reference) == 200 for c in mc.HAND_TABLE)
    assert me.sites_of(mc.REF).tolist() == mc.SITES and me.sites_of("acgCgcG").tolist() == [1, 3, 5] and me.sites_of("C").tolist() == []


def test_the_parts_of_the_restatement():
    deltas, probs, mode, state = me.parse_mm(b"C+h,0,1;C+mh?,5,2;", [9, 9, 1, 2, 3, 4])
    assert (deltas.tolist(), probs.tolist(), mode, state) == ([5, 2], [1, 3], 1, me.USABLE) and deltas.dtype == np.int32
    assert me.parse_mm(None)[3] == me.NONE and me.parse_mm(b"")[3] == me.NONE and me.parse_mm(b"C+h,0;", [1])[3] == me.NONE
    assert me.parse_mm(b"C+m;", b"")[3] == me.USABLE and me.parse_mm(b"C+m;", None)[3] == me.BAD
    assert me.parse_mm(b"C+m,2147483647;", [1])[0].tolist() == [2147483647]
    for broken in (b"C+m,0", b"C+m", b"C", b"C+", b"C+;", b"C+,0;", b"X+m,0;", b"c+m,0;", b"C*m,0;", b"C+m,;", b"C+m,a;", b"C+m,-1;",
                   b"C+m,0,;", b"C+m,0;;", b";", b"C+m,0; ", b"C+M,0;", b"C+m!,0;", b"C+m.?,0;", b"C+m 0;", b"C+1m,0;", b"C+m1,0;",
                   b"C+m,0;C+", b"C+m,2147483648;", b"C+m,99999999999999999999999;", b"C+h,2147483648;C+m,0;", b"C+m,0;C+m,1;"):
        assert me.parse_mm(broken, [1])[3] == me.BAD, broken                       # the list of tests/abi/mods_check.cpp
    bases = np.frombuffer(b"ACCGTCG", np.uint8)
    assert me.listed(bases, False, [0, 1]).tolist() == [1, 5] and me.listed(bases, False, [3]) is None
    assert me.listed(bases, True, [0, 0]).tolist() == [6, 3] and me.listed(bases, True, [1, 0]) is None
    assert me.listed(bases, False, []).tolist() == [] and me.listed(np.frombuffer(b"AT", np.uint8), False, [0]) is None
    with pytest.raises(ValueError, match="does not consume exactly"):
        rd = one_read([(0, 5)], 4)
        me.tables_of(rd, Mods(np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(2, np.int64), np.zeros(1, np.uint8),
                              np.ones(1, np.uint8)), mc.REF, 0, 200)


# ---- the BAM reader -------------------------------------------------------------------------------------------------------------
_made: dict = {}


def stress_bam(tmp_path_factory):
    """The edge-stress chromosome as a BAM and a FASTA-like dictionary -- made once, for this file and tests/test_gpu_methylation.py."""
    if not _made:
        tmp = tmp_path_factory.mktemp("methylation")
        reference, rows = mc.stress()
        path = str(tmp / "s.bam")
        write_bam(path, [("chr1", mc.LENGTH)], mc.bam_records(rows), index=True, block_bytes=3000)
        _made.update(path=path, genome={"chr1": reference}, rows=rows, whole=me.measure(path, {"chr1": reference}, restatement=True))
    return _made


def test_fetch_with_mods_parses_what_the_restatement_parses(tmp_path):
    rows = sorted((r for c in mc.HAND_TABLE if c.reference == mc.REF for r in c.rows), key=lambda r: r.pos)
    assert len(rows) > 30 and sum(r.parsed()[3] == me.BAD for r in rows) >= 9
    for block_bytes in (65280, 211):                                            # 211: records lie across BGZF block edges
        path = str(tmp_path / ("hand%d.bam" % block_bytes))
        write_bam(path, [("chr1", 200)], mc.bam_records(rows), index=True, block_bytes=block_bytes)
        want_reads, want_mods = mc.read_set(rows)
        with BamFile(path) as bam:
            reads, mods = bam.fetch_with_mods("chr1")
            plain = bam.fetch("chr1")
            part_reads, part_mods = bam.fetch_with_mods("chr1", 40, 60)
        same_mods(mods, want_mods)
        assert reads.n_blocks >= (1 if block_bytes > 211 else 10)
        for f in dataclasses.fields(type(plain)):                               # a plain fetch is what it was, and so are the reads
            a, b = getattr(plain, f.name), getattr(reads, f.name)
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, f.name
        for name in ("bases", "read_offsets", "cigars", "cigar_offsets", "ref_starts", "ref_ends", "mapq", "flags", "hp"):
            assert np.array_equal(getattr(plain, name), getattr(want_reads, name)), name
        same_mods(part_mods, mc.read_set(mc.overlapping(rows, 40, 60))[1])
        assert part_reads.n_reads == len(mc.overlapping(rows, 40, 60)) > 0
    lib, p, n = me._lib(), C.c_void_p(), C.c_int64()                           # after a plain fetch the new arrays are empty
    with BamFile(path) as bam:
        r = C.c_void_p()
        assert lib.hello_bam_fetch(bam._h, b"chr1", 0, 200, -1, C.byref(r)) == 0
        for which, count in ((12, 0), (13, 0), (14, 1), (15, 0), (16, 0)):
            assert lib.hello_bam_reads_array(r, which, C.byref(p), C.byref(n)) == 0 and n.value == count
        assert lib.hello_bam_reads_array(r, 17, C.byref(p), C.byref(n)) == ERR_ARG
        lib.hello_bam_reads_free(r)


def test_the_stress_bam_round_trips_and_the_tables_do_not_depend_on_the_spans(tmp_path_factory):
    s = stress_bam(tmp_path_factory)
    with BamFile(s["path"]) as bam:
        reads, mods = bam.fetch_with_mods("chr1")
    want_reads, want_mods = mc.read_set(s["rows"])
    same_mods(mods, want_mods)
    assert np.array_equal(reads.hp, want_reads.hp) and np.array_equal(reads.bases, want_reads.bases)
    whole = s["whole"].tables["chr1"]
    small = me.measure(s["path"], s["genome"], ["chr1"], max_span=mc.SPAN, restatement=True).tables["chr1"]
    same_tables(small, whole)
    assert np.array_equal(small["STATS"], whole["STATS"])
    direct, counts = me.restated([(want_reads, want_mods, 0, mc.LENGTH)], s["genome"]["chr1"])      # without a BAM in between
    same_tables(whole, direct)
    assert whole["STATS"].tolist() == [counts[k] for k in me.METRIC_STATS]
    assert whole["COUNTS"][:, 1:].sum() > 0 and (whole["COUNTS"][:, 0] >= whole["COUNTS"][:, 1] + whole["COUNTS"][:, 2]).all()
    with pytest.raises(ValueError, match="no sequence named"):
        me.measure(s["path"], s["genome"], ["chr9"], restatement=True)
    with pytest.raises(ValueError, match="in the BAM header"):
        me.measure(s["path"], {"chr1": s["genome"]["chr1"][:-1]}, restatement=True)

    class Ones:                                                                 # a haplotagger's tags replace the BAM's own
        def retag(self, chromosome, rd):
            return dataclasses.replace(rd, hp=np.ones(rd.n_reads, np.uint8))
    tagged = me.measure(s["path"], s["genome"], haplotagger=Ones(), restatement=True).tables["chr1"]["COUNTS"]
    assert np.array_equal(tagged[:, 1], whole["COUNTS"][:, 0]) and not tagged[:, 2].any()


# ---- files ----------------------------------------------------------------------------------------------------------------------
def small_methylation():
    m = me.Methylation()
    counts = np.zeros((3, 3, 3), np.int64)
    counts[0] = [[3, 1, 700], [2, 0, 500], [1, 1, 200]]
    counts[2] = [[0, 2, 10], [0, 0, 0], [0, 2, 10]]
    m.set("chr1", dict(SITES=[10, 20, 198], COUNTS=counts), dict(dict.fromkeys(me.COUNT_NAMES, 0), counting=4, observations=6, n_sites=3))
    return m


def test_save_load_and_the_exact_text_of_the_files(tmp_path):
    m = small_methylation()
    files = m.write_bed(str(tmp_path / "methylation"))
    assert [os.path.basename(f) for f in files] == ["methylation.combined.bed", "methylation.hap1.bed", "methylation.hap2.bed"]
    head = "#chrom\tstart\tend\tpercent_modified\tcoverage\tmodified\tunmodified\tmean_probability\n"
    # (700 + 2) / 1024 = 0.68555; (10 + 1) / 512 = 0.02148; (500 + 1) / 512 = 0.97852; (200 + 1) / 512 = 0.39258
    assert open(files[0]).read() == head + "chr1\t10\t12\t75.0\t4\t3\t1\t0.6855\nchr1\t198\t200\t0.0\t2\t0\t2\t0.0215\n"
    assert open(files[1]).read() == head + "chr1\t10\t12\t100.0\t2\t2\t0\t0.9785\n"
    assert open(files[2]).read() == head + "chr1\t10\t12\t50.0\t2\t1\t1\t0.3926\nchr1\t198\t200\t0.0\t2\t0\t2\t0.0215\n"
    saved = m.save(str(tmp_path / "m.npz"))
    loaded = me.Methylation.load(saved)
    assert list(loaded.tables) == ["chr1"] and loaded.total() == m.total() and loaded.total()["observations"] == 6
    same_tables(loaded.tables["chr1"], m.tables["chr1"])
    assert open(loaded.save(str(tmp_path / "again.npz")), "rb").read() == open(saved, "rb").read()
    for a, b in zip(files, loaded.write_bed(str(tmp_path / "again"))):
        assert open(a, "rb").read() == open(b, "rb").read()


# ---- the refusals and the flags -------------------------------------------------------------------------------------------------
def _args(*extra):
    return call.parser().parse_args(["--workdir", "w", "--network", "m.npz"] + list(extra))


def test_refusals_of_methylation_name_the_fix(monkeypatch):
    bam = ["--pbam", "p.bam", "--ref", "g.fa"]
    with pytest.raises(SystemExit, match="add --from_bam .*or --from_bams"):
        call.check_methylation(_args("--methylation", *bam))
    with pytest.raises(SystemExit, match="drop --shards"):
        call.check_methylation(_args("--methylation", "--from_bam", "--shards", "s", *bam))
    with pytest.raises(SystemExit, match="--gpus 1"):
        call.check_methylation(_args("--methylation", "--from_bam", "--gpus", "2", *bam))
    with pytest.raises(SystemExit, match="give it as --pbam"):
        call.check_methylation(_args("--methylation", "--from_bam", "--ibam", "i.bam", "--ref", "g.fa"))
    with pytest.raises(SystemExit, match="--methylation"):
        call.main(_args("--methylation", "--shards", "s"))
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="plain command"):
        call.check_methylation(_args("--methylation", "--from_bam", *bam))
    monkeypatch.delenv("RANK")
    call.check_methylation(_args("--methylation", "--from_bam", *bam))
    call.check_methylation(_args("--methylation", "--from_bams", "--resident", "--ibam", "i.bam", *bam))
    call.check_methylation(_args("--shards", "s"))
    plain = _args("--shards", "s")
    assert plain.methylation is False and call.methylation_pass(plain, {}, "w/results.output.vcf") == []
    assert "--methylation" in call._argv_of(_args("--methylation")) and "--methylation" not in call._argv_of(plain)
    args = me.parser().parse_args(["--bam", "b.bam", "--ref", "g.fa", "--output_prefix", "p", "--phased_vcf", "v.vcf", "--chromosomes",
                                   "a,b", "--mapq_threshold", "3", "--device", "1"])
    assert (args.bam, args.ref, args.output_prefix, args.phased_vcf, args.chromosomes, args.mapq_threshold, args.device) == \
        ("b.bam", "g.fa", "p", "v.vcf", "a,b", 3, 1)


def test_methylation_is_cleared_for_pass_1_of_haplotag(monkeypatch):
    seen = []
    monkeypatch.setattr(call, "main", lambda args: seen.append(args) or os.path.join(args.workdir, "results.output.vcf"))
    args = _args("--from_bam", "--pbam", "p.bam", "--ref", "g.fa", "--include_hp", "--haplotag", "--methylation")
    call.haplotag_passes(args)
    first, second = seen
    assert (first.methylation, first.phase) == (False, True)
    assert (second.methylation, second.haplotag, second.haplotag_vcf) == (True, False, os.path.join("w", "haplotag_pass1", "results.output.phased.vcf"))
    assert args.methylation is True and args.haplotag is True                   # the caller's arguments are left as they were


def test_the_route_names_the_files_its_threshold_and_the_source_of_the_haplotypes(monkeypatch, tmp_path):
    from hello_amd import haplotag
    calls = []

    class Tagger:
        def __init__(self, vcf, chromosomes, q_threshold, mapq_threshold, device):
            self.vcf = vcf

        def close(self):
            calls.append("closed")

    def measure(bam, genome, chromosomes, haplotagger, mapq_threshold, **kw):
        calls.append((bam, tuple(chromosomes), getattr(haplotagger, "vcf", None), mapq_threshold))
        return small_methylation()
    monkeypatch.setattr(me, "measure", measure)
    monkeypatch.setattr(haplotag, "Haplotagger", Tagger)
    work = str(tmp_path / "w")
    os.makedirs(work)
    result = os.path.join(work, "results.output.vcf")
    tail = ["--workdir", work, "--network", "m.npz", "--ref", "g.fa", "--methylation", "--mapq_threshold", "3"]
    both = call.parser().parse_args(tail + ["--from_bams", "--ibam", "i.bam", "--pbam", "p.bam"])
    written = call.methylation_pass(both, {"chr1": "ACGT"}, result)
    assert calls == [("p.bam", ("chr1",), None, 3)]                             # the PacBio BAM, the HP tags, the route's threshold
    assert sorted(os.listdir(work)) == ["methylation.combined.bed", "methylation.hap1.bed", "methylation.hap2.bed", "methylation.npz"]
    assert [os.path.basename(f) for f in written] == ["methylation.combined.bed", "methylation.hap1.bed", "methylation.hap2.bed", "methylation.npz"]
    del calls[:]
    one = call.parser().parse_args(tail + ["--from_bam", "--pbam", "p.bam", "--phase", "--chromosomes", "chr1"])
    call.methylation_pass(one, {"chr1": "ACGT"}, result)
    assert calls == [("p.bam", ("chr1",), os.path.join(work, "results.output.phased.vcf"), 10), "closed"]      # --from_bam: the defaults
    del calls[:]
    given = call.parser().parse_args(tail + ["--from_bam", "--pbam", "p.bam", "--phase", "--include_hp", "--haplotag_vcf", "v.vcf"])
    call.methylation_pass(given, {"chr1": "ACGT"}, result)
    assert calls[0][2] == "v.vcf"                                               # --haplotag_vcf goes before --phase


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("hello_meth_create", "hello_meth_add", "hello_meth_array", "hello_meth_stats", "hello_bam_fetch_mods")


def test_abi_symbols_are_declared_exported_and_mirrored():
    from hello_amd.engine import load_library
    header = open(os.path.join(ROOT, "include", "hello_mi355x.h")).read()
    lib = load_library()
    for symbol in SYMBOLS:
        assert re.search(r"^int %s\(" % symbol, header, flags=re.M), symbol
        assert hasattr(lib, symbol), symbol
    assert re.search(r"^void hello_meth_free\(", header, flags=re.M) and hasattr(lib, "hello_meth_free")
    assert int(re.search(r"#define HELLO_METH_STATS (\d+)", header).group(1)) == len(me.STAT_NAMES) == 10
    for which, name in enumerate(("SITES", "COUNTS", "STATUS")):
        assert int(re.search(r"HELLO_METH_%s = (\d+)" % name, header).group(1)) == which
    for name, which in (("DELTAS", 12), ("PROBS", 13), ("OFFSETS", 14), ("MODE", 15), ("STATE", 16)):
        assert int(re.search(r"HELLO_BAM_MOD_%s = (\d+)" % name, header).group(1)) == which
    assert re.search(r"#define HELLO_ABI_VERSION 2\b", header)
    bound = me._lib()
    assert len(bound.hello_meth_add.argtypes) == 22 and bound.hello_meth_free.restype is None
    assert me.MAX_COUNTING_READS == 8421504
    makefile = open(os.path.join(ROOT, "hello_amd", "csrc", "Makefile")).read()
    assert " methylation.hip" in re.search(r"^SRCS = (.*)$", makefile, flags=re.M).group(1)
    text = open(os.path.join(ROOT, "hello_amd", "csrc", "mods.h")).read()      # the parser is plain C++: no HIP in it
    assert "hip/hip_runtime.h" not in text and "__global__" not in text


def test_the_host_code_is_clean_under_sanitizers(tmp_path):
    """mods.h and cigar.h: the MM / ML parser and the walks as a stand-alone host program under AddressSanitizer and UBSan
    (tests/abi/mods_check.cpp)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler on this box"
    exe = str(tmp_path / "mods_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                            os.path.join(ROOT, "tests", "abi", "mods_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "mods_check: ok" in run.stdout, (run.returncode, run.stdout, run.stderr[-3000:])


REFERENCE = np.frombuffer(b"ACGT" * 50, np.uint8)


def mods_for(n, deltas=(), state=1, mode=0):
    """Every read lists ``deltas``."""
    d = np.array(list(deltas) * n, np.int32)
    return Mods(d, np.full(d.shape[0], 9, np.uint8), np.arange(n + 1, dtype=np.int64) * len(deltas), np.full(n, mode, np.uint8),
                np.full(n, state, np.uint8))


def call_add(rd, mods=None, lo=0, hi=200, n_probs=None, handle=None):
    lib, h = me._lib(), handle or C.c_void_p()
    if not handle:
        assert lib.hello_meth_create(REFERENCE.ctypes.data, 200, 10, 0, C.byref(h)) == 0      # needs no device
    mods = mods or mods_for(rd.n_reads)
    rc = lib.hello_meth_add(h, *rd.pointers(rd.hp), rd.n_reads, mods.deltas.ctypes.data, mods.deltas.shape[0], mods.probs.ctypes.data,
                            mods.probs.shape[0] if n_probs is None else n_probs, mods.offsets.ctypes.data, mods.mode.ctypes.data,
                            mods.state.ctypes.data, lo, hi)
    said = lib.hello_last_error().decode()
    if not handle:
        lib.hello_meth_free(h)
    return rc, said


def two_reads():
    from tests.qc_cases import M4, read_set
    return read_set([(1, 0, 10, M4, "ACGT", [30] * 4, 60), (2, 0, 12, M4, "ACGT", [30] * 4, 60)])


# (what is wrong, the message): every one is HELLO_ERR_ARG, before the device is looked for
REFUSALS = [
    (dict(read=dict(cigar=[(0, 5)], n_bases=4)), "read 0: CIGAR query length 5, 4 bases"),
    (dict(read=dict(cigar=[(0, 5)], n_bases=6)), "read 0: CIGAR query length 5, 6 bases"),
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
    (dict(mods=dict(offsets=np.array([1, 1, 2], np.int64))), "modification offsets do not start at 0"),
    (dict(mods=dict(offsets=np.array([0, 2, 1], np.int64))), "read 1: modification offsets decrease"),
    (dict(mods=dict(offsets=np.array([0, 1, 1], np.int64))), "modification offsets end at 1, 2 deltas"),
    (dict(n_probs=1), "1 probabilities for 2 deltas"),
    (dict(mods=dict(deltas=np.array([0, -1], np.int32))), "read 1: delta -1"),
    (dict(mods=dict(state=np.array([1, 3], np.uint8))), "read 1: modification state 3"),
    (dict(mods=dict(mode=np.array([2, 0], np.uint8))), "read 0: modification mode 2"),
]


@pytest.mark.parametrize("wrong,message", REFUSALS, ids=[r[1][:34].strip() + ("-%d" % i) for i, r in enumerate(REFUSALS)])
def test_add_refuses_before_it_looks_for_a_device(wrong, message):
    wrong = dict(wrong)
    rd = one_read(**wrong.pop("read")) if "read" in wrong else dataclasses.replace(two_reads(), **wrong.pop("change", {}))
    mods = dataclasses.replace(mods_for(rd.n_reads, (0,)), **wrong.pop("mods", {}))
    assert call_add(rd, mods, **wrong) == (ERR_ARG, message)


def test_host_side_validation_needs_no_device():
    lib = me._lib()
    error = lambda: lib.hello_last_error().decode()      # noqa: E731
    h = C.c_void_p()
    assert lib.hello_meth_create(None, 0, 10, 0, C.byref(h)) == ERR_ARG and "NULL pointer" in error()
    assert lib.hello_meth_create(REFERENCE.ctypes.data, -1, 10, 0, C.byref(h)) == ERR_ARG and "reference of -1 bases" in error()
    assert lib.hello_meth_create(REFERENCE.ctypes.data, 1 << 31, 10, 0, C.byref(h)) == ERR_ARG and not h.value
    assert lib.hello_meth_add(None, *([None] * 11), 0, None, 0, None, 0, None, None, None, 0, 0) == ERR_ARG and "NULL pointer" in error()
    assert lib.hello_meth_stats(None, (C.c_double * 10)()) == ERR_ARG and "NULL pointer" in error()
    p, n = C.c_void_p(), C.c_int64()
    assert lib.hello_meth_array(None, 0, C.byref(p), C.byref(n)) == ERR_ARG and "NULL pointer" in error()
    # a read that is not counted is not looked at: what the call answers then needs a device or needs none
    rc, said = call_add(one_read([(0, 5)], 4, flag=0x200))
    assert rc in (0, -5) and "read 0" not in said
    # a refused add leaves the handle where it was: the next span may still begin at 0
    assert lib.hello_meth_create(REFERENCE.ctypes.data, 200, 10, 0, C.byref(h)) == 0
    assert call_add(two_reads(), mods_for(2, (0,), state=3), handle=h) == (ERR_ARG, "read 0: modification state 3")
    assert call_add(two_reads(), lo=0, hi=300, handle=h)[0] == ERR_ARG
    st = (C.c_double * 10)()
    assert lib.hello_meth_stats(h, st) == 0 and list(st) == [0.0] * 10
    assert lib.hello_meth_array(h, 2, C.byref(p), C.byref(n)) == 0 and n.value == 0       # STATUS: no add yet
    assert lib.hello_meth_array(h, 3, C.byref(p), C.byref(n)) == ERR_ARG and "array selector 3" in error()
    lib.hello_meth_free(h)
