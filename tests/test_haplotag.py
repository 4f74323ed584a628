"""The haplotag rule of DESIGN.md section 7h, on the CPU: the parser and the restatement of hello_amd/haplotag.py against the tables
worked by hand (tests/haplotag_cases.py), the equivalence with the phasing of section 7g (phase with its restatement, write the
phased lines, read them back: every read gets the hp and ps ``phase.haplotags_of`` gives it), the refusals of
``call --haplotag_vcf`` / ``--haplotag``, and the new symbols of the C ABI.  The GPU is held to the restatement in
tests/test_gpu_haplotag.py."""
import ctypes as C
import logging
import os
import re

import numpy as np
import pytest

from hello_amd import call, haplotag as ht, phase
from tests import haplotag_cases as hc, phase_cases as pc
from tests.gvcf_cases import reads_of_bam_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (1) the parser -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, line, want, without_ps", hc.PARSER_TABLE, ids=[c[0] for c in hc.PARSER_TABLE])
def test_parser_by_hand(name, line, want, without_ps):
    assert ht.phased(line) == want
    assert ht._parse(line) == (want, without_ps)
    if want is not None:
        assert isinstance(want.ps, int) and want.ps > 0 and want.pos == want.start + 1


def test_phased_records_per_chromosome_sorted_counted_and_warned_once(tmp_path, caplog):
    lines = [b"##fileformat=VCFv4.1\n", b"#CHROM\tPOS\n",
             hc.line(5, "G", "T", "GT:PS", "0|1:5", "chrB"), hc.line(9, "A", "C", "GT", "0|1", "chrB"),
             hc.line(9, "A", "C", "GT:PS", "1|0:5", "chrB"), hc.line(3, "A", "G", "GT:PS", "0|1:3", "chrA"),
             hc.line(12, "A", "G", "GT", "0/1", "chrB"), hc.line(14, "A", "G", "GT:PS", "0|1:.", "chrB")]
    path = str(tmp_path / "p.vcf")
    open(path, "wb").write(b"".join(lines))
    stats = {}
    with caplog.at_level(logging.WARNING, logger="hello_amd.haplotag"):
        got = ht.phased_records(path, stats=stats)
    assert list(got) == ["chrB", "chrA"] and got["chrB"] == [hc.rec(4, "G", "G", "T", 5), hc.rec(8, "A", "C", "A", 5, 1, 0)]
    assert got["chrA"] == [hc.rec(2, "A", "A", "G", 3)] and stats == {"lines_without_ps": 2, "phased_records": 3}
    assert len([r for r in caplog.records if "without a positive PS" in r.getMessage()]) == 1
    assert list(ht.phased_records(path, ["chrA"])) == ["chrA"]
    open(path, "ab").write(hc.line(7, "A", "C", "GT:PS", "0|1:5", "chrB"))                         # POS 7 behind POS 9
    with pytest.raises(ValueError, match="not sorted"):
        ht.phased_records(path)
    assert ht.phased_records(path, ["chrA"])["chrA"] == got["chrA"]                              # another chromosome's order is not its business


# ---- (2) the reads worked by hand ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hc.READ_TABLE, ids=[c.name for c in hc.READ_TABLE])
def test_restatement_by_hand(case):
    reads = pc.reads_of(case.reads)
    hp, ps = ht.haplotags_restated(reads, case.records)
    assert hp.dtype == np.uint8 and ps.dtype == np.int64
    assert list(zip(hp.tolist(), ps.tolist())) == case.want
    for r, why in enumerate(case.why):                                                           # the first candidate shows nothing, and why
        first = min(t for t, rec in enumerate(case.records) if rec.start >= int(reads.ref_starts[r]))
        assert phase.observe_why(reads, r, case.records[first]) == (phase.NONE, why), r


def test_rounds_case_by_hand():
    records = hc.rounds_records()
    reads, want = hc.rounds_reads()
    rd = pc.reads_of(reads)
    hp, ps = ht.haplotags_restated(rd, records)
    assert list(zip(hp.tolist(), ps.tolist())) == want
    seen = [phase.observe(rd, 0, rec) for rec in records]
    assert len(records) == 140 and all(o < 0 for o in seen[:hc.FIRST_SEEN]) and seen[hc.FIRST_SEEN] == 0      # round 1 shows nothing
    assert records[126].ps == records[128].ps == hc.SET_X and records[127].ps == hc.SET_Y         # X straddles the rounds, interleaved
    assert {1, 2} <= set(hp.tolist())


def test_the_restatement_refuses_what_the_library_refuses():
    beyond = pc.reads_of([(0, [(pc.M, 9)], "ACGTGCAT", [30] * 8, 0, 60)])
    with pytest.raises(ValueError, match="consumes more bases"):
        ht.haplotags_restated(beyond, [hc.G_T])
    fine = pc.reads_of([(0, [(pc.M, 8)], "ACGTGCAT", [30] * 8, 0, 60)])
    with pytest.raises(ValueError, match="not sorted"):
        ht.haplotags_restated(fine, [hc.rec(6, "A", "A", "C", 5), hc.G_T])
    with pytest.raises(ValueError, match="not sorted"):
        ht.Haplotagger(None, records={"chr1": [hc.rec(6, "A", "A", "C", 5), hc.G_T]})


# ---- (3) equivalence with section 7g ------------------------------------------------------------------------------------------
def phased_lines_of(lines, records, flip, set_pos):
    """The lines of ``write_phased_vcf``: those of the records in a set of two or more rewritten by ``phase.phased_line``."""
    out, t = [], 0
    for line in lines:
        rec = phase.phasable(line)
        if rec is None:
            out.append(line)
            continue
        assert rec == records[t]
        out.append(phase.phased_line(line, rec, int(flip[t]), int(set_pos[t])) if set_pos[t] else line)
        t += 1
    return out


def test_haplotags_from_the_phased_file_equal_those_of_the_phasing_that_wrote_it():
    """Every read of both sources (all of them: the restatements take well under a second here)."""
    _, lines, short, long = pc.synthetic(1)
    records = [r for r in map(phase.phasable, lines) if r]
    sets = [reads_of_bam_records(short), reads_of_bam_records(long)]
    slots, offsets, first = phase.slots_of(sets, records)
    chained, flip = phase.chain(phase.links_of(slots, offsets, first, len(records), pc.WINDOW), pc.WINDOW, 2)
    positions = [r.pos for r in records]
    want_hp, want_ps = phase.haplotags_of(slots, offsets, first, chained, flip, positions)
    back = [r for r in map(ht.phased, phased_lines_of(lines, records, flip, phase.set_positions(chained, positions))) if r]
    hp, ps = ht.haplotags_restated(sets, back)
    assert hp.dtype == want_hp.dtype and ps.dtype == want_ps.dtype
    assert np.array_equal(hp, want_hp) and np.array_equal(ps, want_ps)
    # what makes this worth something: every tag occurs, a record came back flipped, sets differ, a read has more than one round
    assert set(hp.tolist()) == {0, 1, 2} and flip.any() and len(set(r.ps for r in back)) >= 2
    assert any(r.a > r.b for r in back) and 2 <= len(back) < len(records)
    assert np.diff(offsets).max() > 64
    for source in (0, 1):                                                                        # per read: each source alone
        lo = 0 if source == 0 else sets[0].n_reads
        alone = ht.haplotags_restated(sets[source], back)
        assert np.array_equal(alone[0], hp[lo:lo + sets[source].n_reads]) and np.array_equal(alone[1], ps[lo:lo + sets[source].n_reads])


def test_the_file_written_by_hand_in_test_phase_reads_back(tmp_path):
    from tests.test_phase import EXPECTED, _small
    bam, vcf = _small(tmp_path)
    tags = {}
    out = phase.write_phased_vcf(vcf, [bam], str(tmp_path / "results.output.phased.vcf"), restatement=True, haplotags=tags)
    assert open(out).read().endswith("".join(EXPECTED))
    records = ht.phased_records(out)
    assert list(records) == ["chrB"] and [(r.pos, r.a, r.b, r.ps) for r in records["chrB"]] == [(5, 0, 1, 5), (9, 0, 1, 5), (13, 0, 1, 5)]
    from hello_amd.bam import BamFile
    with BamFile(bam) as b:
        reads = b.fetch("chrB", 0, 40)
    hp, ps = ht.haplotags_restated(reads, records["chrB"])
    assert np.array_equal(hp, tags["chrB"][0]) and np.array_equal(ps, tags["chrB"][1])


# ---- (4) refusals and flags ---------------------------------------------------------------------------------------------------
def _args(*extra):
    return call.parser().parse_args(["--workdir", "w", "--network", "m.npz"] + list(extra))


BAM = ["--from_bam", "--pbam", "x.bam", "--ref", "g.fa"]


@pytest.mark.parametrize("flag", [["--haplotag_vcf", "p.vcf"], ["--haplotag"]], ids=["haplotag_vcf", "haplotag"])
def test_the_flags_need_a_bam_route_include_hp_and_one_gpu(flag, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    name = flag[0]
    with pytest.raises(SystemExit, match=name + r" tags the reads the candidate stage fetches.*add --from_bam .*or --from_bams"):
        call.main(_args("--shards", "s", "--include_hp", *flag))
    with pytest.raises(SystemExit, match="drop --shards"):
        call.main(_args("--shards", "s", "--include_hp", *BAM, *flag))
    with pytest.raises(SystemExit, match=name + " without --include_hp.*add --include_hp"):
        call.main(_args(*BAM, *flag))
    with pytest.raises(SystemExit, match=name + ".*--gpus 1"):
        call.main(_args(*BAM, "--include_hp", "--gpus", "2", *flag))
    with pytest.raises(SystemExit, match=name + ".*--gpus 1"):
        call.main(_args("--from_bams", "--resident", "--ibam", "x.bam", "--pbam", "y.bam", "--ref", "g.fa", "--include_hp", "--gpus", "2", *flag))
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match=name + ".*on one GPU"):
        call.main(_args(*BAM, "--include_hp", *flag))


def test_the_two_flags_exclude_each_other():
    with pytest.raises(SystemExit, match="give one of the two"):
        call.main(_args(*BAM, "--include_hp", "--haplotag", "--haplotag_vcf", "p.vcf"))


def test_without_the_flags_nothing_is_checked_made_or_written(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    args = _args("--shards", "s")
    assert args.haplotag is False and args.haplotag_vcf is None
    call.check_haplotag(args)                                                                    # no --from_bam, no --include_hp: not its business
    assert call.haplotagger_of(args) is None
    from hello_amd import pacbio
    find, kw = call.Route.from_args(_args(*BAM)).finder(None)                                    # no tagger: the finder itself, nothing bound
    assert find is pacbio.find_pacbio_candidates and "tagger" not in kw
    call._close_haplotagger(None)
    assert os.listdir(tmp_path) == []
    call.check_haplotag(call.argparse.Namespace(shards="s"))                                     # an args object from before the flags


def test_argv_of_carries_both_flags():
    for extra in (["--haplotag"], ["--haplotag_vcf", "some dir/p.vcf"]):
        args = _args(*BAM, "--include_hp", *extra)
        again = call.parser().parse_args(call._argv_of(args))
        assert vars(again) == vars(args)
        assert (again.haplotag, again.haplotag_vcf) == (extra == ["--haplotag"], None if extra == ["--haplotag"] else "some dir/p.vcf")


def test_the_passes_of_haplotag_are_the_command_with_other_flags(monkeypatch):
    seen = []
    monkeypatch.setattr(call, "main", lambda a: seen.append(a) or os.path.join(a.workdir, "results.output.vcf"))
    args = _args(*BAM, "--include_hp", "--haplotag", "--gvcf", "--annotate", "--annotate_evidence", "--phase_window", "5", "--resident")
    assert call.haplotag_passes(args) == os.path.join("w", "results.output.vcf")
    first, second = seen
    changed = dict(haplotag=False, gvcf=False, annotate=False, annotate_evidence=False, phase=True, workdir=os.path.join("w", "haplotag_pass1"))
    assert vars(first) == dict(vars(args), **changed)
    assert vars(second) == dict(vars(args), haplotag=False, haplotag_vcf=os.path.join("w", "haplotag_pass1", "results.output.phased.vcf"))
    assert args.haplotag and args.haplotag_vcf is None                                           # the caller's arguments are left alone


# ---- (5) the C ABI ------------------------------------------------------------------------------------------------------------
def test_abi_symbols_are_declared_exported_and_mirrored():
    from hello_amd.engine import load_library
    header = open(os.path.join(ROOT, "include", "hello_mi355x.h")).read()
    lib = load_library()
    for symbol in ("hello_haplotag_create", "hello_haplotag_reads", "hello_haplotag_stats"):
        assert re.search(r"\bint\s+%s\(" % symbol, header), symbol
        assert hasattr(lib, symbol), symbol
    assert re.search(r"\bvoid hello_haplotag_free\(", header) and hasattr(lib, "hello_haplotag_free")
    assert int(re.search(r"#define HELLO_ABI_VERSION (\d+)", header).group(1)) == lib.hello_abi_version() == 2          # additions only
    assert int(re.search(r"#define HELLO_HAPLOTAG_STATS (\d+)", header).group(1)) == len(ht.STAT_NAMES)
    lib = ht._lib()
    assert len(lib.hello_haplotag_create.argtypes) == 8 and len(lib.hello_haplotag_reads.argtypes) == 17
    assert "haplotag.hip" in open(os.path.join(ROOT, "hello_amd", "csrc", "Makefile")).read()
    assert '#include "phase_walk.h"' in open(os.path.join(ROOT, "hello_amd", "csrc", "phase.hip")).read()


def test_the_library_refuses_bad_tables_without_a_gpu():
    lib = ht._lib()
    h = C.c_void_p()
    ptr = lambda a: a.ctypes.data  # noqa: E731
    assert lib.hello_haplotag_create(None, None, None, None, None, 1, 0, C.byref(h)) == -1 and b"NULL pointer" in lib.hello_last_error()
    starts, ends, alleles, offsets, ps = ht.record_table([hc.G_T, hc.rec(8, "A", "A", "C", 9)])
    assert lib.hello_haplotag_create(ptr(starts), ptr(ends), ptr(alleles), ptr(offsets), ptr(ps), 2, 0, None) == -1
    assert lib.hello_haplotag_create(ptr(starts), ptr(ends), ptr(alleles), ptr(offsets), None, 2, 0, C.byref(h)) == -1
    assert lib.hello_haplotag_create(ptr(starts), ptr(ends), ptr(alleles), ptr(offsets), ptr(ps), -1, 0, C.byref(h)) == -1
    assert b"negative" in lib.hello_last_error()
    back = ht.record_table([hc.rec(8, "A", "A", "C", 9), hc.G_T])
    assert lib.hello_haplotag_create(*map(ptr, back), 2, 0, C.byref(h)) == -1 and b"not sorted" in lib.hello_last_error()
    zero = ps.copy()
    zero[1] = 0
    assert lib.hello_haplotag_create(ptr(starts), ptr(ends), ptr(alleles), ptr(offsets), ptr(zero), 2, 0, C.byref(h)) == -1
    assert b"not positive" in lib.hello_last_error() and not h.value
    assert lib.hello_haplotag_reads(None, *([None] * 11), 0, 10, 10, None, None) == -1 and b"NULL pointer" in lib.hello_last_error()
    assert lib.hello_haplotag_stats(None, None) == -1


def test_an_empty_table_needs_no_gpu():
    """No record: the handle opens no device, a call launches nothing and gives zeros -- also where no GPU exists."""
    reads = pc.reads_of(hc.READ_TABLE[0].reads)
    with ht.Haplotagger(None, records={"chr1": [], "chr2": [hc.G_T]}) as tagger:
        hp, ps = tagger.tag("chr1", reads)
        assert hp.tolist() == [0, 0] and ps.tolist() == [0, 0] and hp.dtype == np.uint8 and ps.dtype == np.int64
        assert tagger.tag("chrX", reads)[0].tolist() == [0, 0]                                   # a chromosome the file does not have
        assert tagger.retag("chr1", reads).hp.tolist() == [0, 0] and tagger.retag("chr1", reads) is not reads
        st = tagger.stats
        assert st["calls"] == 4 and st["reads"] == 8 and st["kernel_ms"] == 0 and st["records"] == 1
    lib = ht._lib()
    h = C.c_void_p()
    empty = ht.record_table([])
    assert lib.hello_haplotag_create(*(a.ctypes.data for a in empty), 0, 0, C.byref(h)) == 0 and h.value
    hp, ps = np.full(2, 9, np.uint8), np.full(2, 9, np.int64)
    assert lib.hello_haplotag_reads(h, *reads.pointers(reads.hp), 2, 10, 10, hp.ctypes.data, ps.ctypes.data) == 0
    assert hp.tolist() == [0, 0] and ps.tolist() == [0, 0]
    beyond = pc.reads_of([(0, [(pc.M, 9)], "ACGTGCAT", [30] * 8, 0, 60)])
    assert lib.hello_haplotag_reads(h, *beyond.pointers(beyond.hp), 1, 10, 10, hp.ctypes.data, ps.ctypes.data) == -1
    assert b"consumes 9 bases, it has 8" in lib.hello_last_error()
    lib.hello_haplotag_free(h)
