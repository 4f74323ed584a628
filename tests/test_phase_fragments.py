"""The fragment rules of DESIGN.md section 7i, on the CPU: the restatement in hello_amd/phase.py against the tables worked by hand
(tests/fragment_cases.py), its agreement with section 7g when nobody has a mate, the refusal of a lone ``--phase_fragments``, the new
symbols of the C ABI and what the feature is for -- a paired-end chromosome that ``--phase`` cannot phase at all and
``--phase_fragments`` phases completely.  The GPU is held to the restatement in tests/test_gpu_phase_fragments.py."""
import os
import re

import numpy as np
import pytest

from hello_amd import call, phase
from tests import fragment_cases as fc
from tests.bam_writer import write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE1\n"


def restated(case):
    sets = case.sets()
    counts = {}
    mate = phase.mates_of(sets, 10, counts)
    slots, offsets, first = phase.slots_of(sets, case.records)
    links = phase.links_of(slots, offsets, first, len(case.records), case.window, mate=mate)
    sets_, flip = phase.chain(links, case.window, 1)
    hp, ps = phase.haplotags_of(slots, offsets, first, sets_, flip, [r.pos for r in case.records], mate=mate)
    return dict(mate=mate, links=links, hp=hp, ps=ps, set=sets_, flip=flip, **counts)


# ---- the hand tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.HAND_TABLE, ids=[c.name for c in fc.HAND_TABLE])
def test_fragment_rules_by_hand(case):
    got = restated(case)
    assert got["mate"].dtype == np.int64 and got["mate"].tolist() == case.mate
    assert (got["pairs"], got["groups_refused"]) == (case.pairs, case.refused)
    assert got["links"].dtype == np.int32 and np.array_equal(got["links"], case.dense_links())
    assert got["hp"].tolist() == case.hp and got["ps"].tolist() == case.ps


def test_the_table_has_a_case_per_clause():
    names = " | ".join(c.name for c in fc.HAND_TABLE)
    for clause in ("within the window", "beyond the window", "agree", "disagree", "one mate observes", "not counted", "group of three",
                   "two first mates", "0x1 unset", "source 0 and source 1", "before the first", "mate is absent", "2^64 - 1",
                   "empty read set", "empty record table"):
        assert clause in names, clause


def test_fragment_observations_by_hand():
    """Overlap with a disagreement: reads over records 0-2 and 1-3; both mates get F over records 0..3, none at record 1.  With a
    gap: the records between the mates are none."""
    case = next(c for c in fc.HAND_TABLE if "disagree" in c.name)
    slots, offsets, first = phase.slots_of(case.sets(), case.records)
    assert slots.tolist() == [0, 0, 0, 1, 0, 0]
    f_slots, f_offsets, f_first = phase.fragment_observations(slots, offsets, first, np.array(case.mate))
    assert f_slots.tolist() == [0, -1, 0, 0] * 2 and f_offsets.tolist() == [0, 4, 8] and f_first.tolist() == [0, 0]
    alone = phase.fragment_observations(slots, offsets, first, np.array([-1, -1]))
    assert alone[0].tolist() == slots.tolist() and alone[1].tolist() == offsets.tolist() and alone[2].tolist() == first.tolist()
    gap = fc.HAND_TABLE[0]
    slots, offsets, first = phase.slots_of(gap.sets(), gap.records)
    f_slots, f_offsets, f_first = phase.fragment_observations(slots, offsets, first, np.array(gap.mate))
    assert f_slots.tolist() == [0, 0, -1, -1, 1, 1] * 2 and f_first.tolist() == [0, 0]


def test_the_first_probed_slot_is_restated_for_every_bit_of_the_name():
    assert [phase.pair_table_size(n) for n in (0, 1, 2, 3, 4, 5, 4096, 4097)] == [2, 2, 4, 8, 8, 16, 8192, 16384]
    size = 1 << 14
    base = np.uint64(0x0123456789ABCDEF)
    names = np.array([base] + [base ^ np.uint64(1 << b) for b in range(64)], np.uint64)
    slots = phase.pair_table_slot(names, np.zeros(65, np.uint8), size)
    assert slots.dtype == np.uint32 and (slots < size).all()
    assert (slots[1:] != slots[0]).sum() >= 60                                  # a change in any bit moves the slot
    assert phase.pair_table_slot(names[:1], np.ones(1, np.uint8), size)[0] == (int(slots[0]) + 1) % size
    # worked by hand for name 1: x = 1; x ^= x >> 29 -> 1; x *= 0xBF58476D1CE4E5B9; x ^= x >> 32 -> low word 0x1CE4E5B9 ^ 0xBF58476D
    assert int(phase.pair_table_slot(np.array([1], np.uint64), [0], 1 << 30)[0]) == (0x1CE4E5B9 ^ 0xBF58476D) & ((1 << 30) - 1)


# ---- nobody has a mate: section 7g ----------------------------------------------------------------------------------------------
def test_without_mates_the_functions_are_those_of_7g():
    from tests import phase_cases as pc
    from tests.test_gpu_phase import chromosome
    c = chromosome()
    want = c["want"]
    nobody = np.full(want["first"].shape[0], -1, np.int64)
    args = (want["slots"], want["slot_offsets"], want["first"])
    assert np.array_equal(phase.links_of(*args, len(c["records"]), pc.WINDOW, mate=nobody), want["links"])
    hp, ps = phase.haplotags_of(*args, want["set"], want["flip"], [r.pos for r in c["records"]], mate=nobody)
    assert np.array_equal(hp, want["hp"]) and np.array_equal(ps, want["ps"])
    assert (phase.mates_of(c["sets"]) == -1).all()                              # flag 0 everywhere: no pair


# ---- what the feature is for ----------------------------------------------------------------------------------------------------
def test_paired_reads_phase_nothing_alone_and_everything_as_fragments(tmp_path):
    lines, hap, reads = fc.illumina_pairs()
    bam, vcf = str(tmp_path / "pairs.bam"), str(tmp_path / "results.output.vcf")
    write_bam(bam, [("chr1", fc.LENGTH)], reads, index=True)
    with open(vcf, "wb") as fh:
        fh.write(HEADER.encode() + b"".join(lines))
    assert len(lines) == 20 and len(reads) == 1200

    def genotypes(path):
        return [line.split(b"\t")[9].rstrip(b"\n").split(b":") for line in open(path, "rb") if not line.startswith(b"#")]
    alone = phase.write_phased_vcf(vcf, [bam], str(tmp_path / "alone.vcf"), restatement=True)
    assert all(g == [b"0/1"] for g in genotypes(alone))                         # no PS at all: no read holds two records
    tags, stats = {}, {}
    joined = phase.write_phased_vcf(vcf, [bam], str(tmp_path / "joined.vcf"), restatement=True, fragments=True, haplotags=tags,
                                    stats=stats)
    got = genotypes(joined)
    assert all(len(g) == 2 and g[1] == b"151" for g in got)                     # one set, opened by the record at POS 151
    left = [int(g[0].split(b"|")[0]) for g in got]
    assert left in (hap, [1 - h for h in hap]) and 0 < sum(hap) < 20            # the planted haplotypes, up to one global flip
    assert stats["pairs"] == 600 and stats["groups_refused"] == 0
    # both reads of every pair get one tag, and the tag is the pair's planted haplotype (up to that flip)
    hp, ps = tags["chr1"]
    by_name = {}
    for r, h, p in zip(reads, hp.tolist(), ps.tolist()):
        by_name.setdefault(r.name, []).append((h, p))
    assert all(len(v) == 2 and v[0] == v[1] for v in by_name.values())
    tagged = {name: v[0] for name, v in by_name.items() if v[0][1]}
    assert len(tagged) > 280 and all(p == 151 for _, p in tagged.values())     # half the pairs hold no record at all
    flipped = left != hap
    assert all(h == 1 + ((int(name[1:]) % 2) ^ flipped) for name, (h, _) in tagged.items())
    # spans of 1 000 positions put mates into different spans: nothing changes
    small = phase.write_phased_vcf(vcf, [bam], str(tmp_path / "small.vcf"), restatement=True, fragments=True, max_span=1000)
    assert open(small, "rb").read() == open(joined, "rb").read()


# ---- the refusal and the flags --------------------------------------------------------------------------------------------------
def _args(*extra):
    return call.parser().parse_args(["--workdir", "w", "--network", "m.npz"] + list(extra))


def test_a_lone_phase_fragments_is_refused_and_names_the_fix():
    with pytest.raises(SystemExit, match=r"add --phase .*or --haplotag"):
        call.check_phase(_args("--from_bam", "--ibam", "x.bam", "--ref", "g.fa", "--phase_fragments"))
    with pytest.raises(SystemExit, match="--phase_fragments"):
        call.main(_args("--shards", "s", "--phase_fragments"))
    call.check_phase(_args("--from_bam", "--ibam", "x.bam", "--ref", "g.fa", "--phase", "--phase_fragments"))
    call.check_phase(_args("--from_bam", "--ibam", "x.bam", "--ref", "g.fa", "--include_hp", "--haplotag", "--phase_fragments"))
    assert _args("--shards", "s").phase_fragments is False and _args("--shards", "s", "--phase_fragments").phase_fragments is True
    base = ["--vcf", "none.vcf", "--bam", "none.bam", "--output", "o.vcf"]
    assert phase.parser().parse_args(base).phase_fragments is False
    assert phase.parser().parse_args(base + ["--phase_fragments"]).phase_fragments is True


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_are_declared_exported_and_mirrored():
    from hello_amd.engine import load_library
    header = open(os.path.join(ROOT, "include", "hello_mi355x.h")).read()
    lib = load_library()
    for symbol in ("hello_phase_fragments", "hello_phase_tag_fragments", "hello_phase_fragment_stats"):
        assert re.search(r"\bint %s\(" % symbol, header), symbol
        assert hasattr(lib, symbol), symbol
    assert int(re.search(r"#define HELLO_PHASE_FRAGMENT_STATS (\d+)", header).group(1)) == len(phase.FRAGMENT_STAT_NAMES)
    for name in ("MATE", "FRAGMENT_LINKS"):
        assert int(re.search(r"HELLO_PHASE_%s = (\d+)" % name, header).group(1)) == getattr(phase, name)
    bound = phase._lib()
    assert len(bound.hello_phase_fragments.argtypes) == 5 and len(bound.hello_phase_tag_fragments.argtypes) == 3
    assert len(bound.hello_phase_observe.argtypes) == 22 and len(bound.hello_phase_tag.argtypes) == 3      # the old ones stay


def test_null_handles_are_refused_without_a_gpu():
    lib = phase._lib()
    some = np.zeros(1, np.uint64)
    assert lib.hello_phase_fragments(None, some.ctypes.data, some.ctypes.data, some.ctypes.data, 1) == -1
    assert b"NULL pointer" in lib.hello_last_error()
    assert lib.hello_phase_tag_fragments(None, some.ctypes.data, some.ctypes.data) == -1
    assert b"NULL pointer" in lib.hello_last_error()
    import ctypes as C
    assert lib.hello_phase_fragment_stats(None, (C.c_double * 5)()) == -1
    assert b"NULL pointer" in lib.hello_last_error()
