"""The phasing rules of DESIGN.md section 7g, on the CPU: the restatement in hello_amd/phase.py against the tables worked by hand
(tests/phase_cases.py), the header and the file against an expected file written out by hand, the host-side chain of the built
library (``hello_phase_chain``, no GPU) against ``phase.chain`` on random link arrays, the refusals of ``call --phase`` and of
``python -m hello_amd.phase``, and the new symbols of the C ABI.  The GPU is held to the restatement in tests/test_gpu_phase.py."""
import os
import re

import numpy as np
import pytest

from hello_amd import call, phase
from tests import phase_cases as pc
from tests.bam_writer import Read, write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def per_read(slots, offsets):
    return [slots[int(offsets[i]):int(offsets[i + 1])].tolist() for i in range(len(offsets) - 1)]


# ---- observations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.OBSERVE_TABLE, ids=[c.name for c in pc.OBSERVE_TABLE])
def test_observation_rule_by_hand(case):
    reads = pc.reads_of(case.reads)
    slots, offsets, first = phase.slots_of([reads], case.records, q_threshold=10, mapq_threshold=10)
    assert slots.dtype == np.int8 and offsets.dtype == np.int64 and first.dtype == np.int64
    assert per_read(slots, offsets) == case.slots
    for r, why in enumerate(case.why):
        assert phase.observe_why(reads, r, case.records[int(first[r])])[1] == why, r


def test_two_read_sets_observe_alike_and_follow_one_another():
    case = pc.OBSERVE_TABLE[0]
    a, b = pc.reads_of(case.reads[:1]), pc.reads_of(case.reads[1:])
    slots, offsets, _ = phase.slots_of([a, b], case.records)
    assert per_read(slots, offsets) == case.slots


def test_a_cigar_that_leaves_its_bases_and_unsorted_records_are_refused():
    reads = pc.reads_of([(0, [(pc.M, 9)], "ACGTGCAT", [30] * 8, 0, 60)])
    with pytest.raises(ValueError, match="consumes more bases"):
        phase.slots_of([reads], [pc.G_T])
    fine = pc.reads_of([(0, [(pc.M, 8)], "ACGTGCAT", [30] * 8, 0, 60)])
    with pytest.raises(ValueError, match="not sorted"):
        phase.slots_of([fine], [pc.snp(6, "A", "C"), pc.G_T])


def test_phasable():
    for line, rec, _, _, _ in pc.LINE_TABLE:
        assert phase.phasable(line) == rec
    assert phase.phasable(b"chr1\t5\t.\tg\tt\t30\t.\tHELLO\tGT\t0/1\n") == pc.G_T                 # upper-cased
    assert phase.phasable(b"chr1\t5\t.\tG\tT\t30\t.\tHELLO\tGT\t1/0\n") == pc.snp(4, "G", None, 1, 0, ["T"])
    for line in pc.NOT_PHASABLE:
        assert phase.phasable(line) is None, line


# ---- links, chain, haplotags --------------------------------------------------------------------------------------------------
def test_links_by_hand():
    slots, offsets, first = phase.slots_of([pc.reads_of(pc.LINK_READS)], pc.LINK_RECORDS)
    assert per_read(slots, offsets) == pc.LINK_SLOTS
    link = phase.links_of(slots, offsets, first, len(pc.LINK_RECORDS), pc.LINK_WINDOW)
    assert link.dtype == np.int32 and link.shape == (4, 2, 2) and link.tolist() == pc.LINKS
    wide = phase.links_of(slots, offsets, first, len(pc.LINK_RECORDS), 3)                          # k = 3 reaches from record 3 to 0
    assert wide[:, :2].tolist() == pc.LINKS and wide[3, 2].tolist() == [0, 1] and not wide[:3, 2].any()


@pytest.mark.parametrize("case", pc.CHAIN_TABLE, ids=[c.name for c in pc.CHAIN_TABLE])
@pytest.mark.parametrize("native", [False, True], ids=["restatement", "hello_phase_chain"])
def test_chain_by_hand(case, native):
    run = phase.chain_native if native else phase.chain
    sets, flip = run(np.array(case.link, np.int32), case.window, case.min_margin, list(case.chromosome) or None)
    assert sets.dtype == np.int32 and flip.dtype == np.uint8
    assert sets.tolist() == case.sets and flip.tolist() == case.flip


@pytest.mark.parametrize("n, window", [(0, 8), (1, 8), (5, 8), (300, 8), (300, 1), (120, 32), (64, 3)])
def test_hello_phase_chain_equals_the_restatement(n, window):
    rng = np.random.default_rng(100 * n + window)
    for margin in (1, 2, 4):
        link = rng.integers(0, 6, size=(n, window, 2)).astype(np.int32)
        link[rng.random((n, window)) < 0.5] = 0                                                  # many records without a link
        chromosome = np.sort(rng.integers(0, 3, size=n)).astype(np.int32)                        # changes inside the window
        want = phase.chain(link, window, margin, chromosome)
        got = phase.chain_native(link, window, margin, chromosome)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        if n >= 64:
            assert 1 < len(set(want[0].tolist())) < n and want[1].any() and len(set(chromosome.tolist())) == 3


def test_hello_phase_chain_refuses_bad_arguments():
    link = np.zeros((2, 8, 2), np.int32)
    with pytest.raises(RuntimeError, match="window"):
        phase.chain_native(np.zeros((2, 33, 2), np.int32), 33, 2)
    with pytest.raises(RuntimeError, match="min_margin"):
        phase.chain_native(link, 8, 0)


def test_haplotags_by_hand():
    assert phase.set_positions(pc.TAG_SETS, pc.TAG_POSITIONS).tolist() == pc.TAG_SET_POSITIONS
    slots = np.array([x for _, s, _ in pc.TAG_READS for x in s], np.int8)
    offsets = np.concatenate([[0], np.cumsum([len(s) for _, s, _ in pc.TAG_READS])]).astype(np.int64)
    hp, ps = phase.haplotags_of(slots, offsets, [f for f, _, _ in pc.TAG_READS], pc.TAG_SETS, pc.TAG_FLIP, pc.TAG_POSITIONS)
    assert hp.dtype == np.uint8 and ps.dtype == np.int64
    assert list(zip(hp.tolist(), ps.tolist())) == [want for _, _, want in pc.TAG_READS]


# ---- lines, header, file ------------------------------------------------------------------------------------------------------
def test_phased_line():
    for line, rec, flip, ps, want in pc.LINE_TABLE:
        assert phase.phased_line(line, rec, flip, ps) == want


def test_header_adds_ps_in_front_of_the_column_line():
    plain = call.header(["chr1"], {"chr1": 1000})
    got = phase.phased_header(plain)
    assert got.splitlines(keepends=True)[-2:] == [phase.PS_HEADER, plain.splitlines(keepends=True)[-1]]
    assert got.replace(phase.PS_HEADER, "") == plain and got.splitlines()[-1].startswith("#CHROM")
    assert phase.PS_HEADER == '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set: POS of its first record">\n'


HEADER = "##fileformat=VCFv4.1\n##contig=<ID=chrB,length=40>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE1\n"
# chrB: SNPs at 5 (G/T), 9 (A/C), 13 (C/G) and 30 (T/A); three reads carry T, C, C (so 13 is flipped against its GT 0/1 ... 1/0
# below), three carry G, A, G; nobody links 30; chrA: one record, one read
INPUT = ["chrB\t5\t.\tG\tT\t30\t.\tHELLO\tGT\t0/1\n",
         "chrB\t7\t.\tA\tC\t30\t.\tHELLO\tGT\t1/1\n",
         "chrB\t9\t.\tA\tC\t9.5\tFAIL\tHELLO;MQ=60\tGT:GQ:DP\t0/1:8:12\n",
         "chrB\t13\t.\tC\tG\t30\t.\tHELLO\tGT\t1/0\n",
         "chrB\t30\t.\tT\tA\t30\t.\tHELLO\tGT\t0/1\n",
         "chrA\t3\t.\tA\tG\t30\t.\tHELLO\tGT\t0/1\n"]
EXPECTED = ["chrB\t5\t.\tG\tT\t30\t.\tHELLO\tGT:PS\t0|1:5\n",
            "chrB\t7\t.\tA\tC\t30\t.\tHELLO\tGT\t1/1\n",
            "chrB\t9\t.\tA\tC\t9.5\tFAIL\tHELLO;MQ=60\tGT:GQ:DP:PS\t0|1:8:12:5\n",
            "chrB\t13\t.\tC\tG\t30\t.\tHELLO\tGT:PS\t0|1:5\n",
            "chrB\t30\t.\tT\tA\t30\t.\tHELLO\tGT\t0/1\n",
            "chrA\t3\t.\tA\tG\t30\t.\tHELLO\tGT\t0/1\n"]


def _small(tmp_path):
    #            0         1
    #            0123456789012345678
    ref_like = "AAAAGAAAAAAACAAAAAAA"
    hap1 = ref_like                                    # G at 4, A at 8, C at 12: the a alleles of 5 and 9, the b allele (0) of 13
    hap2 = "AAAATAAACAAAGAAAAAAA"                      # T, C, G
    reads = [Read("h1_%d" % i, 0, [(0, 20)], hap1, [30] * 20, 0, 60, ref_id=0) for i in range(3)]
    reads += [Read("h2_%d" % i, 0, [(0, 20)], hap2, [30] * 20, 0, 60, ref_id=0) for i in range(3)]
    reads += [Read("far", 25, [(0, 10)], "AAAATAAAAA", [30] * 10, 0, 60, ref_id=0), Read("a", 0, [(0, 8)], "AAGAAAAA", [30] * 8, 0, 60, ref_id=1)]
    bam, vcf = str(tmp_path / "x.bam"), str(tmp_path / "results.output.vcf")
    write_bam(bam, [("chrB", 40), ("chrA", 20)], reads, index=True)
    with open(vcf, "w") as fh:
        fh.write(HEADER + "".join(INPUT))
    return bam, vcf


def test_write_phased_vcf_against_a_file_written_by_hand(tmp_path):
    """Record 13 is written 1/0: a = 1 (G) lies on the haplotype of the b alleles of 5 and 9, so it is flipped and comes out 0|1."""
    bam, vcf = _small(tmp_path)
    tags, stats = {}, {}
    out = phase.write_phased_vcf(vcf, [bam], str(tmp_path / "results.output.phased.vcf"), restatement=True, haplotags=tags, stats=stats)
    want = HEADER.replace("#CHROM", phase.PS_HEADER + "#CHROM") + "".join(EXPECTED)
    assert open(out).read() == want
    assert open(vcf).read() == HEADER + "".join(INPUT)                                         # the input is untouched
    assert tags["chrB"][0].tolist() == [1, 1, 1, 2, 2, 2, 0] and tags["chrB"][1].tolist() == [5] * 6 + [0]
    assert tags["chrA"][0].tolist() == [0] and stats["calls"] == 2
    # spans of 7 positions: a read belongs to the span of its start, and nothing changes
    small = phase.write_phased_vcf(vcf, [bam], str(tmp_path / "small.vcf"), restatement=True, max_span=7)
    assert open(small).read() == want
    # only chrA: the records of chrB pass through
    part = phase.write_phased_vcf(vcf, [bam], str(tmp_path / "part.vcf"), chromosomes=["chrA"], restatement=True)
    assert open(part).read() == HEADER.replace("#CHROM", phase.PS_HEADER + "#CHROM") + "".join(INPUT)
    # a margin nobody reaches: everything stays unphased
    none = phase.write_phased_vcf(vcf, [bam], str(tmp_path / "none.vcf"), min_margin=7, restatement=True)
    assert open(none).read() == HEADER.replace("#CHROM", phase.PS_HEADER + "#CHROM") + "".join(INPUT)
    with pytest.raises(ValueError, match="window"):
        phase.write_phased_vcf(vcf, [bam], str(tmp_path / "w.vcf"), window=33, restatement=True)
    with pytest.raises(ValueError, match="min_margin"):
        phase.write_phased_vcf(vcf, [bam], str(tmp_path / "w.vcf"), min_margin=0, restatement=True)


def test_a_chromosome_the_bam_does_not_have_is_refused(tmp_path):
    bam, vcf = _small(tmp_path)
    with open(vcf, "a") as fh:
        fh.write("chrZ\t3\t.\tA\tG\t30\t.\tHELLO\tGT\t0/1\n")
    with pytest.raises(ValueError, match="chrZ"):
        phase.write_phased_vcf(vcf, [bam], str(tmp_path / "z.vcf"), restatement=True)


# ---- the refusals -------------------------------------------------------------------------------------------------------------
def _args(*extra):
    return call.parser().parse_args(["--workdir", "w", "--network", "m.npz"] + list(extra))


def test_phase_needs_a_bam_route_one_gpu_and_sane_numbers(monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit, match="--from_bam .*or --from_bams"):
        call.main(_args("--shards", "s", "--phase"))
    with pytest.raises(SystemExit, match="--gpus 1"):
        call.main(_args("--from_bam", "--ibam", "x.bam", "--ref", "g.fa", "--phase", "--gpus", "2"))
    with pytest.raises(SystemExit, match="--gpus 1"):
        call.main(_args("--from_bams", "--resident", "--ibam", "x.bam", "--pbam", "y.bam", "--ref", "g.fa", "--phase", "--gpus", "2"))
    for bad in ("0", "33"):
        with pytest.raises(SystemExit, match="phase_window"):
            call.main(_args("--from_bam", "--ibam", "x.bam", "--ref", "g.fa", "--phase", "--phase_window", bad))
    with pytest.raises(SystemExit, match="phase_min_margin"):
        call.main(_args("--from_bam", "--ibam", "x.bam", "--ref", "g.fa", "--phase", "--phase_min_margin", "0"))
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process on one GPU"):
        call.main(_args("--from_bam", "--ibam", "x.bam", "--ref", "g.fa", "--phase"))


def test_without_the_flag_nothing_is_checked_or_written():
    args = _args("--shards", "s", "--phase_window", "99")
    assert args.phase is False and _args("--shards", "s").phase_window == 8 and args.phase_min_margin == 2
    call.check_phase(args)
    assert call.phase_pass(args, "w/results.output.vcf") is None


def test_the_module_refuses_bad_numbers_before_it_opens_anything():
    base = ["--vcf", "none.vcf", "--bam", "none.bam", "--output", "o.vcf"]
    with pytest.raises(SystemExit, match="phase_window"):
        phase.main(base + ["--phase_window", "0"])
    with pytest.raises(SystemExit, match="phase_window"):
        phase.main(base + ["--phase_window", "33"])
    with pytest.raises(SystemExit, match="phase_min_margin"):
        phase.main(base + ["--phase_min_margin", "0"])
    with pytest.raises(SystemExit, match="one or two"):
        phase.main(["--vcf", "none.vcf", "--bam", "a.bam,b.bam,c.bam", "--output", "o.vcf"])
    args = phase.parser().parse_args(base)
    assert (args.q_threshold, args.mapq_threshold, args.phase_window, args.phase_min_margin, args.device, args.chromosomes) == \
        (10, 10, 8, 2, 0, None)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_are_declared_exported_and_mirrored():
    from hello_amd.engine import load_library
    header = open(os.path.join(ROOT, "include", "hello_mi355x.h")).read()
    lib = load_library()
    for symbol in ("hello_phase_observe", "hello_phase_array", "hello_phase_stats", "hello_phase_tag", "hello_phase_chain"):
        assert re.search(r"\bint %s\(" % symbol, header), symbol
        assert hasattr(lib, symbol), symbol
    assert re.search(r"\bvoid hello_phase_free\(", header) and hasattr(lib, "hello_phase_free")
    assert int(re.search(r"#define HELLO_ABI_VERSION (\d+)", header).group(1)) == lib.hello_abi_version() == 2          # additions only
    assert int(re.search(r"#define HELLO_PHASE_MAX_WINDOW (\d+)", header).group(1)) == phase.MAX_WINDOW
    assert int(re.search(r"#define HELLO_PHASE_STATS (\d+)", header).group(1)) == len(phase.STAT_NAMES)
    for name in ("SLOTS", "SLOT_OFFSETS", "FIRST", "LINKS", "HP", "PS"):
        assert int(re.search(r"HELLO_PHASE_%s = (\d+)" % name, header).group(1)) == getattr(phase, name)
    assert len(phase._lib().hello_phase_observe.argtypes) == 22
    # without a GPU: NULL pointers are refused with HELLO_ERR_ARG before anything is opened
    assert lib.hello_phase_observe(*([None] * 11), 0, None, None, None, None, 0, 10, 10, 8, 0, None) == -1
    assert b"NULL pointer" in lib.hello_last_error()
    assert "phase.hip" in open(os.path.join(ROOT, "hello_amd", "csrc", "Makefile")).read()
