"""The gVCF rules of DESIGN.md section 7f, on the CPU: the restatement in hello_amd/gvcf.py against a table of cases worked by
hand (tests/gvcf_cases.py), the banding and the blocks, the block line and the header, the file ``write_gvcf`` writes from a
small BAM, and the refusals of ``python -m hello_amd.call --gvcf``.  The GPU is held to the restatement in
tests/test_gpu_refblocks.py."""
import numpy as np
import pytest

from hello_amd import call, gvcf
from tests import gvcf_cases as gc
from tests import hotspot_synth as synth
from tests.bam_writer import write_bam


# ---- counting ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.HAND_TABLE, ids=[c.name for c in gc.HAND_TABLE])
def test_counting_rule_by_hand(case):
    lo, hi = case.span()
    n_ref, n_total = gvcf.count_positions([gc.reads_of(case.reads)], case.reference, lo, hi, q_threshold=10, mapq_threshold=10)
    assert n_ref.dtype == np.int32 and n_total.dtype == np.int32
    assert n_ref.tolist() == case.n_ref and n_total.tolist() == case.n_total


def test_two_read_sets_count_into_the_same_counters():
    a = gc.reads_of([(0, [(gc.M, 4)], "ACGT", [30] * 4, 0, 60)])
    b = gc.reads_of([(1, [(gc.M, 3)], "CTT", [30] * 3, 0, 60)])
    n_ref, n_total = gvcf.count_positions([a, b], "ACGT", 0, 4)
    assert n_ref.tolist() == [1, 2, 1, 2] and n_total.tolist() == [1, 2, 2, 2]


def test_a_cigar_that_leaves_its_bases_is_refused():
    reads = gc.reads_of([(0, [(gc.M, 5)], "ACGT", [30] * 4, 0, 60)])
    with pytest.raises(ValueError, match="consumes more bases"):
        gvcf.count_positions([reads], "ACGTACGT", 0, 8)


# ---- likelihoods, GQ, bands -------------------------------------------------------------------------------------------------
def _call(n_ref, n_total):
    called, gq, pl = gvcf.position_calls([n_ref], [n_total])
    return bool(called[0]), int(gq[0]), pl[0].tolist()


def test_the_constants_are_the_phred_values_of_the_model():
    assert gvcf.A == pytest.approx(30.0, abs=1e-12) and gvcf.HET == pytest.approx(3.0102999566398, abs=1e-12)
    assert gvcf.B == pytest.approx(0.0043451177401, abs=1e-12)


def test_zero_depth_is_a_no_call_by_the_strict_comparison():
    # L00 = L01 = L11 = 0: L00 < L01 does not hold
    assert _call(0, 0) == (False, 0, [0, 0, 0])


def test_even_support_is_a_no_call():
    # 15 ref / 15 alt: L00 = L11 = 15 a + 15 b = 450.07 > L01 = 30 c = 90.31
    assert _call(15, 30) == (False, 0, [255, 0, 255])


def test_the_call_needs_l00_strictly_smallest():
    # 9 ref / 1 alt: L00 = 30.0391 < L01 = 30.1030, so called, with PL01 = floor(0.0639 + 0.5) = 0: a called position of GQ 0
    assert _call(9, 10) == (True, 0, [0, 0, 240])
    # 8 ref / 1 alt: L00 = 30.0348 > L01 = 27.0927
    assert _call(8, 9) == (False, 0, [3, 0, 213])
    assert _call(0, 40) == (False, 0, [255, 120, 0])


def test_the_caps_of_gq_and_pl():
    # 33 reference reads: PL01 = floor(33 (c - b) + 0.5) = floor(99.70) = 99; 34: 102, GQ stays 99; PL11 = 33 (a - b) > 255
    assert _call(32, 32) == (True, 96, [0, 96, 255])
    assert _call(33, 33) == (True, 99, [0, 99, 255])
    assert _call(34, 34) == (True, 99, [0, 102, 255])
    assert _call(40, 40) == (True, 99, [0, 120, 255])
    assert _call(100, 100) == (True, 99, [0, 255, 255])


@pytest.mark.parametrize("binsize, bands", [(1, [3, 6, 9, 12, 15, 27, 30]), (5, [0, 1, 1, 2, 3, 5, 6]), (10, [0, 0, 0, 1, 1, 2, 3])])
def test_band_edges(binsize, bands):
    depth = [1, 2, 3, 4, 5, 9, 10]                        # GQ 3, 6, 9, 12, 15, 27, 30: 15 and 30 sit on edges of 5 and 10
    got = []
    for d in depth:
        b = gvcf.blocks_of([d], [d], (), binsize)
        assert b["gq"].tolist() == [_call(d, d)[1]]
        got += b["band"].tolist()
    assert got == bands
    with pytest.raises(ValueError):
        gvcf.blocks_of([1], [1], (), 0)


# ---- blocks -----------------------------------------------------------------------------------------------------------------
def _rows(b):
    return [tuple(int(b[name][i]) for name, _, _ in gvcf.FIELDS) for i in range(b["start"].shape[0])]


def test_blocks_are_maximal_runs_of_one_band():
    #            band 6 (GQ 30, 33) | no-call | band 0 (GQ 3)
    n_ref = [10, 11, 10, 0, 0, 1, 1]
    b = gvcf.blocks_of(n_ref, n_ref, (), 5, lo=100)
    assert _rows(b) == [(100, 103, 6, 10, 30, 10, 10), (103, 105, gvcf.NO_CALL, 0, 0, 0, 0), (105, 107, 0, 1, 3, 1, 1)]


def test_excluded_intervals_cut_blocks():
    n = [10] * 20
    # one inside, one at the span's start, one at its end, two that touch
    b = gvcf.blocks_of(n, n, [(0, 3), (8, 11), (13, 14), (14, 16), (17, 20)], 5)
    assert [(s, e) for s, e, *_ in _rows(b)] == [(3, 8), (11, 13), (16, 17)]
    assert all(row[2:] == (6, 10, 30, 10, 10) for row in _rows(b))
    assert gvcf.excluded_intervals([(14, 2), (8, 3), (13, 1), (0, 3), (9, 1)]) == [(0, 3), (8, 11), (13, 16)]
    # intervals given in genome coordinates reach into a span that starts elsewhere
    b = gvcf.blocks_of(n, n, [(95, 103), (119, 130)], 5, lo=100)
    assert [(s, e) for s, e, *_ in _rows(b)] == [(103, 119)]
    assert _rows(gvcf.blocks_of(n, n, [(0, 20)], 5)) == []


def test_the_first_position_of_the_smallest_gq_is_reported():
    # GQ 33, 30, 30, 33 in one band of width 5: the two GQ 30 positions have other counters; depth 10 is the smallest
    b = gvcf.blocks_of([11, 10, 19, 11], [11, 10, 20, 11], (), 5)
    assert _rows(b) == [(0, 4, 6, 10, 30, 10, 10)]
    b = gvcf.blocks_of([11, 19, 10, 11], [11, 20, 10, 11], (), 5)
    assert _rows(b) == [(0, 4, 6, 10, 30, 19, 20)]
    # a no-call block reports its first position
    b = gvcf.blocks_of([4, 0, 15], [9, 0, 30], (), 5)
    assert _rows(b) == [(0, 3, gvcf.NO_CALL, 0, 0, 4, 9)]


def test_blocks_join_across_a_span_boundary():
    rng = np.random.default_rng(3)
    n_total = rng.integers(0, 14, size=400).astype(np.int32)
    n_total[150:230] = 11                                  # a block that crosses the cuts at 200 and 201
    n_total[199], n_total[201] = 10, 10                    # GQ 30 on both sides of the cut: the earlier position is reported
    n_ref = np.maximum(n_total - (rng.random(400) < 0.1), 0).astype(np.int32)
    n_ref[150:230] = n_total[150:230]
    excluded = [(40, 44), (198, 199), (300, 301)]
    whole = gvcf.blocks_of(n_ref, n_total, excluded, 5, lo=0)
    assert any(s < 200 < e for s, e, *_ in _rows(whole))
    for cuts in ([200], [200, 201], [1, 399], [44, 198, 199, 300]):
        edges = [0] + cuts + [400]
        parts = [gvcf.blocks_of(n_ref[a:b], n_total[a:b], excluded, 5, lo=a) for a, b in zip(edges, edges[1:])]
        assert _rows(gvcf.join_blocks(parts)) == _rows(whole), cuts
    joined = gvcf.join_blocks([gvcf.blocks_of(n_ref[:200], n_total[:200], excluded, 5), gvcf.empty_blocks(),
                               gvcf.blocks_of(n_ref[200:], n_total[200:], excluded, 5, lo=200)])
    assert _rows(joined) == _rows(whole)
    assert _rows(gvcf.join_blocks([])) == []


# ---- lines and header -------------------------------------------------------------------------------------------------------
def test_block_line():
    assert gvcf.block_line("chr1", 99, 140, 6, 30, 10, 10, 10, "a") == \
        "chr1\t100\t.\tA\t<NON_REF>\t.\t.\tEND=140\tGT:GQ:MIN_DP:PL\t0/0:30:10:0,30,255"
    assert gvcf.block_line("2", 0, 1, gvcf.NO_CALL, 0, 0, 15, 30, ord("n")) == \
        "2\t1\t.\tN\t<NON_REF>\t.\t.\tEND=1\tGT:GQ:MIN_DP:PL\t./.:0:0:255,0,255"
    assert gvcf.block_line("2", 4, 9, gvcf.NO_CALL, 0, 0, 0, 0, "R").split("\t")[3::6] == ["N", "./.:0:0:0,0,0"]
    assert gvcf.block_line("2", 4, 9, 0, 0, 10, 9, 10, "t").endswith("\tT\t<NON_REF>\t.\t.\tEND=9\tGT:GQ:MIN_DP:PL\t0/0:0:10:0,0,240")


def test_block_lines_are_block_line_of_every_block():
    rng = np.random.default_rng(0)
    n_total = rng.integers(0, 50, 300).astype(np.int32)
    n_ref = np.maximum(n_total - rng.integers(0, 4, 300), 0).astype(np.int32)
    reference = "".join(rng.choice(list("ACGTacgtNn"), 300))
    b = gvcf.blocks_of(n_ref, n_total, [(10, 20)], 5)
    want = [gvcf.block_line("c", int(b["start"][i]), int(b["end"][i]), int(b["band"][i]), int(b["gq"][i]), int(b["min_dp"][i]),
                            int(b["n_ref"][i]), int(b["n_total"][i]), reference[int(b["start"][i])]) for i in range(b["start"].shape[0])]
    assert len(want) > 100 and gvcf.block_lines("c", b, reference) == want
    assert gvcf.block_lines("c", gvcf.empty_blocks(), reference) == []


def test_header_adds_what_the_run_did_not_declare():
    plain = call.header(["chr1"], {"chr1": 1000})
    got = gvcf.gvcf_header(plain)
    assert got.splitlines()[-1] == plain.splitlines()[-1] and got.splitlines()[-1].startswith("#CHROM")
    assert [line for line in got.splitlines() if line not in plain.splitlines()] == (
        gvcf.NON_REF_HEADER + gvcf.FORMAT_HEADER["GQ"] + gvcf.FORMAT_HEADER["MIN_DP"] + gvcf.FORMAT_HEADER["PL"]).splitlines()
    assert [line for line in got.splitlines() if line in plain.splitlines()] == plain.splitlines()
    annotated = gvcf.gvcf_header(call.header(["chr1"], {"chr1": 1000}, annotate=True))
    assert annotated.count("##FORMAT=<ID=GQ,") == 1 and annotated.count("##FORMAT=<ID=PL,") == 1
    evidence = gvcf.gvcf_header(call.header(["chr1"], {"chr1": 1000}, evidence=(False, False)))
    for key in ("GQ", "PL", "MIN_DP"):
        assert evidence.count("##FORMAT=<ID=%s," % key) == 1
    assert evidence.count("##ALT=<ID=NON_REF,") == 1 and evidence.count("##INFO=<ID=END,") == 1


# ---- the file ---------------------------------------------------------------------------------------------------------------
def covered(path, lengths):
    """Every data line of a gVCF as (chromosome, start, end, is a block); asserts they tile every chromosome [0, length)."""
    rows = []
    for line in open(path):
        if line.startswith("#"):
            continue
        f = line.rstrip("\n").split("\t")
        start = int(f[1]) - 1
        block = f[4] == "<NON_REF>"
        rows.append((f[0], start, int(f[7][4:]) if block else start + len(f[3]), block))
    at = {c: 0 for c in lengths}
    order = []
    for c, start, end, block in rows:
        if c not in order:
            order.append(c)
        if block:
            assert start == at[c], (c, start, at[c])              # no gap, no overlap
            at[c] = end
        else:
            assert start <= at[c], (c, start, at[c])              # records may lie inside one another, never behind a gap
            at[c] = max(at[c], end)
    assert order == sorted(order)
    assert at == {c: n for c, n in lengths.items()}, at
    return rows


def test_write_gvcf_keeps_the_records_and_tiles_the_chromosomes(tmp_path):
    rng = np.random.default_rng(8)
    refs = {"chrB": synth.random_reference(rng, 1500, masked_fraction=0.1), "chrA": synth.random_reference(rng, 700), "chrC": "ACGT" * 50}
    order = ["chrB", "chrA", "chrC"]                                     # the BAM's and the FASTA's order, not the sorted one
    reads = []
    for i, c in enumerate(order[:2]):
        rs = synth.sample_reads(rng, refs[c], 12, 100, prefix=c)
        rs = [r for r in rs if not (400 <= r.pos < 520 or 400 < r.ref_end <= 520)]
        for r in rs:
            r.ref_id = i
        reads += rs
    bam, fa, vcf_path = str(tmp_path / "x.bam"), str(tmp_path / "g.fa"), str(tmp_path / "results.output.vcf")
    write_bam(bam, [(c, len(refs[c])) for c in order], reads, index=True)
    with open(fa, "w") as fh:
        for c in order:
            fh.write(">%s\n%s\n" % (c, refs[c]))
    records = ["chrA\t1\t.\t%s\tT\t50\t.\tHELLO\tGT\t0/1\n" % refs["chrA"][0],
               "chrA\t301\t.\t%s\tA\t7.5\tFAIL\tHELLO;MQ=60\tGT:GQ:DP\t1/1:8:12\n" % refs["chrA"][300:304],
               "chrA\t303\t.\t%s\tA,C\t9\t.\tHELLO\tGT\t1/2\n" % refs["chrA"][302:303],          # inside the one before
               "chrA\t305\t.\t%s\tG\t9\t.\tHELLO\tGT\t0/1\n" % refs["chrA"][304],              # touches it
               "chrB\t1500\t.\t%s\tG\t30\t.\tHELLO\tGT\t0/1\n" % refs["chrB"][1499]]
    with open(vcf_path, "w") as fh:
        fh.write(call.header(["chrA", "chrB"], {c: len(s) for c, s in refs.items()}) + "".join(records))
    out = gvcf.write_gvcf(vcf_path, [bam], fa, str(tmp_path / "results.output.g.vcf"), restatement=True)
    lines = open(out).read().splitlines(keepends=True)
    assert "".join(line for line in lines if line.startswith("#")) == gvcf.gvcf_header(call.header(["chrA", "chrB"], {c: len(s) for c, s in refs.items()}))
    data = [line for line in lines if not line.startswith("#")]
    assert [line for line in data if "<NON_REF>" not in line] == records             # byte for byte, in order
    rows = covered(out, {c: len(s) for c, s in refs.items()})
    assert [c for c, *_ in rows] == sorted(c for c, *_ in rows)
    # the blocks around the records of chrA: [0, 1) is a record, [300, 305) is excluded as one interval
    blocks_a = [(s, e) for c, s, e, b in rows if c == "chrA" and b]
    assert blocks_a[0][0] == 1 and (300, 305) not in blocks_a and any(e == 300 for _, e in blocks_a) and any(s == 305 for s, _ in blocks_a)
    assert not any(s < 305 and e > 300 for s, e in blocks_a)
    # chrC has no read: one no-call block; the uncovered stretch of chrB is a no-call block too
    assert [line for line in data if line.startswith("chrC\t")] == ["chrC\t1\t.\tA\t<NON_REF>\t.\t.\tEND=200\tGT:GQ:MIN_DP:PL\t./.:0:0:0,0,0\n"]
    assert any(line.startswith("chrB\t") and "\t./.:0:0:0,0,0" in line and int(line.split("\t")[1]) <= 521 <= int(line.split("\t")[7][4:])
               for line in data)
    # every block equals the restatement over the decoded reads of its chromosome, cut differently
    small = gvcf.write_gvcf(vcf_path, [bam], fa, str(tmp_path / "small.g.vcf"), restatement=True, max_span=256)
    assert open(small, "rb").read() == open(out, "rb").read()
    # only some chromosomes: the records of the others stay, without blocks
    part = gvcf.write_gvcf(vcf_path, [bam], fa, str(tmp_path / "part.g.vcf"), chromosomes=["chrA"], restatement=True)
    got = [line for line in open(part).read().splitlines(keepends=True) if not line.startswith("#")]
    assert [line for line in got if line.startswith("chrA\t")] == [line for line in data if line.startswith("chrA\t")]
    assert [line for line in got if not line.startswith("chrA\t")] == records[-1:]


# ---- the driver's refusals --------------------------------------------------------------------------------------------------
def _args(*extra):
    return call.parser().parse_args(["--workdir", "w", "--network", "m.npz"] + list(extra))


def test_gvcf_needs_a_bam_route(monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit, match="--from_bam .*or --from_bams"):
        call.main(_args("--shards", "s", "--gvcf"))
    with pytest.raises(SystemExit, match="--gpus 1"):
        call.main(_args("--from_bam", "--ibam", "x.bam", "--ref", "g.fa", "--gvcf", "--gpus", "2"))
    with pytest.raises(SystemExit, match="--gpus 1"):
        call.main(_args("--from_bams", "--resident", "--ibam", "x.bam", "--pbam", "y.bam", "--ref", "g.fa", "--gvcf", "--gpus", "2"))
    with pytest.raises(SystemExit, match="gvcf_gq_binsize"):
        call.main(_args("--from_bam", "--ibam", "x.bam", "--ref", "g.fa", "--gvcf", "--gvcf_gq_binsize", "0"))
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process on one GPU"):
        call.main(_args("--from_bam", "--ibam", "x.bam", "--ref", "g.fa", "--gvcf"))


def test_without_the_flag_nothing_is_checked_or_written():
    args = _args("--shards", "s")
    assert args.gvcf is False and args.gvcf_gq_binsize == 5
    call.check_gvcf(args)
    assert call.gvcf_pass(args, "w/results.output.vcf", {}) is None
