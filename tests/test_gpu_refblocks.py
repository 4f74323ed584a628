"""Reference-confidence blocks on the GPU (hello_refblocks_find, hello_amd/csrc/refblocks.hip): the per-position counters and every
field of every block equal the restatement of hello_amd/gvcf.py exactly -- on the table of cases worked by hand, and on a span of
3 tiles + 17 positions that is not aligned to a tile (tests/gvcf_cases.py); ``python -m hello_amd.call --gvcf`` writes the file the
restatement writes and leaves results.output.vcf as it was.  The seed was chosen with the restatement on the CPU so that the
conditions asserted in ``tile_case`` hold."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hello_amd import gvcf
from tests import gvcf_cases as gc
from tests.test_gvcf import covered

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 3
LO, HI = gc.SPAN_LO, gc.SPAN_LO + gc.SPAN


def same_blocks(got, want):
    for name, _, dtype in gvcf.FIELDS:
        assert got[name].dtype == dtype and got[name].tolist() == want[name].tolist(), name


# ---- (a) the hand table through host arrays ---------------------------------------------------------------------------------
def test_hand_table_counts_and_blocks():
    for case in gc.HAND_TABLE:
        lo, hi = case.span()
        reads = gc.reads_of(case.reads)
        blocks, stats, (n_ref, n_total) = gvcf.find_blocks([reads], case.reference, lo, hi, keep_counts=True)
        assert n_ref.tolist() == case.n_ref and n_total.tolist() == case.n_total, case.name
        same_blocks(blocks, gvcf.blocks_of(case.n_ref, case.n_total, (), 5, lo))
        assert stats["tiles"] == 1 and stats["blocks"] == blocks["start"].shape[0], case.name


def test_bands_and_first_minimum_through_the_kernel():
    """Depths 1 to 40 of reference reads side by side: every GQ from 3 to the cap, banded by 1, 5 and 10; then the tie of
    test_the_first_position_of_the_smallest_gq_is_reported."""
    reference = "ACGT" * 12
    records = [(p, [(gc.M, 48 - p)], reference[p:], [30] * (48 - p), 0, 60) for p in range(40)]        # depth p + 1 at p < 40
    for binsize in (1, 5, 10):
        blocks, _, (n_ref, n_total) = gvcf.find_blocks([gc.reads_of(records)], reference, 0, 48, gq_binsize=binsize, keep_counts=True)
        assert n_total.tolist() == list(range(1, 41)) + [40] * 8 and n_ref.tolist() == n_total.tolist()
        same_blocks(blocks, gvcf.blocks_of(n_ref, n_total, (), binsize))
    # positions 0..3 at depth 11, 10, 20 (one mismatch), 11
    reference = "AAAA"
    tie = [(0, [(gc.M, 4)], "AAAA", [30] * 4, 0, 60)] * 10 + [(0, [(gc.M, 1)], "A", [30], 0, 60), (2, [(gc.M, 1)], "C", [30], 0, 60)] \
        + [(2, [(gc.M, 1)], "A", [30], 0, 60)] * 9 + [(3, [(gc.M, 1)], "A", [30], 0, 60)]
    tie.sort(key=lambda r: r[0])
    blocks, _, (n_ref, n_total) = gvcf.find_blocks([gc.reads_of(tie)], reference, 0, 4, keep_counts=True)
    assert n_ref.tolist() == [11, 10, 19, 11] and n_total.tolist() == [11, 10, 20, 11]
    assert [blocks[name].tolist() for name, _, _ in gvcf.FIELDS] == [[0], [4], [6], [10], [30], [10], [10]]


@pytest.mark.parametrize("dips", [(1010,), (1030,), (1010, 1030), (1023,), (1024,), (1023, 1024), ()])
def test_a_covered_block_across_a_tile_edge_takes_the_smaller_gq_and_the_earlier_position(dips):
    """Ten reads over [900, 1100) and an eleventh cut into pieces that leave out the positions of `dips`: one block of GQ band 6
    (GQ 33 at depth 11, 30 at depth 10) across the tile edge at 1024, whose reported position lies in either tile."""
    rng = np.random.default_rng(1)
    reference = "".join(rng.choice(list("ACGT"), size=1200))
    exact = lambda a, b: (a, [(gc.M, b - a)], reference[a:b], [30] * (b - a), 0, 60)     # noqa: E731
    edges = [900] + [x for d in dips for x in (d, d + 1)] + [1100]
    records = [exact(900, 1100)] * 10 + [exact(a, b) for a, b in zip(edges[::2], edges[1::2]) if b > a]
    records.sort(key=lambda r: r[0])
    blocks, stats, (n_ref, n_total) = gvcf.find_blocks([gc.reads_of(records)], reference, 0, 1200, keep_counts=True)
    assert n_total[900:1100].tolist() == [10 if p in dips else 11 for p in range(900, 1100)] and not n_total[:900].any()
    want = gvcf.blocks_of(n_ref, n_total, (), 5)
    assert want["start"].tolist() == [0, 900, 1100] and want["gq"].tolist() == [0, 30 if dips else 33, 0]
    same_blocks(blocks, want)
    assert stats["tiles"] == 2 and stats["runs"] == 4 and stats["blocks"] == 3


def test_refusals_before_the_launch():
    beyond = gc.reads_of([(0, [(gc.M, 5)], "ACGT", [30] * 4, 0, 60)])
    with pytest.raises(RuntimeError, match="consumes 5 bases, it has 4"):
        gvcf.find_blocks([beyond], "ACGTACGT", 0, 8)
    fine = gc.reads_of([(0, [(gc.M, 4)], "ACGT", [30] * 4, 0, 60)])
    with pytest.raises(RuntimeError, match="span"):
        gvcf.find_blocks([fine], "ACGTACGT", 0, 9)
    with pytest.raises(RuntimeError, match="excluded interval 1"):
        gvcf.find_blocks([fine], "ACGTACGT", 0, 8, excluded=[(2, 5), (4, 6)])
    with pytest.raises(RuntimeError, match="gq_binsize"):
        gvcf.find_blocks([fine], "ACGTACGT", 0, 8, gq_binsize=0)
    unsorted = gc.reads_of([(3, [(gc.M, 4)], "TACG", [30] * 4, 0, 60), (0, [(gc.M, 4)], "ACGT", [30] * 4, 0, 60)])
    with pytest.raises(RuntimeError, match="coordinate-sorted"):
        gvcf.find_blocks([unsorted], "ACGTACGT", 0, 8)
    blocks, stats, counts = gvcf.find_blocks([fine], "ACGTACGT", 3, 3, keep_counts=True)         # an empty span: nothing to do
    assert blocks["start"].shape == (0,) and stats["tiles"] == 0 and counts[0].shape == (0,)


# ---- (b) - (e) three tiles and 17 positions ---------------------------------------------------------------------------------
_tile: dict = {}


def tile_case():
    """The input and its restatement, computed once: (reference, the two read sets, n_ref, n_total, blocks)."""
    if not _tile:
        reference, short, long = gc.tile_input(SEED)
        sets = [gc.reads_of_bam_records(short), gc.reads_of_bam_records(long)]
        n_ref, n_total = gvcf.count_positions(sets, reference, LO, HI)
        blocks = gvcf.blocks_of(n_ref, n_total, gc.EXCLUDED, 5, LO)
        # the input exercises what the kernel can get wrong
        edges = [LO + gc.TILE * i for i in (1, 2, 3)]
        rows = list(zip(blocks["start"].tolist(), blocks["end"].tolist(), blocks["band"].tolist()))
        assert len({b for _, _, b in rows if b >= 0}) >= 3                                   # three distinct called bands
        assert any(b == gvcf.NO_CALL for _, _, b in rows)                                    # a no-call block
        assert any(s < edges[0] and e > edges[1] and b == gvcf.NO_CALL for s, e, b in rows)  # a block over a whole tile and two edges
        cut = (edges[2] - 3, edges[2] + 4)                                                   # an excluded interval over a tile edge
        assert cut in gc.EXCLUDED and any(e == cut[0] for _, e, _ in rows) and any(s == cut[1] for s, _, _ in rows)
        assert not n_total[gc.GAP[0] - LO:gc.GAP[1] - LO].any() and gc.GAP[1] - gc.GAP[0] > gc.TILE
        assert len(long) == 1 and len(long[0].cigar) > 64 and long[0].pos < LO and long[0].ref_end > HI
        assert reference[LO + 200:LO + 420].islower() and n_ref[200:420].sum() > 0.9 * n_total[200:420].sum() > 0   # soft-masked bases match
        assert 6 < n_total[:gc.TILE - 200].mean() < 12
        merged = gc.reads_of_bam_records(sorted(short + long, key=lambda r: r.pos))
        _tile.update(reference=reference, sets=sets, merged=merged, n_ref=n_ref, n_total=n_total, blocks=blocks)
    return _tile


def test_three_tiles_and_a_remainder_equal_the_restatement():
    t = tile_case()
    blocks, stats, (n_ref, n_total) = gvcf.find_blocks([t["merged"]], t["reference"], LO, HI, gc.EXCLUDED, keep_counts=True)
    assert np.array_equal(n_ref, t["n_ref"]) and np.array_equal(n_total, t["n_total"])
    same_blocks(blocks, t["blocks"])
    assert stats["tiles"] == 4 and stats["runs"] > stats["blocks"] == t["blocks"]["start"].shape[0]   # runs were joined at tile edges
    assert stats["reads_counted"] < t["merged"].n_reads                                               # the filter dropped some
    assert stats["kernel_ms"] > 0


def test_two_bams_count_into_the_same_counters():
    t = tile_case()
    blocks, _, (n_ref, n_total) = gvcf.find_blocks(t["sets"], t["reference"], LO, HI, gc.EXCLUDED, keep_counts=True)
    assert np.array_equal(n_ref, t["n_ref"]) and np.array_equal(n_total, t["n_total"])
    same_blocks(blocks, t["blocks"])


@pytest.mark.parametrize("cut", [LO + gc.TILE + 500, LO + 2 * gc.TILE, LO + 160, LO + 2270])
def test_two_launches_give_the_same_joined_blocks(cut):
    t = tile_case()
    assert any(s < cut < e for s, e in zip(t["blocks"]["start"].tolist(), t["blocks"]["end"].tolist()))   # a block crosses the cut
    parts = []
    for lo, hi in ((LO, cut), (cut, HI)):
        inside = [(a, b) for a, b in gc.EXCLUDED if b > lo and a < hi]
        parts.append(gvcf.find_blocks(t["sets"], t["reference"], lo, hi, inside)[0])
    same_blocks(gvcf.join_blocks(parts), t["blocks"])


def test_two_runs_give_the_same_bytes():
    t = tile_case()
    runs = [gvcf.find_blocks(t["sets"], t["reference"], LO, HI, gc.EXCLUDED, keep_counts=True) for _ in range(2)]
    for name, _, _ in gvcf.FIELDS:
        assert runs[0][0][name].tobytes() == runs[1][0][name].tobytes(), name
    assert runs[0][2][0].tobytes() == runs[1][2][0].tobytes() and runs[0][2][1].tobytes() == runs[1][2][1].tobytes()


# ---- the driver -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["illumina", "hybrid"])
def test_call_gvcf_writes_the_restatements_file_and_leaves_the_vcf(kind, tmp_path):
    from hello_amd import candidates as cd
    from tests.test_gpu_candidates import _fasta, _write
    from tests.test_gpu_hybrid_candidates import synthetic as hybrid_synthetic
    from tests.test_gpu_resident import HYBRID_SEED, _network, illumina_input
    hybrid = kind == "hybrid"
    if hybrid:
        reference, illumina, pacbio = hybrid_synthetic(HYBRID_SEED, 20000)
        bams = [_write(tmp_path, "i.bam", "chr1", reference, illumina), _write(tmp_path, "p.bam", "chr1", reference, pacbio)]
        route = ["--ibam", bams[0], "--pbam", bams[1], "--from_bams", "--resident", "--annotate_evidence"]
        thresholds = (10, 10)                                         # the driver's --q_threshold / --mapq_threshold defaults
    else:
        reference, reads = illumina_input()
        bams = [_write(tmp_path, "i.bam", "chr1", reference, reads)]
        route = ["--ibam", bams[0], "--from_bam"]
        thresholds = (cd.DEFAULT_Q_THRESHOLD, cd.DEFAULT_MIN_MAPQ)
    fa = _fasta(tmp_path, "chr1", reference)
    network, model = _network(tmp_path, hybrid)
    network.close()

    def run(extra, workdir):
        done = subprocess.run([sys.executable, "-m", "hello_amd.call", "--ref", fa, "--workdir", workdir, "--network", model] + route + extra,
                              cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0, done.stderr[-3000:]
    plain, with_gvcf = str(tmp_path / "w1"), str(tmp_path / "w2")
    run([], plain)
    run(["--gvcf"], with_gvcf)
    read = lambda *p: open(os.path.join(*p), "rb").read()      # noqa: E731
    vcf = read(with_gvcf, "results.output.vcf")
    assert vcf == read(plain, "results.output.vcf")
    assert not os.path.exists(os.path.join(plain, "results.output.g.vcf"))
    records = [line for line in vcf.splitlines(keepends=True) if not line.startswith(b"#")]
    assert records
    got = read(with_gvcf, "results.output.g.vcf")
    data = [line for line in got.splitlines(keepends=True) if not line.startswith(b"#")]
    assert [line for line in data if b"<NON_REF>" not in line] == records
    assert sum(b"<NON_REF>" in line for line in data) > len(records)
    want = gvcf.write_gvcf(os.path.join(plain, "results.output.vcf"), bams, fa, str(tmp_path / "want.g.vcf"), None, *thresholds, restatement=True)
    assert got == open(want, "rb").read()
    covered(os.path.join(with_gvcf, "results.output.g.vcf"), {"chr1": len(reference)})
