"""Contamination and identity without a GPU (hello_amd/contamination.py): the plain-Python restatement of the
pileup against the tables worked by hand (tests/contamination_cases.py), the sites file, the host-only estimates of the built library
(hello_amd/csrc/contam.h) against the restatement evaluated in long double, planted mixtures, the files' exact text, the refusals of
``call --contamination`` and the C ABI -- declarations, exports and the host-side validation, which needs no device."""
import ctypes as C
import dataclasses
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hello_amd import call, contamination as cn
from tests import contamination_cases as cc
from tests.test_stage_host import one_read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def same_counts(got, want):
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


def spans_of(case, cuts):
    edges = [0] + list(cuts) + [len(case.reference)]
    return [(cc.read_set(cc.overlapping(case.rows, lo, hi)), lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]


# ---- the restatement of the pileup ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.HAND_TABLE, ids=[c.name for c in cc.HAND_TABLE])
def test_restatement_equals_the_hand_table(case):
    for cuts in ((), (case.cut(),)):                                            # whole, and cut through the first read
        got, counts = cn.restated(spans_of(case, cuts), case.sites, len(case.reference))
        same_counts(got["COUNTS"], case.expected())
        assert {k: counts[k] for k in cn.METRIC_STATS} == case.want_counts()
    assert counts["reads_given"] > len(case.rows)                              # the read that was cut is given twice


def test_the_hand_table_names_every_rule():
    names = " / ".join(c.name for c in cc.HAND_TABLE)
    for rule in ("each base on each strand", "q_threshold - 1 and at q_threshold", "mapq at the threshold and below", "each filter flag",
                 "an insertion before a site", "D over a site", "N over a site", "a soft clip where a site would be", "= and X",
                 "a lower-case and a non-ACGT byte", "first and last aligned base", "without a CIGAR", "positions 0 and 199",
                 "bit 63 of a word and at bit 0 of the next", "two adjacent sites", "starts in one span and observes a site in the next"):
        assert rule in names, rule
    assert len(cc.REF) == 200 and all(len(c.reference) == 200 for c in cc.HAND_TABLE)
    assert {0, 199, 63, 64, 10, 11} <= set(cc.SITES) and cn.BINS == ("A", "C", "G", "T", "OTHER", "DEL", "LOWQ")
    with pytest.raises(ValueError, match="does not consume exactly"):
        cn.tables_of(one_read([(0, 5)], 4), cc.SITES, 200, 0, 200)
    with pytest.raises(ValueError, match="leaves the reference"):
        cn.tables_of(one_read([(0, 5)], 5), cc.SITES, 200, 0, 201)


# ---- the sites file -------------------------------------------------------------------------------------------------------------
SITES_VCF = "\n".join([
    "##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO",
    "chr1\t21\t.\tA\tC\t.\t.\tAF=0.25",                       # position 20 holds A: a site
    "chr1\t3\t.\tg\tt\t.\t.\tDP=9;AF=0.5;X",                  # lower case, AF among other keys, before the first in position
    "chr1\t5\t.\tAC\tA\t.\t.\tAF=0.1",                        # not_snv: a deletion
    "chr1\t6\t.\tC\tN\t.\t.\tAF=0.1",                         # not_snv: N
    "chr1\t7\t.\tG\tA,T\t.\t.\tAF=0.1,0.2",                   # multiallelic
    "chr1\t8\t.\tT\tA\t.\t.\tDP=3",                           # no_af
    "chr1\t9\t.\tA\tC\t.\t.\tAF=x",                           # no_af: no number
    "chr1\t10\t.\tC\tA\t.\t.\tAF=0",                          # af_out_of_range
    "chr1\t11\t.\tG\tA\t.\t.\tAF=1.0",                        # af_out_of_range
    "chr1\t12\t.\tA\tC\t.\t.\tAF=0.3",                        # ref_mismatch: position 11 holds T
    "chr1\t201\t.\tA\tC\t.\t.\tAF=0.3",                       # ref_mismatch: behind the end
    "chr9\t1\t.\tA\tC\t.\t.\tAF=0.3",                         # unknown_chromosome
    "chr1\t21\t.\tA\tG\t.\t.\tAF=0.75",                       # duplicate_position: the first stays
    "chr1\t200\t.\tT\tC\t.\t.\tAF=1e-6",                      # the last position
    "chr2\t1\t.\tA\tT\t.\t.\tAF=0.999999", ""])


def test_read_sites_keeps_the_sites_and_counts_every_other_record_by_cause(tmp_path):
    genome = {"chr1": cc.REF, "chr2": "acgt"}
    plain, zipped = str(tmp_path / "s.vcf"), str(tmp_path / "s.vcf.gz")
    open(plain, "w").write(SITES_VCF)
    with gzip.open(zipped, "wt") as fh:
        fh.write(SITES_VCF)
    for path in (plain, zipped):
        s = cn.read_sites(path, genome)
        assert s.records == 15 and s.n_sites == 4
        assert s.skipped == dict(not_snv=2, multiallelic=1, no_af=2, af_out_of_range=2, ref_mismatch=2, unknown_chromosome=1,
                                 duplicate_position=1) and tuple(s.skipped) == cn.SKIP_CAUSES
        one, two = s.per_chromosome["chr1"], s.per_chromosome["chr2"]
        assert one["POS"].tolist() == [2, 20, 199] and one["POS"].dtype == np.int64
        assert one["REF"].tolist() == [2, 0, 3] and one["ALT"].tolist() == [3, 1, 1] and one["REF"].dtype == np.uint8
        assert one["AF"].tolist() == [0.5, 0.25, 1e-6] and one["AF"].dtype == np.float64
        assert (two["POS"].tolist(), two["REF"].tolist(), two["ALT"].tolist(), two["AF"].tolist()) == ([0], [0], [3], [0.999999])
    only = cn.read_sites(plain, genome, ["chr2"])                              # the chromosomes of the run
    assert list(only.per_chromosome) == ["chr2"] and only.skipped["unknown_chromosome"] == 14 and only.n_sites == 1
    open(plain, "w").write("chr1\t5\t.\tA\n")
    with pytest.raises(ValueError, match="a record of 4 fields"):
        cn.read_sites(plain, genome)


# ---- the estimates of the library against long double ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,depth,seed,alpha", [(200, 30, 1, 0.05), (2000, 300, 2, 0.02), (500, 3000, 3, 0.2)])
def test_the_library_equals_the_restatement_in_long_double(n, depth, seed, alpha):
    """For every k, |LL_lib[k] - LL_ld[k]| <= (n + 32) 2^-53 sum_i (|l_ik| + 1): the textbook bound for a sum of n terms, each good to
    32 ulp.  Measured here: 0.05, 0.016 and 0.03 of the bound.  The inputs are chosen so that the greatest LL and the interval's
    ends are decided by margins of 10^6 bounds and more, which the first assert keeps true for a later edit."""
    r, a, o, af, _ = cc.planted(seed, alpha, n, depth)
    ld = cn.estimate_restated(r, a, o, af, np.longdouble)
    used = ld["n_used"]
    assert used > 0.9 * n and ld["LL"].dtype == np.longdouble
    bound = (used + 32) * 2.0 ** -53 * (ld["abs_sum"] + used)
    ranked = np.sort(ld["LL"])[::-1]
    assert ranked[0] - ranked[1] > 1000 * bound.max() and np.abs(ld["LL"] - (ranked[0] - cn.DROP)).min() > 1000 * bound.max()
    got = cn.estimate_native(r, a, o, af)
    error = np.abs(got["LL"].astype(np.longdouble) - ld["LL"])
    print("n %d depth %d: max |LL_lib - LL_ld| / bound = %.4f" % (n, depth, float((error / bound).max())))
    assert (error <= bound).all(), float((error / bound).max())
    assert (got["k"], got["k_lo"], got["k_hi"]) == (ld["k"], ld["k_lo"], ld["k_hi"]) and got["error_rate"] == ld["error_rate"]
    assert got["k_lo"] <= round(alpha * 1000) <= got["k_hi"]
    plain = cn.estimate_restated(r, a, o, af)                                  # float64 NumPy: the files of the restatement
    assert (plain["k"], plain["k_lo"], plain["k_hi"]) == (got["k"], got["k_lo"], got["k_hi"])
    # the LOD of the same counts against themselves, by the same bound over its three sums
    lod_ld, used_ld = cn.identity_restated(r, a, o, r, a, o, af, np.longdouble)
    lod, used_lib = cn.identity_native(r, a, o, r, a, o, af)
    assert used_lib == used_ld == used and lod > 0
    assert abs(np.longdouble(lod) - lod_ld) <= 3 * (used + 32) * 2.0 ** -53 * (abs(lod_ld) + ld["abs_sum"][0] * 2 + used)


# Seeds 0 .. 5 were drawn for every alpha with the NumPy restatement alone, 24 draws in all; one interval of the 24 missed its truth
# (alpha 0, seed 2: [0.001, 0.010]), as about one 95 % interval in twenty does.  Seeds 0 and 1 are kept for every alpha.
@pytest.mark.parametrize("alpha", [0.0, 0.02, 0.05, 0.2])
@pytest.mark.parametrize("seed", [0, 1])
def test_planted_mixtures_come_back_inside_their_interval(seed, alpha):
    r, a, o, af, _ = cc.planted(seed, alpha)                                   # 200 sites, depth Poisson 30, error 0.004
    got, want = cn.estimate_native(r, a, o, af), cn.estimate_restated(r, a, o, af)
    assert got["k_lo"] <= round(alpha * 1000) <= got["k_hi"], (got["k_lo"], got["k"], got["k_hi"])
    assert got["k_lo"] <= got["k"] <= got["k_hi"] and got["k_hi"] - got["k_lo"] < 100
    assert (got["k"], got["k_lo"], got["k_hi"], got["error_rate"]) == (want["k"], want["k_lo"], want["k_hi"], want["error_rate"])
    assert np.allclose(got["LL"], want["LL"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_identity_tells_the_same_genotypes_from_independent_ones(seed):
    r1, a1, o1, af, genotypes = cc.planted(seed, 0.0, 200, 30)
    r2, a2, o2, af2, _ = cc.planted(seed, 0.0, 200, 10, genotypes=genotypes)   # the same person at depth 10
    r3, a3, o3, _, _ = cc.planted(seed + 100, 0.0, 200, 10)                    # another one
    assert np.array_equal(af, af2)
    same, used = cn.identity_native(r1, a1, o1, r2, a2, o2, af)
    assert same > 0 and used > 190 and cn.verdict(same, used) == "same_sample"
    other, used = cn.identity_native(r1, a1, o1, r3, a3, o3, af)
    assert other < 0 and cn.verdict(other, used) == "different_sample"
    for args in ((r1, a1, o1, r2, a2, o2, af), (r1, a1, o1, r3, a3, o3, af)):
        lod, n = cn.identity_restated(*args)
        assert n == cn.identity_native(*args)[1] and abs(lod - cn.identity_native(*args)[0]) < 1e-9 * abs(lod)
    assert cn.verdict(0.0, 5) == cn.verdict(3.0, 0) == "undetermined"


def test_degenerate_inputs_stay_finite():
    z = np.zeros(0, np.int64)
    big = 2 ** 31 - 1
    cases = [(z, z, z, np.zeros(0)), (np.zeros(3, np.int64),) * 3 + (np.array([0.1, 0.5, 0.9]),), ([30], [0], [0], [0.3]),
             ([big, 0, big], [0, big, big], [0, 0, 7], [0.5, 0.5, 0.5]), ([30, 0, 12], [0, 30, 14], [0, 1, 0], [1e-6, 1 - 1e-6, 0.5])]
    for r, a, o, af in cases:
        for f in (cn.estimate_native, cn.estimate_restated):
            e = f(r, a, o, af)
            assert np.isfinite(e["LL"]).all() and np.isfinite(e["error_rate"]) and 0 <= e["k_lo"] <= e["k"] <= e["k_hi"] <= 500
            lod, used = (cn.identity_native if f is cn.estimate_native else cn.identity_restated)(r, a, o, r, a, o, af)
            assert np.isfinite(float(lod)) and used == e["n_used"]
    flat = cn.estimate_native(z, z, z, np.zeros(0))
    assert (flat["error_rate"], flat["k"], flat["k_lo"], flat["k_hi"]) == (1e-4, 0, 0, 500) and not flat["LL"].any()
    assert cn.identity_native(z, z, z, z, z, z, np.zeros(0)) == (0.0, 0)
    assert cn.error_rate([90, 0], [0, 90], [10, 10]) == 0.1 and cn.error_rate([90, 0], [0, 90], [1, 1]) == 1.5 * 2.0 / 182.0
    lib = cn._lib()
    one, af = np.array([-1], np.int64), np.array([0.5])
    out = np.zeros(505)
    assert lib.hello_contam_estimate(one.ctypes.data, one.ctypes.data, one.ctypes.data, af.ctypes.data, 1, out.ctypes.data) == ERR_ARG
    assert lib.hello_last_error().decode() == "site 0: count -1"
    one[0] = 1
    for bad in (0.0, 1.0, float("nan")):
        af[0] = bad
        assert lib.hello_contam_estimate(one.ctypes.data, one.ctypes.data, one.ctypes.data, af.ctypes.data, 1, out.ctypes.data) == ERR_ARG
        assert "is not inside (0, 1)" in lib.hello_last_error().decode()
    assert lib.hello_contam_estimate(None, None, None, None, 1, out.ctypes.data) == ERR_ARG
    assert lib.hello_contam_identity(None, None, None, None, None, None, None, 0, None) == ERR_ARG


# ---- files ----------------------------------------------------------------------------------------------------------------------
def small_contamination(native=True):
    sites = cn.Sites(["chr1", "chr2"])
    sites.records, sites.skipped["no_af"], sites.skipped["ref_mismatch"] = 7, 2, 1
    m = cn.Contamination(sites, native=native)
    counts = np.zeros((3, 2, 7), np.int64)
    counts[0, 0, [cc.A, cc.C, cc.G, cc.LOWQ]] = [10, 2, 1, 3]                  # REF A, ALT C
    counts[0, 1, [cc.A, cc.OTHER, cc.DEL]] = [9, 1, 2]
    counts[2, 1, cc.T] = 4                                                      # REF T, ALT G: the middle site has no coverage
    m.set("chr1", dict(POS=[2, 20, 199], REF=[0, 1, 3], ALT=[1, 2, 2], AF=[0.25, 0.5, 1e-6]), counts,
          dict(dict.fromkeys(cn.COUNT_NAMES, 0), belonging=9, counting=7, reads_on_a_site=6, observations=32, n_sites=3))
    m.set("chr2", dict(POS=[], REF=[], ALT=[], AF=[]), np.zeros((0, 2, 7), np.int64), dict.fromkeys(cn.COUNT_NAMES, 0))
    return m


def test_save_load_and_the_exact_text_of_the_files(tmp_path):
    m = small_contamination()
    r, a, o, af = m.arrays()
    assert (r.tolist(), a.tolist(), o.tolist(), af.tolist()) == ([19, 0, 4], [2, 0, 0], [1, 0, 0], [0.25, 0.5, 1e-6])
    est = m.estimate()
    assert est["error_rate"] == 1.5 * 1 / 26 and est["n_used"] == 2
    files = m.write_all(str(tmp_path / "contamination.illumina"))
    assert [os.path.basename(f) for f in files] == ["contamination.illumina.txt", "contamination.illumina.pileup.tsv", "contamination.illumina.npz"]
    assert open(files[0]).read() == (
        "sites_read\t7\nsites_skipped_not_snv\t0\nsites_skipped_multiallelic\t0\nsites_skipped_no_af\t2\nsites_skipped_af_out_of_range\t0\n"
        "sites_skipped_ref_mismatch\t1\nsites_skipped_unknown_chromosome\t0\nsites_skipped_duplicate_position\t0\nsites\t3\n"
        "sites_with_coverage\t2\nreads_not_counted\t2\nreads_counting\t7\nreads_on_a_site\t6\nobservations\t32\nerror_rate\t0.057692\n"
        "contamination\t%.3f\ncontamination_lo\t%.3f\ncontamination_hi\t%.3f\nmean_depth_at_sites\t10.667\n"
        % (est["k"] / 1000, est["k_lo"] / 1000, est["k_hi"] / 1000))
    assert 0 <= est["k_lo"] <= est["k"] <= est["k_hi"] <= 500
    assert open(files[1]).read() == (
        "#chrom\tpos\tref\talt\taf\tref_fwd\tref_rev\talt_fwd\talt_rev\tother\tdeletions\tlow_quality\n"
        "chr1\t3\tA\tC\t0.25\t10\t9\t2\t0\t2\t2\t3\nchr1\t200\tT\tG\t1e-06\t0\t4\t0\t0\t0\t0\t0\n")
    loaded = cn.Contamination.load(files[2])
    assert list(loaded.tables) == ["chr1", "chr2"] and loaded.total() == m.total() and loaded.total()["observations"] == 32
    assert loaded.skipped == m.skipped and loaded.records == 7
    for name in ("POS", "REF", "ALT", "AF", "COUNTS", "STATS"):
        assert np.array_equal(loaded.tables["chr1"][name], m.tables["chr1"][name]) and loaded.tables["chr1"][name].dtype == m.tables["chr1"][name].dtype
    for x, y in zip(files, loaded.write_all(str(tmp_path / "again"))):
        assert open(x, "rb").read() == open(y, "rb").read()
    assert small_contamination(native=False).report() == m.report()            # the restatement writes the same text
    # the identity file: these counts against themselves, against nothing, and at other sites
    assert cn.identity_of(m, m)[1:] == (2, "same_sample")
    path = cn.write_identity(str(tmp_path / "contamination.identity.txt"), m, m)
    assert open(path).read() == "sites_used\t2\nlod\t%.3f\nverdict\tsame_sample\n" % cn.identity_of(m, m)[0]
    empty = small_contamination()
    empty.tables["chr1"]["COUNTS"] = np.zeros((3, 2, 7), np.int64)
    assert cn.identity_text(*cn.identity_of(m, empty)) == "sites_used\t0\nlod\t0.000\nverdict\tundetermined\n"
    empty.tables["chr1"]["AF"] = np.array([0.25, 0.5, 0.5])
    with pytest.raises(ValueError, match="not measured at the same sites"):
        cn.identity_of(m, empty)


# ---- the refusals and the flags -------------------------------------------------------------------------------------------------
def _args(*extra):
    return call.parser().parse_args(["--workdir", "w", "--network", "m.npz"] + list(extra))


def test_refusals_of_contamination_name_the_fix(monkeypatch):
    bam = ["--ibam", "i.bam", "--ref", "g.fa"]
    on = ["--contamination", "--contamination_sites", "s.vcf"]
    with pytest.raises(SystemExit, match="add --contamination, or drop --contamination_sites"):
        call.check_contamination(_args("--from_bam", "--contamination_sites", "s.vcf", *bam))
    with pytest.raises(SystemExit, match="add --contamination_sites with a VCF"):
        call.check_contamination(_args("--from_bam", "--contamination", *bam))
    with pytest.raises(SystemExit, match="drop --shards"):
        call.check_contamination(_args("--from_bam", "--shards", "s", *on, *bam))
    with pytest.raises(SystemExit, match="add --from_bam .*or --from_bams"):
        call.check_contamination(_args(*on, *bam))
    with pytest.raises(SystemExit, match="--gpus 1"):
        call.check_contamination(_args("--from_bam", "--gpus", "2", *on, *bam))
    with pytest.raises(SystemExit, match="--contamination"):
        call.main(_args("--shards", "s", *on))
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="plain command"):
        call.check_contamination(_args("--from_bam", *on, *bam))
    monkeypatch.delenv("RANK")
    call.check_contamination(_args("--from_bam", *on, *bam))
    call.check_contamination(_args("--from_bams", "--resident", "--pbam", "p.bam", *on, *bam))
    call.check_contamination(_args("--shards", "s"))
    plain = _args("--shards", "s")
    assert plain.contamination is False and plain.contamination_sites is None and call.contamination_pass(plain, {}) == []
    argv = call._argv_of(_args(*on))
    assert "--contamination" in argv and argv[argv.index("--contamination_sites") + 1] == "s.vcf" and "--contamination" not in call._argv_of(plain)
    args = cn.parser().parse_args(["--bam", "b.bam,p.bam", "--ref", "g.fa", "--sites", "s.vcf", "--output_prefix", "p", "--chromosomes",
                                   "a,b", "--q_threshold", "7", "--mapq_threshold", "3", "--device", "1"])
    assert (args.bam, args.ref, args.sites, args.output_prefix, args.chromosomes, args.q_threshold, args.mapq_threshold, args.device) == \
        ("b.bam,p.bam", "g.fa", "s.vcf", "p", "a,b", 7, 3, 1)


def test_contamination_is_cleared_for_pass_1_of_haplotag(monkeypatch):
    seen = []
    monkeypatch.setattr(call, "main", lambda args: seen.append(args) or os.path.join(args.workdir, "results.output.vcf"))
    args = _args("--from_bam", "--pbam", "p.bam", "--ref", "g.fa", "--include_hp", "--haplotag", "--contamination", "--contamination_sites", "s.vcf")
    call.haplotag_passes(args)
    first, second = seen
    assert (first.contamination, first.contamination_sites) == (False, None)
    assert (second.contamination, second.contamination_sites) == (True, "s.vcf") and args.contamination is True


def test_the_route_measures_every_bam_at_its_thresholds_and_names_the_files(monkeypatch, tmp_path):
    calls = []

    def measure(bam, genome, chromosomes, sites, q_threshold, mapq_threshold, device, stats):
        calls.append((bam, tuple(chromosomes), sites.n_sites, q_threshold, mapq_threshold, device))
        return small_contamination()
    monkeypatch.setattr(cn, "measure", measure)
    work, vcf = str(tmp_path / "w"), str(tmp_path / "s.vcf")
    os.makedirs(work)
    open(vcf, "w").write(SITES_VCF)
    tail = ["--workdir", work, "--network", "m.npz", "--ref", "g.fa", "--contamination", "--contamination_sites", vcf]
    both = call.parser().parse_args(tail + ["--from_bams", "--ibam", "i.bam", "--pbam", "p.bam", "--mapq_threshold", "3", "--q_threshold", "7"])
    written = call.contamination_pass(both, {"chr1": cc.REF})
    assert calls == [("i.bam", ("chr1",), 3, 7, 3, 0), ("p.bam", ("chr1",), 3, 7, 3, 0)]
    names = ["contamination.illumina.txt", "contamination.illumina.pileup.tsv", "contamination.illumina.npz", "contamination.pacbio.txt",
             "contamination.pacbio.pileup.tsv", "contamination.pacbio.npz", "contamination.identity.txt"]
    assert [os.path.basename(f) for f in written] == names and sorted(os.listdir(work)) == sorted(names)
    del calls[:]
    one = call.parser().parse_args(tail + ["--from_bam", "--pbam", "p.bam", "--chromosomes", "chr1"])
    written = call.contamination_pass(one, {"chr1": cc.REF, "chr2": "ACGT"})
    assert calls == [("p.bam", ("chr1",), 3, 10, 10, 0)]                        # --from_bam: the defaults
    assert [os.path.basename(f) for f in written] == names[3:6]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("hello_pileup_create", "hello_pileup_option", "hello_pileup_add", "hello_pileup_array", "hello_pileup_stats",
           "hello_contam_estimate", "hello_contam_identity")


def test_abi_symbols_are_declared_exported_and_mirrored():
    from hello_amd.engine import load_library
    header = open(os.path.join(ROOT, "include", "hello_mi355x.h")).read()
    lib = load_library()
    for symbol in SYMBOLS:
        assert re.search(r"^int %s\(" % symbol, header, flags=re.M), symbol
        assert hasattr(lib, symbol), symbol
    assert re.search(r"^void hello_pileup_free\(", header, flags=re.M) and hasattr(lib, "hello_pileup_free")
    assert int(re.search(r"#define HELLO_PILEUP_STATS (\d+)", header).group(1)) == len(cn.STAT_NAMES) == 8
    assert int(re.search(r"#define HELLO_PILEUP_BINS (\d+)", header).group(1)) == len(cn.BINS) == 7
    assert int(re.search(r"#define HELLO_CONTAM_GRID (\d+)", header).group(1)) == cn.GRID == 501
    assert int(re.search(r"#define HELLO_CONTAM_OUT (\d+)", header).group(1)) == cn.GRID + 4
    for which, name in enumerate(("COUNTS", "STATUS")):
        assert int(re.search(r"HELLO_PILEUP_%s = (\d+)" % name, header).group(1)) == which
    assert re.search(r"#define HELLO_ABI_VERSION 2\b", header)
    bound = cn._lib()
    assert len(bound.hello_pileup_add.argtypes) == 15 and len(bound.hello_pileup_create.argtypes) == 7 and bound.hello_pileup_free.restype is None
    assert len(bound.hello_contam_estimate.argtypes) == 6 and len(bound.hello_contam_identity.argtypes) == 9
    assert cn.MAX_COUNTING_READS == 2 ** 31 - 1 and cn.MAX_SHARE == 1024
    assert re.search(r"HELLO_PILEUP_FORM = 0, HELLO_PILEUP_SHARE = 1", header)
    makefile = open(os.path.join(ROOT, "hello_amd", "csrc", "Makefile")).read()
    assert " pileup.hip" in re.search(r"^SRCS = (.*)$", makefile, flags=re.M).group(1)
    text = open(os.path.join(ROOT, "hello_amd", "csrc", "contam.h")).read()    # the estimates are plain C++: no HIP in them
    assert "hip/hip_runtime.h" not in text and "__global__" not in text and "stage_host.h" not in text


def test_the_host_code_is_clean_under_sanitizers(tmp_path):
    """cigar.h's pileup_walk and contam.h as a stand-alone host program under AddressSanitizer and UBSan
    (tests/abi/contam_check.cpp), degenerate inputs included."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler on this box"
    exe = str(tmp_path / "contam_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                            "-pthread", os.path.join(ROOT, "tests", "abi", "contam_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "contam_check: ok" in run.stdout, (run.returncode, run.stdout, run.stderr[-3000:])


POS = np.array([0, 10, 11, 199], np.int64)


def call_add(rd, lo=0, hi=200, handle=None):
    lib, h = cn._lib(), handle or C.c_void_p()
    if not handle:
        assert lib.hello_pileup_create(POS.ctypes.data, 4, 200, 10, 10, 0, C.byref(h)) == 0      # needs no device
    rc = lib.hello_pileup_add(h, *rd.pointers(rd.hp), rd.n_reads, lo, hi)
    said = lib.hello_last_error().decode()
    if not handle:
        lib.hello_pileup_free(h)
    return rc, said


def two_reads():
    return cc.read_set([(1, 0, 10, cc.M4, "ACGT", [30] * 4, 60), (2, 0, 12, cc.M4, "ACGT", [30] * 4, 60)])


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
]


@pytest.mark.parametrize("wrong,message", REFUSALS, ids=[r[1][:34].strip() + ("-%d" % i) for i, r in enumerate(REFUSALS)])
def test_add_refuses_before_it_looks_for_a_device(wrong, message):
    wrong = dict(wrong)
    rd = one_read(**wrong.pop("read")) if "read" in wrong else dataclasses.replace(two_reads(), **wrong.pop("change", {}))
    assert call_add(rd, **wrong) == (ERR_ARG, message)


CREATE_REFUSALS = [
    (dict(pos=[0, 10, 10]), "site 2: position 10 is not above 10 before it"),
    (dict(pos=[5, 3]), "site 1: position 3 is not above 5 before it"),
    (dict(pos=[-1, 3]), "site 0: position -1 of a chromosome of 200 bases"),
    (dict(pos=[3, 200]), "site 1: position 200 of a chromosome of 200 bases"),
    (dict(pos=[3], length=-1), "chromosome of -1 bases: 0 to 2147483647"),
    (dict(pos=[3], length=1 << 31), "chromosome of 2147483648 bases: 0 to 2147483647"),
    (dict(pos=[3], n=-1), "negative count"),
    (dict(pos=None, n=2), "NULL pointer"),
]


@pytest.mark.parametrize("wrong,message", CREATE_REFUSALS, ids=[r[1][:30].strip() + ("-%d" % i) for i, r in enumerate(CREATE_REFUSALS)])
def test_create_refuses_what_it_cannot_index_with(wrong, message):
    lib, h = cn._lib(), C.c_void_p()
    pos = None if wrong["pos"] is None else np.array(wrong["pos"], np.int64)
    n = wrong.get("n", 0 if pos is None else pos.shape[0])
    assert lib.hello_pileup_create(None if pos is None else pos.ctypes.data, n, wrong.get("length", 200), 10, 10, 0, C.byref(h)) == ERR_ARG
    assert lib.hello_last_error().decode() == message and not h.value


def test_host_side_validation_needs_no_device():
    lib = cn._lib()
    error = lambda: lib.hello_last_error().decode()      # noqa: E731
    h = C.c_void_p()
    assert lib.hello_pileup_create(POS.ctypes.data, 4, 200, 10, 10, 0, None) == ERR_ARG and "NULL pointer" in error()
    assert lib.hello_pileup_add(None, *([None] * 11), 0, 0, 0) == ERR_ARG and "NULL pointer" in error()
    assert lib.hello_pileup_stats(None, (C.c_double * 8)()) == ERR_ARG and "NULL pointer" in error()
    assert lib.hello_pileup_option(None, 0, 0) == ERR_ARG and "NULL pointer" in error()
    p, n = C.c_void_p(), C.c_int64()
    assert lib.hello_pileup_array(None, 0, C.byref(p), C.byref(n)) == ERR_ARG and "NULL pointer" in error()
    # a read that is not counted is not looked at: what the call answers then needs a device or needs none
    rc, said = call_add(one_read([(0, 5)], 4, flag=0x200))
    assert rc in (0, -5) and "read 0" not in said
    # a refused add leaves the handle where it was: the next span may still begin at 0; an empty site list is a handle too
    assert lib.hello_pileup_create(POS.ctypes.data, 4, 200, 10, 10, 0, C.byref(h)) == 0
    assert call_add(one_read([(0, 5)], 4), handle=h) == (ERR_ARG, "read 0: CIGAR query length 5, 4 bases")
    assert call_add(two_reads(), lo=0, hi=300, handle=h)[0] == ERR_ARG
    st = (C.c_double * 8)()
    assert lib.hello_pileup_stats(h, st) == 0 and list(st) == [0.0] * 5 + [4.0, 0.0, 0.0]
    assert lib.hello_pileup_array(h, 1, C.byref(p), C.byref(n)) == 0 and n.value == 0       # STATUS: no add yet
    assert lib.hello_pileup_array(h, 2, C.byref(p), C.byref(n)) == ERR_ARG and "array selector 2" in error()
    assert lib.hello_pileup_option(h, 2, 0) == ERR_ARG and "option 2" in error()
    assert lib.hello_pileup_option(h, 1, 1025) == ERR_ARG and "share 1025: 0 (sized by the launch) to 1024" in error()
    assert lib.hello_pileup_option(h, 1, -1) == ERR_ARG and lib.hello_pileup_option(h, 1, 1024) == 0 and lib.hello_pileup_option(h, 1, 0) == 0
    assert lib.hello_pileup_option(h, 0, 2) == ERR_ARG and "form 2" in error()
    assert lib.hello_pileup_option(h, 0, 1) == 0 and lib.hello_pileup_option(h, 0, 0) == 0
    lib.hello_pileup_free(h)
    empty = C.c_void_p()
    assert lib.hello_pileup_create(None, 0, 200, 10, 10, 0, C.byref(empty)) == 0 and empty.value
    lib.hello_pileup_free(empty)
