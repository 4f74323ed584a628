"""The pileup at sites on the GPU (hello_pileup_*; hello_amd/csrc/pileup.hip): COUNTS equal the restatement of
hello_amd/contamination.py integer for integer -- on the tables worked by hand (tests/contamination_cases.py), on an edge stress
whose reads cross the 64-base chunk, the 64-position word, the span edges and the edges of phase 1's compaction, on the fuzz corpus
of tests/read_fuzz.py against an independent count as well, and through the driver, where ``--contamination`` writes the files the
restatement writes and leaves the VCF alone."""
import dataclasses
import os

import numpy as np
import pytest

from hello_amd import call, contamination as cn, markdup
from tests import contamination_cases as cc, read_fuzz as rf
from tests.test_contamination import same_counts, spans_of

pytestmark = pytest.mark.gpu
MODEL_SEED = 1
FORMS = (cn.TWO_PHASE, cn.PLAIN)


# ---- (1) the hand tables through the kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.HAND_TABLE, ids=[c.name for c in cc.HAND_TABLE])
def test_hand_table_through_the_kernels(case):
    length, runs = len(case.reference), []
    for cuts, form, share in (((), 0, 0), ((case.cut(),), 0, 0), ((), 0, 0), ((case.cut(),), 0, 0), ((), 1, 0), ((case.cut(),), 1, 0),
                              ((), 0, 1), ((), 0, cn.MAX_SHARE), ((), 1, 3)):    # each twice; then plain; then other shares
        spans = spans_of(case, cuts)
        got, stats = cn.counted_on_gpu(spans, case.sites, length, form=form, share=share)
        same_counts(got["COUNTS"], case.expected())
        restated, counts = cn.restated(spans, case.sites, length)
        same_counts(got["COUNTS"], restated["COUNTS"])
        assert {k: int(stats[k]) for k in cn.METRIC_STATS} == case.want_counts() == {k: counts[k] for k in cn.METRIC_STATS}
        assert int(stats["reads_given"]) == sum(rd.n_reads for rd, _, _ in spans)
        last = spans[-1]
        assert np.array_equal(got["STATUS"], cn.tables_of(last[0], case.sites, length, last[1], last[2])["status"])
        runs.append(got)
    for other in runs[1:]:
        assert other["COUNTS"].tobytes() == runs[0]["COUNTS"].tobytes()


# ---- (2) the refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points():
    case = next(c for c in cc.HAND_TABLE if c.name.startswith("each base on each strand"))
    rd = cc.read_set(case.rows)
    rest = cc.read_set([(1, cc.REV, 196, cc.M4, "ACGG", [30] * 4, 60)])
    with cn.Pileup(case.sites, 200) as p:
        p.add(rd, 0, 100)
        before, stats = p.arrays(), p.stats()
        with pytest.raises(RuntimeError, match="offsets decrease"):
            p.add(dataclasses.replace(rd, read_offsets=np.array([0, 4, 8, 6, 12, 16, 20, 24, 28], np.int64)), 100, 200)
        with pytest.raises(RuntimeError, match="CIGAR query length"):
            p.add(dataclasses.replace(rest, cigars=rest.cigars + np.uint32(16)), 100, 200)
        with pytest.raises(RuntimeError, match="ref_end does not match"):
            p.add(dataclasses.replace(rest, ref_ends=rest.ref_ends + 1), 100, 200)
        with pytest.raises(RuntimeError, match=r"begins below 100, where the previous one ended"):
            p.add(rest, 99, 200)
        with pytest.raises(RuntimeError, match=r"span \[100, 201\)"):
            p.add(rest, 100, 201)
        with pytest.raises(RuntimeError, match=r"span \[100, 100\)"):
            p.add(rest, 100, 100)
        after = p.arrays()
        assert all(after[k].tobytes() == before[k].tobytes() for k in before) and p.stats() == stats      # nothing was left behind
        p.add(rest, 100, 200)
        got = p.arrays()
        want = case.expected()
        want[case.sites.index(199), cc.REVS, cc.G] = 1
        assert np.array_equal(got["COUNTS"], want) and got["STATUS"].tolist() == [2]
    with pytest.raises(RuntimeError, match="device 99"):
        cn.counted_on_gpu([(rd, 0, 200)], case.sites, 200, device=99)
    with pytest.raises(RuntimeError, match="is not above"):
        cn.Pileup([5, 5], 200)
    with pytest.raises(RuntimeError, match="share 1025"):
        cn.Pileup([5], 200, share=1025)
    with cn.Pileup([], 200) as empty:                                       # no site: nothing to count, nothing to fail
        empty.add(rd, 0, 200)
        assert empty.arrays()["COUNTS"].shape == (0, 2, 7) and empty.stats()["counting"] == 8 and empty.stats()["observations"] == 0


# ---- (3) the edge stress --------------------------------------------------------------------------------------------------------
def _covers(rows, sites):
    """Per row: whether a site lies inside its reference span."""
    end = np.array([r[2] + max(1, sum(k for op, k in r[3] if op in (cc.M, cc.D, cc.N, cc.EQ, cc.X))) for r in rows])
    start = np.array([r[2] for r in rows])
    return np.searchsorted(sites, end, "left") > np.searchsorted(sites, start, "left")


def test_edge_stress_on_one_chromosome():
    reference, sites, rows = cc.stress()
    reads = cc.read_set(rows)
    # each situation really occurs
    long_reads = [r for r in rows if len(r[4]) >= 1500]
    span_sites = lambda r: int(((sites >= r[2]) & (sites < r[2] + 1500)).sum())      # noqa: E731
    assert [span_sites(r) for r in long_reads if r[3] == [(cc.M, 1500)]] == [215, 0]
    assert any(r[2] < cc.SPAN < r[2] + 1500 for r in long_reads)                 # the span edge at 1 000 goes through a read
    words = [r for r in rows if r[3] == [(cc.M, cc.WORDS * 64)]]
    assert len(words) == 1 and words[0][2] % 64 == 0 and (words[0][2] + 1536 - 1) // 64 - words[0][2] // 64 + 1 == 24
    assert int(((sites >= words[0][2]) & (sites < words[0][2] + 1536)).sum()) == 1 and sites[-3] == words[0][2] + 1535 and sites[-3] % 64 == 63
    assert cc.LENGTH % 64 == 48 and sites[-1] == cc.LENGTH - 1 and sites[-1] // 64 == cc.LENGTH // 64 and sites[0] == 0
    assert sum(r[2] == cc.PILE_AT and len(r[4]) == 20 for r in rows) == cc.PILE
    cut = [(cc.read_set(cc.overlapping(rows, lo, lo + cc.SPAN)), lo, lo + cc.SPAN) for lo in range(0, cc.LENGTH, cc.SPAN)]
    want, counts = cn.restated([(reads, 0, cc.LENGTH)], sites, cc.LENGTH)
    rank = {int(p): i for i, p in enumerate(sites)}
    assert want["COUNTS"][rank[cc.PILE_AT + 9]].sum() >= cc.PILE and want["COUNTS"][0].sum() >= 1 and want["COUNTS"][-1].sum() >= 1
    assert want["COUNTS"][rank[int(sites[-3])]].sum() >= 2 and (want["COUNTS"][:, :, cc.DEL].sum() > 5) and want["COUNTS"][:, :, cc.LOWQ].sum() > 50
    assert want["COUNTS"][:, :, cc.OTHER].sum() > 10 and want["COUNTS"][:, 0].sum() > 500 and want["COUNTS"][:, 1].sum() > 500
    runs = []
    for spans in ([(reads, 0, cc.LENGTH)], cut, [(reads, 0, cc.LENGTH)], cut):
        for form, share in ((cn.TWO_PHASE, 0), (cn.PLAIN, 0), (cn.TWO_PHASE, cn.MAX_SHARE), (cn.TWO_PHASE, 300), (cn.PLAIN, 64)):
            got, stats = cn.counted_on_gpu(spans, sites, cc.LENGTH, form=form, share=share)
            same_counts(got["COUNTS"], want["COUNTS"])
            assert {k: int(stats[k]) for k in cn.METRIC_STATS} == {k: counts[k] for k in cn.METRIC_STATS}
            assert stats["sites_ms"] > 0 and stats["reads_ms"] > 0
            runs.append(got["COUNTS"].tobytes())
    assert len(set(runs)) == 1
    with cn.Pileup(sites, cc.LENGTH) as p:
        p.add(reads, 0, cc.LENGTH)
        assert np.array_equal(p.arrays()["STATUS"], cn.tables_of(reads, sites, cc.LENGTH, 0, cc.LENGTH)["status"])


def test_the_site_scan_carries_from_one_round_of_1024_words_into_the_next():
    """A chromosome of 2 049 words: the scan of csrc/site_bits.h makes two full rounds and a third of one word, with sites on the
    last bit of a round and on the first bit of the next."""
    _, sites, rows = cc.carry()
    L = cc.CARRY_LENGTH
    assert L == 2 * 65536 + 48 and (L + 63) // 64 == 2 * 1024 + 1 and cc.CARRY_NAMED == (0, 65535, 65536, 131071, 131072, L - 1)
    assert set(cc.CARRY_NAMED) <= set(sites.tolist()) and sites.shape[0] > 40
    assert all(20 <= len(r[4]) <= 150 for r in rows) and {r[1] & cc.REV for r in rows} == {0, cc.REV}
    assert any(r[2] < 65536 < r[2] + len(r[4]) for r in rows) and any(r[2] < 131072 < r[2] + len(r[4]) for r in rows)
    reads = cc.read_set(rows)
    cut = [(cc.read_set(cc.overlapping(rows, lo, min(lo + cc.CARRY_SPAN, L))), lo, min(lo + cc.CARRY_SPAN, L))
           for lo in range(0, L, cc.CARRY_SPAN)]
    want, counts = cn.restated([(reads, 0, L)], sites, L)
    for p in cc.CARRY_NAMED:                                              # the restatement alone counts on every named site
        assert want["COUNTS"][int(np.searchsorted(sites, p))].sum() >= 1, p
    runs = []
    for spans in ([(reads, 0, L)], cut, [(reads, 0, L)], cut):
        for form in FORMS:
            got, stats = cn.counted_on_gpu(spans, sites, L, form=form)
            same_counts(got["COUNTS"], want["COUNTS"])
            assert {k: int(stats[k]) for k in cn.METRIC_STATS} == {k: counts[k] for k in cn.METRIC_STATS}
            runs.append(got["COUNTS"].tobytes())
    assert len(set(runs)) == 1


@pytest.mark.parametrize("survivors", cc.SURVIVORS)
def test_phase_1_compacts_exactly_so_many_reads_of_a_workgroups_share(survivors):
    _, sites, _ = cc.stress()
    rows = cc.survivor_launch(survivors)
    covered = _covers(rows, sites)
    assert len(rows) == cc.SHARE + 100 and all(a[2] <= b[2] for a, b in zip(rows, rows[1:]))
    assert int(covered[:cc.SHARE].sum()) == survivors and covered[cc.SHARE:].all()          # the last workgroup is partly empty
    reads = cc.read_set(rows)
    want, counts = cn.restated([(reads, 0, cc.LENGTH)], sites, cc.LENGTH)
    assert counts["counting"] == len(rows) and counts["reads_on_a_site"] == survivors + 100
    for form in FORMS:
        got, stats = cn.counted_on_gpu([(reads, 0, cc.LENGTH)], sites, cc.LENGTH, form=form, share=cc.SHARE)
        same_counts(got["COUNTS"], want["COUNTS"])
        assert {k: int(stats[k]) for k in cn.METRIC_STATS} == {k: counts[k] for k in cn.METRIC_STATS}
        assert np.array_equal(got["STATUS"], np.where(covered, 2, 1))


# ---- (4) the fuzz ---------------------------------------------------------------------------------------------------------------
def independent_counts(reference, rows, sites):
    """COUNTS from the alignment table of tests/read_fuzz.py joined with bases, qualities and ``counted``: no cursor walks a CIGAR."""
    o = rf.Oracle(reference, rows)
    t = o.t
    is_site = np.zeros(rf.LENGTH + 1, bool)
    is_site[sites] = True
    rank = np.cumsum(is_site) - 1
    inside = (t.p >= 0) & (t.p < rf.LENGTH)
    use = (o.aligned | (t.op == rf.D)) & o.counted[t.read] & inside & is_site[np.where(inside, t.p, rf.LENGTH)]
    code = np.full(256, cc.OTHER, np.int64)
    code[list(b"ACGT")] = [cc.A, cc.C, cc.G, cc.T]
    which = np.where(t.op == rf.D, cc.DEL, np.where(o.qual < rf.Q_THRESHOLD, cc.LOWQ, code[(o.raw & 0xDF) & 0xFF]))
    out = np.zeros((len(sites), 2, 7), np.int64)
    np.add.at(out, (rank[t.p[use]], (o.flag[t.read[use]] & rf.REV != 0).astype(np.int64), which[use]), 1)
    return out


@pytest.mark.parametrize("profile", rf.PROFILES)
@pytest.mark.parametrize("seed", rf.SEEDS)
def test_fuzz_corpus_dense_and_sparse_whole_and_cut(seed, profile):
    reference, rows, _ = rf.corpus(seed, profile)
    L = rf.LENGTH
    reads = cc.read_set(rows)
    edges = [0] + list(rf.CUTS) + [L]
    cut = [(cc.read_set(cc.overlapping(rows, lo, hi)), lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]
    for sites in (np.arange(L), np.arange(seed % 97, L, 97)):                    # every position a site: every rank; then sparse
        want, counts = cn.restated([(reads, 0, L)], sites, L, rf.Q_THRESHOLD, rf.MAPQ_THRESHOLD)
        same_counts(independent_counts(reference, rows, sites), want["COUNTS"])
        assert want["COUNTS"].sum() == counts["observations"] > 0
        for spans in ([(reads, 0, L)], cut):
            got, stats = cn.counted_on_gpu(spans, sites, L, rf.Q_THRESHOLD, rf.MAPQ_THRESHOLD, form=(seed + len(spans)) % 2,
                                           share=(0, 5, 64, 256, cn.MAX_SHARE)[seed % 5])
            same_counts(got["COUNTS"], want["COUNTS"])
            assert {k: int(stats[k]) for k in cn.METRIC_STATS} == {k: counts[k] for k in cn.METRIC_STATS}, (seed, profile, len(spans))


# ---- (5) the driver -------------------------------------------------------------------------------------------------------------
FILES = ("txt", "pileup.tsv", "npz")
_driver: dict = {}


def _run(argv):
    return call.main(call.parser().parse_args(argv))


def _read(*parts):
    return open(os.path.join(*parts), "rb").read()


def driver_input(tmp_path_factory):
    """One person as an Illumina BAM (with PCR copies) and a PacBio BAM, another person as a PacBio BAM, the sites file and models."""
    if not _driver:
        from hello_amd import loader, netspec as ns, weights
        from tests.test_gpu_candidates import _fasta, _write
        from tests.util import load_fixture
        tmp = tmp_path_factory.mktemp("contamination_driver")
        reference, pos, alt, af = cc.population()
        one, other = cc.person(1, af), cc.person(2, af)
        ibam = _write(tmp, "i.bam", "chr1", reference, cc.reads_of_person(1, reference, pos, alt, one, 150, 20, "a", copies=60))
        pbam = _write(tmp, "p.bam", "chr1", reference, cc.reads_of_person(2, reference, pos, alt, one, 2000, 12, "p"))
        qbam = _write(tmp, "q.bam", "chr1", reference, cc.reads_of_person(3, reference, pos, alt, other, 2000, 12, "q"))
        vcf = str(tmp / "sites.vcf")
        open(vcf, "w").write(cc.sites_vcf(reference, pos, alt, af))
        single, hybrid = str(tmp / "single.hello.npz"), str(tmp / "hybrid.hello.npz")
        loader.save_native(single, "single_tech", weights.synth_state(ns.build("single_tech"), seed=MODEL_SEED))
        loader.save_native(hybrid, "hybrid_full", load_fixture("hybrid_full")[1])
        _driver.update(tmp=tmp, ibam=ibam, pbam=pbam, qbam=qbam, vcf=vcf, genome={"chr1": reference}, n_sites=len(pos), single=single,
                       hybrid=hybrid, flags=["--contamination", "--contamination_sites", vcf], fasta=_fasta(tmp, "chr1", reference))
    return _driver


def _want(d, bam, directory, name):
    os.makedirs(directory, exist_ok=True)
    sites = cn.read_sites(d["vcf"], d["genome"])
    found = cn.measure(bam, d["genome"], ["chr1"], sites, restatement=True)
    found.write_all(os.path.join(directory, "contamination." + name))
    return found


@pytest.mark.parametrize("resident", [False, True], ids=["shards", "resident"])
def test_the_driver_writes_the_files_of_the_restatement_and_leaves_the_vcf_alone(resident, tmp_path_factory):
    d = driver_input(tmp_path_factory)
    tail = ["--ibam", d["ibam"], "--ref", d["fasta"], "--network", d["single"], "--from_bam"] + (["--resident"] if resident else [])
    work = {name: str(d["tmp"] / ("%s_%d" % (name, resident))) for name in ("counted", "plain", "want")}
    _run(["--workdir", work["counted"]] + d["flags"] + tail)
    _run(["--workdir", work["plain"]] + tail)
    assert _read(work["counted"], "results.output.vcf") == _read(work["plain"], "results.output.vcf")
    assert not [f for f in os.listdir(work["plain"]) if f.startswith("contamination")]
    want = _want(d, d["ibam"], work["want"], "illumina")
    for suffix in FILES:
        assert _read(work["counted"], "contamination.illumina." + suffix) == _read(work["want"], "contamination.illumina." + suffix), suffix
    assert not os.path.exists(os.path.join(work["counted"], "contamination.pacbio.txt"))
    assert not os.path.exists(os.path.join(work["counted"], "contamination.identity.txt"))
    total, est = want.total(), want.estimate()
    assert total["n_sites"] == d["n_sites"] > 200 and total["observations"] > 15 * d["n_sites"] and est["k_lo"] == 0 and est["k"] < 20


def test_under_mark_duplicates_the_marked_reads_leave_the_pileup(tmp_path_factory):
    d = driver_input(tmp_path_factory)
    work = {name: str(d["tmp"] / name) for name in ("marked", "want_marked", "want_unmarked")}
    _run(["--workdir", work["marked"], "--mark_duplicates", "--ibam", d["ibam"], "--ref", d["fasta"], "--network", d["single"], "--from_bam"] + d["flags"])
    marks = markdup.find_duplicates(d["ibam"], restatement=True)
    with markdup.applied({d["ibam"]: marks}):
        marked = _want(d, d["ibam"], work["want_marked"], "illumina")
    unmarked = _want(d, d["ibam"], work["want_unmarked"], "illumina")
    for suffix in FILES:
        assert _read(work["marked"], "contamination.illumina." + suffix) == _read(work["want_marked"], "contamination.illumina." + suffix), suffix
    n_marked = marks.total()["duplicate_reads"]
    assert n_marked >= 60 and unmarked.total()["counting"] - marked.total()["counting"] == n_marked
    lost = unmarked.tables["chr1"]["COUNTS"] - marked.tables["chr1"]["COUNTS"]
    assert (lost >= 0).all() and lost.sum() == unmarked.total()["observations"] - marked.total()["observations"] > 60


def test_two_bams_of_one_person_and_of_two(tmp_path_factory):
    d = driver_input(tmp_path_factory)
    tail = ["--ibam", d["ibam"], "--ref", d["fasta"], "--network", d["hybrid"], "--from_bams"]
    work = {name: str(d["tmp"] / ("both_" + name)) for name in ("counted", "plain", "swapped", "want")}
    _run(["--workdir", work["counted"], "--pbam", d["pbam"]] + d["flags"] + tail)
    _run(["--workdir", work["plain"], "--pbam", d["pbam"]] + tail)
    assert _read(work["counted"], "results.output.vcf") == _read(work["plain"], "results.output.vcf")
    assert not [f for f in os.listdir(work["plain"]) if f.startswith("contamination")]
    first, second = _want(d, d["ibam"], work["want"], "illumina"), _want(d, d["pbam"], work["want"], "pacbio")
    cn.write_identity(os.path.join(work["want"], "contamination.identity.txt"), first, second)
    names = ["contamination.%s.%s" % (name, suffix) for name in ("illumina", "pacbio") for suffix in FILES] + ["contamination.identity.txt"]
    for name in names:
        assert _read(work["counted"], name) == _read(work["want"], name), name
    said = dict(line.split("\t") for line in _read(work["counted"], "contamination.identity.txt").decode().splitlines())
    assert said["verdict"] == "same_sample" and float(said["lod"]) > 50 and int(said["sites_used"]) > 200
    # the PacBio BAM of another person is told apart
    _run(["--workdir", work["swapped"], "--pbam", d["qbam"]] + d["flags"] + tail)
    said = dict(line.split("\t") for line in _read(work["swapped"], "contamination.identity.txt").decode().splitlines())
    assert said["verdict"] == "different_sample" and float(said["lod"]) < -50
    assert _read(work["swapped"], "contamination.illumina.npz") == _read(work["counted"], "contamination.illumina.npz")
