"""CpG methylation on the GPU (hello_meth_*; hello_amd/csrc/methylation.hip): SITES and COUNTS equal the restatement of
hello_amd/methylation.py integer for integer -- on the tables worked by hand (tests/methylation_cases.py), on an edge stress whose
reads cross the 64-base chunk, the 64-position word and the span edges, and through the driver, where ``--methylation`` writes the
files the restatement writes and leaves the VCF alone."""
import dataclasses
import os

import numpy as np
import pytest

from hello_amd import call, haplotag as ht, methylation as me
from tests import methylation_cases as mc
from tests.test_methylation import same_tables, spans_of, stress_bam

pytestmark = pytest.mark.gpu
MODEL_SEED = 1


# ---- (1) the hand tables through the kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.HAND_TABLE, ids=[c.name for c in mc.HAND_TABLE])
def test_hand_table_through_the_kernels(case):
    want = dict(SITES=np.array(case.sites, np.int64), COUNTS=case.expected())
    runs = []
    for cuts in ((), (case.cut(),), (), (case.cut(),)):                        # whole and cut through a read, each twice
        spans = spans_of(case, cuts)
        got, stats = me.counted_on_gpu(spans, case.reference)
        same_tables(got, want)
        restated, counts = me.restated(spans, case.reference)
        same_tables(got, restated)
        assert {k: int(stats[k]) for k in me.METRIC_STATS} == case.want_counts() == {k: counts[k] for k in me.METRIC_STATS}
        assert int(stats["reads_given"]) == sum(rd.n_reads for rd, _, _, _ in spans)
        last = spans[-1]
        assert np.array_equal(got["STATUS"], me.tables_of(last[0], last[1], case.reference, last[2], last[3])["status"])
        runs.append(got)
    for a, b in ((0, 2), (1, 3), (0, 1)):
        assert runs[a]["COUNTS"].tobytes() == runs[b]["COUNTS"].tobytes() and runs[a]["SITES"].tobytes() == runs[b]["SITES"].tobytes()


# ---- (2) the refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points():
    case = next(c for c in mc.HAND_TABLE if c.name.startswith("HP 0, 1, 2"))
    rd, mods = mc.read_set(case.rows)
    far = [mc.Row(0, 196, mc.M4, mc.REF[196:200], b"C+m,0;", [150])]
    rest = mc.read_set(far)
    with me.Counter(case.reference) as c:
        c.add(rd, mods, 0, 100)
        before, stats = c.arrays(), c.stats()
        with pytest.raises(RuntimeError, match="offsets decrease"):
            c.add(dataclasses.replace(rd, read_offsets=np.array([0, 4, 8, 6, 12], np.int64)), mods, 100, 200)
        with pytest.raises(RuntimeError, match="CIGAR query length"):
            c.add(dataclasses.replace(rest[0], cigars=rest[0].cigars + np.uint32(16)), rest[1], 100, 200)
        with pytest.raises(RuntimeError, match=r"begins below 100, where the previous one ended"):
            c.add(*rest, 99, 200)
        with pytest.raises(RuntimeError, match=r"span \[100, 201\)"):
            c.add(*rest, 100, 201)
        with pytest.raises(RuntimeError, match=r"span \[100, 100\)"):
            c.add(*rest, 100, 100)
        with pytest.raises(RuntimeError, match="delta -1"):
            c.add(rest[0], dataclasses.replace(rest[1], deltas=np.array([-1], np.int32)), 100, 200)
        with pytest.raises(RuntimeError, match="modification state 3"):
            c.add(rest[0], dataclasses.replace(rest[1], state=np.array([3], np.uint8)), 100, 200)
        with pytest.raises(RuntimeError, match="modification mode 2"):
            c.add(rest[0], dataclasses.replace(rest[1], mode=np.array([2], np.uint8)), 100, 200)
        with pytest.raises(RuntimeError, match="2 probabilities for 1 deltas"):
            c.add(rest[0], dataclasses.replace(rest[1], probs=np.array([1, 2], np.uint8)), 100, 200)
        with pytest.raises(RuntimeError, match="modification offsets end at 0, 1 deltas"):
            c.add(rest[0], dataclasses.replace(rest[1], offsets=np.zeros(2, np.int64)), 100, 200)
        after = c.arrays()
        assert all(after[k].tobytes() == before[k].tobytes() for k in before) and c.stats() == stats      # nothing was left behind
        c.add(*rest, 100, 200)
        got = c.arrays()
        want = case.expected()
        want[mc.SITES.index(198), 0] = [1, 0, 150]
        assert np.array_equal(got["COUNTS"], want) and got["STATUS"].tolist() == [1]
    with pytest.raises(RuntimeError, match="device 99"):
        me.counted_on_gpu([(rd, mods, 0, 200)], case.reference, device=99)
    with pytest.raises(RuntimeError, match="NULL pointer"):
        me.check(me._lib().hello_meth_create(None, 0, 10, 0, None))


# ---- (3) the edge stress --------------------------------------------------------------------------------------------------------
def test_edge_stress_on_one_chromosome(tmp_path_factory):
    s = stress_bam(tmp_path_factory)
    rows, reference = s["rows"], s["genome"]["chr1"]
    reads, mods = mc.read_set(rows)
    listed = np.diff(mods.offsets)
    sites = me.sites_of(reference)
    # each situation really occurs
    assert {63, 64, 65, 130} <= set(listed.tolist())
    assert sorted(listed[listed > mc.SHARE].tolist()) == [1125, 1125] and 375 in listed.tolist()        # two scratch slices
    assert any("C" not in r.bases and not r.flag & mc.REV and r.parsed()[3] == me.USABLE for r in rows)
    long_reads = [r for r in rows if len(r.bases) == mc.LONG]
    assert sorted(r.flag for r in long_reads) == [0, 0, mc.REV] and all(r.pos < mc.SPAN < r.end for r in long_reads)
    for edge in list(range(mc.LONG_AT + 64, mc.LONG_AT + mc.LONG, 64)) + [mc.SPAN]:                      # CpGs on both sides
        assert ((sites >= edge - 4) & (sites < edge)).any() and ((sites >= edge) & (sites < edge + 4)).any(), edge
    assert 2047 in sites and 2047 % 64 == 63 and 2112 in sites and 2112 % 64 == 0
    assert sum(r.pos == mc.PILE_AT and len(r.bases) == 20 for r in rows) == mc.PILE
    assert sites[0] == 0 and sites[-1] == mc.LENGTH - 2
    whole = s["whole"].tables["chr1"]
    stats = dict(zip(me.METRIC_STATS, whole["STATS"].tolist()))
    assert stats["reads_bad_mods"] == 1 and stats["counting"] == len(rows) - 1 and stats["n_sites"] == sites.shape[0]
    pile = int(np.searchsorted(sites, mc.PILE_AT + 9))
    assert whole["COUNTS"][pile, 0, :2].sum() >= mc.PILE - 100 and whole["COUNTS"][0, 0, :2].sum() >= 1 and whole["COUNTS"][-1, 0, :2].sum() >= 1
    for p in (2047, 2112):
        assert whole["COUNTS"][int(np.searchsorted(sites, p)), 0, :2].sum() >= 2
    assert whole["COUNTS"][:, 1, :2].sum() > 100 and whole["COUNTS"][:, 2, :2].sum() > 100
    # max_span 1 000 and unset: equal arrays, equal to the restatement; twice for equal bytes
    runs = [me.measure(s["path"], s["genome"], ["chr1"], max_span=span) for span in (mc.SPAN, None, mc.SPAN, None)]
    for got in runs:
        same_tables(got.tables["chr1"], whole)
        assert np.array_equal(got.tables["chr1"]["STATS"], whole["STATS"])
        assert got.tables["chr1"]["COUNTS"].tobytes() == runs[0].tables["chr1"]["COUNTS"].tobytes()
    # straight from the rows: the status of every read, and the kernels' times
    with me.Counter(reference) as c:
        c.add(reads, mods, 0, mc.LENGTH)
        got, st = c.arrays(), c.stats()
    same_tables(got, whole)
    assert np.array_equal(got["STATUS"], me.tables_of(reads, mods, reference, 0, mc.LENGTH)["status"]) and (got["STATUS"] == 2).sum() == 1
    assert st["sites_ms"] > 0 and st["reads_ms"] > 0


def test_the_site_scan_carries_from_one_round_of_1024_words_into_the_next():
    """A chromosome of 2 049 words: the scan of csrc/site_bits.h makes two full rounds and a third of one word.  A CpG takes two
    positions, so of the two positions at a round edge one is a site (mc.CARRY_NAMED)."""
    reference, sites, rows = mc.carry()
    L = mc.CARRY_LENGTH
    assert L == 2 * 65536 + 48 and (L + 63) // 64 == 2 * 1024 + 1 and np.array_equal(me.sites_of(reference), sites)
    assert set(mc.CARRY_NAMED) <= set(sites.tolist()) and sites[0] == 0 and sites[-1] == L - 2 and sites.shape[0] > 40
    assert [p >> 6 for p in mc.CARRY_NAMED] == [0, 1023, 1024, 2047, 2048, 2048] and 65535 % 64 == 63 and 131072 % 64 == 0
    assert all(20 <= len(r.bases) <= 150 for r in rows) and {r.flag & mc.REV for r in rows} == {0, mc.REV}
    assert any(r.pos < 65536 < r.end for r in rows) and any(r.pos < 131072 < r.end for r in rows)        # a read across each edge
    reads, mods = mc.read_set(rows)
    cut = [mc.read_set(mc.overlapping(rows, lo, min(lo + mc.CARRY_SPAN, L))) + (lo, min(lo + mc.CARRY_SPAN, L))
           for lo in range(0, L, mc.CARRY_SPAN)]
    want, counts = me.restated([(reads, mods, 0, L)], reference)
    for p in mc.CARRY_NAMED:                                              # the restatement alone counts on every named site
        assert want["COUNTS"][int(np.searchsorted(sites, p)), 0, :2].sum() >= 1, p
    runs = []
    for spans in ([(reads, mods, 0, L)], cut, [(reads, mods, 0, L)], cut):
        got, stats = me.counted_on_gpu(spans, reference)
        assert np.array_equal(got["SITES"], want["SITES"]) and np.array_equal(got["COUNTS"], want["COUNTS"])
        assert {k: int(stats[k]) for k in me.METRIC_STATS} == {k: counts[k] for k in me.METRIC_STATS}
        runs.append(got["SITES"].tobytes() + got["COUNTS"].tobytes())
    assert len(set(runs)) == 1


# ---- (4) the driver -------------------------------------------------------------------------------------------------------------
FILES = ("methylation.combined.bed", "methylation.hap1.bed", "methylation.hap2.bed", "methylation.npz")
_driver: dict = {}


def _run(argv):
    return call.main(call.parser().parse_args(argv))


def _read(*parts):
    return open(os.path.join(*parts), "rb").read()


def driver_input(tmp_path_factory):
    """The long reads of the 6 kb chromosome of the phasing tests, each with the calls an instrument writes and every fifth with an
    HP tag, as a PacBio BAM; and a model."""
    if not _driver:
        from hello_amd import loader, netspec as ns, weights
        from tests.test_gpu_candidates import _fasta, _write
        from tests.test_gpu_haplotag import chromosome
        c = chromosome()
        rng = np.random.default_rng(3)
        tmp = tmp_path_factory.mktemp("methylation_driver")
        tagged = []
        for n, r in enumerate(c["long"]):
            reverse = bool(r.flag & mc.REV)
            wanted = mc.cpgs_of(r.seq, reverse)
            row = mc.Row(r.flag, r.pos, r.cigar, r.seq, mc.mm_of(r.seq, reverse, wanted, ("", "?")[n % 2]),
                         [int(x) for x in rng.integers(0, 256, size=len(wanted))], hp=(n % 5 == 0) * (1 + n % 2))
            tagged.append(dataclasses.replace(r, tags=row.tags()))
        model = str(tmp / "m.hello.npz")
        loader.save_native(model, "single_tech", weights.synth_state(ns.build("single_tech"), seed=MODEL_SEED))
        bam = _write(tmp, "p.bam", "chr1", c["reference"], tagged)
        _driver.update(tmp=tmp, bam=bam, genome={"chr1": c["reference"]},
                       tail=["--pbam", bam, "--ref", _fasta(tmp, "chr1", c["reference"]), "--network", model, "--from_bam"])
    return _driver


@pytest.mark.parametrize("resident", [False, True], ids=["shards", "resident"])
def test_the_driver_writes_the_files_of_the_restatement_and_leaves_the_vcf_alone(resident, tmp_path_factory):
    d = driver_input(tmp_path_factory)
    tail = d["tail"] + (["--resident"] if resident else [])
    work = {name: str(d["tmp"] / ("%s_%d" % (name, resident))) for name in ("counted", "plain", "phased", "want", "want_phased")}
    _run(["--workdir", work["counted"], "--methylation"] + tail)
    _run(["--workdir", work["plain"]] + tail)
    assert _read(work["counted"], "results.output.vcf") == _read(work["plain"], "results.output.vcf")
    assert not [f for f in os.listdir(work["plain"]) if f.startswith("methylation")]
    for name in ("want", "want_phased"):
        os.makedirs(work[name])
    want = me.measure(d["bam"], d["genome"], ["chr1"], restatement=True)                     # the haplotypes: the BAM's HP tags
    want.write_bed(os.path.join(work["want"], "methylation"))
    want.save(os.path.join(work["want"], "methylation.npz"))
    for name in FILES:
        assert _read(work["counted"], name) == _read(work["want"], name), name
    total = want.total()
    assert total["counting"] > 0 and total["observations"] > 1000 and len(_read(work["want"], FILES[1]).splitlines()) > 10
    # with --phase the haplotypes are what the Haplotagger gives the reads from the phased VCF written just before
    _run(["--workdir", work["phased"], "--methylation", "--phase"] + tail)
    phased = os.path.join(work["phased"], "results.output.phased.vcf")
    with ht.Haplotagger(phased, ["chr1"]) as tagger:
        assert len(tagger.records["chr1"]) > 20
        fed = me.measure(d["bam"], d["genome"], ["chr1"], tagger, restatement=True)
    fed.write_bed(os.path.join(work["want_phased"], "methylation"))
    fed.save(os.path.join(work["want_phased"], "methylation.npz"))
    for name in FILES:
        assert _read(work["phased"], name) == _read(work["want_phased"], name), name
    assert _read(work["phased"], FILES[0]) == _read(work["counted"], FILES[0])              # the combined track does not depend on it
    assert _read(work["phased"], FILES[1]) != _read(work["counted"], FILES[1])
    assert _read(work["phased"], "results.output.vcf") == _read(work["plain"], "results.output.vcf")
