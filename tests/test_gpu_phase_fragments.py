"""Fragments on the GPU (hello_phase_fragments, hello_phase_tag_fragments; hello_amd/csrc/phase.hip): ``mate``, the fragment links,
``hp``, ``ps`` and the statistics ``pairs`` / ``groups_refused`` equal the restatement of hello_amd/phase.py integer for integer --
on the tables worked by hand (tests/fragment_cases.py), on a pairing stress whose probes collide and wrap at the table's end, on a
6 kb chromosome of two sources with mates in different spans, and through the driver."""
import os

import numpy as np
import pytest

from hello_amd import call, phase
from hello_amd.bam import BamFile
from tests import fragment_cases as fc
from tests.bam_writer import write_bam
from tests.test_phase_fragments import HEADER, restated

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SEED = 1
PER_READ = ("slots", "slot_offsets", "first", "links")


def same(got, want, names):
    for name in names:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name


# ---- (1) the hand tables through the kernels, the chain on the fragment links -------------------------------------------------
@pytest.mark.parametrize("case", fc.HAND_TABLE, ids=[c.name for c in fc.HAND_TABLE])
def test_hand_table_through_the_kernels(case):
    want, details = restated(case), {}
    hp, ps = phase.find_haplotags(case.sets(), case.records, window=case.window, min_margin=1, details=details, fragments=True)
    got = dict(details, hp=hp, ps=ps, links=details["fragment_links"])
    same(got, want, ("mate", "links", "set", "flip", "hp", "ps"))
    assert got["mate"].tolist() == case.mate and hp.tolist() == case.hp and ps.tolist() == case.ps
    assert (details["stats"]["pairs"], details["stats"]["groups_refused"]) == (case.pairs, case.refused)


def test_refusals_of_the_new_entry_points():
    case = fc.HAND_TABLE[0]
    rd = case.sets()[0]
    source = np.zeros(rd.n_reads, np.uint8)
    sets, flip = np.arange(6, dtype=np.int32), np.zeros(6, np.uint8)
    with phase.Phaser(case.records, window=3) as ph:
        ph.observe([rd])
        with pytest.raises(RuntimeError, match="needs hello_phase_fragments"):
            ph.tag(sets, flip, fragments=True)
        with pytest.raises(RuntimeError, match="n_reads 1: the handle holds 2"):
            ph.fragments(rd.name_hash[:1], rd.flags[:1], source[:1])
        with pytest.raises(RuntimeError, match="source"):
            ph.fragments(rd.name_hash, rd.flags, source + 2)
        assert ph.fragments(rd.name_hash, rd.flags, source).tolist() == [1, 0]
        with pytest.raises(RuntimeError, match="called once"):
            ph.fragments(rd.name_hash, rd.flags, source)
        with pytest.raises(RuntimeError, match="cannot be added"):
            ph.observe([rd])
    with phase.Phaser(case.records, window=3) as ph:
        ph.observe([rd])
        ph.tag(sets, flip)
        with pytest.raises(RuntimeError, match="after a tag"):
            ph.fragments(rd.name_hash, rd.flags, source)


# ---- (2) the pairing stress ---------------------------------------------------------------------------------------------------
def stress():
    """4 096 pairs and 64 groups that are refused, in shuffled order.  1 024 names differ only in their top 16 bits, 1 024 only in
    their low 16 bits; 12 names have their first probe three slots before the table's end, so their groups fill those three
    slots and go on from slot 0; the rest are random."""
    rng = np.random.default_rng(11)
    n_reads = 2 * 4096 + 32 * 3 + 32 * 2
    size = phase.pair_table_size(n_reads)
    tried = rng.integers(0, 2 ** 63, size=2_000_000, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    run = tried[phase.pair_table_slot(tried, np.zeros(tried.shape[0], np.uint8), size) == size - 3][:12]
    assert run.shape[0] == 12 and size == 32768
    names = [(np.uint64(i) << np.uint64(48)) | np.uint64(0x123456789ABC) for i in range(1024)]
    names += [np.uint64(0xDEADBEEFCAFE0000) | np.uint64(i) for i in range(1024)]
    names += run.tolist()
    names += (rng.integers(0, 2 ** 62, size=4096 + 64 - len(names), dtype=np.uint64) * np.uint64(4) + np.uint64(2)).tolist()
    assert len(set(int(x) for x in names)) == 4096 + 64
    rows = []
    for i, name in enumerate(int(x) for x in names):
        if i < 4096:
            rows += [(name, fc.FIRST, 60, *fc.LEFT), (name, fc.SECOND, 60, *fc.RIGHT)]
        elif i < 4096 + 32:
            rows += [(name, fc.FIRST, 60, *fc.LEFT), (name, fc.SECOND, 60, *fc.RIGHT), (name, fc.SECOND, 60, *fc.RIGHT)]
        else:
            rows += [(name, fc.FIRST, 60, *fc.LEFT), (name, fc.FIRST, 60, *fc.RIGHT)]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    assert len(rows) == n_reads
    return fc.read_set(rows), size


def test_pairing_stress_collisions_and_a_probe_that_wraps():
    rd, size = stress()
    source = np.zeros(rd.n_reads, np.uint8)
    want_mate, counts = phase.join_mates(rd.name_hash, rd.flags, source, np.ones(rd.n_reads, bool))
    assert counts == dict(pairs=4096, groups_refused=64)
    first_probe = phase.pair_table_slot(rd.name_hash, source, size)
    assert (first_probe == size - 3).sum() == 24                                # 12 groups on 3 slots: the probe wraps
    with phase.Phaser(fc.RECORDS, window=3) as ph:
        ph.observe([rd])
        before = ph.arrays()
        mate = ph.fragments(rd.name_hash, rd.flags, source)
        after = ph.arrays()
        st = ph.fragment_stats()
    assert mate.dtype == np.int64 and np.array_equal(mate, want_mate)
    assert (st["pairs"], st["groups_refused"]) == (4096, 64) and st["pair_ms"] > 0 and st["fragment_link_ms"] > 0
    same(after, before, PER_READ)                                               # the per-read arrays stay what they were
    assert before["slots"].shape[0] == 2 * rd.n_reads and int(before["slots"].sum()) == 2 * (4096 + 64 + 32)      # a, a or b, b
    want = phase.links_of(before["slots"], before["slot_offsets"], before["first"], 6, 3, mate=want_mate)
    assert np.array_equal(after["fragment_links"], want) and want[4, 2, 1] == 4096 and before["links"][4, 2, 1] == 0


# ---- (3) the 6 kb chromosome of two sources -------------------------------------------------------------------------------------
_made: dict = {}


def chromosome(tmp_path_factory):
    """The BAMs, the records and, per max_span, the restatement -- computed once, with what makes the comparison worth something."""
    if not _made:
        tmp = tmp_path_factory.mktemp("fragments")
        lines, short, long = fc.two_sources()
        paths = [str(tmp / "s.bam"), str(tmp / "l.bam")]
        for path, reads in zip(paths, (short, long)):
            write_bam(path, [("chr1", fc.LENGTH)], reads, index=True, block_bytes=20000)
        records = [r for r in map(phase.phasable, lines) if r]
        _made.update(paths=paths, records=records, short=short, want={})
    return _made


def run(c, max_span, restatement=False, stats=None):
    handles = [BamFile(p) for p in c["paths"]]
    try:
        return phase.chromosome_phase(handles, "chr1", fc.LENGTH, c["records"], max_span=max_span, restatement=restatement,
                                      stats=stats, fragments=True)
    finally:
        for h in handles:
            h.close()


ARRAYS = PER_READ + ("mate", "fragment_links", "set", "flip", "hp", "ps")


@pytest.mark.parametrize("max_span", [1000, None])
def test_two_sources_equal_the_restatement_whatever_the_spans(max_span, tmp_path_factory):
    c = chromosome(tmp_path_factory)
    want_stats, stats = {}, {}
    want = c["want"][max_span] = run(c, max_span, restatement=True, stats=want_stats)
    got, again = run(c, max_span, stats=stats), run(c, max_span)
    same(got, want, ARRAYS)
    for name in ARRAYS:
        assert got[name].tobytes() == again[name].tobytes(), name               # two runs: the same bytes
    assert (stats["pairs"], stats["groups_refused"]) == (want_stats["pairs"], want_stats["groups_refused"])
    # worth something: most pairs joined, a mate left alone because the other is not counted, links that only a fragment has,
    # links that two overlapping mates would have counted twice, tags of both haplotypes, and reads whose tag the mate changed
    mate = want["mate"]
    assert 380 <= want_stats["pairs"] < 400 and (mate >= 0).sum() == 2 * want_stats["pairs"]
    assert (want["fragment_links"] > want["links"]).sum() > 100
    n, first, p = np.diff(want["slot_offsets"]), want["first"], np.flatnonzero(mate >= 0)
    shared = np.minimum(first[p] + n[p], first[mate[p]] + n[mate[p]]) - np.maximum(first[p], first[mate[p]])
    assert (shared >= 2).sum() >= 6 and (shared == 1).sum() >= 60 and (shared < 0).sum() >= 400  # per read: 2 x the pairs
    assert set(want["hp"].tolist()) == {0, 1, 2} and (want["hp"][mate >= 0] == want["hp"][mate[mate >= 0]]).all()
    alone = phase.haplotags_of(want["slots"], want["slot_offsets"], want["first"], want["set"], want["flip"],
                               [r.pos for r in c["records"]])
    assert (alone[0] != want["hp"]).any()
    if max_span:                                                                # mates in different spans are joined too
        assert stats["calls"] == 6
        span_of = np.full(mate.shape[0], -1)
        at = 0
        handles = [BamFile(p) for p in c["paths"]]
        try:
            for k, lo in enumerate(range(0, fc.LENGTH, max_span)):
                for h in handles:
                    n = phase._from(h.fetch("chr1", lo, lo + max_span), lo).n_reads
                    span_of[at:at + n] = k
                    at += n
        finally:
            for h in handles:
                h.close()
        paired = np.flatnonzero(mate >= 0)
        assert at == mate.shape[0] and (span_of[paired] != span_of[mate[paired]]).sum() >= 20
    if len(c["want"]) == 2:                                                     # the spans change the read order, nothing per record
        same(c["want"][1000], c["want"][None], ("links", "fragment_links", "set", "flip"))


# ---- (4) nobody has a mate: the per-read results ------------------------------------------------------------------------------
def test_without_a_paired_flag_fragments_are_the_reads():
    from tests import phase_cases as pc
    from tests.test_gpu_phase import chromosome as unpaired
    c = unpaired()
    rd, source = phase.Reads.concat(c["sets"])
    with phase.Phaser(c["records"], window=pc.WINDOW) as ph:
        ph.observe(c["sets"])
        before = ph.arrays()
        mate = ph.fragments(rd.name_hash, rd.flags, source)
        after = ph.arrays()
        sets, flip = phase.chain_native(after["fragment_links"], pc.WINDOW, 2)
        joined = ph.tag(sets, flip, fragments=True)
        alone = ph.tag(sets, flip)
        st = ph.fragment_stats()
    assert (mate == -1).all() and (st["pairs"], st["groups_refused"]) == (0, 0)
    same(after, before, PER_READ)
    same(after, c["want"], PER_READ)
    assert np.array_equal(after["fragment_links"], after["links"])
    assert np.array_equal(joined[0], alone[0]) and np.array_equal(joined[1], alone[1])
    assert np.array_equal(alone[0], c["want"]["hp"]) and np.array_equal(alone[1], c["want"]["ps"])


# ---- (5) the driver -----------------------------------------------------------------------------------------------------------
def paired_illumina_input():
    """The reads of tests/test_gpu_resident.py: illumina_input, every other stretch of 40 reads of one donor joined with the next
    stretch into pairs about 300 bp apart: one name, flags 0x43 / 0x83 beside the strand bit."""
    from tests.test_gpu_resident import illumina_input
    reference, reads = illumina_input()
    for prefix in ("a", "b"):
        mine = [r for r in reads if r.name.startswith(prefix)]
        for i in range(0, len(mine) - 40):
            if (i // 40) % 2 == 0:
                first, second = mine[i], mine[i + 40]
                first.name = second.name = "pair_%s%d" % (prefix, i)
                first.flag |= 0x43
                second.flag |= 0x83
    return reference, reads


def _run(argv):
    return call.main(call.parser().parse_args(argv))


def test_the_driver_and_the_module_write_the_restatements_file(tmp_path):
    from hello_amd import loader, netspec as ns, weights
    from tests.test_gpu_candidates import _fasta, _write
    reference, reads = paired_illumina_input()
    bam, fa = _write(tmp_path, "i.bam", "chr1", reference, reads), _fasta(tmp_path, "chr1", reference)
    model = str(tmp_path / "hp.hello.npz")
    loader.save_native(model, "single_tech_hp", weights.synth_state(ns.build("single_tech_hp"), seed=MODEL_SEED))
    base = ["--ibam", bam, "--ref", fa, "--network", model, "--from_bam", "--resident", "--include_hp"]
    work = {name: str(tmp_path / name) for name in ("plain", "joined", "two")}
    read = lambda *p: open(os.path.join(*p), "rb").read()      # noqa: E731
    plain = _run(base + ["--workdir", work["plain"]])
    _run(base + ["--phase", "--phase_fragments", "--workdir", work["joined"]])
    assert read(work["joined"], "results.output.vcf") == read(plain)                             # the result is what it was
    assert not os.path.exists(os.path.join(work["plain"], "results.output.phased.vcf"))
    route = call.Route.from_args(call.parser().parse_args(base + ["--workdir", work["plain"]]), need_ref=False)
    thresholds = (route.q_threshold, route.mapq_threshold)
    stats = {}
    want = read(phase.write_phased_vcf(plain, [bam], str(tmp_path / "want.vcf"), None, *thresholds, restatement=True, fragments=True,
                                       stats=stats))
    alone = read(phase.write_phased_vcf(plain, [bam], str(tmp_path / "alone.vcf"), None, *thresholds, restatement=True))
    assert stats["pairs"] > 1000 and want.count(b"|") >= 2 and want != alone                     # the mates change the file
    assert read(work["joined"], "results.output.phased.vcf") == want
    # the module on the finished VCF
    out = phase.main(["--vcf", plain, "--bam", bam, "--output", str(tmp_path / "module.vcf"), "--phase_fragments",
                      "--q_threshold", str(thresholds[0]), "--mapq_threshold", str(thresholds[1])])
    assert read(out) == want
    # --haplotag --phase_fragments: pass 1 is that --phase --phase_fragments run
    _run(base + ["--haplotag", "--phase_fragments", "--workdir", work["two"]])
    for name in ("results.output.vcf", "results.output.phased.vcf"):
        assert read(work["two"], "haplotag_pass1", name) == read(work["joined"], name), name
    assert not os.path.exists(os.path.join(work["two"], "results.output.phased.vcf"))
