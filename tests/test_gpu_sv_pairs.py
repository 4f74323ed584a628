"""The read pairs and clipped ends on the GPU (hello_sv_add_pairs, sv_pairs_kernel, sv_clips_kernel; hello_amd/csrc/sv.hip,
sv_pairs.h): rows, PAIR_STATUS, INNER, the clip arrays, statistics and candidates equal the restatement of hello_amd/sv.py integer
for integer -- on the cases worked by hand, the stress and the fuzz of tests/sv_pairs_cases.py, each whole and cut into spans and
each twice with equal bytes; the refusals of a live handle leave it as it was; ``hello_sv_add`` and ``hello_sv_add_split`` give on
the same reads what they gave; a library sampled on the GPU is the restatement's; and the driver with ``--sv_pairs`` writes the
files of the restatement, leaves ``results.output.vcf`` alone, and without the option writes what it wrote before."""
import dataclasses
import os

import numpy as np
import pytest

from hello_amd import call, sv
from hello_amd.bam import Mates, Splits
from tests import sv_cases as sc, sv_pairs_cases as pc
from tests.test_sv import rows_of
from tests.test_sv_pairs import _mated_reads, clusters_of, fuzz_restated, restated, stress_restated

pytestmark = pytest.mark.gpu
KW = dict(contigs=pc.CONTIGS, own=pc.OWN)
PER_SPAN = ("STATUS", "SPLIT_STATUS", "PAIR_STATUS")


def on_gpu(spans, reference, library, params):
    p = dict(params)
    clip_min = p.pop("clip_min")
    return sv.found_on_gpu(spans, reference, **p, **KW, library=library, clip_min=clip_min)


def same_pair_tables(got, want, per_span=True):
    """Every array of both getters, integer for integer and of the same type; DIFF is the restatement's alone."""
    assert set(got) == set(want) - {"DIFF"}
    for k in got:
        if per_span or k not in PER_SPAN:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def same_counts(stats, counts):
    assert {k: int(stats[k]) for k in sv.PAIR_METRIC_STATS} == {k: counts[k] for k in sv.PAIR_METRIC_STATS}


def _bytes(tables) -> bytes:
    return b"".join(tables[k].tobytes() for k in sorted(tables) if k not in PER_SPAN)


# ---- (1) the hand cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.HAND_TABLE, ids=[c.name for c in pc.HAND_TABLE])
def test_hand_cases_through_the_kernels(case):
    for cuts in ((), (case.cut(),)):
        spans = pc.spans_of(case.rows, pc.LENGTH, cuts)
        want, counts = restated(case.rows, case.reference, pc.LIBRARY, case.kw(), cuts)
        runs = []
        for _ in range(2):
            got, stats = on_gpu(spans, case.reference, pc.LIBRARY, case.kw())
            assert rows_of(got, "SIGNATURES_", sv.SIGNATURE_COLUMNS) == case.signatures
            assert clusters_of(got) == case.clusters
            same_pair_tables(got, want)
            same_counts(stats, counts)
            assert {k: int(stats[k]) for k in sv.PAIR_COUNT_NAMES} == case.want_counts()
            runs.append(_bytes(got))
        assert runs[0] == runs[1]
        if not cuts:
            assert got["PAIR_STATUS"].tolist() == case.pair_status


def test_clip_arrays_of_the_hand_case():
    got, _ = on_gpu(pc.spans_of(pc.CLIP_CASE.rows, pc.LENGTH), pc.REFERENCE, pc.LIBRARY, pc.HAND)
    for name, want in pc.CLIPS.items():
        assert got[name].dtype == np.int32 and {int(i): int(got[name][i]) for i in np.flatnonzero(got[name])} == want
    # reads that end beyond the chromosome touch no array; those that end at its last position count in the last entry
    got, _ = on_gpu(pc.spans_of(pc.END_CASE.rows, pc.LENGTH), pc.REFERENCE, pc.LIBRARY, pc.HAND)
    for name, want in pc.END_CLIPS.items():
        assert got[name].shape == (pc.LENGTH + 1,) and {int(i): int(got[name][i]) for i in np.flatnonzero(got[name])} == want
    assert {int(i): int(got["INNER"][i]) for i in np.flatnonzero(got["INNER"])} == {1024: 1} and got["PAIR_STATUS"].tolist() == [0, 0, 1, 0, 4]


# ---- (2) the stress ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.STRESS_SETS))
def test_stress_sets_whole_cut_and_twice(name):
    rows = pc.STRESS_SETS[name]
    want, counts = stress_restated(name)
    whole, cut = pc.spans_of(rows, pc.STRESS_LENGTH), pc.spans_of(rows, pc.STRESS_LENGTH, pc.STRESS_CUTS)
    runs = []
    for spans in (whole, cut, whole, cut):
        got, stats = on_gpu(spans, pc.STRESS_REFERENCE, pc.STRESS_LIBRARY, pc.STRESS)
        same_pair_tables(got, want, per_span=spans is whole)
        same_counts(stats, counts)
        assert (stats["pairs_ms"] > 0) == (name != "no_pairs")               # a span without a paired or clipped read launches nothing
        runs.append(_bytes(got))
    assert len(set(runs)) == 1


# ---- (3) the fuzz ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", pc.FUZZ_SEEDS)
def test_fuzz_whole_and_cut(seed):
    reference, rows, want, counts = fuzz_restated(seed)
    whole = pc.spans_of(rows, pc.FUZZ_LENGTH)
    runs = []
    for spans in (whole, pc.spans_of(rows, pc.FUZZ_LENGTH, (400, 777, 1100, 2048)), whole):
        got, stats = on_gpu(spans, reference, pc.FUZZ_LIBRARY, pc.FUZZ)
        same_pair_tables(got, want, per_span=spans is whole)
        same_counts(stats, counts)
        runs.append(_bytes(got))
    assert len(set(runs)) == 1


# ---- (4) the refusals through a live handle, the adds mixed, and the two old adds unchanged -----------------------------------------
def test_refusals_leave_the_handle_as_it_was_and_the_adds_mix():
    reference, rows, want, counts = fuzz_restated(pc.FUZZ_SEEDS[0])
    first, rest = pc.spans_of(rows, pc.FUZZ_LENGTH, (1100,))
    reads, splits, mates = rest[:3]
    p = pc.FUZZ
    with sv.Caller(reference, p["min_size"], p["flank"], p["mapq_threshold"], 0, p["cluster_gap"], p["len_ratio_percent"], p["min_support"]) as caller:
        caller.set_contigs(pc.CONTIGS, pc.OWN)
        caller.set_library(*pc.FUZZ_LIBRARY, clip_min=p["clip_min"])
        caller.add(*first)
        before, stats = caller.arrays(), caller.stats()
        assert (before["SIGNATURES_OP"] == sv.PAIR_OP).sum() > 3 and before["INNER"].sum() > 3 and before["CLIP_RIGHT"].sum() > 0
        longer = reads.cigars.copy()
        only_pairs = [r for r in range(reads.n_reads) if reads.ref_starts[r] >= 1100 and not reads.flags[r] & 0x2
                      and sv.pair_counted(int(reads.flags[r]), int(reads.mapq[r]), p["mapq_threshold"])]
        discordant = only_pairs[0]                                           # a CIGAR only the pair rules read: it is validated too
        longer[int(reads.cigar_offsets[discordant])] += 16
        decreasing = splits.offsets.copy()
        decreasing[3:] = decreasing[2] - 1
        for bad, lo, said in (((dataclasses.replace(reads, cigars=longer), splits, mates), 1100, "CIGAR query length"),
                              ((reads, Splits(splits.bytes, decreasing), mates), 1100, "SA offsets decrease"),
                              ((reads, splits, mates), 1099, "begins below 1100")):
            with pytest.raises(RuntimeError, match=said):
                caller.add(*bad, lo, pc.FUZZ_LENGTH)
            after = caller.arrays()
            assert all(after[k].tobytes() == before[k].tobytes() for k in before) and caller.stats() == stats, said
        with pytest.raises(RuntimeError, match="hello_sv_library twice"):
            caller.set_library(*pc.FUZZ_LIBRARY)
        with pytest.raises(RuntimeError, match="hello_sv_clip_min after hello_sv_add_pairs"):
            sv.check(caller._lib.hello_sv_clip_min(caller._h, 7))
        caller.add(*rest)
        caller.finish()
        same_pair_tables(caller.arrays(), want, per_span=False)
        same_counts(caller.stats(), counts)
    # one span by add_split, the other by add_pairs: the first span's mate fields and clips are not read
    mixed, stats = on_gpu([(first[0], first[1], first[3], first[4]), rest], reference, pc.FUZZ_LIBRARY, p)
    later = restated([r for r in rows if r[2] >= 1100], reference, pc.FUZZ_LIBRARY, p)[1]
    assert int(stats["pair_reads"]) == later["pair_reads"] and 0 < later["pair_reads"] < counts["pair_reads"]
    assert int(stats["counting"]) == counts["counting"] and int(stats["split_reads"]) == counts["split_reads"]
    assert mixed["PAIR_STATUS"].shape == (rest[0].n_reads,)


@pytest.mark.parametrize("seed", pc.FUZZ_SEEDS[:4])
def test_the_two_old_adds_give_on_the_same_reads_what_they_gave(seed):
    from tests.test_sv import same_tables
    reference, rows, want, counts = fuzz_restated(seed)
    p = {k: v for k, v in pc.FUZZ.items() if k != "clip_min"}
    whole = pc.spans_of(rows, pc.FUZZ_LENGTH)
    plain = [(s[0], s[3], s[4]) for s in whole]
    got, stats = sv.found_on_gpu(plain, reference, **p)
    old, old_counts = sv.restated(plain, reference, **p)
    same_tables(got, old)
    assert set(got) == {"SIGNATURES_" + n for n in sv.SIGNATURE_COLUMNS} | {"CANDIDATES_" + n for n in sv.CANDIDATE_COLUMNS} | {"STATUS"}
    assert set(stats) == set(sv.STAT_NAMES) and {k: int(stats[k]) for k in sv.METRIC_STATS} == {k: old_counts[k] for k in sv.METRIC_STATS}
    split = [(s[0], s[1], s[3], s[4]) for s in whole]
    got, stats = sv.found_on_gpu(split, reference, **p, **KW)
    old, old_counts = sv.restated(split, reference, **p, **KW)
    same_tables(got, old)
    assert np.array_equal(got["CANDIDATES_SR"], old["CANDIDATES_SR"]) and np.array_equal(got["SPLIT_STATUS"], old["SPLIT_STATUS"])
    assert "INNER" not in got and set(stats) == set(sv.STAT_NAMES)
    assert {k: int(stats[k]) for k in sv.SPLIT_METRIC_STATS} == {k: old_counts[k] for k in sv.SPLIT_METRIC_STATS}
    # and the rows of a handle with pairs that are no pair rows are those rows
    own = want["SIGNATURES_OP"] != sv.PAIR_OP
    for name in sv.SIGNATURE_COLUMNS:
        assert np.array_equal(want["SIGNATURES_" + name][own], old["SIGNATURES_" + name])


# ---- (5) the library ---------------------------------------------------------------------------------------------------------------
def test_a_library_sampled_on_the_gpu_is_the_restatements(tmp_path):
    from tests.mate_writer import write_bam
    rng = np.random.default_rng(13)
    rows = []
    for k in range(400):
        s = 10 + 6 * k
        rows += pc.fr_pair(2 * k, s, s + 10 + int(rng.integers(2, 40)), extra=pc.PROPER)
    rows = sorted(rows, key=lambda r: r[2])
    path = str(tmp_path / "library.bam")
    write_bam(path, [("chr1", pc.LENGTH)], _mated_reads(rows, pc.REFERENCE))
    genome = {"chr1": pc.REFERENCE}
    for kw in (dict(), dict(max_span=700, k=5)):
        want = sv.sampled_library(path, genome, restatement=True, **kw)
        assert sv.sampled_library(path, genome, **kw) == want
    inner = np.bincount([r[10] - (r[2] + 10) + 1024 for r in rows if r[1] & pc.FIRST], minlength=4096)
    assert sv.sampled_library(path, genome) == sv.library_of(inner, 8) and inner.sum() == 400
    # a BAM without a paired read has no library and needs none: the unset triple, and the pairs path gives what --sv_split gives
    from tests.bam_writer import Read, write_bam as write_plain
    rows = sorted([r for r in pc.HAND_TABLE[0].rows if not r[1] & pc.PAIRED] + pc.CLIP_CASE.rows[:5], key=lambda r: r[2])
    unpaired = str(tmp_path / "unpaired.bam")
    write_plain(unpaired, [("chr1", pc.LENGTH)], [Read("r%d" % k, r[2], r[3], r[4], r[5], flag=r[1], mapq=r[6]) for k, r in enumerate(rows)])
    assert sv.sampled_library(unpaired, genome) == sv.UNSET_LIBRARY
    kw = dict(min_size=5, flank=3, cluster_gap=10, len_ratio_percent=70, min_support=3, pairs=True, clip_min=4)
    got, want = sv.measure(unpaired, genome, **kw), sv.measure(unpaired, genome, restatement=True, **kw)
    assert got.vcf_text() == want.vcf_text() and got.library == sv.UNSET_LIBRARY and got.total() == want.total()
    assert got.total()["pair_reads"] == 0 and got.total()["clipped_reads"] == 3 and got.total()["candidates"] == 1


# ---- (6) the driver ----------------------------------------------------------------------------------------------------------------
_driver: dict = {}
DEL_AT, DEL_LEN = 5000, 300
LIBRARY_TEXT, LIBRARY = "200,100,300", (200, 100, 300)


def _run(argv):
    return call.main(call.parser().parse_args(argv))


def _read(*parts):
    return open(os.path.join(*parts), "rb").read()


def driver_input(tmp_path_factory):
    """The short reads of the 20 kb chromosome of the resident tests as an Illumina BAM, and a deletion of 300 bases at 5 000 that six
    discordant pairs straddle, two reads show as a split alignment and three as a clipped end; a model."""
    if not _driver:
        from hello_amd import loader, netspec as ns, weights
        from tests.mate_writer import MatedRead, write_bam
        from tests.test_gpu_candidates import _fasta
        from tests.test_gpu_resident import illumina_input
        from tests import sv_split_cases as ss
        reference, reads = illumina_input()
        planted = []
        for k in range(6):                                                   # a = s + 150, b = ms: (b - a) - 300 = 180 + 5 k
            s, ms = 4700 + 10 * k, 5330 + 15 * k
            planted.append(MatedRead("pair%d" % k, s, [(sc.M, 150)], reference[s:s + 150], [30] * 150, flag=pc.PAIRED | pc.MREV | pc.FIRST,
                                     next_ref_id=0, next_pos=ms, tlen=ms + 150 - s))
            planted.append(MatedRead("pair%d" % k, ms, [(sc.M, 150)], reference[ms:ms + 150], [30] * 150,
                                     flag=pc.PAIRED | sc.REV | pc.SECOND, next_ref_id=0, next_pos=s, tlen=s - ms - 150))
        for k in range(2):
            before, after = 80 + 7 * k, 70 - 7 * k
            seq = reference[DEL_AT - before:DEL_AT] + reference[DEL_AT + DEL_LEN:DEL_AT + DEL_LEN + after]
            tag = b"SAZ" + ss.sa("chr1", DEL_AT + DEL_LEN, "+", "%dS%dM" % (before, after), 60, 0) + b"\0"
            planted.append(MatedRead("split%d" % k, DEL_AT - before, [(sc.M, before), (sc.S, after)], seq, [30] * 150, tags=tag))
        for k in range(3):
            seq = reference[DEL_AT - 100 - k:DEL_AT] + reference[DEL_AT + DEL_LEN:DEL_AT + DEL_LEN + 50 - k]
            planted.append(MatedRead("clip%d" % k, DEL_AT - 100 - k, [(sc.M, 100 + k), (sc.S, 50 - k)], seq, [30] * 150))
        reads = sorted(list(reads) + planted, key=lambda r: r.pos)
        tmp = tmp_path_factory.mktemp("sv_pairs_driver")
        model = str(tmp / "m.hello.npz")
        loader.save_native(model, "single_tech", weights.synth_state(ns.build("single_tech"), seed=17))
        bam = str(tmp / "i.bam")
        write_bam(bam, [("chr1", len(reference))], reads, index=True, block_bytes=20000)
        _driver.update(tmp=tmp, bam=bam, genome={"chr1": reference},
                       tail=["--ibam", bam, "--ref", _fasta(tmp, "chr1", reference), "--network", model, "--from_bam", "--sv_min_support", "2"])
    return _driver


def test_the_driver_with_sv_pairs(tmp_path_factory):
    d = driver_input(tmp_path_factory)
    work = {name: str(d["tmp"] / name) for name in ("pairs", "split", "want_pairs", "want_split")}
    _run(["--workdir", work["pairs"], "--sv", "--sv_split", "--sv_pairs", "--sv_pairs_library", LIBRARY_TEXT] + d["tail"])
    _run(["--workdir", work["split"], "--sv", "--sv_split"] + d["tail"])
    assert _read(work["pairs"], "results.output.vcf") == _read(work["split"], "results.output.vcf")
    for name, kw in (("want_pairs", dict(split=True, pairs=True, library=LIBRARY)), ("want_split", dict(split=True))):
        os.makedirs(work[name])
        sv.measure(d["bam"], d["genome"], ["chr1"], min_support=2, restatement=True, **kw).write_all(os.path.join(work[name], "sv.illumina"))
    for name in ("sv.illumina.vcf", "sv.illumina.npz"):
        assert _read(work["pairs"], name) == _read(work["want_pairs"], name), name
        assert _read(work["split"], name) == _read(work["want_split"], name), name
    assert sorted(os.listdir(work["pairs"])) == sorted(os.listdir(work["split"]))
    want = sv.measure(d["bam"], d["genome"], ["chr1"], min_support=2, restatement=True, split=True, pairs=True, library=LIBRARY)
    event = [c for c in want.candidates("chr1") if c["TYPE"] == sv.DEL and c["LEN"] == DEL_LEN]
    assert len(event) == 1 and (event[0]["DV"], event[0]["SR"], event[0]["PR"], event[0]["CE"], event[0]["IMPRECISE"]) == (2, 2, 6, 3, 0)
    text = _read(work["pairs"], "sv.illumina.vcf").decode()
    assert "SVLEN=-%d;END=%d;SUPPORT=8;" % (DEL_LEN, event[0]["POS"] + DEL_LEN) in text and ";SR=2;PR=6;CE=3\t" in text
    assert "##INFO=<ID=PR," in text and "##INFO=<ID=PR," not in _read(work["split"], "sv.illumina.vcf").decode()
    with np.load(os.path.join(work["pairs"], "sv.illumina.npz")) as z:
        assert z["library"].tolist() == list(LIBRARY) and str(z["library_source"]) == "given"
