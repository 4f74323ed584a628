"""The split alignments on the GPU (hello_sv_add_split, sv_split_kernel; hello_amd/csrc/sv.hip, sv_split.h): rows, SPLIT_STATUS,
statistics and candidates equal the restatement of hello_amd/sv.py integer for integer -- on the cases worked by hand, the stress
and the fuzz of tests/sv_split_cases.py, each whole and cut into spans and each twice with equal bytes; the refusals of a live
handle leave it as it was; a handle fed by ``add`` alone gives what it gave before; and the driver with ``--sv_split`` writes the
files of the restatement, leaves ``results.output.vcf`` alone, and without the option writes what it wrote before."""
import dataclasses
import os

import numpy as np
import pytest

from hello_amd import call, sv
from hello_amd.bam import Splits
from tests import sv_cases as sc, sv_split_cases as ss
from tests.test_sv import rows_of, same_tables, spans_of
from tests.test_sv_split import KW, clusters_of, fuzz_restated, same_split_tables, stress_restated

pytestmark = pytest.mark.gpu
MODEL_SEED = 1


def _bytes(tables) -> bytes:
    return b"".join(tables[k].tobytes() for k in sorted(tables))


def _same_counts(stats, counts):
    assert {k: int(stats[k]) for k in sv.SPLIT_METRIC_STATS} == {k: counts[k] for k in sv.SPLIT_METRIC_STATS}


# ---- (1) the hand cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ss.HAND_TABLE, ids=[c.name for c in ss.HAND_TABLE])
def test_hand_cases_through_the_kernels(case):
    length = len(case.reference)
    for cuts in ((), (case.cut(),)):
        spans = ss.spans_of(case.rows, length, cuts)
        want, counts = sv.restated(spans, case.reference, **ss.HAND, **KW)
        runs = []
        for _ in range(2):
            got, stats = sv.found_on_gpu(spans, case.reference, **ss.HAND, **KW)
            assert rows_of(got, "SIGNATURES_", sv.SIGNATURE_COLUMNS) == case.signatures
            assert clusters_of(got) == case.clusters
            same_split_tables(got, want)
            _same_counts(stats, counts)
            assert {k: int(stats[k]) for k in sv.SPLIT_COUNT_NAMES} == case.want_counts()
            assert np.array_equal(got["SPLIT_STATUS"], want["SPLIT_STATUS"]) and np.array_equal(got["STATUS"], want["STATUS"])
            runs.append(_bytes(got))
        assert runs[0] == runs[1]
    whole, _ = sv.found_on_gpu(ss.spans_of(case.rows, length), case.reference, **ss.HAND, **KW)
    assert whole["SPLIT_STATUS"].tolist() == case.split_status


# ---- (2) the stress ----------------------------------------------------------------------------------------------------------------
def test_stress_on_one_chromosome():
    reference, rows, _, want, counts = stress_restated()
    whole, cut = ss.spans_of(rows, ss.LENGTH), ss.spans_of(rows, ss.LENGTH, range(sc.SPAN, ss.LENGTH, sc.SPAN))
    assert len(cut) == 4
    runs = []
    for spans in (whole, cut, whole, cut):
        got, stats = sv.found_on_gpu(spans, reference, **ss.STRESS, **KW)
        same_split_tables(got, want)
        _same_counts(stats, counts)
        assert stats["split_ms"] > 0 and stats["reads_ms"] > 0
        runs.append(_bytes({k: v for k, v in got.items() if k not in ("STATUS", "SPLIT_STATUS")}))
    assert len(set(runs)) == 1
    got = sv.found_on_gpu(whole, reference, **ss.STRESS, **KW)[0]
    assert np.array_equal(got["SPLIT_STATUS"], want["SPLIT_STATUS"]) and np.array_equal(got["STATUS"], want["STATUS"])
    last = sv.restated(cut, reference, **ss.STRESS, **KW)[0]                   # per span: the status of the last one
    assert np.array_equal(sv.found_on_gpu(cut, reference, **ss.STRESS, **KW)[0]["SPLIT_STATUS"], last["SPLIT_STATUS"])


# ---- (3) the fuzz ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ss.FUZZ_SEEDS)
def test_fuzz_whole_and_cut(seed):
    reference, rows, want, counts = fuzz_restated(seed)
    whole = ss.spans_of(rows, ss.FUZZ_LENGTH)
    runs = []
    for spans in (whole, ss.spans_of(rows, ss.FUZZ_LENGTH, (400, 777, 1100)), whole):
        got, stats = sv.found_on_gpu(spans, reference, **ss.FUZZ, **KW)
        same_split_tables(got, want)
        _same_counts(stats, counts)
        runs.append(_bytes({k: v for k, v in got.items() if k not in ("STATUS", "SPLIT_STATUS")}))
    assert len(set(runs)) == 1
    assert np.array_equal(sv.found_on_gpu(whole, reference, **ss.FUZZ, **KW)[0]["SPLIT_STATUS"], want["SPLIT_STATUS"])


# ---- (4) the refusals through a live handle, and the two adds mixed ----------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was_and_the_adds_mix():
    reference, rows, _, want, counts = stress_restated()
    first, rest = ss.spans_of(rows, ss.LENGTH, (sc.SPAN,))
    reads, splits = rest[0], rest[1]
    p = ss.STRESS
    with sv.Caller(reference, p["min_size"], p["flank"], p["mapq_threshold"], 0, p["cluster_gap"], p["len_ratio_percent"], p["min_support"]) as caller:
        caller.set_contigs(ss.CONTIGS, ss.OWN)
        caller.add(*first)
        before, stats = caller.arrays(), caller.stats()
        assert (before["SIGNATURES_OP"] < 0).sum() > 3
        decreasing = splits.offsets.copy()
        decreasing[3:] = decreasing[2] - 1
        longer = reads.cigars.copy()
        longer[0] += 16
        for bad_reads, bad_splits, lo, said in ((reads, Splits(splits.bytes, decreasing), sc.SPAN, "SA offsets decrease"),
                                                (reads, Splits(splits.bytes[:-1], splits.offsets), sc.SPAN, "SA offsets end at"),
                                                (dataclasses.replace(reads, cigars=longer), splits, sc.SPAN, "CIGAR query length"),
                                                (reads, splits, sc.SPAN - 1, "begins below %d" % sc.SPAN)):
            with pytest.raises(RuntimeError, match=said):
                caller.add(bad_reads, lo, ss.LENGTH, splits=bad_splits)
            after = caller.arrays()
            assert all(after[k].tobytes() == before[k].tobytes() for k in before) and caller.stats() == stats, said
        with pytest.raises(RuntimeError, match="hello_sv_contigs twice"):
            caller.set_contigs(ss.CONTIGS, ss.OWN)
        caller.add(*rest)
        caller.finish()
        same_split_tables(caller.arrays(), want)
        _same_counts(caller.stats(), counts)
    # one span by add, the other by add_split: the first span's tags are not read
    mixed_want, mixed_counts = sv.restated([(first[0], first[2], first[3]), rest], reference, **p, **KW)
    mixed, stats = sv.found_on_gpu([(first[0], first[2], first[3]), rest], reference, **p, **KW)
    same_split_tables(mixed, mixed_want)
    _same_counts(stats, mixed_counts)
    assert 0 < mixed_counts["split_signatures"] < counts["split_signatures"]


def test_a_handle_fed_by_add_alone_gives_what_it_gave():
    reference, rows, _, _, _ = stress_restated()
    plain_rows = [r[:8] for r in rows]
    for cuts in ((), tuple(range(sc.SPAN, ss.LENGTH, sc.SPAN))):
        spans = spans_of(plain_rows, ss.LENGTH, cuts)
        want, counts = sv.restated(spans, reference, **ss.STRESS)
        got, stats = sv.found_on_gpu(spans, reference, **ss.STRESS)
        same_tables(got, want)
        assert "CANDIDATES_SR" not in got and "SPLIT_STATUS" not in got and np.array_equal(got["STATUS"], want["STATUS"])
        assert all(stats[k] == 0 for k in sv.SPLIT_COUNT_NAMES + ("split_ms",)) and {k: int(stats[k]) for k in sv.METRIC_STATS} == {k: counts[k] for k in sv.METRIC_STATS}
        # add_split over reads without any tag: the same arrays and counts, and no launch of the split kernel
        empty = [(rd, Splits(np.zeros(0, np.uint8), np.zeros(rd.n_reads + 1, np.int64)), lo, hi) for rd, lo, hi in spans]
        untagged, untagged_stats = sv.found_on_gpu(empty, reference, **ss.STRESS, **KW)
        assert not untagged.pop("CANDIDATES_SR").any() and not untagged["SPLIT_STATUS"].any()
        assert untagged.pop("SPLIT_STATUS").shape == got["STATUS"].shape and _bytes(untagged) == _bytes(got) and untagged_stats["split_ms"] == 0
        assert {k: untagged_stats[k] for k in sv.COUNT_NAMES + sv.SPLIT_COUNT_NAMES} == {k: stats[k] for k in sv.COUNT_NAMES + sv.SPLIT_COUNT_NAMES}


# ---- (5) the driver ----------------------------------------------------------------------------------------------------------------
_driver: dict = {}
DEL_AT, DEL_LEN = 2000, 400


def _run(argv):
    return call.main(call.parser().parse_args(argv))


def _read(*parts):
    return open(os.path.join(*parts), "rb").read()


def driver_input(tmp_path_factory):
    """The long reads of the 6 kb chromosome of the phasing tests as a PacBio BAM; a deletion of 400 bases at 2 000 that four reads
    carry as 400D and five as a split alignment (the primary before it, forward and reverse; the other segment in the SA tag); a model."""
    if not _driver:
        from hello_amd import loader, netspec as ns, weights
        from tests.bam_writer import Read
        from tests.test_gpu_candidates import _fasta, _write
        from tests.test_gpu_haplotag import chromosome
        c = chromosome()
        reference = c["reference"]
        planted = []
        for k in range(4):
            cigar = [(sc.M, 700 + 31 * k), (sc.D, DEL_LEN), (sc.M, 900)]
            seq = sc.realize(reference, DEL_AT - 700 - 31 * k, cigar)
            planted.append(Read("del%d" % k, DEL_AT - 700 - 31 * k, cigar, seq, [30] * len(seq), sc.REV * (k % 2)))
        for k in range(5):
            before, after = 650 + 23 * k, 800 + 11 * k
            start = DEL_AT - before
            seq = reference[start:DEL_AT] + reference[DEL_AT + DEL_LEN:DEL_AT + DEL_LEN + after]
            strand = "-" if k % 2 else "+"
            tag = b"SAZ" + ss.sa("chr1", DEL_AT + DEL_LEN, strand, "%dS%dM" % (before, after), 60, 3) + b"\0"
            planted.append(Read("split%d" % k, start, [(sc.M, before), (sc.S, after)], seq, [30] * len(seq), sc.REV * (k % 2), tags=tag))
        reads = sorted(list(c["long"]) + planted, key=lambda r: r.pos)
        tmp = tmp_path_factory.mktemp("sv_split_driver")
        model = str(tmp / "m.hello.npz")
        loader.save_native(model, "single_tech", weights.synth_state(ns.build("single_tech"), seed=MODEL_SEED))
        bam = _write(tmp, "p.bam", "chr1", reference, reads)
        _driver.update(tmp=tmp, bam=bam, genome={"chr1": reference},
                       tail=["--pbam", bam, "--ref", _fasta(tmp, "chr1", reference), "--network", model, "--from_bam"])
    return _driver


def test_the_driver_with_sv_split(tmp_path_factory):
    d = driver_input(tmp_path_factory)
    work = {name: str(d["tmp"] / name) for name in ("split", "plain", "want_split", "want_plain")}
    _run(["--workdir", work["split"], "--sv", "--sv_split"] + d["tail"])
    _run(["--workdir", work["plain"], "--sv"] + d["tail"])
    assert _read(work["split"], "results.output.vcf") == _read(work["plain"], "results.output.vcf")
    for name, split in (("want_split", True), ("want_plain", False)):
        os.makedirs(work[name])
        sv.measure(d["bam"], d["genome"], ["chr1"], restatement=True, split=split).write_all(os.path.join(work[name], "sv.pacbio"))
    for name in ("sv.pacbio.vcf", "sv.pacbio.npz"):
        assert _read(work["split"], name) == _read(work["want_split"], name), name
        assert _read(work["plain"], name) == _read(work["want_plain"], name), name
    want = sv.measure(d["bam"], d["genome"], ["chr1"], restatement=True, split=True)
    event = [c for c in want.candidates("chr1") if c["TYPE"] == sv.DEL and c["LEN"] == DEL_LEN]
    assert len(event) == 1 and event[0]["DV"] == 9 and event[0]["SR"] == 5 and event[0]["POS_MAX"] <= DEL_AT
    assert event[0]["DR"] == max(0, event[0]["DP"] - 4)
    plain = [c for c in sv.measure(d["bam"], d["genome"], ["chr1"], restatement=True).candidates("chr1") if c["LEN"] == DEL_LEN]
    assert len(plain) == 1 and plain[0]["DV"] == 4 and "SR" not in plain[0]
    text = _read(work["split"], "sv.pacbio.vcf").decode()
    assert "SVLEN=-%d;END=%d;SUPPORT=9;" % (DEL_LEN, event[0]["POS"] + DEL_LEN) in text and ";SR=5\t" in text and "##INFO=<ID=SR," in text
    assert ";SR=" not in _read(work["plain"], "sv.pacbio.vcf").decode()
