"""The large deletions and insertions on the GPU (hello_sv_*; hello_amd/csrc/sv.hip): the SIGNATURES and CANDIDATES arrays equal the
restatement of hello_amd/sv.py integer for integer, whole and with the chromosome cut into spans, and two runs give the same bytes --
on the cases worked by hand (tests/sv_cases.py), on the edge stress, on the fuzz corpus of tests/read_fuzz.py against a derivation
from its alignment table as well, through the refusals of a live handle, and through the driver, where ``--sv`` writes the files the
restatement writes and leaves the VCF alone."""
import dataclasses
import os

import numpy as np
import pytest

from hello_amd import call, sv
from tests import read_fuzz as rf, sv_cases as sc
from tests.test_sv import FUZZ, assert_situations, independent, rows_of, same_tables, spans_of, stress_restated, with_hp

pytestmark = pytest.mark.gpu
MODEL_SEED = 1


def _bytes(tables) -> bytes:
    return b"".join(tables[k].tobytes() for k in sorted(tables))


def _same_counts(stats, counts):
    assert {k: int(stats[k]) for k in sv.METRIC_STATS} == {k: counts[k] for k in sv.METRIC_STATS}


# ---- (1) the hand tables through the kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.HAND_TABLE, ids=[c.name for c in sc.HAND_TABLE])
def test_hand_table_through_the_kernels(case):
    length = len(case.reference)
    for cuts in ((), (case.cut(),)):
        spans = spans_of(case.rows, length, cuts)
        want, counts = sv.restated(spans, case.reference, **sc.HAND)
        runs = []
        for _ in range(2):
            got, stats = sv.found_on_gpu(spans, case.reference, **sc.HAND)
            assert rows_of(got, "SIGNATURES_", sv.SIGNATURE_COLUMNS) == case.signatures
            assert rows_of(got, "CANDIDATES_", sv.CANDIDATE_COLUMNS) == case.candidates
            same_tables(got, want)
            _same_counts(stats, counts)
            assert {k: int(stats[k]) for k in sv.METRIC_STATS} == case.want_counts()
            assert int(stats["reads_given"]) == sum(rd.n_reads for rd, _, _ in spans)
            assert np.array_equal(got["STATUS"], want["STATUS"])
            runs.append(_bytes(got))
        assert runs[0] == runs[1]
    whole, _ = sv.found_on_gpu(spans_of(case.rows, length), case.reference, **sc.HAND)
    assert whole["STATUS"].tolist() == case.status


# ---- (2) the edge stress --------------------------------------------------------------------------------------------------------
def test_edge_stress_on_one_chromosome():
    reference, rows, named, want, counts = stress_restated()
    assert_situations(reference, rows, named, want, counts)                  # each situation really occurs
    whole, cut = spans_of(rows, sc.LENGTH), spans_of(rows, sc.LENGTH, range(sc.SPAN, sc.LENGTH, sc.SPAN))
    assert len(cut) == 4 and any(rd.n_reads for rd, _, _ in cut[1:])
    runs = []
    for spans in (whole, cut, whole, cut):
        got, stats = sv.found_on_gpu(spans, reference, **sc.STRESS)
        same_tables(got, want)
        _same_counts(stats, counts)
        assert stats["cover_ms"] > 0 and stats["reads_ms"] > 0 and stats["finish_ms"] > 0
        runs.append(_bytes({k: v for k, v in got.items() if k != "STATUS"}))
    assert len(set(runs)) == 1
    assert np.array_equal(sv.found_on_gpu(whole, reference, **sc.STRESS)[0]["STATUS"], want["STATUS"])
    with sv.Caller(reference, sc.STRESS["min_size"], sc.STRESS["flank"]) as caller:      # the signatures are there before finish
        caller.add(*whole[0])
        before = caller.arrays()
        assert "CANDIDATES_POS" not in before and np.array_equal(before["SIGNATURES_POS"], want["SIGNATURES_POS"])
        caller.finish(sc.STRESS["cluster_gap"], sc.STRESS["len_ratio_percent"], sc.STRESS["min_support"])
        same_tables(caller.arrays(), want)


# ---- (3) the fuzz ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", rf.PROFILES)
@pytest.mark.parametrize("seed", rf.SEEDS)
def test_fuzz_corpus_whole_and_cut(seed, profile):
    reference, rows, _ = rf.corpus(seed, profile)
    rows8 = with_hp(rows)
    L = rf.LENGTH
    whole = spans_of(rows8, L)
    want, counts = sv.restated(whole, reference, **FUZZ)
    signatures, spanning = independent(reference, rows)
    assert rows_of(want, "SIGNATURES_", sv.SIGNATURE_COLUMNS) == signatures
    assert np.array_equal(np.cumsum(want["DIFF"]), spanning)
    assert want["CANDIDATES_DP"].tolist() == [int(spanning[p]) for p in want["CANDIDATES_POS"]]
    runs = []
    for spans in (whole, spans_of(rows8, L, rf.CUTS), whole):
        got, stats = sv.found_on_gpu(spans, reference, **FUZZ)
        same_tables(got, want)
        _same_counts(stats, counts)
        runs.append(_bytes({k: v for k, v in got.items() if k != "STATUS"}))
    assert len(set(runs)) == 1


# ---- (4) the refusals through a live handle ---------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    reference, rows, _, want, _ = stress_restated()
    first, rest = spans_of(rows, sc.LENGTH, (sc.SPAN,))
    reads = rest[0]
    p = sc.STRESS
    with sv.Caller(reference, p["min_size"], p["flank"], p["mapq_threshold"], 0, p["cluster_gap"], p["len_ratio_percent"], p["min_support"]) as caller:
        caller.add(*first)
        before, stats = caller.arrays(), caller.stats()
        assert before["SIGNATURES_POS"].shape[0] > 5
        decreasing = reads.read_offsets.copy()
        decreasing[3] = decreasing[2] - 1
        longer = reads.cigars.copy()
        longer[0] += 16
        for bad, lo, hi, said in ((dataclasses.replace(reads, read_offsets=decreasing), sc.SPAN, sc.LENGTH, "offsets decrease"),
                                  (dataclasses.replace(reads, cigars=longer), sc.SPAN, sc.LENGTH, "CIGAR query length"),
                                  (dataclasses.replace(reads, ref_ends=reads.ref_ends + 1), sc.SPAN, sc.LENGTH, "ref_end does not match"),
                                  (reads, sc.SPAN - 1, sc.LENGTH, r"begins below %d, where the previous one ended" % sc.SPAN),
                                  (reads, sc.SPAN, sc.LENGTH + 1, r"span \[%d, %d\)" % (sc.SPAN, sc.LENGTH + 1))):
            with pytest.raises(RuntimeError, match=said):
                caller.add(bad, lo, hi)
            after = caller.arrays()
            assert all(after[k].tobytes() == before[k].tobytes() for k in before) and caller.stats() == stats, said
        with pytest.raises(RuntimeError, match="min_support 0"):
            caller.finish(min_support=0)
        assert caller.stats() == stats
        caller.add(*rest)
        caller.finish()
        done, done_stats = caller.arrays(), caller.stats()
        same_tables(done, want)
        with pytest.raises(RuntimeError, match="hello_sv_finish twice"):
            caller.finish()
        with pytest.raises(RuntimeError, match="hello_sv_add after hello_sv_finish"):
            caller.add(*rest)
        after = caller.arrays()
        assert all(after[k].tobytes() == done[k].tobytes() for k in done) and caller.stats() == done_stats
    with pytest.raises(RuntimeError, match="device 99"):
        sv.found_on_gpu([first], reference, **sc.STRESS, device=99)


# ---- (5) the driver -------------------------------------------------------------------------------------------------------------
_driver: dict = {}
DEL_AT, DEL_LEN, INS_AT, INS_LEN = 2000, 120, 4000, 90


def _run(argv):
    return call.main(call.parser().parse_args(argv))


def _read(*parts):
    return open(os.path.join(*parts), "rb").read()


def driver_input(tmp_path_factory):
    """The long reads of the 6 kb chromosome of the phasing tests as a PacBio BAM, six more with a deletion of 120 bases at 2 000 and
    five with an insertion of 90 at 4 000; and a model."""
    if not _driver:
        from hello_amd import loader, netspec as ns, weights
        from tests.bam_writer import Read
        from tests.test_gpu_candidates import _fasta, _write
        from tests.test_gpu_haplotag import chromosome
        c = chromosome()
        reference = c["reference"]
        rng = np.random.default_rng(5)
        inserted = "".join(rng.choice(list("ACGT"), size=INS_LEN))
        planted = []
        for k in range(6):
            cigar = [(sc.M, 700 + 31 * k), (sc.D, DEL_LEN), (sc.M, 900)]
            seq = sc.realize(reference, DEL_AT - 700 - 31 * k, cigar)
            planted.append(Read("del%d" % k, DEL_AT - 700 - 31 * k, cigar, seq, [30] * len(seq), sc.REV * (k % 2)))
        for k in range(5):
            cigar = [(sc.M, 800 + 17 * k), (sc.I, INS_LEN), (sc.M, 600)]
            seq = sc.realize(reference, INS_AT - 800 - 17 * k, cigar, {1: inserted})
            planted.append(Read("ins%d" % k, INS_AT - 800 - 17 * k, cigar, seq, [30] * len(seq), sc.REV * (k % 2)))
        reads = sorted(list(c["long"]) + planted, key=lambda r: r.pos)
        tmp = tmp_path_factory.mktemp("sv_driver")
        model = str(tmp / "m.hello.npz")
        loader.save_native(model, "single_tech", weights.synth_state(ns.build("single_tech"), seed=MODEL_SEED))
        bam = _write(tmp, "p.bam", "chr1", reference, reads)
        _driver.update(tmp=tmp, bam=bam, genome={"chr1": reference},
                       tail=["--pbam", bam, "--ref", _fasta(tmp, "chr1", reference), "--network", model, "--from_bam"])
    return _driver


@pytest.mark.parametrize("resident", [False, True], ids=["shards", "resident"])
def test_the_driver_writes_the_files_of_the_restatement_and_leaves_the_vcf_alone(resident, tmp_path_factory):
    d = driver_input(tmp_path_factory)
    tail = d["tail"] + (["--resident"] if resident else [])
    work = {name: str(d["tmp"] / ("%s_%d" % (name, resident))) for name in ("found", "plain", "want")}
    _run(["--workdir", work["found"], "--sv"] + tail)
    _run(["--workdir", work["plain"]] + tail)
    assert _read(work["found"], "results.output.vcf") == _read(work["plain"], "results.output.vcf")
    assert not [f for f in os.listdir(work["plain"]) if f.startswith("sv.")]
    os.makedirs(work["want"])
    want = sv.measure(d["bam"], d["genome"], ["chr1"], restatement=True)
    want.write_all(os.path.join(work["want"], "sv.pacbio"))
    for name in ("sv.pacbio.vcf", "sv.pacbio.npz"):
        assert _read(work["found"], name) == _read(work["want"], name), name
    assert not os.path.exists(os.path.join(work["found"], "sv.illumina.vcf"))
    events = {(c["TYPE"], c["LEN"]): c for c in want.candidates("chr1")}
    deletion, insertion = events[(sv.DEL, DEL_LEN)], events[(sv.INS, INS_LEN)]
    assert deletion["DV"] == 6 and deletion["POS_MAX"] <= DEL_AT and insertion["DV"] == 5 and insertion["POS_MAX"] <= INS_AT
    assert deletion["DP"] >= 6 and deletion["DR"] == deletion["DP"] - 6
    lines = [line.split("\t") for line in _read(work["found"], "sv.pacbio.vcf").decode().splitlines() if not line.startswith("#")]
    assert [(f[4], f[9].split(":")[0]) for f in lines] == [("<%s>" % sv.TYPE_NAMES[c["TYPE"]], sv.GT_TEXT[c["GT"]]) for c in want.candidates("chr1")]
    assert {"<DEL>", "<INS>"} <= {f[4] for f in lines} and any("SVLEN=-%d;" % DEL_LEN in f[7] for f in lines)


def test_the_module_s_own_command_line_and_the_haplotypes_of_a_phased_vcf(tmp_path_factory):
    d = driver_input(tmp_path_factory)
    work = {name: str(d["tmp"] / name) for name in ("phased", "own", "want_phased", "want_plain")}
    for name in ("own", "want_phased", "want_plain"):
        os.makedirs(work[name])
    # with --phase the haplotypes are what the Haplotagger gives the reads from the phased VCF written just before
    from hello_amd import haplotag as ht
    _run(["--workdir", work["phased"], "--sv", "--phase", "--sv_min_support", "5"] + d["tail"])
    phased = os.path.join(work["phased"], "results.output.phased.vcf")
    with ht.Haplotagger(phased, ["chr1"]) as tagger:
        fed = sv.measure(d["bam"], d["genome"], ["chr1"], tagger, min_support=5, restatement=True)
    fed.write_all(os.path.join(work["want_phased"], "sv.pacbio"))
    for name in ("sv.pacbio.vcf", "sv.pacbio.npz"):
        assert _read(work["phased"], name) == _read(work["want_phased"], name), name
    tagged = [c["HP1"] + c["HP2"] for c in fed.candidates("chr1")]
    assert len(tagged) == 2 and sum(tagged) > 0                            # min_support 5 keeps both events; reads were tagged
    # python -m hello_amd.sv on the BAM alone: the BAM's own HP tags (it has none)
    written = sv.main(["--bam", d["bam"], "--ref", d["tail"][3], "--output_prefix", os.path.join(work["own"], "sv"), "--chromosomes", "chr1"])
    assert [os.path.basename(p) for p in written] == ["sv.vcf", "sv.npz"]
    plain = sv.measure(d["bam"], d["genome"], ["chr1"], restatement=True)
    plain.write_all(os.path.join(work["want_plain"], "sv"))
    for name in ("sv.vcf", "sv.npz"):
        assert _read(work["own"], name) == _read(work["want_plain"], name), name
    assert all(c["HP1"] + c["HP2"] == 0 for c in plain.candidates("chr1"))
