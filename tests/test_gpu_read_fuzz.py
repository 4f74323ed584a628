"""The BAM-side kernels on the fuzz corpus of tests/read_fuzz.py: every stage of sections 7f - 7k over every
seed and both profiles, integer for integer against its restatement -- which tests/test_read_fuzz.py holds to an independent
oracle on the same corpus -- then two kernels that must count one quantity alike, and the passes over a BAM at three span widths.
Every read set here is valid and has passed the host walks on the CPU."""
import numpy as np
import pytest

from hello_amd import gvcf, haplotag, markdup, phase, qc
from hello_amd.bam import BamFile
from tests import qc_cases, read_fuzz as rf
from tests.bam_writer import write_bam

pytestmark = pytest.mark.gpu

CORPORA = [(seed, profile) for seed in rf.SEEDS for profile in rf.PROFILES]
L = rf.LENGTH
EXCLUDED = [(0, 1), (1020, 1024), (1024, 1030), (2047, 2048), (2048, 2049), (2590, 2600)]      # they touch both tile edges


def same(got, want, names, where):
    for name in names:
        assert np.array_equal(np.asarray(got[name]), np.asarray(want[name])), where + (name,)


def test_qc_over_one_span_and_over_cut_spans():
    for seed, profile in CORPORA:
        reference, rows, _ = rf.corpus(seed, profile)
        want = rf.restated(seed, profile)
        cut = [(qc_cases.read_set(qc_cases.overlapping(rows, lo, min(lo + rf.SPAN, L))), lo, min(lo + rf.SPAN, L)) for lo in range(0, L, rf.SPAN)]
        for how, spans in (("one", [(want["reads"], 0, L)]), ("cut", cut)):
            tables, stats = qc.metered(spans, reference, rf.TARGETS, rf.WINDOW, rf.MAPQ_THRESHOLD)
            same(tables, want["tables"], qc.TABLE_NAMES, (seed, profile, how))
            assert {k: int(stats[k]) for k in qc.METRIC_STATS} == want["stats"], (seed, profile, how)


def test_refblocks_counts_and_blocks_from_one_and_two_read_sets():
    for seed, profile in CORPORA:
        reference, rows, _ = rf.corpus(seed, profile)
        want = rf.restated(seed, profile)
        blocks_want = gvcf.blocks_of(want["n_ref"], want["n_total"], EXCLUDED)
        for how, sets in (("one", [want["reads"]]), ("two", [qc_cases.read_set(rows[0::2]), qc_cases.read_set(rows[1::2])])):
            blocks, _, (n_ref, n_total) = gvcf.find_blocks(sets, reference, 0, L, EXCLUDED, rf.Q_THRESHOLD, rf.MAPQ_THRESHOLD, keep_counts=True)
            assert np.array_equal(n_total, want["n_total"]) and np.array_equal(n_ref, want["n_ref"]), (seed, profile, how)
            same(blocks, blocks_want, [f[0] for f in gvcf.FIELDS], (seed, profile, how))


def test_markdup_arrays():
    for seed, profile in CORPORA:
        want = rf.restated(seed, profile)
        got, stats = markdup.find_arrays(want["reads"])
        same(got, want["duplicates"], ("e", "score", "mate", "kind", "duplicate"), (seed, profile))
        assert {k: int(stats[k]) for k in markdup.COUNT_NAMES} == want["duplicates"]["counts"], (seed, profile)


def test_phase_observations_links_and_tags_with_and_without_fragments():
    seen = set()
    for seed, profile in CORPORA:
        _, _, records = rf.corpus(seed, profile)
        want = rf.restated(seed, profile)
        sets = [want["reads"]]
        slots, offsets, first = want["slots"]
        got, _ = phase.find_observations(sets, records, rf.Q_THRESHOLD, rf.MAPQ_THRESHOLD)
        same(got, dict(slots=slots, slot_offsets=offsets, first=first, links=phase.links_of(slots, offsets, first, len(records))),
             ("slots", "slot_offsets", "first", "links"), (seed, profile))
        positions = [rec.pos for rec in records]
        for fragments in (False, True):
            details: dict = {}
            hp, ps = phase.find_haplotags(sets, records, rf.Q_THRESHOLD, rf.MAPQ_THRESHOLD, details=details, fragments=fragments)
            mate = phase.mates_of(sets, rf.MAPQ_THRESHOLD) if fragments else None
            links = phase.links_of(slots, offsets, first, len(records), mate=mate)
            assert np.array_equal(details["fragment_links" if fragments else "links"], links), (seed, profile, fragments)
            if fragments:
                assert np.array_equal(details["mate"], mate), (seed, profile)
            chained, flip = phase.chain(links)
            assert np.array_equal(details["set"], chained) and np.array_equal(details["flip"], flip), (seed, profile, fragments)
            hp_want, ps_want = phase.haplotags_of(slots, offsets, first, chained, flip, positions, mate)
            assert np.array_equal(hp, hp_want) and np.array_equal(ps, ps_want), (seed, profile, fragments)
            seen |= set(hp.tolist())
    assert seen == {0, 1, 2}


def test_haplotagger_on_the_phased_records():
    seen = set()
    for seed, profile in CORPORA:
        want = rf.restated(seed, profile)
        with haplotag.Haplotagger(None, q_threshold=rf.Q_THRESHOLD, mapq_threshold=rf.MAPQ_THRESHOLD, records={"chrF": want["phased"]}) as tagger:
            hp, ps = tagger.tag("chrF", want["reads"])
        assert np.array_equal(hp, want["tags"][0]) and np.array_equal(ps, want["tags"][1]), (seed, profile)
        seen |= set(hp.tolist())
    assert seen == {0, 1, 2}


def test_refblocks_total_is_the_depth_of_qc_position_for_position():
    """Read bases all ACGT and no quality threshold: ``n_total`` and the depth both count the M / = / X / D bases of the counted
    reads, in two kernels that share no code.  window 1 puts 1 024 windows into a tile of ``qc_depth_kernel``, and the 1 024
    targets of one base over the second tile as many targets: both its declared limits."""
    targets = [(p, p + 1) for p in range(rf.TILE, 2 * rf.TILE)]
    for seed, profile in CORPORA:
        reference, rows, _ = rf.corpus(seed, profile, True)
        assert all(set(row[4]) <= set("ACGT") for row in rows)
        reads = qc_cases.read_set(rows)
        _, _, (_, n_total) = gvcf.find_blocks([reads], reference, 0, L, (), 0, rf.MAPQ_THRESHOLD, keep_counts=True)
        tables, _ = qc.metered([(reads, 0, L)], reference, targets, 1, rf.MAPQ_THRESHOLD)
        assert np.array_equal(tables["WINDOW_SUM"], n_total), (seed, profile)
        want, _ = qc.restated([(reads, 0, L)], reference, targets, 1, rf.MAPQ_THRESHOLD)
        same(tables, want, ("WINDOW_SUM", "DEPTH_HIST", "TARGET_DEPTH_HIST", "TARGET_SUM", "TARGET_COVERED"), (seed, profile))
        assert np.array_equal(tables["TARGET_SUM"], n_total[rf.TILE:2 * rf.TILE])


@pytest.mark.parametrize("profile", rf.PROFILES)
def test_cuts_do_not_matter(profile, tmp_path):
    """The passes over a BAM at max_span None, 700 and 97 -- neither divides the tile; the cuts fall into deletions, skips and
    pairs -- give equal bytes."""
    for seed in range(4):
        reference, rows, records = rf.corpus(seed, profile)
        path = str(tmp_path / ("%s%d.bam" % (profile, seed)))
        write_bam(path, [("chrF", L)], rf.bam_reads(rows), index=True, block_bytes=997)
        results = []
        for max_span in (None, 700, 97):
            metrics = qc.measure(path, {"chrF": reference}, targets={"chrF": rf.TARGETS}, window=rf.WINDOW, max_span=max_span)
            marks = markdup.find_duplicates(path, max_span=max_span)
            with BamFile(path) as handle:
                blocks = gvcf.chromosome_blocks([handle], "chrF", reference, EXCLUDED, rf.Q_THRESHOLD, rf.MAPQ_THRESHOLD,
                                                gvcf.DEFAULT_GQ_BINSIZE, max_span=max_span)
                phased = [phase.chromosome_phase([handle], "chrF", L, records, max_span=max_span, fragments=f) for f in (False, True)]
            results.append(dict(qc=metrics.tables["chrF"], identities=dict(zip("nms", marks.identities["chrF"])),
                                marks={k: np.int64(v) for k, v in marks.metrics["chrF"].items()}, blocks=blocks, phase=phased[0],
                                fragments=phased[1]))
        first = results[0]
        assert first["qc"]["STATS"][0] > 0 and first["blocks"]["start"].shape[0] > 1 and first["phase"]["slots"].shape[0] > 0
        for other, max_span in zip(results[1:], (700, 97)):
            for part, arrays in first.items():
                assert arrays.keys() == other[part].keys()
                for name, a in arrays.items():
                    b = other[part][name]
                    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (seed, max_span, part, name)
