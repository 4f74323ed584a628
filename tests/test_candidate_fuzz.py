"""The fuzz corpus of tests/candidate_fuzz.py on the CPU: the corpus layer, the oracle that walks no CIGAR
against the three restatements on every corpus of every route, every rule of the oracle shown to be reached, the census of what
the corpora contain, and the hand-built read sets of the census lines no corpus reaches."""
import dataclasses
from collections import Counter

import pytest

from tests import candidate_fuzz as cf
from tests import candidate_reference as cr
from tests import pacbio_reference as pr
from tests import read_fuzz as rf

CASES = [(route, pad) for route in cf.ROUTES for pad in (True, False)]


def test_the_padded_corpus_is_the_corpus_shifted_and_the_additions_are_appended():
    assert cf.PAD_LEFT % cf.K_TILE == 0 and cf.PAD_RIGHT >= 1600 and cf.LENGTH == 4904
    for seed in (0, 11, 31):
        for profile in rf.PROFILES:
            reference, rows, records = cf.padded(seed, profile)
            plain, plain_rows, plain_records = rf.corpus(seed, profile)
            assert len(reference) == cf.LENGTH and reference[cf.PAD_LEFT:cf.PAD_LEFT + rf.LENGTH] == plain.upper()
            assert set(reference[:cf.PAD_LEFT] + reference[cf.PAD_LEFT + rf.LENGTH:]) <= set("ACGT")
            assert cf.padded(seed, profile, keep_case=True)[0][cf.PAD_LEFT:cf.PAD_LEFT + rf.LENGTH] == plain
            assert [r[:2] + (r[2] - cf.PAD_LEFT,) + r[3:] for r in rows] == plain_rows
            assert [(r.start - cf.PAD_LEFT, r.end - cf.PAD_LEFT) for r in records] == [(r.start, r.end) for r in plain_records]
    for seed in cf.SEEDS:                                # no read ends behind the chromosome, none begins in its first 10 bases
        for route in cf.ROUTES:
            reference, sets = cf.inputs(seed, route)
            for rows in sets:
                assert all(10 <= r.pos and r.ref_end <= len(reference) for r in cf.reads_of(rows)), (seed, route)
                assert [r[2] for r in rows] == sorted(r[2] for r in rows)
    reference, (rows,) = cf.inputs(3, "illumina")       # the additions lie on top of the corpus: without them it is the padded corpus
    assert cf.inputs(3, "illumina", extra=False)[1][0] == sorted(rf.bam_rows(cf.padded(3, "short")[1]), key=lambda r: r[2])
    assert len(rows) == len(cf.padded(3, "short")[1]) + len(cf.additions(3, "short"))
    short, long_ = cf.inputs(3, "two_bams")[1]          # two BAMs share one chromosome
    assert cf.inputs(3, "two_bams")[0] == cf.inputs(3, "illumina")[0] != cf.inputs(3, "pacbio")[0]
    assert cf.inputs(3, "two_bams", False)[0] == rf.corpus(3, "short")[0].upper()


@pytest.mark.parametrize("route,pad", CASES)
def test_oracle_equals_the_restatements_on_every_seed(route, pad):
    """Hotspot positions, the events per tile against the planner's counts, both passes' regions, the statistics, and for one
    BAM every site, allele and supporting read (for PacBio the clipped read: start, CIGAR, bases)."""
    found, _ = cf.survey(route, pad)
    assert not found, found


RULE_MET_AT = dict(eqx_counted=(0, "illumina", True), n_uncounted=(0, "illumina", True), lead_total=(1, "illumina", True),
                   increment_2=(0, "illumina", True), softclip_anchor=(0, "illumina", True), ph_keep_index=(3, "illumina", True),
                   single_inclusive=(0, "illumina", True), hybrid_exclusive=(0, "hybrid", True), limit_100=(1, "pacbio", True),
                   mapq_by_caller=(0, "pacbio", False), qc_fail_kept=(0, "two_bams", True), improper_dropped=(0, "illumina", True),
                   first_of_name=(0, "illumina", True), del_q60=(0, "illumina", True), n_dropped_from_candidates=(0, "illumina", True),
                   limit_80=(0, "illumina", True), strict_drop=(1, "illumina", True))


@pytest.mark.parametrize("rule", [f.name for f in dataclasses.fields(cf.Rules)])
def test_every_rule_is_reached(rule):
    """The oracle with one rule off differs from the restatement on the named corpus: the corpora meet the rule, and the equality
    above would see it broken.  Three rules are met only through reads built on purpose (``additions``): ``N`` not counted, the
    total of a leading insertion, the soft-clipped anchor of a deletion -- before those reads existed, 8 seeds showed none of them."""
    seed, route, pad = RULE_MET_AT[rule]
    assert cf.disagreements(seed, route, pad, cf.Rules(**{rule: False})), rule
    assert not cf.disagreements(seed, route, pad)


def test_census_every_situation_really_occurs():
    """Each line at least 5 times over the corpora of every route it applies to -- one Illumina BAM, one PacBio BAM, two BAMs (with
    ``hybrid_hotspot`` off and on together); what lives in the one corpus of the caps at least once; the lines no corpus reaches
    are reached by the hand-built read set, and stay listed only while no corpus reaches them."""
    short = {}
    for route in cf.ROUTES[:3]:
        census = Counter()
        for mode in (("two_bams", "hybrid") if route == "two_bams" else (route,)):
            for pad in (True, False):
                census.update(cf.survey(mode, pad)[1])
        print(route, dict(census))
        by_hand = {k for r, k in cf.CENSUS_BY_HAND + cf.CENSUS_NOT_BUILT if r == route}
        once = set(cf.CENSUS_ONCE[route])
        lines = cf.CENSUS_AT_LEAST_5 + cf.CENSUS_TILES + (cf.CENSUS_CLIP if route != "illumina" else cf.CENSUS_ILLUMINA)
        lines += cf.CENSUS_TWO_BAMS if route == "two_bams" else ()
        lines += tuple("stat_" + k for k in cr.STAT_KEYS if "stat_" + k not in cf.CENSUS_UNREACHABLE)
        short.update({(route, k): census[k] for k in lines if census[k] < 5 and k not in by_hand | once})
        short.update({(route, k): census[k] for k in once if census[k] < 1})
        assert not [k for k in by_hand if census[k] >= 5], "a hand-built line is reached by the corpora now: take it off the list"
        assert not [k for k in cf.CENSUS_UNREACHABLE if census[k]], "a line held unreachable is reached"
    assert not short, short


@pytest.mark.parametrize("route", cf.ROUTES)
def test_the_hand_built_read_sets_reach_what_the_corpora_do_not(route):
    """Every hand-built set through the route's restatement and through the oracle: the statistics each set is for, both passes'
    regions, the hotspot positions, and the oracle's census of the lines the set was built for."""
    census = Counter()
    for name in cf.hand_built():
        want = cf.hand_restated(route, name)
        st = want["stats"]
        assert {k: st[k] for k in cf.HAND_STATS[name]} == cf.HAND_STATS[name], (route, name)
        o = cf.Oracle(want["reference"], want["rows"], route == "pacbio", route == "hybrid")
        pass1, pass2, mine, stats, _ = o.find_sites(want["positions"])
        assert pass1 == list(st["regions_pass1"]) and pass2 == list(st["regions_pass2"]), (route, name)
        assert all(stats[k] == st[k] for k in cf.PLAN_KEYS), (route, name)
        theirs = [(s.start, s.stop, [a[0] for a in s.alleles]) for s in want["sites"] if (s.start, s.stop) not in o.reassembled]
        assert [(a, b, [t for t, _ in kept]) for a, b, _, kept in mine] == theirs, (route, name)
        census.update(o.census)
        o = cf.Oracle(want["reference"], want["rows"], route == "pacbio", route == "hybrid")
        assert o.hotspots(*cf.HAND_SPAN) == want["hotspots"], (route, name)
        census.update({"hotspot_" + k: v for k, v in o.census.items()})
        if name == "edges":
            assert st["regions_pass1"] == [(638, 645 if route != "hybrid" else 644)] and all(p in want["hotspots"] for p in (483, 638, 639, 643))
    lines = ("status_RightPartial_partial_stop", "candidate_event_on_the_last_column_of_a_tile", "candidate_event_on_the_first_column_of_a_tile",
             "candidate_flagged_run_across_a_tile_edge", "candidate_flagged_run_across_flag_lo", "hotspot_event_on_the_last_column_of_a_tile",
             "hotspot_event_on_the_first_column_of_a_tile", "hotspot_flagged_run_across_a_tile_edge")
    assert all(census[k] > 0 for k in lines), {k: census[k] for k in lines}
    assert census["hotspot_flagged_run_across_a_chunk_edge"] == (1 if route == "illumina" else 0)
