"""CPU tests of the PacBio candidate stage: tests/pacbio_reference.py against the reference's own strictClipRead
(tests/golden/pacbio_clip_cases.json), hand-written clip results for every rule, the read cap, whole-site hand cases, and the
command lines and refusals."""
import json
import os

import pytest

from tests import candidate_reference as cr
from tests import pacbio_reference as pr
from tests.bam_writer import Read
from tests.test_candidates import REF, _del, _match, _names, _snv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_cases():
    with open(os.path.join(GOLDEN, "pacbio_clip_cases.json")) as fh:
        return json.load(fh)


def _run(case):
    rlen = sum(n for op, n in case["cigar"] if op in pr.REF_OPS)
    state = (case["pos"], case["pos"] + max(rlen, 1), [tuple(c) for c in case["cigar"]], case["seq"], case["qual"])
    for position, left in case["steps"]:
        state = pr.strict_clip(*state, position, left, case["flank"])
    return state


def test_restatement_equals_the_reference_on_every_fixture_case():
    cases = fixture_cases()
    assert len(cases) >= 250
    changed = 0
    for c in cases:
        pos, end, cigar, seq, qual = _run(c)
        want = c["out"]
        assert (pos, end, [list(x) for x in cigar], seq, qual) == (want["pos"], want["end"], want["cigar"], want["seq"], want["qual"]), c["name"]
        changed += want["cigar"] != c["cigar"]
    assert changed > 150                                   # the fixture is not a list of untouched reads
    first = cases[0]                                       # 300M2I300M at 1000, clipped left at 1290 and right at 1400
    assert (first["cigar"], first["pos"], first["steps"]) == ([[0, 300], [1, 2], [0, 300]], 1000, [[1290, True], [1400, False]])
    assert (first["out"]["pos"], first["out"]["cigar"], len(first["out"]["seq"])) == (1090, [[0, 210], [1, 2], [0, 300]], 512)


M, I, D, N, S, H, EQ, X = 0, 1, 2, 3, 4, 5, 7, 8
# (name, pos, cigar, flank, [(position, left)], expected (start, end, cigar, bases dropped in front, bases dropped behind))
HAND_CLIPS = [
    # left at 130: the left half 31M keeps flank + 1 = 11 bases, 120..130; rejoined with the right half 29M
    ("inside an M", 100, [(M, 60)], 10, [(130, True)], (120, 160, [(M, 40)], 20, 0)),
    # right at 130: the right half 29M (131..159) keeps 11 bases, 131..141
    ("inside an M, right", 100, [(M, 60)], 10, [(130, False)], (100, 142, [(M, 42)], 0, 18)),
    # left at 124 inside 10D (120..129): the left half is 20M 5D; D holds no read base, 6 of the 20M are kept
    ("inside a D", 100, [(M, 20), (D, 10), (M, 30)], 5, [(124, True)], (114, 160, [(M, 6), (D, 10), (M, 30)], 14, 0)),
    ("inside a D, right", 100, [(M, 20), (D, 10), (M, 30)], 5, [(124, False)], (100, 136, [(M, 20), (D, 10), (M, 6)], 0, 24)),
    ("inside an N", 100, [(M, 20), (N, 10), (M, 30)], 5, [(125, True)], (114, 160, [(M, 6), (N, 10), (M, 30)], 14, 0)),
    ("inside an N, right", 100, [(M, 20), (N, 10), (M, 30)], 5, [(125, False)], (100, 136, [(M, 20), (N, 10), (M, 6)], 0, 24)),
    # the left half is 1M: nothing to drop.  The right clip at the first base keeps 100 and 6 bases behind it
    ("first aligned base", 100, [(M, 40)], 5, [(100, True)], (100, 140, [(M, 40)], 0, 0)),
    ("first aligned base, right", 100, [(M, 40)], 5, [(100, False)], (100, 107, [(M, 7)], 0, 33)),
    ("last aligned base", 100, [(M, 40)], 5, [(139, True)], (134, 140, [(M, 6)], 34, 0)),
    ("last aligned base, right: an empty right half", 100, [(M, 40)], 5, [(139, False)], (100, 140, [(M, 40)], 0, 0)),
    ("position left of the read", 100, [(M, 40)], 5, [(99, True), (99, False)], (100, 140, [(M, 40)], 0, 0)),
    ("position at reference_end", 100, [(M, 40)], 5, [(140, True), (140, False)], (100, 140, [(M, 40)], 0, 0)),
    ("flank longer than the read", 100, [(M, 40)], 200, [(120, True), (125, False)], (100, 140, [(M, 40)], 0, 0)),
    # left at 114: the left half 10M 6I 5M; 5M (5 bases), then the I holds bases 6..11 and the limit 8: 8 - 5 + 1 = 4 kept, as S
    ("leading I to S, truncated", 100, [(M, 10), (I, 6), (M, 30)], 8, [(114, True)], (110, 140, [(S, 4), (M, 30)], 12, 0)),
    ("leading I to S, nothing dropped", 100, [(I, 4), (M, 30)], 50, [(110, True)], (100, 130, [(S, 4), (M, 30)], 0, 0)),
    ("trailing I to S, truncated", 100, [(M, 30), (I, 6), (M, 10)], 8, [(124, False)], (100, 130, [(M, 30), (S, 4)], 0, 12)),
    ("trailing I to S, nothing dropped", 100, [(M, 30), (I, 4)], 50, [(110, False)], (100, 130, [(M, 30), (S, 4)], 0, 0)),
    # soft clips are read bases: left at 109 the half 6S 10M keeps 10M and 13 - 10 = 3 of the S; right at 120 the half 9M 6S
    # keeps 9M and 4 of the S
    ("soft clips count", 100, [(S, 6), (M, 30), (S, 6)], 12, [(109, True), (120, False)], (100, 130, [(S, 3), (M, 30), (S, 4)], 3, 2)),
    # left at 110: 11M | 9M 3I 20M -> 5M + 9M = 14M
    ("centre merged", 100, [(M, 20), (I, 3), (M, 20)], 4, [(110, True)], (106, 140, [(M, 14), (I, 3), (M, 20)], 6, 0)),
    # left at 119, the last base of the 20M: the halves meet between M and I
    ("centre not merged", 100, [(M, 20), (I, 3), (M, 20)], 4, [(119, True)], (115, 140, [(M, 5), (I, 3), (M, 20)], 15, 0)),
    ("two equal operations meet at the centre", 100, [(M, 20), (M, 20)], 4, [(119, True)], (115, 140, [(M, 25)], 15, 0)),
    # left at 500 keeps 300..500 and what follows; right at 530 then keeps 531..731
    ("left then right in one operation", 100, [(M, 1000)], 200, [(500, True), (530, False)], (300, 732, [(M, 432)], 200, 368)),
    ("left then right", 1000, [(M, 300), (I, 2), (M, 300)], 200, [(1290, True), (1400, False)], (1090, 1600, [(M, 210), (I, 2), (M, 300)], 90, 0)),
    ("hard clips kept", 100, [(H, 7), (M, 30), (H, 9)], 50, [(110, True), (120, False)], (100, 130, [(H, 7), (M, 30), (H, 9)], 0, 0)),
    ("hard clips dropped, nothing consumed", 100, [(H, 7), (M, 30), (H, 9)], 3, [(110, True), (120, False)], (107, 125, [(M, 18)], 7, 5)),
]


@pytest.mark.parametrize("case", HAND_CLIPS, ids=lambda c: c[0])
def test_hand_clips(case):
    name, pos, cigar, flank, steps, (start, end, want_cigar, front, behind) = case
    qlen = sum(n for op, n in cigar if op in pr.QUERY_OPS)
    seq = "".join("ACGT"[(7 * i + i // 5) % 4] for i in range(qlen))
    qual = [2 + i % 40 for i in range(qlen)]
    state = (pos, pos + sum(n for op, n in cigar if op in pr.REF_OPS), cigar, seq, qual)
    for position, left in steps:
        state = pr.strict_clip(*state, position, left, flank)
    assert state == (start, end, want_cigar, seq[front:qlen - behind], qual[front:qlen - behind])
    if len(steps) == 2 and steps[0][1] and not steps[1][1]:          # clip_read is those two steps
        r = pr.clip_read(Read("x", pos, cigar, seq, qual), steps[0][0], steps[1][0] - steps[0][0], flank)
        assert (r.pos, r.ref_end, r.cigar, r.seq, r.qual) == state


def test_the_fixture_holds_the_hand_clips():
    by_key = {(c["pos"], json.dumps(c["cigar"]), c["flank"], json.dumps(c["steps"])): c for c in fixture_cases()}
    found = 0
    for name, pos, cigar, flank, steps, (start, end, want_cigar, front, behind) in HAND_CLIPS:
        c = by_key.get((pos, json.dumps([list(x) for x in cigar]), flank, json.dumps([[p, left] for p, left in steps])))
        if c is None:
            continue
        found += 1
        assert (c["out"]["pos"], c["out"]["end"], c["out"]["cigar"]) == (start, end, [list(x) for x in want_cigar]), name
        assert c["out"]["seq"] == c["seq"][front:len(c["seq"]) - behind], name
    assert found >= 20                                     # the reference itself agrees with the hand-written values


def test_read_cap():
    assert pr.read_cap(0, 100) == 100 and isinstance(pr.read_cap(0, 101), float)
    assert pr.read_cap(0, 101) == 101.0 and pr.read_cap(0, 180) == 180.0 and pr.read_cap(0, 30) == 100


def _long(name, seq_of, **kw):
    """A 540-base read over [30, 570) of REF, spelt by ``seq_of`` (a _match / _snv / _del style builder)."""
    return seq_of(name, 30, 540, **kw)


def pacbio_hand_cases():
    """(name, reads, positions, expected [(start, stop, [(allele, [read names])])]).  REF is 600 bases; the reads are long
    enough to be clipped on both sides."""
    cases = []
    refs = [_match(f"r{i}", 30, 540) for i in range(12)]
    dels = [_del(f"d{i}", 30, 540, 301, 2) for i in range(2)]
    # AT (301, 302) deleted in 2 of 14 reads: 2 / 14 = 0.143 >= 0.12 and 2 >= minCount -> a site under the PacBio thresholds
    cases.append(("an indel with two supporting reads", refs + dels, [300],
                  [(300, 304, [("GATT", _names("r", 12)), ("GT", _names("d", 2))])]))
    alts = [_snv(f"t{i}", 30, 540, 300, "T") for i in range(6)]
    cases.append(("snv on long reads", refs[:6] + alts, [300], [(300, 301, [("G", _names("r", 6)), ("T", _names("t", 6))])]))
    # a read over [0, 400): unclipped its window test fails (min start 0 - 10 < 0, the searcher would be out of bounds and the
    # site lost); clipped at 210 - 200 it starts at 10 (pass 1) and the searcher runs
    edge = [_match(f"e{i}", 0, 400) for i in range(6)] + [_snv(f"t{i}", 0, 400, 300, "T") for i in range(6)]
    cases.append(("the window test passes only after clipping", edge, [300], [(300, 301, [("G", _names("e", 6)), ("T", _names("t", 6))])]))
    return cases


@pytest.mark.parametrize("case", pacbio_hand_cases(), ids=lambda c: c[0])
def test_whole_site_hand_cases(case):
    name, reads, positions, expected = case
    reads = sorted(reads, key=lambda r: r.pos)
    st = {}
    sites = pr.find_candidates(reads, REF, positions, stats=st)
    got = [(s.start, s.stop, [(a, [s.reads[i].name for i in idx]) for a, idx in s.alleles]) for s in sites]
    assert got == expected
    assert st["regions_at_read_cap"] == st["clusters_at_read_cap"] == 0
    lo, hi = st["regions_pass2"][0][0] - 15, st["regions_pass2"][-1][1] + 14       # the one cluster's fetch interval
    for s in sites:                                        # the reads of a site are the clipped reads of pass 2
        for r in s.reads:
            assert r.pos >= max(lo - 200, 0) and r.ref_end <= hi + 202 and len(r.seq) <= hi - lo + 402


def test_two_reads_make_a_pacbio_site_and_no_illumina_site():
    """Two deletion reads among 14, each counted once (the PacBio table): 2 >= minCount flags [300, 304) under the PacBio
    threshold; under the Illumina table's threshold, 2 * minCount = 4, the same counts flag nothing.  (Counted as Illumina
    reads they would weigh 2 each and reach 4: the increment and the threshold belong together.)"""
    from tests import hotspot_reference as hr
    _, reads, positions, expected = pacbio_hand_cases()[0]
    reads = sorted(reads, key=lambda r: r.pos)
    counts = {}
    for r in reads:
        hr.update_counts(counts, pr.clip_read(r, 210, 180), REF, 10, pacbio=True)
    for c in counts.values():
        hr.resolve_partials(c)
    as_pacbio, as_illumina = set(), set()
    hr.flag_single(counts, hr.MIN_COUNT, as_pacbio)
    hr.flag_single(counts, 2 * hr.MIN_COUNT, as_illumina)
    assert as_pacbio == {300, 301, 302, 303} and as_illumina == set()
    assert [(s.start, s.stop) for s in pr.find_candidates(reads, REF, positions)] == [(300, 304)]
    one = [r for r in reads if r.name != "d1"]                   # one read is not enough
    assert pr.find_candidates(one, REF, positions) == []


def test_the_window_test_sees_the_clipped_reads():
    _, reads, positions, _ = pacbio_hand_cases()[2]
    st = {}
    assert cr.find_candidates(reads, REF, positions, stats=st) == [] and st["regions_out_of_bounds"] == 1
    st = {}
    assert len(pr.find_candidates(reads, REF, positions, stats=st)) == 1 and st["regions_out_of_bounds"] == 0


def _probe(name, pos, ops, insert="ACCA"):
    """A read at `pos` with the CIGAR `ops`: M and = spell REF, X a base that differs, I `insert` (cycled), S the text CT..."""
    seq, p = [], pos
    for op, n in ops:
        if op in (M, EQ):
            seq.append(REF[p:p + n]); p += n
        elif op == X:
            seq.append("".join("ACGT"[("ACGT".index(REF[p + i]) + 1) % 4] for i in range(n))); p += n
        elif op == I:
            seq.append((insert * n)[:n])
        elif op == S:
            seq.append(("CT" * n)[:n])
        elif op in (D, N):
            p += n
    seq = "".join(seq)
    return Read(name, pos, list(ops), seq, [20 + (3 * i) % 21 for i in range(len(seq))])


def flank200_cases():
    """One site, the SNV G>T at 300 of REF, whose pass-2 searcher fetches [285, 315): every read is clipped left at 285 and right at
    315 with the flank 200.  Beside 6 + 6 plain reads, one probe read per clip rule, all spelling G at 300.
    -> (reads, {name: (start, CIGAR, bases dropped in front, bases dropped behind)}), the values written out by hand."""
    plain = [_match(f"r{i}", 30, 540) for i in range(6)] + [_snv(f"t{i}", 30, 540, 300, "T") for i in range(6)]
    # 30..569 in one M: the left half 30..285 keeps 85..285, the right half 286..569 is cut to 316..516 behind 315
    want = {r.name: (85, [(M, 432)], 55, 53) for r in plain}
    probes = [
        # 285 inside 10N (280..289): the left half ...220M 6N keeps the N and 201 of the M; right: 260M from 290 keeps 26 + 201
        (_probe("inside_N", 60, [(M, 220), (N, 10), (M, 260)]), (79, [(M, 201), (N, 10), (M, 227)], 19, 33)),
        # 285 inside 6D (282..287): 4D then 201 of 222M; right: 262M from 288 keeps 28 + 201
        (_probe("inside_D", 60, [(M, 222), (D, 6), (M, 262)]), (81, [(M, 201), (D, 6), (M, 229)], 21, 33)),
        # = and X: left of 285 24 = (262..285), 2X, then 175 of the 200 =; right: the 300 = from 262 keep 54 + 201
        (_probe("eq_and_x", 60, [(EQ, 200), (X, 2), (EQ, 300)]), (85, [(EQ, 175), (X, 2), (EQ, 255)], 25, 45)),
        # behind 315: 54M, 6S (60 read bases), 9H -- all kept, H is no I
        (_probe("trailing_S_H_kept", 250, [(M, 120), (S, 6), (H, 9)]), (250, [(M, 120), (S, 6), (H, 9)], 0, 0)),
        # behind 315: 198M, then 3 of the 10S (bases 199..201); the H is dropped
        (_probe("trailing_S_cut", 200, [(M, 314), (S, 10), (H, 9)]), (200, [(M, 314), (S, 3)], 0, 7)),
        (_probe("leading_H_S_kept", 120, [(H, 7), (S, 10), (M, 300)]), (120, [(H, 7), (S, 10), (M, 300)], 0, 0)),
        # up to 285: 196M, then 5 of the 10S; the H is dropped
        (_probe("leading_S_cut", 90, [(H, 7), (S, 10), (M, 300)]), (90, [(S, 5), (M, 300)], 5, 0)),
        # up to 285: 195M (91..285), then 6 of the 10I, as S; the 11M before them are dropped
        (_probe("leading_I_cut", 80, [(M, 11), (I, 10), (M, 400)], "AC"), (91, [(S, 6), (M, 400)], 15, 0)),
        (_probe("leading_I_kept", 200, [(I, 4), (M, 300)], "GT"), (200, [(S, 4), (M, 300)], 0, 0)),
        # behind 315: 195M (316..510), then 6 of the 10I, as S; the 30M behind them are dropped
        (_probe("trailing_I_cut", 100, [(M, 411), (I, 10), (M, 30)], "TG"), (100, [(M, 411), (S, 6)], 0, 34)),
        (_probe("trailing_I_kept", 250, [(M, 150), (I, 5)], "CA"), (250, [(M, 150), (S, 5)], 0, 0)),
        # 285 is the last base of 236M, an I follows: nothing to merge
        (_probe("centre_not_merged", 50, [(M, 236), (I, 3), (M, 200)], "TTG"), (85, [(M, 201), (I, 3), (M, 200)], 35, 0)),
        # 285 is the last base of 236M, 200M follow: 201M + 200M become one operation
        (_probe("equal_ops_left", 50, [(M, 236), (M, 200)]), (85, [(M, 401)], 35, 0)),
        # 315 is the last base of 216M, 150M follow (all kept): one operation
        (_probe("equal_ops_right", 100, [(M, 216), (M, 150)]), (100, [(M, 366)], 0, 0)),
        (_probe("first_base_at_285", 285, [(M, 200)]), (285, [(M, 200)], 0, 0)),
        # 315 is the read's last base: the right half is empty
        (_probe("last_base_at_315", 50, [(M, 266)]), (85, [(M, 231)], 35, 0)),
        (_probe("starts_behind_285", 290, [(M, 250)]), (290, [(M, 227)], 0, 23)),
        (_probe("ends_before_315", 50, [(M, 260)]), (85, [(M, 225)], 35, 0)),
        (_probe("shorter_than_the_flank", 260, [(M, 80)]), (260, [(M, 80)], 0, 0)),
    ]
    for r, w in probes:
        want[r.name] = w
    return sorted(plain + [r for r, _ in probes], key=lambda r: r.pos), want


def test_flank_200_probe_reads():
    reads, want = flank200_cases()
    for r in reads:
        start, cigar, front, behind = want[r.name]
        c = pr.clip_read(r, 285, 30)
        assert (c.pos, c.cigar, c.seq, c.qual) == (start, cigar, r.seq[front:len(r.seq) - behind], r.qual[front:len(r.qual) - behind]), r.name
    st = {}
    sites = pr.find_candidates(reads, REF, [300], stats=st)
    assert [(s.start, s.stop) for s in sites] == [(300, 301)] and st["regions_pass2"] == [(300, 301)]
    assert st["regions_at_read_cap"] == st["clusters_at_read_cap"] == 0
    support = {a: {sites[0].reads[i].name for i in idx} for a, idx in sites[0].alleles}
    assert support["T"] == set(_names("t", 6)) and support["G"] == set(want) - support["T"]       # every probe is in the shard


def test_parser_of_the_pacbio_module():
    from hello_amd import candidates as cd, pacbio as pb
    flags = {s for a in pb.parser()._actions for s in a.option_strings}
    old = {s for a in cd.parser()._actions for s in a.option_strings}
    assert flags == old - {"--pacbio", "--hybrid_hotspot"}
    args = pb.parser().parse_args(["--bam", "p.bam", "--ref", "g.fa", "--activity", "s.txt", "--outputPrefix", "o"])
    assert (args.featureLength, args.q_threshold, args.mapq_threshold, args.device) == (150, 10, 10, 0)
    with pytest.raises(SystemExit):
        pb.parser().parse_args(["--bam", "p.bam", "--ref", "g.fa", "--activity", "s.txt", "--outputPrefix", "o", "--pacbio"])
    with pytest.raises(ValueError, match="one Illumina BAM"):
        pb.main(["--bam", "a.bam,b.bam", "--ref", "g.fa", "--activity", "s.txt", "--outputPrefix", "o"])
    with pytest.raises(ValueError, match="one Illumina BAM"):
        pb.find_pacbio_candidates(["a.bam", "b.bam"], "g.fa", "chr1", [300])
    assert cd.STAT_NAMES[:20][-1] == "total_ms" and cd.STAT_NAMES[20:] == ("clip_kernel_ms", "reads_clipped") and cd.N_STATS == 22


def test_from_bam_routing_and_refusals():
    from hello_amd import call, candidates as cd, pacbio as pb
    assert call.from_bam_route("i.bam", None) == ("i.bam", False, cd.find_candidates)
    assert call.from_bam_route(None, "p.bam") == ("p.bam", True, pb.find_pacbio_candidates)
    for ibam, pbam in (("i.bam", "p.bam"), (None, None), ("a.bam,b.bam", None), (None, "a.bam,b.bam")):
        with pytest.raises(ValueError, match="one Illumina BAM"):
            call.from_bam_route(ibam, pbam)
    args = call.parser().parse_args(["--network", "m", "--workdir", "w", "--from_bam", "--ibam", "i.bam", "--pbam", "p.bam", "--ref", "g.fa"])
    with pytest.raises(ValueError, match="one Illumina BAM"):
        call.shards_from_bam(args)
    assert call.features_dir_name(None, "/d/p.bam") == "features_d___p__bam"


def test_old_entries_still_refuse_and_point_to_the_new_module(tmp_path):
    from hello_amd import candidates as cd
    with pytest.raises(ValueError, match="one Illumina BAM.*hello_amd.pacbio"):
        cd.find_candidates("a.bam", "g.fa", "chr1", [300], pacbio=True)
    with pytest.raises(ValueError, match="one Illumina BAM"):
        cd.main(["--bam", "a.bam", "--ref", "g.fa", "--activity", "s.txt", "--outputPrefix", str(tmp_path / "o"), "--pacbio"])
    with pytest.raises(ValueError, match="one Illumina BAM"):
        cd.find_candidates(["a.bam", "b.bam"], "g.fa", "chr1", [300])
