"""CPU tests of the candidate stage: the hand-derived cases that pin tests/candidate_reference.py (expected sites, alleles and
supporting reads written out), the sharding rule, the refusals, the hp selector of the BAM reader and a shard round trip."""
import numpy as np
import pytest

from tests import candidate_reference as cr
from tests.bam_writer import Read, write_bam

BLOCK = "GATTACAGGCTTCAAGTCCGATAGCTAGGTCCATGCAATCGGATTCAGCTAGCTTAGGCA"     # 60 bases; REF[p] = BLOCK[p % 60]
REF = BLOCK * 10
# around 300: REF[300:313] = G A T T A C A G G C T T C


def _match(name, pos, length, q=30, **kw):
    return Read(name, pos, [(0, length)], REF[pos:pos + length], [q] * length, **kw)


def _snv(name, pos, length, at, base, q=30, **kw):
    seq = REF[pos:at] + base + REF[at + 1:pos + length]
    qual = [30] * length
    qual[at - pos] = q
    return Read(name, pos, [(0, length)], seq, qual, **kw)


def _ins(name, pos, length, after, text):
    """`text` inserted behind reference position `after`."""
    seq = REF[pos:after + 1] + text + REF[after + 1:pos + length]
    return Read(name, pos, [(0, after + 1 - pos), (1, len(text)), (0, pos + length - after - 1)], seq, [30] * len(seq))


def _del(name, pos, length, first, n):
    """Reference positions [first, first + n) deleted."""
    seq = REF[pos:first] + REF[first + n:pos + length]
    return Read(name, pos, [(0, first - pos), (2, n), (0, pos + length - first - n)], seq, [30] * len(seq))


def _names(prefix, n):
    return [f"{prefix}{i}" for i in range(n)]


def hand_cases():
    """(name, reads, positions, keyword arguments, expected [(start, stop, [(allele, [supporting read names])])])."""
    refs = [_match(f"r{i}", 250, 100) for i in range(6)]
    cases = []
    # an SNV G>T at 300: 6 of 12 reads.  Pass 1 flags {300} inside [285, 315]; the cluster [285, 315) flags it again.
    # Beside it: reads with N there (allele "N": supported, no candidate), a low base quality (min_q 5 < 10: no record counts) and
    # a low mapping quality (5 < 10: neither counted nor supporting).  T counts 6 of 17 reads.
    alts = [_snv(f"t{i}", 250, 100, 300, "T") for i in range(6)]
    noise = ([_snv(f"n{i}", 250, 100, 300, "N") for i in range(3)] + [_snv(f"q{i}", 250, 100, 300, "C", q=5) for i in range(2)]
             + [_snv(f"m{i}", 250, 100, 300, "A", mapq=5) for i in range(2)])
    cases.append(("snv", refs + alts, [300], {}, [(300, 301, [("G", _names("r", 6)), ("T", _names("t", 6))])]))
    cases.append(("snv among N, low quality and low mapq", refs + alts + noise, [300], {},
                  [(300, 301, [("G", _names("r", 6)), ("T", _names("t", 6))])]))
    # every read carries the SNV: the reference allele has no support and is left out
    cases.append(("unsupported reference allele", [_snv(f"t{i}", 250, 100, 300, "T") for i in range(8)], [300], {},
                  [(300, 301, [("T", _names("t", 8))])]))
    # TT inserted behind 300: planted at 300 with reference allele G, it flags [300, 300 + 1 + 1) = {300, 301}; the reads spell
    # G+TT at 300 and A at 301.  "trail" ends with the insertion (right partial GTT: a prefix of GTTA only), "lead" starts with
    # it (left partial TTA: a suffix of GTTA only), "amb" starts at 301 (left partial A: a suffix of both -> nothing),
    # "two" ends at 300 and has a left partial in no region and a right partial G (a prefix of both -> nothing).
    ins = [_ins(f"i{i}", 250, 100, 300, "TT") for i in range(6)]
    trail = Read("trail", 251, [(0, 50), (1, 2)], REF[251:301] + "TT", [30] * 52)
    lead = Read("lead", 301, [(1, 2), (0, 49)], "TT" + REF[301:350], [30] * 51)
    amb = _match("amb", 301, 49)
    two = _match("two", 252, 49)
    cases.append(("insertion", refs + ins, [300], {}, [(300, 302, [("GA", _names("r", 6)), ("GTTA", _names("i", 6))])]))
    cases.append(("partials", refs + ins + [trail, two, lead, amb], [300], {},
                  [(300, 302, [("GA", _names("r", 6)), ("GTTA", _names("i", 6) + ["trail", "lead"])])]))
    # AT (301, 302) deleted: planted at 300 with reference allele GAT, it flags [300, 300 + 3 + 1) = {300..303}; the reads spell G, T
    dels = [_del(f"d{i}", 250, 100, 301, 2) for i in range(6)]
    cases.append(("deletion", refs + dels, [300], {}, [(300, 304, [("GATT", _names("r", 6)), ("GT", _names("d", 6))])]))
    # a deletion of [306, 326) flags {305..326}: past the active region's stop 315 in pass 1 and over the cluster's stop in pass 2
    # -> the run is dropped whole, not clipped; the SNV at 290 (REF[290] = A) stays
    both = []
    for i in range(6):
        seq = REF[250:290] + "C" + REF[291:306] + REF[326:370]
        both.append(Read(f"b{i}", 250, [(0, 56), (2, 20), (0, 44)], seq, [30] * 100))
    cases.append(("a run crossing the edge is dropped whole", [_match(f"r{i}", 250, 120) for i in range(6)] + both, [300], {},
                  [(290, 291, [("A", _names("r", 6)), ("C", _names("b", 6))])]))
    # 79 bases inserted: the allele G + 79 + A has 81 bases and is left out; the site keeps its reference allele
    long_ins = [_ins(f"i{i}", 250, 100, 300, "C" * 79) for i in range(6)]
    cases.append(("an allele of 81 bases", refs + long_ins, [300], {}, [(300, 302, [("GA", _names("r", 6))])]))
    # an 85-base deletion [301, 386) flags [300, 387): 87 long.  First location of its chromosome: the empty cluster takes it
    # (the site has only the 2-base allele: the 87-base reference allele is too long) ...
    wide = [_match(f"r{i}", 230, 230) for i in range(6)]
    bigdel = [_del(f"d{i}", 230, 230, 301, 85) for i in range(6)]
    cases.append(("a region over 80 with an empty cluster", wide + bigdel, [300, 330, 360, 390], {},
                  [(300, 387, [("G" + REF[386], _names("d", 6))])]))
    # ... behind the SNV at 270 (REF[270] = C) it closes that cluster and is itself dropped
    snvdel = []
    for i in range(6):
        d = _del(f"d{i}", 230, 230, 301, 85)
        snvdel.append(Read(d.name, d.pos, d.cigar, d.seq[:40] + "G" + d.seq[41:], d.qual))
    cases.append(("a region over 80 behind a cluster", wide + snvdel, [270, 300, 330, 360, 390], {},
                  [(270, 271, [("C", _names("r", 6)), ("G", _names("d", 6))])]))
    # pass 1 fetches [210, 390): the first "dup" [200, 250) hides the second; T counts 2 of 16 = 0.125 >= 0.12.  Pass 2 fetches
    # [285, 315): the second "dup" is the first of its name there; T counts 2 of 17 < 0.12 -> no region, no site
    many = [_match(f"r{i}", 250, 100) for i in range(14)] + [_snv(f"t{i}", 250, 100, 300, "T") for i in range(2)]
    cases.append(("pass 2 finds fewer regions (repeated names)", [_match("dup", 200, 50)] + many + [_match("dup", 250, 100)], [300], {}, []))
    # a deletion followed by an insertion at a region's edge: "di" deletes 303 and inserts CC behind it, so its entry at 303 is
    # "" + "CC" -- not empty, a Success record with allele CC and min_q min(60, 30); "dd" only deletes 303 and 304: the empty entry
    # at start fails the record.  Each indel key has one read and counts 2 < 4: the region is the SNV's alone (T>G at 303, 6 of 12).
    g303 = [_snv(f"g{i}", 250, 100, 303, "G") for i in range(6)]
    di = Read("di", 250, [(0, 53), (2, 1), (1, 2), (0, 46)], REF[250:303] + "CC" + REF[304:350], [30] * 101)
    dd = Read("dd", 250, [(0, 53), (2, 2), (0, 45)], REF[250:303] + REF[305:350], [30] * 98)
    cases.append(("a deletion then an insertion at the region's edge", refs + g303 + [di, dd], [303], {},
                  [(303, 304, [("T", _names("r", 6)), ("CC", ["di"]), ("G", _names("g", 6))])]))
    # an N skip over [295, 305) leaves holes: no entry at start = 300 -> a left partial with the empty string, which is a suffix
    # of every allele: of G and T (two matches, nothing happens) ...
    skip = Read("skip", 250, [(0, 45), (3, 10), (0, 45)], REF[250:295] + REF[305:350], [30] * 90)
    cases.append(("an N skip: the empty partial matches two alleles", refs + alts + [skip], [300], {},
                  [(300, 301, [("G", _names("r", 6)), ("T", _names("t", 6))])]))
    # ... and of T alone where every other read carries the SNV: one match, the read supports it
    cases.append(("an empty partial matches the only allele", [_snv(f"t{i}", 250, 100, 300, "T") for i in range(8)] + [skip], [300], {},
                  [(300, 301, [("T", _names("t", 8) + ["skip"])])]))
    # two regions in one cluster: the SNV G>T at 300 and TT inserted behind 310 (reference allele TT, reads spell TTTT).
    # "P" (45M 6N 1I 5M 4N 1M 2I 39M) creates the entry T at 300 in a hole (partial_start) and has no entry at 309: left partials
    # T in (300, 301) -- a suffix of T alone -- and TTTT in (310, 312); only the LAST is kept, so P supports TTTT and not T.
    # "Q" (45M 8N 8M 2I) has the empty left partial in (300, 301) (matches G and T: nothing) and the right partial TTT in
    # (310, 312), a prefix of TTTT alone; the left partial is the one used, so Q supports nothing.
    v = []
    for i in range(6):
        seq = REF[250:300] + "T" + REF[301:311] + "TT" + REF[311:350]
        v.append(Read(f"v{i}", 250, [(0, 61), (1, 2), (0, 39)], seq, [30] * 102))
    P = Read("P", 250, [(0, 45), (3, 6), (1, 1), (0, 5), (3, 4), (0, 1), (1, 2), (0, 39)],
             REF[250:295] + "T" + REF[301:306] + REF[310] + "TT" + REF[311:350], [30] * 93)
    Q = Read("Q", 250, [(0, 45), (3, 8), (0, 8), (1, 2)], REF[250:295] + REF[303:311] + "TT", [30] * 55)
    cases.append(("the last left partial wins; left before right", refs + v + [P, Q], [300, 310], {},
                  [(300, 301, [("G", _names("r", 6)), ("T", _names("v", 6))]),
                   (310, 312, [("TT", _names("r", 6)), ("TTTT", _names("v", 6) + ["P"])])]))
    # the read cap: pass 1 fetches 180 bases (cap 1000 / 30 * 180 = 6000, all 1003 reads); pass 2 fetches exactly 30 bases
    # (cap 1000, a read is kept while len < cap): the first 1000 reads; x0..x2 behind them support nothing
    crowd = ([_match(f"r{i}", 250, 100) for i in range(850)] + [_snv(f"t{i}", 250, 100, 300, "T") for i in range(150)]
             + [_snv(f"x{i}", 250, 100, 300, "T") for i in range(3)])
    cases.append(("the read cap keeps the first 1000 reads in pass 2", crowd, [300], {},
                  [(300, 301, [("G", _names("r", 850)), ("T", _names("t", 150))])]))
    # the window of a region at the chromosome's start leaves it: min(5, 12 - 15) - 10 < 0
    cases.append(("out of bounds", [_snv(f"t{i}", 5, 100, 12, "G") for i in range(6)], [12], {}, []))
    return cases


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, reads, positions, kw, expected = case
    reads = sorted(reads, key=lambda r: r.pos)
    sites = cr.find_candidates(reads, REF, positions, **kw)
    got = [(s.start, s.stop, [(a, [s.reads[i].name for i in idx]) for a, idx in s.alleles]) for s in sites]
    assert got == expected
    for s in sites:                                        # reference window: feature window, allele span, an anchor base
        lo = (s.start + s.stop) // 2 - 75
        assert s.window_start == min(lo, s.start - 1) and s.reference == REF[s.window_start:max(lo + 150, s.stop)]


def test_statistics_of_the_hand_cases():
    by_name = {c[0]: c for c in hand_cases()}

    def stats(name):
        _, reads, positions, kw, _ = by_name[name]
        st = {}
        cr.find_candidates(sorted(reads, key=lambda r: r.pos), REF, positions, stats=st, **kw)
        return st
    st = stats("pass 2 finds fewer regions (repeated names)")
    assert (st["regions_pass1"], st["regions_pass2"]) == ([(300, 301)], [])
    st = stats("out of bounds")
    assert (st["active_regions"], st["regions_out_of_bounds"], st["clusters"]) == (1, 1, 0)
    st = stats("a region over 80 behind a cluster")
    assert st["regions_pass1"] == [(270, 271), (300, 387)] and st["regions_pass2"] == [(270, 271)]
    st = stats("a run crossing the edge is dropped whole")
    assert st["regions_pass1"] == [(290, 291)]
    st = stats("deletion")
    assert st["regions_pass1"] == st["regions_pass2"] == [(300, 304)]


def test_the_read_cap_keeps_the_first_reads():
    """Pass 1 fetches 180 bases: cap 1000 / 30 * 180 = 6000.  Pass 2 fetches exactly 30: cap 1000, a read is kept while
    len < cap -> the first 1000 of 1003 reads; the 3 reads behind them support nothing."""
    reads = ([_match(f"r{i}", 250, 100) for i in range(850)] + [_snv(f"t{i}", 250, 100, 300, "T") for i in range(150)]
             + [_snv(f"x{i}", 250, 100, 300, "T") for i in range(3)])
    st = {}
    sites = cr.find_candidates(reads, REF, [300], stats=st)
    assert (st["regions_at_read_cap"], st["clusters_at_read_cap"]) == (0, 1)
    assert [(s.start, s.stop, [(a, len(i)) for a, i in s.alleles]) for s in sites] == [(300, 301, [("G", 850), ("T", 150)])]
    assert cr.read_cap(0, 30) == 1000 and cr.read_cap(0, 31) == 1000 / 30 * 31


def test_read_map_edge_cases():
    """Read.cpp:4-137 on single reads: D then I makes the edge entry non-empty; a deletion at an edge fails; N leaves holes."""
    # 10M 2D 3I 10M at 100: positions 110, 111 deleted, the insertion joins the entry at 111
    r = Read("x", 100, [(0, 10), (2, 2), (1, 3), (0, 10)], "A" * 10 + "CCC" + "G" * 10, [30] * 10 + [7, 8, 9] + [30] * 10)
    m = cr.ReadMap(r)
    assert m.aligned_bases(109, 112) == ("ACCC", cr.SUCCESS, 7)          # the entry at stop - 1 = 111 is "CCC": not a failure
    assert m.aligned_bases(109, 111) == ("A", cr.FAIL, 30)               # stop - 1 = 110 is an empty entry
    assert m.aligned_bases(110, 113) == ("CCCG", cr.FAIL, 7)             # start = 110 is an empty entry
    assert (m.partial_start, m.partial_stop, m.last_position) == (False, False, 121)
    # 5M 4N 5M at 100: 105..108 are holes
    n = cr.ReadMap(Read("n", 100, [(0, 5), (3, 4), (0, 5)], "A" * 5 + "C" * 5, [30] * 10))
    assert n.aligned_bases(104, 106) == ("A", cr.RIGHT_PARTIAL, 30)      # stop - 1 = 105 has no entry
    assert n.aligned_bases(106, 110) == ("C", cr.LEFT_PARTIAL, 30)       # start = 106 has no entry
    assert n.aligned_bases(103, 111) == ("AACC", cr.SUCCESS, 30)
    # a read starting with an insertion: the entry at pos - 1 is created, partial_start; one ending with one: partial_stop
    lead = cr.ReadMap(Read("l", 100, [(4, 2), (1, 2), (0, 5)], "NNTTAAAAA", [30] * 9))
    assert lead.pairs[99] == "TT" and lead.partial_start and lead.aligned_bases(99, 101) == ("TTA", cr.LEFT_PARTIAL, 30)
    trail = cr.ReadMap(Read("t", 100, [(0, 5), (1, 2), (5, 3)], "AAAAATT", [30] * 7))
    assert not trail.partial_stop                                         # the hard clip is the last operation (Read.cpp:47)
    trail = cr.ReadMap(Read("t", 100, [(0, 5), (1, 2)], "AAAAATT", [30] * 7))
    assert trail.partial_stop and trail.aligned_bases(104, 106) == ("ATT", cr.RIGHT_PARTIAL, 30)
    # a read keeps only its last left partial and its last right partial
    _, left, right = cr.extract_alleles(Read("p", 100, [(0, 5), (3, 4), (0, 5)], "A" * 5 + "C" * 5, [30] * 10),
                                        [(98, 101), (104, 106), (106, 110), (113, 116)])
    assert left == ("C", 106, 110, 30) and right == ("C", 113, 116, 30)


def test_sharding_rule():
    from hello_amd.candidates import shard_positions
    # items: [1, 2, 3] [50, 51] [100] [200] [210] [400]; ceil(6 / 2) = 3 items, then the next item 25 or more away
    assert shard_positions([1, 2, 3, 50, 51, 100, 200, 210, 400], 2, 25) == [[1, 2, 3, 50, 51, 100], [200, 210, 400]]
    # a shard does not close while the next item is nearer than 25
    assert shard_positions([1, 10, 20, 30, 100], 5, 25) == [[1, 10, 20, 30], [100]]
    assert shard_positions([], 500, 25) == []
    assert shard_positions(list(range(0, 100000, 100)), 500, 25) == [[p, p + 100] for p in range(0, 100000, 200)]


def test_pacbio_two_bams_and_hybrid_are_refused(tmp_path):
    from hello_amd import candidates as cd
    for kw in ({"pacbio": True}, {"hybrid_hotspot": True}):
        with pytest.raises(ValueError, match="one Illumina BAM"):
            cd.find_candidates("a.bam", "g.fa", "chr1", [300], **kw)
    with pytest.raises(ValueError, match="one Illumina BAM"):
        cd.find_candidates(["a.bam", "b.bam"], "g.fa", "chr1", [300])
    for extra in (["--pacbio"], ["--hybrid_hotspot"]):
        with pytest.raises(ValueError, match="one Illumina BAM"):
            cd.main(["--bam", "a.bam", "--ref", "g.fa", "--activity", "s.txt", "--outputPrefix", str(tmp_path / "o")] + extra)
    with pytest.raises(ValueError, match="one Illumina BAM"):
        cd.main(["--bam", "a.bam,b.bam", "--ref", "g.fa", "--activity", "s.txt", "--outputPrefix", str(tmp_path / "o")])


def test_hp_selector_of_the_bam_reader(tmp_path):
    from hello_amd.bam import BamFile
    tags = [b"", b"HPC\x01", b"NMi\x07\0\0\0HPc\x02", b"RGZgroup\0HPS\x01\x00", b"HPi\x02\0\0\0", b"HPI\xff\xff\xff\xff", b"HPs\xff\xff",
            b"XBBs\x02\0\0\0\x01\0\x02\0HPC\x02", b"HPZ1\0"]
    reads = [Read(f"r{i}", 100 + i, [(0, 20)], "ACGT" * 5, [30] * 20, tags=t) for i, t in enumerate(tags)]
    path = str(tmp_path / "hp.bam")
    write_bam(path, [("chr1", 1000)], reads)
    with BamFile(path) as b:
        got = b.fetch("chr1", 0, 1000)
    assert got.hp.dtype == np.uint8 and got.hp.tolist() == [0, 1, 2, 1, 2, 0, 0, 2, 0]
    assert got.strand.tolist() == [0] * 9 and got.n_reads == 9          # the other selectors are what they were


def test_round_trip_of_a_reference_built_shard(tmp_path):
    from hello_amd import shards
    _, reads, positions, kw, expected = [c for c in hand_cases() if c[0] == "partials"][0]
    reads = sorted(reads, key=lambda r: r.pos)
    sites = cr.candidate_sites(cr.find_candidates(reads, REF, positions, **kw), "chr1")
    path = shards.write_shard(str(tmp_path / "s.hshard"), sites)
    shard = shards.PackedShard.from_file(path)
    assert shard.n_sites == 1 and shard.names(0) == ["GA", "GTTA"] and shard.chromosomes == ["chr1"]
    assert np.asarray(shard.z["reads_per_allele0"]).tolist() == [6, 8]
    back = shards.read_shard(path)
    assert [(a, [r.bases for r in r0]) for a, r0, _ in back[0].alleles] == [(a, [r.bases for r in r0]) for a, r0, _ in sites[0].alleles]
    assert back[0].reference == REF[back[0].window_start:back[0].window_start + len(back[0].reference)]
