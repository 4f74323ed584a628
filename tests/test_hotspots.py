"""CPU tests of the hotspot stage: the BAM reader (round trips with and without .bai, refusals), the chunk plan, the CLI surface,
the output format, and the hand-derived cases that pin tests/hotspot_reference.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hotspot_reference as hr
from tests.bam_writer import Read, write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------- BAM reader


def _reads_for_roundtrip():
    rng = np.random.default_rng(3)
    reads = []
    for i in range(300):
        pos = 100 + 3 * i
        seq = "".join(rng.choice(list("ACGTN"), size=40))
        if i % 7 == 0:
            seq = "ACMGRSVTWYHKDBN=" + seq[16:]                    # every IUPAC code and '='
        cigar = [(5, 4), (4, 2), (0, 30), (1, 3), (0, 5)] if i % 5 == 0 else [(0, 20), (2, 4), (0, 20)]
        reads.append(Read(f"read{i}", pos, cigar, seq, [int(q) for q in rng.integers(0, 60, size=40)],
                          flag=16 * (i % 2), mapq=i % 61))
    reads.append(Read("other", 10, [(0, 40)], "A" * 40, [30] * 40, ref_id=1))
    return reads


@pytest.mark.parametrize("index", [True, False])
def test_bam_round_trip(tmp_path, index):
    from hello_amd.bam import BamFile
    reads = _reads_for_roundtrip()
    path = str(tmp_path / "x.bam")
    write_bam(path, [("chr1", 5000), ("chr2", 300)], reads, index=index, block_bytes=333)   # records cross blocks
    with BamFile(path, threads=4) as b:
        assert b.references == [("chr1", 5000), ("chr2", 300)]
        got = b.fetch("chr1", 0, 5000)
        assert got.used_index == index and got.n_blocks > 3
        want = [r for r in reads if r.ref_id == 0]
        assert got.n_reads == len(want)
        for i, r in enumerate(want):
            seq, cigar, qual = got.read(i)
            assert (seq, cigar, list(qual)) == (r.seq, r.cigar, list(r.qual))
            assert (got.ref_starts[i], got.ref_ends[i], got.mapq[i], got.flags[i], got.strand[i]) == (
                r.pos, r.ref_end, r.mapq, r.flag, int(r.is_reverse))
        assert len(set(got.name_hash.tolist())) == len(want)
        # a region: exactly the records overlapping it (pos < stop, end > start), in file order
        sub = b.fetch("chr1", 400, 420)
        assert [int(x) for x in sub.ref_starts] == [r.pos for r in want if r.pos < 420 and r.ref_end > 400]
        assert b.fetch("chr2", 0, 300).n_reads == 1
        assert b.fetch("chr1", 4000, 5000).n_reads == 0


def test_bam_index_and_scan_agree_far_into_the_file(tmp_path):
    from hello_amd.bam import BamFile
    reads = [Read(f"r{i}", 20 * i, [(0, 50)], "ACGT" * 12 + "AC", [30] * 50) for i in range(5000)]
    path = str(tmp_path / "far.bam")
    write_bam(path, [("c", 200000)], reads, index=True, block_bytes=4000)
    with BamFile(path) as b:
        a = b.fetch("c", 70000, 70100, use_index=True)
        s = b.fetch("c", 70000, 70100, use_index=False)
        assert a.used_index and not s.used_index
        assert a.n_blocks < s.n_blocks                              # the index skipped most of the file
        assert a.ref_starts.tolist() == s.ref_starts.tolist() == [20 * i for i in range(5000) if 70000 - 50 < 20 * i < 70100]


def test_bam_cigar_of_more_than_65535_operations_comes_from_the_cg_tag(tmp_path):
    from hello_amd.bam import BamFile
    ops = [(0, 1), (1, 1)] * 35000                                   # 70 000 operations: 70 000 bases over 35 000 positions
    long_read = Read("long", 1000, ops, "AC" * 35000, [30] * 70000,
                     tags=b"NMi" + (7).to_bytes(4, "little") + b"RGZgroup\0" + b"XBBs" + (2).to_bytes(4, "little") + b"\1\0\2\0")
    reads = [Read("short", 900, [(0, 50)], "A" * 50, [30] * 50), long_read, Read("after", 1100, [(0, 50)], "C" * 50, [30] * 50)]
    path = str(tmp_path / "long.bam")
    write_bam(path, [("c", 100000)], reads, block_bytes=5000)
    with BamFile(path) as b:
        got = b.fetch("c", 0, 100000)
        assert got.n_reads == 3
        seq, cigar, _ = got.read(1)
        assert cigar == ops and seq == long_read.seq
        assert (got.ref_starts[1], got.ref_ends[1]) == (1000, 36000)
        assert got.read(2)[1] == [(0, 50)]
        assert b.fetch("c", 30000, 30010).n_reads == 1                # found through its real span


def test_bam_refusals(tmp_path):
    from hello_amd.bam import BamFile
    cram = tmp_path / "x.cram"
    cram.write_bytes(b"CRAM\3\0" + b"\0" * 40)
    with pytest.raises(RuntimeError, match="CRAM"):
        BamFile(str(cram))
    plain = tmp_path / "x.txt"
    plain.write_text("not a bam")
    with pytest.raises(RuntimeError, match="not a BAM"):
        BamFile(str(plain))
    path = str(tmp_path / "noq.bam")
    write_bam(path, [("c", 1000)], [Read("noqual", 100, [(0, 10)], "ACGTACGTAC", None)])
    with BamFile(path) as b:
        with pytest.raises(RuntimeError, match="no stored base qualities"):
            b.fetch("c", 0, 1000)
        with pytest.raises(RuntimeError, match="no reference named"):
            b.fetch("chrX", 0, 10)
    path2 = str(tmp_path / "noidx.bam")
    write_bam(path2, [("c", 1000)], [], index=False)
    with BamFile(path2) as b:
        with pytest.raises(RuntimeError, match="no .bai index"):
            b.fetch("c", 0, 10, use_index=True)


# ---------------------------------------------------------------- chunk plan, CLI, output format


def test_chunk_plan_and_get_chunks():
    from hello_amd import hotspots as hs
    assert hs.get_chunks(1003, 500) == [(2 * i, 2 * i + 2) for i in range(500)] + [(1000, 1003)]
    assert hs.get_chunks(10, 500)[:3] == [(0, 0), (0, 0), (0, 0)] and hs.get_chunks(10, 500)[-1] == (0, 10)
    assert hs.chunk_plan(100, 1000, False, False) == [(100, 500), (500, 900), (900, 1000)]
    assert hs.chunk_plan(0, 25000, False, True) == [(0, 10000), (10000, 20000), (20000, 25000)]
    assert hs.chunk_plan(0, 25000, True, False) == hs.chunk_plan(0, 25000, False, True)
    assert hs.get_workdir("/a/b/x.bam", None, chrom="1", string="hotspots") == "hotspots_1_b___x__bam"


def test_cli_argument_surface():
    from hello_amd import hotspots as hs
    a = hs.parse_args(["--bam", "a.bam,b.bam", "--ref", "g.fa", "--region", "chr1,0,50000", "--output", "h.txt"])
    assert (a.pacbio, a.hybrid_hotspot, a.q_threshold, a.mapq_threshold, a.debug) == (False, False, 10, 10, False)
    a = hs.parse_args(["--bam", "a.bam", "--ref", "g.fa", "--region", "chr1", "--output", "h.txt", "--pacbio", "--hybrid_hotspot",
                       "--q_threshold", "7", "--mapq_threshold", "3", "--debug"])
    assert (a.pacbio, a.hybrid_hotspot, a.q_threshold, a.mapq_threshold, a.debug) == (True, True, 7, 3, True)
    with pytest.raises(SystemExit):
        hs.parse_args(["--bam", "a.bam", "--ref", "g.fa"])                      # neither --region/--output nor --workdir
    with pytest.raises(SystemExit):
        hs.parse_args(["--bam", "a.bam,b.bam,c.bam", "--ref", "g.fa", "--workdir", "w"])
    assert hs.parse_args(["--bam", "a.bam", "--ref", "g.fa", "--workdir", "w"]).workdir == "w"
    out = subprocess.run([sys.executable, "-m", "hello_amd.hotspots", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "--hybrid_hotspot" in out.stdout and "--mapq_threshold" in out.stdout


def test_output_line_format(tmp_path):
    from hello_amd import hotspots as hs
    path = str(tmp_path / "h.txt")
    hs.write_positions(path, "chr1", np.array([5, 17], np.int64))
    assert open(path).read() == "{'chromosome': 'chr1', 'position': 5}\n{'chromosome': 'chr1', 'position': 17}\n"


# ---------------------------------------------------------------- hand cases of the restatement
# Reference: 200 bases of ACGT repeats; ref[p] = "ACGT"[p % 4].  Reads start at >= 41, so windows start at >= 30 and no chunk is
# skipped; the single Illumina chunk is [40, 160).

REF = "ACGT" * 50


def _match(pos, n, name, alt_at=None, alt="T", q=30, flag=0, mapq=60):
    seq = list(REF[pos:pos + n])
    qual = [q] * n
    if alt_at is not None:
        seq[alt_at - pos] = alt
    return Read(name, pos, [(0, n)], "".join(seq), qual, flag, mapq)


def _run(reads, **kw):
    reads = sorted(reads, key=lambda r: r.pos)
    return hr.find_hotspots([reads], REF, 40, 160, **kw)


def hand_cases():
    """(name, read sets, kwargs, expected positions) -- the worked derivation is next to each case."""
    cases = []
    # SNV ratio boundary: ref[55] = 'T'; 3 reads carry 'A' at 55.  With 22 plain reads, total = 25 and 3/25 == 0.12f exactly
    # (float32(3) / float32(25) rounds to float32(0.12)) -> {55}.  With 23 plain reads 3/26 < 0.12 -> {}.
    snv = [_match(50, 20, f"a{i}", 55, "A") for i in range(3)]
    cases.append(("snv_at_0.12", [snv + [_match(50, 20, f"p{i}") for i in range(22)]], {}, [55]))
    cases.append(("snv_below_0.12", [snv + [_match(50, 20, f"p{i}") for i in range(23)]], {}, []))
    # the base quality 9 < q_threshold 10 drops the SNV key -> {}; q_threshold 9 keeps it -> {55}
    lowq = [Read(f"q{i}", 50, [(0, 20)], REF[50:55] + "A" + REF[56:70], [30] * 5 + [9] + [30] * 14) for i in range(3)]
    cases.append(("snv_low_quality", [lowq], {}, []))
    cases.append(("snv_q_threshold_9", [lowq], {"q_threshold": 9}, [55]))
    # one alt read is not enough (count 1 < 2) -> {}
    cases.append(("snv_single_read", [[_match(50, 20, "s")]], {}, []))
    # mapq 5 < 10: not counted -> {}; --mapq_threshold 5 -> {55}.  mapq 0 is not usable at all, at any threshold -> {}
    lowm = [_match(50, 20, f"m{i}", 55, "A", mapq=5) for i in range(3)]
    cases.append(("low_mapq", [lowm], {}, []))
    cases.append(("low_mapq_threshold_5", [lowm], {"mapq_threshold": 5}, [55]))
    cases.append(("mapq_zero", [[_match(50, 20, f"z{i}", 55, "A", mapq=0) for i in range(3)]], {"mapq_threshold": 0}, []))
    # filtered flags: duplicate, secondary, supplementary, unmapped, improper pair -> {}; QC-fail (0x200) and proper pairs stay -> {55}
    for f in (0x400, 0x100, 0x800, 0x4, 0x1):
        cases.append((f"flag_{f:#x}", [[_match(50, 20, f"f{i}", 55, "A", flag=f) for i in range(3)]], {}, []))
    cases.append(("flag_qcfail_proper", [[_match(50, 20, f"g{i}", 55, "A", flag=f) for i, f in enumerate((0x200, 0x3, 0x203))]], {}, [55]))
    # duplicate names: 3 alt reads named "d" forward -> only the first counts (1 < 2) -> {}; one on the other strand is kept -> 2 -> {55}
    cases.append(("duplicate_names", [[_match(50, 20, "d", 55, "A") for _ in range(3)]], {}, []))
    cases.append(("duplicate_names_other_strand", [[_match(50, 20, "d", 55, "A"), _match(50, 20, "d", 55, "A", flag=16)]], {}, [55]))
    # N: a read 'N' at 55 is no SNV key -> {}
    cases.append(("n_base", [[_match(50, 20, f"n{i}", 55, "N") for i in range(3)]], {}, []))
    # deletion 10M2D10M at 50: planted at 59, ref allele ref[59:62], Illumina count 2 per read.  One read: 2 < 4 -> {};
    # two reads: 4 >= 4, total[59] = 2 -> flags [59, 59 + 3 + 1) = 59..62
    def dele(name):
        return Read(name, 50, [(0, 10), (2, 2), (0, 10)], REF[50:60] + REF[62:72], [30] * 20)
    cases.append(("deletion_one_read", [[dele("x")]], {}, []))
    cases.append(("deletion_two_reads", [[dele("x"), dele("y")]], {}, [59, 60, 61, 62]))
    # a deletion as the first operation (rdcounter 0): alt = ref[49], no quality check; two reads 1H2D20M at 50 -> planted at 49,
    # ref allele ref[49:52], count 4, total[49] = 0 (nothing aligned there) -> skipped; add one read over 49 -> total 1 -> 49..52
    def dstart(name):
        return Read(name, 50, [(5, 1), (2, 2), (0, 20)], REF[52:72], [30] * 20)
    cases.append(("deletion_at_read_start_no_total", [[dstart("u"), dstart("v")]], {}, []))
    cases.append(("deletion_at_read_start", [[dstart("u"), dstart("v"), _match(45, 20, "w")]], {}, [49, 50, 51, 52]))
    # insertions: full 9M2I9M at 41 plants at 49 (alt = ref[49] + "TT"), count 2 < 4 -> {}.  Add a left partial 2I18M at 50
    # (alt "TT", a suffix of the full alt: one match, +2 -> 4; its total +1): total[49] = 2, 4/2 >= 0.12 -> [49, 51) = {49, 50}
    full_ins = Read("fi", 41, [(0, 9), (1, 2), (0, 9)], REF[41:50] + "TT" + REF[50:59], [30] * 20)
    left = Read("lp", 50, [(1, 2), (0, 18)], "TT" + REF[50:68], [30] * 20)
    cases.append(("full_insertion_alone", [[full_ins]], {}, []))
    cases.append(("left_partial_resolves", [[full_ins, left]], {}, [49, 50]))
    # hard clips count in the operation index (:250,312): in 3H2I18M the insertion is operation 1, so it is a FULL insertion at the
    # read's first base, alt = ref[49] + "TT" (:289), count 2.  With the 9M2I9M read the key 'CTT' has 4 -> {49, 50} (as above).
    left_h = Read("lh", 50, [(5, 3), (1, 2), (0, 18)], "TT" + REF[50:68], [30] * 20)
    cases.append(("hard_clipped_insertion_with_full", [[full_ins, left_h]], {}, [49, 50]))
    # the case that tells the readings apart: two 3H2I18M reads and one read covering 49, no other insertion.  Full insertions:
    # key 'CTT' count 4, total[49] = 1 (the covering read; a full insertion adds no total) -> [49, 51) = {49, 50}.  Read as left
    # partials they would find no key and be dropped -> {}.
    hard2 = [Read(f"lh{i}", 50, [(5, 3), (1, 2), (0, 18)], "TT" + REF[50:68], [30] * 20) for i in range(2)]
    cases.append(("hard_clipped_insertion_is_full", [hard2 + [_match(45, 20, "cov")]], {}, [49, 50]))
    # without the covering read total[49] = 0 and the position is skipped (:848) -> {}
    cases.append(("hard_clipped_insertion_no_total", [hard2], {}, []))
    # right partial: 18M2I at 32 plants at 49, alt = ref[49] + "TT" (its prefix equals the full alt) -> one match, +2 -> {49, 50}
    right = Read("rp", 32, [(0, 18), (1, 2)], REF[32:50] + "TT", [30] * 20)
    cases.append(("right_partial_resolves", [[full_ins, right]], {}, [49, 50]))
    # two full keys the left partial "T" matches (alts ref[49]+"TT" and ref[49]+"T") -> dropped; each full key has 2 -> {}
    full_ins1 = Read("fj", 41, [(0, 9), (1, 1), (0, 10)], REF[41:50] + "T" + REF[50:60], [30] * 20)
    left1 = Read("lq", 50, [(1, 1), (0, 19)], "T" + REF[50:69], [30] * 20)
    cases.append(("ambiguous_partial_dropped", [[full_ins, full_ins1, left1]], {}, []))
    # a partial alone never creates a key -> {}
    cases.append(("partial_alone", [[left, Read("lr", 50, [(1, 2), (0, 18)], "TT" + REF[50:68], [30] * 20)]], {}, []))
    # a left partial of length 1 matches an SNV key: two reads 'A' at 55 plus... SNV count 2 at 55 (A), total 2 -> flagged anyway;
    # use 2 SNV reads + 20 plain reads: 2/22 < 0.12 -> {}; a left partial "A" planted at 55 (1I19M at 56) adds 2 -> 4, total 23 -> {55}
    snv2 = [_match(50, 20, f"b{i}", 55, "A") for i in range(2)] + [_match(50, 20, f"c{i}") for i in range(20)]
    cases.append(("snv_without_partial", [snv2], {}, []))
    cases.append(("left_partial_into_snv", [snv2 + [Read("ls", 56, [(1, 1), (0, 19)], "A" + REF[56:75], [30] * 20)]], {}, [55]))
    # PacBio: a deletion flags with count 2 (increment 1 per read: two reads) -> 59..62
    cases.append(("pacbio_deletion", [[dele("x"), dele("y")]], {"pacbio": True}, [59, 60, 61, 62]))
    # soft-masked reference: lowercase ref bytes mismatch uppercase read bases -> handled in the GPU suite (needs its own REF)
    # a chunk whose reads end past the chromosome is skipped: a read 10M45D10M at 150 ends at 215 on a 200 bp reference -> {}
    cases.append(("past_chromosome_end", [[_match(50, 20, f"e{i}", 55, "A") for i in range(3)] +
                                          [Read("end", 150, [(0, 10), (2, 45), (0, 10)], "A" * 20, [30] * 20)]], {}, []))
    return cases


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_restatement_hand_cases(case):
    name, read_sets, kw, expected = case
    if len(read_sets) == 1:
        assert _run(read_sets[0], **kw) == expected, name


def test_restatement_hybrid_hand_cases():
    # two BAMs, 10 kbp chunks: Illumina 1 read 'A' at 55, PacBio 1 read 'A' at 55: without --hybrid_hotspot each table has
    # count 1 < 2 -> {}; with it vi + vp = 2 >= 2, total 2 -> {55}.  A key only in the PacBio table is never looked at -> {}
    il = [_match(50, 20, "i", 55, "A")]
    pb = [_match(50, 20, "p", 55, "A")]
    assert hr.find_hotspots([il, pb], REF, 40, 160) == []
    assert hr.find_hotspots([il, pb], REF, 40, 160, hybrid_hotspot=True) == [55]
    assert hr.find_hotspots([[], pb + [_match(50, 20, "p2", 55, "A")]], REF, 40, 160, hybrid_hotspot=True) == []
    # hybrid deletion: Illumina 1 read (vi = 2), PacBio 1 read (vp = 1): vi/2 + vp = 2 -> flags [59, 59 + 3) = 59..61
    dl = Read("di", 50, [(0, 10), (2, 2), (0, 10)], REF[50:60] + REF[62:72], [30] * 20)
    dp = Read("dp", 50, [(0, 10), (2, 2), (0, 10)], REF[50:60] + REF[62:72], [30] * 20)
    assert hr.find_hotspots([[dl], [dp]], REF, 40, 160, hybrid_hotspot=True) == [59, 60, 61]
    # without --hybrid_hotspot: Illumina 2 < 4, PacBio 1 < 2 -> {}
    assert hr.find_hotspots([[dl], [dp]], REF, 40, 160) == []


def test_restatement_clips_to_chunks_and_caps():
    # an indel planted at 398 flags 398..401 but the chunk [0+40.., 440) boundary at 440 clips nothing here: use region [40, 400)
    ref = "ACGT" * 150
    d = [Read(n, 390, [(0, 9), (2, 3), (0, 10)], ref[390:399] + ref[402:412], [30] * 19) for n in ("a", "b")]
    assert hr.find_hotspots([d], ref, 40, 440) == [398, 399, 400, 401, 402]
    assert hr.find_hotspots([d], ref, 40, 400) == [398, 399]          # the chunk [40, 400) keeps its own part only
    # read cap: 10 001 usable reads keep the first 10 000; the statistic says so
    stats = {}
    many = [Read(f"c{i}", 100, [(0, 10)], ref[100:110], [30] * 10) for i in range(10001)]
    hr.find_hotspots([many], ref, 40, 440, stats=stats)
    assert stats.get("capped") == 1
