"""GPU hotspot detection (hello_hotspots_find, hello_amd/csrc/hotspots.hip) against the Python restatement
(tests/hotspot_reference.py): the same positions, exactly, on random regions of every mode and on the hand cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hotspot_reference as hr
from tests import hotspot_synth as synth
from tests.bam_writer import Read, write_bam
from tests.test_hotspots import REF as HAND_REF, hand_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write(tmp_path, name, chrom, reference, reads, index=True):
    path = str(tmp_path / name)
    write_bam(path, [(chrom, len(reference))], reads, index=index, block_bytes=20000)
    return path


def _fasta(tmp_path, chrom, reference):
    path = str(tmp_path / "g.fa")
    with open(path, "w") as fh:
        fh.write(f">{chrom} test\n")
        for i in range(0, len(reference), 60):
            fh.write(reference[i:i + 60] + "\n")
    return path


def _both(tmp_path, sets, reference, start, stop, **kw):
    from hello_amd import hotspots as hs
    paths = [_write(tmp_path, f"s{i}.bam", "chr1", reference, reads) for i, reads in enumerate(sets)]
    fa = _fasta(tmp_path, "chr1", reference)
    got = hs.find_hotspots(paths, fa, "chr1", start, stop, **kw)
    want = hr.find_hotspots(sets, reference, start, stop, **kw)
    return got.tolist(), want


@pytest.mark.parametrize("mode", ["illumina", "pacbio", "two_bams", "hybrid"])
def test_random_regions_match_the_restatement(tmp_path, mode):
    rng = np.random.default_rng({"illumina": 11, "pacbio": 12, "two_bams": 13, "hybrid": 14}[mode])
    length = 70000
    reference = synth.random_reference(rng, length, masked_fraction=0.02)     # soft-masked stretches mismatch upper-case reads
    start = int(rng.integers(0, 5000))
    stop = start + int(rng.integers(20000, 60001))
    il = synth.sample_reads(rng, reference, 8, 150, snv_rate=0.01, indel_rate=0.004, prefix="i")
    pb = synth.sample_reads(rng, reference, 5, 3000, snv_rate=0.01, indel_rate=0.004, pacbio=True, prefix="p")
    if mode == "illumina":
        sets, kw = [il], {}
    elif mode == "pacbio":
        sets, kw = [pb], {"pacbio": True}
    else:
        sets, kw = [il, pb], {"hybrid_hotspot": mode == "hybrid"}
    got, want = _both(tmp_path, sets, reference, start, stop, **kw)
    assert len(want) > 20, "the random case should flag something"
    assert got == want


def test_hand_cases_on_the_gpu(tmp_path):
    from hello_amd import hotspots as hs
    from hello_amd.bam import BamFile
    for i, (name, read_sets, kw, expected) in enumerate(hand_cases()):
        reads = sorted(read_sets[0], key=lambda r: r.pos)
        path = _write(tmp_path, f"h{i}.bam", "chr1", HAND_REF, reads)
        with BamFile(path) as b:
            r = b.fetch("chr1", 40, 160)
        got, _ = hs.find_positions([r], HAND_REF, [(40, 160)], **kw)
        assert got.tolist() == expected, name


def test_edges_chromosome_ends_empty_regions_and_determinism(tmp_path):
    from hello_amd import hotspots as hs
    rng = np.random.default_rng(21)
    reference = synth.random_reference(rng, 30000)
    reads = synth.sample_reads(rng, reference, 12, 150, snv_rate=0.02, indel_rate=0.01, prefix="e")
    # deletions at the start of a read, leading and trailing insertions, N bases and a repeated name, planted by hand
    extra = []
    for k in range(6):
        p = 1000 + 37 * k
        extra.append(Read(f"ds{k}", p, [(5, 2), (2, 3), (0, 40)], reference[p + 3:p + 43].upper(), [35] * 40))
        extra.append(Read(f"li{k}", p, [(1, 3), (0, 40)], "GGG" + reference[p:p + 40].upper(), [35] * 43))
        extra.append(Read(f"ti{k}", p, [(0, 40), (1, 4)], reference[p:p + 40].upper() + "CCCC", [35] * 44))
        extra.append(Read(f"nn{k}", p, [(0, 40)], "N" * 5 + reference[p + 5:p + 40].upper(), [35] * 40))
    reads = sorted(reads + extra, key=lambda r: r.pos)
    # the whole chromosome: chunks at both ends whose windows leave it are skipped
    got, want = _both(tmp_path, [reads], reference, 0, len(reference))
    assert got == want and len(want) > 50
    # indels across chunk edges: regions whose chunk boundaries fall anywhere
    for s in (7, 399, 401):
        got, want = _both(tmp_path, [reads], reference, s, s + 4000)
        assert got == want
    # empty regions, a region without reads
    assert _both(tmp_path, [reads], reference, 500, 500)[0] == []
    assert _both(tmp_path, [[]], reference, 0, len(reference)) == ([], [])
    # two runs, the same bytes
    path = _write(tmp_path, "d.bam", "chr1", reference, reads)
    fa = _fasta(tmp_path, "chr1", reference)
    a = hs.find_hotspots(path, fa, "chr1", 0, len(reference))
    b = hs.find_hotspots(path, fa, "chr1", 0, len(reference))
    assert a.tobytes() == b.tobytes()
    # the same answer whether the region was located with the .bai or by scanning
    noidx = _write(tmp_path, "n.bam", "chr1", reference, reads, index=False)
    assert hs.find_hotspots(noidx, fa, "chr1", 0, len(reference)).tobytes() == a.tobytes()


def test_cli_file_matches_the_api(tmp_path):
    from hello_amd import hotspots as hs
    rng = np.random.default_rng(31)
    reference = synth.random_reference(rng, 60000)
    reads = synth.sample_reads(rng, reference, 10, 150, prefix="c")
    path = _write(tmp_path, "x.bam", "chr1", reference, reads)
    fa = _fasta(tmp_path, "chr1", reference)
    out = str(tmp_path / "h.txt")
    run = subprocess.run([sys.executable, "-m", "hello_amd.hotspots", "--bam", path, "--ref", fa, "--region", "chr1,0,50000",
                          "--output", out], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert run.stderr.strip().splitlines()[-1].endswith("Completed running the script")
    api = hs.find_hotspots(path, fa, "chr1", 0, 50000)
    assert api.tolist() == hr.find_hotspots([reads], reference, 0, 50000)
    assert open(out).read() == "".join(str({'chromosome': 'chr1', 'position': int(p)}) + "\n" for p in api)
    # --workdir: job files per get_chunks(len, 500) region, concatenated into hotspots.txt
    wd = str(tmp_path / "wd")
    run = subprocess.run([sys.executable, "-m", "hello_amd.hotspots", "--bam", path, "--ref", fa, "--workdir", wd],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    d = os.path.join(wd, hs.get_workdir(path, None, chrom="chr1", string="hotspots"))
    jobs = [os.path.join(d, "job_chromosomechr1_job%d.txt" % i) for i in range(len(hs.get_chunks(len(reference), 500)))]
    assert all(os.path.exists(j) for j in jobs)
    want = []
    for a, b in hs.get_chunks(len(reference), 500):
        want += hr.find_hotspots([reads], reference, a, b)
    text = open(os.path.join(d, "hotspots.txt")).read()
    assert text == "".join(str({'chromosome': 'chr1', 'position': p}) + "\n" for p in want)


@pytest.mark.parametrize("hybrid", [False, True])
def test_second_bam_without_reads_keeps_the_two_bam_chunks(tmp_path, hybrid):
    """Two BAMs whose second has no reads in the region: the reference still cuts 10 kbp chunks (hotspotGeneratorHybrid)."""
    rng = np.random.default_rng(41)
    reference = synth.random_reference(rng, 30000)
    il = synth.sample_reads(rng, reference, 8, 150, snv_rate=0.01, indel_rate=0.004, prefix="i")
    got, want = _both(tmp_path, [il, []], reference, 0, 30000, hybrid_hotspot=hybrid)
    assert got == want
    assert want != hr.find_hotspots([il], reference, 0, 30000, hybrid_hotspot=hybrid)    # the case tells the chunkings apart


def test_event_capacity_is_one_slot_per_planted_indel_and_long_cigars_count(tmp_path):
    """Each I/D operation of a counted read takes one slot, in the tile of its planting position; reads whose CIGAR has more than
    65 535 operations (kept in the CG tag) are counted like any other."""
    from hello_amd import hotspots as hs
    from hello_amd.bam import BamFile
    rng = np.random.default_rng(51)
    reference = synth.random_reference(rng, 60000)
    ops = [(0, 1), (1, 1)] * 35000
    reads = []
    for k in range(3):                       # identical 1-base insertions after every base of [20000, 55000)
        seq = "".join(reference[20000 + i].upper() + "G" for i in range(35000))
        reads.append(Read(f"long{k}", 20000, ops, seq, [30] * 70000))
    reads += [Read(f"s{k}", 20100 + 300 * k, [(0, 60), (2, 3), (0, 40)],
                   reference[20100 + 300 * k:20160 + 300 * k].upper() + reference[20163 + 300 * k:20203 + 300 * k].upper(), [30] * 100)
              for k in range(20)]
    reads.sort(key=lambda r: r.pos)
    path = _write(tmp_path, "l.bam", "chr1", reference, reads)
    with BamFile(path) as b:
        r = b.fetch("chr1", 20000, 30000)
    got, stats = hs.find_positions([r], reference, [(20000, 30000)], pacbio=True)   # one 10 kbp chunk holds every read
    assert stats["event_capacity"] == 3 * 35000 + 20
    assert got.tolist() == hr.find_hotspots([reads], reference, 20000, 30000, pacbio=True)
    assert len(got) > 9000
