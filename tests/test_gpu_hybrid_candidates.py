"""GPU candidate sites from an Illumina and a PacBio BAM together (hello_candidates_find_hybrid, hello_amd/csrc/candidates.hip)
against the Python restatement (tests/hybrid_reference.py): both passes' regions, the sites, alleles, per-technology reads per
allele, the clipped bases, quals, CIGARs and starts, read_index and every count statistic, exactly.  The synthetic inputs were
chosen with the restatement on the CPU so that they meet the conditions ``check_conditions`` asserts; the tests filter nothing."""
import copy
import os

import numpy as np
import pytest

from tests import candidate_reference as cr
from tests import hotspot_reference as hr
from tests import hotspot_synth as synth
from tests import hybrid_reference as hy
from tests.bam_writer import Read
from tests.test_gpu_candidates import _fasta, _write
from tests.test_hybrid_candidates import hybrid_hand_cases, site_names

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_KEYS = list(hy.STAT_KEYS)


def _same(shard, sites, chrom="chr1"):
    """Every payload array of the GPU shard equals the payload of the restatement's sites; has_second is set regardless."""
    from hello_amd import shards
    want = shards._payload(hy.candidate_sites(sites, chrom))
    assert int(np.asarray(shard.z["has_second"]).reshape(-1)[0]) == 1 and shard.hybrid
    if not sites:                          # a payload without sites cannot say that it is hybrid: both technologies are empty
        assert shard.n_sites == 0
        for tech in (0, 1):
            assert np.asarray(shard.z[f"reads_per_allele{tech}"]).size == 0 and np.asarray(shard.z[f"bases{tech}"]).size == 0
        return
    assert sorted(shard.z) == sorted(want)
    for k in want:
        a, b = np.asarray(shard.z[k]), np.asarray(want[k])
        assert a.dtype == b.dtype or k == "has_second", k
        assert np.array_equal(a.reshape(-1), b.reshape(-1)), k


def _read_index(sites, illumina, pacbio, positions):
    """The restatement's gathered reads as indices into what the BAM reader returns for the call's interval, per technology."""
    lo = max(0, min(positions) - 15 - 75)
    hi = max(positions) + 15 + 75
    out = []
    for tech, reads in ((0, illumina), (1, pacbio)):
        fetched = {id(r): i for i, r in enumerate(r for r in reads if r.pos < hi and r.ref_end > lo)}
        out.append([fetched[id((s.reads0 if tech == 0 else s.originals1)[i])] for s in sites for a in s.alleles for i in a[1 + tech]])
    return out


def _files(tmp_path, illumina, pacbio, reference, name="h"):
    return (_write(tmp_path, name + "_i.bam", "chr1", reference, illumina), _write(tmp_path, name + "_p.bam", "chr1", reference, pacbio),
            _fasta(tmp_path, "chr1", reference))


def _both(tmp_path, illumina, pacbio, reference, positions, name="h", files=None, **kw):
    from hello_amd import hybrid
    ibam, pbam, fa = files or _files(tmp_path, illumina, pacbio, reference, name)
    st, want_st = {}, {}
    sites = hy.find_candidates(illumina, pacbio, reference, positions, stats=want_st, **kw)
    shard = hybrid.find_hybrid_candidates([ibam, pbam], fa, "chr1", positions, stats=st, **kw)
    assert st["regions_pass1"].reshape(-1, 2).tolist() == [list(r) for r in want_st["regions_pass1"]]
    assert st["regions_pass2"].reshape(-1, 2).tolist() == [list(r) for r in want_st["regions_pass2"]]
    assert {k: int(st[k]) for k in COUNT_KEYS} == {k: want_st[k] for k in COUNT_KEYS}
    _same(shard, sites)
    if len(positions):
        want0, want1 = _read_index(sites, illumina, pacbio, list(positions))
        assert st["read_index0"].tolist() == want0 and st["read_index1"].tolist() == want1
    return shard, sites, st, want_st, (ibam, pbam, fa)


def _edit(read, position, base):
    """`read` with `base` at reference position `position` (inside one of its M operations)."""
    rf, rd = read.pos, 0
    for op, n in read.cigar:
        if op in (0, 7, 8):
            if rf <= position < rf + n:
                k = rd + position - rf
                return Read(read.name, read.pos, read.cigar, read.seq[:k] + base + read.seq[k + 1:], read.qual, read.flag, read.mapq)
            rf += n
            rd += n
        elif op in (2, 3):
            rf += n
        elif op in (1, 4):
            rd += n
    return read


def synthetic(seed, length=60000):
    """Illumina reads (150 bp, about 30x) and PacBio reads (about 3 kb, about 25x, PacBio noise) of one donor and of the reference
    haplotype.  Over an eighth of the chromosome, from a fifth of its length on, two of three Illumina reads are left out (about
    10x: closed gates).  In the middle the reference holds C TTTTTTTT G: five planted Illumina reads delete the run's first T,
    five its last, and two planted PacBio reads lack a T -- two choices of Illumina alleles spell their haplotype (the tie
    rule).  At three quarters ten SNVs three bases apart are written into the donor's reads of both technologies: a cluster of
    ten regions, not reassembled."""
    RUN_AT, DENSE_AT, THIN = length // 2, 3 * length // 4, (length // 5, length // 5 + length // 8)
    rng = np.random.default_rng(seed)
    reference = synth.random_reference(rng, length)
    reference = reference[:RUN_AT] + "C" + "T" * 8 + "G" + reference[RUN_AT + 10:]
    donor = np.random.default_rng(seed + 1000)           # both technologies draw the same donor from a copy of this state
    illumina = synth.sample_reads(copy.deepcopy(donor), reference, 16, 150, snv_rate=0.002, indel_rate=0.001, prefix="a")
    pacbio = synth.sample_reads(copy.deepcopy(donor), reference, 13, 3000, snv_rate=0.002, indel_rate=0.001, pacbio=True, prefix="pa")
    illumina += synth.sample_reads(rng, reference, 14, 150, snv_rate=0.0, indel_rate=0.0, prefix="b")
    pacbio += synth.sample_reads(rng, reference, 12, 3000, snv_rate=0.0, indel_rate=0.0, pacbio=True, prefix="pb")
    illumina.sort(key=lambda r: r.pos)
    illumina = [r for i, r in enumerate(illumina) if not (THIN[0] <= r.pos < THIN[1]) or i % 3 == 0]
    dense = [DENSE_AT + 3 * k for k in range(10)]

    def with_dense(r):
        if not r.name.startswith(("a", "pa")):
            return r
        for p in dense:
            r = _edit(r, p, "ACGT"[("ACGT".index(reference[p].upper()) + 1) % 4])
        return r
    illumina, pacbio = [with_dense(r) for r in illumina], [with_dense(r) for r in pacbio]

    def without(name, pos, n, at):                       # a planted read of the reference with the base at `at` deleted
        k = at - pos
        seq = reference[pos:at] + reference[at + 1:pos + n]
        return Read(name, pos, [(0, k), (2, 1), (0, n - k - 1)], seq.upper(), [30] * (n - 1))
    illumina += [without(f"tl{i}", RUN_AT - 70 + i, 150, RUN_AT + 1) for i in range(5)]
    illumina += [without(f"tr{i}", RUN_AT - 70 + i, 150, RUN_AT + 8) for i in range(5)]
    pacbio += [without(f"pt{i}", max(0, RUN_AT - 1500 + 10 * i), min(3000, length - RUN_AT), RUN_AT + 8) for i in range(2)]
    illumina.sort(key=lambda r: r.pos)
    pacbio.sort(key=lambda r: r.pos)
    return reference, illumina, pacbio


def check_conditions(st):
    """The conditions on a synthetic input, evaluated on the restatement's statistics."""
    assert st["regions_at_read_cap"] + st["clusters_at_read_cap"] == 0                    # no searcher reaches a read cap
    assert st["clusters_reassembled"] >= 20
    ran = st["clusters"] - st["clusters_without_reads"] - st["clusters_out_of_bounds"]
    assert ran - st["clusters_gate_passed"] >= 5                                          # closed gates
    assert st["pacbio_reads_reassigned"] >= 50
    assert st["pacbio_reads_reassigned_by_tie"] >= 1
    assert st["clusters_skipped_for_size"] >= 1                                           # gate open, 10 or more regions


def test_hand_cases_on_the_gpu(tmp_path):
    for i, (name, illumina, pacbio, reference, positions, kw, expected, expected_stats) in enumerate(hybrid_hand_cases()):
        shard, sites, st, want_st, _ = _both(tmp_path, illumina, pacbio, reference, positions, name=f"h{i}", **kw)
        assert site_names(sites) == expected, name
        got = [(int(shard.start[s]), int(shard.stop[s]), shard.names(s)) for s in range(shard.n_sites)]
        assert got == [(a, b, [t for t, _, _ in al]) for a, b, al in expected], name
        counts = iter(zip(np.asarray(shard.z["reads_per_allele0"]).tolist(), np.asarray(shard.z["reads_per_allele1"]).tolist()))
        assert [[next(counts) for _ in al] for _, _, al in expected] == [[(len(i0), len(i1)) for _, i0, i1 in al] for _, _, al in expected], name
        assert {k: int(st[k]) for k in expected_stats} == expected_stats, name


@pytest.mark.parametrize("seed", [305, 306])
def test_synthetic_chromosomes_match_the_restatement(tmp_path, seed):
    """The hotspot positions come from the GPU hotspot stage over both BAMs (tests/test_gpu_hotspots.py holds it to its own
    restatement); the first 10 kbp chunk of a two-BAM run is out of bounds there as in the reference."""
    from hello_amd import hotspots as hs
    reference, illumina, pacbio = synthetic(seed)
    assert np.median([len(r.seq) for r in pacbio]) > 2500
    files = _files(tmp_path, illumina, pacbio, reference)
    positions = hs.find_hotspots(list(files[:2]), files[2], "chr1", 0, len(reference)).tolist()
    shard, sites, st, want_st, _ = _both(tmp_path, illumina, pacbio, reference, positions, files=files)
    check_conditions(want_st)
    assert len(sites) > 100 and any(len(s.alleles) > 1 for s in sites)
    assert st["reassembly_ms"] > 0 and st["clip_kernel_ms"] > 0


def test_hybrid_hotspot_and_two_runs_give_the_same_bytes(tmp_path):
    from hello_amd import hotspots as hs, hybrid
    reference, illumina, pacbio = synthetic(303, 30000)
    files = _files(tmp_path, illumina, pacbio, reference)
    positions = hs.find_hotspots(list(files[:2]), files[2], "chr1", 0, len(reference), hybrid_hotspot=True).tolist()
    shard, sites, st, want_st, (ibam, pbam, fa) = _both(tmp_path, illumina, pacbio, reference, positions, files=files, hybrid_hotspot=True)
    assert len(sites) > 50 and want_st["pacbio_reads_reassigned"] > 0
    plain = {}
    hy.find_candidates(illumina, pacbio, reference, positions, stats=plain)
    assert plain["regions_pass2"] != want_st["regions_pass2"]           # the hybrid rule flags other positions than the union
    st2 = {}
    again = hybrid.find_hybrid_candidates([ibam, pbam], fa, "chr1", positions, hybrid_hotspot=True, stats=st2)
    for k in shard.z:
        assert np.asarray(shard.z[k]).tobytes() == np.asarray(again.z[k]).tobytes(), k
    for k in ("read_index0", "read_index1", "regions_pass1", "regions_pass2"):
        assert st[k].tobytes() == st2[k].tobytes(), k


def test_the_single_bam_entry_still_refuses_two_bams(tmp_path):
    from hello_amd import candidates as cd
    from hello_amd.bam import BamFile
    from hello_amd.hotspots import HOTSPOTS_HYBRID, HOTSPOTS_TWO_BAMS
    name, illumina, pacbio, reference, positions, kw, expected, _ = hybrid_hand_cases()[0]
    path = _write(tmp_path, "i.bam", "chr1", reference, illumina)
    with BamFile(path) as b:
        reads = b.fetch("chr1", 0, len(reference))
    for options in (HOTSPOTS_TWO_BAMS, HOTSPOTS_HYBRID):
        with pytest.raises(ValueError, match="one Illumina BAM"):
            cd.find_sites(reads, reference, positions, options=options)


def test_from_bams_end_to_end(tmp_path):
    """python -m hello_amd.call --from_bams: the VCF equals the one obtained by scoring the restatement's sites, written with
    write_shard, through the same two-technology network."""
    import subprocess
    import sys
    from hello_amd import candidates as cd, hotspots as hs, loader, shards
    from tests.util import load_fixture
    reference, illumina, pacbio = synthetic(304, 20000)
    ibam = _write(tmp_path, "e_i.bam", "chr1", reference, illumina)
    pbam = _write(tmp_path, "e_p.bam", "chr1", reference, pacbio)
    fa = _fasta(tmp_path, "chr1", reference)
    model = str(tmp_path / "model.hello.npz")
    spec, state, _, _ = load_fixture("hybrid_full")          # tests/golden/hybrid_full.npz: the two-technology fixture model
    assert spec.name == "hybrid_full"
    loader.save_native(model, "hybrid_full", state)

    def records_of(vcf_path):
        return [line for line in open(vcf_path) if line.strip() and not line.startswith("#")]

    def run(extra, workdir):
        done = subprocess.run([sys.executable, "-m", "hello_amd.call", "--ibam", ibam, "--pbam", pbam, "--ref", fa, "--workdir", workdir,
                               "--network", model] + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0, done.stderr[-3000:]
        return records_of(os.path.join(workdir, "results.output.vcf"))
    got = run(["--from_bams"], str(tmp_path / "w1"))
    assert os.path.isfile(os.path.join(str(tmp_path / "w1"), hs.get_workdir(ibam, pbam, chrom="chr1", string="hotspots"), "hotspots.txt"))
    hot = []
    for a, b in hs.get_chunks(len(reference), 500):
        hot += hr.find_hotspots([illumina, pacbio], reference, a, b)
    shard_dir = tmp_path / "ref_shards"
    shard_dir.mkdir()
    n_sites = 0
    for n, part in enumerate(cd.shard_positions(hot)):
        sites = hy.candidate_sites(hy.find_candidates(illumina, pacbio, reference, part), "chr1")
        n_sites += len(sites)
        shards.write_shard(str(shard_dir / f"shard{n}.hshard"), sites)
    want = run(["--shards", str(shard_dir)], str(tmp_path / "w2"))
    assert got == want and len(got) > 0 and n_sites > 10
