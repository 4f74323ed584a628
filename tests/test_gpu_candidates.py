"""GPU candidate sites (hello_candidates_find, hello_amd/csrc/candidates.hip) against the Python restatement
(tests/candidate_reference.py): the same sites, alleles, supporting reads and payload arrays, exactly."""
import copy
import os

import numpy as np
import pytest

from tests import candidate_reference as cr
from tests import hotspot_reference as hr
from tests import hotspot_synth as synth
from tests.bam_writer import write_bam
from tests.test_candidates import REF as HAND_REF, hand_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_KEYS = [k for k in cr.STAT_KEYS]


def _write(tmp_path, name, chrom, reference, reads):
    path = str(tmp_path / name)
    write_bam(path, [(chrom, len(reference))], reads, index=True, block_bytes=20000)
    return path


def _fasta(tmp_path, chrom, reference):
    path = str(tmp_path / "g.fa")
    with open(path, "w") as fh:
        fh.write(f">{chrom} test\n")
        for i in range(0, len(reference), 60):
            fh.write(reference[i:i + 60] + "\n")
    return path


def _same(shard, sites, chrom="chr1"):
    """Every payload array of the GPU shard equals the payload of the restatement's sites."""
    from hello_amd import shards
    want = shards._payload(cr.candidate_sites(sites, chrom))
    assert sorted(shard.z) == sorted(want)
    for k in want:
        a, b = np.asarray(shard.z[k]), np.asarray(want[k])
        assert a.dtype == b.dtype or k == "has_second", k
        assert np.array_equal(a.reshape(-1), b.reshape(-1)), k


def _both(tmp_path, reads, reference, positions, name="c.bam", **kw):
    from hello_amd import candidates as cd
    path = _write(tmp_path, name, "chr1", reference, reads)
    fa = _fasta(tmp_path, "chr1", reference)
    st, want_st = {}, {}
    shard = cd.find_candidates(path, fa, "chr1", positions, stats=st, **kw)
    sites = cr.find_candidates(reads, reference, positions, stats=want_st, **kw)
    assert st["regions_pass1"].reshape(-1, 2).tolist() == [list(r) for r in want_st["regions_pass1"]]
    assert st["regions_pass2"].reshape(-1, 2).tolist() == [list(r) for r in want_st["regions_pass2"]]
    assert {k: int(st[k]) for k in COUNT_KEYS} == {k: want_st[k] for k in COUNT_KEYS}
    _same(shard, sites)
    return shard, sites, st


def test_hand_cases_on_the_gpu(tmp_path):
    for i, (name, reads, positions, kw, expected) in enumerate(hand_cases()):
        reads = sorted(reads, key=lambda r: r.pos)
        shard, sites, _ = _both(tmp_path, reads, HAND_REF, positions, name=f"h{i}.bam", **kw)
        got = [(int(shard.start[s]), int(shard.stop[s]), shard.names(s)) for s in range(shard.n_sites)]
        assert got == [(a, b, [t for t, _ in al]) for a, b, al in expected], name


@pytest.mark.parametrize("seed", [101, 102])
def test_synthetic_chromosomes_match_the_restatement_and_runs_are_identical(tmp_path, seed):
    from hello_amd import candidates as cd
    from hello_amd import hotspots as hs
    rng = np.random.default_rng(seed)
    reference = synth.random_reference(rng, 60000, masked_fraction=0.02)
    reads = synth.sample_reads(rng, reference, 25, 150, snv_rate=0.004, indel_rate=0.002, prefix="a")
    reads += synth.sample_reads(rng, reference, 20, 150, snv_rate=0.0, indel_rate=0.0, prefix="b")     # the other haplotype
    reads.sort(key=lambda r: r.pos)
    path = _write(tmp_path, "s.bam", "chr1", reference, reads)
    fa = _fasta(tmp_path, "chr1", reference)
    positions = hs.find_hotspots(path, fa, "chr1", 0, len(reference))
    assert positions.tolist() == hr.find_hotspots([reads], reference, 0, len(reference))
    shard, sites, st = _both(tmp_path, reads, reference, positions.tolist())
    assert len(sites) > 100 and any(len(s.alleles) > 1 for s in sites)
    again = cd.find_candidates(path, fa, "chr1", positions)
    for k in shard.z:
        assert np.asarray(shard.z[k]).tobytes() == np.asarray(again.z[k]).tobytes(), k


def test_featurizer_gives_the_same_pileups_from_the_shard_and_from_the_restatement(tmp_path):
    from hello_amd import candidates as cd, netspec as ns, shards, weights
    from hello_amd.engine import Engine
    from hello_amd.featurizer import featurize
    rng = np.random.default_rng(111)
    reference = synth.random_reference(rng, 20000)
    reads = synth.sample_reads(rng, reference, 20, 150, snv_rate=0.004, indel_rate=0.002, prefix="a")
    reads += synth.sample_reads(rng, reference, 15, 150, snv_rate=0.0, indel_rate=0.0, prefix="b")
    reads.sort(key=lambda r: r.pos)
    positions = hr.find_hotspots([reads], reference, 0, len(reference))
    shard, sites, _ = _both(tmp_path, reads, reference, positions)
    assert shard.n_sites > 20
    back = shards.read_shard(cd.write_packed(str(tmp_path / "f.hshard"), shard))
    spec = ns.build("single_tech")
    eng = Engine(spec, weights.synth_state(spec, seed=2))
    try:
        got = featurize(eng, [s.site_reads(0) for s in back], feature_length=150)
        want = featurize(eng, [s.site_reads(0) for s in cr.candidate_sites(sites, "chr1")], feature_length=150)
    finally:
        eng.close()
    for g, w in zip(got, want):
        assert np.asarray(g).tobytes() == np.asarray(w).tobytes()
    assert np.asarray(got[0]).any()


def test_planted_variants_are_all_found(tmp_path):
    """Error-free reads of a donor and of the reference haplotype: every planted variant at least 31 bp from its neighbours and
    covered by at least 8 reads of each haplotype lies in a site holding the donor's allele and the reference allele.
    Variants within 400 bp of either end of the chromosome are left out on purpose (read starts thin out there and a site's
    feature window must fit the chromosome); 337 of the 389 planted variants qualify."""
    rng = np.random.default_rng(121)
    reference = synth.random_reference(rng, 150000)
    twin = copy.deepcopy(rng)
    donor_reads = synth.sample_reads(rng, reference, 30, 150, snv_rate=0.002, indel_rate=0.0005, error_rate=0.0, noisy=False, prefix="d")
    dseq, where = synth.donor(twin, reference, 0.002, 0.0005)                   # the donor sample_reads drew
    ref_reads = synth.sample_reads(rng, reference, 30, 150, snv_rate=0.0, indel_rate=0.0, error_rate=0.0, noisy=False, prefix="r")
    reads = sorted(donor_reads + ref_reads, key=lambda r: r.pos)
    variants = _variants(reference, dseq, where)
    cover_d = _coverage(donor_reads, len(reference))
    cover_r = _coverage(ref_reads, len(reference))
    qualifying = []
    for i, (a, b) in enumerate(variants):
        near = (i > 0 and a - variants[i - 1][1] < 31) or (i + 1 < len(variants) and variants[i + 1][0] - b < 31)
        if not near and a > 400 and b < len(reference) - 400 and min(cover_d[a - 2:b + 2].min(), cover_r[a - 2:b + 2].min()) >= 8:
            qualifying.append((a, b))
    assert len(qualifying) == 337                       # of 389 planted variants; the issue asks for at least 200
    positions = hr.find_hotspots([reads], reference, 0, len(reference))
    shard, sites, _ = _both(tmp_path, reads, reference, positions)
    donor_at = {w: i for i, w in enumerate(where) if w >= 0}
    for a, b in qualifying:
        hit = [s for s in range(shard.n_sites) if int(shard.start[s]) <= a and b <= int(shard.stop[s])]
        assert len(hit) == 1, (a, b)
        s0, s1 = int(shard.start[hit[0]]), int(shard.stop[hit[0]])
        names = shard.names(hit[0])
        assert reference[s0:s1] in names, (a, b, names)
        assert dseq[donor_at[s0]:donor_at[s1]] in names, (a, b, names)


def _variants(reference, dseq, where):
    """[first differing reference position, one past the last) of every planted SNV, insertion (the base left of it) and deletion."""
    out, last = [], -1
    i = 0
    while i < len(where):
        w = where[i]
        if w < 0:
            k = i
            while k < len(where) and where[k] < 0:
                k += 1
            out.append((max(last, 0), max(last, 0) + 1))
            i = k
            continue
        if last >= 0 and w > last + 1:
            out.append((last + 1, w))
        if dseq[i] != reference[w].upper():
            out.append((w, w + 1))
        last = w
        i += 1
    return sorted(set(out))


def _coverage(reads, n):
    c = np.zeros(n + 1, np.int64)
    for r in reads:
        c[r.pos] += 1
        c[min(r.ref_end, n)] -= 1
    return np.cumsum(c)[:n]


def test_from_bam_end_to_end_writes_the_non_reference_sites_of_the_restatement(tmp_path):
    """python -m hello_amd.call --from_bam: the VCF's record positions are the restatement's sites that the same network calls
    non-reference when scored from a write_shard of the restatement's sites."""
    import subprocess
    import sys
    from hello_amd import candidates as cd, hotspots as hs, loader, netspec as ns, shards, weights
    rng = np.random.default_rng(131)
    reference = synth.random_reference(rng, 20000)
    reads = synth.sample_reads(rng, reference, 20, 150, snv_rate=0.004, indel_rate=0.002, prefix="a")
    reads += synth.sample_reads(rng, reference, 15, 150, snv_rate=0.0, indel_rate=0.0, prefix="b")
    reads.sort(key=lambda r: r.pos)
    bam = _write(tmp_path, "e.bam", "chr1", reference, reads)
    fa = _fasta(tmp_path, "chr1", reference)
    model = str(tmp_path / "model.hello.npz")
    loader.save_native(model, "single_tech", weights.synth_state(ns.build("single_tech"), seed=17))

    def positions_of(vcf_path):
        return [int(line.split("\t")[1]) for line in open(vcf_path) if line.strip() and not line.startswith("#")]

    def call(extra, workdir):
        run = subprocess.run([sys.executable, "-m", "hello_amd.call", "--ibam", bam, "--ref", fa, "--workdir", workdir,
                              "--network", model] + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stderr[-3000:]
        return positions_of(os.path.join(workdir, "results.output.vcf"))
    got = call(["--from_bam"], str(tmp_path / "w1"))
    # the same positions, sharded the same way, through the restatement
    hot = []
    for a, b in hs.get_chunks(len(reference), 500):
        hot += hr.find_hotspots([reads], reference, a, b)
    shard_dir = tmp_path / "ref_shards"
    shard_dir.mkdir()
    for n, part in enumerate(cd.shard_positions(hot)):
        sites = cr.candidate_sites(cr.find_candidates(reads, reference, part), "chr1")
        shards.write_shard(str(shard_dir / f"shard{n}.hshard"), sites)
    want = call(["--shards", str(shard_dir)], str(tmp_path / "w2"))
    assert got == want and len(got) > 0
