"""GPU candidate sites from one PacBio BAM (hello_candidates_find with HELLO_HOTSPOTS_PACBIO, hello_amd/csrc/candidates.hip)
against the Python restatement (tests/pacbio_reference.py): the same sites, alleles, supporting reads and clipped reads, exactly.
The inputs were chosen with the restatement on the CPU so that no searcher reaches the read cap (but in the one test about
it) and nothing is filtered on the test's side; the tests assert both."""
import os

import numpy as np
import pytest

from tests import candidate_reference as cr
from tests import hotspot_reference as hr
from tests import hotspot_synth as synth
from tests import pacbio_reference as pr
from tests.bam_writer import Read, write_bam
from tests.test_candidates import REF as HAND_REF, _match, _snv
from tests.test_gpu_candidates import _fasta, _same, _variants, _write
from tests.test_pacbio_candidates import flank200_cases, pacbio_hand_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_KEYS = [k for k in cr.STAT_KEYS]


def _both(tmp_path, reads, reference, positions, name="p.bam", capped=0):
    from hello_amd import pacbio as pb
    path = _write(tmp_path, name, "chr1", reference, reads)
    fa = _fasta(tmp_path, "chr1", reference)
    st, want_st = {}, {}
    sites = pr.find_candidates(reads, reference, positions, stats=want_st)
    assert want_st["regions_at_read_cap"] + want_st["clusters_at_read_cap"] == capped
    shard = pb.find_pacbio_candidates(path, fa, "chr1", positions, stats=st)
    assert st["regions_pass1"].reshape(-1, 2).tolist() == [list(r) for r in want_st["regions_pass1"]]
    assert st["regions_pass2"].reshape(-1, 2).tolist() == [list(r) for r in want_st["regions_pass2"]]
    assert {k: int(st[k]) for k in COUNT_KEYS} == {k: want_st[k] for k in COUNT_KEYS}
    _same(shard, sites)                                    # sites, alleles, reads per allele, clipped bases, quals, CIGARs, starts
    return shard, sites, st, path, fa


def synthetic(seed, length=60000):
    """A chromosome with long noisy reads of a donor and of the reference haplotype (several kb each)."""
    rng = np.random.default_rng(seed)
    reference = synth.random_reference(rng, length, masked_fraction=0.02)
    reads = synth.sample_reads(rng, reference, 25, 3000, snv_rate=0.004, indel_rate=0.002, pacbio=True, prefix="a")
    reads += synth.sample_reads(rng, reference, 20, 3000, snv_rate=0.0, indel_rate=0.0, pacbio=True, prefix="b")
    reads.sort(key=lambda r: r.pos)
    return reference, reads


def crowd():
    """130 reads over one SNV: pass 1 fetches 180 bases (cap 180.0, all kept); pass 2 fetches 30 (cap 100): the first 100 reads in
    file order -- 80 reference reads and 20 of the 50 that carry T."""
    return [_match(f"r{i}", 30, 540) for i in range(80)] + [_snv(f"t{i}", 30, 540, 300, "T") for i in range(50)]


def monster():
    """An 80 kb chromosome, 12 plain reads over an SNV at 40000 and one read of 68 001 CIGAR operations (the CG tag) through it."""
    rng = np.random.default_rng(77)
    reference = synth.random_reference(rng, 80000)
    site = 40000
    other = "ACGT"[("ACGT".index(reference[site]) + 1) % 4]

    def plain(name, alt):
        seq = reference[site - 1500:site + 1500]
        if alt:
            seq = seq[:1500] + other + seq[1501:]
        return Read(name, site - 1500, [(0, 3000)], seq, [30] * 3000)
    reads = [plain(f"r{i}", False) for i in range(6)] + [plain(f"t{i}", True) for i in range(6)]
    pos = site - 33100                                                 # the SNV is base 100 of the 1000M block
    cigar = [(0, 1), (1, 1)] * 33000 + [(0, 1000)] + [(2, 1), (0, 1)] * 1000
    seq, p = [], pos
    for op, n in cigar:
        if op == 0:
            seq.append(reference[p:p + n]); p += n
        elif op == 1:
            seq.append("A" * n)
        else:
            p += n
    seq = "".join(seq)
    seq = seq[:66000 + 100] + other + seq[66000 + 101:]               # it carries the SNV too
    reads.append(Read("monster", pos, cigar, seq, [30] * len(seq)))
    reads.sort(key=lambda r: r.pos)
    return reference, reads, site, other


def planted(length=160000, head=10000, edge=600, read_len=3000, step=200):
    """Error-free long reads of a donor and of the reference haplotype, 15 of each over every position.  The first `head` and the
    last `edge` bases carry no variant: the hotspot stage's first 10 kbp chunk is out of bounds in the reference too (its window
    starts at min(read starts, 0) - 10 < 0), so a variant there could not become a site."""
    rng = np.random.default_rng(141)
    reference = synth.random_reference(rng, length)
    mid, wmid = synth.donor(rng, reference[head:length - edge], 0.002, 0.0005)
    dseq = reference[:head] + mid + reference[length - edge:]
    where = list(range(head)) + [w + head if w >= 0 else -1 for w in wmid] + list(range(length - edge, length))

    def tile(seq, wh, prefix):
        out = []
        starts = list(range(0, len(seq) - read_len, step)) + [len(seq) - read_len]
        for i, s in enumerate(starts):
            pos, cigar = synth.cigar_of(wh[s:s + read_len])
            out.append(Read(f"{prefix}{i}", pos, cigar, seq[s:s + read_len], [30] * read_len))
        return out
    reads = sorted(tile(dseq, where, "d") + tile(reference, list(range(length)), "r"), key=lambda r: r.pos)
    variants = _variants(reference, dseq, where)
    qualifying = [(a, b) for i, (a, b) in enumerate(variants)
                  if not ((i > 0 and a - variants[i - 1][1] < 31) or (i + 1 < len(variants) and variants[i + 1][0] - b < 31))]
    return reference, reads, dseq, where, variants, qualifying


PLANTED, QUALIFYING = 398, 330          # counted on the CPU from the inputs of planted(); at least 200 must qualify


def test_hand_cases_on_the_gpu(tmp_path):
    for i, (name, reads, positions, expected) in enumerate(pacbio_hand_cases()):
        reads = sorted(reads, key=lambda r: r.pos)
        shard, sites, st, _, _ = _both(tmp_path, reads, HAND_REF, positions, name=f"h{i}.bam")
        got = [(int(shard.start[s]), int(shard.stop[s]), shard.names(s)) for s in range(shard.n_sites)]
        assert got == [(a, b, [t for t, _ in al]) for a, b, al in expected], name
        assert st["reads_clipped"] > 0 and st["clip_kernel_ms"] > 0


def test_clip_rules_at_flank_200_on_the_gpu(tmp_path):
    """One probe read per clip rule through hello_candidates_find: the reads it returns for the site have the hand-written start,
    CIGAR, bases and qualities (and those of pacbio_reference.clip_read)."""
    reads, want = flank200_cases()
    shard, sites, st, _, _ = _both(tmp_path, reads, HAND_REF, [300], name="f.bam")
    z = {k: np.asarray(v) for k, v in shard.z.items()}
    index = st["read_index"].tolist()
    assert sorted(reads[i].name for i in index) == sorted(want) and shard.n_sites == 1
    for k, i in enumerate(index):
        r = reads[i]
        start, cigar, front, behind = want[r.name]
        c = pr.clip_read(r, 285, 30)
        assert (c.pos, c.cigar) == (start, cigar), r.name
        lo, hi = int(z["read_off0"][k]), int(z["read_off0"][k + 1])
        words = z["cigars0"][int(z["cigar_off0"][k]):int(z["cigar_off0"][k + 1])]
        assert int(z["ref_start0"][k]) == start, r.name
        assert [(int(w) & 15, int(w) >> 4) for w in words] == cigar, r.name
        assert z["bases0"][lo:hi].tobytes().decode() == r.seq[front:len(r.seq) - behind] == c.seq, r.name
        assert z["quals0"][lo:hi].tolist() == r.qual[front:len(r.qual) - behind] == c.qual, r.name


@pytest.mark.parametrize("seed", [201, 202])
def test_synthetic_chromosomes_match_the_restatement_and_runs_are_identical(tmp_path, seed):
    from hello_amd import hotspots as hs, pacbio as pb
    reference, reads = synthetic(seed)
    assert np.median([len(r.seq) for r in reads]) > 2500
    want = hr.find_hotspots([reads], reference, 0, len(reference), pacbio=True)
    shard, sites, st, path, fa = _both(tmp_path, reads, reference, want)
    positions = hs.find_hotspots(path, fa, "chr1", 0, len(reference), pacbio=True)
    assert positions.tolist() == want
    assert len(sites) > 100 and any(len(s.alleles) > 1 for s in sites)
    assert any(r.cigar[0][0] == 4 or r.cigar[-1][0] == 4 for s in sites for r in s.reads)      # clips ending in an insertion
    again = pb.find_pacbio_candidates(path, fa, "chr1", want)
    for k in shard.z:
        assert np.asarray(shard.z[k]).tobytes() == np.asarray(again.z[k]).tobytes(), k


def test_the_read_cap_keeps_the_first_reads(tmp_path):
    shard, sites, st, _, _ = _both(tmp_path, crowd(), HAND_REF, [300], capped=1)
    assert (int(st["regions_at_read_cap"]), int(st["clusters_at_read_cap"])) == (0, 1)
    assert [(s.start, s.stop, [(a, len(i)) for a, i in s.alleles]) for s in sites] == [(300, 301, [("G", 80), ("T", 20)])]
    assert np.asarray(shard.z["reads_per_allele0"]).tolist() == [80, 20]


def test_a_read_of_more_than_65535_operations(tmp_path):
    reference, reads, site, other = monster()
    big = [r for r in reads if r.name == "monster"][0]
    assert len(big.cigar) > 65535
    shard, sites, st, _, _ = _both(tmp_path, reads, reference, [site])
    assert [(s.start, s.stop) for s in sites] == [(site, site + 1)]
    support = {a: [sites[0].reads[i].name for i in idx] for a, idx in sites[0].alleles}
    assert "monster" in support[other] and len(support[other]) == 7 and len(support[reference[site]]) == 6
    clipped = [r for r in sites[0].reads if r.name == "monster"][0]
    assert 100 < len(clipped.cigar) < 500 and len(clipped.seq) <= 30 + 402 and clipped.cigar[0] == (4, 1)     # a leading I became S


def test_featurizer_gives_the_same_pileups_from_the_shard_and_from_the_restatement(tmp_path):
    from hello_amd import candidates as cd, netspec as ns, shards, weights
    from hello_amd.engine import Engine
    from hello_amd.featurizer import featurize
    reference, reads = synthetic(211, 20000)
    positions = hr.find_hotspots([reads], reference, 0, len(reference), pacbio=True)
    shard, sites, _, _, _ = _both(tmp_path, reads, reference, positions)
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
    """Every planted variant at least 31 bp from its neighbours (its feature window lies inside the chromosome: none is planted
    within 600 bp of the chromosome's end or in its first 10 kbp) is one site holding the donor's allele and the reference allele."""
    reference, reads, dseq, where, variants, qualifying = planted()
    assert (len(variants), len(qualifying)) == (PLANTED, QUALIFYING)
    positions = hr.find_hotspots([reads], reference, 0, len(reference), pacbio=True)
    shard, sites, _, _, _ = _both(tmp_path, reads, reference, positions)
    donor_at = {w: i for i, w in enumerate(where) if w >= 0}
    for a, b in qualifying:
        hit = [s for s in range(shard.n_sites) if int(shard.start[s]) <= a and b <= int(shard.stop[s])]
        assert len(hit) == 1, (a, b)
        s0, s1 = int(shard.start[hit[0]]), int(shard.stop[hit[0]])
        assert (s0 + s1) // 2 - 75 >= 0 and (s0 + s1) // 2 + 75 <= len(reference)
        names = shard.names(hit[0])
        assert reference[s0:s1] in names, (a, b, names)
        assert dseq[donor_at[s0]:donor_at[s1]] in names, (a, b, names)


def test_from_bam_end_to_end_with_a_pacbio_bam(tmp_path):
    """python -m hello_amd.call --from_bam --pbam: the VCF's record positions are the restatement's sites that the same network
    (the canonical single-technology architecture) calls non-reference when scored from a write_shard of the restatement's
    sites; the files lie under the reference's directory names for a PacBio BAM."""
    import subprocess
    import sys
    from hello_amd import call, candidates as cd, hotspots as hs, loader, netspec as ns, shards, weights
    reference, reads = synthetic(231, 20000)
    bam = _write(tmp_path, "e.bam", "chr1", reference, reads)
    fa = _fasta(tmp_path, "chr1", reference)
    model = str(tmp_path / "model.hello.npz")
    loader.save_native(model, "single_tech", weights.synth_state(ns.build("single_tech"), seed=17))

    def positions_of(vcf_path):
        return [int(line.split("\t")[1]) for line in open(vcf_path) if line.strip() and not line.startswith("#")]

    def run(extra, workdir):
        done = subprocess.run([sys.executable, "-m", "hello_amd.call", "--pbam", bam, "--ref", fa, "--workdir", workdir,
                               "--network", model] + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0, done.stderr[-3000:]
        return positions_of(os.path.join(workdir, "results.output.vcf"))
    got = run(["--from_bam"], str(tmp_path / "w1"))
    assert os.path.isdir(os.path.join(str(tmp_path / "w1"), call.features_dir_name(None, bam)))
    assert os.path.isfile(os.path.join(str(tmp_path / "w1"), hs.get_workdir(None, bam, chrom="chr1", string="hotspots"), "hotspots.txt"))
    hot = []
    for a, b in hs.get_chunks(len(reference), 500):
        hot += hr.find_hotspots([reads], reference, a, b, pacbio=True)
    shard_dir = tmp_path / "ref_shards"
    shard_dir.mkdir()
    for n, part in enumerate(cd.shard_positions(hot)):
        sites = cr.candidate_sites(pr.find_candidates(reads, reference, part), "chr1")
        shards.write_shard(str(shard_dir / f"shard{n}.hshard"), sites)
    want = run(["--shards", str(shard_dir)], str(tmp_path / "w2"))
    assert got == want and len(got) > 0
