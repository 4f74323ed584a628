"""Resident candidate sites on the GPU (HELLO_CANDIDATES_RESIDENT, hello_candidates_gather, hello_amd/resident.py): what the gather
kernel writes equals, byte for byte, what the host path (a non-resident call -> ``PackedShard.featurizer_core`` ->
``ShardScorer._fill``) builds from the same BAMs; scores and the files of ``python -m hello_amd.call --resident`` equal those of
the route through shard files.  The yardstick is the non-resident path, which the candidate, PacBio and hybrid suites hold to
the Python restatements.  Seeds were chosen with the restatements on the CPU so that the conditions asserted below hold."""
import glob
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import hotspot_synth as synth
from tests.bam_writer import Read
from tests.test_gpu_candidates import _fasta, _write
from tests.test_gpu_hybrid_candidates import synthetic as hybrid_synthetic
from tests.test_gpu_pacbio_candidates import synthetic as pacbio_synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
HYBRID_SEED = 304
DTYPES = dict(bases=np.uint8, quals=np.uint8, read_off=np.int64, cigars=np.uint32, cigar_off=np.int64, ref_start=np.int64,
              mapq=np.uint8, orientation=np.int8, hp=np.uint8, site_of_read=np.int32)
SITE_ARRAYS = ("start", "stop", "window_start", "ref", "ref_off", "alleles_per_site", "allele_text", "allele_text_off",
               "chromosome_text", "chromosome_text_off", "chromosome_of_site")


# ---- inputs -----------------------------------------------------------------------------------------------------------
def illumina_input():
    """The reads of test_featurizer_gives_the_same_pileups_from_the_shard_and_from_the_restatement (20 kb)."""
    rng = np.random.default_rng(111)
    reference = synth.random_reference(rng, 20000)
    reads = synth.sample_reads(rng, reference, 20, 150, snv_rate=0.004, indel_rate=0.002, prefix="a")
    reads += synth.sample_reads(rng, reference, 15, 150, snv_rate=0.0, indel_rate=0.0, prefix="b")
    reads.sort(key=lambda r: r.pos)
    return reference, reads


class Case:
    """One input written to disk, with the functions that build its candidates plainly and resident."""

    def __init__(self, kind, directory):
        from hello_amd import candidates as cd, hotspots as hs, hybrid, pacbio as pb
        self.kind, self.techs = kind, (0, 1) if kind == "hybrid" else (0,)
        if kind == "hybrid":
            reference, illumina, pacbio = hybrid_synthetic(HYBRID_SEED, 20000)
            self.bam = [_write(directory, "i.bam", "chr1", reference, illumina), _write(directory, "p.bam", "chr1", reference, pacbio)]
            self._find = hybrid.find_hybrid_candidates
        elif kind == "pacbio":
            reference, reads = pacbio_synthetic(211, 20000)          # the smallest PacBio input of its suite
            self.bam = _write(directory, "p.bam", "chr1", reference, reads)
            self._find = pb.find_pacbio_candidates
        else:
            reference, reads = illumina_input()
            self.bam = _write(directory, "i.bam", "chr1", reference, reads)
            self._find = cd.find_candidates
        self.reference = reference
        self.fa = _fasta(directory, "chr1", reference)
        self.positions = hs.find_hotspots(self.bam, self.fa, "chr1", 0, len(reference), pacbio=kind == "pacbio").tolist()
        self.plain_stats: dict = {}
        self.plain = self.find(self.positions, False, self.plain_stats)

    def find(self, positions, resident, stats=None):
        return self._find(self.bam, self.fa, "chr1", positions, stats=stats, resident=resident)


_cases: dict = {}


@pytest.fixture
def case(request, tmp_path_factory):
    kind = request.param if hasattr(request, "param") else "illumina"
    if kind not in _cases:
        _cases[kind] = Case(kind, tmp_path_factory.mktemp(kind))
    return _cases[kind]


# ---- helpers ----------------------------------------------------------------------------------------------------------
def gather(shard, tech, stream=None):
    """One gather with zero shifts into device arrays surrounded by guard bytes -> the arrays on the host."""
    import torch
    n_reads, n_bases, n_cigars = shard.featurizer_counts(tech)
    counts = dict(bases=n_bases, quals=n_bases, read_off=n_reads + 1, cigars=n_cigars, cigar_off=n_reads + 1, ref_start=n_reads,
                  mapq=n_reads, orientation=n_reads, hp=n_reads, site_of_read=n_reads)
    buffers = {k: torch.full((2 * GUARD + counts[k] * np.dtype(DTYPES[k]).itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
               for k in counts}
    torch.cuda.synchronize()
    shard.gather(tech, {k: b.data_ptr() + GUARD for k, b in buffers.items()})
    torch.cuda.synchronize()
    out = {}
    for k, b in buffers.items():
        host = b.cpu().numpy()
        assert (host[:GUARD] == 0xA5).all() and (host[host.shape[0] - GUARD:] == 0xA5).all(), f"guard bytes of {k}"
        out[k] = host[GUARD:host.shape[0] - GUARD].view(DTYPES[k]).copy()
    return out


def same_as_core(got, plain, tech):
    core = plain.featurizer_core(tech)
    for k in DTYPES:
        want = np.asarray(core[k]).astype(DTYPES[k], copy=False)
        assert got[k].shape == want.shape and got[k].tobytes() == want.tobytes(), (tech, k)


def same_host_side(case, plain, plain_stats, resident, stats):
    for k in SITE_ARRAYS:
        assert np.asarray(getattr(resident, k)).tobytes() == np.asarray(getattr(plain, k)).tobytes(), k
    for t in case.techs:
        assert resident.counts[t].tolist() == np.asarray(plain.z[f"reads_per_allele{t}"]).tolist()
        assert resident.reads_per_allele(t).tobytes() == plain.featurizer_core(t)["reads_per_allele"].tobytes()
        assert resident.n_reads(t) == plain.n_reads(t)
        assert stats[f"read_off{t}"].tobytes() == np.asarray(plain.z[f"read_off{t}"], np.int64).tobytes()
        assert stats[f"cigar_off{t}"].tobytes() == np.asarray(plain.z[f"cigar_off{t}"], np.int64).tobytes()
    arrays = [k for k, v in plain_stats.items() if isinstance(v, np.ndarray)]
    assert sorted(arrays) == sorted(["regions_pass1", "regions_pass2"] + (["read_index0", "read_index1"] if len(case.techs) == 2 else ["read_index"]))
    for k in arrays:
        assert stats[k].tobytes() == plain_stats[k].tobytes(), k
    # every statistic that is not a time; the host gather's time is 0 when nothing is gathered on the host
    numbers = [k for k, v in plain_stats.items() if not isinstance(v, np.ndarray)]
    assert len(numbers) == (29 if len(case.techs) == 2 else 22)
    for k in numbers:
        if not k.endswith("_ms"):
            assert stats[k] == plain_stats[k], k
    assert stats["gather_ms"] == 0 and plain_stats["gather_ms"] > 0


def reads_under_two_sites(shard, read_index, tech):
    """Input reads gathered under alleles of at least two different sites."""
    counts = np.asarray(shard.z[f"reads_per_allele{tech}"], np.int64)
    site_of_allele = np.repeat(np.arange(shard.n_sites), shard.alleles_per_site)
    pairs = {(int(r), int(s)) for r, s in zip(read_index, np.repeat(site_of_allele, counts))}
    reads = [r for r, _ in pairs]
    return sum(1 for r in set(reads) if reads.count(r) > 1)


# ---- 1. the gather equals the host path -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["illumina", "pacbio", "hybrid"], indirect=True)
def test_gather_equals_the_host_path(case):
    plain, plain_stats = case.plain, case.plain_stats
    assert plain.n_sites > 20
    if case.kind == "hybrid":
        for t in (0, 1):                                          # dummy reads in both technologies
            assert (np.asarray(plain.z[f"reads_per_allele{t}"]) == 0).any(), t
    else:
        assert reads_under_two_sites(plain, plain_stats["read_index"], 0) > 0     # such a read crosses to the host twice today
    stats: dict = {}
    with case.find(case.positions, True, stats) as resident:
        same_host_side(case, plain, plain_stats, resident, stats)
        for t in case.techs:
            same_as_core(gather(resident, t), plain, t)
        assert resident.handle is not None
    assert resident.handle is None


# ---- 2. edge shapes -----------------------------------------------------------------------------------------------------
def edge_input():
    """A 3 kb reference; SNVs at 600, 1200, 1800 and 2400 and a 3-base insertion behind 1500, each carried by six 150-base
    reads among eight reads of the reference.  Around the SNVs: supporting reads of 5, 63, 64, 65 and 257 bases, one with a
    leading soft clip (2 operations), one written with =/X runs (65 operations), reverse-strand and HP-tagged reads."""
    rng = np.random.default_rng(7)
    ref = synth.random_reference(rng, 3000)
    other = lambda b: "ACGT"[("ACGT".index(b) + 1) % 4]      # noqa: E731

    def read(name, pos, n, snvs=(), flag=0, tags=b"", clip=0):
        seq = list(ref[pos:pos + n])
        for p in snvs:
            seq[p - pos] = other(ref[p])
        cigar = [(0, n)] if not clip else [(4, clip), (0, n - clip)]
        return Read(name, pos + clip, cigar, "".join(seq), [30] * n, flag, 60, tags=tags)

    def eqx(name, pos, n, mismatches):
        seq = list(ref[pos:pos + n])
        for p in mismatches:
            seq[p - pos] = other(ref[p])
        cigar = []
        for i in range(n):
            op = 8 if pos + i in mismatches else 7
            cigar = cigar[:-1] + [(op, cigar[-1][1] + 1)] if cigar and cigar[-1][0] == op else cigar + [(op, 1)]
        return Read(name, pos, cigar, "".join(seq), [30] * n)
    reads = []
    for k, p in enumerate((600, 1200, 1800, 2400)):
        reads += [read(f"r{k}_{i}", p - 70 - i, 150) for i in range(8)]
        reads += [read(f"t{k}_{i}", p - 80 + i, 150, [p], flag=16 if i % 2 else 0, tags=b"HPC\x01" if i < 2 else b"") for i in range(6)]
    reads += [read("len5", 598, 5, [600], tags=b"HPC\x02"), read("len63", 570, 63, [600], flag=16), read("len64", 1170, 64, [1200]),
              read("len65", 1770, 65, [1800]), read("len257", 2300, 257, [2400], flag=16, tags=b"HPC\x02"),
              read("clip", 1140, 150, [1200], clip=3)]
    reads.append(eqx("eqx", 1800 - 62, 150, {1800 - 62 + 2 + 4 * j for j in range(32)}))           # 33 = runs, 32 X runs; 1800 is one
    ins = "".join(other(b) for b in ref[1501:1504])
    reads += [read(f"ri{i}", 1430 - i, 150) for i in range(8)]
    for i in range(6):
        pos = 1420 + i
        seq = ref[pos:1501] + ins + ref[1501:pos + 147]
        reads.append(Read(f"i{i}", pos, [(0, 1501 - pos), (1, 3), (0, pos + 147 - 1501)], seq, [30] * 150))
    reads.sort(key=lambda r: r.pos)
    return ref, reads, [600, 1200, 1500, 1800, 2400]


def test_edge_shapes_and_guard_bytes(tmp_path):
    from hello_amd import candidates as cd
    reference, reads, positions = edge_input()
    bam, fa = _write(tmp_path, "e.bam", "chr1", reference, reads), _fasta(tmp_path, "chr1", reference)
    plain_stats, stats = {}, {}
    plain = cd.find_candidates(bam, fa, "chr1", positions, stats=plain_stats)
    assert plain.n_sites == 5
    core = plain.featurizer_core(0)
    lengths, operations = set(np.diff(core["read_off"]).tolist()), set(np.diff(core["cigar_off"]).tolist())
    assert {5, 63, 64, 65, 150, 257} <= lengths, sorted(lengths)
    assert {1, 2, 3, 65} <= operations, sorted(operations)
    assert {-1, 1} <= set(core["orientation"].tolist()) and {0, 1, 2} <= set(core["hp"].tolist())
    with cd.find_candidates(bam, fa, "chr1", positions, stats=stats, resident=True) as resident:
        got = gather(resident, 0)                                 # asserts the 64 guard bytes around every array
    same_as_core(got, plain, 0)
    for k in ("read_index", "regions_pass1", "regions_pass2"):
        assert stats[k].tobytes() == plain_stats[k].tobytes(), k


# ---- 3. coalescing shifts ---------------------------------------------------------------------------------------------
def _halves(case):
    """The Illumina positions cut where two neighbours lie furthest apart near the middle: two adjacent shard files."""
    pos = case.positions
    lo, hi = len(pos) // 3, 2 * len(pos) // 3
    cut = lo + int(np.argmax(np.diff(pos[lo:hi]))) + 1
    assert pos[cut] - pos[cut - 1] >= 25                          # shardHotspots' separation
    return pos[:cut], pos[cut:]


def test_consecutive_gathers_build_the_block_of_fill(case):
    import torch
    from hello_amd import shard_pipeline as sp
    parts_of = [case.find(p, False) for p in _halves(case)]
    assert all(sh.n_sites > 5 for sh in parts_of)
    scorer = object.__new__(sp.ShardScorer)                       # the layout and fill code, without a model
    scorer.hybrid, scorer.uses_ref, scorer.L, scorer.compute = False, False, 150, torch.cuda.Stream()
    parts, nbytes, reads, S = scorer._layout(parts_of)
    want = np.zeros(nbytes, np.uint8)
    scorer._fill(parts_of, parts, want, (0,))
    resident = [case.find(p, True) for p in _halves(case)]
    try:
        assert scorer._layout(resident) == (parts, nbytes, reads, S)
        dev = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(scorer.compute):
            scorer._gather(resident, parts, dev, (0,))
        torch.cuda.synchronize()
        got = dev.cpu().numpy()
    finally:
        for sh in resident:
            sh.close()
    for (name, t), (at, dtype, count) in parts.items():
        if t == 0:                                                # every per-read part, its padding element included
            n = count * dtype.itemsize
            assert got[at:at + n].tobytes() == want[at:at + n].tobytes(), name
            assert (got[at + n:at + ((n + 15) & ~15)] == 0xA5).all(), name      # the alignment gap behind it is not written
        else:
            assert (got[at:at + count * dtype.itemsize] == 0xA5).all(), name    # the site arrays are not the gather's


# ---- 4. pileups and scores --------------------------------------------------------------------------------------------
def _network(tmp_path, hybrid):
    from hello_amd import loader, netspec as ns, weights
    from tests.util import load_fixture
    model = str(tmp_path / "model.hello.npz")
    if hybrid:
        spec, state, _, _ = load_fixture("hybrid_full")
        loader.save_native(model, "hybrid_full", state)
    else:
        loader.save_native(model, "single_tech", weights.synth_state(ns.build("single_tech"), seed=17))
    network = loader.load(model, device=0)
    network.eval()
    network.providePredictions = True
    return network, model


@pytest.mark.parametrize("case", ["illumina", "hybrid"], indirect=True)
def test_scores_of_resident_shards_equal_those_of_file_shards(case, tmp_path):
    from hello_amd import shard_pipeline as sp
    network, _ = _network(tmp_path, case.kind == "hybrid")
    try:
        scorer = sp.ShardScorer(network)
        halves = _halves(case)
        plain = [sp.prepare(case.find(p, False), scorer.hybrid, scorer.uses_ref) for p in halves]
        want = (scorer.submit(plain, ["a", "b"]) + scorer.flush())[-1]
        resident = [sp.prepare(case.find(p, True), scorer.hybrid, scorer.uses_ref) for p in halves]
        with pytest.raises(ValueError, match="not both"):
            scorer.submit([plain[0], resident[1]])
        assert scorer.submit(resident, ["a", "b"]) == [] and all(sh.handle is not None for sh in resident)
        slot = [s for s in scorer.slots if s.pending is not None][0]
        got = scorer.flush()[-1]
        assert all(sh.handle is None for sh in resident)          # released once the launch is done
        n = resident[0].n_reads(0) + resident[1].n_reads(0)
        assert bool(slot.pile[0][:n * 150 * scorer.channels[0]].any())
        assert got.posteriors.shape == want.posteriors.shape and got.posteriors.shape[1] > 0
        assert got.posteriors.tobytes() == want.posteriors.tobytes()
        assert (got.meta is None) == (want.meta is None) and (got.meta is None or got.meta.tobytes() == want.meta.tobytes())
        assert got.tags == ["a", "b"] and [sh.n_sites for sh in got.shards] == [sh.n_sites for sh in plain]
    finally:
        network.close()


# ---- 5. end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["illumina", "hybrid"], indirect=True)
def test_call_resident_writes_the_files_of_the_shard_route_and_no_shard(case, tmp_path):
    from hello_amd import call
    network, model = _network(tmp_path, case.kind == "hybrid")
    network.close()
    hybrid = case.kind == "hybrid"
    bams = ["--ibam", case.bam[0], "--pbam", case.bam[1]] if hybrid else ["--ibam", case.bam]
    route = "--from_bams" if hybrid else "--from_bam"

    def run(extra, workdir):
        done = subprocess.run([sys.executable, "-m", "hello_amd.call"] + bams + ["--ref", case.fa, "--workdir", workdir, "--network", model,
                               route] + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0, done.stderr[-3000:]
        return os.path.join(workdir, call.features_dir_name(case.bam[0] if hybrid else case.bam, case.bam[1] if hybrid else None))
    want_dir, got_dir = run([], str(tmp_path / "w1")), run(["--resident"], str(tmp_path / "w2"))
    read = lambda path: open(path, "rb").read()      # noqa: E731
    assert read(str(tmp_path / "w2" / "results.output.vcf")) == read(str(tmp_path / "w1" / "results.output.vcf"))
    assert any(not line.startswith(b"#") for line in read(str(tmp_path / "w2" / "results.output.vcf")).splitlines())
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(want_dir, "features*.vcf")) if not p.endswith(".mean.vcf"))
    assert names and names == sorted(os.path.basename(p) for p in glob.glob(os.path.join(got_dir, "features*.vcf"))
                                     if not p.endswith(".mean.vcf"))
    for name in names:
        assert read(os.path.join(got_dir, name)) == read(os.path.join(want_dir, name)), name
        stem = name[:-len(".vcf")]
        with open(os.path.join(got_dir, stem + ".features"), "rb") as a, open(os.path.join(want_dir, stem + ".features"), "rb") as b:
            got, want = pickle.load(a), pickle.load(b)
        assert len(got) == len(want) and pickle.dumps(got) == pickle.dumps(want), name
        assert "Completed running the script" in open(os.path.join(got_dir, stem + ".log")).read(), name
    assert glob.glob(str(tmp_path / "w1" / "**" / "*.hshard"), recursive=True)
    assert not glob.glob(str(tmp_path / "w2" / "**" / "*.hshard"), recursive=True)
    assert not os.path.exists(str(tmp_path / "w2" / "shards"))


# ---- 6. two runs ------------------------------------------------------------------------------------------------------
def test_two_resident_runs_gather_the_same_bytes(case):
    runs = []
    for _ in range(2):
        with case.find(case.positions, True) as resident:
            runs.append(gather(resident, 0))
    for k in DTYPES:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
