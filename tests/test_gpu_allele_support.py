"""Per-allele read support on the GPU (hello_engine_allele_support, hello_amd/csrc/support.hip) and ``--annotate`` end to end.

The kernel against NumPy, exactly, through host pointers and device pointers, at the read counts where one wave's stride over
an allele changes shape (1, 63, 64, 65, 129, 1000; a dummy read; one allele; many small alleles); its refusals; then
``python -m hello_amd.call --annotate`` on the smallest inputs of the --from_bam / --from_bams driver tests: the annotated lines
without their annotations are the bytes of a run without the flag, the annotations are what NumPy counts in the ``.hshard``
files' read arrays (put into lines by ``hello_amd.vcf.annotate``), and the resident route writes the same bytes."""
import ctypes
import glob
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_candidates import _fasta, _write
from tests.test_gpu_resident import HYBRID_SEED, _network, illumina_input
from tests.test_gpu_hybrid_candidates import synthetic as hybrid_synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [1, 1, 63, 64, 65, 129, 1000]          # the first allele's one read is a dummy: zero CIGAR operations


@pytest.fixture(scope="module")
def engine():
    from hello_amd import netspec as ns, weights
    from hello_amd.engine import Engine
    spec = ns.build("single_tech")
    eng = Engine(spec, weights.synth_state(spec, seed=5), device=0)
    yield eng
    eng.close()


def reads_of(counts, seed, dummies=()):
    """One technology's per-read arrays for alleles of ``counts`` reads; alleles in ``dummies`` hold one dummy read."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    R = int(off[-1])
    mapq = rng.choice(np.array([0, 1, 60, 255], np.uint8), size=R)
    orientation = rng.choice(np.array([-1, 1], np.int8), size=R)
    ops = rng.integers(1, 4, size=R)
    for a in dummies:
        assert counts[a] == 1
        ops[off[a]] = 0
    big = [a for a in range(len(counts)) if a not in dummies]
    mapq[off[big[-1]]:off[big[-1] + 1]] = 255                      # one allele all 255 (the largest sums), one all reverse
    orientation[off[big[0]]:off[big[0] + 1]] = -1
    return np.concatenate([[0], np.cumsum(ops)]).astype(np.int64), mapq, orientation, off


def numpy_support(cigar_off, mapq, orientation, off):
    real = np.diff(cigar_off) > 0
    out = np.zeros((off.shape[0] - 1, 4), np.int64)
    for a in range(out.shape[0]):
        at = slice(int(off[a]), int(off[a + 1]))
        q = mapq[at][real[at]].astype(np.int64)
        out[a] = (q.shape[0], int((orientation[at][real[at]] > 0).sum()), int(q.sum()), int((q * q).sum()))
    return out


CASES = {"the stride's edges": (COUNTS, (0,)), "reversed": (COUNTS[::-1], (len(COUNTS) - 1,)), "a lone allele": ([5], ()),
         "300 small alleles": (np.random.default_rng(9).integers(1, 4, size=300).tolist(), ())}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_numpy_through_host_and_device_pointers(engine, name):
    from hello_amd import featurizer as fz
    counts, dummies = CASES[name]
    if name == "300 small alleles":
        dummies = tuple(a for a in range(0, 300, 37) if counts[a] == 1)
    arrays = reads_of(counts, 17 + len(counts), dummies)
    want = numpy_support(*arrays)
    assert want[:, 0].sum() == sum(counts) - len(dummies) and all(want[a, 0] == 0 for a in dummies)
    assert (want[:, 3] == 255 * 255 * want[:, 0]).any() and ((want[:, 1] == 0) & (want[:, 0] > 0)).any()
    host = fz.allele_support(engine, *arrays)
    assert host.dtype == np.int64 and host.shape == want.shape and np.array_equal(host, want)
    dev = fz.allele_support(engine, *arrays, device=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    assert fz.allele_support(engine, *arrays).tobytes() == host.tobytes()                    # two runs, the same bytes


def test_refusals_and_the_empty_launch(engine):
    import torch
    lib = engine.lib
    cigar_off, mapq, orientation, off = reads_of([3, 4, 2], 1)
    out = np.full((3, 4), -7, np.int64)

    def run(offsets, n_reads, n_alleles):
        offsets = np.ascontiguousarray(offsets, np.int64)
        return lib.hello_engine_allele_support(engine.handle, cigar_off.ctypes.data, mapq.ctypes.data, orientation.ctypes.data,
                                               offsets.ctypes.data, n_reads, n_alleles, out.ctypes.data, 0, None)
    assert run([0, 5, 3, 9], 9, 3) == -2 and b"decreases" in lib.hello_last_error()
    assert run([0, 3, 7, 8], 9, 3) == -2 and b"ends at 8" in lib.hello_last_error()
    assert run([0, 3, 7, 10], 9, 3) == -2
    assert (out == -7).all()
    assert run(off, 9, 0) == 0 and (out == -7).all()                                          # nothing is launched
    dev_out = torch.full((3, 4), -7, dtype=torch.int64, device="cuda:0")
    dev = [torch.from_numpy(a).to("cuda:0") for a in (cigar_off, mapq, orientation, off)]
    assert lib.hello_engine_allele_support(engine.handle, *[t.data_ptr() for t in dev], 9, 0, dev_out.data_ptr(), 3, None) == 0
    torch.cuda.synchronize()
    assert bool((dev_out == -7).all())
    assert run(off, 9, 3) == 0 and np.array_equal(out, numpy_support(cigar_off, mapq, orientation, off))


# ---- end to end -------------------------------------------------------------------------------------------------------
def _call(argv, workdir):
    done = subprocess.run([sys.executable, "-m", "hello_amd.call"] + argv + ["--workdir", workdir], cwd=ROOT, capture_output=True,
                          text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-3000:]
    return open(os.path.join(workdir, "results.output.vcf")).read()


def _split(text):
    lines = text.splitlines(keepends=True)
    return [line for line in lines if line.startswith("#")], [line for line in lines if not line.startswith("#")]


def _expected_lines(workdir, fasta, techs):
    """The final VCF's record lines from NumPy counts over the shard files' read arrays: per shard, the mean call of every
    ``.features`` entry (as the run without the flag makes it) annotated with the support of its site's alleles."""
    from hello_amd import call, shards, vcf
    genome = call.read_fasta(fasta)
    lines = []
    paths = sorted(glob.glob(os.path.join(workdir, "shards", "*.hshard")), key=call.natural_key)
    assert paths
    for path in paths:
        sh = shards.PackedShard.from_file(path)
        support = []
        for t in techs:
            counts = np.asarray(sh.z[f"reads_per_allele{t}"], np.int64)
            off = np.concatenate([[0], np.cumsum(counts)])
            mapq, forward = np.asarray(sh.z[f"mapq{t}"], np.int64), np.asarray(sh.z[f"orientation{t}"]) > 0
            support.append(np.array([(off[a + 1] - off[a], forward[off[a]:off[a + 1]].sum(), mapq[off[a]:off[a + 1]].sum(),
                                      (mapq[off[a]:off[a + 1]] ** 2).sum()) for a in range(counts.shape[0])], np.int64).reshape(-1, 4))
        site_at = {(sh.chromosome_names[int(sh.chromosome_of_site[s])], int(sh.start[s])): s for s in range(sh.n_sites)}
        assert len(site_at) == sh.n_sites
        features = glob.glob(os.path.join(workdir, "features*", "features%d.features" % call.shard_number(path, 0)))
        assert len(features) == 1
        for entry in pickle.load(open(features[0], "rb")):
            mean = vcf.call_site(vcf.mean_posteriors(entry["expertPredictions"], entry["meta"]), entry["chromosome"], entry["position"],
                                 entry["length"], genome[entry["chromosome"]])
            if mean is None:
                continue
            s = site_at[(entry["chromosome"], entry["position"])]
            lo, hi = int(sh.allele_off[s]), int(sh.allele_off[s + 1])
            rows = [t[lo:hi] for t in support] + [None]
            lines.append((mean.position, len(lines), vcf.annotate(mean, sh.names(s), rows[0], rows[1]) + "\n"))
    return [line for _, _, line in sorted(lines)]


def _shard_files(workdir):
    return {os.path.basename(p): open(p, "rb").read() for p in glob.glob(os.path.join(workdir, "features*", "features*"))
            if not p.endswith(".log")}


@pytest.fixture(scope="module")
def illumina_run(tmp_path_factory):
    """The smallest --from_bam input of the driver tests, written once, and its ``--from_bam --annotate`` run."""
    tmp_path = tmp_path_factory.mktemp("annotate")
    network, model = _network(tmp_path, False)
    network.close()
    reference, reads = illumina_input()
    bam, fa = _write(tmp_path, "i.bam", "chr1", reference, reads), _fasta(tmp_path, "chr1", reference)
    base = ["--ibam", bam, "--ref", fa, "--network", model, "--from_bam"]
    workdir = str(tmp_path / "annotated")
    return dict(base=base, fa=fa, workdir=workdir, vcf=_call(base + ["--annotate"], workdir), files=_shard_files(workdir))


def test_from_bam_annotate_end_to_end(illumina_run, tmp_path):
    from hello_amd import vcf
    plain = _call(illumina_run["base"], str(tmp_path / "w0"))
    head0, body0 = _split(plain)
    head1, body1 = _split(illumina_run["vcf"])
    assert len(body0) > 0 and [vcf.strip_annotations(line) for line in body1] == body0
    assert all(line.split("\t")[8] == vcf.ANNOTATED_FORMAT for line in body1)
    assert [line for line in head1 if line not in vcf.ANNOTATION_HEADER.splitlines(keepends=True)] == head0
    assert "".join(line for line in head1 if line not in head0) == vcf.ANNOTATION_HEADER
    assert body1 == _expected_lines(illumina_run["workdir"], illumina_run["fa"], (0,))
    depths = [int(line.split("\t")[9].split(":")[2]) for line in body1]
    assert max(depths) > 10                                                        # real reads were counted
    files0, files1 = _shard_files(str(tmp_path / "w0")), illumina_run["files"]
    assert sorted(files0) == sorted(files1)
    for name in files0:                                                            # .features unchanged, .vcf lines stripped equal
        if name.endswith(".features"):
            assert files1[name] == files0[name], name
        else:
            assert "".join(vcf.strip_annotations(line) for line in files1[name].decode().splitlines(keepends=True)) == files0[name].decode(), name


def test_resident_annotate_writes_the_bytes_of_the_shard_route(illumina_run, tmp_path):
    resident = _call(illumina_run["base"] + ["--annotate", "--resident"], str(tmp_path / "w2"))
    assert resident == illumina_run["vcf"] and any(not line.startswith("#") for line in resident.splitlines())
    assert _shard_files(str(tmp_path / "w2")) == illumina_run["files"]
    assert not os.path.exists(str(tmp_path / "w2" / "shards"))


def test_from_bams_annotate_sums_both_technologies(tmp_path):
    network, model = _network(tmp_path, True)
    network.close()
    reference, illumina, pacbio = hybrid_synthetic(HYBRID_SEED, 20000)
    bams = [_write(tmp_path, "i.bam", "chr1", reference, illumina), _write(tmp_path, "p.bam", "chr1", reference, pacbio)]
    fa = _fasta(tmp_path, "chr1", reference)
    annotated = _call(["--ibam", bams[0], "--pbam", bams[1], "--ref", fa, "--network", model, "--from_bams", "--annotate"], str(tmp_path / "w"))
    _, body = _split(annotated)
    want = _expected_lines(str(tmp_path / "w"), fa, (0, 1))
    assert len(body) > 0 and body == want
    one = _expected_lines(str(tmp_path / "w"), fa, (0,))
    assert one != want                                                             # the second technology's reads are in the sums
