"""Per-allele base-level read evidence on the GPU (hello_engine_allele_evidence, hello_amd/csrc/evidence.hip) and
``--annotate_evidence`` end to end.

The kernel against a table of six integers per read written out by hand (every rule of the CIGAR walk by name); against a plain
Python loop on random small inputs, exactly, through host pointers and device pointers, at the allele sizes where one wave's
stride changes shape and the allele counts around the four-wave workgroup; its refusals; then ``python -m hello_amd.call
--annotate_evidence`` on the smallest inputs of the --from_bam / --from_bams driver tests: without the evidence the lines are the
bytes of an ``--annotate`` run, the evidence is what the Python loop counts in the ``.hshard`` files' read arrays (put into lines
by ``hello_amd.vcf.annotate_evidence``), and the resident route writes the same bytes."""
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
M, I, D, N, S, H, P, EQ, X = range(9)


@pytest.fixture(scope="module")
def engine():
    from hello_amd import netspec as ns, weights
    from hello_amd.engine import Engine
    spec = ns.build("single_tech")
    eng = Engine(spec, weights.synth_state(spec, seed=5), device=0)
    yield eng
    eng.close()


# ---- the plain Python loop ---------------------------------------------------------------------------------------------
def walk(quals, cigar, ref_start, s, e):
    """One read against the span [s, e) -> None when the guard stops it, else the read indices of its belonging bases."""
    n, p, i, mine = len(quals), int(ref_start), 0, []
    for op, length in cigar:
        if op in (M, EQ, X, D, N) and p >= e:
            break
        if op in (M, EQ, X, I, S):
            if i + length > n:
                return None
            if op in (M, EQ, X):
                mine += [i + j for j in range(length) if s <= p + j < e]
                p += length
            elif op == I and s <= p <= e:
                mine += list(range(i, i + length))
            i += length
        elif op in (D, N):
            p += length
    return mine


def python_evidence(a, allele_off, n_sites=None):
    n_sites = len(a["asm_start"]) if n_sites is None else n_sites
    out = np.zeros((len(allele_off) - 1, 6), np.int64)
    for allele in range(out.shape[0]):
        for r in range(int(allele_off[allele]), int(allele_off[allele + 1])):
            words = a["cigars"][int(a["cigar_off"][r]):int(a["cigar_off"][r + 1])]
            if len(words) == 0:
                continue
            quals = [int(q) for q in a["quals"][int(a["read_off"][r]):int(a["read_off"][r + 1])]]
            site = int(a["site_of_read"][r])
            mine = None
            if 0 <= site < n_sites:
                mine = walk(quals, [(int(w) & 15, int(w) >> 4) for w in words], a["ref_start"][r], int(a["asm_start"][site]),
                            int(a["asm_stop"][site]))
            if mine is None:
                out[allele, 5] += 1
                continue
            out[allele, 3] += int(a["hp"][r]) == 1
            out[allele, 4] += int(a["hp"][r]) == 2
            if mine:
                out[allele, 0] += 1
                out[allele, 1] += min(quals[i] for i in mine)
                out[allele, 2] += min(mine[0], len(quals) - 1 - mine[-1])
    return out


# ---- the literal table -------------------------------------------------------------------------------------------------
# (what the read shows, site, ref_start, CIGAR, qualities, hp) -> the six integers of an allele that holds this read alone
TABLE = [
    ("the span lies wholly before the read", 0, 103, [(M, 5)], [30] * 5, 1, (0, 0, 0, 1, 0, 0)),
    ("the span lies wholly behind the read", 0, 90, [(M, 10)], [30] * 10, 2, (0, 0, 0, 0, 1, 0)),
    ("the span starts on the read's first base", 0, 100, [(M, 6)], [11, 12, 13, 4, 4, 4], 0, (1, 11, 0, 0, 0, 0)),
    ("the span ends on the read's last base", 0, 95, [(M, 8)], [4, 4, 4, 4, 4, 25, 9, 26], 0, (1, 9, 0, 0, 0, 0)),
    ("a leading soft clip shifts i", 0, 98, [(S, 3), (M, 7)], [1, 2, 3, 40, 40, 20, 21, 22, 40, 40], 0, (1, 20, 2, 0, 0, 0)),
    ("hard clips", 0, 97, [(H, 2), (M, 8), (H, 1)], [5, 5, 5, 33, 34, 35, 5, 5], 1, (1, 33, 2, 1, 0, 0)),
    ("an N before the span", 0, 80, [(M, 5), (N, 13), (M, 6)], [2] * 7 + [15, 16, 17] + [2], 0, (1, 15, 1, 0, 0, 0)),
    ("= and X operations", 0, 99, [(EQ, 1), (X, 1), (EQ, 2), (X, 2)], [5, 31, 28, 29, 4, 4], 0, (1, 28, 1, 0, 0, 0)),
    ("a deletion covers the whole span", 0, 95, [(M, 5), (D, 3), (M, 5)], [9] * 10, 2, (0, 0, 0, 0, 1, 0)),
    ("an insertion at p = s", 0, 96, [(M, 4), (I, 2), (M, 4)], [3, 3, 3, 3, 18, 19, 30, 31, 32, 3], 0, (1, 18, 1, 0, 0, 0)),
    ("an insertion at p = e", 0, 101, [(S, 2), (M, 2), (I, 3), (M, 2)], [1, 1, 30, 31, 7, 8, 9, 2, 2], 0, (1, 7, 2, 0, 0, 0)),
    ("an insertion at p = s - 1", 0, 97, [(M, 2), (I, 2), (M, 3)], [40, 40, 3, 3, 40, 22, 23], 0, (1, 22, 0, 0, 0, 0)),
    ("an insertion at p = e + 1", 0, 102, [(M, 2), (I, 2), (M, 1)], [27, 40, 2, 2, 40], 0, (1, 27, 0, 0, 0, 0)),
    ("an insertion at the empty span's position", 1, 195, [(M, 5), (I, 2), (M, 5)], [40] * 5 + [12, 14] + [40] * 5, 0, (1, 12, 5, 0, 0, 0)),
    ("aligned bases over the empty span", 1, 195, [(M, 10)], [40] * 10, 1, (0, 0, 0, 1, 0, 0)),
    ("a padding and an unknown operation change nothing", 0, 99, [(P, 4), (M, 2), (9, 7), (M, 3)], [6, 24, 25, 26, 6], 2, (1, 24, 1, 0, 1, 0)),
    ("a CIGAR consumes more bases than the read has", 0, 99, [(M, 3), (M, 4)], [1, 1, 1, 1, 1], 1, (0, 0, 0, 0, 0, 1)),
]
# one allele that holds several of the reads above: (soft clip) + (hard clips) + (insertion at s) + (deletion) + (overrun)
TOGETHER = ([4, 5, 9, 8, 16], (3, 20 + 33 + 18, 2 + 2 + 1, 1, 1, 1))


def table_arrays():
    from hello_amd import featurizer as fz
    read = lambda row: fz.AlignedRead("A" * len(row[4]), row[4], row[3], row[2], hp=row[5])       # noqa: E731
    sites = [fz.SiteReads("A" * 400, 0, 100, 103, []), fz.SiteReads("A" * 400, 0, 200, 200, [])]
    want = []
    for row in TABLE:
        sites[row[1]].alleles.append((row[0], [read(row)]))
    sites[0].alleles.append(("an allele without reads: the dummy row", []))
    sites[0].alleles.append(("several reads", [read(TABLE[k]) for k in TOGETHER[0]]))
    for site in (0, 1):                                                   # pack_sites orders the alleles site by site
        want += [row[6] for row in TABLE if row[1] == site]
        if site == 0:
            want += [(0, 0, 0, 0, 0, 0), TOGETHER[1]]
    arrays = fz.pack_sites(sites)
    names = [name for site in sites for name, _ in site.alleles]
    return arrays, fz.allele_offsets(arrays["reads_per_allele"]), np.array(want, np.int64), names


def test_kernel_equals_the_table_written_by_hand(engine):
    from hello_amd import featurizer as fz
    arrays, off, want, names = table_arrays()
    assert len(names) == len(TABLE) + 2 == want.shape[0]
    got = fz.allele_evidence(engine, arrays, off)
    assert got.dtype == np.int64 and got.shape == want.shape
    for a, name in enumerate(names):
        assert tuple(got[a]) == tuple(want[a]), name
    assert np.array_equal(fz.allele_evidence(engine, arrays, off, device=True).cpu().numpy(), want)
    assert np.array_equal(python_evidence(arrays, off), want)             # the loop the other tests lean on reads the table alike


# ---- random inputs against the loop ------------------------------------------------------------------------------------
def random_arrays(counts, dummies, seed):
    """The evidence kernel's arrays for alleles of ``counts`` reads (those in ``dummies``: one dummy read): reads scattered
    around spans of 0 - 4 bases, CIGARs of 1 - 6 operations of every kind, about one read in twelve with a CIGAR that overruns
    its bases."""
    rng = np.random.default_rng(seed)
    n_sites = 3
    asm_start = np.array([1000, 1200, 1400], np.int64)
    asm_stop = asm_start + np.array([3, 0, 4])
    quals, cigars, read_off, cigar_off, ref_start, hp, site_of_read = [], [], [0], [0], [], [], []
    for a, count in enumerate(counts):
        site = a % n_sites
        for _ in range(count):
            ops = []
            if a not in dummies:
                for k in range(int(rng.integers(1, 7))):
                    op = int(rng.choice([M, M, M, I, D, N, S, H, P, EQ, X, 11]))
                    ops.append((op, int(rng.integers(0, 4) if op in (I, D, N, S, H, P, 11) else rng.integers(1, 9))))
            consumed = sum(length for op, length in ops if op in (M, I, S, EQ, X))
            n = consumed + int(rng.integers(0, 3)) if rng.random() > 1 / 12 else max(0, consumed - int(rng.integers(1, 4)))
            quals += rng.integers(0, 94, size=n).tolist()
            cigars += [(length << 4) | op for op, length in ops]
            read_off.append(read_off[-1] + n)
            cigar_off.append(cigar_off[-1] + len(ops))
            ref_start.append(int(asm_start[site]) + int(rng.integers(-12, 6)))
            hp.append(int(rng.integers(0, 3)))
            site_of_read.append(site)
    arrays = dict(quals=np.array(quals + [0], np.uint8), read_off=np.array(read_off, np.int64), cigars=np.array(cigars + [0], np.uint32),
                  cigar_off=np.array(cigar_off, np.int64), ref_start=np.array(ref_start, np.int64), hp=np.array(hp, np.uint8),
                  site_of_read=np.array(site_of_read, np.int32), asm_start=asm_start, asm_stop=asm_stop)
    return arrays, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


CASES = {"the stride's edges": ([1, 1, 63, 64, 65, 130], (0,)), "one allele": ([7], ()), "four alleles": ([3, 1, 2, 70], (1,)),
         "five alleles": ([3, 1, 2, 7, 66], ())}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_python_loop_through_host_and_device_pointers(engine, name):
    from hello_amd import featurizer as fz
    counts, dummies = CASES[name]
    arrays, off = random_arrays(counts, dummies, 23 + len(counts))
    want = python_evidence(arrays, off)
    assert all((want[a] == 0).all() for a in dummies)
    if len(counts) > 1:                                                    # the inputs reach every column and every hp value
        assert (want.sum(axis=0) > 0).all() and set(arrays["hp"].tolist()) == {0, 1, 2}
    host = fz.allele_evidence(engine, arrays, off)
    assert host.dtype == np.int64 and host.shape == want.shape and np.array_equal(host, want)
    dev = fz.allele_evidence(engine, arrays, off, device=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    assert fz.allele_evidence(engine, arrays, off).tobytes() == host.tobytes()                # two runs, the same bytes
    assert fz.allele_evidence(engine, arrays, off, device=True).cpu().numpy().tobytes() == host.tobytes()


def test_device_arrays_out_of_range_are_guarded(engine):
    """What the host form refuses reaches the kernel through device pointers: a site_of_read outside [0, S) counts in column
    5, allele offsets outside [0, R] are clamped."""
    import torch
    from hello_amd import featurizer as fz
    arrays, off = random_arrays([3, 1, 2, 70], (), 5)
    arrays["site_of_read"][1] = 3
    arrays["site_of_read"][10] = -1
    bad_off = off.copy()
    bad_off[0], bad_off[-1] = -5, off[-1] + 9
    want = python_evidence(arrays, off)
    assert want[0, 5] >= 1 and want[3, 5] >= 1
    dev = {k: torch.from_numpy(np.ascontiguousarray(dict(arrays, allele_off=bad_off)[k], fz.EVIDENCE_DTYPES[k])).to("cuda:0")
           for k in fz.EVIDENCE_ARRAYS}
    out = torch.zeros((4, 6), dtype=torch.int64, device="cuda:0")
    with engine.on_stream(out.device) as handle:
        fz.allele_evidence_device(engine, {k: dev[k].data_ptr() for k in fz.EVIDENCE_ARRAYS}, int(off[-1]), 3, 4, out.data_ptr(), handle)
    assert np.array_equal(out.cpu().numpy(), want)


def test_refusals_and_the_empty_launch(engine):
    import torch
    from hello_amd import featurizer as fz
    lib = engine.lib
    arrays, off = random_arrays([3, 4, 2], (), 1)
    out = np.full((3, 6), -7, np.int64)

    def run(n_alleles=3, n_sites=3, **changed):
        a = {k: np.ascontiguousarray(v, fz.EVIDENCE_DTYPES[k]) for k, v in {**arrays, "allele_off": off, **changed}.items()}
        return lib.hello_engine_allele_evidence(engine.handle, *[a[k].ctypes.data for k in fz.EVIDENCE_ARRAYS], 9, n_sites, n_alleles,
                                                out.ctypes.data, 0, None)
    shifted = lambda v: np.concatenate([[1], v[1:]])                                          # noqa: E731
    assert run(allele_off=[0, 5, 3, 9]) == -2 and b"decreases" in lib.hello_last_error()
    assert run(allele_off=[0, 3, 7, 8]) == -2 and b"ends at 8" in lib.hello_last_error()
    assert run(allele_off=[0, 3, 7, 10]) == -2
    for name in ("read_off", "cigar_off", "allele_off"):
        assert run(**{name: shifted(dict(arrays, allele_off=off)[name])}) == -2 and b"start at 0" in lib.hello_last_error(), name
    for name in ("read_off", "cigar_off"):
        v = arrays[name].copy()
        v[4] = v[3] - 1 if v[3] > 0 else v[5] + 1
        assert run(**{name: v}) == -2 and b"decrease" in lib.hello_last_error(), name
    for site in (3, -1):
        v = arrays["site_of_read"].copy()
        v[8] = site
        assert run(site_of_read=v) == -2 and b"site_of_read[8]" in lib.hello_last_error()
    assert run(n_sites=2) == -2
    assert (out == -7).all()
    assert run(n_alleles=0) == 0 and (out == -7).all()                                        # nothing is launched
    dev_out = torch.full((3, 6), -7, dtype=torch.int64, device="cuda:0")
    dev = {k: torch.from_numpy(np.ascontiguousarray(dict(arrays, allele_off=off)[k], fz.EVIDENCE_DTYPES[k])).to("cuda:0")
           for k in fz.EVIDENCE_ARRAYS}
    assert lib.hello_engine_allele_evidence(engine.handle, *[dev[k].data_ptr() for k in fz.EVIDENCE_ARRAYS], 9, 3, 0, dev_out.data_ptr(), 3,
                                            None) == 0
    torch.cuda.synchronize()
    assert bool((dev_out == -7).all())
    assert run() == 0 and np.array_equal(out, python_evidence(arrays, off))
    with pytest.raises(ValueError, match="do not fit"):
        fz.allele_evidence(engine, dict(arrays, hp=arrays["hp"][:-1]), off)


# ---- end to end -------------------------------------------------------------------------------------------------------
def _call(argv, workdir):
    done = subprocess.run([sys.executable, "-m", "hello_amd.call"] + argv + ["--workdir", workdir], cwd=ROOT, capture_output=True,
                          text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-3000:]
    return open(os.path.join(workdir, "results.output.vcf")).read()


def _split(text):
    lines = text.splitlines(keepends=True)
    return [line for line in lines if line.startswith("#")], [line for line in lines if not line.startswith("#")]


def _fields(line):
    cols = line.rstrip("\n").split("\t")
    return cols[7], dict(zip(cols[8].split(":"), cols[9].split(":")))


def _expected_lines(workdir, fasta, techs, hp=False):
    """The final VCF's record lines from the Python loop over the shard files' read arrays: per shard, the mean call of every
    ``.features`` entry with the support (NumPy counts) and the evidence (``python_evidence``) of its site's alleles."""
    from hello_amd import call, featurizer as fz, shards, vcf
    genome = call.read_fasta(fasta)
    lines = []
    paths = sorted(glob.glob(os.path.join(workdir, "shards", "*.hshard")), key=call.natural_key)
    assert paths
    for path in paths:
        sh = shards.PackedShard.from_file(path)
        support, evidence = [], []
        for t in techs:
            fa = sh.featurizer_core(t)
            off = fz.allele_offsets(fa["reads_per_allele"])
            real = np.diff(fa["cigar_off"]) > 0
            mapq, forward = fa["mapq"].astype(np.int64) * real, (fa["orientation"] > 0) & real
            support.append(np.array([(real[off[a]:off[a + 1]].sum(), forward[off[a]:off[a + 1]].sum(), mapq[off[a]:off[a + 1]].sum(),
                                      (mapq[off[a]:off[a + 1]] ** 2).sum()) for a in range(off.shape[0] - 1)], np.int64).reshape(-1, 4))
            evidence.append(python_evidence(fa, off))
            assert (evidence[-1][:, 5] == 0).all() and (evidence[-1][:, 0] <= support[-1][:, 0]).all()
        site_at = {(sh.chromosome_names[int(sh.chromosome_of_site[s])], int(sh.start[s])): s for s in range(sh.n_sites)}
        features = glob.glob(os.path.join(workdir, "features*", "features%d.features" % call.shard_number(path, 0)))
        assert len(features) == 1
        for entry in pickle.load(open(features[0], "rb")):
            row = vcf.mean_posteriors(entry["expertPredictions"], entry["meta"])
            mean = vcf.call_site(row, entry["chromosome"], entry["position"], entry["length"], genome[entry["chromosome"]])
            if mean is None:
                continue
            s = site_at[(entry["chromosome"], entry["position"])]
            lo, hi = int(sh.allele_off[s]), int(sh.allele_off[s + 1])
            sup, evi = [t[lo:hi] for t in support] + [None], [t[lo:hi] for t in evidence] + [None]
            lines.append((mean.position, len(lines), vcf.annotate_evidence(mean, sh.names(s), row, sup[0], evi[0], sup[1], evi[1], hp=hp) + "\n"))
    return [line for _, _, line in sorted(lines)]


def _shard_files(workdir):
    return {os.path.basename(p): open(p, "rb").read() for p in glob.glob(os.path.join(workdir, "features*", "features*"))
            if not p.endswith(".log")}


@pytest.fixture(scope="module")
def illumina_run(tmp_path_factory):
    """The smallest --from_bam input of the driver tests, written once, and its ``--from_bam --annotate_evidence`` run."""
    tmp_path = tmp_path_factory.mktemp("evidence")
    network, model = _network(tmp_path, False)
    network.close()
    reference, reads = illumina_input()
    bam, fa = _write(tmp_path, "i.bam", "chr1", reference, reads), _fasta(tmp_path, "chr1", reference)
    base = ["--ibam", bam, "--ref", fa, "--network", model, "--from_bam"]
    workdir = str(tmp_path / "evidence")
    return dict(base=base, bam=bam, fa=fa, tmp=tmp_path, workdir=workdir, vcf=_call(base + ["--annotate_evidence"], workdir),
                files=_shard_files(workdir))


def test_from_bam_annotate_evidence_end_to_end(illumina_run, tmp_path):
    from hello_amd import vcf
    annotated = _call(illumina_run["base"] + ["--annotate"], str(tmp_path / "w0"))
    head0, body0 = _split(annotated)
    head1, body1 = _split(illumina_run["vcf"])
    assert len(body0) > 0 and [vcf.strip_evidence(line) for line in body1] == body0
    assert all(line.split("\t")[8] == vcf.evidence_format(False, False) for line in body1)
    assert "".join(line for line in head1 if line not in head0) == vcf.evidence_header(False, False)[len(vcf.ANNOTATION_HEADER):]
    assert [line for line in head1 if line in head0] == head0
    assert body1 == _expected_lines(illumina_run["workdir"], illumina_run["fa"], (0,))
    seen = [_fields(line) for line in body1]
    assert any(re_int(info, "MBQ") > 10 for info, _ in seen) and any(re_int(info, "MPOS") > 10 for info, _ in seen)   # real bases were read
    assert all(f["PL"].split(",")[(lambda g: g[1] * (g[1] + 1) // 2 + g[0])(sorted(int(x) for x in f["GT"].split("/")))] == "0"
               for _, f in seen if f["PL"] != ".")
    files0, files1 = _shard_files(str(tmp_path / "w0")), illumina_run["files"]
    assert sorted(files0) == sorted(files1)
    for name in files0:                                                            # .features unchanged, .vcf lines stripped equal
        if name.endswith(".features"):
            assert files1[name] == files0[name], name
        else:
            assert "".join(vcf.strip_evidence(line) for line in files1[name].decode().splitlines(keepends=True)) == files0[name].decode(), name


def re_int(info, key):
    """The largest value of the INFO field ``key`` (``.`` = -1)."""
    text = [part for part in info.split(";") if part.startswith(key + "=")][0].split("=")[1]
    return max(-1 if v == "." else int(v) for v in text.split(","))


def test_resident_writes_the_bytes_of_the_shard_route(illumina_run, tmp_path):
    resident = _call(illumina_run["base"] + ["--annotate_evidence", "--resident"], str(tmp_path / "w2"))
    assert resident == illumina_run["vcf"] and any(not line.startswith("#") for line in resident.splitlines())
    assert _shard_files(str(tmp_path / "w2")) == illumina_run["files"]
    assert not os.path.exists(str(tmp_path / "w2" / "shards"))


def test_include_hp_decides_whether_the_haplotag_depths_are_written(illumina_run, tmp_path):
    from hello_amd import loader, netspec as ns, vcf, weights
    model = str(tmp_path / "hp.hello.npz")
    loader.save_native(model, "single_tech_hp", weights.synth_state(ns.build("single_tech_hp"), seed=17))
    argv = ["--ibam", illumina_run["bam"], "--ref", illumina_run["fa"], "--network", model, "--from_bam", "--annotate_evidence",
            "--include_hp"]
    head, body = _split(_call(argv, str(tmp_path / "w")))
    assert len(body) > 0 and all(line.split("\t")[8] == vcf.evidence_format(False, True) for line in body)
    assert "ID=AH1" in "".join(head) and "ID=AH2" in "".join(head) and "ID=ADI" not in "".join(head)
    assert body == _expected_lines(str(tmp_path / "w"), illumina_run["fa"], (0,), hp=True)
    head0, body0 = _split(illumina_run["vcf"])                                     # without --include_hp: neither field nor header
    assert "ID=AH1" not in "".join(head0) and all("AH1" not in line.split("\t")[8] for line in body0)


def test_from_bams_splits_the_depths_by_technology(tmp_path):
    from hello_amd import vcf
    network, model = _network(tmp_path, True)
    network.close()
    reference, illumina, pacbio = hybrid_synthetic(HYBRID_SEED, 20000)
    bams = [_write(tmp_path, "i.bam", "chr1", reference, illumina), _write(tmp_path, "p.bam", "chr1", reference, pacbio)]
    fa = _fasta(tmp_path, "chr1", reference)
    got = _call(["--ibam", bams[0], "--pbam", bams[1], "--ref", fa, "--network", model, "--from_bams", "--annotate_evidence"], str(tmp_path / "w"))
    head, body = _split(got)
    assert len(body) > 0 and all(line.split("\t")[8] == vcf.evidence_format(True, False) for line in body)
    assert "".join(line for line in head if line in vcf.evidence_header(True, True).splitlines(keepends=True)) == vcf.evidence_header(True, False)
    both = 0
    for line in body:
        _, f = _fields(line)
        adi, adp, ad = ([int(v) for v in f[k].split(",")] for k in ("ADI", "ADP", "AD"))
        assert [a + b for a, b in zip(adi, adp)] == ad, line
        both += sum(adi) > 0 and sum(adp) > 0
    assert both > 0                                                                # both technologies' reads are in the lines
    assert body == _expected_lines(str(tmp_path / "w"), fa, (0, 1))
