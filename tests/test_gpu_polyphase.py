"""The polyphase form of the read convolver's strided convolution on the GPU (readconv_poly_kernel, the default): per-allele
frames, compressor output and expert-front outputs through the debug capture, against the CPU oracle and against the same
engine built with strided="direct" (the classic kernels of the same library).  Tolerances are those tests/test_gpu_parity.py
holds the same tensors to: frames 1e-5 relative + 1e-5 of their scale, compressor output 2e-5 + 2e-5 of its scale, front
outputs 2e-5 + 2e-6 of their scale, logits rtol 2e-5 / atol 2e-4.  The oracle keeps the frames and the compressor output
only: the expert front has no oracle tensor and is compared with the direct engine's (as tests/test_gpu_parity.py compares it
with another engine's); what follows it is held to the oracle through the logits."""
import numpy as np
import pytest

from hello_amd import compiler, netspec as ns, synth, weights

pytestmark = pytest.mark.gpu

LOGIT_TOL = dict(rtol=2e-5, atol=2e-4)


def _batch(reads_per_allele, alleles_per_site, channels=6, seed=7):
    """A batch of exactly this shape, cut from a seeded pool of synthetic pileups."""
    rpa = np.asarray(reads_per_allele, np.int32)
    aps = np.asarray(alleles_per_site, np.int32)
    assert aps.sum() == rpa.size
    pool = synth.make_sites(max(len(aps), 24), seed=seed, coverage=30, channels=channels)
    assert pool.reads0.shape[0] >= rpa.sum()
    return synth.SiteBatch(np.ascontiguousarray(pool.reads0[:rpa.sum()]), rpa, aps, np.ascontiguousarray(pool.ref_onehot[:len(aps)]))


def _sites_of(n_alleles):
    return [4] * (n_alleles // 4) + ([n_alleles % 4] if n_alleles % 4 else [])


def _rpa(n_alleles, seed):
    return np.random.default_rng(seed).integers(1, 6, size=n_alleles)


# 1 read in 1 allele; 5 reads over 2 alleles (a partly filled group); 9 reads; 1, 7, 9 and 13 alleles (partly filled
# workgroups of the allele stage, item starts anywhere in a 16-triple tile)
SHAPES = {
    "1 read": ([1], [1]),
    "5 reads, 2 alleles": ([3, 2], [2]),
    "9 reads": ([9], [1]),
    "1 allele": (_rpa(1, 1), _sites_of(1)),
    "7 alleles": (_rpa(7, 7), _sites_of(7)),
    "9 alleles": (_rpa(9, 9), _sites_of(9)),
    "13 alleles": (_rpa(13, 13), _sites_of(13)),
}


@pytest.fixture(scope="module")
def models():
    """(spec, state, polyphase engine -- read convolver AND compressor in that form --, direct engine, oracle) per model name,
    built once."""
    from hello_amd.engine import Engine
    from oracle import moe_oracle as mo
    cache = {}

    def get(name):
        if name not in cache:
            spec = ns.build(name)
            state = weights.synth_state(spec, seed=11)
            # (programs compiled here and handed over: the two forms side by side whatever the environment says)
            poly = Engine(spec, state, device=0, arithmetic="fp32", program=compiler.compile_model(spec, state, strided="polyphase+compressor"))
            direct = Engine(spec, state, device=0, arithmetic="fp32", program=compiler.compile_model(spec, state, strided="direct"))
            assert (poly.program.strided, direct.program.strided) == ("polyphase+compressor", "direct")
            assert sum(bool(o.flags & compiler.FLAG_POLYPHASE) for o in poly.program.ops) == 2      # read convolver and compressor
            assert not any(o.flags & compiler.FLAG_POLYPHASE for o in direct.program.ops)
            cache[name] = (spec, state, poly, direct, mo.Oracle(spec, state))
        return cache[name]

    yield get
    for _, _, poly, direct, _ in cache.values():
        poly.close()
        direct.close()


def _capture(eng, op, batch):
    eng.capture_op_output(op)
    logits, _ = eng.forward_batch(batch)
    out = eng.read_op_output().copy()
    eng.capture_op_output(None)
    return out, logits


def _op(program, kind):
    return next(i for i, o in enumerate(program.ops) if o.kind == kind)


def _check(models, name, batch, label):
    from oracle import moe_oracle as mo
    spec, state, poly, direct, oracle = models(name)
    want_logits, _ = mo.forward_batch(oracle, batch, chunk_sites=batch.n_sites)
    want_frames, want_ca = oracle.last["frames0"], oracle.last["ca0"]
    a = batch.n_alleles
    # read-convolver frames [alleles][36][64]
    fp, logits_p = _capture(poly, _op(poly.program, compiler.OP_READCONV_FUSED), batch)
    fd, logits_d = _capture(direct, _op(direct.program, compiler.OP_READCONV_FUSED), batch)
    fp, fd = (f.reshape(a, 36, 64).transpose(0, 2, 1) for f in (fp, fd))
    scale = float(np.abs(want_frames).max())
    print(f"{name} / {label}: frames |poly - oracle| / scale = {np.abs(fp - want_frames).max() / scale:.2e}, "
          f"|poly - direct| / scale = {np.abs(fp - fd).max() / scale:.2e}")
    np.testing.assert_allclose(fp, want_frames, rtol=1e-5, atol=1e-5 * scale, err_msg=f"{label}: frames vs oracle")
    np.testing.assert_allclose(fp, fd, rtol=1e-5, atol=1e-5 * scale, err_msg=f"{label}: frames vs direct")
    # compressor output [alleles][18][128]
    cp, _ = _capture(poly, _op(poly.program, compiler.OP_COMPRESSOR_FUSED), batch)
    cd, _ = _capture(direct, _op(direct.program, compiler.OP_COMPRESSOR_FUSED), batch)
    cp, cd = (c.reshape(a, 18, 128).transpose(0, 2, 1) for c in (cp, cd))
    scale = float(np.abs(want_ca).max())
    np.testing.assert_allclose(cp, want_ca, rtol=2e-5, atol=2e-5 * scale, err_msg=f"{label}: compressor vs oracle")
    np.testing.assert_allclose(cp, cd, rtol=2e-5, atol=2e-5 * scale, err_msg=f"{label}: compressor vs direct")
    # expert front: the strided convolution's rows (dst) and, through the op that consumes it, the shortcut
    front = _op(poly.program, compiler.OP_XATTN_FRONT)
    assert front == _op(direct.program, compiler.OP_XATTN_FRONT)
    for op in (front, front + 1):
        xp, _ = _capture(poly, op, batch)
        xd, _ = _capture(direct, op, batch)
        assert xp.shape == xd.shape and xp.size == a * 9 * 256
        scale = float(np.abs(xd).max())
        np.testing.assert_allclose(xp, xd, rtol=2e-5, atol=2e-6 * scale, err_msg=f"{label}: front op {op} vs direct")
    np.testing.assert_allclose(logits_p, want_logits, **LOGIT_TOL)
    np.testing.assert_allclose(logits_p, logits_d, **LOGIT_TOL)


@pytest.mark.parametrize("label", list(SHAPES))
def test_polyphase_frames_compressor_and_front_match_oracle_and_direct(models, label):
    _check(models, "single_tech", _batch(*SHAPES[label]), label)


def test_one_site_per_call(models):
    """Every site of the 13-allele batch alone: its own launch, one partly filled workgroup everywhere."""
    from oracle import moe_oracle as mo
    batch = _batch(*SHAPES["13 alleles"])
    spec, state, poly, direct, oracle = models("single_tech")
    whole, _ = poly.forward_batch(batch)
    aoff = np.concatenate([[0], np.cumsum(batch.alleles_per_site)])
    for s in range(batch.n_sites):
        _check(models, "single_tech", batch.site_slice(s, s + 1), f"site {s} alone")
        one, _ = poly.forward_batch(batch.site_slice(s, s + 1))
        np.testing.assert_allclose(one[0], whole[0, aoff[s]:aoff[s + 1]], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name,channels", [("single_tech_hp", 7), ("single_tech_addendum", 6)])
def test_seven_channel_and_five_block_models(models, name, channels):
    _check(models, name, _batch(_rpa(9, 5), _sites_of(9), channels=channels), name)


def test_engine_option_and_environment_select_the_form(monkeypatch):
    """The default is the polyphase form; Engine(..., strided="direct") and HELLO_STRIDED=direct select the classic kernels,
    and the program records which form its ops run."""
    import inspect
    from hello_amd.engine import Engine
    spec = ns.build("single_tech")
    state = weights.synth_state(spec, seed=11)
    batch = _batch(*SHAPES["5 reads, 2 alleles"])
    monkeypatch.delenv("HELLO_STRIDED", raising=False)
    eng = Engine(spec, state, device=0, arithmetic="fp32")
    assert eng.program.strided == "polyphase"              # the read convolver; the compressor's form is opt-in
    assert [bool(o.flags & compiler.FLAG_POLYPHASE) for o in eng.program.ops[:2]] == [True, False]
    want, _ = eng.forward_batch(batch)
    eng.close()
    monkeypatch.setenv("HELLO_STRIDED", "direct")
    eng = Engine(spec, state, device=0, arithmetic="fp32")
    assert eng.program.strided == "direct" and not any(o.flags & compiler.FLAG_POLYPHASE for o in eng.program.ops)
    got, _ = eng.forward_batch(batch)
    eng.close()
    np.testing.assert_allclose(got, want, **LOGIT_TOL)
    if "strided" in inspect.signature(Engine.__init__).parameters:      # (a suite-wide arithmetic fixture may wrap the constructor)
        monkeypatch.setenv("HELLO_STRIDED", "polyphase")
        eng = Engine(spec, state, device=0, arithmetic="fp32", strided="direct")
        assert eng.program.strided == "direct"
        eng.close()


def test_two_equal_launches_are_bit_identical(models):
    batch = _batch(*SHAPES["13 alleles"])
    _, _, poly, _, _ = models("single_tech")
    l1, _, p1 = poly.forward_batch(batch, posteriors=True)
    l2, _, p2 = poly.forward_batch(batch, posteriors=True)
    assert np.array_equal(l1, l2) and np.array_equal(p1, p2)
