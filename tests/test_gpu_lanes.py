"""Laned programs (small launches of multi-chain models): the independent chains of a two-technology / three-expert forward
(MixtureOfExpertsAdvanced.py:161-252) on their own streams, ordered by events where one reads another's output -- the same kernels,
the same bits as the sequential program, sooner.  That the ordering is complete is shown on the CPU (tests/test_lane_model.py);
these tests run it."""
import numpy as np
import pytest

from hello_amd import compiler, netspec as ns, synth, weights
from tests.util import SEPARATE_META, load_fixture, separate_meta_spec

pytestmark = pytest.mark.gpu

# every fixture whose laned program has two lanes or more, and the full-size separate-meta model (two fused read convolvers per
# technology): tests/test_lane_model.py derives this list from the compiler and holds it to that
LANED = ["hybrid_no_ensemble", "hybrid_full", "hybrid_ensemble2", "hybrid_compressor2", "merged_hybrid", "hybrid_no_ensemble_addendum",
         "single_tech_softplus", "hybrid_no_ensemble_wide", "merged_hybrid_250", "single_tech_layernorm", SEPARATE_META]


def _separate_meta():
    """(spec, state, batch) of the separate-meta model: weights at gain 0.5, where the meta weights are not saturated (at gain 1.0
    the oracle's smallest weight is 0.0 at every site and a corrupted meta frame would hide behind a softmax of (1, 0, 0))."""
    spec = separate_meta_spec()
    return spec, weights.synth_state(spec, seed=5, gain=0.5), synth.make_sites(6, seed=3, coverage=12, hybrid_coverage=6)


def _same_bits(a, b):
    return all((x is None) == (y is None) and (x is None or np.array_equal(x, y)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", LANED)
def test_laned_program_gives_the_sequential_programs_bits(name):
    """Every model of LANED through an engine that runs lanes (small launch: the default route) and through one that was handed
    the sequential program: logits, meta weights and pair posteriors equal bit for bit, on the fixture's batch and on fifty
    back-to-back launches of varying composition; and both within the golden tolerance of the reference's outputs (the
    separate-meta model has no golden outputs: it is held to the oracle below)."""
    from hello_amd.engine import Engine, LANES_MAX_SITES
    if name == SEPARATE_META:
        (spec, state, batch), exp = _separate_meta(), None
    else:
        spec, state, batch, exp = load_fixture(name)
    laned = Engine(spec, state, device=0)
    sequential = Engine(spec, state, device=0, program=compiler.compile_model(spec, state))
    assert batch.n_sites <= LANES_MAX_SITES and sequential.small_launch_handle().value == sequential.handle.value
    got = laned.forward_batch(batch, posteriors=True)
    assert laned.lanes_handle is not None and laned.lanes_program.n_lanes >= 2 and laned._last_native.value == laned.lanes_handle.value
    want = sequential.forward_batch(batch, posteriors=True)
    assert _same_bits(got, want)
    assert got[2] is not None and (got[1] is not None) == laned.has_meta
    if exp is not None:
        np.testing.assert_allclose(got[0], exp["logits"], rtol=2e-5, atol=2e-4)
    kw = dict(coverage=20, hybrid_coverage=10, window=250) if name == "merged_hybrid_250" else dict(coverage=20, hybrid_coverage=10)
    pool = synth.make_sites(48, seed=5, **kw)
    rng = np.random.default_rng(1)
    for rep in range(50):
        lo = int(rng.integers(0, 40))
        sub = pool.site_slice(lo, lo + int(rng.integers(1, 9)))
        a, b = laned.forward_batch(sub, posteriors=True), sequential.forward_batch(sub, posteriors=True)
        assert _same_bits(a, b), (name, rep)
    # per-op profiling and debug capture time / snapshot the sequential program: an engine with them armed leaves the lanes
    laned.set_profiling(4)
    assert laned.small_launch_handle().value == laned.handle.value
    laned.forward_batch(batch, posteriors=True)
    rows, n = laned.op_times_ms()
    assert n == 1 and len(rows) == len(laned.program.ops)
    laned.set_profiling(0)
    assert laned.small_launch_handle().value == laned.lanes_handle.value
    # a launch larger than the lanes' limit runs the sequential program (several engines sharing a card lose with lanes beyond the
    # latency regime: the default limit is 64 sites) -- and an engine that is told it has the card to itself keeps the lanes, with
    # the sequential program's bits
    mid = synth.make_sites(300, seed=6, **kw)
    b = sequential.forward_batch(mid, posteriors=True)
    laned.forward_batch(mid)
    assert laned._last_native.value == laned.handle.value
    laned.lanes_max_sites = 4096
    a = laned.forward_batch(mid, posteriors=True)
    assert laned._last_native.value == laned.lanes_handle.value
    assert _same_bits(a, b)
    laned.close()
    sequential.close()


def test_separate_meta_model_matches_the_oracle_on_both_programs():
    """Two fused read convolvers per technology (readConv0 / readConv0Meta, readConv1 / readConv1Meta): the laned and the
    sequential program against oracle.moe_oracle, which evaluates the meta convolvers itself, at the parity suite's tolerances --
    with meta weights far enough from (1, 0, 0) that a wrong meta frame shows in them."""
    from hello_amd.engine import Engine
    from oracle import moe_oracle as mo
    from tests.test_gpu_parity import LOGIT_TOL, PROB_ATOL
    spec, state, batch = _separate_meta()
    want, want_meta = mo.forward_batch(mo.Oracle(spec, state, backend="torch"), batch)
    print("smallest oracle meta weight per site:", want_meta.min(axis=1))
    assert want_meta.shape == (batch.n_sites, 3) and want_meta.min() >= 0.05
    aoff = np.concatenate([[0], np.cumsum(batch.alleles_per_site)])
    rows = [mo.posteriors([mo.sigmoid(want[e, aoff[s]:aoff[s + 1]]) for e in range(3)], want_meta[s]) for s in range(batch.n_sites)]
    want_post = np.concatenate([np.stack(r) for r in rows], axis=1)
    laned = Engine(spec, state, device=0)
    sequential = Engine(spec, state, device=0, program=compiler.compile_model(spec, state))
    for label, eng in (("laned", laned), ("sequential", sequential)):
        logits, meta, post = eng.forward_batch(batch, posteriors=True)
        print(label, "max |dlogit|", float(np.abs(logits - want).max()), "max |dmeta|", float(np.abs(meta - want_meta).max()),
              "max |dposterior|", float(np.abs(post - want_post).max()))
        np.testing.assert_allclose(logits, want, **LOGIT_TOL)
        assert np.abs(mo.sigmoid(logits) - mo.sigmoid(want)).max() < PROB_ATOL
        assert np.abs(meta - want_meta).max() < PROB_ATOL
        assert post.shape == want_post.shape and np.abs(post - want_post).max() < PROB_ATOL
    assert laned._last_native.value == laned.lanes_handle.value and laned.lanes_program.n_lanes == 4
    assert sum(o.kind == compiler.OP_READCONV_FUSED for o in laned.lanes_program.ops) == 4
    assert sequential.lanes_handle is None and sequential._last_native.value == sequential.handle.value
    laned.close()
    sequential.close()


def test_separate_meta_model_one_site_per_call_gives_the_sequential_programs_bits():
    """The reference's call form -- one site per call through the plug-in surface (ScoringNetwork -> Engine.forward), which runs
    the laned program: twenty calls, every pair probability, expert probability and meta weight bit-equal to the same site scored
    through the sequential program."""
    from hello_amd.engine import Engine
    from hello_amd.wrapper import ScoringNetwork, pair_keys
    spec, state, _ = _separate_meta()
    pool = synth.make_sites(20, seed=11, coverage=12, hybrid_coverage=6)
    network = ScoringNetwork(spec, state, device=0, providePredictions=True)
    sequential = Engine(spec, state, device=0, program=compiler.compile_model(spec, state))
    aoff = np.concatenate([[0], np.cumsum(pool.alleles_per_site)])
    r0 = np.concatenate([[0], np.cumsum(pool.reads_per_allele0)])
    r1 = np.concatenate([[0], np.cumsum(pool.reads_per_allele1)])
    for s in range(pool.n_sites):
        alleles = [f"allele{k}" for k in range(aoff[s + 1] - aoff[s])]
        fd = {a: (pool.reads0[r0[k]:r0[k + 1]], pool.reads1[r1[k]:r1[k + 1]]) for a, k in zip(alleles, range(aoff[s], aoff[s + 1]))}
        got = network(fd, pool.ref_onehot[s:s + 1])
        assert network.engine._last_native.value == network.engine.lanes_handle.value
        _, meta, post = sequential.forward_batch(pool.site_slice(s, s + 1), posteriors=True)
        keys = pair_keys(alleles)
        for row in range(4):
            assert list(got[row].keys()) == keys
            assert np.array_equal(np.array([float(got[row][k]) for k in keys], np.float32), post[row]), (s, row)
        assert np.array_equal(got[4].numpy(), meta[0]), s
    assert network.engine.lanes_program.n_lanes == 4
    network.close()
    sequential.close()


def test_device_path_launches_on_lanes_stay_ordered_with_the_callers_stream():
    """Asynchronous device-path calls: outputs of back-to-back laned launches on the caller's stream are complete when that stream
    is (the call's stream joins every lane before the posteriors kernel), and equal the host path's."""
    import torch
    from hello_amd.engine import Engine
    spec = ns.build("hybrid_full")
    state = weights.synth_state(spec, seed=3)
    eng = Engine(spec, state, device=0)
    batches = [synth.make_sites(n, seed=20 + n, coverage=25, hybrid_coverage=12) for n in (3, 7, 1, 12, 5)]
    want = [eng.forward_batch(b, posteriors=True) for b in batches]
    stream = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(stream):
        for b in batches * 4:
            dev = synth.SiteBatch(torch.from_numpy(b.reads0).cuda(), b.reads_per_allele0, b.alleles_per_site, torch.from_numpy(b.ref_onehot).cuda(),
                                  torch.from_numpy(b.reads1).cuda(), b.reads_per_allele1)
            outs.append(eng.forward_batch(dev, posteriors=True, stream=stream.cuda_stream))
    stream.synchronize()
    for k, got in enumerate(outs):
        for g, w in zip(got, want[k % len(batches)]):
            assert np.array_equal(g.cpu().numpy(), w)
    eng.close()
