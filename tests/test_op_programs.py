"""hello_engine_create's buffer rules (include/hello_mi355x.h, next to hello_op), the programs the compiler emits against them,
and the per-element error bound of tests/op_programs.py against planted bugs.  Nothing here launches a kernel: a refused
program never reaches a forward, and an accepted one is only created (no GPU: refused later with HELLO_ERR_NOGPU)."""
import copy
import itertools
import re

import numpy as np
import pytest

from hello_amd import compiler as cp, netspec as ns, weights
from tests import op_programs as op


def _create(prog):
    """None when the program passes validation (created on a GPU; status -5 without one), else the refusal message."""
    from hello_amd.engine import Engine
    try:
        Engine(None, None, program=prog).close()
    except RuntimeError as e:
        if "(status -5)" in str(e):
            return None
        return str(e)
    return None


def _refused(prog, match):
    msg = _create(prog)
    assert msg is not None and "(status -3)" in msg, msg
    assert re.search(match, msg), msg


@pytest.fixture(scope="module")
def layered():
    spec = ns.build("single_tech")
    return cp.compile_model(spec, weights.synth_state(spec, seed=21), fused=False)


def _edit(prog, index, **fields):
    p = copy.deepcopy(prog)
    for k, v in fields.items():
        setattr(p.ops[index], k, v)
    return p


def _first(prog, kind, pred=lambda o: True):
    return next(i for i, o in enumerate(prog.ops) if o.kind == kind and pred(o))


# ---- every program the compiler emits passes -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ns.CONFIGS))
def test_every_compiled_program_validates(name):
    spec = ns.build(name)
    state = weights.synth_state(spec, seed=1)
    n = 0
    for fused, wino, lanes, arith in itertools.product([True, False, "trunk"], [True, False], [False, True],
                                                        ["fp32", "bf16x3", "bf16x3+32"]):
        try:
            prog = cp.compile_model(spec, state, fused=fused, winograd=wino, lanes=lanes, arithmetic=arith)
        except ValueError:
            continue                    # the arithmetic mode does not exist for this model / these options
        assert _create(prog) is None, (fused, wino, lanes, arith, _create(prog))
        n += 1
    assert n >= 12


def test_every_case_program_validates():
    for case in op.CASES:
        for size in ("small", "large"):
            assert _create(op.build(case, op.rows_for(case, size, 256)).program) is None, case.id


# ---- one refusal per rule ---------------------------------------------------------------------------------------------
def test_refuses_dst_outside_the_op_domain(layered):
    sites = next(i for i, (d, _) in enumerate(layered.buffers) if d == cp.ROWS_SITES)
    _refused(_edit(layered, 1, dst=sites), r"dst buffer \d+ has rows of domain 3, the op writes domain 0")


def test_refuses_sources_of_another_domain(layered):
    alle = next(i for i, (d, _) in enumerate(layered.buffers) if d == cp.ROWS_ALLELES)
    _refused(_edit(layered, 1, src0=alle), r"src0 buffer \d+ has rows of domain 2, the op reads domain 0")
    mix = _first(layered, cp.OP_MIX)
    _refused(_edit(layered, mix, src1=alle), r"src1 buffer \d+ has rows of domain 2, the op reads domain 3")
    seg = _first(layered, cp.OP_SEGSUM, lambda o: o.seg == cp.SEG_AS)
    _refused(_edit(layered, seg, seg=cp.SEG_R0A), r"op domain 3 is not the domain its segment kind writes")
    res = _first(layered, cp.OP_CONV1D, lambda o: o.res != cp.BUF_NONE and o.domain == cp.ROWS_READS0)
    _refused(_edit(layered, res, res=alle), r"res buffer \d+ has rows of domain 2")


def test_refuses_buffers_too_small(layered):
    p = copy.deepcopy(layered)
    p.buffers.append((cp.ROWS_READS0, 1))
    _refused(_edit(p, 1, dst=len(p.buffers) - 1), r"holds 1 floats per row, the op's output \(lout \* cout\) needs")
    _refused(_edit(layered, 1, lin=400, lout=398), r"the op's input \(lin \* cin\) needs 6400")
    head = _first(layered, cp.OP_HEAD)
    _refused(_edit(layered, head, lin=10 ** 6), r"input \(HEAD: lin \* cin\) needs 256000000")
    b = op.build(op.Case("c", "concat", dict(lin=7, cin=8, c1=12)), 3)
    _refused(_edit(b.program, b.subject, c1=16), r"second source \(lin \* c1\) needs")
    b = op.build(op.Case("t", "conv", dict(wino=True, cin=64, seg=16, cout=64, k=3, pad=1, lin=18, act="relu")), 3)
    b.program.buffers.append((cp.ROWS_READS0, 18 * 47))
    _refused(_edit(b.program, b.subject, src1=len(b.program.buffers) - 1), r"second source \(lin \* \(cin - seg\)\) needs 864")


def test_refuses_uint8_inputs_misread(layered):
    _refused(_edit(layered, 0, flags=layered.ops[0].flags & ~cp.FLAG_SRC_U8), r"HELLO_FLAG_SRC_U8 must be set exactly when src0")
    _refused(_edit(layered, 1, flags=layered.ops[1].flags | cp.FLAG_SRC_U8), r"HELLO_FLAG_SRC_U8 must be set exactly when src0")
    _refused(_edit(layered, 0, cin=5), r"a uint8 input holds \[window 150\]\[6 channels\]")
    _refused(_edit(layered, 0, lin=200, lout=198), r"a uint8 input holds \[window 150\]")
    _refused(_edit(layered, 3, src0=cp.BUF_READS0), r"HELLO_FLAG_SRC_U8 must be set exactly")


def test_refuses_float4_kernels_on_partial_float4s(layered):
    mp = _first(layered, cp.OP_MAXPOOL)
    _refused(_edit(layered, mp, cin=6, cout=6), r"\(maxpool\): channel counts must be positive multiples of 4")
    seg = _first(layered, cp.OP_SEGSUM)
    _refused(_edit(layered, seg, cin=3), r"\(segsum\): channel counts must be positive multiples of 4")
    _refused(_edit(layered, _first(layered, cp.OP_MIX), cin=126), r"\(mix\): channel counts must be positive multiples of 4")
    b = op.build(op.Case("c", "concat", dict(lin=7, cin=8, c1=12)), 3)
    _refused(_edit(b.program, b.subject, c1=10), r"\(concat\): channel counts must be positive multiples of 4")
    b = op.build(op.Case("a", "add", dict(lin=7, cin=12)), 3)
    _refused(_edit(b.program, b.subject, cin=6), r"\(add\): channel counts must be positive multiples of 4")


def test_refuses_length_changes_where_the_op_keeps_the_row():
    for case in (op.Case("a", "add", dict(lin=7, cin=12)), op.Case("c", "concat", dict(lin=7, cin=8, c1=12)),
                 op.Case("m", "mix", dict(lin=9, cin=16, a0=2.0, a1=-1.0)), op.Case("s", "segsum", dict(lin=5, cin=12)),
                 op.Case("l", "layernorm", dict(cin=100, lin=5))):
        b = op.build(case, 3)
        _refused(_edit(b.program, b.subject, lout=b.program.ops[b.subject].lin - 1), r"the op keeps the row length: lin == lout")


def test_refuses_malformed_maxpool_geometry(layered):
    mp = _first(layered, cp.OP_MAXPOOL)
    for fields in (dict(lout=72), dict(k=0), dict(stride=0), dict(pad=2), dict(pad=-1), dict(lin=2, lout=1)):
        _refused(_edit(layered, mp, **fields), r"MaxPool geometry needs k >= 1")


def test_refuses_conv_shorter_than_its_kernel():
    b = op.build(op.Case("c", "conv", dict(cin=16, cout=16, k=3, stride=2, lin=4)), 3)
    _refused(_edit(b.program, b.subject, lin=2, lout=1), r"lout inconsistent")


def test_refuses_malformed_heads(layered):
    head = _first(layered, cp.OP_HEAD)
    _refused(_edit(layered, head, lin=0), r"a HEAD averages lin > 0 positions")
    _refused(_edit(layered, head, cout=2), r"output slot 0 is a logit row")
    _refused(_edit(layered, head, dst=1), r"output slot 1 is a logit row")      # n_experts == 1
    _refused(_edit(layered, head, dst=3), r"output slot 3 is meta")             # no meta, and ALLELES rows
    b = op.build(op.Case("h", "head", dict(cout=3, cin=256, lin=9)), 3)
    _refused(_edit(b.program, b.subject, cout=4), r"output slot 3 is meta \[sites\]\[3\]: a SITES-domain head of at most 3")


def test_refuses_ops_in_place(layered):
    _refused(_edit(layered, 1, dst=layered.ops[1].src0), r"dst buffer \d+ is also a source \(no op runs in place\)")
    mix = _first(layered, cp.OP_MIX)
    _refused(_edit(layered, mix, dst=layered.ops[mix].src0), r"is also a source")


def test_issue_programs_are_refused(layered):
    """The single-op edits of the layer-by-layer single_tech program that used to get through to the device check."""
    seg = _first(layered, cp.OP_SEGSUM)
    mp = _first(layered, cp.OP_MAXPOOL)
    sites = next(i for i, (d, _) in enumerate(layered.buffers) if d == cp.ROWS_SITES)
    p = copy.deepcopy(layered)
    p.buffers.append((cp.ROWS_READS0, 1))
    for prog in (_edit(p, 1, dst=len(p.buffers) - 1), _edit(layered, 1, dst=sites), _edit(layered, 1, dst=layered.ops[1].src0),
                 _edit(layered, mp, cin=6, cout=6), _edit(layered, mp, lout=40), _edit(layered, mp, k=0),
                 _edit(layered, seg, cin=3, lin=1, lout=1), _edit(layered, _first(layered, cp.OP_HEAD), lin=10 ** 6)):
        msg = _create(prog)
        assert msg is not None and "(status -3)" in msg, msg


# ---- laned programs: the lane analysis runs on the host, before the device lookup ----------------------------------------------
@pytest.fixture(scope="module")
def laned():
    spec = ns.build("hybrid_no_ensemble")
    prog = cp.compile_model(spec, weights.synth_state(spec, seed=21), lanes=True)
    assert prog.n_lanes == 3 and _create(prog) is None
    return prog


def test_refuses_a_laned_program_that_reads_a_buffer_before_its_writer(laned):
    """A consumer submitted before its producer on another lane: there is no event to wait for yet.  The op the engine names is
    the one tests/lane_model.py finds unordered with the buffer's writer."""
    from tests import lane_model as lm
    from tests.test_lane_model import move_consumer_before_producer
    edited, consumer, producer, buffer = move_consumer_before_producer(laned)
    msg = _create(edited)
    assert msg is not None and "(status -3)" in msg, msg
    found = re.search(r"laned program: op (\d+) reads buffer (\d+) before any op wrote it", msg)
    assert found, msg
    assert lm.conflicts(edited) == [(consumer, producer)]
    assert int(found.group(1)) == consumer and int(found.group(2)) == buffer == edited.ops[producer].dst


def test_refuses_a_laned_program_that_writes_a_buffer_twice(laned):
    """Technology 1's read convolver (op 1, lane 1) writing into the frames of technology 0's (op 0, lane 0): the two ops the
    engine names are the pair tests/lane_model.py finds unordered (the frames' reader, op 2, follows op 0 on its lane and would
    wait for op 1)."""
    from tests import lane_model as lm
    assert [laned.ops[i].kind for i in (0, 1)] == [cp.OP_READCONV_FUSED] * 2 and lm.lane_of(laned.ops[0]) != lm.lane_of(laned.ops[1])
    edited = _edit(laned, 1, dst=laned.ops[0].dst)
    msg = _create(edited)
    assert msg is not None and "(status -3)" in msg, msg
    found = re.search(r"laned program: ops (\d+) and (\d+) both write buffer (\d+) \(a program with lanes may not reuse buffers\)", msg)
    assert found, msg
    assert lm.conflicts(edited) == [(int(found.group(1)), int(found.group(2)))] == [(0, 1)] and int(found.group(3)) == laned.ops[0].dst
    # the sequential program reuses buffers by design: no lanes, no refusal
    spec = ns.build("hybrid_no_ensemble")
    assert _create(cp.compile_model(spec, weights.synth_state(spec, seed=21))) is None


# ---- the launch mirror and the error bound ------------------------------------------------------------------------------
def test_case_table_reaches_every_instantiation_on_256_cus():
    reached = op.case_instantiations(256)
    assert sorted(reached) == op.INSTANTIATIONS


@pytest.mark.parametrize("m", [2, 3])
def test_winograd_transforms_reproduce_the_direct_form(m):
    t = op.WINO[m]
    rng = np.random.default_rng(m)
    for _ in range(10):
        g, d = rng.standard_normal(3), rng.standard_normal(m + 2)
        y = t["A"] @ ((t["G"] @ g) * (t["B"] @ d))
        assert np.allclose(y, [g @ d[u:u + 3] for u in range(m)], rtol=0, atol=1e-12)
    assert op.wino_bound_weights(m).max() == {2: 2.0, 3: 6.0}[m]


MUTATION_GEOMETRIES = [
    dict(cin=12, cout=20, k=3, stride=1, pad=1, lin=37, groups=1, act="softplus", res=False, wino=0),
    dict(cin=32, cout=36, k=5, stride=2, pad=2, lin=29, groups=1, act="relu", res=True, wino=0),
    dict(cin=16, cout=8, k=7, stride=3, pad=3, lin=40, groups=1, act="softplus", res=True, wino=0),
    dict(cin=32, cout=16, k=3, stride=1, pad=1, lin=18, groups=2, act="relu", res=True, wino=0),
    dict(cin=64, cout=32, k=3, stride=1, pad=1, lin=10, groups=1, act="softplus", res=True, wino=2),
    dict(cin=32, cout=32, k=3, stride=1, pad=1, lin=9, groups=2, act="relu", res=False, wino=3),
]


def _mutations(g):
    out = ["tap_shift", "drop_last_channel", "bias0_missing", "bias_last_missing"]
    if g["res"] and g["act"] != "none":
        out.append("res_before_act")
    if g["pad"]:
        out.append("pad_wrong_side")
    if g["act"] == "softplus":
        out.append("softplus_sign")
    if g["groups"] > 1:
        out.append("group_swap")
    return out


@pytest.mark.parametrize("g", MUTATION_GEOMETRIES, ids=lambda g: "_".join(f"{k}{v}" for k, v in g.items()))
def test_bound_passes_reassociation_and_fails_planted_bugs(g):
    rng = np.random.default_rng(7)
    rows = 5
    lout = (g["lin"] + 2 * g["pad"] - g["k"]) // g["stride"] + 1
    x = rng.standard_normal((rows, g["lin"], g["cin"])).astype(np.float32)
    # weights large enough that pre-activations reach beyond +-20 (the Softplus threshold)
    w = (rng.standard_normal((g["cout"], g["cin"] // g["groups"], g["k"])) * 12 / np.sqrt(g["k"] * g["cin"])).astype(np.float32)
    b = (rng.choice([-1, 1], g["cout"]) * rng.uniform(0.5, 1.5, g["cout"])).astype(np.float32)
    res = rng.standard_normal((rows, lout, g["cout"])).astype(np.float32) if g["res"] else None
    kw = dict(groups=g["groups"], act=g["act"], res=res, wino_m=g["wino"])
    exact, bound = op.conv_reference(x, w, b, g["stride"], g["pad"], **kw)
    assert op.excess(exact.astype(np.float32), exact, bound)[1] == 0
    f32, _ = op.conv_reference(x, w, b, g["stride"], g["pad"], dtype=np.float32, **kw)
    assert op.excess(f32.astype(np.float32), exact, bound)[1] == 0
    for mutation in _mutations(g):
        bad, _ = op.conv_reference(x, w, b, g["stride"], g["pad"], mutation=mutation, **kw)
        ratio, n_bad = op.excess(bad.astype(np.float32), exact, bound)
        assert n_bad > 0, (mutation, ratio)
