"""Laned programs are race-free, shown on the CPU: tests/lane_model.py restates how the engine orders the ops of a laned program
and these tests hold every program the compiler emits to "no two ops share something one of them writes without an order between
them" -- and the model itself to finding the bugs planted below, each with the op pair.  Nothing here needs a GPU."""
import copy
import glob
import itertools
import os

import numpy as np
import pytest

from hello_amd import compiler as cp, netspec as ns, weights
from tests import lane_model as lm
from tests.util import FIXTURES, GOLDEN, SEPARATE_META, load_fixture, separate_meta_spec

PICKLES = sorted(os.path.basename(p)[:-len(".wrapper.dnn")] for p in glob.glob(os.path.join(GOLDEN, "*.wrapper.dnn")))
PARENT = lm.Rules(partial_per_op=False)        # one partial block per read technology in a laned engine too: the engine before


def _model(name):
    if name == SEPARATE_META:
        spec = separate_meta_spec()
        return spec, weights.synth_state(spec, seed=5)
    if name in ns.CONFIGS:
        spec = ns.build(name)
        return spec, weights.synth_state(spec, seed=1)
    from hello_amd import loader
    return loader.load_spec(os.path.join(GOLDEN, name + ".wrapper.dnn"))


def _laned(name, **kw):
    spec, state = _model(name)
    return cp.compile_model(spec, state, lanes=True, **kw)


def _matrix(name):
    spec, state = _model(name)
    for fused, wino, arith in itertools.product([True, "trunk", False], [True, False], cp.ARITHMETICS):
        try:
            yield (fused, wino, arith), cp.compile_model(spec, state, fused=fused, winograd=wino, arithmetic=arith, lanes=True)
        except ValueError:
            continue                    # the arithmetic mode does not exist for this model / these options


# ---- every laned program the compiler emits -----------------------------------------------------------------------------
def test_the_pickles_are_the_golden_directory():
    assert PICKLES == ["mini_addendum", "mini_compressor2", "mini_merged", "mini_merged_concat", "mini_merged_sepmeta", "mini_reference"]


@pytest.mark.parametrize("name", list(ns.CONFIGS) + PICKLES + [SEPARATE_META])
def test_no_laned_program_leaves_a_conflict_unordered(name):
    n = 0
    for options, prog in _matrix(name):
        assert lm.n_lanes(prog) == prog.n_lanes, options
        assert lm.conflicts(prog) == [], (options, lm.conflicts(prog))
        assert lm.unwritten_reads(prog) == [], (options, lm.unwritten_reads(prog))
        n += 1
    assert n >= 6                       # fused x winograd in fp32 at the least


def test_separate_meta_model_has_two_fused_convolvers_per_technology_on_different_lanes():
    """What the matrix above must contain to mean anything for the partial sums: the full-size separate-meta model lowers all
    four convolvers to the fused op, each technology's two on different lanes with no order between them."""
    prog = _laned(SEPARATE_META)
    assert prog.n_lanes == 4 and prog.fused_read_convolver
    order = lm.happens_before(prog)
    fused = [(i, o.name.rsplit(".", 1)[-1], o.seg, order.lanes[i]) for i, o in enumerate(prog.ops) if o.kind == cp.OP_READCONV_FUSED]
    assert fused == [(0, "readConv0", cp.SEG_R0A, 0), (9, "readConv0Meta", cp.SEG_R0A, 3), (10, "readConv1Meta", cp.SEG_R1A, 0),
                     (11, "readConv1", cp.SEG_R1A, 1)]
    assert not order.ordered(0, 9) and not order.ordered(10, 11)
    # and the only separate-meta pickle cannot show it: its 8-channel convolvers are not fusable
    assert not _laned("mini_merged_sepmeta").fused_read_convolver


# ---- planted bugs: the model names the pair -------------------------------------------------------------------------------
def test_flags_two_convolvers_of_one_technology_sharing_their_partial_sums():
    """The engine as it was: one partial block per read technology.  readConv0 / readConv0Meta and readConv1Meta / readConv1
    write and read back the same block from different lanes."""
    prog = _laned(SEPARATE_META)
    assert lm.conflicts(prog, PARENT) == [(0, 9), (10, 11)]
    # "trunk" (the stem layer by layer, then the fused op from the pooled rows) still has the op: there the submission order
    # happens to put one technology's two behind each other's readers, the other's stay unordered; the layer path has no such op
    for fused, n_pairs in (("trunk", 1), (False, 0)):
        p = _laned(SEPARATE_META, fused=fused)
        pairs = lm.conflicts(p, PARENT)
        assert all(p.ops[a].kind == p.ops[b].kind == cp.OP_READCONV_FUSED and p.ops[a].seg == p.ops[b].seg for a, b in pairs)
        assert len(pairs) == n_pairs and sum(o.kind == cp.OP_READCONV_FUSED for o in p.ops) == (4 if fused else 0), fused
    # every model with one fused convolver per technology was safe under the old rule too: that is all the old comment claimed
    for name in ns.CONFIGS:
        assert lm.conflicts(_laned(name), PARENT) == [], name
    # the sequential program shares the block by design -- on one stream
    spec, state = _model(SEPARATE_META)
    sequential = cp.compile_model(spec, state)
    assert lm.n_lanes(sequential) == 1 and lm.conflicts(sequential) == []
    assert lm.footprint(sequential, 0)[1] & lm.footprint(sequential, next(i for i, o in enumerate(sequential.ops) if o.name.endswith("readConv0Meta")))[1] \
        == {("partial", "technology", 0)}


def test_flags_a_laned_program_compiled_with_buffer_reuse(monkeypatch):
    """hybrid_no_ensemble packed by liveness in program order (9 buffers instead of 20).  Technology 1's compressor (op 3, lane 1)
    lands in the buffer technology 0's convolver wrote (op 0) and its compressor reads (op 2), both lane 0: a write against a
    write (0, 3), against a read (2, 3), and op 5 reading op 3's value races op 0's (0, 5); combiner0's second convolution (op 8,
    lane 2) lands in compressor0's output, which lane 0's site sum (op 4) still reads: (4, 8)."""
    plain = cp._allocate
    monkeypatch.setattr(cp, "_allocate", lambda ops, values, reuse=True: plain(ops, values, reuse=True))
    prog = _laned("hybrid_no_ensemble")
    assert prog.n_lanes == 3 and len(prog.buffers) == 9
    assert (prog.ops[0].dst, prog.ops[2].src0, prog.ops[3].dst, prog.ops[5].src0) == (3, 3, 3, 3)
    assert (prog.ops[2].dst, prog.ops[4].src0, prog.ops[8].dst) == (5, 5, 5)
    assert lm.conflicts(prog) == [(0, 3), (0, 5), (2, 3), (4, 8)]
    monkeypatch.undo()
    assert len(_laned("hybrid_no_ensemble").buffers) == 20
    monkeypatch.setattr(cp, "_allocate", lambda ops, values, reuse=True: plain(ops, values, reuse=True))
    for name in ("hybrid_full", "merged_hybrid", SEPARATE_META, "single_tech_layernorm"):
        prog = _laned(name)
        pairs = lm.conflicts(prog)
        assert pairs and all(_shared(prog, a, b) and all(kind == "buffer" for kind, *_ in _shared(prog, a, b)) for a, b in pairs), name


def _shared(prog, a, b):
    """What ops a and b both touch, one of them writing it."""
    (ra, wa), (rb, wb) = lm.footprint(prog, a), lm.footprint(prog, b)
    return wa & (rb | wb) | wb & ra


def move_consumer_before_producer(prog):
    """The first op that opens a lane of its own behind other lanes' outputs, resubmitted just before the last of its producers
    -> (edited program, new index of the consumer, new index of that producer, the buffer)."""
    order = lm.happens_before(prog)
    r = next(i for i, w in enumerate(order.waits) if w and order.lanes[i] not in order.lanes[:i])
    w = max(order.waits[r])
    buffer = next(b for b in (prog.ops[r].src0, prog.ops[r].src1, prog.ops[r].res) if b in (prog.ops[w].dst, prog.ops[w].res))
    p = copy.deepcopy(prog)
    p.ops.insert(w, p.ops.pop(r))
    return p, w, w + 1, buffer


def test_flags_a_consumer_submitted_before_its_producer():
    for name in ("hybrid_no_ensemble", "hybrid_full", "merged_hybrid", SEPARATE_META):
        prog = _laned(name)
        edited, consumer, producer, buffer = move_consumer_before_producer(prog)
        assert edited.ops[consumer].name != edited.ops[producer].name and lm.lane_of(edited.ops[consumer]) != lm.lane_of(edited.ops[producer])
        assert lm.conflicts(edited) == [(consumer, producer)], name      # no event to wait for: recorded only once submitted
        assert (consumer, ("buffer", buffer)) in lm.unwritten_reads(edited)
    # on its OWN lane a consumer in front of its producer is ordered -- and reads what nobody wrote
    prog = _laned("hybrid_no_ensemble")
    p = copy.deepcopy(prog)
    assert p.ops[12].src0 == p.ops[11].dst and lm.lane_of(p.ops[11]) == lm.lane_of(p.ops[12])
    p.ops[11], p.ops[12] = p.ops[12], p.ops[11]
    assert lm.conflicts(p) == [] and lm.unwritten_reads(p) == [(11, ("buffer", prog.ops[11].dst))]


def test_flags_a_dropped_wait_for_the_residual():
    """An engine whose wait lists forget that `res` is read: wherever a block's shortcut was written on another lane and nothing
    else orders the two, the model names (shortcut's writer, reader)."""
    dropped = lm.Rules(waits_follow_res=False)
    found = {}
    for name in ns.CONFIGS:
        prog = _laned(name)
        if prog.n_lanes == 1:
            continue
        order = lm.happens_before(prog)
        pairs = lm.conflicts(prog, dropped)
        for a, b in pairs:
            writes = lm.footprint(prog, a)[1]
            assert ("buffer", prog.ops[b].res) in writes and prog.ops[b].kind != cp.OP_XATTN_FRONT, (name, a, b)
            assert a in order.waits[b] and order.lanes[a] != order.lanes[b] and a not in lm.happens_before(prog, dropped).waits[b]
        found[name] = pairs
    # single_tech_softplus: the strided block's shortcut convolution (op 5) sits on lane 1, the block's second convolution (op 7,
    # lane 0) adds it
    assert found["single_tech_softplus"] == [(5, 7)]
    assert found["hybrid_no_ensemble_wide"] == [(4, 8), (6, 9)] and len(found["single_tech_layernorm"]) == 3
    # where every shortcut stays on its reader's lane (or the expert front writes it) there is nothing to drop
    assert found["hybrid_full"] == [] and found["merged_hybrid"] == []


# ---- accepted re-orderings ---------------------------------------------------------------------------------------------------
def _reordered(prog, rng):
    """A random submission order that keeps every lane's order and every producer before its consumers."""
    order = lm.happens_before(prog)
    writer = {}
    preds = []
    last = {}
    for i, o in enumerate(prog.ops):
        mine = {writer[b] for b in lm._buffer_reads(o) if b in writer}
        if order.lanes[i] in last:
            mine.add(last[order.lanes[i]])
        preds.append(mine)
        last[order.lanes[i]] = i
        for b in lm._buffer_writes(o):
            writer[b] = i
    done, picks = set(), []
    while len(picks) < len(prog.ops):
        ready = [i for i in range(len(prog.ops)) if i not in done and preds[i] <= done]
        pick = int(rng.choice(ready))
        done.add(pick)
        picks.append(pick)
    p = copy.deepcopy(prog)
    p.ops = [p.ops[i] for i in picks]
    return p, picks


@pytest.mark.parametrize("name", ["hybrid_no_ensemble", "hybrid_full", "merged_hybrid_250", "single_tech_layernorm", SEPARATE_META])
def test_any_topological_reordering_within_the_lanes_order_passes(name):
    from tests.test_op_programs import _create
    prog = _laned(name)
    rng = np.random.default_rng(len(name))
    seen = set()
    for rep in range(12):
        p, picks = _reordered(prog, rng)
        seen.add(tuple(picks))
        assert lm.conflicts(p) == [] and lm.unwritten_reads(p) == [], picks
        # the same order between the same ops, whatever their numbers
        a, b = lm.happens_before(prog), lm.happens_before(p)
        new = {old: k for k, old in enumerate(picks)}
        assert all(a.precedes(x, y) == b.precedes(new[x], new[y]) for x in range(len(picks)) for y in range(len(picks)))
        if rep < 3:
            assert _create(p) is None
    assert len(seen) >= 6               # (the generator does vary the order)


# ---- the GPU test's list is derived -------------------------------------------------------------------------------------------
def test_the_gpu_lanes_list_is_every_fixture_with_two_lanes_plus_the_separate_meta_model():
    from tests.test_gpu_lanes import LANED
    want = []
    for name in FIXTURES:
        spec, state, _, _ = load_fixture(name)
        if cp.compile_model(spec, state, lanes=True).n_lanes >= 2:
            want.append(name)
    assert len(LANED) == len(set(LANED)) and sorted(LANED) == sorted(want + [SEPARATE_META])
    assert {"single_tech_softplus", "single_tech_layernorm"} <= set(LANED) and len(LANED) == 11
