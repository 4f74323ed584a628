"""How the engine executes a laned ``compiler.Program``, restated in plain Python: what every op reads and writes, the order the
engine enforces between ops, and the pairs it leaves unordered although they share something one of them writes.  Nothing here
comes from the engine (hello_amd/csrc/engine.hip is the thing under test): the rules below were read off its forward loop and
are kept next to the lane flags in include/hello_mi355x.h.

The engine's rules (``Rules()``: the defaults):

  * an op runs on the stream its lane names (bits 8..10 of ``flags``); lane 0 is the call's stream.  A stream runs its ops in
    submission order, which is program order;
  * op i waits for the event of op w exactly where i reads a scratch buffer whose writer so far (the last op before i, in
    program order, that wrote it) is w, and w sits on another lane.  src0, src1 and res are reads -- except that OP_XATTN_FRONT
    WRITES res, next to dst; OP_HEAD writes an output slot (a logit row, or the meta weights), no buffer; ids below
    BUF_FIRST_SCRATCH are the caller's inputs, staged before the lanes start and only read;
  * every lane starts behind the "go" event, recorded on the call's stream once the inputs and index arrays are staged and the
    logits are zeroed; the call's stream waits for every lane's last op ("join") before the posteriors kernel reads the logit
    rows and the meta weights.  The next launch's go comes after this launch's join (the same stream), so launches do not overlap;
  * device memory beyond the ``hello_op`` buffers: the fused read convolver writes partial sums into a block that its finalize
    kernel reads back.  In a laned engine that block belongs to the op; in a sequential engine (one stream) the convolvers of
    one read technology share one.  Nothing else in the forward loop is written by an op: the weights, the index arrays (offsets,
    owners, slots) and the staged inputs are written before "go".

``Rules(partial_per_op=False)`` is the engine before it gave every fused op its own block; ``Rules(waits_follow_res=False)`` is an
engine that forgets that res is read (a dropped wait).  Both exist for the tests that plant those bugs.
"""
from dataclasses import dataclass
from typing import Dict, FrozenSet, List, Tuple

from hello_amd import compiler as cp

GO, JOIN = "go", "join"


@dataclass(frozen=True)
class Rules:
    partial_per_op: bool = True       # laned engine: a fused read convolver's partial sums are the op's own
    waits_follow_res: bool = True     # the engine's wait lists treat res as a read (it is, except for the expert front)


ENGINE = Rules()


def lane_of(op) -> int:
    return (op.flags >> cp.FLAG_LANE_SHIFT) & 7


def n_lanes(program) -> int:
    return max(lane_of(o) for o in program.ops) + 1


def _buffer_reads(op, with_res=True) -> List[int]:
    front = op.kind == cp.OP_XATTN_FRONT
    ids = [op.src0, op.src1] + ([op.res] if with_res and not front else [])
    return [b for b in ids if b != cp.BUF_NONE]


def _buffer_writes(op) -> List[int]:
    if op.kind == cp.OP_HEAD:
        return []
    return [op.dst] + ([op.res] if op.kind == cp.OP_XATTN_FRONT else [])


def _outputs(program) -> List[Tuple]:
    return [("logits", e) for e in range(program.n_experts)] + ([("meta",)] if program.has_meta else [])


def footprint(program, i, rules: Rules = ENGINE) -> Tuple[FrozenSet, FrozenSet]:
    """(reads, writes) of op ``i`` -- or of "go" / "join" -- as sets of resources: ("buffer", id) for scratch, ("input", id) for the
    caller's inputs, ("logits", slot) / ("meta",) for a HEAD's output, ("partial", ...) for the fused read convolver's sums."""
    if i == GO:       # staging: the inputs; zeroing the logits (experts without a head stay zero)
        return frozenset(), frozenset([("input", b) for b in range(cp.BUF_FIRST_SCRATCH)] + _outputs(program))
    if i == JOIN:     # the posteriors kernel and the copies back
        return frozenset(_outputs(program)), frozenset()
    op = program.ops[i]
    name = lambda b: ("input" if b < cp.BUF_FIRST_SCRATCH else "buffer", b)      # noqa: E731
    reads = {name(b) for b in _buffer_reads(op)}
    writes = {name(b) for b in _buffer_writes(op)}
    assert not any(kind == "input" for kind, _ in writes), f"op {i} writes one of the caller's inputs"
    if op.kind == cp.OP_HEAD:
        writes.add(("meta",) if op.dst == 3 else ("logits", op.dst))
    if op.kind == cp.OP_READCONV_FUSED:
        technology = 1 if op.seg == cp.SEG_R1A else 0
        block = ("partial", "op", i) if rules.partial_per_op and n_lanes(program) > 1 else ("partial", "technology", technology)
        reads.add(block)
        writes.add(block)
    return frozenset(reads), frozenset(writes)


@dataclass
class Order:
    """The order the engine enforces on one launch of a laned program."""
    lanes: List[int]                 # lane of every op
    waits: List[List[int]]           # per op: the ops of OTHER lanes whose event it waits for, in the order the engine finds them
    before: List[int]                # per op: bit set of the ops that happen before it

    def precedes(self, a, b) -> bool:
        """a happens before b ("go" before every op, every op before "join")."""
        if a == GO or b == JOIN:
            return a != b
        if a == JOIN or b == GO:
            return False
        return bool(self.before[b] >> a & 1)

    def ordered(self, a, b) -> bool:
        return self.precedes(a, b) or self.precedes(b, a)

    def describe(self) -> str:
        return "\n".join(f"{i:3d} lane {l} waits {w}" for i, (l, w) in enumerate(zip(self.lanes, self.waits)))


def happens_before(program, rules: Rules = ENGINE) -> Order:
    ops = program.ops
    lanes = [lane_of(o) for o in ops]
    writer: Dict[int, int] = {}
    last_on_lane: Dict[int, int] = {}
    waits: List[List[int]] = []
    before: List[int] = []
    for i, o in enumerate(ops):
        preds = []
        if lanes[i] in last_on_lane:
            preds.append(last_on_lane[lanes[i]])             # a stream is first in, first out
        mine = []
        for b in _buffer_reads(o, with_res=rules.waits_follow_res):
            w = writer.get(b)                                # an event can only be waited for once it has been recorded
            if b >= cp.BUF_FIRST_SCRATCH and w is not None and lanes[w] != lanes[i]:
                mine.append(w)
        waits.append(mine)
        acc = 0
        for p in preds + mine:
            acc |= before[p] | (1 << p)
        before.append(acc)
        for b in _buffer_writes(o):
            writer[b] = i
        last_on_lane[lanes[i]] = i
    return Order(lanes, waits, before)


def conflicts(program, rules: Rules = ENGINE) -> List[Tuple[int, int]]:
    """The pairs (a, b), a < b, of ops that touch a common resource, at least one of them writing it, and are not ordered
    ("go" and "join" are ordered with every op: every lane starts behind the one and is waited for by the other)."""
    order = happens_before(program, rules)
    prints = [footprint(program, i, rules) for i in range(len(program.ops))]
    out = []
    for x, (rx, wx) in enumerate(prints):
        for y in range(x + 1, len(prints)):
            ry, wy = prints[y]
            if (wx & (ry | wy) or wy & rx) and not order.ordered(x, y):
                out.append((x, y))
    return out


def unwritten_reads(program, rules: Rules = ENGINE) -> List[Tuple[int, Tuple]]:
    """(op, resource) wherever an op reads something that nothing before it -- no op that happens before it, nor the staging behind
    "go" -- has written: ordered, hence no race, but not the value the program means (a consumer submitted before its producer on
    its own lane).  What an op writes itself (its partial sums) is its own business."""
    order = happens_before(program, rules)
    nodes = [GO] + list(range(len(program.ops)))
    prints = {n: footprint(program, n, rules) for n in nodes}
    out = []
    for i in range(len(program.ops)):
        for r in sorted(prints[i][0] - prints[i][1]):
            if not any(r in prints[n][1] and order.precedes(n, i) for n in nodes):
                out.append((i, r))
    return out
