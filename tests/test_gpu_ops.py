"""Every layer kernel, one op at a time, against a float64 reference of the op's definition (include/hello_mi355x.h).

The case table (tests/op_programs.py CASES) reaches every kernel instantiation launch_conv1d, launch_kc, launch_conv1d_wino and
the elementwise launchers can start, each in a small launch (a few rows) and a large one (past every small-launch branch).
Every element is held to its own error bound (op_programs: C_ACC u (M + |b|) over the products the kernel rounds), so a
wrong tap, channel, border, bias or group fails while re-association passes."""
import numpy as np
import pytest

from tests import op_programs as op

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_case_table_reaches_every_instantiation(cus):
    reached = op.case_instantiations(cus)
    assert sorted(reached) == op.INSTANTIATIONS, (sorted(set(op.INSTANTIATIONS) - set(reached)), sorted(set(reached) - set(op.INSTANTIATIONS)))


@pytest.mark.parametrize("size", ["small", "large"])
@pytest.mark.parametrize("case", op.CASES, ids=lambda c: c.id)
def test_op_matches_float64(case, size, cus):
    from hello_amd.engine import Engine
    rows = op.rows_for(case, size, cus)
    built = op.build(case, rows, seed=hash(case.id) % 1000)
    eng = Engine(None, None, program=built.program)
    try:
        got_in = {name: op.capture(eng, built, i) for name, i in built.inputs.items()}
        if case.kind == "head":
            eng.capture_op_output(None)
            logits, meta = eng.forward(built.reads0, built.rpa, built.aps)
            o = built.program.ops[built.subject]
            got = np.asarray(meta)[:, :o.cout] if o.dst == 3 else np.asarray(logits)[0][:, None]
        else:
            got = op.capture(eng, built, built.subject)
    finally:
        eng.close()
    ref, bound = op.reference(built, got_in, case)
    ratio, n_bad = op.excess(got, ref, bound)
    name = op.instantiation(built.program.ops[built.subject], built.rows, cus)
    assert n_bad == 0, f"{name}, {built.rows} rows: {n_bad} of {ref.size} elements over their bound (worst error / bound {ratio:.3g})"
