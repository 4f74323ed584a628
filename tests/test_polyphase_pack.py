"""The polyphase form of a k3 / s2 / p1 convolution (hello_amd/readconv_pack.py polyphase_taps, readconv_poly_kernel):
y[p] = w1 e[p] + (w0 o[p-1] + w2 o[p]) with the bracket in Winograd F(3,2).  Float64 identity on the three strided shapes of
the network, evaluated over images stacked the way the kernels stack them, and the MFMA accounting of the new kernel entry."""
import os
import shutil
import sys

import numpy as np
import pytest

from hello_amd import readconv_pack as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HIP = os.path.join(ROOT, "hello_amd", "csrc", "readconv_fused.hip")
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("hipcc") is None, reason="no hipcc")


def _direct(x, w):
    """k3 / s2 / p1 convolution of one item, float64: x [cin, L], w [cout, cin, 3] -> [cout, (L - 1) // 2 + 1]."""
    cin, n = x.shape
    xp = np.zeros((cin, n + 2))
    xp[:, 1:n + 1] = x
    lout = (n - 1) // 2 + 1
    return np.stack([sum(w[:, :, t] @ xp[:, 2 * p + t] for t in range(3)) for p in range(lout)], axis=1)


def _stacked_polyphase(items, w, u, zero_rows):
    """The kernels' walk over a stacked image [rows][cin] whose row 0 is a leading zero row.
    zero_rows: items of odd length L sit at row stride L + 1 (ONE shared zero row between neighbours: the read convolver's
    32-channel image) -- d0 of an item's first triple and d3 of its last ARE those zero rows; else the items of even length
    touch (compressor, expert front) and d0 of an item's first triple is masked.  Flat output row r = triple 3T + i reads
    the even-phase image row 2r + 1 and the odd-phase rows 6T, 6T + 2, 6T + 4, 6T + 6."""
    n_items, cin, length = items.shape
    stride = length + 1 if zero_rows else length
    assert stride % 2 == 0 and (stride // 2) % 3 == 0
    lout = stride // 2
    img = np.zeros((1 + stride * n_items + 1, cin))
    for i in range(n_items):
        img[1 + stride * i:1 + stride * i + length] = items[i].T
    w1 = w[:, :, 1]
    out = np.zeros((n_items * lout, w.shape[0]))
    for t in range(n_items * lout // 3):
        d = [img[6 * t + 2 * i] for i in range(4)]
        if not zero_rows and t % (lout // 3) == 0:
            d[0] = np.zeros(cin)                                         # the previous item's last row: padding instead
        v = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[3] - d[1]]
        m = [u[:, :, c] @ v[c] for c in range(4)]
        z = [m[0] + m[1] + m[2], m[1] - m[2], m[1] + m[2] + m[3]]
        for i in range(3):
            out[3 * t + i] = w1 @ img[6 * t + 2 * i + 1] + z[i]
    return out.reshape(n_items, lout, -1).transpose(0, 2, 1)


@pytest.mark.parametrize("cin,cout,length,n_items,zero_rows", [(32, 64, 71, 4, True), (64, 128, 36, 8, False),
                                                              (128, 256, 18, 8, False)])
def test_polyphase_equals_the_direct_strided_convolution_in_float64(cin, cout, length, n_items, zero_rows):
    rng = np.random.default_rng(cin)
    w = rng.standard_normal((cout, cin, 3)).astype(np.float32) / np.sqrt(3 * cin)
    items = rng.standard_normal((n_items, cin, length))
    g = w.astype(np.float64)
    exact = rp.polyphase_taps(w, np.float64)                 # the packed taps, as formed (float64) before their one rounding
    assert np.array_equal(exact.astype(np.float32), rp.polyphase_taps(w)) and rp.polyphase_taps(w).dtype == np.float32
    assert np.array_equal(exact[..., 0], g[..., 0]) and np.array_equal(exact[..., 3], g[..., 2])
    want = np.stack([_direct(items[i], g) for i in range(n_items)])
    scale = np.abs(want).max()
    got = _stacked_polyphase(items, g, exact, zero_rows)
    assert got.shape == want.shape == (n_items, cout, (length - 1) // 2 + 1)
    assert np.abs(got - want).max() <= 1e-12 * scale
    # item by item, through the module's own float64 evaluation
    for i in range(n_items):
        assert np.abs(rp.polyphase_reference(items[i], g, exact) - want[i]).max() <= 1e-12 * scale


def test_packed_block_is_in_lane_order():
    from hello_amd import netspec as ns, weights
    spec = ns.build("single_tech")
    folded = weights.fold(spec, weights.synth_state(spec, seed=2))
    nodes = spec.nets["read_convolver0"]
    blob = rp.pack_polyphase(nodes, folded)
    w, _ = folded[rp.trunk_convs(nodes)[6].key]
    u = rp.polyphase_taps(w)
    centre = blob[:2048].reshape(4, 2, 64, 4)
    taps = blob[2048:].reshape(4, 2, 4, 64, 4)
    for cb, m, lane, t in ((0, 0, 0, 0), (3, 1, 63, 3), (2, 0, 37, 1)):
        o, i = 16 * cb + (lane & 15), 16 * m + 4 * (lane >> 4) + t
        assert centre[cb, m, lane, t] == w[o, i, 1]
        assert all(taps[cb, m, c, lane, t] == u[o, i, c] for c in range(4))
    assert blob.size == 10240
    # the compressor's strided 64 -> 128 convolution: 8 blocks x 4 input groups
    nodes = spec.nets["compressor0"]
    blob = rp.pack_compressor_polyphase(nodes, folded)
    w, _ = folded[nodes[1].body[0].key]
    u = rp.polyphase_taps(w)
    centre = blob[:8192].reshape(8, 4, 64, 4)
    taps = blob[8192:].reshape(8, 4, 4, 64, 4)
    for cb, m, lane, t in ((0, 0, 0, 0), (7, 3, 63, 3), (5, 2, 21, 2)):
        o, i = 16 * cb + (lane & 15), 16 * m + 4 * (lane >> 4) + t
        assert centre[cb, m, lane, t] == w[o, i, 1]
        assert all(taps[cb, m, c, lane, t] == u[o, i, c] for c in range(4))
    assert blob.size == 40960


def test_compiled_program_prices_the_form_it_runs():
    from hello_amd import compiler, netspec as ns, weights
    for name, ch in (("single_tech", 6), ("single_tech_hp", 7)):
        spec = ns.build(name)
        state = weights.synth_state(spec, seed=1)
        poly = compiler.compile_model(spec, state)
        direct = compiler.compile_model(spec, state, strided="direct")
        assert (poly.strided, direct.strided) == ("polyphase", "direct")
        op_p = next(o for o in poly.ops if o.kind == compiler.OP_READCONV_FUSED)
        op_d = next(o for o in direct.ops if o.kind == compiler.OP_READCONV_FUSED)
        assert op_p.flags & compiler.FLAG_POLYPHASE and not (op_d.flags & compiler.FLAG_POLYPHASE)
        assert op_d.exec_macs_per_row == rp.executed_macs_per_read(True, 0)
        assert op_p.exec_macs_per_row == rp.polyphase_executed_macs_per_read(ch, 0)
        assert op_d.exec_macs_per_row - op_p.exec_macs_per_row == (48 + (10 if ch == 6 else 0)) * 1024
        assert poly.weights.size == direct.weights.size + 10240
        both = compiler.compile_model(spec, state, strided="polyphase+compressor")
        assert both.strided == "polyphase+compressor" and both.weights.size == poly.weights.size + 40960
        assert next(o for o in both.ops if o.kind == compiler.OP_READCONV_FUSED).exec_macs_per_row == op_p.exec_macs_per_row
        comp_p = next(o for o in both.ops if o.kind == compiler.OP_COMPRESSOR_FUSED)
        comp_d = next(o for o in poly.ops if o.kind == compiler.OP_COMPRESSOR_FUSED)          # the default keeps the classic compressor
        assert comp_p.flags & compiler.FLAG_POLYPHASE and not (comp_d.flags & compiler.FLAG_POLYPHASE)
        assert comp_d.exec_macs_per_row == rp.compressor_executed_macs(2) == 3120 * 1024             # per wave: 8 items / 8 waves
        assert comp_p.exec_macs_per_row == rp.compressor_executed_macs(2, polyphase=True) == (3120 - 96) * 1024
    with pytest.raises(ValueError, match="strided"):
        compiler.compile_model(spec, state, strided="winograd")
    # where the polyphase kernel does not exist the program says so
    spec = ns.build("single_tech")
    assert compiler.compile_model(spec, weights.synth_state(spec, seed=1), fused="trunk").strided == "direct"
    split = compiler.compile_model(spec, weights.synth_state(spec, seed=1), arithmetic="bf16x3")      # its read convolver keeps the direct form
    assert not next(o for o in split.ops if o.kind == compiler.OP_READCONV_FUSED).flags & compiler.FLAG_POLYPHASE


POLY_SYMBOL = "_ZN5hello20readconv_poly_kernelINS_2rc3CfgILi4ELi4ELi150ELi0EEELi%dELi%dELb0EEEvNS_12ReadConvArgsE"
COMPRESSOR_POLY_SYMBOL = "_ZN5hello22compressor_poly_kernelILi%dEEEvNS_14CompressorArgsE"


@needs_hipcc
def test_polyphase_accounting_matches_the_instruction_stream():
    """One 16x16x4 MFMA = 1 024 MACs; per wave and group of 4 reads (the group loop is not unrolled)."""
    import check_asm_hazards
    for extra in (0, 2):
        for ch in (6, 7):
            per_wave_and_group = rp.polyphase_executed_macs_per_read(ch, extra) * 4 / 4 / 1024
            assert check_asm_hazards.mfma_count(HIP, POLY_SYMBOL % (3 + extra, ch)) == per_wave_and_group, (extra, ch)
    assert rp.polyphase_executed_macs_per_read(6) / 1024 == 2930 and rp.polyphase_executed_macs_per_read(7) / 1024 == 2940
    # the compressor: per wave and workgroup of 8 items (8 waves).  Its body holds the whole-workgroup path and the
    # partly-filled-workgroup path side by side (one of them runs), so the stream counts every MFMA twice
    for nb in (2, 3, 4):
        per_wave = rp.compressor_executed_macs(nb, polyphase=True) * 8 / 8 / 1024
        assert check_asm_hazards.mfma_count(HIP, COMPRESSOR_POLY_SYMBOL % nb) == 2 * per_wave, nb
    assert rp.compressor_executed_macs(2, polyphase=True) / 1024 == 3024


@needs_hipcc
def test_no_inline_asm_reads_a_fresh_mfma_result_with_the_polyphase_layers():
    import check_asm_hazards
    n, bad = check_asm_hazards.check(HIP)
    assert n > 0 and not bad, bad[:5]
