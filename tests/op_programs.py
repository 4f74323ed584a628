"""Hand-built programs that isolate one layer kernel, float64 references of every op kind, per-element error bounds, and a
mirror of the launchers' kernel choice (tests/test_gpu_ops.py, tests/test_op_programs.py).

A case's program is: a k=1 CONV1D from the uint8 pileup bytes (random signed weights: float activations of both signs), the
SEGSUMs that carry it to the ALLELES / SITES domain when the subject lives there, further input convolutions for a residual or
a second source, the SUBJECT op, and a HEAD that writes logit slot 0.  Every buffer is written by one op, so a debug capture
after any op returns exactly what the subject read.  A buffer is a dense [rows][positions][channels] tensor in the shape of
the op that reads it: a subject whose row is [lin][cin] reads the first rows * lin * cin floats its producer wrote, whatever
that producer's own row shape -- which sets lin and cin free of the window (and gives float rows of any channel count).

Error bounds are per element, from the op's definition (include/hello_mi355x.h), never a global atol:

    |got - ref| <= C_ACC u (M + |b|) + u |ref|          u = 2^-24

where M is the magnitude the kernel's rounding errors scale with.  For a direct convolution M = sum |w x| over the output's
own products.  For the Winograd forms (hello_amd/csrc/conv_wino.hip, file header) the kernel never forms those products: it
forms M_c = U_c . V_c per component c, with U = G g (rounded once on the host) and V = B^T d (one or two roundings in
registers), and combines them with the output transform A.  Every rounding is relative to a |U_c| |V_c| or a partial sum of
them, and

    sum_c |A_uc| |U_c| |V_c|  <=  sum_{j,t} W_u[j, t] |g_j| |d_t|,     W_u[j, t] = sum_c |A_uc| |G_cj| |B_ct|

(the triangle inequality on U_c = sum_j G_cj g_j and V_c = sum_t B_ct d_t).  So M = sum_ch sum_{j,t} W_u[j, t] |g_ch,j| |d_ch,t|
over the tile's inputs.  W_u is computed below from the transforms (largest entry: 2 for F(2,3), 6 for F(3,3), on the last
output of a triple); it is the "larger constant" of the Winograd forms -- an entry per (tap, input) pair of the tile where the
direct form has 1 on the pairs its output uses and 0 elsewhere.  C_ACC = 32 bounds the rounding of a chain of a few thousand
fp32 additions of random signs relative to the sum of their magnitudes (the worst case, K u for K terms of one sign, does not
arise with signed data); the transforms add at most 4 roundings of the same magnitudes (C_WINO = C_ACC + 8).  A dropped
product changes an output by ~M / K, far above C_ACC u M for every K here; re-association stays far below it.

Activation: ReLU is 1-Lipschitz and exact; Softplus (beta 1, threshold 20) is 1-Lipschitz and its hardware exp / log
evaluation adds C_SP u (1 + |x| + |y|) (exp of x log2 e loses |x| log2 e u relative, 1 + e^x and the log lose a few u
of 1 and of y).  The residual is added after the activation: one more rounding, u |ref|.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from hello_amd import compiler as cp

U = 2.0 ** -24
C_ACC = 32
C_WINO = C_ACC + 8
C_SP = 8

ACTS = {"none": 0, "relu": cp.FLAG_RELU, "softplus": cp.FLAG_SOFTPLUS}

# ---- the launchers' kernel choice (hello_amd/csrc/conv_generic.hip, conv_wino.hip, elementwise.hip) ------------------------
# Every instantiation those launchers can start.  A new template instantiation needs a case in tests/test_gpu_ops.py that
# reaches it, and its name here.
INSTANTIATIONS = sorted(
    [f"conv1d_small_kernel<{a}, {r}>" for a in (0, 1, 2) for r in ("false", "true")]
    + [f"conv1d_mfma_kernel<{n}, float, true, 32, {f}>" for n in (1, 2, 4) for f in ("false", "true")]
    + [f"conv1d_mfma_kernel<{n}, float, false, 32, false>" for n in (1, 2)]
    + [f"conv1d_mfma_kernel<{n}, unsigned char, false, 32, false>" for n in (1, 2)]
    + [f"conv1d_wino{s}_kernel<{m}, {a}, {r}, false>" for s in ("", "_small") for m in (2, 3) for a in (0, 1, 2)
       for r in ("false", "true")]
    + [f"conv1d_wino{s}_kernel<{m}, 1, false, true>" for s in ("", "_small") for m in (2, 3)]
    + ["maxpool_kernel", "segsum_kernel", "mix_kernel<false>", "mix_kernel<true>", "head_kernel", "concat_kernel", "add_kernel",
       "layernorm_kernel"])

_ELEMENTWISE = {cp.OP_MAXPOOL: "maxpool_kernel", cp.OP_SEGSUM: "segsum_kernel", cp.OP_HEAD: "head_kernel",
                cp.OP_CONCAT: "concat_kernel", cp.OP_ADD: "add_kernel", cp.OP_LAYERNORM: "layernorm_kernel"}


def _b(x: bool) -> str:
    return "true" if x else "false"


def instantiation(o: cp.Op, rows: int, cus: int) -> str:
    """The kernel instantiation op ``o`` launches over ``rows`` rows of its domain on a device of ``cus`` compute units."""
    if o.kind == cp.OP_MIX:
        return f"mix_kernel<{_b(bool(o.flags & cp.FLAG_MIX_REST))}>"
    if o.kind != cp.OP_CONV1D:
        return _ELEMENTWISE[o.kind]
    groups = o.c1 if o.c1 > 1 else 1
    cin, cin_stride = o.cin // groups, o.cin
    act = 1 if o.flags & cp.FLAG_RELU else (2 if o.flags & cp.FLAG_SOFTPLUS else 0)
    res = o.res != cp.BUF_NONE
    m_total = rows * o.lout
    if o.flags & cp.FLAG_WINOGRAD:                                     # launch_conv1d_wino
        m = 3 if o.lin % 3 == 0 else 2
        tiles = rows * -(-o.lin // m)
        big = -(-tiles // 64) * (o.cout // 64)
        if o.src1 != cp.BUF_NONE:
            small = big * 4 <= cus and m_total * o.cin * 4 < 2 ** 31
            return f"conv1d_wino{'_small' if small else ''}_kernel<{m}, 1, false, true>"
        small = big * 4 <= cus and cin % 16 == 0 and m_total * cin_stride * 4 < 2 ** 31
        return f"conv1d_wino{'_small' if small else ''}_kernel<{m}, {act}, {_b(res)}, false>"
    u8 = bool(o.flags & cp.FLAG_SRC_U8)                                # launch_conv1d
    gx = -(-m_total // 128)
    cout_pad = -(-o.cout // 32) * 32
    two = cout_pad % 64 == 0
    vec = not u8 and cin % 4 == 0
    big = gx * (cout_pad // (128 if vec and cout_pad % 128 == 0 else (64 if two else 32)))
    act_bytes = rows * o.lin * cin_stride * 4
    if not u8 and cin % 16 == 0 and o.cout % 16 == 0 and big * 4 <= cus and act_bytes < 2 ** 31:
        return f"conv1d_small_kernel<{act}, {_b(res)}>"
    ncb = 4 if vec and cout_pad % 128 == 0 else (2 if two else 1)
    kpad = -(-(o.k * cin) // 32) * 32
    span = (128 // o.lout + 2) * o.lin * cin_stride * 4                # launch_kc: a workgroup's bytes in a 32-bit offset
    fast = vec and cin % 32 == 0 and kpad == o.k * cin and span < 2 ** 30
    return f"conv1d_mfma_kernel<{ncb}, {'unsigned char' if u8 else 'float'}, {_b(vec)}, 32, {_b(fast)}>"


# ---- Winograd transforms (conv_wino.hip header) and the bound's weights W_u[j, t] -----------------------------------------
# V = B d (rows: components, columns: tile inputs d_t), U = G g (columns: filter taps g_j), y_u = sum_c A[u, c] U_c V_c
WINO = {
    2: dict(B=np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], float),
            G=np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], float),
            A=np.array([[1, 1, 1, 0], [0, 1, -1, -1]], float)),
    3: dict(B=np.array([[2, -1, -2, 1, 0], [0, -2, -1, 1, 0], [0, 2, -3, 1, 0], [0, -1, 0, 1, 0], [0, 2, -1, -2, 1]], float),
            G=np.array([[.5, 0, 0], [-.5, -.5, -.5], [-1 / 6, 1 / 6, -1 / 6], [1 / 6, 2 / 6, 4 / 6], [0, 0, 1]], float),
            A=np.array([[1, 1, 1, 1, 0], [0, 1, -1, 2, 0], [0, 1, 1, 4, 1]], float)),
}


def wino_bound_weights(m: int) -> np.ndarray:
    """W[u, j, t] = sum_c |A_uc| |G_cj| |B_ct|: how much of |g_j| |d_t| output u of an F(m,3) tile can carry in rounding."""
    t = WINO[m]
    return np.einsum("uc,cj,ct->ujt", np.abs(t["A"]), np.abs(t["G"]), np.abs(t["B"]))


# ---- float64 references -------------------------------------------------------------------------------------------------
def _windows(x: np.ndarray, positions: np.ndarray, taps: int) -> np.ndarray:
    """x [rows, lin, c] -> [rows, len(positions), taps, c] of x at positions[p] + tap (zero outside the row)."""
    lin = x.shape[1]
    idx = positions[:, None] + np.arange(taps)[None, :]
    ok = (idx >= 0) & (idx < lin)
    g = x[:, np.clip(idx, 0, lin - 1)]
    return g * ok[None, :, :, None]


def softplus(x):
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def activation(x, act: str, mutation: Optional[str] = None):
    if act == "relu":
        return np.maximum(x, 0.0)
    if act == "softplus":
        if mutation == "softplus_sign":            # planted bug: threshold on the wrong sign
            return np.where(x < -20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))
        return softplus(x)
    return x


def conv_reference(x, w, b, stride, pad, groups=1, act="none", res=None, wino_m=0, mutation=None, dtype=np.float64):
    """Conv1d (+bias, activation, + residual after the activation) of x [rows, lin, cin] with w [cout, cin/groups, k]:
    -> (out [rows, lout, cout], per-element bound).  ``mutation`` plants one bug (tests of the bound itself); ``dtype``
    float32 evaluates the same sums in float32 in another order."""
    rows, lin, cin = x.shape
    cout, cg, k = w.shape
    lout = (lin + 2 * pad - k) // stride + 1
    og = cout // groups
    x = x.astype(np.float64)
    w = w.astype(np.float64)
    b = b.astype(np.float64).copy()
    if mutation == "bias0_missing":
        b[0] = 0
    if mutation == "bias_last_missing":
        b[-1] = 0
    if mutation == "drop_last_channel":
        x = x.copy()
        x[..., -1] = 0
    starts = np.arange(lout) * stride - pad
    if mutation == "tap_shift":
        starts = starts + 1
    if mutation == "pad_wrong_side":
        starts = starts + pad                      # all padding on the right
    pre = np.empty((rows, lout, cout))
    mag = np.empty((rows, lout, cout))
    for g in range(groups):
        src = (g + 1) % groups if mutation == "group_swap" else g
        xs = x[..., src * cg:(src + 1) * cg]
        cols = _windows(xs, starts, k).reshape(rows * lout, k * cg)             # K index = tap * cg + c
        wg = w[g * og:(g + 1) * og].transpose(0, 2, 1).reshape(og, k * cg)
        if dtype == np.float32:
            p = (cols[:, ::-1].astype(np.float32) @ wg[:, ::-1].T.astype(np.float32)).astype(np.float64)
        else:
            p = cols @ wg.T
        pre[..., g * og:(g + 1) * og] = p.reshape(rows, lout, og)
        if wino_m:
            mag[..., g * og:(g + 1) * og] = _wino_magnitude(np.abs(x[..., g * cg:(g + 1) * cg]), np.abs(w[g * og:(g + 1) * og]), wino_m)
        else:
            mag[..., g * og:(g + 1) * og] = (np.abs(cols) @ np.abs(wg).T).reshape(rows, lout, og)
    pre += b
    if dtype == np.float32:
        pre = pre.astype(np.float32).astype(np.float64)
    out = activation(pre, act, mutation)
    bound = (C_WINO if wino_m else C_ACC) * U * (mag + np.abs(b))
    if act == "softplus":
        bound = bound + C_SP * U * (1 + np.abs(pre) + np.abs(out))
    if res is not None:
        out = (activation(pre + res, act) if mutation == "res_before_act" else out + res)
    return out, bound + U * np.abs(out)


def _wino_magnitude(ax, aw, m):
    """sum_ch sum_{j,t} W_u[j, t] |g_ch,j| |d_ch,t| for every output (k3 / s1 / p1, tiles of m outputs)."""
    rows, lin, cg = ax.shape
    wts = wino_bound_weights(m)                                  # [m, 3, m + 2]
    p = np.arange(lin)
    d = _windows(ax, m * (p // m) - 1, m + 2)                    # [rows, lin, T, cg]: the inputs of each position's tile
    e = np.einsum("pjt,rptc->rpjc", wts[p % m], d)               # [rows, lin, 3, cg]
    return (e.reshape(rows * lin, 3 * cg) @ aw.transpose(2, 1, 0).reshape(3 * cg, -1)).reshape(rows, lin, -1)


def maxpool_reference(x, k, stride, pad):
    rows, lin, c = x.shape
    lout = (lin + 2 * pad - k) // stride + 1
    idx = (np.arange(lout) * stride - pad)[:, None] + np.arange(k)[None, :]
    ok = (idx >= 0) & (idx < lin)
    g = np.where(ok[None, :, :, None], x[:, np.clip(idx, 0, lin - 1)], -np.inf)     # padding never wins
    return g.max(axis=2)


def layernorm_reference(x, gamma, beta, eps, act, res=None):
    x = x.astype(np.float64)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    sd = np.sqrt(var + eps)
    xh = (x - mean) / sd
    pre = xh * gamma + beta
    out = activation(pre, act)
    # mean and variance carry C_ACC u of the channels' magnitude; normalised, that is mean|x| / sd per unit of |xh| + 1
    bound = C_ACC * U * (np.abs(gamma) * (1 + np.abs(xh)) * (np.abs(x).mean(-1, keepdims=True) / sd) + np.abs(gamma * xh) + np.abs(beta))
    if act == "softplus":
        bound = bound + C_SP * U * (1 + np.abs(pre) + np.abs(out))
    if res is not None:
        out = out + res
    return out, bound + U * np.abs(out)


def head_reference(x, w, b, softmax):
    """x [rows, lin, cin] -> (y [rows, cout], bound)."""
    pooled = x.astype(np.float64).mean(1)
    y = pooled @ w.T.astype(np.float64) + b
    bound = C_ACC * U * (np.abs(x).mean(1) @ np.abs(w.T).astype(np.float64) + np.abs(b)) + U * np.abs(y)
    if softmax:
        e = np.exp(y - y.max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
        return p, p * (2 * bound.max(1, keepdims=True) + 4 * U) + U * p
    return y, bound


def segsum_reference(x, off):
    """x [rows, f] summed over the segments [off[s], off[s + 1])."""
    c = np.concatenate([np.zeros((1, x.shape[1])), np.cumsum(x.astype(np.float64), 0)])
    ca = np.concatenate([np.zeros((1, x.shape[1])), np.cumsum(np.abs(x.astype(np.float64)), 0)])
    out = c[off[1:]] - c[off[:-1]]
    mag = ca[off[1:]] - ca[off[:-1]]
    return out, C_ACC * U * mag + U * np.abs(out)


# ---- programs -----------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """One subject op.  kind: conv | maxpool | segsum | mix | head | concat | add | layernorm."""
    id: str
    kind: str
    p: Dict = field(default_factory=dict)

    def get(self, key, default=None):
        return self.p.get(key, default)


@dataclass
class Built:
    program: cp.Program
    reads0: np.ndarray
    rpa: np.ndarray
    aps: np.ndarray
    subject: int                              # op index of the subject
    inputs: Dict[str, int]                    # "src0" / "src1" / "res" -> op index of the producer
    params: Dict                              # weights and what the reference needs
    rows: int                                 # rows of the subject's domain


class _Builder:
    def __init__(self, window, channels0, rng):
        self.window, self.c0, self.rng = window, channels0, rng
        self.ops: List[cp.Op] = []
        self.buffers: List[Tuple[int, int]] = [(0, 0)] * cp.BUF_FIRST_SCRATCH
        self.blob = cp._WeightBlob()

    def buffer(self, domain, floats):
        self.buffers.append((domain, int(floats)))
        return len(self.buffers) - 1

    def add(self, op):
        self.ops.append(op)
        return len(self.ops) - 1

    def input_conv(self, floats, offset=0.0):
        """k=1 conv from the bytes to READS0 rows of >= ``floats`` floats: -> (op index, buffer)."""
        cx = max(4, -(-(-(-floats // self.window)) // 4) * 4)
        w = self.rng.standard_normal((cx, self.c0, 1)) * (2.0 / (255 * math.sqrt(self.c0)))
        b = offset + self.rng.standard_normal(cx) * 0.5
        packed, bias = cp.pack_conv(w.astype(np.float32), b.astype(np.float32))
        buf = self.buffer(cp.ROWS_READS0, self.window * cx)
        i = self.add(cp.Op(cp.OP_CONV1D, cp.ROWS_READS0, src0=cp.BUF_READS0, dst=buf, cin=self.c0, cout=cx, k=1, stride=1, pad=0,
                           lin=self.window, lout=self.window, flags=cp.FLAG_SRC_U8, w_off=self.blob.add(packed),
                           b_off=self.blob.add(bias)))
        return i, buf

    def source(self, domain, floats, offset=0.0):
        """Float rows of ``domain`` holding >= ``floats`` floats: -> (op index of the producer, buffer)."""
        i, buf = self.input_conv(floats, offset)
        f = self.buffers[buf][1]
        if domain in (cp.ROWS_ALLELES, cp.ROWS_SITES):
            i, buf = self.segsum(buf, cp.SEG_R0A, f)
        if domain == cp.ROWS_SITES:
            i, buf = self.segsum(buf, cp.SEG_AS, f)
        return i, buf

    def segsum(self, src, seg, floats):
        dom = cp.ROWS_SITES if seg == cp.SEG_AS else cp.ROWS_ALLELES
        buf = self.buffer(dom, floats)
        return self.add(cp.Op(cp.OP_SEGSUM, dom, src0=src, dst=buf, cin=floats, lin=1, lout=1, seg=seg)), buf

    def finish(self, n_experts=1, has_meta=False):
        # the closing HEAD: logit slot 0 from an ALLELES buffer
        alle = [j for j in range(cp.BUF_FIRST_SCRATCH, len(self.buffers)) if self.buffers[j][0] == cp.ROWS_ALLELES]
        if not alle:
            _, alle_buf = self.segsum(self.ops[0].dst, cp.SEG_R0A, self.buffers[self.ops[0].dst][1])
            alle = [alle_buf]
        f = self.buffers[alle[0]][1]
        w = self.rng.standard_normal((1, f)).astype(np.float32)
        self.add(cp.Op(cp.OP_HEAD, cp.ROWS_ALLELES, src0=alle[0], dst=0, cin=f, cout=1, lin=1, lout=1,
                       w_off=self.blob.add(w), b_off=self.blob.add(np.zeros(1, np.float32))))
        return cp.Program(spec_name="op_case", window=self.window, channels0=self.c0, channels1=0, n_experts=n_experts,
                          has_meta=has_meta, uses_ref=False, ops=self.ops, buffers=self.buffers, weights=self.blob.finish())


def batch_for(domain, rows, rng, reads_per_allele=None):
    """(reads per allele [A], alleles per site [S]) whose ``domain`` has ``rows`` rows."""
    if domain == cp.ROWS_READS0:
        a = max(1, min(rows, 4))
        rpa = np.full(a, rows // a, np.int32)
        rpa[: rows % a] += 1
        return rpa, np.array([a], np.int32)
    if domain == cp.ROWS_ALLELES:
        rpa = np.full(rows, reads_per_allele or 1, np.int32) if reads_per_allele else rng.integers(1, 4, rows).astype(np.int32)
        aps = np.full(-(-rows // 2), 2, np.int32)
        aps[-1] = rows - 2 * (len(aps) - 1)
        return rpa, aps
    aps = rng.integers(1, 3, rows).astype(np.int32)
    return np.ones(int(aps.sum()), np.int32), aps


def _domain_rows(domain, rpa, aps):
    return {cp.ROWS_READS0: int(rpa.sum()), cp.ROWS_ALLELES: len(rpa), cp.ROWS_SITES: len(aps)}[domain]


def build(case: Case, rows: int, seed: int = 0) -> Built:
    """The program isolating ``case``'s subject over ``rows`` rows of its domain, with its batch."""
    rng = np.random.default_rng(seed)
    p = case.p
    domain = p.get("domain", cp.ROWS_READS0)
    if case.kind == "head":
        domain = cp.ROWS_SITES if p["cout"] > 1 else cp.ROWS_ALLELES
    elif case.kind == "mix" or (case.kind == "segsum" and p.get("seg", cp.SEG_R0A) == cp.SEG_R0A):
        domain = cp.ROWS_ALLELES
    elif case.kind == "segsum":
        domain = cp.ROWS_SITES
    rpa, aps = batch_for(domain, rows, rng, p.get("reads_per_allele"))
    u8 = p.get("u8", False)
    c0 = p["cin"] if u8 else p.get("c0", 6)
    lin = p.get("lin", 1)
    window = lin if u8 else p.get("window", 8)
    bld = _Builder(window, c0, rng)
    inputs: Dict[str, int] = {}
    params: Dict = {}
    cin = p.get("cin", 4)
    kind = case.kind
    n_experts, has_meta = 1, False
    if kind == "conv":
        k, stride, pad, cout, groups = p.get("k", 3), p.get("stride", 1), p.get("pad", 0), p["cout"], p.get("groups", 1)
        wino, seg = p.get("wino", False), p.get("seg", 0)
        lout = (lin + 2 * pad - k) // stride + 1
        scale = p.get("w_scale", 1.0) / math.sqrt(k * cin / groups)
        w = (rng.standard_normal((cout, cin // groups, k)) * scale).astype(np.float32)
        if u8:
            w = (w / 128).astype(np.float32)
        b = (rng.choice([-1, 1], cout) * rng.uniform(0.5, 1.5, cout) * p.get("b_scale", 1.0)).astype(np.float32)
        if u8:
            src0, src1 = cp.BUF_READS0, cp.BUF_NONE
        elif seg:
            inputs["src0"], src0 = bld.source(domain, lin * seg)
            inputs["src1"], src1 = bld.source(domain, lin * (cin - seg))
        else:
            inputs["src0"], src0 = bld.source(domain, lin * cin)
            src1 = cp.BUF_NONE
        res = cp.BUF_NONE
        if p.get("res"):
            inputs["res"], res = bld.source(domain, lout * cout)
        if wino:
            packed, bias = cp.pack_conv_winograd(w, b, lin)
        else:
            packed, bias = cp.pack_conv(w, b, groups, expand=groups == 1)
        dst = bld.buffer(domain, lout * cout)
        flags = ACTS[p.get("act", "none")] | (cp.FLAG_WINOGRAD if wino else 0) | (cp.FLAG_SRC_U8 if u8 else 0)
        op = cp.Op(cp.OP_CONV1D, domain, src0=src0, src1=src1, dst=dst, res=res, cin=cin, cout=cout, k=k, stride=stride, pad=pad,
                   lin=lin, lout=lout, flags=flags, seg=seg, c1=groups if groups > 1 else 0, w_off=bld.blob.add(packed),
                   b_off=bld.blob.add(bias))
        params.update(w=w, b=b, lout=lout)
    elif kind == "maxpool":
        k, stride, pad = p["k"], p["stride"], p["pad"]
        lout = (lin + 2 * pad - k) // stride + 1
        inputs["src0"], src0 = bld.source(domain, lin * cin)
        dst = bld.buffer(domain, lout * cin)
        op = cp.Op(cp.OP_MAXPOOL, domain, src0=src0, dst=dst, cin=cin, cout=cin, k=k, stride=stride, pad=pad, lin=lin, lout=lout)
    elif kind == "segsum":
        seg = p.get("seg", cp.SEG_R0A)
        src_dom = cp.ROWS_READS0 if seg == cp.SEG_R0A else cp.ROWS_ALLELES
        inputs["src0"], src0 = bld.source(src_dom, lin * cin)
        dom = cp.ROWS_SITES if seg == cp.SEG_AS else cp.ROWS_ALLELES
        dst = bld.buffer(dom, lin * cin)
        op = cp.Op(cp.OP_SEGSUM, dom, src0=src0, dst=dst, cin=cin, lin=lin, lout=lin, seg=seg)
    elif kind == "mix":
        inputs["src0"], src0 = bld.source(cp.ROWS_ALLELES, lin * cin)
        inputs["src1"], src1 = bld.source(cp.ROWS_SITES, lin * cin)
        dst = bld.buffer(cp.ROWS_ALLELES, lin * cin)
        rest = p.get("rest", False)
        op = cp.Op(cp.OP_MIX, cp.ROWS_ALLELES, src0=src0, src1=src1, dst=dst, cin=cin, lin=lin, lout=lin, seg=cp.SEG_AS,
                   a0=p.get("a0", 0.0), a1=p.get("a1", 0.0), flags=cp.FLAG_MIX_REST if rest else 0)
    elif kind in ("concat", "add"):
        c1 = p.get("c1", cin)
        inputs["src0"], src0 = bld.source(domain, lin * cin)
        inputs["src1"], src1 = bld.source(domain, lin * c1)
        if kind == "concat":
            dst = bld.buffer(domain, lin * (cin + c1))
            op = cp.Op(cp.OP_CONCAT, domain, src0=src0, src1=src1, dst=dst, cin=cin, c1=c1, lin=lin, lout=lin)
        else:
            dst = bld.buffer(domain, lin * cin)
            op = cp.Op(cp.OP_ADD, domain, src0=src0, src1=src1, dst=dst, cin=cin, lin=lin, lout=lin)
    elif kind == "layernorm":
        inputs["src0"], src0 = bld.source(domain, lin * cin, offset=p.get("offset", 0.0))
        res = cp.BUF_NONE
        if p.get("res"):
            inputs["res"], res = bld.source(domain, lin * cin)
        gamma = rng.uniform(0.5, 1.5, cin).astype(np.float32)
        beta = rng.standard_normal(cin).astype(np.float32)
        dst = bld.buffer(domain, lin * cin)
        op = cp.Op(cp.OP_LAYERNORM, domain, src0=src0, dst=dst, res=res, cin=cin, cout=cin, lin=lin, lout=lin,
                   flags=ACTS[p.get("act", "none")], a0=1e-5, w_off=bld.blob.add(gamma), b_off=bld.blob.add(beta))
        params.update(gamma=gamma, beta=beta, eps=np.float32(1e-5))
    elif kind == "head":
        cout, softmax = p["cout"], p.get("softmax", False)
        meta = cout > 1
        hdom = cp.ROWS_SITES if meta else cp.ROWS_ALLELES
        inputs["src0"], src0 = bld.source(hdom, lin * cin)
        w = (rng.standard_normal((cout, cin)) / math.sqrt(cin)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        op = cp.Op(cp.OP_HEAD, hdom, src0=src0, dst=3 if meta else 0, cin=cin, cout=cout, lin=lin, lout=1,
                   flags=cp.FLAG_SOFTMAX if softmax else 0, w_off=bld.blob.add(w), b_off=bld.blob.add(b))
        params.update(w=w, b=b)
        has_meta = meta
    else:
        raise ValueError(kind)
    subject = bld.add(op)
    if kind == "head" and not has_meta:
        prog = cp.Program(spec_name="op_case", window=window, channels0=c0, channels1=0, n_experts=1, has_meta=False,
                          uses_ref=False, ops=bld.ops, buffers=bld.buffers, weights=bld.blob.finish())
    else:
        prog = bld.finish(n_experts, has_meta)
    n_reads = int(rpa.sum())
    reads0 = rng.integers(0, 256, (n_reads, window, c0), dtype=np.uint8)
    return Built(prog, reads0, rpa, aps, subject, inputs, params, _domain_rows(op.domain, rpa, aps))


# ---- running a case and checking it ---------------------------------------------------------------------------------------
def capture(engine, built: Built, op_index: int) -> np.ndarray:
    """Flat float32 output of op ``op_index`` (one forward; the program and its inputs are deterministic)."""
    engine.capture_op_output(op_index)
    engine.forward(built.reads0, built.rpa, built.aps)
    return engine.read_op_output()


def reference(built: Built, got_inputs: Dict[str, np.ndarray], case: Case):
    """-> (reference, bound) of the subject, from the captured inputs (float64)."""
    p, o = case.p, built.program.ops[built.subject]
    rows = built.rows

    def rows_of(name, per_row, count=rows):
        return got_inputs[name][: count * per_row].astype(np.float64).reshape(count, -1)

    if case.kind == "conv":
        if o.flags & cp.FLAG_SRC_U8:
            x = built.reads0.astype(np.float64)
        elif o.src1 != cp.BUF_NONE:
            x = np.concatenate([rows_of("src0", o.lin * o.seg).reshape(rows, o.lin, o.seg),
                                rows_of("src1", o.lin * (o.cin - o.seg)).reshape(rows, o.lin, o.cin - o.seg)], axis=2)
        else:
            x = rows_of("src0", o.lin * o.cin).reshape(rows, o.lin, o.cin)
        res = rows_of("res", o.lout * o.cout).reshape(rows, o.lout, o.cout) if "res" in got_inputs else None
        wino_m = cp.winograd_outputs_per_tile(o.lin) if o.flags & cp.FLAG_WINOGRAD else 0
        return conv_reference(x, built.params["w"], built.params["b"], o.stride, o.pad, max(o.c1, 1), p.get("act", "none"), res,
                              wino_m)
    if case.kind == "maxpool":
        x = rows_of("src0", o.lin * o.cin).reshape(rows, o.lin, o.cin)
        out = maxpool_reference(x, o.k, o.stride, o.pad)
        return out, np.zeros_like(out)
    if case.kind == "segsum":
        src_rows = int(built.rpa.sum()) if o.seg == cp.SEG_R0A else len(built.rpa)
        counts = built.rpa if o.seg == cp.SEG_R0A else built.aps
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return segsum_reference(rows_of("src0", o.lin * o.cin, src_rows), off)
    if case.kind == "mix":
        x = rows_of("src0", o.lin * o.cin)
        s = rows_of("src1", o.lin * o.cin, len(built.aps))[np.repeat(np.arange(len(built.aps)), built.aps)]
        if o.flags & cp.FLAG_MIX_REST:
            out = x - (s - x)
            return out, 4 * U * (2 * np.abs(x) + np.abs(s))
        out = np.float64(o.a0) * x + np.float64(o.a1) * s
        return out, 4 * U * (np.abs(o.a0 * x) + np.abs(o.a1 * s))
    if case.kind == "concat":
        a = rows_of("src0", o.lin * o.cin).reshape(rows, o.lin, o.cin)
        b = rows_of("src1", o.lin * o.c1).reshape(rows, o.lin, o.c1)
        out = np.concatenate([a, b], axis=2)
        return out, np.zeros_like(out)
    if case.kind == "add":
        a, b = rows_of("src0", o.lin * o.cin), rows_of("src1", o.lin * o.cin)
        return a + b, 2 * U * (np.abs(a) + np.abs(b))
    if case.kind == "layernorm":
        x = rows_of("src0", o.lin * o.cin).reshape(rows, o.lin, o.cin)
        res = rows_of("res", o.lin * o.cin).reshape(rows, o.lin, o.cin) if "res" in got_inputs else None
        return layernorm_reference(x, built.params["gamma"].astype(np.float64), built.params["beta"].astype(np.float64),
                                   float(built.params["eps"]), p.get("act", "none"), res)
    if case.kind == "head":
        x = rows_of("src0", o.lin * o.cin).reshape(rows, o.lin, o.cin)
        return head_reference(x, built.params["w"], built.params["b"].astype(np.float64), bool(o.flags & cp.FLAG_SOFTMAX))
    raise ValueError(case.kind)


def excess(got, ref, bound) -> Tuple[float, int]:
    """(largest |got - ref| / bound, number of elements over their bound); exact elements (bound 0) must match exactly."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    return float(ratio.max()) if ratio.size else 0.0, int(bad.sum())


# ---- the case table -------------------------------------------------------------------------------------------------------
def _conv(id_, **p):
    return Case(id_, "conv", p)


CASES: List[Case] = (
    # generic conv, float input: cin across the vector / FAST / small branches, 128 output channels (NCB = 4)
    [_conv(f"gen_cin{c}", cin=c, cout=128, k=3, pad=1, lin=37, act="relu") for c in (4, 12, 16, 32, 48, 64, 256)]
    # cout leaving padded lanes in the last channel block (4 -> 32, 36 -> 64, 100 -> 128), with a residual off the FAST path
    + [_conv(f"gen_cout{c}_cin{ci}", cin=ci, cout=c, k=5, stride=2, pad=2, lin=129, act="none", res=True)
       for c in (4, 36, 100, 128) for ci in (12, 32)]
    # kernel sizes, strides, paddings and output lengths (1, 2, 37, 127, 128, 129, 300); lout 1 and 2 put many rows in a tile
    + [_conv("gen_k1_s1_lout300", cin=64, cout=64, k=1, lin=300, act="relu"),
       _conv("gen_k2_s2_p1_lout128", cin=16, cout=32, k=2, stride=2, pad=1, lin=255, act="relu"),
       _conv("gen_k7_s3_p3_lout127", cin=32, cout=64, k=7, stride=3, pad=3, lin=380, act="softplus"),
       _conv("gen_k5_s1_p2_lout129", cin=48, cout=128, k=5, pad=2, lin=129, act="relu", res=True),
       _conv("gen_k3_s2_p0_lout1", cin=64, cout=64, k=3, stride=2, lin=3),
       _conv("gen_k3_s1_p0_lout2", cin=32, cout=32, k=3, lin=4, act="relu"),
       _conv("gen_k7_s1_p3_cin256", cin=256, cout=128, k=7, pad=3, lin=37, act="relu"),
       _conv("gen_k2_s3_p0_lout37", cin=4, cout=20, k=2, stride=3, lin=110, act="softplus", res=True)]
    # every activation with and without a residual (small kernel and both FAST / non-FAST large ones)
    + [_conv(f"gen_{a}_res{int(r)}_cin{c}", cin=c, cout=64, k=3, pad=1, lin=37, act=a, res=r, w_scale=8.0)
       for a in ("none", "relu", "softplus") for r in (False, True) for c in (64, 48)]
    # grouped, by group
    + [_conv("gen_groups2", cin=64, cout=256, k=3, pad=1, lin=18, groups=2, act="relu"),
       _conv("gen_groups4", cin=64, cout=512, k=1, lin=9, groups=4, res=True, act="softplus")]
    # uint8 input from the bytes (the window is the row): every channel count and NCB = 1 / 2
    + [_conv(f"u8_cin{c}_cout{co}", u8=True, cin=c, cout=co, k=3, pad=1, lin=37, act="relu") for c in (5, 6, 7)
       for co in (16, 20, 64, 128)]
    + [_conv("u8_k7_s2_p3_softplus_res", u8=True, cin=6, cout=64, k=7, stride=2, pad=3, lin=41, act="softplus", res=True)]
    # float rows of 6 channels (the non-vector gather): the subject reads a producer's output as [10][6]
    + [_conv(f"gen_cin6_cout{co}", cin=6, cout=co, k=3, pad=1, lin=10, act="relu") for co in (20, 64)]
    # one row too long for the FAST path's 32-bit span (2^30 bytes for a workgroup's rows)
    + [_conv("gen_span_over_2e30", cin=32, cout=4, k=1, stride=70000, lin=70000, window=2240, large=False)]
    # Winograd: F(2,3) (row length not a multiple of 3) and F(3,3) times every activation, with and without a residual
    + [_conv(f"wino_f{m}_{a}_res{int(r)}", wino=True, cin=64, cout=64, k=3, pad=1, lin=71 if m == 2 else 150, act=a, res=r,
             w_scale=8.0) for m in (2, 3) for a in ("none", "relu", "softplus") for r in (False, True)]
    + [_conv(f"wino_cin{c}", wino=True, cin=c, cout=64, k=3, pad=1, lin=9, act="relu") for c in (8, 24, 40, 16, 48)]
    + [_conv("wino_cout192", wino=True, cin=64, cout=192, k=3, pad=1, lin=5, act="relu", res=True)]
    + [_conv(f"wino_lin{n}", wino=True, cin=32, cout=64, k=3, pad=1, lin=n, act="relu") for n in (1, 2, 3, 4, 5, 9, 71, 150)]
    + [_conv(f"wino_groups2_lin{n}", wino=True, cin=64, cout=256, k=3, pad=1, lin=n, groups=2, act="relu") for n in (18, 10)]
    # two-source (a CONCAT folded in): seg at both ends of its range
    + [_conv(f"wino_two_seg{s}_lin{n}", wino=True, cin=64, seg=s, cout=64, k=3, pad=1, lin=n, act="relu")
       for s in (16, 48) for n in (18, 10)]
    # elementwise
    + [Case(f"maxpool_k{k}_s{s}_p{p}_lin{n}_c{c}", "maxpool", dict(k=k, stride=s, pad=p, lin=n, cin=c))
       for k, s, p, n, c in ((3, 2, 1, 37, 4), (2, 1, 0, 9, 12), (3, 3, 1, 71, 32), (2, 2, 1, 5, 8), (3, 1, 0, 3, 4),
                             (3, 2, 0, 71, 32))]
    + [Case("segsum_reads_1", "segsum", dict(lin=5, cin=12, reads_per_allele=1)),
       Case("segsum_reads_1000", "segsum", dict(lin=3, cin=8, reads_per_allele=1000, rows=2, large_rows=9)),
       Case("segsum_70001_segments", "segsum", dict(lin=1, cin=4, window=1, reads_per_allele=1, rows=70001, large=False)),
       Case("segsum_sites", "segsum", dict(seg=cp.SEG_AS, lin=9, cin=16))]
    + [Case("mix_2_m1", "mix", dict(lin=9, cin=16, a0=2.0, a1=-1.0)),
       Case("mix_075_m125", "mix", dict(lin=7, cin=12, a0=0.75, a1=-1.25)),
       Case("mix_rest", "mix", dict(lin=9, cin=16, rest=True))]
    + [Case(f"head_cout{co}_sm{int(sm)}_cin{c}", "head", dict(cout=co, softmax=sm, cin=c, lin=n))
       for co, c, n in ((1, 100, 37), (2, 1024, 5), (3, 256, 9)) for sm in (False, True)]
    + [Case(f"layernorm_c{c}_{a}_res{int(r)}", "layernorm", dict(cin=c, lin=5, act=a, res=r, offset=1e3 if c >= 100 else 0.0))
       for c in (4, 100, 500, 512) for a, r in (("none", False), ("relu", True), ("softplus", False))]
    + [Case("concat", "concat", dict(lin=7, cin=8, c1=12)), Case("add", "add", dict(lin=7, cin=12))]
)


def _large(o: cp.Op, rows: int, cus: int) -> bool:
    """The launch is past every small-launch branch (as if it were eligible for one)."""
    if o.kind == cp.OP_CONV1D:
        if o.flags & cp.FLAG_WINOGRAD:
            m = 3 if o.lin % 3 == 0 else 2
            return -(-(rows * -(-o.lin // m)) // 64) * (o.cout // 64) * 4 > cus
        cout_pad = -(-o.cout // 32) * 32
        return -(-(rows * o.lout) // 128) * (cout_pad // 128 if cout_pad % 128 == 0 else max(1, cout_pad // 64)) * 4 > cus
    return rows * o.lout * max(o.cin, 4) // 4 > 256 * cus            # the grid-stride kernels' grid is full


def rows_for(case: Case, size: str, cus: int) -> int:
    """Rows of the subject's domain for the ``size`` ("small" | "large") launch of ``case``."""
    small = case.get("rows", 3)
    if size == "small" or case.get("large", True) is False:
        return small
    if case.get("large_rows"):
        return case.get("large_rows")
    rows = 4
    b = build(case, 3)
    subject = b.program.ops[b.subject]
    while not _large(subject, rows, cus) and rows < 1 << 16:
        rows *= 2
    return rows


def case_instantiations(cus: int) -> Dict[str, List[str]]:
    """instantiation -> ids of the launches (case, size) that reach it."""
    out: Dict[str, List[str]] = {}
    for case in CASES:
        for size in ("small", "large"):
            rows = rows_for(case, size, cus)
            b = build(case, rows) if case.kind == "conv" else None
            o = b.program.ops[b.subject] if b else _subject_op(case)
            out.setdefault(instantiation(o, rows, cus), []).append(f"{case.id}[{size}]")
    return out


def _subject_op(case: Case) -> cp.Op:
    b = build(case, case.get("rows", 3))
    return b.program.ops[b.subject]
