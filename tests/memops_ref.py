"""float64 references, with a derived error limit per output element, of the memory-bound kernels that sit between the
convolutions of every inference and streaming program  (TEST INFRASTRUCTURE; numpy only):

    csrc/norm.hip        eab_in_finalize_f32 / _mr_f32, eab_norm_act_f32 / eab_norm_act_win_f32
    csrc/filter_sum.hip  eab_filter_sum_f32, eab_bfw_filter_sum_f32 / _win_f32, eab_mlp_bfw_filter_sum_f32
    csrc/cln.hip         eab_cln_stats_f32, eab_cln_apply_f32, eab_cln_step_f32, eab_gate_rows_f32
    csrc/program.hip     eab_zero_rows_f32

Every function takes named arrays and a dtype and returns {output: (val, lim[, must[, may]])} like train_ref.run_ref: dtype
float64 is the reference, dtype float32 the YARDSTICK of the statistical criterion (every array and operation in fp32, sums
sequential, contractions as fp32 matrix products).  What the training walk already states -- IN_FINALIZE, FILTER_SUM, CLN_STATS,
CLN_APPLY, GATE_FWD -- is train_ref's, reached through train_ref.run_ref; here are only the forms inference alone has.

LIMITS are derived, never measured (u = 2^-24, train_ref's rules):
  norm_act   per operand max(1, |slope|) 2u (|a s| + |h|) + u |y| -- PReLU is Lipschitz with constant max(1, |slope|), so an
             element at the kink needs no exclusion band and none is left out -- plus u |out| for the sum of two operands
  bfw        y1 = relu(h W1^T + b1):  e1 = (64 + 2) u (|h| |W1|^T + |b1|)            (ReLU: Lipschitz 1)
             w  = y1 W2^T + b2:       ew = (64 + 2) u (|y1| |W2|^T + |b2|) + e1 |W2|^T
             out = sum_m w_m x_m:     (2M + 2) u sum |w||x| + sum ew |x|             (real and imaginary part alike)
  state      the cLN running sums are doubles: the limits of the frame sums, added up
MASKS.  must = the elements a launch has to write (and the check compares), may = those it is allowed to write (default:
must).  Everything outside may has to keep its bits (judge).  Rows behind a per-utterance length are exact zeros in the
beam-former output (lim 0); what the dumped weights hold there is nobody's business (may, not must).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

import conv_ref as cr
import train_ref as tref
from train_ref import D64, SECOND, U, _ab, _M, _prelu

SENTINEL = np.float32(7.25)
GUARD = 4096
BFW_K = 64


def rows_mask(B: int, T: int, pos: Optional[int] = None, count: Optional[int] = None, lens=None, extra: int = 0) -> np.ndarray:
    """(B, T) bool: the frames of the window [pos, pos + count) clipped at T, or -- no window -- the frames below each length,
    or all.  extra: the CPU mutation check makes the window that many frames longer."""
    t = np.arange(T)
    if pos is not None:
        return np.broadcast_to((t >= pos) & (t < min(pos + count + extra, T)), (B, T)).copy()
    if lens is not None:
        return t[None, :] < np.asarray(lens)[:, None]
    return np.ones((B, T), bool)


def norm_act(A: Dict[str, np.ndarray], dtype, T: int, rows_per_t: int = 1, pos=None, count=None, lens=None,
             table_shift: int = 0, extra: int = 0):
    """out = prelu(a sa + ha, slope_a) [+ prelu(b sb + hb, slope_b)];  a, b (B, P, C), P = T rows_per_t, xf (B, C, 2) =
    (scale, shift), slope (C,).  A window wins over lens (the kernel ignores lens when a window is set).
    table_shift: the CPU mutation check reads the tables of channel c + table_shift."""
    m = _M(dtype)

    def operand(x, xf, sl):
        x, xf, sl = m(x), m(xf), m(sl)
        if table_shift:
            xf, sl = np.roll(xf, -table_shift, 1), np.roll(sl, -table_shift)
        s, h = xf[:, None, :, 0], xf[:, None, :, 1]
        y = _prelu(x * s + h, sl)
        return y, np.maximum(1.0, _ab(sl)) * 2 * U * (_ab(x * s) + _ab(h)) + U * _ab(y)
    with np.errstate(invalid="ignore"):
        y, lim = operand(A["a"], A["xfa"], A["slopea"])
        if A.get("b") is not None:
            y2, l2 = operand(A["b"], A["xfb"], A["slopeb"])
            y = y + y2
            lim = lim + l2 + U * _ab(y)
    B, P, C = y.shape
    assert P == T * rows_per_t
    must = np.repeat(rows_mask(B, T, pos, count, lens, extra), rows_per_t, 1)
    return {"out": (y, lim * SECOND, np.broadcast_to(must[:, :, None], y.shape).copy())}


def bfw(A: Dict[str, np.ndarray], dtype, M: int, pos=None, count=None, lens=None, drop_mic: Optional[int] = None,
        extra: int = 0):
    """The beam-forming head: h (B, T, F, 64); w1 (64, 64), b1 (64,) when the first Linear + ReLU is fused (else h IS y1);
    w2 (2M, 64), b2 (2M,); x (B, T, F, M, 2).  out (B, 2, T, F) = sum_m w_m x_m (complex, no conjugate) and the dumped
    weights bfw (B, T, F, M, 2).  The rows of the window are written; behind a length out is exactly zero.
    drop_mic: the CPU mutation check leaves that microphone out of the sum."""
    m = _M(dtype)
    h, x = m(A["h"]), m(A["x"])
    B, T, F, K = h.shape
    assert K == BFW_K and x.shape == (B, T, F, M, 2)
    written = rows_mask(B, T, pos, count, None, extra)
    live = written & rows_mask(B, T, lens=lens)
    zero = np.zeros((), m.dt)
    rows = np.where(live[:, :, None, None], h, zero).reshape(-1, K)          # (what lies behind a length is never used)
    x = np.where(live[:, :, None, None, None], x, zero)
    if A.get("w1") is not None:
        W1, b1 = m(A["w1"]), m(A["b1"])
        y1 = np.maximum(rows @ W1.T + b1, zero)
        e1 = (K + 2) * U * (_ab(rows) @ _ab(W1).T + _ab(b1))
    else:
        y1, e1 = rows, np.zeros(rows.shape)
    W2, b2 = m(A["w2"]), m(A["b2"])
    w = (y1 @ W2.T + b2).reshape(B, T, F, M, 2)
    ew = ((K + 2) * U * (_ab(y1) @ _ab(W2).T + _ab(b2)) + e1 @ _ab(W2).T).reshape(B, T, F, M, 2)
    wr, wi, xr, xi = w[..., 0], w[..., 1], x[..., 0], x[..., 1]
    if drop_mic is not None:
        xr, xi = xr.copy(), xi.copy()
        xr[..., drop_mic] = xi[..., drop_mic] = 0
    t = [wr * xr, -wi * xi, wr * xi, wi * xr]
    yr, yi = m.sum(t[0] + t[1], -1), m.sum(t[2] + t[3], -1)
    lr = (2 * M + 2) * U * (_ab(t[0]) + _ab(t[1])).sum(-1) + (ew[..., 0] * _ab(xr) + ew[..., 1] * _ab(xi)).sum(-1)
    li = (2 * M + 2) * U * (_ab(t[2]) + _ab(t[3])).sum(-1) + (ew[..., 0] * _ab(xi) + ew[..., 1] * _ab(xr)).sum(-1)
    out, lim = np.stack([yr, yi], 1), np.stack([lr, li], 1) * SECOND
    full = lambda mask, shape: np.broadcast_to(mask.reshape(mask.shape + (1,) * (len(shape) - 2)), shape).copy()   # noqa: E731
    must_out = np.broadcast_to(written[:, None, :, None], out.shape).copy()
    return {"out": (out, lim, must_out),
            "bfw": (w, ew * SECOND, full(live, w.shape), full(written, w.shape))}


def filter_sum(A, dtype, M: int):
    """eab_filter_sum_f32: w (B, T, F, 2M), x (B, T, F, M, 2) -> y (B, 2, T, F)   (train_ref's FILTER_SUM, ld = 2M)"""
    B, T, F = A["x"].shape[:3]
    return tref.run_ref("FILTER_SUM", [B, T, F, M, 2 * M], [], A, dtype)[0]


def in_finalize(A, dtype, count: int, eps: float):
    """eab_in_finalize[_mr]_f32: stats (B, tiles, nsets, C, 4) Welford partials (n, mean, M2, unused)   (train_ref's IN_FINALIZE)"""
    B, tiles, nsets, C, _ = A["stats"].shape
    return tref.run_ref("IN_FINALIZE", [B, C, nsets, tiles, count], [eps], A, dtype)[0]


def cln_stats(A, dtype, C: int, eps: float):
    """eab_cln_stats_f32 on the whole utterance: x (B, T, P), slope (C,) or absent   (train_ref's CLN_STATS), plus the running
    state it leaves behind: [B][2] (sum, sum of squares) and [B] frames seen, all doubles"""
    B, T, P = A["x"].shape
    outs = tref.run_ref("CLN_STATS", [B, T, P, C], [eps], {k: v for k, v in A.items() if k in ("x", "slope")}, dtype)[0]
    s, L = outs["sums"][:2]
    state = np.concatenate([s.sum(1).reshape(-1), np.full(B, float(T))])
    lim = np.concatenate([(L.sum(1) + T * D64 * np.abs(s).sum(1)).reshape(-1), np.zeros(B)])
    outs["state"] = (state, lim)
    return outs


def cln_apply(A, dtype, C: int, mode: int, pos=None, count=None, extra: int = 0):
    """eab_cln_apply_f32 (train_ref's CLN_APPLY) restricted to the rows of the window"""
    B, T, P = A["x"].shape
    y, lim = tref.run_ref("CLN_APPLY", [B, T, P, C, mode], [], A, dtype)[0]["y"][:2]
    must = np.broadcast_to(rows_mask(B, T, pos, count, None, extra)[:, :, None], y.shape).copy()
    return {"y": (y, lim, must)}


def gate_rows(A, dtype, pos=None, count=None, extra: int = 0):
    """eab_gate_rows_f32: z = a sigmoid(r) on the rows of the window; a, r (B, T, row)   (train_ref's GATE_FWD)"""
    B, T, row = A["a"].shape
    n = B * T * row
    flat = {k: np.asarray(A[k]).reshape(-1) for k in ("a", "r")}
    z, lim = tref.run_ref("GATE_FWD", [n & 0xFFFFFFFF, n >> 32], [], flat, dtype)[0]["z"][:2]
    must = np.broadcast_to(rows_mask(B, T, pos, count, None, extra)[:, :, None], (B, T, row)).copy()
    return {"z": (z.reshape(B, T, row), lim.reshape(B, T, row), must)}


def zero_rows(B: int, T: int, row: int, dtype, pos=None, count=None, extra: int = 0):
    """eab_zero_rows_f32: the rows of the window (or everything) become +0.0"""
    must = np.broadcast_to(rows_mask(B, T, pos, count, None, extra)[:, :, None], (B, T, row)).copy()
    return {"ptr": (np.zeros((B, T, row), dtype), np.zeros((B, T, row)), must)}


# ----------------------------------------------------------------------------------------------------------------------
# the judgement every test of these kernels applies (device, host emulation and the CPU mutation checks)
# ----------------------------------------------------------------------------------------------------------------------
def as_outs(res, f64=()) -> Dict[str, tref.Out]:
    outs = {}
    for name, r in res.items():
        val = np.asarray(r[0])
        must = np.ones(val.shape, bool) if len(r) < 3 else np.asarray(r[2], bool)
        may = must if len(r) < 4 else np.asarray(r[3], bool)
        outs[name] = tref.Out(None, val.shape, val, np.asarray(r[1], np.float64), must, may, name=name, f64=name in f64)
    return outs


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def judge(res, got: Dict[str, np.ndarray], yard, what: str, f64=(), sentinel=SENTINEL):
    """got[name]: the output buffer after the launch, which held ``sentinel`` everywhere before it.  Asserts: every element
    outside ``may`` kept its bits, every ``must`` element is finite, and train_ref.check -- the per-element derived limit and the
    L2 criterion (conv_ref.MARGIN x the fp32 yardstick, both against float64).  Returns (worst err/limit, worst L2 ratio)."""
    outs = as_outs(res, f64)
    for name, o in outs.items():
        g = np.asarray(got[name])
        assert g.shape == o.shape, f"{what} {name}: shape {g.shape} != {o.shape}"
        sent = _bits(np.asarray([sentinel], g.dtype))[0]
        kept = _bits(g)[~o.may] == sent
        assert kept.all(), f"{what} {name}: {int((~kept).sum())} elements outside the rows of the launch changed"
        assert np.isfinite(g[o.must]).all(), f"{what} {name}: a written element is not finite"
    y = None if yard is None else {k: np.asarray(r[0]) for k, r in yard.items()}
    return tref.check(outs, got, y, what, margin=cr.MARGIN)


def line(kernel: str, case: str, worst: float, l2) -> str:
    return f"MEMOPS {kernel} {case} | err/limit {worst:.3f} | L2 ratio {'-' if l2 is None else format(l2, '.2f')}"


# ----------------------------------------------------------------------------------------------------------------------
# the cases: one table per kernel family, used by the device file, the host emulation and the CPU checks alike
# ----------------------------------------------------------------------------------------------------------------------
NA_THREADS, NA_UNROLL = 256, 4            # csrc/norm.hip: block size and float4s in flight per thread of norm_act_kernel
LENS = (9, 1, 5)


def na_cap(B: int) -> int:
    """grid cap of norm_act_kernel per batch element (csrc/norm.hip)"""
    return (1024 + B - 1) // B


def norm_act_cases():
    out = []
    for C in (4, 24, 64, 256):
        for two in (False, True):
            for P in (1, 57, 1300):
                out.append(dict(name=f"C{C}-{'two' if two else 'one'}-P{P}", B=3, T=P, rpt=1, C=C, two=two))
    for P, two in ((1024, False), (1024, True), (1030, False), (1030, True)):      # the capped grid: exactly one sweep, and a second
        out.append(dict(name=f"cap-P{P}-{'two' if two else 'one'}", B=65, T=P, rpt=1, C=64, two=two, capped=P > 1024))
    for C in (24, 64):
        for pos in (0, 4, 8):
            out.append(dict(name=f"win-C{C}-pos{pos}", B=3, T=9, rpt=5, C=C, two=True, pos=pos, count=4))
        out.append(dict(name=f"lens-C{C}", B=3, T=9, rpt=5, C=C, two=C == 24, lens=LENS))
    return out


def norm_act_inputs(c, seed=0):
    rng = np.random.default_rng([11, seed, c["B"], c["T"], c["C"], int(c["two"])])
    B, P, C = c["B"], c["T"] * c["rpt"], c["C"]
    f32 = lambda *s: rng.standard_normal(s, np.float32)                                   # noqa: E731

    def tables():
        xf = np.stack([rng.uniform(0.5, 1.5, (B, C)) * rng.choice([-1.0, 1.0], (B, C)), 0.3 * rng.standard_normal((B, C))], -1)
        return xf.astype(np.float32), rng.uniform(-0.5, 1.5, C).astype(np.float32)
    A = {"a": f32(B, P, C)}
    A["xfa"], A["slopea"] = tables()
    if c["two"]:
        A["b"] = f32(B, P, C)
        A["xfb"], A["slopeb"] = tables()
    if c.get("lens") is not None:                    # what lies behind a length is never read
        for b, n in enumerate(c["lens"]):
            for k in ("a", "b"):
                if k in A:
                    A[k][b, n * c["rpt"]:] = np.nan
    return A


def norm_act_kw(c):
    return dict(T=c["T"], rows_per_t=c["rpt"], pos=c.get("pos"), count=c.get("count"), lens=c.get("lens"))


FIN_TILES = (1, 15, 16, 17, 48, 49, 65, 130)
FIN_C = (16, 64, 100, 256)


def in_finalize_cases():
    out = [dict(name=f"tiles{t}-C{C}-sets{n}", B=3, tiles=t, C=C, nsets=n) for C in FIN_C for t in FIN_TILES for n in (1, 2)]
    out.append(dict(name="empty-tiles", B=3, tiles=65, C=100, nsets=2, empty=True))
    out.append(dict(name="constant-channel", B=3, tiles=49, C=100, nsets=2, const=True))
    return out


def in_finalize_inputs(c, seed=0):
    """Welford triples of real data split into tiles of 1..24 rows.  A tile without rows is (n = 0, any FINITE mean, M2 = 0):
    that is what conv_ref.put_stats says a convolution writes for a tile wholly behind a length ("finite is all the merge
    needs"); the device forms fma(n, mean, .), which a NaN mean would poison even at n = 0, and adds M2 whatever n is.  So the
    empty tiles of the 'empty-tiles' case hold (0, 5.5, 0), not NaN: the mean must not count, and nothing else is defined.  The
    fourth slot is not part of the triple and holds a value that would show."""
    rng = np.random.default_rng([12, seed, c["tiles"], c["C"], c["nsets"]])
    B, tiles, C, nsets = c["B"], c["tiles"], c["C"], c["nsets"]
    sizes = rng.integers(1, 25, tiles)
    if c.get("empty"):
        sizes[rng.permutation(tiles)[:tiles // 3]] = 0
    stats = np.zeros((B, tiles, nsets, C, 4), np.float32)
    stats[..., 3] = 123.0
    off, sc = rng.standard_normal((nsets, C)), rng.uniform(0.2, 2.0, (nsets, C))
    for t, n in enumerate(sizes):
        if n == 0:
            stats[:, t, :, :, 1] = 5.5
            continue
        x = (off + sc * rng.standard_normal((B, n, nsets, C))).astype(np.float32).astype(np.float64)
        if c.get("const"):
            x[..., 0] = 1.75
        mean = x.mean(1).astype(np.float32)
        stats[:, t, :, :, 0] = n
        stats[:, t, :, :, 1] = mean
        stats[:, t, :, :, 2] = ((x - mean[:, None].astype(np.float64)) ** 2).sum(1)
    A = {"stats": stats}
    for s in range(nsets):
        A[f"gamma{s}"] = rng.uniform(0.5, 1.5, C).astype(np.float32)
        A[f"beta{s}"] = (0.3 * rng.standard_normal(C)).astype(np.float32)
    return A, int(sizes.sum())


FS_M = (1, 3, 4, 5, 9, 16, 33)
FS_SHAPES = ((1, 3, 5), (2, 7, 161))
FS_LARGE = (2, 408, 161, 5)               # B T F > 131072 = 2048 workgroups x 64 bins: a second sweep


def filter_sum_inputs(B, T, F, M, seed=0):
    rng = np.random.default_rng([13, seed, B, T, F, M])
    return {"w": rng.standard_normal((B, T, F, 2 * M), np.float32), "x": rng.standard_normal((B, T, F, M, 2), np.float32)}


BFW_M = (1, 4, 8, 9, 16, 17, 24, 32)
BFW_SHAPES = ((2, 5, 161), (23, 1, 7), (4, 3, 21), (3, 137, 161))
BFW_WIN = dict(shape=(2, 9, 161), counts=(1, 4), poss=(0, 4, 7, 8))
BFW_LENS_SHAPE = (3, 9, 161)


def bfw_inputs(B, T, F, M, seed=0, lens=None):
    rng = np.random.default_rng([14, seed, B, T, F, M])
    A = {"h": rng.standard_normal((B, T, F, BFW_K), np.float32), "x": rng.standard_normal((B, T, F, M, 2), np.float32),
         "w1": (rng.standard_normal((BFW_K, BFW_K)) / 8).astype(np.float32), "b1": (0.2 * rng.standard_normal(BFW_K)).astype(np.float32),
         "w2": (rng.standard_normal((2 * M, BFW_K)) / 8).astype(np.float32), "b2": (0.2 * rng.standard_normal(2 * M)).astype(np.float32)}
    if lens is not None:
        for b, n in enumerate(lens):
            A["h"][b, n:] = np.nan
            A["x"][b, n:] = np.nan
    return A


def bfw_args(A, fused: bool):
    """the named arrays of one launch: without the fused first Linear the kernel reads ``h`` as y1"""
    return A if fused else {k: v for k, v in A.items() if k not in ("w1", "b1")}


CLN_BT = (3, 7)
CLN_SHAPES = ((64, 1), (64, 79), (256, 4), (4, 3))            # (C, P / C)
CLN_CHUNKS = (1, 3, 5)
CLN_EPS = 1e-5


def cln_inputs(C, Fq, seed=0, B=CLN_BT[0], T=CLN_BT[1]):
    rng = np.random.default_rng([15, seed, C, Fq, B, T])
    P = C * Fq
    return {"x": (0.4 + rng.standard_normal((B, T, P))).astype(np.float32), "add": rng.standard_normal((B, T, P), np.float32),
            "gain": rng.uniform(0.5, 1.5, C).astype(np.float32), "bias": (0.3 * rng.standard_normal(C)).astype(np.float32),
            "slope": rng.uniform(-0.5, 1.5, C).astype(np.float32), "r": (3 * rng.standard_normal((B, T, P))).astype(np.float32)}


def windows(T: int, chunk: int):
    """(pos, count) of a chunked pass over T frames; the last window may be clipped by the end of the utterance"""
    return [(p, chunk) for p in range(0, T, chunk)]
