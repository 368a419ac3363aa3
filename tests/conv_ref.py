"""float64 reference of ONE convolution launch (eab_conv_desc, include/eabnet_hip.h) with a derived error limit per
output element  (TEST INFRASTRUCTURE).

conv_ref(op, arena) evaluates the formula documented above eab_conv_desc in float64 from the fp32 arrays the op names and
returns, per output region (dst, dst_acc, f2_dst, the GLU factor dump of the training programs, the statistics partials, the
fz_* tables and the arrival counter), the
value, a limit on the error of a correct fp32 evaluation of it, and the set of elements the launch writes.  The weights are
unpacked with the project's own helpers (prg.unpack_frag, prg.glu_row_order, the emulator's unit order and unpack_f16x3).

The limit is DERIVED, never measured.  With u = 2^-24 (fp32 unit roundoff) and, per output element n,

    acc[n] = bias[n] + sum_k w_k f(x)_k,     S[n] = |bias[n]| + sum_k |w_k| m_k,
    m_k = |f(x)_k| without a transform, (|x scale| + |shift|) max(1, |slope|) with one

  * fp32 accumulation of the K = Kpad products in ANY order (fused or not, blocked or sequential) errs by at most
    K u S to first order; the further roundings of the path add c u S:  1 for the bias, 1 for the store / epilogue,
    3 for a fused transform (one fma, one PReLU product, one operand rounding of the product term), 2 more where the
    (scale, shift) table is merged in the kernel from partials (fin_stats: the table entries are fp64 results rounded to
    fp32, so they may differ by an ulp between two correct evaluations).            |err(acc)| <= (K + c) u S
  * EAB_PREC_F16X3: every product is hi*hi + hi*lo + lo*hi of the fp16 splits, "~22-bit products" as the header states:
    + 2^-22 S.  The weights of the reference are the stored hi + lo (exact), so only the product error is added.
  * EAB_PREC_BF16: the reference multiplies the SAME bf16-rounded operands (bf16_round of the weights and of the fp32
    operand, the fused transform evaluated as the kernel does: one fma, one PReLU product), so only the accumulation
    order differs: (K + c) u S with S over the rounded operands.  Where a transform is fused, two correct fp32
    evaluations of f(x) (fma or not, table an ulp apart) differ by <= 3 ulp, which moves an operand across a bf16
    rounding boundary with probability <= 3 * 2^-24 / 2^-8 = 3 * 2^-16 and then changes that product by one bf16 spacing,
    <= 2^-7 |w f|.  With K <= 1024 operands the expected number of such flips per output is < 0.05; more than 6 have
    probability < 1e-11 per element.  Allowance: 6 * 2^-7 * max_k |w_k f_k|, the maximum bounded from above by the
    8-norm (sum_k |w_k f_k|^8)^(1/8) (one more matrix product; within K^(1/8) <= 2.4 of the maximum).  This allowance is
    0.05 to 0.11 of the LARGEST product of the element, i.e. about one typical product at K = 768: in the bf16 variants
    with a fused transform a single dropped product is therefore NOT rejected by the per-element limit, only by the L2
    criterion below (a dropped tap, K / taps products, is rejected by both).
  * epilogues: RELU and PHASE2 / LINEAR are 1-Lipschitz in acc (limit unchanged); ADD rounds the sum once more
    (+ u |out|); out = a sigmoid(g) (GLU, DUALGATE; MULSIG with a = aux, exact):
        |err| <= sigmoid(g) err(a) + |a| sigmoid'(g) err(g) + err(a) err(g) / 4 + |out| ((|g| + 6) 2^-23 + 2 u)
    the last term for the device's approximate exp and reciprocal (1-ulp instructions; the argument is scaled by log2 e,
    so an ulp of the argument is a relative |g| 2^-23 of the exponential) and the two products.
  * dst_acc += out: limit(out) + u |dst_acc|.
  * f2 (second 1x1 on the rows just produced, K2 = N): (K2 + 2) u S2 + sum_c |w2_c| limit(dst_c), S2 = sum |w2_c| |dst_c|.
  * statistics of a tile of n rows with values g (limit l each), D = max |g - mean|: the kernel sums e = g - k0 and e^2 in
    fp32 around one of the tile's own values k0 (|mean - k0| <= D), then merges lanes with Chan's formula:
        |err(mean)| <= mean(l) + (n + 16) u (|mean| + 2 D)
        |err(M2)|   <= 2 sqrt(M2 sum l^2) + sum l^2 + 3 (n + 16) u (M2 + n D^2)
    n itself is exact.
  * fz_* tables: the merge is fp64 on the device; the limits of the partials are propagated through
    mean = sum n mu / N, M2 = sum M2_t + sum n (mu - mean)^2, scale = gamma / sqrt(M2 / N + eps), shift = beta - mean scale,
    plus 2 u for the final roundings to fp32.

A single dropped or misplaced product out of K = 768 is about S / 768, some 28 times the fp32 limit (fp32 and f16x3
launches, and bf16 launches without a fused transform; see the bf16 item for the others).  Because the limit is loose against typical (random-walk) error, check() adds a statistical criterion: the
L2-relative error against float64 may be at most MARGIN times the L2-relative error of a plain fp32 CPU evaluation of the
same op (the emulator's conv) against the same float64 result.
"""
from __future__ import annotations

import ast
import dataclasses
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from eabnet_amd import program as prg
from emulator import Emulator, bf16_round, unpack_f16x3

U = 2.0 ** -24
MARGIN = 8.0             # statistical criterion: device L2 error <= MARGIN * fp32-CPU L2 error (both against float64)
YARD_FLOOR = 2.0 ** -25  # a correctly ROUNDED fp32 result already has an RMS relative error of about u / sqrt(3)
BF16_FLIPS = 6
L2_NAMES = ("dst", "dst_acc", "f2_dst")


# ----------------------------------------------------------------------------------------------------------------------
# what a launch reads and writes
# ----------------------------------------------------------------------------------------------------------------------
def regions(op: prg.ConvOp) -> List[Tuple[str, prg.Ref, tuple, bool, str]]:
    """(field, ref, shape, batched, mode) of every array the op names; mode 'r' read, 'w' written, 'rw' both.  Batched
    arrays have the batch as their first dimension."""
    B, T, N = op.B, op.T, op.N
    dual = op.epi == prg.EPI_DUALGATE
    C1x = op.C0 if dual else op.C1
    act = (B, T, op.Fout, op.Cout)
    out = [("src0", op.src0, (B, T, op.Fin, op.C0), True, "r"), ("src1", op.src1, (B, T, op.Fin, op.C1), True, "r"),
           ("xf0", op.xf0, (B, op.C0, 2), True, "r"), ("xf1", op.xf1, (B, C1x, 2), True, "r"),
           ("slope0", op.slope0, (op.C0,), False, "r"), ("slope1", op.slope1, (C1x,), False, "r"),
           ("w", op.w, (N * op.Kpad,), False, "r"), ("bias", op.bias, (N,), False, "r"),
           ("aux", op.aux, act, True, "r"), ("dst", op.dst, act, True, "w"), ("dst_acc", op.dst_acc, act, True, "rw"),
           ("stats", op.stats, (B, op.stat_tiles, op.nsets, op.Cout, 4), True, "rw"),
           ("stat_slope0", op.stat_slope0, (op.Cout,), False, "r"), ("stat_slope1", op.stat_slope1, (op.Cout,), False, "r"),
           ("fin_stats", op.fin_stats, (B, op.fin_tiles, op.fin_nsets, op.C0, 4), True, "r"),
           ("fin_gamma0", op.fin_gamma0, (op.C0,), False, "r"), ("fin_beta0", op.fin_beta0, (op.C0,), False, "r"),
           ("fin_gamma1", op.fin_gamma1, (op.C0,), False, "r"), ("fin_beta1", op.fin_beta1, (op.C0,), False, "r"),
           ("fz_counter", op.fz_counter, (B,), True, "rw"),
           ("fz_gamma0", op.fz_gamma0, (op.Cout,), False, "r"), ("fz_beta0", op.fz_beta0, (op.Cout,), False, "r"),
           ("fz_gamma1", op.fz_gamma1, (op.Cout,), False, "r"), ("fz_beta1", op.fz_beta1, (op.Cout,), False, "r"),
           ("fz_xf0", op.fz_xf0, (B, op.Cout, 2), True, "w"), ("fz_xf1", op.fz_xf1, (B, op.Cout, 2), True, "w"),
           ("ph1_w", op.ph1_w, (N * op.ph1_Kpad,), False, "r"),
           ("f2_w", op.f2_w, (op.f2_N * N,), False, "r"), ("f2_dst", op.f2_dst, (B, T, 1, op.f2_N), True, "w"),
           ("f2_stats", op.f2_stats, (B, op.f2_stat_tiles, op.f2_nsets, op.f2_N, 4), True, "w"),
           ("f2_stat_slope0", op.f2_stat_slope0, (op.f2_N,), False, "r"),
           ("f2_stat_slope1", op.f2_stat_slope1, (op.f2_N,), False, "r"),
           ("glu_dump", op.glu_dump, (B, T, op.Fout, N), True, "w")]
    assert not op.src_bf16, "bf16-stored sources (bf16 training programs) are not part of this reference"
    assert op.glu_dump is None or op.epi == prg.EPI_GLU, "only the GLU epilogue dumps its factors"
    return [r for r in out if r[1] is not None]


def localize(op: prg.ConvOp, fetch: Callable[[str, prg.Ref, tuple, bool], np.ndarray], B: Optional[int] = None):
    """The op cut out of its program: (op', arena') with every array it names copied into a compact arena 'x' (batched
    arrays for the first ``B`` batch elements only) and the op's Refs rewritten.  fetch(field, ref, full shape, batched)
    returns the array as the program holds it (fp32; of a batched array at least the first B elements)."""
    B = op.B if B is None else B
    place: Dict[prg.Ref, Tuple[int, int]] = {}
    chunks, size, new = [], 0, {}
    for field, ref, shape, batched, _ in regions(op):
        n_full = int(np.prod(shape))
        if ref in place:
            assert place[ref][1] == n_full, f"{op.name}: {field} aliases another array of a different size"
            new[field] = prg.Ref("x", place[ref][0])
            continue
        for (r2, (_, n2)) in place.items():
            if r2.arena == ref.arena:
                assert ref.off + n_full <= r2.off or r2.off + n2 <= ref.off, f"{op.name}: {field} overlaps another array"
        a = np.asarray(fetch(field, ref, shape, batched), dtype=np.float32)
        if batched:
            a = a[:B]
        a = np.ascontiguousarray(a).reshape(-1)
        place[ref] = (size, n_full)
        new[field] = prg.Ref("x", size)
        chunks.append(a)
        pad = (-a.size) % prg.ALIGN
        if pad:
            chunks.append(np.full(pad, np.nan, np.float32))
        size += a.size + pad
    return dataclasses.replace(op, B=B, **new), {"x": np.concatenate(chunks)}


def arena_fetch(arena: Dict[str, np.ndarray]):
    def fetch(field, ref, shape, batched):
        n = int(np.prod(shape))
        return arena[ref.arena][ref.off:ref.off + n].reshape(shape)
    return fetch


def read(arena, ref, shape):
    n = int(np.prod(shape))
    return arena[ref.arena][ref.off:ref.off + n].reshape(shape)


# ----------------------------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Out:
    ref: prg.Ref
    shape: tuple
    val: np.ndarray      # float64
    lim: np.ndarray      # float64, >= 0; 0 = must be exact
    must: np.ndarray     # bool: elements the launch writes (and the check compares)
    may: np.ndarray      # bool: elements the launch is allowed to change (a superset of must)
    integer: bool = False  # int32 bit pattern kept in the fp32 arena (the arrival counter)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _merge(n, mu, m2):
    """Chan merge over axis 1 of (B, tiles, C) float64 triples -> (N, mean, M2) of shape (B, C)"""
    N = n.sum(1)
    mean = (n * mu).sum(1) / N
    return N, mean, m2.sum(1) + (n * (mu - mean[:, None]) ** 2).sum(1)


def _xform(x, tab, a, mode, faithful32):
    """f(x) in float64 and the magnitude m of its terms.  faithful32: round where the kernel rounds (one fma, one PReLU
    product), so that the bf16 rounding that follows sees the operand the kernel sees."""
    r = _f32 if faithful32 else (lambda v: v)
    x = x.astype(np.float64)
    s, h = tab[:, None, None, :, 0].astype(np.float64), tab[:, None, None, :, 1].astype(np.float64)
    a = a.astype(np.float64)
    if mode == prg.XF_NORM_PRELU:
        t = r(x * s + h)
        return np.where(t > 0, t, r(a * t)), (np.abs(x * s) + np.abs(h)) * np.maximum(1.0, np.abs(a))
    q = np.where(x > 0, x, r(a * x))
    return r(q * s + h), np.abs(q * s) + np.abs(h)


def _tile_stats(parts, bm: int, tiles: int):
    """Welford triple per tile with its limits.  parts: [(g, lim, valid)] with g, lim (B, Q, C) float64 and valid (B, Q)
    bool, all indexed by the launch's row q (tile = q // bm); a tile's block is the union of its valid rows over the parts
    (two for EAB_EPI_PHASE2: both output-column phases).  Returns n, mean, M2, lim_mean, lim_M2 of shape (B, tiles, C)."""
    def blocks(a, fill=0.0):
        B, Q = a.shape[:2]
        pad = np.full((B, tiles * bm - Q) + a.shape[2:], fill, a.dtype)
        return np.concatenate([a, pad], 1).reshape((B, tiles, bm) + a.shape[2:])
    gs = np.concatenate([blocks(g) for g, _, _ in parts], 2)
    ls = np.concatenate([blocks(l) for _, l, _ in parts], 2)
    vs = np.concatenate([blocks(v, False) for _, _, v in parts], 2)[..., None]
    n = vs.sum(2).astype(np.float64)                       # (B, tiles, 1)
    nn = np.maximum(n, 1.0)
    mean = np.where(vs, gs, 0.0).sum(2) / nn
    dev = np.where(vs, gs - mean[:, :, None], 0.0)
    M2 = (dev ** 2).sum(2)
    D = np.abs(dev).max(2)
    l1, l2 = np.where(vs, ls, 0.0).sum(2), np.where(vs, ls ** 2, 0.0).sum(2)
    lim_mean = l1 / nn + (n + 16) * U * (np.abs(mean) + 2 * D)
    lim_M2 = 2 * np.sqrt(M2 * l2) + l2 + 3 * (n + 16) * U * (M2 + n * D * D)
    return np.broadcast_to(n, mean.shape).copy(), mean, M2, lim_mean, lim_M2


class _Launch:
    def __init__(self, op, arena, lens):
        self.op, self.arena = op, arena
        self.lens = np.full(op.B, op.T, np.int64) if lens is None else np.asarray(lens, np.int64)
        assert self.lens.shape == (op.B,) and self.lens.min() >= 1 and self.lens.max() <= op.T
        assert not op.win, "streaming windows are not part of this reference (offline programs only)"
        self.outs: Dict[str, Out] = {}
        self.tvalid = np.arange(op.T)[None, :] < self.lens[:, None]          # (B, T)

    def v(self, ref, shape):
        return None if ref is None else read(self.arena, ref, shape)

    def out(self, name, ref, shape, integer=False) -> Out:
        if name not in self.outs:
            self.outs[name] = Out(ref, shape, np.full(shape, np.nan), np.zeros(shape), np.zeros(shape, bool), np.zeros(shape, bool),
                                  integer)
        return self.outs[name]

    # -- sources ---------------------------------------------------------------------------------------------------
    def sources(self):
        """operands X (and X2 for the dual form) as float64 [B][T][Fin][Ct], their magnitudes, and the constant c"""
        op = self.op
        B, T, Fin = op.B, op.T, op.Fin
        dual = op.epi == prg.EPI_DUALGATE
        bf = op.precision == prg.PREC_BF16
        fin_tabs = None
        if op.fin_stats is not None:
            st = self.v(op.fin_stats, (B, op.fin_tiles, op.fin_nsets, op.C0, 4)).astype(np.float64)
            assert not np.isnan(st).any(), f"{op.name}: producer partials not fully written"
            fin_tabs = []
            for k, (g, bb) in enumerate(((op.fin_gamma0, op.fin_beta0), (op.fin_gamma1, op.fin_beta1))):
                if g is None:
                    break
                N, mean, M2 = _merge(st[:, :, k, :, 0], st[:, :, k, :, 1], st[:, :, k, :, 2])
                scale = self.v(g, (op.C0,)).astype(np.float64) / np.sqrt(M2 / N + op.fin_eps)
                fin_tabs.append(np.stack([scale, self.v(bb, (op.C0,)) - mean * scale], -1).astype(np.float32))
        xs, ms, X2, M2_ = [], [], None, None
        self.xformed = False
        for i, (ref, xf, sl, Cs) in enumerate(((op.src0, op.xf0, op.slope0, op.C0), (op.src1, op.xf1, op.slope1, op.C1))):
            if ref is None:
                continue
            x = self.v(ref, (B, T, Fin, Cs))
            tab = fin_tabs[0] if (fin_tabs is not None and i == 0) else (self.v(xf, (B, Cs, 2)) if xf is not None else None)
            if dual:
                assert i == 0 and op.src1 is None
                tab1 = fin_tabs[1] if fin_tabs is not None else self.v(op.xf1, (B, Cs, 2))
                X2, M2_ = _xform(x, tab1, self.v(op.slope1, (Cs,)), op.xf_mode, bf)
                self.xformed = True
            if tab is not None and op.xf_mode != prg.XF_NONE:
                f, m = _xform(x, tab, self.v(sl, (Cs,)), op.xf_mode, bf)
                self.xformed = True
            else:
                f = x.astype(np.float64)
                m = np.abs(f)
            xs.append(f)
            ms.append(m)
        X, M = np.concatenate(xs, -1), np.concatenate(ms, -1)
        if bf:       # the operand the bf16 matrix cores see; S is taken over the rounded operands
            X = bf16_round(X.astype(np.float32)).astype(np.float64)
            M = np.abs(X)
            if X2 is not None:
                X2 = bf16_round(X2.astype(np.float32)).astype(np.float64)
                M2_ = np.abs(X2)
        self.c = 2 + (3 if self.xformed else 0) + (2 if fin_tabs is not None else 0)
        return X, M, X2, M2_

    # -- one pass of the tap-ordered form -----------------------------------------------------------------------------------
    def conv_pass(self, W, Wabs, bias, Kpad, No, ophase, dts, ioffs, st0, src):
        """W, Wabs: float64 [N][ntaps][Ct] in the packed row order of the tap-ordered form (operands as the precision sees
        them and their magnitudes)."""
        op = self.op
        B, T, Fin, N = op.B, op.T, op.Fin, op.N
        X, M, X2, M2_ = src
        Ct = X.shape[-1]
        dual = op.epi == prg.EPI_DUALGATE
        bf, h3 = op.precision == prg.PREC_BF16, op.precision == prg.PREC_F16X3
        flips = bf and self.xformed
        o = np.arange(No)
        rows = B * T * No
        acc = torch.zeros(rows, N, dtype=torch.float64)
        S = torch.zeros(rows, N, dtype=torch.float64)
        P8 = torch.zeros(rows, N, dtype=torch.float64) if flips else None
        if bias is not None:
            acc += _t(bias)
            S += _t(np.abs(bias))
        left = (np.arange(N) % 64) < 32

        def gather(A, dt, fi, ok):
            G = np.zeros((B, T, No, Ct))
            tv = T - abs(dt)
            dst_t = slice(-dt, T) if dt <= 0 else slice(0, tv)
            src_t = slice(0, tv) if dt <= 0 else slice(dt, T)
            if tv > 0:
                G[:, dst_t, ok] = A[:, src_t][:, :, fi[ok]]
            return _t(G.reshape(rows, Ct))

        for j, (dt, io) in enumerate(zip(dts, ioffs)):
            fi = o * op.istride + io
            ok = (fi >= 0) & (fi < Fin)
            Wj, Aj = _t(W[:, j, :Ct]), _t(Wabs[:, j, :Ct])
            sides = [(X, M, slice(None))] if not dual else [(X, M, np.nonzero(left)[0]), (X2, M2_, np.nonzero(~left)[0])]
            for Xs, Ms, r in sides:
                G, Gm = gather(Xs, dt, fi, ok), gather(Ms, dt, fi, ok)
                if dual:
                    acc[:, r] += G @ Wj[r].T
                    S[:, r] += Gm @ Aj[r].T
                    if flips:
                        P8[:, r] += G.abs().pow(8) @ Aj[r].pow(8).T
                else:
                    acc += G @ Wj.T
                    S += Gm @ Aj.T
                    if flips:
                        P8 += G.abs().pow(8) @ Aj.pow(8).T
        shape = (B, T, No, N)
        acc, S = acc.numpy().reshape(shape), S.numpy().reshape(shape)
        lim = (Kpad + self.c) * U * S
        if h3:
            lim = lim + 2.0 ** -22 * S
        if flips:
            lim = lim + BF16_FLIPS * 2.0 ** -7 * P8.numpy().reshape(shape) ** 0.125
        self.epilogue(acc, lim, No, ophase, st0)

    def epilogue(self, acc, lim, No, ophase, st0):
        op = self.op
        B, T, N, Cout, Fout = op.B, op.T, op.N, op.Cout, op.Fout
        act = (B, T, Fout, Cout)
        dst = self.out("dst", op.dst, act)
        tv = self.tvalid[:, :, None, None]
        tiles = prg.conv_tiles(T, No, op.bm)
        rowvalid = np.repeat(self.tvalid, No, axis=1)                        # (B, T*No): row q = t*No + o
        c = np.arange(N // 2)
        rv = (c // 32) * 64 + c % 32

        def put(o_, cols, val, l):
            o_.val[:, :, cols], o_.lim[:, :, cols] = val, l
            o_.may[:, :, cols] = True
            o_.must[:, :, cols] = np.broadcast_to(tv, val.shape)

        if op.epi == prg.EPI_PHASE2:
            assert op.ostride == 2 and op.ophase == 0 and op.aux is None and op.dst_acc is None and op.nsets <= 1
            assert Cout == N // 2
            n1 = Fout // 2
            put(dst, np.arange(0, 2 * No, 2), acc[..., rv], lim[..., rv])
            put(dst, np.arange(1, 2 * n1, 2), acc[..., rv + 32][:, :, :n1], lim[..., rv + 32][:, :, :n1])
            if op.stats is not None:
                ok1 = np.tile(2 * np.arange(No) + 1 < Fout, T)[None, :] & rowvalid
                g0, g1 = acc[..., rv].reshape(B, T * No, Cout), acc[..., rv + 32].reshape(B, T * No, Cout)
                l0, l1 = lim[..., rv].reshape(B, T * No, Cout), lim[..., rv + 32].reshape(B, T * No, Cout)
                a = None if op.stat_slope0 is None else self.v(op.stat_slope0, (Cout,)).astype(np.float64)
                self.put_stats("stats", op.stats, op.stat_tiles, op.nsets, Cout, 0, st0, tiles,
                               [(self.prelu(g0, a), self.prelu_lim(l0, a), rowvalid), (self.prelu(g1, a), self.prelu_lim(l1, a), ok1)])
            return
        if op.epi in (prg.EPI_GLU, prg.EPI_DUALGATE):
            a, g, la, lg = acc[..., rv], acc[..., rv + 32], lim[..., rv], lim[..., rv + 32]
            sg = _sig(g)
            out = a * sg
            lo = sg * la + np.abs(a) * sg * (1 - sg) * lg + 0.25 * la * lg + np.abs(out) * ((np.abs(g) + 6) * 2.0 ** -23 + 2 * U)
            if op.glu_dump is not None:
                # training: the two factors of every row this launch produces, [B][T][Fout][N] in the packed column order --
                # value columns acc + bias (the accumulator's own limit), gate columns sigmoid(acc + bias) (sigmoid' <= 1/4,
                # |sigmoid''| < 0.1, and the epilogue's allowance for the device's exp and reciprocal)
                dump = self.out("glu_dump", op.glu_dump, (B, T, Fout, N))
                dv, dl = np.empty(acc.shape), np.empty(acc.shape)
                dv[..., rv], dl[..., rv] = a, la
                dv[..., rv + 32] = sg
                dl[..., rv + 32] = sg * (1 - sg) * lg + 0.1 * lg * lg + sg * ((np.abs(g) + 6) * 2.0 ** -23 + 2 * U)
                put(dump, np.arange(No) * op.ostride + ophase, dv, dl)
        else:
            out, lo = acc, lim
        assert out.shape[-1] == Cout
        fo = np.arange(No) * op.ostride + ophase
        if op.epi == prg.EPI_RELU:
            out = np.maximum(out, 0)
        elif op.epi == prg.EPI_MULSIG:
            aux = self.v(op.aux, act)[:, :, fo].astype(np.float64)
            sg = _sig(out)
            lo = np.abs(aux) * sg * (1 - sg) * lo + np.abs(aux * sg) * ((np.abs(out) + 6) * 2.0 ** -23 + 2 * U)
            out = aux * sg
        elif op.epi == prg.EPI_ADD:
            out = out + self.v(op.aux, act)[:, :, fo].astype(np.float64)
            lo = lo + U * np.abs(out)
        put(dst, fo, out, lo)
        if op.dst_acc is not None:
            accd = self.out("dst_acc", op.dst_acc, act)
            new = self.v(op.dst_acc, act)[:, :, fo].astype(np.float64) + out
            put(accd, fo, new, lo + U * np.abs(new))
        if op.stats is not None:
            g, l = out.reshape(B, T * No, Cout), lo.reshape(B, T * No, Cout)
            for s, slr in enumerate((op.stat_slope0, op.stat_slope1)[:op.nsets]):
                a = None if slr is None else self.v(slr, (Cout,)).astype(np.float64)
                self.put_stats("stats", op.stats, op.stat_tiles, op.nsets, Cout, s, st0, tiles,
                               [(self.prelu(g, a), self.prelu_lim(l, a), rowvalid)])

    @staticmethod
    def prelu(g, a):
        return g if a is None else np.where(g > 0, g, a * g)

    @staticmethod
    def prelu_lim(l, a):      # PReLU is max(1, |a|)-Lipschitz; its product rounds once more (inside the statistics' own slack)
        return l if a is None else l * np.maximum(1.0, np.abs(a))

    def put_stats(self, name, ref, stat_tiles, nsets, C, s, st0, tiles, parts):
        op = self.op
        shape = (op.B, stat_tiles, nsets, C, 4)
        o = self.out(name, ref, shape)
        if not o.may.any() and ref is not None:           # partials of the other launches feeding this norm: kept as they are
            o.val[:] = read(self.arena, ref, shape).astype(np.float64)
        n, mean, M2, lmean, lM2 = _tile_stats(parts, op.bm, tiles)
        sl = slice(st0, st0 + tiles)
        o.val[:, sl, s, :, 0], o.val[:, sl, s, :, 1], o.val[:, sl, s, :, 2], o.val[:, sl, s, :, 3] = n, mean, M2, 0.0
        o.lim[:, sl, s, :, 0], o.lim[:, sl, s, :, 1], o.lim[:, sl, s, :, 2], o.lim[:, sl, s, :, 3] = 0.0, lmean, lM2, 0.0
        # a tile wholly past an utterance's length writes n = 0; its mean and M2 carry no information (finite is all the
        # merge needs): limit = inf there
        empty = n == 0
        o.lim[:, sl, s, :, 1][empty] = np.inf
        o.lim[:, sl, s, :, 2][empty] = np.inf
        o.must[:, sl, s], o.may[:, sl, s] = True, True

    # -- whole launch ------------------------------------------------------------------------------------------------------
    def weights(self, w2d, ntaps, Ct):
        """packed [N][Kpad] of the tap- or chunk-ordered form -> operands and magnitudes [N][ntaps][upt*16] in float64"""
        op = self.op
        upt = (Ct + 15) // 16

        def by_tap(a):
            if op.korder == prg.KORDER_CHUNK:
                return a.reshape(op.N, upt, ntaps, 16).transpose(0, 2, 1, 3).reshape(op.N, ntaps, upt * 16)
            return a.reshape(op.N, ntaps, upt * 16)
        if op.precision == prg.PREC_F16X3:
            hi, lo = unpack_f16x3(w2d, op.N, w2d.shape[1])
            W = by_tap(hi).astype(np.float64) + by_tap(lo).astype(np.float64)
        elif op.precision == prg.PREC_BF16:
            W = by_tap(bf16_round(w2d)).astype(np.float64)
        else:
            W = by_tap(np.asarray(w2d, np.float32)).astype(np.float64)
        assert not np.any(W[:, :, Ct:]), "padding columns of the packed weights must be zero"
        return W, np.abs(W)

    def run(self) -> Dict[str, Out]:
        op = self.op
        src = self.sources()
        Ct = src[0].shape[-1]
        upt = (Ct + 15) // 16
        tiles_launch = 0
        if op.korder == prg.KORDER_FRAG:
            dual = op.epi in (prg.EPI_DUALGATE, prg.EPI_GLU)
            order = prg.glu_row_order(op.N) if dual else np.arange(op.N)
            bias = None if op.bias is None else self.v(op.bias, (op.N,)).astype(np.float64)
            if bias is not None and op.epi == prg.EPI_GLU:
                bias = bias[order]       # the small-tile kernel reads the bias in the convolution's own row order
            passes = [(op.w, op.Kpad, op.No, op.ophase, op.dt, op.ioff, op.stat_tile0)]
            if op.ph1_No > 0:
                passes.append((op.ph1_w, op.ph1_Kpad, op.ph1_No, op.ph1_ophase, op.ph1_dt, op.ph1_ioff,
                               op.stat_tile0 + prg.conv_tiles(op.T, op.No, op.bm)))
            frag = dataclasses.replace(op, korder=prg.KORDER_TAP)
            for wref, K, No_, oph, dt, ioff, st0 in passes:
                assert K == len(dt) * upt * 16
                w2d = prg.unpack_frag(self.v(wref, (op.N * K,)), op.N, K, dual)[order]
                self.op = frag
                W, Wa = self.weights(w2d, len(dt), Ct)
                self.conv_pass(W, Wa, bias, K, No_, oph, list(dt), list(ioff), st0, src)
                self.op = op
                tiles_launch += prg.conv_tiles(op.T, No_, op.bm)
        else:
            assert op.Kpad == len(op.dt) * upt * 16
            W, Wa = self.weights(self.v(op.w, (op.N, op.Kpad)), len(op.dt), Ct)
            bias = None if op.bias is None else self.v(op.bias, (op.N,)).astype(np.float64)
            self.conv_pass(W, Wa, bias, op.Kpad, op.No, op.ophase, list(op.dt), list(op.ioff), op.stat_tile0, src)
            tiles_launch = prg.conv_tiles(op.T, op.No, op.bm)
        if op.f2_w is not None:
            self.second_1x1()
        if op.fz_counter is not None and op.stats is not None:
            self.fused_finalize(tiles_launch)
        return self.outs

    def second_1x1(self):
        op = self.op
        B, T, N, N2 = op.B, op.T, op.N, op.f2_N
        assert op.No == 1 and op.Fin == 1 and op.Fout == 1 and op.precision == prg.PREC_F32
        d = self.outs["dst"]
        W2 = _t(prg.unpack_frag(self.v(op.f2_w, (N2 * N,)), N2, N))
        x, l = _t(d.val.reshape(B * T, N)), _t(d.lim.reshape(B * T, N))
        val = (x @ W2.T).numpy().reshape(B, T, 1, N2)
        lim = ((N + 2) * U * (x.abs() @ W2.abs().T) + l @ W2.abs().T).numpy().reshape(B, T, 1, N2)
        o = self.out("f2_dst", op.f2_dst, (B, T, 1, N2))
        o.val[:], o.lim[:], o.may[:] = val, lim, True
        o.must[:] = self.tvalid[:, :, None, None]
        if op.f2_stats is not None:
            tiles = prg.conv_tiles(T, 1, op.bm)
            g, lg = val.reshape(B, T, N2), lim.reshape(B, T, N2)
            for s, slr in enumerate((op.f2_stat_slope0, op.f2_stat_slope1)[:op.f2_nsets]):
                a = None if slr is None else self.v(slr, (N2,)).astype(np.float64)
                self.put_stats("f2_stats", op.f2_stats, op.f2_stat_tiles, op.f2_nsets, N2, s, 0, tiles,
                               [(self.prelu(g, a), self.prelu_lim(lg, a), self.tvalid)])

    def fused_finalize(self, tiles_launch):
        op = self.op
        B, Cout = op.B, op.Cout
        cnt0 = self.v(op.fz_counter, (B,)).view(np.int32).astype(np.int64)
        cnt = cnt0 + tiles_launch
        assert np.all(cnt <= op.stat_tiles), f"{op.name}: arrival counter beyond stat_tiles"
        co = self.out("fz_counter", op.fz_counter, (B,), integer=True)
        co.must[:], co.may[:] = True, True
        done = cnt == op.stat_tiles
        co.val[:] = np.where(done, 0, cnt)
        st = self.outs["stats"]
        for s, (g, b, xf) in enumerate(((op.fz_gamma0, op.fz_beta0, op.fz_xf0), (op.fz_gamma1, op.fz_beta1, op.fz_xf1))[:op.nsets]):
            o = self.out(f"fz_xf{s}", xf, (B, Cout, 2))
            if not done.any():
                continue
            v, l = st.val[:, :, s], st.lim[:, :, s]
            assert not np.isnan(v[done]).any(), f"{op.name}: statistics partials not fully written"
            n, mu, m2 = v[..., 0], v[..., 1], v[..., 2]
            lmu, lm2 = np.where(n > 0, l[..., 1], 0.0), np.where(n > 0, l[..., 2], 0.0)
            mu, m2 = np.where(n > 0, mu, 0.0), np.where(n > 0, m2, 0.0)
            N, mean, M2 = _merge(n, mu, m2)
            dmean = (n * lmu).sum(1) / N
            dM2 = lm2.sum(1) + (n * (2 * np.abs(mu - mean[:, None]) * (lmu + dmean[:, None]) + (lmu + dmean[:, None]) ** 2)).sum(1)
            var = M2 / N
            gam, bet = self.v(g, (Cout,)).astype(np.float64), self.v(b, (Cout,)).astype(np.float64)
            scale = gam / np.sqrt(var + op.fz_eps)
            dscale = np.abs(scale) * (dM2 / N) / (2 * (var + op.fz_eps)) + 2 * U * np.abs(scale)
            shift = bet - mean * scale
            dshift = dmean * np.abs(scale) + np.abs(mean) * dscale + dmean * dscale + 2 * U * (np.abs(bet) + np.abs(mean * scale))
            o.val[done, :, 0], o.val[done, :, 1] = scale[done], shift[done]
            o.lim[done, :, 0], o.lim[done, :, 1] = dscale[done], dshift[done]
            o.must[done], o.may[done] = True, True


def conv_ref(op: prg.ConvOp, arena: Dict[str, np.ndarray], lens=None) -> Dict[str, Out]:
    """float64 value, derived limit and written set of everything the launch ``op`` writes, from the arrays in ``arena`` as
    they are BEFORE the launch.  lens: per-utterance frame counts (eab_time_window.lens) or None."""
    with np.errstate(over="ignore", invalid="ignore"):
        return _Launch(op, arena, lens).run()


def conv_f32(op: prg.ConvOp, arena: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """the plain fp32 CPU evaluation of the same op (the emulator's conv) on a copy of ``arena``: the yardstick of the
    statistical criterion and the subject of the CPU tests"""
    emu = Emulator.__new__(Emulator)
    emu.p = None
    emu.arena = {k: v.copy() for k, v in arena.items()}
    with np.errstate(over="ignore", invalid="ignore"):
        emu.conv(op)
    return {k: v for k, v in emu.arena.items() if not k.startswith("tmp")}


# ----------------------------------------------------------------------------------------------------------------------
# the comparator
# ----------------------------------------------------------------------------------------------------------------------
def _l2(err, val):
    return float(np.linalg.norm(err) / max(np.linalg.norm(val), 1e-300))


def check(outs: Dict[str, Out], got: Dict[str, np.ndarray], yard: Optional[Dict[str, np.ndarray]] = None, what: str = "",
          margin: float = MARGIN, got_is_region: bool = False):
    """Both criteria for every output of a launch.  got / yard: arenas after the launch (device result / fp32 CPU
    evaluation), or with got_is_region a dict name -> array of the output's shape.  Returns (worst err / limit,
    worst L2 ratio against the yardstick or None); raises AssertionError naming the first violation."""
    worst, worst_l2 = 0.0, None
    for name, o in outs.items():
        g = got[name] if got_is_region else read(got, o.ref, o.shape)
        if o.integer:
            g = np.ascontiguousarray(g, np.float32).view(np.int32)
            assert np.array_equal(g[o.must], o.val[o.must].astype(np.int32)), f"{what} {name}: {g} != {o.val}"
            continue
        if not o.must.any():
            continue
        g = np.asarray(g, np.float64)
        gv, vv, lv = g[o.must], o.val[o.must], o.lim[o.must]
        assert np.isfinite(vv).all() and not np.isnan(lv).any(), f"{what} {name}: the float64 reference itself is not finite"
        fin = np.isfinite(lv)
        assert np.isfinite(gv).all(), f"{what} {name}: {int((~np.isfinite(gv)).sum())} written elements are not finite"
        err = np.abs(gv - vv)
        bad = fin & (err > lv)
        if bad.any():
            k = int(np.argmax(np.where(fin, err / np.maximum(lv, 1e-300), 0.0)))
            idx = tuple(int(a[k]) for a in np.nonzero(o.must))
            raise AssertionError(f"{what} {name}: {int(bad.sum())} elements beyond the derived limit; worst at {idx}: "
                                 f"got {gv[k]:.9g}, float64 {vv[k]:.9g}, error {err[k]:.3e}, limit {lv[k]:.3e}")
        pos = fin & (lv > 0)
        if pos.any():
            worst = max(worst, float((err[pos] / lv[pos]).max()))
        if name in L2_NAMES and yard is not None:
            y = np.asarray(yard[name] if got_is_region else read(yard, o.ref, o.shape), np.float64)[o.must]
            e_got, e_yard = _l2(gv - vv, vv), max(_l2(y - vv, vv), YARD_FLOOR)
            ratio = e_got / e_yard
            assert ratio <= margin, (f"{what} {name}: L2-relative error {e_got:.3e} is {ratio:.1f} x that of the fp32 CPU "
                                     f"evaluation ({e_yard:.3e}); allowed {margin:g} x")
            worst_l2 = ratio if worst_l2 is None else max(worst_l2, ratio)
    return worst, worst_l2


# ----------------------------------------------------------------------------------------------------------------------
# which kernel variants the lowering selects
# ----------------------------------------------------------------------------------------------------------------------
def variant_key(op: prg.ConvOp) -> tuple:
    """what selects a kernel instantiation and its optional code paths: (k-order, bm, N, epilogue, transform, precision,
    concat, statistics sets, in-kernel fin_stats merge, second phase, fused second 1x1, ragged channels, taps)"""
    return (op.korder, op.bm, op.N, op.epi, op.xf_mode, op.precision, op.src1 is not None, op.nsets if op.stats is not None else 0,
            op.fin_stats is not None, op.ph1_No > 0, op.f2_w is not None, (op.C0 + op.C1) % 16 != 0, len(op.dt))


def key_str(k: tuple) -> str:
    ko = {prg.KORDER_TAP: "tap", prg.KORDER_CHUNK: "chunk", prg.KORDER_FRAG: "frag"}[k[0]]
    epi = ["LINEAR", "GLU", "RELU", "MULSIG", "ADD", "DUALGATE", "PHASE2"][k[3]]
    prec = ["f32", "f16x3", "bf16"][k[5]]
    flags = "".join(f for f, on in (("+cat", k[6]), (f"+st{k[7]}", k[7]), ("+fin", k[8]), ("+ph1", k[9]), ("+f2", k[10]), ("+ragC", k[11])) if on)
    return f"{ko}/bm{k[1]}/N{k[2]}/{epi}/xf{k[4]}/{prec}/taps{k[12]}{flags}"


def bench_shapes() -> List[dict]:
    """The programs bench.py measures, read from bench.py's syntax tree (not from its text layout): the headline batch in
    the three precisions and the single-utterance latency row, the 16-microphone
    8-second network of the streaming sections with the default norm and with the norm types those sections build, then the GaGNet post-filter of
    the wave-to-wave section at the headline batch, the batch of the training section, and the post-filter as the streamed
    two-stage model (BatchNorm, one utterance) and the two-stage training runs (training batch, fp32 and bf16) build it.  The streaming sections run the
    same kernels on a time window and the training section runs training programs; what is lowered here for them is the
    OFFLINE INFERENCE program of the same network, batch and length, which selects the same forward kernel variants."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "bench.py")) as f:
        tree = ast.parse(f.read())
    consts, stream_nets, t_max, gag_all, train, over, enh = {}, [], set(), [], None, None, None

    def lit(node):
        if isinstance(node, ast.Name) and node.id in consts:
            return consts[node.id]
        return ast.literal_eval(node)
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Tuple) and isinstance(node.value, ast.Tuple):
            names = [t.id if isinstance(t, ast.Name) else None for t in node.targets[0].elts]
            try:
                vals = [lit(v) for v in node.value.elts]
            except (ValueError, SyntaxError):
                continue
            if names == ["B", "M", "seconds"]:
                train = dict(zip(names, vals))
            elif all(n and n.isupper() for n in names):
                consts.update(zip(names, vals))
        elif isinstance(node, ast.Call):
            fn = node.func.attr if isinstance(node.func, ast.Attribute) else getattr(node.func, "id", "")
            kws = {k.arg: k.value for k in node.keywords}
            if fn == "EaBNet" and "norm_type" in kws:
                stream_nets.append((lit(kws["M"]), lit(kws["norm_type"])))
            elif fn == "stream_begin" and "T_max" in kws:
                t_max.add(lit(kws["T_max"]))
            elif fn == "Namespace" and "gagnet_k1" in kws:
                gag_all.append({k[len("gagnet_"):]: lit(v) for k, v in kws.items() if k.startswith("gagnet_")})
            elif fn == "Namespace" and None in kws and isinstance(kws[None], ast.Dict):
                # Namespace(**{**vars(pa), "M": .., "gagnet_norm_type": ..}): the two-stage model of the wave-to-wave stream
                d = {k.value: lit(v) for k, v in zip(kws[None].keys, kws[None].values) if isinstance(k, ast.Constant)}
                if "gagnet_norm_type" in d:
                    over = d
            elif fn == "StreamingEnhancer" and "seconds" in kws:
                enh = dict(B=lit(kws["B"]), seconds=lit(kws["seconds"]))
    assert stream_nets and len(t_max) == 1 and gag_all and train and over and enh, "bench.py no longer states the shapes of its sections"
    # the wave-to-wave section and the two-stage training section each spell the post-filter out: they must be the same one
    assert all(g == gag_all[0] for g in gag_all), "bench.py builds two different post-filters: pin each where it is used"
    gag_kw = gag_all[0]
    B, M = consts["B_PER_GPU"], consts["MICS"]
    frames = lambda sec: 1 + int(sec * consts["SR"]) // consts["HOP"]      # noqa: E731
    T = frames(consts["SECONDS"])
    shapes = [dict(M=M, B=B, T=T, precision=p) for p in ("f32", "f16x3", "bf16")]
    shapes += [dict(M=M, B=1, T=T, precision="f32")]
    shapes += [dict(M=max(m for m, _ in stream_nets), B=1, T=t_max.copy().pop(), precision="f32")]   # (default norm: InstanceNorm)
    for Ms, norm in sorted(set(stream_nets)):
        shapes += [dict(M=Ms, B=1, T=t_max.copy().pop(), precision=p, kw=dict(norm_type=norm)) for p in ("f32", "bf16")]
    shapes += [dict(M=M, B=B, T=T, precision=p, gag=gag_kw) for p in ("f32", "f16x3")]
    shapes += [dict(M=train["M"], B=train["B"], T=frames(train["seconds"]), precision=p) for p in ("f32", "bf16")]
    # the post-filter of the streamed two-stage model (its own norm type, one utterance) and of the two-stage training runs
    shapes += [dict(M=over["M"], B=enh["B"], T=frames(enh["seconds"]), precision="f32", gag={**gag_kw, "norm_type": over["gagnet_norm_type"]})]
    shapes += [dict(M=train["M"], B=train["B"], T=frames(train["seconds"]), precision=p, gag=gag_kw) for p in ("f32", "bf16")]
    return shapes


def shape_str(s: dict) -> str:
    net = ("GaGNet" + ("" if s["gag"]["norm_type"] == "IN" else " " + s["gag"]["norm_type"])) if "gag" in s else f"M{s['M']}" + "".join(f" {v}" for v in s.get("kw", {}).values())
    return f"{net} B{s['B']} T{s['T']} {s['precision']}"


PER_OP_SHAPES = [(8, 1, 12, (6, 3), "f32"), (9, 2, 21, (2, 1), "f32"), (16, 1, 9, (1, 1), "f32"), (8, 2, 21, (2, 1), "f16x3"),
                 (9, 1, 12, (1, 1), "f16x3"), (8, 2, 21, (2, 1), "bf16")]      # test_every_op_matches_the_emulator


def lower_shape(shape: dict, varlen: bool = False) -> prg.Program:
    import paramgen
    from eabnet_amd.spec import GagConfig, NetConfig, gag_param_specs, param_specs
    if "gag" in shape:
        cfg = GagConfig(cin=2, **{k: (tuple(v) if isinstance(v, list) else v) for k, v in shape["gag"].items()})
        P = paramgen.make_params(gag_param_specs(cfg), 77)
    else:
        cfg = NetConfig(M=shape["M"], **shape.get("kw", {}))
        P = paramgen.make_params(param_specs(cfg), 50 + shape["M"])
    return prg.lower(cfg, P, shape["B"], shape["T"], 161, precision=shape["precision"], varlen=varlen)


def variants_of(prog: prg.Program) -> Dict[tuple, List[int]]:
    out: Dict[tuple, List[int]] = {}
    for k, op in enumerate(prog.ops):
        if op.kind == prg.OP_CONV:
            out.setdefault(variant_key(op), []).append(k)
    return out


def chosen_ops(prog: prg.Program) -> List[Tuple[tuple, int]]:
    """per variant key of the program: the op with the most ragged last tile (smallest non-zero T*No mod bm), and, if it is
    another one, the op with the largest Kpad"""
    out = []
    for key, idx in sorted(variants_of(prog).items()):
        def rag(k):
            r = (prog.ops[k].T * prog.ops[k].No) % prog.ops[k].bm
            return r if r else 1 << 30
        a = min(idx, key=rag)
        b = max(idx, key=lambda k: prog.ops[k].Kpad)
        out.append((key, a))
        if prog.ops[b].Kpad > prog.ops[a].Kpad:
            out.append((key, b))
    return out


def bench_variants() -> Dict[int, Dict[tuple, List[int]]]:
    """shape index (bench_shapes order) -> variant key -> op indices: THE enumeration the GPU test walks and the census pins"""
    return {i: variants_of(lower_shape(s)) for i, s in enumerate(bench_shapes())}


# ----------------------------------------------------------------------------------------------------------------------
# seeded random operands for one launch cut out of its program
# ----------------------------------------------------------------------------------------------------------------------
def launch_tiles(op: prg.ConvOp) -> int:
    return prg.conv_tiles(op.T, op.No, op.bm) + (prg.conv_tiles(op.T, op.ph1_No, op.bm) if op.ph1_No > 0 else 0)


def _triples(rng, nutt, tiles, nsets, C, count):
    """consistent Welford partials (n, mean, M2 >= 0, 0): counts that add up to ``count``, unit-scale moments"""
    n = np.full(tiles, count // tiles, np.float64)
    n[-1] += count - n.sum()
    st = np.zeros((nutt, tiles, nsets, C, 4), np.float32)
    st[..., 0] = n[None, :, None, None]
    st[..., 1] = 0.3 * rng.standard_normal((nutt, tiles, nsets, C))
    st[..., 2] = st[..., 0] * rng.uniform(0.5, 1.5, (nutt, tiles, nsets, C))
    return st


def random_inputs(op: prg.ConvOp, rng: np.random.Generator, nutt: int = 2) -> Dict[prg.Ref, np.ndarray]:
    """Seeded random data for exactly the batched arrays the launch reads, ``nutt`` utterances each (shape (nutt, ...)):
    sources, aux and dst_acc standard normal; (scale, shift) tables with scales of both signs around 1; the producer's
    partials (fin_stats) and the partials of the OTHER launches feeding the same norm as consistent triples, this launch's
    own tiles NaN; the arrival counter as if every other launch had arrived.  Weights, slopes and norm parameters are the
    program's own and are not part of this."""
    out: Dict[prg.Ref, np.ndarray] = {}
    for field, ref, shape, batched, mode in regions(op):
        if not batched or mode == "w" or ref in out or ref.arena == "w":     # (static tables of the weight arena stay)
            continue
        s = (nutt,) + tuple(shape[1:])
        if field in ("xf0", "xf1"):
            a = np.empty(s, np.float32)
            a[..., 0] = rng.uniform(0.5, 1.5, s[:-1]) * rng.choice([-1.0, 1.0], s[:-1])
            a[..., 1] = 0.3 * rng.standard_normal(s[:-1])
        elif field == "fin_stats":
            a = _triples(rng, nutt, op.fin_tiles, op.fin_nsets, op.C0, max(op.fin_count, op.fin_tiles))
        elif field == "stats":
            a = _triples(rng, nutt, op.stat_tiles, op.nsets, op.Cout, op.stat_tiles * op.bm)
            a[:, op.stat_tile0:op.stat_tile0 + launch_tiles(op)] = np.nan
        elif field == "fz_counter":
            a = np.full(s, op.stat_tiles - launch_tiles(op), np.int32).view(np.float32)
        else:
            a = rng.standard_normal(s).astype(np.float32)
        out[ref] = a
    return out


def cut_out(op: prg.ConvOp, weights: np.ndarray, inputs: Dict[prg.Ref, np.ndarray]):
    """localize() on the program's weight arena and random_inputs(): (op', arena') for conv_ref / conv_f32; arrays the
    launch only writes start as NaN"""
    nutt = next(iter(inputs.values())).shape[0]

    def fetch(field, ref, shape, batched):
        if ref in inputs:
            return inputs[ref]
        if ref.arena == "w":
            return weights[ref.off:ref.off + int(np.prod(shape))].reshape(shape)
        assert batched, (field, ref)
        return np.full((nutt,) + tuple(shape[1:]), np.nan, np.float32)
    return localize(op, fetch, nutt)
