"""float64 reference of the training ops under per-utterance lengths  (TEST INFRASTRUCTURE; numpy only).

Nothing here re-derives an op: every function cuts utterance b's first lens[b] frames out of the padded batch, calls the
UNMASKED reference of tests/train_ref.py (or tests/conv_ref.py for a convolution) on that slice as a batch of one, and puts
the results back -- per-utterance outputs into the valid rows, parameter gradients added utterance by utterance in batch
order (their limits add).  What a masked kernel must leave alone or write as zeros is said by the `must` set and the value:

    op              valid rows                  padding rows (t >= lens[b])
    IN_STATS        y, xf, mr of the slice      y not written (must False)
    NORM_BWD(+MULTI) dx of the slice            dx not written;  dgamma / dbeta / dslope from valid rows only
    LN_BWD          dx of the slice             dx row-local, not compared;  dg / db from valid rows only
    LSTM_BWD        dgates of the slice         dgates = 0 (compared)
    FILTER_SUM      y of the slice              y = 0 exactly (limit 0)
    WGRAD           dw, dbias summed over the slices
    CONV            dst of the slice            dst not written; no tap reads a source row >= lens[b]

The padding rows of the INPUTS never enter: a test fills them with NaN.  dtype float32 gives train_ref's yardstick."""
from __future__ import annotations

import dataclasses
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

import conv_ref as cr
import train_ref as tref
from eabnet_amd import program as prg


def _out(name, val, lim, must, **kw) -> tref.Out:
    val = np.asarray(val)
    return tref.Out(None, val.shape, val, np.asarray(lim, np.float64), np.asarray(must, bool), np.asarray(must, bool), name=name, **kw)


def _chain(prev, res, names):
    """parameter gradients of one utterance added to the running (value, limit): the reference of a batch of one already adds
    its `prev`, so the value chains through the calls and the limits add"""
    for n in names:
        if n in res:
            v, l = res[n][0], np.asarray(res[n][1], np.float64)
            prev[n] = (v, l + (prev[n][1] if n in prev and prev[n][1] is not None else 0.0))
    return prev


def _lens_ok(lens, B, T):
    lens = [int(v) for v in lens]
    assert len(lens) == B and all(1 <= n <= T for n in lens), (lens, B, T)
    return lens


# ----------------------------------------------------------------------------------------------------------------------
# statistics and norm backward:  [B][P][C] with P = T * ppf positions
# ----------------------------------------------------------------------------------------------------------------------
def in_stats(i, f, A, lens, T, dtype=np.float64, multi=False) -> Dict[str, tref.Out]:
    B, P, C = i[0], i[1], i[2]
    xC = i[3] if multi else C
    lens, ppf = _lens_ok(lens, B, T), P // T
    assert ppf * T == P
    x = np.asarray(A["x"]).reshape(B, P, xC)
    form = "IN_STATS_MULTI" if multi else "IN_STATS"
    nv = C // xC
    xf, mr = np.zeros((B, C, 2), dtype), np.zeros((B, C, 2), dtype)
    Lxf, Lmr = np.zeros((B, C, 2)), np.zeros((B, C, 2))
    yshape = (nv, B, P, xC) if multi else (B, P, C)
    y, Ly, My = np.zeros(yshape, dtype), np.zeros(yshape), np.zeros(yshape, bool)
    for b, n in enumerate(lens):
        Pn = n * ppf
        Ab = dict(A, x=x[b:b + 1, :Pn])
        res, _ = tref.run_ref(form, [1, Pn, C, xC if multi else 0], f, Ab, dtype)
        xf[b], Lxf[b], mr[b], Lmr[b] = res["xf"][0][0], res["xf"][1][0], res["mr"][0][0], res["mr"][1][0]
        if "y" in A:
            if multi:
                y[:, b, :Pn], Ly[:, b, :Pn], My[:, b, :Pn] = res["y"][0][:, 0], res["y"][1][:, 0], True
            else:
                y[b, :Pn], Ly[b, :Pn], My[b, :Pn] = res["y"][0][0], res["y"][1][0], True
    outs = {"xf": _out("xf", xf, Lxf, np.ones(xf.shape, bool)), "mr": _out("mr", mr, Lmr, np.ones(mr.shape, bool))}
    if "y" in A:
        outs["y"] = _out("y", y, Ly, My)
    return outs


def norm_bwd(i, f, A, lens, T, dtype=np.float64) -> Tuple[Dict[str, tref.Out], int]:
    """single (i = [B, P, C, mode]) or multi-view (i = [B, P, C, mode, xC]) form; returns (outs, ambiguous elements)"""
    B, P, C = i[0], i[1], i[2]
    multi = len(i) > 4 and i[4] > 0
    xC = i[4] if multi else C
    lens, ppf = _lens_ok(lens, B, T), P // T
    assert ppf * T == P
    form = "NORM_BWD_MULTI" if multi else "NORM_BWD"
    rows = ("dy", "x", "acc_in") + (("dy1",) if multi else ())
    dx, Ldx, Mdx = np.zeros((B, P, xC), dtype), np.zeros((B, P, xC)), np.zeros((B, P, xC), bool)
    params = {n: (np.asarray(A[n]), None) for n in ("dgamma", "dbeta", "dslope") if A.get(n) is not None}
    amb = 0
    for b, n in enumerate(lens):
        Pn = n * ppf
        Ab = dict(A)
        for r in rows:
            if A.get(r) is not None and (multi or r != "dy1"):
                Ab[r] = np.asarray(A[r])[b:b + 1, :Pn]
        if not multi and A.get("beta") is not None:
            Ab["beta"] = A["beta"]
        if A.get("mr") is not None:
            Ab["mr"] = np.asarray(A["mr"])[b:b + 1]
        for k in params:
            Ab[k] = params[k][0]
        ib = [1, Pn, C, i[3]] + ([xC] if multi else [])
        res, a = tref.run_ref(form, ib, f, Ab, dtype)
        amb += a
        dx[b, :Pn], Ldx[b, :Pn] = res["dx"][0][0], res["dx"][1][0]
        Mdx[b, :Pn] = res["dx"][2][0] if len(res["dx"]) > 2 else True
        params = _chain(params, res, ("dgamma", "dbeta", "dslope"))
    outs = {"dx": _out("dx", dx, Ldx, Mdx)}
    for k, (v, l) in params.items():
        outs[k] = _out(k, v, l if l is not None else np.zeros(np.shape(v)), np.ones(np.shape(v), bool))
    return outs, amb


# ----------------------------------------------------------------------------------------------------------------------
# the head:  LayerNorm backward, LSTM backward, filter-and-sum
# ----------------------------------------------------------------------------------------------------------------------
def ln_bwd(A, lens, B, T, dtype=np.float64) -> Dict[str, tref.Out]:
    rows = np.asarray(A["x"]).shape[0]
    F = rows // (B * T)
    lens = _lens_ok(lens, B, T)
    v4 = lambda a, c: np.asarray(a).reshape(B, T, F, c)                              # noqa: E731
    dx, Ldx, Mdx = np.zeros((B, T, F, 64), dtype), np.zeros((B, T, F, 64)), np.zeros((B, T, F, 64), bool)
    params = {"dg": (np.asarray(A["dg"]), None), "db": (np.asarray(A["db"]), None)}
    for b, n in enumerate(lens):
        Ab = dict(A, dy=v4(A["dy"], 64)[b, :n].reshape(-1, 64), x=v4(A["x"], 64)[b, :n].reshape(-1, 64),
                  mr=v4(A["mr"], 2)[b, :n].reshape(-1, 2), dg=params["dg"][0], db=params["db"][0])
        nr = n * F
        res, _ = tref.run_ref("LN_BWD", [nr & 0xFFFFFFFF, nr >> 32], [], Ab, dtype)
        dx[b, :n], Ldx[b, :n], Mdx[b, :n] = res["dx"][0].reshape(n, F, 64), res["dx"][1].reshape(n, F, 64), True
        params = _chain(params, res, ("dg", "db"))
    outs = {"dx": _out("dx", dx.reshape(rows, 64), Ldx.reshape(rows, 64), Mdx.reshape(rows, 64))}
    for k, (v, l) in params.items():
        outs[k] = _out(k, v, l, np.ones(64, bool))
    return outs


def lstm_bwd(i, A, lens, dtype=np.float64) -> Dict[str, tref.Out]:
    B, T, F = i[0], i[1], i[2]
    lens = _lens_ok(lens, B, T)
    gates = np.asarray(A["gates"]).reshape(B, F, T, 5, 64)
    dh = np.asarray(A["dh_out"]).reshape(B, T, F, 64)
    val = np.zeros((B, T, F, 256), dtype)                         # the padding steps: zeros, written
    for b, n in enumerate(lens):
        Ab = dict(A, gates=gates[b, :, :n].reshape(F, n, 5, 64), dh_out=dh[b:b + 1, :n])
        res, _ = tref.run_ref("LSTM_BWD", [1, n, F, i[3]], [], Ab, dtype)
        val[b, :n] = res["dgates"][0][0]
    return {"dgates": _out("dgates", val, np.full(val.shape, np.inf), np.ones(val.shape, bool), lstm=True)}


def filter_sum(i, A, lens, dtype=np.float64) -> Dict[str, tref.Out]:
    B, T, F = i[0], i[1], i[2]
    lens = _lens_ok(lens, B, T)
    y, Ly = np.zeros((B, 2, T, F), dtype), np.zeros((B, 2, T, F))   # the padding frames: exact zeros (limit 0)
    for b, n in enumerate(lens):
        Ab = dict(A, w=np.asarray(A["w"])[b:b + 1, :n], x=np.asarray(A["x"])[b:b + 1, :n])
        res, _ = tref.run_ref("FILTER_SUM", [1, n, F, i[3], i[4]], [], Ab, dtype)
        y[b, :, :n], Ly[b, :, :n] = res["y"][0][0], res["y"][1][0]
    return {"y": _out("y", y, Ly, np.ones(y.shape, bool))}


# ----------------------------------------------------------------------------------------------------------------------
# contractions
# ----------------------------------------------------------------------------------------------------------------------
def wgrad(op, A, lens, dtype=np.float64) -> Dict[str, tref.Out]:
    """op: train.WgradOp of the padded batch; A: dz, src0[, src1] (B, T, ...), dw[, dbias] (previous values)"""
    lens = _lens_ok(lens, op.B, op.T)
    m = tref._M(dtype)
    params = {n: (np.asarray(A[n]), None) for n in ("dw", "dbias") if A.get(n) is not None}
    for b, n in enumerate(lens):
        sub = dataclasses.replace(op, B=1, T=n)
        Ab = {k: np.asarray(A[k])[b:b + 1, :n] for k in ("dz", "src0", "src1") if A.get(k) is not None}
        Ab.update({k: v[0] for k, v in params.items()})
        with np.errstate(over="ignore", invalid="ignore"):
            res, _ = tref.ref_wgrad(sub, Ab, m)
        params = _chain(params, res, ("dw", "dbias"))
    return {k: _out(k, v, l, np.ones(np.shape(v), bool)) for k, (v, l) in params.items()}


_TIME_FIELDS = ("src0", "src1", "aux", "dst", "dst_acc")


def conv(op: prg.ConvOp, arena: Dict[str, np.ndarray], lens: Sequence[int], yard: Optional[dict] = None) -> Dict[str, tref.Out]:
    """A convolution launch without statistics (the data-gradient launches): per utterance the launch of conv_ref on a batch of
    one of lens[b] frames.  Output rows of the padding frames are not written; with look-ahead taps (dt > 0) the rows just
    below the length see zeros where the padded batch holds padding.  yard: a dict that receives the fp32 yardstick
    (conv_ref.conv_f32 of the same slices) per output."""
    lens = _lens_ok(lens, op.B, op.T)
    assert op.stats is None and op.fin_stats is None and op.fz_counter is None and op.glu_dump is None and op.f2_w is None
    full = {fld: (ref, shape) for fld, ref, shape, _, _ in cr.regions(op)}
    outs: Dict[str, tref.Out] = {}
    for b, n in enumerate(lens):
        sub = dataclasses.replace(op, B=1, T=n)

        def fetch(fld, ref, shape, batched, b=b, n=n):
            a = cr.read(arena, *full[fld])
            if not batched:
                return a
            assert fld in _TIME_FIELDS, f"{fld}: a batched operand this reference does not slice"
            return a[b:b + 1, :n]
        lop, la = cr.localize(sub, fetch)
        y32 = cr.conv_f32(lop, la) if yard is not None else None
        for name, o in cr.conv_ref(lop, la).items():
            if name not in outs:
                shp = full[name][1]
                outs[name] = tref.Out(full[name][0], shp, np.full(shp, np.nan), np.zeros(shp), np.zeros(shp, bool), np.zeros(shp, bool),
                                      name=name)
                if yard is not None:
                    yard[name] = np.zeros(shp, np.float32)
            t = outs[name]
            t.val[b, :n], t.lim[b, :n], t.must[b, :n], t.may[b, :n] = o.val[0], o.lim[0], o.must[0], o.may[0]
            if yard is not None:
                yard[name][b, :n] = cr.read(y32, getattr(lop, name), o.shape)[0]
    return outs
