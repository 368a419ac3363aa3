"""Training on padded batches of unequal-length utterances on a real MI355X.

(a) every masked kernel alone, through the C ABI, against the float64 masked reference (tests/train_varlen_ref.py) with
    train_ref.check (derived per-element limits, L2 error at most conv_ref.MARGIN x the fp32 yardstick's); the padding rows
    of every input are NaN, so a read of one shows as a non-finite result; outputs start from a sentinel, so a write to a
    padding row the kernel promises to leave alone shows too.  With lens = [T] * B every kernel must give its lens == NULL
    result bit for bit -- where the result is a sum that several workgroups add with fp32 atomics (dw, dbias, the parameter
    gradients of the norms and of the LayerNorm) two launches of the SAME call differ in the last bits already, so there the
    comparison is the derived bound of an fp32 sum in any order (both against float64), not torch.equal.
(b)-(f) the network: net(x, lengths=...) under autograd with net.varlen_training = True against fp64 autograd through the
    oracle, ONE UTTERANCE AT A TIME on its own frames (outputs zero-padded and concatenated under autograd, one loss).
All of (b)-(f) fail on a tree without the switch: the call is refused."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

import paramgen
import train_ref as tref
import train_varlen_ref as vref
from eabnet_amd import program as prg
from eabnet_amd import runtime
from eabnet_amd import train as tr
from util import assert_close, torch_params

pytestmark = pytest.mark.gpu

B, T, LENS = 3, 24, [24, 13, 5]
SENTINEL = 7.25
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from eabnet_amd import _lib
    return _lib.load()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ck(code, what=""):
    from eabnet_amd import _lib
    _lib.check(code, what)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")


def _lens(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda:0")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _pad_nan(a, lens=LENS, ppf=1):
    """(B, T * ppf, ...) with NaN behind every length"""
    a = np.array(a, np.float32)
    for b, n in enumerate(lens):
        a[b, n * ppf:] = np.nan
    return a


def _untouched(got, must, what):
    """elements outside the must set still hold the sentinel: the kernel did not write there"""
    g = np.asarray(got)
    assert (g[~must] == np.float32(SENTINEL)).all(), f"{what}: a padding row was written"


def _judge(outs64, outs32, got, what, sentinel=()):
    for n in sentinel:
        _untouched(got[n], outs64[n].must, f"{what} {n}")
    yard = None if any(o.lstm for o in outs64.values()) else {n: o.val for n, o in outs32.items()}
    worst, l2 = tref.check(outs64, got, yard, what)
    print(f"MASKED {what} | err/limit {worst:.3f} | L2 ratio {'-' if l2 is None else format(l2, '.2f')}")


def _same_sum(a, b, ref: tref.Out, what):
    """two fp32 sums of the same terms in different orders: each within the derived limit of float64, so within twice that of
    each other"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    assert (d <= 2 * ref.lim).all(), f"{what}: full lengths differ from the lens == NULL call by more than two summation bounds"


# ----------------------------------------------------------------------------------------------------------------------
# (a) InstanceNorm statistics: eab_train_in_stats / in1d / in1d_multi
# ----------------------------------------------------------------------------------------------------------------------
def _in_stats(lib, form, h, Bq, P, Cc, xC, Tq, lens):
    x, sl, ga, be = (_d(h[k]) for k in ("x", "slope", "gamma", "beta"))
    xf, mr = torch.full((Bq, Cc, 2), SENTINEL, device="cuda:0"), torch.full((Bq, Cc, 2), SENTINEL, device="cuda:0")
    y = None if form == "stats" else torch.full((Cc // xC, Bq, P, xC) if form == "multi" else (Bq, P, Cc), SENTINEL, device="cuda:0")
    ld = _lens(lens)
    tail = (_ptr(ld), Tq if lens is not None else 0, _st())
    if form == "stats":
        _ck(lib.eab_train_in_stats_lens_f32(x.data_ptr(), sl.data_ptr(), Bq, P, Cc, EPS, ga.data_ptr(), be.data_ptr(), xf.data_ptr(),
                                            mr.data_ptr(), *tail))
    elif form == "in1d":
        _ck(lib.eab_train_in1d_lens_f32(x.data_ptr(), sl.data_ptr(), Bq, P, Cc, EPS, ga.data_ptr(), be.data_ptr(), xf.data_ptr(),
                                        mr.data_ptr(), y.data_ptr(), *tail))
    else:
        _ck(lib.eab_train_in1d_multi_lens_f32(x.data_ptr(), sl.data_ptr(), Bq, P, Cc, xC, EPS, ga.data_ptr(), be.data_ptr(),
                                              xf.data_ptr(), mr.data_ptr(), y.data_ptr(), *tail))
    torch.cuda.synchronize()
    out = {"xf": xf.cpu().numpy(), "mr": mr.cpu().numpy()}
    if y is not None:
        out["y"] = y.cpu().numpy()
    return out


# ppf = 11: P = 264 >= 256 takes the 1024-thread instance (a lone workgroup per slab)
@pytest.mark.parametrize("form,Cc,ppf", [("stats", 64, 1), ("stats", 256, 3), ("in1d", 64, 1), ("in1d", 256, 1), ("in1d", 64, 11),
                                         ("multi", 128, 1), ("multi", 256, 11)])
def test_masked_instance_norm_statistics(lib, form, Cc, ppf):
    rng = np.random.default_rng(10 + Cc + ppf)
    xC = Cc // 2 if form == "multi" else Cc
    P = T * ppf
    h = dict(x=(1.3 * rng.standard_normal((B, P, xC)) + 0.4).astype(np.float32), slope=rng.uniform(0.05, 0.45, Cc).astype(np.float32),
             gamma=rng.uniform(0.5, 1.5, Cc).astype(np.float32), beta=(0.3 * rng.standard_normal(Cc)).astype(np.float32))
    full = _in_stats(lib, form, h, B, P, Cc, xC, T, [T] * B)
    plain = _in_stats(lib, form, h, B, P, Cc, xC, T, None)
    for k in full:
        assert np.array_equal(full[k].view(np.int32), plain[k].view(np.int32)), f"{form} {k}: full lengths != lens == NULL"
    hp = dict(h, x=_pad_nan(h["x"], ppf=ppf))
    got = _in_stats(lib, form, hp, B, P, Cc, xC, T, LENS)
    A = dict(hp, y=True) if form != "stats" else dict(hp)
    i = [B, P, Cc] + ([xC] if form == "multi" else [])
    o64, o32 = (vref.in_stats(i, [EPS], A, LENS, T, dt, multi=form == "multi") for dt in (np.float64, np.float32))
    _judge(o64, o32, got, f"in_stats {form} C={Cc} P={P}", sentinel=("y",) if form != "stats" else ())


# ----------------------------------------------------------------------------------------------------------------------
# (a) norm backward: reduce + apply (+ the multi-view apply)
# ----------------------------------------------------------------------------------------------------------------------
def _stats_of(v, lens, ppf):
    """(mean, rstd) per (b, c) over the valid positions, as the forward would have left them"""
    mr = np.zeros((v.shape[0], v.shape[2], 2), np.float32)
    for b, n in enumerate(lens):
        s = v[b, :n * ppf].astype(np.float64)
        mr[b, :, 0], mr[b, :, 1] = s.mean(0), 1 / np.sqrt(s.var(0) + EPS)
    return mr


def _norm_bwd(lib, h, Bq, P, Cc, mode, xC, Tq, lens):
    t = {k: (None if h.get(k) is None else _d(h[k])) for k in ("dy", "dy1", "x", "mr", "gamma", "beta", "slope", "acc_in")}
    sums = torch.zeros(tr.NB_SUM_COPIES, Bq, Cc, 4, device="cuda:0")
    dx = torch.full(h["x"].shape, SENTINEL, device="cuda:0")
    dg, db, ds = (_d(h[k]) for k in ("dgamma", "dbeta", "dslope"))
    ld = _lens(lens)
    tail = (_ptr(ld), Tq if lens is not None else 0, _st())
    if xC:
        _ck(lib.eab_train_norm_bwd_multi_lens_f32(t["dy"].data_ptr(), t["dy1"].data_ptr(), t["x"].data_ptr(), t["mr"].data_ptr(),
                                                  t["gamma"].data_ptr(), t["slope"].data_ptr(), sums.data_ptr(), _ptr(t["acc_in"]),
                                                  dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ds.data_ptr(), Bq, P, xC, *tail))
    else:
        _ck(lib.eab_train_norm_bwd_lens_f32(t["dy"].data_ptr(), t["x"].data_ptr(), _ptr(t["mr"]), _ptr(t["gamma"]), _ptr(t["beta"]),
                                            t["slope"].data_ptr(), sums.data_ptr(), _ptr(t["acc_in"]), dx.data_ptr(), dg.data_ptr(),
                                            db.data_ptr(), ds.data_ptr(), Bq, P, Cc, mode | tr.NB_SUMS_ZEROED, *tail))
    torch.cuda.synchronize()
    out = {"dx": dx.cpu().numpy(), "dslope": ds.cpu().numpy()}
    if h.get("mr") is not None:
        out.update(dgamma=dg.cpu().numpy(), dbeta=db.cpu().numpy())
    return out


# ppf = 11: P = 264 is five reduce / apply blocks of 64 positions per (b, channel group): the utterance of 5 frames ends inside
# the first, the one of 13 frames inside the third -- whole blocks lie behind both
@pytest.mark.parametrize("mode,norm,acc,multi,Cc,ppf", [
    (prg.XF_NORM_PRELU, True, False, False, 64, 11), (prg.XF_NORM_PRELU, True, True, False, 256, 1),
    (prg.XF_NORM_PRELU, False, False, False, 64, 11), (prg.XF_PRELU_NORM, True, True, False, 64, 1),
    (prg.XF_PRELU_NORM, True, False, False, 256, 11), (prg.XF_PRELU_NORM, True, True, True, 128, 1),
    (prg.XF_PRELU_NORM, True, False, True, 256, 11)])
def test_masked_norm_backward(lib, mode, norm, acc, multi, Cc, ppf):
    rng = np.random.default_rng(20 + Cc + ppf + mode)
    xC = Cc // 2 if multi else Cc
    P = T * ppf
    f32 = lambda a: np.asarray(a, np.float32)                                   # noqa: E731
    h = dict(x=f32(1.3 * rng.standard_normal((B, P, xC)) + 0.4), dy=f32(rng.standard_normal((B, P, xC))),
             slope=f32(rng.uniform(0.05, 0.45, Cc)), dslope=f32(rng.standard_normal(Cc)),
             dgamma=f32(rng.standard_normal(Cc)), dbeta=f32(rng.standard_normal(Cc)))
    if multi:
        h["dy1"] = f32(rng.standard_normal((B, P, xC)))
    if acc:
        h["acc_in"] = f32(rng.standard_normal((B, P, xC)))
    if norm:
        h.update(gamma=f32(rng.uniform(0.5, 1.5, Cc)), beta=f32(0.3 * rng.standard_normal(Cc)))

    def with_stats(hh, lens):
        if not norm:
            return hh
        xx = np.concatenate([hh["x"]] * (Cc // xC), -1)
        v = np.where(xx > 0, xx, hh["slope"] * xx) if mode == prg.XF_PRELU_NORM else xx
        return dict(hh, mr=_stats_of(v, lens, ppf))
    i = [B, P, Cc, mode] + ([xC] if multi else [])
    hf = with_stats(h, [T] * B)
    full = _norm_bwd(lib, hf, B, P, Cc, mode, xC if multi else 0, T, [T] * B)
    plain = _norm_bwd(lib, hf, B, P, Cc, mode, xC if multi else 0, T, None)
    only = lambda hh: {k: v for k, v in hh.items() if norm or k not in ("dgamma", "dbeta")}      # noqa: E731  (no norm: not touched)
    ref_full, _ = vref.norm_bwd(i, [], only(hf), [T] * B, T)
    assert np.array_equal(full["dx"].view(np.int32), plain["dx"].view(np.int32)), "dx: full lengths != lens == NULL"
    for k in ("dgamma", "dbeta", "dslope"):          # (sums of B partials added with atomics: see the module docstring)
        if k in full:
            _same_sum(full[k], plain[k], ref_full[k], k)
    hp = with_stats({k: (_pad_nan(v, ppf=ppf) if k in ("x", "dy", "dy1", "acc_in") else v) for k, v in h.items()}, LENS)
    got = _norm_bwd(lib, hp, B, P, Cc, mode, xC if multi else 0, T, LENS)
    (o64, amb), (o32, _) = (vref.norm_bwd(i, [], only(hp), LENS, T, dt) for dt in (np.float64, np.float32))
    assert amb <= max(1, int(tref.KINK_CAP * h["x"].size * 50)), f"{amb} elements on the PReLU kink: pick another seed"
    _judge(o64, o32, got, f"norm_bwd mode={mode} norm={norm} acc={acc} multi={multi} C={Cc} P={P}", sentinel=("dx",))


# ----------------------------------------------------------------------------------------------------------------------
# (a) the head: LayerNorm backward, LSTM backward (both kernels), filter-and-sum
# ----------------------------------------------------------------------------------------------------------------------
def test_masked_layernorm_backward(lib):
    rng = np.random.default_rng(31)
    F = 7
    rows = B * T * F
    x = (1.2 * rng.standard_normal((B, T, F, 64)) + 0.3).astype(np.float32)
    dy = rng.standard_normal((B, T, F, 64)).astype(np.float32)
    mr = np.stack([x.astype(np.float64).mean(-1), 1 / np.sqrt(x.astype(np.float64).var(-1) + EPS)], -1).astype(np.float32)
    g, dg0, db0 = (rng.standard_normal(64).astype(np.float32) for _ in range(3))

    def run(xx, dd, mm, lens):
        xd, dyd, mrd, gd = _d(xx), _d(dd), _d(mm), _d(g)
        dx = torch.full((rows, 64), SENTINEL, device="cuda:0")
        dg, db = _d(dg0), _d(db0)
        ld = _lens(lens)
        _ck(lib.eab_layernorm64_bwd_lens_f32(dyd.data_ptr(), xd.data_ptr(), mrd.data_ptr(), gd.data_ptr(), dx.data_ptr(), dg.data_ptr(),
                                             db.data_ptr(), rows, _ptr(ld), B if lens else 0, T if lens else 0, _st()))
        torch.cuda.synchronize()
        return {"dx": dx.cpu().numpy(), "dg": dg.cpu().numpy(), "db": db.cpu().numpy()}
    A = lambda xx, dd, mm: dict(dy=dd.reshape(rows, 64), x=xx.reshape(rows, 64), mr=mm.reshape(rows, 2), g=g, dg=dg0, db=db0)   # noqa: E731
    full, plain = run(x, dy, mr, [T] * B), run(x, dy, mr, None)
    ref_full = vref.ln_bwd(A(x, dy, mr), [T] * B, B, T)
    assert np.array_equal(full["dx"].view(np.int32), plain["dx"].view(np.int32))
    _same_sum(full["dg"], plain["dg"], ref_full["dg"], "dg")
    _same_sum(full["db"], plain["db"], ref_full["db"], "db")
    xp, dp, mp = _pad_nan(x), _pad_nan(dy), _pad_nan(mr)
    got = run(xp, dp, mp, LENS)
    o64, o32 = (vref.ln_bwd(A(xp, dp, mp), LENS, B, T, dt) for dt in (np.float64, np.float32))
    _judge(o64, o32, got, "layernorm_bwd")            # (dx is row-local: its padding rows are written, with whatever they held)


# F = 161: the 4-sequence kernel, whose workgroups straddle two utterances (161 % 4 = 1);  F = 690: 2070 sequences take the
# 16-sequence kernel (fp32 products)
@pytest.mark.parametrize("F,form", [(161, 0), (690, 1)])
def test_masked_lstm_backward(lib, F, form):
    rng = np.random.default_rng(41 + F)
    assert lib.eab_lstm64_bwd_form(B, T, F, prg.PREC_F32) == form
    S = B * F
    sig = lambda v: 1 / (1 + np.exp(-v))                                        # noqa: E731
    gates = rng.standard_normal((S, T, 5, 64))
    gates[:, :, [0, 1, 3]] = sig(gates[:, :, [0, 1, 3]])
    gates[:, :, 2] = np.tanh(gates[:, :, 2])
    gates = gates.astype(np.float32)
    dh = rng.standard_normal((B, T, F, 64)).astype(np.float32)
    wcat = (0.15 * rng.standard_normal((256, 128))).astype(np.float32)

    def run(gg, dd, lens):
        gd, dd_, wd = _d(gg), _d(dd), _d(wcat)
        out = torch.full((B, T, F, 256), SENTINEL, device="cuda:0")
        ld = _lens(lens)
        _ck(lib.eab_lstm64_bwd_lens_f32(gd.data_ptr(), dd_.data_ptr(), wd.data_ptr(), out.data_ptr(), _ptr(ld), B, T, F, prg.PREC_F32,
                                        _st()))
        torch.cuda.synchronize()
        return out.cpu().numpy()
    full, plain = run(gates, dh, [T] * B), run(gates, dh, None)
    assert np.array_equal(full.view(np.int32), plain.view(np.int32)), "full lengths != lens == NULL"
    gp = gates.reshape(B, F, T, 5, 64).copy()
    for b, n in enumerate(LENS):
        gp[b, :, n:] = np.nan
    gp = gp.reshape(S, T, 5, 64)
    dp = _pad_nan(dh)
    got = run(gp, dp, LENS)
    o64 = vref.lstm_bwd([B, T, F, prg.PREC_F32], dict(gates=gp, dh_out=dp, wcat=wcat), LENS)
    for b, n in enumerate(LENS):
        assert (got[b, n:] == 0).all(), "dgates of the padding steps are written as zeros"
    _judge(o64, None, {"dgates": got}, f"lstm_bwd F={F}")


def test_masked_filter_and_sum(lib):
    rng = np.random.default_rng(51)
    F, M, ld = 161, 4, 64
    w = rng.standard_normal((B, T, F, ld)).astype(np.float32)
    x = rng.standard_normal((B, T, F, M, 2)).astype(np.float32)

    def run(ww, xx, lens):
        wd, xd = _d(ww), _d(xx)
        y = torch.full((B, 2, T, F), SENTINEL, device="cuda:0")
        l_ = _lens(lens)
        _ck(lib.eab_filter_sum_ld_lens_f32(wd.data_ptr(), xd.data_ptr(), y.data_ptr(), B, T, F, M, ld, _ptr(l_), _st()))
        torch.cuda.synchronize()
        return y.cpu().numpy()
    assert np.array_equal(run(w, x, [T] * B).view(np.int32), run(w, x, None).view(np.int32))
    wp, xp = _pad_nan(w), _pad_nan(x)
    got = run(wp, xp, LENS)
    o64, o32 = (vref.filter_sum([B, T, F, M, ld], dict(w=wp, x=xp), LENS, dt) for dt in (np.float64, np.float32))
    for b, n in enumerate(LENS):
        assert np.array_equal(got[b, :, n:], np.zeros_like(got[b, :, n:])), "padding frames are exact zeros"
    _judge(o64, o32, {"y": got}, "filter_sum_ld")


# ----------------------------------------------------------------------------------------------------------------------
# (a) weight gradients
# ----------------------------------------------------------------------------------------------------------------------
def _wgrad_op(geom, N, C0, C1, precision):
    return tr.WgradOp(dz=None, src0=None, src1=True if C1 else None, dw=None, N=N, C0=C0, C1=C1, Kpad=geom.kpad(C0 + C1), B=B, T=T,
                      Fin=geom.Fin, Fz=geom.Fout, No=geom.No, ostride=geom.ostride, ophase=geom.ophase, istride=geom.istride,
                      dt=list(geom.dt), ioff=list(geom.ioff), dbias=True, precision=precision)


def _wgrad(lib, op, h, lens):
    from eabnet_amd import _lib
    d = _lib.WgradDesc()
    t = {k: (None if h.get(k) is None else _d(h[k])) for k in ("dz", "src0", "src1", "dw", "dbias")}
    d.dz, d.src0, d.src1, d.dw, d.dbias = (_ptr(t[k]) for k in ("dz", "src0", "src1", "dw", "dbias"))
    for f in ("N", "C0", "C1", "Kpad", "B", "T", "Fin", "Fz", "No", "ostride", "ophase", "istride", "precision"):
        setattr(d, f, getattr(op, f))
    d.ntaps = len(op.dt)
    for j in range(len(op.dt)):
        d.dt[j], d.ioff[j] = op.dt[j], op.ioff[j]
    ld = _lens(lens)
    _ck(lib.eab_wgrad_batch_lens_f32(C.byref(d), 1, C.sizeof(_lib.WgradDesc), _ptr(ld), _st()))
    torch.cuda.synchronize()
    return {"dw": t["dw"].cpu().numpy(), "dbias": t["dbias"].cpu().numpy()}


# pointwise on 161 bins: 3864 rows per utterance -- the one of 13 frames ends inside a 16-row stage (2093 = 130 * 16 + 13), the
# one of 5 frames leaves whole row groups in padding;  dt = -1: the recurrent product;  temporal taps: an S-TCM branch (72 rows);
# a strided 2-D unit;  one phase of a transposed unit on a concatenation of two sources
WG_CASES = [("pw161", prg.Geometry.pointwise(161), 64, 64, 0), ("hh161", prg.Geometry.pointwise(161, dt=-1), 256, 64, 0),
            ("tcm", prg.Geometry.temporal([-4, -2, 0]), 64, 256, 0), ("conv2d", prg.Geometry.strided(39, 2, 3), 128, 64, 0),
            ("deconv", prg.Geometry.transposed(19, 2, 3)[1], 64, 64, 64)]


@pytest.mark.parametrize("name,geom,N,C0,C1", WG_CASES, ids=[c[0] for c in WG_CASES])
@pytest.mark.parametrize("precision", [prg.PREC_F32, prg.PREC_BF16], ids=["f32", "bf16"])
def test_masked_weight_gradient(lib, name, geom, N, C0, C1, precision):
    rng = np.random.default_rng(60 + N + C0)
    op = _wgrad_op(geom, N, C0, C1, precision)
    f32 = lambda a: np.asarray(a, np.float32)                                   # noqa: E731
    h = dict(dz=f32(rng.standard_normal((B, T, geom.Fout, N))), src0=f32(rng.standard_normal((B, T, geom.Fin, C0))),
             dw=f32(rng.standard_normal((N, op.Kpad))), dbias=f32(rng.standard_normal(N)))
    if C1:
        h["src1"] = f32(rng.standard_normal((B, T, geom.Fin, C1)))
    ref_op = dataclasses.replace(op, precision=prg.PREC_F32)

    def rounded(hh):      # bf16 products: both operands rounded to bf16, fp32 accumulation; dbias from the unrounded dz
        if precision != prg.PREC_BF16:
            return hh
        r = lambda a: torch.from_numpy(np.nan_to_num(a)).bfloat16().float().numpy() + (a - a)       # noqa: E731 (keeps the NaN)
        return dict(hh, dz=r(hh["dz"]), src0=r(hh["src0"]), **({"src1": r(hh["src1"])} if C1 else {}))

    def refs(hh, lens):
        o64, o32 = (vref.wgrad(ref_op, rounded(hh), lens, dt) for dt in (np.float64, np.float32))
        if precision == prg.PREC_BF16:
            o64["dbias"], o32["dbias"] = (vref.wgrad(ref_op, hh, lens, dt)["dbias"] for dt in (np.float64, np.float32))
        return o64, o32
    full, plain = _wgrad(lib, op, h, [T] * B), _wgrad(lib, op, h, None)
    ref_full, _ = refs(h, [T] * B)
    for k in ("dw", "dbias"):                        # (split-K sums added with atomics: see the module docstring)
        _same_sum(full[k], plain[k], ref_full[k], f"{name} {k}")
    hp = {k: (_pad_nan(v) if k in ("dz", "src0", "src1") else v) for k, v in h.items()}
    got = _wgrad(lib, op, hp, LENS)
    o64, o32 = refs(hp, LENS)
    _judge(o64, o32, got, f"wgrad {name} {'bf16' if precision else 'f32'}")


# ----------------------------------------------------------------------------------------------------------------------
# (a) data gradients with look-ahead taps: the source-row limit of the convolutions
# ----------------------------------------------------------------------------------------------------------------------
class _V:
    def __init__(self, ref, F, Cc):
        self.ref, self.F, self.C = ref, F, Cc


def _dgrad_launches():
    out = []
    tcm = prg.Geometry.adjoint(prg.Geometry.temporal([-4, -2, 0]))[0]
    out.append(("tcm-gemm", tcm, 64, 64, 64, prg.KORDER_TAP))
    out.append(("tcm-st16", tcm, 64, 64, 16, prg.KORDER_FRAG))
    out.append(("tcm-st32", tcm, 64, 64, 32, prg.KORDER_FRAG))
    for k, g in enumerate(prg.Geometry.adjoint(prg.Geometry.strided(39, 2, 3))):     # the dgrad of a 2-D unit: one launch per parity
        out.append((f"conv2d-par{k}", g, 64, 64, 64, prg.KORDER_TAP))
    out.append(("deconv", prg.Geometry.adjoint(prg.Geometry.transposed(19, 2, 3))[0], 64, 64, 128, prg.KORDER_TAP))
    return out


@pytest.mark.parametrize("name,geom,Cz,N,bm,korder", _dgrad_launches(), ids=[c[0] for c in _dgrad_launches()])
@pytest.mark.parametrize("poison", ["nan", "finite"])
def test_dgrad_with_look_ahead_taps_never_reads_padding(lib, dev, name, geom, Cz, N, bm, korder, poison):
    """A stride-1 data-gradient launch whose taps look AHEAD (dt > 0, Geometry.adjoint of causal taps) on a dz whose padding
    rows hold NaN, or large finite values (the stale gradients of a longer utterance of the step before)."""
    from eabnet_amd import _lib
    assert max(geom.dt) > 0
    rng = np.random.default_rng(70 + Cz + bm)
    w3 = rng.standard_normal((N, Cz, max(geom.taps) + 1)).astype(np.float32)
    wimg = prg.pack_taps(w3, geom.taps)
    wflat = prg.pack_frag(wimg) if korder == prg.KORDER_FRAG else wimg.reshape(-1)
    nz, nd = B * T * geom.Fin * Cz, B * T * geom.Fout * N
    op = prg.conv_launch(name, B, T, [_V(prg.Ref("x", 0), geom.Fin, Cz)], prg.Ref("x", nz + nd), None, geom, N=N, epi=prg.EPI_LINEAR,
                         dst=prg.Ref("x", nz), bm=bm)
    op.korder = korder
    dz = rng.standard_normal((B, T, geom.Fin, Cz)).astype(np.float32)
    for b, n in enumerate(LENS):
        dz[b, n:] = np.nan if poison == "nan" else 1.0e3 * (1 + rng.random(dz[b, n:].shape))
    host = np.concatenate([dz.reshape(-1), np.full(nd, SENTINEL, np.float32), np.asarray(wflat, np.float32).reshape(-1)])
    arena = torch.from_numpy(host).to(dev)
    ld = _lens(LENS)
    enc = runtime.encode([op], {"x": arena.data_ptr()}, lens=ld.data_ptr())
    _ck(lib.eab_conv_f32(C.byref(enc[0].conv), _st()), name)
    torch.cuda.synchronize()
    got = arena[nz:nz + nd].view(B, T, geom.Fout, N).cpu().numpy()
    ref_arena = {"x": host.copy()}
    ref_arena["x"][nz:nz + nd] = np.nan
    yard = {}
    o64 = vref.conv(op, ref_arena, LENS, yard)
    _untouched(got, o64["dst"].may, f"{name} dst")
    assert np.isfinite(got[o64["dst"].must]).all(), f"{name}: a look-ahead tap read the padding"
    worst, l2 = tref.check({"dst": o64["dst"]}, {"dst": got}, yard, name)
    print(f"MASKED dgrad {name} ({poison}) | err/limit {worst:.3f} | L2 ratio {'-' if l2 is None else format(l2, '.2f')}")
    # full lengths: the launch of the same program without lengths, bit for bit
    dzf = rng.standard_normal((B, T, geom.Fin, Cz)).astype(np.float32)
    res = []
    for lens in ([T] * B, None):
        a2 = torch.from_numpy(np.concatenate([dzf.reshape(-1), np.full(nd, SENTINEL, np.float32), host[nz + nd:]])).to(dev)
        l2 = _lens(lens)
        e2 = runtime.encode([op], {"x": a2.data_ptr()}, lens=None if lens is None else l2.data_ptr())
        _ck(lib.eab_conv_f32(C.byref(e2[0].conv), _st()), name)
        torch.cuda.synchronize()
        res.append(a2[nz:nz + nd].cpu().numpy())
    assert np.array_equal(res[0].view(np.int32), res[1].view(np.int32)), f"{name}: full lengths != lens == NULL"


# ----------------------------------------------------------------------------------------------------------------------
# (b)-(f) the network
# ----------------------------------------------------------------------------------------------------------------------
NB, NT, NM = 3, 30, 4
NLENS = [30, 17, 9]
# parameter / input seeds per configuration: chosen on the CPU so that no pre-activation of the head's ReLU (EaBNet.py:594) lies
# within four times its own fp32 forward error of zero for any utterance ALONE at any of the lengths used here
# (_check_training_gradients' docstring, tests/test_hip_parity.py: an fp32 forward may otherwise flip that unit's derivative).
# Seeds (1300 + s, 1400 + s) were tried in order, s = 0, 1, ..: the default configuration (both length orders) fails s = 0 (one
# unit at 0.4 x its error), intra_connect="add" fails s = 0 and 1, the plain U-Net fails s = 0; these are the first that pass.
# The pointwise heads (cnn, miso) have no ReLU.
SEEDS = {"default": (1301, 1401), "add": (1302, 1402), "unet": (1301, 1401), "cnn": (1300, 1400), "miso": (1300, 1400)}
VARIANTS = {"default": {}, "cnn": dict(bf_type="cnn"), "miso": dict(topo_type="miso"), "add": dict(intra_connect="add"),
            "unet": dict(is_u2=False)}


def _setup(variant):
    from eabnet_amd.spec import NetConfig, param_specs
    kw = dict(p=2, q=2, **VARIANTS[variant])
    ps, xs = SEEDS[variant]
    P = torch_params(NM, ps, **kw)
    for k, sp in param_specs(NetConfig(M=NM, **kw)).items():
        if sp.kind == "prelu":
            P[k] = torch.ones_like(P[k])                                      # smooth network
    x = torch.from_numpy(paramgen.make_spec_input(NB, NT, 161, NM, xs))
    label = torch.from_numpy(paramgen.make_spec_input(NB, NT, 161, 1, xs + 1)[..., 0, :]).permute(0, 3, 1, 2).contiguous()
    return kw, P, x, label


@functools.lru_cache(maxsize=None)
def _reference(variant, lens):
    """fp64 autograd through the oracle, one utterance at a time on its own frames; outputs zero-padded, concatenated, ONE loss"""
    from oracle import eabnet_oracle as orc
    kw, P, x, label = _setup(variant)
    Pd = {k: v.double().requires_grad_(True) for k, v in P.items()}
    ys = []
    for b, n in enumerate(lens):
        y = orc.eabnet_forward(Pd, x[b:b + 1, :n].double(), **kw)             # (1, 2, n, F), or (1, 2, n) for miso
        ys.append(torch.nn.functional.pad(y, (0, 0, 0, NT - n) if y.ndim == 4 else (0, NT - n)))
    y = torch.cat(ys, 0)
    loss = _loss(orc.com_mag_mse_loss, y, label.double(), list(lens))
    loss.backward()
    return y.detach(), float(loss.detach()), {k: v.grad.double() for k, v in Pd.items()}


def _loss(com_mag_mse, y, label, lens):
    """com_mag_mse_loss over the valid frames; the miso head returns (B, 2, T) (summed over frequency, as the reference does),
    which that loss does not take: there the mean squared error over the valid frames against the label's frequency sum"""
    if y.ndim == 4:
        return com_mag_mse(y, label, lens)
    mask = (torch.arange(y.shape[2], device=y.device)[None, :] < torch.as_tensor(lens, device=y.device)[:, None]).to(y.dtype)
    return (((y - label.sum(-1)) ** 2) * mask[:, None]).sum() / (2.0 * float(sum(lens)))


def _net(dev, variant, precision="f32"):
    import eabnet_amd
    kw, P, x, label = _setup(variant)
    net = eabnet_amd.EaBNet(M=NM, **kw)
    net.load_state_dict(P, strict=True)
    net = net.to(dev).train()
    net.varlen_training = True
    net.precision = precision
    return net, x.to(dev), label.to(dev)


def _grad_errors(got, ref):
    num = sum(float(((got[k] - ref[k]) ** 2).sum()) for k in ref)
    den = sum(float((ref[k] ** 2).sum()) for k in ref)
    gmax = max(float(v.abs().max()) for v in ref.values())
    per = {k: float((got[k] - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref if float(ref[k].abs().max()) > 1e-6 * gmax}
    return (num / den) ** 0.5, per


def _step(net, x, label, lens, poison=False, g_poison=False):
    """one forward + backward; returns (y, loss, gradients).  poison: NaN into the padding rows of every gradient tap between the
    forward and the backward; g_poison: backward through y.backward(g) with NaN in g's padding."""
    import eabnet_amd
    for p in net.parameters():
        p.grad = None
    y = net(x, lengths=lens)
    assert y.requires_grad and net.training_backend == "hip"
    host_lens = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
    loss = _loss(eabnet_amd.com_mag_mse_loss, y, label, host_lens)
    if poison:
        _poison_taps(net, host_lens)
    if g_poison:
        (g,) = torch.autograd.grad(loss, y)
        for b, n in enumerate(host_lens):
            g[b, :, n:] = float("nan")
        y.backward(g)
    else:
        loss.backward()
    return y.detach(), float(loss.detach()), {k: p.grad.detach().cpu().double() for k, p in net.named_parameters()}


def _bound(net):
    return next(reversed(net._train_bound.values()))


def _poison_taps(net, lens):
    bound = _bound(net)
    prog = bound.prog
    half = set()                                       # tensors stored as bf16 (first half of their region)
    for op in list(prog.fwd) + list(prog.bwd):
        if isinstance(op, tr.GenOp):
            if op.kind == tr.OP_NORM_BWD and op.i[3] & tr.STORE_BF16:
                half.add(op.p[8])
            elif op.kind == tr.OP_TR_NORM_ACT and op.i[3] & tr.STORE_BF16:
                half.add(op.p[4])
            elif op.kind == tr.OP_GLU_BWD and len(op.i) > 3 and op.i[3] & tr.STORE_BF16:
                half.add(op.p[2])
    assert prog.grad_taps
    for name, (r, Fv, Cv) in prog.grad_taps.items():
        n = prog.B * prog.T * Fv * Cv
        reg = bound.acts[r.off:r.off + n]
        v = (reg.view(torch.bfloat16)[:n] if r in half else reg).view(prog.B, prog.T, Fv * Cv)
        for b, nb in enumerate(lens):
            v[b, nb:] = float("nan")


def _check_f32(y, loss, grads, ref, lens, what):
    ry, rloss, rg = ref
    for b, n in enumerate(lens):
        assert torch.equal(y[b, :, n:].cpu(), torch.zeros_like(y[b, :, n:]).cpu()), f"{what}: padding frames of y are exact zeros"
    assert torch.isfinite(y).all()
    assert_close(y.cpu().numpy(), ry.numpy(), 1e-5, f"{what}: forward vs per-utterance fp64")
    assert abs(loss - rloss) <= 1e-5 * abs(rloss), (loss, rloss)
    got = {k: grads[k] for k in rg}
    assert all(torch.isfinite(g).all() for g in got.values()), f"{what}: a gradient is not finite"
    total, per = _grad_errors(got, rg)
    bad = sorted(((e, k) for k, e in per.items() if e > 1e-4), reverse=True)
    print(f"VARLEN {what}: loss {loss:.6f} (fp64 {rloss:.6f}), gradients global l2-rel {total:.2e}, worst tensor {max(per.values()):.2e}")
    assert total <= 1e-4 and not bad, f"{what}: global l2-rel {total:.3e}; tensors over 1e-4: {bad[:8]}"


@pytest.mark.parametrize("lens", [(30, 17, 9), (9, 30, 17)])
def test_b_padded_batch_matches_one_utterance_at_a_time_fp64(dev, lens):
    net, x, label = _net(dev, "default")
    y, loss, grads = _step(net, x, label, list(lens))
    _check_f32(y, loss, grads, _reference("default", tuple(lens)), lens, f"lens {list(lens)}")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_c_stale_rows_and_poison_stay_out_of_the_gradients(dev, precision):
    """One bound program: a step at full length leaves valid gradients in every row; the next step, shorter, carries NaN in the
    padding of x, of grad_output and of every tapped gradient tensor."""
    net, x, label = _net(dev, "default", precision)
    _step(net, x, label, [NT] * NB)
    bound = _bound(net)
    xp = x.clone()
    for b, n in enumerate(NLENS):
        xp[b, n:] = float("nan")
    y, loss, grads = _step(net, xp, label, NLENS, poison=True, g_poison=True)
    assert _bound(net) is bound and len(net._train_bound) == 1, "one pair of graphs serves every combination of lengths"
    ref = _reference("default", tuple(NLENS))
    if precision == "f32":
        _check_f32(y, loss, grads, ref, NLENS, "poisoned step")
        return
    got = {k: grads[k] for k in ref[2]}
    assert torch.isfinite(y).all() and all(torch.isfinite(g).all() for g in got.values()), "NaN reached an output or a gradient"
    for b, n in enumerate(NLENS):
        assert torch.equal(y[b, :, n:].cpu(), torch.zeros_like(y[b, :, n:]).cpu())
    total, _ = _grad_errors(got, ref[2])
    gmax = max(float(v.abs().max()) for v in ref[2].values())
    cos = {k: float(torch.nn.functional.cosine_similarity(got[k].reshape(-1), ref[2][k].reshape(-1), dim=0))
           for k in ref[2] if float(ref[2][k].abs().max()) > 1e-3 * gmax}
    print(f"VARLEN bf16 poisoned step: global l2-rel {total:.2e}, min cosine {min(cos.values()):.4f}")
    assert total <= 1e-1 and min(cos.values()) >= 0.99


@pytest.mark.parametrize("variant", ["cnn", "miso", "add", "unet"])
def test_d_every_head_topology_and_skip_form(dev, variant):
    net, x, label = _net(dev, variant)
    y, loss, grads = _step(net, x, label, NLENS)
    _check_f32(y, loss, grads, _reference(variant, tuple(NLENS)), NLENS, variant)


def test_e_independence_device_lengths_and_direct_launches(dev):
    net, x, label = _net(dev, "default")
    y, loss, grads = _step(net, x, label, NLENS)
    # utterance 1 alone, B = 1, T = 17: the tile set follows (B, T), so the bar is the InstanceNorm one of the inference form
    y1 = net(x[1:2, :17].contiguous(), lengths=[17]).detach()
    assert_close(y[1:2, :, :17].cpu().numpy(), y1.cpu().numpy(), 1e-5, "utterance 1 in the batch vs alone")
    # device lengths: the same program, the same bits of the output (the gradients are sums added with atomics: two runs of
    # the SAME call differ in the last bits, so they get the bar the flat / DDP tests use for that)
    net2, _, _ = _net(dev, "default")
    yd, lossd, gd = _step(net2, x, label, torch.tensor(NLENS, device=dev))
    assert torch.equal(yd, y) and lossd == loss
    gmax = max(float(v.abs().max()) for v in grads.values())
    for k in grads:                                    # (tensors at the noise floor -- biases in front of an InstanceNorm -- aside)
        top = float(grads[k].abs().max())
        if top > 1e-6 * gmax:
            assert float((gd[k] - grads[k]).abs().max()) <= 1e-5 * top, k
    # the same module without lengths: another bound program (the cache key carries varlen), both stay resident
    net(x).sum().backward()
    keys = list(net._train_bound)
    assert sorted(k[-1] for k in keys if k[1] == NT) == [False, True] and all(len(k) == 6 for k in keys), keys
    assert [b.prog.varlen for k, b in net._train_bound.items() if k[1] == NT and k[-1]] == [True]
    net3, _, _ = _net(dev, "default")
    net3.use_graph = False
    yn, lossn, gn = _step(net3, x, label, NLENS)
    assert_close(yn.cpu().numpy(), y.cpu().numpy(), 1e-5, "direct launches vs the captured graphs")
    assert abs(lossn - loss) <= 1e-5 * abs(loss)
    for k in grads:
        top = float(grads[k].abs().max())
        if top > 1e-6 * gmax:
            assert float((gn[k] - grads[k]).abs().max()) <= 1e-5 * top, k


def test_f_a_whole_training_step_on_a_mixed_length_batch(dev):
    """net(x, lengths=frames) -> istft(lengths=frames) -> si_sdr_loss(lengths=samples) + com_mag_mse_loss, backward, FlatAdam:
    the loss falls over five steps on one batch"""
    import eabnet_amd
    hop, n_fft = 160, 320
    Bq, Tq, M = 3, 20, 2
    frames = [20, 13, 8]
    samples = [hop * (n - 1) for n in frames]
    window = torch.hann_window(n_fft)
    net = eabnet_amd.EaBNet(M=M, p=1, q=1)
    net.load_state_dict(torch_params(M, 1510, p=1, q=1), strict=True)
    net = net.to(dev).train()
    net.varlen_training = True
    x = torch.from_numpy(paramgen.make_spec_input(Bq, Tq, 161, M, 1511)).to(dev)
    target = torch.from_numpy(paramgen.make_wave(Bq, 1, hop * (Tq - 1), 1512)).to(dev)
    for b, n in enumerate(frames):
        x[b, n:] = float("nan")                            # what lies behind an utterance does not matter
    label = eabnet_amd.stft_compress(target, n_fft, hop, window, 1)
    opt = eabnet_amd.FlatAdam(net.parameters(), lr=1e-3)
    dl = torch.tensor(frames, device=dev)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        y = net(x, lengths=dl)
        wav = eabnet_amd.istft(y, n_fft, hop, window, lengths=frames)
        loss = eabnet_amd.com_mag_mse_loss(y, label, frames) + 0.05 * eabnet_amd.si_sdr_loss(wav, target[:, 0], lengths=samples, eps=1e-8)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("VARLEN whole step, loss per step:", [f"{v:.5f}" for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
