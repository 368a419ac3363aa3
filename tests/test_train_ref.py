"""The float64 references of the training ops (tests/train_ref.py) pinned on the CPU: no GPU, no library.

  * per op kind against torch float64 autograd of the reference layer the op differentiates (random PReLU slopes in
    (0.05, 0.45), never 1; accumulate operands and previous gradient values non-zero).  float64 against float64: REL = 1e-10.
    On the same inputs (rounded to fp32) the float32 yardstick evaluation of the reference must stay inside the derived
    limit -- a limit its own fp32 evaluation breaks is wrong;
  * the dry walk of every case the device walk runs (tests/test_train_walk_gpu.py), using only the read / write table:
    regions inside their arenas, overlaps only as declared aliases, nothing read before it is written;
  * the same cases interpreted on the CPU: every op's yardstick evaluation, on the activations and gradients the program
    really produces, stays inside the limits, and the share of PReLU-kink elements is below its cap.
"""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as cr
import train_ref as tref
from eabnet_amd import program as prg
from eabnet_amd import train as tr

REL = 1e-10
f64 = torch.float64


def _r32(g, *shape, scale=1.0, shift=0.0):
    """fp32-representable float64 tensor"""
    return (torch.randn(*shape, generator=g, dtype=torch.float32) * scale + shift).double()


def _slopes(g, n):
    return (torch.rand(n, generator=g, dtype=torch.float32) * 0.4 + 0.05).double()


def _np(t):
    return t.detach().numpy() if isinstance(t, torch.Tensor) else t


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), _np(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    assert err <= REL, f"{what}: float64 reference deviates from autograd by {err:.3e} (relative to max)"


def _both(form, i, f, A, what=""):
    """float64 result on A; and, on A rounded to fp32, the yardstick inside the limit"""
    A = {k: _np(v) for k, v in A.items()}
    res, amb = tref.run_ref(form, i, f, A)
    A32 = {k: (v if v is True or v is None else np.asarray(v, np.float32)) for k, v in A.items()}
    r64, _ = tref.run_ref(form, i, f, A32)
    r32, _ = tref.run_ref(form, i, f, A32, np.float32)
    for name, r in r64.items():
        val, lim = np.asarray(r[0], np.float64), np.asarray(r[1], np.float64)
        must = np.ones(val.shape, bool) if len(r) < 3 else r[2]
        y = np.asarray(r32[name][0], np.float64)
        ok = must & np.isfinite(lim)
        if len(r32[name]) > 2:
            ok &= r32[name][2]
        assert not np.isnan(lim).any() and (lim >= 0).all(), f"{what} {form} {name}: bad limit"
        bad = ok & (np.abs(y - val) > lim)
        assert not bad.any(), (f"{what} {form} {name}: the fp32 evaluation of the reference breaks its own limit at {int(bad.sum())} "
                               f"elements, worst ratio {float((np.abs(y - val)[bad] / np.maximum(lim[bad], 1e-300)).max()):.2f}")
    return res, amb


# ----------------------------------------------------------------------------------------------------------------------
# per kind against autograd
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [prg.XF_NORM_PRELU, prg.XF_PRELU_NORM])
def test_instance_norm_units_match_autograd(mode):
    g = torch.Generator().manual_seed(3 + mode)
    B, P, C = 2, 37, 8
    x = _r32(g, B, P, C, scale=1.3, shift=0.4).requires_grad_(True)
    gam, bet, slp = (_r32(g, C, scale=0.3, shift=1.0).requires_grad_(True), _r32(g, C, scale=0.3).requires_grad_(True),
                     _slopes(g, C).requires_grad_(True))
    add, acc, dy = _r32(g, B, P, C), _r32(g, B, P, C), _r32(g, B, P, C)
    prev = {k: _r32(g, C) for k in ("dgamma", "dbeta", "dslope")}
    xc = x.permute(0, 2, 1)
    if mode == prg.XF_NORM_PRELU:
        y = F.prelu(F.instance_norm(xc, weight=gam, bias=bet, eps=1e-5), slp)
        stat_of = xc
    else:
        y = F.instance_norm(F.prelu(xc, slp), weight=gam, bias=bet, eps=1e-5)
        stat_of = F.prelu(xc, slp)
    y = y.permute(0, 2, 1)
    (y * dy).sum().backward()
    mean = stat_of.mean(2)
    rstd = 1 / torch.sqrt(stat_of.var(2, unbiased=False) + 1e-5)
    A = {"x": x, "gamma": gam, "beta": bet, "xf": True, "mr": True}
    if mode == prg.XF_PRELU_NORM:
        A.update(slope=slp, y=True)
    st, _ = _both("IN_STATS", [B, P, C], [1e-5], A)
    _close(st["mr"][0][..., 0], mean, "mean")
    _close(st["mr"][0][..., 1], rstd, "rstd")
    if mode == prg.XF_PRELU_NORM:
        _close(st["y"][0], y, "y of the one-launch unit")
    na, _ = _both("TR_NORM_ACT", [B, P, C, mode], [], {"x": x, "xf": st["xf"][0], "slope": slp, "add": add, "y": True})
    _close(na["y"][0], y.detach() + add, "norm_act + add")
    for acc_in in (None, acc):
        A = {"dy": dy, "x": x, "mr": st["mr"][0], "gamma": gam, "beta": bet, "slope": slp, "sums": True, "dx": True, **prev}
        if acc_in is not None:
            A["acc_in"] = acc_in
        r, _ = _both("NORM_BWD", [B, P, C, mode | tr.NB_SUMS_ZEROED], [], A)
        _close(r["dx"][0], x.grad + (0 if acc_in is None else acc_in), "dx")
        _close(r["dgamma"][0], gam.grad + prev["dgamma"], "dgamma")
        _close(r["dbeta"][0], bet.grad + prev["dbeta"], "dbeta")
        _close(r["dslope"][0], slp.grad + prev["dslope"], "dslope")


def test_prelu_without_a_norm_matches_autograd():
    """xf == NULL / mr == NULL: y = prelu(x) [+ add], dx = dy prelu'(x) (+ acc_in), only dslope accumulates"""
    g = torch.Generator().manual_seed(5)
    B, P, C = 2, 19, 8
    x, slp = _r32(g, B, P, C).requires_grad_(True), _slopes(g, C).requires_grad_(True)
    dy, acc, prev = _r32(g, B, P, C), _r32(g, B, P, C), _r32(g, C)
    y = F.prelu(x.permute(0, 2, 1), slp).permute(0, 2, 1)
    (y * dy).sum().backward()
    na, _ = _both("TR_NORM_ACT", [B, P, C, prg.XF_NORM_PRELU], [], {"x": x, "slope": slp, "y": True})
    _close(na["y"][0], y, "prelu")
    r, amb = _both("NORM_BWD", [B, P, C, prg.XF_NORM_PRELU], [], {"dy": dy, "x": x, "slope": slp, "sums": True, "acc_in": acc, "dx": True,
                                                                   "dslope": prev})
    assert amb == 0 and set(r) == {"dx", "dslope"}
    _close(r["dx"][0], x.grad + acc, "dx")
    _close(r["dslope"][0], slp.grad + prev, "dslope")


def test_two_views_on_one_input_match_autograd():
    """the branch norms of an S-TCM: IN_STATS with xC > 0 (each view its own contiguous tensor) and the multi-view backward"""
    g = torch.Generator().manual_seed(7)
    B, P, xC = 2, 23, 8
    C = 2 * xC
    x = _r32(g, B, P, xC, scale=1.2, shift=-0.2).requires_grad_(True)
    gam, bet, slp = (_r32(g, C, scale=0.3, shift=1.0).requires_grad_(True), _r32(g, C, scale=0.3).requires_grad_(True),
                     _slopes(g, C).requires_grad_(True))
    dys, acc = [_r32(g, B, P, xC), _r32(g, B, P, xC)], _r32(g, B, P, xC)
    prev = {k: _r32(g, C) for k in ("dgamma", "dbeta", "dslope")}
    xc = x.permute(0, 2, 1)
    ys = [F.instance_norm(F.prelu(xc, slp[v * xC:(v + 1) * xC]), weight=gam[v * xC:(v + 1) * xC], bias=bet[v * xC:(v + 1) * xC],
                          eps=1e-5).permute(0, 2, 1) for v in range(2)]
    sum((y * d).sum() for y, d in zip(ys, dys)).backward()
    st, _ = _both("IN_STATS_MULTI", [B, P, C, xC], [1e-5], {"x": x, "slope": slp, "gamma": gam, "beta": bet, "xf": True, "mr": True, "y": True})
    assert st["y"][0].shape == (2, B, P, xC)
    for v in range(2):
        _close(st["y"][0][v], ys[v], f"view {v}")
    r, _ = _both("NORM_BWD_MULTI", [B, P, C, prg.XF_PRELU_NORM | tr.NB_SUMS_ZEROED, xC], [],
                 {"dy": dys[0], "dy1": dys[1], "x": x, "mr": st["mr"][0], "gamma": gam, "slope": slp, "sums": True, "acc_in": acc, "dx": True,
                  **prev})
    _close(r["dx"][0], x.grad + acc, "dx = acc_in + both input gradients")
    _close(r["dgamma"][0], gam.grad + prev["dgamma"], "dgamma")
    _close(r["dbeta"][0], bet.grad + prev["dbeta"], "dbeta")
    _close(r["dslope"][0], slp.grad + prev["dslope"], "dslope")


def test_finalize_of_welford_partials_matches_the_statistics():
    g = torch.Generator().manual_seed(9)
    B, C, cuts = 2, 8, [0, 5, 12, 13, 30]
    xs = [_r32(g, B, cuts[-1], C, scale=1.1, shift=0.7), _r32(g, B, cuts[-1], C, scale=0.6, shift=-1.5)]
    gam, bet = _r32(g, 2, C, scale=0.3, shift=1.0), _r32(g, 2, C, scale=0.3)
    tiles = len(cuts) - 1
    st = np.zeros((B, tiles, 2, C, 4))
    for s, x in enumerate(xs):
        for t in range(tiles):
            blk = x[:, cuts[t]:cuts[t + 1]]
            st[:, t, s, :, 0], st[:, t, s, :, 1] = blk.shape[1], blk.mean(1).numpy()
            st[:, t, s, :, 2] = ((blk - blk.mean(1, keepdim=True)) ** 2).sum(1).numpy()
    A = {"stats": st, "gamma0": gam[0], "beta0": bet[0], "gamma1": gam[1], "beta1": bet[1], "xf0": True, "xf1": True, "mr0": True, "mr1": True}
    r, _ = _both("IN_FINALIZE", [B, C, 2, tiles, cuts[-1]], [1e-5], A)
    for s, x in enumerate(xs):
        mean, rstd = x.mean(1), 1 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)
        _close(r[f"mr{s}"][0][..., 0], mean, "mean")
        _close(r[f"mr{s}"][0][..., 1], rstd, "rstd")
        _close(r[f"xf{s}"][0][..., 0], gam[s] * rstd, "scale")
        _close(r[f"xf{s}"][0][..., 1], bet[s] - mean * gam[s] * rstd, "shift")


def test_elementwise_and_reduction_ops_match_autograd():
    g = torch.Generator().manual_seed(11)
    rows, N = 53, 128
    a, gt = _r32(g, rows, 64).requires_grad_(True), _r32(g, rows, 64).requires_grad_(True)
    dy = _r32(g, rows, 64)
    y = F.glu(torch.cat([a, gt], 1), 1)
    (y * dy).sum().backward()
    r = np.arange(N)
    half, ch = (r % 64) // 32, (r // 64) * 32 + r % 32                       # packed column r: (value | gate), channel
    dump = torch.where(torch.from_numpy(half == 0), a.detach()[:, ch], torch.sigmoid(gt.detach())[:, ch])
    res, _ = _both("GLU_BWD", [rows, 0, N], [], {"dy": dy, "dump": dump, "dz": True})
    _close(res["dz"][0], torch.where(torch.from_numpy(half == 0), a.grad[:, ch], gt.grad[:, ch]), "glu_bwd")
    n = rows * 64
    flat = lambda t: t.detach().reshape(-1)                                  # noqa: E731
    res, _ = _both("GATE_FWD", [n, 0], [], {"a": flat(a), "r": flat(gt), "z": True})
    _close(res["z"][0], flat(y), "gate_fwd")
    res, _ = _both("GATE_BWD", [n, 0], [], {"dz": flat(dy), "a": flat(a), "r": flat(gt), "da": True, "dr": True})
    _close(res["da"][0], flat(a.grad), "gate da")
    _close(res["dr"][0], flat(gt.grad), "gate dr")
    res, _ = _both("ADD", [n, 0], [], {"a": flat(a), "b": flat(gt), "out": True})
    _close(res["out"][0], flat(a) + flat(gt), "add")
    yv = torch.relu(a.detach())
    res, _ = _both("RELU_BWD", [n, 0], [], {"dy": flat(dy), "y": flat(yv), "dx": True})
    _close(res["dx"][0], flat(dy * (yv > 0)), "relu_bwd")
    prev = _r32(g, 64)
    res, _ = _both("COLSUM", [rows, 0, 64], [], {"x": a.detach(), "out": prev})
    _close(res["out"][0], prev + a.detach().sum(0), "colsum")
    # filter-and-sum with rows padded to ld, and its backward
    B, T, Fq, M, ld = 2, 3, 7, 3, 16
    w, x = _r32(g, B, T, Fq, M, 2).requires_grad_(True), _r32(g, B, T, Fq, M, 2)
    yy = torch.stack(((w[..., 0] * x[..., 0] - w[..., 1] * x[..., 1]).sum(-1), (w[..., 0] * x[..., 1] + w[..., 1] * x[..., 0]).sum(-1)), 1)
    dout = _r32(g, *yy.shape)
    (yy * dout).sum().backward()
    wp = torch.full((B, T, Fq, ld), 7.0, dtype=f64)                          # (padding columns are never read)
    wp[..., :2 * M] = w.detach().reshape(B, T, Fq, 2 * M)
    res, _ = _both("FILTER_SUM", [B, T, Fq, M, ld], [], {"w": wp, "x": x, "y": True})
    _close(res["y"][0], yy, "filter_sum")
    res, _ = _both("FS_BWD", [B, T, Fq, M, ld], [], {"dout": dout, "x": x, "dw": True})
    _close(res["dw"][0][..., :2 * M], w.grad.reshape(B, T, Fq, 2 * M), "filter_sum_bwd")
    assert not res["dw"][0][..., 2 * M:].any()
    # LayerNorm(64)
    rows = 41
    xl, gl, bl = (_r32(g, rows, 64, shift=0.3).requires_grad_(True), _r32(g, 64, scale=0.3, shift=1.0).requires_grad_(True),
                  _r32(g, 64).requires_grad_(True))
    dyl, pg, pb = _r32(g, rows, 64), _r32(g, 64), _r32(g, 64)
    yl = F.layer_norm(xl, (64,), gl, bl, 1e-5)
    (yl * dyl).sum().backward()
    fw, _ = _both("LN_FWD", [rows, 0], [1e-5], {"x": xl, "g": gl, "b": bl, "y": True, "mr": True})
    _close(fw["y"][0], yl, "layernorm")
    res, _ = _both("LN_BWD", [rows, 0], [], {"dy": dyl, "x": xl, "mr": fw["mr"][0], "g": gl, "dx": True, "dg": pg, "db": pb})
    _close(res["dx"][0], xl.grad, "layernorm dx")
    _close(res["dg"][0], gl.grad + pg, "layernorm dgamma")
    _close(res["db"][0], bl.grad + pb, "layernorm dbeta")


def _wgrad_op(N, C0, C1, B, T, Fin, Fz, No, ostride, ophase, istride, dt, ioff, dbias=True):
    upt = (C0 + C1 + 15) // 16
    return tr.WgradOp(dz=prg.Ref("a", 0), src0=prg.Ref("a", 0), src1=prg.Ref("a", 0) if C1 else None, dw=prg.Ref("g", 0), N=N, C0=C0, C1=C1,
                      Kpad=len(dt) * upt * 16, B=B, T=T, Fin=Fin, Fz=Fz, No=No, ostride=ostride, ophase=ophase, istride=istride, dt=list(dt),
                      ioff=list(ioff), dbias=prg.Ref("g", 0) if dbias else None)


def _wgrad_both(op, A):
    A = {k: _np(v) for k, v in A.items()}
    res, _ = tref.ref_wgrad(op, A, tref._M(np.float64))
    A32 = {k: np.asarray(v, np.float32) for k, v in A.items()}
    r64, _ = tref.ref_wgrad(op, A32, tref._M(np.float64))
    r32, _ = tref.ref_wgrad(op, A32, tref._M(np.float32))
    for k in r64:
        assert (np.abs(np.asarray(r32[k][0], np.float64) - r64[k][0]) <= r64[k][1]).all(), f"wgrad {k}: fp32 evaluation beyond its limit"
    return res


def test_weight_gradients_match_autograd():
    g = torch.Generator().manual_seed(13)
    # strided causal Conv2d (2, 3), stride (1, 2): GateConv2d / Conv2dunit
    N, C0, kt, kf, B, T, Fin = 8, 12, 2, 3, 2, 5, 11
    Fout = (Fin - kf) // 2 + 1
    x, w = _r32(g, B, C0, T, Fin), _r32(g, N, C0, kt, kf).requires_grad_(True)
    bias = _r32(g, N).requires_grad_(True)
    y = F.conv2d(F.pad(x, (0, 0, kt - 1, 0)), w, bias, stride=(1, 2))
    dz = _r32(g, *y.shape)
    (y * dz).sum().backward()
    taps = [(a, c) for a in range(kt) for c in range(kf)]
    op = _wgrad_op(N, C0, 0, B, T, Fin, Fout, Fout, 1, 0, 2, [a - (kt - 1) for a, _ in taps], [c for _, c in taps])
    pw, pb = _r32(g, N, op.Kpad), _r32(g, N)
    res = _wgrad_both(op, {"dz": dz.permute(0, 2, 3, 1), "src0": x.permute(0, 2, 3, 1), "dw": pw, "dbias": pb})
    got = (res["dw"][0] - pw.numpy()).reshape(N, len(taps), 16)
    _close(got[:, :, :C0], w.grad.reshape(N, C0, kt * kf).permute(0, 2, 1), "dW of a strided convolution")
    assert not got[:, :, C0:].any(), "padding columns receive nothing"
    _close(res["dbias"][0], bias.grad + pb, "dbias")
    # ConvTranspose2d (2, 3), stride (1, 2), chomped, on a concatenation: one launch per output-column parity
    N, C0, C1, kt, kf, B, T, Fin = 8, 16, 16, 2, 3, 2, 4, 5
    Fout = (Fin - 1) * 2 + kf
    xa, xb = _r32(g, B, C0, T, Fin), _r32(g, B, C1, T, Fin)
    w = _r32(g, C0 + C1, N, kt, kf).requires_grad_(True)
    y = F.conv_transpose2d(torch.cat((xa, xb), 1), w, stride=(1, 2))[:, :, :T]
    dz = _r32(g, *y.shape)
    (y * dz).sum().backward()
    for ph in (0, 1):
        tp = [(a, c) for a in range(kt) for c in range(ph, kf, 2)]
        No = (Fout + 1) // 2 if ph == 0 else Fout // 2
        op = _wgrad_op(N, C0, C1, B, T, Fin, Fout, No, 2, ph, 1, [-a for a, _ in tp], [-(c - ph) // 2 for _, c in tp], dbias=False)
        res = _wgrad_both(op, {"dz": dz.permute(0, 2, 3, 1), "src0": xa.permute(0, 2, 3, 1), "src1": xb.permute(0, 2, 3, 1),
                               "dw": torch.zeros(N, op.Kpad, dtype=f64)})
        _close(res["dw"][0].reshape(N, len(tp), C0 + C1), torch.stack([w.grad[:, :, a, c].T for a, c in tp], 1), f"dW, phase {ph}")


def test_lstm_recurrences_match_autograd():
    g = torch.Generator().manual_seed(17)
    B, T, Fq = 2, 5, 3
    S = B * Fq
    lstm = torch.nn.LSTM(64, 64, batch_first=True).double()
    x = _r32(g, S, T, 64).requires_grad_(True)
    h, _ = lstm(x)
    dh = _r32(g, S, T, 64)
    (h * dh).sum().backward()
    wcat = torch.cat((lstm.weight_ih_l0, lstm.weight_hh_l0), 1).detach()
    bias = (lstm.bias_ih_l0 + lstm.bias_hh_l0).detach()
    btf = lambda t: t.detach().view(B, Fq, T, -1).permute(0, 2, 1, 3)       # noqa: E731  (B*F, T, C) -> (B, T, F, C)
    fw, _ = tref.run_ref("LSTM_TRAIN", [B, T, Fq, 0], [], {"x": _np(btf(x)), "wcat": _np(wcat), "bias": _np(bias), "h_out": True, "gates": True})
    _close(fw["h_out"][0], btf(h), "h")
    bw, _ = tref.run_ref("LSTM_BWD", [B, T, Fq, 0], [], {"gates": fw["gates"][0], "dh_out": _np(btf(dh)), "wcat": _np(wcat), "dgates": True})
    dg = torch.from_numpy(bw["dgates"][0]).permute(0, 2, 1, 3).reshape(S, T, 256)
    hprev = torch.cat((torch.zeros(S, 1, 64, dtype=f64), h.detach()[:, :-1]), 1)
    _close(torch.einsum("stk,stc->kc", dg, x.detach()), lstm.weight_ih_l0.grad, "dW_ih")
    _close(torch.einsum("stk,stc->kc", dg, hprev), lstm.weight_hh_l0.grad, "dW_hh")
    _close(dg.sum((0, 1)), lstm.bias_ih_l0.grad, "db")
    _close(dg @ lstm.weight_ih_l0.detach(), x.grad, "dx")
    # the two weight gradients as the program takes them: taps dt = 0 (input) and dt = -1 (previous hidden state)
    for src, dt, want in ((btf(x), 0, lstm.weight_ih_l0.grad), (btf(h), -1, lstm.weight_hh_l0.grad)):
        op = _wgrad_op(256, 64, 0, B, T, Fq, Fq, Fq, 1, 0, 1, [dt], [0], dbias=False)
        res = _wgrad_both(op, {"dz": bw["dgates"][0], "src0": src, "dw": torch.zeros(256, 64, dtype=f64)})
        _close(res["dw"][0], want, f"wgrad with dt = {dt}")


def _cln(x, gain, bias):
    """CumulativeLayerNorm2d as tests/operator_path.py::_norm writes it; x (B, C, T, F)"""
    per_frame = x.shape[1] * x.shape[3]
    cs, cq = torch.cumsum(x.sum((1, 3)), dim=1), torch.cumsum(x.pow(2).sum((1, 3)), dim=1)
    cnt = per_frame * torch.arange(1, x.shape[2] + 1, dtype=x.dtype).view(1, -1)
    mean = cs / cnt
    std = ((cq - 2 * mean * cs) / cnt + mean.pow(2) + 1e-5).sqrt()
    return (x - mean.view(x.shape[0], 1, -1, 1)) / std.view(x.shape[0], 1, -1, 1) * gain.view(1, -1, 1, 1) + bias.view(1, -1, 1, 1)


@pytest.mark.parametrize("mode", [prg.XF_NORM_PRELU, prg.XF_PRELU_NORM])
def test_cumulative_layer_norm_unit_matches_autograd(mode):
    g = torch.Generator().manual_seed(19 + mode)
    B, C, T, Fq = 2, 8, 5, 3
    P = Fq * C
    x = _r32(g, B, C, T, Fq, scale=1.2, shift=0.3).requires_grad_(True)
    gain, bias, slp = (_r32(g, C, scale=0.3, shift=1.0).requires_grad_(True), _r32(g, C, scale=0.3).requires_grad_(True),
                       _slopes(g, C).requires_grad_(True))
    ours = lambda t: t.detach().permute(0, 2, 3, 1).reshape(B, T, P)        # noqa: E731  channel = index % C
    add, acc, dy = _r32(g, B, C, T, Fq), _r32(g, B, C, T, Fq), _r32(g, B, C, T, Fq)
    y = F.prelu(_cln(x, gain, bias), slp) if mode == prg.XF_NORM_PRELU else _cln(F.prelu(x, slp), gain, bias)
    (y * dy).sum().backward()
    A = {"x": ours(x), "sums": True, "mr": True}
    if mode == prg.XF_PRELU_NORM:
        A["slope"] = slp
    st, _ = _both("CLN_STATS", [B, T, P, C], [1e-5], A)
    ap, _ = _both("CLN_APPLY", [B, T, P, C, mode], [], {"x": ours(x), "mr": st["mr"][0], "gain": gain, "bias": bias, "slope": slp,
                                                        "add": ours(add), "y": True})
    _close(ap["y"][0], ours(y + add), "cLN unit + add")
    r, _ = _both("CLN_BWD", [B, T, P, C, mode], [], {"dy": ours(dy), "x": ours(x), "mr": st["mr"][0], "gain": gain, "bias": bias, "slope": slp,
                                                     "rowsums": True, "ab": True, "part": True, "acc_in": ours(acc), "dx": True})
    _close(r["dx"][0], ours(x.grad + acc), "dx")
    part = r["part"][0].sum(0)                                              # what the COLSUM behind it adds up
    _close(part[0], gain.grad, "dgain")
    _close(part[1], bias.grad, "dbias")
    _close(part[2], slp.grad, "dslope")


@pytest.mark.parametrize("act", [prg.ACT_SIGMOID, prg.ACT_TANH, prg.ACT_RELU])
def test_gagnet_tail_matches_autograd(act):
    g = torch.Generator().manual_seed(23 + act)
    B, T, Fq, ld, lin = 2, 3, 5, 12, 8
    inpt, pre_x = _r32(g, B, 2, T, Fq), _r32(g, B, 2, T, Fq)
    pk, _ = _both("GAG_PACK", [B, T, Fq, ld], [], {"inpt": inpt, "pre_x": pre_x, "enc_in": True, "pre": True})
    assert np.array_equal(pk["enc_in"][0], torch.cat((inpt, pre_x), 1).permute(0, 2, 3, 1).numpy())
    pre = torch.from_numpy(pk["pre"][0][:, :, :2 * Fq]).reshape(B, T, Fq, 2).clone().requires_grad_(True)
    assert np.array_equal(pre.detach().numpy(), pre_x.permute(0, 2, 3, 1).numpy()) and not pk["pre"][0][:, :, 2 * Fq:].any()
    gv, rv, iv = (_r32(g, B, T, Fq).requires_grad_(True) for _ in range(3))
    gain = {prg.ACT_SIGMOID: torch.sigmoid, prg.ACT_TANH: torch.tanh, prg.ACT_RELU: torch.relu}[act](gv)
    y = pre * gain[..., None] + torch.stack((rv, iv), -1)
    dpl, dnx, acc = _r32(g, B, 2, T, Fq), _r32(g, B, T, ld), _r32(g, B, T, ld)
    (y.permute(0, 3, 1, 2) * dpl).sum().backward(retain_graph=True)
    (y.reshape(B, T, 2 * Fq) * dnx[:, :, :2 * Fq]).sum().backward()
    pad = lambda t, n: F.pad(t.detach(), (0, n - t.shape[-1]), value=3.0)    # noqa: E731  (padding columns are never read)
    Af = {"pre": pad(pre.reshape(B, T, 2 * Fq), ld), "g": pad(gv, lin), "r": pad(rv, lin), "i": pad(iv, lin)}
    fw, _ = _both("GAG_CRM", [B, T, Fq, ld, lin, act], [], {**Af, "pre_out": True, "planar": True})
    _close(fw["planar"][0], y.permute(0, 3, 1, 2), "stage output")
    _close(fw["pre_out"][0][:, :, :2 * Fq], y.reshape(B, T, 2 * Fq), "next pre")
    assert not fw["pre_out"][0][:, :, 2 * Fq:].any()
    bw, _ = _both("GAG_CRM_BWD", [B, T, Fq, ld, lin, act], [], {"pre": Af["pre"], "g": Af["g"], "dplanar": dpl, "dpre_out": dnx, "acc_in": acc,
                                                                "dg": True, "dr": True, "di": True, "dpre": True})
    for name, want in (("dg", gv.grad), ("dr", rv.grad), ("di", iv.grad)):
        _close(bw[name][0][:, :, :Fq], want, name)
        assert not bw[name][0][:, :, Fq:].any()
    want = acc.clone()
    want[:, :, :2 * Fq] += pre.grad.reshape(B, T, 2 * Fq)
    _close(bw["dpre"][0], want, "dpre = acc_in + dy gain")


def test_conv_ref_returns_the_glu_factor_dump():
    """a gated convolution of a training program: the dump holds, for the rows of this launch, acc + bias in the value columns
    and sigmoid(acc + bias) in the gate columns of the packed order -- their product is the launch's output"""
    case = tref.make_case("eabnet-B2-T6")
    ops = [o for o in case.prog.fwd if o.kind == prg.OP_CONV and o.glu_dump is not None]
    assert ops
    w = np.zeros(case.prog.w_floats, np.float32)
    ia, ib = case.prog.ia, case.prog.ib
    w[:] = np.where(ia >= 0, case.flat[ia], 0) + (np.where(ib >= 0, case.flat[ib], 0) if ib is not None else 0)
    for op in (ops[0], ops[-1]):                                             # a strided unit and a transposed phase
        rng = np.random.default_rng(5)
        lop, arena = cr.cut_out(op, w, cr.random_inputs(op, rng, 2))
        outs = cr.conv_ref(lop, arena)
        d, o = outs["glu_dump"], outs["dst"]
        c = np.arange(op.N // 2)
        rv = (c // 32) * 64 + c % 32
        fo = np.arange(op.No) * op.ostride + op.ophase
        assert d.must[:, :, fo].all() and d.must.sum() == d.must[:, :, fo].size, "the dump covers exactly the rows of this launch"
        assert np.abs(d.val[:, :, fo][..., rv] * d.val[:, :, fo][..., rv + 32] - o.val[:, :, fo]).max() < 1e-12
        gate = d.val[:, :, fo][..., rv + 32]
        assert (gate > 0).all() and (gate < 1).all() and (d.lim[:, :, fo] > 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# the dry walk
# ----------------------------------------------------------------------------------------------------------------------
def _spans(acc):
    return acc.ref.arena, acc.ref.off, acc.ref.off + acc.words


@pytest.mark.parametrize("name", list(tref.CASES))
def test_dry_walk_of_the_training_programs(name):
    """forward then backward, with nothing but the read / write table"""
    case = tref.make_case(name)
    sizes = tref.arena_sizes(case)
    written = {k: np.zeros(n, bool) for k, n in sizes.items()}
    for k in ("in", "in2", "dout", "w", "g"):            # boundary buffers, the packed weights, the zero-filled gradient arena
        if k in written:
            written[k][:] = True
    kinds = {}
    for lst_name, ops in (("fwd", case.prog.fwd), ("bwd", case.prog.bwd)):
        for k, op in enumerate(ops):
            what = f"{name} {lst_name}[{k}] {op.name}"
            acc = tref.accesses(op)
            kinds[tref.kind_name(op)] = kinds.get(tref.kind_name(op), 0) + 1
            for a in acc:
                arena, lo, hi = _spans(a)
                assert arena in sizes and 0 <= lo and hi <= sizes[arena], f"{what}: {a.name} leaves its arena"
                assert a.dtype == "f32" or lo % 2 == 0, f"{what}: {a.name} (doubles) is not 8-byte aligned"
            for a in acc:
                for b in acc:
                    if a is b or a.mode == "r" or b.mode != "r":
                        continue
                    (aa, alo, ahi), (ba, blo, bhi) = _spans(a), _spans(b)
                    if aa == ba and alo < bhi and blo < ahi:
                        assert (a.name, b.name) in tref.ALIASES and (alo, ahi) == (blo, bhi), \
                            f"{what}: {a.name} (written) overlaps {b.name} (read) and is no declared alias"
            outs = [a for a in acc if a.mode != "r"]
            for n_, a in enumerate(outs):
                for b in outs[n_ + 1:]:
                    (aa, alo, ahi), (ba, blo, bhi) = _spans(a), _spans(b)
                    assert not (aa == ba and alo < bhi and blo < ahi), f"{what}: outputs {a.name} and {b.name} overlap"
            for a in acc:
                if a.mode in ("r", "rw"):
                    arena, lo, hi = _spans(a)
                    w = written[arena][lo:hi]
                    if a.sel is not None:
                        w = w[a.sel.reshape(-1)]
                    assert w.all(), f"{what}: reads {a.name} ({arena} + {lo}) before anything wrote {int((~w).sum())} of its elements"
            for a in acc:
                if a.mode != "r":
                    arena, lo, hi = _spans(a)
                    if a.sel is None:
                        written[arena][lo:hi] = True
                    else:
                        written[arena][lo:hi] |= a.sel.reshape(-1)
    assert written["out"].all(), "the program does not write its whole output"
    print(f"{name}: {len(case.prog.fwd)} + {len(case.prog.bwd)} ops; " + ", ".join(f"{k} {v}" for k, v in sorted(kinds.items())))


# ----------------------------------------------------------------------------------------------------------------------
# the cases on the CPU: the yardstick inside the limits on the program's own activations and gradients
# ----------------------------------------------------------------------------------------------------------------------
def cpu_walk(case):
    """Interpret the programs with the references themselves: non-convolution ops take their fp32 yardstick values (checked
    against float64 and its limits first), convolutions and the LSTM the float64 result rounded to fp32.  Returns
    (ambiguous elements, elements of the ops that can have any, worst error / limit per kind)."""
    prog = case.prog
    arena = {k: np.full(n, np.nan, np.float32) for k, n in tref.arena_sizes(case).items()}
    ia, ib = prog.ia, prog.ib
    arena["w"][:] = np.where(ia >= 0, case.flat[ia], 0) + (np.where(ib >= 0, case.flat[ib], 0) if ib is not None else 0)
    arena["g"][:] = 0
    for k in ("in", "in2", "dout"):
        if k in case.boundary:
            arena[k][:] = case.boundary[k].reshape(-1)

    def fetch(a):
        v = arena[a.ref.arena][a.ref.off:a.ref.off + a.words]
        return (v.view(np.float64) if a.dtype == "f64" else v).reshape(a.shape)
    amb_total = kink_elems = 0
    worst = {}
    for lst_name, ops in (("fwd", prog.fwd), ("bwd", prog.bwd)):
        for k, op in enumerate(ops):
            what = f"{case.name} {lst_name}[{k}] {op.name}"
            outs, amb = tref.evaluate(op, fetch)
            own_yard = op.kind != prg.OP_CONV and op.kind not in (tr.OP_LSTM_TRAIN, tr.OP_LSTM_BWD)
            vals = tref.evaluate(op, fetch, np.float32)[0] if own_yard else outs
            if own_yard:
                w, _ = tref.check(outs, {n: o.val for n, o in vals.items()}, None, what)
                kn = tref.kind_name(op)
                worst[kn] = max(worst.get(kn, 0.0), w)
            if op.kind in (tr.OP_NORM_BWD, tr.OP_CLN_BWD) and "dx" in outs:
                amb_total += amb
                kink_elems += outs["dx"].val.size
            for n, o in outs.items():
                if op.kind not in (prg.OP_CONV, tr.OP_WGRAD) and tref.form_of(op) in tref.NOT_COMPARED.get(n, ()):
                    continue                                             # (reduction scratch: nothing reads it afterwards)
                dst = arena[o.ref.arena]
                if o.f64:
                    dst[o.ref.off:o.ref.off + 2 * o.val.size].view(np.float64)[:] = np.asarray(vals[n].val, np.float64).reshape(-1)
                    continue
                view = dst[o.ref.off:o.ref.off + o.val.size].reshape(o.shape)
                if o.integer:
                    view.view(np.int32)[o.must] = o.val[o.must].astype(np.int32)
                    continue
                wr = o.must if op.kind == prg.OP_CONV else np.ones(o.shape, bool)
                view[wr] = np.asarray(vals[n].val)[wr].astype(np.float32)
    assert not np.isnan(arena["out"]).any()
    return amb_total, kink_elems, worst


@pytest.mark.parametrize("name", list(tref.CASES))
def test_yardstick_stays_inside_the_limits_on_the_programs_own_data(name):
    t0 = time.time()
    case = tref.make_case(name)
    amb, elems, worst = cpu_walk(case)
    print(f"{name}: {amb} ambiguous of {elems} elements (cap {tref.KINK_CAP:g}); worst fp32 error / limit per kind: "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())) + f"; {time.time() - t0:.1f} s")
    assert amb <= tref.KINK_CAP * elems, f"{name}: {amb} of {elems} elements lie on the PReLU kink: pick another seed"
