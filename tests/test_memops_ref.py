"""The float64 references of the memory-bound inference kernels (tests/memops_ref.py), on the CPU:

1. each new reference is pinned, at 1e-12, to an independent statement of the same operation -- torch float64 modules, the
   oracle's filter_and_sum and the two Linears of LSTM_BF.w_dnn -- and the masks to the rows spelt out by hand;
2. the fp32 yardstick stays inside the derived limit on EVERY case tests/test_memops_gpu.py runs, so the limits are shown
   attainable before a device is involved;
3. a deliberately wrong reference -- microphone 16 of 17 dropped, the tables of channel c + 4, a window one frame too long, a
   running state that forgets a frame -- FAILS the same judgement: the limits tell those errors from rounding;
4. more microphones than the beam-forming kernel holds are refused where the network is described, with the reason."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import memops_ref as mo
from eabnet_amd import program as prg
from eabnet_amd.spec import NetConfig
from oracle import eabnet_oracle as orc

PIN = 1e-12


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _pin(val, want, what):
    want = want.numpy() if isinstance(want, torch.Tensor) else want
    err = float(np.abs(np.asarray(val, np.float64) - want).max())
    assert err <= PIN * max(1.0, float(np.abs(want).max())), f"{what}: {err:.3e}"


def _vals(res):
    return {k: np.asarray(r[0]) for k, r in res.items()}


def _inside(res64, res32, what, f64=()):
    """the fp32 yardstick as the 'device': inside the limits, and (trivially) the L2 criterion"""
    got = {k: (v if k in f64 else v.astype(np.float32)) for k, v in _vals(res32).items()}
    for k, r in res64.items():                       # what a launch does not write holds the sentinel
        if len(r) > 2:
            got[k] = np.where(r[3] if len(r) > 3 else r[2], got[k], mo.SENTINEL).astype(got[k].dtype)
    worst, _ = mo.judge(res64, got, res32, what, f64=f64)
    assert worst <= 1.0
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# 1. pins
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True])
def test_norm_act_is_scale_shift_prelu_of_torch(two):
    c = dict(B=3, T=9, rpt=5, C=24, two=two)
    A = mo.norm_act_inputs(c)
    got = mo.norm_act(A, np.float64, **mo.norm_act_kw(c))["out"][0]

    def operand(x, xf, sl):                          # channels-last (B, P, C) -> nn.PReLU's (B, C, P)
        x, xf = _t(x).permute(0, 2, 1), _t(xf)
        act = torch.nn.PReLU(c["C"]).double()
        with torch.no_grad():
            act.weight.copy_(_t(sl))
            return act(x * xf[:, :, 0:1] + xf[:, :, 1:2]).permute(0, 2, 1)
    want = operand(A["a"], A["xfa"], A["slopea"])
    if two:
        want = want + operand(A["b"], A["xfb"], A["slopeb"])
    _pin(got, want, "norm_act")


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("M", [1, 9, 17, 32])
def test_bfw_is_the_oracles_w_dnn_and_filter_and_sum(M, fused):
    B, T, Fq = 2, 3, 21
    A = mo.bfw_args(mo.bfw_inputs(B, T, Fq, M), fused)
    res = mo.bfw(A, np.float64, M)
    h = _t(A["h"])
    y1 = F.relu(F.linear(h, _t(A["w1"]), _t(A["b1"]))) if fused else h                 # LSTM_BF.w_dnn (oracle lstm_bf)
    w = F.linear(y1, _t(A["w2"]), _t(A["b2"])).view(B, T, Fq, M, 2)
    _pin(res["bfw"][0], w, "bfw dump")
    _pin(res["out"][0], orc.filter_and_sum(w, _t(A["x"])), "bfw out")
    assert res["out"][2].all() and res["bfw"][2].all()


def test_bfw_window_and_lengths_masks():
    B, T, Fq, M = 3, 9, 7, 5
    A = mo.bfw_inputs(B, T, Fq, M, lens=mo.LENS)
    full = mo.bfw(mo.bfw_inputs(B, T, Fq, M), np.float64, M)
    res = mo.bfw(A, np.float64, M, lens=mo.LENS)
    out, lim, must = res["out"]
    assert must.all() and np.isfinite(out).all()
    for b, n in enumerate(mo.LENS):
        assert (out[b, :, n:] == 0).all() and (lim[b, :, n:] == 0).all(), "behind a length: exact zeros"
        _pin(out[b, :, :n], full["out"][0][b, :, :n], "below a length")
        assert res["bfw"][2][b, :n].all() and not res["bfw"][2][b, n:].any() and res["bfw"][3][b].all()
    win = mo.bfw(mo.bfw_inputs(B, T, Fq, M), np.float64, M, pos=7, count=4)
    assert win["out"][2][:, :, 7:9].all() and not win["out"][2][:, :, :7].any(), "a window clipped by the end: frames 7 and 8"
    _pin(win["out"][0][:, :, 7:9], full["out"][0][:, :, 7:9], "inside the window")


def test_row_masks_by_hand():
    assert mo.rows_mask(2, 9, 8, 4).tolist() == [[False] * 8 + [True]] * 2
    assert mo.rows_mask(2, 9, 4, 4).tolist() == [[False] * 4 + [True] * 4 + [False]] * 2
    assert mo.rows_mask(3, 9, lens=mo.LENS).sum(1).tolist() == list(mo.LENS)
    c = dict(B=3, T=9, rpt=5, C=4, two=False, lens=mo.LENS)
    must = mo.norm_act(mo.norm_act_inputs(c), np.float64, **mo.norm_act_kw(c))["out"][2]
    assert [int(must[b, :, 0].sum()) for b in range(3)] == [45, 5, 25] and must[1, :5].all()
    c = dict(B=3, T=9, rpt=5, C=4, two=False, pos=8, count=4, lens=mo.LENS)            # a window wins over the lengths
    must = mo.norm_act(mo.norm_act_inputs(dict(c, lens=None)), np.float64, **mo.norm_act_kw(c))["out"][2]
    assert must[:, 40:].all() and not must[:, :40].any()


def test_cln_state_gate_rows_and_zero_rows_by_hand():
    C, Fq = 4, 3
    A = mo.cln_inputs(C, Fq)
    B, T, P = A["x"].shape
    st = mo.cln_stats(A, np.float64, C, mo.CLN_EPS)
    x64 = A["x"].astype(np.float64)
    v = np.where(x64 > 0, x64, (A["slope"].astype(np.float64) * x64.reshape(B, T, Fq, C)).reshape(B, T, P))
    want = np.concatenate([np.stack([v.sum((1, 2)), (v * v).sum((1, 2))], -1).reshape(-1), np.full(B, 7.0)])
    _pin(st["state"][0], want, "cLN running state")
    mean = v.cumsum(1).sum(2)[:, -1] / (P * T)
    _pin(st["mr"][0][:, -1, 0], mean, "cumulative mean of the last frame")
    g = mo.gate_rows(A | {"a": A["x"]}, np.float64, pos=5, count=5)
    _pin(g["z"][0], _t(A["x"]) * torch.sigmoid(_t(A["r"])), "gate")
    assert g["z"][2][:, 5:].all() and not g["z"][2][:, :5].any()
    z = mo.zero_rows(2, 7, 8, np.float64, pos=6, count=3)["ptr"]
    assert (z[0] == 0).all() and (z[1] == 0).all() and z[2].sum() == 2 * 8


# ----------------------------------------------------------------------------------------------------------------------
# 2. the yardstick is inside the limits on every case of the device file
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", mo.norm_act_cases(), ids=lambda c: c["name"])
def test_norm_act_yardstick_is_inside_the_limits(c):
    A = mo.norm_act_inputs(c)
    _inside(mo.norm_act(A, np.float64, **mo.norm_act_kw(c)), mo.norm_act(A, np.float32, **mo.norm_act_kw(c)), c["name"])


@pytest.mark.parametrize("C", mo.FIN_C)
def test_in_finalize_yardstick_is_inside_the_limits(C):
    for c in mo.in_finalize_cases():
        if c["C"] != C:
            continue
        A, count = mo.in_finalize_inputs(c)
        for s in range(c["nsets"]):
            A[f"mr{s}"] = True
        _inside(mo.in_finalize(A, np.float64, count, 1e-5), mo.in_finalize(A, np.float32, count, 1e-5), c["name"])


def test_filter_sum_yardstick_is_inside_the_limits():
    for shape in mo.FS_SHAPES + (mo.FS_LARGE[:3],):
        for M in (mo.FS_M if shape in mo.FS_SHAPES else (mo.FS_LARGE[3],)):
            A = mo.filter_sum_inputs(*shape, M)
            _inside(mo.filter_sum(A, np.float64, M), mo.filter_sum(A, np.float32, M), f"filter_sum {shape} M={M}")


@pytest.mark.parametrize("shape", mo.BFW_SHAPES, ids=str)
def test_bfw_yardstick_is_inside_the_limits(shape):
    for M in mo.BFW_M:
        for fused in (False, True):
            A = mo.bfw_args(mo.bfw_inputs(*shape, M), fused)
            _inside(mo.bfw(A, np.float64, M), mo.bfw(A, np.float32, M), f"bfw {shape} M={M} fused={fused}")


def test_bfw_yardstick_with_windows_and_lengths():
    B, T, Fq = mo.BFW_WIN["shape"]
    for M in (9, 17):
        A = mo.bfw_inputs(B, T, Fq, M)
        for count in mo.BFW_WIN["counts"]:
            for pos in mo.BFW_WIN["poss"]:
                _inside(mo.bfw(A, np.float64, M, pos=pos, count=count), mo.bfw(A, np.float32, M, pos=pos, count=count), "bfw window")
        A = mo.bfw_inputs(*mo.BFW_LENS_SHAPE, M, lens=mo.LENS)
        _inside(mo.bfw(A, np.float64, M, lens=mo.LENS), mo.bfw(A, np.float32, M, lens=mo.LENS), "bfw lens")


@pytest.mark.parametrize("C,Fq", mo.CLN_SHAPES)
def test_cln_gate_yardsticks_are_inside_the_limits(C, Fq):
    A = mo.cln_inputs(C, Fq)
    for slope in (False, True):
        S = {"x": A["x"], **({"slope": A["slope"]} if slope else {})}
        r64, r32 = mo.cln_stats(S, np.float64, C, mo.CLN_EPS), mo.cln_stats(S, np.float32, C, mo.CLN_EPS)
        _inside(r64, r32, "cln_stats", f64=("sums", "state"))
        for mode in (prg.XF_NORM_PRELU, prg.XF_PRELU_NORM):
            for add in (False, True):
                Q = {k: A[k] for k in ("x", "gain", "bias", "slope") + (("add",) if add else ())} | {"mr": r64["mr"][0].astype(np.float32)}
                _inside(mo.cln_apply(Q, np.float64, C, mode), mo.cln_apply(Q, np.float32, C, mode), "cln_apply")
    G = {"a": A["x"], "r": A["r"]}
    _inside(mo.gate_rows(G, np.float64, pos=3, count=3), mo.gate_rows(G, np.float32, pos=3, count=3), "gate_rows")


# ----------------------------------------------------------------------------------------------------------------------
# 3. wrong references fail
# ----------------------------------------------------------------------------------------------------------------------
def _as_device(res, sentinel=mo.SENTINEL):
    out = {}
    for k, r in res.items():
        v = np.asarray(r[0]).astype(np.float32)
        out[k] = np.where(r[3] if len(r) > 3 else r[2], v, sentinel) if len(r) > 2 else v
    return out


def test_a_dropped_microphone_fails():
    M = 17
    A = mo.bfw_inputs(2, 5, 161, M)
    good, yard = mo.bfw(A, np.float64, M), mo.bfw(A, np.float32, M)
    mo.judge(good, _as_device(yard), yard, "intact")
    wrong = _as_device(mo.bfw(A, np.float32, M, drop_mic=16))
    with pytest.raises(AssertionError, match="beyond the derived limit"):
        mo.judge(good, wrong, yard, "microphone 16 of 17 dropped")
    # ... also when its weight is small: a thousandth of the others' still stands out of the rounding of 17 products
    A["w2"][32:34] *= 1e-3
    A["b2"][32:34] *= 1e-3
    good, yard = mo.bfw(A, np.float64, M), mo.bfw(A, np.float32, M)
    with pytest.raises(AssertionError, match="beyond the derived limit"):
        mo.judge(good, _as_device(mo.bfw(A, np.float32, M, drop_mic=16)), yard, "a quiet microphone dropped")


@pytest.mark.parametrize("C", [24, 64])
def test_the_tables_of_another_channel_fail(C):
    c = dict(B=3, T=57, rpt=1, C=C, two=True)
    A = mo.norm_act_inputs(c)
    good, yard = mo.norm_act(A, np.float64, **mo.norm_act_kw(c)), mo.norm_act(A, np.float32, **mo.norm_act_kw(c))
    mo.judge(good, _as_device(yard), yard, "intact")
    with pytest.raises(AssertionError, match="beyond the derived limit"):
        mo.judge(good, _as_device(mo.norm_act(A, np.float32, table_shift=4, **mo.norm_act_kw(c))), yard, "tables of c + 4")
    # ... and in the last partial sweep only: the last 4 float4s of the utterance read the next float4's tables
    wrong = _as_device(yard)
    wrong["out"].reshape(3, -1)[:, -16:] = _as_device(mo.norm_act(A, np.float32, table_shift=4, **mo.norm_act_kw(c)))["out"].reshape(3, -1)[:, -16:]
    with pytest.raises(AssertionError, match="beyond the derived limit"):
        mo.judge(good, wrong, yard, "tables of c + 4 in the tail")


def test_a_window_one_frame_too_long_fails():
    c = dict(B=3, T=9, rpt=5, C=24, two=True, pos=4, count=4)
    A = mo.norm_act_inputs(c)
    good, yard = mo.norm_act(A, np.float64, **mo.norm_act_kw(c)), mo.norm_act(A, np.float32, **mo.norm_act_kw(c))
    with pytest.raises(AssertionError, match="outside the rows of the launch"):
        mo.judge(good, _as_device(mo.norm_act(A, np.float32, extra=1, **mo.norm_act_kw(c))), yard, "window + 1")
    G = mo.cln_inputs(4, 3)
    G = {"a": G["x"], "r": G["r"]}
    with pytest.raises(AssertionError, match="outside the rows of the launch"):
        mo.judge(mo.gate_rows(G, np.float64, pos=3, count=3), _as_device(mo.gate_rows(G, np.float32, pos=3, count=3, extra=1)), None, "gate + 1")
    with pytest.raises(AssertionError, match="outside the rows of the launch"):
        mo.judge(mo.zero_rows(2, 7, 8, np.float64, pos=2, count=2), _as_device(mo.zero_rows(2, 7, 8, np.float32, pos=2, count=2, extra=1)),
                 None, "zero + 1")
    # ... and one frame too short: the frame keeps the sentinel, which is no value the limit allows
    short = _as_device(yard)
    short["out"][:, 35:40] = mo.SENTINEL
    with pytest.raises(AssertionError, match="beyond the derived limit"):
        mo.judge(good, short, yard, "window - 1")


def test_a_running_state_that_forgets_a_frame_fails():
    A = mo.cln_inputs(64, 79)
    S = {"x": A["x"]}
    good = mo.cln_stats(S, np.float64, 64, mo.CLN_EPS)
    got = {k: np.asarray(v[0]).copy() for k, v in mo.cln_stats(S, np.float32, 64, mo.CLN_EPS).items()}
    mo.judge(good, got, None, "intact", f64=("sums", "state"))
    got["state"][0] -= got["sums"][0, 3, 0]
    with pytest.raises(AssertionError, match="beyond the derived limit"):
        mo.judge(good, got, None, "state without frame 3", f64=("sums", "state"))


# ----------------------------------------------------------------------------------------------------------------------
# 4. more microphones than the beam-forming kernel holds
# ----------------------------------------------------------------------------------------------------------------------
def test_more_than_32_microphones_are_refused_with_the_reason():
    import paramgen
    from eabnet_amd import model as mdl
    from eabnet_amd.spec import MAX_MICS, param_specs
    assert MAX_MICS == 32                            # BFW_MAXM of csrc/filter_sum.hip
    for make in (lambda: NetConfig(M=33), lambda: mdl.EaBNet(M=33)):
        with pytest.raises(NotImplementedError, match=r"M=33") as e:
            make()
        assert "BFW_MAXM" in str(e.value)
    cfg = NetConfig(M=32, p=1, q=1)
    prog = prg.lower(cfg, paramgen.make_params(param_specs(cfg), 3), 1, 4)
    assert any(op.kind == prg.OP_BFW_FS and op.M == 32 for op in prog.ops)
