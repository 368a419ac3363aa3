"""Training with per-utterance lengths, host side (no GPU): the opt-in switch and its refusals, the flagged lowering and its
encoding, the masked float64 references (tests/train_varlen_ref.py) proven against the unmasked ones, and the dispatch bound
of the LSTM backward."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import conv_ref as cr
import train_ref as tref
import train_varlen_ref as vref
from eabnet_amd import _lib
from eabnet_amd import model as mdl
from eabnet_amd import program as prg
from eabnet_amd import runtime
from eabnet_amd import train as tr
from eabnet_amd.spec import NetConfig

X5 = lambda B, T, M=2: torch.zeros(B, T, 161, M, 2)          # noqa: E731


# ----------------------------------------------------------------------------------------------------------------------
# 1. the switch
# ----------------------------------------------------------------------------------------------------------------------
def test_the_switch_defaults_to_off_and_the_pinned_refusals_stand():
    net = mdl.EaBNet(M=2)
    assert net.varlen_training is False
    assert mdl.GaGNet(p=1, q=1, dilas=(1,)).varlen_training is False
    with pytest.raises(NotImplementedError, match="per-utterance lengths are an inference form; training with lengths "
                                                  r"\(masked batch statistics, gradients\) is not implemented"):
        net(X5(1, 10), lengths=[4])
    bn = mdl.EaBNet(M=2, norm_type="BN").train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="is not implemented"):
        bn(X5(1, 10), lengths=[4])


def test_with_the_switch_on_a_differentiable_call_takes_the_exact_padded_width():
    net = mdl.EaBNet(M=2)
    net.varlen_training = True
    assert net._varlen_call(30, 3, [30, 17, 9], needs_graph=True) == (30, [30, 17, 9])
    dev_like = torch.tensor([30, 17, 9])
    assert net._varlen_call(30, 3, dev_like, needs_graph=True) == (30, [30, 17, 9])     # host tensor: checked values
    with pytest.raises(ValueError):
        net._varlen_call(30, 3, [30, 31, 9], needs_graph=True)
    with torch.no_grad():                                              # inference is what it was
        assert net._varlen_call(30, 3, [30, 17, 9], needs_graph=False) == (30, [30, 17, 9])
    assert net._varlen_call(30, 3, None, needs_graph=True) is None     # no lengths: the exact-shape training program


# ----------------------------------------------------------------------------------------------------------------------
# 3. refusals with the switch on, each with its reason
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,train_mode,grad,reason", [
    (dict(norm_type="BN"), True, True, "masked batch statistics"),
    (dict(norm_type="BN"), True, False, "masked batch statistics"),
    (dict(norm_type="cLN"), True, True, "reverse scan"),
    (dict(is_causal=False), True, True, "is_causal=True"),
])
def test_out_of_scope_configurations_are_refused_with_the_reason(kw, train_mode, grad, reason):
    net = mdl.EaBNet(M=2, **kw).train(train_mode)
    net.varlen_training = True
    with torch.set_grad_enabled(grad), pytest.raises(NotImplementedError, match=reason):
        net(X5(2, 10), lengths=[4, 10])


def test_buckets_and_the_post_filter_are_refused_with_the_reason():
    net = mdl.EaBNet(M=2)
    net.varlen_training, net.length_buckets = True, "auto"
    with pytest.raises(NotImplementedError, match="length_buckets"):
        net(X5(2, 10), lengths=[4, 10])
    gag = mdl.GaGNet(p=1, q=1, dilas=(1,))
    gag.varlen_training = True
    x = torch.zeros(2, 2, 10, 161)
    with pytest.raises(NotImplementedError, match="GaGNet"):
        gag(x, x, lengths=[3, 10])
    with pytest.raises(NotImplementedError, match="norm_type='BN'"):
        tr.lower_train(NetConfig(M=2, p=1, q=1, norm_type="BN"), 2, 8, varlen=True)
    with pytest.raises(NotImplementedError, match="cLN"):
        tr.lower_train(NetConfig(M=2, p=1, q=1, norm_type="cLN"), 2, 8, varlen=True)
    with pytest.raises(NotImplementedError, match="is_causal"):
        tr.lower_train(NetConfig(M=2, p=1, q=1, is_causal=False), 2, 8, varlen=True)


def _two_stage_args():
    import argparse
    return argparse.Namespace(
        k1=(2, 3), k2=(1, 3), c=64, M=2, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=1, q=1, is_causal=True, is_u2=True,
        bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="IN", ref_mic=0, freeze_eabnet=False,
        gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=1,
        gagnet_q=1, gagnet_dilas=[1], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=True,
        gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="IN")


def test_the_two_stage_wrapper_sets_the_switch_on_both_stages(monkeypatch):
    monkeypatch.setattr(mdl.GaGNet, "cuda", lambda self, *a, **k: self)         # (make_gag_net moves the post-filter to the device)
    two = mdl.EaBNetWithPostNet(_two_stage_args())
    assert two.varlen_training is False and two.eabnet.varlen_training is False and two.postnet.varlen_training is False
    two.varlen_training = True
    assert two.varlen_training is True and two.eabnet.varlen_training is True and two.postnet.varlen_training is True
    # the beam-former would take the call; the post-filter refuses it with the reason, before anything reaches a device
    x = torch.zeros(2, 2, 10, 161)
    with pytest.raises(NotImplementedError, match="GaGNet"):
        two.postnet(x, x, lengths=[3, 10])
    two.varlen_training = False
    assert two.eabnet.varlen_training is False and two.postnet.varlen_training is False


# ----------------------------------------------------------------------------------------------------------------------
# 2. the flagged lowering and its encoding
# ----------------------------------------------------------------------------------------------------------------------
CONFIGS = [dict(), dict(bf_type="cnn"), dict(topo_type="miso"), dict(intra_connect="add"), dict(is_u2=False)]
MASKED = {tr.OP_IN_STATS, tr.OP_NORM_BWD, tr.OP_LN_BWD, tr.OP_LSTM_BWD, tr.OP_FILTER_SUM, tr.OP_WGRAD, prg.OP_CONV}
ROW_LOCAL = {tr.OP_TR_NORM_ACT, tr.OP_GLU_BWD, tr.OP_GATE_FWD, tr.OP_GATE_BWD, tr.OP_ADD, tr.OP_RELU_BWD, tr.OP_LN_FWD,
             tr.OP_FS_BWD, tr.OP_LSTM_TRAIN}


def _bases(prog):
    return {"a": 1 << 20, "w": 1 << 30, "g": 1 << 32, "in": 1 << 34, "out": 1 << 35, "dout": 1 << 36, "in2": None}


@pytest.mark.parametrize("kw", CONFIGS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()) or "default")
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_flagged_program_same_ops_and_every_masked_kind_carries_the_lengths(kw, precision):
    cfg = NetConfig(M=4, p=2, q=2, **kw)
    B, T = 3, 30
    plain = tr.lower_train(cfg, B, T, 161, precision)
    flagged = tr.lower_train(cfg, B, T, 161, precision, varlen=True)
    assert flagged.varlen and not plain.varlen
    addr = 0x7F0012345600
    for name in ("fwd", "bwd"):
        a, b = getattr(plain, name), getattr(flagged, name)
        assert [(o.kind, o.name) for o in a] == [(o.kind, o.name) for o in b]
        bases = _bases(plain)
        e_plain = runtime.encode(a, bases)
        e_none = runtime.encode(b, bases)                               # lens=None: the unflagged program, byte for byte
        assert bytes(e_plain) == bytes(e_none)
        e_lens = runtime.encode(b, bases, lens=addr)
        e_plain_lens = runtime.encode(a, bases, lens=addr)              # the unflagged ops never take the pointer (convs aside)
        kinds = set()
        for o, op, p0 in zip(e_lens, b, e_plain_lens):
            got = o.conv.win.lens if op.kind == prg.OP_CONV else o.win.lens
            if op.kind in MASKED:
                assert got == addr, f"{op.name}: no lengths pointer"
                kinds.add(op.kind)
            elif op.kind in ROW_LOCAL:
                assert got is None, f"{op.name}: a row-local op needs no lengths"
            else:                           # (the zero fill and the finalisation take a window in streaming programs: both ignore lens)
                assert op.kind in (prg.OP_IN_FINALIZE, prg.OP_MEMSET0), op.name
            if op.kind in MASKED - {prg.OP_CONV} or op.kind in ROW_LOCAL:
                assert p0.win.lens is None, f"{op.name}: an unflagged program must not hand out the pointer"
            if op.kind == tr.OP_IN_STATS:
                assert o.i[4] == T and o.i[1] % T == 0
            elif op.kind == tr.OP_NORM_BWD:
                assert o.i[5] == T and o.i[1] % T == 0
            elif op.kind == tr.OP_LN_BWD:
                assert (o.i[2], o.i[3]) == (B, T)
            elif op.kind == tr.OP_WGRAD:
                assert (o.wgrad.B, o.wgrad.T) == (B, T)
            elif op.kind in (tr.OP_LSTM_BWD, tr.OP_FILTER_SUM):
                assert (o.i[0], o.i[1]) == (B, T)
        want = {prg.OP_CONV, tr.OP_IN_STATS, tr.OP_FILTER_SUM} if name == "fwd" else {prg.OP_CONV, tr.OP_NORM_BWD, tr.OP_WGRAD}
        if name == "bwd" and cfg.bf_type == "lstm" and cfg.topo_type == "mimo":
            want |= {tr.OP_LN_BWD, tr.OP_LSTM_BWD}
        assert want <= kinds, (name, want - kinds)
    # every op kind of the programs is either masked, or row-local, or one of the two that need nothing
    for o in list(flagged.fwd) + list(flagged.bwd):
        assert o.kind in MASKED | ROW_LOCAL | {prg.OP_IN_FINALIZE, prg.OP_MEMSET0}, f"{o.name}: a kind nobody classified"


def test_lens_entry_points_exist_and_check_their_frame_count():
    lib = _lib.load()
    for n in ("eab_train_in_stats_lens_f32", "eab_train_in1d_lens_f32", "eab_train_in1d_multi_lens_f32", "eab_train_norm_bwd_lens_f32",
              "eab_train_norm_bwd_multi_lens_f32", "eab_layernorm64_bwd_lens_f32", "eab_lstm64_bwd_lens_f32",
              "eab_filter_sum_ld_lens_f32", "eab_wgrad_batch_lens_f32", "eab_lstm64_bwd_form"):
        assert hasattr(lib, n)
    assert lib.eab_abi_version() == 10
    # lengths without the frame count they divide, or positions no whole number of frames: refused before any launch
    one = C.c_void_p(16)
    assert lib.eab_train_in_stats_lens_f32(one, one, 2, 50, 64, 1e-5, one, one, one, one, one, 7, None) == 1
    assert lib.eab_train_norm_bwd_lens_f32(*([one] * 12), 2, 50, 64, 1, one, 0, None) == 1
    assert lib.eab_layernorm64_bwd_lens_f32(*([one] * 7), 100, one, 3, 7, None) == 1


# ----------------------------------------------------------------------------------------------------------------------
# 5. the LSTM backward's choice of kernel
# ----------------------------------------------------------------------------------------------------------------------
def test_lstm_backward_takes_the_4_sequence_kernel_only_below_2_gib():
    """The 4-sequence kernel masks loads with the offset 2^31 of a buffer descriptor over the whole gate tensor; between 2 and
    4 GiB that offset lies INSIDE the tensor.  B = 12, F = 161: T = 868 is the last frame count below 2^31 bytes."""
    lib = _lib.load()
    S = 12 * 161
    assert S * 868 * 5 * 64 * 4 < 2 ** 31 <= S * 869 * 5 * 64 * 4 < 2 ** 32
    Q, K16, K16B = 0, 1, 2
    assert lib.eab_lstm64_bwd_form(12, 868, 161, prg.PREC_F32) == Q
    assert lib.eab_lstm64_bwd_form(12, 869, 161, prg.PREC_F32) == K16
    assert lib.eab_lstm64_bwd_form(12, 869, 161, prg.PREC_BF16) == K16       # (1932 sequences: exact products in every mode)
    assert lib.eab_lstm64_bwd_form(6, 601, 161, prg.PREC_F32) == Q           # the benchmark's training shape
    assert lib.eab_lstm64_bwd_form(6, 601, 161, prg.PREC_BF16) == Q
    assert lib.eab_lstm64_bwd_form(13, 100, 161, prg.PREC_F32) == K16        # 2093 sequences
    assert lib.eab_lstm64_bwd_form(13, 100, 161, prg.PREC_BF16) == K16B
    assert lib.eab_lstm64_bwd_form(0, 100, 161, prg.PREC_F32) < 0
    assert lib.eab_lstm64_bwd_form(1, 100, 161, prg.PREC_F16X3) < 0


# ----------------------------------------------------------------------------------------------------------------------
# 4. the masked references: the padded batch (NaN in every padding row) == every utterance alone, summed where the op sums
# ----------------------------------------------------------------------------------------------------------------------
B_, T_, LENS = 3, 24, [24, 13, 5]
REL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(got).all(), f"{what}: padding reached the result"
    err = np.abs(got - want).max(initial=0.0)
    assert err <= REL * max(np.abs(want).max(initial=0.0), 1e-300), f"{what}: {err:.3e}"


def _padded(rng, shape_of, lens=LENS, T=T_, axis=1):
    """per-utterance random arrays (made first, each on its own) and the padded batch with NaN behind every length"""
    alone = [rng.standard_normal(shape_of(n)) for n in lens]
    full = np.full((len(lens),) + shape_of(T), np.nan)
    for b, (a, n) in enumerate(zip(alone, lens)):
        full[b][:a.shape[0]] = a
    return alone, full


@pytest.mark.parametrize("multi,ppf", [(False, 1), (False, 3), (True, 1)])
def test_masked_in_stats_reference(multi, ppf):
    rng = np.random.default_rng(1)
    xC, C = (16, 32) if multi else (16, 16)
    alone, x = _padded(rng, lambda n: (n * ppf, xC))
    par = dict(slope=rng.uniform(0.05, 0.5, C), gamma=rng.uniform(0.5, 1.5, C), beta=rng.standard_normal(C))
    outs = vref.in_stats([B_, T_ * ppf, C] + ([xC] if multi else []), [1e-5], dict(par, x=x, y=True), LENS, T_, multi=multi)
    form = "IN_STATS_MULTI" if multi else "IN_STATS"
    for b, n in enumerate(LENS):
        want, _ = tref.run_ref(form, [1, n * ppf, C, xC if multi else 0], [1e-5], dict(par, x=alone[b][None], y=True))
        _close(outs["xf"].val[b], want["xf"][0][0], "xf")
        _close(outs["mr"].val[b], want["mr"][0][0], "mr")
        yb = outs["y"].val[:, b] if multi else outs["y"].val[b]
        mb = outs["y"].must[:, b] if multi else outs["y"].must[b]
        wy = want["y"][0][:, 0] if multi else want["y"][0][0]
        _close(yb[..., :n * ppf, :], wy, "y")
        assert mb[..., :n * ppf, :].all() and not mb[..., n * ppf:, :].any()


@pytest.mark.parametrize("mode,norm,multi", [(prg.XF_NORM_PRELU, True, False), (prg.XF_NORM_PRELU, False, False),
                                             (prg.XF_PRELU_NORM, True, False), (prg.XF_PRELU_NORM, True, True)])
def test_masked_norm_bwd_reference(mode, norm, multi):
    rng = np.random.default_rng(2)
    ppf, xC = 2, 16
    C = 2 * xC if multi else xC
    xs, x = _padded(rng, lambda n: (n * ppf, xC))
    ds, dy = _padded(rng, lambda n: (n * ppf, xC))
    d1s, dy1 = _padded(rng, lambda n: (n * ppf, xC))
    accs, acc = _padded(rng, lambda n: (n * ppf, xC))
    par = dict(slope=rng.uniform(0.05, 0.5, C), gamma=rng.uniform(0.5, 1.5, C))
    if not multi:
        par["beta"] = rng.standard_normal(C)
    mr = np.stack([rng.standard_normal((B_, C)), rng.uniform(0.5, 2.0, (B_, C))], -1) if norm else None
    prev = {k: rng.standard_normal(C) for k in ("dgamma", "dbeta", "dslope")}
    if not norm:
        par.pop("gamma"), par.pop("beta"), prev.pop("dgamma"), prev.pop("dbeta")
    A = dict(par, dy=dy, x=x, acc_in=acc, **prev)
    if norm:
        A["mr"] = mr
    if multi:
        A["dy1"] = dy1
    i = [B_, T_ * ppf, C, mode] + ([xC] if multi else [])
    outs, _ = vref.norm_bwd(i, [], A, LENS, T_)
    want_p = {k: v.copy() for k, v in prev.items()}
    form = "NORM_BWD_MULTI" if multi else "NORM_BWD"
    for b, n in enumerate(LENS):
        Ab = dict(par, dy=ds[b][None], x=xs[b][None], acc_in=accs[b][None], **{k: np.zeros(C) for k in prev})
        if norm:
            Ab["mr"] = mr[b:b + 1]
        if multi:
            Ab["dy1"] = d1s[b][None]
        w, _ = tref.run_ref(form, [1, n * ppf, C, mode] + ([xC] if multi else []), [], Ab)
        _close(outs["dx"].val[b, :n * ppf], w["dx"][0][0], "dx")
        assert not outs["dx"].must[b, n * ppf:].any()
        for k in prev:
            want_p[k] = want_p[k] + w[k][0]
    for k in prev:
        _close(outs[k].val, want_p[k], k)


def test_masked_head_references():
    rng = np.random.default_rng(3)
    F = 5
    # LayerNorm backward
    xs, x = _padded(rng, lambda n: (n, F, 64))
    ds, dy = _padded(rng, lambda n: (n, F, 64))
    ms, mr = _padded(rng, lambda n: (n, F, 2))
    g, dg0, db0 = rng.standard_normal(64), rng.standard_normal(64), rng.standard_normal(64)
    rows = B_ * T_ * F
    outs = vref.ln_bwd(dict(dy=dy.reshape(rows, 64), x=x.reshape(rows, 64), mr=mr.reshape(rows, 2), g=g, dg=dg0, db=db0), LENS, B_, T_)
    dg, db = dg0.copy(), db0.copy()
    for b, n in enumerate(LENS):
        nr = n * F
        w, _ = tref.run_ref("LN_BWD", [nr, 0], [], dict(dy=ds[b].reshape(nr, 64), x=xs[b].reshape(nr, 64), mr=ms[b].reshape(nr, 2), g=g,
                                                        dg=np.zeros(64), db=np.zeros(64)))
        _close(outs["dx"].val.reshape(B_, T_, F, 64)[b, :n].reshape(nr, 64), w["dx"][0], "ln dx")
        dg, db = dg + w["dg"][0], db + w["db"][0]
    _close(outs["dg"].val, dg, "dg")
    _close(outs["db"].val, db, "db")
    # LSTM backward: sequence s = b * F + f
    gs, _ = _padded(rng, lambda n: (n, F, 5, 64))
    gates = np.full((B_ * F, T_, 5, 64), np.nan)
    for b, n in enumerate(LENS):
        gs[b] = 1 / (1 + np.exp(-gs[b]))
        gates[b * F:(b + 1) * F, :n] = gs[b].transpose(1, 0, 2, 3)
    hs, dh = _padded(rng, lambda n: (n, F, 64))
    wcat = 0.2 * rng.standard_normal((256, 128))
    outs = vref.lstm_bwd([B_, T_, F, prg.PREC_F32], dict(gates=gates, dh_out=dh, wcat=wcat, dgates=True), LENS)
    for b, n in enumerate(LENS):
        w, _ = tref.run_ref("LSTM_BWD", [1, n, F, prg.PREC_F32], [], dict(gates=gs[b].transpose(1, 0, 2, 3), dh_out=hs[b][None], wcat=wcat))
        _close(outs["dgates"].val[b, :n], w["dgates"][0][0], "dgates")
        assert (outs["dgates"].val[b, n:] == 0).all() and outs["dgates"].must[b, n:].all()
    # filter-and-sum
    M, ld = 3, 8
    ws, wt = _padded(rng, lambda n: (n, F, ld))
    xs, x = _padded(rng, lambda n: (n, F, M, 2))
    outs = vref.filter_sum([B_, T_, F, M, ld], dict(w=wt, x=x), LENS)
    for b, n in enumerate(LENS):
        w, _ = tref.run_ref("FILTER_SUM", [1, n, F, M, ld], [], dict(w=ws[b][None], x=xs[b][None]))
        _close(outs["y"].val[b, :, :n], w["y"][0][0], "filter_sum")
        assert (outs["y"].val[b, :, n:] == 0).all() and (outs["y"].lim[b, :, n:] == 0).all() and outs["y"].must[b, :, n:].all()


@pytest.mark.parametrize("geom,N,C0,C1", [(prg.Geometry.pointwise(5), 64, 16, 0), (prg.Geometry.pointwise(5, dt=-1), 64, 16, 0),
                                          (prg.Geometry.temporal([-4, -2, 0]), 64, 32, 0), (prg.Geometry.strided(9, 2, 3), 64, 16, 0),
                                          (prg.Geometry.transposed(4, 2, 3)[1], 64, 16, 16)])
def test_masked_wgrad_reference(geom, N, C0, C1):
    rng = np.random.default_rng(4)
    op = tr.WgradOp(dz=None, src0=None, src1=True if C1 else None, dw=None, N=N, C0=C0, C1=C1, Kpad=geom.kpad(C0 + C1), B=B_, T=T_, Fin=geom.Fin,
                    Fz=geom.Fout, No=geom.No, ostride=geom.ostride, ophase=geom.ophase, istride=geom.istride, dt=list(geom.dt),
                    ioff=list(geom.ioff), dbias=True)
    zs, dz = _padded(rng, lambda n: (n, geom.Fout, N))
    s0, src0 = _padded(rng, lambda n: (n, geom.Fin, C0))
    s1, src1 = _padded(rng, lambda n: (n, geom.Fin, C1)) if C1 else (None, None)
    dw0, db0 = rng.standard_normal((N, op.Kpad)), rng.standard_normal(N)
    outs = vref.wgrad(op, dict(dz=dz, src0=src0, src1=src1, dw=dw0, dbias=db0), LENS)
    dw, db = dw0.copy(), db0.copy()
    m = tref._M(np.float64)
    for b, n in enumerate(LENS):
        sub = dataclasses.replace(op, B=1, T=n)
        A = dict(dz=zs[b][None], src0=s0[b][None], src1=None if s1 is None else s1[b][None])
        t = tref.wgrad_terms(sub, A, m)
        dw, db = dw + t[0], db + t[2]
    _close(outs["dw"].val, dw, "dw")
    _close(outs["dbias"].val, db, "dbias")


def test_masked_dgrad_reference_with_look_ahead_taps():
    """The adjoint of a causal dilated convolution reads LATER frames (dt > 0): frames just below an utterance's end must see
    zeros where the padded batch holds padding -- here NaN, so any read of it shows."""
    rng = np.random.default_rng(5)
    fwd = prg.Geometry.temporal([-4, -2, 0])
    gd, = prg.Geometry.adjoint(fwd)
    assert max(gd.dt) > 0
    N, Cz = 16, 32                                        # output channels of the dgrad = input channels of the forward

    class V:                                              # what conv_launch asks of a source
        def __init__(self, ref, F, C):
            self.ref, self.F, self.C = ref, F, C
    wimg = prg.pack_taps(rng.standard_normal((N, Cz, 3)).astype(np.float32), gd.taps)
    nz, nd, nw = B_ * T_ * Cz, B_ * T_ * N, wimg.size
    op = prg.conv_launch("dgrad", B_, T_, [V(prg.Ref("x", 0), 1, Cz)], prg.Ref("x", nz + nd), None, gd, N=N, epi=prg.EPI_LINEAR,
                         dst=prg.Ref("x", nz), bm=64)
    zs, dz = _padded(rng, lambda n: (n, 1, Cz))
    arena = {"x": np.concatenate([dz.reshape(-1), np.full(nd, np.nan), wimg.reshape(-1)]).astype(np.float32)}
    outs = vref.conv(op, arena, LENS)
    for b, n in enumerate(LENS):
        sub = dataclasses.replace(op, B=1, T=n, src0=prg.Ref("y", 0), dst=prg.Ref("y", n * Cz), w=prg.Ref("y", n * Cz + n * N))
        a = {"y": np.concatenate([zs[b].reshape(-1), np.full(n * N, np.nan), wimg.reshape(-1)]).astype(np.float32)}
        want = cr.conv_ref(sub, a)["dst"]
        _close(outs["dst"].val[b, :n], want.val[0], "dgrad dst")
        assert outs["dst"].must[b, :n].all() and not outs["dst"].must[b, n:].any() and not outs["dst"].may[b, n:].any()
    # and the unmasked launch on the padded batch is NOT that: its look-ahead taps read the padding
    with np.errstate(invalid="ignore"):
        plain = cr.conv_ref(op, arena)["dst"].val
    assert np.isnan(plain[1, LENS[1] - 1]).any()
