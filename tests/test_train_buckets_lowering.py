"""Training length buckets, host side (no GPU): the switch, its validation and cap selection; the pinned behaviour
with the switch unset; the refusals on CPU tensors; the flagged lowering of the post-filter (four configurations, both
precisions) and of the beam-former's bucket form with their encodings; the new entry points; the masked float64 references of
the post-filter's tail (tests/train_buckets_ref.py) proven against the unmasked ones."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_buckets_ref as bref
import train_ref as tref
from eabnet_amd import _lib
from eabnet_amd import model as mdl
from eabnet_amd import program as prg
from eabnet_amd import runtime
from eabnet_amd import train as tr
from eabnet_amd import train_gag as tg
from eabnet_amd.spec import GagConfig, NetConfig

X5 = lambda B, T, M=2: torch.zeros(B, T, 161, M, 2)          # noqa: E731
X4 = lambda B, T: torch.zeros(B, 2, T, 161)                  # noqa: E731
GAG = dict(p=1, q=1, dilas=(1,))


# ----------------------------------------------------------------------------------------------------------------------
# 1. the switch
# ----------------------------------------------------------------------------------------------------------------------
def test_the_switch_defaults_to_none_and_is_validated_like_length_buckets():
    for net in (mdl.EaBNet(M=2), mdl.GaGNet(**GAG)):
        assert net.train_length_buckets is None
        assert net._varlen_call(30, 3, None, needs_graph=True) is None          # unset: the exact-shape training program
        net.train_length_buckets = "auto"
        assert net._bucket_caps("train_length_buckets") == mdl.AUTO_BUCKETS
        net.train_length_buckets = (32, 48)
        assert net._bucket_caps("train_length_buckets") == (32, 48)
        assert net._bucket_caps() == ()                                         # the inference buckets are another switch
        for bad in ("big", (), (0, 8), (16, 16), (32, 16), (8.5, "x")):
            net.train_length_buckets = bad
            with pytest.raises(ValueError, match="train_length_buckets"):
                net._varlen_call(10, 2, [4, 10], needs_graph=True)


def test_cap_selection_and_lengths():
    net = mdl.EaBNet(M=2)
    net.train_length_buckets = (32, 64)
    assert net._varlen_call(30, 3, [30, 17, 9], needs_graph=True) == (32, [30, 17, 9])
    assert net._varlen_call(32, 3, [30, 17, 9], needs_graph=True) == (32, [30, 17, 9])
    assert net._varlen_call(33, 3, [30, 17, 9], needs_graph=True) == (64, [30, 17, 9])
    assert net._varlen_call(65, 3, [65, 17, 9], needs_graph=True) == (65, [65, 17, 9])      # past every cap: the exact width
    assert net._varlen_call(30, 3, None, needs_graph=True) == (32, 30)                      # no lengths: every utterance T frames
    assert net._varlen_call(30, 3, torch.tensor([30, 17, 9]), needs_graph=True) == (32, [30, 17, 9])
    with pytest.raises(ValueError):
        net._varlen_call(30, 3, [30, 31, 9], needs_graph=True)
    with pytest.raises(ValueError):
        net._varlen_call(30, 3, [30, 9], needs_graph=True)
    # inference is what it was: the training switch does not reach it
    assert net._varlen_call(30, 3, [30, 17, 9], needs_graph=False) == (30, [30, 17, 9])
    assert net._varlen_call(30, 3, None, needs_graph=False) is None
    # varlen_training need not be set; set, the bucket switch wins for the calls it covers
    net.varlen_training = True
    assert net._varlen_call(30, 3, [30, 17, 9], needs_graph=True) == (32, [30, 17, 9])
    # ... and varlen_training together with length_buckets keeps its refusal
    net.length_buckets = "auto"
    with pytest.raises(NotImplementedError, match="length_buckets together with a differentiable call"):
        net._varlen_call(30, 3, [30, 17, 9], needs_graph=True)


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
    assert two.train_length_buckets is None and two.eabnet.train_length_buckets is None and two.postnet.train_length_buckets is None
    two.train_length_buckets = (32,)
    assert two.train_length_buckets == (32,) and two.eabnet.train_length_buckets == (32,) and two.postnet.train_length_buckets == (32,)
    assert two.postnet._varlen_call(26, 3, [26, 15, 7], needs_graph=True) == (32, [26, 15, 7])
    two.train_length_buckets = None
    assert two.eabnet.train_length_buckets is None and two.postnet.train_length_buckets is None
    # the other two switches are untouched by it
    assert two.length_buckets is None and two.varlen_training is False


# ----------------------------------------------------------------------------------------------------------------------
# 2. with the switch unset every pinned behaviour holds (re-asserted here; tests/test_train_varlen_lowering.py is the pin)
# ----------------------------------------------------------------------------------------------------------------------
def test_with_the_switch_unset_the_pinned_refusals_stand():
    net = mdl.EaBNet(M=2)
    with pytest.raises(NotImplementedError, match="per-utterance lengths are an inference form; training with lengths "
                                                  r"\(masked batch statistics, gradients\) is not implemented"):
        net(X5(1, 10), lengths=[4])
    net.varlen_training, net.length_buckets = True, "auto"
    with pytest.raises(NotImplementedError, match="length_buckets"):
        net(X5(2, 10), lengths=[4, 10])
    gag = mdl.GaGNet(**GAG)
    with pytest.raises(NotImplementedError, match="is not implemented"):
        gag(X4(2, 10), X4(2, 10), lengths=[3, 10])
    gag.varlen_training = True
    with pytest.raises(NotImplementedError, match="GaGNet"):
        gag(X4(2, 10), X4(2, 10), lengths=[3, 10])


# ----------------------------------------------------------------------------------------------------------------------
# 3. refusals with the switch set, each with its reason, before anything reaches a device (CPU tensors)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,grad,reason", [
    (dict(norm_type="BN"), True, "masked batch statistics"),
    (dict(norm_type="BN"), False, "masked batch statistics"),
    (dict(norm_type="cLN"), True, "reverse scan"),
    (dict(is_causal=False), True, "is_causal=True"),
])
@pytest.mark.parametrize("lengths", [[4, 10], None])
def test_out_of_scope_configurations_are_refused_with_the_reason(kw, grad, reason, lengths):
    want = tr.varlen_unsupported_reason(NetConfig(M=2, **kw))
    assert reason in want
    gag = kw.get("norm_type") != "cLN"                       # (the post-filter is offered with IN / BN only)
    nets = [(mdl.EaBNet(M=2, **kw), (X5(2, 10),))] + ([(mdl.GaGNet(**GAG, **kw), (X4(2, 10), X4(2, 10)))] if gag else [])
    for net, args in nets:
        net.train().train_length_buckets = "auto"
        with torch.set_grad_enabled(grad), pytest.raises(NotImplementedError) as e:
            net(*args, lengths=lengths)
        assert want in str(e.value)
    lowers = [(tr.lower_train, NetConfig(M=2, p=1, q=1, **kw))] + ([(tg.lower_train, GagConfig(p=1, q=1, dilas=(1,), **kw))] if gag else [])
    for lower, cfg in lowers:
        for flags in (dict(bucket=True), dict(varlen=True)):
            with pytest.raises(NotImplementedError) as e:
                lower(cfg, 2, 8, **flags)
            assert want in str(e.value)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the flagged lowerings and their encodings
# ----------------------------------------------------------------------------------------------------------------------
# every op kind of the post-filter's two programs, classified (DESIGN §4.27's table)
GAG_MASKED = {prg.OP_CONV, prg.OP_GAG_PACK, prg.OP_GAG_CRM, prg.OP_GAG_CRM_BWD, tr.OP_IN_STATS, tr.OP_NORM_BWD, tr.OP_WGRAD}
GAG_ROW_LOCAL = {tr.OP_TR_NORM_ACT, tr.OP_GLU_BWD, tr.OP_ADD}
NEED_NOTHING = {prg.OP_IN_FINALIZE, prg.OP_MEMSET0}          # (they take a window in streaming programs; both ignore lens)
GAG_CONFIGS = {"default": {}, "squeezed": dict(is_squeezed=True), "unet": dict(is_u2=False), "add": dict(intra_connect="add")}
ADDR = 0x7F0012345600


def _bases():
    return {"a": 1 << 20, "w": 1 << 30, "g": 1 << 32, "in": 1 << 34, "out": 1 << 35, "dout": 1 << 36, "in2": 1 << 37}


def _lens_of(o, op):
    return o.conv.win.lens if op.kind == prg.OP_CONV else o.win.lens


def _check_bt(o, op, B, T):
    if op.kind == prg.OP_CONV:
        assert (o.conv.B, o.conv.T) == (B, T)
    elif op.kind == tr.OP_WGRAD:
        assert (o.wgrad.B, o.wgrad.T) == (B, T)
    elif op.kind == tr.OP_IN_STATS:
        assert o.i[4] == T and o.i[1] % T == 0 and o.i[0] == B
    elif op.kind == tr.OP_NORM_BWD:
        assert o.i[5] == T and o.i[1] % T == 0 and o.i[0] == B
    elif op.kind == tr.OP_LN_BWD:
        assert (o.i[2], o.i[3]) == (B, T)
    else:                                                    # GAG_PACK, GAG_CRM, GAG_CRM_BWD, LSTM_*, FILTER_SUM: i[0..1] = B, T
        assert (o.i[0], o.i[1]) == (B, T), op.name


@pytest.mark.parametrize("name", sorted(GAG_CONFIGS))
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("flag", ["varlen", "bucket"])
def test_post_filter_flagged_program_same_ops_and_every_masked_kind_carries_the_lengths(name, precision, flag):
    cfg = GagConfig(p=1, q=2, dilas=(1, 2), **GAG_CONFIGS[name])
    B, T = 3, 32
    plain = tg.lower_train(cfg, B, T, 161, precision)
    flagged = tg.lower_train(cfg, B, T, 161, precision, **{flag: True})
    assert flagged.varlen and not plain.varlen and flagged.bucket == (flag == "bucket") and not plain.bucket
    assert flagged.lanes == plain.lanes and flagged.sync == plain.sync          # the three lanes: one program, one lengths array
    assert max(flagged.lanes["fwd"]) == (1 if cfg.is_squeezed else 2) and max(flagged.lanes["bwd"]) == max(flagged.lanes["fwd"])
    for which in ("fwd", "bwd"):
        a, b = getattr(plain, which), getattr(flagged, which)
        assert [(o.kind, o.name) for o in a] == [(o.kind, o.name) for o in b]
        assert bytes(runtime.encode(a, _bases())) == bytes(runtime.encode(b, _bases()))       # lens=None: byte for byte
        kinds = set()
        for o, op in zip(runtime.encode(b, _bases(), lens=ADDR), b):
            assert op.kind in GAG_MASKED | GAG_ROW_LOCAL | NEED_NOTHING, f"{op.name}: a kind nobody classified"
            if op.kind in GAG_MASKED:
                assert _lens_of(o, op) == ADDR, f"{op.name}: no lengths pointer"
                _check_bt(o, op, B, T)
                kinds.add(op.kind)
            elif op.kind in GAG_ROW_LOCAL:
                assert _lens_of(o, op) is None, f"{op.name}: a row-local op needs no lengths"
        want = ({prg.OP_CONV, prg.OP_GAG_PACK, prg.OP_GAG_CRM, tr.OP_IN_STATS} if which == "fwd" else
                {prg.OP_CONV, prg.OP_GAG_CRM_BWD, tr.OP_NORM_BWD, tr.OP_WGRAD})
        assert want <= kinds, (which, want - kinds)
        # all lanes of one lane-tagged list read the same pointer
        assert {_lens_of(o, op) for o, op in zip(runtime.encode(b, _bases(), lens=ADDR), b) if op.kind in GAG_MASKED} == {ADDR}
    # the unflagged program's own ops take no pointer either way (the convolutions and pack / CRM, which have a window, aside)
    for o, op in zip(runtime.encode(plain.bwd, _bases(), lens=ADDR), plain.bwd):
        if op.kind in (prg.OP_GAG_CRM_BWD, tr.OP_NORM_BWD, tr.OP_WGRAD):
            assert o.win.lens is None, op.name


EAB_MASKED = {tr.OP_IN_STATS, tr.OP_NORM_BWD, tr.OP_LN_BWD, tr.OP_LSTM_BWD, tr.OP_FILTER_SUM, tr.OP_WGRAD, prg.OP_CONV}
EAB_ROW_LOCAL = {tr.OP_TR_NORM_ACT, tr.OP_GLU_BWD, tr.OP_GATE_FWD, tr.OP_GATE_BWD, tr.OP_ADD, tr.OP_RELU_BWD, tr.OP_LN_FWD, tr.OP_FS_BWD}


@pytest.mark.parametrize("kw", [dict(), dict(bf_type="cnn"), dict(is_u2=False)], ids=["default", "cnn", "unet"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_beam_former_bucket_form_flags_the_lstm_forward_there_and_only_there(kw, precision):
    cfg = NetConfig(M=4, p=2, q=2, **kw)
    B, T = 3, 32
    plain = tr.lower_train(cfg, B, T, 161, precision)
    varlen = tr.lower_train(cfg, B, T, 161, precision, varlen=True)
    bucket = tr.lower_train(cfg, B, T, 161, precision, bucket=True)
    assert bucket.varlen and bucket.bucket and varlen.varlen and not varlen.bucket
    lstm = cfg.bf_type == "lstm"
    for which in ("fwd", "bwd"):
        a, v, b = (getattr(p_, which) for p_ in (plain, varlen, bucket))
        assert [(o.kind, o.name) for o in a] == [(o.kind, o.name) for o in b]
        assert bytes(runtime.encode(a, _bases())) == bytes(runtime.encode(b, _bases()))
        seen = set()
        for ob, ov, op in zip(runtime.encode(b, _bases(), lens=ADDR), runtime.encode(v, _bases(), lens=ADDR), b):
            assert op.kind in EAB_MASKED | EAB_ROW_LOCAL | NEED_NOTHING | {tr.OP_LSTM_TRAIN}, f"{op.name}: a kind nobody classified"
            if op.kind in EAB_MASKED:
                assert _lens_of(ob, op) == ADDR and _lens_of(ov, op) == ADDR, op.name
                _check_bt(ob, op, B, T)
            elif op.kind in EAB_ROW_LOCAL:
                assert _lens_of(ob, op) is None and _lens_of(ov, op) is None, op.name
            if op.kind == tr.OP_LSTM_TRAIN:                  # flagged by the bucket form, row-local under varlen=True (pinned)
                assert ob.win.lens == ADDR and ov.win.lens is None
                _check_bt(ob, op, B, T)
            if op.kind == tr.OP_LSTM_BWD:                    # the bound flag travels in i[4], only with the pointer
                assert ob.i[4] == 1 and ov.i[4] == 0
            seen.add(op.kind)
        assert (tr.OP_LSTM_TRAIN in seen) == (lstm and which == "fwd") and (tr.OP_LSTM_BWD in seen) == (lstm and which == "bwd")
        for o in runtime.encode(b, _bases()):               # without the pointer no slot is written
            if o.kind == tr.OP_LSTM_BWD:
                assert o.i[4] == 0
    # the measurement switch: the bucket form with both recurrences walking the cap
    off = tr.lower_train(cfg, B, T, 161, precision, bucket=True, lstm_bound=False)
    assert off.bucket
    for which in ("fwd", "bwd"):
        for o, op in zip(runtime.encode(getattr(off, which), _bases(), lens=ADDR), getattr(off, which)):
            if op.kind == tr.OP_LSTM_TRAIN:
                assert o.win.lens is None
            if op.kind == tr.OP_LSTM_BWD:
                assert o.win.lens == ADDR and o.i[4] == 0


# ----------------------------------------------------------------------------------------------------------------------
# 5. the entry points
# ----------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_exist_and_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    for n in ("eab_gag_crm_bwd_lens_f32", "eab_lstm64_train_fwd_lens_f32", "eab_lstm64_train_fwd_lens_prec_f32", "eab_lstm64_bwd_bound_f32"):
        assert hasattr(lib, n) and n in _lib.EXPORTS
    assert lib.eab_abi_version() == 10
    one = C.c_void_p(16)
    EINVAL = 1
    crm = lambda *a: lib.eab_gag_crm_bwd_lens_f32(*a)                            # noqa: E731
    ok_tail = (3, 24, 161, 384, 192, prg.ACT_SIGMOID, one, None)
    assert crm(None, one, one, one, None, one, one, one, one, *ok_tail) == EINVAL                        # no pre
    assert crm(one, one, None, None, None, one, one, one, one, *ok_tail) == EINVAL                       # neither gradient
    assert crm(one, one, one, None, None, one, one, one, one, 3, 24, 161, 320, 192, 0, one, None) == EINVAL    # ld < 2F
    assert crm(one, one, one, None, None, one, one, one, one, 3, 24, 161, 384, 160, 0, one, None) == EINVAL    # lin_ld < F
    assert crm(one, one, one, None, None, one, one, one, one, 3, 24, 161, 384, 192, 7, one, None) == EINVAL    # activation
    assert crm(one, one, one, None, None, one, one, one, one, 0, 24, 161, 384, 192, 0, one, None) == EINVAL    # B
    fwd = lib.eab_lstm64_train_fwd_lens_prec_f32
    assert fwd(None, one, one, one, one, one, 3, 24, 161, prg.PREC_F32, None) == EINVAL
    assert fwd(one, one, one, one, one, one, 3, 24, 161, prg.PREC_F16X3, None) == EINVAL
    assert fwd(one, one, one, one, one, one, 3, 0, 161, prg.PREC_F32, None) == EINVAL
    assert fwd(one, one, one, one, one, one, 64, 1 << 14, 161, prg.PREC_BF16, None) == EINVAL          # past 31-bit byte offsets
    assert lib.eab_lstm64_train_fwd_lens_f32(one, one, one, one, None, one, 3, 24, 161, None) == EINVAL
    bwd = lib.eab_lstm64_bwd_bound_f32
    assert bwd(one, one, one, one, None, 1, 3, 24, 161, prg.PREC_F32, None) == EINVAL                   # a bound needs lengths
    assert bwd(one, one, one, None, one, 1, 3, 24, 161, prg.PREC_F32, None) == EINVAL
    assert bwd(one, one, one, one, one, 1, 3, 24, 161, prg.PREC_F16X3, None) == EINVAL


# ----------------------------------------------------------------------------------------------------------------------
# 6. the masked references of the post-filter's tail: the padded batch (NaN behind every length) == every utterance alone
# ----------------------------------------------------------------------------------------------------------------------
B_, T_, LENS = 3, 24, [24, 13, 5]
F_, LD, LIN = 7, 16, 12
REL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(got).all(), f"{what}: padding reached the result"
    err = np.abs(got - want).max(initial=0.0)
    assert err <= REL * max(np.abs(want).max(initial=0.0), 1e-300), f"{what}: {err:.3e}"


def _padded(rng, shape_of, time_axis=1):
    """per-utterance random arrays (made first, each on its own) and the padded batch with NaN behind every length"""
    alone = [rng.standard_normal(shape_of(n)) for n in LENS]
    full = np.full((B_,) + shape_of(T_), np.nan)
    for b, (a, n) in enumerate(zip(alone, LENS)):
        idx = [b] + [slice(None)] * (time_axis - 1) + [slice(0, n)]
        full[tuple(idx)] = a
    return alone, full


def test_masked_pack_reference():
    rng = np.random.default_rng(11)
    ins, inpt = _padded(rng, lambda n: (2, n, F_), 2)
    ps, pre_x = _padded(rng, lambda n: (2, n, F_), 2)
    outs = bref.gag_pack([B_, T_, F_, LD], dict(inpt=inpt, pre_x=pre_x), LENS)
    for b, n in enumerate(LENS):
        want, _ = tref.run_ref("GAG_PACK", [1, n, F_, LD], [], dict(inpt=ins[b][None], pre_x=ps[b][None]))
        for k in ("enc_in", "pre"):
            _close(outs[k].val[b, :n], want[k][0][0], k)
            assert outs[k].must[b, :n].all() and not outs[k].must[b, n:].any()


@pytest.mark.parametrize("act", [prg.ACT_SIGMOID, prg.ACT_TANH, prg.ACT_RELU])
def test_masked_crm_references(act):
    rng = np.random.default_rng(12 + act)
    ps, pre = _padded(rng, lambda n: (n, LD))
    gs, g = _padded(rng, lambda n: (n, LIN))
    rs, r = _padded(rng, lambda n: (n, LIN))
    is_, im = _padded(rng, lambda n: (n, LIN))
    outs = bref.gag_crm([B_, T_, F_, LD, LIN, act], dict(pre=pre, g=g, r=r, i=im), LENS)
    for b, n in enumerate(LENS):
        want, _ = tref.run_ref("GAG_CRM", [1, n, F_, LD, LIN, act], [], dict(pre=ps[b][None], g=gs[b][None], r=rs[b][None], i=is_[b][None]))
        _close(outs["pre_out"].val[b, :n], want["pre_out"][0][0], "pre_out")
        _close(outs["planar"].val[b, :, :n], want["planar"][0][0], "planar")
        assert (outs["pre_out"].val[b, n:] == 0).all() and (outs["pre_out"].lim[b, n:] == 0).all() and outs["pre_out"].must[b, n:].all()
        assert (outs["planar"].val[b, :, n:] == 0).all() and (outs["planar"].lim[b, :, n:] == 0).all()
    # backward: both gradients and the accumulate operand; then each gradient alone, without dpre
    ds, dplanar = _padded(rng, lambda n: (2, n, F_), 2)
    qs, dpre_out = _padded(rng, lambda n: (n, LD))
    as_, acc = _padded(rng, lambda n: (n, LD))
    for use_pl, use_po, use_acc, want_dpre in [(True, True, True, True), (True, False, False, True), (False, True, False, False)]:
        A = dict(pre=pre, g=g, dplanar=dplanar if use_pl else None, dpre_out=dpre_out if use_po else None, acc_in=acc if use_acc else None)
        if want_dpre:
            A["dpre"] = True
        outs = bref.gag_crm_bwd([B_, T_, F_, LD, LIN, act], A, LENS)
        assert ("dpre" in outs) == want_dpre
        for b, n in enumerate(LENS):
            Ab = dict(pre=ps[b][None], g=gs[b][None], dplanar=ds[b][None] if use_pl else None, dpre_out=qs[b][None] if use_po else None,
                      acc_in=as_[b][None] if use_acc else None)
            if want_dpre:
                Ab["dpre"] = True
            want, _ = tref.run_ref("GAG_CRM_BWD", [1, n, F_, LD, LIN, act], [], Ab)
            for k in outs:
                _close(outs[k].val[b, :n], want[k][0][0], k)
                assert outs[k].must[b, :n].all() and not outs[k].must[b, n:].any()
