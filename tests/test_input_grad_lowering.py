"""Input gradients, host side (no GPU): the switch and the refusal that stays, the lowering with input_grad=True -- every op of
the program without the switch in its place, the added ops pinned --, the `din` boundary and the lengths flags of the new ops,
and the float64 reference of OP_INPUT_GRAD (tests/input_grad_ref.py): against float64 autograd of the filter-and-sum's formula,
and inside the float64 walk of a whole program against float64 autograd through the oracle with respect to the input."""
import numpy as np
import pytest
import torch

import input_grad_ref as igr
import train_ref as tref
from eabnet_amd import _lib
from eabnet_amd import model as mdl
from eabnet_amd import program as prg
from eabnet_amd import runtime
from eabnet_amd import train as tr
from eabnet_amd.program import Geometry
from eabnet_amd.spec import NetConfig

CONFIGS = [dict(), dict(bf_type="cnn"), dict(topo_type="miso"), dict(intra_connect="add"), dict(is_u2=False),
           dict(norm_type="BN"), dict(norm_type="cLN"), dict(is_causal=False), dict(k1=(3, 3)), dict(M=1), dict(M=32)]
IDS = lambda d: "-".join(f"{k}={v}" for k, v in d.items()) or "default"      # noqa: E731
BASES = {"a": 1 << 20, "w": 1 << 30, "g": 1 << 32, "in": 1 << 34, "out": 1 << 35, "dout": 1 << 36, "in2": None, "din": 1 << 37}


@pytest.fixture(autouse=True)
def _new_op_in_the_reference_tables():
    """train_ref's tables know OP_INPUT_GRAD while a test of this file runs, and only then"""
    with igr.registered():
        yield


def _cfg(kw):
    return NetConfig(**{**dict(M=4, p=1, q=1), **kw})


def _added(op) -> bool:
    return op.name == "input_grad" or ".dgrad_in." in op.name


def _first_conv(cfg) -> str:
    return "en.meta_unet_list.0.in_conv" if cfg.is_u2 else "en.unet_list.0"


# ----------------------------------------------------------------------------------------------------------------------
# 1. the switch, and the refusal that stays
# ----------------------------------------------------------------------------------------------------------------------
def test_the_switch_defaults_to_off_and_the_refusal_names_it_after_the_pinned_text():
    net = mdl.EaBNet(M=2)
    assert net.input_grad is False and mdl.GaGNet(p=1, q=1, dilas=(1,)).input_grad is False
    msg = str(mdl._refuse_differentiable(net, *net._input_grad_refusal))
    assert "input requires grad" in msg and msg.index("input requires grad") < msg.index("input_grad = True")
    # the post-filter's refusal is what it was: joint two-stage input gradients are out of scope
    gag = mdl.GaGNet(p=1, q=1, dilas=(1,))
    assert not gag._has_input_grad and "input_grad" not in str(mdl._refuse_differentiable(gag, *gag._input_grad_refusal))
    assert "the reference detaches" in gag._input_grad_refusal[1]


def test_without_the_switch_the_lowering_has_no_input_gradient():
    prog = tr.lower_train(_cfg({}), 2, 12)
    assert not prog.input_grad and not any(_added(o) for o in prog.bwd)
    assert not any(getattr(r, "arena", None) == "din" for o in prog.bwd if isinstance(o, tr.GenOp) for r in o.p)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the lowering: the old program untouched, the added ops pinned
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CONFIGS, ids=IDS)
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_flag_on_is_flag_off_plus_the_added_ops(kw, precision):
    cfg = _cfg(kw)
    B, T = 2, 12
    off = tr.lower_train(cfg, B, T, 161, precision, input_grad=False)
    on = tr.lower_train(cfg, B, T, 161, precision, input_grad=True)
    assert on.input_grad and not off.input_grad
    kept = [o for o in on.bwd if not _added(o)]
    assert [o.name for o in on.fwd] == [o.name for o in off.fwd] and [o.name for o in kept] == [o.name for o in off.bwd]
    # the shared ops, encoded against the same bases, are the same bytes: kinds, operands (arena offsets), geometry, flags
    for a_ops, b_ops in ((on.fwd, off.fwd), (kept, off.bwd)):
        ea, eb = runtime.encode(a_ops, BASES), runtime.encode(b_ops, BASES)
        for k, (x, y) in enumerate(zip(ea, eb)):
            assert bytes(x) == bytes(y), f"{a_ops[k].name}: a shared op changed under input_grad"
    assert [o.lane for o in kept] == [o.lane for o in off.bwd] and on.sync == off.sync
    # the arenas only grow at their ends; the gradient arena and its inverse table do not change at all
    assert on.g_floats == off.g_floats and np.array_equal(on.inv, off.inv) and on.n_params == off.n_params
    assert on.w_floats > off.w_floats and np.array_equal(on.ia[:off.w_floats], off.ia)
    assert on.a_floats == off.a_floats + B * T * 161 * tr.MLP_LD

    # the added ops: the data-gradient launches of the one convolution that reads the input -- the existing dgrad path gives a
    # strided convolution one launch per input-column parity that has taps -- and ONE op that writes din
    added = [o for o in on.bwd if _added(o)]
    first = _first_conv(cfg)
    fwd_conv = next(o for o in on.fwd if o.name == first)
    fwd_geom = Geometry.strided(161, len(set(fwd_conv.dt)), len(set(fwd_conv.ioff)))      # (its kernel: the weight's own shape)
    assert (list(fwd_geom.dt), list(fwd_geom.ioff), fwd_geom.Fout) == (list(fwd_conv.dt), list(fwd_conv.ioff), fwd_conv.Fout)
    geoms = Geometry.adjoint(fwd_geom)
    assert len(geoms) == 2 and len(added) == len(geoms) + 1
    convs, ig = added[:-1], added[-1]
    assert [o.name for o in convs] == [f"{first}.dgrad_in.{k}" for k in range(len(geoms))]
    assert fwd_conv.src0 == prg.Ref("in") and [o.name for o in on.fwd if getattr(o, "src0", None) == prg.Ref("in")] == [first]
    dz = next(o for o in on.bwd if o.name == first + ".glu_bwd").p[2]
    tile = convs[0].dst
    assert tile.arena == "a" and tile.off == off.a_floats            # the [rows][64] scratch: the last region of the arena
    for o, g in zip(convs, geoms):
        assert o.kind == prg.OP_CONV and o.N == tr.MLP_LD and o.Cout == tr.MLP_LD and o.epi == prg.EPI_LINEAR
        assert o.src0 == dz and o.src1 is None and o.C0 == fwd_conv.N and o.dst == tile and o.aux is None and o.bias is None
        assert (o.Fin, o.Fout, o.No, o.ostride, o.ophase, o.istride) == (g.Fin, 161, g.No, g.ostride, g.ophase, g.istride)
        assert list(o.dt) == list(g.dt) and list(o.ioff) == list(g.ioff)
        assert o.precision == (prg.PREC_BF16 if precision == "bf16" else prg.PREC_F32)
    assert sorted(np.concatenate([np.arange(g.No) * g.ostride + g.ophase for g in geoms])) == list(range(161))
    assert ig.kind == tr.OP_INPUT_GRAD == prg.OP_INPUT_GRAD == 39
    bw = next(o for o in on.fwd if o.name == "filter_sum").p[0]
    assert ig.p == [prg.Ref("dout"), bw, tile, prg.Ref("din")] and ig.i == [B, T, 161, cfg.M, tr.MLP_LD]
    # it comes after everything that writes its operands and before the weight gradients (the leaves at the end)
    k_ig = on.bwd.index(ig)
    assert all(on.bwd.index(o) < k_ig for o in convs)
    assert all(o.kind == tr.OP_WGRAD for o in on.bwd[k_ig + 1:]) and on.bwd[k_ig - 1].kind != tr.OP_WGRAD


@pytest.mark.parametrize("kw", [dict(), dict(is_u2=False), dict(M=1), dict(M=32)], ids=IDS)
def test_the_padded_weight_image_has_zero_weights_in_the_pad_columns(kw):
    """the transposed weights of the first convolution, padded to one 64-column tile with index -1 (a zero weight), rows in
    memory-channel order m*2+ri: the first 2M rows are the unpadded data-gradient image the program already packs"""
    cfg = _cfg(kw)
    low = tr.TrainLowering(cfg, 2, 12, input_grad=True)
    prog = low.build()
    wkey = ("en.meta_unet_list.0.in_conv.0.conv.1" if cfg.is_u2 else "en.unet_list.0.0.conv.1")
    for op in [o for o in prog.bwd if ".dgrad_in." in o.name]:
        ref64, ref = low.w_index[f"{wkey}.wd64.{op.ophase}"], low.w_index[f"{wkey}.wd.0.{op.ophase}"]
        assert op.w == ref64
        img64 = prog.ia[ref64.off:ref64.off + tr.MLP_LD * op.Kpad].reshape(tr.MLP_LD, op.Kpad)
        img = prog.ia[ref.off:ref.off + 2 * cfg.M * op.Kpad].reshape(2 * cfg.M, op.Kpad)
        assert np.array_equal(img64[:2 * cfg.M], img) and (img64[2 * cfg.M:] == -1).all() and (img >= 0).any()
    # memory-channel order: row m*2+ri of the image holds the weights of the reference's input channel ri*M+m
    w_idx = low.idx(f"{wkey}.weight")                                   # (N, 2M, kt, kf) flat parameter indices
    op = next(o for o in prog.bwd if o.name.endswith(".dgrad_in.0"))
    ref64 = low.w_index[f"{wkey}.wd64.{op.ophase}"]
    img64 = prog.ia[ref64.off:ref64.off + tr.MLP_LD * op.Kpad].reshape(tr.MLP_LD, op.Kpad)
    for m in range(cfg.M):
        for ri in range(2):
            row = img64[2 * m + ri]
            assert set(row[row >= 0]) <= set(w_idx[:, ri * cfg.M + m].reshape(-1))


# ----------------------------------------------------------------------------------------------------------------------
# 3. the din boundary and the lengths flags
# ----------------------------------------------------------------------------------------------------------------------
def test_din_is_a_boundary_buffer_next_to_the_others():
    assert tr.TrainBound.BOUNDARY == ("in", "out", "dout", "in2", "din")
    on = tr.lower_train(_cfg({}), 2, 12, input_grad=True)
    arr = runtime.encode(on.bwd, BASES)
    k = next(k for k, o in enumerate(on.bwd) if o.kind == tr.OP_INPUT_GRAD)
    assert arr[k].kind == 39 and arr[k].p[3] == BASES["din"] and arr[k].p[0] == BASES["dout"]
    assert [arr[k].i[j] for j in range(5)] == [2, 12, 161, 4, 64] and not arr[k].win.lens
    with pytest.raises(TypeError):                                     # an unbound din cannot be encoded by accident
        runtime.encode(on.bwd, {**BASES, "din": None})


@pytest.mark.parametrize("bucket", [False, True], ids=["varlen", "bucket"])
def test_the_new_ops_carry_the_lengths(bucket):
    cfg = _cfg({})
    plain = tr.lower_train(cfg, 2, 12, input_grad=True)
    flagged = tr.lower_train(cfg, 2, 12, input_grad=True, varlen=not bucket, bucket=bucket)
    assert flagged.varlen and flagged.input_grad and flagged.bucket == bucket
    assert [o.name for o in flagged.bwd] == [o.name for o in plain.bwd]
    assert tr.OP_INPUT_GRAD in tr.VARLEN_KINDS
    lens = 1 << 40
    arr = runtime.encode(flagged.bwd, BASES, lens=lens)
    seen = 0
    for o, op in zip(arr, flagged.bwd):
        if _added(op):
            seen += 1
            assert hasattr(op, "win")
            assert (o.conv.win.lens if op.kind == prg.OP_CONV else o.win.lens) == lens, op.name
    assert seen == 3
    for kw in (dict(norm_type="BN"), dict(norm_type="cLN"), dict(is_causal=False)):      # the same limits as without the switch
        with pytest.raises(NotImplementedError):
            tr.lower_train(_cfg(kw), 2, 12, input_grad=True, varlen=True)


def test_the_flag_is_part_of_the_cache_key(monkeypatch):
    """forward_train keys its bound programs by the flag: the same shape with and without an input gradient are two programs,
    and a call whose input needs no gradient asks for the lowering without the switch"""
    seen = []

    class Stop(Exception):
        pass

    def lower(cfg, B, T, F, prec, **kw):
        seen.append(kw)
        raise Stop
    monkeypatch.setattr(_lib, "load", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    net = mdl.EaBNet(M=2, p=1, q=1)
    x = torch.zeros(1, 4, 161, 2, 2)
    for leaf in (None, x):
        with pytest.raises(Stop):
            tr.forward_train(net, (x,), lower, x_leaf=leaf)
    assert seen == [{}, {"input_grad": True}]


# ----------------------------------------------------------------------------------------------------------------------
# 4. the float64 reference of the new op
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 8])
def test_reference_matches_float64_autograd_of_the_filter_and_sum(M):
    """Y = sum_m W_m X_m (EaBNet.py:114-117) plus a second reader of X with a given gradient: dL/dX by float64 autograd"""
    g = torch.Generator().manual_seed(M)
    B, T, F, ld = 2, 5, 7, 64
    f64 = torch.float64
    w = torch.randn(B, T, F, M, 2, generator=g, dtype=f64)
    x = torch.randn(B, T, F, M, 2, generator=g, dtype=f64, requires_grad=True)
    dout = torch.randn(B, 2, T, F, generator=g, dtype=f64)
    dconv = torch.randn(B, T, F, ld, generator=g, dtype=f64)
    yr = (w[..., 0] * x[..., 0] - w[..., 1] * x[..., 1]).sum(-1)
    yi = (w[..., 0] * x[..., 1] + w[..., 1] * x[..., 0]).sum(-1)
    loss = (torch.stack([yr, yi], 1) * dout).sum() + (x.reshape(B, T, F, 2 * M) * dconv[..., :2 * M]).sum()
    loss.backward()
    bw = torch.full((B, T, F, ld), float("nan"), dtype=f64)            # columns >= 2M are never read
    bw[..., :2 * M] = w.reshape(B, T, F, 2 * M)
    A = dict(dout=dout.numpy(), bw=bw.numpy(), dconv=dconv.numpy(), din=True)
    res, _ = tref.run_ref(igr.FORM, [B, T, F, M, ld], [], A)
    val, lim = res["din"]
    assert np.abs(val - x.grad.numpy()).max() <= 1e-10 * np.abs(x.grad.numpy()).max()
    # the fp32 evaluation of the same formula stays inside the derived limit
    A32 = {k: (v if v is True else np.nan_to_num(v).astype(np.float32)) for k, v in A.items()}
    r64, _ = tref.run_ref(igr.FORM, [B, T, F, M, ld], [], A32)
    r32, _ = tref.run_ref(igr.FORM, [B, T, F, M, ld], [], A32, np.float32)
    assert (np.abs(r32["din"][0].astype(np.float64) - r64["din"][0]) <= r64["din"][1]).all()
    # lengths: exact zeros behind them, whatever the operands hold
    A["dout"] = A["dout"].copy()
    A["dout"][1, :, 2:] = np.nan
    masked, _ = igr.ref_input_grad([B, T, F, M, ld], [], A, tref._M(np.float64), lens=[5, 2])
    assert np.isfinite(masked["din"][0]).all() and (masked["din"][0][1, 2:] == 0).all() and (masked["din"][1][1, 2:] == 0).all()
    assert np.array_equal(masked["din"][0][0], val[0]) and np.array_equal(masked["din"][0][1, :2], val[1, :2])


def _walk64(case):
    """the float64 walk of DESIGN §5.2 with the references themselves: every op's float64 result feeds the next op"""
    prog = case.prog
    arena = {k: np.full(n, np.nan, np.float64) for k, n in tref.arena_sizes(case).items()}
    flat = case.flat.astype(np.float64)
    arena["w"][:] = np.where(prog.ia >= 0, flat[prog.ia], 0) + (np.where(prog.ib >= 0, flat[prog.ib], 0) if prog.ib is not None else 0)
    arena["g"][:] = 0
    for k in ("in", "dout"):
        arena[k][:] = case.boundary[k].reshape(-1)

    def fetch(a):
        assert a.dtype == "f32"
        return arena[a.ref.arena][a.ref.off:a.ref.off + a.words].reshape(a.shape)
    kinds = []
    for ops in (prog.fwd, prog.bwd):
        for op in ops:
            outs, _ = tref.evaluate(op, fetch)
            kinds.append(tref.kind_name(op))
            for n, o in outs.items():
                if op.kind not in (prg.OP_CONV, tr.OP_WGRAD) and tref.form_of(op) in tref.NOT_COMPARED.get(n, ()):
                    continue
                view = arena[o.ref.arena][o.ref.off:o.ref.off + o.val.size].reshape(o.shape)
                wr = o.must if op.kind == prg.OP_CONV else np.ones(o.shape, bool)
                view[wr] = np.asarray(o.val, np.float64)[wr]
    return arena, kinds


@pytest.mark.parametrize("name", ["eabnet-B2-T6", "plain-cnn-B2-T6"])
def test_float64_walk_of_the_program_gives_the_oracles_input_gradient(name):
    """The whole program lowered with input_grad, interpreted op by op in float64 (conv_ref for the padded data gradient,
    input_grad_ref for the new op): `din` is the gradient of sum(out * dout) with respect to the input by float64 autograd
    through the oracle.  The walk's references keep a few quantities as the device stores them (its forward output deviates
    from the oracle's by ~2e-7 of max on these cases), so the bar is 1e-5 of max|ref|, the bar of DESIGN §4.8 for a backward
    kernel; a missing term, a wrong channel order or a wrong tap of the added ops is an error of order 1."""
    from oracle import eabnet_oracle as orc
    case = igr.make_case(name)
    arena, kinds = _walk64(case)
    assert kinds.count(igr.FORM) == 1
    prog, net = case.prog, tref.CASES[name]["net"]
    P, o = {}, 0
    for k, shp in zip(prog.keys, prog.shapes):
        n = int(np.prod(shp)) if len(shp) else 1
        P[k] = torch.from_numpy(case.flat[o:o + n].astype(np.float64).reshape(shp))
        o += n
    x = torch.from_numpy(case.boundary["in"]).double().requires_grad_(True)
    y = orc.eabnet_forward(P, x, **{k: v for k, v in net.items() if k != "M"})
    (y * torch.from_numpy(case.boundary["dout"]).double()).sum().backward()
    want = x.grad.numpy()
    din = arena["din"].reshape(want.shape)
    assert np.isfinite(din).all()
    e_out = np.abs(arena["out"].reshape(y.shape) - y.detach().numpy()).max() / float(y.detach().abs().max())
    err = np.abs(din - want).max() / np.abs(want).max()
    print(f"{name}: out {e_out:.2e}, din {err:.2e} of max|ref|")
    assert e_out <= 1e-5 and err <= 1e-5
