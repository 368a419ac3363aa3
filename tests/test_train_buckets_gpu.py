"""Training length buckets on a real MI355X: `train_length_buckets` on EaBNet, GaGNet and the two-stage model.

(a), (b) the new entry points alone, through the C ABI: eab_gag_crm_bwd_lens_f32 against the masked float64 reference
    (tests/train_buckets_ref.py) with train_ref.check; eab_lstm64_train_fwd_lens_prec_f32 bit for bit against the launch without
    lengths at the valid steps, with sentinels surviving behind the longest length of a workgroup, and the reverse pass on its
    output (eab_lstm64_bwd_lens_f32 against ref_lstm_bwd per slice, eab_lstm64_bwd_bound_f32 against that launch).
(c)-(h) the networks under autograd through a cap wider than the call, against fp64 autograd through the oracle ONE UTTERANCE AT
    A TIME on its own frames (outputs zero-padded and concatenated under autograd, one loss), at the bars of
    tests/test_train_varlen_gpu.py: outputs 1e-5, loss 1e-5, gradients global l2-rel <= 1e-4 and no tensor over 1e-4.
All of (c)-(h) fail on a tree without the switch: GaGNet refuses lengths= under autograd and no call is served by a wider program."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import paramgen
import train_buckets_ref as bref
import train_ref as tref
import train_varlen_ref as vref
from eabnet_amd import program as prg
from eabnet_amd import train as tr
from test_train_varlen_gpu import _check_f32 as _check_eab, _grad_errors, _loss as _eab_loss, _reference as _eab_reference, _setup as _eab_setup
from util import assert_close, torch_params

pytestmark = pytest.mark.gpu

B, T, LENS = 3, 24, [24, 13, 5]
SENTINEL = 7.25


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
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")


def _lens(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda:0")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ----------------------------------------------------------------------------------------------------------------------
# (a) the CRM backward alone
# ----------------------------------------------------------------------------------------------------------------------
F_, LD, LIN = 161, 384, 192


def _crm_bwd(lib, h, act, lens):
    t = {k: _d(h.get(k)) for k in ("pre", "g", "dplanar", "dpre_out", "acc_in")}
    outs = {k: torch.full((B, T, LIN if k != "dpre" else LD), SENTINEL, device="cuda:0") for k in ("dg", "dr", "di", "dpre")}
    ld = _lens(lens)
    _ck(lib.eab_gag_crm_bwd_lens_f32(*(_ptr(t[k]) for k in ("pre", "g", "dplanar", "dpre_out", "acc_in")),
                                     *(outs[k].data_ptr() for k in ("dg", "dr", "di", "dpre")), B, T, F_, LD, LIN, act, _ptr(ld), _st()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


@pytest.mark.parametrize("act", [prg.ACT_SIGMOID, prg.ACT_TANH, prg.ACT_RELU], ids=["sigmoid", "tanh", "relu"])
def test_a_crm_backward_alone(lib, act):
    rng = np.random.default_rng(100 + act)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)                 # noqa: E731
    h = dict(pre=f32(B, T, LD), g=f32(B, T, LIN), dplanar=f32(B, 2, T, F_), dpre_out=f32(B, T, LD), acc_in=f32(B, T, LD))
    full, plain = _crm_bwd(lib, h, act, [T] * B), _crm_bwd(lib, h, act, None)
    old = {k: torch.full((B, T, LIN if k != "dpre" else LD), SENTINEL, device="cuda:0") for k in ("dg", "dr", "di", "dpre")}
    t = {k: _d(v) for k, v in h.items()}
    _ck(lib.eab_gag_crm_bwd_f32(*(t[k].data_ptr() for k in ("pre", "g", "dplanar", "dpre_out", "acc_in")),
                                *(old[k].data_ptr() for k in ("dg", "dr", "di", "dpre")), B, T, F_, LD, LIN, act, _st()))
    torch.cuda.synchronize()
    for k in full:
        assert np.array_equal(_bits(full[k]), _bits(plain[k])), f"{k}: full lengths != lens == NULL"
        assert np.array_equal(_bits(plain[k]), _bits(old[k].cpu().numpy())), f"{k}: the entry point without lengths changed"
    hp = {k: v.copy() for k, v in h.items()}
    for b, n in enumerate(LENS):                                               # NaN in every padding row of every input
        for k in ("pre", "g", "dpre_out", "acc_in"):
            hp[k][b, n:] = np.nan
        hp["dplanar"][b, :, n:] = np.nan
    got = _crm_bwd(lib, hp, act, LENS)
    o64, o32 = (bref.gag_crm_bwd([B, T, F_, LD, LIN, act], dict(hp, dpre=True), LENS, dt) for dt in (np.float64, np.float32))
    for k, o in o64.items():
        assert (got[k][~o.must] == np.float32(SENTINEL)).all(), f"{k}: a padding frame was written"
    worst, l2 = tref.check(o64, got, {k: o.val for k, o in o32.items()}, "gag_crm_bwd")
    print(f"MASKED gag_crm_bwd act={act} | err/limit {worst:.3f} | L2 ratio {'-' if l2 is None else format(l2, '.2f')}")


# ----------------------------------------------------------------------------------------------------------------------
# (b) the LSTM training forward alone, and the reverse pass on its output
# ----------------------------------------------------------------------------------------------------------------------
def _group(F, precision):
    """sequences per workgroup of the training forward (the dispatchers of csrc/lstm.hip and csrc/lstm_h3.hip)"""
    S = B * F
    return (4 if S <= 4096 else 16) if precision == prg.PREC_BF16 else (4 if S <= 2048 else 16)


def _t_hi(F, ns, lens):
    """per sequence s = b * F + f: the longest length among the utterances its workgroup of `ns` sequences touches"""
    S = B * F
    s = np.arange(S)
    lo, hi = (s // ns) * ns, np.minimum((s // ns) * ns + ns, S) - 1
    ln = np.asarray(lens)
    return np.array([ln[a // F:b // F + 1].max() for a, b in zip(lo, hi)])


@pytest.mark.parametrize("F", [161, 690])
@pytest.mark.parametrize("precision", [prg.PREC_F32, prg.PREC_BF16], ids=["f32", "bf16"])
def test_b_lstm_training_forward_alone_and_the_reverse_pass_on_it(lib, F, precision):
    rng = np.random.default_rng(200 + F + precision)
    S = B * F
    x = rng.standard_normal((B, T, F, 64)).astype(np.float32)
    wcat = (0.15 * rng.standard_normal((256, 128))).astype(np.float32)
    bias = (0.1 * rng.standard_normal(256)).astype(np.float32)
    wd, bd = _d(wcat), _d(bias)

    def fwd(xx, lens):
        xd, ld = _d(xx), _lens(lens)
        h = torch.full((B, T, F, 64), SENTINEL, device="cuda:0")
        g = torch.full((S, T, 5, 64), SENTINEL, device="cuda:0")
        _ck(lib.eab_lstm64_train_fwd_lens_prec_f32(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), h.data_ptr(), g.data_ptr(), _ptr(ld), B, T, F,
                                                   precision, _st()))
        torch.cuda.synchronize()
        return h.cpu().numpy(), g.cpu().numpy()
    h0, g0 = fwd(x, None)                                                       # finite padding, no lengths
    hf, gf = fwd(x, [T] * B)
    assert np.array_equal(_bits(hf), _bits(h0)) and np.array_equal(_bits(gf), _bits(g0)), "full lengths != lens == NULL"
    ho = torch.full((B, T, F, 64), SENTINEL, device="cuda:0")
    go = torch.full((S, T, 5, 64), SENTINEL, device="cuda:0")
    _ck(lib.eab_lstm64_train_fwd_prec_f32(_d(x).data_ptr(), wd.data_ptr(), bd.data_ptr(), ho.data_ptr(), go.data_ptr(), B, T, F, precision, _st()))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ho.cpu().numpy()), _bits(h0)) and np.array_equal(_bits(go.cpu().numpy()), _bits(g0))
    xp = x.copy()
    for b, n in enumerate(LENS):
        xp[b, n:] = np.nan
    h1, g1 = fwd(xp, LENS)
    top = _t_hi(F, _group(F, precision), LENS).reshape(B, F)
    assert (top < T).any() and (top > np.asarray(LENS)[:, None]).any(), "the case holds workgroups that stop early and ones that straddle"
    g1v, g0v = g1.reshape(B, F, T, 5, 64), g0.reshape(B, F, T, 5, 64)
    t = np.arange(T)
    valid = t[None, :, None] < np.asarray(LENS)[:, None, None]                              # (B, T, 1)
    behind = t[None, :, None] >= top[:, None, :]                                            # (B, T, F)
    vh = np.broadcast_to(valid[..., None], h1.shape)
    assert np.array_equal(_bits(h1)[vh], _bits(h0)[vh]), "h_out at valid steps: other bits than the launch without lengths"
    vg = np.broadcast_to(valid.transpose(0, 2, 1)[..., None, None], g1v.shape)
    assert np.array_equal(_bits(g1v)[vg], _bits(g0v)[vg]), "gates at valid steps: other bits than the launch without lengths"
    assert (h1[behind] == np.float32(SENTINEL)).all(), "h_out behind the workgroup's longest length was written"
    assert (g1v[behind.transpose(0, 2, 1)] == np.float32(SENTINEL)).all(), "gates behind the workgroup's longest length were written"
    # the reverse pass on that output: gates as the forward left them (NaN products or sentinels in the padding), NaN in dh's padding
    dh = rng.standard_normal((B, T, F, 64)).astype(np.float32)
    for b, n in enumerate(LENS):
        dh[b, n:] = np.nan
    gd, dd = _d(g1), _d(dh)
    ld = _lens(LENS)

    def bwd(bound, prec):
        out = torch.full((B, T, F, 256), SENTINEL, device="cuda:0")
        if bound is None:
            _ck(lib.eab_lstm64_bwd_lens_f32(gd.data_ptr(), dd.data_ptr(), wd.data_ptr(), out.data_ptr(), ld.data_ptr(), B, T, F, prec, _st()))
        else:
            _ck(lib.eab_lstm64_bwd_bound_f32(gd.data_ptr(), dd.data_ptr(), wd.data_ptr(), out.data_ptr(), ld.data_ptr(), bound, B, T, F, prec,
                                             _st()))
        torch.cuda.synchronize()
        return out.cpu().numpy()
    got = bwd(None, prg.PREC_F32)
    o64 = vref.lstm_bwd([B, T, F, prg.PREC_F32], dict(gates=g1, dh_out=dh, wcat=wcat), LENS)
    worst, _ = tref.check(o64, {"dgates": got}, None, f"lstm_bwd on the bounded forward F={F}")
    print(f"MASKED lstm fwd(lens) -> bwd F={F} prec={precision} | err/tol {worst:.3f}")
    # the bounded walk, in this precision's own form: bound == 0 is the launch above; bound != 0 gives its bits up to the longest length
    # of a workgroup of the backward (4 or 16 sequences, eab_lstm64_bwd_form) and leaves the rows behind alone
    form = lib.eab_lstm64_bwd_form(B, T, F, precision)
    lens_form, zero, one = bwd(None, precision), bwd(0, precision), bwd(1, precision)
    assert np.array_equal(_bits(zero), _bits(lens_form))
    btop = _t_hi(F, 4 if form == 0 else 16, LENS).reshape(B, F)
    bb = t[None, :, None] >= btop[:, None, :]
    assert (one[bb] == np.float32(SENTINEL)).all(), "dgates behind the workgroup's longest length were written"
    assert np.array_equal(_bits(one)[~bb], _bits(lens_form)[~bb]), "bounded walk: other bits than the full walk at the steps it runs"


# ----------------------------------------------------------------------------------------------------------------------
# (c), (d), (f) the post-filter
# ----------------------------------------------------------------------------------------------------------------------
GB, GT, CAP = 3, 26, 32
GLENS = (26, 15, 7)
# parameter / input seeds (2300, 2400..2402).  For acti_type="relu" they were checked on the CPU so that no gain pre-activation (the
# input of the ReLU of linear_g, both stages) lies within four times its own fp32 forward error (oracle in fp32 against fp64) of
# zero for any utterance ALONE at the lengths used: an fp32 forward may otherwise flip that bin's derivative.  Seeds (2300 + s,
# 2400 + s) were tried in order, s = 0 .. 7: all eight pass (closest pre-activation at 40, 23, 9, 49, 26, 26, 16 and 2.8 times the
# margin), so the first is used.
GSEED = 2300
GAG_KW = dict(p=1, q=2, dilas=[1, 2])
GAG_VARIANTS = {"default": {}, "squeezed": dict(is_squeezed=True), "tanh": dict(acti_type="tanh"), "relu": dict(acti_type="relu"),
                "unet": dict(is_u2=False), "add": dict(intra_connect="add")}


def _planar(Bq, Tq, seed):
    return torch.from_numpy(paramgen.make_spec_input(Bq, Tq, 161, 1, seed)[..., 0, :]).permute(0, 3, 1, 2).contiguous()


def _gag_params(kw, seed=GSEED):
    import eabnet_amd
    from eabnet_amd.spec import GagConfig
    cfg = GagConfig(**{**kw, "dilas": tuple(kw["dilas"])})
    specs = eabnet_amd.gag_param_specs(cfg)
    P = {k: torch.from_numpy(v) for k, v in paramgen.make_params(specs, seed).items()}
    for k, sp in specs.items():
        if sp.kind == "prelu":
            P[k] = torch.ones_like(P[k])                                       # smooth network
    return P


def _gag_setup(variant):
    kw = dict(GAG_KW, **GAG_VARIANTS[variant])
    inpt, pre_x = _planar(GB, GT, GSEED + 100), _planar(GB, GT, GSEED + 101)
    label = _planar(GB, GT, GSEED + 102).permute(0, 1, 3, 2).contiguous()      # (B, 2, F, T)
    return kw, _gag_params(kw), inpt, pre_x, label


@functools.lru_cache(maxsize=None)
def _gag_reference(variant, lens):
    """fp64 autograd through the oracle, one utterance at a time on its own frames; stage outputs zero-padded, concatenated, ONE
    stage-wise loss"""
    from oracle import eabnet_oracle as orc
    kw, P, inpt, pre_x, label = _gag_setup(variant)
    Pd = {k: v.double().requires_grad_(True) for k, v in P.items()}
    per = []
    for b, n in enumerate(lens):
        outs = orc.gagnet_forward(Pd, inpt[b:b + 1, :, :n].double(), pre_x[b:b + 1, :, :n].double(), kd1=3, **kw)      # q x (1, 2, F, n)
        per.append([torch.nn.functional.pad(o, (0, GT - n)) for o in outs])
    outs = [torch.cat([p_[j] for p_ in per], 0) for j in range(kw["q"])]
    loss = orc.stagewise_com_mag_mse_loss(outs, label.double(), list(lens))
    loss.backward()
    return [o.detach() for o in outs], float(loss.detach()), {k: v.grad.double() for k, v in Pd.items()}


def _gag_net(dev, variant, precision="f32"):
    import eabnet_amd
    kw, P, inpt, pre_x, label = _gag_setup(variant)
    net = eabnet_amd.GaGNet(**kw)
    net.load_state_dict(P, strict=True)
    net = net.to(dev).train()
    net.train_length_buckets = (CAP,)
    net.precision = precision
    return net, inpt.to(dev), pre_x.to(dev), label.to(dev)


def _bound(net):
    return next(reversed(net._train_bound.values()))


def _poison_taps(net, lens):
    """NaN into the rows behind every length -- the call's padding and the rows up to the cap -- of every tapped gradient tensor"""
    bound = _bound(net)
    prog = bound.prog
    assert prog.grad_taps
    for name, (r, Fv, Cv) in prog.grad_taps.items():
        n = prog.B * prog.T * Fv * Cv
        v = bound.acts[r.off:r.off + n].view(prog.B, prog.T, Fv * Cv)
        for b, nb in enumerate(lens):
            v[b, nb:] = float("nan")


def _gag_step(net, inpt, pre_x, label, lens, poison=False):
    import eabnet_amd
    for p in net.parameters():
        p.grad = None
    Tq = inpt.shape[2]
    outs = net(inpt, pre_x, lengths=lens)
    assert outs[0].requires_grad and net.training_backend == "hip" and tuple(outs[0].shape) == (inpt.shape[0], 2, 161, Tq)
    host = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
    loss = eabnet_amd.stagewise_com_mag_mse_loss(outs, label[..., :Tq].contiguous(), host)
    if poison:
        _poison_taps(net, host)
        gs = [g.clone() for g in torch.autograd.grad(loss, outs, retain_graph=True)]
        for g in gs:
            for b, n in enumerate(host):
                g[b, :, :, n:] = float("nan")
        torch.autograd.backward(outs, gs)
    else:
        loss.backward()
    return [o.detach() for o in outs], float(loss.detach()), {k: p.grad.detach().cpu().double() for k, p in net.named_parameters()}


def _check_gag(outs, loss, grads, ref, lens, what):
    routs, rloss, rg = ref
    for j, (o, r) in enumerate(zip(outs, routs)):
        for b, n in enumerate(lens):
            assert torch.equal(o[b, :, :, n:].cpu(), torch.zeros_like(o[b, :, :, n:]).cpu()), f"{what}: padding of stage {j} is exact zeros"
        assert torch.isfinite(o).all()
        m, l2 = assert_close(o.cpu().numpy(), r.numpy(), 1e-5, f"{what}: stage {j} vs per-utterance fp64")
        print(f"BUCKETS {what}: stage {j} max-rel {m:.2e}, l2-rel {l2:.2e}")
    assert abs(loss - rloss) <= 1e-5 * abs(rloss), (loss, rloss)
    got = {k: grads[k] for k in rg}
    assert all(torch.isfinite(g).all() for g in got.values()), f"{what}: a gradient is not finite"
    total, per = _grad_errors(got, rg)
    bad = sorted(((e, k) for k, e in per.items() if e > 1e-4), reverse=True)
    print(f"BUCKETS {what}: loss {loss:.6f} (fp64 {rloss:.6f}), gradients global l2-rel {total:.2e}, worst tensor {max(per.values()):.2e}")
    assert total <= 1e-4 and not bad, f"{what}: global l2-rel {total:.3e}; tensors over 1e-4: {bad[:8]}"


@pytest.mark.parametrize("lens", [(26, 15, 7), (7, 26, 15)])
def test_c_post_filter_through_a_cap_matches_one_utterance_at_a_time_fp64(dev, lens):
    net, inpt, pre_x, label = _gag_net(dev, "default")
    outs, loss, grads = _gag_step(net, inpt, pre_x, label, list(lens))
    assert _bound(net).prog.T == CAP and _bound(net).prog.bucket
    _check_gag(outs, loss, grads, _gag_reference("default", tuple(lens)), lens, f"post-filter lens {list(lens)}")


@pytest.mark.parametrize("variant", ["squeezed", "tanh", "relu", "unet", "add"])
def test_d_post_filter_variants(dev, variant):
    net, inpt, pre_x, label = _gag_net(dev, variant)
    outs, loss, grads = _gag_step(net, inpt, pre_x, label, list(GLENS))
    _check_gag(outs, loss, grads, _gag_reference(variant, GLENS), GLENS, f"post-filter {variant}")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_f_one_program_for_every_width_and_poison_stays_out(dev, precision):
    """Calls at T = 20, 26, 32 with different lengths on one module: one bound program, one pair of graphs.  The call at the cap with
    full lengths leaves valid gradients in every row; the next step, shorter, carries NaN in the padding of both inputs, of
    grad_output and of every tapped gradient tensor (up to the cap)."""
    net, inpt, pre_x, label = _gag_net(dev, "default", precision)
    wide = lambda t, ax: torch.cat([t, t.flip(ax)[(slice(None),) * ax + (slice(0, CAP - GT),)]], ax).contiguous()     # noqa: E731
    _gag_step(net, inpt[:, :, :20].contiguous(), pre_x[:, :, :20].contiguous(), label, [20, 9, 14])
    bound = _bound(net)
    graphs = bound.graphs
    assert graphs is not None and set(graphs) == {"fwd", "bwd"}
    _gag_step(net, wide(inpt, 2), wide(pre_x, 2), wide(label, 3), [CAP] * GB)
    ip, pp = inpt.clone(), pre_x.clone()
    for b, n in enumerate(GLENS):
        ip[b, :, n:] = float("nan")
        pp[b, :, n:] = float("nan")
    outs, loss, grads = _gag_step(net, ip, pp, label, list(GLENS), poison=True)
    assert len(net._train_bound) == 1 and _bound(net) is bound and bound.graphs is graphs, "one program and one pair of graphs"
    (key,) = net._train_bound
    assert key[1] == CAP and key[-1] is True and len(key) == 7, key           # the cap in place of T, and the bucket flag
    ref = _gag_reference("default", GLENS)
    if precision == "f32":
        _check_gag(outs, loss, grads, ref, GLENS, "post-filter, poisoned step after wider ones")
        return
    got = {k: grads[k] for k in ref[2]}
    assert all(torch.isfinite(o).all() for o in outs) and all(torch.isfinite(g).all() for g in got.values()), "NaN reached an output or a gradient"
    for o in outs:
        for b, n in enumerate(GLENS):
            assert torch.equal(o[b, :, :, n:].cpu(), torch.zeros_like(o[b, :, :, n:]).cpu())
    total, _ = _grad_errors(got, ref[2])
    gmax = max(float(v.abs().max()) for v in ref[2].values())
    cos = {k: float(torch.nn.functional.cosine_similarity(got[k].reshape(-1), ref[2][k].reshape(-1), dim=0))
           for k in ref[2] if float(ref[2][k].abs().max()) > 1e-3 * gmax}
    print(f"BUCKETS bf16 poisoned step: global l2-rel {total:.2e}, min cosine {min(cos.values()):.4f}")
    assert total <= 1e-1 and min(cos.values()) >= 0.99


# ----------------------------------------------------------------------------------------------------------------------
# (g) the beam-former through a cap
# ----------------------------------------------------------------------------------------------------------------------
NB, NT, NM = 3, 30, 4
NLENS = [30, 17, 9]


def _eab_net(dev, buckets=(CAP,)):
    import eabnet_amd
    kw, P, x, label = _eab_setup("default")
    net = eabnet_amd.EaBNet(M=NM, **kw)
    net.load_state_dict(P, strict=True)
    net = net.to(dev).train()
    net.train_length_buckets = buckets
    return net, x.to(dev), label.to(dev)


def _eab_step(net, x, label, lens, loss_lens=None):
    import eabnet_amd
    for p in net.parameters():
        p.grad = None
    y = net(x, lengths=lens)
    assert y.requires_grad and net.training_backend == "hip" and tuple(y.shape) == (x.shape[0], 2, x.shape[1], 161)
    host = loss_lens if loss_lens is not None else [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
    loss = _eab_loss(eabnet_amd.com_mag_mse_loss, y, label, host)
    loss.backward()
    return y.detach(), float(loss.detach()), {k: p.grad.detach().cpu().double() for k, p in net.named_parameters()}


def test_g_beam_former_through_a_cap(dev):
    net, x, label = _eab_net(dev)
    xp = x.clone()
    for b, n in enumerate(NLENS):
        xp[b, n:] = float("nan")
    y, loss, grads = _eab_step(net, xp, label, NLENS)
    bound = _bound(net)
    assert bound.prog.T == CAP and bound.prog.bucket and bound.graphs is not None
    flagged = [op for op in bound.prog.fwd if op.kind == tr.OP_LSTM_TRAIN]
    assert len(flagged) == 2 and all(hasattr(op, "win") for op in flagged)
    _check_eab(y, loss, grads, _eab_reference("default", tuple(NLENS)), NLENS, "beam-former, T = 30 in cap 32")
    # device-tensor lengths: the same program, the output's bits
    yd, lossd, _ = _eab_step(net, xp, label, torch.tensor(NLENS, device=dev))
    assert torch.equal(yd, y) and lossd == loss and _bound(net) is bound
    # lengths=None is lens = [T] * B: one program also serves equal-length batches of any width
    ya, _, ga = _eab_step(net, x, label, [NT] * NB)
    yb, _, _ = _eab_step(net, x, label, None, loss_lens=[NT] * NB)
    assert torch.equal(ya, yb) and len(net._train_bound) == 1 and _bound(net) is bound
    y20, _, _ = _eab_step(net, x[:, :20].contiguous(), label[:, :, :20].contiguous(), None, loss_lens=[20] * NB)
    assert tuple(y20.shape) == (NB, 2, 20, 161) and len(net._train_bound) == 1
    # a call wider than every cap runs at its exact width
    net.train_length_buckets = (16,)
    yw, _, _ = _eab_step(net, xp, label, NLENS)
    assert _bound(net).prog.T == NT and _bound(net).prog.bucket and len(net._train_bound) == 2
    assert_close(yw.cpu().numpy(), y.cpu().numpy(), 1e-5, "exact width vs cap 32")
    # direct launches
    net3, _, _ = _eab_net(dev)
    net3.use_graph = False
    yn, lossn, gn = _eab_step(net3, xp, label, NLENS)
    assert _bound(net3).graphs is None
    # (judged on its own against the per-utterance fp64 reference, at the bars of (c), and then against the captured graphs)
    _check_eab(yn, lossn, gn, _eab_reference("default", tuple(NLENS)), NLENS, "beam-former, T = 30 in cap 32, direct launches")
    assert_close(yn.cpu().numpy(), y.cpu().numpy(), 1e-5, "direct launches vs the captured graphs")
    assert abs(lossn - loss) <= 1e-5 * abs(loss)
    gmax = max(float(v.abs().max()) for v in grads.values())
    for k in grads:
        top = float(grads[k].abs().max())
        if top > 1e-6 * gmax:
            assert float((gn[k] - grads[k]).abs().max()) <= 1e-5 * top, k


# ----------------------------------------------------------------------------------------------------------------------
# (e), (h) the two-stage model
# ----------------------------------------------------------------------------------------------------------------------
def _two_stage_args(M, **over):
    import argparse
    d = dict(k1=(2, 3), k2=(1, 3), c=64, M=M, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=2, q=2, is_causal=True, is_u2=True,
             bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="IN", ref_mic=0, freeze_eabnet=False,
             gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=1,
             gagnet_q=2, gagnet_dilas=[1, 2], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=True,
             gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="IN")
    d.update(over)
    return argparse.Namespace(**d)


def test_e_two_stage_model_through_a_cap(dev):
    """M = 4, EaBNet p = q = 2 (the parameters, input and label of test_train_varlen_gpu's default case: its head's ReLU margins
    were checked for these lengths), post-filter as in (c), cap 32, T = 30, lens (30, 17, 9), eabnet_with_postnet_loss"""
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    lens = NLENS
    kw, Pe, x, label = _eab_setup("default")
    Pg = _gag_params(GAG_KW)
    two = eabnet_amd.EaBNetWithPostNet(_two_stage_args(NM))
    two.eabnet.load_state_dict(Pe, strict=True)
    two.postnet.load_state_dict(Pg, strict=True)
    two = two.to(dev).train()
    two.train_length_buckets = (CAP,)
    xp = x.clone()
    for b, n in enumerate(lens):
        xp[b, n:] = float("nan")
    out = two(xp.to(dev), lengths=lens)
    losses = eabnet_amd.eabnet_with_postnet_loss(out, label.to(dev), lens)
    losses["final"].backward()
    assert _bound(two.eabnet).prog.T == CAP and _bound(two.postnet).prog.T == CAP and _bound(two.postnet).prog.bucket
    # reference: the two-stage oracle on every utterance alone
    P = {**{f"eabnet.{k}": v for k, v in Pe.items()}, **{f"postnet.{k}": v for k, v in Pg.items()}}
    Pd = {k: v.double().requires_grad_(True) for k, v in P.items()}
    # (oracle.eabnet_postnet_forward feeds the post-filter the beam-former's estimate as it is; the reference model and the
    # package detach it, EaBNet.py:142, so the gradient graph is composed here from the same two oracle functions with the
    # detach, and its forward is asserted equal to eabnet_postnet_forward's)
    Pde = {k[len("eabnet."):]: v for k, v in Pd.items() if k.startswith("eabnet.")}
    Pdg = {k[len("postnet."):]: v for k, v in Pd.items() if k.startswith("postnet.")}
    e0, stages = [], []
    for b, n in enumerate(lens):
        xb = x[b:b + 1, :n].double()
        est = orc.eabnet_forward(Pde, xb, **kw)
        lst = orc.gagnet_forward(Pdg, xb[..., 0, :].permute(0, 3, 1, 2), est.detach(), kd1=3, **GAG_KW)
        with torch.no_grad():
            o = orc.eabnet_postnet_forward(Pd, xb, ref_mic=0, eab_kw=kw, gag_kw=dict(kd1=3, **GAG_KW))
        assert torch.equal(o["esti0_stft"], est.detach()) and all(torch.equal(a, c.detach()) for a, c in zip(o["esti1_stft_list"], lst))
        e0.append(torch.nn.functional.pad(est, (0, 0, 0, NT - n)))
        stages.append([torch.nn.functional.pad(s_, (0, NT - n)) for s_ in lst])
    ref_out = {"esti0_stft": torch.cat(e0, 0), "esti1_stft_list": [torch.cat([s[j] for s in stages], 0) for j in range(GAG_KW["q"])]}
    rl = orc.com_mag_mse_loss(ref_out["esti0_stft"], label.double(), lens) + orc.stagewise_com_mag_mse_loss(
        ref_out["esti1_stft_list"], label.double().permute(0, 1, 3, 2), lens)
    rl.backward()
    m, l2 = assert_close(out["esti0_stft"].detach().cpu().numpy(), ref_out["esti0_stft"].detach().numpy(), 1e-5, "esti0 vs per-utterance fp64")
    print(f"BUCKETS two-stage: esti0 max-rel {m:.2e}, l2-rel {l2:.2e}")
    for j, (a, r) in enumerate(zip(out["esti1_stft_list"], ref_out["esti1_stft_list"])):
        for b, n in enumerate(lens):
            assert torch.equal(a[b, :, :, n:].detach().cpu(), torch.zeros_like(a[b, :, :, n:]).cpu())
        m, l2 = assert_close(a.detach().cpu().numpy(), r.detach().numpy(), 1e-5, f"stage {j} vs per-utterance fp64")
        print(f"BUCKETS two-stage: stage {j} max-rel {m:.2e}, l2-rel {l2:.2e}")
    assert torch.equal(out["esti_stft"], out["esti1_stft_list"][-1].permute(0, 1, 3, 2))
    loss = float(losses["final"].detach())
    assert abs(loss - float(rl.detach())) <= 1e-5 * abs(float(rl.detach())), (loss, float(rl.detach()))
    rg = {k: v.grad.double() for k, v in Pd.items()}
    got = {k: two.get_parameter(k).grad.detach().cpu().double() for k in rg}
    assert all(torch.isfinite(g).all() for g in got.values())
    total, per = _grad_errors(got, rg)
    bad = sorted(((e, k) for k, e in per.items() if e > 1e-4), reverse=True)
    print(f"BUCKETS two-stage: loss {loss:.6f} (fp64 {float(rl.detach()):.6f}), gradients global l2-rel {total:.2e}, "
          f"worst tensor {max(per.values()):.2e}")
    assert total <= 1e-4 and not bad, f"global l2-rel {total:.3e}; tensors over 1e-4: {bad[:8]}"


def test_h_a_whole_two_stage_step_on_a_mixed_batch(dev):
    """two(x, lengths=frames) -> istft(lengths=frames) -> si_sdr_loss(lengths=samples) + eabnet_with_postnet_loss, backward, FlatAdam
    over both stages: the loss falls over five steps on one batch"""
    import eabnet_amd
    hop, n_fft = 160, 320
    Bq, Tq, M = 3, 20, 2
    frames = [20, 13, 8]
    samples = [hop * (n - 1) for n in frames]
    window = torch.hann_window(n_fft)
    two = eabnet_amd.EaBNetWithPostNet(_two_stage_args(M, p=1, q=1, gagnet_q=1, gagnet_dilas=[1]))
    two.eabnet.load_state_dict(torch_params(M, 1510, p=1, q=1), strict=True)
    two.postnet.load_state_dict(_gag_params(dict(p=1, q=1, dilas=[1]), 1513), strict=True)
    two = two.to(dev).train()
    two.train_length_buckets = "auto"
    x = torch.from_numpy(paramgen.make_spec_input(Bq, Tq, 161, M, 1511)).to(dev)
    target = torch.from_numpy(paramgen.make_wave(Bq, 1, hop * (Tq - 1), 1512)).to(dev)
    for b, n in enumerate(frames):
        x[b, n:] = float("nan")                            # what lies behind an utterance does not matter
    label = eabnet_amd.stft_compress(target, n_fft, hop, window, 1)
    opt = eabnet_amd.FlatAdam(two.parameters(), lr=1e-3)
    dl = torch.tensor(frames, device=dev)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        out = two(x, lengths=dl)
        wav = eabnet_amd.istft(out["esti_stft"], n_fft, hop, window, lengths=frames)
        loss = eabnet_amd.eabnet_with_postnet_loss(out, label, frames)["final"] + 0.05 * eabnet_amd.si_sdr_loss(
            wav, target[:, 0], lengths=samples, eps=1e-8)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert _bound(two.eabnet).prog.T == 64 and _bound(two.postnet).prog.T == 64 and len(two.postnet._train_bound) == 1
    print("BUCKETS whole two-stage step, loss per step:", [f"{v:.5f}" for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
