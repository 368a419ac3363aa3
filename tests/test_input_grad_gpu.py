"""Input gradients on the device: eab_input_grad_f32 against its float64 reference, ``EaBNet.input_grad`` against
fp64 autograd through the oracle with respect to the input (the scheme of test_hip_parity._check_training_gradients: seeded
parameters, PReLU slopes of 1 for the smooth cases, the oracle's own fp32 autograd as the floor otherwise), per-utterance
lengths, bf16, and the chain from a wave leaf to a waveform loss."""
import ctypes as C

import numpy as np
import pytest
import torch

import input_grad_ref as igr
import paramgen
import train_ref as tref
import wave_ref
from util import rel_errs, torch_params

pytestmark = pytest.mark.gpu

OP_TOL = 1e-5          # a backward kernel against float64, relative to max|ref|
GRAD_TOL = 1e-4        # gradients of the training programs against fp64 autograd, relative to the tensor's largest entry
BF16_BOUND = 5e-2      # the project's stated l2 bound of the bf16 mode against fp32 (tests/test_hip_parity.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------------------------------
# the op
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize("M", [1, 3, 8, 9, 16, 32])
def test_input_grad_op_matches_its_float64_reference(dev, M, lengths):
    from eabnet_amd import _lib
    lib = _lib.load()
    B, T, F, ld = 2, 5, 7, 64
    rng = np.random.default_rng(100 + M)
    dout = rng.standard_normal((B, 2, T, F)).astype(np.float32)
    bw = rng.standard_normal((B, T, F, ld)).astype(np.float32)
    dconv = rng.standard_normal((B, T, F, ld)).astype(np.float32)
    lens = [5, 2] if lengths else None
    if lengths:                                    # NaN behind every length in all three operands
        for b, n in enumerate(lens):
            dout[b, :, n:] = np.nan
            bw[b, n:] = np.nan
            dconv[b, n:] = np.nan
    d_dout, d_bw, d_dconv = (torch.from_numpy(a).to(dev) for a in (dout, bw, dconv))
    din = torch.full((B, T, F, M, 2), float("nan"), device=dev)
    d_lens = torch.tensor(lens, dtype=torch.int32, device=dev) if lengths else None
    _lib.check(lib.eab_input_grad_f32(d_dout.data_ptr(), d_bw.data_ptr(), d_dconv.data_ptr(), din.data_ptr(), B, T, F, M, ld,
                                      d_lens.data_ptr() if lengths else None, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "eab_input_grad_f32")
    got = din.cpu().numpy()
    assert np.isfinite(got).all(), "an element was not stored, or padding leaked"
    A = dict(dout=np.nan_to_num(dout), bw=np.nan_to_num(bw), dconv=np.nan_to_num(dconv), din=True)
    want = igr.ref_input_grad([B, T, F, M, ld], [], A, tref._M(np.float64), lens=lens)[0]["din"][0]
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"M {M} lengths {lens}: {err:.3e} of max|ref|")
    assert err <= OP_TOL
    if lengths:
        assert (got[1, 2:] == 0).all() and np.abs(got[1, :2]).min() > 0


# ----------------------------------------------------------------------------------------------------------------------
# the network
# ----------------------------------------------------------------------------------------------------------------------
def _params(M, kw, smooth, seed=None):
    from eabnet_amd.spec import NetConfig, param_specs
    P = torch_params(M, (910 + M) if seed is None else seed, **kw)
    specs = param_specs(NetConfig(M=M, **kw))
    if smooth:
        for k, sp in specs.items():
            if sp.kind == "prelu":
                P[k] = torch.ones_like(P[k])
    return P, {k for k, sp in specs.items() if not sp.kind.startswith("bn_")}


def _loss_fns(label, frames, miso, dev):
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    if miso:                                        # (B, 2, T): the reference sums the masked spectrum over frequency
        lab = label.sum(-1)
        return (lambda y: ((y - lab.to(dev)) ** 2).mean()), (lambda y: ((y - lab.to(y.dtype)) ** 2).mean())
    return (lambda y: eabnet_amd.com_mag_mse_loss(y, label.to(dev), frames)), (lambda y: orc.com_mag_mse_loss(y, label.to(y.dtype), frames))


def _oracle(P, is_param, x, loss_fn, dtype, kw):
    """autograd through the oracle in `dtype`: loss, d loss / d x and d loss / d parameter, returned in fp64"""
    from oracle import eabnet_oracle as orc
    # (copies: .to() of the same dtype would mark the caller's own tensors as requiring grad)
    Pd = {k: (v.detach().clone().to(dtype).requires_grad_(True) if k in is_param else v.to(dtype)) for k, v in P.items()}
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    y = orc.eabnet_forward(Pd, xx, bn_train=kw.get("norm_type") == "BN", **kw)
    loss = loss_fn(y)
    loss.backward()
    return float(loss.detach()), xx.grad.double(), {k: Pd[k].grad.double() for k in is_param}


def _grad_errors(got, ref):
    """as tests/test_hip_parity._grad_errors: global l2-rel; per tensor max-abs error relative to its largest entry"""
    num = sum(float(((got[k] - ref[k]) ** 2).sum()) for k in ref)
    den = sum(float((ref[k] ** 2).sum()) for k in ref)
    gmax = max(float(v.abs().max()) for v in ref.values())
    per = {k: float((got[k] - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref if float(ref[k].abs().max()) > 1e-6 * gmax}
    return (num / den) ** 0.5, per


def _hip(dev, M, B, T, kw, P, x_leaf, loss_fn, *, use_graph=True, freeze=False, precision="f32", net=None):
    import eabnet_amd
    if net is None:
        net = eabnet_amd.EaBNet(M=M, **kw)
        net.load_state_dict(P, strict=True)
        net = net.to(dev).train()
        net.input_grad, net.use_graph, net.precision = True, use_graph, precision
        if freeze:
            net.requires_grad_(False)
    y = net(x_leaf)
    assert y.requires_grad and net.training_backend == "hip"
    assert all("input_grad" in k for k in net._train_bound), "the program lowered with input_grad did not serve the call"
    loss = loss_fn(y)
    loss.backward()
    return net, float(loss.detach())


def _case(M, B, T, kw):
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, 920))
    label = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 1, 921)[..., 0, :]).permute(0, 3, 1, 2).contiguous()
    return x, label, [T] * B


SMOOTH = [(4, 2, 30, (2, 2), {}), (9, 2, 24, (2, 2), {}), (1, 1, 17, (1, 1), {}), (16, 2, 19, (1, 2), {})] + \
         [(4, 2, 30, (2, 2), e) for e in (dict(bf_type="cnn"), dict(topo_type="miso"), dict(is_u2=False), dict(intra_connect="add"),
                                         dict(norm_type="BN"), dict(norm_type="cLN"), dict(is_causal=False), dict(k1=(3, 3)))]


@pytest.mark.parametrize("M,B,T,pq,extra", SMOOTH, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_input_gradient_of_the_smooth_network_vs_fp64_autograd(dev, M, B, T, pq, extra):
    kw = dict(p=pq[0], q=pq[1], **extra)
    P, is_param = _params(M, kw, smooth=True)
    x, label, frames = _case(M, B, T, kw)
    hip_loss, ref_loss = _loss_fns(label, frames, extra.get("topo_type") == "miso", dev)
    # M = 1: the 4-D one-microphone form (B, T, F, 2) is the leaf
    leaf = (x[..., 0, :] if M == 1 else x).to(dev).requires_grad_(True)
    net, loss = _hip(dev, M, B, T, kw, P, leaf, hip_loss)
    want_loss, want_x, want_p = _oracle(P, is_param, x, ref_loss, torch.float64, kw)
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)
    assert leaf.grad is not None and leaf.grad.shape == leaf.shape and leaf.grad.dtype == leaf.dtype
    got_x = leaf.grad.cpu().double().reshape(want_x.shape)
    assert torch.isfinite(got_x).all()
    ex = float((got_x - want_x).abs().max() / want_x.abs().max())
    total, per = _grad_errors({k: net.get_parameter(k).grad.cpu().double() for k in want_p}, want_p)
    print(f"M {M} B {B} T {T} {kw}: x.grad {ex:.2e} of max|ref|; parameter gradients l2-rel {total:.2e}, worst tensor {max(per.values()):.2e}")
    assert ex <= GRAD_TOL
    bad = sorted(((e, k) for k, e in per.items() if e > GRAD_TOL), reverse=True)
    assert total <= GRAD_TOL and not bad, f"parameter gradients: global l2-rel {total:.3e}; tensors over 1e-4: {bad[:8]}"


def test_input_gradient_with_random_slopes_within_four_times_the_fp32_floor(dev):
    """Random PReLU slopes: the reference's own fp32 autograd deviates from its fp64 autograd (derivative flips amplified through
    the norm chain), so the bound is 4 x that deviation on the same case, computed here; the HIP path is never its own yardstick."""
    M, B, T, kw = 4, 2, 30, dict(p=2, q=2)
    P, is_param = _params(M, kw, smooth=False)
    x, label, frames = _case(M, B, T, kw)
    hip_loss, ref_loss = _loss_fns(label, frames, False, dev)
    leaf = x.to(dev).requires_grad_(True)
    _hip(dev, M, B, T, kw, P, leaf, hip_loss)
    _, want_x, _ = _oracle(P, is_param, x, ref_loss, torch.float64, kw)
    _, x32, _ = _oracle(P, is_param, x, ref_loss, torch.float32, kw)
    floor = rel_errs(x32.numpy(), want_x.numpy())[1]
    got = rel_errs(leaf.grad.cpu().double().numpy(), want_x.numpy())[1]
    print(f"random slopes: x.grad l2-rel {got:.2e}; the oracle's fp32 autograd {floor:.2e}")
    assert got <= max(GRAD_TOL, 4.0 * floor)


def test_graph_replay_direct_launches_frozen_parameters_and_dtype(dev):
    M, B, T, kw = 4, 2, 30, dict(p=2, q=2)
    P, is_param = _params(M, kw, smooth=True)
    x, label, frames = _case(M, B, T, kw)
    hip_loss, ref_loss = _loss_fns(label, frames, False, dev)
    _, want_x, _ = _oracle(P, is_param, x, ref_loss, torch.float64, kw)
    _, want_half, _ = _oracle(P, is_param, 0.5 * x, ref_loss, torch.float64, kw)

    def err(leaf, want):
        return float((leaf.grad.cpu().double() - want).abs().max() / want.abs().max())
    # captured graphs: the first call captures and replays, the second replays on new data
    leaf = x.to(dev).requires_grad_(True)
    net, _ = _hip(dev, M, B, T, kw, P, leaf, hip_loss)
    assert next(iter(net._train_bound.values())).graphs is not None, "the graphs were not captured"
    leaf2 = (0.5 * x).to(dev).requires_grad_(True)
    _hip(dev, M, B, T, kw, P, leaf2, hip_loss, net=net)
    # direct launches
    leaf3 = x.to(dev).requires_grad_(True)
    net3, _ = _hip(dev, M, B, T, kw, P, leaf3, hip_loss, use_graph=False)
    assert next(iter(net3._train_bound.values())).graphs is None
    # all parameters frozen, a double input: the gradient arrives in the input's dtype
    leaf4 = x.double().to(dev).requires_grad_(True)
    net4, _ = _hip(dev, M, B, T, kw, P, leaf4, hip_loss, freeze=True)
    assert leaf4.grad.dtype == torch.float64 and all(p.grad is None for p in net4.parameters())
    errs = [err(leaf, want_x), err(leaf2, want_half), err(leaf3, want_x), err(leaf4, want_x)]
    print(f"x.grad vs fp64 autograd: graph {errs[0]:.2e}, replay {errs[1]:.2e}, direct {errs[2]:.2e}, frozen {errs[3]:.2e}")
    assert max(errs) <= GRAD_TOL
    # an input that needs no gradient runs the program without the switch, under its old key
    net(x.to(dev)).sum().backward()
    assert sum("input_grad" in k for k in net._train_bound) == 1 and len(net._train_bound) == 2
    # without the switch the refusal stands, and names the switch
    net.input_grad = False
    with pytest.raises(NotImplementedError, match="input requires grad.*input_grad = True"):
        net(x.to(dev).requires_grad_(True))


def test_two_forwards_then_one_backward_raise_the_overwritten_error(dev):
    M, B, T, kw = 4, 1, 12, dict(p=1, q=1)
    P, _ = _params(M, kw, smooth=True)
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=M, **kw)
    net.load_state_dict(P, strict=True)
    net = net.to(dev).train()
    net.input_grad = True
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, 920)).to(dev).requires_grad_(True)
    y1 = net(x)
    net(x)
    with pytest.raises(RuntimeError, match="overwritten"):
        y1.sum().backward()


# ----------------------------------------------------------------------------------------------------------------------
# lengths
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["varlen_training", "train_length_buckets"])
def test_input_gradient_under_per_utterance_lengths(dev, mode):
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    M, B, T, kw, lens = 4, 2, 30, dict(p=2, q=2), [30, 17]
    P, _ = _params(M, kw, smooth=True)
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, 920))
    G = torch.from_numpy(np.random.default_rng(922).standard_normal((B, 2, T, 161)).astype(np.float32))
    xn, Gn = x.clone(), G.clone()
    for b, n in enumerate(lens):                    # NaN in the padding of the input and of grad_output
        xn[b, n:] = float("nan")
        Gn[b, :, n:] = float("nan")
    net = eabnet_amd.EaBNet(M=M, **kw)
    net.load_state_dict(P, strict=True)
    net = net.to(dev).train()
    net.input_grad = True
    if mode == "varlen_training":
        net.varlen_training = True
    else:
        net.train_length_buckets = (64,)
    leaf = xn.to(dev).requires_grad_(True)
    y = net(leaf, lengths=lens)
    assert all("input_grad" in k for k in net._train_bound)
    y.backward(Gn.to(dev))
    got = leaf.grad.cpu().double()
    assert got.shape == x.shape and torch.isfinite(got).all()
    for b, n in enumerate(lens):
        assert (got[b, n:] == 0).all(), "the gradient behind a length is not exactly zero"
        Pd = {k: v.double() for k, v in P.items()}
        xb = x[b:b + 1, :n].double().requires_grad_(True)
        (orc.eabnet_forward(Pd, xb, **kw) * G[b:b + 1, :, :n].double()).sum().backward()
        e = float((got[b:b + 1, :n] - xb.grad).abs().max() / xb.grad.abs().max())
        print(f"{mode}: utterance {b} ({n} frames) x.grad {e:.2e} of max|ref|")
        assert e <= GRAD_TOL


# ----------------------------------------------------------------------------------------------------------------------
# bf16
# ----------------------------------------------------------------------------------------------------------------------
def test_bf16_input_gradient_within_the_stated_bound_of_fp32(dev):
    M, B, T, kw = 4, 2, 30, dict(p=2, q=2)
    P, _ = _params(M, kw, smooth=True)
    x, label, frames = _case(M, B, T, kw)
    hip_loss, _ = _loss_fns(label, frames, False, dev)
    a, b = x.to(dev).requires_grad_(True), x.to(dev).requires_grad_(True)
    _hip(dev, M, B, T, kw, P, a, hip_loss)
    _hip(dev, M, B, T, kw, P, b, hip_loss, precision="bf16")
    l2 = rel_errs(b.grad.cpu().numpy(), a.grad.cpu().numpy())[1]
    print(f"bf16 x.grad vs fp32 HIP: l2-rel {l2:.2e} (bound {BF16_BOUND:.0e})")
    assert torch.isfinite(b.grad).all() and l2 <= BF16_BOUND


# ----------------------------------------------------------------------------------------------------------------------
# wave to loss
# ----------------------------------------------------------------------------------------------------------------------
def _cpu_chain(P, wav, clean, window, kw, dtype):
    """wave leaf -> torch.stft -> X |X|^-1/2 -> oracle -> torch.istft -> negative SI-SDR (eps 1e-8), mean over the batch"""
    from oracle import eabnet_oracle as orc
    Bc, Mc, L = wav.shape
    w = wav.detach().clone().to(dtype).requires_grad_(True)
    win = window.to(dtype)
    X = torch.stft(w.reshape(Bc * Mc, L), 320, hop_length=160, win_length=320, window=win, center=True, pad_mode="reflect",
                   return_complex=True)
    s = torch.view_as_real(X * X.abs().pow(-0.5)).reshape(Bc, Mc, 161, -1, 2).permute(0, 3, 2, 1, 4)          # (B, T, F, M, 2)
    y = orc.eabnet_forward({k: v.to(dtype) for k, v in P.items()}, s, **kw)                                     # (B, 2, T, F)
    est = torch.istft(torch.complex(y[:, 0], y[:, 1]).transpose(1, 2), 320, hop_length=160, win_length=320, window=win)
    c = clean.to(dtype)[:, :est.shape[1]]
    es, ss, ee = (est * c).sum(1), (c * c).sum(1), (est * est).sum(1)
    tgt = es * es / ss
    loss = (-wave_ref.K * (torch.log(tgt + 1e-8) - torch.log(ee - tgt + 1e-8))).mean()
    loss.backward()
    return float(loss.detach()), w.grad.double()


def test_wave_leaf_to_waveform_loss(dev):
    """wav -> stft_compress -> net (input_grad) -> istft -> si_sdr_loss -> backward(): every stage on the device.  The chain
    passes through the compression at small |X|, so the bound is max(1e-4, 4 x the deviation of the same chain in fp32 on the
    CPU from float64), computed here."""
    import eabnet_amd
    M, B, T, kw = 4, 2, 12, dict(p=1, q=1)
    L = 160 * (T - 1)
    P, _ = _params(M, kw, smooth=True)
    g = torch.Generator().manual_seed(5)
    wav = 0.1 * torch.randn(B, M, L, generator=g)
    clean = 0.1 * torch.randn(B, L, generator=g)
    window = torch.hann_window(320)
    want_loss, want = _cpu_chain(P, wav, clean, window, kw, torch.float64)
    _, g32 = _cpu_chain(P, wav, clean, window, kw, torch.float32)
    floor = float((g32 - want).abs().max() / want.abs().max())
    net = eabnet_amd.EaBNet(M=M, **kw)
    net.load_state_dict(P, strict=True)
    net = net.to(dev).train()
    net.input_grad = True
    leaf = wav.to(dev).requires_grad_(True)
    spec = eabnet_amd.stft_compress(leaf, 320, 160, window)
    assert spec.shape == (B, T, 161, M, 2) and spec.requires_grad
    est = eabnet_amd.istft(net(spec), 320, 160, window)
    loss = eabnet_amd.si_sdr_loss(est, clean.to(dev), eps=1e-8)
    loss.backward()
    got = leaf.grad.cpu().double()
    assert torch.isfinite(got).all() and np.isfinite(float(loss.detach())) and np.isfinite(want_loss)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"wave to loss: wav.grad {err:.2e} of max|ref|; the fp32 chain on the CPU {floor:.2e} (bound {max(1e-4, 4 * floor):.2e})")
    assert err <= max(1e-4, 4.0 * floor)
