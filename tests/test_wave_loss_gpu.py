"""Training on the waveform on the MI355X: the ISTFT adjoint (csrc/istft.hip) and the SI-SDR loss (csrc/wave_loss.hip) against
the float64 restatements of tests/wave_ref.py, ``istft`` and ``si_sdr_loss`` under autograd, their chain against float64 torch on
the CPU, and the spectral + waveform loss through both networks' HIP training programs.

Bounds: 1e-5 of max |ref| on a gradient (the bar of DESIGN.md §4.8 for every backward kernel), 4.34e-4 dB = 10 log10(1 + 1e-4) on
a value (tests/test_score_gpu.py), util.TOL_HIP = 1e-4 of the global maximum on parameter gradients (the summation-order noise
of the weight gradient's float atomics)."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import paramgen
import wave_ref as W
from util import TOL_HIP, torch_params

pytestmark = pytest.mark.gpu

TOL_DB = 10.0 * np.log10(1.0 + TOL_HIP)
TOL_GRAD = 1e-5
ROW = 12544                                             # row width of the loss batch
LENGTHS = [(1, 5000), (4097, 4096), (12517, 12000)]     # (est, clean) samples: one sample, across a span, three spans and a tail


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _adjoint(dev, dwav, window, n_fft, hop, T, lens=None):
    """eab_istft_bwd_f32 on host arrays: dwav (B, hop (T-1)), window (n_fft,) already padded -> dspec (B, 2, T, F) on the device"""
    from eabnet_amd import _lib, model
    lib = _lib.load()
    B = dwav.shape[0]
    g = torch.from_numpy(np.ascontiguousarray(dwav, np.float32)).to(dev)
    w = torch.from_numpy(np.ascontiguousarray(window, np.float32)).to(dev)
    n = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    out = torch.full((B, 2, T, n_fft // 2 + 1), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(lib.eab_istft_bwd_f32(g.data_ptr(), w.data_ptr(), model._twiddle(n_fft, dev).data_ptr(), out.data_ptr(),
                                     None if n is None else n.data_ptr(), B, T, n_fft, hop,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "eab_istft_bwd_f32")
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ the ISTFT adjoint
@pytest.mark.parametrize("n_fft,hop,win,T,B", [(320, 160, 320, 2, 1), (320, 160, 320, 9, 2), (320, 100, 320, 17, 2),
                                               (256, 64, 200, 12, 1), (320, 40, 320, 20, 1)])
def test_istft_adjoint_vs_float64_restatement(dev, n_fft, hop, win, T, B):
    window = W.padded(W.window_for(n_fft, hop, win), n_fft).astype(np.float32)
    dwav = np.random.default_rng(100 + T).standard_normal((B, hop * (T - 1))).astype(np.float32)
    want = W.istft_bwd(dwav, window, n_fft, hop, T)
    got = _adjoint(dev, dwav, window, n_fft, hop, T)
    again = _adjoint(dev, dwav, window, n_fft, hop, T)
    rel = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"({n_fft},{hop},{win},{T},{B}): max |got - ref| / max |ref| = {rel:.2e} (bound {TOL_GRAD:.0e})")
    assert rel <= TOL_GRAD
    assert torch.equal(got, again), "two calls on the same input must give the same bits"
    assert (got[:, 1, :, 0] == 0).all() and (got[:, 1, :, -1] == 0).all()


def test_istft_adjoint_with_lengths(dev):
    n_fft, hop, T, lens = 320, 160, 12, [12, 5, 2]
    window = W.window_for(n_fft, hop, n_fft).astype(np.float32)
    dwav = np.random.default_rng(112).standard_normal((3, hop * (T - 1))).astype(np.float32)
    poisoned = dwav.copy()
    for b, n in enumerate(lens):
        poisoned[b, hop * (n - 1):] = np.nan                  # constants of the forward: never read
    got = _adjoint(dev, poisoned, window, n_fft, hop, T, lens)
    assert torch.isfinite(got).all()
    want = W.istft_bwd(dwav, window, n_fft, hop, T, lens)
    assert np.abs(got.cpu().numpy() - want).max() <= TOL_GRAD * np.abs(want).max()
    for b, n in enumerate(lens):
        assert (got[b, :, n:] == 0).all(), b
        alone = _adjoint(dev, dwav[b:b + 1, :hop * (n - 1)], window, n_fft, hop, n)
        assert torch.equal(alone[0], got[b, :, :n]), b


def test_istft_under_autograd_keeps_its_values_and_runs_the_adjoint(dev):
    import eabnet_amd
    n_fft, hop, win, T, B = 256, 64, 200, 12, 2
    window = torch.hann_window(win)
    x = torch.from_numpy(np.random.default_rng(120).standard_normal((B, 2, T, n_fft // 2 + 1)).astype(np.float32)).to(dev)
    dwav = np.random.default_rng(121).standard_normal((B, hop * (T - 1))).astype(np.float32)
    for lengths in (None, [12, 7]):
        plain = eabnet_amd.istft(x, n_fft, hop, window, lengths=lengths)
        leaf = x.clone().requires_grad_(True)
        wav = eabnet_amd.istft(leaf, n_fft, hop, window, lengths=lengths)
        assert wav.requires_grad and torch.equal(wav, plain)
        (g,) = torch.autograd.grad(wav, leaf, grad_outputs=torch.from_numpy(dwav).to(dev))
        want = _adjoint(dev, dwav, W.padded(window.numpy(), n_fft), n_fft, hop, T, lengths)
        assert g.dtype == leaf.dtype and torch.equal(g, want)
        with torch.no_grad():                                 # grad disabled: the plain path, no graph
            assert not eabnet_amd.istft(leaf, n_fft, hop, window, lengths=lengths).requires_grad
    # a device window: the NOLA verdict is cached under the caller's tensor, a second call makes no host copy of it
    from eabnet_amd import model
    wdev = window.to(dev)
    eabnet_amd.istft(x, n_fft, hop, wdev)
    keys = set(model._NOLA)
    assert torch.equal(eabnet_amd.istft(x, n_fft, hop, wdev), eabnet_amd.istft(x, n_fft, hop, window))
    assert set(model._NOLA) == keys
    wdev.zero_()                                              # in place: the version counter moves, the verdict is taken again
    with pytest.raises(RuntimeError, match="NOLA"):
        eabnet_amd.istft(x, n_fft, hop, wdev)


# ------------------------------------------------------------------ the SI-SDR loss
@pytest.fixture(scope="module")
def batch(dev):
    """the padded batch of the loss tests, built once: fp32 pairs, their float64 (loss, gradient) at eps = 1e-8 and 0, and the
    device rows with NaN past every length"""
    pairs = [W.make_pair(le, ls, 200 + k, onset=60.0 if le == 1 else None) for k, (le, ls) in enumerate(LENGTHS)]
    ref = {eps: [W.si_sdr_loss(e, s, eps) for e, s in pairs] for eps in (0.0, 1e-8)}
    for eps, rows in ref.items():
        for (loss, _), lens in zip(rows, LENGTHS):
            assert -5.0 <= -loss <= 20.0, f"the reference itself must be well conditioned: SI-SDR {-loss:.2f} dB at {lens}"
    est = torch.full((3, ROW), float("nan"))
    clean = torch.full((3, ROW), float("nan"))
    for b, (e, s) in enumerate(pairs):
        est[b, :len(e)], clean[b, :len(s)] = torch.from_numpy(e), torch.from_numpy(s)
    return {"pairs": pairs, "ref": ref, "est": est.to(dev), "clean": clean.to(dev), "lengths": [list(p) for p in LENGTHS]}


def _grad_scale(pair, wgrad, eps):
    """what a gradient's error is measured against: max |ref|.  The one-sample estimate is the exception: SI-SDR does not depend
    on the scale of the estimate, and a one-sample estimate has nothing but a scale, so its gradient a_b e_0 + c_b s_0 is
    analytically zero (at eps = 0) and the float64 reference holds only the rounding of that cancellation, ~1e-16 of either
    term.  No output can agree with rounding noise to 1e-5 of itself; there the scale is the size of the cancelling terms,
    |a_b e_0| with a_b = 2 k / (res + eps)."""
    e, s = (np.asarray(v, np.float64) for v in pair)
    if len(e) > 1:
        return np.abs(wgrad).max()
    res = e[0] ** 2 - (e[0] * s[0]) ** 2 / (s @ s)
    return abs(2.0 * W.K / (res + eps) * e[0])


def _loss_and_grad(est, clean, lengths, eps, reduction="none", weights=None):
    import eabnet_amd
    leaf = est.detach().requires_grad_(True)                 # (shares est's memory and strides: a view stays a view)
    loss = eabnet_amd.si_sdr_loss(leaf, clean, lengths=lengths, eps=eps, reduction=reduction)
    (g,) = torch.autograd.grad(loss, leaf, grad_outputs=weights if weights is not None else torch.ones_like(loss))
    return loss.detach(), g


@pytest.mark.parametrize("eps", [0.0, 1e-8])
def test_si_sdr_loss_values_and_gradients_vs_float64(dev, batch, eps):
    import eabnet_amd
    loss, grad = _loss_and_grad(batch["est"], batch["clean"], batch["lengths"], eps)
    assert loss.dtype == torch.float32 and loss.shape == (3,) and grad.shape == batch["est"].shape
    for b, ((want, wgrad), (le, ls)) in enumerate(zip(batch["ref"][eps], LENGTHS)):
        err = abs(float(loss[b]) - want)
        gerr = np.abs(grad[b, :le].cpu().numpy() - wgrad).max() / _grad_scale(batch["pairs"][b], wgrad, eps)
        print(f"eps {eps:g}, lengths {(le, ls)}: loss {float(loss[b]):.5f} dB |diff| {err:.2e} (bound {TOL_DB:.2e}); "
              f"gradient {gerr:.2e} (bound {TOL_GRAD:.0e})")
        assert err <= TOL_DB and gerr <= TOL_GRAD, (b, err, gerr)
        assert (grad[b, le:] == 0).all(), "the gradient is exactly zero past the estimate's length"
    if eps == 0.0:
        noisy = torch.nan_to_num(batch["clean"]) + 0.5 * torch.randn(3, ROW, generator=torch.Generator().manual_seed(5)).to(dev)
        cols = list(zip(*batch["lengths"]))
        ratios = eabnet_amd.energy_ratios(batch["est"], batch["clean"], noisy, lengths=(list(cols[0]), list(cols[1]), list(cols[1])))
        assert (loss.double() + ratios[:, 0]).abs().max() <= TOL_DB


def test_si_sdr_loss_rows_have_the_same_bits_alone_and_in_the_batch(dev, batch):
    loss, grad = _loss_and_grad(batch["est"], batch["clean"], batch["lengths"], 1e-8)
    for b in range(3):
        l1, g1 = _loss_and_grad(batch["est"][b:b + 1], batch["clean"][b:b + 1], [batch["lengths"][b]], 1e-8)
        assert torch.equal(l1[0], loss[b]) and torch.equal(g1[0], grad[b]), b
    # a device (B, 2) tensor of lengths, (B, 1, Ls) clean rows and rows that are views of a wider, unaligned buffer: the same bits
    wide = torch.full((3, ROW + 7), float("nan"), device=dev)
    wide[:, 3:3 + ROW] = batch["est"]
    l2, g2 = _loss_and_grad(wide[:, 3:3 + ROW], batch["clean"][:, None], torch.tensor(batch["lengths"], device=dev), 1e-8)
    assert torch.equal(l2, loss) and torch.equal(g2, grad)


def test_si_sdr_loss_reductions_and_grad_output_weights(dev, batch):
    args = (batch["est"], batch["clean"], batch["lengths"], 1e-8)
    none, g_none = _loss_and_grad(*args)
    total, g_sum = _loss_and_grad(*args, reduction="sum")
    mean, g_mean = _loss_and_grad(*args, reduction="mean")
    assert total.shape == () and mean.shape == () and total.dtype == torch.float32
    scale = float(none.abs().sum())
    assert abs(float(total) - float(none.double().sum())) <= 1e-6 * scale
    assert abs(float(mean) - float(none.double().sum()) / 3) <= 1e-6 * scale
    assert torch.equal(g_sum, g_none)
    assert (g_mean - g_none / 3).abs().max() <= 1e-6 * g_none.abs().max()
    weights = torch.tensor([0.5, -2.0, 3.0], device=dev)
    _, g_w = _loss_and_grad(*args, weights=weights)
    for b, ((_, wgrad), (le, _)) in enumerate(zip(batch["ref"][1e-8], LENGTHS)):
        w = float(weights[b])
        assert np.abs(g_w[b, :le].cpu().numpy() - w * wgrad).max() <= TOL_GRAD * abs(w) * _grad_scale(batch["pairs"][b], wgrad, 1e-8), b
    # a weight that reaches the node through later arithmetic, as in `spectral + 0.3 * si_sdr_loss(...)`
    import eabnet_amd
    leaf = batch["est"].clone().requires_grad_(True)
    (0.3 * eabnet_amd.si_sdr_loss(leaf, batch["clean"], lengths=batch["lengths"], eps=1e-8)).backward()
    assert (leaf.grad - 0.3 * g_mean).abs().max() <= 1e-6 * g_mean.abs().max()


# ------------------------------------------------------------------ the chain
def test_gradient_of_the_chain_vs_float64_torch(dev):
    import eabnet_amd
    B, T, n_fft, hop = 2, 12, 320, 160
    rng = np.random.default_rng(300)
    out = rng.standard_normal((B, 2, T, n_fft // 2 + 1)).astype(np.float32)
    window = torch.hann_window(n_fft)

    def chain64(x, clean):
        wav = torch.istft(torch.view_as_complex(x.permute(0, 3, 2, 1).contiguous()), n_fft, hop, n_fft, window.double())
        es, ss, ee = (wav * clean).sum(1), (clean * clean).sum(1), (wav * wav).sum(1)
        tgt = es * es / ss
        return (-10.0 * (torch.log10(tgt + 1e-8) - torch.log10(ee - tgt + 1e-8))).mean()

    x64 = torch.from_numpy(out).double().requires_grad_(True)
    with torch.no_grad():
        wav64 = torch.istft(torch.view_as_complex(x64.permute(0, 3, 2, 1).contiguous()), n_fft, hop, n_fft, window.double())
    clean = (0.8 * wav64 + 0.3 * wav64.std() * torch.from_numpy(rng.standard_normal(tuple(wav64.shape)))).float()
    ref_loss = chain64(x64, clean.double())
    (want,) = torch.autograd.grad(ref_loss, x64)
    ref_loss = ref_loss.detach()
    assert -5.0 <= -float(ref_loss) <= 20.0
    leaf = torch.from_numpy(out).to(dev).requires_grad_(True)
    loss = eabnet_amd.si_sdr_loss(eabnet_amd.istft(leaf, n_fft, hop, window), clean.to(dev), eps=1e-8)
    loss.backward()
    rel = float((leaf.grad.cpu().double() - want).abs().max() / want.abs().max())
    print(f"chain: loss {float(loss):.5f} (float64 {float(ref_loss):.5f}), gradient max |diff| / max |ref| = {rel:.2e} (bound {TOL_GRAD:.0e})")
    assert abs(float(loss) - float(ref_loss)) <= TOL_DB and rel <= TOL_GRAD


# ------------------------------------------------------------------ through the networks
def _two_stage_args():
    return argparse.Namespace(
        k1=(2, 3), k2=(1, 3), c=64, M=2, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=1, q=1, is_causal=True, is_u2=True,
        bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="IN", ref_mic=0, freeze_eabnet=False,
        gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=1,
        gagnet_q=1, gagnet_dilas=[1], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=True,
        gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="IN")


@pytest.mark.parametrize("kind", ["eabnet", "two_stage"])
def test_spectral_plus_waveform_loss_trains_the_network(dev, kind):
    """one backward() of spectral + 0.05 * waveform loss gives every parameter the gradient that the training program's own
    backward gives for d = d loss / d out, taken on detached copies of the outputs"""
    import eabnet_amd
    B, T, M, hop = 2, 12, 2, 160
    window = torch.hann_window(320)
    if kind == "eabnet":
        net = eabnet_amd.EaBNet(M=M, p=1, q=1)
        net.load_state_dict(torch_params(M, 410, p=1, q=1), strict=True)
    else:
        torch.manual_seed(4)
        net = eabnet_amd.make_eabnet_with_postnet(_two_stage_args())
    net = net.to(dev).train()
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, 411)).to(dev)
    target = torch.from_numpy(paramgen.make_wave(B, 1, hop * (T - 1), 412)).to(dev)          # (B, 1, L), as the loader yields it
    label = eabnet_amd.stft_compress(target, 320, hop, window, 1)
    frames = [T] * B

    def total(out):
        if kind == "eabnet":
            spectral, final = eabnet_amd.com_mag_mse_loss(out, label, frames), out
        else:
            spectral, final = eabnet_amd.eabnet_with_postnet_loss(out, label, frames)["final"], out["esti_stft"]
        return spectral + 0.05 * eabnet_amd.si_sdr_loss(eabnet_amd.istft(final, 320, hop, window), target, eps=1e-8)

    def leaves(out):
        return [out] if kind == "eabnet" else [out["esti0_stft"], *out["esti1_stft_list"]]

    params = [p for p in net.parameters() if p.requires_grad]
    loss = total(net(x))
    loss.backward()
    assert all(p.grad is not None for p in params)
    got = [p.grad.detach().clone() for p in params]
    assert torch.isfinite(loss) and all(torch.isfinite(g).all() for g in got)
    norm = float(torch.sqrt(sum(g.double().square().sum() for g in got)))
    assert norm > 0.0

    out = net(x)
    held = [t.detach().requires_grad_(True) for t in leaves(out)]
    copy = held[0] if kind == "eabnet" else {"esti0_stft": held[0], "esti1_stft_list": held[1:],
                                             "esti_stft": held[-1].permute(0, 1, 3, 2)}
    d = torch.autograd.grad(total(copy), held)
    want = torch.autograd.grad(leaves(out), params, grad_outputs=d)
    top = max(float(w.abs().max()) for w in want)
    worst = max(float((g - w).abs().max()) for g, w in zip(got, want))
    print(f"{kind}: loss {float(loss):.5f}, gradient norm {norm:.3e}, max |diff| / global max = {worst / top:.2e} (bound {TOL_HIP:.0e})")
    assert worst <= TOL_HIP * top
    # the waveform term reaches the parameters: without it the gradient is another one
    assert any(float(w.abs().max()) > 0 for w in d)
