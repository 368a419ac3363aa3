"""Linear-domain waves on the MI355X: ``istft(decompress=True)`` (eab_istft_lin_f32) and its adjoint (eab_istft_lin_bwd_f32) against
the float64 restatements of tests/istft_lin_ref.py, the per-utterance lengths, ``istft`` under autograd, the round trip through the
compressing front end, ``Enhancer`` / ``Scorer`` / ``StreamingEnhancer`` with the switch against their per-file chains, and the
gradient of the chain with ``si_sdr_loss`` against float64 torch.

Bounds: 1e-5 of max |ref| on a wave (the bar of test_istft_other_hops_and_windows_vs_torch) and on a gradient (the bar of DESIGN.md
§4.8 for every backward kernel) -- fp32 torch doing the same composition sits at 1.5e-7 .. 2.4e-7 on these inputs; util.TOL_HIP =
1e-4 of max |w| on the round trip (the front end's parity bar; fp32 torch: 2.5e-7); 4.34e-4 dB = 10 log10(1 + 1e-4) on a loss value."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import istft_lin_ref as R
import paramgen
import wave_ref as W
from util import TOL_HIP, torch_params

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_DB = 10.0 * np.log10(1.0 + TOL_HIP)
LENS_T, LENS = 12, [12, 5, 2]                               # the lengths case: 320/160, two workgroups of the adjoint per utterance


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _window(n_fft, hop, win):
    return torch.from_numpy(W.window_for(n_fft, hop, win)).float()


def _adjoint(dev, dwav, spec, window, n_fft, hop, lens=None):
    """eab_istft_lin_bwd_f32 on host arrays: dwav (B, hop (T-1)), spec (B, 2, T, F), window (n_fft,) padded -> dspec on the device"""
    from eabnet_amd import _lib, model
    lib = _lib.load()
    B, _, T, _ = spec.shape
    g = torch.from_numpy(np.ascontiguousarray(dwav, np.float32)).to(dev)
    s = torch.from_numpy(np.ascontiguousarray(spec, np.float32)).to(dev)
    w = torch.from_numpy(np.ascontiguousarray(window, np.float32)).to(dev)
    n = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    out = torch.full((B, 2, T, n_fft // 2 + 1), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(lib.eab_istft_lin_bwd_f32(g.data_ptr(), s.data_ptr(), w.data_ptr(), model._twiddle(n_fft, dev).data_ptr(), out.data_ptr(),
                                         None if n is None else n.data_ptr(), B, T, n_fft, hop,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "eab_istft_lin_bwd_f32")
    torch.cuda.synchronize()
    return out


def _lens_case():
    """(spec, dwav, window) of the lengths case and their copies with NaN behind every length"""
    spec, dwav, window, _ = R.make_case(320, 160, 320, LENS_T, len(LENS), seed=3)
    ps, pd = spec.copy(), dwav.copy()
    for b, n in enumerate(LENS):
        ps[b, :, n:] = np.nan
        pd[b, 160 * (n - 1):] = np.nan
    return spec, dwav, window, ps, pd


# ------------------------------------------------------------------ the forward
@pytest.mark.parametrize("n_fft,hop,win,T,B", R.CASES)
def test_linear_istft_vs_float64_restatement(dev, n_fft, hop, win, T, B):
    import eabnet_amd
    spec, _, window, _ = R.make_case(n_fft, hop, win, T, B)
    want = R.istft(spec, window, n_fft, hop)
    x = torch.from_numpy(spec).to(dev)
    got = eabnet_amd.istft(x, n_fft, hop, _window(n_fft, hop, win), decompress=True)
    again = eabnet_amd.istft(x, n_fft, hop, _window(n_fft, hop, win), decompress=True)
    rel = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"({n_fft},{hop},{win},{T},{B}): max |got - ref| / max |ref| = {rel:.2e} (bound {TOL:.0e})")
    assert got.shape == (B, hop * (T - 1)) and got.dtype == torch.float32
    assert rel <= TOL
    assert torch.equal(got, again), "two calls on the same input must give the same bits"


def test_linear_istft_with_lengths(dev):
    import eabnet_amd
    spec, _, window, poisoned, _ = _lens_case()
    win = torch.from_numpy(window)
    got = eabnet_amd.istft(torch.from_numpy(poisoned).to(dev), 320, 160, win, lengths=LENS, decompress=True)
    assert torch.isfinite(got).all(), "a frame behind a length was read"
    want = R.istft(poisoned, window, 320, 160, LENS)
    assert np.abs(got.cpu().numpy() - want).max() <= TOL * np.abs(want).max()
    for b, n in enumerate(LENS):
        alone = eabnet_amd.istft(torch.from_numpy(spec[b:b + 1, :, :n]).to(dev), 320, 160, win, decompress=True)
        assert torch.equal(alone[0], got[b, :160 * (n - 1)]), f"utterance {b}: not the bits of the call on it alone"
        assert (got[b, 160 * (n - 1):] == 0).all(), f"utterance {b}: zeros must follow it"


# ------------------------------------------------------------------ the adjoint
@pytest.mark.parametrize("n_fft,hop,win,T,B", R.CASES)
def test_linear_adjoint_vs_float64_restatement(dev, n_fft, hop, win, T, B):
    spec, dwav, window, zero = R.make_case(n_fft, hop, win, T, B)
    want = R.istft_bwd(dwav, spec, window, n_fft, hop)
    got = _adjoint(dev, dwav, spec, window, n_fft, hop)
    again = _adjoint(dev, dwav, spec, window, n_fft, hop)
    rel = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"({n_fft},{hop},{win},{T},{B}): max |got - ref| / max |ref| = {rel:.2e} (bound {TOL:.0e})")
    assert rel <= TOL
    assert torch.equal(got, again), "two calls on the same input must give the same bits"
    b, t, f = zero
    assert (got[b, :, t, f] == 0).all(), "the gradient at a zero bin is exactly zero"
    assert (got[:, 1, :, 0] != 0).any() and (got[:, 1, :, -1] != 0).any(), "imaginary DC / Nyquist parts act through the modulus"


def test_linear_adjoint_with_lengths(dev):
    spec, dwav, window, ps, pd = _lens_case()
    got = _adjoint(dev, pd, ps, window, 320, 160, LENS)
    assert torch.isfinite(got).all(), "dwav or spec was read behind a length"
    want = R.istft_bwd(pd, ps, window, 320, 160, LENS)
    assert np.abs(got.cpu().numpy() - want).max() <= TOL * np.abs(want).max()
    for b, n in enumerate(LENS):
        assert (got[b, :, n:] == 0).all(), b
        alone = _adjoint(dev, dwav[b:b + 1, :160 * (n - 1)], spec[b:b + 1, :, :n], window, 320, 160)
        assert torch.equal(alone[0], got[b, :, :n]), f"utterance {b}: not the bits of the call on it alone"


# ------------------------------------------------------------------ istft under autograd
def test_istft_under_autograd_with_the_switch(dev):
    import eabnet_amd
    n_fft, hop, win, T, B = 256, 64, 200, 12, 2
    spec, dwav, _, _ = R.make_case(n_fft, hop, win, T, B, seed=5)
    window = torch.hann_window(win)
    padded = W.padded(window.numpy(), n_fft)                  # the very fp32 window ``istft`` pads and uploads
    x = torch.from_numpy(spec).to(dev)
    assert torch.equal(eabnet_amd.istft(x, n_fft, hop, window), eabnet_amd.istft(x, n_fft, hop, window, decompress=False))
    for lengths in (None, [12, 7]):
        plain = eabnet_amd.istft(x, n_fft, hop, window, lengths=lengths, decompress=True)
        leaf = x.clone().requires_grad_(True)
        wav = eabnet_amd.istft(leaf, n_fft, hop, window, lengths=lengths, decompress=True)
        assert wav.requires_grad and torch.equal(wav, plain), "the values under autograd are those of the no-grad call"
        (g,) = torch.autograd.grad(wav, leaf, grad_outputs=torch.from_numpy(dwav).to(dev))
        want = _adjoint(dev, dwav, spec, padded, n_fft, hop, lengths)
        assert g.dtype == leaf.dtype and torch.equal(g, want), "the gradient is the C-ABI call's, bit for bit"
        # the default under autograd is still the reference's node
        ref = x.clone().requires_grad_(True)
        assert torch.equal(eabnet_amd.istft(ref, n_fft, hop, window, lengths=lengths),
                           eabnet_amd.istft(x, n_fft, hop, window, lengths=lengths))
    half = x.half().requires_grad_(True)
    (gh,) = torch.autograd.grad(eabnet_amd.istft(half, n_fft, hop, window, decompress=True).sum(), half)
    assert gh.dtype == torch.float16, "the gradient has the input's dtype"
    # the fused launch against the unfused composition (two more passes over the spectrum)
    unfused = eabnet_amd.istft(x * x.norm(dim=1, keepdim=True), n_fft, hop, window)
    fused = eabnet_amd.istft(x, n_fft, hop, window, decompress=True)
    rel = float((fused - unfused).abs().max() / unfused.abs().max())
    print(f"fused vs istft(x * |x|): {rel:.2e} of max (bound {TOL:.0e})")
    assert rel <= TOL


# ------------------------------------------------------------------ the round trip
def test_round_trip_through_the_compressing_front_end(dev):
    import eabnet_amd
    L, hop = 2085, 160
    w = torch.from_numpy(np.random.default_rng(2085).standard_normal((1, 1, L)).astype(np.float32)).to(dev)
    win = torch.hann_window(320)
    spec = eabnet_amd.stft_compress(w, 320, hop, win, layout=1)
    T = spec.shape[2]
    assert T == 1 + L // hop
    want = w[0, :, :hop * (T - 1)]
    top = float(w.abs().max())
    back = eabnet_amd.istft(spec, 320, hop, win, decompress=True)
    err = float((back - want).abs().max()) / top
    ref_err = float((eabnet_amd.istft(spec, 320, hop, win) - want).abs().max()) / top
    print(f"round trip: {err:.2e} of max |w| with decompress (bound {TOL_HIP:.0e}), {ref_err:.2f} without (must exceed 0.1)")
    assert err <= TOL_HIP
    assert ref_err > 0.1, "the compressed-domain wave is not an estimate of the signal"


# ------------------------------------------------------------------ the tools
SAMPLES = [48000, 16000, 30123, 9999, 41000, 16007, 22222]      # the unequal files of tests/test_enhance_gpu.py


def _files(seed):
    """noisy (4, L_i) waves and clean (L_i,) waves that correlate with them, as tests/test_score_gpu.py makes them"""
    noisy = [torch.from_numpy(paramgen.make_wave(1, 4, n, seed + k))[0] for k, n in enumerate(SAMPLES)]
    clean = [torch.from_numpy(paramgen.make_wave(1, 1, n, seed + 50 + k))[0, 0] for k, n in enumerate(SAMPLES)]
    return noisy, [0.7 * x[0] + 0.3 * c for x, c in zip(noisy, clean)]


def _chain(model, waves, dev):
    """the one-at-a-time loop on the exact-shape path -> (linear-domain waves, the reference's waves) of the same estimates"""
    import eabnet_amd
    win = torch.hann_window(320)
    lin, ref = [], []
    with torch.no_grad():
        for w in waves:
            y = model(eabnet_amd.stft_compress(w[None].to(dev), 320, 160, win))
            lin.append(eabnet_amd.istft(y, 320, 160, win, decompress=True)[0])
            ref.append(eabnet_amd.istft(y, 320, 160, win)[0])
    return lin, ref


def test_enhancer_and_scorer_with_the_switch(dev, monkeypatch):
    """no statistic over time and the kernel choice pinned (as tests/test_enhance_gpu.py pins it), so the padded batches give
    the per-file chain's bits: with the switch every wave is the chain's with ``istft(decompress=True)``, without it nothing
    moved; the scorer's ``loss`` and ``si_sdr_mix`` keep their bits and its wave scores are those of the linear-domain waves"""
    import eabnet_amd
    monkeypatch.setenv("EAB_ST", "0")
    monkeypatch.setenv("EAB_BM", "64")
    net = eabnet_amd.EaBNet(M=4, norm_type="BN")
    net.load_state_dict(torch_params(4, 5, norm_type="BN"), strict=True)
    net = net.to(dev).eval()
    noisy, clean = _files(300)
    lin, ref = _chain(net, noisy, dev)
    got = eabnet_amd.Enhancer(net, max_batch=4, decompress=True)(noisy)
    default = eabnet_amd.Enhancer(net, max_batch=4)(noisy)
    for k in range(len(noisy)):
        assert torch.equal(got[k], lin[k]), f"file {k}: not the per-file chain with decompress=True"
        assert torch.equal(default[k], ref[k]), f"file {k}: the default output moved"
        assert not torch.equal(got[k], default[k])
    scorer = eabnet_amd.Scorer(net, max_batch=4, ref_mic=1, decompress=True)
    scores, waves = scorer(noisy, clean, return_waves=True)
    base = eabnet_amd.Scorer(net, max_batch=4, ref_mic=1)(noisy, clean)
    assert list(scores) == list(base) == ["si_sdr", "si_sir", "si_sar", "si_sdr_mix", "loss"]
    assert np.array_equal(scores["loss"], base["loss"]), "the loss is the compressed-spectrum loss, bit for bit"
    assert np.array_equal(scores["si_sdr_mix"], base["si_sdr_mix"])
    for k in range(len(noisy)):
        assert torch.equal(waves[k], lin[k]), f"file {k}: the scorer's wave is not the enhancer's"
        row = eabnet_amd.energy_ratios(waves[k][None], clean[k][None].to(dev), noisy[k][1][None].to(dev))[0].cpu().numpy()
        for j, m in enumerate(("si_sdr", "si_sir", "si_sar")):
            assert abs(row[j] - scores[m][k]) <= 1e-9, (k, m, row[j], scores[m][k])      # fp64 in a fixed order (test_score_gpu.py)
        assert scores["si_sdr"][k] != base["si_sdr"][k]
    print("si_sdr compressed-domain waves:", base["si_sdr"], "\nsi_sdr linear-domain waves:   ", scores["si_sdr"])


def _postnet_args(M):
    return argparse.Namespace(
        k1=(2, 3), k2=(1, 3), c=64, M=M, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=1, q=1, is_causal=True, is_u2=True,
        bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="BN", ref_mic=0, freeze_eabnet=False,
        gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=1,
        gagnet_q=1, gagnet_dilas=[1, 2], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=True,
        gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="BN")


@pytest.fixture(scope="module")
def streamed(dev):
    """the two-stage model, wave and offline linear-domain wave at the size of test_wave_to_wave_streaming_enhancer_bit_exact"""
    import eabnet_amd
    M, L = 4, 160 * 30
    net = eabnet_amd.make_eabnet_with_postnet(_postnet_args(M))
    specs = {**{"eabnet." + k: s for k, s in net.eabnet._specs.items()}, **{"postnet." + k: s for k, s in net.postnet._specs.items()}}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in paramgen.make_params(specs, 570).items()}, strict=True)
    net = net.to(dev).eval()
    wav = torch.from_numpy(paramgen.make_wave(2, M, L, 571)).to(dev)
    win = torch.hann_window(320)
    with torch.no_grad():
        off = eabnet_amd.istft(net(eabnet_amd.stft_compress(wav, 320, 160, win))["esti_stft"], 320, 160, win, decompress=True)
    return net, wav, off


@pytest.mark.parametrize("chunk", [1, 3])
def test_streaming_enhancer_with_the_switch_bit_exact(dev, streamed, chunk):
    import eabnet_amd
    net, wav, off = streamed
    L = wav.shape[2]
    enh = eabnet_amd.StreamingEnhancer(net, B=2, seconds=L / 16000, chunk=chunk, decompress=True)
    step = chunk * 160
    got = torch.cat([enh.push(wav[:, :, a:a + step], last=a + step >= L) for a in range(0, L, step)], dim=1)
    assert got.shape == off.shape == (2, L)
    assert torch.equal(got, off)


# ------------------------------------------------------------------ the chain
def test_gradient_of_the_linear_chain_vs_float64_torch(dev):
    import eabnet_amd
    B, T, n_fft, hop = 2, 12, 320, 160
    rng = np.random.default_rng(300)
    out = rng.standard_normal((B, 2, T, n_fft // 2 + 1)).astype(np.float32)
    window = torch.hann_window(n_fft)

    def wave64(x):
        y = x * x.norm(dim=1, keepdim=True)
        return torch.istft(torch.view_as_complex(y.permute(0, 3, 2, 1).contiguous()), n_fft, hop, n_fft, window.double())

    def chain64(x, clean):
        wav = wave64(x)
        es, ss, ee = (wav * clean).sum(1), (clean * clean).sum(1), (wav * wav).sum(1)
        tgt = es * es / ss
        return (-10.0 * (torch.log10(tgt + 1e-8) - torch.log10(ee - tgt + 1e-8))).mean()

    x64 = torch.from_numpy(out).double().requires_grad_(True)
    with torch.no_grad():
        wav64 = wave64(x64)
    clean = (0.8 * wav64 + 0.3 * wav64.std() * torch.from_numpy(rng.standard_normal(tuple(wav64.shape)))).float()
    ref_loss = chain64(x64, clean.double())
    (want,) = torch.autograd.grad(ref_loss, x64)
    ref_loss = ref_loss.detach()
    assert -5.0 <= -float(ref_loss) <= 20.0, "the reference itself must be well conditioned"
    leaf = torch.from_numpy(out).to(dev).requires_grad_(True)
    loss = eabnet_amd.si_sdr_loss(eabnet_amd.istft(leaf, n_fft, hop, window, decompress=True), clean.to(dev), eps=1e-8)
    loss.backward()
    loss = loss.detach()
    rel = float((leaf.grad.cpu().double() - want).abs().max() / want.abs().max())
    print(f"chain: loss {float(loss):.5f} (float64 {float(ref_loss):.5f}), gradient max |diff| / max |ref| = {rel:.2e} (bound {TOL:.0e})")
    assert abs(float(loss) - float(ref_loss)) <= TOL_DB and rel <= TOL
