"""The adjoint of the STFT front end on the device (eab_stft_compress_bwd_f32) and ``stft_compress`` under
autograd.  The kernel is compared with the float64 restatement of its contract (tests/stft_bwd_ref.py, pinned to float64
torch autograd by tests/test_stft_bwd_ref.py) evaluated at the device's own stored output; the chain from a wave leaf, which
passes through the ill-conditioned compression at small |X|, is bounded by torch's own fp32 floor on the same inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import stft_bwd_ref as sref

pytestmark = pytest.mark.gpu

B, M = 2, 3
OP_TOL = 1e-5          # the bar of a backward kernel against float64, relative to max|ref|


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _inputs(n_fft, hop, win, layout, seed=0, silent=None):
    g = torch.Generator().manual_seed(seed)
    Mc = M if layout == 0 else 1
    L = 11 * hop + 37
    T, F = 1 + L // hop, n_fft // 2 + 1
    wav = 0.1 * torch.randn(B, Mc, L, generator=g)
    if silent is not None:
        wav[silent[0], silent[1]] = 0.0
    cot = torch.randn((B, T, F, Mc, 2) if layout == 0 else (B, 2, T, F), generator=g)
    window = torch.from_numpy(sref.padded_window(n_fft, win)).float()
    return wav, cot, window, L, T


def _bwd(dev, dspec, spec, window, lens, n_fft, hop, layout, shape):
    """one call of the C entry point on device tensors"""
    from eabnet_amd import _lib
    from eabnet_amd import model as mdl
    lib = _lib.load()
    Bc, Mc, L = shape
    dwav = torch.full(shape, float("nan"), device=dev)
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    _lib.check(lib.eab_stft_compress_bwd_f32(dspec.data_ptr(), spec.data_ptr(), window.data_ptr(), mdl._twiddle(n_fft, dev).data_ptr(),
                                             dwav.data_ptr(), None if lens_d is None else lens_d.data_ptr(), Bc, Mc, L, n_fft, hop,
                                             layout, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "eab_stft_compress_bwd_f32")
    torch.cuda.synchronize()
    return dwav


def _frame_mask(cot, lens, hop, layout):
    """True at the frames behind each utterance's last one"""
    mask = torch.zeros(cot.shape, dtype=torch.bool)
    for b, n in enumerate(lens):
        Tb = 1 + n // hop
        if layout == 0:
            mask[b, Tb:] = True
        else:
            mask[b, :, Tb:] = True
    return mask


@pytest.mark.parametrize("lengths", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n_fft,hop,win", sref.CASES)
def test_kernel_matches_the_float64_restatement_at_its_own_output(dev, n_fft, hop, win, layout, lengths):
    import eabnet_amd
    wav, cot, window, L, T = _inputs(n_fft, hop, win, layout)
    lens = [L, L - 3 * hop - 5] if lengths else None
    wd, win_d = wav.to(dev), window.to(dev)
    spec = eabnet_amd.stft_compress(wd, n_fft, hop, win_d, layout=layout, lengths=lens)
    dspec = cot.to(dev)
    if lengths:                                     # NaN behind every length in both operands: never read
        mask = _frame_mask(cot, lens, hop, layout).to(dev)
        spec = torch.where(mask, torch.full_like(spec, float("nan")), spec)
        dspec = torch.where(mask, torch.full_like(dspec, float("nan")), dspec)
    got = _bwd(dev, dspec, spec, win_d, lens, n_fft, hop, layout, tuple(wav.shape))
    again = _bwd(dev, dspec, spec, win_d, lens, n_fft, hop, layout, tuple(wav.shape))
    assert torch.equal(got, again), "two calls on the same operands differ in bits"
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    want = sref.stft_compress_bwd_ref(dspec.cpu().numpy(), spec.cpu().numpy(), window.numpy(), n_fft, hop, layout, L, lens)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"n_fft {n_fft} hop {hop} win {win} layout {layout} lengths {lens}: {err:.3e} of max|ref|")
    assert err <= OP_TOL
    if lengths:
        assert (got[1, :, lens[1]:] == 0).all()
        # the same bits alone: utterance 1 as a batch of one, at its own length in the same capacity
        alone = _bwd(dev, dspec[1:2].contiguous(), spec[1:2].contiguous(), win_d, lens[1:], n_fft, hop, layout, (1,) + tuple(wav.shape[1:]))
        assert np.array_equal(alone.cpu().numpy()[0], got[1]), "an utterance has other bits alone than in the batch"


def test_a_silent_microphone_gets_an_exact_zero_gradient(dev):
    import eabnet_amd
    n_fft, hop, win = sref.CASES[0]
    wav, cot, window, L, T = _inputs(n_fft, hop, win, 0, silent=(0, 1))
    spec = eabnet_amd.stft_compress(wav.to(dev), n_fft, hop, window.to(dev))
    assert (spec[0, :, :, 1] == 0).all()
    got = _bwd(dev, cot.to(dev), spec, window.to(dev), None, n_fft, hop, 0, tuple(wav.shape)).cpu().numpy()
    assert np.isfinite(got).all() and (got[0, 1] == 0).all()
    want = sref.stft_compress_bwd_ref(cot.numpy(), spec.cpu().numpy(), window.numpy(), n_fft, hop, 0, L)
    assert np.abs(got - want).max() <= OP_TOL * np.abs(want).max()
    # and through autograd: finite, zero on the silent channel
    w = wav.to(dev).requires_grad_(True)
    (eabnet_amd.stft_compress(w, n_fft, hop, window.to(dev)) * cot.to(dev)).sum().backward()
    assert torch.isfinite(w.grad).all() and (w.grad[0, 1] == 0).all() and torch.equal(w.grad.cpu(), torch.from_numpy(got))


def test_stft_compress_under_autograd_keeps_its_bits_and_the_waves_dtype(dev):
    import eabnet_amd
    n_fft, hop, win = sref.CASES[0]
    wav, cot, window, L, T = _inputs(n_fft, hop, win, 0)
    lens = [L, L - 3 * hop - 5]
    for kw in (dict(), dict(lengths=lens)):
        plain = eabnet_amd.stft_compress(wav.to(dev), n_fft, hop, window, **kw)
        w = wav.to(dev).requires_grad_(True)
        out = eabnet_amd.stft_compress(w, n_fft, hop, window, **kw)
        assert out.requires_grad and not plain.requires_grad and torch.equal(out.detach(), plain)
        (out * cot.to(dev)).sum().backward()
        assert w.grad.dtype == torch.float32 and w.grad.shape == w.shape and torch.isfinite(w.grad).all()
        if kw:
            assert (w.grad[1, :, lens[1]:] == 0).all()
        with torch.no_grad():
            assert not eabnet_amd.stft_compress(w, n_fft, hop, window, **kw).requires_grad
    for dt in (torch.float16, torch.float64):
        wh = wav.to(dev).to(dt).requires_grad_(True)
        out = eabnet_amd.stft_compress(wh, n_fft, hop, window, lengths=lens)
        (out * cot.to(dev)).sum().backward()
        assert wh.grad.dtype == dt and wh.grad.shape == wh.shape and torch.isfinite(wh.grad).all()
    # layout 1 (one microphone, planar) under autograd
    w1, c1, window1, _, _ = _inputs(n_fft, hop, win, 1)
    w1 = w1.to(dev).requires_grad_(True)
    out1 = eabnet_amd.stft_compress(w1, n_fft, hop, window1, layout=1)
    assert torch.equal(out1.detach(), eabnet_amd.stft_compress(w1.detach(), n_fft, hop, window1, layout=1))
    (out1 * c1.to(dev)).sum().backward()
    assert torch.isfinite(w1.grad).all() and float(w1.grad.abs().max()) > 0


def test_more_than_eight_overlapping_frames_are_refused_under_autograd(dev):
    import eabnet_amd
    w = torch.zeros(1, 1, 4000, device=dev).requires_grad_(True)
    window = torch.hann_window(320)
    with pytest.raises(NotImplementedError, match="at most 8"):
        eabnet_amd.stft_compress(w, 320, 32, window)
    assert eabnet_amd.stft_compress(w.detach(), 320, 32, window).shape == (1, 126, 161, 1, 2)      # the forward itself is served
    # a size the LDS FFT does not factor (n_fft / 2 = 14 = 2 * 7) and a hop beyond n_fft: refused where the call is made
    with pytest.raises(NotImplementedError, match="factors 2 and 5"):
        eabnet_amd.stft_compress(w, 28, 14, torch.hann_window(28))
    with pytest.raises(NotImplementedError, match="hop <= n_fft"):
        eabnet_amd.stft_compress(w, 320, 400, window)
    assert eabnet_amd.stft_compress(w.detach(), 28, 14, torch.hann_window(28)).shape == (1, 286, 15, 1, 2)


def _torch_chain(wav, window, n_fft, hop, cot, dtype):
    """torch autograd on the CPU in `dtype`: wave -> torch.stft -> X |X|^-1/2 -> sum(s * cot); the wave's gradient as float64"""
    w = wav.detach().clone().to(dtype).requires_grad_(True)          # (a copy: .to() of the same dtype would mark the caller's tensor)
    X = torch.stft(w.reshape(-1, w.shape[-1]), n_fft, hop_length=hop, win_length=n_fft, window=window.to(dtype), center=True,
                   pad_mode="reflect", return_complex=True)                    # (B M, F, T)
    s = torch.view_as_real(X * X.abs().pow(-0.5)).reshape(w.shape[0], w.shape[1], X.shape[1], X.shape[2], 2)
    (s.permute(0, 3, 2, 1, 4) * cot.to(dtype)).sum().backward()
    return w.grad.double().numpy()


@pytest.mark.parametrize("seed", [0, 1])
def test_wave_gradient_end_to_end_within_torchs_own_fp32_floor(dev, seed):
    """From the wave the map is ill-conditioned at small |X| (the compression's derivative grows like |X|^-1/2): fp32 torch
    autograd of the same composition deviates from float64 by 6e-6 to 3e-4 of max|ref| depending on the seed, so the bound is
    computed here: max(1e-5, 4 x that deviation) -- the margin the project gives a path against the reference's own fp32 floor."""
    import eabnet_amd
    n_fft, hop, win = sref.CASES[0]
    wav, cot, window, L, T = _inputs(n_fft, hop, win, 0, seed=seed)
    want = _torch_chain(wav, window, n_fft, hop, cot, torch.float64)
    floor = np.abs(_torch_chain(wav, window, n_fft, hop, cot, torch.float32) - want).max() / np.abs(want).max()
    w = wav.to(dev).requires_grad_(True)
    (eabnet_amd.stft_compress(w, n_fft, hop, window) * cot.to(dev)).sum().backward()
    err = np.abs(w.grad.cpu().double().numpy() - want).max() / np.abs(want).max()
    print(f"seed {seed}: device {err:.3e}, fp32 torch autograd {floor:.3e} of max|ref| (bound {max(1e-5, 4 * floor):.3e})")
    assert err <= max(1e-5, 4.0 * floor)
