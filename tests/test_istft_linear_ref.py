"""The float64 restatements of tests/istft_lin_ref.py (``istft(decompress=True)`` and its adjoint) against float64 torch autograd of
``torch.istft(view_as_complex(decompress(x)))``, and the Python surface of the switch: the signatures, the bool check, the refusal
of CPU tensors.  No GPU needed.

Bound: both sides are float64 evaluations of the same formula in another order, so they agree to rounding; 1e-12 of max |ref|
leaves four decimal orders above the 2.2e-16 of the format times the few hundred terms of a bin's sum."""
import inspect

import numpy as np
import pytest
import torch

import eabnet_amd
import istft_lin_ref as R

TOL64 = 1e-12


def _torch64(spec, dwav, window, n_fft, hop, lens=None):
    """(wav, dspec) of float64 torch: x |x| by ``norm`` over the (re, im) axis (whose derivative at 0 is 0), then torch.istft"""
    B, _, T, _ = spec.shape
    wavs, grads = np.zeros((B, hop * (T - 1))), np.zeros(spec.shape)
    for b in range(B):
        Tb = T if lens is None else lens[b]
        x = torch.from_numpy(spec[b:b + 1, :, :Tb]).double().requires_grad_(True)
        y = x * x.norm(dim=1, keepdim=True)
        wav = torch.istft(torch.view_as_complex(y.permute(0, 3, 2, 1).contiguous()), n_fft, hop, n_fft,
                          torch.from_numpy(window).double())
        n = hop * (Tb - 1)
        (g,) = torch.autograd.grad(wav, x, grad_outputs=torch.from_numpy(dwav[b:b + 1, :n]).double())
        wavs[b, :n], grads[b, :, :Tb] = wav[0].detach().numpy(), g[0].numpy()
    return wavs, grads


@pytest.mark.parametrize("n_fft,hop,win,T,B", R.CASES)
def test_restatement_vs_float64_autograd(n_fft, hop, win, T, B):
    spec, dwav, window, zero = R.make_case(n_fft, hop, win, T, B)
    want_wav, want_grad = _torch64(spec, dwav, window, n_fft, hop)
    wav = R.istft(spec, window, n_fft, hop)
    grad = R.istft_bwd(dwav, spec, window, n_fft, hop)
    ew = np.abs(wav - want_wav).max() / np.abs(want_wav).max()
    eg = np.abs(grad - want_grad).max() / np.abs(want_grad).max()
    print(f"({n_fft},{hop},{win},{T},{B}): wave {ew:.2e}, gradient {eg:.2e} of max |ref| (bound {TOL64:.0e})")
    assert np.isfinite(want_grad).all() and ew <= TOL64 and eg <= TOL64
    b, t, f = zero
    assert (grad[b, :, t, f] == 0).all() and (want_grad[b, :, t, f] == 0).all()
    # the imaginary parts at DC and Nyquist act through the modulus: their gradient is im re g_re / r, not zero
    assert (np.abs(grad[:, 1, :, 0]) > 0).any() and (np.abs(grad[:, 1, :, -1]) > 0).any()


def test_restatement_with_lengths_vs_float64_autograd():
    n_fft, hop, win, T, lens = 320, 160, 320, 9, [9, 4]
    spec, dwav, window, _ = R.make_case(n_fft, hop, win, T, 2)
    want_wav, want_grad = _torch64(spec, dwav, window, n_fft, hop, lens)
    poisoned, dpoisoned = spec.copy(), dwav.copy()
    for b, n in enumerate(lens):
        poisoned[b, :, n:] = np.nan
        dpoisoned[b, hop * (n - 1):] = np.nan
    wav = R.istft(poisoned, window, n_fft, hop, lens)
    grad = R.istft_bwd(dpoisoned, poisoned, window, n_fft, hop, lens)
    assert np.isfinite(wav).all() and np.isfinite(grad).all()
    assert np.abs(wav - want_wav).max() <= TOL64 * np.abs(want_wav).max()
    assert np.abs(grad - want_grad).max() <= TOL64 * np.abs(want_grad).max()
    for b, n in enumerate(lens):
        assert (wav[b, hop * (n - 1):] == 0).all() and (grad[b, :, n:] == 0).all()


def test_signatures_carry_the_switch_with_the_default_off():
    p = inspect.signature(eabnet_amd.istft).parameters
    assert list(p) == ["esti_stft", "fft_num", "win_shift", "window", "lengths", "decompress"]
    assert p["lengths"].default is None and p["decompress"].default is False
    for tool in (eabnet_amd.Enhancer, eabnet_amd.Scorer, eabnet_amd.StreamingEnhancer):
        q = inspect.signature(tool).parameters
        assert "decompress" in q and q["decompress"].default is False, tool.__name__
        assert q["decompress"].kind is inspect.Parameter.KEYWORD_ONLY
        assert tool.decompress is False
    for fn in (eabnet_amd.istft, eabnet_amd.Enhancer, eabnet_amd.Scorer, eabnet_amd.StreamingEnhancer):
        assert "clean files" in " ".join(fn.__doc__.split()), "the docstring says what True means"


def test_decompress_must_be_a_bool():
    x = torch.zeros(1, 2, 4, 161)
    for bad in (1, 0, None, "yes", np.bool_(True)):
        with pytest.raises(TypeError, match="decompress must be a bool"):
            eabnet_amd.istft(x, 320, 160, torch.hann_window(320), decompress=bad)
    net = eabnet_amd.EaBNet(M=2, p=1, q=1)
    for tool, args in ((eabnet_amd.Enhancer, (net,)), (eabnet_amd.Scorer, (net,)), (eabnet_amd.StreamingEnhancer, (net, 1, 1.0))):
        with pytest.raises(TypeError, match="decompress must be a bool"):
            tool(*args, decompress=1)
    assert eabnet_amd.Enhancer(net, decompress=True).decompress is True
    assert eabnet_amd.Scorer(net, decompress=True, distortion=True).decompress is True
    assert eabnet_amd.Enhancer(net).decompress is False and eabnet_amd.Scorer(net).decompress is False


def test_cpu_tensors_are_refused_with_and_without_the_switch():
    x = torch.zeros(1, 2, 4, 161)
    for flag in (False, True):
        with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
            eabnet_amd.istft(x, 320, 160, torch.hann_window(320), decompress=flag)
        with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
            eabnet_amd.istft(x.clone().requires_grad_(True), 320, 160, torch.hann_window(320), decompress=flag)
