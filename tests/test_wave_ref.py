"""The float64 restatements of tests/wave_ref.py against float64 autograd (``torch.istft`` and the SI-SDR formula), and the
host-side surface of the waveform loss: the ABI, the new entry points and their refusals.  No GPU needed."""
import numpy as np
import pytest
import torch

import score_ref
import wave_ref as W

REL = 1e-12


def _spec(B, T, F, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.standard_normal((B, 2, T, F)))


def _autograd_istft(spec, window, n_fft, hop, win, dwav):
    """d <istft(spec), dwav> / d spec by float64 autograd: spec (B, 2, T, F) as the package lays it out"""
    x = spec.clone().requires_grad_(True)
    y = torch.istft(torch.view_as_complex(x.permute(0, 3, 2, 1).contiguous()), n_fft, hop, win, torch.from_numpy(window))
    assert y.shape == dwav.shape
    (g,) = torch.autograd.grad((y * dwav).sum(), x)
    return g.numpy()


@pytest.mark.parametrize("n_fft,hop,win,T", W.ISTFT_CASES)
def test_istft_adjoint_matches_float64_autograd(n_fft, hop, win, T):
    B, F = 2, n_fft // 2 + 1
    window = W.window_for(n_fft, hop, win)
    dwav = torch.from_numpy(np.random.default_rng(7).standard_normal((B, hop * (T - 1))))
    want = _autograd_istft(_spec(B, T, F, 3), window, n_fft, hop, win, dwav)
    got = W.istft_bwd(dwav.numpy(), W.padded(window, n_fft), n_fft, hop, T)
    rel = np.abs(got - want).max() / np.abs(want).max()
    print(f"({n_fft},{hop},{win},{T}): max |diff| / max |ref| = {rel:.2e}")
    assert rel <= REL
    assert (got[:, 1, :, 0] == 0).all() and (got[:, 1, :, -1] == 0).all()


def test_istft_adjoint_with_lengths_is_the_per_utterance_adjoint():
    n_fft, hop, T, lens = 320, 160, 12, [12, 5, 2]
    window = W.window_for(n_fft, hop, n_fft)
    dwav = np.random.default_rng(11).standard_normal((3, hop * (T - 1)))
    got = W.istft_bwd(dwav, window, n_fft, hop, T, lens)
    for b, n in enumerate(lens):
        d = torch.from_numpy(dwav[b:b + 1, :hop * (n - 1)].copy())
        want = _autograd_istft(_spec(1, n, n_fft // 2 + 1, 5), window, n_fft, hop, n_fft, d)
        assert np.abs(got[b:b + 1, :, :n] - want).max() <= REL * np.abs(want).max(), b
        assert (got[b, :, n:] == 0).all(), b


def _autograd_si_sdr(est, clean, eps):
    n = max(est.shape[0], clean.shape[0])
    e = torch.zeros(n, dtype=torch.float64)
    s = torch.zeros(n, dtype=torch.float64)
    e[:est.shape[0]], s[:clean.shape[0]] = torch.from_numpy(est.astype(np.float64)), torch.from_numpy(clean.astype(np.float64))
    e.requires_grad_(True)
    tgt = (e @ s) ** 2 / (s @ s)
    loss = -10.0 * (torch.log10(tgt + eps) - torch.log10(e @ e - tgt + eps))
    (g,) = torch.autograd.grad(loss, e)
    return float(loss.detach()), g.numpy()[:est.shape[0]]


@pytest.mark.parametrize("eps", [0.0, 1e-8])
@pytest.mark.parametrize("Le,Ls", [(900, 1000), (1000, 900), (777, 777)])
def test_si_sdr_loss_and_gradient_match_float64_autograd(Le, Ls, eps):
    # rows wider than the lengths: the signals are the first Le / Ls samples of rows of 1100 with NaN behind them
    rows = np.full((2, 1100), np.nan, np.float32)
    rows[0, :Le], rows[1, :Ls] = W.make_pair(Le, Ls, 31 + Le)
    est, clean = rows[0, :Le], rows[1, :Ls]
    loss, grad = W.si_sdr_loss(est, clean, eps)
    want, wgrad = _autograd_si_sdr(est, clean, eps)
    assert np.isfinite(loss) and abs(loss - want) <= REL * abs(want)
    assert np.abs(grad - wgrad).max() <= 1e-11 * np.abs(wgrad).max()
    if eps == 0.0:
        noisy = np.zeros(max(Le, Ls), np.float32)                # (the mixture plays no part in column 0)
        noisy[:Ls] = clean
        noisy[:Le] += est
        sdr = score_ref.ratios(est, clean, noisy)[0]
        assert abs(loss + sdr) <= 1e-9, (loss, sdr)


def test_abi_stays_and_the_new_entry_points_refuse_bad_arguments_on_the_host():
    from eabnet_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.eab_abi_version() == 10
    for name in ("eab_istft_bwd_f32", "eab_si_sdr_loss_f32", "eab_si_sdr_loss_bwd_f32"):
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes is not None
    one = 16                                                     # (a non-NULL address that is never dereferenced: nothing launches)
    assert lib.eab_istft_bwd_f32(None, None, None, None, None, 1, 9, 320, 160, None) == 1
    assert lib.eab_istft_bwd_f32(one, one, one, one, None, 1, 1, 320, 160, None) == 1        # T < 2
    assert lib.eab_istft_bwd_f32(one, one, one, one, None, 1, 9, 321, 160, None) == 1        # odd n_fft
    assert lib.eab_istft_bwd_f32(one, one, one, one, None, 1, 9, 320, 32, None) == 2         # ten covering frames: unsupported
    assert lib.eab_si_sdr_loss_f32(None, 8, 8, None, 8, 8, None, 1, 0.0, None, 1, None, None, None, None) == 1
    assert lib.eab_si_sdr_loss_f32(one, 8, 8, one, 8, 8, one, 0, 0.0, one, 1, one, one, one, None) == 1      # B = 0
    assert lib.eab_si_sdr_loss_f32(one, 4, 8, one, 8, 8, one, 2, 0.0, one, 1, one, one, one, None) == 1      # rows overlap
    assert lib.eab_si_sdr_loss_f32(one, 8, 8, one, 8, 8, one, 1, -1.0, one, 1, one, one, one, None) == 1     # eps < 0
    assert lib.eab_si_sdr_loss_f32(one, 8, 5000, one, 8, 8, one, 1, 0.0, one, 1, one, one, one, None) == 1   # too few spans
    assert lib.eab_si_sdr_loss_bwd_f32(None, 8, 8, None, 8, 8, None, 1, None, None, 0, 1.0, None, 8, None) == 1
    assert lib.eab_si_sdr_loss_bwd_f32(one, 8, 8, one, 8, 8, one, 2, one, one, 1, 1.0, one, 4, None) == 1    # grad rows overlap
    assert lib.eab_si_sdr_loss_bwd_f32(one, 8, 8, one, 8, 8, one, 1, one, one, -1, 1.0, one, 8, None) == 1


def test_wave_functions_refuse_what_they_do_not_run():
    import eabnet_amd
    assert "si_sdr_loss" in eabnet_amd.__all__
    x = torch.zeros(1, 2, 4, 161, requires_grad=True)
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        eabnet_amd.istft(x, 320, 160, torch.hann_window(320))
    est, clean = torch.zeros(2, 100), torch.ones(2, 100)
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        eabnet_amd.si_sdr_loss(est, clean)
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        eabnet_amd.si_sdr_loss(est.requires_grad_(True), clean[:, None])
    with pytest.raises(ValueError, match="reduction"):
        eabnet_amd.si_sdr_loss(est, clean, reduction="max")
    with pytest.raises(ValueError, match="eps"):
        eabnet_amd.si_sdr_loss(est, clean, eps=-1.0)
    with pytest.raises(ValueError, match="same number of rows"):
        eabnet_amd.si_sdr_loss(est, clean[:1])


def test_si_sdr_loss_refuses_a_differentiable_clean_and_other_dtypes():
    """refused with the reason before anything touches a device"""
    from eabnet_amd import si_sdr_loss
    with pytest.raises(NotImplementedError, match="clean requires grad"):
        si_sdr_loss(torch.zeros(2, 100), torch.ones(2, 100, requires_grad=True))
    with pytest.raises(TypeError, match="fp32"):
        si_sdr_loss(torch.zeros(2, 100, dtype=torch.float64), torch.ones(2, 100))
    with pytest.raises(ValueError, match=r"lengths must lie in \[1, 100\]"):
        si_sdr_loss(torch.zeros(2, 100), torch.ones(2, 100), lengths=[100, 101])
    with pytest.raises(ValueError, match="pairs"):
        si_sdr_loss(torch.zeros(2, 100), torch.ones(2, 100), lengths=[(100, 100)])
