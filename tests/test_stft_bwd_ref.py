"""The float64 restatement of the STFT front end's adjoint (tests/stft_bwd_ref.py, the contract of eab_stft_compress_bwd_f32,
DESIGN.md §4.28) against float64 torch autograd through torch.stft(center=True, pad_mode="reflect") followed by X |X|^-1/2.
No GPU, no library.  Both sides are float64: the bar is 1e-10 of max|ref|."""
import numpy as np
import pytest
import torch

import stft_bwd_ref as sref

REL = 1e-10
B, M = 2, 3


def autograd_case(n_fft, hop, win, layout, lengths, seed=0, silent=None, guard=False):
    """(spec, dspec, dwav by autograd, L, window): waves N(0, 0.1) in float64, a random cotangent on the compressed spectrum;
    every utterance goes through torch.stft alone at its own length, as the device's lengths form defines it.
    silent = (b, m): that channel is all zeros.  guard: the composition with the 0 -> 0 convention written with torch.where,
    so that the other channels of a case with a silent one have an autograd result to compare with."""
    g = torch.Generator().manual_seed(seed)
    Mc = M if layout == 0 else 1
    L = 11 * hop + 37
    T, F = 1 + L // hop, n_fft // 2 + 1
    lens = [L, L - 3 * hop - 5] if lengths else [L, L]
    wav = (0.1 * torch.randn(B, Mc, L, generator=g, dtype=torch.float64))
    if silent is not None:
        wav[silent[0], silent[1]] = 0.0
    wav.requires_grad_(True)
    window = torch.from_numpy(sref.padded_window(n_fft, win))
    cot = torch.randn(B, Mc, T, F, generator=g, dtype=torch.float64) + 1j * torch.randn(B, Mc, T, F, generator=g, dtype=torch.float64)
    spec = torch.zeros(B, Mc, T, F, dtype=torch.complex128)
    loss = 0.0
    for b in range(B):
        X = torch.stft(wav[b, :, :lens[b]], n_fft, hop_length=hop, win_length=n_fft, window=window, center=True, pad_mode="reflect",
                       return_complex=True).transpose(1, 2)                       # (M, T_b, F)
        mag = X.abs()
        if guard:
            s = torch.where(mag > 0, X / torch.where(mag > 0, mag, torch.ones_like(mag)).sqrt(), torch.zeros_like(X))
        else:
            s = X * mag.pow(-0.5)
        Tb = s.shape[1]
        assert Tb == 1 + lens[b] // hop
        spec[b, :, :Tb] = s.detach()
        loss = loss + (s.real * cot[b, :, :Tb].real + s.imag * cot[b, :, :Tb].imag).sum()
    loss.backward()
    cot = cot.numpy().copy()
    spec = spec.numpy().copy()
    for b in range(B):                                                            # frames behind an utterance are never read
        Tb = 1 + lens[b] // hop
        cot[b, :, Tb:] = np.nan
        spec[b, :, Tb:] = np.nan
    return (sref.from_bmtf(spec, layout), sref.from_bmtf(cot, layout), wav.grad.numpy(), L, window.numpy(),
            lens if lengths else None)


@pytest.mark.parametrize("lengths", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n_fft,hop,win", sref.CASES)
def test_restatement_matches_float64_autograd(n_fft, hop, win, layout, lengths):
    spec, dspec, want, L, window, lens = autograd_case(n_fft, hop, win, layout, lengths)
    assert np.abs(sref.to_bmtf(np.nan_to_num(spec, nan=1.0), layout)).min() > 0, "the case must have no zero bin"
    got = sref.stft_compress_bwd_ref(dspec, spec, window, n_fft, hop, layout, L, lens)
    assert got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"n_fft {n_fft} hop {hop} win {win} layout {layout} lengths {lens}: {err:.3e}")
    assert err <= REL
    if lens is not None:
        assert (got[1, :, lens[1]:] == 0).all() and (want[1, :, lens[1]:] == 0).all()


def test_a_silent_channel_gives_exact_zeros_where_torch_gives_nan():
    n_fft, hop, win = sref.CASES[0]
    spec, dspec, nan_grad, L, window, _ = autograd_case(n_fft, hop, win, 0, False, silent=(0, 1))
    assert np.isnan(nan_grad[0, 1]).all(), "the unguarded torch composition is expected to give NaN on a silent channel"
    got = sref.stft_compress_bwd_ref(dspec, spec, window, n_fft, hop, 0, L)
    assert np.isfinite(got).all() and (got[0, 1] == 0).all()
    # the other channels: the guarded composition has a finite autograd result, and the restatement equals it
    _, _, want, _, _, _ = autograd_case(n_fft, hop, win, 0, False, silent=(0, 1), guard=True)
    keep = np.ones((B, M), bool)
    keep[0, 1] = False
    assert np.abs(got[keep] - want[keep]).max() / np.abs(want[keep]).max() <= REL


def test_compression_jacobian_has_no_cancellation_form():
    """g / rho - s (s . g) / (2 rho^3): along s the gradient is halved, across s it is kept"""
    s = np.array([3.0 + 4.0j])
    rho = 5.0
    along, across = s / rho, 1j * s / rho
    assert np.allclose(sref.compress_grad(s, along), along / (2 * rho))
    assert np.allclose(sref.compress_grad(s, across), across / rho)
    assert (sref.compress_grad(np.zeros(2, complex), np.ones(2, complex)) == 0).all()
