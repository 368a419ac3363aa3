"""Shared by the multi-resolution STFT loss tests: the float64 numpy restatement of the definition of DESIGN.md §4.21 (value and
analytic gradient, no autograd), and the same loss written with ``torch.stft`` (any dtype; under autograd it is the reference the
restatement is pinned to in tests/test_mrstft_ref.py, and in fp32 on the CPU it is the yardstick for what an fp32 evaluation can
reach).

    for (N, H, W):  X = torch.stft(x[:n], N, H, W, hann(W), center=True, pad_mode="reflect"),  T = 1 + n // H,  F = N/2 + 1
    P = max(re^2 + im^2, floor),  E = sqrt(P_est),  S = sqrt(P_clean)
    sc = sqrt(sum (S - E)^2) / sqrt(sum S^2),   lm = sum |ln S - ln E| / (T F)
    loss = 1/R sum_r (factor_sc sc_r + factor_mag lm_r)          (sums over the utterance's own frames and bins)"""
from __future__ import annotations

import numpy as np
import torch

DEFAULT = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
# radix 5 (40 = 2 * 20), win < n_fft with an odd remainder (64 - 49), a hop that does not divide
SMALL = ((64, 16, 48), (40, 10, 40), (64, 24, 49))

# the utterances of the GPU tests (tests/test_mrstft_gpu.py) and the seed of each: chosen on the CPU so that at floor = 0.02 no bin
# power of either signal lies within 1e-5 relative of the floor, and at the default floor the fp32 torch restatement's gradient is
# at most 1e-4 off (both asserted in tests/test_mrstft_ref.py).  That error depends on the host's FFT: on two machines these seeds
# gave 4e-7 to 6e-5, each within a factor of two between the machines; other seeds moved by a factor of forty
SEEDS = {33: 1, 129: 3, 257: 14, 1025: 3, 4099: 4, 12517: 8}
GRAD_FLOOR = 0.02
ROW, BATCH = 12600, (12517, 1025, 4099)
SILENT = (2000, 5548)


def make_signals(n: int, seed: int):
    """clean = 0.1 randn, est = clean + 0.05 randn: float64 draws rounded to fp32"""
    rng = np.random.default_rng(seed)
    clean = 0.1 * rng.standard_normal(n)
    est = clean + 0.05 * rng.standard_normal(n)
    return est.astype(np.float32), clean.astype(np.float32)


def window(N: int, W: int) -> np.ndarray:
    """the periodic Hann window of W samples at offset (N - W) // 2 of the N-frame, float64"""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)
    left = (N - W) // 2
    return np.pad(w, (left, N - W - left))


def _frames(x: np.ndarray, N: int, H: int, w: np.ndarray) -> np.ndarray:
    n = x.shape[0]
    pad = np.pad(x, N // 2, mode="reflect")
    return np.stack([pad[t * H:t * H + N] * w for t in range(1 + n // H)])


def loss_and_grad(est, clean, resolutions=DEFAULT, factor_sc=1.0, factor_mag=1.0, floor=1e-7):
    """est, clean (n,) -- one utterance, already cut to its length -> (loss, d loss / d est (n,)) in float64.  The gradient is zero
    through a clamped bin, the gradient of |.| at 0 is 0, and the sc part is zero where sum (S - E)^2 = 0."""
    e, s = np.asarray(est, np.float64), np.asarray(clean, np.float64)
    n, R = e.shape[0], len(resolutions)
    assert s.shape[0] == n and n > max(N for N, _, _ in resolutions) // 2
    loss, grad = 0.0, np.zeros(n)
    for N, H, W in resolutions:
        NH, w = N // 2, window(N, W)
        Xe, Xc = np.fft.rfft(_frames(e, N, H, w), axis=1), np.fft.rfft(_frames(s, N, H, w), axis=1)
        T, F = Xe.shape
        raw = Xe.real ** 2 + Xe.imag ** 2
        E, S = np.sqrt(np.maximum(raw, floor)), np.sqrt(np.maximum(Xc.real ** 2 + Xc.imag ** 2, floor))
        A, Q = ((S - E) ** 2).sum(), (S ** 2).sum()
        d = np.log(S) - np.log(E)
        loss += (factor_sc * np.sqrt(A) / np.sqrt(Q) + factor_mag * np.abs(d).sum() / (T * F)) / R
        gE = -factor_mag * np.sign(d) / (T * F * E)
        if A > 0.0:
            gE = gE - factor_sc * (S - E) / (np.sqrt(A) * np.sqrt(Q))
        G = np.where(raw >= floor, gE / R / E, 0.0) * Xe                 # d loss / d (re, im) as re + i im
        # d frame[m] = Re sum_k G_k e^{+2 pi i k m / N} = N/2 irfft(Y)[m],  Y = G inside, 2 Re G at DC and Nyquist
        Y = G.copy()
        Y[:, 0], Y[:, NH] = 2.0 * G[:, 0].real, 2.0 * G[:, NH].real
        dfr = NH * np.fft.irfft(Y, n=N, axis=1) * w
        dpad = np.zeros(n + N)
        for t in range(T):
            dpad[t * H:t * H + N] += dfr[t]
        grad += dpad[NH:NH + n]
        grad[1:NH + 1] += dpad[:NH][::-1]                                # reflect: padded p < NH is sample NH - p
        grad[n - 1 - NH:n - 1] += dpad[n + NH:][::-1]                    # padded NH + m, m >= n, is sample 2 (n - 1) - m
    return float(loss), grad


def torch_loss(est: torch.Tensor, clean: torch.Tensor, lengths=None, resolutions=DEFAULT, factor_sc=1.0, factor_mag=1.0,
               floor=1e-7) -> torch.Tensor:
    """the definition in torch operators, per utterance: est (B, Le), clean (B, Ls) of one dtype -> (B,) losses; differentiable"""
    B = est.shape[0]
    out = []
    for b in range(B):
        n = min(est.shape[1], clean.shape[1]) if lengths is None else int(lengths[b])
        v = 0.0
        for N, H, W in resolutions:
            win = torch.hann_window(W, dtype=est.dtype, device=est.device)
            P = [torch.clamp(torch.view_as_real(torch.stft(x[b, :n], N, H, W, win, center=True, pad_mode="reflect",
                                                           return_complex=True)).square().sum(-1), min=floor) for x in (est, clean)]
            E, S = torch.sqrt(P[0]), torch.sqrt(P[1])
            sc = torch.sqrt((S - E).square().sum()) / torch.sqrt(S.square().sum())
            lm = (torch.log(S) - torch.log(E)).abs().mean()
            v = v + factor_sc * sc + factor_mag * lm
        out.append(v / len(resolutions))
    return torch.stack(out)


def floor_margin(est, clean, resolutions, floor) -> float:
    """the smallest relative distance of a bin power of either signal to ``floor`` (float64): an fp32 evaluation rounds a power
    to about 1e-6, so a bin closer than that may fall on the other side of the clamp"""
    m = np.inf
    for N, H, W in resolutions:
        w = window(N, W)
        for x in (est, clean):
            X = np.fft.rfft(_frames(np.asarray(x, np.float64), N, H, w), axis=1)
            m = min(m, float(np.abs((X.real ** 2 + X.imag ** 2) / floor - 1.0).min()))
    return m


def fp32_restatement_error(est, clean, resolutions, floor):
    """(relative error of the value, max |diff| / max |ref| of the gradient) of the fp32 torch restatement on the CPU against the
    float64 restatement: what an fp32 evaluation of the definition reaches on this input"""
    want, wgrad = loss_and_grad(est, clean, resolutions, floor=floor)
    leaf = torch.from_numpy(np.asarray(est, np.float32)).requires_grad_(True)
    loss = torch_loss(leaf[None], torch.from_numpy(np.asarray(clean, np.float32))[None], None, resolutions, floor=floor)[0]
    (g,) = torch.autograd.grad(loss, leaf)
    return abs(float(loss.detach()) - want) / abs(want), float(np.abs(g.numpy() - wgrad).max() / np.abs(wgrad).max())


def silent_samples(n: int, resolutions, stretch) -> np.ndarray:
    """(n,) bool: the samples that only silent frames touch, when est and clean are zero over samples stretch[0]..stretch[1]: a
    frame is silent when every sample under its window's support lies in the stretch; its spectrum is then exactly zero, every
    bin is clamped, and it contributes exactly nothing to the gradient"""
    touched = np.zeros(n, bool)
    for N, H, W in resolutions:
        idx = np.pad(np.arange(n), N // 2, mode="reflect")
        left = (N - W) // 2
        for t in range(1 + n // H):
            under = idx[t * H + left:t * H + left + W]
            if not ((under >= stretch[0]) & (under < stretch[1])).all():
                touched[under] = True
    return ~touched
