"""Shared by the waveform-loss tests: float64 numpy restatements, written from the definitions of DESIGN.md §4.20, of the adjoint
of the ISTFT back end and of the negative SI-SDR with its gradient.  tests/test_wave_ref.py pins both to float64 autograd
(``torch.istft`` and the formula), so GPU tests may use them at any shape."""
from __future__ import annotations

import numpy as np
import torch

K = 10.0 / np.log(10.0)
# (n_fft, hop, win_length, T): the reference's geometry at its shortest and at several frames, a hop that does not divide, a
# padded window, eight covering frames, no overlap
ISTFT_CASES = [(320, 160, 320, 2), (320, 160, 320, 9), (320, 100, 320, 7), (256, 64, 200, 5), (320, 40, 320, 12), (16, 16, 16, 4)]


def window_for(n_fft: int, hop: int, win: int) -> np.ndarray:
    """the analysis window of a case as float64, before padding (rectangular where the hop leaves a Hann window no overlap)"""
    return np.ones(win) if hop >= win else torch.hann_window(win, dtype=torch.float64).numpy()


def padded(window: np.ndarray, n_fft: int) -> np.ndarray:
    """a window shorter than n_fft zero-padded on both sides, centred (torch.istft)"""
    left = (n_fft - window.shape[0]) // 2
    return np.pad(np.asarray(window, np.float64), (left, n_fft - window.shape[0] - left))


def istft_bwd(dwav, window, n_fft: int, hop: int, T: int, lens=None) -> np.ndarray:
    """dwav (B, hop (T-1)), window (n_fft,) already padded -> dspec (B, 2, T, F) float64: with NH = n_fft/2 and Tb = lens[b] (or T)
        env(p) = sum over frames t' < Tb that cover p of w[p - t' hop]^2
        u_t[idx] = w[idx] dwav[b][j] / env(p),  p = t hop + idx, j = p - NH, for 0 <= j < hop (Tb - 1), else 0
        dspec[b][.][t][k] = c_k / n_fft rfft(u_t)[k],  c = 1 at k = 0 and NH else 2, imaginary parts 0 at those two bins;
    frames t >= Tb are zeros, dwav is not read at j >= hop (Tb - 1)"""
    dwav = np.asarray(dwav, np.float64)
    w = np.asarray(window, np.float64)
    B, NH = dwav.shape[0], n_fft // 2
    out = np.zeros((B, 2, T, NH + 1))
    c = np.full(NH + 1, 2.0)
    c[0] = c[NH] = 1.0
    for b in range(B):
        Tb = T if lens is None else int(lens[b])
        env = np.zeros(n_fft + hop * (Tb - 1))
        for t in range(Tb):
            env[t * hop:t * hop + n_fft] += w ** 2
        n = hop * (Tb - 1)
        for t in range(Tb):
            u = np.zeros(n_fft)
            for idx in range(n_fft):
                p = t * hop + idx
                j = p - NH
                if 0 <= j < n:
                    u[idx] = w[idx] * dwav[b, j] / env[p]
            U = np.fft.rfft(u) * c / n_fft
            out[b, 0, t], out[b, 1, t] = U.real, U.imag
            out[b, 1, t, 0] = out[b, 1, t, NH] = 0.0
    return out


def si_sdr_loss(est, clean, eps: float = 0.0):
    """est (Le,), clean (Ls,), each zero from its own length up to the longer -> (loss, grad (Le,)) in float64:
        loss = -K [ln(tgt + eps) - ln(res + eps)],  tgt = <e,s>^2 / <s,s>,  res = <e,e> - tgt
        d loss / d e_i = -K [2 alpha s_i / (tgt + eps) - (2 e_i - 2 alpha s_i) / (res + eps)],  alpha = <e,s> / <s,s>"""
    n = max(est.shape[0], clean.shape[0])
    e, s = np.zeros(n), np.zeros(n)
    e[:est.shape[0]], s[:clean.shape[0]] = est, clean
    es, ss, ee = e @ s, s @ s, e @ e
    alpha, tgt = es / ss, es * es / ss
    res = ee - tgt
    loss = -K * (np.log(tgt + eps) - np.log(res + eps))
    grad = -K * (2.0 * alpha * s / (tgt + eps) - (2.0 * e - 2.0 * alpha * s) / (res + eps))
    return float(loss), grad[:est.shape[0]]


def make_pair(Le: int, Ls: int, seed: int, gain: float = 0.7, noise: float = 0.3, onset=None):
    """seeded fp32 (est (Le,), clean (Ls,)): est = gain clean + noise on the overlap, so the SI-SDR is moderate.  onset: the
    clean wave's first sample (a click) -- an estimate much shorter than its clean wave has a moderate SI-SDR only if the
    samples it covers carry a fair share of the clean energy"""
    rng = np.random.default_rng(seed)
    n = max(Le, Ls)
    s = rng.standard_normal(n).astype(np.float32)
    s[Ls:] = 0.0
    if onset is not None:
        s[0] = onset
    e = (np.float32(gain) * s + np.float32(noise) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    return e[:Le].copy(), s[:Ls].copy()
