"""Shared by the linear-domain ISTFT tests: float64 numpy restatements, written from the definitions of DESIGN.md §4.26, of
``istft(decompress=True)`` and of its adjoint, lengths included.  tests/test_istft_linear_ref.py pins both to float64 autograd of
``torch.istft(view_as_complex(decompress(x)))``, so the GPU and host-emulation tests may use them at any shape.

    y = s |s| per bin (s = (re, im)); the wave is the back end's wave of y: irfft frames (the imaginary parts of y at DC and
    Nyquist ignored) times the window, overlap-added, divided by the squared-window envelope of the frames that exist, trimmed
    by n_fft/2; with lengths utterance b is its first lens[b] frames and zeros follow its hop (lens[b] - 1) samples.
    adjoint: g = the back end's adjoint of dwav (wave_ref.istft_bwd), dspec = r g + s (s . g) / r, exactly 0 where r == 0."""
from __future__ import annotations

import numpy as np

import wave_ref as W

# (n_fft, hop, win_length, T, B): the reference's geometry at its shortest and over two workgroups, a hop that does not divide
# and three workgroups of the adjoint, a padded window, eight covering frames
CASES = [(320, 160, 320, 2, 1), (320, 160, 320, 9, 2), (320, 100, 320, 17, 2), (256, 64, 200, 12, 1), (320, 40, 320, 20, 1)]


def decompress(spec: np.ndarray) -> np.ndarray:
    """(B, 2, T, F) -> s |s| in float64"""
    s = np.asarray(spec, np.float64)
    return s * np.sqrt(s[:, :1] ** 2 + s[:, 1:] ** 2)


def istft(spec, window, n_fft: int, hop: int, lens=None) -> np.ndarray:
    """spec (B, 2, T, F), window (n_fft,) already padded -> wav (B, hop (T-1)) float64; frames t >= lens[b] are not read"""
    spec = np.asarray(spec, np.float64)
    w = np.asarray(window, np.float64)
    B, _, T, _ = spec.shape
    NH = n_fft // 2
    out = np.zeros((B, hop * (T - 1)))
    for b in range(B):
        Tb = T if lens is None else int(lens[b])
        y = decompress(spec[b:b + 1, :, :Tb])[0]
        acc, env = np.zeros(n_fft + hop * (Tb - 1)), np.zeros(n_fft + hop * (Tb - 1))
        for t in range(Tb):
            Y = y[0, t] + 1j * y[1, t]
            Y[0], Y[NH] = Y[0].real, Y[NH].real                      # a C2R transform ignores these two imaginary parts
            acc[t * hop:t * hop + n_fft] += np.fft.irfft(Y, n_fft) * w
            env[t * hop:t * hop + n_fft] += w ** 2
        n = hop * (Tb - 1)
        out[b, :n] = acc[NH:NH + n] / env[NH:NH + n]
    return out


def istft_bwd(dwav, spec, window, n_fft: int, hop: int, lens=None) -> np.ndarray:
    """dwav (B, hop (T-1)), spec (B, 2, T, F) -> dspec (B, 2, T, F) float64; neither is read behind a length, where dspec is 0"""
    spec = np.asarray(spec, np.float64)
    B, _, T, _ = spec.shape
    dwav = np.array(dwav, np.float64)
    s = spec.copy()
    if lens is not None:
        for b in range(B):
            dwav[b, hop * (int(lens[b]) - 1):] = 0.0
            s[b, :, int(lens[b]):] = 0.0
    g = W.istft_bwd(dwav, window, n_fft, hop, T, lens)
    r = np.sqrt(s[:, :1] ** 2 + s[:, 1:] ** 2)
    dot = (s * g).sum(1, keepdims=True)
    safe = np.where(r == 0.0, 1.0, r)
    return np.where(r == 0.0, 0.0, r * g + s * dot / safe)


def make_case(n_fft: int, hop: int, win: int, T: int, B: int, seed: int = 0):
    """seeded fp32 (spec (B, 2, T, F), dwav (B, hop (T-1)), padded window (n_fft,), zero bin (b, t, f)): a spectrum of unit
    normal parts -- the imaginary parts at DC and Nyquist among them, non-zero -- with one bin exactly 0"""
    rng = np.random.default_rng(1000 * seed + 10 * T + B)
    F = n_fft // 2 + 1
    spec = rng.standard_normal((B, 2, T, F)).astype(np.float32)
    zero = (B - 1, 1, F // 3)                                         # (frame 1: inside every utterance of two frames or more)
    spec[zero[0], :, zero[1], zero[2]] = 0.0
    assert (spec[:, 1, :, 0] != 0).all() and (spec[:, 1, :, -1] != 0).all()
    dwav = rng.standard_normal((B, hop * (T - 1))).astype(np.float32)
    window = W.padded(W.window_for(n_fft, hop, win), n_fft).astype(np.float32)
    return spec, dwav, window, zero
