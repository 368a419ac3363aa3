"""Shared by the scoring tests: seeded cases (clean, noisy, estimate) and a float64 numpy restatement of the reference's energy
ratios (metrics.py:14-39) and mixture SI-SDR (metrics.py:71-75), written from the formulas.  tests/test_score_ref.py pins the
restatement to the reference's recorded values (tests/golden/score_cases.npz), so GPU tests may use it at any shape."""
from __future__ import annotations

import numpy as np

import paramgen

# (clean, noisy, estimate) samples, seed, g_s, g_n, g_a[, quiet_tail]: the fixture's cases, in its order
CASES = [
    (161, 161, 160, 900, 0.8, 0.2, 0.1),            # shortest admissible file, 2 frames
    (1763, 1763, 1600, 901, 0.8, 0.2, 0.1),         # odd length
    (3203, 3203, 3200, 902, 0.8, 0.2, 0.1),         # L % 4 = 3
    (4000, 4000, 3840, 903, 0.8, 0.2, 0.1),         # aligned length
    (48001, 48001, 47840, 904, 0.8, 0.2, 0.1),      # several spans and workgroups
    (2085, 1700, 1920, 905, 0.8, 0.2, 0.1),         # zero extension: clean longest
    (1700, 2085, 1920, 906, 0.8, 0.2, 0.1),         # zero extension: noisy longest
    # SAR between 40 and 60 dB: only with a silent tail (make_case) and a seed whose clean and noise are nearly orthogonal --
    # the two separate projections leave g_s (s.n / n.n) n + g_n (s.n / s.s) s behind, ~35 dB below the target at most seeds
    (4000, 4000, 3840, 913, 0.8, 0.2, 0.002, True),
    (4000, 4000, 3840, 908, 0.05, 0.9, 0.3),        # negative ratios
]


def make_case(Ls, Ly, Le, seed, g_s, g_n, g_a, quiet_tail=False):
    """three INDEPENDENT seeded fp32 waves (their own make_wave seeds: the channels of one call share a source) -> fp32
    (clean (Ls,), noisy (Ly,), estimate (Le,)): y = s + noise on the overlap, est = g_s s + g_n noise + g_a artefact.
    quiet_tail: clean and noise are silent from Le on (a recording that ends in digital silence), so the cut of the estimate
    takes nothing away -- without it the samples the estimate lacks are an artefact of their own (SAR <= ~14 dB at 3840 of
    4000 samples)"""
    n = max(Ls, Ly, Le)
    s, noise, art = (paramgen.make_wave(1, 1, n, 3 * seed + k)[0, 0] for k in range(3))
    if quiet_tail:
        s[Le:] = 0.0
        noise[Le:] = 0.0
    clean = s[:Ls].copy()
    ext = np.zeros(n, np.float32)
    ext[:Ls] = clean
    noisy = (ext + noise)[:Ly].astype(np.float32)
    est = (np.float32(g_s) * ext + np.float32(g_n) * noise + np.float32(g_a) * art)[:Le].astype(np.float32)
    return clean, noisy, est


def _extend(x, n):
    out = np.zeros(n, np.float64)
    out[:x.shape[0]] = x
    return out


def ratios(est, clean, noisy):
    """[si_sdr, si_sir, si_sar, si_sdr_mix] in dB, float64, element by element (the two-pass form): every signal zero-extended
    to the longest (test.py:126-138), n = y - s, s_target / e_noise the projections of the estimate on s / n, e_art the rest;
    the mixture's SI-SDR is that of y against s"""
    n = max(est.shape[0], clean.shape[0], noisy.shape[0])
    e, s, y = _extend(est, n), _extend(clean, n), _extend(noisy, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = y - s
        target = (e @ s) / (s @ s) * s
        noise = (e @ d) / (d @ d) * d
        art = e - target - noise
        pw = lambda v: float(v @ v)  # noqa: E731
        db = lambda a, b: 10.0 * np.log10(np.float64(a) / np.float64(b))  # noqa: E731
        mix_t = (y @ s) / (s @ s) * s
        return np.array([db(pw(target), pw(noise + art)), db(pw(target), pw(noise)), db(pw(target), pw(art)),
                         db(pw(mix_t), pw(mix_t - y))])


def loss_one(esti, label, n):
    """com_mag_mse_loss of ONE utterance at n frames, float64 numpy, from the formula (EaBNet.py:627-640): esti, label (2, T, F)"""
    e, l = np.asarray(esti[:, :n], np.float64), np.asarray(label[:, :n], np.float64)
    mag = (np.sqrt((e ** 2).sum(0)) - np.sqrt((l ** 2).sum(0))) ** 2
    return 0.5 * (mag.mean() + ((e - l) ** 2).mean())
