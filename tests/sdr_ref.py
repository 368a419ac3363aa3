"""Shared by the SDR tests: a float64 numpy restatement of the BSS-eval SDR, its loss and its gradient, written from the
definition of DESIGN.md §4.25, and the signal generator of the tests.  It does not import the package.  The correlations are
direct sums and the Toeplitz system goes through a DENSE solve (the device runs a Levinson recursion: the two share nothing), and
every call asserts on its own inputs that the system is well conditioned and solved, so that a test never compares two wrong
answers.  tests/test_sdr_ref.py pins the gradient to central differences and K = 1 to the SI-SDR restatement."""
from __future__ import annotations

import numpy as np

K10 = 10.0 / np.log(10.0)
AR = (1.0, -2.6, 2.5, -0.88)                  # s = lfilter([1], AR, white): a resonant, strongly coloured "speech"
COND_MAX = 1e8
RESID_MAX = 1e-9


def colored(n: int, rng) -> np.ndarray:
    """n samples of white noise through 1 / AR, the first 200 dropped, as float64 (callers round to fp32)"""
    w = rng.standard_normal(n + 200)
    y = np.zeros(n + 200 + 3)
    for i in range(n + 200):
        y[i + 3] = w[i] - AR[1] * y[i + 2] - AR[2] * y[i + 1] - AR[3] * y[i]
    return y[203:]


def make_pair(Le: int, Ls: int, seed: int, sigma: float):
    """seeded fp32 (est (Le,), clean (Ls,)): est = (clean * g) + sigma white, g 40 random taps under exp(-k / 8) -- a lightly
    filtered copy plus noise (the clean wave's rms is about 15, that of clean * g about 38)"""
    rng = np.random.default_rng(seed)
    s = colored(Ls, rng).astype(np.float32)
    g = rng.standard_normal(40) * np.exp(-np.arange(40) / 8.0)
    full = np.convolve(s.astype(np.float64), g)
    e = sigma * rng.standard_normal(Le)
    e[:min(Le, full.shape[0])] += full[:Le]
    return e.astype(np.float32), s


def make_delayed(L: int, seed: int, delay: int = 37, snr_db: float = 10.0):
    """seeded fp32 (est, clean) of L samples: est = clean delayed by ``delay`` samples plus white noise at ``snr_db``"""
    rng = np.random.default_rng(seed)
    s = colored(L, rng).astype(np.float32)
    d = np.zeros(L)
    d[delay:] = s[:L - delay]
    noise = rng.standard_normal(L)
    noise *= np.sqrt(np.sum(d ** 2) / np.sum(noise ** 2) / 10.0 ** (snr_db / 10.0))
    return (d + noise).astype(np.float32), s


def correlations(est, clean, K: int):
    """(r (K,), c (K,), ee, e, s) by direct sums, e and s zero-extended to N = max(Le, Ls) in float64"""
    n = max(est.shape[0], clean.shape[0])
    e, s = np.zeros(n), np.zeros(n)
    e[:est.shape[0]], s[:clean.shape[0]] = est, clean
    r = np.array([s[:n - k] @ s[k:] if k < n else 0.0 for k in range(K)])
    c = np.array([s[:n - k] @ e[k:] if k < n else 0.0 for k in range(K)])
    return r, c, float(e @ e), e, s


def project(est, clean, K: int, load_diag: float = 0.0):
    """(tgt, ee, h (K,), e, s): h = (Toeplitz(r) + load_diag r[0] I)^-1 c by a dense solve, tgt = c . h"""
    r, c, ee, e, s = correlations(est, clean, K)
    idx = np.abs(np.arange(K)[:, None] - np.arange(K)[None, :])
    R = r[idx] + load_diag * r[0] * np.eye(K)
    cond = np.linalg.cond(R)
    assert cond <= COND_MAX, f"cond(R) = {cond:.2e}: not an input for this reference"
    h = np.linalg.solve(R, c)
    resid = np.linalg.norm(R @ h - c)
    assert resid <= RESID_MAX * np.linalg.norm(c), f"|R h - c| = {resid:.2e} of |c| = {np.linalg.norm(c):.2e}"
    return float(c @ h), ee, h, e, s


def sdr(est, clean, K: int, load_diag: float = 0.0):
    """(sdr in dB, h (K,)) of one utterance: est (Le,), clean (Ls,)"""
    tgt, ee, h, _, _ = project(est, clean, K, load_diag)
    return 10.0 * np.log10(tgt / max(ee - tgt, 0.0)), h


def sdr_loss(est, clean, K: int, load_diag: float = 0.0, eps: float = 0.0):
    """(loss, grad (Le,)) in float64: loss = -K10 [ln(tgt + eps) - ln(res + eps)], grad = a e + c p with p = h * s"""
    tgt, ee, h, e, s = project(est, clean, K, load_diag)
    res = max(ee - tgt, 0.0)
    loss = -K10 * (np.log(tgt + eps) - np.log(res + eps))
    p = np.convolve(s, h)[:e.shape[0]]
    a, c = 2.0 * K10 / (res + eps), -2.0 * K10 * (1.0 / (tgt + eps) + 1.0 / (res + eps))
    return float(loss), (a * e + c * p)[:est.shape[0]]


# The rows of the device and host-emulation tests: (est, clean) samples in rows of WIDTH -- one sample of estimate; across the
# boundary of a 4096-sample span, the estimate the longer; three spans and a tail -- and the filter lengths: below, at and above a
# wave of 64, and above one lag per lane of 256.
WIDTH = 12544
LENGTHS = ((1, 5000), (4097, 4096), (12517, 12000))
FILTERS = (1, 2, 63, 64, 257, 512)
SIGMA = 8.0                                   # a moderate SDR (about 10 dB at 64 taps and more)
SIGMA_HIGH = 0.02                             # above 30 dB: e and its projection cancel in the gradient
H_BOUND = 100 * 4e-12                         # |h - h_ref| / |h_ref|: 100 x what a float64 Levinson differs from the dense solve
_CACHE: dict = {}


def rows():
    """the three seeded (est, clean) fp32 pairs of LENGTHS"""
    if "rows" not in _CACHE:
        _CACHE["rows"] = [make_pair(le, ls, 70 + k, SIGMA) for k, (le, ls) in enumerate(LENGTHS)]
    return _CACHE["rows"]


def high_row():
    """(est of 6000, clean of 5900 samples: clean * g ends inside est) whose SDR exceeds 30 dB from 40 taps on"""
    if "high" not in _CACHE:
        _CACHE["high"] = make_pair(6000, 5900, 77, SIGMA_HIGH)
    return _CACHE["high"]


def cached(name: str, idx, K: int, load_diag: float = 0.0, eps: float = 0.0):
    """``sdr`` (name "sdr") or ``sdr_loss`` ("loss") of rows()[idx] (idx "high": high_row()), computed once per process"""
    key = (name, idx, K, load_diag, eps)
    if key not in _CACHE:
        e, s = high_row() if idx == "high" else rows()[idx]
        _CACHE[key] = sdr(e, s, K, load_diag) if name == "sdr" else sdr_loss(e, s, K, load_diag, eps)
    return _CACHE[key]
