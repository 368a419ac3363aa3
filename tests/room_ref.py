"""The image-source room simulation of DESIGN.md 4.18 in float64 numpy: the reference of tests/test_room_ref.py and
tests/test_room_gpu.py, written from the definition (not from eabnet_amd/simulate.py or csrc/room.hip).  A scene is any object
with the fields of eabnet_amd.simulate.Scene."""
import math

import numpy as np
from scipy.signal import fftconvolve

C = 343.0
EPS = 2.0 ** -52
TAPS = 81


def inverse_sabine(rt60, Lr):
    Lx, Ly, Lz = Lr
    V = Lx * Ly * Lz
    A = 2.0 * (Lx * Ly + Ly * Lz + Lx * Lz)
    a = 24.0 * math.log(10.0) * V / (C * A * rt60)
    if a > 1.0:
        raise ValueError("room too large for this rt60")
    return a, int(math.ceil(C * rt60 / min(Lr) - 1.0))


def images(Lr, O, src):
    """(n (N, 3) int, position (N, 3)) of every image with |nx|+|ny|+|nz| <= O"""
    r = np.arange(-O, O + 1)
    n = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    n = n[np.abs(n).sum(1) <= O]
    Lr = np.asarray(Lr, dtype=np.float64)
    src = np.asarray(src, dtype=np.float64)
    pos = np.where(n % 2 == 0, n * Lr + src, (n + 1) * Lr - src)
    return n, pos


def image_pulses(Lr, a, O, fs, src, mic):
    """per image: (n, k0, f, g)"""
    n, pos = images(Lr, O, src)
    diff = pos - np.asarray(mic, dtype=np.float64)
    d = np.sqrt(diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2])
    g = (1.0 - a) ** (np.abs(n).sum(1) / 2.0) / (4.0 * np.pi * d)
    tau = d * fs / C
    k0 = np.floor(tau).astype(np.int64)
    return n, k0, tau - k0, g


def add_pulses(h, k0, f, g, chunk=65536):
    i = np.arange(TAPS, dtype=np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / 80.0)
    for c in range(0, len(k0), chunk):
        kk, ff, gg = k0[c:c + chunk], f[c:c + chunk], g[c:c + chunk]
        taps = gg[:, None] * win[None, :] * np.sinc(i[None, :] - 40.0 - ff[:, None])
        idx = kk[:, None] + np.arange(TAPS)[None, :]
        ok = idx < len(h)
        np.add.at(h, idx[ok], taps[ok])
    return h


def rir(Lr, a, O, fs, src, mic, K):
    _, k0, f, g = image_pulses(Lr, a, O, fs, src, mic)
    return add_pulses(np.zeros(K, dtype=np.float64), k0, f, g)


def rir_length(Lr, O, fs):
    far = max(math.sqrt(sum(((O + 1) * Lr[k]) ** 2 if k == ax else Lr[k] ** 2 for k in range(3))) for ax in range(3))
    return int(math.floor(fs / C * far)) + TAPS


def scene_rirs(sc, K=None):
    """(S, M + 1, K): row M the free-field response of the reference microphone"""
    K = rir_length(sc.room_dim, sc.max_order, sc.fs) if K is None else K
    src, mic = np.asarray(sc.sources, dtype=np.float64), np.asarray(sc.mics, dtype=np.float64)
    h = np.zeros((len(src), len(mic) + 1, K))
    for s in range(len(src)):
        for m in range(len(mic)):
            h[s, m] = rir(sc.room_dim, sc.absorption, sc.max_order, float(sc.fs), src[s], mic[m], K)
        h[s, len(mic)] = rir(sc.room_dim, 1.0, 0, float(sc.fs), src[s], mic[sc.ref_mic], K)
    return h


def active_rms(x, fs):
    W = int(fs / 10)
    total, count = 0.0, 0
    for t0 in range(0, len(x), W):
        w = x[t0:t0 + W]
        if math.sqrt(float((w * w).mean())) > 10.0 ** (-50.0 / 20.0):
            total += float((w * w).sum())
            count += len(w)
    return math.sqrt(total / count) if count else EPS


def dry_gains(xs, snr, dBFS, fs):
    """xs: the S dry sources (float64, one length) -> the S gains"""
    peak = [float(np.abs(x).max()) for x in xs]
    xn = [x / (p + EPS) for x, p in zip(xs, peak)]
    rms_clean = math.sqrt(float((xn[0] * xn[0]).mean()))
    q = [1.0] + [rms_clean / 10.0 ** (s / 20.0) / (active_rms(x, fs) + EPS) for x, s in zip(xn[1:], snr)]
    mix = sum(qj * x for qj, x in zip(q, xn))
    G = 10.0 ** (dBFS / 20.0) / (math.sqrt(float((mix * mix).mean())) + EPS)
    return np.array([G * qj / (p + EPS) for qj, p in zip(q, peak)])


def simulate(sc, xs, h=None):
    """xs (S, L) -> noisy (M, L), clean (L,), gains (S,)"""
    xs = np.asarray(xs, dtype=np.float64)
    S, L = xs.shape
    h = scene_rirs(sc) if h is None else h
    M = h.shape[1] - 1
    gains = dry_gains(list(xs), list(sc.snr), sc.dBFS, float(sc.fs))
    noisy = np.zeros((M, L))
    for m in range(M):
        for s in range(S):
            noisy[m] += gains[s] * fftconvolve(xs[s], h[s, m])[:L]
    clean = gains[0] * fftconvolve(xs[0], h[0, M])[:L]
    return noisy, clean, gains
