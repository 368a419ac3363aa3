"""The resampler's definition in float64 numpy, written from the formula and NOT through ``eabnet_amd.resample.filter_bank``:

    o = orig/gcd, n = new/gcd, base = rolloff * min(o, n)
    h(t) = (base/o) sinc(base t) w(base t)  for |base t| < lw, else 0
    y[q*n + p] = sum_m h(m/o - p/n) x[q*o + m],   x = 0 outside [0, L),   0 <= q*n + p < ceil(n L / o)

``ref_resample`` is that sum; ``ref_abs`` the same sum over |h| |x| (the scale of the fp32 rounding bound of the tests).  The
loop over m is explicit (every m that can lie inside the support, tested against |base t| < lw one by one); the outputs of a
row -- and the rows of a batch -- go through it as one numpy vector."""
import math

import numpy as np

BETA = 14.769656459379492


def window_value(u, lw, window):
    if window == "hann":
        return np.cos(np.pi * u / (2.0 * lw)) ** 2
    if window == "kaiser":
        return np.i0(BETA * np.sqrt(np.maximum(1.0 - (u / lw) ** 2, 0.0))) / np.i0(BETA)
    raise ValueError(window)


def h(t, o, n, window="hann", lw=6, rolloff=0.99):
    """the continuous prototype at times t (float64 array)"""
    base = rolloff * min(o, n)
    u = base * np.asarray(t, dtype=np.float64)
    inside = np.abs(u) < lw
    u = np.where(inside, u, 0.0)
    return np.where(inside, (base / o) * np.sinc(u) * window_value(u, float(lw), window), 0.0)


def ratio(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def out_length(L, orig, new):
    o, n = ratio(orig, new)
    return -(-n * L // o)


def _sums(x, orig, new, window, lw, rolloff):
    x = np.asarray(x, dtype=np.float64)
    o, n = ratio(orig, new)
    L = x.shape[-1]
    n_out = -(-n * L // o)
    i = np.arange(n_out, dtype=np.int64)
    q, p = i // n, i % n
    base = rolloff * min(o, n)
    reach = int(math.ceil(lw * o / base)) + 1                  # |m - o p / n| < lw o / base
    centre = (p * o) // n
    y = np.zeros(x.shape[:-1] + (n_out,))
    ya = np.zeros_like(y)
    for d in range(-reach - 1, reach + 2):
        m = centre + d
        w = h((m * n - p * o) / float(o * n), o, n, window, lw, rolloff)
        j = q * o + m
        ok = (j >= 0) & (j < L)
        xv = np.where(ok, x[..., np.clip(j, 0, max(L - 1, 0))], 0.0) if L else 0.0
        y += w * xv
        ya += np.abs(w) * np.abs(xv)
    return y, ya


def ref_resample(x, orig, new, window="hann", lw=6, rolloff=0.99):
    return _sums(x, orig, new, window, lw, rolloff)[0]


def ref_abs(x, orig, new, window="hann", lw=6, rolloff=0.99):
    return _sums(x, orig, new, window, lw, rolloff)[1]


def upfirdn_resample(x, orig, new, window="hann", lw=6, rolloff=0.99):
    """the same through scipy.signal.upfirdn: hp[k] = h((k - W)/(o n)), W = ceil(lw o n / base), read at W + i o"""
    from scipy.signal import upfirdn
    x = np.asarray(x, dtype=np.float64)
    o, n = ratio(orig, new)
    base = rolloff * min(o, n)
    W = int(math.ceil(lw * o * n / base))
    hp = h((np.arange(2 * W + 1) - W) / float(o * n), o, n, window, lw, rolloff)
    full = upfirdn(hp, x, up=n)
    n_out = -(-n * x.shape[-1] // o)
    pos = W + np.arange(n_out) * o
    full = np.concatenate([full, np.zeros(max(0, pos.max() + 1 - full.shape[-1]) if n_out else 0)])
    return full[pos]
