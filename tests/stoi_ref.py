"""Shared by the intelligibility tests: seeded cases (clean, estimate) at 10 kHz and a float64 numpy restatement of STOI (Taal
et al. 2011) and ESTOI (Jensen & Taal 2016), written from the definition in DESIGN §4.16, not from the kernels.  The definition is
the contract: equality with any host STOI library is NOT verified (none is installed where this suite runs).
tests/test_stoi_ref.py pins the restatement to recorded values and to the invariants of the definition, so GPU tests may use it
at any shape."""
from __future__ import annotations

import numpy as np

import paramgen

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
J_BANDS = 15
MIN_FREQ = 150
N_SEG = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = 2.0 ** -52
SENTINEL = 1e-5

# rule 6 as a literal list: band i sums the bins [lo, hi)
BANDS = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219)]

# (Ls, Le, seed, g_n, g_a, gaps), every gap (start, stop, gain); the recorded (frames, kept, stoi, estoi) are in EXPECTED
CASES = [
    (4097, 4097, 700, 0.3, 0.1, ()),                                                       # 31 frames, one segment
    (4096, 4096, 701, 0.3, 0.1, ()),                                                       # 30 frames, T = 29: too short
    (256, 256, 702, 0.3, 0.1, ()),                                                         # no frame
    (4224, 4100, 703, 0.3, 0.1, ()),                                                       # est shorter
    (9000, 9000, 704, 0.3, 0.1, ((0, 1500, 1e-4), (4000, 5200, 1e-4), (8000, 9000, 1e-4))),   # removal at start, middle, end
    (9000, 9000, 705, 0.3, 0.1, ((0, 1500, 1e-4), (3000, 6500, 1e-4))),
    (20003, 19840, 706, 1.0, 0.3, ((2500, 4100, 1e-4), (9000, 9700, 3e-2), (15000, 16500, 1e-3))),   # odd, several frame tiles
    (12000, 15000, 707, 0.3, 0.1, ((5000, 5600, 1e-4),)),                                  # clean shorter: its zero tail goes
    (60000, 59840, 708, 3.0, 0.5, ((7000, 9000, 1e-4), (30000, 30300, 1e-4), (45000, 52000, 2e-2))),   # six seconds, low scores
    (9000, 9000, 709, 0.02, 3.0, ((4000, 5200, 1e-4),)),                                   # artefact-dominated
]
EXPECTED = [
    (31, 31, 0.911538, 0.741005),
    (30, 30, 1e-5, 1e-5),
    (0, 0, 1e-5, 1e-5),
    (31, 31, 0.927959, 0.770036),
    (69, 47, 0.940746, 0.759761),
    (69, 35, 0.937576, 0.722674),
    (155, 136, 0.610687, 0.300211),
    (116, 92, 0.932589, 0.741843),
    (467, 427, 0.234073, 0.107041),
    (69, 62, 0.596177, 0.547067),
]


def make_case(Ls, Le, seed, g_n, g_a, gaps):
    """fp32 (clean (Ls,), estimate (Le,)): a seeded source with a slow amplitude modulation and near-silent gaps (so that
    frames are removed), plus noise and an artefact that follows the clean signal's sign"""
    n = max(Ls, Le)
    s, noise, art = (paramgen.make_wave(1, 1, n, 3 * seed + k)[0, 0].astype(np.float64) for k in range(3))
    t = np.arange(n, dtype=np.float64)
    env = np.ones(n)
    for start, stop, gain in gaps:
        env *= gain ** np.clip(np.minimum(t - start, stop - t) / 200.0, 0.0, 1.0)
    s = s * env * (0.6 + 0.4 * np.sin(2.0 * np.pi * t / 1700.0))
    ext = np.zeros(n)
    ext[:Ls] = s[:Ls]
    est = (ext + g_n * noise + g_a * np.abs(art) * np.sign(ext))[:Le]
    return ext[:Ls].astype(np.float32), est.astype(np.float32)


def window(n_frame=N_FRAME):
    """rule 2: the inner points of a symmetric Hann window of n_frame + 2 points"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(n_frame) + 1.0) / (n_frame + 1.0))


def derive_bands():
    """rule 6 from the frequency formula: the edges 150 * 2^((2i -+ 1)/6) at the nearest bin, ties to the lowest index"""
    f = np.arange(NFFT // 2 + 1) * (FS / NFFT)
    out = []
    for i in range(J_BANDS):
        lo = MIN_FREQ * 2.0 ** ((2 * i - 1) / 6.0)
        hi = MIN_FREQ * 2.0 ** ((2 * i + 1) / 6.0)
        out.append((int(np.argmin((f - lo) ** 2)), int(np.argmin((f - hi) ** 2))))
    return out


def _frames(sig, w, strict=True):
    """rule 3: (count, 256) windowed frames starting at 0, 128, .. while start + 256 < len (strict) or <= len"""
    L = sig.shape[0]
    last = L - N_FRAME - (1 if strict else 0)
    starts = np.arange(0, last + 1, HOP) if last >= 0 else np.zeros(0, np.int64)
    if starts.size == 0:
        return np.zeros((0, N_FRAME))
    return w[None, :] * sig[starts[:, None] + np.arange(N_FRAME)[None, :]]


def _rows_norm(a):
    a = a - a.mean(axis=-1, keepdims=True)
    return a / (np.linalg.norm(a, axis=-1, keepdims=True) + EPS)


def analyse(clean, est, w=None, bands=None, strict=True):
    """everything the tests look at, float64: dict with frames, K, kept (source frame of every compacted frame), margin (the
    smallest |max e - 40 - e_j|, dB), tob (2, 15, T) band values of (clean, estimate), stoi, estoi, clipped (share of the
    elements on which rule 9's bound binds)"""
    w = window() if w is None else np.asarray(w, np.float64)
    bands = BANDS if bands is None else bands
    n = max(clean.shape[0], est.shape[0])
    x, y = np.zeros(n), np.zeros(n)
    x[:clean.shape[0]] = clean
    y[:est.shape[0]] = est
    xf, yf = _frames(x, w, strict), _frames(y, w, strict)
    out = {"frames": xf.shape[0], "K": 0, "kept": np.zeros(0, np.int64), "margin": np.inf, "tob": np.zeros((2, J_BANDS, 0)),
           "stoi": SENTINEL, "estoi": SENTINEL, "clipped": 0.0}
    if xf.shape[0] == 0:
        return out
    e = 20.0 * np.log10(np.linalg.norm(xf, axis=1) + EPS)                      # rule 4
    d = np.max(e) - DYN_RANGE - e
    kept = np.nonzero(d < 0)[0]
    K = kept.shape[0]
    out.update(K=K, kept=kept, margin=float(np.abs(d).min()))
    tob = []
    for fr in (xf, yf):
        sil = np.zeros((K - 1) * HOP + N_FRAME)
        for t, j in enumerate(kept):                                           # overlap-add of the kept windowed frames
            sil[t * HOP:t * HOP + N_FRAME] += fr[j]
        spec = np.fft.rfft(_frames(sil, w, strict), NFFT, axis=1)              # rule 5: windowed again, padded to 512
        P = np.abs(spec) ** 2
        tob.append(np.stack([np.sqrt(P[:, lo:hi].sum(axis=1)) for lo, hi in bands]))
    X, Y = tob
    T = X.shape[1]
    out["tob"] = np.stack([X, Y])
    if T < N_SEG:
        return out
    S = T - N_SEG + 1
    idx = np.arange(S)[:, None] + np.arange(N_SEG)[None, :]
    Xs, Ys = X[:, idx].transpose(1, 0, 2), Y[:, idx].transpose(1, 0, 2)        # (S, 15, 30)
    # rule 9
    alpha = np.linalg.norm(Xs, axis=2, keepdims=True) / (np.linalg.norm(Ys, axis=2, keepdims=True) + EPS)
    bound = (1.0 + 10.0 ** (-BETA / 20.0)) * Xs
    Yp = np.minimum(alpha * Ys, bound)
    out["clipped"] = float(np.mean(alpha * Ys > bound))
    out["stoi"] = float(np.sum(_rows_norm(Xs) * _rows_norm(Yp)) / (J_BANDS * S))
    # rule 10: rows, then columns
    def both(a):
        a = _rows_norm(a)
        a = a - a.mean(axis=1, keepdims=True)
        return a / (np.linalg.norm(a, axis=1, keepdims=True) + EPS)
    out["estoi"] = float(np.sum(both(Xs) * both(Ys)) / (N_SEG * S))
    return out


def intelligibility(est, clean, **kw):
    """[stoi, estoi] of one 10 kHz pair, float64 (argument order of eabnet_amd.intelligibility)"""
    a = analyse(np.asarray(clean, np.float64), np.asarray(est, np.float64), **kw)
    return np.array([a["stoi"], a["estoi"]])
