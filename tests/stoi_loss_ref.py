"""Shared by the ``stoi_loss`` tests: ``stoi_ref.analyse`` restated in torch under autograd (float64, or float32 for the rounding
floor of the definition itself), written from DESIGN §4.16 rules 2-10 and the three gradient conventions of §4.22, not from the
kernels:

  rule 4   the kept-frame set comes from ``clean`` alone: K, kept and T are constants of the gradient;
  rule 6   a band value Y[i, t] == 0 contributes zero gradient (a guarded sqrt);
  rule 9   element-wise, ``alpha * Y <= bound`` takes the ``alpha * Y`` branch and alpha is differentiated; otherwise the element
           contributes nothing through Y (``torch.where``).  The EPS terms are differentiated as written, a norm that is exactly
           zero contributes zero (the same guarded sqrt).

``misreading=`` swaps in one of four wrong gradients with the SAME value (tests/test_stoi_loss_ref.py shows that each moves the
gradient by far more than the GPU bar).  Also the float64 adjoint of the resampler, from the explicit matrix of
``resample_ref.ref_resample`` and as a differentiable torch restatement of the same sum (for the 16 kHz chain)."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import resample_ref
import stoi_ref as R

CLIP = 1.0 + 10.0 ** (-R.BETA / 20.0)
MISREADINGS = ("alpha_constant", "clip_ignored", "second_window_dropped", "mask_from_est")
# the gradient cases at 10 kHz (indices into stoi_ref.CASES): every element's |alpha Y - bound| / bound > 1e-4 and every frame
# >= 0.05 dB from the removal threshold (asserted by tests/test_stoi_loss_ref.py); 708 misses the first and serves values only
GRAD_CASES = (0, 3, 4, 5, 6, 7, 9)
SENTINEL_CASES = (1, 2)
# est much shorter than clean: whole band frames of est are exactly zero (rule 6's convention is exercised on every tail frame)
SHORT_EST_CASE = (9000, 6000, 711, 0.3, 0.1, ((4000, 5200, 1e-4),))
CLIP_MARGIN = 1e-4
FRAME_MARGIN_DB = 0.05


def _sqrt0(v):
    """sqrt with derivative 0 at 0"""
    pos = v > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, v, torch.ones_like(v))), torch.zeros_like(v))


def _norm(a, dim):
    return _sqrt0((a * a).sum(dim=dim, keepdim=True))


def _starts(L):
    last = L - R.N_FRAME - 1
    return np.arange(0, last + 1, R.HOP) if last >= 0 else np.zeros(0, np.int64)


def _rows_norm(a, dim):
    a = a - a.mean(dim=dim, keepdim=True)
    return a / (_norm(a, dim) + R.EPS)


def _bands(sig, kept, w, dtype, drop_second_window=False):
    """(15, T) band values of one zero-extended signal (torch, (n,)) for the kept source frames"""
    K = len(kept)
    idx = torch.from_numpy(_starts(sig.shape[0])[:, None] + np.arange(R.N_FRAME)[None, :])
    fr = w[None, :] * sig[idx]                                                   # rule 3
    pos = torch.from_numpy((np.arange(K) * R.HOP)[:, None] + np.arange(R.N_FRAME)[None, :]).reshape(-1)
    sil = torch.zeros((K - 1) * R.HOP + R.N_FRAME, dtype=dtype).index_add(0, pos, fr[torch.from_numpy(kept)].reshape(-1))
    idx2 = torch.from_numpy(_starts(sil.shape[0])[:, None] + np.arange(R.N_FRAME)[None, :])
    s2 = sil[idx2]
    c = w[None, :] * s2                                                          # rule 5: windowed again
    if drop_second_window:                                                       # (the value of w s, the gradient of s)
        c = c.detach() + (s2 - s2.detach())
    spec = torch.fft.rfft(c, R.NFFT, dim=1)
    P = spec.real ** 2 + spec.imag ** 2
    return torch.stack([_sqrt0(P[:, lo:hi].sum(dim=1)) for lo, hi in R.BANDS])  # rule 6


def scores(clean, est, dtype=torch.float64, misreading=None):
    """clean: (Ls,) array (a constant); est: (Le,) torch tensor of ``dtype`` (may require grad), both at 10 kHz -> dict with the
    torch scalars ``stoi`` and ``estoi`` and, as numbers, ``K``, ``T``, ``frame_margin`` (dB), ``clip_margin`` (the smallest
    |alpha Y - bound| / bound over all elements of all segments) and ``zero_bands`` (band values of est that are exactly 0)"""
    assert misreading is None or misreading in MISREADINGS
    clean = np.asarray(clean, np.float64)
    n = max(clean.shape[0], est.shape[0])
    x = np.zeros(n)
    x[:clean.shape[0]] = clean
    y = torch.cat([est, torch.zeros(n - est.shape[0], dtype=dtype)])
    wn = R.window()
    w = torch.from_numpy(wn).to(dtype)
    sentinel = torch.tensor(R.SENTINEL, dtype=dtype) + 0.0 * est.sum()           # (a zero gradient, not None)
    out = {"stoi": sentinel, "estoi": sentinel, "K": 0, "T": 0, "frame_margin": math.inf, "clip_margin": math.inf,
           "zero_bands": 0}
    src = y.detach().numpy().astype(np.float64) if misreading == "mask_from_est" else x
    xf = R._frames(src, wn)
    if xf.shape[0] == 0:
        return out
    e = 20.0 * np.log10(np.linalg.norm(xf, axis=1) + R.EPS)                      # rule 4, from constants
    d = np.max(e) - R.DYN_RANGE - e
    kept = np.nonzero(d < 0)[0]
    K = kept.shape[0]
    out.update(K=K, T=K - 1, frame_margin=float(np.abs(d).min()))
    X = _bands(torch.from_numpy(x).to(dtype), kept, w, dtype)
    Y = _bands(y, kept, w, dtype, misreading == "second_window_dropped")
    T = K - 1
    out["zero_bands"] = int((Y == 0).sum())
    if T < R.N_SEG:
        return out
    S = T - R.N_SEG + 1
    Xs, Ys = X.unfold(1, R.N_SEG, 1).permute(1, 0, 2), Y.unfold(1, R.N_SEG, 1).permute(1, 0, 2)      # (S, 15, 30)
    alpha = _norm(Xs, 2) / (_norm(Ys, 2) + R.EPS)                                # rule 9
    if misreading == "alpha_constant":
        alpha = alpha.detach()
    bound = CLIP * Xs
    ay = alpha * Ys
    Yp = torch.where(ay <= bound, ay, bound)
    if misreading == "clip_ignored":
        Yp = Yp.detach() + (ay - ay.detach())
    with torch.no_grad():
        rel = torch.where(bound > 0, (ay - bound).abs() / torch.where(bound > 0, bound, torch.ones_like(bound)),
                          torch.full_like(bound, math.inf))
        out["clip_margin"] = float(rel.min())
    out["stoi"] = (_rows_norm(Xs, 2) * _rows_norm(Yp, 2)).sum() / (R.J_BANDS * S)
    both = lambda a: _rows_norm(_rows_norm(a, 2), 1)                             # noqa: E731  rule 10: rows, then columns
    out["estoi"] = (both(Xs) * both(Ys)).sum() / (R.N_SEG * S)
    return out


def loss_and_grad(clean, est, factor_stoi=1.0, factor_estoi=0.0, dtype=torch.float64, misreading=None):
    """(loss, d loss / d est (Le,) float64 array, info) of loss = -(factor_stoi stoi + factor_estoi estoi) for one 10 kHz pair"""
    e = torch.from_numpy(np.asarray(est, np.float64)).to(dtype).requires_grad_(True)
    info = scores(clean, e, dtype, misreading)
    loss = -(factor_stoi * info["stoi"] + factor_estoi * info["estoi"])
    loss.backward()
    info["stoi"], info["estoi"] = info["stoi"].detach(), info["estoi"].detach()
    return float(loss.detach()), e.grad.numpy().astype(np.float64), info


# --- the resampler -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=16)
def resample_matrix(L, orig, new):
    """the operator of resample_ref.ref_resample on rows of L samples as an explicit (n_out, L) float64 matrix"""
    return np.ascontiguousarray(resample_ref.ref_resample(np.eye(L), orig, new).T)


def resample_adjoint(g, L, orig, new, length=None):
    """R^T g for a row of L samples of which ``length`` are the signal: zero past ``length``, and outputs past ceil(n length / o)
    carry no gradient"""
    length = L if length is None else length
    g = np.asarray(g, np.float64)
    out = np.zeros(L)
    if length:
        M = resample_matrix(length, orig, new)
        out[:length] = M.T @ g[:M.shape[0]]
    return out


def torch_resample(x, orig, new, lw=6, rolloff=0.99):
    """resample_ref._sums as differentiable torch float64: (..., L) -> (..., ceil(n L / o))"""
    o, n = resample_ref.ratio(orig, new)
    L = x.shape[-1]
    n_out = -(-n * L // o)
    i = np.arange(n_out, dtype=np.int64)
    q, p = i // n, i % n
    base = rolloff * min(o, n)
    reach = int(math.ceil(lw * o / base)) + 1
    centre = (p * o) // n
    y = torch.zeros(x.shape[:-1] + (n_out,), dtype=x.dtype)
    for d in range(-reach - 1, reach + 2):
        m = centre + d
        wv = resample_ref.h((m * n - p * o) / float(o * n), o, n, "hann", lw, rolloff)
        j = q * o + m
        ok = (j >= 0) & (j < L)
        y = y + torch.from_numpy(wv * ok).to(x.dtype) * x[..., torch.from_numpy(np.clip(j, 0, max(L - 1, 0)))]
    return y


# --- the 16 kHz chain: a leaf spectrum through the ISTFT, the resampler and the loss --------------------------------------------------
CHAIN = dict(B=2, T=48, n_fft=320, hop=160, seed=730, extra=32)          # clean is `extra` samples longer than the ISTFT's wave


def chain_case():
    """(spectrum (B, 2, T, F) fp32, clean (B, L + extra) fp32) of the chain tests, seeded"""
    c = CHAIN
    rng = np.random.default_rng(c["seed"])
    spec = rng.standard_normal((c["B"], 2, c["T"], c["n_fft"] // 2 + 1)).astype(np.float32)
    wav = chain_wave64(torch.from_numpy(spec).double()).numpy()
    L = wav.shape[1]
    clean = np.zeros((c["B"], L + c["extra"]))
    clean[:, :L] = 0.8 * wav
    clean += 0.3 * wav.std() * rng.standard_normal(clean.shape)
    return spec, clean.astype(np.float32)


def chain_wave64(x):
    c = CHAIN
    window = torch.hann_window(c["n_fft"], dtype=torch.float64)
    return torch.istft(torch.view_as_complex(x.permute(0, 3, 2, 1).contiguous()), c["n_fft"], c["hop"], c["n_fft"], window)


def chain_loss64(x, clean, factor_stoi, factor_estoi, rate=16000):
    """(mean loss as a torch float64 scalar, [info per row]) of spectrum x (float64, may require grad) against clean (B, Ls)"""
    wav = chain_wave64(x)
    est10 = torch_resample(wav, rate, R.FS)
    clean10 = resample_ref.ref_resample(np.asarray(clean, np.float64), rate, R.FS)
    infos = [scores(clean10[b], est10[b]) for b in range(wav.shape[0])]
    loss = torch.stack([-(factor_stoi * i["stoi"] + factor_estoi * i["estoi"]) for i in infos]).mean()
    return loss, infos
