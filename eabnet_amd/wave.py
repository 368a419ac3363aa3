"""Train on the waveform: ``si_sdr_loss``, the negative SI-SDR that ``Scorer`` and ``energy_ratios`` report per file
(reference metrics.py:71-75), as a loss with a gradient -- csrc/wave_loss.hip behind tensor arguments.  With the differentiable
``istft`` the end of a training step reads

    wav = istft(out["esti_stft"], 320, 160, window)
    loss = l["final"] + w * si_sdr_loss(wav, target, eps=1e-8)
    loss.backward()

Two launches for the value, one for the gradient; ``grad_output`` is read on the device, nothing synchronises with the host.

``mr_stft_loss`` is the spectral half of a waveform objective -- spectral convergence plus log-magnitude distance at several
time-frequency resolutions, csrc/spec_loss.hip -- added the same way: ``loss = loss + v * mr_stft_loss(wav, target)``.

``stoi_loss`` trains for the two intelligibility scores ``Scorer(model, intelligibility=True)`` reports: minus a weighted sum of
STOI and ESTOI, the value by the launches of ``intelligibility`` and the gradient by three more on the workspace they leave
(csrc/stoi_bwd.hip); at 16 kHz it chains through the differentiable ``resample``.

``sdr_loss`` is ``si_sdr_loss`` with a filter of up to 512 taps between the clean wave and the estimate -- minus the SDR of
BSS-eval that ``sdr`` reports (csrc/sdr.hip) -- for targets that are a delayed or lightly filtered copy of what
the array should deliver, where the one-tap loss and its gradient say nothing."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from . import _rows as _rw
from . import model as _m
from .score import STOI_RATE, _sdr_rows, check_sdr_filter

REDUCTIONS = ("mean", "sum", "none")


class _SiSdrLoss(torch.autograd.Function):
    """value: eab_si_sdr_loss_f32 leaves (loss_b, a_b, c_b) per utterance; backward: eab_si_sdr_loss_bwd_f32 writes
    g_b (a_b e + c_b s) from grad_output on the device"""

    @staticmethod
    def forward(ctx, est: torch.Tensor, clean: torch.Tensor, lens: torch.Tensor, eps: float, reduction: str) -> torch.Tensor:
        lib = _lib.load()
        B = est.shape[0]
        e, s = est.detach(), clean
        with torch.cuda.device(e.device):
            spans = _rw.spans(max(e.shape[1], s.shape[1]))
            partial = torch.empty((B, spans, 3), dtype=torch.float64, device=e.device)
            coef = torch.empty((B, 3), dtype=torch.float64, device=e.device)
            loss = torch.empty((B,), dtype=torch.float32, device=e.device)
            total = torch.empty((2,), dtype=torch.float32, device=e.device)
            _lib.check(lib.eab_si_sdr_loss_f32(*_rw.row_args(B, e, s), lens.data_ptr(), B, float(eps), partial.data_ptr(), spans,
                                               coef.data_ptr(), loss.data_ptr(), total.data_ptr(), _rw.stream()), "eab_si_sdr_loss_f32")
        ctx.save_for_backward(e, s, lens, coef)
        ctx.reduction = reduction
        return loss if reduction == "none" else total[0 if reduction == "sum" else 1]

    @staticmethod
    def backward(ctx, g):
        e, s, lens, coef = ctx.saved_tensors
        lib = _lib.load()
        B, L = e.shape
        g, gstride, scale = _rw.grad_row(g, B, ctx.reduction)
        grad = torch.empty((B, L), dtype=torch.float32, device=e.device)
        with torch.cuda.device(e.device):
            _lib.check(lib.eab_si_sdr_loss_bwd_f32(*_rw.row_args(B, e, s), lens.data_ptr(), B, coef.data_ptr(), g.data_ptr(), gstride,
                                                   scale, grad.data_ptr(), L, _rw.stream()), "eab_si_sdr_loss_bwd_f32")
        return grad, None, None, None, None


def si_sdr_loss(est: torch.Tensor, clean: torch.Tensor, lengths=None, eps: float = 0.0, reduction: str = "mean") -> torch.Tensor:
    """Negative SI-SDR in dB of B utterances, differentiable with respect to ``est``: est (B, Le), clean (B, Ls) or (B, 1, Ls) (what
    the loader and ``RoomSimulator`` yield), CUDA fp32 -> an fp32 scalar (``reduction`` "mean" or "sum") or (B,) ("none").

        loss_b = -10 log10( (|alpha s|^2 + eps) / (|e - alpha s|^2 + eps) ),   alpha = <e,s> / <s,s>

    With ``eps=0`` loss_b is minus the ``si_sdr`` column of ``energy_ratios`` on the same rows; a silent clean row gives NaN in its
    own value.  lengths: None (the full rows), (B,) sample counts for both signals, or (B, 2) pairs (est, clean) -- sequences or
    integer tensors, host or device, checked as ``energy_ratios`` checks its lengths.  A signal counts as zero from its own length
    up to the longer of the two and is never read there; the gradient is exactly zero from est's length to the row's end.  Rows may
    be strided views whose last dimension is contiguous and are read in place.  Sums in fp64 in a fixed order: an utterance has the
    same bits alone and in any batch.  No operator fallback: CPU tensors, other dtypes and a ``clean`` that requires grad raise."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {REDUCTIONS}, got {reduction!r}")
    if not (isinstance(eps, (int, float)) and 0.0 <= float(eps) < float("inf")):
        raise ValueError(f"eps must be a finite number >= 0, got {eps!r}")
    clean, B = _rw.check_waves("si_sdr_loss", est, clean)
    cols = _rw.check_lens(lengths, B, (est.shape[1], clean.shape[1]))
    est_rows, clean_rows = _rw.device_rows("si_sdr_loss", est, clean)
    with torch.cuda.device(est.device):
        lens = _rw.device_lens(cols, B, est.device)
    return _SiSdrLoss.apply(est_rows, clean_rows, lens, float(eps), reduction)


class _SdrLoss(torch.autograd.Function):
    """value: eab_sdr_f32 leaves (sdr, tgt, ee, loss_b, a_b, c_b) and the filter h per utterance in fp64; backward:
    eab_sdr_loss_bwd_f32 writes g_b (a_b e + c_b h * s) from grad_output on the device"""

    @staticmethod
    def forward(ctx, est, clean, lens, K, load_diag, eps, reduction):
        B = est.shape[0]
        e, s = est.detach(), clean
        out, h = _sdr_rows(e, s, lens, K, load_diag, eps, True)
        with torch.cuda.device(e.device):
            loss = out[:, 3]
            if reduction != "none":
                loss = loss.sum()
                if reduction == "mean":
                    loss = loss / B
            loss = loss.to(torch.float32)
        ctx.save_for_backward(e, s, lens, out, h)
        ctx.cfg = (K, reduction)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        e, s, lens, coef, h = ctx.saved_tensors
        K, reduction = ctx.cfg
        lib = _lib.load()
        B, L = e.shape
        g, gstride, scale = _rw.grad_row(g, B, reduction)
        with torch.cuda.device(e.device):
            grad = torch.empty((B, L), dtype=torch.float32, device=e.device)
            _lib.check(lib.eab_sdr_loss_bwd_f32(*_rw.row_args(B, e, s), lens.data_ptr(), B, K, coef.data_ptr(), h.data_ptr(), g.data_ptr(),
                                                gstride, scale, grad.data_ptr(), L, _rw.stream()), "eab_sdr_loss_bwd_f32")
        return grad, None, None, None, None, None, None


def sdr_loss(est: torch.Tensor, clean: torch.Tensor, lengths=None, filter_length: int = 512, load_diag: float = 0.0, eps: float = 0.0,
             reduction: str = "mean") -> torch.Tensor:
    """Negative SDR of BSS-eval in dB of B utterances, differentiable with respect to ``est``: est (B, Le), clean (B, Ls) or
    (B, 1, Ls), CUDA fp32 -> an fp32 scalar (``reduction`` "mean" or "sum") or (B,) ("none").  With K = filter_length, r, c, R and
    h as in ``sdr``, tgt = c.h and res = max(|e|^2 - tgt, 0):

        loss_b = -10 log10( (tgt + eps) / (res + eps) )
        d loss_b / d e[n] = a_b e[n] + c_b (h * s)[n],   a_b = 2 k10 / (res + eps),  c_b = -2 k10 [1 / (tgt + eps) + 1 / (res + eps)]

    With ``eps=0`` loss_b is minus ``sdr`` on the same rows, and with ``filter_length=1`` every formula is that of
    ``si_sdr_loss``.  The filter h * s, the sums and a_b e + c_b (h * s) are fp64, rounded to fp32 once: e and its projection
    cancel at high SDR.  lengths, strided rows, the zero convention past a length and the exactly zero gradient from est's length
    to the row's end: as ``si_sdr_loss``.  A silent clean row, a clean row of fewer than K samples and a row whose recursion
    meets a prediction error <= 0 give NaN in their own value and their own gradient row only.  Every sum has one fixed order:
    an utterance has the same bits alone, in any batch and in a second call, value and gradient.  No double backward.  No
    operator fallback: CPU tensors, other dtypes and a ``clean`` that requires grad raise."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {REDUCTIONS}, got {reduction!r}")
    if not (isinstance(eps, (int, float)) and 0.0 <= float(eps) < float("inf")):
        raise ValueError(f"eps must be a finite number >= 0, got {eps!r}")
    K, load_diag = check_sdr_filter(filter_length, load_diag)
    clean, B = _rw.check_waves("sdr_loss", est, clean)
    cols = _rw.check_lens(lengths, B, (est.shape[1], clean.shape[1]))
    est_rows, clean_rows = _rw.device_rows("sdr_loss", est, clean)
    with torch.cuda.device(est.device):
        lens = _rw.device_lens(cols, B, est.device)
    return _SdrLoss.apply(est_rows, clean_rows, lens, K, load_diag, float(eps), reduction)


MR_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
MR_MAX_RESOLUTIONS = 8
MR_MAX_NFFT = 2048
MR_MAX_COVER = 8        # frames whose window support covers one sample: ceil(win / hop)
FFT_MAX_PASSES = 8
_MR_TABLES: dict = {}


def _fft_passes(n: int):
    """the passes csrc/fft_lds.h plans for an n-point transform (radix 5s, 4s, a trailing 8, 2s), or None where n has another
    prime factor or the plan runs out of passes"""
    passes = 0
    while n % 5 == 0 and passes < FFT_MAX_PASSES:
        n, passes = n // 5, passes + 1
    while n % 4 == 0 and n != 8 and passes < FFT_MAX_PASSES:
        n, passes = n // 4, passes + 1
    if n == 8:
        n, passes = 1, passes + 1
    while n % 2 == 0 and passes < FFT_MAX_PASSES:
        n, passes = n // 2, passes + 1
    return passes if n == 1 else None


def check_resolutions(resolutions) -> tuple:
    """``resolutions`` as a tuple of (n_fft, hop, win) integer triples the LDS transform can plan, or ValueError with the reason"""
    try:
        res = [tuple(r) for r in resolutions]
    except TypeError:
        raise ValueError(f"resolutions must be a sequence of (n_fft, hop, win) triples, got {resolutions!r}") from None
    if not 1 <= len(res) <= MR_MAX_RESOLUTIONS:
        raise ValueError(f"resolutions must hold 1 to {MR_MAX_RESOLUTIONS} (n_fft, hop, win) triples, got {len(res)}")
    for r in res:
        if len(r) != 3 or any(isinstance(v, bool) or not isinstance(v, int) for v in r):
            raise ValueError(f"a resolution is a triple of integers (n_fft, hop, win), got {r!r}")
        n_fft, hop, win = r
        if n_fft % 2 or not 8 <= n_fft <= MR_MAX_NFFT:
            raise ValueError(f"resolution {r}: n_fft must be even and lie in [8, {MR_MAX_NFFT}] (the transform runs in LDS)")
        if _fft_passes(n_fft // 2) is None:
            raise ValueError(f"resolution {r}: n_fft / 2 = {n_fft // 2} must be 2^a 5^b within {FFT_MAX_PASSES} passes "
                             "(the radices of the LDS transform)")
        if not 1 <= hop <= n_fft or not 1 <= win <= n_fft:
            raise ValueError(f"resolution {r}: hop and win must lie in [1, n_fft]")
        if -(-win // hop) > MR_MAX_COVER:
            raise ValueError(f"resolution {r}: at most {MR_MAX_COVER} windows may cover one sample (ceil(win / hop) = {-(-win // hop)})")
    return tuple(res)


def _mr_tables(res: tuple, device: torch.device) -> torch.Tensor:
    """per resolution the zero-padded periodic Hann window (n_fft,) and (cos, sin)(2 pi j / n_fft) (n_fft, 2), fp32 from float64"""
    key = (res, str(device))
    if key not in _MR_TABLES:
        parts = []
        for n_fft, _, win in res:
            w = torch.zeros(n_fft, dtype=torch.float64)
            left = (n_fft - win) // 2
            w[left:left + win] = torch.hann_window(win, dtype=torch.float64)
            th = 2.0 * math.pi * torch.arange(n_fft, dtype=torch.float64) / n_fft
            parts += [w, torch.stack([torch.cos(th), torch.sin(th)], dim=1).reshape(-1)]
        _MR_TABLES[key] = torch.cat(parts).to(torch.float32).to(device)
    return _MR_TABLES[key]


class _MrStftLoss(torch.autograd.Function):
    """value: eab_mrstft_loss_f32 leaves loss_b and two coefficients per (utterance, resolution); backward:
    eab_mrstft_loss_bwd_f32 recomputes the spectra and gathers the frames' gradients, scaled by grad_output on the device"""

    @staticmethod
    def forward(ctx, est, clean, lens, res, factor_sc, factor_mag, floor, reduction):
        lib = _lib.load()
        B, R = est.shape[0], len(res)
        e, s = est.detach(), clean
        cap = min(e.shape[1], s.shape[1])
        res_host = (C.c_int32 * (3 * R))(*[v for r in res for v in r])
        with torch.cuda.device(e.device):
            tables = _mr_tables(res, e.device)
            nbytes = lib.eab_mrstft_workspace_bytes(res_host, R, B, cap, 0)
            if nbytes < 0:
                raise _lib.EabError("eab_mrstft_workspace_bytes refused the resolutions or the rows")
            work = torch.empty((nbytes // 8,), dtype=torch.float64, device=e.device)
            coef = torch.empty((B, R, 2), dtype=torch.float64, device=e.device)
            loss = torch.empty((B,), dtype=torch.float32, device=e.device)
            total = torch.empty((2,), dtype=torch.float32, device=e.device)
            _lib.check(lib.eab_mrstft_loss_f32(*_rw.row_args(B, e, s), lens.data_ptr(), B, res_host, R, tables.data_ptr(), factor_sc,
                                               factor_mag, floor, work.data_ptr(), nbytes, coef.data_ptr(), loss.data_ptr(),
                                               total.data_ptr(), _rw.stream()), "eab_mrstft_loss_f32")
        ctx.save_for_backward(e, s, lens, coef, tables)
        ctx.res, ctx.floor, ctx.reduction = res, floor, reduction
        return loss if reduction == "none" else total[0 if reduction == "sum" else 1]

    @staticmethod
    def backward(ctx, g):
        e, s, lens, coef, tables = ctx.saved_tensors
        lib = _lib.load()
        B, L = e.shape
        res, R = ctx.res, len(ctx.res)
        res_host = (C.c_int32 * (3 * R))(*[v for r in res for v in r])
        g, gstride, scale = _rw.grad_row(g, B, ctx.reduction)
        with torch.cuda.device(e.device):
            nbytes = lib.eab_mrstft_workspace_bytes(res_host, R, B, min(L, s.shape[1]), 1)
            work = torch.empty((nbytes // 4,), dtype=torch.float32, device=e.device)
            grad = torch.empty((B, L), dtype=torch.float32, device=e.device)
            _lib.check(lib.eab_mrstft_loss_bwd_f32(*_rw.row_args(B, e, s), lens.data_ptr(), B, res_host, R, tables.data_ptr(), ctx.floor,
                                                   coef.data_ptr(), g.data_ptr(), gstride, scale, work.data_ptr(), nbytes, grad.data_ptr(), L,
                                                   _rw.stream()), "eab_mrstft_loss_bwd_f32")
        return grad, None, None, None, None, None, None, None


def mr_stft_loss(est: torch.Tensor, clean: torch.Tensor, lengths=None, resolutions=MR_RESOLUTIONS, factor_sc: float = 1.0,
                 factor_mag: float = 1.0, floor: float = 1e-7, reduction: str = "mean") -> torch.Tensor:
    """Multi-resolution STFT loss of B utterances, differentiable with respect to ``est``: est (B, Le), clean (B, Ls) or (B, 1, Ls),
    CUDA fp32 -> an fp32 scalar (``reduction`` "mean" or "sum") or (B,) ("none").  For every resolution (n_fft, hop, win), with X =
    torch.stft(x[:n_b], n_fft, hop, win, hann_window(win), center=True, pad_mode="reflect"), P = max(|X|^2, floor), E = sqrt(P_est),
    S = sqrt(P_clean) over the utterance's own T = 1 + n_b // hop frames and F = n_fft/2 + 1 bins:

        loss_b = 1/R sum_r [ factor_sc sqrt(sum (S - E)^2) / sqrt(sum S^2) + factor_mag / (T F) sum |ln S - ln E| ]

    The norms are per utterance (the published implementations take them over the batch; at B = 1 the two agree), so an utterance
    has the same bits alone, in any batch and in a second call, value and gradient.  The gradient is zero through a clamped bin and
    where sum (S - E)^2 = 0 its spectral-convergence part is taken as zero.  lengths: None (n_b = min(Le, Ls)) or (B,) sample counts
    <= min(Le, Ls), a sequence or integer tensor, host or device; n_b > max n_fft / 2 (reflect padding).  Samples at and past n_b
    are never read and the gradient is exactly zero from n_b to Le.  Rows may be strided views whose last dimension is contiguous
    and are read in place.  A resolution must have n_fft even in [8, 2048] with n_fft / 2 = 2^a 5^b, hop and win in [1, n_fft] and
    ceil(win / hop) <= 8; at most 8 resolutions.  No operator fallback: CPU tensors, other dtypes and a ``clean`` that requires grad
    raise."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {REDUCTIONS}, got {reduction!r}")
    if not (isinstance(floor, (int, float)) and 0.0 < float(floor) < float("inf")):
        raise ValueError(f"floor must be a finite number > 0, got {floor!r}")
    for name, v in (("factor_sc", factor_sc), ("factor_mag", factor_mag)):
        if not (isinstance(v, (int, float)) and 0.0 <= float(v) < float("inf")):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    res = check_resolutions(resolutions)
    clean, B = _rw.check_waves("mr_stft_loss", est, clean)
    cap, nmin = min(est.shape[1], clean.shape[1]), max(r[0] for r in res) // 2 + 1
    if cap < nmin:
        raise ValueError(f"rows of {cap} samples are too short for reflect padding: more than {nmin - 1} (max n_fft / 2) are needed")
    lens = [cap] * B if lengths is None else _m.check_lengths(lengths, B, cap, lo=nmin, unit="max n_fft / 2 < samples <= min(Le, Ls)",
                                                              integral=True)
    est_rows, clean_rows = _rw.device_rows("mr_stft_loss", est, clean)
    with torch.cuda.device(est.device):
        lens = _m._device_lengths(lens, est.device)
    return _MrStftLoss.apply(est_rows, clean_rows, lens, res, float(factor_sc), float(factor_mag), float(floor), reduction)


class _StoiLoss(torch.autograd.Function):
    """value: the five launches of eab_stoi_f32, unchanged, and the fp32 rounding of -(factor_stoi stoi + factor_estoi estoi) of its
    fp64 scores; the workspace (window, twiddles, K, kept, band values) is kept for eab_stoi_bwd_f32, which reads grad_output on
    the device"""

    @staticmethod
    def forward(ctx, est, clean, lens, factor_stoi, factor_estoi, reduction):
        lib = _lib.load()
        B = est.shape[0]
        e, s = est.detach(), clean
        cap = max(e.shape[1], s.shape[1])
        nbytes = lib.eab_stoi_workspace_bytes(B, cap)
        if nbytes < 0:
            raise ValueError(f"stoi_loss takes at most 65535 rows of at most 2^30 samples, got {B} rows of {cap}")
        with torch.cuda.device(e.device):
            work = torch.empty((nbytes,), dtype=torch.uint8, device=e.device)
            out = torch.empty((B, 2), dtype=torch.float64, device=e.device)
            _lib.check(lib.eab_stoi_f32(*_rw.row_args(B, e, s), lens.data_ptr(), B, work.data_ptr(), nbytes, out.data_ptr(), None, None,
                                        None, _rw.stream()), "eab_stoi_f32")
            loss = -(factor_stoi * out[:, 0] + factor_estoi * out[:, 1])
            if reduction != "none":
                loss = loss.sum()
                if reduction == "mean":
                    loss = loss / B
            loss = loss.to(torch.float32)
        ctx.save_for_backward(e, lens, work)
        ctx.cfg = (s.shape[1], factor_stoi, factor_estoi, reduction)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        e, lens, work = ctx.saved_tensors
        clean_cap, factor_stoi, factor_estoi, reduction = ctx.cfg
        lib = _lib.load()
        B, L = e.shape
        g, gstride, scale = _rw.grad_row(g, B, reduction)
        with torch.cuda.device(e.device):
            nbytes = lib.eab_stoi_bwd_workspace_bytes(B, max(L, clean_cap))
            scratch = torch.empty((nbytes,), dtype=torch.uint8, device=e.device)
            grad = torch.empty((B, L), dtype=torch.float32, device=e.device)
            _lib.check(lib.eab_stoi_bwd_f32(e.data_ptr(), e.stride(0) if B > 1 else L, L, clean_cap, lens.data_ptr(), B, work.data_ptr(),
                                            work.numel(), factor_stoi, factor_estoi, g.data_ptr(), gstride, scale,
                                            scratch.data_ptr(), nbytes, grad.data_ptr(), L, _rw.stream()), "eab_stoi_bwd_f32")
        return grad, None, None, None, None, None


def stoi_loss(est: torch.Tensor, clean: torch.Tensor, lengths=None, sample_rate: int = 16000, factor_stoi: float = 1.0,
              factor_estoi: float = 0.0, reduction: str = "mean") -> torch.Tensor:
    """Negative intelligibility of B utterances, differentiable with respect to ``est``: est (B, Le), clean (B, Ls) or (B, 1, Ls),
    CUDA fp32 -> an fp32 scalar (``reduction`` "mean" or "sum") or (B,) ("none").

        loss_b = -(factor_stoi * stoi_b + factor_estoi * estoi_b)

    with both scores exactly those of ``intelligibility(est, clean, lengths, sample_rate)``: the value runs the
    same launches and is the fp32 rounding of the same fp64 numbers.  The gradient is the literal derivative of
    that definition with three conventions: the kept-frame set comes from ``clean`` alone and is a constant; a band value that
    is exactly zero (every frame in est's zero tail) contributes no gradient; and where rule 9's bound binds an element it
    contributes nothing through est, while ``alpha`` is differentiated on the others.  Fewer than 30 band frames give the
    sentinel value -(factor_stoi + factor_estoi) 1e-5 and an exactly zero gradient.

    lengths: None (the full rows), (B,) sample counts for both signals, or (B, 2) pairs (est, clean), as in ``si_sdr_loss``; a
    signal counts as zero from its own length up to the longer of the two and is never read there, and the gradient is exactly
    zero from est's length to the row's end.  sample_rate: 10000 runs on the rows as they are (strided rows are read in place);
    any other rate resamples each signal with its OWN length as ``intelligibility`` does, est through the differentiable
    ``resample``.  A zero factor skips that half's backward work.  Every sum has one fixed order: an utterance has the same
    bits alone, in any batch and in a second call, value and gradient.  No double backward.  No operator fallback: CPU tensors,
    other dtypes and a ``clean`` that requires grad raise."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {REDUCTIONS}, got {reduction!r}")
    for name, v in (("factor_stoi", factor_stoi), ("factor_estoi", factor_estoi)):
        if isinstance(v, bool) or not (isinstance(v, (int, float)) and 0.0 <= float(v) < float("inf")):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    if float(factor_stoi) == 0.0 and float(factor_estoi) == 0.0:
        raise ValueError("factor_stoi and factor_estoi must not both be zero")
    _rw.check_rate(sample_rate, STOI_RATE)
    clean, B = _rw.check_waves("stoi_loss", est, clean)
    cols = _rw.check_lens(lengths, B, (est.shape[1], clean.shape[1]))
    est_rows, clean_rows = _rw.device_rows("stoi_loss", est, clean)
    (est_rows, clean_rows), cols = _rw.to_rate((est_rows, clean_rows), cols, sample_rate, STOI_RATE)
    with torch.cuda.device(est.device):
        lens = _rw.device_lens(cols, B, est.device)
    return _StoiLoss.apply(est_rows, clean_rows, lens, float(factor_stoi), float(factor_estoi), reduction)
