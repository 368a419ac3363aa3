"""Train on the waveform: ``si_sdr_loss``, the negative SI-SDR that ``Scorer`` and ``energy_ratios`` report per file
(reference metrics.py:71-75), as a loss with a gradient -- csrc/wave_loss.hip behind tensor arguments.  With the differentiable
``istft`` the end of a training step reads

    wav = istft(out["esti_stft"], 320, 160, window)
    loss = l["final"] + w * si_sdr_loss(wav, target, eps=1e-8)
    loss.backward()

Two launches for the value, one for the gradient; ``grad_output`` is read on the device, nothing synchronises with the host."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import model as _m
from .score import _lens, _row_args, _spans

REDUCTIONS = ("mean", "sum", "none")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _SiSdrLoss(torch.autograd.Function):
    """value: eab_si_sdr_loss_f32 leaves (loss_b, a_b, c_b) per utterance; backward: eab_si_sdr_loss_bwd_f32 writes
    g_b (a_b e + c_b s) from grad_output on the device"""

    @staticmethod
    def forward(ctx, est: torch.Tensor, clean: torch.Tensor, lens: torch.Tensor, eps: float, reduction: str) -> torch.Tensor:
        lib = _lib.load()
        B = est.shape[0]
        e, s = est.detach(), clean
        with torch.cuda.device(e.device):
            spans = _spans(max(e.shape[1], s.shape[1]))
            partial = torch.empty((B, spans, 3), dtype=torch.float64, device=e.device)
            coef = torch.empty((B, 3), dtype=torch.float64, device=e.device)
            loss = torch.empty((B,), dtype=torch.float32, device=e.device)
            total = torch.empty((2,), dtype=torch.float32, device=e.device)
            _lib.check(lib.eab_si_sdr_loss_f32(*_row_args(B, e, s), lens.data_ptr(), B, float(eps), partial.data_ptr(), spans,
                                               coef.data_ptr(), loss.data_ptr(), total.data_ptr(), _stream()), "eab_si_sdr_loss_f32")
        ctx.save_for_backward(e, s, lens, coef)
        ctx.reduction = reduction
        return loss if reduction == "none" else total[0 if reduction == "sum" else 1]

    @staticmethod
    def backward(ctx, g):
        e, s, lens, coef = ctx.saved_tensors
        lib = _lib.load()
        B, L = e.shape
        g = g.detach()
        if g.dtype != torch.float32:
            g = g.to(torch.float32)
        per_row = ctx.reduction == "none"
        gstride = g.stride(0) if per_row and B > 1 else 0
        if gstride < 0:
            g, gstride = g.contiguous(), 1
        grad = torch.empty((B, L), dtype=torch.float32, device=e.device)
        with torch.cuda.device(e.device):
            _lib.check(lib.eab_si_sdr_loss_bwd_f32(*_row_args(B, e, s), lens.data_ptr(), B, coef.data_ptr(), g.data_ptr(), gstride,
                                                   1.0 / B if ctx.reduction == "mean" else 1.0, grad.data_ptr(), L, _stream()),
                       "eab_si_sdr_loss_bwd_f32")
        return grad, None, None, None, None


def _rows_in_place(t: torch.Tensor) -> torch.Tensor:
    """rows are read in place when their samples are contiguous and two rows do not overlap; anything else is packed"""
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


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
    if clean.ndim == 3 and clean.shape[1] == 1:
        clean = clean[:, 0]
    for name, t in (("est", est), ("clean", clean)):
        if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{name} must be a (B, L) tensor (clean may be (B, 1, L)), got {tuple(t.shape)}")
    B = est.shape[0]
    if clean.shape[0] != B:
        raise ValueError(f"est and clean must hold the same number of rows, got {B} and {clean.shape[0]}")
    if est.dtype != torch.float32 or clean.dtype != torch.float32:
        raise TypeError(f"si_sdr_loss takes fp32 waves, got {est.dtype} and {clean.dtype} (there is no operator fallback)")
    if clean.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("si_sdr_loss is differentiable with respect to est only: clean requires grad (detach it; "
                                  "there is no operator fallback)")
    widths = (est.shape[1], clean.shape[1])
    if lengths is None:
        cols = [[w] * B for w in widths]
    else:
        if isinstance(lengths, torch.Tensor):
            pairs = lengths.ndim == 2
            if pairs and tuple(lengths.shape) != (B, 2):
                raise ValueError(f"lengths must have shape ({B},) or ({B}, 2), got {tuple(lengths.shape)}")
            cols = [lengths[:, 0], lengths[:, 1]] if pairs else [lengths, lengths]
        else:
            rows = list(lengths)
            pairs = len(rows) > 0 and all(isinstance(r, (list, tuple)) for r in rows)
            if pairs and (len(rows) != B or any(len(r) != 2 for r in rows)):
                raise ValueError(f"lengths must hold {B} counts or {B} (est, clean) pairs")
            cols = [[r[0] for r in rows], [r[1] for r in rows]] if pairs else [rows, rows]
        cols = [_m.check_lengths(c, B, w, lo=1, unit="the signal's row length", integral=True) for c, w in zip(cols, widths)]
    if not (est.is_cuda and clean.is_cuda):
        raise _lib.EabError("si_sdr_loss needs CUDA (ROCm) tensors; there is no CPU fallback by design.")
    if est.device != clean.device:
        raise ValueError("est and clean must be on one device")
    est_rows, clean_rows = _rows_in_place(est), _rows_in_place(clean.detach())
    with torch.cuda.device(est.device):
        lens = _lens(cols, B, est.device)
    return _SiSdrLoss.apply(est_rows, clean_rows, lens, float(eps), reduction)
