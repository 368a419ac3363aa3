"""Padded rows of waves with per-utterance lengths, between a tensor argument and a kernel: what the scores (score.py) and the
wave losses (wave.py) say once -- the stride rule, EabRows and the spans of csrc/rows.h, the ``lengths`` argument in its two
spellings, the est/clean front of a loss, autograd's ``grad_output`` as a device row, and the step to another rate."""
from __future__ import annotations

import ctypes as C
import importlib
from typing import Optional, Sequence

import torch

from . import _lib
from . import model as _m

_rs = importlib.import_module(__package__ + ".resample")     # (the package's attribute `resample` is the function)

SPAN = 4096                                   # EAB_SPAN of csrc/rows.h: samples (bins) per partial row


def spans(n: int) -> int:
    return max(1, -(-int(n) // SPAN))


def stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def in_place(t: torch.Tensor) -> torch.Tensor:
    """rows are read in place when their samples are contiguous and two rows do not overlap; anything else is packed"""
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def row_args(B: int, *tensors: torch.Tensor) -> list:
    """(pointer, floats between two rows, floats of a row that may be read) of every row tensor: EabRows of csrc/rows.h"""
    return [a for t in tensors for a in (t.data_ptr(), t.stride(0) if B > 1 else t.shape[1], t.shape[1])]


def check_lens(lengths, B: int, widths: Sequence[int], what: Optional[str] = None) -> list:
    """the checked sample counts of one signal per width, each a list or a device tensor; None: the full rows.  The scores take
    one member per signal and ``what`` names them ("triple (est, clean, noisy)"); the losses (``what`` None, two signals) take
    (B,) counts for both or (B, 2) pairs -- a tensor or a sequence"""
    if lengths is None:
        return [[w] * B for w in widths]
    if what is not None:
        cols = list(lengths)
        if len(cols) != len(widths):
            raise ValueError(f"lengths must be a {what} of (B,) counts, got {len(cols)} members")
    elif isinstance(lengths, torch.Tensor):
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
    return [_m.check_lengths(c, B, w, lo=1, unit="the signal's row length", integral=True) for c, w in zip(cols, widths)]


def device_lens(cols: list, B: int, device: torch.device) -> torch.Tensor:
    """checked counts as the (B, len(cols)) int32 device array of the kernels"""
    if not any(isinstance(c, torch.Tensor) for c in cols):
        return _m._device_lengths([v for row in zip(*cols) for v in row], device).view(B, len(cols))
    return torch.stack([_m._device_lengths(c, device) for c in cols], dim=1).contiguous()


def check_waves(fn: str, est: torch.Tensor, clean: torch.Tensor):
    """the front of the loss ``fn``, as far as CPU tensors go: est (B, Le) and clean (B, Ls) or (B, 1, Ls), the same B, fp32, no
    gradient to clean -> (clean as (B, Ls), B)"""
    if clean.ndim == 3 and clean.shape[1] == 1:
        clean = clean[:, 0]
    for name, t in (("est", est), ("clean", clean)):
        if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{name} must be a (B, L) tensor (clean may be (B, 1, L)), got {tuple(t.shape)}")
    B = est.shape[0]
    if clean.shape[0] != B:
        raise ValueError(f"est and clean must hold the same number of rows, got {B} and {clean.shape[0]}")
    if est.dtype != torch.float32 or clean.dtype != torch.float32:
        raise TypeError(f"{fn} takes fp32 waves, got {est.dtype} and {clean.dtype} (there is no operator fallback)")
    if clean.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{fn} is differentiable with respect to est only: clean requires grad (detach it; "
                                  "there is no operator fallback)")
    return clean, B


def device_rows(fn: str, est: torch.Tensor, clean: torch.Tensor):
    """the rest of that front: CUDA, one device -> (est, clean detached) as rows the kernels read"""
    if not (est.is_cuda and clean.is_cuda):
        raise _lib.EabError(f"{fn} needs CUDA (ROCm) tensors; there is no CPU fallback by design.")
    if est.device != clean.device:
        raise ValueError("est and clean must be on one device")
    return in_place(est), in_place(clean.detach())


def grad_row(g: torch.Tensor, B: int, reduction: str):
    """autograd's grad_output of a loss over B utterances as the kernels read it: (fp32 tensor, floats between the weights of two
    utterances -- 0 for the scalar of "mean" and "sum" --, the factor of the reduction)"""
    g = g.detach()
    if g.dtype != torch.float32:
        g = g.to(torch.float32)
    stride = g.stride(0) if reduction == "none" and B > 1 else 0
    if stride < 0:
        g, stride = g.contiguous(), 1
    return g, stride, 1.0 / B if reduction == "mean" else 1.0


def check_rate(sample_rate, rate) -> None:
    """ValueError for a pair of rates ``resample`` does not take"""
    _rs._ratio(sample_rate, rate)


def to_rate(signals, cols: list, sample_rate: int, rate: int, prepare=None):
    """every signal to ``rate`` with its OWN length (``prepare``: applied to a signal just before), then the lengths at that rate;
    at ``rate`` already: as they are.  A signal that requires grad goes through the differentiable ``resample``"""
    o, n = _rs._ratio(sample_rate, rate)
    if o == n:
        return signals, cols
    signals = [_rs.resample(prepare(t) if prepare else t, sample_rate, rate, lengths=c) for t, c in zip(signals, cols)]
    cols = [(c.to(torch.int64) * n + (o - 1)) // o if isinstance(c, torch.Tensor) else [-(-n * v // o) for v in c] for c in cols]
    return signals, cols
