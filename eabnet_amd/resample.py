"""Sample-rate conversion on the device: what the reference's loops do per file on the host before the first STFT
(``torchaudio.transforms.Resample(sr, 16000)``, enhance.py:35-37 and test.py:65-68) and the microphone reordering of
enhance.py:41-42, for the rows of a padded batch in one launch of csrc/resample.hip.

The definition (the windowed-sinc resampler of ``torchaudio.functional.resample`` with its default arguments; the taps it
keeps at the clamp |base*t| = lw, about 1e-33, are dropped).  For rates orig -> new: g = gcd, o = orig/g, n = new/g,
base = rolloff * min(o, n).  The prototype is h(t) = (base/o) sinc(base t) w(base t) for |base t| < lw and 0 otherwise, with
w(u) = cos^2(pi u / (2 lw)) ("hann") or I0(beta sqrt(1 - (u/lw)^2)) / I0(beta) ("kaiser").  Output sample i = q*n + p of a
signal x of L samples is

    y[i] = sum_m h(m/o - p/n) x[q*o + m],        x[j] = 0 for j < 0 or j >= L,        0 <= i < ceil(n L / o).

``filter_bank`` cuts h into n phases (host, float64); ``resample`` is the offline call, ``StreamResampler`` the same kernel on
a carry buffer with absolute positions.  Every output sample is ONE fp32 sum in ascending tap order, so its bits are the same
alone, in any batch and in a stream."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import model as _m

KAISER_BETA = 14.769656459379492
MAX_BANK = 16384                              # RS_MAX_BANK of csrc/resample.hip: floats of a bank (64 KB of LDS)
MAX_SPAN = 12288                              # RS_MAX_SPAN: floats of the input span of one tile
_BANKS: Dict[tuple, tuple] = {}
_DEVICE_BANKS: Dict[tuple, tuple] = {}
_ROW_MAPS: Dict[tuple, torch.Tensor] = {}


def _ratio(orig_freq, new_freq) -> Tuple[int, int]:
    if isinstance(orig_freq, bool) or isinstance(new_freq, bool) or int(orig_freq) != orig_freq or int(new_freq) != new_freq \
            or orig_freq < 1 or new_freq < 1:
        raise ValueError(f"sample rates must be positive integers, got {orig_freq} and {new_freq}")
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def resampled_length(L: int, orig_freq: int, new_freq: int) -> int:
    """samples of a signal of L samples after resampling: ceil(n L / o)"""
    o, n = _ratio(orig_freq, new_freq)
    return -(-n * int(L) // o)


def prototype(t, o: int, n: int, window: str = "hann", lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """h(t) of the module docstring for an array of times t (in input samples / o), float64"""
    base = rolloff * min(o, n)
    u = base * np.asarray(t, dtype=np.float64)
    lw = float(lowpass_filter_width)
    inside = np.abs(u) < lw
    uc = np.where(inside, u, 0.0)
    if window == "hann":
        w = np.cos(np.pi * uc / (2.0 * lw)) ** 2
    elif window == "kaiser":
        w = np.i0(KAISER_BETA * np.sqrt(np.maximum(1.0 - (uc / lw) ** 2, 0.0))) / np.i0(KAISER_BETA)
    else:
        raise ValueError(f"window must be 'hann' or 'kaiser', got {window!r}")
    return np.where(inside, (base / o) * np.sinc(uc) * w, 0.0)


def filter_bank(orig_freq: int, new_freq: int, window: str = "hann", lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(tab, first, o, n, K): per phase p the contiguous run of m with |base (m/o - p/n)| < lw -- first[p] (int32) its first m,
    tab[p][k] = h((first[p] + k)/o - p/n) (float64), zero-padded to the longest run K.  Pure host code, cached.  A bank of more
    than 16384 floats (64 KB of LDS) raises ValueError."""
    o, n = _ratio(orig_freq, new_freq)
    if lowpass_filter_width < 1 or not 0.0 < rolloff <= 1.0:
        raise ValueError(f"lowpass_filter_width must be positive and 0 < rolloff <= 1, got {lowpass_filter_width} and {rolloff}")
    key = (o, n, window, int(lowpass_filter_width), float(rolloff))
    hit = _BANKS.get(key)
    if hit is not None:
        return hit
    base = rolloff * min(o, n)
    D = lowpass_filter_width * o * n / base                           # |m n - p o| < D
    if (2.0 * D / n + 2.0) * n > 4 * MAX_BANK:
        raise ValueError(f"resampling {orig_freq} -> {new_freq} Hz needs a filter bank of about {int(2 * D) + n} floats; the "
                         f"kernel holds {MAX_BANK} (64 KB of LDS)")
    p = np.arange(n, dtype=np.int64)[:, None]
    m0 = np.floor((p * o - D) / n).astype(np.int64) - 1
    m = m0 + np.arange(int(math.ceil(2.0 * D / n)) + 4, dtype=np.int64)[None, :]
    num = m * n - p * o                                               # t = num / (o n), exact
    inside = np.abs(base * (num / float(o * n))) < lowpass_filter_width
    count = inside.sum(axis=1)
    K = int(count.max())
    if K * n > MAX_BANK:
        raise ValueError(f"resampling {orig_freq} -> {new_freq} Hz needs a filter bank of {n} x {K} = {K * n} floats; the kernel "
                         f"holds {MAX_BANK} (64 KB of LDS)")
    first = m[np.arange(n), inside.argmax(axis=1)]
    mm = first[:, None] + np.arange(K, dtype=np.int64)[None, :]
    tab = prototype((mm * n - p * o) / float(o * n), o, n, window, lowpass_filter_width, rolloff)
    tab[np.arange(K)[None, :] >= count[:, None]] = 0.0
    out = (tab, first.astype(np.int32), o, n, K)
    if len(_BANKS) > 64:
        _BANKS.clear()
    _BANKS[key] = out
    return out


def _check_span(o: int, n: int, K: int, orig_freq, new_freq) -> None:
    if (256 // n + 2) * o + K + 8 > MAX_SPAN:
        raise ValueError(f"resampling {orig_freq} -> {new_freq} Hz reads {o}/{n} input samples per output: the span of one tile "
                         f"exceeds the kernel's {MAX_SPAN} floats of LDS; resample in two steps")


def _device_bank(orig_freq, new_freq, window, lw, rolloff, device: torch.device):
    """the bank as fp32 / int32 device arrays, cached per device"""
    tab, first, o, n, K = filter_bank(orig_freq, new_freq, window, lw, rolloff)
    _check_span(o, n, K, orig_freq, new_freq)
    key = (o, n, window, int(lw), float(rolloff), str(device))
    hit = _DEVICE_BANKS.get(key)
    if hit is None:
        if len(_DEVICE_BANKS) > 64:
            _DEVICE_BANKS.clear()
        hit = _DEVICE_BANKS[key] = (torch.from_numpy(tab.astype(np.float32)).to(device), torch.from_numpy(first.copy()).to(device),
                                    o, n, K)
    return hit


def _row_map(B: int, M_out: int, pitch: int, order: Optional[Tuple[int, ...]], device: torch.device) -> torch.Tensor:
    """input row of every output row (b, m): b * pitch + order[m], as a cached int32 device array"""
    key = (B, M_out, pitch, order, str(device))
    hit = _ROW_MAPS.get(key)
    if hit is None:
        sel = np.arange(M_out, dtype=np.int64) if order is None else np.asarray(order, dtype=np.int64)
        rows = (np.arange(B, dtype=np.int64)[:, None] * pitch + sel[None, :]).reshape(-1)
        if len(_ROW_MAPS) > 256:
            _ROW_MAPS.clear()
        hit = _ROW_MAPS[key] = torch.from_numpy(rows.astype(np.int32)).pin_memory().to(device, non_blocking=True)
    return hit


def _row_layout(x3: torch.Tensor) -> Optional[Tuple[int, int]]:
    """(row stride in floats, rows between two groups) of a (G, M, L) view whose rows can be read in place -- row (g, m) at
    (g * pitch + m) * stride --, or None"""
    G, M, L = x3.shape
    sG, sM, sL = x3.stride()
    if L > 1 and sL != 1:
        return None
    if M == 1:
        return (sG if G > 1 else max(L, 1), 1) if sG >= 0 else None
    if G == 1:
        return (sM, M) if sM >= 0 else None
    if sM <= 0 or sG < 0 or sG % sM:
        return None
    return sM, sG // sM


def check_mic_order(mic_order, M: int) -> Optional[Tuple[int, ...]]:
    """a permutation or selection (repeats allowed) of M microphones as a tuple; None stays None"""
    if mic_order is None:
        return None
    order = tuple(mic_order.tolist()) if isinstance(mic_order, (torch.Tensor, np.ndarray)) else tuple(mic_order)
    if not order or any(isinstance(v, bool) or int(v) != v or not 0 <= v < M for v in order):
        raise ValueError(f"mic_order must hold microphone indices in [0, {M}), got {list(order)[:8]}")
    return tuple(int(v) for v in order)


def _launch(x: torch.Tensor, stride: int, cols: int, row_map, in_lens, rows: int, rows_per_utt: int, y: torch.Tensor, n_out: int,
            bank, in_origin: int = 0, out_origin: int = 0, valid_hi: int = -1) -> None:
    tab, first, o, n, K = bank
    _lib.check(_lib.load().eab_resample_f32(
        x.data_ptr(), stride, cols, None if row_map is None else row_map.data_ptr(), None if in_lens is None else in_lens.data_ptr(),
        rows, rows_per_utt, y.data_ptr(), n_out, n_out, tab.data_ptr(), first.data_ptr(), o, n, K, in_origin, out_origin, valid_hi,
        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "eab_resample_f32")


def _resample_rows(x3: torch.Tensor, orig_freq: int, new_freq: int, lens_in, order, n_out: int, window: str = "hann",
                   lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """one launch for a padded (B, M, L) fp32 device buffer: -> (B, len(order) or M, n_out); lens_in: the B valid sample counts
    (host values or a device tensor) or None; order: a checked mic_order or None.  n_out may differ from ceil(n L / o): the
    rows are written up to it, zeros past every utterance's own end (with lens_in)."""
    B, M, L = x3.shape
    layout = _row_layout(x3)
    if layout is None:
        x3 = x3.contiguous()
        layout = _row_layout(x3)
    stride, pitch = layout
    M_out = M if order is None else len(order)
    rows = B * M_out
    if rows > 65535:
        raise ValueError(f"resample takes at most 65535 rows per call, got {rows}")
    with torch.cuda.device(x3.device):
        bank = _device_bank(orig_freq, new_freq, window, lowpass_filter_width, rolloff, x3.device)
        y = torch.empty((B, M_out, n_out), dtype=torch.float32, device=x3.device)
        if rows and n_out:
            plain = order is None and (B == 1 or pitch == M)
            row_map = None if plain else _row_map(B, M_out, pitch, order, x3.device)
            lens = None if lens_in is None else _m._device_lengths(lens_in, x3.device)
            _launch(x3, stride, L, row_map, lens, rows, M_out, y, n_out, bank)
    return y


class _Resample(torch.autograd.Function):
    """the forward is ``_resample_rows``' one launch, unchanged; the backward is eab_resample_bwd_f32, the bank's adjoint as a
    gather per input sample (ascending output index, one fmaf per term)"""

    @staticmethod
    def forward(ctx, x3: torch.Tensor, lens, n_out: int, args: tuple) -> torch.Tensor:
        x3 = x3.detach()
        if lens is not None:
            with torch.cuda.device(x3.device):
                lens = _m._device_lengths(lens, x3.device)
        ctx.lens, ctx.args, ctx.shape = lens, args, tuple(x3.shape)
        return _resample_rows(x3, args[0], args[1], lens, None, n_out, *args[2:])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        B, M, L = ctx.shape
        gy = gy.detach().to(torch.float32).contiguous()
        n_out = gy.shape[-1]
        with torch.cuda.device(gy.device):
            tab, first, o, n, K = _device_bank(*ctx.args, gy.device)
            gx = torch.empty((B, M, L), dtype=torch.float32, device=gy.device)
            if B * M and L:
                _lib.check(_lib.load().eab_resample_bwd_f32(
                    gy.data_ptr(), n_out, n_out, None if ctx.lens is None else ctx.lens.data_ptr(), B * M, M, gx.data_ptr(), L, L,
                    tab.data_ptr(), first.data_ptr(), o, n, K, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                    "eab_resample_bwd_f32")
        return gx, None, None, None


def resample(wav: torch.Tensor, orig_freq: int, new_freq: int, lengths=None, mic_order=None, window: str = "hann",
             lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """(..., L) CUDA fp32 at ``orig_freq`` -> (..., ceil(n L / o)) at ``new_freq`` (module docstring); ``orig_freq == new_freq``
    returns the input (indexed by ``mic_order``, if given).

    lengths: per-utterance sample counts of a padded (B, M, L) or (B, L) batch (a sequence or an integer tensor, host or
    device): utterance b is wav[b, ..., :len[b]]; the samples past it are never read, its ceil(n len / o) output samples are
    those of a call on it alone, bit for bit, and the rest of its output rows is zero.  mic_order: a permutation, or a
    selection with repeats, of the second-to-last dimension, applied while reading (``wav[..., mic_order, :]`` at no cost).
    Rows are read in place when the last dimension is contiguous and the leading strides are multiples of one row pitch (a
    channel block of a wider buffer); anything else is copied first.

    A ``wav`` that requires grad goes through an autograd node: the same launch and the same bits forward, the bank's adjoint
    (one gather launch) backward -- zero past a row's length, and outputs past ceil(n len / o) carry no gradient.  ``mic_order``
    is refused there (a selection with repeats would need a row sum); a ``wav`` that does not require grad takes the plain
    path."""
    if wav.ndim < 1:
        raise ValueError("resample takes a (..., L) tensor")
    o, n = _ratio(orig_freq, new_freq)
    L = wav.shape[-1]
    order = None
    if mic_order is not None:
        if wav.ndim < 2:
            raise ValueError("mic_order needs a (..., M, L) tensor")
        order = check_mic_order(mic_order, wav.shape[-2])
    diff = wav.requires_grad and torch.is_grad_enabled()
    if diff and order is not None:
        raise NotImplementedError("resample is differentiable without mic_order only (a selection with repeats would need a "
                                  "row sum); index the waves first.  There is no operator fallback.")
    if lengths is not None:
        if wav.ndim not in (2, 3) or (wav.ndim == 2 and order is not None):
            raise ValueError(f"lengths needs a padded (B, M, L) batch, or (B, L) without mic_order, got {tuple(wav.shape)}")
        lengths = _m.check_lengths(lengths, wav.shape[0], L, lo=0, unit="the samples of a row", integral=True)
    if o == n:
        filter_bank(orig_freq, new_freq, window, lowpass_filter_width, rolloff)        # (the arguments are checked all the same)
        if not wav.is_cuda:
            raise _lib.EabError("resample needs a CUDA (ROCm) tensor; there is no CPU fallback by design.")
        return wav if order is None else wav[..., list(order), :]
    tab, first, o, n, K = filter_bank(orig_freq, new_freq, window, lowpass_filter_width, rolloff)
    _check_span(o, n, K, orig_freq, new_freq)
    if not wav.is_cuda:
        raise _lib.EabError("resample needs a CUDA (ROCm) tensor; there is no CPU fallback by design.")
    if wav.dtype != torch.float32:
        wav = wav.to(torch.float32)
    n_out = -(-n * L // o)
    lead = tuple(wav.shape[:-1])
    M_in = wav.shape[-2] if wav.ndim >= 2 else 1
    M_out = M_in if order is None else len(order)
    groups = int(np.prod(lead[:-1])) if wav.ndim >= 2 else 1            # blocks of M_in rows
    out_shape = (lead[:-1] + (M_out,) if wav.ndim >= 2 else ()) + (n_out,)
    if wav.ndim == 1:
        x3 = wav.reshape(1, 1, L)
    elif wav.ndim == 2:
        x3 = wav[None]
    elif wav.ndim == 3:
        x3 = wav
    else:
        x3 = wav.reshape((groups,) + tuple(wav.shape[-2:]))               # (a view where it can be, a copy where not)
    if lengths is not None and wav.ndim == 2:
        x3 = x3.transpose(0, 1)                                           # (B, L): every row an utterance of its own
    if diff:
        if x3.shape[0] * x3.shape[1] > 65535:
            raise ValueError(f"resample takes at most 65535 rows per call, got {x3.shape[0] * x3.shape[1]}")
        y = _Resample.apply(x3, lengths, n_out, (orig_freq, new_freq, window, lowpass_filter_width, rolloff))
    else:
        y = _resample_rows(x3, orig_freq, new_freq, lengths, order, n_out, window, lowpass_filter_width, rolloff)
    return y.view(out_shape)


class StreamResampler:
    """``rs = StreamResampler(48000, 16000); y = rs.push(x)``: the resampler on a stream cut anywhere.  ``push`` takes the next
    (..., n_in) samples (any n_in >= 0, the same leading shape in every call) and returns the output samples that became final:
    those whose last tap lies inside what has been pushed.  ``last=True`` zero-fills the right rim; the total returned then
    equals ``resampled_length(total_in)``.  The concatenation of all pushes is bit-identical to one offline ``resample``: the
    same kernel runs on a carry of the last K + o input samples with the absolute positions of its buffers.  ``reset()``
    restarts the stream.  The output trails the input by the filter's half-width (19 samples at 48 -> 16 kHz, 0.4 ms)."""

    def __init__(self, orig_freq: int, new_freq: int, window: str = "hann", lowpass_filter_width: int = 6, rolloff: float = 0.99):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self._bank_args = (window, lowpass_filter_width, rolloff)
        _, first, self.o, self.n, self.K = filter_bank(orig_freq, new_freq, *self._bank_args)
        _check_span(self.o, self.n, self.K, orig_freq, new_freq)
        self._first = [int(v) for v in first]
        self.reset()

    def reset(self) -> None:
        self._carry: Optional[torch.Tensor] = None      # (rows, <= K + o) last input samples
        self.total_in = 0                               # samples pushed
        self.total_out = 0                              # samples returned
        self._lead: Optional[tuple] = None

    def _last_tap(self, i: int) -> int:
        q, p = divmod(i, self.n)
        return q * self.o + self._first[p] + self.K - 1

    def _final_count(self, total: int, last: bool) -> int:
        """outputs [0, c) are final once `total` samples are in: their last tap (zero-padded taps included) is below total"""
        cap = -(-self.n * total // self.o)
        if last or self.o == self.n:
            return cap
        lo, hi = self.total_out, cap                    # _last_tap is nondecreasing in i
        while lo < hi:
            mid = (lo + hi) // 2
            if self._last_tap(mid) < total:
                lo = mid + 1
            else:
                hi = mid
        return lo

    def push(self, samples: torch.Tensor, last: bool = False) -> torch.Tensor:
        if samples.ndim < 1:
            raise ValueError("push takes a (..., n_in) tensor")
        if samples.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("StreamResampler is not differentiable (whole signals only: use resample); there is no "
                                      "operator fallback.")
        if not samples.is_cuda:
            raise _lib.EabError("StreamResampler needs CUDA (ROCm) tensors; there is no CPU fallback by design.")
        lead = tuple(samples.shape[:-1])
        if self._lead is None:
            self._lead = lead
        elif lead != self._lead:
            raise ValueError(f"the stream's pushes are {self._lead + ('n_in',)}, got {tuple(samples.shape)}")
        rows = int(np.prod(lead)) if lead else 1
        x = samples.to(torch.float32).reshape(rows, samples.shape[-1])
        if self.o == self.n:
            self.total_in += x.shape[1]
            self.total_out = self.total_in
            return samples
        origin = self.total_in - (0 if self._carry is None else self._carry.shape[1])
        buf = x.contiguous() if self._carry is None else torch.cat((self._carry, x), dim=1)
        self.total_in += x.shape[1]
        done = self.total_out
        count = self._final_count(self.total_in, last) - done
        keep = min(self.K + self.o, buf.shape[1])
        self._carry = buf[:, buf.shape[1] - keep:].clone()
        if rows > 65535:
            raise ValueError(f"StreamResampler takes at most 65535 rows, got {rows}")
        with torch.cuda.device(samples.device):
            y = torch.empty((rows, count), dtype=torch.float32, device=samples.device)
            if rows and count:
                bank = _device_bank(self.orig_freq, self.new_freq, *self._bank_args, samples.device)
                _launch(buf, buf.shape[1], buf.shape[1], None, None, rows, 1, y, count, bank, origin, done, self.total_in)
        self.total_out = done + count
        return y.view(lead + (count,))
