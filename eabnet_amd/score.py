"""Score enhanced files on the device: the reference's evaluation loops (test.py:175-198 -- forward, istft, ``.cpu().numpy()``,
``metrics.energy_ratios`` per file on the host; ``evaluate()`` of train_distributed.py:98-156, the same plus
``com_mag_mse_loss`` per file) on the padded batches of ``Enhancer``.

``energy_ratios`` and ``com_mag_mse_loss_per_utterance`` are the two kernels of csrc/score.hip behind tensor arguments;
``Scorer`` is an ``Enhancer`` that also packs the clean waves, takes their label spectrum and fills one (N, 5) float64 device
table -- si_sdr, si_sir, si_sar, si_sdr_mix, loss per file -- which it copies to the host once per call.

``intelligibility`` is csrc/stoi.hip behind tensor arguments: STOI and ESTOI per utterance at 10 kHz (the two remaining
closed-form metrics of cal_single_metrics), ``stoi`` the same with the host library's argument order, and
``Scorer(..., intelligibility=True)`` adds them as two more columns.

``sdr`` is csrc/sdr.hip behind tensor arguments: the SDR of BSS-eval -- the estimate projected on 512 shifts of the clean wave, the
distortion number reported next to PESQ and STOI, which does not ask for alignment to the sample -- and
``Scorer(..., distortion=True)`` adds it for the enhanced and the unprocessed wave as the columns ``sdr`` and ``sdr_mix``."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import _rows as _rw
from . import model as _m
from .enhance import MODEL_RATE, Batch, Enhancer

METRICS = ("si_sdr", "si_sir", "si_sar", "si_sdr_mix", "loss")
INTELLIGIBILITY_METRICS = ("stoi", "estoi")
DISTORTION_METRICS = ("sdr", "sdr_mix")
SDR_MAX_TAPS = 512                            # SDR_MAX_TAPS of csrc/sdr.hip
STOI_RATE = 10000                             # the rate of the definition: other rates are resampled to it first


def _rows(t: torch.Tensor, fn: str = "energy_ratios") -> torch.Tensor:
    """a signal of the scores as fp32 rows the kernels read (the losses refuse other dtypes; the scores cast them)"""
    if not t.is_cuda:
        raise _lib.EabError(f"{fn} needs CUDA (ROCm) tensors; there is no CPU fallback by design.")
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return _rw.in_place(t)


def energy_ratios(est: torch.Tensor, clean: torch.Tensor, noisy: torch.Tensor, lengths=None, energies: bool = False) -> torch.Tensor:
    """``metrics.energy_ratios(est, clean, noisy - clean)`` and ``metrics.si_sdr(clean, noisy)`` (reference metrics.py:14-39,
    71-75) of B utterances in one launch: (B, Le), (B, Ls), (B, Ly) CUDA fp32 tensors -> a (B, 4) float64 device tensor
    ``[si_sdr, si_sir, si_sar, si_sdr_mix]`` in dB (``energies=True``: (B, 8), followed by |s_target|^2, |e_noise|^2,
    |e_art|^2, |e_noise + e_art|^2).

    Rows may be strided views whose last dimension is contiguous (a channel of a (B, M, L) buffer, the first samples of a
    wider buffer): they are read in place.  lengths: an optional triple of (B,) sample counts (sequences or integer tensors,
    host or device) for (est, clean, noisy); every signal counts as zero from its own length up to the longest of the three, as
    cal_single_metrics (test.py:126-138) pads them, and is never read there.  A silent clean or noise row gives NaN in its
    own row.  All products and sums are fp64 in a fixed order: a row has the same bits alone and in any batch."""
    for name, t in (("est", est), ("clean", clean), ("noisy", noisy)):
        if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{name} must be a (B, L) tensor, got {tuple(t.shape)}")
    B = est.shape[0]
    if clean.shape[0] != B or noisy.shape[0] != B:
        raise ValueError(f"est, clean and noisy must hold the same number of rows, got {B}, {clean.shape[0]}, {noisy.shape[0]}")
    cols = _rw.check_lens(lengths, B, (est.shape[1], clean.shape[1], noisy.shape[1]), "triple (est, clean, noisy)")
    est, clean, noisy = _rows(est), _rows(clean), _rows(noisy)
    if not (est.device == clean.device == noisy.device):
        raise ValueError("est, clean and noisy must be on one device")
    widths = (est.shape[1], clean.shape[1], noisy.shape[1])
    lib = _lib.load()
    with torch.cuda.device(est.device):
        lens = _rw.device_lens(cols, B, est.device)
        spans = _rw.spans(max(widths))
        partial = torch.empty((B, spans, 6), dtype=torch.float64, device=est.device)
        out = torch.empty((B, 8), dtype=torch.float64, device=est.device)
        _lib.check(lib.eab_energy_ratios_f32(*_rw.row_args(B, est, clean, noisy), lens.data_ptr(), B, partial.data_ptr(), spans, out.data_ptr(),
                                             _rw.stream()), "eab_energy_ratios_f32")
    return out if energies else out[:, :4]


def com_mag_mse_loss_per_utterance(esti: torch.Tensor, label: torch.Tensor, frame_list) -> torch.Tensor:
    """(B,) float64 device tensor: ``com_mag_mse_loss(esti[b:b+1, :, :n_b], label[b:b+1, :, :n_b], [n_b])`` for every utterance
    b of a padded batch, what ``evaluate()`` (reference train_distributed.py:98-156) takes file by file.  esti (B, 2, Te, F),
    label (B, 2, Tl, F) CUDA tensors (the frame capacities may differ), frame_list (B,) counts in [1, min(Te, Tl)], host or
    device; frames at and past n_b are never read.  Any B; value only (the training loss with its gradient is
    ``com_mag_mse_loss``).  fp64 sums in a fixed order: an utterance has the same bits alone and in any batch."""
    if esti.ndim != 4 or label.ndim != 4 or esti.shape[1] != 2 or label.shape[1] != 2 or esti.shape[0] != label.shape[0] \
            or esti.shape[3] != label.shape[3]:
        raise ValueError(f"expected (B,2,Te,F) and (B,2,Tl,F), got {tuple(esti.shape)} and {tuple(label.shape)}")
    B, _, Te, F = esti.shape
    Tl = label.shape[2]
    frames = _m.check_lengths(frame_list, B, min(Te, Tl), lo=1, integral=True)
    if not (esti.is_cuda and label.is_cuda):
        raise _lib.EabError("com_mag_mse_loss_per_utterance needs CUDA (ROCm) tensors; there is no CPU fallback by design.")
    lib = _lib.load()
    e = esti.detach().to(torch.float32).contiguous()
    lab = label.detach().to(device=e.device, dtype=torch.float32).contiguous()
    with torch.cuda.device(e.device):
        fr = _m._device_lengths(frames, e.device)
        spans = _rw.spans(min(Te, Tl) * F)
        partial = torch.empty((B, spans, 2), dtype=torch.float64, device=e.device)
        out = torch.empty((B,), dtype=torch.float64, device=e.device)
        _lib.check(lib.eab_com_mag_mse_loss_lens_f32(e.data_ptr(), lab.data_ptr(), fr.data_ptr(), B, Te, Tl, F, partial.data_ptr(),
                                                     spans, out.data_ptr(), _rw.stream()),
                   "eab_com_mag_mse_loss_lens_f32")
    return out


def _stoi_rows(est: torch.Tensor, clean: torch.Tensor, cols: list, taps: bool):
    """the five launches of csrc/stoi.hip on 10 kHz rows: (B, 2) float64 [stoi, estoi] (and the taps)"""
    est, clean = _rows(est), _rows(clean)
    if est.device != clean.device:
        raise ValueError("est and clean must be on one device")
    B = est.shape[0]
    lib = _lib.load()
    cap = max(est.shape[1], clean.shape[1])
    FC, nbytes = lib.eab_stoi_frame_capacity(cap), lib.eab_stoi_workspace_bytes(B, cap)
    if FC < 0 or nbytes < 0:
        raise ValueError(f"intelligibility takes at most 65535 rows of at most 2^30 samples, got {B} rows of {cap}")
    with torch.cuda.device(est.device):
        lens = _rw.device_lens(cols, B, est.device)
        work = torch.empty((nbytes,), dtype=torch.uint8, device=est.device)
        out = torch.empty((B, 2), dtype=torch.float64, device=est.device)
        tap = None
        if taps:                              # (zeros: the kernels write the first K, K and K - 1 entries of a row only)
            tap = {"K": torch.zeros((B,), dtype=torch.int32, device=est.device),
                   "kept": torch.zeros((B, FC), dtype=torch.int32, device=est.device),
                   "tob": torch.zeros((B, 2, 15, FC), dtype=torch.float32, device=est.device)}
        ptrs = [tap[k].data_ptr() for k in ("K", "kept", "tob")] if taps else [None, None, None]
        _lib.check(lib.eab_stoi_f32(*_rw.row_args(B, est, clean), lens.data_ptr(), B, work.data_ptr(), nbytes, out.data_ptr(), *ptrs,
                                    _rw.stream()), "eab_stoi_f32")
    return (out, tap) if taps else out


def intelligibility(est: torch.Tensor, clean: torch.Tensor, lengths=None, sample_rate: int = 16000, taps: bool = False):
    """STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) of B utterances: (B, Le), (B, Ls) CUDA fp32 tensors -> a (B, 2)
    float64 device tensor ``[stoi, estoi]``, the two intelligibility numbers of cal_single_metrics (reference test.py:126-153).
    The definition of DESIGN.md §4.16 is the contract (frames of 256 at hop 128 under the inner points of a 258-point Hann
    window, frames more than 40 dB below the loudest clean frame removed, 15 third-octave bands from 150 Hz, segments of 30
    frames; fewer than 30 band frames give the sentinel 1e-5 for both); it follows the widely used Python implementation, but
    equality with that library's output is NOT verified.

    Rows may be strided views whose last dimension is contiguous and are read in place, as in ``energy_ratios``.  lengths: an
    optional pair of (B,) sample counts for (est, clean), host or device; a signal counts as zero from its own length up to the
    longer of the two (test.py:126-138) and is never read there.  sample_rate: 10000 skips the resampler; at any other rate
    each signal goes through ``resample(sig, sample_rate, 10000, lengths=...)`` with its default bank and its OWN length, and
    the shorter output is then zero-extended -- this differs from "pad, then resample" only in the filter's ringing past the
    shorter signal's end.  A silent clean row gives (0, 0).  fp64 sums in a fixed order: a row has the same bits alone, in any
    batch and in a second call.  taps=True (tests): ``(scores, {"K", "kept", "tob"})``, the kept-frame counts, the source
    frame of every compacted frame and the (B, 2, 15, frames) band values of (clean, est)."""
    for name, t in (("est", est), ("clean", clean)):
        if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{name} must be a (B, L) tensor, got {tuple(t.shape)}")
    B = est.shape[0]
    if clean.shape[0] != B:
        raise ValueError(f"est and clean must hold the same number of rows, got {B} and {clean.shape[0]}")
    cols = _rw.check_lens(lengths, B, (est.shape[1], clean.shape[1]), "pair (est, clean)")
    _rw.check_rate(sample_rate, STOI_RATE)
    if not (est.is_cuda and clean.is_cuda):
        raise _lib.EabError("intelligibility needs CUDA (ROCm) tensors; there is no CPU fallback by design.")
    (est, clean), cols = _rw.to_rate((est, clean), cols, sample_rate, STOI_RATE, prepare=_rows)
    return _stoi_rows(est, clean, cols, taps)


def check_sdr_filter(filter_length, load_diag):
    """(filter_length, load_diag) of ``sdr`` and ``sdr_loss`` checked, or ValueError"""
    if isinstance(filter_length, bool) or not isinstance(filter_length, int) or not 1 <= filter_length <= SDR_MAX_TAPS:
        raise ValueError(f"filter_length must be an integer in [1, {SDR_MAX_TAPS}], got {filter_length!r}")
    if isinstance(load_diag, bool) or not (isinstance(load_diag, (int, float)) and 0.0 <= float(load_diag) < float("inf")):
        raise ValueError(f"load_diag must be a finite number >= 0, got {load_diag!r}")
    return filter_length, float(load_diag)


def _sdr_rows(est: torch.Tensor, clean: torch.Tensor, lens: torch.Tensor, K: int, load_diag: float, eps: float, filters: bool):
    """the two launches of csrc/sdr.hip on fp32 rows and (B, 2) device lengths: out (B, 6) float64 [sdr_dB, tgt, ee, loss, a, c]
    and the filters (B, K) float64 (None unless asked for)"""
    lib = _lib.load()
    B = est.shape[0]
    with torch.cuda.device(est.device):
        spans = _rw.spans(max(est.shape[1], clean.shape[1]))
        partial = torch.empty((B, spans, 2 * K + 1), dtype=torch.float64, device=est.device)
        out = torch.empty((B, 6), dtype=torch.float64, device=est.device)
        h = torch.empty((B, K), dtype=torch.float64, device=est.device) if filters else None
        _lib.check(lib.eab_sdr_f32(*_rw.row_args(B, est, clean), lens.data_ptr(), B, K, load_diag, eps, partial.data_ptr(), spans,
                                   out.data_ptr(), h.data_ptr() if filters else None, _rw.stream()), "eab_sdr_f32")
    return out, h


def sdr(est: torch.Tensor, clean: torch.Tensor, lengths=None, filter_length: int = 512, load_diag: float = 0.0, filters: bool = False):
    """The SDR of BSS-eval of B utterances: (B, Le), (B, Ls) CUDA fp32 tensors -> a (B,) float64 device tensor in dB
    (``filters=True``: ``(sdr, h)`` with the (B, filter_length) float64 projection filters).  With K = filter_length and each
    signal zero from its own length up to the longer of the two (never read there):

        r[k] = sum_n s[n] s[n+k]   c[k] = sum_n s[n] e[n+k]   R = Toeplitz(r) + load_diag r[0] I   h = R^-1 c
        sdr = 10 log10( c.h / (sum_n e[n]^2 - c.h) )                                                  k = 0 .. K-1

    c.h is the energy of the estimate's projection on the clean wave shifted by 0 .. K-1 samples: the single-source SDR of
    mir_eval / fast_bss_eval in exact arithmetic (equality with those libraries is NOT verified; DESIGN §4.25 is the contract).
    It does not ask for alignment to the sample: a delayed or lightly filtered copy of the clean wave scores by its noise alone.
    K = 1 is the ``si_sdr`` of ``energy_ratios``.  Rows may be strided views whose last dimension is contiguous and are read in
    place; lengths: an optional pair of (B,) sample counts for (est, clean), host or device, as in ``intelligibility``.  A silent
    clean row, a clean row of fewer than K samples and a row whose recursion meets a prediction error <= 0 give NaN in their
    own row only.  Correlations, the Levinson recursion and the ratio in fp64 in a fixed order: a row has the same bits alone,
    in any batch and in a second call."""
    for name, t in (("est", est), ("clean", clean)):
        if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{name} must be a (B, L) tensor, got {tuple(t.shape)}")
    B = est.shape[0]
    if clean.shape[0] != B:
        raise ValueError(f"est and clean must hold the same number of rows, got {B} and {clean.shape[0]}")
    K, load_diag = check_sdr_filter(filter_length, load_diag)
    cols = _rw.check_lens(lengths, B, (est.shape[1], clean.shape[1]), "pair (est, clean)")
    est, clean = _rows(est, "sdr"), _rows(clean, "sdr")
    if est.device != clean.device:
        raise ValueError("est and clean must be on one device")
    with torch.cuda.device(est.device):
        lens = _rw.device_lens(cols, B, est.device)
    out, h = _sdr_rows(est, clean, lens, K, load_diag, 0.0, bool(filters))
    return (out[:, 0], h) if filters else out[:, 0]


def stoi(clean, est, fs_sig: int, extended: bool = False) -> float:
    """``stoi(clean, est, fs_sig, extended)`` with the host library's argument order, as test.py calls it: 1-D tensors or arrays
    -> a Python float, STOI or (``extended=True``) ESTOI by ``intelligibility`` (whose definition, not that library's output, is
    the contract).  Host inputs are copied to the current device; the call synchronises."""
    sig = []
    for v in (est, clean):
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
        if t.ndim != 1 or t.shape[0] < 1:
            raise ValueError(f"stoi takes 1-D signals, got {tuple(t.shape)}")
        sig.append(t)
    if not torch.cuda.is_available():
        raise _lib.EabError("stoi runs on MI355X only; there is no CPU fallback by design.")
    device = next((t.device for t in sig if t.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    e, c = (t.to(device=device, dtype=torch.float32)[None] for t in sig)
    return float(intelligibility(e, c, sample_rate=fs_sig)[0, 1 if extended else 0])


class _ScorerType(_m._DecompressType):
    """``Scorer(..., intelligibility=True)``: the switch is a keyword of the class call, not of ``__init__``, whose parameter list
    is pinned together with the other tools' (tests/test_resample_ref.py::test_defaults_of_the_tools_are_unchanged).
    ``decompress`` is ``Enhancer``'s, named here so that the signature of the class shows it."""

    def __call__(cls, *args, intelligibility: bool = False, distortion: bool = False, decompress: bool = False, **kw):
        self = super().__call__(*args, decompress=decompress, **kw)
        self.intelligibility = bool(intelligibility)
        if distortion:                        # (off: the instance keeps the class's False and nothing else changes)
            self.distortion = True
        return self


class Scorer(Enhancer, metaclass=_ScorerType):
    """``scores = Scorer(model)(noisy_waves, clean_waves)``: lists of (M, L_i) noisy and (L_i,) or (1, L_i) clean waves, host or
    device -> a dict of (N,) float64 numpy arrays ``si_sdr, si_sir, si_sar, si_sdr_mix, loss`` in input order
    (``return_waves=True``: ``(scores, waves)`` with exactly ``Enhancer``'s waves).

    It runs ``Enhancer``'s plan and, per batch and on the same stream, packs the clean waves into a (B, 1, L) buffer through the
    same staging path, takes ``stft_compress(clean, layout=1, lengths=samples)`` as the label, the per-utterance loss of the
    model's final estimate against it (``com_mag_mse_loss_per_utterance``) and the energy ratios of (enhanced wave, clean,
    noisy[ref_mic]) with the lengths (hop * (T_b - 1), L_b, L_b) (``energy_ratios``).  The rows go into one (N, 5) float64
    device table at the files' input positions, dummy slots dropped; the table is copied to the host once, at the end of the
    call -- nothing synchronises per file or per batch.  ``sample_rate`` / ``mic_order`` as in ``Enhancer``: the noisy AND the clean
    waves are resampled to 16 kHz on the device (test.py:65-68), the clean ones by a second launch with the same bank, and the
    scores are those of the 16 kHz signals; ``ref_mic`` counts in the model's microphone order.  Non-causal models and files above the largest cap run one file at a
    time through the same kernels at B = 1.  ``summary(scores)``: {metric: (mean, std)} with NaNs dropped (metrics.mean_std).

    ``intelligibility=True`` adds the keys ``stoi`` and ``estoi`` (a (N, 7) table): per batch, on the same stream, the enhanced
    waves and the clean buffer are resampled from 16 kHz to 10 kHz and scored by ``intelligibility`` with the lengths
    (hop * (T_b - 1), L_b).  The default changes nothing: not the keys, the table, the launches or the bits.  (The attribute
    ``scorer.intelligibility`` may also be set between calls.)

    ``distortion=True`` adds the keys ``sdr`` and ``sdr_mix`` after those: per batch, on the same stream, ``sdr`` (the SDR of
    BSS-eval with 512 taps) of the enhanced waves against the clean buffer with the lengths (hop * (T_b - 1), L_b), and of
    noisy[ref_mic] against it with (L_b, L_b).  A file of fewer than 512 samples gives NaN in these two.  Off, nothing changes.

    ``decompress=True`` (a bool; ``Enhancer``'s switch) takes the enhanced waves in the linear domain -- ``istft(decompress=True)``,
    an estimate of the signal in the clean files -- and every wave score (``si_sdr, si_sir, si_sar, stoi, estoi, sdr``) on them.
    ``loss`` stays the loss of the compressed spectra and keeps its bits; ``si_sdr_mix`` and ``sdr_mix`` do not see the
    estimate.  The default False scores the reference's waves, whose spectra have square-rooted magnitudes."""

    intelligibility = False
    distortion = False

    def __init__(self, model, max_batch: int = 16, fft_num: int = 320, hop: int = 160, window: Optional[torch.Tensor] = None,
                 length_buckets="auto", ref_mic: int = 0, sample_rate: int = 16000, mic_order=None):
        super().__init__(model, max_batch, fft_num, hop, window, length_buckets, sample_rate=sample_rate, mic_order=mic_order)
        if int(ref_mic) != ref_mic or ref_mic < 0:
            raise ValueError(f"ref_mic must be a microphone index, got {ref_mic}")
        self.ref_mic = int(ref_mic)
        self._clean: List[torch.Tensor] = []
        self._stage: Optional[torch.Tensor] = None
        self._filled = 0

    def _batch_done(self, batch: Batch, noisy, ev, est, wav, samples, counts, varlen: bool, device) -> None:
        fft, hop = self.fft_num, self.hop
        B, M, L = noisy.shape
        clean = [self._clean[i] for i in batch.indices]
        if self._ratio[0] != self._ratio[1]:                  # the clean waves through the same bank, in their own staging role
            lens_in = None
            if varlen:
                dummy_in = -(-(fft // 2 + 1) * self._ratio[0] // self._ratio[1])
                lens_in = [c.shape[1] for c in clean] + [dummy_in] * batch.dummies
            cbuf, cev = self._to_model_rate(clean, 1, B, L, lens_in, device, role=1)
        else:
            cbuf, cev = self._pack(clean, 1, B, L, device, role=1)
        self._tick("pack_clean")
        label = _m.stft_compress(cbuf, fft, hop, self.window, 1, lengths=samples if varlen else None)
        self._tick("stft_clean")
        loss = com_mag_mse_loss_per_utterance(est, label, counts)
        ratios = energy_ratios(wav, cbuf[:, 0], noisy[:, self.ref_mic], lengths=([hop * (t - 1) for t in counts], samples, samples))
        if self.intelligibility:              # (before the events below: it reads the staged clean waves too)
            intel = intelligibility(wav, cbuf[:, 0], lengths=([hop * (t - 1) for t in counts], samples), sample_rate=MODEL_RATE)
        if self.distortion:
            dist = sdr(wav, cbuf[:, 0], lengths=([hop * (t - 1) for t in counts], samples))
            dist_mix = sdr(noisy[:, self.ref_mic], cbuf[:, 0], lengths=(samples, samples))
        for e in (ev, cev):
            if e is not None:                 # the staged noisy and clean waves have no reader after this point
                e.record(torch.cuda.current_stream(device))
        n = len(batch.indices)
        rows = self._stage[self._filled:self._filled + n]
        rows[:, :4].copy_(ratios[:n])
        rows[:, 4].copy_(loss[:n])
        if self.intelligibility:
            rows[:, 5:7].copy_(intel[:n])
        if self.distortion:
            col = len(self.metrics) - 2
            rows[:, col].copy_(dist[:n])
            rows[:, col + 1].copy_(dist_mix[:n])
        self._filled += n
        self._tick("score")

    @property
    def metrics(self) -> Tuple[str, ...]:
        """the keys of the scores, in the order of the table's columns"""
        return METRICS + (INTELLIGIBILITY_METRICS if self.intelligibility else ()) + (DISTORTION_METRICS if self.distortion else ())

    @torch.no_grad()
    def __call__(self, noisy_waves: Sequence[torch.Tensor], clean_waves: Sequence[torch.Tensor], return_waves: bool = False):
        noisy, clean = list(noisy_waves), list(clean_waves)
        if len(noisy) != len(clean):
            raise ValueError(f"Scorer: {len(noisy)} noisy files but {len(clean)} clean files")
        clean = [c[None] if c.ndim == 1 else c for c in clean]
        for k, (x, c) in enumerate(zip(noisy, clean)):
            if c.ndim != 2 or c.shape[0] != 1:
                raise ValueError(f"Scorer: clean waves must be (L,) or (1, L) tensors, file {k} is {tuple(c.shape)}")
            if x.ndim != 2 or x.shape[1] != c.shape[1]:
                raise ValueError(f"Scorer: file {k} has {tuple(x.shape)} noisy but {c.shape[1]} clean samples; the lengths must agree")
            mics = x.shape[0] if self.mic_order is None else len(self.mic_order)
            if self.ref_mic >= mics:
                raise ValueError(f"Scorer: ref_mic = {self.ref_mic} but file {k} has {mics} microphones"
                                 + ("" if self.mic_order is None else " after mic_order"))
        if self.model.training:
            raise RuntimeError("Scorer: call model.eval() first")
        N = len(noisy)
        if N == 0:
            super().__call__([])
            scores = {m: np.zeros(0) for m in self.metrics}
            return (scores, []) if return_waves else scores
        device = next(self.model.parameters()).device
        if device.type != "cuda":
            raise _lib.EabError("Scorer runs on MI355X only: move the model to 'cuda'. There is no CPU fallback by design.")
        self._clean, self._filled = clean, 0
        try:
            with torch.cuda.device(device):
                self._stage = torch.empty((N, len(self.metrics)), dtype=torch.float64, device=device)        # rows in plan order
            waves = super().__call__(noisy)
            assert self._filled == N
            with torch.cuda.device(device):
                order = [i for b in self.last_plan["batches"] for i in b["indices"]]
                pos = torch.as_tensor(order, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
                table = torch.empty_like(self._stage).index_copy_(0, pos, self._stage)       # rows at the input positions
                host = table.cpu().numpy()                                                   # the call's one device-to-host copy
        finally:
            self._clean, self._stage = [], None
        scores = {m: np.ascontiguousarray(host[:, j]) for j, m in enumerate(self.metrics)}
        return (scores, waves) if return_waves else scores

    @staticmethod
    def summary(scores: Dict[str, np.ndarray]) -> Dict[str, Tuple[float, float]]:
        """{metric: (mean, std)} with NaNs dropped, as metrics.mean_std (reference metrics.py:110-114)"""
        out = {}
        for m, v in scores.items():
            v = np.asarray(v, dtype=np.float64)
            v = v[~np.isnan(v)]
            out[m] = (float(np.mean(v)), float(np.std(v))) if v.size else (float("nan"), float("nan"))
        return out
