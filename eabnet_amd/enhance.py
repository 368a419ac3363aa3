"""Enhance many recordings in padded batches: the reference's enhance.py / test.py loop (wave -> STFT -> model -> ISTFT ->
wave, one file at a time at B = 1) with the files grouped by length, so that one call of the front end, of a length-bucketed
program and of the back end serves up to ``max_batch`` of them.

``plan_batches`` is the grouping rule (pure, no device); ``Enhancer`` runs a plan on the HIP front end, model and back end
with per-utterance lengths (``stft_compress(lengths=)``, ``forward(lengths=)``, ``istft(lengths=)``)."""
from __future__ import annotations

import importlib
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import model as _m

_rs = importlib.import_module(__package__ + ".resample")     # (the package's attribute `resample` is the function)

MODEL_RATE = 16000                            # the sample rate of the networks (enhance.py:35-37 resamples every file to it)


class Batch(NamedTuple):
    """One padded batch of a plan: the input positions of its files (slot order: longest first), the frame cap of the
    program it runs in (None: above every cap -- alone, on the exact-shape path) and the batch size of that program
    (len(indices) files, the other slots filled with dummy utterances)."""
    indices: Tuple[int, ...]
    cap: Optional[int]
    batch_size: int

    @property
    def dummies(self) -> int:
        return self.batch_size - len(self.indices)


def batch_sizes(max_batch: int) -> Tuple[int, ...]:
    """the batch sizes programs are built for, descending: max_batch, max_batch // 4 and 1 -- a short fixed set, so at most
    three programs per cap are ever lowered and captured"""
    if max_batch < 1:
        raise ValueError(f"max_batch must be positive, got {max_batch}")
    return tuple(sorted({max_batch, max(max_batch // 4, 1), 1}, reverse=True))


def plan_batches(frame_counts: Sequence[int], caps: Sequence[int], max_batch: int, sizes: Optional[Sequence[int]] = None) -> List[Batch]:
    """Group files of ``frame_counts`` frames into padded batches.

    Files longer than the largest cap run alone (cap None, batch size 1).  The others are sorted by length, longest first
    (ties in input order), and cut into groups of at most ``max_batch``; a group runs in the smallest cap that holds its
    longest member (``bucket_for``) at the smallest batch size of ``sizes`` (default ``batch_sizes(max_batch)``) that holds
    the group.  Neighbours in length share a batch, so the padding inside a batch stays small; the batches come longest
    first."""
    sizes = batch_sizes(max_batch) if sizes is None else tuple(sorted({int(s) for s in sizes}, reverse=True))
    if not sizes or sizes[-1] < 1 or sizes[0] < max_batch:
        raise ValueError(f"sizes must be positive and hold max_batch = {max_batch}, got {sizes}")
    caps = tuple(int(c) for c in caps)
    frames = [int(t) for t in frame_counts]
    if any(t < 1 for t in frames):
        raise ValueError("frame counts must be positive")
    order = sorted(range(len(frames)), key=lambda i: (-frames[i], i))
    plan = [Batch((i,), None, 1) for i in order if _m.bucket_for(frames[i], caps) is None]
    rest = [i for i in order if _m.bucket_for(frames[i], caps) is not None]
    for a in range(0, len(rest), max_batch):
        group = tuple(rest[a:a + max_batch])
        plan.append(Batch(group, _m.bucket_for(frames[group[0]], caps), min(s for s in sizes if s >= len(group))))
    return plan


def _padded_len(longest: int, frames: int, hop: int) -> int:
    """row length of a wave buffer of ``frames`` frames (1 + L // hop) that holds ``longest`` samples: the largest multiple of
    four that keeps the frame count (the four-samples-per-load gather of the STFT wants aligned rows), else ``longest``"""
    L = (hop * frames - 1) // 4 * 4
    return L if L >= longest else longest


class Enhancer(metaclass=_m._DecompressType):
    """``enh = Enhancer(model); waves_out = enh(waves)``: a list of (M, L_i) waves, host or device, any mix of lengths ->
    the list of enhanced (hop * (T_i - 1),) waves on the model's device, in input order (T_i = 1 + L_i // hop frames, what
    the one-at-a-time chain ``stft_compress -> model -> istft`` returns for each file).

    ``model`` is an ``EaBNet`` or an ``EaBNetWithPostNet`` (its ``output["esti_stft"]``) in eval mode; the call runs under
    ``torch.no_grad()``.  The files are grouped by ``plan_batches`` over the model's length buckets (``length_buckets`` of
    this enhancer when the model has none set; the model's attribute is restored after the call).  Per batch: the waves are
    packed into one zero-padded (B, M, L) buffer -- host waves through the staging ring of ``prepare_data`` --, then
    ``stft_compress(lengths=samples)``, ``model(lengths=frames)``, ``istft(lengths=frames)``, and each wave is sliced out.
    Free slots of a batch hold dummy utterances of the shortest admissible length (fft_num/2 + 1 zero samples), whose
    outputs are dropped.  A (cap, batch size) whose program would not fit ``max_resident_bytes`` of one of the model's
    networks is not built: its files are planned again at the next smaller batch size.

    Utterances of a batch do not influence each other, so every wave equals the one-at-a-time result up to the summation
    order of the kernels its batch shape selects (bit for bit where no statistic over time exists and the kernel choice is
    the same; see tests/test_enhance_gpu.py).  Non-causal configurations cannot run with per-utterance lengths (their last
    frames would read the padding): they -- and files above the largest cap -- run one file at a time on the exact-shape
    path, with the same result and no speed-up.

    ``sample_rate``: the rate of the waves handed in (the reference resamples every file to 16 kHz first, enhance.py:35-37).
    Other than 16000, the waves are packed at their own rate and ONE launch of the resampling kernel per batch
    (``eabnet_amd.resample``, with the files' lengths) writes the 16 kHz (B, M, L) buffer the front end reads; the plan runs on
    the frame counts of the resampled lengths, and every wave equals, bit for bit, what the 16 kHz enhancer returns for
    ``resample(wave, sample_rate, 16000)``.  ``mic_order``: the microphones of a file in the model's order (a permutation or a
    selection, enhance.py:41-42); the resampling kernel applies it as its row map, the packing does where the rate stays.
    ``output_rate``: None returns 16 kHz waves (enhance.py:63), an int or "input" resamples each batch's enhanced waves, with
    their lengths, before they are sliced out.

    ``Enhancer(..., decompress=True)`` (a bool, default False: the reference's waves; a keyword of the class call, see
    ``model._DecompressType``) is passed to every ``istft`` call: True undoes the front end's sqrt compression inside the
    back-end kernel, so each wave is an estimate of the signal in the clean files rather than of one whose spectrum has
    square-rooted magnitudes.  (The attribute ``enhancer.decompress`` may also be set between calls.)

    ``last_plan`` describes the last call: its batches (files, cap, batch size, dummies, frames), the dummy count, and the
    valid frames against the frames padded up to each batch's longest member and up to its cap."""

    decompress = False

    def __init__(self, model, max_batch: int = 16, fft_num: int = 320, hop: int = 160, window: Optional[torch.Tensor] = None,
                 length_buckets="auto", sample_rate: int = MODEL_RATE, mic_order=None, output_rate=None):
        if isinstance(model, _m.EaBNetWithPostNet):
            self.nets = (model.eabnet, model.postnet)
        elif isinstance(model, _m.EaBNet):
            self.nets = (model,)
        else:
            raise TypeError(f"Enhancer takes an EaBNet or an EaBNetWithPostNet, got {type(model).__name__}")
        if fft_num < 4 or fft_num % 2 or not 0 < hop <= fft_num:
            raise ValueError(f"fft_num must be even and 0 < hop <= fft_num, got {fft_num} and {hop}")
        self.model, self.max_batch, self.fft_num, self.hop = model, int(max_batch), fft_num, hop
        self.sizes = batch_sizes(self.max_batch)
        self.window = torch.hann_window(fft_num) if window is None else window
        self.length_buckets = length_buckets
        self.last_plan: Optional[dict] = None
        self._too_big: set = set()          # (cap, batch size, F, precisions, budgets) whose arena exceeds the budget
        self.phase_hook = None              # tools: called with "pack" / "stft" / "model" / "istft" / "slice" after each phase
        self.sample_rate = int(sample_rate)
        self._ratio = _rs._ratio(sample_rate, MODEL_RATE)                 # (o, n): o input samples per n model samples
        if self._ratio[0] != self._ratio[1]:
            _rs._check_span(*self._ratio, _rs.filter_bank(sample_rate, MODEL_RATE)[4], sample_rate, MODEL_RATE)
        self.mic_order = _rs.check_mic_order(mic_order, 1 << 30)           # (against the files' microphone count: in the call)
        self.output_rate = MODEL_RATE if output_rate is None else self.sample_rate if output_rate == "input" else output_rate
        if isinstance(self.output_rate, (str, bool)) or int(self.output_rate) != self.output_rate or self.output_rate < 1:
            raise ValueError(f'output_rate must be None, "input" or a sample rate, got {output_rate!r}')
        self.output_rate = int(self.output_rate)
        if self.output_rate != MODEL_RATE:
            ro, rn = _rs._ratio(MODEL_RATE, self.output_rate)
            _rs._check_span(ro, rn, _rs.filter_bank(MODEL_RATE, self.output_rate)[4], MODEL_RATE, self.output_rate)

    def _tick(self, phase: str) -> None:
        if self.phase_hook is not None:
            self.phase_hook(phase)

    # -- the plan ------------------------------------------------------------------
    def _fits(self, cap: int, size: int, F: int, device: torch.device) -> bool:
        """builds (or finds) the programs of (size, cap) in every network; False when one would exceed its arena budget"""
        key = (cap, size, F, tuple((n.precision, n.max_resident_bytes) for n in self.nets))
        if key in self._too_big:
            return False
        for net in self.nets:
            if net._program(size, cap, F, device, varlen=True, fit=True) is None:
                self._too_big.add(key)
                return False
        return True

    def _fit_plan(self, frames: List[int], caps, F: int, device: torch.device) -> List[Batch]:
        """plan_batches, then every batch whose program exceeds the budget planned again at the next smaller batch size"""
        todo = plan_batches(frames, caps, self.max_batch, self.sizes)[::-1]
        plan = []
        while todo:
            b = todo.pop()
            smaller = [s for s in self.sizes if s < b.batch_size]
            if b.cap is None or not smaller or self._fits(b.cap, b.batch_size, F, device):
                plan.append(b)                                    # (batch size 1 runs whatever its size: the LRU makes room)
                continue
            sub = plan_batches([frames[i] for i in b.indices], caps, smaller[0], smaller)
            todo.extend(Batch(tuple(b.indices[j] for j in s.indices), s.cap, s.batch_size) for s in sub[::-1])
        return plan

    # -- one batch -------------------------------------------------------------------
    def _pack(self, waves, M: int, B: int, L: int, device: torch.device, role: int = 0, order=None):
        """the waves of a batch as one zero-padded (B, M, L) device buffer (+ the staging ring's event, or None); role: the
        staging ring (``_HostStager.upload``) -- a second input of the batch keeps its own; order: the microphones to take"""
        if order is not None:
            waves = [w[list(order)] for w in waves]
        if all(w.is_cuda for w in waves):
            buf = torch.zeros((B, M, L), dtype=torch.float32, device=device)
            ev = None
        else:
            host = torch.zeros((B, M, L), dtype=torch.float32)
            for k, w in enumerate(waves):
                if not w.is_cuda:
                    host[k, :, :w.shape[1]] = w
            buf, ev = _m._upload(host, device, role)
        for k, w in enumerate(waves):
            if w.is_cuda:
                buf[k, :, :w.shape[1]].copy_(w, non_blocking=True)
        return buf, ev

    def _model(self, spec: torch.Tensor, lengths) -> torch.Tensor:
        out = self.model(spec, lengths=lengths) if lengths is not None else self.model(spec)
        return out["esti_stft"] if isinstance(out, dict) else out

    def _batch_done(self, batch: Batch, noisy, ev, est, wav, samples, counts, varlen: bool, device: torch.device) -> None:
        """what a subclass adds to a batch, on the same stream, after its back end (eabnet_amd.score.Scorer): the packed noisy
        (B, M, L) buffer and its staging event (already recorded after the front end; record it again after a later reader),
        the model's final estimate (B, 2, T, F), the padded waves (B, hop * (T - 1)), and the sample and frame counts of all B
        slots, dummies included (varlen False: one file on the exact-shape path)"""

    def _to_model_rate(self, waves, M_file: int, B: int, L: int, lens_in, device: torch.device, role: int = 0, order=None):
        """waves at ``sample_rate`` -> the (B, M, L) buffer at 16 kHz: packed at their own rate into (B, M_file, L o // n) and
        resampled by one launch with their lengths (None: one file, its full row) and ``order`` as the row map; the rows past
        ceil(n len / o) samples are zeros.  Returns (buffer, staging event or None); the event is recorded after the launch"""
        o, n = self._ratio
        raw, ev = self._pack(waves, M_file, B, max(L * o // n, max(w.shape[1] for w in waves)), device, role)
        buf = _rs._resample_rows(raw, self.sample_rate, MODEL_RATE, lens_in, order, L)
        if ev is not None:
            ev.record(torch.cuda.current_stream(device))
        return buf, ev

    def _output(self, wav: torch.Tensor, lens) -> torch.Tensor:
        """the enhanced (B, W) waves of a batch at ``output_rate`` (lens: their sample counts, or None for full rows)"""
        if self.output_rate == MODEL_RATE:
            return wav
        return _rs.resample(wav, MODEL_RATE, self.output_rate, lengths=lens)

    def _out_len(self, samples: int) -> int:
        return _rs.resampled_length(samples, MODEL_RATE, self.output_rate)

    def _run(self, batch: Batch, waves, frames, device: torch.device, varlen: bool) -> List[torch.Tensor]:
        fft, hop = self.fft_num, self.hop
        mine = [waves[i] for i in batch.indices]
        M_file = mine[0].shape[0]
        M = M_file if self.mic_order is None else len(self.mic_order)
        o, n = self._ratio
        convert = o != n
        if not varlen or batch.cap is None:                       # one file, exact-shape path
            if convert:
                buf, ev = self._to_model_rate(mine, M_file, 1, _rs.resampled_length(mine[0].shape[1], o, n), None, device,
                                              order=self.mic_order)
            else:
                buf, ev = self._pack(mine, M, 1, mine[0].shape[1], device, order=self.mic_order)
            spec = _m.stft_compress(buf, fft, hop, self.window)
            if ev is not None:
                ev.record(torch.cuda.current_stream(device))
            est = self._model(spec, None)
            wav = _m.istft(est, fft, hop, self.window, decompress=self.decompress)
            self._batch_done(batch, buf, ev, est, wav, [buf.shape[2]], [est.shape[2]], False, device)
            return [self._output(wav, None)[0]]
        B, T_max = batch.batch_size, frames[batch.indices[0]]
        # host waves: one buffer shape per (cap, batch size), so the staging ring is allocated once; device waves: no longer
        # than the longest file needs
        host = not all(w.is_cuda for w in mine)
        # a dummy utterance: the fewest input samples that resample to more than fft_num/2
        dummy_in = -(-(fft // 2 + 1) * o // n)
        lens_in = [w.shape[1] for w in mine] + [dummy_in] * batch.dummies
        samples = [_rs.resampled_length(v, o, n) for v in lens_in]
        L = _padded_len(max(samples), batch.cap if host else T_max, hop)
        counts = [1 + v // hop for v in samples]
        if convert:
            buf, ev = self._to_model_rate(mine, M_file, B, L, lens_in, device, order=self.mic_order)
        else:
            buf, ev = self._pack(mine, M, B, L, device, order=self.mic_order)
        self._tick("pack")
        spec = _m.stft_compress(buf, fft, hop, self.window, lengths=samples)
        if ev is not None:
            ev.record(torch.cuda.current_stream(device))
        self._tick("stft")
        est = self._model(spec[:, :T_max], counts)
        self._tick("model")
        wav = _m.istft(est, fft, hop, self.window, lengths=counts, decompress=self.decompress)
        self._tick("istft")
        res = self._output(wav, [hop * (c - 1) for c in counts])
        out = [res[k, :self._out_len(hop * (counts[k] - 1))].clone() for k in range(len(mine))]
        self._tick("slice")
        self._batch_done(batch, buf, ev, est, wav, samples, counts, True, device)
        return out

    @torch.no_grad()
    def __call__(self, waves: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        waves = list(waves)
        if self.model.training:
            raise RuntimeError("Enhancer: call model.eval() first")
        if not waves:
            self.last_plan = dict(batches=[], dummies=0, valid_frames=0, padded_frames=0, cap_frames=0)
            return []
        M = waves[0].shape[0] if waves[0].ndim == 2 else -1
        o, n = self._ratio
        for w in waves:
            if w.ndim != 2 or w.shape[0] != M or _rs.resampled_length(w.shape[1], o, n) <= self.fft_num // 2:
                raise ValueError(f"waves must be (M, L) tensors of one microphone count with L > fft_num/2 = {self.fft_num // 2}"
                                 f"{'' if o == n else ' at 16 kHz'}, got {tuple(w.shape)}")
        if self.mic_order is not None:
            _rs.check_mic_order(self.mic_order, M)
        M_model = self.nets[0].cfg.M
        if (M if self.mic_order is None else len(self.mic_order)) != M_model:
            raise ValueError(f"the model takes {M_model} microphones, the files hold {M}"
                             + ("" if self.mic_order is None else f" and mic_order selects {len(self.mic_order)}"))
        _m._lib.load()
        device = next(self.model.parameters()).device
        if device.type != "cuda":
            raise _m._lib.EabError("Enhancer runs on MI355X only: move the model to 'cuda'. There is no CPU fallback by design.")
        frames = [1 + _rs.resampled_length(w.shape[1], o, n) // self.hop for w in waves]
        F = self.fft_num // 2 + 1
        varlen = all(n.cfg.is_causal for n in self.nets)
        own = self.model.length_buckets is None
        if own and varlen:
            self.model.length_buckets = self.length_buckets
        try:
            with torch.cuda.device(device):
                if varlen:
                    plan = self._fit_plan(frames, self.nets[0]._bucket_caps(), F, device)
                else:
                    plan = [Batch((i,), None, 1) for i in range(len(waves))]
                out: List[Optional[torch.Tensor]] = [None] * len(waves)
                for b in plan:
                    for i, y in zip(b.indices, self._run(b, waves, frames, device, varlen)):
                        out[i] = y
        finally:
            if own and varlen:
                self.model.length_buckets = None
        rows = []
        for b in plan:
            valid = sum(frames[i] for i in b.indices)
            longest = frames[b.indices[0]]
            rows.append(dict(indices=list(b.indices), cap=b.cap, batch_size=b.batch_size, dummies=b.dummies, valid_frames=valid,
                             padded_frames=longest * len(b.indices) - valid,
                             cap_frames=(b.cap if b.cap is not None else longest) * b.batch_size))
        self.last_plan = dict(batches=rows, dummies=sum(r["dummies"] for r in rows),
                              valid_frames=sum(r["valid_frames"] for r in rows),
                              padded_frames=sum(r["padded_frames"] for r in rows),
                              cap_frames=sum(r["cap_frames"] for r in rows))
        return out
