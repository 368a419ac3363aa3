"""The end of the training step on the device: ``FlatAdam`` = ``clip_grad_norm_`` + ``torch.optim.Adam`` over flat buffers, two
launches per param group (csrc/optim.hip).

    opt = eabnet_amd.FlatAdam(net.parameters(), lr=5e-4, max_grad_norm=1.0)      # instead of Adam + clip_grad_norm_(1.0)
    loss.backward(); opt.step(); opt.zero_grad(set_to_none=True)

The parameters of a group live in ONE fp32 buffer (``p.data`` are views of it, in the order given), and so do ``exp_avg`` and
``exp_avg_sq``; ``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.Adam``'s format in both directions.  The gradients
are read where they are when they are consecutive slices of a few contiguous buffers (``last_path == "flat"``: what the training
programs' backward leaves behind) and gathered by one ``torch.cat`` otherwise (``"gathered"``); both give the same bits.

Differences from ``torch.optim.Adam`` + ``clip_grad_norm_``, all deliberate:
  * a group in which only SOME gradients are None raises (torch would skip those parameters alone); a group whose every
    gradient is None is skipped and its step count does not advance, as in torch;
  * one step count per group (the per-parameter ``"step"`` tensors are brought up to date by ``state_dict()``);
  * the norm is summed in fp64 in one fixed order: the same bits in every run (torch's fp32 norm is 7.8e-5 off at 2.8 M elements);
  * a non-finite gradient is not skipped: a NaN norm makes the clip factor NaN and with it every updated value, an Inf norm makes
    it zero (0 * Inf = NaN for the infinite elements), exactly as ``clip_grad_norm_(error_if_nonfinite=False)`` then ``Adam``;
  * ``step()`` has no CPU fallback and refuses a stream capture (the step count lives on the host).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional

import torch

from . import _lib

MAX_SEGMENTS = 8          # EAB_OPTIM_MAX_SEGMENTS
CHUNK = 4096              # EAB_OPTIM_CHUNK


class _Flat:
    """one param group's buffers: params (those that require grad, in order), their element counts and offsets, the three flat
    buffers and the host step count"""
    __slots__ = ("params", "numel", "offset", "total", "p", "m", "v", "t")


class FlatAdam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 5e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: Optional[float] = None):
        if isinstance(lr, torch.Tensor):
            raise ValueError("FlatAdam: lr is a host number (the scalars of a step are computed on the host)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm: Optional[torch.Tensor] = None      # 0-dim float64 device tensor: the pre-clip norm of the last step
        self.last_path: Optional[str] = None               # "flat" | "gathered"
        self.last_segments = 0                             # gradient buffers the last step read, over all groups
        self.stats = {"flat": 0, "gathered": 0, "launches": 0, "reflattened": 0}
        self._flat: List[Optional[_Flat]] = []
        # the keys (and fixed values) of torch.optim.Adam's groups, so that either optimizer loads the other's state dict
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)

    # -- flat buffers ------------------------------------------------------------------------------------------------
    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        self._flat.append(self._flatten(self.param_groups[-1]))

    def _flatten(self, group) -> Optional[_Flat]:
        ps = [p for p in group["params"] if p.requires_grad]
        if not ps:
            return None
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32 or p.device != dev or p.is_sparse:
                raise TypeError("FlatAdam: the parameters of a group are dense fp32 tensors on one device")
        f = _Flat()
        f.params, f.numel, f.offset, o = ps, [p.numel() for p in ps], [], 0
        for n in f.numel:
            f.offset.append(o)
            o += n
        f.total, f.t = o, 0
        f.m = torch.zeros(o, dtype=torch.float32, device=dev)
        f.v = torch.zeros(o, dtype=torch.float32, device=dev)
        self._adopt_params(f)
        self._view_state(f)
        return f

    @staticmethod
    def _adopt_params(f: _Flat) -> None:
        """copy the parameters' current values into a new flat buffer and re-point every ``p.data`` at its slice"""
        with torch.no_grad():
            f.p = torch.cat([p.detach().reshape(-1) for p in f.params])
            for p, piece in zip(f.params, f.p.split(f.numel)):
                p.data = piece.view(p.shape)

    def _view_state(self, f: _Flat) -> None:
        for p, m, v in zip(f.params, f.m.split(f.numel), f.v.split(f.numel)):
            self.state[p] = {"step": torch.tensor(float(f.t), dtype=torch.float32), "exp_avg": m.view(p.shape),
                             "exp_avg_sq": v.view(p.shape)}

    def _reflatten(self, f: _Flat) -> None:
        """a parameter left the flat buffer (.to(), load_state_dict(assign=True), a re-assigned .data): the CURRENT values are
        the truth; the moments follow to the parameters' device"""
        dev = f.params[0].device
        for p in f.params:
            if p.dtype != torch.float32 or p.device != dev:
                raise TypeError("FlatAdam: the parameters of a group are dense fp32 tensors on one device")
        self._adopt_params(f)
        if f.m.device != dev:
            f.m, f.v = f.m.to(dev), f.v.to(dev)
            self._view_state(f)
        self.stats["reflattened"] += 1

    # -- checkpoints -------------------------------------------------------------------------------------------------
    def state_dict(self):
        for f in self._flat:
            if f is not None:
                for p in f.params:
                    self.state[p]["step"].fill_(float(f.t))
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        """torch.optim.Adam's format (from either optimizer): the base class validates and casts, then the moments are copied
        into the flat buffers and the state points at the views again"""
        self._validate(state_dict)                 # before the base class replaces state and groups: a refusal changes nothing
        super().load_state_dict(state_dict)
        for f, group in zip(self._flat, self.param_groups):
            self._check_group(group)
            if f is None:
                continue
            loaded = [self.state.get(p) for p in f.params]
            have = [s for s in loaded if s]
            f.t = int(float(have[0]["step"])) if have else 0
            with torch.no_grad():
                if have:
                    for s, m, v in zip(loaded, f.m.split(f.numel), f.v.split(f.numel)):
                        m.copy_(s["exp_avg"].reshape(-1))
                        v.copy_(s["exp_avg_sq"].reshape(-1))
                else:
                    f.m.zero_()
                    f.v.zero_()
            self._view_state(f)

    def _validate(self, state_dict) -> None:
        """what FlatAdam itself refuses in a state dict (the base class checks the group and parameter counts after it)"""
        groups, state = state_dict["param_groups"], state_dict["state"]
        if len(groups) != len(self.param_groups):
            raise ValueError("FlatAdam: loaded state dict has a different number of parameter groups")
        for saved, mine in zip(groups, self.param_groups):
            self._check_group({**self.defaults, **saved})
            if len(saved["params"]) != len(mine["params"]):
                continue                                    # (the base class raises its own error)
            have = [state[i] for i, p in zip(saved["params"], mine["params"]) if p.requires_grad and state.get(i)]
            if have and len(have) != sum(p.requires_grad for p in mine["params"]):
                raise ValueError("FlatAdam: the state dict holds moments for some parameters of a group only "
                                 "(one step count per group)")
            steps = {int(float(s["step"])) for s in have}
            if len(steps) > 1:
                raise ValueError(f"FlatAdam: the parameters of a group are at different steps {sorted(steps)} (one step count per group)")

    @staticmethod
    def _check_group(group) -> None:
        for k in ("amsgrad", "maximize", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
            if group.get(k):
                raise ValueError(f"FlatAdam does not implement {k}={group[k]!r}")
        if isinstance(group["lr"], torch.Tensor):
            raise ValueError("FlatAdam: lr is a host number")

    # -- the step ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _walk(f: _Flat, grads) -> tuple:
        """One pass over the group: (aliased, segments).  aliased: every parameter still is its slice of the flat buffer.
        segments: [[offset in the group, address, elements]] when the gradients are consecutive slices of at most MAX_SEGMENTS
        contiguous dense fp32 buffers on the parameters' device, else None.  Exact over every parameter: an address that is not
        where the arithmetic says starts a new segment (whose device is checked; addresses are unique across devices), and
        anything that is not plain contiguous fp32 memory ends the attempt."""
        f32, strided = torch.float32, torch.strided
        base, dev, aliased, segs, nxt = f.p.data_ptr(), f.p.device, True, [], None
        for p, g, n, o in zip(f.params, grads, f.numel, f.offset):
            if p.data_ptr() != base + 4 * o or p.dtype is not f32 or not p.is_contiguous():
                aliased = False
            if segs is None or n == 0:
                continue
            if g.dtype is not f32 or g.layout is not strided or g.numel() != n or not g.is_contiguous():
                segs = None
                continue
            ptr = g.data_ptr()
            if ptr == nxt:
                segs[-1][2] += n
            elif len(segs) == MAX_SEGMENTS or g.device != dev:
                segs = None
                continue
            else:
                segs.append([o, ptr, n])
            nxt = ptr + 4 * n
        return aliased and f.params[0].device == dev, segs

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []                                            # (flat buffers, group, gradients) of the groups that step
        for f, group in zip(self._flat, self.param_groups):
            if f is None:
                continue
            grads = [p.grad for p in f.params]
            missing = [i for i, g in enumerate(grads) if g is None]
            if len(missing) == len(grads):
                continue
            if missing:
                raise RuntimeError(f"FlatAdam.step: parameter {missing[0]} of its group (shape {tuple(f.params[missing[0]].shape)}) "
                                   "has no gradient while others of the group have one; a group steps as a whole")
            self._check_group(group)
            work.append((f, group, grads))
        if not work:
            return loss
        dev = work[0][0].params[0].device
        for f, _, grads in work:
            if any(not p.is_cuda for p in f.params) or any(not g.is_cuda for g in grads):
                raise _lib.EabError("FlatAdam.step needs parameters and gradients on the GPU: eabnet_amd has no CPU fallback by design")
            if f.params[0].device != dev:
                raise _lib.EabError("FlatAdam.step: the param groups live on different devices")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FlatAdam.step cannot be captured: the step count and the bias corrections live on the host")
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            tables, chunks, path, keep = [], 0, "flat", []
            for f, group, grads in work:
                aliased, segs = self._walk(f, grads)
                if not aliased:
                    self._reflatten(f)
                if segs is None:
                    gbuf = torch.cat([g.reshape(-1).to(torch.float32) for g in grads])
                    keep.append(gbuf)
                    segs, path = [[0, gbuf.data_ptr(), f.total]], "gathered"
                bp, bm, bv = f.p.data_ptr(), f.m.data_ptr(), f.v.data_ptr()
                table = (_lib.OptimSegment * len(segs))(*[(bp + 4 * o, ptr, bm + 4 * o, bv + 4 * o, n) for o, ptr, n in segs])
                tables.append((table, len(segs), chunks))
                chunks += (f.total + CHUNK - 1) // CHUNK
            # the chunk sums of every group side by side, and the norm behind them
            scratch = torch.empty(chunks + 1, dtype=torch.float64, device=dev)
            norm = scratch[chunks]
            for table, nseg, first in tables:
                _lib.check(lib.eab_grad_sumsq_f64(table, nseg, scratch.data_ptr() + 8 * first, chunks - first, stream),
                           "eab_grad_sumsq_f64")
                self.stats["launches"] += 1
            clip = self.max_grad_norm if self.max_grad_norm is not None else 0.0
            for (f, group, _), (table, nseg, _) in zip(work, tables):
                b1, b2 = group["betas"]
                t = f.t + 1
                _lib.check(lib.eab_adam_clip_f32(table, nseg, scratch.data_ptr(), chunks, clip, group["lr"] / (1.0 - b1 ** t), b1, b2,
                                                 math.sqrt(1.0 - b2 ** t), group["eps"], group["weight_decay"], norm.data_ptr(), stream),
                           "eab_adam_clip_f32")
                self.stats["launches"] += 1
                f.t = t
                # the kernel wrote through raw addresses: bump the version counters, which is what the packed-weight fingerprint
                # of the modules that own these parameters (and of no other module) looks at
                torch.autograd.graph.increment_version(f.params)
        self.grad_norm, self.last_path, self.last_segments = norm, path, sum(n for _, n, _ in tables)
        self.stats[path] += 1
        return loss
