"""Drop-in boundary: ``EaBNet`` (reference EaBNet.py:9-125), ``prepare_data``
(reference train_distributed.py:68-95), ``numParams`` (EaBNet.py:653-659) and
``com_mag_mse_loss`` (EaBNet.py:627-640) with the reference's names, argument
meaning and tensor signatures, executing on libeabnet_hip.so.

The module owns ordinary ``nn.Parameter``s under the reference's state-dict
keys (eabnet_amd/spec.py), so reference checkpoints load with
``strict=True``.  ``forward`` lowers the network once per (B, T, parameter
version) to an op program (eabnet_amd/program.py), binds it to device
addresses and replays it with ONE foreign call per forward.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import OrderedDict
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import program as prg
from .graphs import LaneGraphs
from .runtime import BoundProgram, chain_planner, chain_tables, encode, fuse_step
from .runtime import graph_branches_allowed  # noqa: F401 (API)
from .spec import GagConfig, NetConfig, ParamSpec, gag_param_specs, param_specs


# ----------------------------------------------------------------------------
# parameter container with the reference's dotted names
# ----------------------------------------------------------------------------
class _Scope(nn.Module):
    """Anonymous container: only exists so that ``state_dict()`` produces the
    dotted keys of the reference's module tree."""


def _default_init(spec: ParamSpec) -> torch.Tensor:
    """PyTorch's default initialisers for the layer types the reference uses."""
    t = torch.empty(spec.shape, dtype=torch.float32)
    k = spec.kind
    if k in ("conv_w", "convT_w", "lin_w", "bias", "lstm"):
        a = 1.0 / math.sqrt(max(spec.fan_in, 1))      # kaiming_uniform(a=sqrt 5) == U(-1/sqrt(fan_in), +)
        return t.uniform_(-a, a)
    if k in ("norm_w", "ln_w"):
        return t.fill_(1.0)
    if k in ("norm_b", "ln_b"):
        return t.zero_()
    if k == "prelu":
        return t.fill_(0.25)
    if k == "bn_mean":
        return t.zero_()
    if k == "bn_var":
        return t.fill_(1.0)
    if k == "bn_count":
        return torch.zeros((), dtype=torch.long)
    raise ValueError(k)


def _attach(root: nn.Module, dotted: str, p: torch.Tensor) -> None:
    """Register a parameter (nn.Parameter) or a buffer (plain tensor: BatchNorm statistics)."""
    node = root
    parts = dotted.split(".")
    for name in parts[:-1]:
        child = node._modules.get(name)
        if child is None:
            child = _Scope()
            node.add_module(name, child)
        node = child
    if isinstance(p, nn.Parameter):
        node.register_parameter(parts[-1], p)
    else:
        node.register_buffer(parts[-1], p)


# ----------------------------------------------------------------------------
# bound program
# ----------------------------------------------------------------------------
class _Bound(BoundProgram):
    """A lowered inference program with its device arenas: the op list "run", bound to in / out (/ in2) buffers."""
    BOUNDARY = ("in", "out", "in2")

    def __init__(self, prog: prg.Program, device: torch.device):
        self.prog = prog
        self.weights = torch.from_numpy(prog.weights).to(device)
        self.acts = torch.empty(max(prog.act_floats, 1), dtype=torch.float32, device=device)
        super().__init__(device, {"w": self.weights, "a": self.acts}, {"run": prog.ops}, {"run": prog.lanes}, {"run": prog.sync})
        self.ops = self.arrays["run"]
        self.reset_counters()
        # streaming programs: the frame position every windowed op reads (device memory, so one captured
        # graph serves all chunks)
        self.t_pos = torch.zeros(1, dtype=torch.int32, device=device) if prog.chunk else None
        # per-utterance lengths (varlen programs): device array [B] every windowed op reads; written on the launch stream
        # before each run, so one captured graph serves every combination of lengths
        self.lens = torch.full((prog.B,), prog.T, dtype=torch.int32, device=device) if prog.varlen else None
        self.window = {"t_pos": self.t_pos.data_ptr() if prog.chunk else None, "chunk": prog.chunk,
                       "lens": self.lens.data_ptr() if prog.varlen else None}
        # a whole-program run of a streaming step: the fused launches (runtime.fuse_step) as [(op, first, count)] and their
        # encoded array; None when the program has nothing to fuse.  self.ops keeps one entry per program op for partial runs.
        self.fused, self.exec_ops = None, None
        self._carry_dev = None              # the carry table in device memory (eab_shift_desc[]), for the current binding

    def reset_counters(self) -> None:
        """arrival counters of the fused InstanceNorm finalisation: zero before the first run (the kernels re-arm them
        after every complete run; needed again only if the arena was overwritten from outside, as the tests do)"""
        for ref, n in self.prog.zero_init:
            self.acts[ref.off:ref.off + n].zero_()

    def __del__(self):
        # The arenas may have been used on streams other than the one they were allocated under (Pipeline slot
        # streams, hipGraph replays): the caching allocator would hand the blocks out again while such work is
        # still queued.  Dropping a bound program is rare (shape / precision change), so drain the device first.
        try:
            if torch.cuda.is_available():
                torch.cuda.synchronize(self.device)
        except Exception:                                 # noqa: BLE001 - interpreter shutdown
            pass

    @property
    def graph(self) -> Optional[LaneGraphs]:
        """the captured program (None before a capture or after a refused one)"""
        return self.graphs["run"] if self.graphs else None

    # the captured form's boundary buffers (None before a capture)
    static_in = property(lambda self: self.static.get("in"))
    static_out = property(lambda self: self.static.get("out"))
    static_in2 = property(lambda self: self.static.get("in2"))

    def update_weights(self, flat: np.ndarray) -> None:
        self.weights.copy_(torch.from_numpy(flat), non_blocking=False)

    def bind(self, in_ptr: int, out_ptr: int, in2_ptr: Optional[int] = None) -> bool:
        if not super().bind(in_ptr, out_ptr, in2_ptr):
            return False
        self._carry_dev = None
        # the fused step follows the binding: the chain launch reads the encoded descriptors of the ops it stands for from
        # device memory (arena 'chain').  EAB_ST_CHAIN=0 / EAB_CLN_STEP=0 keep the separate launches.
        p = self.prog
        if not p.chunk:
            return True
        self.fused, self.exec_ops = None, None
        self.arenas.pop("chain", None)
        fused = fuse_step(p.ops, p.chunk, os.environ.get("EAB_ST_CHAIN", "1") != "0", os.environ.get("EAB_CLN_STEP", "1") != "0",
                          chain_planner(self.ops))
        if len(fused) < len(p.ops):
            tables = chain_tables(self.ops, fused)
            if tables:
                self.arenas["chain"] = torch.frombuffer(bytearray(tables), dtype=torch.uint8).to(self.device)
            self.fused = fused
            self.exec_ops = encode([op for op, _, _ in fused], self.bases(), **self.window)
        return True

    @property
    def chains(self) -> list:
        """(first, count) of every run of program ops the bound step executes as one chain launch"""
        return [(first, count) for op, first, count in (self.fused or []) if op.kind == prg.OP_CONV_CHAIN]

    @property
    def n_exec(self) -> int:
        """launches of a whole-program run of the fused step (0: nothing fused, the program runs its own array)"""
        return len(self.exec_ops) if self.exec_ops is not None else 0

    def upload_carry(self) -> None:
        """The carry table of a streaming program (prog.carry) as eab_shift_desc[] in device memory, for the boundary
        buffers the program is bound to: uploaded once per binding, like the descriptors of a chain launch."""
        if self._carry_dev is not None or not self.prog.carry:
            return
        bases = self.bases()
        descs = (_lib.ShiftDesc * len(self.prog.carry))()
        for d, (ref, row, rows) in zip(descs, self.prog.carry):
            d.ptr, d.row_floats, d.rows = bases[ref.arena] + 4 * ref.off, row, rows
        self._carry_dev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(self.device)

    def rebase(self, src_pos: int, stream: int) -> int:
        """Move the rows a streaming program can still read at frame position ``src_pos`` to the front of the resident
        window (one launch on ``stream``, eab_shift_rows_f32) and return the position the stream continues at
        (prog.history).  Not part of the step's graph: it runs between two replays, on the launch stream."""
        p = self.prog
        if not (p.chunk and 2 * p.history <= src_pos <= p.T):
            raise ValueError(f"rebase at position {src_pos} of a window of {p.T} frames with history {p.history}")
        self.upload_carry()
        if p.carry:
            _lib.check(_lib.load().eab_shift_rows_f32(self._carry_dev.data_ptr(), len(p.carry), p.B, p.T, src_pos, p.history,
                                                      C.c_void_p(stream)), "eab_shift_rows_f32")
        return p.history

    def buffers(self, use_graph: bool, in_shape, out_shape, in2_shape=None):
        """(in, out, in2), launch: boundary buffers the program is bound to and the call that runs it on them -- the
        captured form's static buffers and its replay, or (use_graph False, or the capture refused) fresh zero-filled
        buffers and direct launches on torch's current stream.  in2 is None without in2_shape."""
        if use_graph and self.capture(in_shape, out_shape, in2_shape):
            return (self.static_in, self.static_out, self.static_in2), self.graph.replay
        bufs = tuple(None if s is None else torch.zeros(s, dtype=torch.float32, device=self.device)
                     for s in (in_shape, out_shape, in2_shape))
        self.bind(*(None if b is None else b.data_ptr() for b in bufs))
        return bufs, lambda: self.run(torch.cuda.current_stream().cuda_stream)

    def _launch(self, name: str, stream: int, first: int, n: int) -> None:
        if first == 0 and n == len(self.prog.ops) and self.exec_ops is not None:
            _lib.check(_lib.load().eab_run_program(self.exec_ops, self.n_exec, C.c_void_p(stream)), "eab_run_program")
            return
        super()._launch(name, stream, first, n)

    def run(self, stream: int, first: int = 0, count: Optional[int] = None) -> None:
        """Enqueue ops [first, first+count) on ``stream`` (a raw hipStream_t) with direct kernel launches (BoundProgram.run)."""
        super().run("run", stream, first, count)

    def view(self, act: prg.Act) -> torch.Tensor:
        """Debug view of a named activation as (B, T, F, C)."""
        p = self.prog
        n = p.B * p.T * act.F * act.C
        assert act.ref.arena == "a"
        return self.acts[act.ref.off:act.ref.off + n].view(p.B, p.T, act.F, act.C)


# ----------------------------------------------------------------------------
# the module
# ----------------------------------------------------------------------------
AUTO_BUCKETS = tuple(64 << k for k in range(8))          # length_buckets="auto": 64, 128, .., 8192 frames


def bucket_for(T: int, caps) -> Optional[int]:
    """smallest cap >= T, or None when T exceeds every cap (the call then takes the exact-shape path)"""
    for c in caps:
        if c >= T:
            return int(c)
    return None


def check_lengths(lengths, B: int, T: int, lo: int = 1, unit: str = "the call's frame count", integral: bool = False):
    """Validate a ``lengths=`` argument: a (B,) sequence or integer tensor with lo <= len <= T.  Host values are checked and
    returned as a list; a device tensor is checked for shape and dtype only (its values would need a host synchronisation)
    and returned as is -- the kernels stay in bounds for any value.  integral: also refuse sequence members that are not
    whole numbers (the front and back end; the networks' forward converts them with int(), as it always has)."""
    if isinstance(lengths, torch.Tensor):
        if lengths.dtype.is_floating_point or lengths.dtype == torch.bool or lengths.is_complex():
            raise ValueError(f"lengths must be integers, got {lengths.dtype}")
        if tuple(lengths.shape) != (B,):
            raise ValueError(f"lengths must have shape ({B},), got {tuple(lengths.shape)}")
        if lengths.is_cuda:
            return lengths
        vals = [int(v) for v in lengths.tolist()]
    else:
        vals = list(lengths)
        if integral and any(isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v
                            for v in vals):
            raise ValueError(f"lengths must be integers, got {vals[:4]}")
        vals = [int(v) for v in vals]
        if len(vals) != B:
            raise ValueError(f"lengths must hold {B} values (one per utterance), got {len(vals)}")
    bad = [v for v in vals if not lo <= v <= T]
    if bad:
        raise ValueError(f"lengths must lie in [{lo}, {T}] ({unit}), got {bad[:4]}")
    return vals


def _device_lengths(lens, device: torch.device) -> torch.Tensor:
    """checked lengths (check_lengths) as an int32 device array, enqueued on the current stream without a host synchronisation:
    a device tensor device-to-device, host values through a pinned copy"""
    if isinstance(lens, torch.Tensor):
        return lens.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()
    return torch.as_tensor(lens, dtype=torch.int32).pin_memory().to(device, non_blocking=True)


def _refuse_differentiable(module: nn.Module, what: str, reason: str):
    """A differentiable call the HIP training programs do not cover is refused, never served by another backend: the package
    has one (the PyTorch-ROCm operator evaluation that used to sit here is now test infrastructure, tests/operator_path.py)."""
    return NotImplementedError(
        f"{type(module).__name__}: {what} ({reason}).  eabnet_amd runs differentiable calls on its HIP training programs "
        "(eabnet_amd/train.py, train_gag.py) and has no operator fallback; call under torch.no_grad() for inference.")


class _HipModule(nn.Module):
    """Shared machinery of the two networks: reference-keyed parameters, the lowered-program cache
    (one resident shape, re-packed when a parameter or buffer changes) and the replay knobs."""

    def _init_params(self, specs) -> None:
        self._specs = specs
        for key, spec in specs.items():
            t = _default_init(spec)
            _attach(self, key, t if spec.is_buffer else nn.Parameter(t))
        self._bound: "OrderedDict[tuple, _Bound]" = OrderedDict()
        self._packed_version: Dict[tuple, tuple] = {}
        self.dump_bfw = False                         # tests: also emit the (B,T,F,M,2) beam-forming weights
        # replay the lowered program as ONE hipGraph launch (static internal in/out buffers, one
        # device copy of the input and of the output per call); False = direct kernel launches
        self.use_graph = True
        # arithmetic of the MFMA contractions: "f32" = exact fp32 MFMA; "f16x3" = error-compensated
        # fp16 split on the f16 matrix cores, same end-to-end error class as fp32;
        # "bf16" = operands rounded to bf16, fp32 accumulate / norms / activations (BASELINE configs[3]/[4];
        # outside the 1e-4 bar: ~1e-2)
        self.precision = "f32"
        # "hip" once a differentiable forward has run (train.py / train_gag.py programs -- the only backend); None before
        self.training_backend = None
        # length-bucketed programs (causal configurations, inference): None = one exact-shape program per (B, T), as always;
        # "auto" = caps of 64, 128, .. 8192 frames; or an ascending tuple of caps.  A call of T frames then runs in the
        # program of the smallest cap >= T with every utterance T frames long (lengths = T) and is sliced back to T; longer
        # calls take the exact-shape path.  Bucketed programs live in an LRU of their own, bounded by a count and by the
        # bytes of their activation arenas (varlen_arena_bytes() reports them per bucket).
        self.length_buckets = None
        self.max_resident_programs = 8
        self.max_resident_bytes = 8 << 30
        self._varlen_bound: "OrderedDict[tuple, _Bound]" = OrderedDict()
        self._varlen_version: Dict[tuple, tuple] = {}
        # lengths= under autograd: False = refused, as always; True = the training programs run with per-utterance
        # lengths (masked statistics, recurrences and weight gradients) -- EaBNet, is_causal=True, norm_type="IN"
        self.varlen_training = False
        # length buckets for differentiable calls: None = nothing changes; "auto" (AUTO_BUCKETS) or an ascending
        # tuple of caps.  A differentiable call of T frames, with or without lengths=, then runs on the masked training programs
        # of the smallest cap >= T (wider calls: of width T) -- one lowering and one pair of graphs per (B, cap) for every
        # narrower width and every combination of lengths.  EaBNet and GaGNet, is_causal=True, norm_type="IN"
        self.train_length_buckets = None
        # gradient with respect to the input: False = an input that requires grad is refused, as always; True
        # (EaBNet only) = such a call runs the training programs lowered with input_grad=True and x.grad arrives from
        # loss.backward(); a call whose input needs no gradient runs the very program it ran before
        self.input_grad = False

    def _param_fingerprint(self) -> tuple:
        """Change detector for the packed weights (runs on every forward).  Every parameter / buffer slot
        contributes (storage address, version counter): in-place updates bump the version, ``.data =``
        re-assignment, a device move or ``load_state_dict(assign=True)`` change the address or the object in the
        slot; a kernel that writes parameters through raw addresses bumps the versions itself (FlatAdam.step).  The slot list (owning module, name) is cached -- walking the ~800-node module tree costs more
        than the rest of the host side of a step; looking the ~500 slots up does not."""
        slots = self.__dict__.get("_slot_list")
        if slots is None:
            slots = []
            for mod in self.modules():
                slots += [(mod._parameters, n) for n in mod._parameters] + [(mod._buffers, n) for n in mod._buffers]
            self.__dict__["_slot_list"] = slots
        fp = []
        for d, n in slots:
            t = d[n]
            fp.append((t.data_ptr(), t._version))
        return tuple(fp)

    def _numpy_params(self) -> Dict[str, np.ndarray]:
        sd = self.state_dict()
        return {k: sd[k].detach().to("cpu", torch.float32).numpy() for k, s in self._specs.items()
                if s.kind != "bn_count"}

    def _program(self, B: int, T: int, F: int, device: torch.device, varlen: bool = False, fit: bool = False) -> Optional[_Bound]:
        """The bound program of (B, T, F) on ``device``, its packed weights current.  Exact-shape programs keep one shape
        resident (activations can be GBs); length-bucketed (varlen) ones live in an LRU bounded by max_resident_programs
        and max_resident_bytes.  fit: a new program whose arena alone exceeds the byte budget is not built (None; the
        caches stay as they are) instead of being admitted alone."""
        chains = bool(self.__dict__.get("parallel_chains", True))
        key = (B, T, F, str(device), self.precision, chains)
        cache, versions = (self._varlen_bound, self._varlen_version) if varlen else (self._bound, self._packed_version)
        limit, budget = (self.max_resident_programs, self.max_resident_bytes) if varlen else (1, math.inf)
        fp = self._param_fingerprint()
        bound = cache.get(key)
        stale = bound is None or ("bf_w" in bound.prog.taps) != self.dump_bfw
        if stale or versions.get(key) != fp:
            prog = prg.lower(self.cfg, self._numpy_params(), B, T, F, dump_bfw=self.dump_bfw, precision=self.precision,
                             parallel_chains=chains, varlen=varlen)
            if stale:
                need = 4 * max(prog.act_floats, 1)
                if fit and need > budget:
                    return None
                while cache and (len(cache) >= limit or sum(4 * b.acts.numel() for b in cache.values()) + need > budget):
                    old, _ = cache.popitem(last=False)            # least recently used
                    versions.pop(old, None)
                bound = cache[key] = _Bound(prog, device)
            else:
                bound.update_weights(prog.weights)
            versions[key] = fp
        cache.move_to_end(key)
        return bound

    # -- per-utterance lengths / length buckets ----------------------------------------
    def _bucket_caps(self, what: str = "length_buckets") -> Tuple[int, ...]:
        lb = getattr(self, what)
        if lb is None:
            return ()
        if isinstance(lb, str):
            if lb != "auto":
                raise ValueError(f"{what} must be None, 'auto' or an ascending tuple of frame counts, got {lb!r}")
            return AUTO_BUCKETS
        try:
            caps = tuple(int(c) for c in lb)
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be None, 'auto' or an ascending tuple of frame counts, got {lb!r}") from None
        if not caps or any(c < 1 for c in caps) or any(b <= a for a, b in zip(caps, caps[1:])):
            raise ValueError(f"{what} must be an ascending tuple of positive frame counts, got {lb!r}")
        return caps

    def _train_bucket_call(self, T: int, B: int, lengths) -> Tuple[int, object]:
        """(width of the program, lengths) of a differentiable call under train_length_buckets: the smallest cap >= T, or T
        itself when it exceeds every cap; lengths=None means every utterance is T frames long.  Configurations the masked
        training programs do not cover are refused here, before anything reaches a device."""
        caps = self._bucket_caps("train_length_buckets")
        lens = T if lengths is None else check_lengths(lengths, B, T)
        from . import train
        why = train.varlen_unsupported_reason(self.cfg)
        if why:
            raise NotImplementedError(f"{type(self).__name__}: a differentiable call with train_length_buckets: {why}")
        cap = bucket_for(T, caps)
        return (cap if cap is not None else T), lens

    def _varlen_call(self, T: int, B: int, lengths, needs_graph: bool) -> Optional[Tuple[int, object]]:
        """(T_cap, lengths) of a call that runs in a per-utterance-length program, or None for the exact-shape path.
        Explicit ``lengths`` are validated here (ValueError) and refused (NotImplementedError) where they cannot be served."""
        if needs_graph and self.train_length_buckets is not None and not (self.varlen_training and self.length_buckets is not None):
            return self._train_bucket_call(T, B, lengths)
        if lengths is None:
            if self.length_buckets is None or not self.cfg.is_causal or needs_graph or self.dump_bfw:
                return None
            cap = bucket_for(T, self._bucket_caps())
            return None if cap is None else (cap, T)
        lens = check_lengths(lengths, B, T)
        if needs_graph and self.varlen_training:
            why = self._varlen_training_refusal()
            if why:
                raise NotImplementedError(f"{type(self).__name__}: lengths= under autograd with varlen_training: {why}")
            return T, lens                                       # the exact padded width of the call
        if needs_graph:
            raise _refuse_differentiable(self, "lengths= under autograd (or BatchNorm in train mode)",
                                         "per-utterance lengths are an inference form; training with lengths (masked batch "
                                         "statistics, gradients) is not implemented")
        if not self.cfg.is_causal:
            raise NotImplementedError(f"{type(self).__name__}: lengths= needs is_causal=True -- the non-causal S-TCM taps of "
                                      "the last frames of an utterance read the frames after it, so a padded batch cannot "
                                      "reproduce the one-at-a-time result")
        if self.dump_bfw:
            raise NotImplementedError(f"{type(self).__name__}: lengths= with dump_bfw (a test hook of the exact-shape path)")
        cap = bucket_for(T, self._bucket_caps()) if self.length_buckets is not None else None
        return (cap if cap is not None else T), lens

    def _varlen_training_refusal(self) -> str:
        """why a differentiable call with lengths= cannot run on the masked training programs ('' when it can)"""
        cfg = self.cfg
        if isinstance(cfg, prg.GagConfig):
            return ("GaGNet (and with it EaBNetWithPostNet) has no masked training lowering yet; train the post-filter on "
                    "equal-length batches")
        from . import train
        why = train.varlen_unsupported_reason(cfg)               # norm and causality: one wording, shared with lower_train
        if why:
            return why
        if self.length_buckets is not None:
            return ("length_buckets together with a differentiable call: the training programs take the exact padded width "
                    "(set length_buckets = None)")
        return ""

    def varlen_arena_bytes(self) -> Dict[tuple, int]:
        """Activation-arena bytes of every resident length-bucketed program, keyed (B, T_cap, F, device, precision, chains)."""
        return {k: 4 * b.acts.numel() for k, b in self._varlen_bound.items()}

    def _forward(self, inputs: tuple, out_shape: tuple, tax: int, lengths) -> torch.Tensor:
        """The forward of either network: ``inputs`` with the time axis ``tax`` -> its output arena of ``out_shape``
        ((B, 2, T, F) or (q, B, 2, T, F)), fp32.  Differentiable calls run the training programs, the
        others the exact-shape program or, with lengths= or length buckets, a per-utterance-length program."""
        x0, name = inputs[0], type(self).__name__
        noun = "input" if len(inputs) == 1 else "inputs"
        B, T, F = x0.shape[0], x0.shape[tax], x0.shape[tax + 1]
        needs_graph = self._needs_graph(*inputs)
        vl = self._varlen_call(T, B, lengths, needs_graph)
        if needs_graph:
            # training: forward AND backward on the hand-written kernels (train.py: two static op programs behind one
            # autograd node) for every supported configuration; BatchNorm = train mode (batch statistics + buffer update)
            from . import train
            if not (all(x.is_cuda for x in inputs) and next(self.parameters()).is_cuda):
                raise _lib.EabError(f"eabnet_amd.{name} trains on MI355X only: move the {noun} and the module to 'cuda'. "
                                    "There is no CPU fallback by design.")
            x_leaf = None
            if any(x.requires_grad for x in inputs):
                if not (self.input_grad and self._has_input_grad):
                    raise _refuse_differentiable(self, *self._input_grad_refusal)
                x_leaf = inputs[0].to(torch.float32).contiguous()      # (stays in the caller's graph: the cast gives x.grad its dtype)
            if self.norm_type == "BN" and not self.training:
                raise _refuse_differentiable(self, "BatchNorm in eval mode under autograd", "the training programs implement "
                                             "BatchNorm's train mode; call .train(), or torch.no_grad() for inference")
            lower = self._training_lowering()
            self.training_backend = "hip"
            xs = (x_leaf.detach(),) if x_leaf is not None else tuple(x.detach().to(torch.float32).contiguous() for x in inputs)
            if self.train_length_buckets is not None and vl is not None:
                return train.forward_train(self, xs, lower, lengths=vl[1], cap=vl[0], x_leaf=x_leaf)
            return train.forward_train(self, xs, lower, lengths=None if (vl is None or lengths is None) else vl[1], x_leaf=x_leaf)
        if not all(x.is_cuda for x in inputs):
            raise _lib.EabError(f"eabnet_amd.{name} inference runs on MI355X only: move the {noun} (and module) to "
                                "'cuda'. There is no CPU fallback by design.")
        _lib.load()
        xs = tuple(x.detach().to(torch.float32) for x in inputs)
        use_graph = self.use_graph and not self.dump_bfw and not torch.cuda.is_current_stream_capturing()
        with torch.cuda.device(x0.device):
            if vl is None:
                xs = tuple(x.contiguous() for x in xs)
                bound = self._program(B, T, F, x0.device)
                if use_graph and bound.capture(xs[0].shape, out_shape, xs[1].shape if len(xs) > 1 else None):
                    for buf, x in zip((bound.static_in, bound.static_in2), xs):
                        buf.copy_(x, non_blocking=True)
                    bound.graph.replay()
                    out = bound.static_out.clone()
                else:
                    out = torch.empty(out_shape, dtype=torch.float32, device=x0.device)
                    bound.bind(xs[0].data_ptr(), out.data_ptr(), xs[1].data_ptr() if len(xs) > 1 else None)
                    bound.run(torch.cuda.current_stream().cuda_stream)
            else:
                # per-utterance lengths: the program of cap T_cap, the lengths written to its device array on the launch
                # stream (pinned host copy or device-to-device, no host synchronisation), the inputs into its padded buffers
                T_cap, lens = vl
                bound = self._program(B, T_cap, F, x0.device, varlen=True)
                if isinstance(lens, int):
                    bound.lens.fill_(lens)
                elif isinstance(lens, torch.Tensor) and lens.is_cuda:
                    bound.lens.copy_(lens.to(torch.int32), non_blocking=True)
                else:
                    bound.lens.copy_(torch.as_tensor(lens, dtype=torch.int32).pin_memory(), non_blocking=True)
                pad = lambda shp, ax: tuple(shp[:ax]) + (T_cap,) + tuple(shp[ax + 1:])  # noqa: E731
                (b_in, b_out, b_in2), launch = bound.buffers(use_graph, pad(xs[0].shape, tax), pad(out_shape, -2),
                                                             pad(xs[1].shape, tax) if len(xs) > 1 else None)
                for buf, x in zip((b_in, b_in2), xs):
                    buf.narrow(tax, 0, T).copy_(x, non_blocking=True)
                launch()
                out = b_out[..., :T, :].clone()
                self._last_varlen = (b_in, b_out, b_in2)          # direct launches: keep the buffers alive
        self._last = (bound, *xs)                     # keep the inputs alive until the stream has consumed them
        return out

    # -- streaming ------------------------------------------------------------------
    def stream_begin(self, B: int, T_max: int, chunk: int = 1, F: int = 161, device=None, endless: bool = False) -> EaBNetStream:
        """Frame-synchronous inference (BASELINE config 5): returns a stream object whose
        ``step`` takes ``chunk`` new frames and returns the matching output frames (see EaBNetStream.step).
        Needs a configuration in which the network really is causal -- ``norm_type="BN"`` in eval mode (running
        statistics) or ``norm_type="cLN"`` (cumulative statistics), and ``is_causal=True`` -- and raises
        NotImplementedError otherwise.  ``T_max`` is the longest utterance the stream takes; with ``endless=True`` it is
        the resident window of a stream that takes frames forever (at least ``2 * history + chunk`` frames, ValueError
        otherwise; see EaBNetStream)."""
        if self.training:
            raise RuntimeError("stream_begin: call .eval() first (BatchNorm must use its running statistics)")
        _lib.load()
        device = torch.device(device) if device is not None else next(self.parameters()).device
        if device.type != "cuda":
            raise _lib.EabError("streaming inference runs on MI355X only: move the module to 'cuda'")
        if chunk < 1 or T_max < 1:
            raise ValueError("chunk and T_max must be positive")
        with torch.cuda.device(device):
            prog = prg.lower(self.cfg, self._numpy_params(), B, T_max, F, precision=self.precision, chunk=chunk)
            if endless and T_max < prog.min_window:
                raise ValueError(f"endless stream: a window of T_max={T_max} frames is too small, this network reads "
                                 f"{prog.history} frames back and needs at least {prog.min_window} "
                                 f"(2 * {prog.history} + chunk)")
            return EaBNetStream(self, _Bound(prog, device), B, T_max, F, chunk, endless)

    _has_input_grad = False      # the training lowering of this network takes input_grad=True (EaBNet)

    def _needs_graph(self, *inputs) -> bool:
        needs = torch.is_grad_enabled() and (any(x.requires_grad for x in inputs)
                                             or any(p.requires_grad for p in self.parameters()))
        return needs or (self.norm_type == "BN" and self.training)


class EaBNet(_HipModule):
    """MI355X implementation of the reference ``EaBNet`` (EaBNet.py:9-125).

    Same constructor keywords and defaults, same ``forward`` signature:
    ``inpt`` (B, T, F, M, 2) [or (B, T, F, 2) for one microphone] ->
    (B, 2, T, F), same state-dict keys.  ``torch.no_grad()`` / ``requires_grad=False`` calls run
    the hand-written HIP inference program; a call that must be differentiable (training: train.py /
    train_distributed.py:218-230) runs the HIP training programs (eabnet_amd/train.py: forward and
    backward as two static op programs behind one autograd node), so ``loss.backward()``, the optimiser,
    ``clip_grad_norm_`` and DistributedDataParallel work on the ordinary ``nn.Parameter``s.  CUDA
    tensors only; there is no second backend.  Refused (NotImplementedError): a gradient w.r.t. the input
    spectrogram unless ``input_grad = True`` is set (then ``x.grad`` comes from the same programs),
    BatchNorm in eval mode under autograd, more than 32 microphones.
    """

    def __init__(self, k1: tuple = (2, 3), k2: tuple = (1, 3), c: int = 64, M: int = 9, embed_dim: int = 64,
                 kd1: int = 5, cd1: int = 64, d_feat: int = 256, p: int = 6, q: int = 3, is_causal: bool = True,
                 is_u2: bool = True, bf_type: str = "lstm", topo_type: str = "mimo", intra_connect: str = "cat",
                 norm_type: str = "IN"):
        super().__init__()
        self.k1, self.k2, self.c, self.M, self.embed_dim = tuple(k1), tuple(k2), c, M, embed_dim
        self.kd1, self.cd1, self.d_feat, self.p, self.q = kd1, cd1, d_feat, p, q
        self.is_causal, self.is_u2, self.bf_type = is_causal, is_u2, bf_type
        self.topo_type, self.intra_connect, self.norm_type = topo_type, intra_connect, norm_type
        self.cfg = NetConfig(k1=tuple(k1), k2=tuple(k2), c=c, M=M, embed_dim=embed_dim, kd1=kd1, cd1=cd1,
                             d_feat=d_feat, p=p, q=q, is_causal=is_causal, is_u2=is_u2, bf_type=bf_type,
                             topo_type=topo_type, intra_connect=intra_connect, norm_type=norm_type)
        self._init_params(param_specs(self.cfg))     # raises NotImplementedError for unsupported topologies

    # -- forward -------------------------------------------------------------------
    def forward(self, inpt: torch.Tensor, lengths=None) -> torch.Tensor:
        """:param inpt: (B, T, F, M, 2) compressed multichannel spectrogram
        :param lengths: optional (B,) frame counts, 1 <= len <= T (causal configurations, inference): utterance b is
            inpt[b, :len[b]]; frames >= len[b] of the input are ignored and those of the output are zero
        :return: beamformed estimate (B, 2, T, F)   (reference EaBNet.py:88-117)"""
        if inpt.ndim == 4:
            inpt = inpt.unsqueeze(-2)
        if inpt.ndim != 5 or inpt.shape[-1] != 2 or inpt.shape[-2] != self.M:
            raise ValueError(f"expected (B,T,F,{self.M},2), got {tuple(inpt.shape)}")
        out = self._forward((inpt,), (inpt.shape[0], 2, inpt.shape[1], inpt.shape[2]), 1, lengths)
        if self.topo_type == "miso":
            # the reference reduces the masked reference-mic spectrum over frequency (EaBNet.py:122-123:
            # ``.sum(dim=-1)`` on a (B,T,F) tensor) and returns (B,2,T); kept as is
            out = out.sum(dim=-1)
        return out.to(inpt.dtype)

    _input_grad_refusal = ("the input requires grad", "the training programs produce parameter gradients only, as the "
                           "reference's training loop needs, unless the module's switch input_grad = True is set")
    _has_input_grad = True

    def _training_lowering(self):
        from . import train
        if not train.supported(self.cfg):
            raise _refuse_differentiable(self, "topology outside the training programs", train.unsupported_reason(self.cfg))
        return train.lower_train


class EaBNetStream:
    """Frame-synchronous inference state of one batch of utterances (``EaBNet.stream_begin``,
    ``GaGNet.stream_begin``).

    The activations of the whole utterance stay resident in HBM ([B][T_max][..] per layer; 288 GB make
    that cheap) and are the state: each ``step`` appends ``chunk`` frames of input, replays the captured
    program restricted to those time rows (eab_time_window: every kernel reads the frame position from
    device memory) and returns the new output frames.  Results are bit-identical to one offline call
    on the concatenated input, because every kernel computes a row independently of the tile or launch
    it falls into and the LSTM state is carried exactly.

    ``endless=True``: ``T_max`` is a resident window, not a limit.  A causal program reads a bounded number of earlier rows
    (``history``: 128 frames for the default S-TCN, Program.carry per tensor).  When the next step would pass the end of
    the window, the rows later steps can still read move to its front in one launch (eab_shift_rows_f32) and the stream
    goes on at row ``history``; no read then reaches below row 0, so "rows before 0 are causal padding" still means
    "before the start of the stream".  The frames stay those of one offline call on everything pushed since ``reset``."""

    def __init__(self, net, bound: _Bound, B: int, T_max: int, F: int, chunk: int, endless: bool = False):
        self.net, self.bound, self.B, self.T_max, self.F, self.chunk = net, bound, B, T_max, F, chunk
        self.endless = endless
        self.pos = 0                                  # row of the resident window the next frame goes to
        self._closed = False
        self.post = isinstance(net, GaGNet)           # post-filter: two planar inputs, q stage outputs
        if self.post:
            in_shape, out_shape, in2_shape = (B, 2, T_max, F), (net.q, B, 2, T_max, F), (B, 2, T_max, F)
        else:
            in_shape, out_shape, in2_shape = (B, T_max, F, net.M, 2), (B, 2, T_max, F), None
        (self._in, self._out, self._in2), self._launch = bound.buffers(net.use_graph, in_shape, out_shape, in2_shape)
        if endless:
            assert T_max >= bound.prog.min_window
            bound.upload_carry()

    @property
    def history(self) -> int:
        """frames back the farthest reader of the program looks (Program.history): what an endless stream keeps"""
        return self.bound.prog.history

    def reset(self) -> None:
        """Start a new batch of utterances (no buffer needs clearing: position 0 ignores all state)."""
        self.pos, self._closed = 0, False

    def step(self, x: torch.Tensor, pre_x: Optional[torch.Tensor] = None):
        """Beam-former: x (B, n, F, M, 2) new frames -> (B, 2, n, F) [(B, 2, n) for topo_type='miso'].
        Post-filter: x, pre_x (B, 2, n, F) -> list of q (B, 2, F, n).  n == chunk, except for the LAST step
        of an utterance (n < chunk): the recurrent state then sits past the end, so the stream accepts no
        further frames until ``reset``."""
        tdim = 2 if self.post else 1
        n = x.shape[tdim]
        if self._closed:
            raise RuntimeError("the previous step was a short final chunk: call reset() before the next utterance")
        want = (self.B, 2, n, self.F) if self.post else (self.B, n, self.F, self.net.M, 2)
        if tuple(x.shape) != want or not 0 < n <= self.chunk or (self.post and (pre_x is None or pre_x.shape != x.shape)):
            raise ValueError(f"expected {want} with n <= {self.chunk}, got {tuple(x.shape)}")
        if not self.endless and self.pos + n > self.T_max:
            raise ValueError(f"utterance longer than the T_max={self.T_max} given to stream_begin")
        if not x.is_cuda:
            raise _lib.EabError("stream.step needs CUDA (ROCm) tensors; there is no CPU fallback by design.")
        if self.endless and self.pos + self.chunk > self.T_max:
            with torch.cuda.device(x.device):         # on the launch stream, between two replays of the step's graph
                self.pos = self.bound.rebase(self.pos, torch.cuda.current_stream().cuda_stream)
        lo, hi, end = self.pos, self.pos + n, self.pos + self.chunk
        with torch.cuda.device(x.device), torch.no_grad():
            for buf, src in ((self._in, x), (self._in2, pre_x)):
                if buf is None:
                    continue
                buf.narrow(tdim, lo, n).copy_(src, non_blocking=True)
                if n < self.chunk and end > hi:       # rows the kernels touch beyond the new frames must be defined
                    buf.narrow(tdim, hi, min(end, self.T_max) - hi).zero_()
            self.bound.t_pos.fill_(lo)
            self._launch()
            out = self._out[..., lo:hi, :].clone()
        self.pos += n
        self._closed = n < self.chunk
        if self.post:
            out = out.to(x.dtype)
            return [out[j].permute(0, 1, 3, 2) for j in range(self.net.q)]
        if self.net.topo_type == "miso":
            out = out.sum(dim=-1)
        return out.to(x.dtype)


def _replica(module: nn.Module) -> nn.Module:
    """A second handle on the same parameters with its own lowered-program cache (own activation arena, boundary
    buffers and hipGraph): shallow copies down the module tree, ``nn.Parameter`` objects shared."""
    import copy
    rep = copy.copy(module)
    rep._modules = {k: (_replica(v) if v is not None else None) for k, v in module._modules.items()}
    if isinstance(rep, _HipModule):
        rep._bound, rep._packed_version = OrderedDict(), {}
        # the Pipeline serves exact shapes (its replicas own their programs; length buckets stay with the original module)
        rep.length_buckets, rep._varlen_bound, rep._varlen_version = None, OrderedDict(), {}
        rep.__dict__.pop("_slot_list", None)
    return rep


_PIPE_STREAMS: Dict[tuple, list] = {}


def _sync_knobs(src: nn.Module, rep: nn.Module) -> None:
    for k in ("precision", "use_graph", "training"):
        if k in src.__dict__:
            rep.__dict__[k] = src.__dict__[k]
    for name, child in src._modules.items():
        if child is not None:
            _sync_knobs(child, rep._modules[name])


class Pipeline:
    """Throughput executor: keeps ``depth`` batches in flight on ``depth`` HIP streams, each through its own
    replica of the model (own captured program, activations and boundary buffers; shared parameters).  One
    program alone leaves capacity idle -- the LSTM occupies 161 of 256 CUs for a fifth of the step, the S-TCM
    launches 112, every kernel ends in a partial round of workgroups -- and a second, independent batch fills
    it: 9.06 -> 7.48 ms per 16-utterance step in exact fp32, 5.74 -> 4.49 ms in f16x3 (deeper pipelines add
    nothing).  Results come back in submission order and are bit-identical to calling the model directly.
    Works for ``EaBNet``, ``GaGNet`` (two inputs) and ``EaBNetWithPostNet``; inference only.

        pipe = Pipeline(net, depth=2, front_end=(320, 160, torch.hann_window(320)))
        for wav in batches:            # (B, M, L) waves; without front_end: whatever the model takes
            if pipe.outstanding == pipe.depth:
                y = pipe.collect()     # what model(x) returns, ordered on the current stream
            pipe.submit(wav)
        while pipe.outstanding: y = pipe.collect()
    """

    def __init__(self, model: nn.Module, depth: int = 2, front_end: Optional[tuple] = None, prepare=None):
        """front_end = (fft_num, hop, window): ``submit(wav)`` takes (B, M, L) waves -- on the device, or in HOST memory: the
        upload then goes through the pinned staging ring on its own copy stream and overlaps the batches already in flight.
        prepare = the ``args`` of ``prepare_data`` (train_distributed.py:68-95): ``submit(x, target)`` takes what the
        reference's loader yields (host or device), runs ``prepare_data`` on the slot's stream and ``collect()`` returns
        ``(model(noisy_stft), target_stft)`` -- the reference's step with its host-to-device copies hidden behind compute."""
        if depth < 1:
            raise ValueError("depth must be >= 1")
        if front_end is not None and prepare is not None:
            raise ValueError("front_end and prepare are alternatives")
        self.model, self.depth, self.front_end, self.prepare = model, depth, front_end, prepare
        self._replicas = [_replica(model) for _ in range(depth)] if depth > 1 else [model]
        if depth > 1:
            # with several batches in flight the post-filter's three S-TCM chains run back to back: the
            # parallelism comes from the other batch, and hipGraphs with internal branches do not overlap
            # each other (two-stage step 13.99 -> 12.13 ms; with branches kept: no gain at all)
            for rep in self._replicas:
                for m in rep.modules():
                    if isinstance(m, GaGNet):
                        m.parallel_chains = False
        self._streams: list = []
        self._pending: list = []
        self._n = 0

    @property
    def outstanding(self) -> int:
        return len(self._pending)

    @staticmethod
    def _tensors(obj):
        if torch.is_tensor(obj):
            yield obj
        elif isinstance(obj, dict):
            for v in obj.values():
                yield from Pipeline._tensors(v)
        elif isinstance(obj, (list, tuple)):
            for v in obj:
                yield from Pipeline._tensors(v)

    def submit(self, *inputs: torch.Tensor) -> None:
        """Enqueue one batch (the model's positional inputs, or the front end's: see __init__); returns immediately.  At most
        ``depth`` batches may be outstanding.  Host tensors are accepted where a front end takes them (waves): they are staged
        through the pinned ring, so the caller may refill its buffer as soon as submit returns."""
        if self.outstanding >= self.depth:
            raise RuntimeError("collect() a result before submitting more than `depth` batches")
        if not inputs:
            raise ValueError("nothing to submit")
        takes_host = self.front_end is not None or self.prepare is not None
        if not takes_host and not all(x.is_cuda for x in inputs):
            raise _lib.EabError("Pipeline.submit needs CUDA (ROCm) tensors (host waves only with front_end= / prepare=); "
                                "there is no CPU fallback by design.")
        dev_in = next((x.device for x in inputs if x.is_cuda), None)
        device = dev_in if dev_in is not None else next(self.model.parameters()).device
        if device.type != "cuda":
            raise _lib.EabError("Pipeline runs on MI355X only: move the module to 'cuda'. There is no CPU fallback by design.")
        with torch.cuda.device(device):
            if not self._streams:
                # one set of streams per (device, depth) for the whole process: HIP maps streams onto a few
                # hardware queues in creation order, and two streams that land on the same queue do not overlap
                # (observed: a later Pipeline with freshly created streams gained nothing)
                key = (str(device), self.depth)
                if key not in _PIPE_STREAMS:
                    from .graphs import overlapping_streams
                    _PIPE_STREAMS[key] = overlapping_streams(device, self.depth)   # (probed: on distinct hardware queues)
                self._streams = _PIPE_STREAMS[key]
            if takes_host and not all(x.is_cuda for x in inputs):
                _stager(device).run_beside(self._streams)              # the upload stream on a hardware queue of its own
            slot = self._n % self.depth
            self._n += 1
            st = self._streams[slot]
            st.wait_stream(torch.cuda.current_stream())            # device inputs were produced on the caller's stream
            extra = None
            with torch.cuda.stream(st), torch.no_grad():
                for x in inputs:
                    if x.is_cuda:
                        x.record_stream(st)
                if self.prepare is not None:
                    if len(inputs) != 2:
                        raise ValueError("prepare=: submit(x (B,M,L), target (B,1,L))")
                    noisy, extra = prepare_data(inputs[0], inputs[1], device, self.prepare)     # uploads + both STFTs on `st`
                    inputs = (noisy,)
                elif self.front_end is not None:
                    fft_num, hop, window = self.front_end
                    wav, consumed = _upload(inputs[0], device)     # (device tensors pass through)
                    spec = stft_compress(wav, fft_num, hop, window)
                    if consumed is not None:
                        consumed.record(st)                        # the staged wave has no reader after the STFT
                    inputs = (spec,) + tuple(inputs[1:])
                rep = self._replicas[slot]
                if rep is not self.model:
                    _sync_knobs(self.model, rep)                   # precision / use_graph / train-eval follow the model
                out = rep(*inputs)
                ev = torch.cuda.Event()
                ev.record(st)
            self._pending.append((out if extra is None else (out, extra), ev, inputs))

    def calibrate(self, *inputs: torch.Tensor, tries: int = 4, steps: int = 6) -> float:
        """Optional, once per process and depth: whether two streams overlap depends on how the runtime maps them
        onto hardware queues.  Times ``steps`` pipelined batches on up to ``tries`` candidate stream sets and keeps
        the fastest (also for later pipelines of this depth).  Returns its seconds per batch."""
        import time
        if self.depth == 1:
            return 0.0
        device = next((x.device for x in inputs if x.is_cuda), None) or next(self.model.parameters()).device
        key = (str(device), self.depth)
        best, best_streams = None, None
        for attempt in range(tries):
            if attempt > 0 or not self._streams:
                with torch.cuda.device(device):
                    torch.cuda.synchronize(device)
                    self._streams = [torch.cuda.Stream(device=device) for _ in range(self.depth)]
            for _ in range(self.depth + 1):                  # programs lowered / captured, caches warm
                self.submit(*inputs)
                self.collect()
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(steps):
                if self.outstanding == self.depth:
                    self.collect()
                self.submit(*inputs)
            while self._pending:
                self.collect()
            torch.cuda.synchronize(device)
            dt = (time.perf_counter() - t0) / steps
            if best is None or dt < best:
                best, best_streams = dt, self._streams
            if attempt == 0:
                first = dt
            elif best < 0.9 * first or attempt >= 1 and abs(dt - first) < 0.03 * first:
                break                                        # clearly better found, or nothing changes: stop
        self._streams = _PIPE_STREAMS[key] = best_streams
        return best

    def collect(self):
        """The oldest outstanding result; the caller's current stream is ordered behind its computation."""
        if not self._pending:
            raise RuntimeError("nothing outstanding")
        out, ev, _ = self._pending.pop(0)
        first = next(self._tensors(out))
        cur = torch.cuda.current_stream(first.device)
        cur.wait_event(ev)
        for t in self._tensors(out):
            t.record_stream(cur)
        return out

    def map(self, batches):
        """Generator over the results of ``batches`` in order, with ``depth`` of them in flight."""
        for x in batches:
            if self.outstanding == self.depth:
                yield self.collect()
            self.submit(*(x if isinstance(x, (tuple, list)) else (x,)))
        while self._pending:
            yield self.collect()


class GaGNet(_HipModule):
    """MI355X implementation of the reference post-filter ``GaGNet`` (GaGNet.py:5-90): same
    constructor keywords, same state-dict keys, ``forward(inpt, pre_x)`` with both (B, 2, T, F)
    returning the list of the q stage estimates, each (B, 2, F, T).  Inference runs the HIP program
    (U2-encoder on the conv kernels, 24 single-branch S-TCMs per stage, fused gain/residual tail);
    a call that needs autograd runs the HIP training programs (eabnet_amd/train_gag.py)."""

    def __init__(self, cin: int = 2, k1: tuple = (2, 3), k2: tuple = (1, 3), c: int = 64, kd1: int = 3, cd1: int = 64,
                 d_feat: int = 256, p: int = 2, q: int = 3, dilas=(1, 2, 5, 9), fft_num: int = 320, is_u2: bool = True,
                 is_causal: bool = True, is_squeezed: bool = False, acti_type: str = "sigmoid",
                 intra_connect: str = "cat", norm_type: str = "IN"):
        super().__init__()
        self.cin, self.k1, self.k2, self.c, self.kd1, self.cd1 = cin, tuple(k1), tuple(k2), c, kd1, cd1
        self.d_feat, self.p, self.q, self.dilas, self.fft_num = d_feat, p, q, list(dilas), fft_num
        self.is_u2, self.is_causal, self.is_squeezed = is_u2, is_causal, is_squeezed
        self.acti_type, self.intra_connect, self.norm_type = acti_type, intra_connect, norm_type
        self.cfg = GagConfig(cin=cin, k1=tuple(k1), k2=tuple(k2), c=c, kd1=kd1, cd1=cd1, d_feat=d_feat, p=p, q=q,
                             dilas=tuple(dilas), fft_num=fft_num, is_u2=is_u2, is_causal=is_causal,
                             is_squeezed=is_squeezed, acti_type=acti_type, intra_connect=intra_connect,
                             norm_type=norm_type)
        self._init_params(gag_param_specs(self.cfg))

    def forward(self, inpt: torch.Tensor, pre_x: torch.Tensor, lengths=None) -> list:
        """:param inpt, pre_x: (B, 2, T, F) noisy reference-microphone spectrum and previous estimate
        :param lengths: optional (B,) frame counts, 1 <= len <= T (causal configurations, inference); frames >= len[b] of
            the inputs are ignored and those of every estimate are zero
        :return: list of q estimates (B, 2, F, T)   (reference GaGNet.py:76-90)"""
        if inpt.ndim != 4 or inpt.shape[1] != 2 or inpt.shape[3] != self.cfg.freq or pre_x.shape != inpt.shape:
            raise ValueError(f"expected two (B,2,T,{self.cfg.freq}) tensors, got {tuple(inpt.shape)} and {tuple(pre_x.shape)}")
        out = self._forward((inpt, pre_x), (self.q,) + tuple(inpt.shape), 2, lengths).to(inpt.dtype)
        return [out[j].permute(0, 1, 3, 2) for j in range(self.q)]

    # no gradient flows to the inputs: the reference feeds the detached beam-former estimate (EaBNet.py:142)
    _input_grad_refusal = ("an input requires grad", "the reference detaches the beam-former's estimate, EaBNet.py:142; the "
                           "training programs produce parameter gradients only")

    def _training_lowering(self):
        from . import train_gag
        if not train_gag.supported(self.cfg):
            raise _refuse_differentiable(self, "post-filter topology outside the training programs", "see train_gag.supported")
        return train_gag.lower_train


def make_gag_net(args) -> GaGNet:
    """Reference GaGNet.py:651-671 (reads the ``gagnet_*`` fields of ``args``), on cuda:current."""
    return GaGNet(cin=2, k1=args.gagnet_k1, k2=args.gagnet_k2, c=args.gagnet_c, kd1=args.gagnet_kd1, cd1=args.gagnet_cd1,
                  d_feat=args.gagnet_d_feat, p=args.gagnet_p, q=args.gagnet_q, dilas=args.gagnet_dilas,
                  fft_num=args.gagnet_fft_num, is_u2=args.gagnet_is_u2, is_causal=args.gagnet_is_causal,
                  is_squeezed=args.gagnet_is_squeezed, acti_type=args.gagnet_acti_type,
                  intra_connect=args.gagnet_intra_connect, norm_type=args.gagnet_norm_type).cuda()


class EaBNetWithPostNet(nn.Module):
    """Reference EaBNet.py:127-155: beam-former, then the GaGNet post-filter on (reference microphone,
    detached beam-former estimate).  Same ``args`` fields, ``eabnet.`` / ``postnet.`` key prefixes and
    output dictionary."""

    def __init__(self, args):
        super().__init__()
        self.eabnet = EaBNet(k1=args.k1, k2=args.k2, c=args.c, M=args.M, embed_dim=args.embed_dim, kd1=args.kd1,
                             cd1=args.cd1, d_feat=args.d_feat, p=args.p, q=args.q, is_causal=args.is_causal,
                             is_u2=args.is_u2, bf_type=args.bf_type, topo_type=args.topo_type,
                             intra_connect=args.intra_connect, norm_type=args.norm_type)
        self.ref_mic = args.ref_mic
        self.postnet = make_gag_net(args)
        if args.freeze_eabnet:
            self.freeze_eabnet()

    @property
    def length_buckets(self):
        """length buckets of both stages (see EaBNet.length_buckets)"""
        return self.eabnet.length_buckets

    @length_buckets.setter
    def length_buckets(self, value) -> None:
        self.eabnet.length_buckets = value
        self.postnet.length_buckets = value

    @property
    def train_length_buckets(self):
        """length buckets of both stages for differentiable calls (see EaBNet.train_length_buckets)"""
        return self.eabnet.train_length_buckets

    @train_length_buckets.setter
    def train_length_buckets(self, value) -> None:
        self.eabnet.train_length_buckets = value
        self.postnet.train_length_buckets = value

    @property
    def varlen_training(self):
        """lengths= under autograd, both stages (see EaBNet.varlen_training; the post-filter refuses it with the reason)"""
        return self.eabnet.varlen_training

    @varlen_training.setter
    def varlen_training(self, value) -> None:
        self.eabnet.varlen_training = value
        self.postnet.varlen_training = value

    def forward(self, noisy_stft: torch.Tensor, lengths=None) -> dict:
        """lengths: optional (B,) frame counts, passed to both stages (EaBNet.forward)"""
        if lengths is not None and isinstance(lengths, torch.Tensor) and not lengths.is_cuda:
            lengths = lengths.tolist()                                          # validated once per stage, host values
        esti0_stft = self.eabnet(noisy_stft, lengths=lengths)
        inpt = noisy_stft[..., self.ref_mic, :].permute(0, 3, 1, 2)            # 'b t f c -> b c t f'
        esti1_stft_list = self.postnet(inpt, esti0_stft.detach(), lengths=lengths)
        return {"esti0_stft": esti0_stft, "esti1_stft_list": esti1_stft_list,
                "esti_stft": esti1_stft_list[-1].permute(0, 1, 3, 2)}

    def freeze_eabnet(self) -> None:
        for p in self.eabnet.parameters():
            p.requires_grad = False

    def stream_begin(self, B: int, T_max: int, chunk: int = 1, endless: bool = False) -> "TwoStageStream":
        """Frame-synchronous two-stage inference: both stages need BatchNorm norms and causal S-TCMs.  endless: T_max is
        the resident window of both stages, each of which moves its own rows when it reaches the end (EaBNetStream)."""
        return TwoStageStream(self, self.eabnet.stream_begin(B, T_max, chunk, endless=endless),
                              self.postnet.stream_begin(B, T_max, chunk, endless=endless))


class TwoStageStream:
    """EaBNetWithPostNet.forward (EaBNet.py:138-148) chunk by chunk: beam-former step, then post-filter
    step on (reference microphone, estimate)."""

    def __init__(self, net: EaBNetWithPostNet, first: EaBNetStream, second: EaBNetStream):
        self.net, self.first, self.second = net, first, second

    def reset(self) -> None:
        self.first.reset()
        self.second.reset()

    def step(self, noisy: torch.Tensor) -> dict:
        esti0 = self.first.step(noisy)
        inpt = noisy[..., self.net.ref_mic, :].permute(0, 3, 1, 2)
        lst = self.second.step(inpt, esti0)
        return {"esti0_stft": esti0, "esti1_stft_list": lst, "esti_stft": lst[-1].permute(0, 1, 3, 2)}


class _DecompressType(type):
    """``Enhancer(..., decompress=True)``, ``Scorer(...)``, ``StreamingEnhancer(...)``: the switch is a keyword of the class call
    (what ``inspect.signature`` of the class shows), not of ``__init__``, whose parameter lists are pinned
    (tests/test_resample_ref.py::test_defaults_of_the_tools_are_unchanged).  It must be a bool; the instance attribute
    ``decompress`` is what the ``istft`` calls of the tool are given.  False leaves the instance as ``__init__`` made it."""

    def __call__(cls, *args, decompress: bool = False, **kw):
        if not isinstance(decompress, bool):
            raise TypeError(f"decompress must be a bool, got {type(decompress).__name__}")
        self = super().__call__(*args, **kw)
        if decompress:
            self.decompress = True
        return self


class StreamingEnhancer(metaclass=_DecompressType):
    """enhance.py:45-62 as a real-time loop on the device: ``push`` takes the next ``chunk`` hops of
    multichannel samples (B, M, chunk*hop) and returns the enhanced samples that became final.

    Frame t of the centred STFT needs samples up to (t+1)*hop and output segment k of the ISTFT needs frames
    k and k+1, so the enhanced wave trails the input by two hops (20 ms at 16 kHz) plus the compute time of a
    step.  Front and back end are the offline kernels on short windows (a frame / segment is computed
    identically wherever its window starts), so the streamed wave is bit-identical to the offline
    wave -> prepare_data -> model -> istft chain.

    ``sample_rate`` (None: ``sr``): the rate of the pushed samples.  ``push`` then takes chunk*hop*sample_rate/sr samples per
    call; a ``StreamResampler`` turns them into ``sr`` samples (bit for bit those of the offline ``resample``), which queue up
    until a whole chunk*hop block is there for the push logic above.  The output (at ``sr``) trails the input by the filter's
    half-width more -- 19 samples at 48 kHz, 0.4 ms -- so the first call returns one block less and ``last=True`` returns the
    rest.  ``mic_order``: the microphones of the pushed samples in the model's order.

    ``StreamingEnhancer(..., decompress=True)`` (a bool, default False: the reference's wave) is passed to the ``istft`` call
    of every push: True undoes the front end's sqrt compression, so the streamed wave is an estimate of the signal in the
    clean files, bit for bit the offline chain with ``istft(decompress=True)``."""

    decompress = False

    def __init__(self, model, B: int, seconds: float, chunk: int = 1, sr: int = 16000, fft_num: int = 320, hop: int = 160,
                 endless: bool = False, sample_rate: Optional[int] = None, mic_order=None):
        """seconds: the longest stream; with endless=True the resident window of a stream of any length (see
        EaBNetStream: it must hold twice the network's history plus a chunk)."""
        import importlib
        _rs = importlib.import_module(__package__ + ".resample")     # (the package's attribute `resample` is the function)
        self._rs, self._push_in = None, chunk * hop
        self._order = None if mic_order is None else list(_rs.check_mic_order(mic_order, 1 << 30))
        if sample_rate is not None and int(sample_rate) != int(sr):
            o, n = _rs._ratio(sample_rate, sr)
            if (chunk * hop * o) % n:
                raise ValueError(f"push takes chunk*hop*{o}/{n} = {chunk * hop * o / n} samples at {sample_rate} Hz per call: "
                                 f"not a whole number; choose a chunk that makes it one")
            self._rs, self._push_in = _rs.StreamResampler(sample_rate, sr), chunk * hop * o // n
        self.model, self.B, self.chunk, self.fft, self.hop = model, B, chunk, fft_num, hop
        self.T_max = 1 + int(seconds * sr) // hop
        self.stream = model.stream_begin(B, self.T_max, chunk, endless=endless)
        self.window = torch.hann_window(fft_num)
        self.reset()

    def reset(self) -> None:
        self.stream.reset()
        self._tail = None          # the last hop samples (B, M, hop): left half of the next frame
        self._hold = None          # samples of a first push too short to form frame 0
        self._frames = 0           # frames handed to the model so far
        self._spec_prev = None     # last estimate frame, for the overlap-add with the next one
        self._fifo = None          # resampled samples (B, M, < chunk*hop) waiting for a whole block
        if self._rs is not None:
            self._rs.reset()

    def push(self, samples: torch.Tensor, last: bool = False) -> torch.Tensor:
        """samples (B, M, n*hop), n == chunk (any 0 <= n <= chunk with last=True).  Returns (B, k*hop)
        enhanced samples, k = frames that became final in this call.  With ``sample_rate``: (B, M, chunk*hop*sample_rate/sr)
        samples per call (fewer with last=True, as long as the whole stream comes to whole hops at ``sr``)."""
        if self._order is not None:
            samples = samples[:, self._order]
        if self._rs is None:
            return self._push(samples, last)
        if samples.shape[2] > self._push_in or (samples.shape[2] != self._push_in and not last):
            raise ValueError(f"push takes {self._push_in} samples per call (fewer only with last=True)")
        new = self._rs.push(samples, last)
        fifo = new if self._fifo is None else torch.cat((self._fifo, new), dim=2)
        blk, outs = self.chunk * self.hop, []
        while fifo.shape[2] >= blk and not (last and fifo.shape[2] == blk):
            outs.append(self._push(fifo[:, :, :blk], False))
            fifo = fifo[:, :, blk:]
        if last:
            outs.append(self._push(fifo, True))               # the rest: at most one block
            fifo = None
        self._fifo = fifo
        outs = [y for y in outs if y.shape[1]]
        if not outs:
            return samples.new_zeros((samples.shape[0], 0))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)

    def _push(self, samples: torch.Tensor, last: bool) -> torch.Tensor:
        B, M, L = samples.shape
        if L % self.hop or L // self.hop > self.chunk or (L // self.hop != self.chunk and not last):
            raise ValueError(f"push takes chunk*hop = {self.chunk * self.hop} samples per call (fewer only with last=True)")
        first = self._tail is None
        if first and self._hold is not None:
            samples, self._hold = torch.cat((self._hold, samples), dim=2), None
        if first and samples.shape[2] <= self.fft // 2 and not last:
            self._hold = samples                      # frame 0 reflects about sample 0 and needs sample fft_num/2
            return samples.new_zeros((B, 0))
        buf = samples if first else torch.cat((self._tail, samples), dim=2)
        # window of `buf`: as an utterance of its own, its interior frames are exact; its first frame is exact only
        # at the true start (reflection), its last one only at the true end
        if buf.shape[2] <= self.fft // 2:
            raise ValueError("an utterance must be longer than fft_num/2 samples")
        spec = stft_compress(buf, self.fft, self.hop, self.window)                # (B, T', F, M, 2)
        lo = 0 if first else 1
        hi = spec.shape[1] if last else spec.shape[1] - 1
        new = spec[:, lo:hi]
        self._tail = buf[:, :, buf.shape[2] - self.hop:]       # the next window starts one hop before its first new frame
        outs = []
        for a in range(0, new.shape[1], self.chunk):
            blk = new[:, a:a + self.chunk]
            o = self.stream.step(blk)
            outs.append(o["esti_stft"] if isinstance(o, dict) else o)
        if not outs:
            return samples.new_zeros((B, 0))
        est = torch.cat(outs, dim=2)                                                # (B, 2, k, F)
        self._frames += est.shape[2]
        seq = est if self._spec_prev is None else torch.cat((self._spec_prev, est), dim=2)
        self._spec_prev = est[:, :, -1:].clone()
        if seq.shape[2] < 2:
            return samples.new_zeros((B, 0))
        return istft(seq, self.fft, self.hop, self.window, decompress=self.decompress)


def make_eabnet_with_postnet(args) -> EaBNetWithPostNet:
    """Reference EaBNet.py:815-816."""
    return EaBNetWithPostNet(args)


# ----------------------------------------------------------------------------
# front end and helpers
# ----------------------------------------------------------------------------
_TWIDDLE: Dict[Tuple[int, str], torch.Tensor] = {}
_WINDOW: Dict[tuple, torch.Tensor] = {}


def _device_window(window: torch.Tensor, device: torch.device) -> torch.Tensor:
    """The analysis/synthesis window on the device.  prepare_data builds it on the CPU on every call, as the
    reference does (train_distributed.py:83), and a pageable host-to-device copy blocks the host until the
    stream has drained -- one full pipeline bubble per step.  CPU windows are therefore cached by content."""
    if window.is_cuda:
        return window.to(device=device, dtype=torch.float32).contiguous()
    w = window.detach().to(torch.float32).contiguous()
    key = (str(device), w.numpy().tobytes())
    hit = _WINDOW.get(key)
    if hit is None:
        if len(_WINDOW) > 16:
            _WINDOW.clear()
        hit = _WINDOW[key] = w.to(device)
    return hit


def _twiddle(n_fft: int, device: torch.device) -> torch.Tensor:
    key = (n_fft, str(device))
    if key not in _TWIDDLE:
        k = np.arange(n_fft, dtype=np.float64)
        tw = np.stack([np.cos(2 * np.pi * k / n_fft), np.sin(2 * np.pi * k / n_fft)], axis=1).astype(np.float32)
        _TWIDDLE[key] = torch.from_numpy(tw).to(device)
    return _TWIDDLE[key]


def stft_compress(wav: torch.Tensor, n_fft: int, hop: int, window: torch.Tensor, layout: int = 0, lengths=None) -> torch.Tensor:
    """(B, M, L) -> (B, T, F, M, 2)  [layout 0]  or (B, 1, L) -> (B, 2, T, F)  [layout 1].

    lengths: optional (B,) sample counts, n_fft/2 < len <= L (a sequence or an integer tensor, host or device): utterance b
    is wav[b, :, :len[b]] and the rest of its rows is padding.  Its 1 + len[b] // hop frames are those of a call on that
    utterance alone, bit for bit (the last frames reflect about ITS last sample); the frames after them are zeros.

    Differentiable: with grad enabled and ``wav.requires_grad`` the same launch runs inside an autograd node (the same bits)
    whose backward is the adjoint kernel eab_stft_compress_bwd_f32 on the same window and lengths; the
    gradient has the wave's dtype.  At a bin that is exactly zero -- a silent microphone, digital silence -- the compression
    X |X|^-1/2 has an unbounded derivative and torch's own autograd returns NaN; this backward returns an exact (0, 0) there, so
    the gradient of a wave with silent stretches stays finite.  More than 8 overlapping frames (ceil(n_fft / hop) > 8), or an
    n_fft / 2 with a prime factor other than 2 and 5, are refused under autograd, as ``istft`` refuses them."""
    if lengths is not None:
        lengths = check_lengths(lengths, wav.shape[0], wav.shape[2], lo=n_fft // 2 + 1, unit="n_fft/2 < samples <= L", integral=True)
    if not wav.is_cuda:
        raise _lib.EabError("stft_compress needs a CUDA (ROCm) tensor; there is no CPU fallback by design.")
    if torch.is_grad_enabled() and wav.requires_grad:
        if hop > n_fft or -(-n_fft // hop) > 8:
            raise NotImplementedError("stft_compress under autograd: the adjoint kernel implements any hop <= n_fft with at most 8 "
                                      f"overlapping frames (ceil(n_fft / hop) in 1..8), got n_fft={n_fft}, hop={hop}; istft has "
                                      "the same limit")
        rest = n_fft // 2                             # (the factors of csrc/fft_lds.h: fft_plan)
        for r in (5, 2):
            while rest > 1 and rest % r == 0:
                rest //= r
        if n_fft % 2 or rest != 1:
            raise NotImplementedError(f"stft_compress under autograd: n_fft={n_fft} -- the adjoint kernel runs its transform on the "
                                      "LDS FFT, which needs an n_fft / 2 made of factors 2 and 5 (the forward's direct-DFT form has "
                                      "no adjoint yet)")
        return _StftCompress.apply(wav, _device_window(window, wav.device), lengths, n_fft, hop, layout)
    x = wav.to(torch.float32).contiguous()
    out = torch.empty(_stft_shape(x, n_fft, hop, layout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        lens = None if lengths is None else _device_lengths(lengths, x.device)
        _stft_launch(_lib.load(), x, _device_window(window, x.device), _twiddle(n_fft, x.device), out, lens, n_fft, hop, layout)
    return out


def _stft_shape(wav: torch.Tensor, n_fft: int, hop: int, layout: int) -> tuple:
    B, M, L = wav.shape
    T, F = 1 + L // hop, n_fft // 2 + 1
    return (B, T, F, M, 2) if layout == 0 else (B, 2, T, F)


def _stft_launch(lib, wav: torch.Tensor, window: torch.Tensor, tw: torch.Tensor, out: torch.Tensor, lens, n_fft: int, hop: int,
                 layout: int) -> None:
    """the one forward launch of ``stft_compress``, with and without autograd: fp32 contiguous wav (B, M, L); lens: the device
    sample counts or None"""
    B, M, L = wav.shape
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if lens is not None:
        _lib.check(lib.eab_stft_compress_lens_f32(wav.data_ptr(), window.data_ptr(), tw.data_ptr(), out.data_ptr(), lens.data_ptr(),
                                                  B, M, L, n_fft, hop, layout, stream), "eab_stft_compress_lens_f32")
    else:
        _lib.check(lib.eab_stft_compress_f32(wav.data_ptr(), window.data_ptr(), tw.data_ptr(), out.data_ptr(), B, M, L, n_fft, hop,
                                             layout, stream), "eab_stft_compress_f32")


class _StftCompress(torch.autograd.Function):
    """``stft_compress`` on a wave that requires grad: the forward is the launch ``stft_compress`` makes for any other input (the
    same values), the backward the adjoint kernel eab_stft_compress_bwd_f32 at the saved output, on the same window and, where
    given, the same lengths."""

    @staticmethod
    def forward(ctx, wav: torch.Tensor, window: torch.Tensor, lengths, n_fft: int, hop: int, layout: int) -> torch.Tensor:
        lib = _lib.load()
        x = wav.detach().to(torch.float32).contiguous()
        out = torch.empty(_stft_shape(x, n_fft, hop, layout), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            tw = _twiddle(n_fft, x.device)
            lens = None if lengths is None else _device_lengths(lengths, x.device)
            _stft_launch(lib, x, window, tw, out, lens, n_fft, hop, layout)
        ctx.save_for_backward(window, tw, out, *(() if lens is None else (lens,)))
        ctx.geom = (tuple(x.shape), n_fft, hop, layout, wav.dtype)
        return out

    @staticmethod
    def backward(ctx, dspec):
        window, tw, spec, *rest = ctx.saved_tensors
        (B, M, L), n_fft, hop, layout, dtype = ctx.geom
        lib = _lib.load()
        g = dspec.detach().to(torch.float32).contiguous()
        dwav = torch.empty((B, M, L), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            rc = lib.eab_stft_compress_bwd_f32(g.data_ptr(), spec.data_ptr(), window.data_ptr(), tw.data_ptr(), dwav.data_ptr(),
                                               rest[0].data_ptr() if rest else None, B, M, L, n_fft, hop, layout,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc == _lib.EAB_EUNSUPPORTED:
            raise NotImplementedError(f"stft_compress under autograd: n_fft={n_fft}, hop={hop} -- the adjoint kernel needs hop <= "
                                      "n_fft, at most 8 overlapping frames and an n_fft / 2 made of factors 2 and 5")
        _lib.check(rc, "eab_stft_compress_bwd_f32")
        return dwav.to(dtype), None, None, None, None, None


_COPY_POOL = None
_COPY_THREADS = 4


def _host_copy(dst: torch.Tensor, src: torch.Tensor) -> None:
    """dst.copy_(src) on the host; a large contiguous fp32 tensor is copied as _COPY_THREADS slices on worker threads (the copy
    is one memcpy per call and releases the GIL): the 33 MB of a batch of waves are 3.3 ms of ONE core otherwise, and on a busy host
    that single memcpy is what a pipelined step waits for."""
    global _COPY_POOL
    n = src.numel()
    if n < (1 << 21) or not (src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype):
        dst.copy_(src)
        return
    if _COPY_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _COPY_POOL = ThreadPoolExecutor(max_workers=_COPY_THREADS, thread_name_prefix="eab-stage")
    d, s_ = dst.view(-1), src.view(-1)
    step = (n + _COPY_THREADS - 1) // _COPY_THREADS
    futs = [_COPY_POOL.submit(d[a:a + step].copy_, s_[a:a + step]) for a in range(0, n, step)]
    for f in futs:
        f.result()


class _HostStager:
    """Host -> device path of ``prepare_data`` (train_distributed.py:76-77 does two blocking ``.to(device)``): a ring of
    pinned staging buffers and resident device buffers plus a dedicated copy stream.  The upload of batch k+1 is
    enqueued while batch k still computes and nothing on the path allocates or synchronises the device; a slot is
    reused only after the kernels that read its device buffer have been enqueued AND its previous copy completed."""

    # True: every host tensor is copied into the ring's own pinned slot first.  The direct path (the copy kernel reads the
    # caller's pinned buffer) measured SLOWER on MI355X (20 ms vs 10-12 ms per 32.8 MB batch, bench.py next_rows.pcie_inclusive)
    # and has to block until the read has finished, because nothing else protects a caller's pinned buffer from being refilled.
    always_stage = True

    def __init__(self, device: torch.device, depth: int = 4):
        # (one slot more than the deepest Pipeline keeps in flight: a slot is refilled only when its batch has been consumed)
        self.device, self.depth, self.k = device, depth, {}
        self.slots: Dict[tuple, list] = {}
        # high priority: the copy kernel is a few dozen workgroups that must get their CU slots while other batches compute --
        # on a normal-priority stream its workgroups queue behind the convolutions' and every pipeline slot waits for its upload
        self.stream = torch.cuda.Stream(device=device, priority=-1)
        self._beside: tuple = ()

    def run_beside(self, streams) -> None:
        """The copy stream must not share a hardware queue with a stream whose batches it feeds: a queue is in order, so an
        upload behind a whole program of another batch arrives a step late (measured: 7-9 ms per step became 17-22 whenever the
        creation-order lottery put the two together).  Picks -- once per set of streams -- a high-priority stream that a spin-kernel
        probe shows overlapping with all of them (graphs.overlapping_streams)."""
        key = tuple(s.cuda_stream for s in streams)
        if key == self._beside:
            return
        from .graphs import overlapping_streams
        torch.cuda.synchronize(self.device)
        self.stream = overlapping_streams(self.device, 1, beside=list(streams), priority=-1)[0]
        self._beside = key

    def upload(self, t: torch.Tensor, role: int = 0) -> Tuple[torch.Tensor, "torch.cuda.Event"]:
        """CPU tensor -> contiguous fp32 device tensor, ordered on the CURRENT stream.  Returns (tensor, consumed):
        record `consumed` on the current stream after the last kernel that reads the tensor has been enqueued.
        role: which input of the step this is (x = 0, target = 1) -- inputs of equal shape (one microphone) keep their own rings."""
        key = (role,) + tuple(t.shape)
        ring = self.slots.get(key)
        if ring is None:
            if len(self.slots) > 8:
                torch.cuda.synchronize(self.device)
                self.slots.clear()
                self.k.clear()
            ring = self.slots[key] = [dict(pin=torch.empty(key[1:], dtype=torch.float32).pin_memory(),
                                           dev=torch.empty(key[1:], dtype=torch.float32, device=self.device),
                                           copied=torch.cuda.Event(), consumed=torch.cuda.Event(), used=False)
                                      for _ in range(self.depth)]
        # (one counter per ring: x and target of a step use different rings -- a shared counter walked each of them with a
        # stride of two, i.e. gave a pipeline of three batches TWO slots per ring and made submit() wait for the GPU)
        self.k[key] = self.k.get(key, 0) + 1
        slot = ring[self.k[key] % self.depth]
        if slot["used"]:
            slot["copied"].synchronize()                 # the pinned buffer is free again (depth steps ago)
            self.stream.wait_event(slot["consumed"])     # the device buffer's readers were enqueued before this
        else:
            # first use of a slot: its device buffer is fresh from the caching allocator, which hands out blocks freed on the
            # launch stream while kernels queued there may still write them -- the copy must not overtake those
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
        src = t
        if self.always_stage or not (t.is_pinned() and t.is_contiguous() and t.dtype == torch.float32):
            _host_copy(slot["pin"], t)                   # pageable / strided / other dtype: one host pass into pinned memory
            src = slot["pin"]
        with torch.cuda.stream(self.stream):
            # a copy KERNEL reading the pinned buffer over the bus (device-visible under unified addressing), not
            # hipMemcpyAsync: DMA copies submitted between compute kernels cost milliseconds each on this stack
            _lib.check(_lib.load().eab_copy_f32(src.data_ptr(), slot["dev"].data_ptr(), src.numel(), C.c_void_p(self.stream.cuda_stream)),
                       "eab_copy_f32")
            slot["copied"].record(self.stream)
        torch.cuda.current_stream(self.device).wait_event(slot["copied"])
        slot["used"] = True
        if src is t:
            # the copy kernel reads the CALLER's pinned buffer: nothing ties that buffer's contents or lifetime to our side
            # stream (a reused pinned batch, a DataLoader(pin_memory=True) block recycled for the next batch), so return only
            # when the read has finished -- what the reference's blocking x.to(device) gives (train_distributed.py:76-77)
            slot["copied"].synchronize()
        return slot["dev"], slot["consumed"]


_STAGERS: Dict[str, _HostStager] = {}


def _stager(device: torch.device) -> _HostStager:
    st = _STAGERS.get(str(device))
    if st is None:
        st = _STAGERS[str(device)] = _HostStager(device)
    return st


def _upload(t: torch.Tensor, device: torch.device, role: int = 0):
    """(device tensor, event to record after its consumers) for any input of prepare_data"""
    if t.is_cuda:
        return t.to(device), None
    return _stager(device).upload(t, role)


def prepare_data(x: torch.Tensor, target: torch.Tensor, device, args):
    """Reference train_distributed.py:68-95.  ``args`` provides mics, sr,
    wav_len, win_size, win_shift (seconds) and fft_num.
    x (B, M, L), target (B, 1, L) -> noisy_stft (B, T, F, M, 2), target_stft (B, 2, T, F)."""
    sr = args.sr
    win_size = int(args.win_size * sr)
    win_shift = int(args.win_shift * sr)
    fft_num = args.fft_num
    if win_size > fft_num:
        raise RuntimeError(f"win_size ({win_size} samples) must not exceed fft_num ({fft_num}), as in torch.stft")
    batch_size = x.shape[0]
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(device):
        xd, ev_x = _upload(x, device)
        td, ev_t = _upload(target, device, 1)
        noisy_wav = xd.contiguous().view(batch_size, args.mics, -1)
        target_wav = td.reshape(batch_size, 1, -1)
        window = torch.hann_window(win_size)
        if win_size < fft_num:                        # torch.stft(win_length < n_fft): zero-padded on both sides, centred
            left = (fft_num - win_size) // 2
            window = torch.nn.functional.pad(window, (left, fft_num - win_size - left))
        noisy_stft = stft_compress(noisy_wav, fft_num, win_shift, window, 0)
        target_stft = stft_compress(target_wav, fft_num, win_shift, window, 1)
        for ev in (ev_x, ev_t):
            if ev is not None:
                ev.record(torch.cuda.current_stream(device))         # the staged waves have no reader after this point
    return noisy_stft, target_stft


_NOLA: Dict[tuple, object] = {}            # verdict; for a device window (verdict, the keyed tensor)


def _check_nola(window: torch.Tensor, fft_num: int, hop: int, T: int, key_window: Optional[torch.Tensor] = None) -> None:
    """torch.istft's window-overlap condition, on the host, before the kernel divides by the envelope: the squared-window
    overlap-add over the frames that exist must stay above 1e-11 at every output sample (a short zero-padded window with a
    large hop leaves gaps).  The envelope's two rims and its interior (periodic in the hop, whether or not the hop divides
    fft_num) are those of a signal of 2R+2 frames, R = ceil(fft_num / hop).  key_window: the caller's tensor that ``window`` was
    padded from (a device window's verdict is cached under the tensor the caller holds, not under the padded temporary)."""
    frames = min(T, 2 * -(-fft_num // hop) + 2)
    src = window if key_window is None else key_window
    if src.is_cuda:
        # a device window is keyed by its storage and version counter and copied to the host on a miss only (inside a training
        # step the copy would be a device synchronisation per step).  The entry keeps the keyed tensor alive, so its address
        # cannot pass to another window while the verdict is cached; an in-place write bumps _version.
        key = (str(src.device), src.data_ptr(), src._version, src.numel(), tuple(src.stride()), fft_num, hop, frames)
        hit = _NOLA.get(key)
        ok = None if hit is None else hit[0]
    else:
        w = window.detach().to(torch.float64).numpy()                        # (already zero-padded to fft_num by the caller)
        key = (w.tobytes(), fft_num, hop, frames)                            # by content: a pointer can be reused by another window
        ok = _NOLA.get(key)
    if ok is None:
        if src.is_cuda:
            w = window.detach().to("cpu", torch.float64).numpy()
        w2 = w ** 2
        Te = frames
        env = np.zeros(fft_num + hop * (Te - 1))
        for t in range(Te):
            env[t * hop:t * hop + fft_num] += w2
        trimmed = env[fft_num // 2:fft_num // 2 + hop * (Te - 1)]
        ok = bool(trimmed.size == 0 or np.abs(trimmed).min() > 1e-11)
        if len(_NOLA) > 64:
            _NOLA.clear()
        _NOLA[key] = (ok, src) if src.is_cuda else ok
    if not ok:
        raise RuntimeError("istft: window overlap add min is below 1e-11 (the NOLA condition of torch.istft fails for this "
                           f"window / hop: fft_num={fft_num}, win_shift={hop})")


def _istft_launch(lib, x: torch.Tensor, window: torch.Tensor, tw: torch.Tensor, wav: torch.Tensor, lens, fft_num: int, hop: int,
                  decompress: bool) -> None:
    """the one forward launch of ``istft``, with and without autograd: fp32 contiguous x (B, 2, T, F) -> wav (B, hop (T-1));
    lens: the device frame counts or None"""
    B, _, T, _ = x.shape
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if decompress:
        _lib.check(lib.eab_istft_lin_f32(x.data_ptr(), window.data_ptr(), tw.data_ptr(), wav.data_ptr(),
                                         None if lens is None else lens.data_ptr(), B, T, fft_num, hop, stream), "eab_istft_lin_f32")
    elif lens is not None:
        _lib.check(lib.eab_istft_lens_f32(x.data_ptr(), window.data_ptr(), tw.data_ptr(), wav.data_ptr(), lens.data_ptr(),
                                          B, T, fft_num, hop, stream), "eab_istft_lens_f32")
    else:
        _lib.check(lib.eab_istft_f32(x.data_ptr(), window.data_ptr(), tw.data_ptr(), wav.data_ptr(), B, T, fft_num, hop, stream),
                   "eab_istft_f32")


class _Istft(torch.autograd.Function):
    """``istft`` on an input that requires grad: the forward is the launch ``istft`` makes for any other input (the same
    values), the backward the adjoint kernel eab_istft_bwd_f32 on the same window and, where given, the same lengths.  With
    ``decompress`` the node keeps the fp32 spectrum and its backward is eab_istft_lin_bwd_f32 at that spectrum."""

    @staticmethod
    def forward(ctx, esti: torch.Tensor, window: torch.Tensor, lengths, fft_num: int, hop: int, decompress: bool) -> torch.Tensor:
        lib = _lib.load()
        B, _, T, _ = esti.shape
        x = esti.detach().to(torch.float32).contiguous()
        wav = torch.empty((B, hop * (T - 1)), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            tw = _twiddle(fft_num, x.device)
            lens = None if lengths is None else _device_lengths(lengths, x.device)
            _istft_launch(lib, x, window, tw, wav, lens, fft_num, hop, decompress)
        ctx.save_for_backward(window, tw, *((x,) if decompress else ()), *(() if lens is None else (lens,)))
        ctx.geom = (B, T, fft_num, hop, esti.dtype, decompress)
        return wav

    @staticmethod
    def backward(ctx, dwav):
        window, tw, *rest = ctx.saved_tensors
        B, T, fft_num, hop, dtype, decompress = ctx.geom
        spec = rest.pop(0) if decompress else None
        lib = _lib.load()
        g = dwav.detach().to(torch.float32).contiguous()
        dspec = torch.empty((B, 2, T, fft_num // 2 + 1), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            lens = rest[0].data_ptr() if rest else None
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if decompress:
                _lib.check(lib.eab_istft_lin_bwd_f32(g.data_ptr(), spec.data_ptr(), window.data_ptr(), tw.data_ptr(), dspec.data_ptr(),
                                                     lens, B, T, fft_num, hop, stream), "eab_istft_lin_bwd_f32")
            else:
                _lib.check(lib.eab_istft_bwd_f32(g.data_ptr(), window.data_ptr(), tw.data_ptr(), dspec.data_ptr(), lens, B, T, fft_num,
                                                 hop, stream), "eab_istft_bwd_f32")
        return dspec.to(dtype), None, None, None, None, None


def istft(esti_stft: torch.Tensor, fft_num: int, win_shift: int, window: torch.Tensor, lengths=None,
          decompress: bool = False) -> torch.Tensor:
    """The reference's back end (enhance.py:59-62, test.py:189-191, train_distributed.py:128-130)
    ``torch.istft(view_as_complex(esti.permute(0,3,2,1)), fft_num, win_shift, win_size, hann)`` in one
    HIP kernel: (B, 2, T, F) -> (B, win_shift*(T-1)).  Like the reference it inverts the estimate as
    it is (compressed domain) unless ``decompress`` is set.

    lengths: optional (B,) frame counts, 2 <= len <= T (a sequence or an integer tensor, host or device): utterance b is
    esti_stft[b, :, :len[b]], later frames are never read.  Its first win_shift*(len[b]-1) samples are those of a call on
    that utterance alone, bit for bit (the envelope counts its own frames only); the samples after them are zeros.  The
    window-overlap condition is checked for the shortest and the longest host length (a device tensor: for T).

    decompress (a bool; default False = the reference, today's launch and bits): True undoes the sqrt compression of
    ``stft_compress`` / ``prepare_data`` inside the same kernel -- every bin X is inverted as X |X| (eab_istft_lin_f32;
    DESIGN.md §4.26) -- so the wave is an estimate of the signal in the clean files, the target the waveform losses and the
    scores compare it with, not of a signal whose spectrum has square-rooted magnitudes.

    Differentiable: with grad enabled and ``esti_stft.requires_grad`` the same launch runs inside an autograd node whose
    backward is the adjoint kernel (eab_istft_bwd_f32; with ``decompress`` eab_istft_lin_bwd_f32 at the
    saved fp32 spectrum), so a loss on the wave -- ``si_sdr_loss`` -- trains the network.  The values are those of the call
    without grad, bit for bit; the gradient has the input's dtype."""
    if not isinstance(decompress, bool):
        raise TypeError(f"decompress must be a bool, got {type(decompress).__name__}")
    if lengths is not None:
        if esti_stft.ndim != 4:
            raise ValueError(f"expected (B,2,T,{fft_num // 2 + 1}), got {tuple(esti_stft.shape)}")
        lengths = check_lengths(lengths, esti_stft.shape[0], esti_stft.shape[2], lo=2, integral=True)
    if not esti_stft.is_cuda:
        raise _lib.EabError("istft needs a CUDA (ROCm) tensor; there is no CPU fallback by design.")
    if esti_stft.ndim != 4 or esti_stft.shape[1] != 2 or esti_stft.shape[3] != fft_num // 2 + 1:
        raise ValueError(f"expected (B,2,T,{fft_num // 2 + 1}), got {tuple(esti_stft.shape)}")
    if window.numel() > fft_num:
        raise RuntimeError(f"window ({window.numel()} samples) must not exceed fft_num ({fft_num}), as in torch.istft")
    if not 0 < win_shift <= window.numel():
        raise RuntimeError(f"istft: expected 0 < win_shift <= win_length, got {win_shift} and {window.numel()} (as torch.istft)")
    given = window
    if window.numel() < fft_num:                  # torch.istft(win_length < n_fft): zero-padded on both sides, centred
        left = (fft_num - window.numel()) // 2
        window = torch.nn.functional.pad(window, (left, fft_num - window.numel() - left))
    if -(-fft_num // win_shift) > 8:
        raise NotImplementedError("the HIP back end implements any hop with at most 8 overlapping frames "
                                  "(ceil(fft_num / win_shift) in 1..8; the reference's 320/160 is 2)")
    lib = _lib.load()
    B, _, T, _ = esti_stft.shape
    for n in ((T,) if lengths is None or isinstance(lengths, torch.Tensor) else sorted({min(lengths), max(lengths)})):
        _check_nola(window, fft_num, win_shift, n, key_window=given)
    if torch.is_grad_enabled() and esti_stft.requires_grad:
        # training on the waveform: the same launch, with the adjoint kernel as its backward
        return _Istft.apply(esti_stft, _device_window(window, esti_stft.device), lengths, fft_num, win_shift, decompress)
    x = esti_stft.detach().to(torch.float32).contiguous()
    window = _device_window(window, x.device)
    wav = torch.empty((B, win_shift * (T - 1)), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        lens = None if lengths is None else _device_lengths(lengths, x.device)
        _istft_launch(lib, x, window, _twiddle(fft_num, x.device), wav, lens, fft_num, win_shift, decompress)
    return wav


def filter_and_sum(w: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Stand-alone K13 (reference EaBNet.py:114-117): (B,T,F,M,2)^2 -> (B,2,T,F)."""
    if not (w.is_cuda and x.is_cuda):
        raise _lib.EabError("filter_and_sum needs CUDA (ROCm) tensors; there is no CPU fallback by design.")
    lib = _lib.load()
    B, T, F, M, _ = x.shape
    w = w.to(torch.float32).contiguous()
    x = x.to(torch.float32).contiguous()
    y = torch.empty((B, 2, T, F), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.eab_filter_sum_f32(w.data_ptr(), x.data_ptr(), y.data_ptr(), B, T, F, M,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "eab_filter_sum_f32")
    return y


def numParams(net: nn.Module) -> int:
    """Reference EaBNet.py:653-659."""
    return sum(int(np.prod(p.size())) for p in net.parameters() if p.requires_grad)


class _ComMagMseLoss(torch.autograd.Function):
    """Loss value and d loss / d esti from one fused HIP pass (csrc/loss.hip); the backward is a scale."""

    @staticmethod
    def forward(ctx, esti: torch.Tensor, label: torch.Tensor, frames: tuple) -> torch.Tensor:
        lib = _lib.load()
        B, _, T, F = esti.shape
        e = esti.detach().to(torch.float32).contiguous()
        lab = label.detach().to(torch.float32).contiguous()
        grad = torch.empty_like(e) if ctx.needs_input_grad[0] else None
        nblocks = 1024
        partial = torch.empty(2 * nblocks, dtype=torch.float32, device=e.device)
        loss = torch.empty((), dtype=torch.float32, device=e.device)
        fr = (C.c_int32 * B)(*[int(n) for n in frames])
        with torch.cuda.device(e.device):
            _lib.check(lib.eab_com_mag_mse_loss_f32(e.data_ptr(), lab.data_ptr(), fr, B, T, F, partial.data_ptr(), nblocks,
                                                    loss.data_ptr(), grad.data_ptr() if grad is not None else None,
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "eab_com_mag_mse_loss_f32")
        ctx.save_for_backward(grad)
        ctx.in_dtype = esti.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (g * grad).to(ctx.in_dtype), None, None


def _loss_on_device(esti: torch.Tensor, label: torch.Tensor, frame_list) -> bool:
    return (esti.is_cuda and label.is_cuda and esti.ndim == 4 and esti.shape == label.shape and esti.shape[1] == 2
            and esti.shape[0] <= 64 and len(frame_list) == esti.shape[0] and not label.requires_grad
            and all(0 <= int(n) <= esti.shape[2] for n in frame_list) and sum(int(n) for n in frame_list) > 0)


def com_mag_mse_loss(esti: torch.Tensor, label: torch.Tensor, frame_list) -> torch.Tensor:
    """Reference EaBNet.py:627-640: 0.5*(masked magnitude MSE + masked complex MSE), esti/label (B,2,T,F).
    CUDA tensors: one fused HIP pass produces the value and the gradient w.r.t. ``esti``
    (eab_com_mag_mse_loss_f32); anything else (CPU tensors, > 64 utterances, a label that needs a gradient)
    is evaluated with the reference's tensor expressions."""
    if _loss_on_device(esti, label, frame_list):
        return _ComMagMseLoss.apply(esti, label, tuple(int(n) for n in frame_list))
    B, _, T, F = esti.shape
    mask = torch.zeros((B, T, F), dtype=esti.dtype, device=esti.device)
    for i, n in enumerate(frame_list):
        mask[i, :n] = 1.0
    com_mask = torch.stack((mask, mask), dim=1)
    mag_e, mag_l = torch.norm(esti, dim=1), torch.norm(label, dim=1)
    loss1 = (((mag_e - mag_l) ** 2.0) * mask).sum() / mask.sum()
    loss2 = (((esti - label) ** 2.0) * com_mask).sum() / com_mask.sum()
    return 0.5 * (loss1 + loss2)


def stagewise_com_mag_mse_loss(esti_list, label: torch.Tensor, frame_list) -> torch.Tensor:
    """Reference GaGNet.py:601-619: the complex + magnitude MSE of every stage, weight 0.1 (1 for the
    last stage).  esti (B,2,F,T) each, label (B,2,F,T)."""
    lab_t = label.permute(0, 1, 3, 2)
    if all(_loss_on_device(e.permute(0, 1, 3, 2), lab_t, frame_list) for e in esti_list):
        # every stage is the same masked loss on (B,2,T,F) views; the stage outputs of eabnet_amd.GaGNet are
        # already laid out that way, so nothing is copied
        total = 0.0
        for i, e in enumerate(esti_list):
            alpha = 1.0 if i == len(esti_list) - 1 else 0.1
            total = total + alpha * com_mag_mse_loss(e.permute(0, 1, 3, 2), lab_t, frame_list)
        return total
    B, _, Fq, T = label.shape
    mask = torch.zeros((B, Fq, T), dtype=label.dtype, device=label.device)
    for i, n in enumerate(frame_list):
        mask[i, :, :n] = 1.0
    com_mask = torch.stack((mask, mask), dim=1)
    loss1 = loss2 = 0.0
    mag_label = torch.norm(label, dim=1)
    for i, e in enumerate(esti_list):
        alpha = 1.0 if i == len(esti_list) - 1 else 0.1
        loss1 = loss1 + alpha * (((e - label) ** 2.0) * com_mask).sum() / com_mask.sum()
        loss2 = loss2 + alpha * (((torch.norm(e, dim=1) - mag_label) ** 2.0) * mask).sum() / mask.sum()
    return 0.5 * (loss1 + loss2)


def eabnet_with_postnet_loss(output: dict, label: torch.Tensor, frame_list) -> dict:
    """Reference EaBNet.py:642-650 (called at train_distributed.py:225): the beam-former's loss on
    ``esti0_stft`` plus the stage-wise loss of the post-filter estimates; label (B,2,T,F)."""
    loss0 = com_mag_mse_loss(output["esti0_stft"], label, frame_list)
    loss1 = stagewise_com_mag_mse_loss(output["esti1_stft_list"], label.permute(0, 1, 3, 2), frame_list)
    return {"eabnet": loss0, "postnet": loss1, "final": loss0 + loss1}
