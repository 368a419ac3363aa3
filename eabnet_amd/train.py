"""Training on the hand-written kernels (BASELINE config 4): EaBNet.forward and its backward pass
(what autograd executes for train_distributed.py:221-228 on the reference) lowered to TWO static op lists that
libeabnet_hip.so replays -- forward (keeping what the backward needs) and backward -- behind one
``torch.autograd.Function``.  PyTorch sees a single node: parameters in, (B,2,T,F) out; gradients of all
parameters come back as views of one flat buffer.

Differences to the inference lowering (program.py): every normalised activation is materialised (the
convolutions read plain sources, so the same tensors are the operands of the weight gradients); gated
convolutions also dump their two GLU factors; InstanceNorm finalisation keeps (mean, rstd); the LSTM layers keep
their activated gates and cell states; the MLP and the filter-and-sum are separate ops.

Backward contractions:
  * dgrad = eab_conv_f32 on the output gradient with re-packed weights: the dgrad of a strided convolution
    (GateConv2d / Conv2dunit, EaBNet.py:402,450) is the gather form of a transposed convolution, one launch per
    input-column parity; the dgrad of a transposed convolution (EaBNet.py:423,478) is a strided convolution;
  * wgrad = eab_wgrad_f32 (csrc/wgrad.hip) with the forward's own gather geometry;
  * LSTM: eab_lstm64_bwd_f32 (reverse time) -> dgates, then dx / dW_ih / dW_hh / db as a 1x1 dgrad, two wgrads
    (taps dt = 0 and dt = -1) and a column sum.
Parameters reach the kernels through ONE gather launch (flat parameter vector -> every packed operand, forward
and dgrad layouts; index tables built here from the same packing rules as program.py) and the packed gradient
arena goes back to the flat gradient through the inverse table.

Scope: every constructor branch of the reference (`supported`): U2 / plain U-Net, LSTM / cnn head, mimo / miso, cat / add,
causal or not, InstanceNorm, BatchNorm (train mode) and cLN, up to 32 microphones.  This is the package's only differentiable
path; what it does not cover (eval-mode BatchNorm under autograd) is refused by model.py.

input_grad: the same programs plus the gradient with respect to the input -- the data gradient of the one
convolution that reads it, padded to a 64-column tile, and ONE op (eab_input_grad_f32) that adds the filter-and-sum's adjoint
with respect to X and writes the boundary buffer `din` (B, T, F, M, 2).  Every op of the programs without the switch keeps its
place, name and operands; the added ops and their arena regions come last.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import os

import numpy as np
import torch

from . import _lib
from . import program as prg
from .runtime import BoundProgram
from .program import ALIGN, EPS_IN, EPS_LN, Geometry, Ref, Stats, conv_tiles, pack_taps, unit_rows
from .program import (NB_SUM_COPIES, NB_SUMS_ZEROED, OP_ADD, OP_CLN_BWD, OP_COLSUM, OP_FILTER_SUM, OP_FS_BWD, OP_GATE_BWD,  # noqa: F401
                      OP_GATE_FWD, OP_GATHER, OP_GLU_BWD, OP_IN_STATS, OP_INPUT_GRAD, OP_LN_BWD, OP_LN_FWD, OP_LSTM_BWD, OP_LSTM_TRAIN,
                      OP_NORM_BWD, OP_RELU_BWD, OP_TR_NORM_ACT, OP_WGRAD, STORE_BF16, XF_NORM_PRELU, XF_PRELU_NORM)
from .spec import NetConfig, gate_key, param_specs

MLP_LD = 64          # the second Linear of w_dnn is run with its 2M rows padded to one 64-column tile
TRAIN_BOUND_CACHE = 3   # bound training programs kept per module (LRU over (B, T or cap, F, device, precision, varlen[, bucket]))


def supported(cfg: NetConfig) -> bool:
    return (cfg.bf_type in ("lstm", "cnn") and cfg.topo_type in ("mimo", "miso") and cfg.intra_connect in ("cat", "add")
            and cfg.norm_type in ("IN", "BN", "cLN") and 2 * cfg.M <= MLP_LD)


def unsupported_reason(cfg: NetConfig) -> str:
    """which constructor switch keeps a configuration off the HIP training programs ('' when supported)"""
    why = []
    if cfg.bf_type not in ("lstm", "cnn"):
        why.append(f"bf_type={cfg.bf_type!r}")
    if cfg.topo_type not in ("mimo", "miso"):
        why.append(f"topo_type={cfg.topo_type!r}")
    if cfg.intra_connect not in ("cat", "add"):
        why.append(f"intra_connect={cfg.intra_connect!r}")
    if cfg.norm_type not in ("IN", "BN", "cLN"):
        why.append(f"norm_type={cfg.norm_type!r}")
    if 2 * cfg.M > MLP_LD:
        why.append(f"M={cfg.M} > {MLP_LD // 2}")
    return ", ".join(why)


@dataclass
class GenOp:
    """A non-convolution op of the training programs: kind + the i / f / p fields of eab_op."""
    kind: int
    p: List[Optional[Ref]]
    i: List[int] = field(default_factory=list)
    f: List[float] = field(default_factory=list)
    name: str = ""


@dataclass
class WgradOp:
    dz: Ref
    src0: Ref
    src1: Optional[Ref]
    dw: Ref
    N: int
    C0: int
    C1: int
    Kpad: int
    B: int
    T: int
    Fin: int
    Fz: int
    No: int
    ostride: int
    ophase: int
    istride: int
    dt: List[int]
    ioff: List[int]
    name: str = ""
    kind: int = OP_WGRAD
    dbias: Optional[Ref] = None          # bias gradient (column sums of dz over this launch's rows) rides along
    precision: int = 0                   # EAB_PREC_F32, or EAB_PREC_BF16 (operands rounded to bf16, fp32 accumulation)
    bf16_mask: int = 0                   # bit 0 / 1 / 2: dz / src0 / src1 is stored as bf16 (eab_wgrad_desc.bf16_mask)


class Slot:
    """Gradient accumulator of one tensor (shared by all views of it)."""

    def __init__(self):
        self.ref: Optional[Ref] = None
        self.owned = False


@dataclass
class TVar:
    """A materialised channels-last activation [B][T][F][C] of the training forward."""
    ref: Ref
    F: int
    C: int
    slot: Slot = field(default_factory=Slot)
    needs_grad: bool = True

    def view(self, F: int, C: int) -> "TVar":
        assert F * C == self.F * self.C
        return TVar(self.ref, F, C, self.slot, self.needs_grad)


def _split64(n: int) -> Tuple[int, int]:
    return n & 0xFFFFFFFF, n >> 32


class _LaneList(list):
    """op list that tags every appended op with the lane (stream) the lowering is currently emitting for"""

    def __init__(self, owner):
        super().__init__()
        self.owner = owner

    def append(self, op) -> None:
        op.lane = self.owner.cur_lane
        super().append(op)


class _Tape(list):
    """backward closures; each one is replayed on the lane that was current when it was recorded"""

    def __init__(self, owner):
        super().__init__()
        self.owner = owner

    def append(self, fn) -> None:
        owner, lane = self.owner, self.owner.cur_lane

        def run():
            prev, owner.cur_lane = owner.cur_lane, lane
            fn()
            owner.cur_lane = prev
        super().append(run)


class TrainLowering:
    spec_fn = staticmethod(param_specs)              # parameter inventory of the network being lowered (subclasses: GaGNet)
    supports = staticmethod(supported)

    def __init__(self, cfg, B: int, T: int, F: int = 161, precision: str = "f32", input_grad: bool = False):
        self.input_grad = bool(input_grad)
        if precision not in ("f32", "bf16"):
            raise ValueError("training precision is 'f32' or 'bf16' (bf16: forward, dgrad and wgrad contractions on the bf16 "
                             "matrix cores with fp32 accumulation -- the LSTM's recurrent products included; cell state, norms, "
                             "gradients and the optimiser state stay fp32)")
        self.prec = prg.PREC_CODE[precision]
        # bf16 programs: the LSTM's recurrent products on the bf16 matrix cores too (what torch.autocast does for nn.LSTM);
        # EAB_BF16_LSTM=0 keeps the fp32 recurrence of rounds 2-3
        self.lstm_prec = prg.PREC_BF16 if (self.prec == prg.PREC_BF16 and os.environ.get("EAB_BF16_LSTM", "1") != "0") else prg.PREC_F32
        # small-tile kernel (csrc/conv_st.hip) for the 1-D convolutions of the S-TCMs and their dgrads
        self.st = os.environ.get("EAB_ST", "1") != "0"
        if not self.supports(cfg):
            raise NotImplementedError("the HIP training path does not cover this configuration: " + (unsupported_reason(cfg) if self.supports is supported else "post-filter topology"))
        cfg.check_supported()
        self.cfg, self.B, self.T, self.F = cfg, B, T, F
        # (the BatchNorm buffers are not parameters of the programs: train mode normalises with batch statistics)
        self.specs = {k: s for k, s in self.spec_fn(cfg).items() if s.kind not in ("bn_count", "bn_mean", "bn_var")}
        # BatchNorm in train mode (NormSwitch BN branch, EaBNet.py:677-681; nn.BatchNorm{1,2}d): statistics per channel over
        # the whole batch.  Every tensor is [B][positions][C], channels-last and contiguous, so the batch is ONE virtual
        # utterance of B * positions rows: the InstanceNorm kernels (statistics merge, apply, both backward launches) run
        # unchanged with (B, P) -> (1, B * P).  bn_layers: (norm key, offset of its (mean, rstd) table, C, samples per channel)
        # cLN (the cumulative LayerNorm NormSwitch means to build, EaBNet.py:696-769): its own statistics / apply / backward ops
        self.cln = getattr(cfg, "norm_type", "IN") == "cLN"
        self.bn = getattr(cfg, "norm_type", "IN") == "BN"
        self.nB, self.nP = (1, B * T) if self.bn else (B, T)
        self.bn_layers: List[Tuple[str, int, int, int]] = []
        self.poff: Dict[str, int] = {}
        n = 0
        for k, s in self.specs.items():
            self.poff[k] = n
            n += int(np.prod(s.shape)) if s.shape else 1
        self.n_params = n
        self.a_size = 0
        self.allocs: List[Tuple[int, int]] = []                               # (offset, floats) of every activation-arena region
        # bf16 STORAGE of the tensors only bf16 contractions read (assign_bf16_storage); EAB_BF16_STORE=0: everything fp32
        self.bf16_store = os.environ.get("EAB_BF16_STORE", "1") != "0"
        self.bf16_tensors = 0
        self.w_imgs: List[Tuple[np.ndarray, Optional[np.ndarray]]] = []      # packed-parameter images (flat indices, -1 = 0)
        self.w_size = 0
        self.w_index: Dict[str, Ref] = {}
        self.g_imgs: List[Tuple[int, List[np.ndarray]]] = []                 # (offset, param-index images) of gradient entries
        self.g_size = 0
        self.cur_lane = 0                                                     # 0 = the caller's stream; > 0: parallel branches
        self.fwd: list = _LaneList(self)
        self.bwd: list = _LaneList(self)
        self.sync = {"fwd": {}, "bwd": {}}                                    # op index -> [("fork" | "join", lanes)]
        self.tape: List[Callable[[], None]] = _Tape(self)
        self.deferred: List[WgradOp] = []                                     # weight gradients, appended to bwd by finish()
        self.flops_fwd = 0
        self.flops_bwd = 0
        self.emit = self.fwd                                                  # the list ops are appended to
        self.gtaps: Dict[str, TVar] = {}                                      # named activations whose gradient tests read back
        self.din_tile: Optional[TVar] = None                                  # input_grad: the input's gradient through its convolution
        self.bf_w: Optional[TVar] = None                                      # the beam-forming weight rows of the forward

    def mark(self, which: str, what: str, lanes: Sequence[int]) -> None:
        """fork / join of parallel branches in front of the next op of the forward or backward list (executed by TrainBound.run
        with side streams and events; inside a hipGraph capture they become parallel branches)"""
        lst = self.fwd if which == "fwd" else self.bwd
        self.sync[which].setdefault(len(lst), []).append((what, list(lanes)))

    # ---- arenas ------------------------------------------------------------------------------------
    def alloc(self, nfloats: int) -> Ref:
        ref = Ref("a", self.a_size)
        self.allocs.append((self.a_size, nfloats))
        self.a_size += nfloats + ((-nfloats) % ALIGN)
        return ref

    def act(self, F: int, C: int, needs_grad: bool = True) -> TVar:
        return TVar(self.alloc(self.B * self.T * F * C), F, C, Slot(), needs_grad)

    def idx(self, key: str) -> np.ndarray:
        s = self.specs[key]
        return (self.poff[key] + np.arange(int(np.prod(s.shape)), dtype=np.int64)).reshape(s.shape)

    def wadd(self, name: str, img: np.ndarray, img2: Optional[np.ndarray] = None) -> Ref:
        """packed parameter operand: value[i] = flat[img[i]] (+ flat[img2[i]]), -1 = 0"""
        if name in self.w_index:
            return self.w_index[name]
        flat = np.ascontiguousarray(img, dtype=np.int64).reshape(-1)
        pad = (-flat.size) % ALIGN
        ref = Ref("w", self.w_size)
        f2 = None if img2 is None else np.ascontiguousarray(img2, dtype=np.int64).reshape(-1)
        self.w_imgs.append((np.concatenate([flat, np.full(pad, -1, np.int64)]),
                            None if f2 is None else np.concatenate([f2, np.full(pad, -1, np.int64)])))
        self.w_size += flat.size + pad
        self.w_index[name] = ref
        return ref

    def gadd(self, imgs: Sequence[np.ndarray]) -> Ref:
        """gradient entry shaped like imgs[0]; element i is the gradient of flat[img[i]] for every image (-1: discarded)"""
        flats = [np.ascontiguousarray(m, dtype=np.int64).reshape(-1) for m in imgs]
        n = flats[0].size
        assert all(f.size == n for f in flats)
        ref = Ref("g", self.g_size)
        self.g_imgs.append((self.g_size, flats))
        self.g_size += n + ((-n) % ALIGN)
        return ref

    def vec(self, key: str) -> Ref:
        return self.wadd(key, self.idx(key))

    def gvec(self, key: str) -> Ref:
        return self.gadd([self.idx(key)])

    # ---- gradient bookkeeping ------------------------------------------------------------------------
    def contribute(self, var: TVar, ref: Ref) -> None:
        """grad(var) += tensor at `ref` (same shape), emitted into the backward list"""
        if not var.needs_grad:
            return
        s = var.slot
        n = self.B * self.T * var.F * var.C
        if s.ref is None:
            s.ref, s.owned = ref, False                          # alias: nobody may write into it
            return
        dst = s.ref if s.owned else self.alloc(n)
        self.bwd.append(GenOp(OP_ADD, [s.ref, ref, dst], list(_split64(n)), name="grad+="))
        s.ref, s.owned = dst, True

    def grad_target(self, var: TVar) -> Tuple[Ref, Optional[Ref]]:
        """(dst, aux) for a kernel that can compute dst = contribution + aux (aux None: plain store)"""
        s = var.slot
        n = self.B * self.T * var.F * var.C
        if s.ref is None:
            s.ref, s.owned = self.alloc(n), True
            return s.ref, None
        if s.owned:
            return s.ref, s.ref
        old = s.ref
        s.ref, s.owned = self.alloc(n), True
        return s.ref, old

    def grad_of(self, var: TVar) -> Ref:
        assert var.slot.ref is not None, "backward reached a tensor nobody differentiated"
        return var.slot.ref

    # ---- convolution machinery --------------------------------------------------------------------------
    def pick_bm(self, No: int) -> int:
        return 128 if self.B * conv_tiles(self.T, No, 128) >= 2 * prg.CUS else 64

    def conv_op(self, name, srcs: Sequence[TVar], w: Ref, bias: Optional[Ref], geom: Geometry, *, N: int, epi: int, dst: Ref,
                stats: Optional[Stats] = None, bm=None, aux=None, dst_acc=None, glu_dump=None, st: bool = False) -> prg.ConvOp:
        """st: `w` is in MFMA-fragment order and the launch goes to the small-tile kernel (csrc/conv_st.hip, KORDER_FRAG)"""
        s0, s1 = srcs[0], (srcs[1] if len(srcs) > 1 else None)
        op = prg.conv_launch(name, self.B, self.T, srcs, w, bias, geom, N=N, epi=epi, dst=dst, bm=bm or self.pick_bm(geom.No),
                             stats=stats, aux=aux, dst_acc=dst_acc, glu_dump=glu_dump)
        if st:
            op.korder = prg.KORDER_FRAG
        if self.prec != prg.PREC_F32 and s0.ref.arena != "in" and s0.C % 4 == 0 and (s1 is None or s1.C % 4 == 0):
            op.precision = self.prec                  # the convolution on the raw network input stays exact
        self.emit.append(op)
        fl = 2 * self.B * self.T * geom.No * N * geom.ntaps * (op.C0 + op.C1)
        if self.emit is self.fwd:
            self.flops_fwd += fl
        else:
            self.flops_bwd += fl
        return op

    def wgrad_op(self, name, dz: Ref, srcs: Sequence[TVar], geom: Geometry, gimg, *, N: int, dbias: Optional[Ref] = None) -> None:
        """dW of the launch that read `srcs` with `geom` and N output channels, dz = gradient of its output; gimg: the
        parameter-index image of its packed weights"""
        s0, s1 = srcs[0], (srcs[1] if len(srcs) > 1 else None)
        Ctot = s0.C + (s1.C if s1 else 0)
        Kpad = geom.kpad(Ctot)
        assert tuple(gimg.shape) == (N, Kpad), (gimg.shape, N, Kpad)
        # Weight gradients are leaves of the backward graph (nothing reads dW before the step ends; their operands -- the
        # finished gradient of a convolution output and a forward activation -- are never written again, no buffer is
        # recycled), so they are all emitted at the END of the backward program, sorted by geometry: eab_run_program
        # then serves every run of identical geometry (the 18 S-TCMs, the repeated U-Net levels) with one launch.
        self.deferred.append(WgradOp(dz=dz, src0=s0.ref, src1=s1.ref if s1 else None, dw=self.gadd([gimg]), N=N, C0=s0.C,
                                     C1=s1.C if s1 else 0, Kpad=Kpad, B=self.B, T=self.T, Fin=s0.F, Fz=geom.Fout, No=geom.No,
                                     ostride=geom.ostride, ophase=geom.ophase, istride=geom.istride, dt=list(geom.dt),
                                     ioff=list(geom.ioff), name=name, dbias=dbias,
                                     precision=self.prec if self.prec == prg.PREC_BF16 else prg.PREC_F32))
        self.flops_bwd += 2 * self.B * self.T * geom.No * N * geom.ntaps * Ctot

    def colsum(self, name, x: Ref, rows: int, N: int, imgs: Sequence[np.ndarray]) -> None:
        self.bwd.append(GenOp(OP_COLSUM, [x, self.gadd(imgs)], list(_split64(rows)) + [N], name=name))

    def dgrad(self, name: str, var: TVar, dz: Ref, launches: Sequence[Tuple[Ref, Geometry]], *, N: int, st_bm: int = 0) -> None:
        """grad(var) (+)= conv(dz; w) with the forward kernel on the gradient tensor dz [B][T][Fin][N] of each geometry
        (Geometry.adjoint of the forward launch); `launches` = (weights, geometry) per launch -- the launches of one call
        write disjoint output columns and share the accumulate operand."""
        if not var.needs_grad or not launches:
            return
        dst, aux = self.grad_target(var)
        self.emit = self.bwd
        for k, (w, geom) in enumerate(launches):
            assert geom.Fout == var.F
            self.conv_op(f"{name}.{k}", [TVar(dz, geom.Fin, N)], w, None, geom, N=var.C,
                         epi=prg.EPI_ADD if aux is not None else prg.EPI_LINEAR, dst=dst, aux=aux, st=st_bm > 0, bm=st_bm or None)
        self.emit = self.fwd

    # ---- norm + activation ---------------------------------------------------------------------------------
    def norm_act(self, name: str, raw: TVar, norm: str, act: str, mode: int, xf: Ref, mr: Ref, add: Optional[TVar] = None) -> TVar:
        """a = f(raw) [+ add]; records the backward (norm/PReLU gradients, dparams)"""
        out = self.act(raw.F, raw.C)
        P = self.nP * raw.F
        slp = self.vec(f"{act}.weight")
        # norm None: PReLU only (xf / mr NULL -- the kernels' no-norm form; the plain U-Net's middle encoder layers)
        gam, bet = (self.vec(f"{norm}.norm.weight"), self.vec(f"{norm}.norm.bias")) if norm else (None, None)
        self.fwd.append(GenOp(OP_TR_NORM_ACT, [raw.ref, xf, slp, add.ref if add else None, out.ref], [self.nB, P, raw.C, mode],
                              name=name))

        self.tape.append(self._norm_back(name, raw, out, add, norm, act, mode, mr, gam, bet, slp, P))
        return out

    def _norm_back(self, name, raw: TVar, out: TVar, add: Optional[TVar], norm: str, act: str, mode: int, mr: Ref, gam: Ref,
                   bet: Ref, slp: Ref, P: int) -> Callable[[], None]:
        def back():
            d = self.grad_of(out)
            if add is not None:
                self.contribute(add, d)
            dst, aux = self.grad_target(raw)
            # reduction scratch in the gradient arena: that arena is zero-filled once before every backward run, so the
            # kernel needs no zero-fill launch of its own (EAB_NB_SUMS_ZEROED)
            sums = Ref("g", self.g_size)
            self.g_size += NB_SUM_COPIES * self.nB * raw.C * 4 + ((-NB_SUM_COPIES * self.nB * raw.C * 4) % ALIGN)
            self.bwd.append(GenOp(OP_NORM_BWD, [d, raw.ref, mr, gam, bet, slp, sums, aux, dst,
                                                self.gvec(f"{norm}.norm.weight") if norm else None,
                                                self.gvec(f"{norm}.norm.bias") if norm else None, self.gvec(f"{act}.weight")],
                                  [self.nB, P, raw.C, mode | NB_SUMS_ZEROED], name=name + ".bwd"))
        return back

    def finalize(self, name: str, stats: Ref, C: int, tiles: int, count: int, norm: str) -> Tuple[Ref, Ref]:
        xf, mr = self.alloc(self.nB * C * 2), self.alloc(self.nB * C * 2)
        # BatchNorm in train mode: the partials are [b][tile][C][4] back to back, so the batch statistics are the same
        # merge over B * tiles partials of ONE virtual utterance (see __init__)
        bt = self.B // self.nB
        op = prg.FinalizeOp(stats=stats, B=self.nB, C=C, nsets=1, stat_tiles=tiles * bt, count=count * bt, eps=EPS_IN,
                            gamma0=self.vec(f"{norm}.norm.weight"), beta0=self.vec(f"{norm}.norm.bias"), xf0=xf, name=name)
        op.mr0 = mr
        self.fwd.append(op)
        self.note_bn(norm, mr, 0, C, count * bt)
        return xf, mr

    def cln_unit(self, name: str, raw: TVar, norm: str, act: str, mode: int, add: Optional[TVar] = None) -> TVar:
        """cumulative LayerNorm + PReLU (either order) [+ add] as statistics + apply ops (eab_cln_stats_f32 / eab_cln_apply_f32,
        whole utterance) and ONE backward op (eab_train_cln_bwd_f32: row sums, reverse scan over t, apply) followed by the
        column sum of its per-row parameter-gradient partials"""
        B, T, C = self.B, self.T, raw.C
        P = raw.F * C
        out = self.act(raw.F, C)
        sums, mr = self.alloc(B * T * 4), self.alloc(B * T * 2)              # [B][T][2] doubles | (cum_mean, rstd)
        gimg, bimg, simg = self.idx(f"{norm}.norm.gain").reshape(C), self.idx(f"{norm}.norm.bias").reshape(C), self.idx(f"{act}.weight")
        gain, bias, slp = self.wadd(f"{norm}.norm.gain", gimg), self.wadd(f"{norm}.norm.bias", bimg), self.vec(f"{act}.weight")
        self.fwd.append(prg.ClnStatsOp(x=raw.ref, slope=slp if mode == XF_PRELU_NORM else None, sums=sums, state=None, mr=mr,
                                       B=B, T=T, P=P, C=C, eps=EPS_IN, name=name + ".cln_stats"))
        self.fwd.append(prg.ClnApplyOp(x=raw.ref, mr=mr, gain=gain, bias=bias, slope=slp, add=add.ref if add else None, out=out.ref,
                                       B=B, T=T, P=P, C=C, mode=mode, name=name + ".cln"))

        def back():
            d = self.grad_of(out)
            if add is not None:
                self.contribute(add, d)
            dst, aux = self.grad_target(raw)
            rs, ab, part = self.alloc(B * T * 4), self.alloc(B * T * 2), self.alloc(B * T * 3 * C)
            self.bwd.append(GenOp(OP_CLN_BWD, [d, raw.ref, mr, gain, bias, slp, rs, ab, part, aux, dst], [B, T, P, C, mode],
                                  name=name + ".cln_bwd"))
            self.colsum(name + ".cln_dparams", part, B * T, 3 * C, [np.concatenate([gimg, bimg, simg.reshape(C)])])
        self.tape.append(back)
        return out

    def note_bn(self, norm: str, mr: Ref, c0: int, C: int, n: int) -> None:
        """BatchNorm: where this layer's batch (mean, rstd) table lies, for the update of its running buffers"""
        if self.bn:
            self.bn_layers.append((norm, mr.off + 2 * c0, C, n))

    # ---- 2-D units -----------------------------------------------------------------------------------------
    def conv2d(self, name, srcs: Sequence[TVar], wkey: str, glu: bool, norm: str, act: str, in_perm: Optional[np.ndarray] = None,
               add: Optional[TVar] = None, *, transposed: bool) -> TVar:
        """A 2-D unit (+GLU) + InstanceNorm + PReLU.  conv2d_fwd: strided causal Conv2d, the launch of Geometry.strided
        (GateConv2d EaBNet.py:434-460 / Conv2dunit :391-407); conv2d_transposed: ConvTranspose2d + chomp, the phase pair of
        Geometry.transposed (EaBNet.py:463-490, 410-431).  The launches write one raw output; the backward is one weight
        gradient per launch and, per source, the launches of Geometry.adjoint."""
        wkey = gate_key({f"{k}": 1 for k in self.specs}, wkey)
        wi = self.idx(f"{wkey}.weight")                                      # flat indices, as (N, Cin, kt, kf)
        if transposed:
            wi = wi.transpose(1, 0, 2, 3)
        N, Cin, kt, kf = wi.shape
        assert Cin == sum(s.C for s in srcs)
        if in_perm is not None:
            wi = wi[:, in_perm]
        geoms = Geometry.transposed(srcs[0].F, kt, kf) if transposed else (Geometry.strided(srcs[0].F, kt, kf),)
        tags = [str(g.ophase) for g in geoms] if transposed else [""]           # names: .ph0 / .ph1, .wgrad0 / .wgrad1
        Fout = geoms[0].Fout
        order, Cout = unit_rows(N, glu)
        wn = np.ascontiguousarray(wi).reshape(N, Cin, kt * kf)[order]
        wimgs = [pack_taps(wn, g.taps) for g in geoms]
        bimg = self.idx(f"{wkey}.bias")[order]
        if transposed:                                                       # (arena order: the bias, then the phases' weights)
            self.wadd(f"{wkey}.b", bimg)
        raw = self.act(Fout, Cout)
        bm = self.pick_bm(geoms[0].No)
        tiles = [conv_tiles(self.T, g.No, bm) for g in geoms]
        stats = self.alloc(self.B * sum(tiles) * Cout * 4) if (norm and not self.cln) else None
        dump = self.alloc(self.B * self.T * Fout * N) if glu else None
        for g, tag, wimg in zip(geoms, tags, wimgs):
            ph = f".ph{tag}" if tag else ""
            self.conv_op(name + ph, srcs, self.wadd(f"{wkey}.w{ph}", wimg), self.wadd(f"{wkey}.b", bimg), g, N=N,
                         epi=prg.EPI_GLU if glu else prg.EPI_LINEAR, dst=raw.ref, bm=bm, glu_dump=dump,
                         stats=Stats(stats, sum(tiles), tile0=g.ophase * tiles[0]))
        xf, mr = self.finalize(name + ".in", stats, Cout, sum(tiles), self.T * Fout, norm) if stats is not None else (None, None)
        rows = self.B * self.T * Fout

        def back():
            dr = self.grad_of(raw)
            if glu:
                dz = self.alloc(rows * N)
                self.bwd.append(GenOp(OP_GLU_BWD, [dr, dump, dz], list(_split64(rows)) + [N], name=name + ".glu_bwd"))
            else:
                dz = dr
            gb = self.gadd([bimg])               # every launch adds its rows' column sums
            for g, tag, wimg in zip(geoms, tags, wimgs):
                self.wgrad_op(f"{name}.wgrad{tag}", dz, srcs, g, wimg, N=N, dbias=gb)
            c_lo = 0
            for s in srcs:
                wd = np.ascontiguousarray(wn[:, c_lo:c_lo + s.C].transpose(1, 0, 2))      # (C_s, N packed, kt * kf)
                self.dgrad(f"{name}.dgrad", s, dz, [(self.wadd(f"{wkey}.wd.{c_lo}" + ("" if transposed else f".{g.ophase}"),
                                                               pack_taps(wd, g.taps)), g) for g in Geometry.adjoint(geoms)], N=N)
                if s.ref.arena == "in" and self.input_grad:
                    # the gradient of the network input: the same launches with the transposed weights padded to
                    # one 64-column tile (index -1 = a zero weight in the pad rows, as w2 of the head), into a [rows][64] scratch
                    # in memory-channel order m*2+ri that eab_input_grad_f32 gathers
                    assert not transposed and len(srcs) == 1 and self.din_tile is None and s.C <= MLP_LD
                    wd64 = np.full((MLP_LD,) + wd.shape[1:], -1, np.int64)
                    wd64[:s.C] = wd
                    self.din_tile = TVar(s.ref, s.F, MLP_LD, Slot())
                    self.dgrad(f"{name}.dgrad_in", self.din_tile, dz,
                               [(self.wadd(f"{wkey}.wd64.{g.ophase}", pack_taps(wd64, g.taps)), g) for g in Geometry.adjoint(geoms)], N=N)
                c_lo += s.C
        self.tape.append(back)          # before the norm/PReLU closure on the tape = after it in the backward
        if self.cln and norm:
            return self.cln_unit(name + ".act", raw, norm, act, XF_NORM_PRELU, add)
        return self.norm_act(name + ".act", raw, norm, act, XF_NORM_PRELU, xf, mr, add)

    conv2d_fwd = functools.partialmethod(conv2d, transposed=False)
    conv2d_transposed = functools.partialmethod(conv2d, transposed=True)

    def unet_module(self, pre: str, srcs: Sequence[TVar], scale: int, transposed: bool, in_perm=None) -> TVar:
        """En_unet_module.forward (EaBNet.py:372-388): the residual add is fused into the last norm+PReLU."""
        if transposed:
            g = self.conv2d_transposed(f"{pre}.in_conv", srcs, f"{pre}.in_conv.0.conv.0", True, f"{pre}.in_conv.1", f"{pre}.in_conv.2")
        else:
            g = self.conv2d_fwd(f"{pre}.in_conv", srcs, f"{pre}.in_conv.0.conv.1", True, f"{pre}.in_conv.1", f"{pre}.in_conv.2", in_perm)
        y, downs = g, []
        for j in range(scale):
            q = f"{pre}.enco.{j}.conv"
            y = self.conv2d_fwd(q, [y], f"{q}.0", False, f"{q}.1", f"{q}.2")
            downs.append(y)
        for j in range(scale):
            q = f"{pre}.deco.{j}.deconv"
            if j == 0:
                ins = [y]
            elif self.cfg.intra_connect == "add":
                ins = [self.add_vars(f"{q}.skip_add", y, downs[-(j + 1)])]       # Skip_connect 'add' (EaBNet.py:499-500)
            else:
                ins = [y, downs[-(j + 1)]]
            y = self.conv2d_transposed(q, ins, f"{q}.0", False, f"{q}.1", f"{q}.2", add=g if j == scale - 1 else None)
        return y

    def add_vars(self, name: str, a: TVar, b: TVar) -> TVar:
        """s = a + b, materialised (the training programs materialise every operand of a backward op anyway); the gradient
        of s flows to both summands unchanged"""
        assert a.F == b.F and a.C == b.C
        out = self.act(a.F, a.C)
        n = self.B * self.T * a.F * a.C
        self.fwd.append(GenOp(OP_ADD, [a.ref, b.ref, out.ref], list(_split64(n)), name=name))

        def back():
            d = self.grad_of(out)
            self.contribute(a, d)
            self.contribute(b, d)
        self.tape.append(back)
        return out

    # ---- 1-D units (S-TCM, Linear) -------------------------------------------------------------------------
    def conv1d(self, name: str, src: TVar, wimg_nck: np.ndarray, bimg: Optional[np.ndarray], geom: Geometry, *, epi: int,
               aux: Optional[TVar] = None, dst_acc: Optional[Ref] = None, wname: str = "") -> Tuple[TVar, Callable[[Ref], None]]:
        """out[t] = sum_j W[:, :, j] src[t + geom.dt[j]] (+ bias) with epilogue LINEAR / RELU / ADD(aux).  Returns the output
        and a function that, given the gradient w.r.t. the pre-epilogue sum, emits wgrad / dbias / dgrad."""
        N, Cc, _ = wimg_nck.shape
        wimg = pack_taps(wimg_nck, geom.taps)
        out = self.act(1, N)

        def st_geometry(n, c, kp, epi_=prg.EPI_LINEAR):
            """rows per tile of a small-tile launch (csrc/conv_st.hip), 0 = conv_gemm_kernel"""
            if not (self.st and self.prec in (prg.PREC_F32, prg.PREC_BF16) and n in (64, 128, 256) and c in (64, 128, 256)
                    and kp <= {64: 320, 128: 320, 256: 64}[n] and epi_ in (prg.EPI_LINEAR, prg.EPI_RELU, prg.EPI_ADD)):
                return 0
            return 32 if self.B * ((self.T + 31) // 32) >= 2 * prg.CUS else 16
        st_bm = st_geometry(N, Cc, wimg.shape[1], epi)
        wref = self.wadd(wname + (".wf" if st_bm else ".w"), prg.pack_frag(wimg) if st_bm else wimg)
        bref = self.wadd(wname + ".b", bimg) if bimg is not None else None
        self.conv_op(name, [src], wref, bref, geom, N=N, epi=epi, dst=out.ref, bm=st_bm or 64,
                     aux=aux.ref if aux is not None else None, dst_acc=dst_acc, st=st_bm > 0)

        def back(dz: Ref):
            self.wgrad_op(name + ".wgrad", dz, [src], geom, wimg, N=N, dbias=self.gadd([bimg]) if bimg is not None else None)
            gd, = Geometry.adjoint(geom)
            img = pack_taps(np.ascontiguousarray(wimg_nck.transpose(1, 0, 2)), gd.taps)      # (Cc, N, K)
            d_bm = st_geometry(Cc, N, img.shape[1])
            self.dgrad(name + ".dgrad", src, dz, [(self.wadd(wname + (".wdf" if d_bm else ".wd"), prg.pack_frag(img) if d_bm else img), gd)],
                       N=N, st_bm=d_bm)
        return out, back

    def in1d(self, name: str, raw: TVar, norm: str, act: str) -> TVar:
        """prelu -> InstanceNorm1d (S-TCM order, EaBNet.py:545-547) as ONE launch: statistics, (xf, mr) and the normalised
        tensor (eab_train_in1d_f32); backward = the norm backward of the PRELU_NORM form"""
        if self.cln:
            return self.cln_unit(name, raw, norm, act, XF_PRELU_NORM)
        xf, mr = self.alloc(self.nB * raw.C * 2), self.alloc(self.nB * raw.C * 2)
        out = self.act(raw.F, raw.C)
        P = self.nP * raw.F
        gam, bet, slp = self.vec(f"{norm}.norm.weight"), self.vec(f"{norm}.norm.bias"), self.vec(f"{act}.weight")
        self.fwd.append(GenOp(OP_IN_STATS, [raw.ref, slp, gam, bet, xf, mr, out.ref], [self.nB, P, raw.C], [EPS_IN], name=name))
        self.note_bn(norm, mr, 0, raw.C, P)
        self.tape.append(self._norm_back(name, raw, out, None, norm, act, XF_PRELU_NORM, mr, gam, bet, slp, P))
        return out

    def in1d_multi(self, name: str, raw: TVar, norms: Sequence[str], acts: Sequence[str]) -> List[TVar]:
        """Two units prelu -> InstanceNorm1d on the SAME input (the branch norms of an S-TCM): one forward launch writing two
        contiguous tensors, one two-launch backward that sums both input gradients"""
        assert len(norms) == 2 and len(acts) == 2
        if self.cln:      # two separate units on the same input: their input gradients add up through the gradient slot
            return [self.cln_unit(f"{name}.{v}", raw, norms[v], acts[v], XF_PRELU_NORM) for v in range(2)]
        C = raw.C * 2
        P = self.nP * raw.F
        n = self.nB * P * raw.C
        xf, mr = self.alloc(self.nB * C * 2), self.alloc(self.nB * C * 2)
        for v, k in enumerate(norms):
            self.note_bn(k, mr, v * raw.C, raw.C, P)
        base = self.alloc(2 * n)                                            # view v at base + v * n
        outs = [TVar(Ref("a", base.off + v * n), raw.F, raw.C) for v in range(2)]
        img_g = np.concatenate([self.idx(f"{k}.norm.weight") for k in norms])
        img_b = np.concatenate([self.idx(f"{k}.norm.bias") for k in norms])
        img_s = np.concatenate([self.idx(f"{k}.weight") for k in acts])
        gam, bet, slp = self.wadd(name + ".gamma", img_g), self.wadd(name + ".beta", img_b), self.wadd(name + ".slope", img_s)
        self.fwd.append(GenOp(OP_IN_STATS, [raw.ref, slp, gam, bet, xf, mr, base], [self.nB, P, C, raw.C], [EPS_IN], name=name))

        def back():
            d0, d1 = self.grad_of(outs[0]), self.grad_of(outs[1])
            dst, aux = self.grad_target(raw)
            sums = Ref("g", self.g_size)                                     # zero-filled with the gradient arena
            self.g_size += NB_SUM_COPIES * self.nB * C * 4 + ((-NB_SUM_COPIES * self.nB * C * 4) % ALIGN)
            # (p[4], beta in the one-view form, carries the second view's gradient here: the PRELU_NORM backward never reads beta)
            self.bwd.append(GenOp(OP_NORM_BWD, [d0, raw.ref, mr, gam, d1, slp, sums, aux, dst, self.gadd([img_g]), self.gadd([img_b]),
                                                self.gadd([img_s])], [self.nB, P, C, XF_PRELU_NORM | NB_SUMS_ZEROED, raw.C],
                                  name=name + ".bwd"))
        self.tape.append(back)
        return outs

    def tcm(self, pre: str, x: TVar, dilation: int, x_acc: Optional[Ref], perm: np.ndarray) -> TVar:
        """SqueezedTCM.forward, EaBNet.py:572-578.  The closures go on the tape in forward order (they bind their
        operands late): in_conv | left norm | right norm | branch convs + gate | out norm | out_conv."""
        cfg = self.cfg
        n = self.B * self.T * cfg.cd1
        one, gd = Geometry.pointwise(1), Geometry.temporal(prg.tcm_taps(cfg.kd1, dilation, cfg.is_causal))
        w_in = self.idx(f"{pre}.in_conv.weight")[:, perm, :]                 # (cd, D, 1)
        y, back_in = self.conv1d(f"{pre}.in_conv", x, w_in, None, one, epi=prg.EPI_LINEAR, wname=f"{pre}.in_conv")
        self.tape.append(lambda: back_in(self.grad_of(y)))
        # both branch norms read y: one launch normalises it twice (eab_train_in1d_multi_f32, two contiguous outputs) and one
        # two-launch backward sums the two input gradients into dy
        yL, yR = self.in1d_multi(f"{pre}.lr", y, [f"{pre}.left_conv.1", f"{pre}.right_conv.1"],
                                 [f"{pre}.left_conv.0", f"{pre}.right_conv.0"])
        a, back_l = self.conv1d(f"{pre}.left_conv", yL, self.idx(f"{pre}.left_conv.3.weight"), None, gd, epi=prg.EPI_LINEAR,
                                wname=f"{pre}.left_conv")
        r, back_r = self.conv1d(f"{pre}.right_conv", yR, self.idx(f"{pre}.right_conv.3.weight"), None, gd, epi=prg.EPI_LINEAR,
                                wname=f"{pre}.right_conv")
        z = self.act(1, cfg.cd1)
        self.fwd.append(GenOp(OP_GATE_FWD, [a.ref, r.ref, z.ref], list(_split64(n)), name=f"{pre}.gate"))

        def back_gate():
            da, dr = self.alloc(n), self.alloc(n)
            self.bwd.append(GenOp(OP_GATE_BWD, [self.grad_of(z), a.ref, r.ref, da, dr], list(_split64(n)), name=f"{pre}.gate_bwd"))
            back_l(da)
            back_r(dr)
        self.tape.append(back_gate)
        zo = self.in1d(f"{pre}.out", z, f"{pre}.out_conv.1", f"{pre}.out_conv.0")
        w_out = self.idx(f"{pre}.out_conv.2.weight")[perm]                   # (D, cd, 1), rows permuted
        out, back_out = self.conv1d(f"{pre}.out_conv", zo, w_out, None, one, epi=prg.EPI_ADD, aux=x, dst_acc=x_acc,
                                    wname=f"{pre}.out_conv")

        def back():
            d = self.grad_of(out)
            self.contribute(x, d)                                            # residual
            back_out(d)
        self.tape.append(back)
        return out

    # ---- whole network -----------------------------------------------------------------------------------------
    def build(self) -> "TrainProgram":
        cfg, B, T, F = self.cfg, self.B, self.T, self.F
        M, c = cfg.M, cfg.c
        x_in = TVar(Ref("in"), F, 2 * M, Slot(), needs_grad=False)
        mem = np.arange(2 * M)
        in_perm = (mem % 2) * M + mem // 2                                   # memory channel m*2+ri <- reference ri*M+m
        skips: List[TVar] = []
        x = x_in
        if cfg.is_u2:
            for i in range(4):
                x = self.unet_module(f"en.meta_unet_list.{i}", [x], 4 - i, False, in_perm if i == 0 else None)
                skips.append(x)
                self.gtaps[f"en.{i}"] = x
            x = self.conv2d_fwd("en.last_conv", [x], "en.last_conv.0.conv.1", True, "en.last_conv.1", "en.last_conv.2")
            skips.append(x)
            self.gtaps["en.4"] = x
        else:
            # UNet_Encoder (EaBNet.py:213-239): five gated convolutions; layers 1 and 2 have no norm in front of their PReLU
            from .spec import unet_encoder_layers
            for i, (_, _, _, has_norm) in enumerate(unet_encoder_layers(cfg)):
                q = f"en.unet_list.{i}"
                x = self.conv2d_fwd(q, [x], f"{q}.0.conv.1", True, f"{q}.1" if has_norm else None,
                                    f"{q}.2" if has_norm else f"{q}.1", in_perm if i == 0 else None)
                skips.append(x)
                self.gtaps[f"en.{i}"] = x
        Fb = x.F
        assert Fb * x.C == cfg.d_feat
        k = np.arange(cfg.d_feat)
        perm = (k % c) * Fb + k // c                                         # memory channel f*64+c <- reference c*4+f
        xt = x.view(1, cfg.d_feat)
        x_acc = self.act(1, cfg.d_feat)
        self.fwd.append(prg.MemsetOp(x_acc.ref, B * T * cfg.d_feat, name="stcns.acc0"))
        lasts = []
        for gi in range(cfg.q):
            for i in range(cfg.p):
                xt = self.tcm(f"stcns.{gi}.tcm_list.{i}", xt, 2 ** i, x_acc.ref if i == cfg.p - 1 else None, perm)
            lasts.append(xt)

        def back_acc():                                                      # x_acc = sum of the group outputs (EaBNet.py:101-105)
            d = self.grad_of(x_acc)
            for v in lasts:
                self.contribute(v, d)
        # the group outputs are produced before x_acc is complete, but every consumer of x_acc comes later:
        # running this first in the backward hands d(x_acc) to the three group outputs before their own closures
        self.tape.append(back_acc)
        x = x_acc.view(Fb, c)
        self.gtaps["stcns"] = x
        if cfg.is_u2:
            for i in range(4):
                x = self.unet_module(f"de.meta_unet_list.{i}", [x, skips[-(i + 1)]], i + 1, True)
                self.gtaps[f"de.{i}"] = x
            e = self.conv2d_transposed("de.last_conv", [x, skips[0]], "de.last_conv.0.conv.0", True, "de.last_conv.1",
                                       "de.last_conv.2")
        else:
            for i in range(5):                        # UNet_Decoder (EaBNet.py:297-328)
                q = f"de.unet_list.{i}"
                x = e = self.conv2d_transposed(q, [x, skips[-(i + 1)]], f"{q}.0.conv.0", True, f"{q}.1", f"{q}.2")
                self.gtaps[f"de.{i}"] = x
        assert e.F == F and e.C == 64
        self.gtaps["de.4"] = e

        rows = B * T * F
        pw = Geometry.pointwise(F)           # the heads, the MLP and the LSTM's input / recurrent products: 1x1 on every bin
        if cfg.bf_type == "cnn" or cfg.topo_type == "miso":
            # ---- pointwise head (EaBNet.py:80-81,111-113): Conv2d(64 -> 2M, 1x1); output plane m*2+ri is the column order the
            # filter-and-sum kernels read (rows padded to one 64-column tile).  miso (EaBNet.py:78-79,118-125): Conv2d(64 -> 2),
            # one complex mask on microphone 0 = the same head with zero rows for the other microphones; the caller sums the
            # (B,2,T,F) result over frequency, as the reference does
            wk = self.idx("bf_map.weight").reshape(-1, 64)
            wc = np.full((MLP_LD, 64, 1), -1, np.int64)
            wc[:wk.shape[0]] = wk[:, :, None]
            bcimg = np.full(MLP_LD, -1, np.int64)
            bcimg[:wk.shape[0]] = self.idx("bf_map.bias")
            wcimg = pack_taps(wc, pw.taps)
            bw = self.act(F, MLP_LD)
            self.conv_op("bf_map", [e], self.wadd("bf_map.w", wcimg), self.wadd("bf_map.b", bcimg), pw, N=MLP_LD, epi=prg.EPI_LINEAR,
                         dst=bw.ref)
            self.fwd.append(GenOp(OP_FILTER_SUM, [bw.ref, Ref("in"), Ref("out")], [B, T, F, M, MLP_LD], name="filter_sum"))
            self.gtaps["bf_w"] = self.bf_w = bw

            def back_head_cnn():
                dbw = self.alloc(rows * MLP_LD)
                bw.slot.ref = dbw
                self.bwd.append(GenOp(OP_FS_BWD, [Ref("dout"), Ref("in"), dbw], [B, T, F, M, MLP_LD], name="filter_sum.bwd"))
                self.wgrad_op("bf_map.wgrad", dbw, [e], pw, wcimg, N=MLP_LD, dbias=self.gadd([bcimg]))
                wcd = pack_taps(np.ascontiguousarray(wc.transpose(1, 0, 2)), pw.taps)      # (64 channels of e, 64 padded rows)
                self.dgrad("bf_map.dgrad", e, dbw, [(self.wadd("bf_map.wd", wcd), pw)], N=MLP_LD)
            self.tape.append(back_head_cnn)
            return self._finish_build()

        # ---- LSTM_BF (EaBNet.py:600-614), unfused
        x_ln, mr_ln = self.act(F, 64), self.alloc(rows * 2)
        lg, lb = self.vec("bf_map.norm.weight"), self.vec("bf_map.norm.bias")
        self.fwd.append(GenOp(OP_LN_FWD, [e.ref, lg, lb, x_ln.ref, mr_ln], list(_split64(rows)), [EPS_LN], name="bf_map.norm"))
        h_in, layers = x_ln, []
        for nm in ("rnn1", "rnn2"):
            p = f"bf_map.{nm}"
            wcat_img = np.concatenate([self.idx(f"{p}.weight_ih_l0"), self.idx(f"{p}.weight_hh_l0")], axis=1)
            wcat = self.wadd(f"{p}.wcat", wcat_img)
            bias = self.wadd(f"{p}.bias", self.idx(f"{p}.bias_ih_l0"), self.idx(f"{p}.bias_hh_l0"))
            h, gates = self.act(F, 64), self.alloc(rows * 5 * 64)
            self.fwd.append(GenOp(OP_LSTM_TRAIN, [h_in.ref, wcat, bias, h.ref, gates], [B, T, F, self.lstm_prec], name=p))
            self.flops_fwd += 2 * rows * 256 * 128
            layers.append((p, h_in, h, gates, wcat))
            self.gtaps[p] = h
            h_in = h
        h2 = h_in
        # w_dnn: Linear 64->64 + ReLU, Linear 64->2M (rows padded to one 64-column tile), then the filter-and-sum
        w1 = self.idx("bf_map.w_dnn.0.weight")[:, :, None]
        y1 = self.act(F, 64)
        w1img = pack_taps(w1, pw.taps)
        b1img = self.idx("bf_map.w_dnn.0.bias")
        self.conv_op("bf_map.w_dnn.0", [h2], self.wadd("w_dnn.0.w", w1img), self.wadd("w_dnn.0.b", b1img), pw, N=64, epi=prg.EPI_RELU,
                     dst=y1.ref)
        w2 = np.full((MLP_LD, 64, 1), -1, np.int64)
        w2[:2 * M] = self.idx("bf_map.w_dnn.2.weight")[:, :, None]
        b2img = np.full(MLP_LD, -1, np.int64)
        b2img[:2 * M] = self.idx("bf_map.w_dnn.2.bias")
        w2img = pack_taps(w2, pw.taps)
        bw = self.act(F, MLP_LD)
        self.conv_op("bf_map.w_dnn.2", [y1], self.wadd("w_dnn.2.w", w2img), self.wadd("w_dnn.2.b", b2img), pw, N=MLP_LD,
                     epi=prg.EPI_LINEAR, dst=bw.ref)
        self.fwd.append(GenOp(OP_FILTER_SUM, [bw.ref, Ref("in"), Ref("out")], [B, T, F, M, MLP_LD], name="filter_sum"))

        self.gtaps["bf_w"] = self.bf_w = bw
        self.gtaps["bf_map.ln"] = x_ln
        self.gtaps["bf_map.y1"] = y1

        def back_head():
            dbw = self.alloc(rows * MLP_LD)
            bw.slot.ref = dbw
            self.bwd.append(GenOp(OP_FS_BWD, [Ref("dout"), Ref("in"), dbw], [B, T, F, M, MLP_LD], name="filter_sum.bwd"))
            self.wgrad_op("w_dnn.2.wgrad", dbw, [y1], pw, w2img, N=MLP_LD, dbias=self.gadd([b2img]))
            dy1 = self.alloc(rows * 64)
            src = TVar(dbw, F, MLP_LD)
            self.emit = self.bwd
            w2d = pack_taps(np.ascontiguousarray(w2.transpose(1, 0, 2)), pw.taps)          # (64 y1-channels, 64 padded rows)
            self.conv_op("w_dnn.2.dgrad", [src], self.wadd("w_dnn.2.wd", w2d), None, pw, N=64, epi=prg.EPI_LINEAR, dst=dy1)
            self.emit = self.fwd
            dpre = self.alloc(rows * 64)
            self.bwd.append(GenOp(OP_RELU_BWD, [dy1, y1.ref, dpre], list(_split64(rows * 64)), name="w_dnn.relu_bwd"))
            self.wgrad_op("w_dnn.0.wgrad", dpre, [h2], pw, w1img, N=64, dbias=self.gadd([b1img]))
            w1d = pack_taps(np.ascontiguousarray(w1.transpose(1, 0, 2)), pw.taps)
            self.dgrad("w_dnn.0.dgrad", h2, dpre, [(self.wadd("w_dnn.0.wd", w1d), pw)], N=64)
            for p, hin, h, gates, wcat in reversed(layers):
                dg = self.alloc(rows * 256)
                self.bwd.append(GenOp(OP_LSTM_BWD, [gates, self.grad_of(h), wcat, dg], [B, T, F, self.lstm_prec], name=p + ".bwd"))
                self.flops_bwd += 2 * rows * 256 * 64
                self.wgrad_op(p + ".wgrad_ih", dg, [hin], pw, self.idx(f"{p}.weight_ih_l0"), N=256,
                              dbias=self.gadd([self.idx(f"{p}.bias_ih_l0"), self.idx(f"{p}.bias_hh_l0")]))
                # (the recurrent product reads the hidden state of the previous frame)
                self.wgrad_op(p + ".wgrad_hh", dg, [h], Geometry.pointwise(F, dt=-1), self.idx(f"{p}.weight_hh_l0"), N=256)
                wih_d = pack_taps(np.ascontiguousarray(self.idx(f"{p}.weight_ih_l0").T)[:, :, None], pw.taps)   # (64, 256)
                self.dgrad(p + ".dgrad", hin, dg, [(self.wadd(p + ".wd", wih_d), pw)], N=256)
            de = self.alloc(rows * 64)
            self.bwd.append(GenOp(OP_LN_BWD, [self.grad_of(x_ln), e.ref, mr_ln, lg, de, self.gvec("bf_map.norm.weight"),
                                              self.gvec("bf_map.norm.bias")], list(_split64(rows)), name="bf_map.norm.bwd"))
            self.contribute(e, de)
        self.tape.append(back_head)
        return self._finish_build()

    def _finish_build(self) -> "TrainProgram":
        # ---- backward: replay the tape in reverse
        for fn in reversed(self.tape):
            fn()
        if self.input_grad:
            # din = the filter-and-sum's adjoint w.r.t. X + the first convolution's data gradient, one launch (csrc/input_grad.hip)
            assert self.din_tile is not None and self.bf_w is not None, "no convolution read the network input"
            self.bwd.append(GenOp(OP_INPUT_GRAD, [Ref("dout"), self.bf_w.ref, self.grad_of(self.din_tile), Ref("din")],
                                  [self.B, self.T, self.F, self.cfg.M, MLP_LD], name="input_grad"))
        return self.finish()

    def assign_bf16_storage(self) -> None:
        """bf16 programs: STORE as bf16 every tensor that nothing but bf16 contractions read (BASELINE configs[3]: "bf16").
        Those kernels round their operands to bf16 on the way into LDS, so a tensor whose only readers are the gather of a bf16
        convolution (forward or dgrad) and the bf16 weight-gradient kernel can be written in bf16 by its producer: the
        contractions see the same bits, the producer writes and the consumers read half the bytes, and the consumers convert
        nothing.  What qualifies in practice: the normalised activations between the 2-D units (producer tr_norm_act) and the
        gradients of the 2-D convolution outputs (producers: the apply pass of the norm backward, the GLU backward).  Everything
        else -- raw convolution outputs and their statistics, residual operands, gradients that accumulate, the S-TCN (small-
        tile kernel), LSTM, head -- stays fp32.  Decided on the finished op lists: a region of the activation arena becomes bf16
        iff it has exactly one writer, that writer can store bf16, and every reader is such a contraction; regions keep their
        size and offset (a bf16 tensor occupies the first half), so nothing else of the program changes."""
        import bisect
        starts = [a for a, _ in self.allocs]

        def region(ref: Optional[Ref]) -> Optional[int]:
            if ref is None or ref.arena != "a":
                return None
            k = bisect.bisect_right(starts, ref.off) - 1
            return k if k >= 0 and ref.off < starts[k] + max(self.allocs[k][1], 1) else None
        uses: Dict[int, list] = {}

        def note(ref, what, op, arg=None):
            k = region(ref)
            if k is not None:
                # a use that does not start at the region's first element is a partial view: never converted
                uses.setdefault(k, []).append((what if ref.off == starts[k] else "other", op, arg))

        def conv_reads_bf16(op) -> bool:
            return (op.precision == prg.PREC_BF16 and op.korder == prg.KORDER_TAP and op.xf_mode == prg.XF_NONE and op.Fin > 1
                    and op.C0 % 16 == 0 and op.C1 % 16 == 0 and op.epi != prg.EPI_DUALGATE and not getattr(op, "win", False)
                    and op.fin_stats is None)
        for op in list(self.fwd) + list(self.bwd) + list(self.deferred):
            if isinstance(op, prg.ConvOp):
                ok = conv_reads_bf16(op)
                note(op.src0, "read" if ok and op.C0 % 32 == 0 else "other", op, ("conv", 1))      # (walked in 32-channel units)
                note(op.src1, "read" if ok and op.C1 % 32 == 0 else "other", op, ("conv", 2))
                for f in ("aux", "dst", "dst_acc", "stats", "glu_dump", "xf0", "xf1", "fin_stats", "f2_dst", "f2_stats"):
                    note(getattr(op, f, None), "other", op)
            elif isinstance(op, WgradOp):
                ok = op.precision == prg.PREC_BF16
                note(op.dz, "read" if ok and op.N % 4 == 0 else "other", op, ("wgrad", 1))
                note(op.src0, "read" if ok and op.C0 % 16 == 0 else "other", op, ("wgrad", 2))
                note(op.src1, "read" if ok and op.C0 % 16 == 0 and op.C1 % 16 == 0 else "other", op, ("wgrad", 4))
            elif isinstance(op, GenOp):
                writer = {OP_TR_NORM_ACT: 4, OP_GLU_BWD: 2}.get(op.kind)
                if op.kind == OP_NORM_BWD and len(op.i) == 4 and op.p[7] is None:
                    writer = 8                                   # dx of the single-tensor norm backward, not accumulating
                for j, r in enumerate(op.p):
                    note(r, "write" if j == writer else "other", op, j)
            else:                                                # MemsetOp, FinalizeOp, ...: whatever they touch stays fp32
                for v in vars(op).values():
                    if isinstance(v, Ref):
                        note(v, "other", op)
        chosen = {k for k, lst in uses.items()
                  if "other" not in [w for w, _, _ in lst] and [w for w, _, _ in lst].count("write") == 1
                  and "read" in [w for w, _, _ in lst]}
        # the two sources of a concatenation are read by ONE launch: keep the weight-gradient kernel's operand loads uniform
        # (both sources bf16, or both fp32) -- drop a tensor whose partner in some two-source launch does not qualify
        while True:
            drop = set()
            for op in list(self.fwd) + list(self.bwd) + list(self.deferred):
                if isinstance(op, (prg.ConvOp, WgradOp)) and op.src1 is not None:
                    a, b = region(op.src0), region(op.src1)
                    if (a in chosen) != (b in chosen):
                        drop |= {a, b} & chosen
            if not drop:
                break
            chosen -= drop
        for k in sorted(chosen):
            lst = uses[k]
            self.bf16_tensors += 1
            for what, op, arg in lst:
                if what == "write":
                    if op.kind == OP_GLU_BWD:
                        op.i = list(op.i[:3]) + [STORE_BF16]
                    else:
                        op.i[3] |= STORE_BF16                    # (mode word of eab_train_norm_act_f32 / eab_train_norm_bwd_f32)
                elif arg[0] == "conv":
                    op.src_bf16 = getattr(op, "src_bf16", 0) | arg[1]
                else:
                    op.bf16_mask |= arg[1]

    def finish(self) -> "TrainProgram":
        ia = np.concatenate([a for a, _ in self.w_imgs]).astype(np.int32)
        has_b = any(b is not None for _, b in self.w_imgs)
        ib = np.concatenate([(b if b is not None else np.full(a.size, -1, np.int64)) for a, b in self.w_imgs]).astype(np.int32) \
            if has_b else None
        inv = np.full(self.n_params, -1, np.int64)
        for off, flats in self.g_imgs:
            for fl in flats:
                m = fl >= 0
                tgt = fl[m]
                assert (inv[tgt] == -1).all(), "a parameter element received two gradient entries"
                inv[tgt] = off + np.nonzero(m)[0]
        if self.prec == prg.PREC_BF16 and self.bf16_store:
            self.assign_bf16_storage()

        def geometry(o: WgradOp):
            return (o.N, o.C0, o.C1, o.Kpad, o.Fin, o.Fz, o.No, o.ostride, o.ophase, o.istride, tuple(o.dt), tuple(o.ioff),
                    o.src1 is None, o.dbias is None, o.precision, o.bf16_mask)
        order: Dict[tuple, int] = {}
        for o in self.deferred:
            order.setdefault(geometry(o), len(order))
        for o in self.deferred:
            o.lane = 0
        self.bwd.extend(sorted(self.deferred, key=lambda o: order[geometry(o)]))      # stable: first-seen geometry first
        self.deferred = []
        return TrainProgram(cfg=self.cfg, B=self.B, T=self.T, F=self.F, fwd=self.fwd, bwd=self.bwd, a_floats=self.a_size,
                            w_floats=self.w_size, g_floats=self.g_size, ia=ia, ib=ib, inv=inv.astype(np.int32),
                            n_params=self.n_params, keys=list(self.specs), shapes=[tuple(s.shape) for s in self.specs.values()],
                            flops_fwd=self.flops_fwd, flops_bwd=self.flops_bwd,
                            grad_taps={k: (v.slot.ref, v.F, v.C) for k, v in self.gtaps.items() if v.slot.ref is not None},
                            lanes={"fwd": [o.lane for o in self.fwd], "bwd": [o.lane for o in self.bwd]}, sync=self.sync,
                            bn_layers=list(self.bn_layers), input_grad=self.input_grad)


@dataclass
class TrainProgram:
    cfg: NetConfig
    B: int
    T: int
    F: int
    fwd: list
    bwd: list
    a_floats: int
    w_floats: int
    g_floats: int
    ia: np.ndarray
    ib: Optional[np.ndarray]
    inv: np.ndarray
    n_params: int
    keys: List[str]
    shapes: List[tuple]
    flops_fwd: int = 0
    flops_bwd: int = 0
    grad_taps: Dict[str, tuple] = field(default_factory=dict)       # name -> (Ref of d loss / d activation, F, C)
    out_shape: Optional[tuple] = None        # shape of the 'out' / 'dout' arenas (default: the beam-former's (B, 2, T, F))
    has_in2: bool = False                    # a second input arena 'in2' (the post-filter's previous estimate)
    lanes: Dict[str, list] = field(default_factory=dict)          # per program: lane of every op (0 = the caller's stream)
    sync: Dict[str, dict] = field(default_factory=dict)           # per program: op index -> [("fork" | "join", lanes)]
    # BatchNorm (train mode): (norm key, offset of the layer's batch (mean, rstd) table in the activation arena, C, samples)
    bn_layers: List[tuple] = field(default_factory=list)
    varlen: bool = False                     # the ops that sum or recurse across rows read per-utterance lengths (flag_varlen)
    bucket: bool = False                     # T is a cap serving every call of T frames or fewer (train_length_buckets)
    input_grad: bool = False                 # the backward list also writes the boundary buffer 'din' (B, T, F, M, 2)


# op kinds that honour eab_op.win.lens in the training programs, with the i[] slots that carry (B, T) where the op has none
# (written by runtime.encode only together with the lengths pointer); the convolutions carry lens in their own descriptor
VARLEN_KINDS = {OP_IN_STATS: ("T", 4), OP_NORM_BWD: ("T", 5), OP_LN_BWD: ("BT", 2), OP_LSTM_BWD: None, OP_FILTER_SUM: None,
                OP_WGRAD: None, prg.OP_GAG_CRM_BWD: None, OP_INPUT_GRAD: None}
# (the post-filter's GAG_PACK and GAG_CRM are prg.GagPackOp / GagCrmOp: they have a `win` attribute of their own and honour lens)
# the length-bucket form also bounds the two LSTM recurrences by the longest length of a workgroup: the forward
# takes the pointer, the backward a flag in i[4] (written, like every lens_i slot, only together with the pointer)
BUCKET_KINDS = {OP_LSTM_TRAIN: None, OP_LSTM_BWD: ("flag", 4)}


def flag_varlen(prog: TrainProgram, bucket: bool = False, lstm_bound: bool = True) -> TrainProgram:
    """Mark the readers that sum or recurse across rows: runtime.encode hands the lengths pointer of the binding
    to every op that has a ``win`` attribute.  The op lists themselves do not change; row-local ops stay unflagged (they carry
    whatever the padding rows hold to padding rows only).  bucket: prog.T is a cap that serves every narrower call -- the LSTM
    recurrences stop at the longest length of a workgroup (BUCKET_KINDS); lstm_bound=False leaves them walking the cap (what
    tools/bench_train_buckets.py measures the bound against)."""
    lstm = bucket and lstm_bound
    for op in list(prog.fwd) + list(prog.bwd):
        if op.kind in VARLEN_KINDS:
            op.win = False                                       # (no streaming window: the attribute is what encode looks for)
            slot = VARLEN_KINDS[op.kind]
            if slot is not None:
                op.lens_i = {slot[1]: prog.T} if slot[0] == "T" else {slot[1]: prog.B, slot[1] + 1: prog.T}
        if lstm and op.kind in BUCKET_KINDS:
            op.win = False
            if BUCKET_KINDS[op.kind] is not None:
                op.lens_i = {BUCKET_KINDS[op.kind][1]: 1}
    prog.varlen = True
    prog.bucket = bucket
    return prog


def varlen_unsupported_reason(cfg) -> str:
    """why a configuration cannot train with per-utterance lengths ('' when it can)"""
    norm = getattr(cfg, "norm_type", "IN")
    if norm == "BN":
        return ("norm_type='BN' in train mode needs masked batch statistics and a masked update of the running buffers, "
                "which are not implemented")
    if norm == "cLN":
        return "norm_type='cLN': the three-launch reverse scan of its backward has no per-utterance masks yet"
    if not cfg.is_causal:
        return ("is_causal=True is needed -- the non-causal S-TCM taps of the last frames of an utterance read the frames "
                "after it, so a padded batch cannot reproduce the one-at-a-time result")
    return ""


def lower_train(cfg: NetConfig, B: int, T: int, F: int = 161, precision: str = "f32", varlen: bool = False,
                bucket: bool = False, lstm_bound: bool = True, input_grad: bool = False) -> TrainProgram:
    """varlen: the same op list with the cross-row readers flagged for per-utterance lengths (flag_varlen); T is the padded
    width.  bucket: the same with T a cap (the LSTM recurrences flagged too).  Configurations outside is_causal=True /
    norm_type='IN' are refused.  input_grad: the backward list also produces the gradient of the input in the boundary buffer
    'din' (see the module docstring); False is the program as it always was."""
    if (varlen or bucket) and varlen_unsupported_reason(cfg):
        raise NotImplementedError("training with per-utterance lengths: " + varlen_unsupported_reason(cfg))
    prog = TrainLowering(cfg, B, T, F, precision, input_grad=input_grad).build()
    return flag_varlen(prog, bucket, lstm_bound) if (varlen or bucket) else prog


# ----------------------------------------------------------------------------------------------------------------
# binding and execution
# ----------------------------------------------------------------------------------------------------------------
class TrainBound(BoundProgram):
    """Device arenas + the forward ("fwd") and backward ("bwd") op lists of a lowered training program."""
    BOUNDARY = ("in", "out", "dout", "in2", "din")

    def __init__(self, prog: TrainProgram, device: torch.device):
        self.prog = prog
        self.acts = torch.empty(max(prog.a_floats, 1), dtype=torch.float32, device=device)
        self.w = torch.empty(max(prog.w_floats, 1), dtype=torch.float32, device=device)
        self.g = torch.empty(max(prog.g_floats, 1), dtype=torch.float32, device=device)
        super().__init__(device, {"a": self.acts, "w": self.w, "g": self.g}, {"fwd": prog.fwd, "bwd": prog.bwd},
                         prog.lanes, prog.sync)
        self.ia = torch.from_numpy(prog.ia).to(device)
        self.ib = torch.from_numpy(prog.ib).to(device) if prog.ib is not None else None
        self.inv = torch.from_numpy(prog.inv).to(device)
        # per-utterance lengths (varlen programs): ONE device array [B] that both op lists -- and so both captured graphs --
        # read through a fixed pointer; written on the launch stream before the forward, read again by the backward
        self.lens = torch.full((prog.B,), prog.T, dtype=torch.int32, device=device) if prog.varlen else None
        if prog.varlen:
            self.window = {"lens": self.lens.data_ptr()}
        self.serial = 0                     # forward passes run so far: a backward must belong to the latest one
        self.use_graph = True
        self.flat_param_hits = 0            # forward passes that read the parameters from one flat buffer (no torch.cat)

    def update_bn_buffers(self, module, momentum: float = 0.1) -> None:
        """nn.BatchNorm's train-mode side effect (NormSwitch BN branch, EaBNet.py:677-681): running_mean / running_var move
        by `momentum` towards the batch mean / UNBIASED batch variance, num_batches_tracked counts the step.  The batch
        statistics are read back from the (mean, rstd) tables the forward program just wrote -- a handful of torch
        foreach launches on the caller's stream for all norms of the network."""
        L = self.prog.bn_layers
        if not L:
            return
        if getattr(self, "_bn_idx", None) is None:
            idx = np.concatenate([off + 2 * np.arange(C, dtype=np.int64) for _, off, C, _ in L])
            unb = np.concatenate([np.full(C, n / max(n - 1, 1), np.float32) for _, _, C, n in L])
            self._bn_idx = torch.from_numpy(idx).to(self.acts.device)
            self._bn_unb = torch.from_numpy(unb).to(self.acts.device)
            self._bn_split = [C for _, _, C, _ in L]
        with torch.no_grad():
            mean = self.acts[self._bn_idx]
            rstd = self.acts[self._bn_idx + 1]
            var = (1.0 / (rstd * rstd) - EPS_IN).clamp_min_(0.0) * self._bn_unb
            rm = [module.get_buffer(f"{k}.norm.running_mean") for k, *_ in L]
            rv = [module.get_buffer(f"{k}.norm.running_var") for k, *_ in L]
            torch._foreach_lerp_(rm, list(mean.split(self._bn_split)), momentum)
            torch._foreach_lerp_(rv, list(var.split(self._bn_split)), momentum)
            torch._foreach_add_([module.get_buffer(f"{k}.norm.num_batches_tracked") for k, *_ in L], 1)

    def pack(self, flat: torch.Tensor, stream: int) -> None:
        _lib.check(_lib.load().eab_gather_f32(flat.data_ptr(), self.ia.data_ptr(), self.ib.data_ptr() if self.ib is not None else None,
                                              self.w.data_ptr(), self.prog.w_floats, C.c_void_p(stream)), "eab_gather_f32")

    def unpack_grads(self, gflat: torch.Tensor, stream: int) -> None:
        _lib.check(_lib.load().eab_gather_f32(self.g.data_ptr(), self.inv.data_ptr(), None, gflat.data_ptr(), self.prog.n_params,
                                              C.c_void_p(stream)), "eab_gather_f32(grads)")


class TrainFn(torch.autograd.Function):
    """One autograd node for a whole network: forward program, backward program.  ``inputs``: (x,) for EaBNet, (inpt, pre_x)
    for GaGNet; no gradient flows to them.  ``sync_group``: see finish_flat_gradient."""

    @staticmethod
    def forward(ctx, bound: TrainBound, sync_group, inputs: tuple, *params: torch.Tensor) -> torch.Tensor:
        prog = bound.prog
        ctx.sync_group = sync_group
        st = torch.cuda.current_stream().cuda_stream
        flat = flat_parameter_view(params)                              # FlatAdam's buffer: nothing to copy
        if flat is not None:
            bound.flat_param_hits += 1
        else:
            flat = torch.cat([p.detach().reshape(-1) for p in params])  # (one batched copy; fp32 parameters)
            if flat.dtype != torch.float32:
                flat = flat.to(torch.float32)
        bound.pack(flat, st)
        bound.serial += 1
        ctx.serial = bound.serial
        x, x2 = inputs[0], (inputs[1] if len(inputs) > 1 else None)
        out_shape = prog.out_shape or (prog.B, 2, prog.T, prog.F)
        # a length-bucket program (prog.T is a cap) serves a call of Tc <= prog.T frames: the inputs go into the first Tc frames
        # of its boundary buffers, the output's first Tc frames come back; what lies behind stays as it is (its readers are masked)
        tax = 1 if x.ndim == 5 else 2
        Tc = ctx.Tc = x.shape[tax]
        wide = lambda t: None if t is None else tuple(t.shape[:tax]) + (prog.T,) + tuple(t.shape[tax + 1:])  # noqa: E731
        din_shape = wide(x) if prog.input_grad else None        # the input's gradient: a boundary buffer of the backward list
        if bound.use_graph and bound.capture(wide(x), out_shape, out_shape, wide(x2), din_shape):
            if Tc == prog.T:
                bound.static["in"].copy_(x)
                if x2 is not None:
                    bound.static["in2"].copy_(x2)
            else:
                bound.static["in"].narrow(tax, 0, Tc).copy_(x)
                if x2 is not None:
                    bound.static["in2"].narrow(tax, 0, Tc).copy_(x2)
            bound.graphs["fwd"].replay()
            out = bound.static["out"].clone() if Tc == prog.T else bound.static["out"][..., :Tc, :].clone()
            ctx.io = None
        else:
            if Tc != prog.T:
                xw = x.new_empty(wide(x))
                xw.narrow(tax, 0, Tc).copy_(x)
                x = xw
                if x2 is not None:
                    x2w = x2.new_empty(wide(x2))
                    x2w.narrow(tax, 0, Tc).copy_(x2)
                    x2 = x2w
            out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
            ctx.io = (x, out, torch.empty_like(out), x2, None if din_shape is None else x.new_empty(din_shape))
            bound.bind(*(None if t is None else t.data_ptr() for t in ctx.io))
            bound.run("fwd", st)
            if Tc != prog.T:
                out = out[..., :Tc, :].clone()
        ctx.bound = bound
        ctx.shapes = [p.shape for p in params]
        ctx.dtypes = [p.dtype for p in params]
        return out

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        bound, prog = ctx.bound, ctx.bound.prog
        st = torch.cuda.current_stream().cuda_stream
        if ctx.serial != bound.serial:
            raise RuntimeError("eabnet_amd: backward of a forward pass whose saved activations were overwritten by a later "
                               "forward of the same module (one training program holds one set of activations)")
        bound.g.zero_()
        if ctx.io is None:
            (bound.static["dout"] if ctx.Tc == prog.T else bound.static["dout"][..., :ctx.Tc, :]).copy_(grad_out)
            bound.graphs["bwd"].replay()
        else:
            (ctx.io[2] if ctx.Tc == prog.T else ctx.io[2][..., :ctx.Tc, :]).copy_(grad_out.to(torch.float32))
            bound.bind(*(None if t is None else t.data_ptr() for t in ctx.io))
            bound.run("bwd", st)
        gflat = torch.empty(prog.n_params, dtype=torch.float32, device=bound.device)     # fresh per call: .grad may keep views of it
        bound.unpack_grads(gflat, st)
        grads = finish_flat_gradient(gflat, ctx.sync_group, ctx.shapes, ctx.dtypes, ctx.needs_input_grad[3:])
        ctx.din = None
        if prog.input_grad:                                            # (a fresh tensor per call: .grad may keep it)
            din = bound.static["din"] if ctx.io is None else ctx.io[4]
            ctx.din = din.narrow(1, 0, ctx.Tc).clone() if (ctx.io is None or ctx.Tc != prog.T) else din
        return (None, None, None, *grads)


class TrainInputFn(TrainFn):
    """TrainFn for a program lowered with input_grad: the network input is an argument of the node, and the backward returns
    the boundary buffer `din`, narrowed to the call's width, as its gradient.  ``x`` is fp32 and contiguous."""

    @staticmethod
    def forward(ctx, bound: TrainBound, sync_group, x: torch.Tensor, *params: torch.Tensor) -> torch.Tensor:
        assert bound.prog.input_grad
        return TrainFn.forward(ctx, bound, sync_group, (x.detach(),), *params)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        _, _, _, *grads = TrainFn.backward(ctx, grad_out)
        return (None, None, ctx.din, *grads)


def flat_parameter_view(params) -> Optional[torch.Tensor]:
    """The 1-D fp32 tensor that ``params`` are consecutive contiguous slices of, in order (what eabnet_amd.FlatAdam leaves
    behind), or None.  Exact: every parameter is checked for its address, dtype and contiguity, and the run for lying inside
    the first parameter's storage (addresses are unique across devices)."""
    first, f32 = params[0], torch.float32
    nxt = start = first.data_ptr()
    for p in params:
        if p.data_ptr() != nxt or p.dtype is not f32 or not p.is_contiguous():
            return None
        nxt += 4 * p.numel()
    store = first.untyped_storage()
    if start < store.data_ptr() or nxt > store.data_ptr() + store.nbytes():
        return None
    return torch.as_strided(first.detach(), ((nxt - start) // 4,), (1,))


def finish_flat_gradient(gflat: torch.Tensor, sync_group, shapes, dtypes, needs) -> list:
    """What a training autograd node does with the flat gradient its backward program produced: average it over the ranks
    (ONE all-reduce of the contiguous buffer -- the reference's DDP bucket all-reduce, train_distributed.py:198,228, without
    per-parameter hooks or bucket copies; sync_group None = no synchronisation, True = the default process group) and hand it
    back as one view per parameter (None for parameters that need no gradient).  Device-agnostic: tests/test_dist_gloo.py runs
    it on two gloo ranks."""
    if sync_group is not None:
        import torch.distributed as td
        grp = sync_group if sync_group is not True else None
        td.all_reduce(gflat, group=grp)
        gflat.div_(td.get_world_size(grp))
    # one split call + a view per parameter (a Python loop over ~500-800 parameters is on the step's critical path)
    sizes = [int(np.prod(shp)) if len(shp) else 1 for shp in shapes]
    grads = [g.view(shp) if dt == torch.float32 else g.view(shp).to(dt) for g, shp, dt in zip(gflat.split(sizes), shapes, dtypes)]
    if not all(needs):
        grads = [g if need else None for g, need in zip(grads, needs)]
    return grads


def forward_train(module, inputs: tuple, lower, lengths=None, cap: Optional[int] = None, x_leaf: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A differentiable forward of ``module`` on its HIP training programs, lowered by ``lower(cfg, B, T, F, precision)``
    (lower_train here, train_gag.lower_train for GaGNet).  ``inputs``: fp32, contiguous, (B, T, F, M, 2) for EaBNet or two
    (B, 2, T, F) for GaGNet.  Returns the program's output arena ((B, 2, T, F), or (q, B, 2, T, F) for GaGNet).
    ``lengths`` (checked by model.check_lengths: a list or a device tensor of B frame counts): the program lowered with
    varlen=True, its lengths array written on the current stream before the forward replay -- no host synchronisation.
    ``cap`` (train_length_buckets): the program lowered with bucket=True at width ``cap`` >= T serves the call;
    ``lengths`` is then a list, a device tensor or one int for every utterance; returned tensors have the call's width T.
    ``x_leaf`` (EaBNet.input_grad): inputs[0] as a tensor of the caller's graph, fp32 and contiguous -- the program is lowered
    with input_grad=True and the node hands the gradient of the input back to it."""
    _lib.load()
    x = inputs[0]
    B, T, F = (x.shape[0], x.shape[1], x.shape[2]) if x.ndim == 5 else (x.shape[0], x.shape[2], x.shape[3])
    cache = module.__dict__.setdefault("_train_bound", {})
    prec = "bf16" if module.precision == "bf16" else "f32"
    varlen = lengths is not None
    bucket = cap is not None
    assert not bucket or (varlen and cap >= T)
    Tp = cap if bucket else T                          # the width of the program
    # (a bucket program's key carries the cap in place of T and one more member, the bucket flag; the others keep their form)
    # (module.train_bucket_lstm_bound = False, a measurement switch: the bucket program with both LSTM recurrences walking the cap)
    lstm_bound = bool(getattr(module, "train_bucket_lstm_bound", True))
    key = (B, Tp, F, str(x.device), prec, varlen) + (((True,) if lstm_bound else ("lstm_walks_cap", True)) if bucket else ())
    ig = x_leaf is not None
    if ig:                                             # (the other keys keep their form)
        key += ("input_grad",)
        lower = functools.partial(lower, input_grad=True)
    bound = cache.pop(key, None)
    if bound is None:
        # a small LRU of bound programs (variable-length batches, a smaller last batch, alternating train / validation
        # shapes): re-lowering and re-capturing two hipGraphs on every shape change costs seconds
        while len(cache) >= TRAIN_BOUND_CACHE:
            torch.cuda.synchronize(x.device)      # the dropped program's arenas may still be read by kernels in flight
            cache.pop(next(iter(cache)))
        with torch.cuda.device(x.device):
            prog = (lower(module.cfg, B, Tp, F, prec, bucket=True, lstm_bound=lstm_bound) if bucket else
                    lower(module.cfg, B, T, F, prec, varlen=True) if varlen else lower(module.cfg, B, T, F, prec))
            bound = TrainBound(prog, x.device)
    cache[key] = bound                               # most recently used last
    bound.use_graph = bool(getattr(module, "use_graph", True)) and not torch.cuda.is_current_stream_capturing()
    sd = dict(module.named_parameters())
    params = [sd[k] for k in bound.prog.keys]
    sync = module.__dict__.get("grad_allreduce", None)          # None | True (default group) | a process group
    with torch.cuda.device(x.device):
        if varlen:
            if isinstance(lengths, int):
                bound.lens.fill_(lengths)
            elif isinstance(lengths, torch.Tensor):
                bound.lens.copy_(lengths.to(torch.int32), non_blocking=True)
            else:
                bound.lens.copy_(torch.as_tensor(lengths, dtype=torch.int32).pin_memory(), non_blocking=True)
        out = TrainInputFn.apply(bound, sync, x_leaf, *params) if ig else TrainFn.apply(bound, sync, inputs, *params)
        bound.update_bn_buffers(module)
    return out


def enable_flat_allreduce(module, group=True) -> None:
    """Data-parallel training without a DistributedDataParallel wrapper: every backward of ``module`` (an
    eabnet_amd.EaBNet on the HIP training path) all-reduces its flat gradient once and averages it over the ranks.
    Parameters must start identical on all ranks (broadcast them once, as DDP's constructor does)."""
    module.grad_allreduce = group


def broadcast_parameters(module, src: int = 0) -> None:
    import torch.distributed as td
    if td.is_available() and td.is_initialized():
        for t in list(module.parameters()) + list(module.buffers()):
            td.broadcast(t.data, src)
