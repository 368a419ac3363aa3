"""Bound op programs: the host side of ``eab_run_program`` shared by inference (model._Bound) and training
(train.TrainBound).

``encode`` turns a list of lowered ops and the base address of every arena into the C ABI's ``eab_op`` array (plain
ctypes: it needs neither a device nor the library).  ``BoundProgram`` owns a program's arenas and one encoded array per
op list, re-encodes them when the boundary pointers change, captures them as single-stream hipGraphs per lane segment
(graphs.LaneGraphs) and runs them directly, whole or op by op."""
from __future__ import annotations

import ctypes as C
import functools
import os
import warnings
from typing import Callable, Dict, List, Mapping, Optional, Sequence, Tuple

import torch

from . import _lib
from . import program as prg
from .graphs import LaneGraphs, plan_segments, single_lane

# eab_conv_desc and eab_wgrad_desc: fields written from the op attribute of the same name
_CONV_PTRS = ("src0", "src1", "xf0", "xf1", "slope0", "slope1", "w", "bias", "aux", "dst", "dst_acc", "stats", "stat_slope0",
              "stat_slope1", "fin_stats", "fin_gamma0", "fin_beta0", "fin_gamma1", "fin_beta1", "fz_counter", "fz_gamma0",
              "fz_beta0", "fz_xf0", "fz_gamma1", "fz_beta1", "fz_xf1", "glu_dump", "ph1_w", "f2_w", "f2_dst", "f2_stats",
              "f2_stat_slope0", "f2_stat_slope1")
_CONV_INTS = ("C0", "C1", "xf_mode", "N", "Kpad", "B", "T", "Fin", "Fout", "No", "ostride", "ophase", "istride", "epi", "Cout",
              "nsets", "stat_tiles", "stat_tile0", "bm", "fin_tiles", "fin_nsets", "fin_count", "precision", "korder",
              "p2_mask1", "src_bf16", "ph1_No", "ph1_ophase", "ph1_Kpad", "f2_N", "f2_nsets", "f2_stat_tiles")
_CONV_FLOATS = ("fin_eps", "fz_eps")
_WGRAD_PTRS = ("dz", "src0", "src1", "dw", "dbias")
_WGRAD_INTS = ("N", "C0", "C1", "Kpad", "B", "T", "Fin", "Fz", "No", "ostride", "ophase", "istride", "precision", "bf16_mask")
# every other op class: the attributes that fill eab_op.i[], .p[] and .f[] in order (an int is a constant).  An op of a
# class not listed (train.GenOp) carries its own i / p / f lists.
_LAYOUT = {
    prg.FinalizeOp: (("B", "C", "nsets", "stat_tiles", "count"),
                     ("stats", "gamma0", "beta0", "xf0", "gamma1", "beta1", "xf1", "mr0"), ("eps",)),
    prg.NormActOp: (("B", "P", "C", "T"), ("a", "xfa", "slopea", "b", "xfb", "slopeb", "out"), ()),
    prg.LstmOp: (("B", "T", "F", "precision"), ("x", "ln_g", "ln_b", "wcat", "bias", "h_out", "c_state"), ("ln_eps",)),
    prg.BfwOp: (("B", "T", "F", "M"), ("y1", "w2", "b2", "x", "out", "bfw", "w1", "b1"), ()),
    prg.MemsetOp: ((None, None, "B", "T", "row"), ("ptr",), ()),           # i[0:2]: the byte count, split below
    prg.ClnStatsOp: (("B", "T", "P", "C"), ("x", "slope", "sums", "state", "mr"), ("eps",)),
    prg.ClnApplyOp: (("B", "T", "P", "C", "mode"), ("x", "mr", "gain", "bias", "slope", "add", "out"), ()),
    prg.GateRowsOp: (("B", "T", "row"), ("a", "r", "z"), ()),
    prg.GagPackOp: (("B", "T", "F", "pre_ld"), ("inpt", "pre_x", "enc_in", "pre"), ()),
    prg.GagCrmOp: (("B", "T", "F", "pre_ld", prg.GAG_LIN_LD, "act"), ("pre", "g", "r", "i", "pre_out", "planar"), ()),
    prg.ClnStepOp: (("B", "T", "P", "C", "mode"),
                    ("x", "stat_slope", "sums", "state", "mr", "gain", "bias", "slope", "add", "out"), ("eps",)),
    prg.ConvChainOp: (("n", "B", "lds_bytes", "bf16"), ("descs", "codes"), ()),
}


def _i32(v) -> int:
    return C.c_int32(int(v) & 0xFFFFFFFF).value


def _taps(dt, ioff, n: int, dst_dt, dst_ioff) -> None:
    for j in range(n):
        dst_dt[j] = dt[j] if j < len(dt) else 0
        dst_ioff[j] = ioff[j] if j < len(ioff) else 0


def encode(ops: Sequence, bases: Mapping[str, Optional[int]], t_pos: Optional[int] = None, chunk: int = 0,
           lens: Optional[int] = None, out=None):
    """The ``eab_op`` array of ``ops`` with every Ref resolved against ``bases`` (arena name -> base address).  Windowed ops
    (op.win) of a streaming program read the frame position at ``t_pos`` and advance ``chunk`` frames; ``lens`` is the
    per-utterance length array of a varlen program, given to every op that has a time window.  ``out``: an array of
    len(ops) to encode into (default: a new one)."""
    arr = (_lib.Op * len(ops))() if out is None else out

    def A(r):
        return None if r is None else bases[r.arena] + 4 * r.off
    for o, op in zip(arr, ops):
        o.kind = op.kind
        win = o.conv.win if op.kind == prg.OP_CONV else o.win
        if getattr(op, "win", False):
            win.pos, win.count = t_pos, chunk
        if lens is not None and hasattr(op, "win"):
            win.lens = lens
        if op.kind == prg.OP_CONV:
            d = o.conv
            for f in _CONV_PTRS:
                setattr(d, f, A(getattr(op, f)))
            for f in _CONV_INTS:
                setattr(d, f, int(getattr(op, f)))
            for f in _CONV_FLOATS:
                setattr(d, f, float(getattr(op, f)))
            d.ntaps, d.ph1_ntaps = len(op.dt), len(op.ph1_dt)
            _taps(op.dt, op.ioff, _lib.MAX_TAPS, d.dt, d.ioff)
            _taps(op.ph1_dt, op.ph1_ioff, _lib.MAX_TAPS, d.ph1_dt, d.ph1_ioff)
        elif op.kind == prg.OP_WGRAD:
            d = o.wgrad
            for f in _WGRAD_PTRS:
                setattr(d, f, A(getattr(op, f)))
            for f in _WGRAD_INTS:
                setattr(d, f, int(getattr(op, f)))
            d.ntaps = len(op.dt)
            _taps(op.dt, op.ioff, _lib.MAX_TAPS, d.dt, d.ioff)
        else:
            layout = _LAYOUT.get(type(op))
            if layout is None:
                ints, ptrs, flts = op.i, op.p, op.f
            else:
                ints = [a if a is None or isinstance(a, int) else getattr(op, a) for a in layout[0]]
                ptrs = [getattr(op, a) for a in layout[1]]
                flts = [getattr(op, a) for a in layout[2]]
                if op.kind == prg.OP_MEMSET0:
                    nbytes = 4 * op.nfloats
                    ints[0:2] = [nbytes & 0xFFFFFFFF, nbytes >> 32]
            for j, v in enumerate(ints):
                o.i[j] = _i32(v)
            if lens is not None:                        # (B, T) of a training op that carries none, for its lengths form
                for j, v in (getattr(op, "lens_i", None) or {}).items():
                    o.i[j] = _i32(v)
            for j, r in enumerate(ptrs):
                o.p[j] = A(r)
            for j, v in enumerate(flts):
                o.f[j] = float(v)
    return arr


def _aligned(nfloats: int) -> int:
    return nfloats + (-nfloats) % prg.ALIGN


def fuse_step(ops: Sequence, chunk: int, chain: bool, cln_step: bool,
              plan_chain: Callable[[int, int], Optional[Tuple[Sequence[int], int, int]]]) -> List[Tuple[object, int, int]]:
    """The launches of a whole streaming step: ``[(op, first, count)]``, every entry standing for ``ops[first:first + count]``
    (an op passed through: itself, count 1).
      * ``chain``: runs of consecutive small-tile convolutions that give every utterance ONE tile (the S-TCN of a
        frame-synchronous step) become one ConvChainOp (eab_conv_st_chain_run, csrc/conv_st.hip: one workgroup per utterance
        walks the run's descriptors).  ``plan_chain(first, count)`` says whether the chain kernel carries that run as a whole:
        (kernel code per op, LDS bytes, bf16?) or None.  Every candidate is asked on its own first, then the maximal runs of at
        least two accepted ops of one precision.  The tables go to the 'chain' arena, in the order of chain_tables.
      * ``cln_step``, one frame per step: the statistics / scan / apply launches of a cLN unit (eab_cln_stats_f32 = two
        launches, then eab_cln_apply_f32) become one ClnStepOp (eab_cln_step_f32: one workgroup per utterance sums the new
        frame, advances the running sums and normalises the frame -- the same code paths, so the same bits).
    An offline program (chunk 0) is passed through."""
    n = len(ops)
    single = [plan_chain(k, 1) if chain and chunk and op.kind == prg.OP_CONV and op.korder == prg.KORDER_FRAG else None
              for k, op in enumerate(ops)]

    def cln_pair(k: int) -> bool:
        a, b = ops[k], ops[k + 1] if k + 1 < n else None
        return (cln_step and chunk == 1 and b is not None and a.kind == prg.OP_CLN_STATS and b.kind == prg.OP_CLN_APPLY
                and a.x == b.x and a.mr == b.mr and (a.B, a.T, a.P, a.C) == (b.B, b.T, b.P, b.C) and a.win and b.win
                and a.state is not None)
    fused, k, table = [], 0, 0                  # table: floats of the 'chain' arena handed out
    while k < n:
        j = k
        while j < n and single[j] is not None and single[j][2] == single[k][2]:
            j += 1
        got = plan_chain(k, j - k) if j - k >= 2 else None
        if got:
            codes, lds, bf16 = got
            descs = table
            table += _aligned((j - k) * C.sizeof(_lib.ConvDesc) // 4)
            op = prg.ConvChainOp(descs=prg.Ref("chain", descs), codes=prg.Ref("chain", table), n=j - k, B=ops[k].B,
                                 lds_bytes=lds, bf16=bf16, plan=tuple(codes), name=f"chain[{ops[k].name}..{ops[j - 1].name}]")
            table += _aligned(j - k)
            fused.append((op, k, j - k))
        elif cln_pair(k):
            a, b = ops[k], ops[k + 1]
            op = prg.ClnStepOp(x=a.x, stat_slope=a.slope, sums=a.sums, state=a.state, mr=a.mr, gain=b.gain, bias=b.bias,
                               slope=b.slope, add=b.add, out=b.out, B=b.B, T=b.T, P=b.P, C=b.C, mode=b.mode, eps=a.eps,
                               name=b.name + "_step")
            fused.append((op, k, 2))
            j = k + 2
        else:                                   # (a run the planner refuses as a whole stays separate launches)
            j = max(j, k + 1)
            fused += [(ops[t], t, 1) for t in range(k, j)]
        k = j
    return fused


def chain_planner(arr) -> Callable:
    """fuse_step's ``plan_chain`` for the encoded array ``arr`` of the same ops: the library's host-side planner
    (eab_conv_st_chain_plan) on the encoded descriptors; it needs no device."""
    lib = _lib.load()

    def plan(first: int, count: int):
        descs = (_lib.ConvDesc * count)(*[arr[first + t].conv for t in range(count)])
        codes = (C.c_int * count)()
        lds, bf16 = C.c_int(0), C.c_int(0)
        if lib.eab_conv_st_chain_plan(descs, count, codes, C.byref(lds), C.byref(bf16)) != 0:
            return None
        return list(codes), lds.value, bf16.value
    return plan


def chain_tables(arr, fused: Sequence) -> bytes:
    """The 'chain' arena of a fused list: per ConvChainOp the encoded ``conv`` members of ``arr`` (the per-op array of the
    same binding) for its range, then its kernel codes, each at the Ref the op carries.  Empty without a chain."""
    buf = bytearray()
    for op, first, count in fused:
        if op.kind == prg.OP_CONV_CHAIN:
            buf += bytes(4 * op.descs.off - len(buf)) + b"".join(bytes(arr[first + t].conv) for t in range(count))
            buf += bytes(4 * op.codes.off - len(buf)) + bytes((C.c_int * count)(*op.plan))
    return bytes(buf)


def graph_branches_allowed() -> bool:
    """Parallel branches (side streams) for programs that mark independent chains?  EAB_GRAPH_BRANCHES=0 runs every program
    on one stream.  (Rounds 1-3 also switched them off while a torch.distributed process group was alive: a hipGraph with
    internal branches could crash the HIP runtime at replay.  The cause is an unchecked index in the runtime's stream
    assignment, graphs.py; since branches replay as separate single-stream graphs the condition no longer exists.)"""
    return os.environ.get("EAB_GRAPH_BRANCHES", "1") != "0"


class BoundProgram:
    """A lowered program on one device: its arenas, one encoded ``eab_op`` array per op list (``lists``: name -> ops, with
    the stream lane of every op and the fork / join points per name), their capture and their direct launches.  A subclass
    names the boundary buffers in ``bind`` order (BOUNDARY)."""
    BOUNDARY: tuple = ()

    def __init__(self, device: torch.device, arenas: Dict[str, torch.Tensor], lists: Dict[str, list],
                 lanes: Dict[str, list], sync: Dict[str, dict]):
        self.device, self.arenas = device, arenas
        self.lists, self.lanes, self.sync = lists, lanes, sync
        self.arrays = {name: (_lib.Op * len(ops))() for name, ops in lists.items()}
        self.window: dict = {}              # encode()'s t_pos / chunk / lens
        self._ptrs = None                   # boundary pointers the arrays are encoded for
        self.graphs: Optional[Dict[str, LaneGraphs]] = None      # name -> captured lane graphs
        self.graph_failed = False
        self.static: Dict[str, torch.Tensor] = {}               # boundary name -> static buffer of the captured form
        self._direct: Dict[str, LaneGraphs] = {}                # name -> LaneGraphs for direct (uncaptured) multi-lane runs

    def bind(self, *ptrs) -> bool:
        """Encode every op list for the boundary pointers ``ptrs`` (BOUNDARY order; missing trailing ones are None).
        Returns False if they are bound already."""
        ptrs += (None,) * (len(self.BOUNDARY) - len(ptrs))
        if ptrs == self._ptrs:
            return False
        self._ptrs = ptrs
        bases = self.bases()
        for name, ops in self.lists.items():
            encode(ops, bases, out=self.arrays[name], **self.window)
        return True

    def bases(self) -> Dict[str, Optional[int]]:
        """arena name -> base address for the current binding (encode's ``bases``)"""
        assert self._ptrs is not None, "bind the program first"
        bases = {k: t.data_ptr() for k, t in self.arenas.items()}
        bases.update(zip(self.BOUNDARY, self._ptrs))
        return bases

    def capture(self, *shapes) -> bool:
        """Capture every op list on static boundary buffers of ``shapes`` (BOUNDARY order; None = no such buffer): one
        single-stream hipGraph per lane segment (graphs.py: a hipGraph with internal branches can crash the HIP runtime at
        replay), so a replay is one graph launch per segment instead of hundreds of host-side kernel launches.  Returns
        False (and stays on direct launches) if the runtime refuses the capture."""
        if self.graphs is not None or self.graph_failed:
            return self.graphs is not None
        try:
            self.static = {k: torch.zeros(s, dtype=torch.float32, device=self.device)
                           for k, s in zip(self.BOUNDARY, shapes) if s is not None}
            self.bind(*(self.static[k].data_ptr() if k in self.static else None for k in self.BOUNDARY))
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                 # warm-up outside the capture (program order on one stream)
                for name, ops in self.lists.items():
                    self._launch(name, side.cuda_stream, 0, len(ops))
            torch.cuda.current_stream().wait_stream(side)
            graphs = {name: LaneGraphs(self.device, self._plan(name), functools.partial(self._launch, name))
                      for name in self.lists}
            for lg in graphs.values():
                lg.capture()
            self.graphs = graphs
        except Exception as e:                            # noqa: BLE001 - any capture failure -> direct launches
            warnings.warn(f"eabnet_amd: hipGraph capture failed ({e!r}); using direct launches")
            self.graphs, self.graph_failed, self._ptrs = None, True, None
        return self.graphs is not None

    def _plan(self, name: str) -> list:
        n = len(self.lists[name])
        sync = self.sync.get(name)
        return plan_segments(n, self.lanes[name], sync) if sync and graph_branches_allowed() else single_lane(n)

    def _launch(self, name: str, stream: int, first: int, n: int) -> None:
        ops = C.cast(C.byref(self.arrays[name], first * C.sizeof(_lib.Op)), C.POINTER(_lib.Op))
        _lib.check(_lib.load().eab_run_program(ops, n, C.c_void_p(stream)), f"eab_run_program({name})")

    def run(self, name: str, stream: int, first: int = 0, count: Optional[int] = None) -> None:
        """Direct launches of ops [first, first + count) of op list ``name`` on ``stream`` (a raw hipStream_t).  A whole
        list with parallel branches forks onto side streams with events, exactly as its captured form replays."""
        if first == 0 and count is None and self.sync.get(name) and graph_branches_allowed():
            assert torch.cuda.current_stream().cuda_stream == stream, "multi-lane programs run on torch's current stream"
            if name not in self._direct:
                self._direct[name] = LaneGraphs(self.device, self._plan(name), functools.partial(self._launch, name))
            self._direct[name].run_direct()
            return
        self._launch(name, stream, first, len(self.lists[name]) - first if count is None else count)
