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
from typing import Dict, Mapping, Optional, Sequence

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
    prg.GagPackOp: (("B", "T", "F", prg.GAG_PRE_LD), ("inpt", "pre_x", "enc_in", "pre"), ()),
    prg.GagCrmOp: (("B", "T", "F", prg.GAG_PRE_LD, prg.GAG_LIN_LD, "act"), ("pre", "g", "r", "i", "pre_out", "planar"), ()),
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
            for j, r in enumerate(ptrs):
                o.p[j] = A(r)
            for j, v in enumerate(flts):
                o.f[j] = float(v)
    return arr


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
        bases = {k: t.data_ptr() for k, t in self.arenas.items()}
        bases.update(zip(self.BOUNDARY, ptrs))
        for name, ops in self.lists.items():
            encode(ops, bases, out=self.arrays[name], **self.window)
        self._ptrs = ptrs
        return True

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
