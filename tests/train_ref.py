"""float64 reference of ONE op of a training program (eabnet_amd/train.py, train_gag.py) with a derived error limit per
output element  (TEST INFRASTRUCTURE; numpy only).

accesses(op) lists every array the op names -- which p[] it reads, writes or accumulates into and their shapes from i[] --
from ONE table (FORMS), encoded from the op table of include/eabnet_hip.h ("op kinds of the training programs" and the
CLN / GAG rows) and the dispatch of csrc/program.hip.  The dry walk (tests/test_train_ref.py) and the lockstep walk on the
device (tests/test_train_walk_gpu.py) both use that table and nothing else.

    mode 'r'        read
         'w'        written (every element unless the reference says otherwise)
         'rw'       accumulated into (read, then written)
         'scratch'  written by the op for its own later launches; needs no earlier content.  The reduction scratch of the
                    norm backward must be ZERO on entry (EAB_NB_SUMS_ZEROED): it lies in the gradient arena
    dtype 'f32' | 'f64' (doubles: two arena words per element)
    declared aliases: acc_in == dx / dpre, aux == dst (convolutions, EPI_ADD), out == a (the "grad +=" add)

evaluate(op, fetch, dtype) returns per output an Out (conv_ref.Out: val, lim, must, may) and the number of PReLU-kink
elements (below).  dtype float64 is the reference; dtype float32 is the YARDSTICK of the statistical criterion: the same
code with every array and every operation in fp32 and every reduction summed sequentially (np.add.accumulate), never
pairwise -- contractions (WGRAD) as fp32 matrix products, like conv_ref.conv_f32.  Where the C ABI itself says a quantity
is a double (the frame sums and scans of the cLN ops), it stays a double in both modes.

LIMITS are derived, never measured.  u = 2^-24.
  * a sum of n terms in any order (sequential, blocked, atomics):  (n + c) u sum |term|, c = the other roundings on the path
  * an elementwise chain:  c u times the magnitudes it passes through (an fma counts as one rounding but is not assumed)
  * sigmoid / tanh:  relative (|g| + 6) 2^-23, conv_ref's allowance for the device's exp and reciprocal
  * quantities fed by an earlier reduction are propagated to first order: mean -> variance -> rstd -> (scale, shift) of the
    statistics ops;  A / P and Q / P of the norm backward into dx;  the row sums of the cLN backward through its reverse
    scan (A_t, Bq_t: doubles on the device, so their own error is the fp32 rounding of the stored pair) into dx
  * accumulating outputs (dw, dbias, dgamma / dbeta / dslope, the COLSUM output, acc_in / EPI_ADD forms): + u |previous|
    and one rounding per partial added
  * the two LSTM recurrences keep the project's bar for exactly these kernels (LSTM_TOL = 1e-5, max-abs / max and L2, as
    tests/test_hip_train_ops.py): a derived bound through T matrix-core steps is not worth its length.

PReLU KINK.  Only NORM_BWD and CLN_BWD in mode EAB_XF_NORM_PRELU re-derive u = g xh + be in fp32 and branch on its sign;
every other kink is on a stored input and exact.  An element with |u_ref| <= KINK u (|g xh| + |be|) is AMBIGUOUS: its dx is
not compared, and what it could contribute to the sums it enters (A, Q, S of its (b, c) or row) under the other branch is
added to their limits (the branches differ by the factor |1 - a_c|).  KINK_CAP bounds the share of such elements over a
whole case; the band is never widened.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

import conv_ref as cr
from eabnet_amd import program as prg
from eabnet_amd import runtime
from eabnet_amd import train as tr

U = cr.U
KINK = 8.0
KINK_CAP = 1e-5
LSTM_TOL = 1e-5
SIG = 2.0 ** -23
D64 = 2.0 ** -50          # slack of a double evaluation, relative to the magnitudes summed
SECOND = 1 + 2.0 ** -10   # second-order terms of the first-order bounds (run_ref)


@dataclass
class Out(cr.Out):
    f64: bool = False      # doubles in the arena
    lstm: bool = False     # LSTM recurrence: LSTM_TOL instead of lim
    name: str = ""


# ----------------------------------------------------------------------------------------------------------------------
# the read / write table
# ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Arg:
    p: int
    name: str
    shape: Callable[[list], tuple]
    mode: str
    dtype: str = "f32"


@dataclass
class Access:
    name: str
    ref: prg.Ref
    shape: tuple
    mode: str
    dtype: str = "f32"
    sel: Optional[np.ndarray] = None        # bool over shape: the part a 'w' access writes (None = all of it)

    @property
    def words(self) -> int:
        return int(np.prod(self.shape)) * (2 if self.dtype == "f64" else 1)


def _n64(i, k=0):
    return (i[k] & 0xFFFFFFFF) | (i[k + 1] << 32)


def _flat(i):
    return (_n64(i),)


_BPC = lambda i: (i[0], i[1], i[2])                   # noqa: E731
_C = lambda i: (i[2],)                                # noqa: E731
_BC2 = lambda i: (i[0], i[2], 2)                      # noqa: E731
_BPX = lambda i: (i[0], i[1], i[4])                   # noqa: E731  (NORM_BWD multi: xC = i[4])
_BTP = lambda i: (i[0], i[1], i[2])                   # noqa: E731
_BT2 = lambda i: (i[0], i[1], 2)                      # noqa: E731
_C3 = lambda i: (i[3],)                               # noqa: E731
_BTF64 = lambda i: (i[0], i[1], i[2], 64)             # noqa: E731
_PLANAR = lambda i: (i[0], 2, i[1], i[2])             # noqa: E731
_PRE = lambda i: (i[0], i[1], i[3])                   # noqa: E731
_LIN = lambda i: (i[0], i[1], i[4])                   # noqa: E731

FORMS: Dict[str, List[Arg]] = {
    "IN_STATS": [Arg(0, "x", _BPC, "r"), Arg(1, "slope", _C, "r"), Arg(2, "gamma", _C, "r"), Arg(3, "beta", _C, "r"),
                 Arg(4, "xf", _BC2, "w"), Arg(5, "mr", _BC2, "w"), Arg(6, "y", _BPC, "w")],
    "IN_STATS_MULTI": [Arg(0, "x", lambda i: (i[0], i[1], i[3]), "r"), Arg(1, "slope", _C, "r"), Arg(2, "gamma", _C, "r"),
                       Arg(3, "beta", _C, "r"), Arg(4, "xf", _BC2, "w"), Arg(5, "mr", _BC2, "w"),
                       Arg(6, "y", lambda i: (i[2] // i[3], i[0], i[1], i[3]), "w")],
    "IN_FINALIZE": [Arg(0, "stats", lambda i: (i[0], i[3], i[2], i[1], 4), "r"),
                    Arg(1, "gamma0", lambda i: (i[1],), "r"), Arg(2, "beta0", lambda i: (i[1],), "r"),
                    Arg(3, "xf0", lambda i: (i[0], i[1], 2), "w"),
                    Arg(4, "gamma1", lambda i: (i[1],), "r"), Arg(5, "beta1", lambda i: (i[1],), "r"),
                    Arg(6, "xf1", lambda i: (i[0], i[1], 2), "w"),
                    Arg(7, "mr0", lambda i: (i[0], i[1], 2), "w"), Arg(8, "mr1", lambda i: (i[0], i[1], 2), "w")],
    "TR_NORM_ACT": [Arg(0, "x", _BPC, "r"), Arg(1, "xf", _BC2, "r"), Arg(2, "slope", _C, "r"), Arg(3, "add", _BPC, "r"),
                    Arg(4, "y", _BPC, "w")],
    "NORM_BWD": [Arg(0, "dy", _BPC, "r"), Arg(1, "x", _BPC, "r"), Arg(2, "mr", _BC2, "r"), Arg(3, "gamma", _C, "r"),
                 Arg(4, "beta", _C, "r"), Arg(5, "slope", _C, "r"),
                 Arg(6, "sums", lambda i: (tr.NB_SUM_COPIES, i[0], i[2], 4), "scratch"), Arg(7, "acc_in", _BPC, "r"),
                 Arg(8, "dx", _BPC, "w"), Arg(9, "dgamma", _C, "rw"), Arg(10, "dbeta", _C, "rw"), Arg(11, "dslope", _C, "rw")],
    "NORM_BWD_MULTI": [Arg(0, "dy", _BPX, "r"), Arg(1, "x", _BPX, "r"), Arg(2, "mr", _BC2, "r"), Arg(3, "gamma", _C, "r"),
                       Arg(4, "dy1", _BPX, "r"), Arg(5, "slope", _C, "r"),
                       Arg(6, "sums", lambda i: (tr.NB_SUM_COPIES, i[0], i[2], 4), "scratch"), Arg(7, "acc_in", _BPX, "r"),
                       Arg(8, "dx", _BPX, "w"), Arg(9, "dgamma", _C, "rw"), Arg(10, "dbeta", _C, "rw"),
                       Arg(11, "dslope", _C, "rw")],
    "GLU_BWD": [Arg(0, "dy", lambda i: (_n64(i), i[2] // 2), "r"), Arg(1, "dump", lambda i: (_n64(i), i[2]), "r"),
                Arg(2, "dz", lambda i: (_n64(i), i[2]), "w")],
    "GATE_FWD": [Arg(0, "a", _flat, "r"), Arg(1, "r", _flat, "r"), Arg(2, "z", _flat, "w")],
    "GATE_BWD": [Arg(0, "dz", _flat, "r"), Arg(1, "a", _flat, "r"), Arg(2, "r", _flat, "r"), Arg(3, "da", _flat, "w"),
                 Arg(4, "dr", _flat, "w")],
    "ADD": [Arg(0, "a", _flat, "r"), Arg(1, "b", _flat, "r"), Arg(2, "out", _flat, "w")],
    "RELU_BWD": [Arg(0, "dy", _flat, "r"), Arg(1, "y", _flat, "r"), Arg(2, "dx", _flat, "w")],
    "COLSUM": [Arg(0, "x", lambda i: (_n64(i), i[2]), "r"), Arg(1, "out", _C, "rw")],
    "FILTER_SUM": [Arg(0, "w", lambda i: (i[0], i[1], i[2], i[4]), "r"), Arg(1, "x", lambda i: (i[0], i[1], i[2], i[3], 2), "r"),
                   Arg(2, "y", _PLANAR, "w")],
    "FS_BWD": [Arg(0, "dout", _PLANAR, "r"), Arg(1, "x", lambda i: (i[0], i[1], i[2], i[3], 2), "r"),
               Arg(2, "dw", lambda i: (i[0], i[1], i[2], i[4]), "w")],
    "LN_FWD": [Arg(0, "x", lambda i: (_n64(i), 64), "r"), Arg(1, "g", lambda i: (64,), "r"), Arg(2, "b", lambda i: (64,), "r"),
               Arg(3, "y", lambda i: (_n64(i), 64), "w"), Arg(4, "mr", lambda i: (_n64(i), 2), "w")],
    "LN_BWD": [Arg(0, "dy", lambda i: (_n64(i), 64), "r"), Arg(1, "x", lambda i: (_n64(i), 64), "r"),
               Arg(2, "mr", lambda i: (_n64(i), 2), "r"), Arg(3, "g", lambda i: (64,), "r"),
               Arg(4, "dx", lambda i: (_n64(i), 64), "w"), Arg(5, "dg", lambda i: (64,), "rw"), Arg(6, "db", lambda i: (64,), "rw")],
    "LSTM_TRAIN": [Arg(0, "x", _BTF64, "r"), Arg(1, "wcat", lambda i: (256, 128), "r"), Arg(2, "bias", lambda i: (256,), "r"),
                   Arg(3, "h_out", _BTF64, "w"), Arg(4, "gates", lambda i: (i[0] * i[2], i[1], 5, 64), "w")],
    "LSTM_BWD": [Arg(0, "gates", lambda i: (i[0] * i[2], i[1], 5, 64), "r"), Arg(1, "dh_out", _BTF64, "r"),
                 Arg(2, "wcat", lambda i: (256, 128), "r"), Arg(3, "dgates", lambda i: (i[0], i[1], i[2], 256), "w")],
    "CLN_STATS": [Arg(0, "x", _BTP, "r"), Arg(1, "slope", _C3, "r"), Arg(2, "sums", _BT2, "w", "f64"),
                  Arg(3, "state", lambda i: (3 * i[0],), "rw", "f64"), Arg(4, "mr", _BT2, "w")],
    "CLN_APPLY": [Arg(0, "x", _BTP, "r"), Arg(1, "mr", _BT2, "r"), Arg(2, "gain", _C3, "r"), Arg(3, "bias", _C3, "r"),
                  Arg(4, "slope", _C3, "r"), Arg(5, "add", _BTP, "r"), Arg(6, "y", _BTP, "w")],
    "CLN_BWD": [Arg(0, "dy", _BTP, "r"), Arg(1, "x", _BTP, "r"), Arg(2, "mr", _BT2, "r"), Arg(3, "gain", _C3, "r"),
                Arg(4, "bias", _C3, "r"), Arg(5, "slope", _C3, "r"), Arg(6, "rowsums", _BT2, "scratch", "f64"),
                Arg(7, "ab", _BT2, "scratch"), Arg(8, "part", lambda i: (i[0] * i[1], 3, i[3]), "w"),
                Arg(9, "acc_in", _BTP, "r"), Arg(10, "dx", _BTP, "w")],
    "GAG_PACK": [Arg(0, "inpt", _PLANAR, "r"), Arg(1, "pre_x", _PLANAR, "r"), Arg(2, "enc_in", lambda i: (i[0], i[1], i[2], 4), "w"),
                 Arg(3, "pre", _PRE, "w")],
    "GAG_CRM": [Arg(0, "pre", _PRE, "r"), Arg(1, "g", _LIN, "r"), Arg(2, "r", _LIN, "r"), Arg(3, "i", _LIN, "r"),
                Arg(4, "pre_out", _PRE, "w"), Arg(5, "planar", _PLANAR, "w")],
    "GAG_CRM_BWD": [Arg(0, "pre", _PRE, "r"), Arg(1, "g", _LIN, "r"), Arg(2, "dplanar", _PLANAR, "r"), Arg(3, "dpre_out", _PRE, "r"),
                    Arg(4, "acc_in", _PRE, "r"), Arg(5, "dg", _LIN, "w"), Arg(6, "dr", _LIN, "w"), Arg(7, "di", _LIN, "w"),
                    Arg(8, "dpre", _PRE, "w")],
    "MEMSET0": [Arg(0, "ptr", lambda i: (_n64(i) // 4,), "w")],
}
ALIASES = {("dx", "acc_in"), ("dpre", "acc_in"), ("dst", "aux"), ("out", "a")}

_KIND_FORM = {prg.OP_IN_FINALIZE: "IN_FINALIZE", tr.OP_TR_NORM_ACT: "TR_NORM_ACT", tr.OP_GLU_BWD: "GLU_BWD",
              tr.OP_GATE_FWD: "GATE_FWD", tr.OP_GATE_BWD: "GATE_BWD", tr.OP_ADD: "ADD", tr.OP_RELU_BWD: "RELU_BWD",
              tr.OP_COLSUM: "COLSUM", tr.OP_FILTER_SUM: "FILTER_SUM", tr.OP_FS_BWD: "FS_BWD", tr.OP_LN_FWD: "LN_FWD",
              tr.OP_LN_BWD: "LN_BWD", tr.OP_LSTM_TRAIN: "LSTM_TRAIN", tr.OP_LSTM_BWD: "LSTM_BWD",
              prg.OP_CLN_STATS: "CLN_STATS", prg.OP_CLN_APPLY: "CLN_APPLY", tr.OP_CLN_BWD: "CLN_BWD",
              prg.OP_GAG_PACK: "GAG_PACK", prg.OP_GAG_CRM: "GAG_CRM", prg.OP_GAG_CRM_BWD: "GAG_CRM_BWD",
              prg.OP_MEMSET0: "MEMSET0"}


def fields(op) -> Tuple[list, list, list]:
    """(i, p, f) of eab_op as runtime.encode fills them (i padded with zeros, p with None)"""
    layout = runtime._LAYOUT.get(type(op))
    if layout is None:
        ints, ptrs, flts = list(op.i), list(op.p), list(op.f)
    else:
        ints = [a if a is None or isinstance(a, int) else getattr(op, a) for a in layout[0]]
        ptrs = [getattr(op, a) for a in layout[1]]
        flts = [getattr(op, a) for a in layout[2]]
        if op.kind == prg.OP_MEMSET0:
            ints[0:2] = [(4 * op.nfloats) & 0xFFFFFFFF, (4 * op.nfloats) >> 32]
    return [int(v) for v in ints] + [0] * (8 - len(ints)), ptrs + [None] * (12 - len(ptrs)), [float(v) for v in flts] + [0.0] * 4


def form_of(op) -> str:
    """which row of FORMS describes the op (the dispatch of eab_run_program)"""
    if op.kind == tr.OP_IN_STATS:
        i, p, _ = fields(op)
        return "IN_STATS_MULTI" if p[6] is not None and i[3] > 0 else "IN_STATS"
    if op.kind == tr.OP_NORM_BWD:
        return "NORM_BWD_MULTI" if fields(op)[0][4] > 0 else "NORM_BWD"
    return _KIND_FORM[op.kind]


def kind_name(op) -> str:
    if op.kind == prg.OP_CONV:
        return "CONV"
    if op.kind == tr.OP_WGRAD:
        return "WGRAD"
    return form_of(op)


def _conv_sel(op: prg.ConvOp, field: str, shape: tuple) -> Optional[np.ndarray]:
    """the part of dst / dst_acc / glu_dump (output columns of the phase) and of the partials (its own tiles) a launch writes"""
    if field in ("dst", "dst_acc", "glu_dump"):
        sel = np.zeros(shape, bool)
        sel[:, :, np.arange(op.No) * op.ostride + op.ophase] = True
        if op.ph1_No > 0:
            sel[:, :, np.arange(op.ph1_No) * op.ostride + op.ph1_ophase] = True
        if op.epi == prg.EPI_PHASE2:
            sel[:] = True
        return sel
    if field == "stats":
        sel = np.zeros(shape, bool)
        sel[:, op.stat_tile0:op.stat_tile0 + cr.launch_tiles(op)] = True
        return sel
    return None


def accesses(op) -> List[Access]:
    if op.kind == prg.OP_CONV:
        out = []
        for field, ref, shape, _, mode in cr.regions(op):
            sel = _conv_sel(op, field, shape) if mode != "r" else None
            # the partials of a norm are written tile by tile by the launches that feed it; nothing of them is read
            out.append(Access(field, ref, tuple(shape), "w" if field == "stats" else mode, "f32", sel))
        return out
    if op.kind == tr.OP_WGRAD:
        assert op.precision == prg.PREC_F32 and not op.bf16_mask, "bf16 training programs are not part of this reference"
        out = [Access("dz", op.dz, (op.B, op.T, op.Fz, op.N), "r"), Access("src0", op.src0, (op.B, op.T, op.Fin, op.C0), "r")]
        if op.src1 is not None:
            out.append(Access("src1", op.src1, (op.B, op.T, op.Fin, op.C1), "r"))
        out.append(Access("dw", op.dw, (op.N, op.Kpad), "rw"))
        if op.dbias is not None:
            out.append(Access("dbias", op.dbias, (op.N,), "rw"))
        return out
    i, p, _ = fields(op)
    form = FORMS[form_of(op)]
    assert all(p[k] is None for k in range(12) if k not in {a.p for a in form}), f"{op.name}: a pointer the table does not know"
    return [Access(a.name, p[a.p], tuple(int(v) for v in a.shape(i)), a.mode, a.dtype) for a in form if p[a.p] is not None]


# ----------------------------------------------------------------------------------------------------------------------
# arithmetic in the reference's or the yardstick's number format
# ----------------------------------------------------------------------------------------------------------------------
class _M:
    def __init__(self, dt):
        self.dt = np.dtype(dt)
        self.seq = self.dt == np.float32

    def __call__(self, x):
        return None if x is None else np.asarray(x).astype(self.dt)

    def sum(self, x, axis):
        if not self.seq:
            return x.sum(axis)
        axes = tuple(a % x.ndim for a in ((axis,) if isinstance(axis, int) else axis))
        keep = [a for a in range(x.ndim) if a not in axes]
        y = np.transpose(x, keep + list(axes)).reshape([x.shape[a] for a in keep] + [-1])
        return np.add.accumulate(y, axis=-1, dtype=np.float32)[..., -1]


def _L(x):
    return np.asarray(x, np.float64)


def _ab(x):
    return np.abs(np.asarray(x, np.float64))


def _prelu(x, a):
    return np.where(x > 0, x, a * x)


def _sig(x):
    return 1 / (1 + np.exp(-x))


def _rstd_lim(rstd, ev):
    """limit of (var + eps)^-1/2 given the limit ev of var (first order, with the second-order term) and its own roundings"""
    r = _ab(rstd)
    return 0.5 * r ** 3 * ev * (1 + 3 * ev * r * r) + 3 * U * r


# ----------------------------------------------------------------------------------------------------------------------
# the references: fn(i, f, A, m) -> {output: (val, lim) or (val, lim, must)}, number of ambiguous elements
# ----------------------------------------------------------------------------------------------------------------------
def _moments(v, P, eps, m):
    """mean, rstd over axis 1 of v (B, P, C) and their limits: two-pass formulas"""
    mean = m.sum(v, 1) / P
    d = v - mean[:, None]
    var = m.sum(d * d, 1) / P
    rstd = 1 / np.sqrt(var + eps)
    em = (P + 2) * U * _ab(v).sum(1) / P                                 # (one rounding for a PReLU product in front)
    ed = em[:, None] + U * (_ab(v) + _ab(d))
    ev = (P + 4) * U * _L(var) + (2 * _ab(d) * ed + ed * ed).sum(1) / P
    return mean, rstd, em, _rstd_lim(rstd, ev)


def ref_in_stats(i, f, A, m, multi=False):
    B, P, C = i[0], i[1], i[2]
    xC = i[3] if multi else C
    nv = C // xC
    x = m(A["x"]).reshape(B, P, xC)
    xx = np.concatenate([x] * nv, -1)                                    # channel c reads input channel c % xC
    a = m(A.get("slope"))
    v = xx if a is None else _prelu(xx, a)
    gamma, beta = m(A["gamma"]), m(A["beta"])
    mean, rstd, em, er = _moments(v, P, f[0], m)
    scale = gamma * rstd
    shift = beta - mean * scale
    es = _ab(gamma) * er + U * _ab(scale)
    eh = em * _ab(scale) + _ab(mean) * es + em * es + 2 * U * (_ab(beta) + _ab(mean * scale))
    out = {"xf": (np.stack([scale, shift], -1), np.stack([es + U * _ab(scale), eh + U * _ab(shift)], -1)),
           "mr": (np.stack([mean, rstd], -1), np.stack([em + U * _ab(mean), er], -1))}
    if "y" in A:
        y = v * scale[:, None] + shift[:, None]
        ey = _ab(v) * es[:, None] + eh[:, None] + 3 * U * (_ab(v * scale[:, None]) + _ab(shift)[:, None])
        if multi:                                                        # view v: its own contiguous [B][P][xC] tensor
            y, ey = (t.reshape(B, P, nv, xC).transpose(2, 0, 1, 3) for t in (y, ey))
        out["y"] = (y, ey)
    return out, 0


def ref_in_finalize(i, f, A, m):
    B, C, nsets, tiles = i[0], i[1], i[2], i[3]
    st = m(A["stats"])
    out = {}
    for s in range(nsets):
        n, mu, m2 = st[:, :, s, :, 0], st[:, :, s, :, 1], st[:, :, s, :, 2]
        N = m.sum(n, 1)
        assert np.all(_L(N) == i[4]), "the partial counts do not add up to the op's count"
        mean = m.sum(n * mu, 1) / N
        d = mu - mean[:, None]
        M2 = m.sum(m2, 1) + m.sum(n * d * d, 1)
        var = M2 / N
        rstd = 1 / np.sqrt(var + f[0])
        em = (tiles + 2) * U * _ab(n * mu).sum(1) / _L(N)
        ed = em[:, None] + U * _ab(d)
        ev = (2 * tiles + 5) * U * _L(var) + (_L(n) * (2 * _ab(d) * ed + ed * ed)).sum(1) / _L(N)
        er = _rstd_lim(rstd, ev)
        gamma, beta = m(A[f"gamma{s}"]), m(A[f"beta{s}"])
        scale = gamma * rstd
        shift = beta - mean * scale
        es = _ab(gamma) * er + 2 * U * _ab(scale)
        eh = em * _ab(scale) + _ab(mean) * es + em * es + 2 * U * (_ab(beta) + _ab(mean * scale))
        out[f"xf{s}"] = (np.stack([scale, shift], -1), np.stack([es, eh + U * _ab(shift)], -1))
        if f"mr{s}" in A:
            out[f"mr{s}"] = (np.stack([mean, rstd], -1), np.stack([em + U * _ab(mean), er], -1))
    return out, 0


def ref_tr_norm_act(i, f, A, m):
    mode = i[3]
    x, a = m(A["x"]), m(A["slope"])
    if A.get("xf") is None:
        assert mode == prg.XF_NORM_PRELU
        y = _prelu(x, a)
        lim = U * _ab(y)
    else:
        xf = m(A["xf"])
        s, h = xf[:, None, :, 0], xf[:, None, :, 1]
        if mode == prg.XF_NORM_PRELU:
            t = x * s + h
            y = _prelu(t, a)
            lim = np.maximum(1.0, _ab(a)) * 2 * U * (_ab(x * s) + _ab(h)) + U * _ab(y)
        else:
            q = _prelu(x, a)
            y = q * s + h
            lim = 3 * U * _ab(q * s) + 2 * U * _ab(h)
    if A.get("add") is not None:
        y = y + m(A["add"])
        lim = lim + U * _ab(y)
    return {"y": (y, lim)}, 0


def _norm_bwd_view(dy, x, mr, g, be, a, mode, P, m):
    """input gradient of one norm unit without the accumulate operand, its parameter sums per (b, c), and their limits.
    mr None: no norm in front of the PReLU (NORM_PRELU order only)."""
    one = np.ones((), m.dt)
    amb = np.zeros(x.shape, bool)
    if mode == prg.XF_NORM_PRELU:
        if mr is None:
            uu, xh = x, x
            mag = _ab(x)
        else:
            mean, rstd = mr[:, None, :, 0], mr[:, None, :, 1]
            xh = (x - mean) * rstd
            uu = g * xh + be
            mag = _ab(g * xh) + _ab(be)
            amb = _ab(uu) <= KINK * U * mag
        pos = uu > 0
        du = np.where(pos, dy, a * dy)
        flip = np.where(amb, np.abs(1 - _L(a)) * _ab(dy), 0.0)            # what the other branch would change of du
        A_ = m.sum(du, 1)
        S_ = m.sum(np.where(pos, 0 * one, dy * uu), 1)
        LA = (P + 1) * U * _ab(du).sum(1) + flip.sum(1)
        LS = (P + 5) * U * np.where(pos & ~amb, 0.0, _ab(dy) * mag).sum(1) + np.where(amb, _ab(dy * uu), 0.0).sum(1)
        if mr is None:
            return dict(dx=du, Ldx=U * _ab(du), A=None, Q=None, S=S_, LS=LS, amb=amb)
        Q_ = m.sum(du * xh, 1)
        LQ = (P + 4) * U * _ab(du * xh).sum(1) + (flip * _ab(xh)).sum(1)
        k = rstd * g
        Am, Qm = A_[:, None] / P, Q_[:, None] / P
        dx = k * (du - Am - xh * Qm)
        Ldx = _ab(k) * (LA[:, None] / P + _ab(xh) * LQ[:, None] / P + 8 * U * (_ab(du) + _ab(Am) + _ab(xh * Qm)))
        return dict(dx=dx, Ldx=Ldx, A=A_, Q=Q_, S=S_, LA=LA, LQ=LQ, LS=LS, amb=amb)
    mean, rstd = mr[:, None, :, 0], mr[:, None, :, 1]
    p = _prelu(x, a)
    xh = (p - mean) * rstd
    exh = 2 * U * _ab(xh) + U * _ab(p * rstd)
    A_ = m.sum(dy, 1)
    Q_ = m.sum(dy * xh, 1)
    LA = (P + 1) * U * _ab(dy).sum(1)
    LQ = (P + 2) * U * _ab(dy * xh).sum(1) + (_ab(dy) * exh).sum(1)
    k = rstd * g
    Am, Qm = A_[:, None] / P, Q_[:, None] / P
    dp = k * (dy - Am - xh * Qm)
    Ldp = _ab(k) * (LA[:, None] / P + _ab(xh) * LQ[:, None] / P + exh * _ab(Qm) + 8 * U * (_ab(dy) + _ab(Am) + _ab(xh * Qm)))
    pos = x > 0
    dx = np.where(pos, dp, a * dp)
    Ldx = np.maximum(1.0, _ab(a)) * Ldp + U * _ab(dx)
    S_ = m.sum(np.where(pos, 0 * one, dp * x), 1)
    LS = np.where(pos, 0.0, _ab(x) * Ldp).sum(1) + (P + 2) * U * np.where(pos, 0.0, _ab(dp * x)).sum(1)
    return dict(dx=dx, Ldx=Ldx, A=A_, Q=Q_, S=S_, LA=LA, LQ=LQ, LS=LS, amb=amb)


def _param_acc(prev, per_b, lim_b, m):
    """prev[c] += sum_b per_b[b][c]: B partials added one by one (atomics)"""
    B = per_b.shape[0]
    val = prev + m.sum(per_b, 0)
    return val, lim_b.sum(0) + (B + 1) * U * (_ab(prev) + _ab(per_b).sum(0))


def ref_norm_bwd(i, f, A, m):
    B, P, C, mode = i[0], i[1], i[2], i[3] & 0xFF
    assert not i[3] & tr.STORE_BF16, "bf16 storage is not part of this reference"
    dy, x, a = m(A["dy"]), m(A["x"]), m(A["slope"])
    mr = m(A.get("mr"))
    r = _norm_bwd_view(dy, x, mr, m(A.get("gamma")), m(A.get("beta")), a, mode, P, m)
    dx, Ldx = r["dx"], r["Ldx"]
    if A.get("acc_in") is not None:
        dx = dx + m(A["acc_in"])
        Ldx = Ldx + U * _ab(dx)
    out = {"dx": (dx, Ldx, ~r["amb"]), "dslope": _param_acc(m(A["dslope"]), r["S"], r["LS"], m)}
    if mr is not None:
        out["dgamma"] = _param_acc(m(A["dgamma"]), r["Q"], r["LQ"], m)
        out["dbeta"] = _param_acc(m(A["dbeta"]), r["A"], r["LA"], m)
    return out, int(r["amb"].sum())


def ref_norm_bwd_multi(i, f, A, m):
    B, P, C, xC = i[0], i[1], i[2], i[4]
    assert C == 2 * xC and i[3] & 0xFF == prg.XF_PRELU_NORM
    x, mr, g, a = m(A["x"]), m(A["mr"]), m(A["gamma"]), m(A["slope"])
    views = [_norm_bwd_view(m(A[n]), x, mr[:, v * xC:(v + 1) * xC], g[v * xC:(v + 1) * xC], None, a[v * xC:(v + 1) * xC],
                            prg.XF_PRELU_NORM, P, m) for v, n in enumerate(("dy", "dy1"))]
    dx = views[0]["dx"] + views[1]["dx"]
    Ldx = views[0]["Ldx"] + views[1]["Ldx"] + U * _ab(dx)
    if A.get("acc_in") is not None:
        dx = dx + m(A["acc_in"])
        Ldx = Ldx + U * _ab(dx)
    cat = lambda key: np.concatenate([views[0][key], views[1][key]], -1)          # noqa: E731  view-major [2 xC]
    return {"dx": (dx, Ldx), "dgamma": _param_acc(m(A["dgamma"]), cat("Q"), cat("LQ"), m),
            "dbeta": _param_acc(m(A["dbeta"]), cat("A"), cat("LA"), m),
            "dslope": _param_acc(m(A["dslope"]), cat("S"), cat("LS"), m)}, 0


def ref_glu_bwd(i, f, A, m):
    N = i[2]
    assert not i[3], "bf16 storage is not part of this reference"
    dy, dump = m(A["dy"]), m(A["dump"])
    r = np.arange(N)
    half, ch = (r % 64) // 32, (r // 64) * 32 + r % 32
    mate = np.where(half == 1, r - 32, r + 32)
    d, me, ot = dy[:, ch], dump, dump[:, mate]
    val = np.where(half == 1, d * ot * me * (1 - me), d * ot)
    lim = np.where(half == 1, 3 * U * _ab(val) + U * _ab(d * ot * me), U * _ab(val))
    return {"dz": (val, lim)}, 0


def ref_gate_fwd(i, f, A, m):
    a, r = m(A["a"]), m(A["r"])
    z = a * _sig(r)
    return {"z": (z, _ab(z) * ((_ab(r) + 6) * SIG + 2 * U))}, 0


def ref_gate_bwd(i, f, A, m):
    dz, a, r = m(A["dz"]), m(A["a"]), m(A["r"])
    s = _sig(r)
    es = (_ab(r) + 6) * SIG                                              # relative error of the device's sigmoid
    da, dr = dz * s, dz * a * s * (1 - s)
    Ldr = _ab(dz * a) * (np.abs(1 - 2 * _L(s)) * _L(s) * es + U * _L(s)) + 3 * U * _ab(dr)
    return {"da": (da, _ab(da) * (es + 2 * U)), "dr": (dr, Ldr)}, 0


def ref_add(i, f, A, m):
    v = m(A["a"]) + m(A["b"])
    return {"out": (v, U * _ab(v))}, 0


def ref_relu_bwd(i, f, A, m):
    v = np.where(m(A["y"]) > 0, m(A["dy"]), np.zeros((), m.dt))
    return {"dx": (v, np.zeros(v.shape))}, 0


def ref_colsum(i, f, A, m):
    x, prev = m(A["x"]), m(A["out"])
    return {"out": (prev + m.sum(x, 0), (x.shape[0] + 2) * U * (_ab(x).sum(0) + _ab(prev)))}, 0


def ref_filter_sum(i, f, A, m):
    M = i[3]
    w = m(A["w"])[..., :2 * M].reshape(A["w"].shape[:3] + (M, 2))
    x = m(A["x"])
    t = [w[..., 0] * x[..., 0], -w[..., 1] * x[..., 1], w[..., 0] * x[..., 1], w[..., 1] * x[..., 0]]
    yr, yi = m.sum(t[0] + t[1], -1), m.sum(t[2] + t[3], -1)
    lr, li = ((2 * M + 2) * U * (_ab(p) + _ab(q)).sum(-1) for p, q in ((t[0], t[1]), (t[2], t[3])))
    return {"y": (np.stack([yr, yi], 1), np.stack([lr, li], 1))}, 0


def ref_fs_bwd(i, f, A, m):
    B, T, F, M, ld = i[:5]
    d, x = m(A["dout"]), m(A["x"])
    dr, di = d[:, 0][..., None], d[:, 1][..., None]
    val, lim = np.zeros((B, T, F, ld), m.dt), np.zeros((B, T, F, ld))
    val[..., 0:2 * M:2] = dr * x[..., 0] + di * x[..., 1]
    val[..., 1:2 * M:2] = di * x[..., 0] - dr * x[..., 1]
    lim[..., 0:2 * M:2] = 3 * U * (_ab(dr * x[..., 0]) + _ab(di * x[..., 1]))
    lim[..., 1:2 * M:2] = 3 * U * (_ab(di * x[..., 0]) + _ab(dr * x[..., 1]))
    return {"dw": (val, lim)}, 0


def ref_ln_fwd(i, f, A, m):
    x, g, b = m(A["x"]), m(A["g"]), m(A["b"])
    mean = m.sum(x, 1) / 64
    d = x - mean[:, None]
    var = m.sum(d * d, 1) / 64
    rstd = 1 / np.sqrt(var + f[0])
    em = (64 + 2) * U * _ab(x).sum(1) / 64
    ed = em[:, None] + U * _ab(d)
    ev = (64 + 4) * U * _L(var) + (2 * _ab(d) * ed + ed * ed).sum(1) / 64
    er = _rstd_lim(rstd, ev)
    y = d * rstd[:, None] * g + b
    ey = (ed * _ab(rstd)[:, None] + _ab(d) * er[:, None]) * _ab(g) + 4 * U * _ab(d * rstd[:, None] * g) + 2 * U * _ab(b)
    return {"y": (y, ey), "mr": (np.stack([mean, rstd], -1), np.stack([em + U * _ab(mean), er], -1))}, 0


def ref_ln_bwd(i, f, A, m):
    dy, x, mr, g = m(A["dy"]), m(A["x"]), m(A["mr"]), m(A["g"])
    rows = x.shape[0]
    mu, r = mr[:, 0:1], mr[:, 1:2]
    xh = (x - mu) * r
    dh = dy * g
    Am, Qm = m.sum(dh, 1)[:, None] / 64, m.sum(dh * xh, 1)[:, None] / 64
    dx = r * (dh - Am - xh * Qm)
    LA = (64 + 3) * U * _ab(dh).sum(1)[:, None] / 64
    LQ = (64 + 6) * U * _ab(dh * xh).sum(1)[:, None] / 64
    Ldx = _ab(r) * (LA + _ab(xh) * LQ + 8 * U * (_ab(dh) + _ab(Am) + _ab(xh * Qm)))
    dg0, db0 = m(A["dg"]), m(A["db"])
    dg, db = dg0 + m.sum(dy * xh, 0), db0 + m.sum(dy, 0)
    return {"dx": (dx, Ldx), "dg": (dg, (rows + 5) * U * (_ab(dy * xh).sum(0) + _ab(dg0))),
            "db": (db, (rows + 2) * U * (_ab(dy).sum(0) + _ab(db0)))}, 0


def ref_lstm_train(i, f, A, m):
    """nn.LSTM(64, 64) over time for the B*F sequences (sequence s = b*F + f): h_out [B][T][F][64] and the activated gates and
    cell state [B*F][T][5][64] = (i, f, g, o, c)"""
    B, T, F = i[0], i[1], i[2]
    assert i[3] == prg.PREC_F32
    x = m(A["x"]).transpose(0, 2, 1, 3).reshape(B * F, T, 64)
    W, bias = m(A["wcat"]), m(A["bias"])
    h, c = np.zeros((B * F, 64), m.dt), np.zeros((B * F, 64), m.dt)
    hs, gs = [], []
    for t in range(T):
        pre = np.concatenate([x[:, t], h], -1) @ W.T + bias
        ig, fg, gg, og = _sig(pre[:, :64]), _sig(pre[:, 64:128]), np.tanh(pre[:, 128:192]), _sig(pre[:, 192:])
        c = fg * c + ig * gg
        h = og * np.tanh(c)
        hs.append(h)
        gs.append(np.stack([ig, fg, gg, og, c], 1))
    h_out = np.stack(hs, 1).reshape(B, F, T, 64).transpose(0, 2, 1, 3)
    inf = lambda v: np.full(v.shape, np.inf)                                        # noqa: E731
    gates = np.stack(gs, 1)
    return {"h_out": (h_out, inf(h_out)), "gates": (gates, inf(gates))}, 0


def ref_lstm_bwd(i, f, A, m):
    """reverse-time pass on the stored gates: dgates [B][T][F][256], row g*64+u in the order (i, f, g, o)"""
    B, T, F = i[0], i[1], i[2]
    assert i[3] == prg.PREC_F32
    gk = m(A["gates"])
    dh = m(A["dh_out"]).transpose(0, 2, 1, 3).reshape(B * F, T, 64)
    Whh = m(A["wcat"])[:, 64:]
    dhr, dcc = np.zeros((B * F, 64), m.dt), np.zeros((B * F, 64), m.dt)
    want = np.zeros((B * F, T, 256), m.dt)
    for t in range(T - 1, -1, -1):
        ig, fg, gg, og, c = (gk[:, t, k] for k in range(5))
        cp = gk[:, t - 1, 4] if t > 0 else np.zeros_like(c)
        d = dh[:, t] + dhr
        tc = np.tanh(c)
        dc = dcc + d * og * (1 - tc * tc)
        want[:, t] = np.concatenate([dc * gg * ig * (1 - ig), dc * cp * fg * (1 - fg), dc * ig * (1 - gg * gg),
                                     d * tc * og * (1 - og)], 1)
        dcc = dc * fg
        dhr = want[:, t] @ Whh
    val = want.reshape(B, F, T, 256).transpose(0, 2, 1, 3)
    return {"dgates": (val, np.full(val.shape, np.inf))}, 0


def ref_cln_stats(i, f, A, m):
    B, T, P, C = i[:4]
    assert A.get("state") is None, "whole-utterance form only"
    x = m(A["x"]).reshape(B, T, P // C, C)
    a = m(A.get("slope"))
    v = x if a is None else _prelu(x, a)
    v64 = _L(v)                                   # the device sums the fp32 values (PReLU product rounded to fp32) in doubles
    s, q = v64.sum((2, 3)), (v64 * v64).sum((2, 3))
    neg = (x <= 0) if a is not None else np.zeros(x.shape, bool)
    Ls = np.where(neg, U * _ab(v), 0.0).sum((2, 3)) + D64 * _ab(v).sum((2, 3))
    Lq = np.where(neg, 2 * U * v64 * v64, 0.0).sum((2, 3)) + D64 * q
    cs, cq = np.cumsum(s, 1), np.cumsum(q, 1)
    cnt = P * np.arange(1.0, T + 1)
    mean = cs / cnt
    var = (cq - 2 * mean * cs) / cnt + mean * mean
    rstd = 1 / np.sqrt(var + f[0])
    em = np.cumsum(Ls, 1) / cnt
    ev = np.cumsum(Lq, 1) / cnt + 2 * np.abs(mean) * em + em * em + 8 * D64 * (cq / cnt + mean * mean)
    er = 0.5 * rstd ** 3 * ev * (1 + 3 * ev * rstd * rstd) + 2 * U * rstd
    return {"sums": (np.stack([s, q], -1), np.stack([Ls, Lq], -1)),
            "mr": (m(np.stack([mean, rstd], -1)), np.stack([em + U * np.abs(mean), er], -1))}, 0


def ref_cln_apply(i, f, A, m):
    B, T, P, C, mode = i[:5]
    x = m(A["x"]).reshape(B, T, P // C, C)
    mr = m(A["mr"])
    mu, r = mr[:, :, None, None, 0], mr[:, :, None, None, 1]
    g, be, a = m(A["gain"]), m(A["bias"]), m(A["slope"])
    if mode == prg.XF_NORM_PRELU:
        xh = (x - mu) * r
        t = xh * g + be
        y = _prelu(t, a)
        lim = np.maximum(1.0, _ab(a)) * (3 * U * _ab(xh * g) + U * _ab(be)) + U * _ab(y)
    else:
        pv = _prelu(x, a)
        xh = (pv - mu) * r
        y = xh * g + be
        lim = _ab(g) * (U * _ab(pv * r) + 2 * U * _ab(xh)) + U * (_ab(xh * g) + _ab(be))
    if A.get("add") is not None:
        y = y + m(A["add"]).reshape(x.shape)
        lim = lim + U * _ab(y)
    return {"y": (y.reshape(B, T, P), lim.reshape(B, T, P))}, 0


def ref_cln_bwd(i, f, A, m, count_shift=1):
    """count_shift: the frames counted at row t are t + count_shift (1; the CPU mutation check passes 0)"""
    B, T, P, C, mode = i[:5]
    Fq = P // C
    sh = (B, T, Fq, C)
    dy, x = m(A["dy"]).reshape(sh), m(A["x"]).reshape(sh)
    mr = m(A["mr"])
    mu, r = mr[:, :, None, None, 0], mr[:, :, None, None, 1]
    g, be, a = m(A["gain"]), m(A["bias"]), m(A["slope"])
    one = np.ones((), m.dt)
    amb = np.zeros(sh, bool)
    flip = np.zeros(sh)
    if mode == prg.XF_NORM_PRELU:
        xh = (x - mu) * r
        uu = xh * g + be
        mag = _ab(xh * g) + _ab(be)
        amb = _ab(uu) <= KINK * U * mag
        pos = uu > 0
        dd = np.where(pos, dy, a * dy)
        flip = np.where(amb, np.abs(1 - _L(a)) * _ab(dy), 0.0)
        vv = x
        S_ = m.sum(np.where(pos, 0 * one, dy * uu), 2)
        LS = (Fq + 5) * U * np.where(pos & ~amb, 0.0, _ab(dy) * mag).sum(2) + np.where(amb, _ab(dy * uu), 0.0).sum(2)
        evv = np.zeros(sh)
    else:
        dd = dy
        vv = _prelu(x, a)
        evv = np.where(x > 0, 0.0, U * _ab(vv))
    cen = vv - mu
    G_ = m.sum(dd * (cen * r), 2)
    Bt = m.sum(dd, 2)
    LG = (Fq + 4) * U * _ab(dd * cen * r).sum(2) + ((flip * _ab(cen) + _ab(dd) * evv) * _ab(r)).sum(2)
    LB = (Fq + 1) * U * _ab(dd).sum(2) + flip.sum(2)
    # row sums: doubles on the device, of the fp32 dd (one product rounding in the NORM_PRELU order) and the fp32 cen
    dh = _L(dd) * _L(g)
    c64 = _L(cen)
    ra, rb = dh.sum((2, 3)), (dh * c64).sum((2, 3))
    edd = (U * np.abs(dh) if mode == prg.XF_NORM_PRELU else 0.0) + flip * _ab(g)
    La = (edd + D64 * np.abs(dh)).sum((2, 3))
    Lb = (edd * np.abs(c64) + np.abs(dh) * (U * np.abs(c64) + evv) + D64 * np.abs(dh * c64)).sum((2, 3))
    # reverse scan over t (doubles); stored as fp32 (A_t, 2 Bq_t)
    n = P * (np.arange(T) + float(count_shift))
    mu1, r1 = _L(mr[..., 0]), _L(mr[..., 1])
    c = -0.5 * r1 ** 3 * rb
    Lc = 0.5 * r1 ** 3 * Lb
    rev = lambda t: np.cumsum(t[:, ::-1], 1)[:, ::-1]                    # noqa: E731
    At, Bq2 = rev((-r1 * ra - 2 * mu1 * c) / n), 2 * rev(c / n)
    LAt = rev((r1 * La + 2 * np.abs(mu1) * Lc) / n) + 8 * D64 * rev((np.abs(r1 * ra) + 2 * np.abs(mu1 * c)) / n) + U * np.abs(At)
    LB2 = 2 * rev(Lc / n) + 16 * D64 * rev(np.abs(c) / n) + U * np.abs(Bq2)
    At_, B2_ = m(At)[:, :, None, None], m(Bq2)[:, :, None, None]
    dv = dd * g * r + At_ + vv * B2_
    Ldv = (_ab(vv) * LB2[:, :, None, None] + LAt[:, :, None, None] + evv * np.abs(Bq2)[:, :, None, None]
           + 4 * U * (_ab(dd * g * r) + _ab(vv * B2_) + np.abs(At)[:, :, None, None]))
    part = np.zeros((B, T, 3, C), m.dt)
    Lp = np.zeros((B, T, 3, C))
    if mode == prg.XF_NORM_PRELU:
        dx, Ldx = dv, Ldv
    else:
        pos = x > 0
        dx = np.where(pos, dv, a * dv)
        Ldx = np.maximum(1.0, _ab(a)) * Ldv + U * _ab(dx)
        S_ = m.sum(np.where(pos, 0 * one, dv * x), 2)
        LS = np.where(pos, 0.0, _ab(x) * Ldv).sum(2) + (Fq + 2) * U * np.where(pos, 0.0, _ab(dv * x)).sum(2)
    part[:, :, 0], part[:, :, 1], part[:, :, 2] = G_, Bt, S_
    Lp[:, :, 0], Lp[:, :, 1], Lp[:, :, 2] = LG, LB, LS
    if A.get("acc_in") is not None:
        dx = dx + m(A["acc_in"]).reshape(sh)
        Ldx = Ldx + U * _ab(dx)
    return {"rowsums": (np.stack([ra, rb], -1), np.stack([La, Lb], -1)),
            "ab": (m(np.stack([At, Bq2], -1)), np.stack([LAt, LB2], -1)),
            "part": (part.reshape(B * T, 3, C), Lp.reshape(B * T, 3, C)),
            "dx": (dx.reshape(B, T, P), Ldx.reshape(B, T, P), ~amb.reshape(B, T, P))}, int(amb.sum())


def ref_gag_pack(i, f, A, m):
    B, T, F, ld = i[:4]
    a, b = m(A["inpt"]), m(A["pre_x"])
    enc = np.stack([a[:, 0], a[:, 1], b[:, 0], b[:, 1]], -1)
    pre = np.zeros((B, T, ld), m.dt)
    pre[:, :, 0:2 * F:2], pre[:, :, 1:2 * F:2] = b[:, 0], b[:, 1]
    return {"enc_in": (enc, np.zeros(enc.shape)), "pre": (pre, np.zeros(pre.shape))}, 0


def _gag_act(g, act):
    """gain(g), gain'(g) and the limits of both as the device evaluates them"""
    if act == prg.ACT_SIGMOID:
        s = _sig(g)
        es = _ab(s) * ((_ab(g) + 6) * SIG)
        return s, s * (1 - s), es, np.abs(1 - 2 * _L(s)) * es + 2 * U * _ab(s)
    if act == prg.ACT_TANH:
        s = np.tanh(g)
        es = (_ab(s) + U) * ((2 * _ab(g) + 6) * SIG)
        return s, 1 - s * s, es, 2 * _ab(s) * es + 2 * U
    return np.maximum(g, 0), (g > 0).astype(g.dtype), np.zeros(g.shape), np.zeros(g.shape)


def ref_gag_crm(i, f, A, m):
    B, T, F, ld, lin_ld, act = i[:6]
    pre = m(A["pre"])[:, :, :2 * F].reshape(B, T, F, 2)
    g, r, im = (m(A[k])[:, :, :F] for k in ("g", "r", "i"))
    gain, _, eg, _ = _gag_act(g, act)
    y = pre * gain[..., None] + np.stack([r, im], -1)
    lim = _ab(pre) * eg[..., None] + 2 * U * _ab(pre * gain[..., None]) + U * _ab(y)
    nxt, ln = np.zeros((B, T, ld), m.dt), np.zeros((B, T, ld))
    nxt[:, :, :2 * F], ln[:, :, :2 * F] = y.reshape(B, T, 2 * F), lim.reshape(B, T, 2 * F)
    return {"pre_out": (nxt, ln), "planar": (np.moveaxis(y, -1, 1), np.moveaxis(lim, -1, 1))}, 0


def ref_gag_crm_bwd(i, f, A, m):
    B, T, F, ld, lin_ld, act = i[:6]
    pre = m(A["pre"])[:, :, :2 * F].reshape(B, T, F, 2)
    g = m(A["g"])[:, :, :F]
    dy, edy = np.zeros((B, T, F, 2), m.dt), np.zeros((B, T, F, 2))
    if A.get("dplanar") is not None:
        dy = dy + np.moveaxis(m(A["dplanar"]), 1, -1)
    if A.get("dpre_out") is not None:
        dy = dy + m(A["dpre_out"])[:, :, :2 * F].reshape(B, T, F, 2)
        if A.get("dplanar") is not None:
            edy = U * _ab(dy)
    gain, dact, eg, eda = _gag_act(g, act)
    dot = dy[..., 0] * pre[..., 0] + dy[..., 1] * pre[..., 1]
    mag = _ab(dy[..., 0] * pre[..., 0]) + _ab(dy[..., 1] * pre[..., 1])
    dgv = dot * dact
    Ldg = (3 * U * mag + (edy * _ab(pre)).sum(-1)) * _ab(dact) + _ab(dot) * eda + U * _ab(dgv)
    dp = dy * gain[..., None]
    Ldp = edy * _ab(gain)[..., None] + _ab(dy) * eg[..., None] + U * _ab(dp)
    out = {}
    for name, v, l in (("dg", dgv, Ldg), ("dr", dy[..., 0], edy[..., 0]), ("di", dy[..., 1], edy[..., 1])):
        val, lim = np.zeros((B, T, lin_ld), m.dt), np.zeros((B, T, lin_ld))
        val[:, :, :F], lim[:, :, :F] = v, l
        out[name] = (val, lim)
    if "dpre" in A:
        val, lim = np.zeros((B, T, ld), m.dt), np.zeros((B, T, ld))
        val[:, :, :2 * F], lim[:, :, :2 * F] = dp.reshape(B, T, 2 * F), Ldp.reshape(B, T, 2 * F)
        if A.get("acc_in") is not None:
            val = val + m(A["acc_in"])
            lim = lim + U * _ab(val)
        out["dpre"] = (val, lim)
    return out, 0


def ref_memset0(i, f, A, m):
    n = _n64(i) // 4
    return {"ptr": (np.zeros(n, m.dt), np.zeros(n))}, 0


def wgrad_terms(op: tr.WgradOp, A, m, drop_tap: int = -1):
    """the sums a weight gradient ADDS: (dw [N][Kpad], its limit without the previous value, dbias [N] or None, its limit).
    drop_tap: the CPU mutation check leaves one tap out."""
    B, T, N, No = op.B, op.T, op.N, op.No
    dz = m(A["dz"])[:, :, np.arange(No) * op.ostride + op.ophase]          # (B, T, No, N): the rows of this launch
    src = m(A["src0"]) if op.src1 is None else np.concatenate([m(A["src0"]), m(A["src1"])], -1)
    Ct = src.shape[-1]
    upt = (Ct + 15) // 16
    assert op.Kpad == len(op.dt) * upt * 16
    R = B * T * No
    dw, Ldw = np.zeros((N, len(op.dt), upt * 16), m.dt), np.zeros((N, len(op.dt), upt * 16))
    o = np.arange(No)
    Z = dz.reshape(R, N)
    for j, (dt, io) in enumerate(zip(op.dt, op.ioff)):
        if j == drop_tap:
            continue
        fi = o * op.istride + io
        ok = (fi >= 0) & (fi < op.Fin)
        G = np.zeros((B, T, No, Ct), m.dt)
        tv = T - abs(dt)
        dst_t = slice(-dt, T) if dt <= 0 else slice(0, tv)
        src_t = slice(0, tv) if dt <= 0 else slice(dt, T)
        if tv > 0:
            G[:, dst_t, ok] = src[:, src_t][:, :, fi[ok]]
        G = G.reshape(R, Ct)
        dw[:, j, :Ct] = Z.T @ G
        Ldw[:, j, :Ct] = (R + 2) * U * (_ab(Z).T @ _ab(G))
    db = Ldb = None
    if op.dbias is not None:
        db = m.sum(Z, 0)
        Ldb = (R + 2) * U * _ab(Z).sum(0)
    return dw.reshape(N, op.Kpad), Ldw.reshape(N, op.Kpad), db, Ldb


def ref_wgrad(op, A, m, drop_tap: int = -1):
    dw, Ldw, db, Ldb = wgrad_terms(op, A, m, drop_tap)
    prev = m(A["dw"])
    out = {"dw": (prev + dw, SECOND * (Ldw + (op.B * op.T * op.No + 2) * U * _ab(prev)))}
    if db is not None:
        pb = m(A["dbias"])
        out["dbias"] = (pb + db, SECOND * (Ldb + (op.B * op.T * op.No + 2) * U * _ab(pb)))
    return out, 0


REFS = {"IN_STATS": ref_in_stats, "IN_STATS_MULTI": lambda i, f, A, m: ref_in_stats(i, f, A, m, multi=True),
        "IN_FINALIZE": ref_in_finalize, "TR_NORM_ACT": ref_tr_norm_act, "NORM_BWD": ref_norm_bwd,
        "NORM_BWD_MULTI": ref_norm_bwd_multi, "GLU_BWD": ref_glu_bwd, "GATE_FWD": ref_gate_fwd, "GATE_BWD": ref_gate_bwd,
        "ADD": ref_add, "RELU_BWD": ref_relu_bwd, "COLSUM": ref_colsum, "FILTER_SUM": ref_filter_sum, "FS_BWD": ref_fs_bwd,
        "LN_FWD": ref_ln_fwd, "LN_BWD": ref_ln_bwd, "LSTM_TRAIN": ref_lstm_train, "LSTM_BWD": ref_lstm_bwd,
        "CLN_STATS": ref_cln_stats, "CLN_APPLY": ref_cln_apply, "CLN_BWD": ref_cln_bwd, "GAG_PACK": ref_gag_pack,
        "GAG_CRM": ref_gag_crm, "GAG_CRM_BWD": ref_gag_crm_bwd, "MEMSET0": ref_memset0}
NOT_COMPARED = {"sums": ("NORM_BWD", "NORM_BWD_MULTI")}      # scratch whose layout over the copies is the kernel's own business


def run_ref(form: str, i, f, A: Dict[str, np.ndarray], dtype=np.float64):
    """the reference function of ``form`` on named arrays: {output: (val, lim[, must])}, ambiguous count"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        res, amb = REFS[form](list(i) + [0] * (8 - len(i)), list(f) + [0.0] * 4, A, _M(dtype))
    # the bounds above are first order in u; the exact constant of n roundings in a row is n u / (1 - n u) <= n u (1 + 2 n u),
    # and 2 n u <= 2^-10 for the reductions of up to 2^13 terms the walk's shapes have
    return {k: (r[0], np.asarray(r[1], np.float64) * SECOND) + tuple(r[2:]) for k, r in res.items()}, amb


def evaluate(op, fetch: Callable[[Access], np.ndarray], dtype=np.float64) -> Tuple[Dict[str, Out], int]:
    """Outs of everything ``op`` writes (keyed by the table's names), from the arrays fetch(access) returns for what it
    reads (fp32, or float64 for a 'f64' access), and the number of ambiguous elements.  Convolutions go through conv_ref
    (dtype float32: conv_ref.conv_f32, values only)."""
    if op.kind == prg.OP_CONV:
        return _evaluate_conv(op, fetch, dtype), 0
    acc = accesses(op)
    A = {a.name: fetch(a) for a in acc if a.mode in ("r", "rw")}
    A.update({a.name: True for a in acc if a.name not in A})            # written operands: present, never read
    if op.kind == tr.OP_WGRAD:
        with np.errstate(over="ignore", invalid="ignore"):
            res, amb = ref_wgrad(op, A, _M(dtype))
    else:
        i, _, f = fields(op)
        res, amb = run_ref(form_of(op), i, f, A, dtype)
    outs = {}
    for a in acc:
        if a.mode == "r":
            continue
        if a.name not in res:
            assert form_of(op) in NOT_COMPARED.get(a.name, ()), f"{op.name}: the reference does not produce {a.name}"
            outs[a.name] = Out(a.ref, a.shape, np.zeros(a.shape), np.full(a.shape, np.inf), np.zeros(a.shape, bool),
                               np.ones(a.shape, bool), name=a.name, f64=a.dtype == "f64")
            continue
        r = res[a.name]
        val, lim = np.asarray(r[0]), np.asarray(r[1], np.float64)
        assert val.shape == a.shape and lim.shape == a.shape, (op.name, a.name, val.shape, a.shape)
        must = np.ones(a.shape, bool) if len(r) < 3 else np.asarray(r[2], bool)
        outs[a.name] = Out(a.ref, a.shape, val, lim, must, np.ones(a.shape, bool), name=a.name, f64=a.dtype == "f64",
                           lstm=op.kind in (tr.OP_LSTM_TRAIN, tr.OP_LSTM_BWD))
    return outs, amb


def _evaluate_conv(op: prg.ConvOp, fetch, dtype) -> Dict[str, Out]:
    by_field = {a.name: a for a in accesses(op)}

    def conv_fetch(field, ref, shape, batched):
        a = by_field[field]
        if a.mode == "w" and field not in ("stats",):
            return np.full(shape, np.nan, np.float32)
        return fetch(a)
    lop, arena = cr.localize(op, conv_fetch)
    if np.dtype(dtype) == np.float32:
        yard = cr.conv_f32(dataclasses.replace(lop, glu_dump=None), arena)
        return {n: Out(by_field[n].ref, by_field[n].shape, cr.read(yard, getattr(lop, n), by_field[n].shape), None, None, None, name=n)
                for n in cr.L2_NAMES if getattr(lop, n, None) is not None}
    outs = {}
    for n, o in cr.conv_ref(lop, arena).items():
        outs[n] = Out(by_field[n].ref, o.shape, o.val, o.lim, o.must, o.may, o.integer, name=n)
    return outs


# ----------------------------------------------------------------------------------------------------------------------
# the comparator
# ----------------------------------------------------------------------------------------------------------------------
def check(outs: Dict[str, Out], got: Dict[str, np.ndarray], yard: Optional[Dict[str, np.ndarray]], what: str,
          margin: float = cr.MARGIN, l2_names=None) -> Tuple[float, Optional[float]]:
    """Both criteria for every output of an op.  got / yard: name -> array of the output's shape (device result / the fp32
    yardstick's value).  Per element: error <= lim on the compared (must) elements.  Per output region with a yardstick:
    L2-relative error against float64 <= margin x that of the yardstick (floor conv_ref.YARD_FLOOR).  LSTM outputs: LSTM_TOL.
    Returns (worst error / limit, worst L2 ratio); raises AssertionError naming the first violation."""
    worst, worst_l2 = 0.0, None
    for name, o in outs.items():
        g = np.asarray(got[name])
        if o.integer:
            g = np.ascontiguousarray(g, np.float32).view(np.int32)
            assert np.array_equal(g[o.must], o.val[o.must].astype(np.int32)), f"{what} {name}: {g} != {o.val}"
            continue
        if not o.must.any():
            continue
        gv, vv, lv = np.asarray(g, np.float64)[o.must], np.asarray(o.val, np.float64)[o.must], o.lim[o.must]
        assert np.isfinite(vv).all() and not np.isnan(lv).any(), f"{what} {name}: the float64 reference itself is not finite"
        assert np.isfinite(gv).all(), f"{what} {name}: {int((~np.isfinite(gv)).sum())} written elements are not finite"
        if o.lstm:
            mx = float(np.abs(gv - vv).max() / max(np.abs(vv).max(), 1e-30))
            l2 = float(np.linalg.norm(gv - vv) / max(np.linalg.norm(vv), 1e-30))
            assert mx <= LSTM_TOL and l2 <= LSTM_TOL, f"{what} {name}: max-rel {mx:.3e}, l2-rel {l2:.3e} (bound {LSTM_TOL:.0e})"
            worst = max(worst, mx / LSTM_TOL)
            continue
        fin = np.isfinite(lv)
        err = np.abs(gv - vv)
        bad = fin & (err > lv)
        if bad.any():
            k = int(np.argmax(np.where(fin, err / np.maximum(lv, 1e-300), 0.0)))
            idx = tuple(int(a[k]) for a in np.nonzero(o.must))
            raise AssertionError(f"{what} {name}: {int(bad.sum())} elements beyond the derived limit; worst at {idx}: "
                                 f"got {gv[k]:.9g}, float64 {vv[k]:.9g}, error {err[k]:.3e}, limit {lv[k]:.3e}")
        pos = fin & (lv > 0)
        if pos.any():
            worst = max(worst, float((err[pos] / lv[pos]).max()))
        if yard is not None and name in yard and (l2_names is None or name in l2_names) and not o.f64:
            y = np.asarray(yard[name], np.float64)[o.must]
            nv = max(float(np.linalg.norm(vv)), 1e-300)
            e_got, e_yard = float(np.linalg.norm(gv - vv)) / nv, max(float(np.linalg.norm(y - vv)) / nv, cr.YARD_FLOOR)
            ratio = e_got / e_yard
            assert ratio <= margin, (f"{what} {name}: L2-relative error {e_got:.3e} is {ratio:.1f} x that of the fp32 "
                                     f"evaluation ({e_yard:.3e}); allowed {margin:g} x")
            worst_l2 = ratio if worst_l2 is None else max(worst_l2, ratio)
    return worst, worst_l2


# ----------------------------------------------------------------------------------------------------------------------
# the cases both walks run
# ----------------------------------------------------------------------------------------------------------------------
CASES = {
    "eabnet-B2-T6": dict(net=dict(M=4, p=1, q=2), B=2, T=6),
    "eabnet-B3-T11": dict(net=dict(M=4, p=1, q=2), B=3, T=11),
    "cLN-B2-T6": dict(net=dict(M=4, p=1, q=2, norm_type="cLN"), B=2, T=6),
    "plain-cnn-B2-T6": dict(net=dict(M=4, p=1, q=2, is_u2=False, bf_type="cnn", is_causal=False), B=2, T=6),
    "BN-add-B2-T6": dict(net=dict(M=4, p=1, q=2, norm_type="BN", intra_connect="add"), B=2, T=6),
    "gagnet-B2-T6": dict(gag=dict(cin=2, p=1, q=1, dilas=(1, 2)), B=2, T=6),
}
F_BINS = 161


@dataclass
class Case:
    name: str
    prog: tr.TrainProgram
    flat: np.ndarray                 # parameters in prog.keys order
    boundary: Dict[str, np.ndarray]  # 'in', 'in2', 'dout' (fp32); 'out' is the program's


def make_case(name: str, seed: int = 0) -> Case:
    import paramgen
    from eabnet_amd import train_gag
    from eabnet_amd.spec import GagConfig, NetConfig, gag_param_specs, param_specs
    c = CASES[name]
    B, T = c["B"], c["T"]
    rng = np.random.default_rng([seed, len(name)])
    if "gag" in c:
        cfg = GagConfig(**c["gag"])
        prog = train_gag.lower_train(cfg, B, T, F_BINS)
        P = paramgen.make_params(gag_param_specs(cfg), 77 + seed)
        bnd = {"in": (0.3 * rng.standard_normal((B, 2, T, F_BINS))).astype(np.float32),
               "in2": (0.3 * rng.standard_normal((B, 2, T, F_BINS))).astype(np.float32)}
    else:
        cfg = NetConfig(**c["net"])
        prog = tr.lower_train(cfg, B, T, F_BINS)
        P = paramgen.make_params(param_specs(cfg), 50 + cfg.M + seed)
        bnd = {"in": paramgen.make_spec_input(B, T, F_BINS, cfg.M, 60 + cfg.M + seed)}
    out_shape = prog.out_shape or (B, 2, T, F_BINS)
    bnd["dout"] = rng.standard_normal(out_shape).astype(np.float32)
    bnd["out"] = np.full(out_shape, np.nan, np.float32)
    flat = np.concatenate([np.asarray(P[k], np.float32).reshape(-1) for k in prog.keys])
    assert flat.size == prog.n_params
    return Case(name, prog, flat, bnd)


def arena_sizes(case: Case) -> Dict[str, int]:
    p = case.prog
    out = {"a": p.a_floats, "w": p.w_floats, "g": p.g_floats}
    out.update({k: v.size for k, v in case.boundary.items()})
    return out


def wgrad_runs(ops) -> List[Tuple[int, int]]:
    """(first, count) of every maximal run of consecutive weight gradients"""
    runs, k = [], 0
    while k < len(ops):
        if ops[k].kind == tr.OP_WGRAD:
            j = k
            while j < len(ops) and ops[j].kind == tr.OP_WGRAD:
                j += 1
            runs.append((k, j - k))
            k = j
        else:
            k += 1
    return runs
