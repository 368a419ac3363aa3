"""float64 reference of OP_INPUT_GRAD (eab_input_grad_f32) for the op-by-op walk of DESIGN §5.2, and the
cases of the training programs lowered with input_grad=True  (TEST INFRASTRUCTURE; numpy only).

tests/train_ref.py keeps one table per op kind (read / write table, kind -> form, reference function).  ``registered()`` adds
the new op's row to each of them for the duration of a ``with`` block (or a fixture), so accesses(), evaluate() and the walks
know it there, and takes the rows out again: importing this module changes nothing, and train_ref.py itself is unchanged.

    din[b][t][f][m].re = dr w.re + di w.im + dconv[b][t][f][2m]
    din[b][t][f][m].im = di w.re - dr w.im + dconv[b][t][f][2m+1]      (dr, di) = dout[b][0|1][t][f],  w = bw[b][t][f][2m..2m+1]

Limit per element: two products and two additions, 4 u on the magnitudes summed (train_ref's rule for an elementwise chain).
Lengths (lens, B frame counts): frames t >= lens[b] are exact zeros whatever the operands hold (limit 0)."""
import contextlib

import numpy as np

import train_ref as tref
from eabnet_amd import train as tr

FORM = "INPUT_GRAD"
_ROWS = lambda i: (i[0], i[1], i[2], i[4])            # noqa: E731

ARGS = [tref.Arg(0, "dout", tref._PLANAR, "r"), tref.Arg(1, "bw", _ROWS, "r"), tref.Arg(2, "dconv", _ROWS, "r"),
        tref.Arg(3, "din", lambda i: (i[0], i[1], i[2], i[3], 2), "w")]


def ref_input_grad(i, f, A, m, lens=None):
    B, T, F, M, ld = i[:5]
    d = m(A["dout"])
    w = m(A["bw"])[..., :2 * M].reshape(B, T, F, M, 2)
    c = m(A["dconv"])[..., :2 * M].reshape(B, T, F, M, 2)
    dr, di = d[:, 0][..., None], d[:, 1][..., None]
    re = dr * w[..., 0] + di * w[..., 1] + c[..., 0]
    im = di * w[..., 0] - dr * w[..., 1] + c[..., 1]
    lre = 4 * tref.U * (tref._ab(dr * w[..., 0]) + tref._ab(di * w[..., 1]) + tref._ab(c[..., 0]))
    lim_ = 4 * tref.U * (tref._ab(di * w[..., 0]) + tref._ab(dr * w[..., 1]) + tref._ab(c[..., 1]))
    val, lim = np.stack([re, im], -1), np.stack([lre, lim_], -1)
    if lens is not None:
        pad = np.arange(T)[None, :] >= np.asarray(lens)[:, None]
        val = np.where(pad[:, :, None, None, None], np.zeros((), m.dt), val)
        lim = np.where(pad[:, :, None, None, None], 0.0, lim)
    return {"din": (val, lim)}, 0


@contextlib.contextmanager
def registered():
    """train_ref's tables with the new op's rows, for the duration of the block"""
    tables = ((tref.FORMS, FORM, ARGS), (tref._KIND_FORM, tr.OP_INPUT_GRAD, FORM), (tref.REFS, FORM, ref_input_grad))
    assert not any(key in table for table, key, _ in tables)
    for table, key, row in tables:
        table[key] = row
    try:
        yield
    finally:
        for table, key, _ in tables:
            del table[key]


def make_case(name: str, seed: int = 0) -> tref.Case:
    """tests/train_ref.make_case for the same network and data, the program lowered with input_grad=True ('din' joins the
    boundary buffers)"""
    from eabnet_amd.spec import NetConfig
    base = tref.make_case(name, seed)
    c = tref.CASES[name]
    prog = tr.lower_train(NetConfig(**c["net"]), c["B"], c["T"], tref.F_BINS, input_grad=True)
    bnd = dict(base.boundary)
    bnd["din"] = np.full((c["B"], c["T"], tref.F_BINS, prog.cfg.M, 2), np.nan, np.float32)
    return tref.Case(name + "+input_grad", prog, base.flat, bnd)
