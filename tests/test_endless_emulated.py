"""The carry table against the numpy interpreter (no GPU): a streaming program is run in its smallest window, the move
of an endless stream is done with numpy from Program.carry, and EVERYTHING that is not carried -- every other row of every
workspace tensor, the input and the output buffers -- is overwritten with NaN at each move.  The frames must still be those
of the offline program, with no NaN: a tensor missing from the table, or listed with too few rows, shows at once.

tests/emulator.py recomputes every op from row 0 and restores the rows outside the window, so it cannot carry an LSTM or a
cumulative-LayerNorm count across a move; this covers the convolutional body (BatchNorm norms, pointwise head).  The
device tests (tests/test_endless_gpu.py) cover the rest."""
import numpy as np
import pytest

import paramgen
from eabnet_amd import program as prg
from eabnet_amd.spec import NetConfig, param_specs
from emulator import Emulator


def _windowed(emu, op, pos, hi):
    """one op of a streaming step, as Emulator.run_stream does it: only rows [pos, hi) of its outputs change"""
    outs = emu._outputs(op)
    if op.kind == prg.OP_CONV and op.f2_dst is not None:          # the fused second convolution writes the window's rows too
        outs = outs + [(op.f2_dst, (op.B, op.T, op.f2_N), 1)]
    saved = [emu.v(r, shp).copy() for r, shp, _ in outs]
    with np.errstate(invalid="ignore"):
        emu.step(op)
    for (r, shp, ax), old in zip(outs, saved):
        cur = emu.v(r, shp)
        idx = [slice(None)] * len(shp)
        idx[ax] = slice(pos, hi)
        new = cur[tuple(idx)].copy()
        cur[:] = old
        cur[tuple(idx)] = new


@pytest.mark.parametrize("chunk", [1, 3])
def test_a_window_with_only_the_carried_rows_reproduces_the_offline_program(chunk):
    cfg = NetConfig(M=2, norm_type="BN", p=2, q=2, bf_type="cnn")
    specs = param_specs(cfg)
    P = {k: v for k, v in paramgen.make_params(specs, 5).items() if specs[k].kind != "bn_count"}
    B, N, F, M = 1, 61, 161, 2
    x = paramgen.make_spec_input(B, N, F, M, 6)
    off = Emulator(prg.lower(cfg, P, B, N, F), x).run().copy()
    W = prg.lower(cfg, P, B, 1, F, chunk=chunk).min_window
    pw = prg.lower(cfg, P, B, W, F, chunk=chunk)
    H = pw.history
    assert (H, W) == ((8, 17) if chunk == 1 else (9, 21)) and not pw.zero_init
    emu = Emulator(pw, np.full((B, W, F, M, 2), np.nan, np.float32))
    out = np.full((B, 2, N, F), np.nan, np.float32)
    pos = moves = 0
    for t in range(0, N, chunk):
        n = min(chunk, N - t)
        if pos + chunk > W:
            assert pos >= 2 * H
            keep = [(ref, row, rows, emu.v(ref, (B, W, row))[:, pos - rows:pos].copy()) for ref, row, rows in pw.carry]
            for name in ("a", "in", "out"):
                emu.arena[name][:] = np.nan
            for ref, row, rows, data in keep:
                emu.v(ref, (B, W, row))[:, H - rows:H] = data
            pos, moves = H, moves + 1
        xin = emu.arena["in"].reshape(B, W, F, M, 2)
        xin[:, pos:pos + n] = x[:, t:t + n]
        hi = min(pos + chunk, W)
        xin[:, pos + n:hi] = 0.0                                  # a short final chunk: the rows the kernels touch are defined
        emu._win = (pos, hi)
        for op in pw.ops:
            _windowed(emu, op, pos, hi)
        out[:, :, t:t + n] = emu.arena["out"].reshape(B, 2, W, F)[:, :, pos:pos + n]
        pos += n
    assert moves >= 3
    assert not np.isnan(out).any(), f"frames {np.isnan(out).any(axis=(0, 1, 3)).nonzero()[0].tolist()} read a row that was not carried"
    assert np.array_equal(out, off)
