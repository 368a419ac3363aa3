"""The three kernels of csrc/sdr.hip compiled for the HOST against tests/hip_host_shim (one thread per lane, pthread barriers) into
a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer, run as a child process on the rows and filter lengths
of tests/test_sdr_gpu.py: the same source the GPU runs, checked for accesses past a length or a capacity (alone, every array of a
row is an allocation of exactly its size), for reads past a length in a batch (NaN there), against the dense float64 restatement of
tests/sdr_ref.py, and for the same-bits contract.  No GPU needed; the compiler is the one that builds the library.

Bounds: 4.34e-4 dB = 10 log10(1 + 1e-4) on a value and 1e-5 of max |ref| on a gradient (tests/test_wave_loss_gpu.py), and
sdr_ref.H_BOUND on the filter."""
import struct

import numpy as np
import pytest

import host_emulation
import sdr_ref as R
from util import TOL_HIP

TOL_DB = 10.0 * np.log10(1.0 + TOL_HIP)
TOL_GRAD = 1e-5
EPS = 1e-8
WEIGHTS = (1.0, -0.5, 2.0)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_emulation.build(tmp_path_factory, "sdr")


def _run(program, tmp_path, pairs, K, load_diag, eps, weights):
    """-> (alone, batch), each (out (B, 6), h (B, K), [gradient rows])"""
    B = len(pairs)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("=iidd", B, K, load_diag, eps))
        for e, s in pairs:
            f.write(struct.pack("ii", len(e), len(s)))
        f.write(np.asarray(weights, np.float32).tobytes())
        for k in (0, 1):
            for p in pairs:
                f.write(p[k].tobytes())
    host_emulation.run(program, src, dst)
    raw = open(dst, "rb").read()
    pos, out1, h1, g1 = 0, [], [], []
    for e, _ in pairs:
        out1.append(np.frombuffer(raw, np.float64, 6, pos))
        h1.append(np.frombuffer(raw, np.float64, K, pos + 48))
        g1.append(np.frombuffer(raw, np.float32, len(e), pos + 48 + 8 * K))
        pos += 48 + 8 * K + 4 * len(e)
    cap = max(len(e) for e, _ in pairs)
    out = np.frombuffer(raw, np.float64, 6 * B, pos).reshape(B, 6)
    h = np.frombuffer(raw, np.float64, K * B, pos + 48 * B).reshape(B, K)
    g = np.frombuffer(raw, np.float32, B * cap, pos + (48 + 8 * K) * B).reshape(B, cap)
    assert pos + (48 + 8 * K) * B + 4 * B * cap == len(raw)
    return (np.array(out1), np.array(h1), g1), (out, h, [g[b] for b in range(B)])


@pytest.mark.parametrize("K", R.FILTERS)
def test_sdr_kernels_on_the_host_match_the_restatement_and_stay_in_bounds(program, tmp_path, K):
    pairs = R.rows()
    alone, batch = _run(program, tmp_path, pairs, K, 0.0, EPS, WEIGHTS)
    for b, (e, s) in enumerate(pairs):
        assert np.array_equal(alone[0][b], batch[0][b]) and np.array_equal(alone[1][b], batch[1][b]), "a row alone and in the batch"
        assert np.array_equal(alone[2][b], batch[2][b][:len(e)])
        assert (batch[2][b][len(e):] == 0).all(), "the gradient past the estimate's length must be exactly zero"
        out, h, grad = batch[0][b], batch[1][b], batch[2][b][:len(e)]
        assert np.isfinite(out).all() and np.isfinite(h).all() and np.isfinite(grad).all(), "a sample past a length was read"
        want, wh = R.cached("sdr", b, K)
        wloss, wgrad = R.cached("loss", b, K, 0.0, EPS)
        herr = np.linalg.norm(h - wh) / np.linalg.norm(wh)
        tgt, ee = out[1], out[2]
        loss0 = -R.K10 * (np.log(tgt) - np.log(max(ee - tgt, 0.0)))
        if len(e) == 1:     # one sample: the gradient is zero on paper (the loss ignores a gain); measured against its two terms
            gerr = abs(float(grad[0])) / abs(WEIGHTS[b] * out[4] * float(e[0]))
        else:
            gerr = np.abs(grad - WEIGHTS[b] * wgrad).max() / np.abs(WEIGHTS[b] * wgrad).max()
        print(f"K {K} lengths {R.LENGTHS[b]}: {out[0]:.4f} dB, |diff| {abs(out[0] - want):.2e} dB (bound {TOL_DB:.2e}); "
              f"|h - ref| / |ref| {herr:.2e} (bound {R.H_BOUND:.0e}); gradient {gerr:.2e} (bound {TOL_GRAD:.0e})")
        assert abs(out[0] - want) <= TOL_DB and abs(out[0] + loss0) <= 1e-9 and abs(out[3] - wloss) <= TOL_DB
        assert herr <= R.H_BOUND
        assert gerr <= TOL_GRAD


def test_loaded_diagonal_high_sdr_and_rows_that_cannot_be_scored_on_the_host(program, tmp_path):
    e, s = R.high_row()
    quiet = (e[:700].copy(), np.zeros(600, np.float32))
    short = (e[:700].copy(), s[:100].copy())
    K = 512
    _, (out, h, grad) = _run(program, tmp_path, [quiet, (e, s), short], K, 0.0, 0.0, (1.0, 1.0, 1.0))
    for b in (0, 2):
        assert np.isnan(out[b]).all() and np.isnan(h[b]).all() and np.isnan(grad[b][:700]).all() and (grad[b][700:] == 0).all()
    want, _ = R.cached("sdr", "high", K)
    wloss, wgrad = R.cached("loss", "high", K)
    gerr = np.abs(grad[1] - wgrad).max() / np.abs(wgrad).max()
    print(f"high SDR: {out[1, 0]:.4f} dB (reference {want:.4f}), gradient {gerr:.2e} (bound {TOL_GRAD:.0e})")
    assert want > 30.0 and abs(out[1, 0] - want) <= TOL_DB and gerr <= TOL_GRAD
    e, s = R.rows()[1]
    _, (out, h, _) = _run(program, tmp_path, [(e, s)], 64, 1e-3, 0.0, (1.0,))
    want, wh = R.cached("sdr", 1, 64, 1e-3)
    assert abs(out[0, 0] - want) <= TOL_DB and np.linalg.norm(h[0] - wh) <= R.H_BOUND * np.linalg.norm(wh)
