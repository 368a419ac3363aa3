"""The kernels of csrc/spec_loss.hip compiled for the HOST against tests/hip_host_shim (one thread per lane, pthread barriers) into a
stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer, run as a child process on the small resolutions at the
shortest utterance reflect padding allows (33 samples), on both sides of a frame group (129, 257: 9 and 17 frames at hop 16) and on
a batch of unequal lengths: the same source the GPU runs, checked for accesses past a row, a table or a workspace (every array is
allocated at its exact size), for reads past a length (NaN there), against the float64 restatement of tests/mrstft_ref.py, and for
the same-bits contract.  No GPU needed; the compiler is the one that builds the library.

Bounds: those of tests/test_mrstft_gpu.py -- 1e-4 relative on a value, 1e-5 of max |ref| on a gradient at floor = 0.02 (no bin power
within 1e-5 relative of the floor, asserted on the float64 reference)."""
import struct

import numpy as np
import pytest

import host_emulation
import mrstft_ref as M
from util import TOL_HIP

TOL_GRAD = 1e-5
FLOOR = 0.02
LENGTHS = [33, 129, 257]
SEEDS = {33: 11, 129: 12, 257: 13}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_emulation.build(tmp_path_factory, "mrstft")


def _run(program, tmp_path, pairs, weights, unaligned, floor=FLOOR, cap=None, factors=(1.0, 1.0)):
    """pairs: (est, clean) fp32, each utterance at its own length; rows of `cap` samples with NaN past the length ->
    (coef (B, R, 2) float64, loss (B,), total (2,), grad (B, cap))"""
    B, R = len(pairs), len(M.SMALL)
    lens = [len(e) for e, _ in pairs]
    cap = cap or max(lens)
    rows = np.full((2, B, cap), np.nan, np.float32)
    for b, (e, s) in enumerate(pairs):
        rows[0, b, :lens[b]], rows[1, b, :lens[b]] = e, s
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("=4i3d", B, R, cap, cap, factors[0], factors[1], floor))
        f.write(np.asarray(M.SMALL, np.int32).tobytes())
        f.write(np.asarray(lens, np.int32).tobytes())
        f.write(np.asarray(weights, np.float32).tobytes())
        f.write(rows.tobytes())
    host_emulation.run(program, src, dst, str(int(unaligned)))
    raw = open(dst, "rb").read()
    coef = np.frombuffer(raw, np.float64, B * R * 2).reshape(B, R, 2)
    loss = np.frombuffer(raw, np.float32, B, 16 * B * R)
    total = np.frombuffer(raw, np.float32, 2, 16 * B * R + 4 * B)
    grad = np.frombuffer(raw, np.float32, B * cap, 16 * B * R + 4 * B + 8).reshape(B, cap)
    return coef, loss, total, grad


@pytest.fixture(scope="module")
def pairs():
    return {n: M.make_signals(n, SEEDS[n]) for n in LENGTHS}


def test_small_resolutions_on_the_host_match_the_restatement_and_stay_in_bounds(program, tmp_path, pairs):
    for n in LENGTHS:
        e, s = pairs[n]
        margin = M.floor_margin(e, s, M.SMALL, FLOOR)
        assert margin > 1e-5, (n, margin)
        for floor in (FLOOR, 1e-7):
            want, wgrad = M.loss_and_grad(e, s, M.SMALL, floor=floor)
            _, loss, total, grad = _run(program, tmp_path, [(e, s)], [1.0], unaligned=False, floor=floor)
            rel = abs(float(loss[0]) - want) / abs(want)
            gerr = np.abs(grad[0] - wgrad).max() / np.abs(wgrad).max()
            print(f"n {n} floor {floor:g}: loss {loss[0]:.6f}, rel {rel:.2e} (bound {TOL_HIP:.0e}); gradient {gerr:.2e}"
                  + (f" (bound {TOL_GRAD:.0e}, floor margin {margin:.1e})" if floor == FLOOR else ""))
            assert np.isfinite(grad).all()
            assert rel <= TOL_HIP and total[0] == loss[0] and total[1] == loss[0]
            if floor == FLOOR:
                assert gerr <= TOL_GRAD, (n, gerr)


def test_a_batch_of_unequal_lengths_factors_weights_and_the_same_bits(program, tmp_path, pairs):
    trio = [pairs[257], pairs[33], pairs[129]]
    weights, factors = [1.0, -0.5, 2.0], (0.7, 1.3)
    _, loss, total, grad = _run(program, tmp_path, trio, weights, unaligned=True, cap=300, factors=factors)
    assert np.isfinite(loss).all() and np.isfinite(grad).all(), "a sample past a length was read, or a gradient not written"
    for b, (e, s) in enumerate(trio):
        want, wgrad = M.loss_and_grad(e, s, M.SMALL, *factors, floor=FLOOR)
        n = len(e)
        gerr = np.abs(grad[b, :n] - weights[b] * wgrad).max() / np.abs(weights[b] * wgrad).max()
        print(f"row {b} (n = {n}): rel {abs(float(loss[b]) - want) / want:.2e}, gradient {gerr:.2e}")
        assert abs(float(loss[b]) - want) <= TOL_HIP * abs(want) and gerr <= TOL_GRAD
        assert (grad[b, n:] == 0).all(), "the gradient past the utterance's length must be exactly zero"
    assert abs(total[0] - loss.sum()) <= 1e-6 * abs(loss).sum() and abs(total[1] - loss.mean()) <= 1e-6 * abs(loss).max()
    # a row alone -- at a 16-byte boundary and off it, in rows of its own length and of the batch's -- and as row 2 of three
    for unaligned in (False, True):
        for cap in (129, 300):
            c1, l1, _, g1 = _run(program, tmp_path, [pairs[129]], [2.0], unaligned=unaligned, cap=cap, factors=factors)
            assert l1[0] == loss[2] and np.array_equal(g1[0, :129], grad[2, :129]), (unaligned, cap)
    _, l2, _, g2 = _run(program, tmp_path, trio, weights, unaligned=True, cap=300, factors=factors)
    assert np.array_equal(l2, loss) and np.array_equal(g2, grad), "a second call gives other bits"
