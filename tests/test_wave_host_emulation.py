"""The kernels of csrc/wave_loss.hip and the ISTFT adjoint of csrc/istft.hip, compiled for the HOST against tests/hip_host_shim (one
thread per lane, pthread barriers) into a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer, and run as a
child process on the smallest cases that can still go wrong: the same source the GPU runs, checked for accesses past a row (the
arrays are allocated at their exact sizes), for reads past a length (NaN there), against the float64 restatement of
tests/wave_ref.py, and for the same-bits contract.  No GPU needed; the compiler is the one that builds the library.

Bounds: those of tests/test_wave_loss_gpu.py -- 4.34e-4 dB = 10 log10(1 + 1e-4) on a value, 1e-5 of max |ref| on a gradient."""
import struct

import numpy as np
import pytest

import host_emulation
import wave_ref as W
from util import TOL_HIP

TOL_DB = 10.0 * np.log10(1.0 + TOL_HIP)
TOL_GRAD = 1e-5
# (est, clean) samples: one sample; one below, on and one above the 4096-sample span; two spans and a scalar tail -- shorter and
# longer than their clean waves
LENGTHS = [(1, 300), (4095, 4097), (4096, 4096), (4097, 4095), (2 * 4096 + 3, 5000)]
EPS = 1e-8


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_emulation.build(tmp_path_factory, "wave", "wave_loss.hip")


def _child(program, mode, src, dst, flag):
    host_emulation.run(program, mode, src, dst, str(int(flag)))
    return open(dst, "rb").read()


def _loss(program, tmp_path, pairs, weights, unaligned):
    """pairs: (est, clean) fp32 -> (out (B, 3) float64, loss (B,), total (2,), grad (B, cap_e))"""
    B, cap = len(pairs), max(len(e) for e, _ in pairs)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("=id", B, EPS))
        for e, s in pairs:
            f.write(struct.pack("ii", len(e), len(s)))
        f.write(np.asarray(weights, np.float32).tobytes())
        for k in (0, 1):
            for p in pairs:
                f.write(p[k].tobytes())
    raw = _child(program, "loss", src, dst, unaligned)
    out = np.frombuffer(raw, np.float64, 3 * B).reshape(B, 3)
    loss = np.frombuffer(raw, np.float32, B, 24 * B)
    total = np.frombuffer(raw, np.float32, 2, 28 * B)
    grad = np.frombuffer(raw, np.float32, B * cap, 28 * B + 8).reshape(B, cap)
    return out, loss, total, grad


def test_si_sdr_kernels_on_the_host_match_the_restatement_and_stay_in_bounds(program, tmp_path):
    pairs = [W.make_pair(le, ls, 40 + k) for k, (le, ls) in enumerate(LENGTHS)]
    weights = [1.0, -0.5, 2.0, 0.25, 3.0]
    out, loss, total, grad = _loss(program, tmp_path, pairs, weights, unaligned=True)
    assert np.isfinite(out).all() and np.isfinite(grad).all(), "a sample past a length was read, or a gradient not written"
    for b, (e, s) in enumerate(pairs):
        want, wgrad = W.si_sdr_loss(e, s, EPS)
        err = abs(out[b, 0] - want)
        gerr = np.abs(grad[b, :len(e)] - weights[b] * wgrad).max() / np.abs(weights[b] * wgrad).max()
        print(f"lengths {LENGTHS[b]}: loss {out[b, 0]:.6f} dB, |diff| {err:.2e} dB (bound {TOL_DB:.2e}); gradient {gerr:.2e} (bound {TOL_GRAD:.0e})")
        assert err <= TOL_DB and abs(float(loss[b]) - want) <= TOL_DB, LENGTHS[b]
        assert gerr <= TOL_GRAD, LENGTHS[b]
        assert (grad[b, len(e):] == 0).all(), "the gradient past the estimate's length must be exactly zero"
    assert abs(total[0] - out[:, 0].sum()) <= 1e-5 * abs(out[:, 0]).sum() and abs(total[1] - out[:, 0].mean()) <= 1e-5 * abs(out[:, 0]).max()
    # a row alone -- at a 16-byte boundary and off it -- and as row 2 of a batch of three: the same bits
    trio = [pairs[1], pairs[4], pairs[3]]
    o3, _, _, g3 = _loss(program, tmp_path, trio, [1.0, 2.0, 1.0], unaligned=False)
    for unaligned in (False, True):
        o1, _, _, g1 = _loss(program, tmp_path, [pairs[4]], [2.0], unaligned=unaligned)
        assert np.array_equal(o1[0], o3[1]), (unaligned, o1, o3)
        assert np.array_equal(g1[0], g3[1, :g1.shape[1]])
    assert np.array_equal(o3[1], out[4])


@pytest.mark.parametrize("n_fft,hop,win,T,lens", [(320, 160, 320, 9, [9, 4]), (256, 64, 200, 5, [5, 3])])
def test_istft_adjoint_on_the_host_matches_the_restatement_and_stays_in_bounds(program, tmp_path, n_fft, hop, win, T, lens):
    B = len(lens)
    window = W.padded(W.window_for(n_fft, hop, win), n_fft)
    dwav = np.random.default_rng(9).standard_normal((B, hop * (T - 1))).astype(np.float32)
    for with_lens in (False, True):
        d = dwav.copy()
        if with_lens:
            for b, n in enumerate(lens):
                d[b, hop * (n - 1):] = np.nan                     # never read: constants of the forward
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("5i", B, T, n_fft, hop, int(with_lens)))
            f.write(struct.pack(f"{B}i", *lens))
            f.write(window.astype(np.float32).tobytes())
            f.write(d.tobytes())
        got = np.frombuffer(_child(program, "istft", src, dst, 0), np.float32).reshape(B, 2, T, n_fft // 2 + 1)
        want = W.istft_bwd(np.nan_to_num(d), window.astype(np.float32), n_fft, hop, T, lens if with_lens else None)
        assert np.isfinite(got).all(), "an element was not written, or dwav was read past an utterance"
        rel = np.abs(got - want).max() / np.abs(want).max()
        print(f"({n_fft},{hop},{win},{T}) lens={with_lens}: max |diff| / max |ref| = {rel:.2e} (bound {TOL_GRAD:.0e})")
        assert rel <= TOL_GRAD
        assert (got[:, 1, :, 0] == 0).all() and (got[:, 1, :, -1] == 0).all()
        if with_lens:
            for b, n in enumerate(lens):
                assert (got[b, :, n:] == 0).all()
