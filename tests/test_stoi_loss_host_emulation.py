"""The gradient kernels of csrc/stoi_bwd.hip (with csrc/stoi.hip for the value they build on), compiled for the HOST against tests/hip_host_shim into a stand-alone program with
AddressSanitizer and UndefinedBehaviorSanitizer (tests/hip_host_shim/stoi_bwd_main.cpp): eab_stoi_f32, then eab_stoi_bwd_f32 on the
workspace it leaves, on rows allocated at their exact size and NaN past every utterance's own length.  The same source the GPU
runs, checked for reads and writes past a row, for reads past a length, against the float64 reference of tests/stoi_loss_ref.py,
and for the same-bits contract.  No GPU needed.

Measured here (fp32 frames, fp32 transforms both ways, fp32 stored band values, fp64 segment statistics): the gradient is
1.6e-7 to 5.1e-7 of max |ref| off float64 on every gradient case and factor setting -- the bar of the GPU tests, 1e-5, is asserted."""
import struct

import numpy as np
import pytest

import host_emulation
import stoi_loss_ref as G
import stoi_ref as R

BAR = 1e-5
PICK = (2, 3, 4, -1)                                     # no frame (sentinel); one segment, est shorter; frames removed; est much shorter
WEIGHTS = (1.0, 0.7, -1.3, 2.0)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_emulation.build(tmp_path_factory, "stoi_bwd", "stoi.hip", "stoi_bwd.hip")


def _run(program, tmp_path, cases, weights, factors, unaligned=False):
    B = len(cases)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", B))
        for clean, est in cases:
            f.write(struct.pack("ii", len(est), len(clean)))
        f.write(np.asarray(weights, np.float32).tobytes())
        for _, est in cases:
            f.write(est.tobytes())
        for clean, _ in cases:
            f.write(clean.tobytes())
    host_emulation.run(program, src, dst, str(int(unaligned)), repr(factors[0]), repr(factors[1]), timeout=900)
    raw = open(dst, "rb").read()
    cap = struct.unpack("i", raw[:4])[0]
    out = np.frombuffer(raw, np.float64, 2 * B, 4).reshape(B, 2)
    grad = np.frombuffer(raw, np.float32, B * cap, 4 + 16 * B).reshape(B, cap)
    return out, grad


def _case(k):
    return R.make_case(*(R.CASES[k] if k >= 0 else G.SHORT_EST_CASE))


def test_gradient_kernels_on_the_host_match_float64_and_stay_in_bounds(program, tmp_path):
    cases = [_case(k) for k in PICK]
    factors = (0.5, 0.5)
    out, grad = _run(program, tmp_path, cases, WEIGHTS, factors)
    assert np.isfinite(grad).all(), "a sample past an utterance's length was read, or a gradient sample was not written"
    for b, k in enumerate(PICK):
        clean, est = cases[b]
        _, ref, info = G.loss_and_grad(clean, est, *factors)
        ref = ref * float(np.float32(WEIGHTS[b]))
        assert (grad[b, len(est):] == 0).all(), "the gradient past est's own length"
        assert (grad[b, :len(est)][ref == 0] == 0).all(), "samples that reach no kept band frame"
        scale = np.abs(ref).max()
        err = float(np.abs(grad[b, :len(est)] - ref).max() / scale) if scale else float(np.abs(grad[b]).max())
        print(f"case {k}: K {info['K']}, max |ref| {scale:.3e}, gradient max |diff| / max |ref| = {err:.2e}")
        assert err <= BAR, k
        assert abs(out[b, 0] - float(info["stoi"])) <= 1e-6 and abs(out[b, 1] - float(info["estoi"])) <= 1e-6
    assert (grad[0] == 0).all(), "the sentinel row"
    # one half alone (the other half's work is skipped), on a row by itself at a base that is not 16-byte aligned
    for factors in ((1.0, 0.0), (0.0, 1.0)):
        _, alone = _run(program, tmp_path, [cases[1]], [WEIGHTS[1]], factors, unaligned=True)
        _, ref, _ = G.loss_and_grad(*cases[1], *factors)
        ref = ref * float(np.float32(WEIGHTS[1]))
        err = float(np.abs(alone[0] - ref).max() / np.abs(ref).max())
        print(f"case {PICK[1]} alone, factors {factors}: {err:.2e}")
        assert err <= BAR
    # alone and unaligned: the same bits as in the batch
    _, alone = _run(program, tmp_path, [cases[1]], [WEIGHTS[1]], (0.5, 0.5), unaligned=True)
    assert np.array_equal(alone[0], grad[1, :alone.shape[1]])
