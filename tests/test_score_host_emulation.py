"""The kernels of csrc/score.hip, compiled for the HOST against tests/hip_host_shim (one thread per lane, pthread barriers for
``__syncthreads`` and the wave operations) into a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer, and run
on the smallest seeded cases that can still go wrong: the same source the GPU runs, checked for reads past a row (the rows are
allocated at their exact size), for reads past a signal's length (NaN there), against the float64 restatement, and for the
same-bits contract.  No GPU needed; the compiler is the one that builds the library.

Bounds: those of tests/test_score_gpu.py -- 4.34e-4 dB = 10 log10(1 + 1e-4) on a ratio, 1e-5 relative on a loss."""
import struct

import numpy as np
import pytest

import host_emulation
import score_ref as R
from util import TOL_HIP

TOL_DB = 10.0 * np.log10(1.0 + TOL_HIP)
# odd length with a scalar tail; L % 4 = 3; three different lengths (zero extension); and one that crosses the 4096-sample span: its
# row has two workgroups, the other rows' second workgroups return early
PICK = (R.CASES[1], R.CASES[2], R.CASES[5], (4101, 4099, 4090, 920, 0.8, 0.2, 0.1))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_emulation.build(tmp_path_factory, "score", "score.hip")


def _run(program, tmp_path, cases, spectra=None, unaligned=False):
    """cases: (clean, noisy, est) triples; spectra: (esti (B, 2, Te, F), label (B, 2, Tl, F), frames) -> ratios (B, 8), losses"""
    B = len(cases)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", B))
        for clean, noisy, est in cases:
            f.write(struct.pack("iii", len(est), len(clean), len(noisy)))
        for j in (2, 0, 1):                                  # the est rows, the clean rows, the noisy rows
            for c in cases:
                f.write(c[j].tobytes())
        if spectra is None:
            f.write(struct.pack("iiii", 0, 0, 0, 0))
        else:
            esti, label, frames = spectra
            f.write(struct.pack("iiii", esti.shape[0], esti.shape[3], esti.shape[2], label.shape[2]))
            f.write(struct.pack(f"{len(frames)}i", *frames))
            f.write(esti.astype(np.float32).tobytes())
            f.write(label.astype(np.float32).tobytes())
    host_emulation.run(program, src, dst, str(int(unaligned)))
    raw = open(dst, "rb").read()
    Bl = 0 if spectra is None else spectra[0].shape[0]
    return np.frombuffer(raw, np.float64, 8 * B).reshape(B, 8), np.frombuffer(raw, np.float64, Bl, 64 * B)


def test_kernels_on_the_host_match_the_restatement_and_stay_in_bounds(program, tmp_path):
    cases = [R.make_case(*c) for c in PICK]
    # frames * F is no multiple of four and the two frame capacities differ; NaN in every frame past an utterance's count
    rng = np.random.default_rng(921)
    B, F, Te, Tl, frames = 2, 7, 5, 6, (5, 3)
    esti = rng.standard_normal((B, 2, Te, F)).astype(np.float32)
    label = rng.standard_normal((B, 2, Tl, F)).astype(np.float32)
    want_loss = [R.loss_one(esti[b], label[b], frames[b]) for b in range(B)]
    for b in range(B):
        esti[b, :, frames[b]:] = np.nan
        label[b, :, frames[b]:] = np.nan
    out, loss = _run(program, tmp_path, cases, (esti, label, frames))
    for b, (clean, noisy, est) in enumerate(cases):
        err = float(np.abs(out[b, :4] - R.ratios(est, clean, noisy)).max())
        print(f"case {PICK[b][:3]}: {out[b, :4]} max |diff| {err:.3e} dB (bound {TOL_DB:.3e})")
        assert err <= TOL_DB, PICK[b]
    for b in range(B):
        rel = abs(loss[b] - want_loss[b]) / want_loss[b]
        print(f"loss of {frames[b]} frames: {loss[b]} |diff| {rel:.2e} of it")
        assert rel <= 1e-5, b
    assert np.isfinite(out).all() and np.isfinite(loss).all(), "a sample past a length was read"
    # the last case alone, at a base that is not 16-byte aligned (one load at a time) and at one that is (dwordx4): the same bits
    # as its row in the batch, so neither the batch nor the load path shows in them
    for unaligned in (True, False):
        alone = _run(program, tmp_path, [cases[-1]], unaligned=unaligned)[0]
        assert np.array_equal(alone[0], out[-1]), (unaligned, alone, out[-1])
