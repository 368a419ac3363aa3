"""The kernels of csrc/stoi.hip, compiled for the HOST against tests/hip_host_shim (one thread per lane, pthread barriers for
``__syncthreads`` and the wave operations) into a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer, and run
on a few of the seeded cases: the same source the GPU runs, checked for reads past a row (the rows are allocated at their exact
size), for reads past an utterance's length (NaN there), against the float64 restatement, and for the same-bits contract.  No GPU
needed; the compiler is the one that builds the library.

Bounds: the kept frames must be exact (integer logic, and tests/test_stoi_ref.py shows >= 0.05 dB of margin on every frame).  The
band values come from fp32 frames and an fp32 512-point FFT: a few fp32 roundings (6e-8) relative to the largest band, bound 1e-6.
The scores are fp64 functions of those, normalised to [-1, 1]: bound 1e-6."""
import struct

import numpy as np
import pytest

import host_emulation
import stoi_ref as R

PICK = (2, 3, 4)                                         # no frame; one segment, est shorter; frames removed


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_emulation.build(tmp_path_factory, "stoi", "stoi.hip")


def _run(program, tmp_path, cases, unaligned=False, taps=True):
    B = len(cases)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", B))
        for clean, est in cases:
            f.write(struct.pack("ii", len(est), len(clean)))
        for _, est in cases:
            f.write(est.tobytes())
        for clean, _ in cases:
            f.write(clean.tobytes())
    host_emulation.run(program, src, dst, str(int(unaligned)), str(int(taps)))
    raw = open(dst, "rb").read()
    FC = struct.unpack("i", raw[:4])[0]
    o = 4
    out = np.frombuffer(raw, np.float64, 2 * B, o).reshape(B, 2)
    o += 16 * B
    K = np.frombuffer(raw, np.int32, B, o)
    o += 4 * B
    kept = np.frombuffer(raw, np.int32, B * FC, o).reshape(B, FC)
    o += 4 * B * FC
    tob = np.frombuffer(raw, np.float32, B * 30 * FC, o).reshape(B, 2, 15, FC)
    return out, K, kept, tob


def test_kernels_on_the_host_match_the_restatement_and_stay_in_bounds(program, tmp_path):
    cases = [R.make_case(*R.CASES[k]) for k in PICK]
    out, K, kept, tob = _run(program, tmp_path, cases)
    for b, k in enumerate(PICK):
        clean, est = cases[b]
        a = R.analyse(clean.astype(np.float64), est.astype(np.float64))
        assert K[b] == a["K"] and np.array_equal(kept[b, :K[b]], a["kept"]), k
        T = max(a["K"] - 1, 0)
        rel = float(np.abs(tob[b, :, :, :T] - a["tob"]).max() / a["tob"].max()) if T else 0.0
        err = max(abs(out[b, 0] - a["stoi"]), abs(out[b, 1] - a["estoi"]))
        print(f"case {k}: K {K[b]} scores {out[b]} |diff| {err:.2e}, bands {rel:.2e} of the largest")
        assert rel <= 1e-6 and err <= 1e-6, k
    assert np.isfinite(out).all(), "a sample past an utterance's length was read"
    # without the taps, alone and at a base that is not 16-byte aligned: the same bits
    alone = _run(program, tmp_path, [cases[2]], unaligned=True, taps=False)[0]
    assert np.array_equal(alone[0], out[2]), (alone, out[2])
