"""The kernels of csrc/optim.hip, compiled for the HOST against tests/hip_host_shim (one thread per lane, pthread barriers for
``__syncthreads`` and the wave operations) into a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer: the
same source the GPU runs, on arrays allocated at their exact size, checked for accesses past a segment, against the float64
restatement (tests/optim_ref.py) within its bounds, and for the same-bits contract of the chunk sums.  No GPU needed; the compiler
is the one that builds the library."""
import struct

import numpy as np
import pytest

import host_emulation
import optim_ref as R

CHUNK = 4096


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_emulation.build(tmp_path_factory, "optim", "optim.hip")


def _run(program, tmp_path, segs, t, lr, betas, eps, wd, max_norm, grad_offset=0):
    """segs: [(p, g, m, v)] fp32 arrays.  Returns (partial run 1, partial run 2, norm, [(p', m', v')])."""
    b1, b2 = betas
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(segs)))
        f.write(struct.pack("7d", max_norm or 0.0, lr / (1.0 - b1 ** t), b1, b2, np.sqrt(1.0 - b2 ** t), eps, wd))
        f.write(struct.pack(f"{len(segs)}q", *[len(s[0]) for s in segs]))
        for s in segs:
            for a in s:
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
    host_emulation.run(program, src, dst, str(grad_offset))
    raw = open(dst, "rb").read()
    chunks = struct.unpack("q", raw[:8])[0]
    o = 8
    p1 = np.frombuffer(raw, np.float64, chunks, o)
    o += 8 * chunks
    p2 = np.frombuffer(raw, np.float64, chunks, o)
    o += 8 * chunks
    norm = np.frombuffer(raw, np.float64, 1, o)[0]
    o += 8
    out = []
    for s in segs:
        n, got = len(s[0]), []
        for _ in range(3):
            got.append(np.frombuffer(raw, np.float32, n, o))
            o += 4 * n
        out.append(tuple(got))
    assert o == len(raw)
    return p1, p2, norm, out


def _check(segs, res, t, lr, betas, eps, wd, max_norm, what):
    p1, p2, norm, out = res
    n = sum(len(s[0]) for s in segs)
    assert len(p1) == (n + CHUNK - 1) // CHUNK
    assert p1.tobytes() == p2.tobytes(), "the chunk sums of two runs differ in their bits"
    ref_norm = R.grad_norm([s[1] for s in segs])
    rel = abs(norm - ref_norm) / ref_norm
    c = R.clip_coef([s[1] for s in segs], max_norm)
    print(f"{what}: norm {norm:.9g}, relative error {rel:.2e}, c {c:.6g}")
    assert rel <= R.norm_rel_bound(n)
    for k, (s, got) in enumerate(zip(segs, out)):
        R.assert_within(got, *s, t, lr, betas=betas, eps=eps, weight_decay=wd, c=c, what=f"{what} segment {k}")


@pytest.mark.parametrize("n", [1, 63, 1025, 2 * CHUNK + 3])
def test_kernels_on_the_host_match_the_restatement_and_stay_in_bounds(program, tmp_path, n):
    case = R.make_case(n, 100 + n, 10.0)
    hyper = dict(t=7, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, wd=1e-2, max_norm=1.0)
    res = _run(program, tmp_path, [case], **hyper)
    _check([case], res, what=f"n {n}, clipped, weight decay", **hyper)
    if n == 1025:                                             # first step from zero state, no clipping, no decay
        fresh = R.make_case(n, 7, 1e-3, with_state=False)
        hyper = dict(t=1, lr=1e-3, betas=(0.8, 0.99), eps=1e-8, wd=0.0, max_norm=None)
        _check([fresh], _run(program, tmp_path, [fresh], **hyper), what=f"n {n}, first step", **hyper)


def test_one_unaligned_segment_of_several_chunks_has_the_bits_of_the_aligned_one(program, tmp_path):
    """chunks that lie inside one segment whose gradient is NOT 16-byte aligned: the one-by-one loads of the sum of squares and
    the lane-after-lane loop of the update (what the second module of a two-stage model gets)"""
    case = R.make_case(CHUNK + 3, 321, 2.0)
    hyper = dict(t=7, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, wd=1e-2, max_norm=1.0)
    off = _run(program, tmp_path, [case], grad_offset=1, **hyper)
    _check([case], off, what="4099 elements, gradient one float past a 16-byte boundary", **hyper)
    al = _run(program, tmp_path, [case], **hyper)
    assert off[0].tobytes() == al[0].tobytes() and off[2] == al[2]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off[3][0], al[3][0]))


def test_three_segments_with_unaligned_gradients_have_the_bits_of_one_segment(program, tmp_path):
    segs = [R.make_case(n, 200 + n, 3.0) for n in (18, 1025, 7)]
    hyper = dict(t=2, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, wd=0.0, max_norm=1.0)
    res = _run(program, tmp_path, segs, grad_offset=1, **hyper)
    _check(segs, res, what="18 + 1025 + 7, gradients one float past a 16-byte boundary", **hyper)
    one = [tuple(np.concatenate([s[k] for s in segs]) for k in range(4))]
    whole = _run(program, tmp_path, one, **hyper)
    assert whole[0].tobytes() == res[0].tobytes() and whole[2] == res[2], "the norm depends on how the run is cut into segments"
    for k in range(3):
        assert np.concatenate([o[k] for o in res[3]]).tobytes() == whole[3][0][k].tobytes()
