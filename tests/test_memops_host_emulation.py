"""csrc/norm.hip and the inference side of csrc/cln.hip -- eab_norm_act[_win]_f32, eab_in_finalize[_mr]_f32, eab_cln_stats_f32,
eab_cln_apply_f32, eab_cln_step_f32, eab_gate_rows_f32 -- compiled for the HOST against tests/hip_host_shim (one thread per lane)
into a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process: the same source the
GPU runs, on arrays allocated at exactly their size and outputs that start from a sentinel, judged by the float64 references of
tests/memops_ref.py exactly as tests/test_memops_gpu.py judges the device (memops_ref.judge).  Covered: the last sweep of
norm_act's four-float4 walk with its clamped loads in both hoist forms, a window clipped by the end of the utterance for every
windowed kernel, per-utterance lengths for norm_act (NaN behind each length), and in_finalize with C = 100 (the c < C guard)
and more than 48 tiles (four loads in flight).  (A capped norm_act grid needs at least 1024 workgroups of 256 lanes -- more
than half a minute of thread starts here; the device file runs it.)  No GPU needed; the compiler is the one that builds the library; nothing
sanitized is loaded into Python.

csrc/filter_sum.hip is NOT run here: its beam-forming kernel is written on the matrix-core builtins
(__builtin_amdgcn_mfma_f32_*), which the host shim does not have.  tests/test_memops_gpu.py checks it on the device, with
guards around every output."""
import struct

import numpy as np
import pytest

import host_emulation
import memops_ref as mo
from eabnet_amd import program as prg

EPS = float(np.float32(1e-5))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_emulation.build(tmp_path_factory, "memops")


def _run(program, tmp_path, header, lens, arrays, outs):
    """outs: (name, shape, dtype) in the order the program writes them"""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    B = header[1]
    with open(src, "wb") as f:
        f.write(struct.pack("12i", *(list(header) + [0] * (12 - len(header)))))
        f.write(struct.pack("f", EPS))
        f.write(struct.pack(f"{B}i", *(lens if lens is not None else [0] * B)))
        for a in arrays:
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    host_emulation.run(program, src, dst)
    raw, o, got = open(dst, "rb").read(), 0, {}
    for name, shape, dt in outs:
        n = int(np.prod(shape))
        got[name] = np.frombuffer(raw, dt, n, o).reshape(shape)
        o += n * np.dtype(dt).itemsize
    assert o == len(raw)
    return got


def _report(kernel, case, res, got, yard, f64=()):
    worst, l2 = mo.judge(res, got, yard, f"host {kernel} {case}", f64=f64)
    print("HOST " + mo.line(kernel, case, worst, l2))


NORM_ACT = [
    # the last sweep: n4 = 1806 (1808) float4s per utterance on two blocks of 256 lanes x 4 float4s -- lanes whose later loads
    # are clamped, lanes with nothing to do -- in the non-hoisted (C / 4 = 6) and the hoisted (C / 4 = 16) form
    dict(name="tail-C24", B=2, T=301, rpt=1, C=24, two=True),
    dict(name="tail-C64", B=2, T=113, rpt=1, C=64, two=True),
    dict(name="tail-C24-one", B=1, T=301, rpt=1, C=24, two=False),
    dict(name="win-clipped-C24", B=3, T=9, rpt=5, C=24, two=True, pos=8, count=4),
    dict(name="win-clipped-C64", B=3, T=9, rpt=5, C=64, two=False, pos=8, count=4),
    dict(name="win-inside-C24", B=3, T=9, rpt=5, C=24, two=False, pos=4, count=4),
    dict(name="lens-C24", B=3, T=9, rpt=5, C=24, two=True, lens=mo.LENS),
    dict(name="lens-C64", B=3, T=9, rpt=5, C=64, two=True, lens=mo.LENS),
]


@pytest.mark.parametrize("c", NORM_ACT, ids=lambda c: c["name"])
def test_norm_act_on_the_host(program, tmp_path, c):
    B, T, rpt, Cc = c["B"], c["T"], c["rpt"], c["C"]
    n4, sweep = T * rpt * (Cc // 4), mo.NA_THREADS * mo.NA_UNROLL
    assert (mo.NA_THREADS % (Cc // 4) == 0) == (Cc != 24)
    if c["name"].startswith("tail"):
        blocks = -(-n4 // sweep)
        assert blocks <= mo.na_cap(B) and n4 % sweep != 0
        assert blocks * mo.NA_THREADS < n4 < blocks * sweep, "a lane's first float4 is inside the utterance, a later one is not: clamped"
    A = mo.norm_act_inputs(c)
    kw = mo.norm_act_kw(c)
    win = c.get("pos") is not None
    header = [1, B, T, rpt, Cc, int(c["two"]), int(win), c.get("pos") or 0, c.get("count") or 0, int(c.get("lens") is not None)]
    arrays = [A["a"], A["xfa"], A["slopea"]] + ([A["b"], A["xfb"], A["slopeb"]] if c["two"] else [])
    got = _run(program, tmp_path, header, c.get("lens"), arrays, [("out", (B, T * rpt, Cc), np.float32)])
    _report("norm_act", c["name"], mo.norm_act(A, np.float64, **kw), got, mo.norm_act(A, np.float32, **kw))


@pytest.mark.parametrize("with_mr", [False, True])
@pytest.mark.parametrize("c", [dict(name="C100-tiles65", B=2, tiles=65, C=100, nsets=2),
                               dict(name="C100-empty", B=2, tiles=65, C=100, nsets=2, empty=True),
                               dict(name="C100-const-tiles17", B=2, tiles=17, C=100, nsets=1, const=True),
                               dict(name="C16-tiles1", B=1, tiles=1, C=16, nsets=1)], ids=lambda c: c["name"])
def test_in_finalize_on_the_host(program, tmp_path, c, with_mr):
    B, tiles, Cc, nsets = c["B"], c["tiles"], c["C"], c["nsets"]
    assert Cc != 100 or (Cc % 64 != 0 and (tiles > 48 or "const" in c))
    A, count = mo.in_finalize_inputs(c)
    arrays = [A["stats"]] + [A[f"{k}{s}"] for s in range(nsets) for k in ("gamma", "beta")]
    names = [f"xf{s}" for s in range(nsets)] + ([f"mr{s}" for s in range(nsets)] if with_mr else [])
    got = _run(program, tmp_path, [2, B, Cc, nsets, tiles, count, int(with_mr)], None, arrays, [(n, (B, Cc, 2), np.float32) for n in names])
    Aq = dict(A, **{n: True for n in names if n.startswith("mr")})
    _report("in_finalize", c["name"], mo.in_finalize(Aq, np.float64, count, EPS), got, mo.in_finalize(Aq, np.float32, count, EPS))


@pytest.mark.parametrize("Cc,Fq,slope", [(4, 300, True), (64, 3, False)])
def test_cln_unit_on_the_host_offline_chunked_and_stepped(program, tmp_path, Cc, Fq, slope):
    """offline against float64; windows of 3 frames over T = 7 (the last one clipped to one frame) and the one-frame fused step:
    bit-identical to offline"""
    B, T, P = 2, 7, Cc * Fq
    assert Cc != 4 or P > 4 * 256, "a lane of the frame sums walks more than one float4"
    A = mo.cln_inputs(Cc, Fq, B=B, T=T)
    mode, add = (prg.XF_PRELU_NORM, True) if slope else (prg.XF_NORM_PRELU, False)
    arrays = [A["x"], A["slope"], A["gain"], A["bias"], A["add"]]
    outs = [("sums", (B, T, 2), np.float64), ("state", (3 * B,), np.float64), ("mr", (B, T, 2), np.float32), ("y", (B, T, P), np.float32)]
    run = lambda chunk: _run(program, tmp_path, [3, B, T, P, Cc, mode, int(slope), int(add), chunk], None, arrays, outs)   # noqa: E731
    off = run(0)
    S = {"x": A["x"], **({"slope": A["slope"]} if slope else {})}
    stats = {k: off[k] for k in ("sums", "state", "mr")}
    _report("cln_stats", f"C{Cc}", mo.cln_stats(S, np.float64, Cc, EPS), stats, mo.cln_stats(S, np.float32, Cc, EPS), f64=("sums", "state"))
    Q = {k: A[k] for k in ("x", "gain", "bias", "slope") + (("add",) if add else ())} | {"mr": off["mr"]}
    _report("cln_apply", f"C{Cc}", mo.cln_apply(Q, np.float64, Cc, mode), {"y": off["y"]}, mo.cln_apply(Q, np.float32, Cc, mode))
    assert mo.windows(T, 3)[-1] == (6, 3), "clipped by the end of the utterance"
    for chunk in (3, -1):
        got = run(chunk)
        for k in off:
            assert got[k].tobytes() == off[k].tobytes(), f"chunk {chunk}: {k} differs from the offline launch"


@pytest.mark.parametrize("pos,count", [(None, 0), (2, 3), (5, 5)])
def test_gate_rows_on_the_host(program, tmp_path, pos, count):
    B, T, row = 2, 7, 300
    assert pos != 5 or pos + count > T, "clipped by the end of the utterance"
    rng = np.random.default_rng(9)
    G = {"a": rng.standard_normal((B, T, row), np.float32), "r": (3 * rng.standard_normal((B, T, row))).astype(np.float32)}
    got = _run(program, tmp_path, [4, B, T, row, int(pos is not None), pos or 0, count], None, [G["a"], G["r"]], [("z", (B, T, row), np.float32)])
    kw = dict(pos=pos, count=count if pos is not None else None)
    _report("gate_rows", f"pos{pos}", mo.gate_rows(G, np.float64, **kw), got, mo.gate_rows(G, np.float32, **kw))
