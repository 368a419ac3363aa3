"""The memory-bound kernels between the convolutions of every inference and streaming program, ONE LAUNCH AT A TIME through
the C ABI against the float64 references of tests/memops_ref.py on a real MI355X:

    csrc/norm.hip        eab_in_finalize_f32 / _mr_f32, eab_norm_act_f32 / eab_norm_act_win_f32
    csrc/filter_sum.hip  eab_filter_sum_f32, eab_bfw_filter_sum_f32 / _win_f32, eab_mlp_bfw_filter_sum_f32
    csrc/cln.hip         eab_cln_stats_f32, eab_cln_apply_f32, eab_cln_step_f32, eab_gate_rows_f32
    csrc/program.hip     eab_zero_rows_f32

Inputs come from seeded generators (memops_ref.*_inputs; the CPU file runs the fp32 yardstick over the same cases).  Every
output buffer holds a sentinel and carries a guard of 4096 elements in front and behind.  Asserted on every launch: return code
0; guards and every element outside the rows of the launch bit-identical to the sentinel; every element the launch must write
finite; train_ref.check -- the derived per-element limit, and the L2 criterion (conv_ref.MARGIN x the fp32 yardstick, both
against float64).  Refused arguments return non-zero and write nothing.  Each case asserts the shape-derived condition that
makes it select its code path, so a later change of a cap or a threshold fails here instead of silently un-covering the path.
One line per case: MEMOPS <kernel> <case> | err/limit .. | L2 ratio .."""
import ctypes as C

import numpy as np
import pytest
import torch

import memops_ref as mo
from eabnet_amd import program as prg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = float(np.float32(1e-5))        # what the C ABI receives (a float)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    return _lib.load()


class Outs:
    """sentinel-filled device buffers with guards; ptr(name) for the call, collect() -> host arrays after the guard check"""

    def __init__(self, **shapes):
        self.shape, self.whole = {}, {}
        for name, sh in shapes.items():
            dt = torch.float32
            if isinstance(sh[-1], str):
                sh, dt = sh[:-1], torch.float64
            n = int(np.prod(sh))
            self.shape[name] = tuple(sh)
            self.whole[name] = torch.full((n + 2 * mo.GUARD,), float(mo.SENTINEL), dtype=dt, device=DEV)

    def view(self, name):
        return self.whole[name][mo.GUARD:mo.GUARD + int(np.prod(self.shape[name]))]

    def ptr(self, name):
        return self.view(name).data_ptr()

    def collect(self, what):
        torch.cuda.synchronize()
        got = {}
        for name, w in self.whole.items():
            n = int(np.prod(self.shape[name]))
            guards = torch.cat((w[:mo.GUARD], w[mo.GUARD + n:]))
            assert bool((guards == float(mo.SENTINEL)).all()), f"{what}: wrote outside {name}"
            got[name] = w[mo.GUARD:mo.GUARD + n].cpu().numpy().reshape(self.shape[name])
        return got

    def untouched(self, what):
        torch.cuda.synchronize()
        for name, w in self.whole.items():
            assert bool((w == float(mo.SENTINEL)).all()), f"{what}: a refused call wrote to {name}"


def _dev(A):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in A.items() if isinstance(v, np.ndarray)}


def _p(d, k):
    return d[k].data_ptr() if k in d else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _win(pos=None, count=0, lens=None):
    """(eab_time_window, the device tensors it points to -- keep them alive over the launch)"""
    from eabnet_amd import _lib
    keep = [None if pos is None else torch.tensor([pos], dtype=torch.int32, device=DEV),
            None if lens is None else torch.tensor(list(lens), dtype=torch.int32, device=DEV)]
    return _lib.TimeWindow(None if pos is None else keep[0].data_ptr(), count if pos is not None else 0,
                           None if lens is None else keep[1].data_ptr()), keep


def _report(kernel, case, res, got, yard, f64=()):
    worst, l2 = mo.judge(res, got, yard, f"{kernel} {case}", f64=f64)
    print(mo.line(kernel, case, worst, l2))


# ----------------------------------------------------------------------------------------------------------------------
# norm_act / norm_act_win
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", mo.norm_act_cases(), ids=lambda c: c["name"])
def test_norm_act_matches_float64(lib, c):
    B, T, rpt, Cc = c["B"], c["T"], c["rpt"], c["C"]
    P, C4 = T * rpt, Cc // 4
    # the code path this case is here for
    hoist = mo.NA_THREADS % C4 == 0
    assert hoist == (Cc != 24), "C = 24 is the case of the non-hoisted instances (256 % (C / 4) != 0)"
    sweep = mo.NA_THREADS * mo.NA_UNROLL
    if "capped" in c:
        need, cap = -(-P * C4 // sweep), mo.na_cap(B)
        assert cap == 16 and (need > cap if c["capped"] else need == cap and P * C4 == cap * sweep)
        assert not c["capped"] or 0 < P * C4 - cap * sweep < cap * sweep // 100, "the second sweep is mostly idle lanes"
    if c.get("pos") == 8:
        assert c["pos"] + c["count"] > T, "the window is clipped by the end of the utterance"
    A = mo.norm_act_inputs(c)
    kw = mo.norm_act_kw(c)
    res, yard = mo.norm_act(A, np.float64, **kw), mo.norm_act(A, np.float32, **kw)
    d, o = _dev(A), Outs(out=(B, P, Cc))
    windowed = c.get("pos") is not None or c.get("lens") is not None
    if windowed:
        win, keep = _win(c.get("pos"), c.get("count", 0), c.get("lens"))
        rc = lib.eab_norm_act_win_f32(_p(d, "a"), _p(d, "xfa"), _p(d, "slopea"), _p(d, "b"), _p(d, "xfb"), _p(d, "slopeb"), o.ptr("out"),
                                      B, T, rpt, Cc, win, _stream())
    else:
        rc = lib.eab_norm_act_f32(_p(d, "a"), _p(d, "xfa"), _p(d, "slopea"), _p(d, "b"), _p(d, "xfb"), _p(d, "slopeb"), o.ptr("out"),
                                  B, P, Cc, _stream())
    assert rc == 0
    _report("norm_act_win" if windowed else "norm_act", c["name"], res, o.collect(c["name"]), yard)


def test_norm_act_refusals(lib):
    c = dict(B=3, T=9, rpt=5, C=24, two=False)
    d, o = _dev(mo.norm_act_inputs(c)), Outs(out=(3, 45, 24))
    win, keep = _win(0, 0)                                             # a window of no frames
    args = (_p(d, "a"), _p(d, "xfa"), _p(d, "slopea"), None, None, None, o.ptr("out"))
    assert lib.eab_norm_act_win_f32(*args, 3, 9, 5, 24, win, _stream()) != 0
    assert lib.eab_norm_act_f32(*args, 3, 45 * 4, 6, _stream()) != 0   # C no multiple of 4
    assert lib.eab_norm_act_f32(_p(d, "a"), _p(d, "xfa"), _p(d, "slopea"), _p(d, "a"), None, None, o.ptr("out"), 3, 45, 24, _stream()) != 0
    o.untouched("norm_act refusals")


# ----------------------------------------------------------------------------------------------------------------------
# in_finalize / in_finalize_mr
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", mo.FIN_C)
def test_in_finalize_matches_float64(lib, Cc):
    cases = [c for c in mo.in_finalize_cases() if c["C"] == Cc]
    assert {c["tiles"] for c in cases} >= set(mo.FIN_TILES) and max(mo.FIN_TILES) > 2 * 4 * 16
    assert any(t > 3 * 16 for t in mo.FIN_TILES), "four loads in flight need stat_tiles > 48 (FIN_SLICES = 16)"
    if Cc == 100:
        assert Cc % 64 != 0 and any(c.get("empty") for c in cases) and any(c.get("const") for c in cases)
    for c in cases:
        B, tiles, nsets = c["B"], c["tiles"], c["nsets"]
        A, count = mo.in_finalize_inputs(c)
        d = _dev(A)
        for with_mr in (False, True):
            names = [f"xf{s}" for s in range(nsets)] + ([f"mr{s}" for s in range(nsets)] if with_mr else [])
            Aq = dict(A, **{n: True for n in names if n.startswith("mr")})
            res, yard = mo.in_finalize(Aq, np.float64, count, EPS), mo.in_finalize(Aq, np.float32, count, EPS)
            o = Outs(**{n: (B, Cc, 2) for n in names})
            q = lambda n: o.ptr(n) if n in names else None                        # noqa: E731
            head = (_p(d, "stats"), B, Cc, nsets, tiles, count, EPS, _p(d, "gamma0"), _p(d, "beta0"), q("xf0"), _p(d, "gamma1"),
                    _p(d, "beta1"), q("xf1"))
            rc = lib.eab_in_finalize_mr_f32(*head, q("mr0"), q("mr1"), _stream()) if with_mr else lib.eab_in_finalize_f32(*head, _stream())
            assert rc == 0
            what = f"{c['name']}{'-mr' if with_mr else ''}"
            got = o.collect(what)
            if c.get("const"):                        # variance 0 (clamped at 0 if the subtraction went below): rstd = eps^-1/2
                for s in range(nsets):
                    want = A[f"gamma{s}"][0].astype(np.float64) / np.sqrt(np.float64(np.float32(EPS)))
                    assert np.all(np.abs(got[f"xf{s}"][:, 0, 0] - want) <= 4 * mo.U * abs(want)), "constant channel"
            _report("in_finalize_mr" if with_mr else "in_finalize", what, res, got, yard)


def test_in_finalize_refusals(lib):
    c = dict(B=3, tiles=2, C=16, nsets=2)
    A, count = mo.in_finalize_inputs(c)
    d, o = _dev(A), Outs(xf0=(3, 16, 2), xf1=(3, 16, 2))
    full = [_p(d, "stats"), 3, 16, 2, 2, count, EPS, _p(d, "gamma0"), _p(d, "beta0"), o.ptr("xf0"), _p(d, "gamma1"), _p(d, "beta1"), o.ptr("xf1")]
    for k, v in ((3, 3), (4, 0), (10, None), (12, None)):             # three sets, no tiles, a second set without gamma / tables
        bad = list(full)
        bad[k] = v
        assert lib.eab_in_finalize_f32(*bad, _stream()) != 0
    o.untouched("in_finalize refusals")


# ----------------------------------------------------------------------------------------------------------------------
# filter_sum
# ----------------------------------------------------------------------------------------------------------------------
def _filter_sum(lib, B, T, F, M):
    A = mo.filter_sum_inputs(B, T, F, M)
    res, yard = mo.filter_sum(A, np.float64, M), mo.filter_sum(A, np.float32, M)
    d, o = _dev(A), Outs(y=(B, 2, T, F))
    assert lib.eab_filter_sum_f32(_p(d, "w"), _p(d, "x"), o.ptr("y"), B, T, F, M, _stream()) == 0
    case = f"B{B}-T{T}-F{F}-M{M}"
    _report("filter_sum", case, res, o.collect(case), yard)


@pytest.mark.parametrize("M", mo.FS_M)
def test_filter_sum_matches_float64(lib, M):
    for shape in mo.FS_SHAPES:
        _filter_sum(lib, *shape, M)


def test_filter_sum_second_sweep_matches_float64(lib):
    B, T, F, M = mo.FS_LARGE
    assert 2048 * 64 < B * T * F < 2048 * 64 + 64 * 64, "just above the 2048-workgroup cap: a short second sweep"
    _filter_sum(lib, B, T, F, M)


# ----------------------------------------------------------------------------------------------------------------------
# bfw / bfw_win / mlp_bfw
# ----------------------------------------------------------------------------------------------------------------------
def _bfw_launch(lib, d, o, B, T, F, M, fused, dump, win):
    """the entry point a program would use for this form"""
    bf = o.ptr("bfw") if dump else None
    plain = win.pos is None and win.lens is None
    if fused:
        return "mlp_bfw", lib.eab_mlp_bfw_filter_sum_f32(_p(d, "h"), _p(d, "w1"), _p(d, "b1"), _p(d, "w2"), _p(d, "b2"), _p(d, "x"),
                                                         o.ptr("out"), bf, B, T, F, M, win, _stream())
    if plain:
        return "bfw", lib.eab_bfw_filter_sum_f32(_p(d, "h"), _p(d, "w2"), _p(d, "b2"), _p(d, "x"), o.ptr("out"), bf, B, T, F, M, _stream())
    return "bfw_win", lib.eab_bfw_filter_sum_win_f32(_p(d, "h"), _p(d, "w2"), _p(d, "b2"), _p(d, "x"), o.ptr("out"), bf, B, T, F, M,
                                                     win, _stream())


def _bfw_case(lib, A, d, B, T, F, M, fused, dump, case, pos=None, count=0, lens=None, refs=None):
    key = (fused, pos, count)
    if refs is None or key not in refs:
        Aq = mo.bfw_args(A, fused)
        pair = tuple(mo.bfw(Aq, dt, M, pos=pos, count=count if pos is not None else None, lens=lens) for dt in (np.float64, np.float32))
        if refs is not None:
            refs[key] = pair
    res, yard = pair if refs is None else refs[key]
    if not dump:
        res, yard = {"out": res["out"]}, {"out": yard["out"]}
    o = Outs(out=(B, 2, T, F), **({"bfw": (B, T, F, M, 2)} if dump else {}))
    win, keep = _win(pos, count, lens)
    kernel, rc = _bfw_launch(lib, d, o, B, T, F, M, fused, dump, win)
    assert rc == 0
    what = f"{case}-M{M}{'-fused' if fused else ''}{'-dump' if dump else ''}"
    got = o.collect(what)
    if lens is not None:
        for b, n in enumerate(lens):
            assert not got["out"][b, :, n:].any() and not np.signbit(got["out"][b, :, n:]).any(), "behind a length: +0.0"
    _report(kernel, what, res, got, yard)


@pytest.mark.parametrize("M", mo.BFW_M)
@pytest.mark.parametrize("shape", mo.BFW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bfw_matches_float64(lib, shape, M):
    B, T, F = shape
    tiles = -(-B * T * F // 64)
    if shape == (2, 5, 161):
        assert T * F >= 64, "the flat path"
    elif shape == (3, 137, 161):
        assert T * F >= 64 and B * T * F > 65536 and 1024 < tiles < 1024 + 16, "a few workgroups walk a second tile (grid cap 1024)"
    else:
        assert T * F < 64 and B * T * F > 64, "the non-flat path with several utterances inside a 64-row tile, more than one tile"
    if M > 16:
        assert (2 * M + 15) // 16 >= 3, "microphones past the four prefetched ones per lane, NB = 3 or 4 column blocks"
    A = mo.bfw_inputs(B, T, F, M)
    d, refs = _dev(A), {}
    for fused in (False, True):
        for dump in (False, True):
            _bfw_case(lib, A, d, B, T, F, M, fused, dump, "x".join(map(str, shape)), refs=refs)


@pytest.mark.parametrize("M", mo.BFW_M)
def test_bfw_window_matches_float64_and_keeps_the_other_rows(lib, M):
    B, T, F = mo.BFW_WIN["shape"]
    assert max(mo.BFW_WIN["poss"]) + max(mo.BFW_WIN["counts"]) > T, "one window is clipped by the end of the utterance"
    A = mo.bfw_inputs(B, T, F, M)
    d = _dev(A)
    for count in mo.BFW_WIN["counts"]:
        for pos in mo.BFW_WIN["poss"]:
            for fused in (False, True):
                _bfw_case(lib, A, d, B, T, F, M, fused, True, f"win-pos{pos}-count{count}", pos=pos, count=count)
    _bfw_case(lib, A, d, B, T, F, M, True, False, "win-pos8-count4-nodump", pos=8, count=4)


@pytest.mark.parametrize("M", mo.BFW_M)
def test_bfw_with_per_utterance_lengths(lib, M):
    """NaN in y1 (or h) and in x behind each length: exact zeros there, finite and within the limits below"""
    B, T, F = mo.BFW_LENS_SHAPE
    A = mo.bfw_inputs(B, T, F, M, lens=mo.LENS)
    assert all(np.isnan(A["h"][b, n:]).all() and np.isnan(A["x"][b, n:]).all() for b, n in enumerate(mo.LENS))
    d = _dev(A)
    for fused in (False, True):
        for dump in (False, True):
            _bfw_case(lib, A, d, B, T, F, M, fused, dump, "lens", lens=mo.LENS)


def test_bfw_refusals(lib):
    B, T, F, M = 2, 5, 161, 33
    A = mo.bfw_inputs(B, T, F, M)
    d, o = _dev(A), Outs(out=(B, 2, T, F), bfw=(B, T, F, M, 2))
    none, _ = _win()
    for fused in (False, True):
        assert _bfw_launch(lib, d, o, B, T, F, M, fused, True, none)[1] != 0, "M = 33 > BFW_MAXM"
    zero, keep = _win(0, 0)
    assert _bfw_launch(lib, d, o, B, T, F, 32, True, True, zero)[1] != 0, "a window of no frames"
    assert lib.eab_mlp_bfw_filter_sum_f32(_p(d, "h"), _p(d, "w1"), None, _p(d, "w2"), _p(d, "b2"), _p(d, "x"), o.ptr("out"), None, B, T, F, 32,
                                          none, _stream()) != 0, "w1 without b1"
    o.untouched("bfw refusals")


# ----------------------------------------------------------------------------------------------------------------------
# cLN: stats, apply, step; gate_rows; zero_rows
# ----------------------------------------------------------------------------------------------------------------------
MODES = (prg.XF_NORM_PRELU, prg.XF_PRELU_NORM)


def _cln_stats(lib, d, o, B, T, P, Cc, slope, win):
    return lib.eab_cln_stats_f32(_p(d, "x"), _p(d, "slope") if slope else None, B, T, P, Cc, EPS, o.ptr("sums"), o.ptr("state"),
                                 o.ptr("mr"), win, _stream())


def _cln_apply(lib, d, mr_ptr, y_ptr, B, T, P, Cc, mode, add, win):
    return lib.eab_cln_apply_f32(_p(d, "x"), mr_ptr, _p(d, "gain"), _p(d, "bias"), _p(d, "slope"), _p(d, "add") if add else None, y_ptr,
                                 B, T, P, Cc, mode, win, _stream())


@pytest.mark.parametrize("Cc,Fq", mo.CLN_SHAPES)
def test_cln_stats_apply_and_step_match_float64_and_stream_bit_for_bit(lib, Cc, Fq):
    B, T = mo.CLN_BT
    P = Cc * Fq
    A = mo.cln_inputs(Cc, Fq)
    d = _dev(A)
    none, _ = _win()
    case = f"C{Cc}-F{Fq}"
    for slope in (False, True):
        S = {"x": A["x"], **({"slope": A["slope"]} if slope else {})}
        res, yard = mo.cln_stats(S, np.float64, Cc, EPS), mo.cln_stats(S, np.float32, Cc, EPS)
        o = Outs(sums=(B, T, 2, "f64"), state=(3 * B, "f64"), mr=(B, T, 2))
        assert _cln_stats(lib, d, o, B, T, P, Cc, slope, none) == 0
        off = o.collect(case)
        _report("cln_stats", f"{case}{'-slope' if slope else ''}", res, off, yard, f64=("sums", "state"))
        offline_y = {}
        for mode in MODES:
            for add in (False, True):
                Q = {k: A[k] for k in ("x", "gain", "bias", "slope") + (("add",) if add else ())} | {"mr": off["mr"]}
                oy = Outs(y=(B, T, P))
                assert _cln_apply(lib, d, o.ptr("mr"), oy.ptr("y"), B, T, P, Cc, mode, add, none) == 0
                offline_y[mode, add] = oy.collect(case)["y"]
                _report("cln_apply", f"{case}-mode{mode}{'-add' if add else ''}", mo.cln_apply(Q, np.float64, Cc, mode),
                        {"y": offline_y[mode, add]}, mo.cln_apply(Q, np.float32, Cc, mode))
        # chunked: windows of 1, 3 and 5 frames with the state carried; the last window of 3 and of 5 is clipped by the end
        mode, add = MODES[1] if slope else MODES[0], slope
        for chunk in mo.CLN_CHUNKS:
            wins = mo.windows(T, chunk)
            assert chunk == 1 or wins[-1][0] + chunk > T
            oc, oy = Outs(sums=(B, T, 2, "f64"), state=(3 * B, "f64"), mr=(B, T, 2)), Outs(y=(B, T, P))
            for pos, count in wins:
                win, keep = _win(pos, count)
                assert _cln_stats(lib, d, oc, B, T, P, Cc, slope, win) == 0
                assert _cln_apply(lib, d, oc.ptr("mr"), oy.ptr("y"), B, T, P, Cc, mode, add, win) == 0
                if pos == 0 and len(wins) > 1:           # after the first window: only its rows are written
                    part = dict(oc.collect(case), **oy.collect(case))
                    for k in ("sums", "mr", "y"):
                        assert (part[k][:, count:] == mo.SENTINEL).all(), f"{k}: a row behind the first window of {count} was written"
            got = dict(oc.collect(case), **oy.collect(case))
            for k in ("sums", "state", "mr"):
                assert got[k].tobytes() == off[k].tobytes(), f"{case} chunk {chunk}: {k} differs from the offline launch"
            assert got["y"].tobytes() == offline_y[mode, add].tobytes(), f"{case} chunk {chunk}: y differs from the offline launch"
        # one frame per launch: statistics, running sums and apply fused (eab_cln_step_f32) == the three-launch form
        os_, oy = Outs(sums=(B, T, 2, "f64"), state=(3 * B, "f64"), mr=(B, T, 2)), Outs(y=(B, T, P))
        for t in range(T):
            win, keep = _win(t, 1)
            rc = lib.eab_cln_step_f32(_p(d, "x"), _p(d, "slope") if slope else None, os_.ptr("sums"), os_.ptr("state"), os_.ptr("mr"),
                                      _p(d, "gain"), _p(d, "bias"), _p(d, "slope"), _p(d, "add") if add else None, oy.ptr("y"), B, T, P, Cc,
                                      mode, EPS, win, _stream())
            assert rc == 0
            if t == 2:
                part = dict(os_.collect(case), **oy.collect(case))
                for k in ("sums", "mr", "y"):
                    assert (part[k][:, 3:] == mo.SENTINEL).all(), f"cln_step: {k} of a later frame was written"
        got = dict(os_.collect(case), **oy.collect(case))
        for k in ("sums", "state", "mr"):
            assert got[k].tobytes() == off[k].tobytes(), f"{case} cln_step: {k} differs from the offline launch"
        assert got["y"].tobytes() == offline_y[mode, add].tobytes(), f"{case} cln_step: y differs from stats + apply"
        print(mo.line("cln_step", f"{case}{'-slope' if slope else ''}", 0.0, None) + " (bit-identical to cln_stats + cln_apply)")


def test_cln_apply_and_gate_rows_at_their_grid_caps(lib):
    T, Cc = 7, 4
    none, _ = _win()
    # apply: ceil(2048 / B) blocks of 256 float4s per utterance
    B, P = 64, 4684
    cap = -(-2048 // B)
    assert cap == 32 and P % Cc == 0 and 0 < T * (P // 4) - cap * 256 <= 8, "the smallest size above the cap: a second sweep of a few lanes"
    A = mo.cln_inputs(Cc, P // Cc, B=B, T=T)
    d = _dev(A)
    mr = np.stack([0.4 + 0.01 * np.arange(B * T), 1.0 / (1.0 + 0.01 * np.arange(B * T))], -1).reshape(B, T, 2).astype(np.float32)
    dm = torch.from_numpy(mr).to(DEV)
    Q = {k: A[k] for k in ("x", "gain", "bias", "slope", "add")} | {"mr": mr}
    o = Outs(y=(B, T, P))
    assert _cln_apply(lib, d, dm.data_ptr(), o.ptr("y"), B, T, P, Cc, MODES[0], True, none) == 0
    _report("cln_apply", "cap-B64", mo.cln_apply(Q, np.float64, Cc, MODES[0]), o.collect("cap"), mo.cln_apply(Q, np.float32, Cc, MODES[0]))
    # gate_rows: 1024 blocks per utterance
    B, row = 2, 149800
    assert row % 4 == 0 and 0 < T * (row // 4) - 1024 * 256 <= 8
    rng = np.random.default_rng(5)
    G = {"a": rng.standard_normal((B, T, row), np.float32), "r": (3 * rng.standard_normal((B, T, row))).astype(np.float32)}
    d, o = _dev(G), Outs(z=(B, T, row))
    assert lib.eab_gate_rows_f32(_p(d, "a"), _p(d, "r"), o.ptr("z"), B, T, row, none, _stream()) == 0
    _report("gate_rows", "cap-1024", mo.gate_rows(G, np.float64), o.collect("cap"), mo.gate_rows(G, np.float32))


@pytest.mark.parametrize("Cc,Fq", mo.CLN_SHAPES)
def test_gate_rows_and_zero_rows_windows(lib, Cc, Fq):
    B, T = mo.CLN_BT
    P = Cc * Fq
    A = mo.cln_inputs(Cc, Fq)
    G = {"a": A["x"], "r": A["r"]}
    d = _dev(G)
    case = f"C{Cc}-F{Fq}"
    for pos, count in ((None, 0), (0, 1), (2, 3), (6, 1), (5, 5)):
        assert pos != 5 or pos + count > T, "clipped by the end of the utterance"
        win, keep = _win(pos, count)
        kw = dict(pos=pos, count=count if pos is not None else None)
        o = Outs(z=(B, T, P))
        assert lib.eab_gate_rows_f32(_p(d, "a"), _p(d, "r"), o.ptr("z"), B, T, P, win, _stream()) == 0
        what = f"{case}-{'all' if pos is None else f'pos{pos}-count{count}'}"
        _report("gate_rows", what, mo.gate_rows(G, np.float64, **kw), o.collect(what), mo.gate_rows(G, np.float32, **kw))
        o = Outs(ptr=(B, T, P))
        assert lib.eab_zero_rows_f32(o.ptr("ptr"), B, T, P, win, _stream()) == 0
        got = o.collect(what)
        _report("zero_rows", what, mo.zero_rows(B, T, P, np.float64, **kw), got, None)
        must = mo.zero_rows(B, T, P, np.float64, **kw)["ptr"][2]
        assert not np.signbit(got["ptr"][must]).any(), "+0.0"


def test_zero_rows_whole_tensor_of_an_odd_size_and_refusals(lib):
    B, T, row = 3, 7, 300
    assert (B * T * row) % (4 * 256) != 0 and (B * T * row) // 4 > 256, "more than one block, the last one partly idle"
    none, _ = _win()
    o = Outs(ptr=(B, T, row))
    assert lib.eab_zero_rows_f32(o.ptr("ptr"), B, T, row, none, _stream()) == 0
    _report("zero_rows", "whole-odd", mo.zero_rows(B, T, row, np.float64), o.collect("zero"), None)
    o = Outs(ptr=(B, T, row), z=(B, T, row))
    zero, keep = _win(0, 0)
    assert lib.eab_zero_rows_f32(o.ptr("ptr"), B, T, row, zero, _stream()) != 0, "a window of no frames"
    assert lib.eab_zero_rows_f32(o.ptr("ptr"), B, T, row - 2, none, _stream()) != 0, "rows of no whole float4s"
    assert lib.eab_zero_rows_f32(o.ptr("ptr") + 4, B, T, row - 4, none, _stream()) != 0, "a misaligned tensor"
    assert lib.eab_gate_rows_f32(o.ptr("ptr"), o.ptr("ptr"), o.ptr("z"), B, T, row - 2, none, _stream()) != 0
    assert lib.eab_gate_rows_f32(o.ptr("ptr"), o.ptr("ptr"), o.ptr("z"), B, T, row, zero, _stream()) != 0
    assert lib.eab_cln_stats_f32(o.ptr("ptr"), None, B, T, row, 64, EPS, o.ptr("z"), None, o.ptr("z"), none, _stream()) != 0, "P % C != 0"
    one, keep1 = _win(0, 1)
    assert lib.eab_cln_stats_f32(o.ptr("ptr"), None, B, T, row, 4, EPS, o.ptr("z"), None, o.ptr("z"), one, _stream()) != 0, "a window without state"
    two, keep2 = _win(0, 2)
    assert lib.eab_cln_step_f32(o.ptr("ptr"), None, o.ptr("z"), o.ptr("z"), o.ptr("z"), o.ptr("ptr"), o.ptr("ptr"), o.ptr("ptr"), None, o.ptr("z"),
                                B, T, row, 4, MODES[0], EPS, two, _stream()) != 0, "cln_step is one frame"
    assert lib.eab_cln_apply_f32(o.ptr("ptr"), o.ptr("ptr"), o.ptr("ptr"), o.ptr("ptr"), o.ptr("ptr"), None, o.ptr("z"), B, T, row, 4, 7, none,
                                 _stream()) != 0, "an unknown mode"
    o.untouched("refusals")
