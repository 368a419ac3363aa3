"""The 64- and 128-row convolution tiles (csrc/conv_gemm.hip) at the edges of their row table, patch prologue and phase-pair
epilogue: EVERY convolution launch of small EaBNet programs, one launch at a time, against the float64 reference of that
launch (tests/conv_ref.py: value, derived per-element limit, written-element set), with the walker of
test_conv_variants_gpu.py.

The programs are M = 2, B = 2 with InstanceNorm norms on the standard 161-bin chain (No = 79, 39, 19, 9, 4 down and 5, 10,
20, 40, 80 / 81 up).  There every phase-pair launch has an odd Fout = 2 No - 1 (9, 19, 39, 79: odd and even No); the even
Fout = 2 No the kernel also serves -- every row owns both columns, the epilogue's mask-free variant -- is run on the same
launches with one more output column.  The lowering's own tuning knobs put every launch on the big-tile kernel (EAB_ST=0)
with a fixed tile height (EAB_BM = 64 / 128), which small shapes would otherwise leave to the small-tile kernel.

  * T in {2, 3, 7, 33}: tiles that are all tail (T * No < bm), tiles whose rows wrap through many frames (No = 4, 5, 9, 10)
    and tiles inside one frame (No = 79 .. 81, bm = 64);
  * per-utterance lengths: one utterance full, one ending inside a tile and leaving whole tiles past its length;
  * a streaming window that starts at t_lo > 0 (BatchNorm norms; the reference is the offline launch of the same op, of
    which the window must produce exactly the rows [t_lo, t_lo + chunk) and touch nothing else);
  * the phase-pair launches with Fout = 2 No;
  * the dead-pass skip of the patch prologue: tiles whose patch size P is a multiple of 64, one position below and two
    above one (P is computed here with the kernel's formula and asserted, so the cases cannot silently go missing).
"""
import dataclasses
import time

import numpy as np
import pytest
import torch

import conv_ref as cr
import paramgen
import test_conv_variants_gpu as tv
from eabnet_amd import program as prg
from eabnet_amd.spec import NetConfig, param_specs

pytestmark = pytest.mark.gpu

M, B, F = 2, 2, 161


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def patch_sizes(op: prg.ConvOp, T: int = None) -> list:
    """P of every tile of a patch-pipeline launch, by the kernel's formula (conv_gemm_kernel, PATCH): the frames the tile's
    rows span, plus the frames its taps reach back, times the padded frame width"""
    T = op.T if T is None else T
    dt_min, io_min, io_max = min(0, min(op.dt)), min(0, min(op.ioff)), max(0, max(op.ioff))
    hi_need = (op.No - 1) * op.istride + io_max - (op.Fin - 1)
    Fp = op.Fin - io_min + max(hi_need, 0)
    Q, out = T * op.No, []
    for tile in range(prg.conv_tiles(T, op.No, op.bm)):
        q0 = tile * op.bm
        t_first, t_last = q0 // op.No, (min(q0 + op.bm, Q) - 1) // op.No
        out.append((t_last - t_first + 1 - dt_min) * Fp)
    return out


def _lower(monkeypatch, T, bm, **kw):
    monkeypatch.setenv("EAB_ST", "0")
    monkeypatch.setenv("EAB_BM", str(bm))
    cfg = NetConfig(M=M, **({"norm_type": "BN"} if kw.get("chunk") else {}))
    P = paramgen.make_params(param_specs(cfg), 50 + M)
    prog = prg.lower(cfg, P, B, T, F, precision="f32", **kw)
    convs = [k for k, op in enumerate(prog.ops) if op.kind == prg.OP_CONV]
    assert convs and all(prog.ops[k].korder != prg.KORDER_FRAG for k in convs), "a launch left the big-tile kernel"
    return prog, convs


def _bind(prog, dev):
    from eabnet_amd.model import _Bound
    bound = _Bound(prog, dev)
    xin = torch.empty((B, prog.T, F, M, 2), device=dev)
    out = torch.empty((B, 2, prog.T, F), device=dev)
    bound.bind(xin.data_ptr(), out.data_ptr())
    return bound, xin, out


def _walk_all(dev, prog, convs, lens=None, what=""):
    t0 = time.time()
    bound, xin, out = _bind(prog, dev)
    if lens is not None:
        bound.lens.copy_(torch.tensor(lens, dtype=torch.int32))
    worst = 0.0
    for k in convs:
        w, _ = tv._run_launch(bound, prog, k, xin, out, dev, [0, 1], lens, 2)
        worst = max(worst, w)
    print(f"ROWS {what}: {len(convs)} launches, worst err/limit {worst:.3f}, {time.time() - t0:.1f} s")


@pytest.mark.parametrize("bm", [64, 128])
@pytest.mark.parametrize("T", [2, 3, 7, 33])
def test_every_conv_launch_of_a_small_program_matches_float64(dev, monkeypatch, T, bm):
    prog, convs = _lower(monkeypatch, T, bm)
    ph2 = [prog.ops[k] for k in convs if prog.ops[k].epi == prg.EPI_PHASE2]
    assert {op.Fout % 2 for op in ph2} == {1} and {op.No for op in ph2} >= {5, 10, 20, 40}, "phase-pair launches with an odd Fout"
    nos = {prog.ops[k].No for k in convs}
    assert nos >= {4, 5, 9, 10, 79, 80, 81}, "rows that wrap through many frames and rows inside one frame"
    _walk_all(dev, prog, convs, what=f"T={T} bm={bm}")


def test_every_conv_launch_with_per_utterance_lengths(dev, monkeypatch):
    """utterance 0 has all 33 frames, utterance 1 six: 6 * No is no multiple of 128 for any No of the chain, and from No = 40 down
    whole tiles lie past its end (n = 0 partials, nothing stored); the padding frames of the sources hold NaN"""
    prog, convs = _lower(monkeypatch, 33, 128, varlen=True)
    lens = [33, 6]
    assert any(prg.conv_tiles(6, prog.ops[k].No, 128) < prg.conv_tiles(33, prog.ops[k].No, 128) for k in convs)
    _walk_all(dev, prog, convs, lens=lens, what="T=33 bm=128 lens=[33, 6]")


def _run_window_launch(bound, prog, k, xin, out, dev, lo):
    """op k of a streaming program alone at frame position lo: rows [lo, lo + chunk) of its outputs obey the limits of the
    offline launch of the same op, and nothing else of the arena changes"""
    op = prog.ops[k]
    hi = min(lo + prog.chunk, op.T)
    rng = np.random.default_rng(7000 + k)
    inputs = cr.random_inputs(op, rng, 2)
    arenas = {"a": bound.acts, "in": xin.view(-1)}
    bound.acts.fill_(float("nan"))
    xin.fill_(float("nan"))
    out.fill_(float("nan"))
    for ref, a in inputs.items():
        n = a[0].size
        arenas[ref.arena][ref.off:ref.off + B * n].view(B, n).copy_(torch.from_numpy(a.reshape(B, n)).to(dev))
    lop, arena = cr.cut_out(op, prog.weights, inputs)
    off_op = dataclasses.replace(lop, win=False)                         # the offline launch: every row
    outs = cr.conv_ref(off_op, arena)
    yard_arena = cr.conv_f32(off_op, arena)
    bound.t_pos.fill_(lo)
    before = bound.acts.clone()
    bound.run(torch.cuda.current_stream().cuda_stream, k, 1)
    torch.cuda.synchronize()
    changed = bound.acts.view(torch.int32) != before.view(torch.int32)
    what = f"op {k} {op.name} [{cr.key_str(cr.variant_key(op))}] window [{lo}, {hi})"
    full_ref = {f: r for f, r, _, _, _ in cr.regions(op)}
    got, yard = {}, {}
    for name, o in outs.items():
        assert name in ("dst", "dst_acc", "f2_dst") and o.shape[:2] == (B, op.T), f"{what}: {name} is not a (B, T, ...) output"
        for m in (o.must, o.may):                                        # the window writes its own frames only
            m[:, :lo] = False
            m[:, hi:] = False
        ref = full_ref[name]
        assert ref.arena == "a"
        n = int(np.prod(o.shape[1:]))
        sl = slice(ref.off, ref.off + B * n)
        may, must = torch.from_numpy(o.may.reshape(B, n)).to(dev), torch.from_numpy(o.must.reshape(B, n)).to(dev)
        ch = changed[sl].view(B, n)
        assert not (ch & ~may).any(), f"{what}: {name} changed outside the rows of the window"
        if name != "dst_acc":
            assert not (must & ~ch).any(), f"{what}: {name} has elements the window should have written and did not"
        got[name] = bound.acts[sl].view(B, n).cpu().numpy().reshape(o.shape)
        yard[name] = cr.read(yard_arena, o.ref, o.shape)
        changed[sl] = False
    assert not changed.any(), f"{what}: {int(changed.sum())} elements changed outside the launch's output regions"
    assert torch.isnan(out).all(), f"{what}: the network output was touched"
    return cr.check(outs, got, yard, what, got_is_region=True)


@pytest.mark.parametrize("bm", [64, 128])
def test_every_two_dimensional_conv_launch_in_a_streaming_window(dev, monkeypatch, bm):
    """chunk = 3 of T = 33 at t_lo = 4 (the window starts inside a tile's worth of rows: 4 * No is no multiple of the tile
    height for No = 79 .. 81) and at t_lo = 30 (it ends with the utterance)"""
    prog, convs = _lower(monkeypatch, 33, bm, chunk=3)
    convs = [k for k in convs if prog.ops[k].Fin > 1]
    assert len(convs) > 50 and all(prog.ops[k].win for k in convs)
    bound, xin, out = _bind(prog, dev)
    t0, worst = time.time(), 0.0
    for lo in (4, 30):
        for k in convs:
            w, _ = _run_window_launch(bound, prog, k, xin, out, dev, lo)
            worst = max(worst, w)
    print(f"ROWS window bm={bm}: 2 x {len(convs)} launches, worst err/limit {worst:.3f}, {time.time() - t0:.1f} s")


@pytest.mark.parametrize("bm,sizes", [(64, (64, 63, 66)), (128, (128, 126, 66))])
def test_patch_sizes_at_and_around_a_multiple_of_64(dev, monkeypatch, bm, sizes):
    """T = 31: the gated No = 4 launch has tiles of exactly 64 (bm 64: 16 frames of 4 positions) / 128 positions, the
    phase-pair No = 20 launch one of 63 (126), the No = 10 launches one of 66 -- a pass of the patch prologue that is just
    live, just dead, and live for two positions"""
    prog, convs = _lower(monkeypatch, 31, bm)
    chosen, found = [], set()
    for k in convs:
        op = prog.ops[k]
        if op.korder == prg.KORDER_CHUNK and set(patch_sizes(op)) & set(sizes):
            chosen.append(k)
            found |= set(patch_sizes(op)) & set(sizes)
    assert found == set(sizes), f"patch sizes {sorted(set(sizes) - found)} are not realised by T = 31, bm = {bm}"
    assert {prog.ops[k].epi for k in chosen} >= {prg.EPI_GLU, prg.EPI_PHASE2}
    _walk_all(dev, prog, chosen, what=f"T=31 bm={bm} P in {sizes}")


@pytest.mark.parametrize("T,bm", [(33, 128), (7, 64)])
def test_phase_pair_launches_with_an_even_fout(dev, monkeypatch, T, bm):
    """Fout = 2 No: column 2o+1 exists for every row, full tiles take the epilogue without masks and with the tile's own
    count (T = 33, bm = 128: No = 5, 10, 20, 40 give 1 to 10 full tiles and a tail; T = 7, bm = 64: full tiles from No = 10 up).
    The launches are the program's own with one more output column, written to a region behind the arena."""
    prog, convs = _lower(monkeypatch, T, bm)
    chosen = [k for k in convs if prog.ops[k].epi == prg.EPI_PHASE2]
    assert len(chosen) >= 4
    for k in chosen:
        op = prog.ops[k]
        assert op.Fout == 2 * op.No - 1
        prog.ops[k] = dataclasses.replace(op, Fout=2 * op.No, dst=prg.Ref("a", prog.act_floats))
        n = B * T * 2 * op.No * op.Cout
        prog.act_floats += n + (-n) % prg.ALIGN
    assert any(T * prog.ops[k].No >= bm for k in chosen), "no full tile"
    _walk_all(dev, prog, chosen, what=f"T={T} bm={bm} Fout = 2 No")
