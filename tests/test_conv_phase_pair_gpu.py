"""The phase-pair launches (EAB_EPI_PHASE2: both output-column phases of a stride-2 transposed convolution from one staged
patch, csrc/conv_gemm.hip) one at a time against the float64 reference of the launch (tests/conv_ref.py: value, derived
per-element limit, written-element set), with the walker of test_conv_variants_gpu.py and the helpers of
test_conv_epilogue_rows_gpu.py.

What is special about them since the four-pass instance: eab_conv_f32 sends an exact-fp32 launch whose worst-case patch holds
at most 256 positions (prg.phase_pair_passes) to an instance with four patch passes and a 256-position patch area, anything
larger to the six-pass one; both multiply one column block at a time, and every tile requests its first patch and weights
before it fills the transform tables and meets the kernel's first barrier.

  * programs M = 2, B = 2, T in {2, 3, 7, 33}, tile heights 64 and 128: every phase-pair launch of the 161-bin chain
    (No = 5, 10, 20, 40; odd Fout = 2 No - 1; all of them four-pass); tile 0 of each starts at t_first = 0;
  * the same with per-utterance lengths -- whole tiles past an utterance's end skip their main loop and meet the first
    barrier on their own -- and with Fout = 2 No;
  * patch sizes either side of every pass boundary, on launches built from a launch of the program with another frame
    width (the reference knows a launch by its fields alone).  The P of a tile is (frames the tile spans - dt_min) x (No + 1)
    here, computed with the kernel's formula and asserted: 63 / 64 / 66, 126 / 128 / 130, 190 / 192 / 194, 255 / 256 in tiles of
    four-pass launches, and a launch with a worst case of 258 positions, which must take the six-pass instance.
    191, 193 and 257 cannot occur.  They are primes; a tile's P is frames x width, so only a tile inside one frame of that
    width could have it, and the worst case of its launch -- at least two frames, which is what the entry point goes by and
    bounds by 352 -- would be 2 P.  190 / 194 and 258 are the nearest sizes that do occur;
  * a launch whose second tap reaches one frame back (dt = -1): the first patch row of the tiles at t_first = 0 is causal
    padding.
"""
import dataclasses

import pytest
import torch

import test_conv_epilogue_rows_gpu as tr
from eabnet_amd import program as prg

pytestmark = pytest.mark.gpu

B = tr.B


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _phase_pairs(prog, convs):
    return [k for k in convs if prog.ops[k].epi == prg.EPI_PHASE2]


@pytest.mark.parametrize("bm", [64, 128])
@pytest.mark.parametrize("T", [2, 3, 7, 33])
def test_every_phase_pair_launch_of_a_small_program_matches_float64(dev, monkeypatch, T, bm):
    prog, convs = tr._lower(monkeypatch, T, bm)
    chosen = _phase_pairs(prog, convs)
    ops = [prog.ops[k] for k in chosen]
    assert {op.No for op in ops} == {5, 10, 20, 40} and all(op.Fout == 2 * op.No - 1 and op.bm == bm for op in ops)
    assert {prg.phase_pair_passes(op) for op in ops} == {4}
    tr._walk_all(dev, prog, chosen, what=f"phase pairs T={T} bm={bm}")


@pytest.mark.parametrize("bm", [64, 128])
def test_phase_pair_launches_with_per_utterance_lengths(dev, monkeypatch, bm):
    """utterance 1 ends after six of 33 frames: tiles straddling its end and, from No = 20 up, whole tiles past it"""
    prog, convs = tr._lower(monkeypatch, 33, bm, varlen=True)
    chosen = _phase_pairs(prog, convs)
    assert any(prg.conv_tiles(6, prog.ops[k].No, bm) + 1 < prg.conv_tiles(33, prog.ops[k].No, bm) for k in chosen)
    tr._walk_all(dev, prog, chosen, lens=[33, 6], what=f"phase pairs T=33 bm={bm} lens=[33, 6]")


@pytest.mark.parametrize("T,bm", [(33, 128), (7, 64)])
def test_phase_pair_launches_with_an_even_fout(dev, monkeypatch, T, bm):
    """Fout = 2 No: every row owns both columns; the program's own launches with one more output column behind the arena"""
    prog, convs = tr._lower(monkeypatch, T, bm)
    chosen = _phase_pairs(prog, convs)
    for k in chosen:
        op = prog.ops[k]
        prog.ops[k] = dataclasses.replace(op, Fout=2 * op.No, dst=prg.Ref("a", prog.act_floats))
        n = B * T * 2 * op.No * op.Cout
        prog.act_floats += n + (-n) % prg.ALIGN
    assert any(T * prog.ops[k].No >= bm for k in chosen), "no full tile"
    tr._walk_all(dev, prog, chosen, what=f"phase pairs T={T} bm={bm} Fout = 2 No")


def _reshaped(prog, k, No, bm, T, dt=None):
    """launch k of the program with another frame width: No output pairs from Fin = No - 1 input positions per frame, Fout =
    2 No - 1, T frames, tile height bm; sources, output and statistics partials in fresh regions behind the arena"""
    op = prog.ops[k]
    assert op.epi == prg.EPI_PHASE2 and op.C1 > 0 and op.nsets == 1 and op.fin_stats is None and list(op.dt) == [0, 0]

    def region(floats):
        ref = prg.Ref("a", prog.act_floats)
        prog.act_floats += floats + (-floats) % prg.ALIGN
        return ref
    Fin, Fout, tiles = No - 1, 2 * No - 1, prg.conv_tiles(T, No, bm)
    new = dataclasses.replace(op, T=T, Fin=Fin, No=No, Fout=Fout, bm=bm, dt=list(dt or op.dt),
                              src0=region(B * T * Fin * op.C0), src1=region(B * T * Fin * op.C1),
                              dst=region(B * T * Fout * op.Cout), stats=region(B * tiles * op.Cout * 4), stat_tiles=tiles, stat_tile0=0)
    prog.ops[k] = new
    return new


# (No, tile height, frames) -> the patch sizes its tiles must show; worst case of the launch; passes of its instance
BOUNDARY_CASES = [
    ((62, 64, 2), {63, 126}, 189, 4),
    ((63, 64, 2), {64, 128}, 192, 4),
    ((32, 64, 2), {66}, 99, 4),
    ((64, 128, 2), {130}, 195, 4),
    ((94, 64, 2), {95, 190}, 190, 4),
    ((95, 64, 2), {96, 192}, 192, 4),
    ((96, 64, 2), {97, 194}, 194, 4),
    ((84, 128, 4), {170, 255}, 255, 4),
    ((127, 64, 2), {128, 256}, 256, 4),
    ((85, 128, 4), {172, 258}, 258, 6),
]


@pytest.mark.parametrize("shape,sizes,worst,passes", BOUNDARY_CASES, ids=[f"P{max(c[1])}" for c in BOUNDARY_CASES])
def test_patch_sizes_either_side_of_every_pass_boundary(dev, monkeypatch, shape, sizes, worst, passes):
    No, bm, T = shape
    prog, convs = tr._lower(monkeypatch, T, bm)
    k = next(k for k in _phase_pairs(prog, convs) if prog.ops[k].C1 > 0)
    op = _reshaped(prog, k, No, bm, T)
    assert set(tr.patch_sizes(op)) >= sizes, f"tiles of {shape} have patch sizes {sorted(set(tr.patch_sizes(op)))}"
    assert prg.patch_positions(op.bm, op.No, op.Fin, op.istride, op.dt, op.ioff) == worst
    assert prg.phase_pair_passes(op) == passes
    tr._walk_all(dev, prog, [k], what=f"phase pair No={No} bm={bm} T={T} P in {sorted(sizes)}, {passes} passes")


@pytest.mark.parametrize("bm", [64, 128])
def test_first_patch_row_of_causal_padding(dev, monkeypatch, bm):
    """the second tap one frame back: every tile's patch has one more row, and at t_first = 0 that row is frame -1 -- all
    zeros behind the fused transform, never fetched"""
    T, No = 5, 20
    prog, convs = tr._lower(monkeypatch, T, bm)
    k = next(k for k in _phase_pairs(prog, convs) if prog.ops[k].C1 > 0)
    op = _reshaped(prog, k, No, bm, T, dt=[0, -1])
    frames0 = (min(bm, T * No) - 1) // No + 1
    assert tr.patch_sizes(op)[0] == (frames0 + 1) * (No + 1) and prg.phase_pair_passes(op) == 4
    tr._walk_all(dev, prog, [k], what=f"phase pair dt=[0, -1] bm={bm}")
