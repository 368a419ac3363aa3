"""Which phase-pair instance a launch gets (CPU): eab_conv_f32 sends an exact-fp32 EAB_EPI_PHASE2 launch whose worst-case patch
holds at most CG_PSHORT = 256 positions to the four-pass instance (conv_gemm_kernel, MODE CG_PH2S: a 256-position patch area)
and everything else to the six-pass one.  The launch carries no word for the choice -- eab_conv_desc keeps its layout --, so
the lowering's statement of it, prg.phase_pair_passes, must be the rule the entry point applies: same constant, same
positions, same precisions.  The op list itself is what it was before the instance existed.
"""
import dataclasses
import hashlib
import os
import re

import pytest

import conv_ref as cr
import paramgen
from eabnet_amd import program as prg
from eabnet_amd.spec import NetConfig, param_specs

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eabnet_amd", "csrc", "conv_gemm.hip")


def _phase_pairs(prog):
    return [op for op in prog.ops if op.kind == prg.OP_CONV and op.epi == prg.EPI_PHASE2]


def _worst(op):
    return prg.patch_positions(op.bm, op.No, op.Fin, op.istride, op.dt, op.ioff)


def test_the_entry_point_and_the_lowering_share_the_rule():
    src = open(CSRC).read()
    define = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (CG_PMAX|CG_PSHORT)\s+(\d+)", src)}
    assert define == {"CG_PMAX": prg.PATCH_MAX, "CG_PSHORT": prg.PATCH_SHORT}
    # the one place that picks CG_PH2S: exact fp32 and the worst-case positions of cg_patch_positions (= prg.patch_positions)
    picks = re.findall(r"if \((.*)\) \{\s*\n(?:.*\n){0,3}?.*cg_launch<2, 2, 1, CG_PH2S", src)
    assert picks == ["d->precision == EAB_PREC_F32 && cg_patch_positions(d) <= CG_PSHORT"], picks
    # and the kernel sizes its patch area and its passes from the same constant
    assert "PMAX = MODE == CG_PH2S ? CG_PSHORT : CG_PMAX" in src and "PP = (Smem::PMAX + 63) / 64" in src
    assert prg.PATCH_SHORT % 64 == 0 and prg.PATCH_SHORT // 64 == 4 and (prg.PATCH_MAX + 63) // 64 == 6


def test_every_phase_pair_launch_of_the_benchmark_shape_is_four_pass():
    shape = cr.bench_shapes()[0]
    assert (shape["M"], shape["B"], shape["T"], shape["precision"]) == (8, 16, 401, "f32")
    ops = _phase_pairs(cr.lower_shape(shape))
    assert len(ops) >= 12 and {op.No for op in ops} == {10, 20, 40} and {op.bm for op in ops} == {128}
    assert {_worst(op) for op in ops} == {154, 168, 205}
    assert {prg.phase_pair_passes(op) for op in ops} == {4}
    for name in ("f16x3", "bf16"):                       # the other products keep the six-pass instance
        low = _phase_pairs(cr.lower_shape(dict(shape, precision=name)))
        assert low and {op.precision for op in low} == {prg.PREC_CODE[name]} and {prg.phase_pair_passes(op) for op in low} == {6}


# (No, tile height) of a launch with Fin = No - 1, taps (0, 0) and (0, -1): worst-case positions ((bm - 1) // No + 2) (No + 1)
@pytest.mark.parametrize("No,bm,worst,passes", [
    (62, 64, 189, 4), (63, 64, 192, 4), (32, 64, 99, 4), (64, 128, 195, 4), (94, 64, 190, 4), (95, 64, 192, 4),
    (96, 64, 194, 4), (84, 128, 255, 4), (127, 64, 256, 4), (63, 128, 256, 4), (85, 128, 258, 6), (128, 64, 258, 6),
    (128, 128, 258, 6), (116, 128, 351, 6), (175, 64, 352, 6)])
def test_instance_by_worst_case_positions(monkeypatch, No, bm, worst, passes):
    monkeypatch.setenv("EAB_ST", "0")                    # (the lowering's knob: small shapes on the big-tile kernel too)
    monkeypatch.setenv("EAB_BM", str(bm))
    cfg = NetConfig(M=2)
    prog = prg.lower(cfg, paramgen.make_params(param_specs(cfg), 52), 2, 2, 161, precision="f32")
    base = next(op for op in _phase_pairs(prog) if op.C1 > 0)
    op = dataclasses.replace(base, No=No, Fin=No - 1, Fout=2 * No - 1, bm=bm)
    assert _worst(op) == worst <= prg.PATCH_MAX
    assert prg.phase_pair_passes(op) == passes
    assert prg.phase_pair_passes(dataclasses.replace(op, precision=prg.PREC_F16X3)) == 6


def test_the_op_list_is_what_it_was():
    """the choice is made behind the entry point: no field of any op changed.  (The digest was taken from the lowering before
    the four-pass instance existed.)"""
    cfg = NetConfig(M=2)
    prog = prg.lower(cfg, paramgen.make_params(param_specs(cfg), 52), 2, 7, 161, precision="f32")
    digest = hashlib.sha256(repr(prog.ops).encode()).hexdigest()
    assert digest == OPS_DIGEST, digest


OPS_DIGEST = "d313e60ba843f63d0f2bcda41b170c588fabd52dc2c906b9c1aa5ac2a6cd6ae6"
