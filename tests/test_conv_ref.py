"""The float64 reference of one convolution launch (tests/conv_ref.py) pinned on the CPU:
(a) the numpy emulator's fp32 `conv` -- an honest fp32 evaluation, itself pinned to the reference fixtures -- stays inside
    the derived limits for every ConvOp the lowering emits at the small shapes and constructor variants;
(b) the comparator rejects every mutation of a kind a subtly wrong kernel would produce;
(c) the set of kernel variants the benchmark shapes select is the set the GPU test (test_conv_variants_gpu.py) walks.
No GPU is involved; the mutations change test data only."""
import json
import os

import numpy as np
import pytest

import conv_ref as cr
import paramgen
from eabnet_amd import program as prg
from eabnet_amd.spec import GagConfig, NetConfig, gag_param_specs, param_specs
from emulator import Emulator, bf16_round
from util import GOLDEN


def _check_program(prog, emu):
    """every ConvOp of the program, cut out with the arrays the emulator holds when the op is due"""
    worst, n = 0.0, 0
    for k, op in enumerate(prog.ops):
        if op.kind == prg.OP_CONV:
            lop, arena = cr.localize(op, cr.arena_fetch(emu.arena))
            outs = cr.conv_ref(lop, arena)
            got = cr.conv_f32(lop, arena)
            w, _ = cr.check(outs, got, got, f"op {k} {op.name} [{cr.key_str(cr.variant_key(op))}]")
            for name, o in outs.items():        # the emulator writes exactly the elements the reference says are written
                before, after = cr.read(arena, o.ref, o.shape), cr.read(got, o.ref, o.shape)
                changed = before.view(np.int32) != after.view(np.int32)
                assert not (changed & ~o.may).any(), f"op {k} {op.name} {name}: written outside the launch's output set"
            worst, n = max(worst, w), n + 1
        emu.step(op)
    assert n > 0
    return worst, n


@pytest.mark.parametrize("M,B,T,pq,precision", cr.PER_OP_SHAPES)
def test_emulator_conv_within_derived_limits_per_op_shapes(M, B, T, pq, precision):
    cfg = NetConfig(M=M, p=pq[0], q=pq[1])
    P = paramgen.make_params(param_specs(cfg), 50 + M)
    prog = prg.lower(cfg, P, B, T, 161, dump_bfw=True, precision=precision)
    worst, n = _check_program(prog, Emulator(prog, paramgen.make_spec_input(B, T, 161, M, 60 + M)))
    print(f"{n} convolutions, worst err/limit {worst:.3f}")


def _variants():
    with open(os.path.join(GOLDEN, "keys_variants.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(_variants()))
def test_emulator_conv_within_derived_limits_constructor_variants(name):
    e = _variants()[name]
    cfg = NetConfig(M=e["M"], **e["kwargs"])
    P = paramgen.make_params(param_specs(cfg), 7)
    prog = prg.lower(cfg, P, 1, 13, 161)
    worst, n = _check_program(prog, Emulator(prog, paramgen.make_spec_input(1, 13, 161, e["M"], 8)))
    print(f"{name}: {n} convolutions, worst err/limit {worst:.3f}")


def test_emulator_conv_within_derived_limits_gagnet():
    with open(os.path.join(GOLDEN, "keys_gagnet.json")) as f:
        e = json.load(f)["default"]
    cfg = GagConfig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in e["kwargs"].items()})
    P = paramgen.make_params(gag_param_specs(cfg), 9)
    mk = lambda seed: np.ascontiguousarray(paramgen.make_spec_input(1, 11, 161, 1, seed)[..., 0, :].transpose(0, 3, 1, 2))  # noqa: E731
    prog = prg.lower(cfg, P, 1, 11, 161)
    _check_program(prog, Emulator(prog, mk(10), mk(11)))


def test_emulator_conv_within_derived_limits_fused_finalisation(monkeypatch):
    """EAB_FUSE_FIN=1: the last-arriving tile merges the partials (fz_*): tables and the re-armed counter"""
    monkeypatch.setenv("EAB_FUSE_FIN", "1")
    cfg = NetConfig(M=8, p=2, q=1)
    P = paramgen.make_params(param_specs(cfg), 58)
    prog = prg.lower(cfg, P, 2, 21, 161)
    fz = [op for op in prog.ops if op.kind == prg.OP_CONV and op.fz_counter is not None]
    assert fz, "the knob no longer fuses the finalisation"
    # regression: the lowering used to fuse it into launches whose kernels refuse fz_counter (csrc/conv_st.hip and the
    # EAB_EPI_PHASE2 form of csrc/conv_gemm.hip answer EAB_EINVAL), so the whole program failed at its first run
    for shape in (dict(M=8, B=2, T=21, precision="f32"), cr.bench_shapes()[3]):
        big = cr.lower_shape(shape)
        bad = [op.name for op in big.ops if op.kind == prg.OP_CONV and op.fz_counter is not None
               and (op.korder == prg.KORDER_FRAG or op.epi == prg.EPI_PHASE2)]
        assert not bad, bad
        assert any(op.kind == prg.OP_CONV and op.fz_counter is not None for op in big.ops)
    _check_program(prog, Emulator(prog, paramgen.make_spec_input(2, 21, 161, 8, 68)))
    # ... and cut out with random operands, the counter primed as if the other launches had arrived (what the GPU test does)
    rng = np.random.default_rng(3)
    seen = 0
    for op in fz:
        lop, arena = cr.cut_out(op, prog.weights, cr.random_inputs(op, rng))
        outs = cr.conv_ref(lop, arena)
        got = cr.conv_f32(lop, arena)
        cr.check(outs, got, got, op.name)
        assert outs["fz_counter"].val.max() == 0 and outs["fz_xf0"].must.all()
        seen += 1
    assert seen


# ------------------------------------------------------------------------------------------------------------------ (b)
@pytest.fixture(scope="module")
def bench_f32():
    return cr.lower_shape(cr.bench_shapes()[0])


def _pick(prog, pred, limit=3):
    """up to ``limit`` ops of distinct variant keys that satisfy pred"""
    seen, out = set(), []
    for op in prog.ops:
        if op.kind == prg.OP_CONV and pred(op) and cr.variant_key(op) not in seen:
            seen.add(cr.variant_key(op))
            out.append(op)
    assert out, "no op of the benchmark program has the property this mutation needs"
    # the smallest launches first: the CPU cost of a float64 reference grows with T * No * Kpad * N
    return sorted(out, key=lambda o: o.No * o.Kpad * o.N)[:limit]


def _case(prog, op, seed=0):
    rng = np.random.default_rng(seed)
    lop, arena = cr.cut_out(op, prog.weights, cr.random_inputs(op, rng, nutt=1))
    outs = cr.conv_ref(lop, arena)
    yard = cr.conv_f32(lop, arena)
    cr.check(outs, yard, yard, op.name)                  # the unmutated evaluation passes
    return lop, arena, outs, yard


def _rejected(outs, got, yard, what):
    with pytest.raises(AssertionError) as e:
        cr.check(outs, got, yard, what)
    print("rejected:", str(e.value)[:230])


def _weight_rows(lop, arena, wref, K):
    """(get, put) of a launch's weight matrix as [N][K] in the kernel's unit order, rows in the convolution's own order
    for the fragment form; the storage is fp32 except f16x3 (hi | lo halves per group of 4, zeroed together)"""
    n = lop.N * K
    store = arena["x"][wref.off:wref.off + n]
    if lop.korder == prg.KORDER_FRAG:
        dual = lop.epi in (prg.EPI_DUALGATE, prg.EPI_GLU)
        return prg.unpack_frag(store, lop.N, K, dual), lambda w: store.__setitem__(slice(None), prg.pack_frag(w, dual))
    return store.reshape(lop.N, K).copy(), lambda w: store.__setitem__(slice(None), w.reshape(-1))


def _tap_columns(lop, K, ntaps, j):
    upt16 = K // ntaps
    if lop.korder == prg.KORDER_CHUNK:
        return np.arange(K).reshape(upt16 // 16, ntaps, 16)[:, j].reshape(-1)
    return np.arange(j * upt16, (j + 1) * upt16)


def test_rejects_a_dropped_tap_for_one_output_column(bench_f32):
    progs = [bench_f32, cr.lower_shape(cr.bench_shapes()[1]), cr.lower_shape(cr.bench_shapes()[2])]
    n = 0
    for prog in progs:
        kinds = [lambda o: o.korder == prg.KORDER_TAP and len(o.dt) > 1, lambda o: o.korder == prg.KORDER_CHUNK and o.epi == prg.EPI_GLU,
                 lambda o: o.epi == prg.EPI_PHASE2]
        if prog is bench_f32:
            kinds.append(lambda o: o.korder == prg.KORDER_FRAG and len(o.dt) > 1)
        for pred in kinds:
            for op in _pick(prog, pred, 1):
                lop, arena, outs, yard = _case(prog, op)
                mut = {k: v.copy() for k, v in arena.items()}
                w, put = _weight_rows(lop, mut, lop.w, lop.Kpad)
                j = len(lop.dt) - 1 if lop.epi != prg.EPI_PHASE2 else 0
                w[:, _tap_columns(lop, lop.Kpad, len(lop.dt), j)] = 0.0
                put(w)
                # ... spliced into the honest result at ONE output position: time row T/2, the launch's middle column (no tap leaves [0, Fin) there)
                got = {k: v.copy() for k, v in yard.items()}
                shape = (lop.B, lop.T, lop.Fout, lop.Cout)
                fo = (lop.No // 2) * lop.ostride + lop.ophase
                cr.read(got, lop.dst, shape)[0, lop.T // 2, fo] = cr.read(cr.conv_f32(lop, mut), lop.dst, shape)[0, lop.T // 2, fo]
                _rejected(outs, got, yard, f"{op.name}: tap {j} dropped at one output position")
                n += 1
    assert n >= 9


def test_rejects_swapped_phases(bench_f32):
    for op in _pick(bench_f32, lambda o: o.epi == prg.EPI_PHASE2, 2) + _pick(bench_f32, lambda o: o.ph1_No > 0, 2):
        lop, arena, outs, yard = _case(bench_f32, op)
        got = {k: v.copy() for k, v in yard.items()}
        d = cr.read(got, lop.dst, (lop.B, lop.T, lop.Fout, lop.Cout))
        n1 = lop.Fout // 2
        even, odd = d[:, :, 0:2 * n1:2].copy(), d[:, :, 1:2 * n1:2].copy()
        d[:, :, 0:2 * n1:2], d[:, :, 1:2 * n1:2] = odd, even
        _rejected(outs, got, yard, f"{op.name}: phases swapped")


def test_rejects_a_missing_bias_on_the_last_row_of_a_ragged_tile(bench_f32):
    ops = _pick(bench_f32, lambda o: o.bias is not None and o.epi in (prg.EPI_LINEAR, prg.EPI_PHASE2) and (o.T * o.No) % o.bm != 0
                and o.ph1_No == 0, 3)
    for op in ops:
        lop, arena, outs, yard = _case(bench_f32, op)
        got = {k: v.copy() for k, v in yard.items()}
        d = cr.read(got, lop.dst, (lop.B, lop.T, lop.Fout, lop.Cout))
        bias = cr.read(arena, lop.bias, (lop.N,))
        if lop.epi == prg.EPI_PHASE2:       # last row (T-1, No-1) writes column 2(No-1): the packed "value" rows
            c = np.arange(lop.N // 2)
            d[0, -1, 2 * (lop.No - 1)] -= bias[(c // 32) * 64 + c % 32]
        else:
            d[0, -1, (lop.No - 1) * lop.ostride + lop.ophase] -= bias
        _rejected(outs, got, yard, f"{op.name}: bias missing on the last row")


def test_rejects_a_row_of_the_last_tile_left_at_its_poison_value(bench_f32):
    for op in _pick(bench_f32, lambda o: True, 4):
        lop, arena, outs, yard = _case(bench_f32, op)
        got = {k: v.copy() for k, v in yard.items()}
        d = cr.read(got, lop.dst, (lop.B, lop.T, lop.Fout, lop.Cout))
        d[0, -1, (lop.No - 1) * lop.ostride + lop.ophase] = np.nan
        _rejected(outs, got, yard, f"{op.name}: last row not written")
        got = {k: v.copy() for k, v in yard.items()}     # ... or at a stale finite value
        d = cr.read(got, lop.dst, (lop.B, lop.T, lop.Fout, lop.Cout))
        d[0, -1, (lop.No - 1) * lop.ostride + lop.ophase] = d[0, -2, (lop.No - 1) * lop.ostride + lop.ophase]
        _rejected(outs, got, yard, f"{op.name}: last row stale")


def test_rejects_a_tile_count_off_by_one(bench_f32):
    for op in _pick(bench_f32, lambda o: o.stats is not None, 4):
        lop, arena, outs, yard = _case(bench_f32, op)
        got = {k: v.copy() for k, v in yard.items()}
        st = cr.read(got, lop.stats, (lop.B, lop.stat_tiles, lop.nsets, lop.Cout, 4))
        st[0, lop.stat_tile0 + cr.launch_tiles(lop) - 1, 0, 0, 0] += 1
        _rejected(outs, got, yard, f"{op.name}: n of the last tile off by one")


def test_rejects_a_single_weight_rounded_to_bf16_in_an_fp32_launch(bench_f32):
    ops = (_pick(bench_f32, lambda o: o.precision == prg.PREC_F32 and o.korder == prg.KORDER_CHUNK and o.Kpad >= 768, 1)
           + _pick(bench_f32, lambda o: o.precision == prg.PREC_F32 and o.korder == prg.KORDER_FRAG, 2)
           + _pick(bench_f32, lambda o: o.precision == prg.PREC_F32 and o.korder == prg.KORDER_TAP, 1))
    for op in ops:
        lop, arena, outs, yard = _case(bench_f32, op)
        mut = {k: v.copy() for k, v in arena.items()}
        w = mut["x"][lop.w.off:lop.w.off + lop.N * lop.Kpad]
        # the weight the rounding moves most, and one of MEDIAN displacement among those it moves at all
        moved = np.abs(bf16_round(w) - w)
        live = np.nonzero(moved > 0)[0]
        order = live[np.argsort(moved[live])]
        for which, k in (("largest", int(order[-1])), ("median", int(order[len(order) // 2]))):
            mut = {k_: v.copy() for k_, v in arena.items()}
            wm = mut["x"][lop.w.off:lop.w.off + lop.N * lop.Kpad]
            wm[k] = bf16_round(wm[k:k + 1])[0]
            got = cr.conv_f32(lop, mut)
            if which == "median" and lop.Kpad >= 768:
                # where the comparator stops seeing this mutation: 2^-10 of ONE typical product out of 768 in one of 128
                # packed rows is below 8 x the fp32 yardstick of the whole tensor (and far below the per-element limit).
                # Pinned, so that a change of the comparator's sensitivity shows up here: still accepted, and no longer
                # accepted once the margin is a quarter of what it is
                _, ratio = cr.check(outs, got, yard, op.name)
                print(f"not seen: {op.name}: one weight of median displacement rounded to bf16 (K = {lop.Kpad}), L2 ratio {ratio:.2f}")
                with pytest.raises(AssertionError):
                    cr.check(outs, got, yard, op.name, margin=cr.MARGIN / 4)
                continue
            _rejected(outs, got, yard, f"{op.name}: one weight ({which} displacement) rounded to bf16")


# ------------------------------------------------------------------------------------------------------------------ (c)
def test_census_of_the_benchmark_variants():
    """Every (program, variant) bench.py's sections select is one the GPU test walks -- both come from
    conv_ref.bench_shapes / bench_variants / chosen_ops -- and the counts are pinned: a lowering change that adds a kernel
    variant has to show up here (and then in the table of DESIGN.md)."""
    shapes = cr.bench_shapes()
    assert [cr.shape_str(s) for s in shapes] == [
        "M8 B16 T401 f32", "M8 B16 T401 f16x3", "M8 B16 T401 bf16", "M8 B1 T401 f32", "M16 B1 T801 f32",
        "M16 BN B1 T801 f32", "M16 BN B1 T801 bf16", "M16 cLN B1 T801 f32", "M16 cLN B1 T801 bf16",
        "GaGNet B16 T401 f32", "GaGNet B16 T401 f16x3", "M8 B6 T601 f32", "M8 B6 T601 bf16",
        "GaGNet BN B1 T801 f32", "GaGNet B6 T601 f32", "GaGNet B6 T601 bf16"]
    enumerated = cr.bench_variants()
    walked, headline = set(), set()
    for i, s in enumerate(shapes):
        prog = cr.lower_shape(s)
        keys = {cr.variant_key(op) for op in prog.ops if op.kind == prg.OP_CONV}
        assert keys == set(enumerated[i]), f"{cr.shape_str(s)}: the lowering selects variants the GPU test does not enumerate"
        assert {k for k, _ in cr.chosen_ops(prog)} == keys
        walked |= keys
        if i < 5:
            headline |= keys
    small = set()
    for M, B, T, (p, q), prec in cr.PER_OP_SHAPES:
        cfg = NetConfig(M=M, p=p, q=q)
        small |= set(cr.variants_of(prg.lower(cfg, paramgen.make_params(param_specs(cfg), 50 + M), B, T, 161, precision=prec)))
    print(f"{len(headline)} variants at the five inference shapes ({len(headline - small)} not reached at the per-op shapes), "
          f"{len(walked)} over all sections")
    assert len(headline) == 61 and len(headline - small) == 36, sorted(cr.key_str(k) for k in headline)
    assert len(walked) == 126, sorted(cr.key_str(k) for k in walked)
    # the varlen lowering of the headline shape selects the same kernels (it only adds eab_time_window.lens)
    assert set(cr.variants_of(cr.lower_shape(shapes[0], varlen=True))) == set(enumerated[0])
