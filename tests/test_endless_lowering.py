"""Streams of any length, the host side (no GPU): the carry table the lowering derives for a streaming program (which
tensors some op reads at an earlier row, and how far back), the smallest resident window, the new entry point, and the
property the GPU tests lean on -- a window program and a long program pick the same kernel for every convolution."""
import ctypes
import os

import pytest

import paramgen
from eabnet_amd import _lib
from eabnet_amd import program as prg
from eabnet_amd.spec import GagConfig, NetConfig, gag_param_specs, param_specs

SMALL = dict(k1=(5, 3), p=2, q=2)


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in list(os.environ):
        if k.startswith("EAB_"):
            monkeypatch.delenv(k)


def _lower(cfg, B, T, **kw):
    specs = gag_param_specs(cfg) if isinstance(cfg, GagConfig) else param_specs(cfg)
    P = {k: v for k, v in paramgen.make_params(specs, 1).items() if specs[k].kind != "bn_count"}
    return prg.lower(cfg, P, B, T, 161, **kw)


def _reach(prog):
    """ref -> (floats per time row, rows back) of every tensor an op reads at an earlier row, from the tap tables and the
    LSTM ops alone"""
    need = {}
    for op in prog.ops:
        if op.kind == prg.OP_CONV:
            back = -min([0] + list(op.dt) + list(op.ph1_dt))
            for ref, C in ((op.src0, op.C0), (op.src1, op.C1)):
                if ref is not None and back > 0:
                    need[ref] = (op.Fin * C, max(back, need.get(ref, (0, 0))[1]))
        elif op.kind == prg.OP_LSTM64:
            need[op.h_out] = (op.F * 64, max(1, need.get(op.h_out, (0, 0))[1]))
    return need


CASES = {       # name: (config, chunk, history)
    "default_bn": (NetConfig(M=8, norm_type="BN"), 1, 128),
    "default_cln": (NetConfig(M=8, norm_type="cLN"), 1, 128),
    "small_c1": (NetConfig(M=8, norm_type="BN", **SMALL), 1, 8),
    "small_c4": (NetConfig(M=8, norm_type="BN", **SMALL), 4, 8),
    "small_c3": (NetConfig(M=8, norm_type="BN", **SMALL), 3, 9),
    "small_k13": (NetConfig(M=8, norm_type="BN", k1=(1, 3), p=2, q=2), 1, 8),
    "gag": (GagConfig(norm_type="BN"), 1, 18),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_carry_table_is_what_the_tap_tables_say(name):
    cfg, chunk, history = CASES[name]
    prog = _lower(cfg, 1, 300, chunk=chunk)
    assert prog.history == history and prog.history % chunk == 0
    assert prog.min_window == 2 * history + chunk
    need = _reach(prog)
    table = {ref: (row, rows) for ref, row, rows in prog.carry}
    assert len(table) == len(prog.carry), "a tensor is listed twice"
    assert set(table) == set(need), "the table lists exactly the tensors read at an earlier row"
    far = 0
    for ref, (row, rows) in need.items():
        assert table[ref][0] == row and rows <= table[ref][1] <= history, ref
        assert ref.arena != "a" or ref.off + prog.B * prog.T * row <= prog.act_floats, ref
        far = max(far, rows)
    assert history == max(1, -(-far // chunk) * chunk)
    # position-free state is not in the table
    for op in prog.ops:
        if op.kind == prg.OP_LSTM64:
            assert op.c_state not in table
        if op.kind == prg.OP_CLN_STATS:
            assert op.state not in table and op.sums not in table
    has_in = prg.Ref("in") in table
    if name != "gag":
        assert has_in and table[prg.Ref("in")] == (161 * 2 * 8, 1)      # the first gated convolution is (2, 5): one frame back
    else:
        assert not has_in and prg.Ref("in2") not in table               # the pack op reads its inputs at the current row only


def test_table_sizes_of_the_default_configuration():
    """the figures DESIGN.md §4.7 quotes (M = 8, F = 161, chunk 1)"""
    got = {}
    for name in ("default_bn", "default_cln", "small_c1"):
        prog = _lower(CASES[name][0], 1, 300, chunk=1)
        got[name] = (len(prog.carry), sum(4 * row * rows for _, row, rows in prog.carry))
    assert got == {"default_bn": (31, 363072), "default_cln": (49, 556608), "small_c1": (17, 345408)}


def test_offline_programs_carry_nothing():
    for cfg in (NetConfig(M=4, norm_type="BN", **SMALL), NetConfig(M=4, **SMALL), GagConfig(p=1, q=1)):
        prog = _lower(cfg, 1, 20)
        assert prog.carry == [] and prog.history == 0


def test_cln_state_holds_the_frame_count():
    """[B][2] running sums + [B] frames seen, per unit (include/eabnet_hip.h, eab_cln_stats_f32)"""
    B = 11
    prog = _lower(NetConfig(M=4, norm_type="cLN", **SMALL), B, 20, chunk=1)
    stats = [op for op in prog.ops if op.kind == prg.OP_CLN_STATS]
    offs = sorted(r.off for r in {op.state for op in stats} | {op.mr for op in stats})
    for op in stats:
        nxt = min(o for o in offs if o > op.state.off)
        assert nxt - op.state.off >= 6 * B, "3 doubles per utterance"


def test_entry_point_is_declared_exported_and_bound():
    assert _lib.ABI_VERSION == 10
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eabnet_hip.h")).read()
    assert "int eab_shift_rows_f32(const eab_shift_desc* dev_descs, int n, int B, int T, int src_pos, int H, eab_stream_t stream);" in hdr
    assert "#define EAB_ABI_VERSION 10" in hdr
    assert "eab_shift_rows_f32" in _lib.EXPORTS
    assert ctypes.sizeof(_lib.ShiftDesc) == 16
    lib = _lib.load()
    assert lib.eab_abi_version() == 10
    # argument checks happen on the host, before any launch: safe without a GPU
    assert lib.eab_shift_rows_f32(None, 1, 1, 17, 16, 8, None) == 1            # no table
    fake = ctypes.c_void_p(0x1000)
    assert lib.eab_shift_rows_f32(fake, 1, 1, 17, 15, 8, None) == 1            # source rows would overlap the destination
    assert lib.eab_shift_rows_f32(fake, 1, 1, 17, 18, 8, None) == 1            # source rows past the window
    assert lib.eab_shift_rows_f32(fake, 0, 1, 17, 16, 8, None) == 1
    assert lib.eab_shift_rows_f32(fake, 1, 1, 17, 16, 0, None) == 1


# (name of the pairs, B, M, config keywords, precision, chunk, window T, long T): every pair the GPU tests compare bit for bit
PAIRS = [("small_bn_c1", 2, 4, dict(norm_type="BN", p=2, q=2), "f32", 1, 17, 173),
         ("small_cln_c1", 2, 4, dict(norm_type="cLN", p=2, q=2), "f32", 1, 17, 173),
         ("small_bf16_c1", 2, 4, dict(norm_type="BN", p=2, q=2), "bf16", 1, 17, 173),
         ("small_bn_c4", 2, 4, dict(norm_type="BN", p=2, q=2), "f32", 4, 20, 203),
         ("small_cln_c4", 2, 4, dict(norm_type="cLN", p=2, q=2), "f32", 4, 20, 203),
         ("small_bf16_c4", 2, 4, dict(norm_type="BN", p=2, q=2), "bf16", 4, 20, 203),
         ("default_m4", 1, 4, dict(norm_type="BN"), "f32", 1, 257, 700),
         ("default_m16", 1, 16, dict(norm_type="BN"), "f32", 1, 257, 801),
         ("default_m16_bf16", 1, 16, dict(norm_type="BN"), "bf16", 1, 257, 801),
         ("two_stage_first_c1", 2, 4, dict(norm_type="BN", p=1, q=1), "f32", 1, 9, 31),
         ("two_stage_first_c2", 2, 4, dict(norm_type="BN", p=1, q=1), "f32", 2, 10, 31),
         ("two_stage_second_c1", 2, None, dict(norm_type="BN", p=1, q=1, dilas=(1, 2)), "f32", 1, 9, 31),
         ("two_stage_second_c2", 2, None, dict(norm_type="BN", p=1, q=1, dilas=(1, 2)), "f32", 2, 10, 31)]


@pytest.mark.parametrize("env", [{}, {"EAB_ST": "0", "EAB_BM": "64"}], ids=["default", "st0_bm64"])
@pytest.mark.parametrize("pair", PAIRS, ids=[p[0] for p in PAIRS])
def test_window_and_long_programs_pick_the_same_kernels(pair, env, monkeypatch):
    """Tile and kernel choices follow (B, T) and two kernels sum in different orders, so the bit-for-bit comparisons of
    tests/test_endless_gpu.py hold only if the window program and the long program choose alike."""
    _, B, M, kw, precision, chunk, T_win, T_long = pair
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = GagConfig(**kw) if M is None else NetConfig(M=M, **kw)
    a, b = (_lower(cfg, B, T, chunk=chunk, precision=precision) for T in (T_win, T_long))
    assert T_win == a.min_window == b.min_window
    ca, cb = ([(op.name, op.korder, op.bm, op.precision) for op in p.ops if op.kind == prg.OP_CONV] for p in (a, b))
    assert len(ca) == len(cb) and len(ca) > 10
    assert [x for x, y in zip(ca, cb) if x != y] == []
    assert [(r.arena, row, rows) for r, row, rows in a.carry] == [(r.arena, row, rows) for r, row, rows in b.carry]
