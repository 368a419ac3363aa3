"""The eab_op arrays the host encodes (eabnet_amd/runtime.encode) pinned on the CPU: inference, streaming, varlen and
training programs are lowered, encoded against fixed arena base addresses and compared by sha256 with
tests/golden/op_encoding.json, recorded from the per-class encoders this encoder replaced.  The fused form of a streaming
step (runtime.fuse_step, planned by the library's host-side chain planner) is pinned the same way, and its shape case by case."""
import ctypes as C
import hashlib
import json
import os

import pytest

import paramgen
from eabnet_amd import program as prg
from eabnet_amd import runtime, train, train_gag
from eabnet_amd.spec import GagConfig, NetConfig, gag_param_specs, param_specs

# one base per arena, with distinct high bits, so that a pointer into the wrong arena changes the digest
BASES = {"w": 0x1000_0000_0000, "a": 0x2000_0000_0000, "in": 0x3000_0000_0000, "out": 0x4000_0000_0000,
         "in2": 0x5000_0000_0000, "dout": 0x6000_0000_0000, "g": 0x7000_0000_0000, "chain": 0xA000_0000_0000}
T_POS, LENS = 0x8000_0000_0000, 0x9000_0000_0000


def E(**kw):
    return NetConfig(M=8, **kw)


INFER = {               # name: (config, B, T, lower() keywords)
    "eab_f32": (E(), 2, 6, {}),
    "eab_f16x3": (E(), 2, 6, {"precision": "f16x3"}),
    "eab_bf16": (E(), 2, 6, {"precision": "bf16"}),
    "eab_dump_bfw": (E(), 1, 5, {"dump_bfw": True}),
    "eab_varlen": (E(), 2, 6, {"varlen": True}),
    "eab_bn": (E(norm_type="BN"), 2, 6, {}),
    "eab_cln": (E(norm_type="cLN"), 2, 6, {}),
    "eab_noncausal": (E(is_causal=False), 2, 6, {}),
    "eab_miso": (E(topo_type="miso"), 2, 6, {}),
    "eab_cnn_bn_noncausal": (E(bf_type="cnn", norm_type="BN", is_causal=False), 2, 6, {}),
    "eab_stream_cln_c1": (E(norm_type="cLN"), 2, 8, {"chunk": 1}),
    "eab_stream_bn_c4": (E(norm_type="BN"), 2, 8, {"chunk": 4}),
    "gag_chains": (GagConfig(), 1, 6, {"parallel_chains": True}),
    "gag_serial": (GagConfig(), 1, 6, {"parallel_chains": False}),
    "gag_varlen": (GagConfig(), 2, 6, {"varlen": True}),
    "gag_stream_bn_c2": (GagConfig(norm_type="BN"), 1, 6, {"chunk": 2}),
}
TRAIN = {               # name: (config, B, T, precision)
    "train_eab_f32": (E(), 2, 6, "f32"),
    "train_eab_bf16": (E(), 2, 6, "bf16"),
    "train_eab_bn": (E(norm_type="BN"), 2, 6, "f32"),
    "train_eab_cln": (E(norm_type="cLN"), 2, 6, "f32"),
    "train_eab_cnn_miso": (E(bf_type="cnn", topo_type="miso"), 2, 6, "f32"),
    "train_gag_f32": (GagConfig(), 1, 6, "f32"),
    "train_gag_bf16": (GagConfig(), 1, 6, "bf16"),
}


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "op_encoding.json")) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in list(os.environ):
        if k.startswith("EAB_"):
            monkeypatch.delenv(k)


def _digest(arr) -> dict:
    return {"ops": len(arr), "sha256": hashlib.sha256(bytes(arr)).hexdigest()}


def test_cases_cover_the_golden_file(golden):
    assert set(golden) == set(INFER) | set(TRAIN)


def _lowered(cfg, B, T, **kw):
    """(program, its encoded array, the chain planner on that array)"""
    specs = gag_param_specs(cfg) if isinstance(cfg, GagConfig) else param_specs(cfg)
    P = {k: v for k, v in paramgen.make_params(specs, 1).items() if specs[k].kind != "bn_count"}
    prog = prg.lower(cfg, P, B, T, 161, **kw)
    bases = dict(BASES, in2=BASES["in2"] if isinstance(cfg, GagConfig) else None)
    win = dict(t_pos=T_POS if prog.chunk else None, chunk=prog.chunk, lens=LENS if prog.varlen else None)
    arr = runtime.encode(prog.ops, bases, **win)
    return prog, arr, bases, win


@pytest.mark.parametrize("name", sorted(INFER))
def test_inference_encoding(golden, name):
    """"run": the program's own array; "fused": the array a whole streaming step runs, where the step has fused launches"""
    cfg, B, T, kw = INFER[name]
    prog, arr, bases, win = _lowered(cfg, B, T, **kw)
    got = {"run": _digest(arr)}
    fused = runtime.fuse_step(prog.ops, prog.chunk, True, True, runtime.chain_planner(arr))
    if len(fused) < len(prog.ops):
        got["fused"] = _digest(runtime.encode([op for op, _, _ in fused], bases, **win))
    assert got == golden[name]


M4 = dict(M=4, norm_type="BN", p=2, q=2)
FUSED = {               # name: (config, B, T, chunk, program ops, chains [(first, count)], cLN steps, entries)
    "cln_c1": (E(norm_type="cLN"), 2, 8, 1, 377, [], 104, 273),
    "cln_c4": (E(norm_type="cLN"), 2, 8, 4, 377, [], 0, 377),
    "bn_c4": (E(norm_type="BN"), 2, 8, 4, 102, [(31, 37)], 0, 66),
    "bn_c1": (E(norm_type="BN"), 2, 8, 1, 102, [(31, 37)], 0, 66),
    "bn_m4_c16": (NetConfig(**M4), 2, 32, 16, 74, [(31, 9)], 0, 66),
    "bn_m4_c17": (NetConfig(**M4), 2, 34, 17, 74, [], 0, 74),            # a tile no longer holds the chunk
    "gag_bn_c2": (GagConfig(norm_type="BN"), 1, 6, 2, 202, [], 0, 202),
}


@pytest.mark.parametrize("name", sorted(FUSED))
def test_fused_step_shape(name, monkeypatch):
    """What runtime.fuse_step makes of a streaming program (figures: the hand-written pass it replaced, on the same
    programs): which runs become one chain launch, how many cLN pairs one step launch, and that every entry stands for
    exactly the program ops of its range -- with both fusions, with each switched off, and as model._Bound reads the knobs."""
    import torch
    from eabnet_amd import _lib, model
    cfg, B, T, chunk, n_ops, chains, n_steps, n_entries = FUSED[name]
    prog, arr, bases, win = _lowered(cfg, B, T, chunk=chunk)
    ops = prog.ops
    assert len(ops) == n_ops
    plan = runtime.chain_planner(arr)

    def shape(fused):
        return ([(f, c) for op, f, c in fused if op.kind == prg.OP_CONV_CHAIN], sum(op.kind == prg.OP_CLN_STEP for op, _, _ in fused),
                len(fused))
    fused = runtime.fuse_step(ops, chunk, True, True, plan)
    assert shape(fused) == (chains, n_steps, n_entries)
    if n_steps:
        assert n_steps == sum(op.kind == prg.OP_CLN_STATS for op in ops)
    for first, count in chains:
        stcn = [k for k, op in enumerate(ops) if op.kind == prg.OP_CONV and op.name.startswith("stcns.")]
        assert stcn == list(range(first, first + count))
    n_chained = sum(c - 1 for _, c in chains)
    assert shape(runtime.fuse_step(ops, chunk, False, True, plan)) == ([], n_steps, len(ops) - n_steps)
    assert shape(runtime.fuse_step(ops, chunk, True, False, plan)) == (chains, 0, len(ops) - n_chained)
    assert shape(runtime.fuse_step(ops, chunk, False, False, plan)) == ([], 0, len(ops))
    assert shape(runtime.fuse_step(ops, 0, True, True, plan)) == ([], 0, len(ops))
    # the ranges partition the program in order, and every entry is (made of) the ops of its range
    tables = runtime.chain_tables(arr, fused)
    nxt = 0
    for op, first, count in fused:
        assert first == nxt and count >= 1
        nxt += count
        if op.kind == prg.OP_CONV_CHAIN:
            assert (op.n, op.B, len(op.plan)) == (count, B, count) and op.descs.arena == op.codes.arena == "chain"
            assert all(o.kind == prg.OP_CONV and o.korder == prg.KORDER_FRAG for o in ops[first:first + count])
            size = C.sizeof(_lib.ConvDesc)
            for t in range(count):
                assert tables[4 * op.descs.off + t * size:][:size] == bytes(arr[first + t].conv)
            assert tables[4 * op.codes.off:][:4 * count] == bytes((C.c_int * count)(*op.plan))
            assert plan(first, count) == (list(op.plan), op.lds_bytes, op.bf16)
        elif op.kind == prg.OP_CLN_STEP:
            a, b = ops[first:first + count]
            assert (a.kind, b.kind) == (prg.OP_CLN_STATS, prg.OP_CLN_APPLY) and op.win
            assert (op.x, op.stat_slope, op.sums, op.state, op.mr, op.eps) == (a.x, a.slope, a.sums, a.state, a.mr, a.eps)
            assert (op.x, op.mr, op.gain, op.bias, op.slope, op.add, op.out) == (b.x, b.mr, b.gain, b.bias, b.slope, b.add, b.out)
            assert (op.B, op.T, op.P, op.C, op.mode) == (b.B, b.T, b.P, b.C, b.mode) == (a.B, a.T, a.P, a.C, b.mode)
        else:
            assert count == 1 and op is ops[first]
    assert nxt == len(ops)
    if not chains:
        assert tables == b""
    # the bound program reads the two knobs from the environment and runs the plain array when nothing is fused
    for env, want in (({}, fused), ({"EAB_ST_CHAIN": "0"}, runtime.fuse_step(ops, chunk, False, True, plan)),
                      ({"EAB_CLN_STEP": "0"}, runtime.fuse_step(ops, chunk, True, False, plan))):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            bound = model._Bound(prog, torch.device("cpu"))
            bound.bind(BASES["in"], BASES["out"], bases["in2"])
        if len(want) == len(ops):
            assert bound.fused is None and bound.exec_ops is None and bound.chains == []
        else:
            assert [(type(op), f, c) for op, f, c in bound.fused] == [(type(op), f, c) for op, f, c in want]
            assert len(bound.exec_ops) == len(want) and bound.chains == shape(want)[0]


@pytest.mark.parametrize("name", sorted(TRAIN))
def test_training_encoding(golden, name):
    cfg, B, T, precision = TRAIN[name]
    prog = (train_gag if isinstance(cfg, GagConfig) else train).lower_train(cfg, B, T, 161, precision)
    bases = dict(BASES, in2=BASES["in2"] if prog.has_in2 else None)
    got = {which: _digest(runtime.encode(ops, bases)) for which, ops in (("fwd", prog.fwd), ("bwd", prog.bwd))}
    assert got == golden[name]
