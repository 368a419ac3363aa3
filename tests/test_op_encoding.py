"""The eab_op arrays the host encodes (eabnet_amd/runtime.encode) pinned on the CPU: inference, streaming, varlen and
training programs are lowered, encoded against fixed arena base addresses and compared by sha256 with
tests/golden/op_encoding.json, recorded from the per-class encoders this encoder replaced."""
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
         "in2": 0x5000_0000_0000, "dout": 0x6000_0000_0000, "g": 0x7000_0000_0000}
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


@pytest.mark.parametrize("name", sorted(INFER))
def test_inference_encoding(golden, name):
    cfg, B, T, kw = INFER[name]
    specs = gag_param_specs(cfg) if isinstance(cfg, GagConfig) else param_specs(cfg)
    P = {k: v for k, v in paramgen.make_params(specs, 1).items() if specs[k].kind != "bn_count"}
    prog = prg.lower(cfg, P, B, T, 161, **kw)
    bases = dict(BASES, in2=BASES["in2"] if isinstance(cfg, GagConfig) else None)
    arr = runtime.encode(prog.ops, bases, t_pos=T_POS if prog.chunk else None, chunk=prog.chunk,
                         lens=LENS if prog.varlen else None)
    assert {"run": _digest(arr)} == golden[name]


@pytest.mark.parametrize("name", sorted(TRAIN))
def test_training_encoding(golden, name):
    cfg, B, T, precision = TRAIN[name]
    prog = (train_gag if isinstance(cfg, GagConfig) else train).lower_train(cfg, B, T, 161, precision)
    bases = dict(BASES, in2=BASES["in2"] if prog.has_in2 else None)
    got = {which: _digest(runtime.encode(ops, bases)) for which, ops in (("fwd", prog.fwd), ("bwd", prog.bwd))}
    assert got == golden[name]
