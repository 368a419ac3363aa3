"""What a lowered program hands to the device, reduced to a JSON-able record: the encoded eab_op arrays and everything the
arenas are filled from.  tests/golden/make_program_images.py records these in tests/golden/program_images.json from the commit
a lowering rewrite starts from; tests/test_program_images.py re-lowers and compares.  Arrays are recorded as sha256 over dtype,
shape and bytes, tables (lanes, sync, carry ...) as sha256 over their canonical JSON text, scalars as they are.

Cases: every case of tests/test_op_encoding.py; the toy network once under each lowering knob alone (each selects an emission
path the knob-free cases never reach); every program of conv_ref.bench_shapes() plus the varlen lowering of the first (the only
places where 128-row tiles, the patch pipeline and the phase-pair launch are chosen); the training programs bench.py runs."""
from __future__ import annotations

import contextlib
import hashlib
import json
import os
from typing import Callable, Dict

import numpy as np

import conv_ref
import test_op_encoding as enc
from eabnet_amd import program as prg
from eabnet_amd import runtime, train, train_gag
from eabnet_amd.spec import GagConfig, NetConfig

INFER_KNOBS = ("EAB_ST=0", "EAB_ST_GLU=0", "EAB_ST_FUSE=0", "EAB_PATCH=0", "EAB_PHASE2=0", "EAB_FUSE_FIN=1")
TRAIN_KNOBS = (("train_eab_bf16", "EAB_BF16_STORE=0"), ("train_eab_f32", "EAB_ST=0"))


def _sha(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()


def _array(a) -> str:
    a = np.ascontiguousarray(a)
    return _sha(f"{a.dtype.str}{a.shape}".encode() + a.tobytes())


def _plain(v):
    if isinstance(v, prg.Ref):
        return [v.arena, v.off]
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in sorted(v.items(), key=lambda kv: str(kv[0]))}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def _table(v) -> str:
    return _sha(json.dumps(_plain(v), sort_keys=True).encode())


def _ops(ops, prog, has_in2: bool) -> dict:
    bases = dict(enc.BASES, in2=enc.BASES["in2"] if has_in2 else None)
    chunk, varlen = getattr(prog, "chunk", 0), getattr(prog, "varlen", False)
    arr = runtime.encode(ops, bases, t_pos=enc.T_POS if chunk else None, chunk=chunk, lens=enc.LENS if varlen else None)
    return {"ops": len(arr), "sha256": _sha(bytes(arr))}


def inference_image(prog: prg.Program) -> dict:
    return {"ops": _ops(prog.ops, prog, isinstance(prog.cfg, GagConfig)), "weights": _array(prog.weights),
            "act_floats": prog.act_floats, "flops": prog.flops, "lanes": _table(prog.lanes), "sync": _table(prog.sync),
            "zero_init": _table(prog.zero_init), "carry": _table(prog.carry), "history": prog.history}


def training_image(prog: train.TrainProgram) -> dict:
    return {"fwd": _ops(prog.fwd, prog, prog.has_in2), "bwd": _ops(prog.bwd, prog, prog.has_in2), "ia": _array(prog.ia),
            "ib": None if prog.ib is None else _array(prog.ib), "inv": _array(prog.inv), "a_floats": prog.a_floats,
            "w_floats": prog.w_floats, "g_floats": prog.g_floats, "flops_fwd": prog.flops_fwd, "flops_bwd": prog.flops_bwd,
            "lanes": _table(prog.lanes), "sync": _table(prog.sync), "bn_layers": _table(prog.bn_layers),
            "grad_taps": _table(prog.grad_taps)}


@contextlib.contextmanager
def knobs(setting: str = ""):
    """the environment with no EAB_ knob set but `setting` ("NAME=value")"""
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("EAB_")}
    if setting:
        name, value = setting.split("=")
        os.environ[name] = value
    try:
        yield
    finally:
        for k in [k for k in os.environ if k.startswith("EAB_")]:
            del os.environ[k]
        os.environ.update(saved)


def _infer(name: str, knob: str = "") -> Callable[[], dict]:
    def run():
        cfg, B, T, kw = enc.INFER[name]
        with knobs(knob):
            return inference_image(enc._lowered(cfg, B, T, **kw)[0])
    return run


def _train(cfg, B: int, T: int, precision: str, knob: str = "") -> Callable[[], dict]:
    def run():
        with knobs(knob):
            return training_image((train_gag if isinstance(cfg, GagConfig) else train).lower_train(cfg, B, T, 161, precision))
    return run


def _bench(shape: dict, varlen: bool = False) -> Callable[[], dict]:
    def run():
        with knobs():
            return inference_image(conv_ref.lower_shape(shape, varlen))
    return run


def cases() -> Dict[str, Callable[[], dict]]:
    """name -> a function that lowers the case and returns its image"""
    out: Dict[str, Callable[[], dict]] = {name: _infer(name) for name in enc.INFER}
    out.update({name: _train(*enc.TRAIN[name]) for name in enc.TRAIN})
    out.update({f"eab_f32 {k}": _infer("eab_f32", k) for k in INFER_KNOBS})
    out.update({f"{name} {k}": _train(*enc.TRAIN[name], knob=k) for name, k in TRAIN_KNOBS})
    shapes = conv_ref.bench_shapes()
    for i, s in enumerate(shapes):
        out[f"bench {i}: {conv_ref.shape_str(s)}"] = _bench(s)
    out[f"bench 0 varlen: {conv_ref.shape_str(shapes[0])}"] = _bench(shapes[0], True)
    # the training section of bench.py: its batch is the last beam-former shape of bench_shapes(), its post-filter the last
    # GaGNet shape; both in fp32 and bf16
    tb = [s for s in shapes if "gag" not in s and "kw" not in s][-1]
    tg = [s for s in shapes if "gag" in s][-1]
    gcfg = GagConfig(cin=2, **{k: (tuple(v) if isinstance(v, list) else v) for k, v in tg["gag"].items()})
    for p in ("f32", "bf16"):
        out[f"bench train M{tb['M']} B{tb['B']} T{tb['T']} {p}"] = _train(NetConfig(M=tb["M"]), tb["B"], tb["T"], p)
        out[f"bench train GaGNet B{tg['B']} T{tg['T']} {p}"] = _train(gcfg, tg["B"], tg["T"], p)
    return out
