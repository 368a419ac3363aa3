#!/usr/bin/env python
"""What the end of the training step costs: clip_grad_norm_ + torch.optim.Adam against eabnet_amd.FlatAdam (csrc/optim.hip).

    python tools/bench_optim.py [--repeats 3] [--blocks 3] [--block-steps 6] [--configs beam_former_f32,...] [--out profiles/optim_bench.json]

Workload: the training step of bench.py's train_measure -- B = 6 utterances of 6 s, 8 microphones, prepare_data -> forward ->
loss -> backward -> clip at 1.0 -> Adam(5e-4) -- for the beam-former alone and the two-stage model, fp32 and bf16 products.
Per configuration two copies of the model from the same seed live in ONE process:
    (a) "torch"  clip_grad_norm_ + torch.optim.Adam: the behaviour without this optimizer, unchanged
    (b) "flat"   FlatAdam(max_grad_norm=1.0)
Both are warmed up, then measured in alternating blocks of ``block-steps`` steps; the whole run is repeated ``repeats`` times and
the spread is that of the repeats' medians.  Every step ends in a synchronise and is timed with the host clock around it.  Inside
a step: the optimizer phase (clip + step) between two HIP events (device time) and its host enqueue time (host clock, no
synchronise inside), and the host time of TrainFn.forward from its entry to the end of the weight pack's enqueue, which is where
torch.cat goes (summed over the stages).  "host_ms" times the flat path's own host walks alone: the walk over parameters and
gradients in step(), the flat parameter view of the first stage's forward, the version bump of all parameters.  Launches of
the optimizer phase: counted by FlatAdam itself (opt.stats) for (b); for (a) none is counted here (a kernel trace run of its
own would).

Prints one JSON object (and writes it to --out when given)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import eabnet_amd  # noqa: E402
from eabnet_amd import train as tr  # noqa: E402

B, SECONDS = 6, 6.0
_mark = {"t0": None, "host": 0.0}


def _instrument():
    """host clock from TrainFn.forward's first statement (flat_parameter_view) to the return of TrainBound.pack"""
    view, pack = tr.flat_parameter_view, tr.TrainBound.pack

    def timed_view(params):
        _mark["t0"] = time.perf_counter()
        return view(params)

    def timed_pack(self, flat, stream):
        pack(self, flat, stream)
        _mark["host"] += time.perf_counter() - _mark["t0"]

    tr.flat_parameter_view, tr.TrainBound.pack = timed_view, timed_pack


def _model(two_stage: bool, precision: str, dev):
    net, _ = bench.make_model(bench.MICS, dev)
    net.train()
    net.precision = precision
    if not two_stage:
        return net
    pa = argparse.Namespace(
        k1=(2, 3), k2=(1, 3), c=64, M=bench.MICS, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=6, q=3, is_causal=True, is_u2=True,
        bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="IN", ref_mic=0, freeze_eabnet=False,
        gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=2,
        gagnet_q=3, gagnet_dilas=[1, 2, 5, 9], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=True,
        gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="IN")
    torch.manual_seed(1)
    two = eabnet_amd.make_eabnet_with_postnet(pa).to(dev).train()
    two.eabnet.load_state_dict(net.state_dict(), strict=True)
    two.eabnet.precision = two.postnet.precision = precision
    return two


class Variant:
    def __init__(self, name: str, two_stage: bool, precision: str, dev):
        self.name, self.two_stage = name, two_stage
        self.net = _model(two_stage, precision, dev)
        self.params = list(self.net.parameters())
        if name == "flat":
            self.opt = eabnet_amd.FlatAdam(self.params, lr=5e-4, max_grad_norm=1.0)
        else:
            self.opt = torch.optim.Adam(self.params, lr=5e-4)
        self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        self.rows = []

    def step(self, wav, tgt, pd_args, frames, dev, record: bool):
        torch.cuda.synchronize()
        _mark["host"] = 0.0
        t0 = time.perf_counter()
        self.opt.zero_grad(set_to_none=True)
        noisy, target = eabnet_amd.prepare_data(wav, tgt, dev, pd_args)
        if self.two_stage:
            loss = eabnet_amd.eabnet_with_postnet_loss(self.net(noisy), target, frames)["final"]
        else:
            loss = eabnet_amd.com_mag_mse_loss(self.net(noisy), target, frames)
        loss.backward()
        self.ev[0].record()
        h0 = time.perf_counter()
        if self.name == "torch":
            torch.nn.utils.clip_grad_norm_(self.params, 1.0)
        self.opt.step()
        h1 = time.perf_counter()
        self.ev[1].record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if record:
            self.rows.append((1e3 * (t1 - t0), self.ev[0].elapsed_time(self.ev[1]), 1e3 * (h1 - h0), 1e3 * _mark["host"]))
        return loss


def _host_ms(fn, n=50):
    fn()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return 1e3 * (time.perf_counter() - t0) / n


view_of = tr.flat_parameter_view                     # (the uninstrumented function)


def _median_columns(rows):
    return [statistics.median(r[k] for r in rows) for k in range(4)]


def measure(two_stage: bool, precision: str, dev, repeats: int, blocks: int, block_steps: int, warmup: int) -> dict:
    L = int(SECONDS * bench.SR)
    T = 1 + L // bench.HOP
    pd_args = argparse.Namespace(mics=bench.MICS, sr=bench.SR, wav_len=SECONDS, win_size=0.020, win_shift=0.010, fft_num=bench.N_FFT)
    wav, tgt = bench.synth_waves(B, bench.MICS, L, 1234).to(dev), bench.synth_waves(B, 1, L, 4321).to(dev)
    variants = [Variant("torch", two_stage, precision, dev), Variant("flat", two_stage, precision, dev)]
    for v in variants:
        for _ in range(warmup):
            loss = v.step(wav, tgt, pd_args, [T] * B, dev, False)
    per_repeat = {v.name: [] for v in variants}
    for _ in range(repeats):
        for v in variants:
            v.rows = []
        for _ in range(blocks):
            for v in variants:
                for _ in range(block_steps):
                    loss = v.step(wav, tgt, pd_args, [T] * B, dev, True)
                assert bool(torch.isfinite(loss)), "training diverged"
        for v in variants:
            per_repeat[v.name].append(_median_columns(v.rows))
    flat = variants[1].opt
    assert flat.last_path == "flat" and flat.stats["gathered"] == 0 and flat.stats["reflattened"] == 0, flat.stats
    out = {"elements": sum(p.numel() for p in variants[0].params), "parameters": len(variants[0].params),
           "steps_per_variant_and_repeat": blocks * block_steps}
    names = ("ms_per_step", "optimizer_device_ms", "optimizer_host_enqueue_ms", "forward_host_ms_until_weights_packed")
    for v in variants:
        cols = list(zip(*per_repeat[v.name]))
        out[v.name] = {n: {"median": statistics.median(c), "min": min(c), "max": max(c)} for n, c in zip(names, cols)}
    steps = flat.stats["flat"]
    out["flat"]["optimizer_launches_per_step"] = flat.stats["launches"] / steps
    out["flat"]["gradient_segments"] = flat.last_segments
    out["flat"]["forwards_without_cat"] = [next(iter(m._train_bound.values())).flat_param_hits
                                           for m in ((variants[1].net.eabnet, variants[1].net.postnet) if two_stage else (variants[1].net,))]
    # the host walks of the flat path alone (inside the enqueue and forward figures above), on this model's parameters
    f, fps = flat._flat[0], variants[1].params
    grads = [p.grad for p in f.params]
    stage = [p for p in (variants[1].net.eabnet if two_stage else variants[1].net).parameters()]
    out["flat"]["host_ms"] = {"step_walk_over_parameters_and_gradients": _host_ms(lambda: flat._walk(f, grads)),
                              "forward_flat_parameter_view_first_stage": _host_ms(lambda: view_of(stage)),
                              "version_bump_of_all_parameters": _host_ms(lambda: torch.autograd.graph.increment_version(fps))}
    a, b = out["torch"]["ms_per_step"], out["flat"]["ms_per_step"]
    out["flat_minus_torch_ms"] = b["median"] - a["median"]
    out["spread_ms"] = max(a["max"] - a["min"], b["max"] - b["min"])
    out["not_slower_beyond_spread"] = bool(b["median"] <= a["median"] + out["spread_ms"])
    del variants
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--block-steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="beam_former_f32,beam_former_bf16,two_stage_f32,two_stage_bf16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _instrument()
    res = {"workload": f"training step, B {B}, {SECONDS:g} s, {bench.MICS} microphones; clip at 1.0, Adam(5e-4)",
           "method": "two model copies in one process, alternating blocks after warm-up of both; per step a host clock around a step "
                     "that ends in a synchronise; medians per repeat, min/max over the repeats",
           "repeats": a.repeats, "blocks": a.blocks, "block_steps": a.block_steps, "configs": {}}
    for key in a.configs.split(","):
        kind, prec = key.rsplit("_", 1)
        res["configs"][key] = measure(kind == "two_stage", prec, dev, a.repeats, a.blocks, a.block_steps, a.warmup)
        print(key, json.dumps(res["configs"][key]), file=sys.stderr, flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
