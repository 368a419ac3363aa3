#!/usr/bin/env python
"""What the multi-resolution STFT term costs: alone (value plus gradient), in the training step, and against the same loss written
with torch.stft under autograd on the device.

    python tools/bench_spec_loss.py [--repeats 3] [--blocks 3] [--block-steps 6] [--precisions f32,bf16] [--out profiles/spec_loss_bench.json]

Workload: B = 6 utterances of 6 s (est rows of 95,840 samples against clean rows of 96,000: unequal, as a loader's), the default
resolutions.
  term      value + gradient of mr_stft_loss on a leaf wave: device time between two HIP events and host enqueue time (host clock,
            no synchronise inside) per call, medians of ``--term-iters`` calls per repeat; the entry points alone on preallocated
            buffers (per-launch device times: the value's R + 1 launches, the gradient's R + 1 launches)
  operator  the same loss written with torch.stft / clamp / sqrt / log under autograd on the device (tests/mrstft_ref.torch_loss
            restated here per utterance -- the operator stand-in: in this tool only, never in the package), timed the same way
  step      the training step of bench.py's train_measure (configs[3]: prepare_data -> forward -> loss -> backward ->
            FlatAdam(5e-4, max_grad_norm=1.0)) on two copies of the model in one process, alternating blocks:
            (a) com_mag_mse_loss alone, (b) the same plus 0.5 * mr_stft_loss(istft(out), target)
The whole run is repeated ``repeats`` times; the spread is that of the repeats' medians.

Prints one JSON object (and writes it to --out when given)."""
from __future__ import annotations

import argparse
import ctypes as C
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
from eabnet_amd import _lib, wave  # noqa: E402

B, SECONDS, WEIGHT = 6, 6.0, 0.5
RES = wave.MR_RESOLUTIONS


def _stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def operator_loss(est, clean, floor=1e-7):
    """the definition in torch operators on the device, per utterance norms as in the package"""
    total = 0.0
    for n_fft, hop, win in RES:
        w = torch.hann_window(win, device=est.device)
        P = [torch.clamp(torch.view_as_real(torch.stft(x, n_fft, hop, win, w, center=True, pad_mode="reflect",
                                                       return_complex=True)).square().sum(-1), min=floor) for x in (est, clean)]
        E, S = torch.sqrt(P[0]), torch.sqrt(P[1])
        sc = torch.sqrt((S - E).square().sum((1, 2))) / torch.sqrt(S.square().sum((1, 2)))
        lm = (torch.log(S) - torch.log(E)).abs().mean((1, 2))
        total = total + sc + lm
    return (total / len(RES)).mean()


def term(dev, repeats: int, iters: int) -> dict:
    L = int(SECONDS * bench.SR)
    n = bench.HOP * (L // bench.HOP - 1)                          # a hop shorter than the clean rows
    g = torch.Generator().manual_seed(7)
    clean = (0.1 * torch.randn(B, 1, L, generator=g)).to(dev)
    est = (clean[:, 0, :n] + 0.05 * torch.randn(B, n, generator=g).to(dev)).contiguous()

    def fused():
        leaf = est.detach().requires_grad_(True)
        eabnet_amd.mr_stft_loss(leaf, clean).backward()
        return leaf.grad

    def operator():
        leaf = est.detach().requires_grad_(True)
        operator_loss(leaf, clean[:, 0, :n]).backward()
        return leaf.grad

    gf, go = fused(), operator()
    agree = float((gf - go).abs().max() / go.abs().max())

    def timed(fn):
        for _ in range(5):
            fn()
        dev_ms, host_ms = [], []
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(iters):
            torch.cuda.synchronize()
            a.record()
            h0 = time.perf_counter()
            fn()
            h1 = time.perf_counter()
            b.record()
            torch.cuda.synchronize()
            dev_ms.append(a.elapsed_time(b))
            host_ms.append(1e3 * (h1 - h0))
        return statistics.median(dev_ms), statistics.median(host_ms)

    rows = {"fused": [], "operator": []}
    for _ in range(repeats):
        rows["fused"].append(timed(fused))
        rows["operator"].append(timed(operator))
    out = {k: {"device_ms": _stats([r[0] for r in v]), "host_enqueue_ms": _stats([r[1] for r in v])} for k, v in rows.items()}
    out["gradient_max_diff_over_max_fused_vs_operator"] = agree
    out["samples"] = n
    out["launches"] = entry_points(dev, est, clean[:, 0], iters)
    return out


def entry_points(dev, est, clean, iters: int) -> dict:
    """the C entry points alone on preallocated buffers, microseconds per call between two HIP events over back-to-back calls;
    then each resolution alone (a one-resolution call minus nothing: its frames launch plus the finalize or gather launch)"""
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, cap = est.shape[1], min(est.shape[1], clean.shape[1])
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    one = torch.ones((), device=dev)
    loss, total, grad = torch.empty(B, device=dev), torch.empty(2, device=dev), torch.empty_like(est)
    rows = (est.data_ptr(), est.stride(0), n, clean.data_ptr(), clean.stride(0), clean.shape[1], lens.data_ptr(), B)

    def timed(fn):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / iters

    out = {}
    for name, res in [("all", RES)] + [(f"{r[0]}_{r[1]}_{r[2]}", (r,)) for r in RES]:
        R = len(res)
        host = (C.c_int32 * (3 * R))(*[v for r in res for v in r])
        tables = wave._mr_tables(tuple(res), dev)
        fb, bb = lib.eab_mrstft_workspace_bytes(host, R, B, cap, 0), lib.eab_mrstft_workspace_bytes(host, R, B, cap, 1)
        wf, wb = torch.empty(fb // 8, dtype=torch.float64, device=dev), torch.empty(bb // 4, device=dev)
        coef = torch.empty((B, R, 2), dtype=torch.float64, device=dev)
        out[name] = {
            "value_us": timed(lambda: _lib.check(lib.eab_mrstft_loss_f32(*rows, host, R, tables.data_ptr(), 1.0, 1.0, 1e-7, wf.data_ptr(), fb,
                                                                         coef.data_ptr(), loss.data_ptr(), total.data_ptr(), stream))),
            "gradient_us": timed(lambda: _lib.check(lib.eab_mrstft_loss_bwd_f32(*rows, host, R, tables.data_ptr(), 1e-7, coef.data_ptr(),
                                                                                one.data_ptr(), 0, 1.0 / B, wb.data_ptr(), bb,
                                                                                grad.data_ptr(), n, stream))),
            "value_workspace_bytes": fb, "gradient_workspace_bytes": bb}
    out["note"] = ("back-to-back calls of the entry points: where the host enqueues slower than the device runs, a figure is the host's "
                   "pace per call, an upper bound of the device time; a one-resolution row holds that resolution's frames launch plus the "
                   "finalize (value) or gather (gradient) launch")
    return out


class Variant:
    def __init__(self, name: str, precision: str, dev):
        self.name = name
        self.net, _ = bench.make_model(bench.MICS, dev)
        self.net.train()
        self.net.precision = precision
        self.opt = eabnet_amd.FlatAdam(list(self.net.parameters()), lr=5e-4, max_grad_norm=1.0)
        self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        self.rows = []

    def step(self, wav, tgt, pd_args, frames, window, dev, record: bool):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.opt.zero_grad(set_to_none=True)
        noisy, target = eabnet_amd.prepare_data(wav, tgt, dev, pd_args)
        out = self.net(noisy)
        self.ev[0].record()
        h0 = time.perf_counter()
        loss = eabnet_amd.com_mag_mse_loss(out, target, frames)
        if self.name == "mrstft":
            loss = loss + WEIGHT * eabnet_amd.mr_stft_loss(eabnet_amd.istft(out, bench.N_FFT, bench.HOP, window), tgt)
        h1 = time.perf_counter()
        self.ev[1].record()
        loss.backward()
        self.opt.step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if record:
            self.rows.append((1e3 * (t1 - t0), self.ev[0].elapsed_time(self.ev[1]), 1e3 * (h1 - h0)))
        return loss


def step(precision: str, dev, repeats: int, blocks: int, block_steps: int, warmup: int) -> dict:
    L = int(SECONDS * bench.SR)
    T = 1 + L // bench.HOP
    pd_args = argparse.Namespace(mics=bench.MICS, sr=bench.SR, wav_len=SECONDS, win_size=0.020, win_shift=0.010, fft_num=bench.N_FFT)
    wav, tgt = bench.synth_waves(B, bench.MICS, L, 1234).to(dev), bench.synth_waves(B, 1, L, 4321).to(dev)
    window = torch.hann_window(bench.N_FFT, device=dev)
    variants = [Variant("spectral", precision, dev), Variant("mrstft", precision, dev)]
    for v in variants:
        for _ in range(warmup):
            loss = v.step(wav, tgt, pd_args, [T] * B, window, dev, False)
    per_repeat = {v.name: [] for v in variants}
    for _ in range(repeats):
        for v in variants:
            v.rows = []
        for _ in range(blocks):
            for v in variants:
                for _ in range(block_steps):
                    loss = v.step(wav, tgt, pd_args, [T] * B, window, dev, True)
                assert bool(torch.isfinite(loss)), "training diverged"
        for v in variants:
            per_repeat[v.name].append([statistics.median(r[k] for r in v.rows) for k in range(3)])
    names = ("ms_per_step", "loss_section_device_ms", "loss_section_host_enqueue_ms")
    out = {"steps_per_variant_and_repeat": blocks * block_steps}
    for v in variants:
        out[v.name] = {n: _stats(c) for n, c in zip(names, zip(*per_repeat[v.name]))}
    a, b = out["spectral"]["ms_per_step"], out["mrstft"]["ms_per_step"]
    out["mrstft_minus_spectral_ms"] = b["median"] - a["median"]
    out["spread_ms"] = max(a["max"] - a["min"], b["max"] - b["min"])
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
    ap.add_argument("--term-iters", type=int, default=30)
    ap.add_argument("--precisions", default="f32,bf16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"workload": f"B {B}, {SECONDS:g} s; resolutions {list(RES)}; training step of the beam-former, {bench.MICS} microphones, "
                       f"FlatAdam(5e-4, clip 1.0), term {WEIGHT} * mr_stft_loss(istft(out), target)",
           "method": "term and operator: HIP events and the host clock around one value + gradient call, medians per repeat; step: two "
                     "model copies in one process, alternating blocks after warm-up of both, a host clock around a step that ends in a "
                     "synchronise; min/max over the repeats",
           "repeats": a.repeats, "blocks": a.blocks, "block_steps": a.block_steps}
    res["term"] = term(dev, a.repeats, a.term_iters)
    print("term", json.dumps(res["term"]), file=sys.stderr, flush=True)
    res["step"] = {}
    for prec in [p for p in a.precisions.split(",") if p]:
        res["step"][prec] = step(prec, dev, a.repeats, a.blocks, a.block_steps, a.warmup)
        print(prec, json.dumps(res["step"][prec]), file=sys.stderr, flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
