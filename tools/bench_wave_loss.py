#!/usr/bin/env python
"""What the waveform term costs in the training step: spectral loss alone against spectral + w * si_sdr_loss(istft(out), target).

    python tools/bench_wave_loss.py [--repeats 3] [--blocks 3] [--block-steps 6] [--precisions f32,bf16] [--out profiles/wave_loss_bench.json]

Workload: the training step of bench.py's train_measure -- B = 6 utterances of 6 s, 8 microphones, prepare_data -> forward ->
loss -> backward -> FlatAdam(5e-4, max_grad_norm=1.0) -- for the beam-former, fp32 and bf16 products.  Per precision two copies
of the model from the same seed live in ONE process:
    (a) "spectral"  com_mag_mse_loss alone: the step as it was, nothing on its path changes
    (b) "wave"      the same plus 0.05 * si_sdr_loss(istft(out, 320, 160, window), target, eps=1e-8)
Both are warmed up, then measured in alternating blocks of ``block-steps`` steps; the whole run is repeated ``repeats`` times and
the spread is that of the repeats' medians.  Every step ends in a synchronise and is timed with the host clock around it.  Inside
a step the loss section (from the network's output to the loss tensor) lies between two HIP events (device time) and two reads of
the host clock (enqueue time, no synchronise inside).  The new launches are also timed alone at the step's shapes, each between
two HIP events over ``--kernel-iters`` back-to-back launches after a warm-up: the ISTFT adjoint, the loss's two forward launches
and its backward launch.

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

B, SECONDS, WEIGHT = 6, 6.0, 0.05


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
        if self.name == "wave":
            est = eabnet_amd.istft(out, bench.N_FFT, bench.HOP, window)
            loss = loss + WEIGHT * eabnet_amd.si_sdr_loss(est, tgt[:, :, :est.shape[1]], eps=1e-8)
        h1 = time.perf_counter()
        self.ev[1].record()
        loss.backward()
        self.opt.step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if record:
            self.rows.append((1e3 * (t1 - t0), self.ev[0].elapsed_time(self.ev[1]), 1e3 * (h1 - h0)))
        return loss


def _stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def measure(precision: str, dev, repeats: int, blocks: int, block_steps: int, warmup: int) -> dict:
    L = int(SECONDS * bench.SR)
    T = 1 + L // bench.HOP
    pd_args = argparse.Namespace(mics=bench.MICS, sr=bench.SR, wav_len=SECONDS, win_size=0.020, win_shift=0.010, fft_num=bench.N_FFT)
    wav, tgt = bench.synth_waves(B, bench.MICS, L, 1234).to(dev), bench.synth_waves(B, 1, L, 4321).to(dev)
    window = torch.hann_window(bench.N_FFT, device=dev)
    variants = [Variant("spectral", precision, dev), Variant("wave", precision, dev)]
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
    a, b = out["spectral"]["ms_per_step"], out["wave"]["ms_per_step"]
    out["wave_minus_spectral_ms"] = b["median"] - a["median"]
    out["spread_ms"] = max(a["max"] - a["min"], b["max"] - b["min"])
    del variants
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    return out


def kernels(dev, iters: int) -> dict:
    """device time of the new launches alone, at the step's shapes: microseconds per call, HIP events around `iters` calls"""
    L = int(SECONDS * bench.SR)
    T = 1 + L // bench.HOP
    window = torch.hann_window(bench.N_FFT, device=dev)
    spec = torch.randn(B, 2, T, bench.N_FFT // 2 + 1, device=dev, requires_grad=True)
    clean = torch.randn(B, 1, L, device=dev)
    wav = eabnet_amd.istft(spec, bench.N_FFT, bench.HOP, window)
    est = wav.detach().requires_grad_(True)
    dwav = torch.randn_like(wav)
    one = torch.ones((), device=dev)

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

    # the entry points themselves on preallocated buffers (the wrappers' allocations and autograd's bookkeeping would make the
    # host the slower side of a back-to-back loop)
    import ctypes as C
    from eabnet_amd import _lib, model
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tw = model._twiddle(bench.N_FFT, dev)
    x, dspec = spec.detach(), torch.empty_like(spec)
    e, s = est.detach(), clean[:, 0, :est.shape[1]]
    n = e.shape[1]
    lens = torch.full((B, 2), n, dtype=torch.int32, device=dev)
    spans = -(-n // 4096)
    partial = torch.empty((B, spans, 3), dtype=torch.float64, device=dev)
    coef = torch.empty((B, 3), dtype=torch.float64, device=dev)
    loss, total, grad = torch.empty(B, device=dev), torch.empty(2, device=dev), torch.empty_like(e)
    rows = (e.data_ptr(), e.stride(0), n, s.data_ptr(), s.stride(0), n, lens.data_ptr(), B)

    def fwd():
        _lib.check(lib.eab_si_sdr_loss_f32(*rows, 1e-8, partial.data_ptr(), spans, coef.data_ptr(), loss.data_ptr(), total.data_ptr(), stream))

    res = {"istft_forward_us": timed(lambda: _lib.check(lib.eab_istft_f32(x.data_ptr(), window.data_ptr(), tw.data_ptr(), wav.data_ptr(),
                                                                          B, T, bench.N_FFT, bench.HOP, stream))),
           "istft_adjoint_us": timed(lambda: _lib.check(lib.eab_istft_bwd_f32(dwav.data_ptr(), window.data_ptr(), tw.data_ptr(),
                                                                              dspec.data_ptr(), None, B, T, bench.N_FFT, bench.HOP, stream))),
           "si_sdr_forward_two_launches_us": timed(fwd),
           "si_sdr_backward_launch_us": timed(lambda: _lib.check(lib.eab_si_sdr_loss_bwd_f32(*rows, coef.data_ptr(), one.data_ptr(), 0, 1.0 / B,
                                                                                             grad.data_ptr(), n, stream)))}
    res["note"] = ("back-to-back calls of the entry points: where the host enqueues slower than the device runs, a figure is the "
                   "host's pace per call, an upper bound of the device time")
    res["bytes_moved_by_the_new_launches"] = 4 * (dwav.numel() + dspec.numel() + 2 * (e.numel() + s.numel()) + grad.numel())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--block-steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--precisions", default="f32,bf16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"workload": f"training step of the beam-former, B {B}, {SECONDS:g} s, {bench.MICS} microphones, FlatAdam(5e-4, clip 1.0); "
                       f"waveform term {WEIGHT} * si_sdr_loss(istft(out), target, eps=1e-8)",
           "method": "two model copies in one process, alternating blocks after warm-up of both; per step a host clock around a step "
                     "that ends in a synchronise; medians per repeat, min/max over the repeats",
           "repeats": a.repeats, "blocks": a.blocks, "block_steps": a.block_steps, "precisions": {}}
    for prec in a.precisions.split(","):
        res["precisions"][prec] = measure(prec, dev, a.repeats, a.blocks, a.block_steps, a.warmup)
        print(prec, json.dumps(res["precisions"][prec]), file=sys.stderr, flush=True)
    res["kernels"] = kernels(dev, a.kernel_iters)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
