#!/usr/bin/env python
"""What the intelligibility term costs: alone (value plus gradient), in the training step, and against the same definition written
with torch operators under autograd on the device.

    python tools/bench_stoi_loss.py [--repeats 3] [--blocks 3] [--block-steps 6] [--precisions f32,bf16] [--out profiles/stoi_loss_bench.json]

Workload: B = 6 utterances of 6 s at 16 kHz (est rows of 95,840 samples against clean rows of 96,000: unequal, as a loader's),
factor_stoi = factor_estoi = 0.5.
  term      value + gradient of stoi_loss(sample_rate=16000) on a leaf wave (two resampler launches, five value launches, three
            gradient launches, one resampler-adjoint launch): device time between two HIP events and host enqueue time (host clock,
            no synchronise inside) per call, medians of ``--term-iters`` calls per repeat; the same at 10 kHz on the resampled rows
            (no resampler); the entry points alone on preallocated buffers
  operator  DESIGN §4.16 with the conventions of §4.22 in fp32 torch operators under autograd on the device, on the SAME 10 kHz
            rows (the package's resampler is not part of it), one utterance after the other because the kept-frame count is data
            (``nonzero`` synchronises, as operator code must) -- the operator stand-in: in this tool only, never in the package
  step      the training step of bench.py's train_measure (configs[3]: prepare_data -> forward -> loss -> backward ->
            FlatAdam(5e-4, max_grad_norm=1.0)) on two copies of the model in one process, alternating blocks:
            (a) com_mag_mse_loss alone, (b) the same plus 0.5 * stoi_loss(istft(out), target, factor_stoi=0.5, factor_estoi=0.5)
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
from eabnet_amd import _lib  # noqa: E402

B, SECONDS, WEIGHT, FACTORS = 6, 6.0, 0.5, (0.5, 0.5)
EPS = 2.0 ** -52
EDGES = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)


def _stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def _sqrt0(v):
    pos = v > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, v, torch.ones_like(v))), torch.zeros_like(v))


def _rows_norm(a, dim):
    a = a - a.mean(dim=dim, keepdim=True)
    return a / (_sqrt0((a * a).sum(dim=dim, keepdim=True)) + EPS)


def operator_scores(est, clean):
    """(stoi, estoi) of one 10 kHz pair of equal length in torch operators (fp32 tensors on the device)"""
    n = torch.arange(256, device=est.device, dtype=torch.float64)
    w = (0.5 - 0.5 * torch.cos(2.0 * torch.pi * (n + 1.0) / 257.0)).to(est.dtype)
    count = (est.shape[0] - 256 + 127) // 128
    xf, yf = (w * s.unfold(0, 256, 128)[:count] for s in (clean, est))
    e = 20.0 * torch.log10(torch.linalg.vector_norm(xf.double(), dim=1) + EPS)
    kept = torch.nonzero(e.max() - 40.0 - e < 0)[:, 0]
    K = kept.shape[0]
    pos = (128 * torch.arange(K, device=est.device)[:, None] + torch.arange(256, device=est.device)[None, :]).reshape(-1)
    bands = []
    for fr in (xf, yf):
        sil = torch.zeros(128 * (K - 1) + 256, device=est.device, dtype=est.dtype).index_add(0, pos, fr[kept].reshape(-1))
        spec = torch.fft.rfft(w * sil.unfold(0, 256, 128)[:K - 1], 512, dim=1)
        P = spec.real ** 2 + spec.imag ** 2
        bands.append(torch.stack([_sqrt0(P[:, lo:hi].sum(dim=1)) for lo, hi in zip(EDGES[:-1], EDGES[1:])]))
    X, Y = bands
    S = K - 1 - 29
    Xs, Ys = X.unfold(1, 30, 1).permute(1, 0, 2), Y.unfold(1, 30, 1).permute(1, 0, 2)
    alpha = _sqrt0((Xs * Xs).sum(2, keepdim=True)) / (_sqrt0((Ys * Ys).sum(2, keepdim=True)) + EPS)
    bound = (1.0 + 10.0 ** 0.75) * Xs
    Yp = torch.where(alpha * Ys <= bound, alpha * Ys, bound)
    stoi = (_rows_norm(Xs, 2) * _rows_norm(Yp, 2)).sum() / (15 * S)
    both = lambda a: _rows_norm(_rows_norm(a, 2), 1)             # noqa: E731
    return stoi, (both(Xs) * both(Ys)).sum() / (30 * S)


def operator_loss(est10, clean10, le, ls):
    total = 0.0
    for b in range(B):
        pad = max(le, ls)
        e = torch.nn.functional.pad(est10[b, :le], (0, pad - le))
        s = torch.nn.functional.pad(clean10[b, :ls], (0, pad - ls))
        stoi, estoi = operator_scores(e, s)
        total = total - (FACTORS[0] * stoi + FACTORS[1] * estoi)
    return total / B


def term(dev, repeats: int, iters: int) -> dict:
    L = int(SECONDS * bench.SR)
    n = bench.HOP * (L // bench.HOP - 1)                          # a hop shorter than the clean rows
    g = torch.Generator().manual_seed(7)
    t = torch.arange(L) / bench.SR
    clean = (0.1 * torch.randn(B, 1, L, generator=g) * (0.6 + 0.4 * torch.sin(2 * torch.pi * 3.0 * t))).to(dev)
    est = (clean[:, 0, :n] + 0.05 * torch.randn(B, n, generator=g).to(dev)).contiguous()
    est10, clean10 = eabnet_amd.resample(est, bench.SR, 10000), eabnet_amd.resample(clean[:, 0], bench.SR, 10000)
    le, ls = est10.shape[1], clean10.shape[1]

    def fused():
        leaf = est.detach().requires_grad_(True)
        eabnet_amd.stoi_loss(leaf, clean, None, bench.SR, *FACTORS).backward()
        return leaf.grad

    def fused10():
        leaf = est10.detach().requires_grad_(True)
        eabnet_amd.stoi_loss(leaf, clean10, None, 10000, *FACTORS).backward()
        return leaf.grad

    def operator():
        leaf = est10.detach().requires_grad_(True)
        operator_loss(leaf, clean10, le, ls).backward()
        return leaf.grad

    gf, go = fused10(), operator()
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

    rows = {"fused_16k": [], "fused_10k": [], "operator_10k": []}
    for _ in range(repeats):
        rows["fused_16k"].append(timed(fused))
        rows["fused_10k"].append(timed(fused10))
        rows["operator_10k"].append(timed(operator))
    out = {k: {"device_ms": _stats([r[0] for r in v]), "host_enqueue_ms": _stats([r[1] for r in v])} for k, v in rows.items()}
    out["gradient_max_diff_over_max_fused_vs_operator"] = agree
    out["samples_16k"], out["samples_10k"] = n, le
    out["launches"] = entry_points(dev, est10, clean10, iters)
    return out


def entry_points(dev, est, clean, iters: int) -> dict:
    """the C entry points alone on preallocated buffers at 10 kHz, microseconds per call between two HIP events over back-to-back
    calls"""
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, cap = est.shape[1], max(est.shape[1], clean.shape[1])
    lens = torch.tensor([[n, clean.shape[1]]] * B, dtype=torch.int32, device=dev)
    one = torch.ones((), device=dev)
    fb, bb = lib.eab_stoi_workspace_bytes(B, cap), lib.eab_stoi_bwd_workspace_bytes(B, cap)
    wf, wb = torch.empty(fb, dtype=torch.uint8, device=dev), torch.empty(bb, dtype=torch.uint8, device=dev)
    out, grad = torch.empty((B, 2), dtype=torch.float64, device=dev), torch.empty_like(est)

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

    res = {"value_us": timed(lambda: _lib.check(lib.eab_stoi_f32(est.data_ptr(), est.stride(0), n, clean.data_ptr(), clean.stride(0),
                                                                 clean.shape[1], lens.data_ptr(), B, wf.data_ptr(), fb, out.data_ptr(),
                                                                 None, None, None, stream)))}
    for name, f in (("gradient_us", FACTORS), ("gradient_stoi_only_us", (1.0, 0.0)), ("gradient_estoi_only_us", (0.0, 1.0))):
        res[name] = timed(lambda: _lib.check(lib.eab_stoi_bwd_f32(est.data_ptr(), est.stride(0), n, clean.shape[1], lens.data_ptr(), B,
                                                                  wf.data_ptr(), fb, f[0], f[1], one.data_ptr(), 0, 1.0 / B,
                                                                  wb.data_ptr(), bb, grad.data_ptr(), n, stream)))
    res.update(value_workspace_bytes=fb, gradient_workspace_bytes=bb,
               note="back-to-back calls of the entry points: where the host enqueues slower than the device runs, a figure is the host's "
                    "pace per call, an upper bound of the device time")
    return res


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
        if self.name == "stoi":
            loss = loss + WEIGHT * eabnet_amd.stoi_loss(eabnet_amd.istft(out, bench.N_FFT, bench.HOP, window), tgt, None, bench.SR, *FACTORS)
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
    variants = [Variant("spectral", precision, dev), Variant("stoi", precision, dev)]
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
    a, b = out["spectral"]["ms_per_step"], out["stoi"]["ms_per_step"]
    out["stoi_minus_spectral_ms"] = b["median"] - a["median"]
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
    res = {"workload": f"B {B}, {SECONDS:g} s at {bench.SR} Hz; factors {list(FACTORS)}; training step of the beam-former, {bench.MICS} "
                       f"microphones, FlatAdam(5e-4, clip 1.0), term {WEIGHT} * stoi_loss(istft(out), target)",
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
