#!/usr/bin/env python
"""What undoing the sqrt compression inside the ISTFT costs, and what it does to the scores.

    python tools/bench_istft_decompress.py [--repeats 7] [--iters 200] [--out profiles/istft_decompress_bench.json]

Sizes: B = 16, T = 401 and B = 6, T = 601 frames of 320/160 (the benchmark's inference and training batches).  Rows:
    (a) "istft"      istft(x)                                        -- the reference's back end, today's launch
    (b) "fused"      istft(x, decompress=True)                       -- the same launch with y = s |s| formed in LDS
    (c) "unfused"    istft(x * x.norm(dim=1, keepdim=True))          -- the same wave by two more passes over (B, 2, T, F)
each measured forward alone (no grad) and forward + backward under autograd (a leaf spectrum, ``wav.backward(dwav)``).  All variants
live in ONE process; after a warm-up of every one they are measured in alternating blocks: per repeat and variant ``iters``
back-to-back calls between two HIP events.  Reported per variant: median, min and max of the repeats in microseconds per call; the
spread of a row is max - min.  The Python wrappers allocate and enqueue slower than a launch-sized kernel runs, so the rows above
are the pace a caller sees; ``entry_points`` times the four C entry points alone on preallocated buffers, the device's side of it.

``scores``: ``Scorer`` with and without ``decompress`` on synthetic files (modulated noise, a small untrained network), and the
ceiling of either wave: the SI-SDR of a PERFECT estimate -- the label spectrum of the clean wave itself -- inverted both ways.

Prints one JSON object (and writes it to --out when given)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import eabnet_amd  # noqa: E402

N_FFT, HOP = 320, 160
SIZES = [(16, 401), (6, 601)]


def _stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "spread": max(values) - min(values)}


def _timed(fn, iters: int) -> float:
    """microseconds per call: HIP events around `iters` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def _alternate(variants: dict, repeats: int, iters: int) -> dict:
    for fn in variants.values():
        for _ in range(20):
            fn()
    rows = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            rows[k].append(_timed(fn, iters))
    return {k: _stats(v) for k, v in rows.items()}


def measure(B: int, T: int, dev, repeats: int, iters: int) -> dict:
    window = torch.hann_window(N_FFT, device=dev)
    x = torch.randn(B, 2, T, N_FFT // 2 + 1, device=dev)
    leaf = x.clone().requires_grad_(True)
    dwav = torch.randn(B, HOP * (T - 1), device=dev)
    forms = {"istft": lambda s: eabnet_amd.istft(s, N_FFT, HOP, window),
             "fused": lambda s: eabnet_amd.istft(s, N_FFT, HOP, window, decompress=True),
             "unfused": lambda s: eabnet_amd.istft(s * s.norm(dim=1, keepdim=True), N_FFT, HOP, window)}

    def fwd(form):
        def run():
            with torch.no_grad():
                form(x)
        return run

    def fwd_bwd(form):
        def run():
            leaf.grad = None
            form(leaf).backward(dwav)
        return run

    out = {"forward_us": _alternate({k: fwd(f) for k, f in forms.items()}, repeats, iters),
           "forward_backward_us": _alternate({k: fwd_bwd(f) for k, f in forms.items()}, repeats, iters)}
    # the entry points alone, on preallocated buffers
    from eabnet_amd import _lib, model
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tw = model._twiddle(N_FFT, dev)
    wav, dspec = torch.empty_like(dwav), torch.empty_like(x)
    p = {k: t.data_ptr() for k, t in (("x", x), ("w", window), ("tw", tw), ("wav", wav), ("dwav", dwav), ("dspec", dspec))}
    out["entry_points_us"] = _alternate({
        "eab_istft_f32": lambda: _lib.check(lib.eab_istft_f32(p["x"], p["w"], p["tw"], p["wav"], B, T, N_FFT, HOP, stream)),
        "eab_istft_lin_f32": lambda: _lib.check(lib.eab_istft_lin_f32(p["x"], p["w"], p["tw"], p["wav"], None, B, T, N_FFT, HOP, stream)),
        "eab_istft_bwd_f32": lambda: _lib.check(lib.eab_istft_bwd_f32(p["dwav"], p["w"], p["tw"], p["dspec"], None, B, T, N_FFT, HOP,
                                                                      stream)),
        "eab_istft_lin_bwd_f32": lambda: _lib.check(lib.eab_istft_lin_bwd_f32(p["dwav"], p["x"], p["w"], p["tw"], p["dspec"], None, B, T,
                                                                              N_FFT, HOP, stream))}, repeats, iters)
    for mode in ("forward_us", "forward_backward_us"):
        r = out[mode]
        out[mode + "_verdict"] = {
            "fused_minus_istft": r["fused"]["median"] - r["istft"]["median"], "spread_of_istft": r["istft"]["spread"],
            "fused_minus_istft_exceeds_the_spread": r["fused"]["median"] - r["istft"]["median"] > r["istft"]["spread"],
            "fused_below_unfused": r["fused"]["median"] < r["unfused"]["median"]}
    return out


def scores(dev) -> dict:
    """synthetic files: clean = noise under a slow envelope, noisy = clean + white noise per microphone"""
    M, samples = 4, [48000, 32000, 20011, 64000]
    g = torch.Generator().manual_seed(7)
    clean, noisy = [], []
    for n in samples:
        t = torch.arange(n) / 16000.0
        c = 0.1 * (0.55 + 0.45 * torch.sin(2 * np.pi * 3.0 * t)) * torch.randn(n, generator=g)
        clean.append(c)
        noisy.append(c[None] + 0.05 * torch.randn(M, n, generator=g))
    torch.manual_seed(0)
    net = eabnet_amd.EaBNet(M=M, p=1, q=1).to(dev).eval()
    table = {}
    for flag in (False, True):
        s = eabnet_amd.Scorer(net, max_batch=4, intelligibility=True, distortion=True, decompress=flag)(noisy, clean)
        table["decompress" if flag else "reference"] = {m: [float(v) for v in col] for m, col in s.items()}
    window = torch.hann_window(N_FFT)
    ceiling = {"reference": [], "decompress": []}
    for c, y in zip(clean, noisy):
        w = c[None, None].to(dev)
        label = eabnet_amd.stft_compress(w, N_FFT, HOP, window, layout=1)
        for flag in (False, True):
            est = eabnet_amd.istft(label, N_FFT, HOP, window, decompress=flag)
            ceiling["decompress" if flag else "reference"].append(float(eabnet_amd.energy_ratios(est, w[0], y[:1].to(dev))[0, 0]))
    return {"files_samples": samples, "microphones": M, "network": "EaBNet(M=4, p=1, q=1), untrained, seed 0", "scorer": table,
            "si_sdr_of_a_perfect_estimate_db": ceiling}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"method": "all variants in one process, warmed up, then alternating: per repeat and variant `iters` back-to-back calls between "
                     "two HIP events; microseconds per call, median / min / max over the repeats, spread = max - min",
           "repeats": a.repeats, "iters": a.iters, "sizes": {}}
    for B, T in SIZES:
        res["sizes"][f"B{B}_T{T}"] = measure(B, T, dev, a.repeats, a.iters)
        print(f"B {B} T {T}", json.dumps(res["sizes"][f"B{B}_T{T}"]), file=sys.stderr, flush=True)
    res["scores"] = scores(dev)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
