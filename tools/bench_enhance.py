#!/usr/bin/env python
"""A folder of files, waves in and waves out: ``eabnet_amd.Enhancer`` (padded batches with per-utterance lengths) against
the one-file-at-a-time loop.

    python tools/bench_enhance.py [--files 50] [--max-batch 16] [--budget-gib 8 16] [--out FILE]

50 seeded file lengths of 2-10 s (the seeds of tools/bench_varlen.py), M = 8, fp32, default configuration, EaBNet alone and
the two-stage model, device-resident waves.  Baseline: per file ``stft_compress -> model (length_buckets="auto") -> istft`` at
B = 1.  Both loops run twice from a cold cache; the first pass is reported as ``cold_s``, the second (programs resident) gives
files/s and ms per file.  For the enhancer also: the plan (batches, caps, batch sizes, dummies, padded / valid frames), the
activation-arena bytes per (batch size, cap), and the time per phase (pack, STFT, model, ISTFT, slicing; a pass of its own with
a device synchronisation after every phase).  ``--budget-gib`` runs the enhancer once per value of ``max_resident_bytes``
(8 GiB is the networks' default; the 1024-frame program of 16 utterances needs more).

Prints one JSON object (and writes it to --out when given).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import eabnet_amd  # noqa: E402
from bench_varlen import fresh, two_stage_args  # noqa: E402

FFT, HOP = 320, 160


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def one_at_a_time(net, waves, window):
    out = []
    with torch.no_grad():
        for w in waves:
            y = net(eabnet_amd.stft_compress(w[None], FFT, HOP, window))
            y = y["esti_stft"] if isinstance(y, dict) else y
            out.append(eabnet_amd.istft(y, FFT, HOP, window)[0])
    return out


def nets_of(model):
    return [m for m in model.modules() if isinstance(m, eabnet_amd.model._HipModule)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=50)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--budget-gib", type=float, nargs="+", default=[8.0, 16.0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    M = 8
    seconds = np.random.default_rng(1234).uniform(2.0, 10.0, size=args.files)
    samples = [int(s * 16000) for s in seconds]
    g = torch.Generator().manual_seed(0)
    waves = [(0.05 * torch.randn(M, n, generator=g)).to(dev) for n in samples]
    window = torch.hann_window(FFT)
    res = {"files": args.files, "max_batch": args.max_batch, "frames_total": sum(1 + n // HOP for n in samples), "models": {}}

    models = (("eabnet", eabnet_amd.EaBNet(M=M).to(dev).eval()),
              ("two_stage", eabnet_amd.make_eabnet_with_postnet(two_stage_args(M)).to(dev).eval()))
    for name, model in models:
        row = res["models"][name] = {}
        fresh(model)
        model.length_buckets = "auto"
        cold, _ = timed(lambda: one_at_a_time(model, waves, window))
        warm, ref = timed(lambda: one_at_a_time(model, waves, window))
        model.length_buckets = None
        row["one_at_a_time"] = {"cold_s": round(cold, 3), "warm_s": round(warm, 4), "files_per_s": round(args.files / warm, 1),
                                "ms_per_file": round(1e3 * warm / args.files, 3)}
        print(name, "one_at_a_time", row["one_at_a_time"], flush=True)
        for gib in args.budget_gib:
            fresh(model)
            for n in nets_of(model):
                n.max_resident_bytes = int(gib * (1 << 30))
            enh = eabnet_amd.Enhancer(model, max_batch=args.max_batch)
            cold, _ = timed(lambda: enh(waves))
            warm, got = timed(lambda: enh(waves))
            err = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, ref))
            plan = enh.last_plan
            phases: dict = {}
            last = [0.0]

            def hook(phase):
                torch.cuda.synchronize()
                now = time.perf_counter()
                phases[phase] = phases.get(phase, 0.0) + now - last[0]
                last[0] = now
            enh.phase_hook = hook
            torch.cuda.synchronize()
            last[0] = time.perf_counter()
            enh(waves)
            enh.phase_hook = None
            arena = {}
            for n in nets_of(model):
                for k, v in n.varlen_arena_bytes().items():
                    arena[f"{type(n).__name__}_B{k[0]}_T{k[1]}"] = v
            r = {"cold_s": round(cold, 3), "warm_s": round(warm, 4), "files_per_s": round(args.files / warm, 1),
                 "ms_per_file": round(1e3 * warm / args.files, 3),
                 "speedup_vs_one_at_a_time": round(row["one_at_a_time"]["warm_s"] / warm, 2),
                 "max_err_vs_one_at_a_time": err,
                 "batches": [(len(b["indices"]), b["cap"], b["batch_size"], b["dummies"]) for b in plan["batches"]],
                 "dummies": plan["dummies"], "padded_to_valid": round(plan["padded_frames"] / plan["valid_frames"], 3),
                 "cap_to_valid": round(plan["cap_frames"] / plan["valid_frames"], 3),
                 "phase_ms": {k: round(1e3 * v, 2) for k, v in phases.items()}, "arena_bytes": arena}
            row[f"enhancer_{gib:g}GiB"] = r
            print(name, f"enhancer {gib:g} GiB", r, flush=True)
        fresh(model)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
