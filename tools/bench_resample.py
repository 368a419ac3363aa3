#!/usr/bin/env python
"""Resampling on the device: the kernel of csrc/resample.hip alone, and ``eabnet_amd.Enhancer`` on files at 48 kHz against the
same files handed in at 16 kHz.

    python tools/bench_resample.py [--reps 50] [--files 50] [--max-batch 16] [--out FILE]

Kernel: a padded batch of 16 utterances x 8 microphones x 4 s, to 16 kHz from 48 kHz (one phase, 37 taps) and from 44.1 kHz
(160 phases, 34 taps) -- and, for the other code paths, from 32 kHz (even stride: skewed LDS span) and up to 48 kHz; ``reps``
back-to-back launches between two HIP events, best of three: microseconds per launch and the fraction of the 8 TB/s HBM peak on
algorithmic bytes (every input sample read once, every output sample written once).  For scale, the STFT front end on the
16 kHz result, same protocol.

Enhancer: the 50 seeded file lengths of tools/bench_enhance.py (2-10 s, M = 8, EaBNet, fp32, device-resident waves), generated
at 48 kHz; ``Enhancer(sample_rate=48000)`` on them against ``Enhancer()`` on the same files resampled beforehand.  Each runs
once cold, then three times with its programs resident; the best of the three is reported.

Prints one JSON object (and writes it to --out when given)."""
from __future__ import annotations

import argparse
import importlib
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

rsm = importlib.import_module("eabnet_amd.resample")
HBM = 8e12


def events(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e-3)
    return best


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_rows(dev, reps):
    B, M, seconds = 16, 8, 4
    out = {}
    for orig, new in ((48000, 16000), (44100, 16000), (32000, 16000), (16000, 48000)):
        L = orig * seconds
        x = 0.05 * torch.randn(B, M, L, device=dev)
        n_out = eabnet_amd.resampled_length(L, orig, new)
        bank = rsm._device_bank(orig, new, "hann", 6, 0.99, dev)
        y = torch.empty(B, M, n_out, device=dev)

        def launch():
            rsm._launch(x, L, L, None, None, B * M, M, y, n_out, bank)
        t = events(launch, reps)
        by = B * M * (L + n_out) * 4
        out[f"{orig}->{new}"] = {"n": bank[3], "K": bank[4], "us": round(1e6 * t, 2), "bytes": by,
                                 "TB_per_s": round(by / t / 1e12, 3), "hbm_fraction": round(by / t / HBM, 3)}
        print(f"resample {orig}->{new}: {1e6 * t:8.2f} us  {by / t / 1e12:6.3f} TB/s  frac {by / t / HBM:.3f}", flush=True)
        if (orig, new) == (48000, 16000):
            window = torch.hann_window(320)
            T = 1 + n_out // 160
            ts = events(lambda: eabnet_amd.stft_compress(y, 320, 160, window), reps)
            bs = B * T * (160 * M * 4 + 161 * M * 2 * 4)
            out["stft_compress_16k"] = {"us": round(1e6 * ts, 2), "bytes": bs, "hbm_fraction": round(bs / ts / HBM, 3)}
            print(f"stft_compress on the result: {1e6 * ts:8.2f} us  frac {bs / ts / HBM:.3f}", flush=True)
    return out


def enhancer_rows(dev, files, max_batch):
    from bench_varlen import fresh
    M = 8
    seconds = np.random.default_rng(1234).uniform(2.0, 10.0, size=files)
    g = torch.Generator().manual_seed(0)
    at48 = [(0.05 * torch.randn(M, int(s * 48000), generator=g)).to(dev) for s in seconds]
    at16 = [eabnet_amd.resample(w, 48000, 16000) for w in at48]
    model = eabnet_amd.EaBNet(M=M).to(dev).eval()
    out = {"files": files, "max_batch": max_batch, "samples_48k": sum(w.shape[1] for w in at48)}
    ref = None
    for name, enh, waves in (("at_16k", eabnet_amd.Enhancer(model, max_batch=max_batch), at16),
                             ("at_48k", eabnet_amd.Enhancer(model, max_batch=max_batch, sample_rate=48000), at48)):
        fresh(model)
        cold, _ = wall(lambda: enh(waves))
        warm, got = min((wall(lambda: enh(waves)) for _ in range(3)), key=lambda r: r[0])
        if ref is None:
            ref = got
        out[name] = {"cold_s": round(cold, 3), "warm_s": round(warm, 4), "files_per_s": round(files / warm, 1),
                     "ms_per_file": round(1e3 * warm / files, 3), "equal_to_16k": all(torch.equal(a, b) for a, b in zip(got, ref))}
        print(name, out[name], flush=True)
    fresh(model)
    out["added_ms_per_file"] = round(out["at_48k"]["ms_per_file"] - out["at_16k"]["ms_per_file"], 3)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--files", type=int, default=50)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"kernel": kernel_rows(dev, args.reps), "enhancer": enhancer_rows(dev, args.files, args.max_batch)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
