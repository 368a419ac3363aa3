#!/usr/bin/env python
"""Per-utterance lengths: what the length-bucketed program cache buys in an enhance-style loop.

    python tools/bench_varlen.py [--files 50] [--out FILE]

1. One file at a time (B = 1, M = 8), 50 seeded lengths between 2 and 10 s (201 .. 1001 frames), through EaBNet alone and
   through the two-stage model (EaBNet + GaGNet post-filter), once on the default path (one exact-shape program per new
   length: lowering, arena, graph capture) and once with ``length_buckets = "auto"``.  Reports the loop's total time and
   the number of ``program.lower`` calls.  The input is the compressed spectrogram itself (the STFT is the same either way).
2. Warm per-call time at T in {100, 301, 700} inside the 1024-frame bucket against warm exact-shape calls at the same T,
   at B = 1 and B = 16, and the activation-arena bytes of each bucket program.

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

import eabnet_amd  # noqa: E402
from eabnet_amd import program as prg  # noqa: E402


def two_stage_args(M: int):
    return argparse.Namespace(
        k1=(2, 3), k2=(1, 3), c=64, M=M, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=6, q=3, is_causal=True, is_u2=True,
        bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="IN", ref_mic=0, freeze_eabnet=False,
        gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=2,
        gagnet_q=3, gagnet_dilas=[1, 2, 5, 9], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=True,
        gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="IN")


class LowerCounter:
    def __init__(self):
        self.n = 0
        self.real = prg.lower

    def __enter__(self):
        def counted(*a, **k):
            self.n += 1
            return self.real(*a, **k)
        prg.lower = counted
        return self

    def __exit__(self, *exc):
        prg.lower = self.real


def set_buckets(net, value):
    net.length_buckets = value


def fresh(net):
    """drop every resident program (exact-shape slot and buckets) so that each pass starts cold"""
    for m in net.modules():
        if isinstance(m, eabnet_amd.model._HipModule):
            for cache in (m._bound, m._packed_version, m._varlen_bound, m._varlen_version):
                cache.clear()
    import gc
    gc.collect()
    torch.cuda.synchronize()


def enhance_loop(net, frames, M, dev, buckets):
    fresh(net)
    set_buckets(net, buckets)
    g = torch.Generator().manual_seed(0)
    xs = [(0.3 * torch.randn(1, T, 161, M, 2, generator=g)).to(dev) for T in frames]
    torch.cuda.synchronize()
    with LowerCounter() as lc, torch.no_grad():
        t0 = time.perf_counter()
        for x in xs:
            net(x)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    set_buckets(net, None)
    return dt, lc.n


def warm_ms(net, x, reps=20):
    with torch.no_grad():
        for _ in range(3):
            net(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            net(x)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    M = 8
    rng = np.random.default_rng(1234)
    seconds = rng.uniform(2.0, 10.0, size=args.files)
    frames = [1 + int(s * 16000) // 160 for s in seconds]
    res = {"files": args.files, "frames_min": min(frames), "frames_max": max(frames), "loop": {}, "warm": [], "arena_bytes": {}}

    eab = eabnet_amd.EaBNet(M=M).to(dev).eval()
    two = eabnet_amd.make_eabnet_with_postnet(two_stage_args(M)).to(dev).eval()
    for name, net in (("eabnet", eab), ("two_stage", two)):
        d_s, d_n = enhance_loop(net, frames, M, dev, None)
        b_s, b_n = enhance_loop(net, frames, M, dev, "auto")
        res["loop"][name] = {"default_s": round(d_s, 3), "default_lower_calls": d_n, "bucketed_s": round(b_s, 3),
                             "bucketed_lower_calls": b_n, "speedup": round(d_s / b_s, 1)}
        print(name, res["loop"][name], flush=True)
        fresh(net)

    for B in (1, 16):
        g = torch.Generator().manual_seed(B)
        xfull = (0.3 * torch.randn(B, 1024, 161, M, 2, generator=g)).to(dev)
        for T in (100, 301, 700):
            x = xfull[:, :T].contiguous()
            fresh(eab)
            exact = warm_ms(eab, x)
            fresh(eab)
            eab.length_buckets = (1024,)
            bucket = warm_ms(eab, x)
            for k, v in eab.varlen_arena_bytes().items():
                res["arena_bytes"][f"B{k[0]}_T{k[1]}"] = v
            eab.length_buckets = None
            row = {"B": B, "T": T, "exact_ms": round(exact, 3), "bucket1024_ms": round(bucket, 3),
                   "ratio": round(bucket / exact, 3)}
            res["warm"].append(row)
            print(row, flush=True)
        fresh(eab)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
