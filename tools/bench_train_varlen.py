#!/usr/bin/env python
"""Training on padded batches of unequal-length utterances (EaBNet.varlen_training): what it costs and buys.

    python tools/bench_train_varlen.py [--rounds 5] [--steps 8] [--out profiles/train_varlen_bench.json]

At the training shape of BASELINE configs[3] (6 utterances, 8 microphones, T = 601 frames), fp32 and bf16, a step = forward,
com_mag_mse_loss, backward.  Device events around `steps` steps, after warm-up of every shape; `rounds` repetitions, the two
sides of a comparison alternating inside every round; reported: the median and the (min, max) of the per-round step times.

1. full lengths: the varlen program with every length = T against the exact-shape program (the same work; the masks ride along)
2. mixed lengths, frames [601, 520, 440, 360, 280, 200]: the padded step against the only correct alternative without the
   feature -- six warm B = 1 exact-shape steps, one per utterance, back to back -- and against the padded step that trains on
   the padding (same batch, no lengths: wrong statistics, for the time only)
3. per-launch share: the forward and backward programs of the mixed-length step op by op (direct launches, one event pair per
   op), summed per op kind, next to the full-length step -- which launches still walk the padding

Prints one JSON object (and writes it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import eabnet_amd  # noqa: E402
from eabnet_amd import program as prg  # noqa: E402
from eabnet_amd import train as tr  # noqa: E402

B, M, T, F = 6, 8, 601, 161
MIXED = [601, 520, 440, 360, 280, 200]
TRAIN_BOUND_CACHE = 8                     # keep the six B = 1 programs and the two padded ones resident


def make_net(dev, precision, varlen):
    torch.manual_seed(0)
    net = eabnet_amd.EaBNet(M=M).to(dev).train()
    net.precision = precision
    net.varlen_training = varlen
    return net


def step(net, x, label, lens, frames):
    for p in net.parameters():
        p.grad = None
    y = net(x) if lens is None else net(x, lengths=lens)
    eabnet_amd.com_mag_mse_loss(y, label, frames).backward()


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def summary(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def per_kind(bound, which):
    """ms per op kind of one direct pass over the op list `which` of a bound program (its boundary already bound)"""
    names = {v: k[3:] for k, v in vars(prg).items() if k.startswith("OP_") and isinstance(v, int)}
    ops = bound.lists[which]
    st = torch.cuda.current_stream().cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(ops) + 1)]
    k = 0
    ev[0].record()
    marks = []
    while k < len(ops):
        n = 1
        if ops[k].kind == tr.OP_WGRAD:                 # a run of weight gradients is batched by eab_run_program
            while k + n < len(ops) and ops[k + n].kind == tr.OP_WGRAD:
                n += 1
        bound.run(which, st, k, n)
        k += n
        ev[k].record()
        marks.append((k - n, k))
    torch.cuda.synchronize()
    out = {}
    for a, b_ in marks:
        kind = names.get(ops[a].kind, str(ops[a].kind))
        if ops[a].kind == prg.OP_CONV:
            kind += "/st" if ops[a].korder == prg.KORDER_FRAG else ("/2d" if ops[a].Fin > 1 else "/1d")
        out[kind] = out.get(kind, 0.0) + ev[a].elapsed_time(ev[b_])
    return {k_: round(v, 3) for k_, v in sorted(out.items(), key=lambda kv: -kv[1])}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_varlen_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X: no device, no numbers"
    dev = torch.device("cuda:0")
    tr.TRAIN_BOUND_CACHE = TRAIN_BOUND_CACHE
    g = torch.Generator().manual_seed(1)
    x = (0.3 * torch.randn(B, T, F, M, 2, generator=g)).to(dev)
    label = (0.3 * torch.randn(B, 2, T, F, generator=g)).to(dev)
    singles = [(x[b:b + 1, :n].contiguous(), label[b:b + 1, :, :n].contiguous(), n) for b, n in enumerate(MIXED)]
    res = {"shape": {"B": B, "M": M, "T": T, "mixed_frames": MIXED, "valid_share": round(sum(MIXED) / (B * T), 3)},
           "rounds": args.rounds, "steps_per_round": args.steps}
    for precision in ("f32", "bf16"):
        exact, varlen = make_net(dev, precision, False), make_net(dev, precision, True)
        full_lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        mixed_lens = torch.tensor(MIXED, dtype=torch.int32, device=dev)
        runs = {
            "exact": lambda: step(exact, x, label, None, [T] * B),
            "varlen_full": lambda: step(varlen, x, label, full_lens, [T] * B),
            "varlen_mixed": lambda: step(varlen, x, label, mixed_lens, MIXED),
            "six_b1": lambda: [step(exact, xs, ls, None, [n]) for xs, ls, n in singles],
        }
        for fn in runs.values():                       # warm-up: lowering, capture, code objects -- every shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(args.rounds):                   # alternating inside every round
            for k, fn in runs.items():
                times[k].append(timed(fn, args.steps))
        r = {k: summary(v) for k, v in times.items()}
        r["full_over_exact"] = round(r["varlen_full"]["median_ms"] / r["exact"]["median_ms"], 4)
        r["six_b1_over_mixed"] = round(r["six_b1"]["median_ms"] / r["varlen_mixed"]["median_ms"], 3)
        r["mixed_over_exact_padded"] = round(r["varlen_mixed"]["median_ms"] / r["exact"]["median_ms"], 3)
        # which launches still walk the padding: op by op, the same bound program at full and at mixed lengths
        bound = next(b_ for key, b_ in varlen._train_bound.items() if key[0] == B)
        kinds = {}
        for tag, lens in (("full", full_lens), ("mixed", mixed_lens)):
            bound.lens.copy_(lens)
            io = (x, torch.empty(B, 2, T, F, device=dev), label.clone(), None)
            bound._ptrs = None
            bound.bind(*(None if t is None else t.data_ptr() for t in io))
            bound.g.zero_()
            for which in ("fwd", "bwd"):
                per_kind(bound, which)                 # warm
                bound.g.zero_()
                kinds[f"{which}_{tag}"] = per_kind(bound, which)
        bound._ptrs = None                             # (the next captured replay binds its static buffers again)
        r["per_kind_ms"] = kinds
        res[precision] = r
        print(precision, json.dumps(r), flush=True)
        del exact, varlen
        import gc
        gc.collect()
        torch.cuda.synchronize()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
