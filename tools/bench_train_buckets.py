#!/usr/bin/env python
"""Training length buckets (train_length_buckets): what a cap wider than the batch costs, and what one program for
every width buys.

    python tools/bench_train_buckets.py [--rounds 5] [--steps 6] [--out profiles/train_buckets_bench.json]
    python tools/bench_train_buckets.py --profile-case cap1024 [--model eabnet] [--precision f32]      (under rocprofv3, see 3.)
    python tools/bench_train_buckets.py --summarize DIR_OF_CASE ... [--out ...]

Size of BASELINE configs[3]: 6 utterances, 8 microphones, frames 601, 520, 440, 360, 280, 200 padded to T = 601; fp32 and bf16; the
beam-former (EaBNet) and the two-stage model (EaBNetWithPostNet, both stages trained).  A step = forward, loss (com_mag_mse_loss /
eabnet_with_postnet_loss), backward.  Device events around `steps` steps after warm-up of every program; `rounds` repetitions, all
cases alternating inside every round; reported: the median and the (min, max) of the per-round step times.

1. step time of four programs on the same batch:
     exact     the masked program of the call's own width T = 601 (EaBNet: varlen_training; the two-stage model has no such
               program without the switch, so there it is the bucket program at the exact width, caps = (1,))
     cap640    train_length_buckets = (640,)
     cap1024   train_length_buckets = "auto"
     cap1024_lstm_walks_cap   the same with train_bucket_lstm_bound = False on the module: both LSTM recurrences walk the cap -- what the bound buys
   and, for the two-stage model, what exists without the switch: the padded batch without lengths (trains on the padding; for
   the time only) and six warm B = 1 exact-shape steps, one per utterance.
2. a width sweep (EaBNet): one step at each of eight distinct padded widths between 300 and 640, wall time including lowering
   and capture (host clock around a step that ends in a device synchronise), buckets (640,) against the exact-width path.
3. --profile-case runs warm-up + 5 steps of ONE case with direct launches, for `rocprofv3 --kernel-trace --stats -- python ...`;
   --summarize reads the *_kernel_stats.csv of such runs and sums the kernel time per step by kernel kind.

Prints one JSON object (and writes it to --out)."""
from __future__ import annotations

import argparse
import csv
import gc
import glob
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, M, T, F = 6, 8, 601, 161
MIXED = [601, 520, 440, 360, 280, 200]
SWEEP = [(640, 7), (601, 3), (555, 11), (512, 5), (470, 13), (421, 2), (366, 9), (310, 4)]      # (padded width, seed)
CASES = ("exact", "cap640", "cap1024", "cap1024_lstm_walks_cap")
PROFILE_STEPS, PROFILE_WARMUP = 5, 2


def two_stage_args():
    return argparse.Namespace(
        k1=(2, 3), k2=(1, 3), c=64, M=M, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=6, q=3, is_causal=True, is_u2=True,
        bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="IN", ref_mic=0, freeze_eabnet=False,
        gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=2,
        gagnet_q=3, gagnet_dilas=[1, 2, 5, 9], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=True,
        gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="IN")


def make_net(model, dev, precision, case):
    """the module of one case; case None: no switch at all (the exact-shape programs without lengths)"""
    import torch
    import eabnet_amd
    torch.manual_seed(0)
    if model == "eabnet":
        net = eabnet_amd.EaBNet(M=M).to(dev).train()
        net.precision = precision
    else:
        net = eabnet_amd.make_eabnet_with_postnet(two_stage_args()).to(dev).train()
        net.eabnet.precision = net.postnet.precision = precision
    if case == "exact":
        if model == "eabnet":
            net.varlen_training = True
        else:
            net.train_length_buckets = (1,)
    elif case == "cap640":
        net.train_length_buckets = (640,)
    elif case is not None:
        net.train_length_buckets = "auto"
    if case == "cap1024_lstm_walks_cap":
        for m_ in ([net] if model == "eabnet" else [net.eabnet, net.postnet]):
            m_.train_bucket_lstm_bound = False
    return net


def step(model, net, x, label, lens, frames, case=None):
    import eabnet_amd
    for p in net.parameters():
        p.grad = None
    out = net(x) if lens is None else net(x, lengths=lens)
    if model == "eabnet":
        eabnet_amd.com_mag_mse_loss(out, label, frames).backward()
    else:
        eabnet_amd.eabnet_with_postnet_loss(out, label, frames)["final"].backward()


def timed(fn, steps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def summary(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def batch(dev, width=T, frames=MIXED, seed=1):
    import torch
    g = torch.Generator().manual_seed(seed)
    x = (0.3 * torch.randn(B, width, F, M, 2, generator=g)).to(dev)
    label = (0.3 * torch.randn(B, 2, width, F, generator=g)).to(dev)
    for b, n in enumerate(frames):                     # what lies behind an utterance is zeros, as a loader pads
        x[b, n:] = 0.0
        label[b, :, n:] = 0.0
    return x, label


def step_times(dev, model, precision, rounds, steps):
    import torch
    from eabnet_amd import train as tr
    x, label = batch(dev)
    lens = torch.tensor(MIXED, dtype=torch.int32, device=dev)
    nets = {c: make_net(model, dev, precision, c) for c in CASES}
    runs = {c: (lambda c=c: step(model, nets[c], x, label, lens, MIXED, c)) for c in CASES}
    if model == "two_stage":
        plain = make_net(model, dev, precision, None)
        singles = [(x[b:b + 1, :n].contiguous(), label[b:b + 1, :, :n].contiguous(), n) for b, n in enumerate(MIXED)]
        runs["padded_no_lengths"] = lambda: step(model, plain, x, label, None, [T] * B)
        runs["six_b1"] = lambda: [step(model, plain, xs, ls, None, [n]) for xs, ls, n in singles]
    for fn in runs.values():                           # warm-up: lowering, capture, code objects -- every program
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):                            # alternating inside every round
        for k, fn in runs.items():
            times[k].append(timed(fn, steps))
    r = {k: summary(v) for k, v in times.items()}
    for c in CASES[1:]:
        r[f"{c}_over_exact"] = round(r[c]["median_ms"] / r["exact"]["median_ms"], 4)
    r["lstm_bound_saves_ms"] = round(r["cap1024_lstm_walks_cap"]["median_ms"] - r["cap1024"]["median_ms"], 3)
    if model == "two_stage":
        r["six_b1_over_cap640"] = round(r["six_b1"]["median_ms"] / r["cap640"]["median_ms"], 3)
    stage = nets["cap1024"] if model == "eabnet" else nets["cap1024"].eabnet
    (key,) = stage._train_bound
    assert key[1] == 1024 and key[-1] is True and tr.OP_LSTM_TRAIN in {op.kind for op in stage._train_bound[key].prog.fwd}
    return r


def width_sweep(dev, precision):
    """eight batches of distinct padded widths, one step each, on a fresh module: host clock from the call to the synchronise
    after the backward, so lowering, binding and graph capture are inside"""
    import torch
    out = {}
    for tag, case in (("buckets_640", "cap640"), ("exact_width", "exact")):
        net = make_net("eabnet", dev, precision, case)
        per = []
        for width, seed in SWEEP:
            frames = [max(width - 53 * b, 40) for b in range(B)]
            x, label = batch(dev, width, frames, seed)
            lens = torch.tensor(frames, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step("eabnet", net, x, label, lens, frames, case)
            torch.cuda.synchronize()
            per.append(round(time.perf_counter() - t0, 3))
        out[tag] = {"per_step_s": per, "total_s": round(sum(per), 3), "programs_resident_at_the_end": len(net._train_bound)}
        del net
        gc.collect()
        torch.cuda.synchronize()
    out["widths"] = [w for w, _ in SWEEP]
    out["exact_over_buckets"] = round(out["exact_width"]["total_s"] / out["buckets_640"]["total_s"], 2)
    return out


def profile_case(dev, model, precision, case):
    import torch
    x, label = batch(dev)
    lens = torch.tensor(MIXED, dtype=torch.int32, device=dev)
    net = make_net(model, dev, precision, case)
    for m_ in ([net] if model == "eabnet" else [net.eabnet, net.postnet]):
        m_.use_graph = False                           # direct launches: every kernel is a record of its own
    for _ in range(PROFILE_WARMUP + PROFILE_STEPS):
        step(model, net, x, label, lens, MIXED, case)
    torch.cuda.synchronize()
    print(json.dumps({"profiled": case, "model": model, "precision": precision, "steps": PROFILE_WARMUP + PROFILE_STEPS}))


# kernel base name -> kind (what DESIGN §4.27's table is about: which launches follow the lengths and which walk the cap)
KINDS = (("lstm64_bwd", "lstm backward"), ("lstm64", "lstm forward"), ("conv_gemm", "convolutions"), ("conv_st", "convolutions"),
         ("wgrad", "weight gradients"), ("in_stats", "norm statistics / backward (masked)"), ("norm_bwd", "norm statistics / backward (masked)"),
         ("in_finalize", "norm statistics / backward (masked)"), ("layernorm_bwd", "norm statistics / backward (masked)"),
         ("filter_sum_ld", "filter-and-sum, pack, crm (masked)"), ("gag_", "filter-and-sum, pack, crm (masked)"),
         ("tr_norm_act", "row-local"), ("glu_bwd", "row-local"), ("gate_", "row-local"), ("add_kernel", "row-local"),
         ("relu_bwd", "row-local"), ("layernorm_fwd", "row-local"), ("filter_sum_bwd", "row-local"))


def summarize(dirs):
    """ms per step and kernel kind from the *_kernel_stats.csv of one --profile-case run per directory"""
    out = {}
    for d in dirs:
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        assert files, f"no kernel_stats.csv under {d}"
        kinds, total = {}, 0.0
        for fn in files:
            with open(fn, newline="") as f:
                for row in csv.DictReader(f):
                    name = re.sub(r"^void ", "", row["Name"])
                    ms = float(row["TotalDurationNs"]) * 1e-6 / (PROFILE_WARMUP + PROFILE_STEPS)
                    kind = next((k for p, k in KINDS if name.startswith(p)), "other (loss, gather, zero fill, torch)")
                    kinds[kind] = kinds.get(kind, 0.0) + ms
                    total += ms
        out[os.path.basename(os.path.normpath(d))] = dict({k: round(v, 3) for k, v in sorted(kinds.items(), key=lambda kv: -kv[1])},
                                                          total_kernel_ms=round(total, 3))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--models", default="eabnet,two_stage")
    ap.add_argument("--precisions", default="f32,bf16")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--profile-case", choices=CASES)
    ap.add_argument("--model", default="eabnet", choices=("eabnet", "two_stage"))
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16"))
    ap.add_argument("--summarize", nargs="+", metavar="DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_buckets_bench.json"))
    args = ap.parse_args()
    if args.summarize:
        res = {"kernel_ms_per_step": summarize(args.summarize)}
    else:
        import torch
        from eabnet_amd import train as tr
        assert torch.cuda.is_available(), "this benchmark measures the MI355X: no device, no numbers"
        dev = torch.device("cuda:0")
        if args.profile_case:
            profile_case(dev, args.model, args.precision, args.profile_case)
            return
        res = {"shape": {"B": B, "M": M, "T": T, "mixed_frames": MIXED, "valid_share": round(sum(MIXED) / (B * T), 3)},
               "rounds": args.rounds, "steps_per_round": args.steps}
        tr.TRAIN_BOUND_CACHE = 8                       # the six B = 1 programs stay resident next to the padded one
        for model in args.models.split(","):
            for precision in args.precisions.split(","):
                res[f"{model}_{precision}"] = step_times(dev, model, precision, args.rounds, args.steps)
                print(model, precision, json.dumps(res[f"{model}_{precision}"]), flush=True)
                gc.collect()
                torch.cuda.synchronize()
        tr.TRAIN_BOUND_CACHE = 3                       # the package's own value: the exact-width path evicts as a user's would
        if not args.no_sweep:
            res["width_sweep_f32"] = width_sweep(dev, "f32")
            print("sweep", json.dumps(res["width_sweep_f32"]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
