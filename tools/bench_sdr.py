#!/usr/bin/env python
"""What the BSS-eval SDR costs: the value, value plus gradient, inside ``Scorer`` and inside a training step, each against its
comparator in the same run, and the three kernels' own times from one kernel trace.

    python tools/bench_sdr.py [--rounds 5] [--iters 20] [--sections value,loss,scorer,step] [--trace-dir DIR] [--out profiles/sdr_bench.json]

  value     ``sdr`` on sixteen 6 s rows at 16 kHz (est a hop shorter than clean), 512 and 64 taps
  loss      ``sdr_loss(...).backward()`` on six such rows, 512 taps
  operator  the same definition in torch operators on the device, float64: ``torch.fft`` correlations, ``torch.linalg.solve`` on the
            Toeplitz matrix, under autograd for the loss -- the comparator: in this tool only, never in the package
  scorer    ``Scorer(model)`` against ``Scorer(model, distortion=True)`` on sixteen 6 s files of 8 microphones, host clock around a
            call (it ends in the call's one device-to-host copy)
  step      the training step of bench.py --train (B = 6, 6 s, FlatAdam(5e-4, clip 1.0)) on two copies of the model:
            com_mag_mse_loss alone, and plus 0.05 * sdr_loss(istft(out), target)
Device time between two HIP events around ``--iters`` back-to-back calls after warm-up, the two sides alternating ``--rounds``
times: medians of the rounds with their min and max.  ``--trace-dir``: one more child process under
``rocprofv3 --kernel-trace --stats`` runs the value and the gradient a few times; the three kernels' rows of its statistics are
added.  Prints one JSON object (and writes it to --out when given; with ``--sections`` a subset is measured again and replaces
those sections of an existing --out file, each section carrying its own ``rounds``)."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import eabnet_amd  # noqa: E402

SECONDS, WEIGHT = 6.0, 0.05
KERNELS = ("sdr_corr_kernel", "sdr_solve_kernel", "sdr_bwd_kernel")


def _stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def rows(B: int, dev):
    """(est (B, L - hop), clean (B, L)): est is clean 5 samples late plus noise at about 10 dB"""
    L = int(SECONDS * bench.SR)
    g = torch.Generator().manual_seed(7)
    t = torch.arange(L) / bench.SR
    clean = 0.1 * torch.randn(B, L, generator=g) * (0.6 + 0.4 * torch.sin(2 * torch.pi * 3.0 * t))
    clean = clean + 0.9 * torch.roll(clean, 1, 1) + 0.5 * torch.roll(clean, 2, 1)                 # (coloured)
    est = torch.roll(clean, 5, 1) + 0.3 * clean.std() * torch.randn(B, L, generator=g)
    return est[:, :L - bench.HOP].contiguous().to(dev), clean.to(dev)


def operator_sdr(est, clean, K: int):
    """the definition in float64 torch operators -> (sdr (B,) in dB, tgt, ee)"""
    L = clean.shape[1]
    e, s = torch.nn.functional.pad(est.double(), (0, L - est.shape[1])), clean.double()
    n = L + K
    Sf, Ef = torch.fft.rfft(s, n), torch.fft.rfft(e, n)
    r = torch.fft.irfft(Sf.conj() * Sf, n)[:, :K]
    c = torch.fft.irfft(Sf.conj() * Ef, n)[:, :K]
    idx = (torch.arange(K, device=est.device)[:, None] - torch.arange(K, device=est.device)[None, :]).abs()
    h = torch.linalg.solve(r[:, idx], c)
    tgt, ee = (c * h).sum(1), (e * e).sum(1)
    return 10.0 * torch.log10(tgt / (ee - tgt)), tgt, ee


def operator_loss(est, clean, K: int):
    return -operator_sdr(est, clean, K)[0].mean()


def timed(fn, iters: int) -> float:
    """milliseconds per call between two HIP events over back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(sides: dict, rounds: int, iters: int) -> dict:
    for fn in sides.values():
        for _ in range(3):
            fn()
    got = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            got[k].append(timed(fn, iters))
    return {k: _stats(v) for k, v in got.items()}


def value(dev, rounds: int, iters: int) -> dict:
    est, clean = rows(16, dev)
    out = {"rows": 16, "samples": [est.shape[1], clean.shape[1]]}
    for K in (512, 64):
        ours, theirs = eabnet_amd.sdr(est, clean, filter_length=K), operator_sdr(est, clean, K)[0]
        res = alternate({"sdr_ms": lambda: eabnet_amd.sdr(est, clean, filter_length=K),
                         "operator_ms": lambda: operator_sdr(est, clean, K)}, rounds, iters)
        res["max_abs_diff_db"] = float((ours - theirs).abs().max())
        res["sdr_db_row0"] = float(ours[0])
        out[f"taps_{K}"] = res
    return out


def loss(dev, rounds: int, iters: int) -> dict:
    est, clean = rows(6, dev)
    K = 512

    def fused():
        leaf = est.detach().requires_grad_(True)
        eabnet_amd.sdr_loss(leaf, clean, filter_length=K).backward()
        return leaf.grad

    def operator():
        leaf = est.detach().requires_grad_(True)
        operator_loss(leaf, clean, K).backward()
        return leaf.grad

    gf, go = fused(), operator()
    res = alternate({"sdr_loss_ms": fused, "operator_ms": operator}, rounds, iters)
    res.update(rows=6, taps=K, gradient_max_diff_over_max=float((gf - go).abs().max() / go.abs().max()))
    return res


def scorer(dev, rounds: int) -> dict:
    net, _ = bench.make_model(bench.MICS, dev)
    net.eval()
    L = int(SECONDS * bench.SR)
    noisy = [w for w in bench.synth_waves(16, bench.MICS, L, 1234)]
    clean = [0.7 * x[0] + 0.3 * c[0] for x, c in zip(noisy, bench.synth_waves(16, 1, L, 4321))]
    sides = {"scorer_ms": eabnet_amd.Scorer(net, max_batch=16), "scorer_distortion_ms": eabnet_amd.Scorer(net, max_batch=16, distortion=True)}
    got = {k: [] for k in sides}
    for s in sides.values():
        for _ in range(3):
            s(noisy, clean)
    for _ in range(rounds):
        for k, s in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s(noisy, clean)
            got[k].append(1e3 * (time.perf_counter() - t0))
    res = {k: _stats(v) for k, v in got.items()}
    res.update(files=16, microphones=bench.MICS, seconds=SECONDS, rounds=rounds,
               distortion_minus_plain_ms=res["scorer_distortion_ms"]["median"] - res["scorer_ms"]["median"])
    return res


def step(dev, rounds: int, block_steps: int) -> dict:
    B, L = 6, int(SECONDS * bench.SR)
    T = 1 + L // bench.HOP
    pd_args = argparse.Namespace(mics=bench.MICS, sr=bench.SR, wav_len=SECONDS, win_size=0.020, win_shift=0.010, fft_num=bench.N_FFT)
    wav, tgt = bench.synth_waves(B, bench.MICS, L, 1234).to(dev), bench.synth_waves(B, 1, L, 4321).to(dev)
    window = torch.hann_window(bench.N_FFT, device=dev)
    nets, opts = {}, {}
    for name in ("spectral_ms", "with_sdr_loss_ms"):
        nets[name], _ = bench.make_model(bench.MICS, dev)
        nets[name].train()
        opts[name] = eabnet_amd.FlatAdam(list(nets[name].parameters()), lr=5e-4, max_grad_norm=1.0)

    def one(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opts[name].zero_grad(set_to_none=True)
        noisy, target = eabnet_amd.prepare_data(wav, tgt, dev, pd_args)
        out = nets[name](noisy)
        total = eabnet_amd.com_mag_mse_loss(out, target, [T] * B)
        if name == "with_sdr_loss_ms":
            total = total + WEIGHT * eabnet_amd.sdr_loss(eabnet_amd.istft(out, bench.N_FFT, bench.HOP, window), tgt)
        total.backward()
        opts[name].step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(total)), "training diverged"
        return 1e3 * (time.perf_counter() - t0)

    for name in nets:
        for _ in range(3):
            one(name)
    got = {k: [] for k in nets}
    for _ in range(rounds):
        for name in nets:
            got[name].append(statistics.median(one(name) for _ in range(block_steps)))
    res = {k: _stats(v) for k, v in got.items()}
    res.update(batch=B, seconds=SECONDS, weight=WEIGHT, taps=512, steps_per_round=block_steps,
               with_minus_spectral_ms=res["with_sdr_loss_ms"]["median"] - res["spectral_ms"]["median"])
    return res


def kernels_section(dev) -> None:
    """what the traced child runs: the value on sixteen rows at 512 and 64 taps, value plus gradient on six"""
    est, clean = rows(16, dev)
    for _ in range(5):
        eabnet_amd.sdr(est, clean, filter_length=512)
        eabnet_amd.sdr(est, clean, filter_length=64)
        leaf = est[:6].detach().requires_grad_(True)
        eabnet_amd.sdr_loss(leaf, clean[:6]).backward()
    torch.cuda.synchronize()


def trace(directory: str) -> dict:
    os.makedirs(directory, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory, "-o", "sdr", "--",
           sys.executable, os.path.abspath(__file__), "--section", "kernels"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
    if r.returncode != 0:
        return {"error": f"rocprofv3 returned {r.returncode}", "stderr": r.stderr[-500:]}
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"error": "no kernel statistics written"}
    out = {"workload": "5 x (value 16 rows at 512 taps, value 16 rows at 64 taps, value + gradient 6 rows at 512 taps), 6 s rows"}
    for row in csv.DictReader(open(files[0])):
        for k in KERNELS:
            if k in row["Name"]:
                out[k] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                          "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--block-steps", type=int, default=4)
    ap.add_argument("--section", default="all", choices=("all", "kernels"))
    ap.add_argument("--sections", default="value,loss,scorer,step")
    ap.add_argument("--trace-dir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if a.section == "kernels":
        kernels_section(dev)
        return
    res = {"workload": f"{SECONDS:g} s rows at {bench.SR} Hz, est a hop shorter than clean; see the tool's docstring",
           "method": f"HIP events around {a.iters} back-to-back calls, sides alternating, {a.rounds} rounds: median, min, max of the rounds' "
                     "means (value, loss); host clock around a call that ends in a synchronise (scorer, step)",
           "rounds": a.rounds, "iters": a.iters}
    chosen = [s for s in a.sections.split(",") if s]
    if a.out and os.path.exists(a.out) and set(chosen) != {"value", "loss", "scorer", "step"}:
        with open(a.out) as f:
            res = json.load(f)
    for name, fn in (("value", lambda: value(dev, a.rounds, a.iters)), ("loss", lambda: loss(dev, a.rounds, a.iters)),
                     ("scorer", lambda: scorer(dev, a.rounds)), ("step", lambda: step(dev, a.rounds, a.block_steps))):
        if name not in chosen:
            continue
        res[name] = fn()
        print(name, json.dumps(res[name]), file=sys.stderr, flush=True)
    if a.trace_dir or "kernel_trace" not in res:
        res["kernel_trace"] = trace(a.trace_dir) if a.trace_dir else "not measured (no --trace-dir)"
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
