#!/usr/bin/env python
"""Scoring a folder of files: ``eabnet_amd.Scorer`` (scores on the device, one copy to the host) against ``Enhancer`` alone on the
same files (what scoring adds) and against the reference-style loop (one file at a time, ``.cpu().numpy()``, numpy ratios).

    python tools/bench_score.py [--files 50] [--max-batch 16] [--rounds 3] [--model eabnet|two_stage] [--out FILE]
                                [--seconds S] [--intelligibility]

50 seeded file lengths of 2-10 s (the seeds of tools/bench_enhance.py), M = 8, fp32, default configuration, device-resident noisy
and clean waves.  One process: a warm-up pass of each of the three (programs lowered and bound), then ``--rounds`` rounds that
alternate them, a device synchronisation around every timed window; the median round is reported.  The reference-style loop is
test.py:175-198 with the loss of evaluate(): per file ``stft_compress -> model (length_buckets="auto") -> istft`` at B = 1,
``com_mag_mse_loss`` against the file's label, the three arrays copied to the host and scored in float64 numpy.

``--seconds S``: every file S seconds long instead of the seeded 2-10 s.  ``--intelligibility``: the three runs become ``Scorer``,
``Scorer(intelligibility=True)`` and ``Enhancer`` (no reference-style loop): ms per batch with and without the STOI / ESTOI columns,
what they add, and next to them the host time of the float64 numpy restatement (tests/stoi_ref.py) on the same files -- the
enhanced and clean waves already resampled to 10 kHz on the device and copied to the host outside the timed window -- as a
stand-in for a host STOI library, which is not installed here.

``--kernels-only``: nothing but 20 calls of each of the two score kernels on a batch of 16 files of 10 s, for a
``rocprofv3 --kernel-trace --stats`` run of its own.

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


def numpy_ratios(est, clean, noisy):
    """cal_single_metrics' zero extension and the energy ratios plus the mixture's SI-SDR, float64 on the host"""
    n = max(len(est), len(clean), len(noisy))
    e, s, y = (np.concatenate([v.astype(np.float64), np.zeros(n - len(v))]) for v in (est, clean, noisy))
    d = y - s
    target = np.dot(e, s) / np.dot(s, s) * s
    noise = np.dot(e, d) / np.dot(d, d) * d
    art = e - target - noise
    pw = lambda v: float(np.dot(v, v))  # noqa: E731
    mix = np.dot(y, s) / np.dot(s, s) * s
    return [10 * np.log10(pw(target) / pw(noise + art)), 10 * np.log10(pw(target) / pw(noise)),
            10 * np.log10(pw(target) / pw(art)), 10 * np.log10(pw(mix) / pw(mix - y))]


def reference_style(net, noisy, clean, window):
    rows = []
    with torch.no_grad():
        for x, c in zip(noisy, clean):
            y = net(eabnet_amd.stft_compress(x[None], FFT, HOP, window))
            y = y["esti_stft"] if isinstance(y, dict) else y
            label = eabnet_amd.stft_compress(c[None, None], FFT, HOP, window, 1)
            loss = eabnet_amd.com_mag_mse_loss(y, label, [y.shape[2]])
            wav = eabnet_amd.istft(y, FFT, HOP, window)[0]
            rows.append(numpy_ratios(wav.cpu().numpy(), c.cpu().numpy(), x[0].cpu().numpy()) + [loss.item()])
    return np.array(rows)


def intelligibility_columns(both, noisy, clean, last, times, batches: int) -> dict:
    """ms per batch with and without the STOI / ESTOI columns, and the float64 numpy restatement of the same scores on the host"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import stoi_ref
    _, waves = both(noisy, clean, return_waves=True)
    pairs = [(eabnet_amd.resample(w[None], 16000, 10000)[0].cpu().numpy(), eabnet_amd.resample(c[None], 16000, 10000)[0].cpu().numpy())
             for w, c in zip(waves, clean)]
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref = np.stack([stoi_ref.intelligibility(e, c) for e, c in pairs])
        host.append(time.perf_counter() - t0)
    got = np.stack([last["scorer_intelligibility"][m] for m in ("stoi", "estoi")], axis=1)
    same = all(np.array_equal(last["scorer"][m], last["scorer_intelligibility"][m]) for m in last["scorer"])
    with_ms, without_ms = (1e3 * float(np.median(times[k])) / batches for k in ("scorer_intelligibility", "scorer"))
    return {"ms_per_batch": round(without_ms, 3), "ms_per_batch_with_intelligibility": round(with_ms, 3),
            "intelligibility_adds_ms_per_batch": round(with_ms - without_ms, 3),
            "intelligibility_adds_percent": round(100.0 * (with_ms / without_ms - 1.0), 2),
            "first_five_columns_unchanged": bool(same),
            "host_float64_numpy_restatement_ms": round(1e3 * float(np.median(host)), 1),
            "host_float64_numpy_restatement_ms_per_file": round(1e3 * float(np.median(host)) / len(pairs), 2),
            "max_score_diff_vs_restatement": float(np.abs(got - ref).max()),
            "stoi": [round(float(v), 4) for v in got[:4, 0]], "estoi": [round(float(v), 4) for v in got[:4, 1]]}


def kernels_only(dev) -> None:
    B, L, T = 16, 160000, 1001
    g = torch.Generator().manual_seed(0)
    s, n = torch.randn(B, L, generator=g).to(dev), torch.randn(B, L, generator=g).to(dev)
    est = (0.8 * s + 0.2 * n)[:, :HOP * (T - 1)].contiguous()
    e, lab = torch.randn(B, 2, T, 161, generator=g).to(dev), torch.randn(B, 2, T, 161, generator=g).to(dev)
    frames = torch.full((B,), T, device=dev)
    for _ in range(20):
        eabnet_amd.energy_ratios(est, s, s + n)
        eabnet_amd.com_mag_mse_loss_per_utterance(e, lab, frames)
    torch.cuda.synchronize()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=50)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", choices=("eabnet", "two_stage"), default="eabnet")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--seconds", type=float, default=None)
    ap.add_argument("--intelligibility", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.kernels_only:
        kernels_only(dev)
        return
    M = 8
    seconds = np.random.default_rng(1234).uniform(2.0, 10.0, size=args.files)
    if args.seconds is not None:
        seconds = np.full(args.files, args.seconds)
    samples = [int(s * 16000) for s in seconds]
    g = torch.Generator().manual_seed(0)
    clean = [(0.05 * torch.randn(n, generator=g)).to(dev) for n in samples]
    noisy = [(c[None].cpu() + 0.05 * torch.randn(M, n, generator=g)).to(dev) for c, n in zip(clean, samples)]
    window = torch.hann_window(FFT)
    model = eabnet_amd.EaBNet(M=M) if args.model == "eabnet" else eabnet_amd.make_eabnet_with_postnet(two_stage_args(M))
    model = model.to(dev).eval()
    fresh(model)
    scorer = eabnet_amd.Scorer(model, max_batch=args.max_batch)
    enhancer = eabnet_amd.Enhancer(model, max_batch=args.max_batch)

    def loop():
        model.length_buckets = "auto"
        try:
            return reference_style(model, noisy, clean, window)
        finally:
            model.length_buckets = None

    runs = {"scorer": lambda: scorer(noisy, clean), "enhancer": lambda: enhancer(noisy), "reference_style": loop}
    if args.intelligibility:
        both = eabnet_amd.Scorer(model, max_batch=args.max_batch, intelligibility=True)
        runs = {"scorer": runs["scorer"], "scorer_intelligibility": lambda: both(noisy, clean), "enhancer": runs["enhancer"]}
    cold = {k: timed(fn)[0] for k, fn in runs.items()}                     # warm-up: lowering, binding, capture
    times = {k: [] for k in runs}
    last = {}
    for _ in range(args.rounds):
        for k, fn in runs.items():                                         # alternating, one process
            t, last[k] = timed(fn)
            times[k].append(t)
    res = {"files": args.files, "max_batch": args.max_batch, "model": args.model, "rounds": args.rounds,
           "frames_total": sum(1 + n // HOP for n in samples),
           "batches": [(len(b["indices"]), b["cap"], b["batch_size"], b["dummies"]) for b in scorer.last_plan["batches"]]}
    if args.intelligibility:
        res.update(intelligibility_columns(both, noisy, clean, last, times, len(res["batches"])))
    else:
        got = np.stack([last["scorer"][m] for m in ("si_sdr", "si_sir", "si_sar", "si_sdr_mix", "loss")], axis=1)
        ref = last["reference_style"]
        res["max_db_diff_vs_reference_style"] = float(np.abs(got[:, :4] - ref[:, :4]).max())
        res["max_rel_loss_diff_vs_reference_style"] = float(np.abs(got[:, 4] / ref[:, 4] - 1.0).max())
    for k in runs:
        med = float(np.median(times[k]))
        res[k] = {"cold_s": round(cold[k], 3), "warm_s": [round(t, 4) for t in times[k]], "files_per_s": round(args.files / med, 1),
                  "ms_per_file": round(1e3 * med / args.files, 3)}
    res["scoring_adds_ms_per_file"] = round(res["scorer"]["ms_per_file"] - res["enhancer"]["ms_per_file"], 3)
    if args.intelligibility:
        res["scoring_with_intelligibility_adds_ms_per_file"] = round(
            res["scorer_intelligibility"]["ms_per_file"] - res["enhancer"]["ms_per_file"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
