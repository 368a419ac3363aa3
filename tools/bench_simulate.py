#!/usr/bin/env python
"""Room simulation on the device: the three entry points of csrc/room.hip on the training workload.

    python tools/bench_simulate.py [--reps 5] [--method ism|ism_tail|both] [--train-step-ms MS] [--no-host | --host-only]
                                   [--out profiles/simulate_bench.json]

Workload: B = 6 utterances of 6 s at 16 kHz, the 8 microphones of the v3 array (tests/golden/mcse_dataset_settings_v3.json),
1 target + 4 noises per scene.  "settings": rooms and rt60 drawn from the settings with fixed seeds.  "worst": the same draws
with rt60 = 0.7 s for every scene (image orders 79 to 95, 0.7 to 1.2 million images per response).  Per entry point (gains,
impulse responses, convolution): ``reps`` back-to-back calls between two HIP events, best of three, in ms per batch; "all" is
``simulate_rooms`` as a whole (uploads of the scene records included).  --method picks the response model (DESIGN.md 4.18,
4.23); "both" times "ism" and "ism_tail" on the same draws in one session and nests the rows under the method's name.

What to hold it against: one training step of the same batch (``bench.py --train``, measured in the same session and handed in
with --train-step-ms): a batch made on RoomSimulator's side stream hides behind a step when "all" is below it.

Host stand-in: tests/room_ref.py (float64 numpy, scipy.signal.fftconvolve) on ONE host thread for the first "settings"
utterance.  It stands in for the host library the reference uses, which is not installed; it is NOT pyroomacoustics, whose
compiled image-source engine is faster than numpy's scatter-add.

Prints one JSON object (and writes it to --out when given)."""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eabnet_amd  # noqa: E402
from eabnet_amd import simulate as sim  # noqa: E402

B, SECONDS, FS, NOISES = 6, 6, 16000, 4


def events(fn, reps):
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
        best = min(best, e0.elapsed_time(e1) / reps)
    return best


def scenes_of(settings, rt60=None, method="ism"):
    st = copy.deepcopy(settings)
    st["noise"]["n"] = [NOISES, NOISES]
    if rt60 is not None:
        st["room"]["rt60"] = [rt60, rt60]
    return [sim.sample_scene(st, np.random.default_rng(1000 + b), rir_method=method) for b in range(B)]


def workload(name, scenes, x, dev, reps):
    L = x.shape[2]
    fs, M, S = sim._check_batch(scenes, x.shape[1])
    ks = sim.response_lengths(scenes)
    K = max(ks)
    lib = eabnet_amd._lib.load()
    method = scenes[0].rir_method
    records = sim._to_device(np.stack([sim._scene_record(sc) for sc in scenes]), dev)
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    klen = torch.tensor([[k, sim.first_arrival(sc)] for k, sc in zip(ks, scenes)], dtype=torch.int32, device=dev)
    nwin = sim._windows(L, fs)
    partial = torch.empty((B, nwin, sim.GAIN_SUMS), dtype=torch.float64, device=dev)
    gains = torch.empty((B, S), dtype=torch.float64, device=dev)
    h = torch.empty((B, S, M + 1, K), dtype=torch.float32, device=dev)
    wb = lib.eab_room_workspace_bytes(B, S, M, L, K)
    work = torch.empty((wb + 7) // 8, dtype=torch.float64, device=dev)
    noisy, clean = torch.empty((B, M, L), device=dev), torch.empty((B, 1, L), device=dev)
    tw = sim._twiddles(dev)

    def conv():
        eabnet_amd._lib.check(lib.eab_room_convolve_f32(x.data_ptr(), B, S, L, lens.data_ptr(), records.data_ptr(), klen.data_ptr(),
                                                        gains.data_ptr(), h.data_ptr(), M, K, tw.data_ptr(), work.data_ptr(), wb,
                                                        noisy.data_ptr(), clean.data_ptr(), sim._stream()))
    row = {"orders": [int(sc.max_order) for sc in scenes], "rt60": [round(float(sc.rt60), 3) for sc in scenes], "K": ks,
           "images_per_response": [(2 * o + 1) * (2 * o * o + 2 * o + 3) // 3 for o in (int(sc.max_order) for sc in scenes)],
           "workspace_MB": round(wb / 2 ** 20, 1), "responses_MB": round(h.numel() * 4 / 2 ** 20, 1)}
    if method == "ism_tail":                                           # what the launch adds instead: images inside r_mix, and the tail's
        row["tail_start"], row["tail_density"] = scenes[0].tail_start, scenes[0].tail_density
        row["tail_images_per_response"] = [int(np.ceil(sc.tail_density * max(0, k - sim.TAPS - int(sc.tail_start * sc.fs)))) for sc, k in zip(scenes, ks)]
    row["gains_ms"] = round(events(lambda: sim._launch_gains(x, lens, records, fs, partial, nwin, gains), reps), 3)
    row["rirs_ms"] = round(events(lambda: sim._launch_rirs(records, B, S, M, K, fs, h, method), reps), 3)
    row["convolve_ms"] = round(events(conv, reps), 3)
    row["all_ms"] = round(events(lambda: sim.simulate_rooms(x, scenes), reps), 3)
    print(name, row, flush=True)
    return row


def host_stand_in(scene, x):
    import room_ref as ref
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    h = ref.scene_rirs(scene)
    t1 = time.perf_counter()
    ref.simulate(scene, x, h)
    t2 = time.perf_counter()
    return {"what": "tests/room_ref.py (float64 numpy + scipy fftconvolve), one host thread, one utterance; a stand-in for the "
                    "host library the reference uses, not pyroomacoustics",
            "order": int(scene.max_order), "rirs_s": round(t1 - t0, 2), "gains_and_convolution_s": round(t2 - t1, 2),
            "utterance_s": round(t2 - t0, 2)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--train-step-ms", type=float, default=None, help="one training step of the same batch (bench.py --train)")
    ap.add_argument("--method", choices=["ism", "ism_tail", "both"], default="ism", help="the response model of the scenes")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-only", action="store_true", help="only the host stand-in (needs no GPU); merged into --out when it exists")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with open(os.path.join(ROOT, "tests", "golden", "mcse_dataset_settings_v3.json")) as f:
        settings = json.load(f)
    gen = torch.Generator().manual_seed(0)
    x = 0.05 * torch.randn(B, 1 + NOISES, SECONDS * FS, generator=gen)
    if args.host_only:
        res = {}
        if args.out and os.path.exists(args.out):
            with open(args.out) as f:
                res = json.loads(f.read())
        res["host_stand_in"] = host_stand_in(scenes_of(settings)[0], x[0].numpy().astype(np.float64))
        return finish(res, args.out)
    dev = torch.device("cuda:0")
    x = x.to(dev)
    res = {"workload": {"B": B, "seconds": SECONDS, "fs": FS, "mics": 8, "sources": 1 + NOISES}}
    draws = scenes_of(settings)
    if args.train_step_ms is not None:
        res["train_step_ms"] = args.train_step_ms
    for method in (["ism", "ism_tail"] if args.method == "both" else [args.method]):
        rows = res.setdefault(method, {}) if args.method == "both" else res
        rows["settings"] = workload(f"{method} settings", scenes_of(settings, method=method), x, dev, args.reps)
        rows["worst"] = workload(f"{method} worst", scenes_of(settings, 0.7, method=method), x, dev, max(1, args.reps // 2))
        if args.train_step_ms is not None:
            for k in ("settings", "worst"):
                rows[k]["hides_behind_a_step"] = bool(rows[k]["all_ms"] < args.train_step_ms)
                rows[k]["bound_by"] = max(("gains_ms", "rirs_ms", "convolve_ms"), key=lambda n: rows[k][n])
    if not args.no_host:
        res["host_stand_in"] = host_stand_in(draws[0], x[0].cpu().numpy().astype(np.float64))
        print("host", res["host_stand_in"], flush=True)
    finish(res, args.out)


def finish(res, out) -> None:
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
