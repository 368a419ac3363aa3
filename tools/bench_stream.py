#!/usr/bin/env python
"""Streams of any length: what the resident window costs per hop.

    python tools/bench_stream.py [--out FILE]

BASELINE config 5's shape (B = 1, M = 16, BatchNorm norms, chunk = 1), fp32 and bf16, in one process:

  plain          stream_begin(T_max=801): the whole utterance resident, stops after 801 frames (the yardstick)
  endless_min    stream_begin(T_max=2 * history + 1, endless=True): the smallest window, a move every history + 1 frames
  endless_801    stream_begin(T_max=801, endless=True): the plain stream's window, a move every 673 frames

Three rounds per stream -- 2,000 steps for the endless ones, 800 for the plain one with a reset() between rounds, since it
cannot go further.  A step is timed on the host from the call to the end of a device synchronise (what a real-time caller
waits for).  Reported per stream: the median of every round, the median and the worst step over all rounds, the same for
the steps that moved the window first, and the activation-arena bytes; and the time of the move alone (eab_shift_rows_f32
back to back between device events, and one launch to its synchronise).  Prints one JSON object (and writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import eabnet_amd  # noqa: E402

WARMUP = 20          # steps of the first round left out (first replays: code objects, clocks)


def run_round(st, frames, steps: int):
    """[(milliseconds, moved the window first)] of `steps` steps"""
    out = []
    for k in range(steps):
        x = frames[k % len(frames)]
        moves = st.endless and st.pos + st.chunk > st.T_max
        t0 = time.perf_counter()
        st.step(x)
        torch.cuda.synchronize()
        out.append(((time.perf_counter() - t0) * 1e3, moves))
    return out


def summary(rounds) -> dict:
    every = [r for rnd in rounds for r in rnd]
    ms = [t for t, _ in every]
    moved = [t for t, m in every if m]
    plain = [t for t, m in every if not m]
    res = {"round_median_ms": [round(statistics.median(t for t, _ in rnd), 4) for rnd in rounds],
           "median_ms": round(statistics.median(ms), 4), "worst_ms": round(max(ms), 4), "steps": len(ms),
           "median_no_move_ms": round(statistics.median(plain), 4)}
    if moved:
        res.update(moves=len(moved), move_step_median_ms=round(statistics.median(moved), 4), move_step_worst_ms=round(max(moved), 4))
    return res


def move_alone(st, reps: int = 200) -> dict:
    """the move launch on its own, at the position where the stream makes it (it copies rows the stream has written; the
    stream is reset afterwards)"""
    bound, src = st.bound, st.T_max
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(5):
        bound.rebase(src, stream)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        bound.rebase(src, stream)
    b.record()
    torch.cuda.synchronize()
    single = []
    for _ in range(reps):
        t0 = time.perf_counter()
        bound.rebase(src, stream)
        torch.cuda.synchronize()
        single.append((time.perf_counter() - t0) * 1e3)
    st.reset()
    table = bound.prog.carry
    return {"tensors": len(table), "bytes_per_utterance": sum(4 * row * rows for _, row, rows in table),
            "back_to_back_us": round(a.elapsed_time(b) / reps * 1e3, 2), "launch_to_sync_median_us": round(statistics.median(single) * 1e3, 2)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2000, help="steps per round of the endless streams")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stream.py measures on the MI355X"
    dev = torch.device("cuda:0")
    B, M, T = 1, 16, 801
    torch.manual_seed(0)
    net = eabnet_amd.EaBNet(M=M, norm_type="BN").to(dev).eval()
    frames = [(0.3 * torch.randn(B, 1, 161, M, 2)).to(dev) for _ in range(64)]
    res = {"B": B, "M": M, "norm": "BN", "chunk": 1, "rounds": args.rounds, "warmup_steps": WARMUP}
    for prec in ("f32", "bf16"):
        net.precision = prec
        plain = net.stream_begin(B, T_max=T, chunk=1)
        window = 2 * plain.history + 1
        streams = {"plain": (plain, T - 1),
                   "endless_min": (net.stream_begin(B, T_max=window, chunk=1, endless=True), args.steps),
                   "endless_801": (net.stream_begin(B, T_max=T, chunk=1, endless=True), args.steps)}
        rows = {}
        for name, (st, steps) in streams.items():
            rounds = []
            for r in range(args.rounds):
                if not st.endless:
                    st.reset()
                rnd = run_round(st, frames, steps)
                rounds.append(rnd[WARMUP:] if r == 0 else rnd)
            rows[name] = summary(rounds)
            rows[name].update(T_max=st.T_max, history=st.history, arena_bytes=4 * st.bound.acts.numel())
            print(prec, name, rows[name], flush=True)
        meds = rows["plain"]["round_median_ms"]
        rows["plain_round_spread_ms"] = round(max(meds) - min(meds), 4)
        rows["move"] = move_alone(streams["endless_min"][0])
        print(prec, "move", rows["move"], flush=True)
        res[prec] = rows
        del streams, plain
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
