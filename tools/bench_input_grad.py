#!/usr/bin/env python
"""Input gradients (EaBNet.input_grad, stft_compress under autograd): what they cost.

    python tools/bench_input_grad.py [--rounds 5] [--steps 8] [--out profiles/input_grad_bench.json]

Device events around `steps` steps, after warm-up of every shape; `rounds` repetitions, the sides of a comparison alternating
inside every round; reported: the median and the (min, max) of the per-round times.

1. training step (forward, com_mag_mse_loss, backward) at the shape of BASELINE configs[3] (6 utterances, 8 microphones,
   T = 601 frames), fp32 and bf16, in one process: the switch off (an input that needs no gradient: the program as it always
   was -- the comparison) against the switch on with an input that requires grad; and the device time of the added launches
   alone (direct launches of the bound backward program, one event pair around them)
2. eab_stft_compress_bwd_f32 alone at B = 6, M = 8, 6 s, against the backward of torch.stft + X |X|^-1/2 under torch autograd on
   the same device
3. the wave-to-loss step (wav -> stft_compress -> net -> istft -> si_sdr_loss -> backward) with a wave leaf against the same
   step with the spectrogram detached (no gradient in front of the network)

Prints one JSON object (and writes it to --out)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import eabnet_amd  # noqa: E402
from eabnet_amd import _lib  # noqa: E402
from eabnet_amd import model as mdl  # noqa: E402
from eabnet_amd import train as tr  # noqa: E402

B, M, T, F = 6, 8, 601, 161
N_FFT, HOP, SR = 320, 160, 16000


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def compare(runs, rounds, steps, warm=3):
    for fn in runs.values():                           # warm-up: lowering, capture, code objects -- every side
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):                            # alternating inside every round
        for k, fn in runs.items():
            times[k].append(timed(fn, steps))
    return {k: summary(v) for k, v in times.items()}


def train_step(net, x, label):
    for p in net.parameters():
        p.grad = None
    x.grad = None
    eabnet_amd.com_mag_mse_loss(net(x), label, [T] * B).backward()


def added_launches_ms(net, x, rounds):
    """device time of the launches input_grad adds to the backward program: direct launches on the bound program of the
    switched-on step, whose activations the last step left in place"""
    bound = next(b for k, b in net._train_bound.items() if "input_grad" in k)
    ops = bound.lists["bwd"]
    idx = [k for k, o in enumerate(ops) if ".dgrad_in." in o.name or o.name == "input_grad"]
    assert idx == list(range(idx[0], idx[0] + len(idx)))
    io = (x.detach(), torch.empty(B, 2, T, F, device=x.device), torch.randn(B, 2, T, F, device=x.device), None, torch.empty_like(x))
    bound._ptrs = None
    bound.bind(*(None if t is None else t.data_ptr() for t in io))
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for name, first, n in [("dgrad_in", idx[0], len(idx) - 1), ("input_grad", idx[-1], 1)]:
        bound.run("bwd", st, first, n)
        out[name] = summary([timed(lambda: bound.run("bwd", st, first, n), 20) for _ in range(rounds)])
    bound._ptrs = None                                 # (the next captured replay binds its static buffers again)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_grad_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X: no device, no numbers"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    x = (0.3 * torch.randn(B, T, F, M, 2, generator=g)).to(dev)
    label = (0.3 * torch.randn(B, 2, T, F, generator=g)).to(dev)
    res = {"shape": {"B": B, "M": M, "T": T}, "rounds": args.rounds, "steps_per_round": args.steps}

    # 1. the training step, switch off and on
    for precision in ("f32", "bf16"):
        torch.manual_seed(0)
        net = eabnet_amd.EaBNet(M=M).to(dev).train()
        net.precision, net.input_grad = precision, True
        x_leaf = x.clone().requires_grad_(True)
        r = compare({"off": lambda: train_step(net, x, label), "on": lambda: train_step(net, x_leaf, label)}, args.rounds, args.steps)
        assert len(net._train_bound) == 2 and x_leaf.grad is not None
        r["on_minus_off_ms"] = round(r["on"]["median_ms"] - r["off"]["median_ms"], 4)
        r["on_over_off"] = round(r["on"]["median_ms"] / r["off"]["median_ms"], 4)
        r["added_launches"] = added_launches_ms(net, x_leaf, args.rounds)
        res[precision] = r
        print(precision, json.dumps(r), flush=True)
        del net
        torch.cuda.synchronize()

    # 2. the front end's adjoint alone
    Bw, L = 6, 6 * SR
    wav = (0.1 * torch.randn(Bw, M, L, generator=g)).to(dev)
    window = torch.hann_window(N_FFT, device=dev)
    spec = eabnet_amd.stft_compress(wav, N_FFT, HOP, window)
    dspec = torch.randn_like(spec)
    dwav = torch.empty_like(wav)
    lib, tw = _lib.load(), mdl._twiddle(N_FFT, dev)

    def kernel():
        _lib.check(lib.eab_stft_compress_bwd_f32(dspec.data_ptr(), spec.data_ptr(), window.data_ptr(), tw.data_ptr(), dwav.data_ptr(),
                                                 None, Bw, M, L, N_FFT, HOP, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    wl = wav.clone().requires_grad_(True)
    X = torch.stft(wl.reshape(Bw * M, L), N_FFT, hop_length=HOP, win_length=N_FFT, window=window, center=True, pad_mode="reflect",
                   return_complex=True)
    s = torch.view_as_real(X * X.abs().pow(-0.5))
    cot = torch.randn_like(s)

    def torch_bwd():
        wl.grad = None
        s.backward(cot, retain_graph=True)
    r = compare({"kernel": kernel, "torch_autograd_backward": torch_bwd}, args.rounds, 20)
    r["bytes_moved_MB"] = round((2 * spec.numel() + wav.numel()) * 4 / 1e6, 1)
    r["kernel_GBps"] = round(r["bytes_moved_MB"] / r["kernel"]["median_ms"], 1)
    res["stft_compress_bwd"] = dict(r, shape={"B": Bw, "M": M, "L": L})
    print("stft_compress_bwd", json.dumps(r), flush=True)

    # 3. wave to loss, with and without the gradient in front of the network
    torch.manual_seed(0)
    net = eabnet_amd.EaBNet(M=M).to(dev).train()
    net.input_grad = True
    clean = (0.1 * torch.randn(Bw, HOP * (1 + L // HOP - 1), generator=g)).to(dev)

    def wave_step(leaf):
        for p in net.parameters():
            p.grad = None
        w = wav.clone().requires_grad_(leaf)
        sp = eabnet_amd.stft_compress(w, N_FFT, HOP, window)
        est = eabnet_amd.istft(net(sp), N_FFT, HOP, window)
        eabnet_amd.si_sdr_loss(est, clean, eps=1e-8).backward()
    r = compare({"detached_input": lambda: wave_step(False), "wave_leaf": lambda: wave_step(True)}, args.rounds, args.steps)
    r["leaf_minus_detached_ms"] = round(r["wave_leaf"]["median_ms"] - r["detached_input"]["median_ms"], 4)
    res["wave_to_loss"] = dict(r, shape={"B": Bw, "M": M, "L": L})
    print("wave_to_loss", json.dumps(r), flush=True)

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
