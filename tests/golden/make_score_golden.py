"""Writes tests/golden/score_cases.npz: the reference's own ``metrics.energy_ratios`` / ``metrics.si_sdr`` on the seeded cases of
tests/score_ref.py, and its ``com_mag_mse_loss`` for each utterance of e2e_M8_B2_T20.npz alone.  Run once in the authoring
container; not run by the test-suite (the reference does not exist where the tests run).  Signals are regenerated from their
seeds, so the file holds lengths, seeds, gains and float64 results only."""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")

for name in ("pesq", "pystoi"):                  # metrics.py imports both at the top; energy_ratios needs neither
    if name not in sys.modules:
        stub = types.ModuleType(name)
        setattr(stub, "pesq" if name == "pesq" else "stoi", None)
        sys.modules[name] = stub

import metrics as ref_metrics  # noqa: E402  (reference)
from EaBNet import com_mag_mse_loss as ref_loss  # noqa: E402  (reference)
import paramgen  # noqa: E402
import score_ref  # noqa: E402


def main() -> None:
    cases = np.array([tuple(c) + (0,) * (8 - len(c)) for c in score_ref.CASES], dtype=np.float64)
    want = np.zeros((len(score_ref.CASES), 4))
    for k, c in enumerate(score_ref.CASES):
        clean, noisy, est = score_ref.make_case(*c)
        n = max(len(clean), len(noisy), len(est))
        gt, y, x = (np.concatenate([v.astype(np.float64), np.zeros(n - len(v))]) for v in (clean, noisy, est))   # test.py:126-138
        want[k, :3] = ref_metrics.energy_ratios(x, gt, y - gt)
        want[k, 3] = ref_metrics.si_sdr(gt, y)
    assert np.isfinite(want).all() and want.min() >= -30.0 and want.max() <= 70.0, want
    assert 40.0 < want[7, 2] < 60.0 and (want[8, :3] < 0).all(), want[7:]
    g = np.load(os.path.join(HERE, "e2e_M8_B2_T20.npz"))
    out = torch.from_numpy(g["out"]).double()
    label = torch.from_numpy(paramgen.make_spec_input(2, 20, 161, 1, int(g["label_seed"]))[..., 0, :]).permute(0, 3, 1, 2).double()
    frames = (20, 13)
    loss = np.array([[float(ref_loss(out[b:b + 1, :, :n], label[b:b + 1, :, :n], [n])) for n in frames] for b in range(2)])
    np.savez(os.path.join(HERE, "score_cases.npz"), cases=cases, ratios=want, loss_frames=np.array(frames), loss=loss)
    print(want, loss, sep="\n")


if __name__ == "__main__":
    main()
