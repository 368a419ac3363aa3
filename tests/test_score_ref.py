"""Scoring without a device: the float64 restatement of the energy ratios (tests/score_ref.py) against the reference's recorded
values, the two new entry points in the header, the binding and the library, and the refusals of ``Scorer``."""
import ctypes
import os

import numpy as np
import pytest
import torch

import eabnet_amd
import paramgen
import score_ref
from util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eab_energy_ratios_f32", "eab_com_mag_mse_loss_lens_f32")


def test_fixture_holds_the_cases_of_score_ref():
    g = load("score_cases.npz")
    want = np.array([tuple(c) + (0,) * (8 - len(c)) for c in score_ref.CASES], dtype=np.float64)
    assert np.array_equal(g["cases"], want), "tests/score_ref.py CASES and the fixture disagree: run make_score_golden.py"
    assert g["ratios"].shape == (len(score_ref.CASES), 4) and g["ratios"].dtype == np.float64
    assert np.isfinite(g["ratios"]).all() and g["ratios"].min() >= -30.0 and g["ratios"].max() <= 70.0
    assert 40.0 < g["ratios"][7, 2] < 60.0 and (g["ratios"][8, :3] < 0.0).all()


@pytest.mark.parametrize("k", range(len(score_ref.CASES)))
def test_restatement_equals_the_reference(k):
    g = load("score_cases.npz")
    clean, noisy, est = score_ref.make_case(*score_ref.CASES[k])
    assert (len(clean), len(noisy), len(est)) == score_ref.CASES[k][:3] and clean.dtype == np.float32
    got = score_ref.ratios(est, clean, noisy)
    err = np.abs(got - g["ratios"][k]).max()
    print(f"case {k}: {got} max |diff| {err:.2e} dB")
    assert err <= 1e-9


def test_restated_loss_equals_the_reference_per_utterance():
    g, gs = load("e2e_M8_B2_T20.npz"), load("score_cases.npz")
    label = np.transpose(paramgen.make_spec_input(2, 20, 161, 1, int(g["label_seed"]))[..., 0, :], (0, 3, 1, 2))
    for b in range(2):
        for j, n in enumerate(gs["loss_frames"]):
            v = score_ref.loss_one(g["out"][b], label[b], int(n))
            assert abs(v - gs["loss"][b, j]) <= 1e-9 * gs["loss"][b, j]


def test_degenerate_rows_are_nan_in_the_restatement():
    clean, noisy, est = score_ref.make_case(*score_ref.CASES[1])
    assert np.isnan(score_ref.ratios(est, np.zeros_like(clean), noisy)).all()
    assert np.isnan(score_ref.ratios(est, clean, clean)[:3]).all()


def test_score_entry_points_are_declared_bound_and_exported():
    from eabnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "eabnet_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 10 and "#define EAB_ABI_VERSION 10" in header, "only entry points were added: the ABI stays 10"
    assert _lib.load().eab_abi_version() == 10


def test_score_argument_validation_happens_before_any_launch():
    from eabnet_amd import _lib
    lib = _lib.load()
    assert lib.eab_energy_ratios_f32(None, 8, 8, None, 8, 8, None, 8, 8, None, 1, None, 1, None, None) == 1
    assert lib.eab_com_mag_mse_loss_lens_f32(None, None, None, 1, 9, 9, 161, None, 1, None, None) == 1
    buf = (ctypes.c_double * 64)()                        # host memory stands in: a refused call launches and reads nothing
    p = ctypes.addressof(buf)
    assert lib.eab_energy_ratios_f32(p, 8, 8, p, 8, 8, p, 8, 8, p, 0, p, 1, p, None) == 1          # B = 0
    assert lib.eab_energy_ratios_f32(p, 8, 8, p, 8, 0, p, 8, 8, p, 1, p, 1, p, None) == 1          # an empty row
    assert lib.eab_energy_ratios_f32(p, 8, 8, p, 4, 8, p, 8, 8, p, 2, p, 1, p, None) == 1          # overlapping rows
    assert lib.eab_energy_ratios_f32(p, 8, 8, p, 8, 8, p, 5000, 5000, p, 2, p, 1, p, None) == 1    # scratch of one span, two needed
    assert lib.eab_com_mag_mse_loss_lens_f32(p, p, p, 1, 0, 9, 161, p, 1, p, None) == 1            # no frames
    assert lib.eab_com_mag_mse_loss_lens_f32(p, p, p, 1, 30, 30, 161, p, 1, p, None) == 1          # 4830 bins: two spans


def test_functions_refuse_cpu_tensors_after_validating():
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        eabnet_amd.energy_ratios(torch.zeros(2, 160), torch.zeros(2, 161), torch.zeros(2, 161))
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        eabnet_amd.com_mag_mse_loss_per_utterance(torch.zeros(2, 2, 9, 161), torch.zeros(2, 2, 9, 161), [9, 4])
    with pytest.raises(ValueError):
        eabnet_amd.energy_ratios(torch.zeros(2, 160, 1), torch.zeros(2, 161), torch.zeros(2, 161))
    with pytest.raises(ValueError):
        eabnet_amd.com_mag_mse_loss_per_utterance(torch.zeros(2, 2, 9, 161), torch.zeros(2, 2, 9, 161), [9, 10])
    with pytest.raises(ValueError):
        eabnet_amd.com_mag_mse_loss_per_utterance(torch.zeros(2, 2, 9, 161), torch.zeros(3, 2, 9, 161), [9, 9])


def test_scorer_refusals_without_a_device():
    net = eabnet_amd.EaBNet(M=2).eval()
    sc = eabnet_amd.Scorer(net)
    assert isinstance(sc, eabnet_amd.Enhancer) and sc.ref_mic == 0 and sc.sizes == (16, 4, 1)
    with pytest.raises(ValueError, match="2 noisy files but 1 clean"):
        sc([torch.zeros(2, 4000), torch.zeros(2, 4000)], [torch.zeros(4000)])                  # count mismatch
    with pytest.raises(ValueError, match="lengths must agree"):
        sc([torch.zeros(2, 4000)], [torch.zeros(3999)])                                        # length mismatch
    with pytest.raises(ValueError):
        sc([torch.zeros(2, 4000)], [torch.zeros(2, 4000)])                                     # clean is one channel
    with pytest.raises(ValueError):
        eabnet_amd.Scorer(net, ref_mic=2)([torch.zeros(2, 4000)], [torch.zeros(4000)])         # no such microphone
    with pytest.raises(ValueError):
        eabnet_amd.Scorer(net, ref_mic=-1)
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        sc([torch.zeros(2, 4000)], [torch.zeros(1, 4000)])                                     # the model is on the CPU
    with pytest.raises(RuntimeError, match="eval"):
        eabnet_amd.Scorer(eabnet_amd.EaBNet(M=2).train())([torch.zeros(2, 4000)], [torch.zeros(4000)])
    with pytest.raises(TypeError):
        eabnet_amd.Scorer(torch.nn.Linear(2, 2))
    empty = sc([], [])
    assert set(empty) == {"loss", "si_sdr", "si_sdr_mix", "si_sir", "si_sar"} and all(v.shape == (0,) for v in empty.values())
    assert net.length_buckets is None


def test_summary_drops_nans_like_mean_std():
    s = eabnet_amd.Scorer.summary({"si_sdr": np.array([1.0, np.nan, 3.0]), "loss": np.array([np.nan])})
    assert s["si_sdr"] == (2.0, 1.0) and all(np.isnan(v) for v in s["loss"])
