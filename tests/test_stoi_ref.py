"""The float64 restatement of STOI / ESTOI (tests/stoi_ref.py) against the values recorded with the definition, the
invariants of that definition, and its sensitivity to four plausible misreadings -- so that the GPU tests may use the restatement
as their yardstick.  Also what the new Python surface does without a GPU.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import stoi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return [R.make_case(*c) for c in R.CASES]


@pytest.fixture(scope="module")
def analysed(cases):
    return [R.analyse(c.astype(np.float64), e.astype(np.float64)) for c, e in cases]


def test_restatement_reproduces_the_recorded_counts_and_scores(analysed):
    for k, (a, (frames, kept, stoi, estoi)) in enumerate(zip(analysed, R.EXPECTED)):
        print(f"case {k}: frames {a['frames']} kept {a['K']} stoi {a['stoi']:.6f} estoi {a['estoi']:.6f} clipped {a['clipped']:.4f}")
        assert (a["frames"], a["K"]) == (frames, kept), k
        assert abs(a["stoi"] - stoi) <= 2e-6 and abs(a["estoi"] - estoi) <= 2e-6, k
        assert a["tob"].shape == (2, 15, max(a["K"] - 1, 0))
    # rule 9's bound binds on 0.5 % to 7.5 % of the elements of cases 4-9: the clipping is exercised
    assert all(0.004 <= a["clipped"] <= 0.08 for a in analysed[4:])


def test_no_frame_sits_within_a_rounding_error_of_the_silence_threshold(analysed):
    """a condition on the cases: an fp32 / fp64 difference of ~1e-5 dB in a frame energy can never flip the mask"""
    for k, a in enumerate(analysed):
        print(f"case {k}: smallest |max e - 40 - e_j| = {a['margin']:.3f} dB")
        assert a["margin"] >= 0.05, k


def test_band_table_is_what_the_frequency_formula_gives():
    assert R.derive_bands() == R.BANDS
    assert len(R.BANDS) == 15 and all(R.BANDS[i][1] == R.BANDS[i + 1][0] for i in range(14))


def test_invariants_of_the_definition(cases):
    for k in range(4, 10):
        clean, est = cases[k]
        same = R.intelligibility(clean, clean)
        assert np.abs(same - 1.0).max() <= 1e-12, (k, same)
        a = R.intelligibility(est, clean)
        b = R.intelligibility(est.astype(np.float64) * 3.7, clean)
        assert np.abs(a - b).max() <= 1e-9, (k, a, b)
        silent = R.intelligibility(est, np.zeros_like(clean))
        assert silent[0] == 0.0 and silent[1] == 0.0, (k, silent)


@pytest.mark.parametrize("name", ["hanning", "band14_wider", "band0_narrower", "non_strict"])
def test_a_wrong_reading_of_the_definition_moves_a_score(cases, analysed, name):
    """each variant moves at least one score of at least one case by more than the GPU tests' bound of 1e-4"""
    kw = {"hanning": dict(w=np.hanning(256)),
          "band14_wider": dict(bands=R.BANDS[:14] + [(174, 220)]),
          "band0_narrower": dict(bands=[(8, 9)] + R.BANDS[1:]),
          "non_strict": dict(strict=False)}[name]
    shift = 0.0
    for (clean, est), a in zip(cases, analysed):
        got = R.intelligibility(est, clean, **kw)
        shift = max(shift, abs(got[0] - a["stoi"]), abs(got[1] - a["estoi"]))
    print(f"{name}: largest shift {shift:.2e}")
    assert shift > 1e-4


def test_scorer_key_sets_without_files():
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=2, p=1, q=1).eval()
    seven = eabnet_amd.Scorer(net, intelligibility=True)([], [])
    assert list(seven) == ["si_sdr", "si_sir", "si_sar", "si_sdr_mix", "loss", "stoi", "estoi"]
    assert all(v.shape == (0,) for v in seven.values())
    five = eabnet_amd.Scorer(net)([], [])
    assert list(five) == ["si_sdr", "si_sir", "si_sar", "si_sdr_mix", "loss"]
    scores, waves = eabnet_amd.Scorer(net, intelligibility=True)([], [], return_waves=True)
    assert len(scores) == 7 and waves == []


def test_intelligibility_refuses_cpu_tensors_and_bad_arguments():
    import eabnet_amd
    x = torch.zeros(2, 5000)
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        eabnet_amd.intelligibility(x, x)
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        eabnet_amd.intelligibility(x, x, sample_rate=10000)
    with pytest.raises(ValueError):
        eabnet_amd.intelligibility(x, x[:1])
    with pytest.raises(ValueError):
        eabnet_amd.intelligibility(x, x, lengths=([5000, 5000],))
    with pytest.raises(ValueError):
        eabnet_amd.intelligibility(x, x, lengths=([5001, 5000], [5000, 5000]))
    with pytest.raises(ValueError):
        eabnet_amd.stoi(np.zeros((2, 100)), np.zeros(100), 10000)


def test_header_binding_and_library_agree_on_the_new_entry_points():
    from eabnet_amd import _lib
    src = open(os.path.join(ROOT, "include", "eabnet_hip.h")).read()
    declared = set(re.findall(r"\b(eab_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    for name in ("eab_stoi_f32", "eab_stoi_workspace_bytes", "eab_stoi_frame_capacity"):
        assert name in declared and name in _lib.EXPORTS
    assert sorted(declared) == sorted(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 10
    lib = _lib.load()
    # frames of a signal: start + 256 < L
    assert [lib.eab_stoi_frame_capacity(n) for n in (1, 256, 257, 384, 385, 4096, 4097)] == [1, 1, 1, 1, 2, 30, 31]
    assert lib.eab_stoi_frame_capacity(0) == -1 and lib.eab_stoi_workspace_bytes(0, 100) == -1
    assert lib.eab_stoi_workspace_bytes(16, 60000) > 0
    # null pointers and bad shapes are refused on the host, before any launch
    assert lib.eab_stoi_f32(None, 1, 1, None, 1, 1, None, 1, None, 0, None, None, None, None, None) == 1
