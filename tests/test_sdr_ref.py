"""The float64 restatement of the BSS-eval SDR (tests/sdr_ref.py) against central differences, against the SI-SDR restatement at
K = 1 and on the delay property that is the reason for the score; then what ``sdr`` and ``sdr_loss`` refuse on CPU tensors, and
where the new names are registered.  No GPU needed."""
import os

import numpy as np
import pytest
import torch

import sdr_ref as R
import wave_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("eps", [0.0, 1e-3])
def test_reference_gradient_against_central_differences(eps):
    """K = 16, L = 300 in float64; bound 1e-5 of the largest entry (the project's gradient bar; the formula measured 1.1e-6, the
    error of the differences themselves)"""
    e, s = R.make_pair(300, 300, 11, 8.0)
    e = e.astype(np.float64)
    _, grad = R.sdr_loss(e, s, 16, eps=eps)
    num = np.zeros_like(grad)
    for i in range(e.shape[0]):
        d = 1e-4 * max(1.0, abs(e[i]))
        up, dn = e.copy(), e.copy()
        up[i] += d
        dn[i] -= d
        num[i] = (R.sdr_loss(up, s, 16, eps=eps)[0] - R.sdr_loss(dn, s, 16, eps=eps)[0]) / (2.0 * d)
    err = np.abs(grad - num).max() / np.abs(num).max()
    print(f"eps {eps}: max |formula - differences| / max |differences| = {err:.2e} (bound 1e-5)")
    assert err <= 1e-5


@pytest.mark.parametrize("lengths", [(300, 300), (5, 200), (257, 130)])          # (not one sample: its gradient is zero on paper)
def test_one_tap_is_the_si_sdr_loss(lengths):
    e, s = R.make_pair(*lengths, 12, 8.0)
    for eps in (0.0, 1e-8):
        want, wgrad = W.si_sdr_loss(e.astype(np.float64), s.astype(np.float64), eps)
        got, grad = R.sdr_loss(e, s, 1, eps=eps)
        assert abs(got - want) <= 1e-10 * max(1.0, abs(want))
        assert np.abs(grad - wgrad).max() <= 1e-10 * np.abs(wgrad).max()
    assert abs(R.sdr(e, s, 1)[0] + W.si_sdr_loss(e.astype(np.float64), s.astype(np.float64))[0]) <= 1e-10 * 50


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_delayed_copy_scores_by_its_noise(seed):
    """the estimate is the clean wave delayed by 37 samples plus white noise at 10 dB, L = 8000: 64 and 512 taps read 10 dB within
    0.5 dB, one tap (SI-SDR) reads below 0 dB"""
    e, s = R.make_delayed(8000, seed)
    got = {K: R.sdr(e, s, K)[0] for K in (1, 64, 512)}
    print(f"seed {seed}: " + ", ".join(f"K = {K}: {v:.2f} dB" for K, v in got.items()))
    assert abs(got[64] - 10.0) <= 0.5 and abs(got[512] - 10.0) <= 0.5
    assert got[1] < 0.0


def test_load_diag_moves_the_reference_and_bad_inputs_are_not_its_business():
    e, s = R.make_pair(4000, 4000, 13, 8.0)
    assert R.sdr(e, s, 64, 1e-3)[0] < R.sdr(e, s, 64)[0]
    with pytest.raises(AssertionError, match="cond"):
        R.sdr(e[:100], s[:100] * 0.0, 64)                         # a silent clean wave


def _w(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def test_the_argument_front_of_sdr_and_sdr_loss_on_cpu_tensors():
    import eabnet_amd
    from eabnet_amd._lib import EabError
    B, L = 2, 40
    for fn in (eabnet_amd.sdr, eabnet_amd.sdr_loss):
        with pytest.raises(ValueError, match=r"est must be a \(B, L\) tensor"):
            fn(_w(L), _w(B, L))
        with pytest.raises(ValueError, match="same number of rows, got 2 and 3"):
            fn(_w(B, L), _w(B + 1, L))
        for K in (0, 513, 2.0, True):
            with pytest.raises(ValueError, match=r"filter_length must be an integer in \[1, 512\]"):
                fn(_w(B, L), _w(B, L), filter_length=K)
        for bad in (-1e-3, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="load_diag must be a finite number >= 0"):
                fn(_w(B, L), _w(B, L), load_diag=bad)
        with pytest.raises(ValueError, match=r"lengths must lie in \[1, 40\]"):
            fn(_w(B, L), _w(B, L), lengths=([10, L + 1], [10, 10]))
        with pytest.raises(EabError, match="no CPU fallback"):
            fn(_w(B, L), _w(B, L), lengths=([10, L], [10, L]), filter_length=4)
    # the score casts other dtypes (as energy_ratios), the loss refuses them (as si_sdr_loss)
    with pytest.raises(EabError, match="sdr needs CUDA"):
        eabnet_amd.sdr(_w(B, L, dtype=torch.float64), _w(B, L))
    with pytest.raises(ValueError, match=r"pair \(est, clean\)"):
        eabnet_amd.sdr(_w(B, L), _w(B, L), lengths=([10, 10],))
    with pytest.raises(TypeError, match="sdr_loss takes fp32 waves"):
        eabnet_amd.sdr_loss(_w(B, L, dtype=torch.float64), _w(B, L))
    with pytest.raises(NotImplementedError, match="sdr_loss is differentiable with respect to est only"):
        eabnet_amd.sdr_loss(_w(B, L), _w(B, L).requires_grad_())
    with pytest.raises(ValueError, match=r"reduction must be one of \('mean', 'sum', 'none'\), got 'avg'"):
        eabnet_amd.sdr_loss(_w(B, L), _w(B, L), reduction="avg")
    for bad in (-1.0, float("inf")):
        with pytest.raises(ValueError, match="eps must be a finite number >= 0"):
            eabnet_amd.sdr_loss(_w(B, L), _w(B, L), eps=bad)
    for red in ("mean", "sum", "none"):
        with pytest.raises(EabError, match="sdr_loss needs CUDA"):
            eabnet_amd.sdr_loss(_w(B, L), _w(B, 1, L), reduction=red)


def test_the_c_entry_points_refuse_bad_arguments_before_any_launch():
    """EAB_EINVAL (1) on the host: nothing is launched, so no GPU is needed"""
    import ctypes as C
    from eabnet_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 4200)()
    p = C.addressof(buf)
    ok = dict(K=512, load_diag=0.0, eps=0.0, spans=1, B=1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.eab_sdr_f32(p, 4096, 4096, p, 4096, 4096, p, a["B"], a["K"], a["load_diag"], a["eps"], p, a["spans"], p, None, None)

    for kw in (dict(K=0), dict(K=513), dict(load_diag=-1e-9), dict(load_diag=float("nan")), dict(load_diag=float("inf")),
               dict(eps=-1.0), dict(eps=float("nan")), dict(spans=0), dict(B=0), dict(B=65536)):
        assert call(**kw) == 1, kw
    assert lib.eab_sdr_f32(None, 4096, 4096, p, 4096, 4096, p, 1, 512, 0.0, 0.0, p, 1, p, None, None) == 1
    assert lib.eab_sdr_f32(p, 8192, 8192, p, 4096, 4096, p, 1, 512, 0.0, 0.0, p, 1, p, None, None) == 1       # two spans needed
    assert lib.eab_sdr_loss_bwd_f32(p, 4096, 4096, p, 4096, 4096, p, 1, 513, p, p, p, 0, 1.0, p, 4096, None) == 1
    assert lib.eab_sdr_loss_bwd_f32(p, 4096, 4096, p, 4096, 4096, p, 1, 512, p, None, p, 0, 1.0, p, 4096, None) == 1
    assert lib.eab_sdr_loss_bwd_f32(p, 4096, 4096, p, 4096, 4096, p, 1, 512, p, p, p, -1, 1.0, p, 4096, None) == 1


def test_the_names_are_registered():
    import eabnet_amd
    from eabnet_amd import _lib
    assert "sdr" in eabnet_amd.__all__ and "sdr_loss" in eabnet_amd.__all__
    assert {"eab_sdr_f32", "eab_sdr_loss_bwd_f32"} <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 10
    srcs = [l for l in open(os.path.join(ROOT, "eabnet_amd", "csrc", "Makefile")) if l.startswith("SRCS")]
    assert len(srcs) == 1 and "sdr.hip" in srcs[0].split()


def test_the_scorer_switch_adds_two_keys_and_nothing_else():
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=2, p=1, q=1)
    assert eabnet_amd.Scorer(net).metrics == ("si_sdr", "si_sir", "si_sar", "si_sdr_mix", "loss")
    assert eabnet_amd.Scorer(net, intelligibility=True).metrics == ("si_sdr", "si_sir", "si_sar", "si_sdr_mix", "loss", "stoi", "estoi")
    assert eabnet_amd.Scorer(net, distortion=True).metrics[-2:] == ("sdr", "sdr_mix")
    assert eabnet_amd.Scorer(net, distortion=True).metrics[:-2] == eabnet_amd.Scorer(net).metrics
    both = eabnet_amd.Scorer(net, intelligibility=True, distortion=True).metrics
    assert both[-4:] == ("stoi", "estoi", "sdr", "sdr_mix")
    assert eabnet_amd.Scorer(net, max_batch=4, distortion=True).max_batch == 4
