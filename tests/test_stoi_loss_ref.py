"""tests/stoi_loss_ref.py, the float64 reference of the ``stoi_loss`` GPU tests, pinned three ways on the CPU -- to
``stoi_ref.analyse``'s scores, to float64 central differences, and against four misreadings of the gradient's conventions -- plus
the margin condition every gradient case must hold, and the float64 adjoint of the resampler.

Recorded here (float64, CPU): the restatement's scores agree with ``analyse`` to 3e-16; the directional derivatives agree with
central differences (step 1e-6 of the signal's rms along seeded Gaussian directions) to 3e-11 of |grad| |direction|, five orders
below the GPU bar of 1e-5; the misreadings move the gradient by 1.3e-3 (alpha constant, at factors 0.5 / 0.5; 7.2e-3 for STOI
alone) to 6.8e-1 (mask from est) of max |ref|, against 100 x the GPU bar = 1e-3."""
import numpy as np
import pytest
import torch

import resample_ref
import stoi_loss_ref as G
import stoi_ref as R

GPU_BAR = 1e-5


def _case(k):
    return R.make_case(*(R.CASES[k] if k >= 0 else G.SHORT_EST_CASE))


@pytest.mark.parametrize("k", list(range(len(R.CASES))) + [-1])
def test_scores_are_those_of_the_numpy_restatement(k):
    clean, est = _case(k)
    a = R.analyse(clean.astype(np.float64), est.astype(np.float64))
    with torch.no_grad():
        info = G.scores(clean, torch.from_numpy(est.astype(np.float64)))
    assert info["K"] == a["K"]
    assert abs(float(info["stoi"]) - a["stoi"]) <= 1e-12 and abs(float(info["estoi"]) - a["estoi"]) <= 1e-12


@pytest.mark.parametrize("k", list(G.GRAD_CASES) + [-1])
def test_gradient_cases_hold_the_margin_condition(k):
    """one flipped clip branch changes a segment's gradient by far more than any rounding bar, so no gradient case may have an
    element within 1e-4 relative of rule 9's bound, or a frame within 0.05 dB of rule 4's threshold"""
    clean, est = _case(k)
    _, grad, info = G.loss_and_grad(clean, est, 0.5, 0.5)
    print(f"case {k}: K {info['K']}, frame margin {info['frame_margin']:.3f} dB, clip margin {info['clip_margin']:.3e}")
    assert info["clip_margin"] > G.CLIP_MARGIN and info["frame_margin"] >= G.FRAME_MARGIN_DB
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0
    if k == -1:                                              # est's zero tail: whole band frames of est are exactly zero
        assert len(grad) == 6000 and len(clean) == 9000 and info["zero_bands"] >= 15
    else:
        assert info["zero_bands"] == 0


def test_the_six_second_case_misses_the_margin_and_serves_values_only():
    clean, est = _case(8)
    with torch.no_grad():
        info = G.scores(clean, torch.from_numpy(est.astype(np.float64)))
    print(f"case 708: clip margin {info['clip_margin']:.3e}")
    assert info["clip_margin"] < G.CLIP_MARGIN and 8 not in G.GRAD_CASES


def test_the_chain_case_holds_the_margin_condition():
    spec, clean = G.chain_case()
    with torch.no_grad():
        _, infos = G.chain_loss64(torch.from_numpy(spec).double(), clean, 0.5, 0.5)
    for i in infos:
        print(f"chain row: K {i['K']}, frame margin {i['frame_margin']:.3f} dB, clip margin {i['clip_margin']:.3e}")
        assert i["T"] >= R.N_SEG and i["clip_margin"] > G.CLIP_MARGIN and i["frame_margin"] >= G.FRAME_MARGIN_DB


@pytest.mark.parametrize("k", G.SENTINEL_CASES)
def test_sentinel_cases_have_an_all_zero_gradient(k):
    clean, est = _case(k)
    loss, grad, _ = G.loss_and_grad(clean, est, 0.5, 0.5)
    assert loss == -R.SENTINEL and grad.shape == est.shape and (grad == 0).all()


@pytest.mark.parametrize("k", (0, 4, -1))
def test_gradient_agrees_with_central_differences(k):
    clean, est = _case(k)
    e64 = est.astype(np.float64)
    _, grad, _ = G.loss_and_grad(clean, est, 0.5, 0.5)
    rng = np.random.default_rng(900 + k)
    h = 1e-6 * float(np.sqrt(np.mean(e64 ** 2)))
    worst = 0.0
    for _ in range(3):
        d = rng.standard_normal(e64.shape)
        with torch.no_grad():
            lp, lm = (G.scores(clean, torch.from_numpy(e64 + s * h * d)) for s in (1.0, -1.0))
        num = -(0.5 * (float(lp["stoi"]) - float(lm["stoi"])) + 0.5 * (float(lp["estoi"]) - float(lm["estoi"]))) / (2.0 * h)
        worst = max(worst, abs(num - grad @ d) / (np.linalg.norm(grad) * np.linalg.norm(d)))
    print(f"case {k}: directional derivative vs central differences, worst {worst:.2e} of |grad| |direction|")
    assert worst <= 1e-7, "far tighter than the GPU bar of 1e-5"


@pytest.mark.parametrize("misreading", G.MISREADINGS)
def test_every_misreading_moves_the_gradient_far_beyond_the_gpu_bar(misreading):
    """case 704 (frames removed, 13 % of the elements clipped) for the first three; the artefact-dominated case 709, whose estimate
    keeps other frames than its clean signal, for the mask"""
    k = 9 if misreading == "mask_from_est" else 4
    clean, est = _case(k)
    for fs, fe in ((1.0, 0.0), (0.5, 0.5)):
        if misreading in ("alpha_constant", "clip_ignored") and fs == 0.0:
            continue
        loss, grad, _ = G.loss_and_grad(clean, est, fs, fe)
        wl, wrong, _ = G.loss_and_grad(clean, est, fs, fe, misreading=misreading)
        moved = float(np.abs(wrong - grad).max() / np.abs(grad).max())
        print(f"{misreading} ({fs}, {fe}): the gradient moves by {moved:.2e} of max |ref|")
        assert moved > 100.0 * GPU_BAR
        if misreading != "mask_from_est":
            assert wl == loss, "a misreading changes the gradient, not the value"


@pytest.mark.parametrize("orig,new", [(16000, 10000), (48000, 16000), (16000, 48000), (44100, 16000)])
def test_resampler_adjoint_in_float64(orig, new):
    rng = np.random.default_rng(orig // 100 + new)
    for L in (1, 7, 300):
        M = G.resample_matrix(L, orig, new)
        x, g = rng.standard_normal(L), rng.standard_normal(M.shape[0])
        y = resample_ref.ref_resample(x, orig, new)
        assert np.abs(M @ x - y).max() <= 1e-13 * max(1.0, np.abs(y).max())
        gx = G.resample_adjoint(g, L, orig, new)
        assert abs(y @ g - x @ gx) <= 1e-12 * (np.linalg.norm(y) * np.linalg.norm(g) + 1e-300)       # <R x, g> == <x, R^T g>
        # a padded row: L samples of which 5 fewer are the signal
        if L > 5:
            gp = G.resample_adjoint(g, L, orig, new, length=L - 5)
            assert (gp[L - 5:] == 0).all()
            n5 = resample_ref.out_length(L - 5, orig, new)
            assert np.abs(gp[:L - 5] - G.resample_matrix(L - 5, orig, new).T @ g[:n5]).max() == 0
        # the differentiable torch restatement of the same sum has this adjoint
        xt = torch.from_numpy(x).requires_grad_(True)
        yt = G.torch_resample(xt, orig, new)
        assert np.abs(yt.detach().numpy() - y).max() <= 1e-13 * max(1.0, np.abs(y).max())
        yt.backward(torch.from_numpy(g))
        assert np.abs(xt.grad.numpy() - gx).max() <= 1e-12 * max(1.0, np.abs(gx).max())


# --- refusals: all of them are raised before anything is launched, so they show on a machine without a GPU ------------------------------
def test_stoi_loss_refusals():
    import eabnet_amd
    from eabnet_amd import stoi_loss
    e, s = torch.zeros(2, 5000), torch.zeros(2, 5000)
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        stoi_loss(e, s)
    with pytest.raises(TypeError, match="fp32"):
        stoi_loss(e.double(), s)
    with pytest.raises(TypeError, match="fp32"):
        stoi_loss(e, s.half())
    with pytest.raises(NotImplementedError, match="est only"):
        stoi_loss(e, s.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="reduction"):
        stoi_loss(e, s, reduction="batchmean")
    for bad in (dict(factor_stoi=-1.0), dict(factor_estoi=float("inf")), dict(factor_stoi=float("nan")),
                dict(factor_stoi=0.0, factor_estoi=0.0), dict(factor_estoi="1")):
        with pytest.raises(ValueError, match="factor"):
            stoi_loss(e, s, **bad)
    with pytest.raises(ValueError, match="rows"):
        stoi_loss(e, s[:1])
    with pytest.raises(ValueError):
        stoi_loss(e, s, lengths=[5001, 10])
    with pytest.raises(ValueError, match="sample rates"):
        stoi_loss(e, s, sample_rate=0)
    assert "stoi_loss" in eabnet_amd.__all__


def test_rows_on_different_devices_are_refused(monkeypatch):
    """the check sits behind the CUDA check; without a second device the two rows are given two device labels"""
    import eabnet_amd
    from eabnet_amd import wave

    class Row:
        def __init__(self, device):
            self.t, self.device = torch.zeros(1, 5000), device
        ndim, shape, dtype, requires_grad, is_cuda = 2, (1, 5000), torch.float32, False, True

    with pytest.raises(ValueError, match="one device"):
        wave.stoi_loss(Row("cuda:0"), Row("cuda:1"))


def test_resample_under_autograd_refuses_mic_order_and_streams():
    import eabnet_amd
    x = torch.zeros(1, 2, 400, requires_grad=True)
    with pytest.raises(NotImplementedError, match="mic_order"):
        eabnet_amd.resample(x, 16000, 10000, mic_order=[1, 0])
    with pytest.raises(NotImplementedError, match="not differentiable"):
        eabnet_amd.StreamResampler(16000, 10000).push(x)
    with torch.no_grad(), pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):      # (without grad: today's path)
        eabnet_amd.resample(x, 16000, 10000, mic_order=[1, 0])
