"""``sdr`` / ``sdr_loss`` (csrc/sdr.hip) on the MI355X against the dense float64 restatement of tests/sdr_ref.py, which
tests/test_sdr_ref.py pins to central differences and to the SI-SDR restatement.

Bounds: 4.34e-4 dB = 10 log10(1 + 1e-4) on a value and 1e-5 of max |ref| on a gradient (tests/test_score_gpu.py,
tests/test_wave_loss_gpu.py); on the filter h, sdr_ref.H_BOUND = 100 x the 4e-12 by which a float64 Levinson recursion differs from
the dense solve on the same inputs (the margin covers another summation order of the correlations)."""
import numpy as np
import pytest
import torch

import paramgen
import sdr_ref as R
from util import TOL_HIP, torch_params

pytestmark = pytest.mark.gpu

TOL_DB = 10.0 * np.log10(1.0 + TOL_HIP)
TOL_GRAD = 1e-5
LENS = [list(p) for p in R.LENGTHS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _poisoned(pairs, width, dev):
    """(est, clean) device rows of ``width`` with NaN behind every length"""
    est = torch.full((len(pairs), width), float("nan"))
    clean = torch.full((len(pairs), width), float("nan"))
    for b, (e, s) in enumerate(pairs):
        est[b, :len(e)], clean[b, :len(s)] = torch.from_numpy(e), torch.from_numpy(s)
    return est.to(dev), clean.to(dev)


def _cols(lens):
    return ([p[0] for p in lens], [p[1] for p in lens])


@pytest.fixture(scope="module")
def batch(dev):
    est, clean = _poisoned(R.rows(), R.WIDTH, dev)
    return {"est": est, "clean": clean}


# ------------------------------------------------------------------ the value and the filters
@pytest.mark.parametrize("K", R.FILTERS)
def test_values_and_filters_vs_the_dense_float64_solve(dev, batch, K):
    import eabnet_amd
    got, h = eabnet_amd.sdr(batch["est"], batch["clean"], lengths=_cols(LENS), filter_length=K, filters=True)
    assert got.dtype == torch.float64 and got.shape == (3,) and h.dtype == torch.float64 and h.shape == (3, K)
    assert torch.isfinite(got).all() and torch.isfinite(h).all(), "a sample past a length was read"
    for b in range(3):
        want, wh = R.cached("sdr", b, K)
        err = abs(float(got[b]) - want)
        herr = np.linalg.norm(h[b].cpu().numpy() - wh) / np.linalg.norm(wh)
        print(f"K {K}, lengths {R.LENGTHS[b]}: {float(got[b]):.5f} dB |diff| {err:.2e} (bound {TOL_DB:.2e}); "
              f"|h - ref| / |ref| = {herr:.2e} (bound {R.H_BOUND:.0e})")
        assert err <= TOL_DB and herr <= R.H_BOUND, (b, err, herr)
    again, h2 = eabnet_amd.sdr(batch["est"], batch["clean"], lengths=_cols(LENS), filter_length=K, filters=True)
    assert torch.equal(again, got) and torch.equal(h2, h), "a second call"
    for b in range(3):
        one, h1 = eabnet_amd.sdr(batch["est"][b:b + 1], batch["clean"][b:b + 1], lengths=_cols(LENS[b:b + 1]), filter_length=K, filters=True)
        assert torch.equal(one[0], got[b]) and torch.equal(h1[0], h[b]), f"row {b} alone"
    only = eabnet_amd.sdr(batch["est"], batch["clean"], lengths=_cols(LENS), filter_length=K)
    assert torch.equal(only, got), "without the filters"


def test_a_strided_view_is_read_in_place_and_power_of_two_gains_keep_the_bits(dev, batch):
    import eabnet_amd
    lens = tuple(torch.tensor(c, device=dev) for c in _cols(LENS))                   # device lengths
    want = eabnet_amd.sdr(batch["est"], batch["clean"], lengths=_cols(LENS))
    wide = torch.full((3, 3, R.WIDTH), float("nan"), device=dev)
    wide[:, 1] = batch["est"]
    view = wide[:, 1]
    assert not view.is_contiguous()
    assert torch.equal(eabnet_amd.sdr(view, batch["clean"], lengths=lens), want)
    off = torch.full((3, R.WIDTH + 5), float("nan"), device=dev)                      # rows 4 bytes off a 16-byte boundary
    off[:, 1:1 + R.WIDTH] = batch["clean"]
    assert torch.equal(eabnet_amd.sdr(view, off[:, 1:1 + R.WIDTH], lengths=lens), want)
    assert torch.equal(eabnet_amd.sdr(0.5 * batch["est"], 4.0 * batch["clean"], lengths=lens), want), "every operation scales by 2^n"


def test_rows_that_cannot_be_scored_give_nan_in_their_own_rows_only(dev, batch):
    import eabnet_amd
    pairs = R.rows()
    e, s = pairs[2]
    est, clean = _poisoned([(e, np.zeros(3000, np.float32)), pairs[2], (e, s[:100].copy()), pairs[1]], R.WIDTH, dev)
    lens = [[len(e), 3000], LENS[2], [len(e), 100], LENS[1]]
    got, h = eabnet_amd.sdr(est, clean, lengths=_cols(lens), filters=True)
    want = eabnet_amd.sdr(batch["est"], batch["clean"], lengths=_cols(LENS))
    assert torch.isnan(got[0]) and torch.isnan(got[2]) and torch.isnan(h[0]).all() and torch.isnan(h[2]).all()
    assert torch.equal(got[1], want[2]) and torch.equal(got[3], want[1])
    leaf = est.clone().requires_grad_(True)
    loss = eabnet_amd.sdr_loss(leaf, clean, lengths=lens, reduction="none")
    loss.sum().backward()
    assert torch.isnan(loss[0]) and torch.isnan(loss[2]) and torch.isfinite(loss[1]) and torch.isfinite(loss[3])
    for b in (0, 2):
        assert torch.isnan(leaf.grad[b, :lens[b][0]]).all() and (leaf.grad[b, lens[b][0]:] == 0).all()
    for b in (1, 3):
        assert torch.isfinite(leaf.grad[b]).all() and leaf.grad[b].abs().max() > 0
    # 100 samples are enough for 64 taps
    assert torch.isfinite(eabnet_amd.sdr(est[2:3], clean[2:3], lengths=_cols(lens[2:3]), filter_length=64)).all()


def test_a_loaded_diagonal_vs_float64(dev, batch):
    import eabnet_amd
    for K in (64, 512):
        got, h = eabnet_amd.sdr(batch["est"], batch["clean"], lengths=_cols(LENS), filter_length=K, load_diag=1e-3, filters=True)
        for b in range(3):
            want, wh = R.cached("sdr", b, K, 1e-3)
            herr = np.linalg.norm(h[b].cpu().numpy() - wh) / np.linalg.norm(wh)
            print(f"load_diag 1e-3, K {K}, row {b}: {float(got[b]):.5f} dB (float64 {want:.5f}), |h - ref| / |ref| = {herr:.2e}")
            assert abs(float(got[b]) - want) <= TOL_DB and herr <= R.H_BOUND


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_delayed_copy_scores_by_its_noise_on_the_device(dev, seed):
    import eabnet_amd
    e, s = R.make_delayed(8000, seed)
    e, s = torch.from_numpy(e)[None].to(dev), torch.from_numpy(s)[None].to(dev)
    got = {K: float(eabnet_amd.sdr(e, s, filter_length=K)[0]) for K in (1, 64, 512)}
    print(f"seed {seed}: " + ", ".join(f"K = {K}: {v:.2f} dB" for K, v in got.items()))
    assert abs(got[64] - 10.0) <= 0.5 and abs(got[512] - 10.0) <= 0.5 and got[1] < 0.0
    assert float(eabnet_amd.sdr(e, s)[0]) == got[512], "512 taps are the default"


# ------------------------------------------------------------------ the loss and its gradient
LOSS_ROWS = (0, 1, 2, "high")


@pytest.fixture(scope="module")
def loss_batch(dev):
    pairs = R.rows() + [R.high_row()]
    est, clean = _poisoned(pairs, R.WIDTH, dev)
    return {"pairs": pairs, "est": est, "clean": clean, "lengths": [[len(e), len(s)] for e, s in pairs]}


def _loss_and_grad(est, clean, lengths, K, eps, reduction="none", weights=None):
    import eabnet_amd
    leaf = est.detach().requires_grad_(True)
    loss = eabnet_amd.sdr_loss(leaf, clean, lengths=lengths, filter_length=K, eps=eps, reduction=reduction)
    (g,) = torch.autograd.grad(loss, leaf, grad_outputs=weights if weights is not None else torch.ones_like(loss))
    return loss.detach(), g


def _grad_scale(pair, idx, K, wgrad, eps):
    """what a gradient's error is measured against: max |ref|.  The one-sample estimate is the exception, as in
    tests/test_wave_loss_gpu.py: the SDR does not depend on the estimate's gain and one sample has nothing but a gain, so its
    gradient a_b e_0 + c_b p_0 is zero on paper and the float64 reference holds only the rounding of that cancellation; there the
    scale is the size of the cancelling terms, |a_b e_0| with a_b = 2 k10 / (res + eps)."""
    if len(pair[0]) > 1:
        return np.abs(wgrad).max()
    tgt, ee, _, _, _ = R.project(pair[0], pair[1], K)
    return abs(2.0 * R.K10 / (ee - tgt + eps) * float(pair[0][0]))


@pytest.mark.parametrize("eps", [0.0, 1e-8])
@pytest.mark.parametrize("K", [63, 512])
def test_loss_values_and_gradients_vs_float64(dev, loss_batch, K, eps):
    import eabnet_amd
    lb = loss_batch
    loss, grad = _loss_and_grad(lb["est"], lb["clean"], lb["lengths"], K, eps)
    assert loss.dtype == torch.float32 and loss.shape == (4,) and grad.shape == lb["est"].shape and grad.dtype == torch.float32
    for b, idx in enumerate(LOSS_ROWS):
        want, wgrad = R.cached("loss", idx, K, 0.0, eps)
        le = lb["lengths"][b][0]
        err = abs(float(loss[b]) - want)
        gerr = np.abs(grad[b, :le].cpu().numpy() - wgrad).max() / _grad_scale(lb["pairs"][b], idx, K, wgrad, eps)
        print(f"K {K}, eps {eps:g}, lengths {tuple(lb['lengths'][b])}: loss {float(loss[b]):.5f} dB |diff| {err:.2e} (bound {TOL_DB:.2e}); "
              f"gradient {gerr:.2e} (bound {TOL_GRAD:.0e})")
        assert err <= TOL_DB and gerr <= TOL_GRAD, (b, err, gerr)
        assert (grad[b, le:] == 0).all(), "the gradient is exactly zero past the estimate's length"
    assert -R.cached("loss", "high", K)[0] > 30.0, "the row the fp64 filter exists for"
    if eps == 0.0:
        score = eabnet_amd.sdr(lb["est"], lb["clean"], lengths=_cols(lb["lengths"]), filter_length=K)
        assert (score + loss.double()).abs().max() <= TOL_DB, "with eps = 0 the loss is minus the score"
    l2, g2 = _loss_and_grad(lb["est"], lb["clean"], lb["lengths"], K, eps)
    assert torch.equal(l2, loss) and torch.equal(g2, grad), "a second call"
    b = 2
    l1, g1 = _loss_and_grad(lb["est"][b:b + 1], lb["clean"][b:b + 1, None], torch.tensor(lb["lengths"][b:b + 1], device=dev), K, eps)
    assert torch.equal(l1[0], loss[b]) and torch.equal(g1[0], grad[b]), "a row alone, (B, 1, L) clean rows, device lengths"


def test_loss_reductions_and_grad_output_weights(dev, loss_batch):
    import eabnet_amd
    lb, K, eps = loss_batch, 512, 1e-8
    args = (lb["est"], lb["clean"], lb["lengths"], K, eps)
    none, g_none = _loss_and_grad(*args)
    total, g_sum = _loss_and_grad(*args, reduction="sum")
    mean, g_mean = _loss_and_grad(*args, reduction="mean")
    assert total.shape == () and mean.shape == () and total.dtype == torch.float32 and mean.dtype == torch.float32
    scale = float(none.abs().sum())
    assert abs(float(total) - float(none.double().sum())) <= 1e-6 * scale
    assert abs(float(mean) - float(none.double().sum()) / 4) <= 1e-6 * scale
    assert torch.equal(g_sum, g_none)
    assert (g_mean - g_none / 4).abs().max() <= 1e-6 * g_none.abs().max()
    weights = torch.tensor([0.5, -2.0, 3.0, 0.25], device=dev)
    _, g_w = _loss_and_grad(*args, weights=weights)
    for b, idx in enumerate(LOSS_ROWS):
        _, wgrad = R.cached("loss", idx, K, 0.0, eps)
        w, le = float(weights[b]), lb["lengths"][b][0]
        assert np.abs(g_w[b, :le].cpu().numpy() - w * wgrad).max() <= TOL_GRAD * abs(w) * _grad_scale(lb["pairs"][b], idx, K, wgrad, eps), b
    leaf = lb["est"].clone().requires_grad_(True)                 # a weight that reaches the node through later arithmetic
    (0.3 * eabnet_amd.sdr_loss(leaf, lb["clean"], lengths=lb["lengths"], filter_length=K, eps=eps)).backward()
    assert (leaf.grad - 0.3 * g_mean).abs().max() <= 1e-6 * g_mean.abs().max()


@pytest.mark.parametrize("eps", [0.0, 1e-8])
def test_one_tap_is_si_sdr_loss_on_the_same_rows(dev, loss_batch, eps):
    import eabnet_amd
    lb = loss_batch
    loss, grad = _loss_and_grad(lb["est"], lb["clean"], lb["lengths"], 1, eps)
    leaf = lb["est"].detach().requires_grad_(True)
    want = eabnet_amd.si_sdr_loss(leaf, lb["clean"], lengths=lb["lengths"], eps=eps, reduction="none")
    (wgrad,) = torch.autograd.grad(want, leaf, grad_outputs=torch.ones_like(want))
    want = want.detach()
    for b in range(4):
        le = lb["lengths"][b][0]
        scale = float(wgrad[b].abs().max()) if le > 1 else _grad_scale(lb["pairs"][b], b, 1, None, eps)
        gerr = float((grad[b] - wgrad[b]).abs().max()) / scale
        print(f"K 1, eps {eps:g}, row {b}: {float(loss[b]):.5f} against {float(want[b]):.5f} dB; gradient {gerr:.2e} (bound {TOL_GRAD:.0e})")
        assert abs(float(loss[b]) - float(want[b])) <= TOL_DB and gerr <= TOL_GRAD


# ------------------------------------------------------------------ the chain and the network
def _loss64(wav, clean, K, eps):
    """the definition in float64 torch operators: wav, clean (B, L) -> the mean loss"""
    B, L = wav.shape
    sp = torch.nn.functional.pad(clean, (K - 1, 0))
    S = torch.stack([sp[:, K - 1 - k:K - 1 - k + L] for k in range(K)], 1)                    # S[b, k, n] = s[n - k]
    r = torch.stack([(clean[:, :L - k] * clean[:, k:]).sum(1) for k in range(K)], 1)
    idx = (torch.arange(K)[:, None] - torch.arange(K)[None, :]).abs()
    c = (S * wav[:, None]).sum(2)
    h = torch.linalg.solve(r[:, idx], c)
    tgt, ee = (c * h).sum(1), (wav * wav).sum(1)
    return (-10.0 * (torch.log10(tgt + eps) - torch.log10(ee - tgt + eps))).mean()


def test_gradient_of_the_chain_vs_float64_torch(dev):
    import eabnet_amd
    B, T, n_fft, hop, K = 2, 12, 320, 160, 24
    rng = np.random.default_rng(300)
    out = rng.standard_normal((B, 2, T, n_fft // 2 + 1)).astype(np.float32)
    window = torch.hann_window(n_fft)

    def wave64(x):
        return torch.istft(torch.view_as_complex(x.permute(0, 3, 2, 1).contiguous()), n_fft, hop, n_fft, window.double())

    x64 = torch.from_numpy(out).double().requires_grad_(True)
    with torch.no_grad():
        wav64 = wave64(x64)
    early = torch.zeros_like(wav64)                               # the estimate is the clean wave 3 samples late, plus noise
    early[:, :-3] = wav64[:, 3:]
    clean = (0.8 * early + 0.3 * wav64.std() * torch.from_numpy(rng.standard_normal(tuple(wav64.shape)))).float()
    ref_loss = _loss64(wave64(x64), clean.double(), K, 1e-8)
    (want,) = torch.autograd.grad(ref_loss, x64)
    ref_loss = ref_loss.detach()
    assert -5.0 <= -float(ref_loss) <= 30.0
    leaf = torch.from_numpy(out).to(dev).requires_grad_(True)
    loss = eabnet_amd.sdr_loss(eabnet_amd.istft(leaf, n_fft, hop, window), clean.to(dev), filter_length=K, eps=1e-8)
    loss.backward()
    rel = float((leaf.grad.cpu().double() - want).abs().max() / want.abs().max())
    print(f"chain: loss {float(loss):.5f} (float64 {float(ref_loss):.5f}), gradient max |diff| / max |ref| = {rel:.2e} (bound {TOL_GRAD:.0e})")
    assert abs(float(loss) - float(ref_loss)) <= TOL_DB and rel <= TOL_GRAD


def test_one_training_step_with_the_term_leaves_finite_gradients(dev):
    import eabnet_amd
    B, T, M, hop = 2, 30, 2, 160
    window = torch.hann_window(320)
    net = eabnet_amd.EaBNet(M=M, p=1, q=1)
    net.load_state_dict(torch_params(M, 410, p=1, q=1), strict=True)
    net = net.to(dev).train()
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, 411)).to(dev)
    target = torch.from_numpy(paramgen.make_wave(B, 1, hop * (T - 1), 412)).to(dev)
    label = eabnet_amd.stft_compress(target, 320, hop, window, 1)
    y = net(x)
    l = eabnet_amd.com_mag_mse_loss(y, label, [T] * B)
    term = eabnet_amd.sdr_loss(eabnet_amd.istft(y, 320, hop, window), target, filter_length=64)
    (l + 0.05 * term).backward()
    grads = [p.grad for p in net.parameters() if p.requires_grad]
    assert torch.isfinite(term) and all(g is not None and torch.isfinite(g).all() for g in grads)
    spectral = [g.clone() for g in grads]
    net.zero_grad()
    eabnet_amd.com_mag_mse_loss(net(x), label, [T] * B).backward()
    assert any(not torch.equal(a, p.grad) for a, p in zip(spectral, [p for p in net.parameters() if p.requires_grad])), "the term reached the parameters"


# ------------------------------------------------------------------ the scorer
SAMPLES = [16007, 11200, 12999]


def test_scorer_adds_two_columns_and_changes_nothing_else(dev):
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=4, p=1, q=1)
    net.load_state_dict(torch_params(4, 12, p=1, q=1), strict=True)
    net = net.to(dev).eval()
    noisy = [torch.from_numpy(paramgen.make_wave(1, 4, n, 300 + k))[0] for k, n in enumerate(SAMPLES)]
    other = [torch.from_numpy(paramgen.make_wave(1, 1, n, 350 + k))[0, 0] for k, n in enumerate(SAMPLES)]
    clean = [0.7 * x[0] + 0.3 * c for x, c in zip(noisy, other)]
    base = eabnet_amd.Scorer(net, max_batch=4)(noisy, clean)
    scores, waves = eabnet_amd.Scorer(net, max_batch=4, distortion=True)(noisy, clean, return_waves=True)
    assert list(base) == ["si_sdr", "si_sir", "si_sar", "si_sdr_mix", "loss"]
    assert list(scores) == list(base) + ["sdr", "sdr_mix"]
    for m in base:
        assert np.array_equal(base[m], scores[m]), f"{m} changed with distortion=True"
    for k, n in enumerate(SAMPLES):
        c = clean[k][None].to(dev)
        by_hand = float(eabnet_amd.sdr(waves[k][None].to(dev), c)[0])
        mix = float(eabnet_amd.sdr(noisy[k][0][None].to(dev), c)[0])
        print(f"file {k}: sdr {scores['sdr'][k]:.4f} dB (si_sdr {scores['si_sdr'][k]:.4f}), sdr_mix {scores['sdr_mix'][k]:.4f} dB")
        assert scores["sdr"][k] == by_hand and scores["sdr_mix"][k] == mix, (k, by_hand, mix)
        assert scores["sdr"][k] >= scores["si_sdr"][k] - TOL_DB, "512 taps project on more than one"
    assert all(v.shape == (3,) and np.isfinite(v).all() for v in scores.values())
    both = eabnet_amd.Scorer(net, max_batch=4, intelligibility=True, distortion=True)(noisy, clean)
    assert list(both) == list(base) + ["stoi", "estoi", "sdr", "sdr_mix"]
    assert np.array_equal(both["sdr"], scores["sdr"]) and np.array_equal(both["sdr_mix"], scores["sdr_mix"])
