"""``eabnet_amd.stoi_loss`` and the differentiable ``resample`` on the MI355X against the float64 references of
tests/stoi_loss_ref.py: the gradient at 10 kHz on one NaN-poisoned padded batch (three factor settings, random grad_output), the
exact zeros, the value and same-bits contracts, the resampler's adjoint, the chain ``istft -> stoi_loss(sample_rate=16000)`` and two
optimiser steps of a small network.

Bounds.  Gradients: 1e-5 of max |ref| per utterance, the bar of the two other waveform-loss gradients; the host emulation of the same
kernels (tests/test_stoi_loss_host_emulation.py) sits at 2e-7 to 5e-7 on these cases, so no fp32-restatement floor is needed.
Every gradient case keeps |alpha Y - bound| / bound > 1e-4 on every element and 0.05 dB on every frame
(tests/test_stoi_loss_ref.py asserts it on the CPU); no element is excluded from a comparison.  Values: bit for bit the fp32
rounding of ``intelligibility``'s fp64 scores.  Resampler adjoint: 1e-5 of max |ref| per row, the ISTFT adjoint's bar."""
import numpy as np
import pytest
import torch

import paramgen
import stoi_loss_ref as G
import stoi_ref as R
from util import torch_params

pytestmark = pytest.mark.gpu

TOL_GRAD = 1e-5
FACTORS = ((1.0, 0.0), (0.0, 1.0), (0.5, 0.5))
KS = tuple(G.GRAD_CASES) + (-1,) + tuple(G.SENTINEL_CASES)          # the padded batch: gradient cases, short est, sentinels


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def data(dev):
    """every 10 kHz utterance of these tests, built once: the fp32 pairs, their float64 gradients at the three factor settings, and
    the padded batch on the device with NaN past every length"""
    pairs = [R.make_case(*(R.CASES[k] if k >= 0 else G.SHORT_EST_CASE)) for k in KS]
    ref = {f: [G.loss_and_grad(c, e, *f)[1] for c, e in pairs] for f in FACTORS}
    le, ls = [len(e) for _, e in pairs], [len(c) for c, _ in pairs]
    est, clean = torch.full((len(KS), max(le)), float("nan")), torch.full((len(KS), max(ls)), float("nan"))
    for b, (c, e) in enumerate(pairs):
        est[b, :le[b]], clean[b, :ls[b]] = torch.from_numpy(e), torch.from_numpy(c)
    rng = np.random.default_rng(77)
    weights = torch.from_numpy((rng.uniform(0.5, 2.0, len(KS)) * rng.choice([-1.0, 1.0], len(KS))).astype(np.float32))
    return {"pairs": pairs, "ref": ref, "est": est.to(dev), "clean": clean.to(dev), "lengths": [[a, b] for a, b in zip(le, ls)],
            "weights": weights.to(dev)}


def _loss_and_grad(est, clean, lengths=None, reduction="none", weights=None, sample_rate=10000, factors=(1.0, 0.0)):
    import eabnet_amd
    leaf = est.detach().requires_grad_(True)                 # (shares est's memory and strides: a view stays a view)
    loss = eabnet_amd.stoi_loss(leaf, clean, lengths, sample_rate, factors[0], factors[1], reduction)
    (g,) = torch.autograd.grad(loss, leaf, grad_outputs=weights if weights is not None else torch.ones_like(loss))
    return loss.detach(), g


@pytest.mark.parametrize("factors", FACTORS)
def test_gradient_of_a_padded_batch_vs_float64(dev, data, factors):
    loss, grad = _loss_and_grad(data["est"], data["clean"], data["lengths"], weights=data["weights"], factors=factors)
    assert torch.isfinite(grad).all(), "a sample past an utterance's length was read"
    g = grad.cpu().numpy()
    for b, k in enumerate(KS):
        n = data["lengths"][b][0]
        ref = data["ref"][factors][b] * float(data["weights"][b])
        assert (g[b, n:] == 0).all(), "the gradient from est's own length to the row's end is exactly zero"
        assert (g[b, :n][ref == 0] == 0).all(), "samples of removed frames that no kept frame covers, or past the last frame"
        scale = np.abs(ref).max()
        if k in G.SENTINEL_CASES:
            assert scale == 0 and (g[b] == 0).all() and float(loss[b]) == np.float32(-(factors[0] + factors[1]) * R.SENTINEL)
            continue
        rel = float(np.abs(g[b, :n] - ref).max() / scale)
        print(f"case {k} factors {factors}: gradient max |diff| / max |ref| = {rel:.2e} (bound {TOL_GRAD:.0e})")
        assert rel <= TOL_GRAD, (k, factors)
    # the case with removed frames has zeros strictly inside the signal (the middle of its gap)
    b = KS.index(4)
    assert (data["ref"][factors][b][4300:4900] == 0).all() and (g[b, 4300:4900] == 0).all()


def test_value_is_the_fp32_rounding_of_the_scores_bit_for_bit(dev, data):
    import eabnet_amd
    est, clean, lengths = data["est"], data["clean"], data["lengths"]
    pair = ([l[0] for l in lengths], [l[1] for l in lengths])
    sc = eabnet_amd.intelligibility(est, clean, pair, sample_rate=10000)
    for fs, fe in FACTORS + ((0.3, 1.7),):
        want = -(fs * sc[:, 0] + fe * sc[:, 1])
        with torch.no_grad():
            none = eabnet_amd.stoi_loss(est, clean, lengths, 10000, fs, fe, "none")
            total = eabnet_amd.stoi_loss(est, clean, lengths, 10000, fs, fe, "sum")
            mean = eabnet_amd.stoi_loss(est, clean, lengths, 10000, fs, fe)
        assert none.dtype == torch.float32 and torch.equal(none, want.to(torch.float32))
        assert total.shape == () and torch.equal(total, want.sum().to(torch.float32))
        assert torch.equal(mean, (want.sum() / len(KS)).to(torch.float32))
    # the six-second case (values only: three of its elements lie within 1e-4 of the clip bound)
    c, e = (torch.from_numpy(v)[None].to(dev) for v in R.make_case(*R.CASES[8]))
    with torch.no_grad():
        got = eabnet_amd.stoi_loss(e, c[:, None], sample_rate=10000, factor_stoi=0.5, factor_estoi=0.5, reduction="none")
    s8 = eabnet_amd.intelligibility(e, c, sample_rate=10000)
    assert torch.equal(got, (-(0.5 * s8[:, 0] + 0.5 * s8[:, 1])).to(torch.float32))
    assert abs(float(s8[0, 0]) - R.EXPECTED[8][2]) < 1e-5
    # at 16 kHz: the same resampling as intelligibility, each signal with its own length
    e16, c16 = est[:4, :9000].contiguous(), clean[:4, :9000].contiguous()
    l16 = [[min(a, 9000), min(b, 9000)] for a, b in lengths[:4]]
    s16 = eabnet_amd.intelligibility(e16, c16, ([l[0] for l in l16], [l[1] for l in l16]), sample_rate=16000)
    got = eabnet_amd.stoi_loss(e16.clone().requires_grad_(True), c16, l16, 16000, 0.5, 0.5, "none")
    assert got.requires_grad and torch.equal(got.detach(), (-(0.5 * s16[:, 0] + 0.5 * s16[:, 1])).to(torch.float32))


def test_rows_have_the_same_bits_alone_in_a_batch_strided_at_any_alignment_and_in_a_second_call(dev, data):
    est, clean, lengths, f = data["est"], data["clean"], data["lengths"], (0.5, 0.5)
    loss, grad = _loss_and_grad(est, clean, lengths, factors=f)
    l2, g2 = _loss_and_grad(est, clean, lengths, factors=f)
    assert torch.equal(l2, loss) and torch.equal(g2, grad), "a second call gives other bits"
    for b in (1, 4, 7):                                      # alone, in rows of its own lengths
        c, e = (torch.from_numpy(v)[None].to(dev) for v in data["pairs"][b])
        l1, g1 = _loss_and_grad(e, c, factors=f)
        assert torch.equal(l1[0], loss[b]) and torch.equal(g1[0], grad[b, :e.shape[1]]), KS[b]
    # est rows that are views of a wider, unaligned buffer (a channel of it), (B, 1, Ls) clean rows, a device tensor of lengths
    B, W = est.shape
    wide = torch.full((B, 2, W + 7), float("nan"), device=dev)
    wide[:, 1, 3:3 + W] = est
    l3, g3 = _loss_and_grad(wide[:, 1, 3:3 + W], clean[:, None], torch.tensor(lengths, device=dev), factors=f)
    assert torch.equal(l3, loss) and torch.equal(g3, grad)
    # a batch in another order
    perm = [4, 0, 7]
    l4, g4 = _loss_and_grad(est[perm], clean[perm], [lengths[b] for b in perm], factors=f)
    assert torch.equal(l4, loss[perm]) and torch.equal(g4, grad[perm])


def test_reductions_grad_output_and_no_double_backward(dev, data):
    import eabnet_amd
    est, clean, lengths, f = data["est"], data["clean"], data["lengths"], (0.5, 0.5)
    _, g_none = _loss_and_grad(est, clean, lengths, factors=f)
    _, g_sum = _loss_and_grad(est, clean, lengths, "sum", factors=f)
    _, g_mean = _loss_and_grad(est, clean, lengths, "mean", factors=f)
    assert torch.equal(g_sum, g_none)
    assert (g_mean - g_none / len(KS)).abs().max() <= 1e-6 * g_none.abs().max()
    leaf = est.clone().requires_grad_(True)                  # a weight that reaches the node through later arithmetic
    (0.3 * eabnet_amd.stoi_loss(leaf, clean, lengths, 10000, *f)).backward()
    assert (leaf.grad - 0.3 * g_mean).abs().max() <= 1e-6 * g_mean.abs().max()
    leaf = est.clone().requires_grad_(True)
    w = torch.ones((), device=dev, requires_grad=True)       # (a grad_output that requires grad: the node is asked for a graph)
    loss = w * eabnet_amd.stoi_loss(leaf, clean, lengths, 10000, *f)
    (g,) = torch.autograd.grad(loss, leaf, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


RATES = [(16000, 10000), (48000, 16000), (16000, 48000), (44100, 16000)]


@pytest.mark.parametrize("orig,new", RATES)
def test_resample_adjoint_vs_float64(dev, orig, new):
    import eabnet_amd
    rng = np.random.default_rng(orig // 100 + new // 100)
    worst = 0.0

    def check(x, lengths, tag):
        nonlocal worst
        plain = eabnet_amd.resample(x.to(dev), orig, new, lengths=lengths)
        leaf = x.to(dev).requires_grad_(True)
        y = eabnet_amd.resample(leaf, orig, new, lengths=lengths)
        assert y.requires_grad and torch.equal(y.detach(), plain), "the forward values with and without requires_grad"
        g = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
        y.backward(g.to(dev))
        got = leaf.grad.cpu().numpy().reshape(-1, x.shape[-1])
        g2 = g.numpy().reshape(-1, y.shape[-1]).astype(np.float64)
        per_row = got.shape[0] // (len(lengths) if lengths is not None else got.shape[0])
        for r in range(got.shape[0]):
            n = x.shape[-1] if lengths is None else lengths[r // per_row]
            ref = G.resample_adjoint(g2[r], x.shape[-1], orig, new, length=n)
            assert (got[r, n:] == 0).all(), "the gradient past a row's length"
            rel = float(np.abs(got[r] - ref).max() / np.abs(ref).max())
            worst = max(worst, rel)
            assert rel <= TOL_GRAD, (tag, r, rel)

    for L in (1, 7, 300, 1025):                              # 1025: a second tile of 256 input samples and of 1024 outputs
        check(torch.from_numpy(rng.standard_normal((2, L)).astype(np.float32)), None, L)
    check(torch.from_numpy(rng.standard_normal((3, 1025)).astype(np.float32)), [1025, 300, 7], "padded")
    check(torch.from_numpy(rng.standard_normal((2, 2, 300)).astype(np.float32)), [300, 123], "padded (B, M, L)")
    print(f"{orig} -> {new}: adjoint max |diff| / max |ref| = {worst:.2e} (bound {TOL_GRAD:.0e})")


def test_gradient_of_the_chain_istft_to_stoi_loss_at_16_khz_vs_float64_torch(dev):
    import eabnet_amd
    c = G.CHAIN
    spec, clean = G.chain_case()
    x64 = torch.from_numpy(spec).double().requires_grad_(True)
    ref_loss, infos = G.chain_loss64(x64, clean, 0.5, 0.5)
    assert all(i["T"] >= R.N_SEG and i["clip_margin"] > G.CLIP_MARGIN for i in infos)
    (want,) = torch.autograd.grad(ref_loss, x64)
    leaf = torch.from_numpy(spec).to(dev).requires_grad_(True)
    wav = eabnet_amd.istft(leaf, c["n_fft"], c["hop"], torch.hann_window(c["n_fft"]))
    loss = eabnet_amd.stoi_loss(wav, torch.from_numpy(clean).to(dev)[:, None], sample_rate=16000, factor_stoi=0.5, factor_estoi=0.5)
    loss.backward()
    rel = float((leaf.grad.cpu().double() - want).abs().max() / want.abs().max())
    print(f"chain: loss {float(loss.detach()):.6f} (float64 {float(ref_loss.detach()):.6f}), gradient max |diff| / max |ref| = {rel:.2e} "
          f"(bound {TOL_GRAD:.0e})")
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-5 and rel <= TOL_GRAD


def test_two_optimiser_steps_with_and_without_the_term(dev):
    """two FlatAdam steps of a small EaBNet on the spectral loss alone, then with the term added, then alone again: the term reaches
    every parameter with a finite gradient and changes the step.  The step without the term calls none of the new code (no
    ``stoi_loss``, and ``resample`` on inputs that do not require grad takes its old path), so it is today's step by construction;
    its bits cannot be compared run against run, because the weight-gradient kernels add with fp32 atomics (DESIGN: "the
    program's own run-to-run floor").  What is compared: the first loss (one forward pass from the same parameters) to 1e-6
    relative, and the second (after one Adam step of lr 5e-4 on gradients that differ by that floor) to 1e-4."""
    import eabnet_amd
    B, T, Mics, hop = 2, 48, 2, 160
    window = torch.hann_window(320)
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, Mics, 741)).to(dev)
    target = torch.from_numpy(paramgen.make_wave(B, 1, hop * (T - 1) + 32, 742)).to(dev)
    label = eabnet_amd.stft_compress(target[:, :, :hop * (T - 1)].contiguous(), 320, hop, window, 1)

    def run(weight):
        net = eabnet_amd.EaBNet(M=Mics, p=1, q=1)
        net.load_state_dict(torch_params(Mics, 740, p=1, q=1), strict=True)
        net = net.to(dev).train()
        params = [p for p in net.parameters() if p.requires_grad]
        opt = eabnet_amd.FlatAdam(params, lr=5e-4, max_grad_norm=1.0)
        losses = []
        for _ in range(2):
            out = net(x)
            loss = eabnet_amd.com_mag_mse_loss(out, label, [T] * B)
            if weight:
                loss = loss + weight * eabnet_amd.stoi_loss(eabnet_amd.istft(out, 320, hop, window), target, factor_estoi=1.0)
            losses.append(float(loss.detach()))
            opt.zero_grad(set_to_none=True)
            loss.backward()
            assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params), "every parameter receives a finite gradient"
            opt.step()
        return losses, torch.cat([p.detach().reshape(-1) for p in params]).clone()

    base_losses, base = run(0.0)
    term_losses, with_term = run(0.5)
    again_losses, again = run(0.0)
    print(f"two FlatAdam steps: spectral {base_losses}, with 0.5 * stoi_loss {term_losses}")
    assert np.isfinite(term_losses).all() and not torch.equal(with_term, base), "the term changes the step"
    assert abs(again_losses[0] - base_losses[0]) <= 1e-6 * abs(base_losses[0]), "the step without the term, after the term ran"
    assert abs(again_losses[1] - base_losses[1]) <= 1e-4 * abs(base_losses[1])
