"""Scores on the MI355X: the energy-ratio and per-utterance-loss kernels (csrc/score.hip) against the reference's recorded values
and the float64 restatement of tests/score_ref.py, and ``eabnet_amd.Scorer`` against ``Enhancer`` plus host scoring of its waves.

4.34e-4 dB = 10 log10(1 + 1e-4): the project's 1e-4 relative bar (util.TOL_HIP) on a power ratio."""
import argparse

import numpy as np
import pytest
import torch

import paramgen
import score_ref
from util import TOL_HIP, load, torch_params

pytestmark = pytest.mark.gpu

TOL_DB = 10.0 * np.log10(1.0 + TOL_HIP)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases():
    """every fixture case as (clean, noisy, estimate) fp32 arrays, built once"""
    return [score_ref.make_case(*c) for c in score_ref.CASES]


def _padded(rows, dev, fill=float("nan")):
    """(B, longest) device buffer, everything past a row's length poisoned"""
    buf = torch.full((len(rows), max(len(r) for r in rows)), fill, dtype=torch.float32)
    for b, r in enumerate(rows):
        buf[b, :len(r)] = torch.from_numpy(r)
    return buf.to(dev)


def _batch(cases, dev):
    import eabnet_amd
    clean, noisy, est = ([c[j] for c in cases] for j in range(3))
    lengths = ([len(r) for r in est], [len(r) for r in clean], [len(r) for r in noisy])
    return eabnet_amd.energy_ratios(_padded(est, dev), _padded(clean, dev), _padded(noisy, dev), lengths=lengths, energies=True)


# ------------------------------------------------------------------ energy ratios
def test_ratios_of_all_fixture_cases_in_one_padded_batch(dev, cases):
    import eabnet_amd
    want = load("score_cases.npz")["ratios"]
    got = _batch(cases, dev)
    assert got.shape == (len(cases), 8) and got.dtype == torch.float64
    g = got.cpu().numpy()
    err = np.abs(g[:, :4] - want)
    for k in range(len(cases)):
        print(f"case {k} {score_ref.CASES[k][:3]}: {g[k, :4]} max |diff| {err[k].max():.3e} dB")
    print(f"largest difference to the reference: {err.max():.3e} dB (bound {TOL_DB:.3e})")
    assert np.isfinite(g).all() and err.max() <= TOL_DB
    # the energies the ratios are made of, and device lengths
    assert np.allclose(10 * np.log10(g[:, 4] / g[:, 7]), g[:, 0], rtol=0, atol=1e-12)
    assert np.allclose(10 * np.log10(g[:, 4] / g[:, 5]), g[:, 1], rtol=0, atol=1e-12)
    assert np.allclose(10 * np.log10(g[:, 4] / g[:, 6]), g[:, 2], rtol=0, atol=1e-12)
    clean, noisy, est = ([c[j] for c in cases] for j in range(3))
    dl = tuple(torch.tensor([len(r) for r in rows], device=dev) for rows in (est, clean, noisy))
    four = eabnet_amd.energy_ratios(_padded(est, dev), _padded(clean, dev), _padded(noisy, dev), lengths=dl)
    assert four.shape == (len(cases), 4) and torch.equal(four, got[:, :4]), "host and device lengths disagree"


def test_ratios_have_the_same_bits_alone_in_a_batch_and_again(dev, cases):
    import eabnet_amd
    got = _batch(cases, dev)
    assert torch.equal(_batch(cases, dev), got), "a second call differs"
    for k, (clean, noisy, est) in enumerate(cases):
        one = eabnet_amd.energy_ratios(*(torch.from_numpy(v)[None].to(dev) for v in (est, clean, noisy)), energies=True)
        assert torch.equal(one[0], got[k]), f"case {k}: alone {one[0].tolist()} != in the batch {got[k].tolist()}"
    sub = _batch(cases[3:6], dev)                        # other neighbours, another row length
    assert torch.equal(sub, got[3:6])


def test_ratios_read_strided_and_unaligned_rows_in_place(dev, cases):
    """y as channel 2 of a (B, 4, L) buffer; the estimate with a row stride above its length at a base that is not 16-byte
    aligned; the clean rows at an odd stride, so that every row has another alignment"""
    import eabnet_amd
    pick = [cases[k] for k in (2, 3, 5, 6, 1)]
    clean, noisy, est = ([c[j] for c in pick] for j in range(3))
    B = len(pick)
    Ly, Le, Ls = (max(len(r) for r in rows) for rows in (noisy, est, clean))
    ybuf = torch.full((B, 4, Ly), float("nan"), device=dev)
    ebig = torch.full((B * (Le + 37) + 1,), float("nan"), device=dev)
    eview = ebig[1:].view(B, Le + 37)[:, :Le]
    sbig = torch.full((B, Ls + 1), float("nan"), device=dev)
    sview = sbig[:, :Ls]
    assert eview.data_ptr() % 16 == 4 and eview.stride(0) == Le + 37 and sview.stride(0) % 4 != 0
    for b in range(B):
        ybuf[b, 2, :len(noisy[b])] = torch.from_numpy(noisy[b]).to(dev)
        ybuf[b, [0, 1, 3], :] = 7.0                       # the other channels are not the reference channel
        eview[b, :len(est[b])] = torch.from_numpy(est[b]).to(dev)
        sview[b, :len(clean[b])] = torch.from_numpy(clean[b]).to(dev)
    lengths = ([len(r) for r in est], [len(r) for r in clean], [len(r) for r in noisy])
    got = eabnet_amd.energy_ratios(eview, sview, ybuf[:, 2], lengths=lengths)
    want = np.stack([score_ref.ratios(est[b], clean[b], noisy[b]) for b in range(B)])
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"strided rows: {err:.3e} dB from the restatement")
    assert err <= TOL_DB
    # the load path (one 16-byte load or four 4-byte loads) does not change the bits
    packed = eabnet_amd.energy_ratios(_padded(est, dev), _padded(clean, dev), _padded(noisy, dev), lengths=lengths)
    assert torch.equal(got, packed)


def test_a_silent_row_is_nan_in_its_own_row_only(dev, cases):
    import eabnet_amd
    pick = [cases[k] for k in (1, 3, 4, 2)]
    good = _batch(pick, dev)
    silent = [(np.zeros_like(c[0]) if k == 1 else c[0], c[1], c[2]) for k, c in enumerate(pick)]
    got = _batch(silent, dev)
    assert torch.isnan(got[1, :4]).all(), got[1]         # (|e_noise|^2 alone needs no clean signal and stays finite)
    for k in (0, 2, 3):
        assert torch.equal(got[k], good[k]), f"row {k} changed beside a silent row"
    # no noise (y = s): the three ratios are NaN as numpy's 0/0 in the reference, that row only
    clean, noisy, est = pick[0]
    same = eabnet_amd.energy_ratios(*(torch.from_numpy(v)[None].to(dev) for v in (est, clean, clean)))
    assert torch.isnan(same[0, :3]).all()


# ------------------------------------------------------------------ per-utterance loss
def _loss_fixture(dev):
    g = load("e2e_M8_B2_T20.npz")
    esti = torch.from_numpy(g["out"]).to(dev)
    label = torch.from_numpy(paramgen.make_spec_input(2, 20, 161, 1, int(g["label_seed"]))[..., 0, :]).permute(0, 3, 1, 2).contiguous().to(dev)
    return esti, label


def test_loss_per_utterance_vs_reference_fixtures(dev):
    import eabnet_amd
    gs = load("score_cases.npz")
    esti, label = _loss_fixture(dev)
    for j, n in enumerate(int(v) for v in gs["loss_frames"]):
        got = eabnet_amd.com_mag_mse_loss_per_utterance(esti, label, [n, n])
        assert got.shape == (2,) and got.dtype == torch.float64
        for b in range(2):
            want = float(gs["loss"][b, j])
            print(f"utterance {b} at {n} frames: {float(got[b]):.9f} vs {want:.9f}")
            assert abs(float(got[b]) - want) <= 1e-5 * want
    # ragged, poisoned past the counts, device counts; each utterance keeps the bits it has alone
    frames = [13, 20]
    pe, pl = esti.clone(), label.clone()
    pe[0, :, 13:] = float("nan")
    pl[0, :, 13:] = float("nan")
    ragged = eabnet_amd.com_mag_mse_loss_per_utterance(pe, pl, torch.tensor(frames, device=dev))
    assert torch.equal(ragged, eabnet_amd.com_mag_mse_loss_per_utterance(esti, label, frames)), "NaN past n_b changed the value"
    for b, n in enumerate(frames):
        alone = eabnet_amd.com_mag_mse_loss_per_utterance(esti[b:b + 1, :, :n].contiguous(), label[b:b + 1], [n])
        assert torch.equal(alone[0], ragged[b]), f"utterance {b}: alone != in the batch"
    # the batch loss is the frame-weighted mean of the rows: both are means over the same masked bins
    batch = float(eabnet_amd.com_mag_mse_loss(esti, label, frames))
    mean = float((ragged.cpu() * torch.tensor(frames)).sum() / sum(frames))
    assert abs(mean - batch) <= 1e-5 * batch, (mean, batch)


def test_loss_per_utterance_has_no_bound_on_the_batch(dev):
    """B = 70 (the batch form stops at 64), T * F = 1127 and 4830 bins: one span and two"""
    import eabnet_amd
    torch.manual_seed(11)
    for T in (7, 30):
        esti, label = torch.randn(70, 2, T, 161), torch.randn(70, 2, T, 161)
        frames = [1 + (3 * b) % T for b in range(70)]
        got = eabnet_amd.com_mag_mse_loss_per_utterance(esti.to(dev), label.to(dev), frames).cpu().numpy()
        want = np.array([score_ref.loss_one(esti[b].numpy(), label[b].numpy(), frames[b]) for b in range(70)])
        assert np.abs(got / want - 1.0).max() <= 1e-5, np.abs(got / want - 1.0).max()


# ------------------------------------------------------------------ the scorer
SAMPLES = [48000, 6400, 30123, 9999, 16007]             # 0.4 s .. 3 s: 301, 41, 189, 63, 101 frames


def _files(seed):
    noisy = [torch.from_numpy(paramgen.make_wave(1, 4, n, seed + k))[0] for k, n in enumerate(SAMPLES)]
    clean = [torch.from_numpy(paramgen.make_wave(1, 1, n, seed + 50 + k))[0, 0] for k, n in enumerate(SAMPLES)]
    return noisy, [0.7 * x[0] + 0.3 * c for x, c in zip(noisy, clean)]            # clean correlates with the noisy channels


def _two_stage(dev):
    import eabnet_amd
    args = argparse.Namespace(
        k1=(2, 3), k2=(1, 3), c=64, M=4, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=1, q=1, is_causal=True, is_u2=True,
        bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="IN", ref_mic=0, freeze_eabnet=False,
        gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=1,
        gagnet_q=2, gagnet_dilas=[1, 2], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=True,
        gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="IN")
    torch.manual_seed(0)
    net = eabnet_amd.make_eabnet_with_postnet(args).to(dev).eval()
    with torch.no_grad():
        for p in net.parameters():                       # off the default initialisation, deterministic
            p.add_(0.02 * torch.randn_like(p))
    return net


def _single(dev, **kw):
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=4, p=1, q=1, **kw)
    net.load_state_dict(torch_params(4, 12, p=1, q=1, **kw), strict=True)
    return net.to(dev).eval()


@pytest.mark.parametrize("kind,ref_mic,on_device", [("eabnet", 1, False), ("two_stage", 0, True), ("non_causal", 0, False)])
def test_scorer_end_to_end(dev, kind, ref_mic, on_device):
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    net = _two_stage(dev) if kind == "two_stage" else _single(dev, is_causal=kind != "non_causal")
    noisy, clean = _files(300)
    if on_device:
        noisy, clean = [x.to(dev) for x in noisy], [c.to(dev) for c in clean]
    scorer = eabnet_amd.Scorer(net, max_batch=4, ref_mic=ref_mic)
    scores, waves = scorer(noisy, clean, return_waves=True)
    assert set(scores) == {"si_sdr", "si_sir", "si_sar", "si_sdr_mix", "loss"}
    assert all(v.shape == (5,) and v.dtype == np.float64 and np.isfinite(v).all() for v in scores.values())
    plan = [(len(b["indices"]), b["cap"], b["batch_size"]) for b in scorer.last_plan["batches"]]
    assert plan == ([(1, None, 1)] * 5 if kind == "non_causal" else [(4, 512, 4), (1, 64, 1)]), plan
    # the waves are Enhancer's
    ref_waves = eabnet_amd.Enhancer(net, max_batch=4)(noisy)
    for k in range(5):
        assert torch.equal(waves[k], ref_waves[k]), f"file {k}: the scorer's wave is not the enhancer's"
    only = scorer(noisy, [c[None] for c in clean])                          # (1, L) clean waves, scores alone
    assert all(np.array_equal(only[m], scores[m]) for m in scores)
    # the four ratios of those waves, scored on the host
    got = np.stack([scores[m] for m in ("si_sdr", "si_sir", "si_sar", "si_sdr_mix")], axis=1)
    want = np.stack([score_ref.ratios(waves[k].cpu().numpy(), clean[k].cpu().numpy(), noisy[k][ref_mic].cpu().numpy())
                     for k in range(5)])
    err = np.abs(got - want).max()
    print(f"{kind}: ratios {err:.3e} dB from the restatement\n{got}")
    assert err <= TOL_DB
    # the mixture's SI-SDR is the ratio kernel's SI-SDR of the noisy channel as the estimate
    for k in range(5):
        y, s = noisy[k][ref_mic][None].to(dev), clean[k][None].to(dev)
        mix = float(eabnet_amd.energy_ratios(y, s, y)[0, 0])
        assert abs(mix - scores["si_sdr_mix"][k]) <= 1e-9, (k, mix, scores["si_sdr_mix"][k])
    # the loss of the one-at-a-time chain's estimate against its label, by the reference's expression on the host
    win = torch.hann_window(320)
    with torch.no_grad():
        for k in range(5):
            y = net(eabnet_amd.stft_compress(noisy[k][None].to(dev), 320, 160, win))
            y = y["esti_stft"] if isinstance(y, dict) else y
            label = eabnet_amd.stft_compress(clean[k][None, None].to(dev), 320, 160, win, 1)
            ref = float(orc.com_mag_mse_loss(y.cpu(), label.cpu(), [y.shape[2]]))
            print(f"{kind} file {k}: loss {scores['loss'][k]:.7f} vs {ref:.7f}")
            assert abs(scores["loss"][k] - ref) <= 1e-4 * ref
    summary = scorer.summary(scores)
    assert summary["si_sdr"] == (float(np.mean(scores["si_sdr"])), float(np.std(scores["si_sdr"])))
    assert net.length_buckets is None
