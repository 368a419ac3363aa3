"""STOI / ESTOI on the MI355X: the kernels of csrc/stoi.hip behind ``eabnet_amd.intelligibility`` against the float64 restatement of
tests/stoi_ref.py (pinned by tests/test_stoi_ref.py), the same-bits contract, rows read in place, the resampled path, ``Scorer``
with the two extra columns and the ``stoi`` wrapper.

1e-4 absolute on a score: the project's bar (util.TOL_HIP) applied to a quantity in [-1, 1].  Measured on the MI355X: scores
within 1.07e-8 and band values within 1.02e-7 of the largest, over the ten cases."""
import numpy as np
import pytest
import torch

import paramgen
import stoi_ref as R
from util import TOL_HIP, torch_params

pytestmark = pytest.mark.gpu

TOL_SCORE = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases():
    """every case as (clean, estimate) fp32 arrays, built once"""
    return [R.make_case(*c) for c in R.CASES]


@pytest.fixture(scope="module")
def analysed(cases):
    return [R.analyse(c.astype(np.float64), e.astype(np.float64)) for c, e in cases]


def _padded(rows, dev, fill=float("nan")):
    """(B, longest) device buffer, everything past a row's length poisoned"""
    buf = torch.full((len(rows), max(len(r) for r in rows)), fill, dtype=torch.float32)
    for b, r in enumerate(rows):
        buf[b, :len(r)] = torch.from_numpy(r)
    return buf.to(dev)


def _batch(pick, dev, device_lengths=False, **kw):
    import eabnet_amd
    clean, est = [c[0] for c in pick], [c[1] for c in pick]
    lengths = ([len(r) for r in est], [len(r) for r in clean])
    if device_lengths:
        lengths = tuple(torch.tensor(l, device=dev) for l in lengths)
    return eabnet_amd.intelligibility(_padded(est, dev), _padded(clean, dev), lengths=lengths, sample_rate=10000, **kw)


def test_all_cases_in_one_poisoned_batch_match_the_restatement(dev, cases, analysed):
    got, tap = _batch(cases, dev, taps=True)
    assert got.shape == (len(cases), 2) and got.dtype == torch.float64
    g, K, kept, tob = got.cpu().numpy(), tap["K"].cpu().numpy(), tap["kept"].cpu().numpy(), tap["tob"].cpu().numpy()
    worst = worst_tob = 0.0
    for k, a in enumerate(analysed):
        assert K[k] == a["K"], (k, K[k], a["K"])
        assert np.array_equal(kept[k, :K[k]], a["kept"]), f"case {k}: the kept frames differ"
        T = max(a["K"] - 1, 0)
        rel = 0.0
        if T:
            rel = float(np.abs(tob[k, :, :, :T] - a["tob"]).max() / a["tob"].max())
        err = max(abs(g[k, 0] - a["stoi"]), abs(g[k, 1] - a["estoi"]))
        print(f"case {k}: K {K[k]} stoi {g[k, 0]:.9f} estoi {g[k, 1]:.9f}  |diff| {err:.3e}  bands {rel:.3e} of the largest")
        assert rel <= TOL_HIP, k
        assert err <= TOL_SCORE, k
        worst, worst_tob = max(worst, err), max(worst_tob, rel)
    print(f"largest difference to the restatement: scores {worst:.3e} (bound {TOL_SCORE:.0e}), bands {worst_tob:.3e} (bound {TOL_HIP:.0e})")
    assert np.isfinite(g).all()
    assert g[1, 0] == 1e-5 and g[1, 1] == 1e-5 and g[2, 0] == 1e-5 and g[2, 1] == 1e-5      # the sentinel, exactly


def test_scores_have_the_same_bits_alone_in_a_batch_and_again(dev, cases):
    import eabnet_amd
    got = _batch(cases, dev)
    assert torch.equal(_batch(cases, dev), got), "a second call differs"
    assert torch.equal(_batch(cases, dev, device_lengths=True), got), "host and device lengths disagree"
    for k, (clean, est) in enumerate(cases):
        one = eabnet_amd.intelligibility(torch.from_numpy(est)[None].to(dev), torch.from_numpy(clean)[None].to(dev), sample_rate=10000)
        assert torch.equal(one[0], got[k]), f"case {k}: alone {one[0].tolist()} != in the batch {got[k].tolist()}"
    assert torch.equal(_batch(cases[4:7], dev), got[4:7])                 # other neighbours, another row length


def test_rows_are_read_in_place_strided_and_unaligned(dev, cases):
    """the clean rows as channel 2 of a (B, 4, L) buffer; the estimate at a row stride above its length and a base that is not
    16-byte aligned, so that the rows take the one-by-one loads"""
    import eabnet_amd
    pick = [cases[k] for k in (5, 3, 7, 0, 4)]
    clean, est = [c[0] for c in pick], [c[1] for c in pick]
    B = len(pick)
    Ls, Le = max(len(r) for r in clean), max(len(r) for r in est)
    sbuf = torch.full((B, 4, Ls), float("nan"), device=dev)
    ebig = torch.full((B * (Le + 37) + 1,), float("nan"), device=dev)
    eview = ebig[1:].view(B, Le + 37)[:, :Le]
    assert eview.data_ptr() % 16 == 4 and eview.stride(0) == Le + 37
    for b in range(B):
        sbuf[b, 2, :len(clean[b])] = torch.from_numpy(clean[b]).to(dev)
        sbuf[b, [0, 1, 3], :] = 7.0
        eview[b, :len(est[b])] = torch.from_numpy(est[b]).to(dev)
    lengths = ([len(r) for r in est], [len(r) for r in clean])
    got = eabnet_amd.intelligibility(eview, sbuf[:, 2], lengths=lengths, sample_rate=10000)
    assert torch.equal(got, _batch(pick, dev)), "the load path changed the bits"


def test_other_rates_go_through_the_resampler(dev, cases, analysed):
    """16 kHz signals: the call equals resample-then-score bit for bit, and the restatement on those resampled signals"""
    import eabnet_amd
    pick = []
    for k in (4, 6):
        Ls, Le, seed, g_n, g_a, gaps = R.CASES[k]
        pick.append(R.make_case(Ls * 8 // 5, Le * 8 // 5, seed, g_n, g_a, tuple((a * 8 // 5, b * 8 // 5, g) for a, b, g in gaps)))
    clean, est = [c[0] for c in pick], [c[1] for c in pick]
    lengths = ([len(r) for r in est], [len(r) for r in clean])
    e16, s16 = _padded(est, dev), _padded(clean, dev)
    got = eabnet_amd.intelligibility(e16, s16, lengths=lengths, sample_rate=16000)
    e10 = eabnet_amd.resample(e16, 16000, 10000, lengths=lengths[0])
    s10 = eabnet_amd.resample(s16, 16000, 10000, lengths=lengths[1])
    l10 = tuple([eabnet_amd.resampled_length(v, 16000, 10000) for v in l] for l in lengths)
    assert torch.equal(got, eabnet_amd.intelligibility(e10, s10, lengths=l10, sample_rate=10000))
    dl = tuple(torch.tensor(l, device=dev) for l in lengths)
    assert torch.equal(got, eabnet_amd.intelligibility(e16, s16, lengths=dl, sample_rate=16000)), "device lengths differ"
    g = got.cpu().numpy()
    for b in range(2):
        want = R.intelligibility(e10[b, :l10[0][b]].cpu().numpy(), s10[b, :l10[1][b]].cpu().numpy())
        print(f"16 kHz case {b}: {g[b]} vs {want}: {np.abs(g[b] - want).max():.3e}")
        assert np.abs(g[b] - want).max() <= TOL_SCORE
        assert want.min() > 1e-3                                          # a real score, not the sentinel


# ------------------------------------------------------------------ the scorer
SAMPLES = [48000, 11200, 30123, 12999, 16007]           # 0.7 s .. 3 s


def _files(seed):
    noisy = [torch.from_numpy(paramgen.make_wave(1, 4, n, seed + k))[0] for k, n in enumerate(SAMPLES)]
    clean = [torch.from_numpy(paramgen.make_wave(1, 1, n, seed + 50 + k))[0, 0] for k, n in enumerate(SAMPLES)]
    return noisy, [0.7 * x[0] + 0.3 * c for x, c in zip(noisy, clean)]            # clean correlates with the noisy channels


def _single(dev, **kw):
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=4, p=1, q=1, **kw)
    net.load_state_dict(torch_params(4, 12, p=1, q=1, **kw), strict=True)
    return net.to(dev).eval()


@pytest.mark.parametrize("causal", [True, False])
def test_scorer_adds_two_columns_and_changes_nothing_else(dev, causal):
    import eabnet_amd
    net = _single(dev, is_causal=causal)
    noisy, clean = _files(300)
    base = eabnet_amd.Scorer(net, max_batch=4)(noisy, clean)
    scorer = eabnet_amd.Scorer(net, max_batch=4, intelligibility=True)
    scores, waves = scorer(noisy, clean, return_waves=True)
    assert list(scores) == ["si_sdr", "si_sir", "si_sar", "si_sdr_mix", "loss", "stoi", "estoi"]
    assert list(base) == ["si_sdr", "si_sir", "si_sar", "si_sdr_mix", "loss"]
    for m in base:
        assert np.array_equal(base[m], scores[m]), f"{m} changed with intelligibility=True"
    ref_waves = eabnet_amd.Enhancer(net, max_batch=4)(noisy)
    for k in range(5):
        assert torch.equal(waves[k], ref_waves[k]), f"file {k}: the scorer's wave is not the enhancer's"
    above = 0
    for k in range(5):
        by_hand = eabnet_amd.intelligibility(waves[k][None].to(dev), clean[k][None].to(dev), sample_rate=16000)[0].cpu().numpy()
        print(f"file {k}: stoi {scores['stoi'][k]:.6f} estoi {scores['estoi'][k]:.6f}")
        assert scores["stoi"][k] == by_hand[0] and scores["estoi"][k] == by_hand[1], (k, by_hand)
        above += scores["stoi"][k] > 1e-5
    assert above >= 1 and all(v.shape == (5,) and np.isfinite(v).all() for v in scores.values())


def test_stoi_wrapper_has_the_host_librarys_argument_order(dev, cases):
    import eabnet_amd
    clean, est = cases[4]
    pair = eabnet_amd.intelligibility(torch.from_numpy(est)[None].to(dev), torch.from_numpy(clean)[None].to(dev), sample_rate=10000)[0]
    assert eabnet_amd.stoi(clean, est, 10000) == float(pair[0])
    assert eabnet_amd.stoi(torch.from_numpy(clean).to(dev), torch.from_numpy(est), 10000, extended=True) == float(pair[1])
