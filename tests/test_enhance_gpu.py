"""Waves in, waves out on the MI355X: per-utterance lengths in the STFT and ISTFT kernels against one-at-a-time calls, and
``eabnet_amd.Enhancer`` against the one-at-a-time chain stft_compress -> model -> istft.  Small shapes (M 4, B <= 4, L <= 3 s)."""
import argparse

import pytest
import torch

import paramgen
from util import TOL_HIP, assert_compressed_close, torch_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------ front end
# L_cap 4000: rows aligned for the four-sample gather (interior frames of every utterance take it, the per-utterance calls
# with L_b % 4 != 0 take the scalar one); 4002: every frame on the scalar path.  Lengths: the cap itself, odd, a multiple of
# the hop, L_b % 4 != 0, and the shortest admissible one.
@pytest.mark.parametrize("layout,M", [(0, 4), (1, 1)])
@pytest.mark.parametrize("L_cap,lens", [(4000, [4000, 3203, 3200, 1762]), (4002, [4002, 3999, 161, 2880])])
def test_stft_lengths_equal_the_per_utterance_calls(dev, layout, M, L_cap, lens):
    import eabnet_amd
    win = torch.hann_window(320)
    wav = torch.from_numpy(paramgen.make_wave(len(lens), M, L_cap, 70 + M)).to(dev)
    for b, n in enumerate(lens):
        wav[b, :, n:] = float("nan")                      # the padding is never read
    got = eabnet_amd.stft_compress(wav, 320, 160, win, layout, lengths=lens)
    dev_lens = eabnet_amd.stft_compress(wav, 320, 160, win, layout, lengths=torch.tensor(lens, device=dev))
    assert torch.equal(got, dev_lens), "host and device lengths disagree"
    tax = 1 if layout == 0 else 2
    assert got.shape[tax] == 1 + L_cap // 160
    for b, n in enumerate(lens):
        ref = eabnet_amd.stft_compress(wav[b:b + 1, :, :n], 320, 160, win, layout)
        Tb = 1 + n // 160
        assert ref.shape[tax] == Tb
        assert torch.equal(got[b:b + 1].narrow(tax, 0, Tb), ref), f"utterance {b} (L = {n}): valid frames differ"
        rest = got[b].narrow(tax - 1, Tb, got.shape[tax] - Tb)
        assert torch.equal(rest, torch.zeros_like(rest)), f"utterance {b} (L = {n}): frames past the length are not zero"


def test_stft_lengths_on_the_dft_fallback(dev):
    """n_fft = 84: 42 = 2 * 3 * 7 has no radix-{5, 4, 2} plan, so stft_dft_kernel runs"""
    import eabnet_amd
    n_fft, hop, L_cap, lens = 84, 42, 1000, [1000, 43, 517, 840]
    win = torch.hann_window(n_fft)
    wav = torch.from_numpy(paramgen.make_wave(4, 3, L_cap, 77)).to(dev)
    got = eabnet_amd.stft_compress(wav, n_fft, hop, win, lengths=lens)
    for b, n in enumerate(lens):
        ref = eabnet_amd.stft_compress(wav[b:b + 1, :, :n], n_fft, hop, win)
        Tb = 1 + n // hop
        assert torch.equal(got[b:b + 1, :Tb], ref), f"utterance {b} (L = {n})"
        assert torch.equal(got[b, Tb:], torch.zeros_like(got[b, Tb:]))


def test_stft_lengths_vs_torch_stft(dev):
    """one short utterance of a padded batch against torch.stft on the CPU (centre, reflect) with the reference's
    sqrt-magnitude compression"""
    import eabnet_amd
    L_cap, n = 4000, 3203
    wav = torch.from_numpy(paramgen.make_wave(2, 4, L_cap, 78))
    got = eabnet_amd.stft_compress(wav.to(dev), 320, 160, torch.hann_window(320), lengths=[L_cap, n])[1].cpu()
    X = torch.stft(wav[1, :, :n], 320, 160, 320, torch.hann_window(320), center=True, pad_mode="reflect", return_complex=True)
    X = torch.view_as_real(X).permute(2, 1, 0, 3)                                   # (M, F, T, 2) -> (T, F, M, 2)
    mag = torch.linalg.vector_norm(X, dim=-1, keepdim=True)
    want = torch.where(mag > 0, X / mag.clamp_min(1e-30).sqrt(), torch.zeros_like(X))
    Tb = 1 + n // 160
    assert_compressed_close(got[:Tb].numpy(), want.numpy(), TOL_HIP, "stft lengths")
    assert torch.count_nonzero(got[Tb:]) == 0


# ------------------------------------------------------------------ back end
@pytest.mark.parametrize("n_fft,hop", [(320, 160), (320, 100)])
def test_istft_lengths_equal_the_per_utterance_calls(dev, n_fft, hop):
    """T_cap = 37 frames are several workgroups per utterance; the utterance of 2 frames leaves most of them without a frame"""
    import eabnet_amd
    torch.manual_seed(n_fft + hop)
    T_cap, lens = 37, [37, 20, 2, 9]
    win = torch.hann_window(n_fft)
    esti = torch.randn(len(lens), 2, T_cap, n_fft // 2 + 1).to(dev)
    poisoned = esti.clone()
    for b, n in enumerate(lens):
        poisoned[b, :, n:] = float("nan")                 # padding frames must not reach a valid sample (nor the zeros)
    got = eabnet_amd.istft(poisoned, n_fft, hop, win, lengths=lens)
    assert got.shape == (len(lens), hop * (T_cap - 1))
    assert torch.equal(got, eabnet_amd.istft(poisoned, n_fft, hop, win, lengths=torch.tensor(lens, device=dev)))
    for b, n in enumerate(lens):
        ref = eabnet_amd.istft(esti[b:b + 1, :, :n], n_fft, hop, win)
        assert torch.equal(got[b:b + 1, :hop * (n - 1)], ref), f"utterance {b} ({n} frames): valid samples differ"
        rest = got[b, hop * (n - 1):]
        assert torch.equal(rest, torch.zeros_like(rest)), f"utterance {b} ({n} frames): samples past the length are not zero"


# ------------------------------------------------------------------ the enhancer
SAMPLES = [48000, 16000, 30123, 9999, 41000, 16007, 22222]      # 301, 101, 189, 63, 257, 101, 139 frames


def _waves(seed=21, M=4, samples=SAMPLES):
    return [torch.from_numpy(paramgen.make_wave(1, M, n, seed + k))[0] for k, n in enumerate(samples)]


def _net(dev, seed=3, **kw):
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=4, **kw)
    net.load_state_dict(torch_params(4, seed, **kw), strict=True)
    return net.to(dev).eval()


def _chain(model, waves, dev):
    """the one-at-a-time loop on the exact-shape path"""
    import eabnet_amd
    win = torch.hann_window(320)
    out = []
    with torch.no_grad():
        for w in waves:
            y = model(eabnet_amd.stft_compress(w[None].to(dev), 320, 160, win))
            y = y["esti_stft"] if isinstance(y, dict) else y
            out.append(eabnet_amd.istft(y, 320, 160, win)[0])
    return out


def _compare(got, refs, tol, what):
    assert len(got) == len(refs)
    for k, (y, ref) in enumerate(zip(got, refs)):
        assert y.shape == ref.shape == (160 * (SAMPLES[k] // 160),), f"{what} file {k}: {tuple(y.shape)}"
        if tol == 0.0:
            assert torch.equal(y, ref), f"{what} file {k}: max diff {float((y - ref).abs().max()):.3e}"
        else:
            err = float((y - ref).abs().max() / ref.abs().max())
            print(f"{what} file {k}: {err:.3e} of the reference wave's range")
            assert err <= tol, f"{what} file {k}: {err:.3e} > {tol:.1e}"


@pytest.mark.parametrize("norm", ["BN", "cLN"])
def test_enhancer_equals_the_one_at_a_time_chain_bit_for_bit(dev, norm, monkeypatch):
    """no statistic over time and the kernel choice pinned (as tests/test_varlen_gpu.py pins it): every wave of the padded
    batches, dummies in the partial group included, is the wave of the one-at-a-time chain; host and device waves agree"""
    import eabnet_amd
    monkeypatch.setenv("EAB_ST", "0")
    monkeypatch.setenv("EAB_BM", "64")
    net = _net(dev, seed=5, norm_type=norm)
    waves = _waves()
    refs = _chain(net, waves, dev)
    enh = eabnet_amd.Enhancer(net, max_batch=4)
    got = enh([w.to(dev) for w in waves])
    plan = enh.last_plan
    assert [(len(b["indices"]), b["cap"], b["batch_size"], b["dummies"]) for b in plan["batches"]] == [(4, 512, 4, 0), (3, 128, 4, 1)]
    assert plan["batches"][0]["indices"] == [0, 4, 2, 6] and plan["batches"][1]["indices"] == [1, 5, 3] and plan["dummies"] == 1
    _compare(got, refs, 0.0, norm)
    assert net.length_buckets is None, "the enhancer must restore the model's length_buckets"
    host = enh(waves)
    mixed = enh([w.to(dev) if k % 2 else w for k, w in enumerate(waves)])
    for k in range(len(waves)):
        assert torch.equal(host[k], got[k]) and torch.equal(mixed[k], got[k]), f"host / device waves differ at file {k}"


def test_enhancer_default_model_one_lowering_per_cap_and_batch_size(dev, monkeypatch):
    """InstanceNorm: the padded program merges its partials in another tile set (1e-5 of the wave's range, the bound of the
    varlen tests).  Each (cap, batch size) is lowered once; other files that plan to the same pairs lower nothing."""
    import eabnet_amd
    from eabnet_amd import program as prg
    net = _net(dev)
    waves = _waves(seed=31)
    refs = _chain(net, waves, dev)
    calls = []
    real = prg.lower
    monkeypatch.setattr(prg, "lower", lambda *a, **k: calls.append((a[3], a[2])) or real(*a, **k))
    enh = eabnet_amd.Enhancer(net, max_batch=4)
    got = enh([w.to(dev) for w in waves])
    assert sorted(calls) == [(128, 4), (512, 4)], f"lower() calls (cap, batch size): {calls}"
    _compare(got, refs, 1e-5, "IN")
    other = _waves(seed=41, samples=[47000, 15000, 31000, 12000, 42000, 17000])   # 4 + 2 files: the same two programs
    enh([w.to(dev) for w in other])
    assert [(b["cap"], b["batch_size"], b["dummies"]) for b in enh.last_plan["batches"]] == [(512, 4, 0), (128, 4, 2)]
    assert len(calls) == 2, f"a second folder lowered again: {calls}"
    assert sorted(k[:2] for k in net.varlen_arena_bytes()) == [(4, 128), (4, 512)]


def test_enhancer_cuts_the_batch_size_to_the_arena_budget(dev):
    """a (cap, batch size) above max_resident_bytes is not built: its files run at the next smaller batch size"""
    import eabnet_amd
    net = _net(dev, seed=6)
    waves = [w.to(dev) for w in _waves(seed=51)]
    enh = eabnet_amd.Enhancer(net, max_batch=4)
    enh(waves[:4])
    (key, nbytes), = net.varlen_arena_bytes().items()
    assert key[:2] == (4, 512)
    for m in (net._varlen_bound, net._varlen_version):
        m.clear()
    net.max_resident_bytes = nbytes - 1                   # B = 4 at cap 512 no longer fits; B = 1 does
    got = enh(waves[:4])                                  # 301, 101, 189, 63 frames, each alone in its own cap
    assert [(b["indices"], b["cap"], b["batch_size"]) for b in enh.last_plan["batches"]] == \
        [([0], 512, 1), ([2], 256, 1), ([1], 128, 1), ([3], 64, 1)]
    assert all(k[0] == 1 and v <= net.max_resident_bytes for k, v in net.varlen_arena_bytes().items())
    assert all(y.shape == (160 * (n // 160),) for y, n in zip(got, SAMPLES))


def _two_stage_args(causal=True):
    return argparse.Namespace(
        k1=(2, 3), k2=(1, 3), c=64, M=4, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=1, q=1, is_causal=causal, is_u2=True,
        bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="IN", ref_mic=0, freeze_eabnet=False,
        gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=1,
        gagnet_q=2, gagnet_dilas=[1, 2], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=causal,
        gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="IN")


def test_enhancer_two_stage_model(dev):
    import eabnet_amd
    torch.manual_seed(0)
    net = eabnet_amd.make_eabnet_with_postnet(_two_stage_args()).to(dev).eval()
    with torch.no_grad():
        for p in net.parameters():                       # off the default initialisation, deterministic
            p.add_(0.02 * torch.randn_like(p))
    waves = _waves(seed=61)
    refs = _chain(net, waves, dev)
    got = eabnet_amd.Enhancer(net, max_batch=4)(waves)
    _compare(got, refs, 1e-5, "two-stage")
    assert net.length_buckets is None and net.postnet.length_buckets is None


def test_enhancer_non_causal_model_runs_one_file_at_a_time(dev):
    import eabnet_amd
    net = _net(dev, seed=8, is_causal=False)
    waves = _waves(seed=71, samples=SAMPLES[:3])
    refs = _chain(net, waves, dev)
    enh = eabnet_amd.Enhancer(net, max_batch=4)
    got = enh(waves)
    assert [(b["cap"], b["batch_size"]) for b in enh.last_plan["batches"]] == [(None, 1)] * 3 and not net._varlen_bound
    for k in range(3):
        assert torch.equal(got[k], refs[k]), f"file {k}"
