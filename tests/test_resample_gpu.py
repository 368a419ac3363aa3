"""Resampling on the MI355X: the kernel of csrc/resample.hip against the float64 definition (tests/resample_ref.py), its bits
alone, in a batch, through a strided view, with a microphone order, in a stream and at large absolute positions, and the three
tools with ``sample_rate`` against the 16 kHz tools on individually resampled waves.

Value bound, per output sample: |y - ref| <= (2K + 2) 2^-24 ref_abs with ref_abs = sum |h| |x|: every tap is rounded to fp32
once (2^-24 relative) and each of the K accumulation steps rounds a partial sum that |h||x| bounds (2^-24 relative to at most
(1 + K 2^-24) ref_abs), fused or not: (1 + K)(1 + ...) 2^-24 ref_abs < (2K + 2) 2^-24 ref_abs.  Derived, not measured; the
largest err / bound seen is printed.  Every padded buffer is NaN past each row's length, so a read past a length shows."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import paramgen
import resample_ref as ref
from util import torch_params

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
PAIRS = [(48000, 16000), (44100, 16000), (22050, 16000), (16000, 48000), (32000, 16000), (16000, 44100)]
TILE = 1024                                   # outputs per workgroup of the kernel (4 per lane)
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _long(orig, new):
    """input samples that give three whole output tiles and a ragged rest"""
    o, n = ref.ratio(orig, new)
    return -(-(3 * TILE + 229) * o // n) + 3


_CASES = {}


def _case(orig, new, window="hann"):
    """(signals, references) of a rate pair, built once: five single rows and a 3 x 5 batch of three lengths"""
    key = (orig, new, window)
    if key not in _CASES:
        rng = np.random.default_rng(orig // 7 + new)
        singles = [rng.standard_normal(L).astype(np.float32) for L in (1, 20, 163, 1003, _long(orig, new))]
        lens = [1003, 20, _long(orig, new)]
        batch = [rng.standard_normal((5, L)).astype(np.float32) for L in lens]
        refs = [(ref.ref_resample(x, orig, new, window), ref.ref_abs(x, orig, new, window)) for x in singles + batch]
        _CASES[key] = (singles, batch, lens, refs)
    return _CASES[key]


def _padded(batch, dev, width=None):
    """(B, M, longest) device buffer, NaN past every utterance's length"""
    L = max(b.shape[1] for b in batch) if width is None else width
    buf = torch.full((len(batch), batch[0].shape[0], L), NAN, dtype=torch.float32)
    for k, b in enumerate(batch):
        buf[k, :, :b.shape[1]] = torch.from_numpy(b)
    return buf.to(dev)


def _ratio_to_bound(got, want, scale, K):
    bound = (2 * K + 2) * EPS * scale
    err = np.abs(got.astype(np.float64) - want)
    assert (err[bound == 0] == 0).all()
    assert (err <= bound).all(), f"err / bound up to {(err[bound > 0] / bound[bound > 0]).max():.3f}"
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _check_values(dev, orig, new, window):
    import eabnet_amd
    singles, batch, lens, refs = _case(orig, new, window)
    K = eabnet_amd.filter_bank(orig, new, window)[4]
    worst = 0.0
    for x, (want, scale) in zip(singles, refs):
        y = eabnet_amd.resample(torch.from_numpy(x).to(dev), orig, new, window=window)
        assert y.shape == (eabnet_amd.resampled_length(len(x), orig, new),) == want.shape
        worst = max(worst, _ratio_to_bound(y.cpu().numpy(), want, scale, K))
    buf = _padded(batch, dev)
    y = eabnet_amd.resample(buf, orig, new, lengths=lens, window=window)
    assert y.shape == (3, 5, eabnet_amd.resampled_length(buf.shape[2], orig, new))
    yh = y.cpu().numpy()
    for k, (want, scale) in enumerate(refs[len(singles):]):
        n_k = eabnet_amd.resampled_length(lens[k], orig, new)
        assert want.shape == (5, n_k)
        worst = max(worst, _ratio_to_bound(yh[k, :, :n_k], want, scale, K))
        assert (yh[k, :, n_k:] == 0).all(), "the padded tail is not zero"
    dl = eabnet_amd.resample(buf, orig, new, lengths=torch.tensor(lens, device=dev), window=window)
    assert torch.equal(dl, y), "host and device lengths disagree"
    print(f"{orig}->{new} {window}: K={K}, largest err / bound {worst:.3f}")
    return y


# ------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("orig,new", PAIRS)
def test_values_against_the_definition(dev, orig, new):
    _check_values(dev, orig, new, "hann")


@pytest.mark.parametrize("orig,new", PAIRS[:2])
def test_values_with_the_kaiser_window(dev, orig, new):
    _check_values(dev, orig, new, "kaiser")


# ------------------------------------------------------------------ 2. same bits in any company
@pytest.mark.parametrize("orig,new", PAIRS)
def test_same_bits_alone_in_a_batch_and_through_a_strided_view(dev, orig, new):
    import eabnet_amd
    _, batch, lens, _ = _case(orig, new)
    buf = _padded(batch, dev)
    y = eabnet_amd.resample(buf, orig, new, lengths=lens)
    for k, b in enumerate(batch):
        alone = eabnet_amd.resample(torch.from_numpy(b).to(dev), orig, new)
        assert torch.equal(alone, y[k, :, :alone.shape[1]]), f"utterance {k}: alone != in the batch"
    # one channel block of a wider buffer, rows at a pitch that is no multiple of four floats, base not 16-byte aligned
    W = buf.shape[2]
    wide = torch.full((3 * 9 * (W + 3) + 1,), NAN, device=dev)
    view = wide[1:].view(3, 9, W + 3)[:, 2:7, :W]
    view.copy_(buf)
    assert view.data_ptr() % 16 != 0 and view.stride() == (9 * (W + 3), W + 3, 1) and not view.is_contiguous()
    assert torch.equal(eabnet_amd.resample(view, orig, new, lengths=lens), y), "a strided view differs from its contiguous copy"


# ------------------------------------------------------------------ 3. mic_order
@pytest.mark.parametrize("orig,new", PAIRS[:2])
def test_mic_order_is_an_index_select(dev, orig, new):
    import eabnet_amd
    _, batch, lens, _ = _case(orig, new)
    buf = _padded(batch, dev)
    order = [4, 0, 0, 2]
    got = eabnet_amd.resample(buf, orig, new, lengths=lens, mic_order=order)
    assert got.shape[:2] == (3, 4)
    assert torch.equal(got, eabnet_amd.resample(buf[:, order], orig, new, lengths=lens))
    one = torch.from_numpy(batch[0]).to(dev)                                  # a single (M, L) file
    assert torch.equal(eabnet_amd.resample(one, orig, new, mic_order=order), eabnet_amd.resample(one[order], orig, new))


# ------------------------------------------------------------------ 4. streaming
@pytest.mark.parametrize("orig,new", PAIRS[:2])
def test_stream_is_bit_identical_to_the_offline_call(dev, orig, new):
    import eabnet_amd
    K = eabnet_amd.filter_bank(orig, new)[4]
    sizes = [1, 7, 500, 33, 1, 1, 2901, K - 1, 0, 260, 3]
    assert min(s for s in sizes if s > 1) < K
    total = sum(sizes)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 3, total)).astype(np.float32)).to(dev)
    off = eabnet_amd.resample(x, orig, new)
    rs = eabnet_amd.StreamResampler(orig, new)
    for rnd in range(2):                                                      # the second round after reset()
        a, pieces = 0, []
        for j, s in enumerate(sizes):
            pieces.append(rs.push(x[:, :, a:a + s], last=j == len(sizes) - 1))
            a += s
            assert pieces[-1].shape[:2] == (2, 3)
            assert rs.total_out == sum(p.shape[2] for p in pieces) <= eabnet_amd.resampled_length(a, orig, new)
        got = torch.cat(pieces, dim=2)
        assert got.shape[2] == eabnet_amd.resampled_length(total, orig, new) == off.shape[2]
        assert torch.equal(got, off), f"round {rnd}"
        assert any(p.shape[2] == 0 for p in pieces) and pieces[0].shape[2] == 0   # one sample makes no output final
        rs.reset()


# ------------------------------------------------------------------ 5. large positions
@pytest.mark.parametrize("orig,new", PAIRS[:2])
def test_large_absolute_positions(dev, orig, new):
    """origins of 2^33 periods: the same buffer, the same bits (a 32-bit index anywhere would show)"""
    import eabnet_amd
    from eabnet_amd import _lib
    rsm = importlib.import_module("eabnet_amd.resample")
    o, n = ref.ratio(orig, new)
    rows, cols = 3, _long(orig, new)
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((rows, cols)).astype(np.float32)).to(dev)
    n_out = eabnet_amd.resampled_length(cols, orig, new)
    tab, first, _, _, K = rsm._device_bank(orig, new, "hann", 6, 0.99, dev)[:5]

    def run(in_origin, out_origin, valid_hi):
        y = torch.full((rows, n_out), NAN, device=dev)
        _lib.check(_lib.load().eab_resample_f32(x.data_ptr(), cols, cols, None, None, rows, 1, y.data_ptr(), n_out, n_out,
                                                tab.data_ptr(), first.data_ptr(), o, n, K, in_origin, out_origin, valid_hi,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "eab_resample_f32")
        return y

    near = run(0, 0, cols)
    far = run(2 ** 33 * o, 2 ** 33 * n, 2 ** 33 * o + cols)
    assert torch.isfinite(near).all() and torch.equal(far, near)
    assert torch.equal(near, eabnet_amd.resample(x, orig, new))


# ------------------------------------------------------------------ 6. - 8. the tools
def _model(dev, M=2, **kw):
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=M, p=1, q=1, **kw)
    net.load_state_dict(torch_params(M, 21, p=1, q=1, **kw), strict=True)
    return net.to(dev).eval()


def _files(rate, dev, M=2, seed=700):
    """five files of 0.2 .. 0.7 s at `rate`, mixed lengths, host and device waves"""
    lens = [int(rate * s) + d for s, d in ((0.2, 13), (0.7, 0), (0.3, 11), (0.5, 7), (0.4, 1))]
    waves = [torch.from_numpy(paramgen.make_wave(1, M, L, seed + k))[0] for k, L in enumerate(lens)]
    return [w.to(dev) if k % 2 else w for k, w in enumerate(waves)]


def test_enhancer_at_48k(dev):
    import eabnet_amd
    net = _model(dev)
    waves = _files(48000, dev)
    at16 = [eabnet_amd.resample(w.to(dev), 48000, 16000) for w in waves]
    want = eabnet_amd.Enhancer(net, max_batch=4)(at16)
    enh = eabnet_amd.Enhancer(net, max_batch=4, sample_rate=48000)
    got = enh(waves)
    assert [len(b["indices"]) for b in enh.last_plan["batches"]] == [4, 1]
    for k in range(5):
        assert got[k].shape == want[k].shape == (160 * (at16[k].shape[1] // 160),)
        assert torch.equal(got[k], want[k]), f"file {k}"
    # the microphones in another order
    swapped = eabnet_amd.Enhancer(net, max_batch=4, sample_rate=48000, mic_order=[1, 0])(waves)
    want_swapped = eabnet_amd.Enhancer(net, max_batch=4)([w[[1, 0]] for w in at16])
    same_rate = eabnet_amd.Enhancer(net, max_batch=4, mic_order=[1, 0])(at16)
    for k in range(5):
        assert torch.equal(swapped[k], want_swapped[k]) and torch.equal(same_rate[k], want_swapped[k]), f"file {k}"
        assert not torch.equal(swapped[k], want[k])
    # back at the input rate
    back = eabnet_amd.Enhancer(net, max_batch=4, sample_rate=48000, output_rate="input")(waves)
    for k in range(5):
        assert torch.equal(back[k], eabnet_amd.resample(want[k], 16000, 48000)), f"file {k}"
        assert back[k].shape == (3 * want[k].shape[0],)
    # a selection may also fit a wider file to the model
    wide = [torch.cat((w, w[:1]), dim=0) for w in waves]
    assert all(torch.equal(a, b) for a, b in zip(eabnet_amd.Enhancer(net, max_batch=4, sample_rate=48000, mic_order=[0, 1])(wide), got))
    with pytest.raises(ValueError, match="microphones"):
        enh(wide)
    assert net.length_buckets is None


def test_scorer_at_44k1(dev):
    import eabnet_amd
    net = _model(dev)
    noisy = _files(44100, dev)
    clean = [0.6 * x[0] + 0.4 * torch.from_numpy(paramgen.make_wave(1, 1, x.shape[1], 760 + k))[0, 0].to(x.device)
             for k, x in enumerate(noisy)]
    got = eabnet_amd.Scorer(net, max_batch=4, sample_rate=44100)(noisy, clean)
    want = eabnet_amd.Scorer(net, max_batch=4)([eabnet_amd.resample(x.to(dev), 44100, 16000) for x in noisy],
                                               [eabnet_amd.resample(c.to(dev), 44100, 16000) for c in clean])
    assert set(got) == {"si_sdr", "si_sir", "si_sar", "si_sdr_mix", "loss"}
    for m in got:
        assert got[m].shape == (5,) and np.isfinite(got[m]).all()
        assert np.array_equal(got[m], want[m]), (m, got[m], want[m])


def test_streaming_enhancer_at_48k(dev):
    import eabnet_amd
    net = _model(dev, norm_type="BN")
    B, chunk, hops = 2, 2, 12
    wav = torch.from_numpy(paramgen.make_wave(B, 2, hops * 160 * 3, 790)).to(dev)
    at16 = eabnet_amd.resample(wav, 48000, 16000)
    assert at16.shape == (B, 2, hops * 160)
    win = torch.hann_window(320)
    with torch.no_grad():
        off = eabnet_amd.istft(net(eabnet_amd.stft_compress(at16, 320, 160, win)), 320, 160, win)
    enh = eabnet_amd.StreamingEnhancer(net, B=B, seconds=hops * 160 / 16000, chunk=chunk, sample_rate=48000)
    pieces = [enh.push(wav[:, :, a:a + 960], last=a + 960 >= wav.shape[2]) for a in range(0, wav.shape[2], 960)]
    got = torch.cat(pieces, dim=1)
    assert got.shape == off.shape == (B, hops * 160)
    assert torch.equal(got, off)
    plain = eabnet_amd.StreamingEnhancer(net, B=B, seconds=hops * 160 / 16000, chunk=chunk)
    fed = torch.cat([plain.push(at16[:, :, a:a + 320], last=a + 320 >= at16.shape[2]) for a in range(0, at16.shape[2], 320)], dim=1)
    assert torch.equal(got, fed)
    with pytest.raises(ValueError, match="960 samples"):
        enh.push(wav[:, :, :500])
