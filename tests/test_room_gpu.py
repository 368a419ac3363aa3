"""Room simulation on the MI355X: the three entry points of csrc/room.hip against the float64 definition (tests/room_ref.py),
their bits alone, in a batch and in a second call, and RoomSimulator feeding one training step.

Bar for every value check: max|got - ref| / max|ref| <= 1e-4 per response and per output channel (the project's parity bar);
the gains are held to it entry by entry.  The measured ratio is printed.  Every padded buffer is NaN past each utterance's
length and in the source rows it does not have, so a read past either shows.  Sizes: SEGMENT = 4096 samples of a response per
workgroup, PARTITION = 512, BLOCK = 4096 output samples per workgroup of the mixing kernel."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import room_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4
BLOCK = 4096
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _scene(Lr, order, S, M, seed, a=0.3, src0=None, mic0=None):
    from eabnet_amd import simulate as sim
    rng = np.random.default_rng(seed)
    Lr = np.asarray(Lr, dtype=np.float64)
    centre = Lr * rng.uniform(0.3, 0.7, 3) if mic0 is None else np.asarray(mic0, dtype=np.float64)
    mics = centre + rng.uniform(-0.05, 0.05, (M, 3))
    src = Lr * rng.uniform(0.05, 0.95, (S, 3))
    if src0 is not None:
        src[0] = src0
    return sim.Scene(room_dim=Lr, absorption=a, max_order=order, fs=16000, sources=src, mics=mics, ref_mic=M - 1,
                     snr=list(rng.uniform(-5.0, 10.0, S - 1)), dBFS=-22.0)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _batch_scenes():
    """three rooms, orders and source counts"""
    return _cached("batch", lambda: [_scene((3.0, 3.0, 2.5), 0, 1, 3, 11), _scene((4.0, 3.5, 2.6), 3, 2, 3, 12, a=0.2),
                                     _scene((6.0, 5.0, 3.0), 5, 3, 3, 13, a=0.45)])


def _href(key, sc):
    return _cached(("h", key), lambda: ref.scene_rirs(sc))


def _ratio(got, want, exact_zero=False):
    """max|got - ref| / max|ref|.  exact_zero: the definition's value is identically zero (the caller has seen that every
    response is exactly zero over the whole span), where the ratio has no meaning and the output must be zero itself."""
    if exact_zero:
        return 0.0 if np.all(got == 0) else float("inf")
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def _check_rirs(h, ks, scenes, keys):
    worst = 0.0
    for b, (sc, key) in enumerate(zip(scenes, keys)):
        want = _href(key, sc)
        S, M1, K = want.shape
        assert K == ks[b]
        got = h[b].cpu().numpy()
        for s in range(S):
            for m in range(M1):
                worst = max(worst, _ratio(got[s, m, :K], want[s, m]))
        assert np.all(got[:S, :, K:] == 0) and np.all(got[S:] == 0), "a response is not zero past its length or its sources"
    return worst


@pytest.mark.parametrize("order", [0, 1, 3, 8])
def test_responses_against_the_definition(dev, order):
    from eabnet_amd import simulate as sim
    sc = _cached(("one", order), lambda: _scene((5.0, 4.0, 2.7), order, 2, 3, 20 + order))
    h, ks = sim.image_source_rirs([sc], dev)
    assert h.shape == (1, 2, 4, sim.rir_length(sc.room_dim, order, 16000)) and h.dtype == torch.float32
    worst = _check_rirs(h, ks, [sc], [("one", order)])
    print(f"responses O = {order}: K = {ks[0]}, max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR


def test_responses_of_a_batch_of_three_rooms(dev):
    from eabnet_amd import simulate as sim
    scenes = _batch_scenes()
    h, ks = sim.image_source_rirs(scenes, dev)
    assert h.shape == (3, 3, 4, max(ks)) and len(set(ks)) == 3
    worst = _check_rirs(h, ks, scenes, ["b0", "b1", "b2"])
    print(f"responses of a batch (O = 0, 3, 5; S = 1, 2, 3): max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR


def test_responses_longer_than_one_segment(dev):
    """(40, 3, 2.5) m at O = 8: 833 images, K = 16874: five segments of SEGMENT = 4096 samples, and pulses that straddle their
    boundaries (the target's image n = (8, 0, 0) towards microphone 0 the one at 16,384)."""
    from eabnet_amd import simulate as sim
    sc = _cached("long", lambda: _scene((40.0, 3.0, 2.5), 8, 2, 3, 30, src0=(35.3, 1.2, 1.3), mic0=(5.0, 1.5, 1.2)))
    n, k0, _, _ = ref.image_pulses(sc.room_dim, sc.absorption, 8, 16000.0, sc.sources[0], sc.mics[0])
    assert len(n) == 833
    assert (k0 // sim.SEGMENT != (k0 + 80) // sim.SEGMENT).any(), "no pulse crosses a segment boundary"
    h, ks = sim.image_source_rirs([sc], dev)
    assert ks == [16874]
    worst = _check_rirs(h, ks, [sc], ["long"])
    print(f"responses across a segment boundary: max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR


def test_max_rir_seconds_cuts_the_responses(dev):
    from eabnet_amd import simulate as sim
    sc = _batch_scenes()[2]
    full, ks = sim.image_source_rirs([sc], dev)
    cut, kc = sim.image_source_rirs([sc], dev, max_rir_seconds=0.05)
    assert kc == [800] and ks[0] > 800 and torch.equal(cut, full[..., :800])


def _gain_case():
    def make():
        rng = np.random.default_rng(40)
        L = 3 * 1600 + 200                                             # a ragged last window of 200 samples
        xs = (0.1 * rng.standard_normal((3, 3, L))).astype(np.float32)
        xs[0, 1, 1600:3200] = 0.0                                      # a silent window
        xs[0, 1, 3200:4800] *= 1e-4                                    # and one below -50 dB of the peak
        xs[1, 2, 4800:] *= 30.0                                        # the peak in the ragged window
        xs[2, 2] = 0.0                                                 # an all-zero noise
        lens = [L, L - 57, L]
        scenes = [_scene((4.0, 3.5, 2.6), 1, 3, 2, 41 + b) for b in range(3)]
        want = [ref.dry_gains(list(xs[b, :, :lens[b]].astype(np.float64)), list(scenes[b].snr), scenes[b].dBFS, 16000.0) for b in range(3)]
        return xs, lens, scenes, want
    return _cached("gains", make)


def test_gains_against_the_definition(dev):
    from eabnet_amd import simulate as sim
    xs, lens, scenes, want = _gain_case()
    assert ref.active_rms(xs[0, 1].astype(np.float64) / np.abs(xs[0, 1]).max(), 16000.0) > \
        1.2 * float(np.sqrt(np.mean((xs[0, 1].astype(np.float64) / np.abs(xs[0, 1]).max()) ** 2))), "the silent windows do not count"
    buf = torch.from_numpy(xs.copy())
    for b, n in enumerate(lens):
        buf[b, :, n:] = NAN
    got = sim.mix_gains(buf.to(dev), scenes, lengths=lens)
    assert got.shape == (3, 3) and got.dtype == torch.float64
    got = got.cpu().numpy()
    assert np.all(np.isfinite(got))
    worst = max(float(np.abs(got[b] / want[b] - 1.0).max()) for b in range(3))
    print(f"gains: largest relative error {worst:.2e}; the all-zero noise's gain {got[2, 2]:.3e} (ref {want[2][2]:.3e})")
    assert worst <= BAR
    # two sources in a three-row table: the third row is never read, its gain is zero
    two = [copy.copy(scenes[0])]
    two[0].sources, two[0].snr = scenes[0].sources[:2], scenes[0].snr[:1]
    buf2 = buf[:1].clone()
    buf2[0, 2] = NAN
    g2 = sim.mix_gains(buf2.to(dev), two).cpu().numpy()
    w2 = ref.dry_gains(list(xs[0, :2].astype(np.float64)), list(two[0].snr), two[0].dBFS, 16000.0)
    assert g2[0, 2] == 0.0 and float(np.abs(g2[0, :2] / w2 - 1.0).max()) <= BAR


def _sources(S, L, seed):
    rng = np.random.default_rng(seed)
    x = (0.1 * rng.standard_normal((S, L))).astype(np.float32)
    x *= (1.0 + np.sin(np.arange(L) / 300.0)).astype(np.float32)       # (not stationary)
    return x


def _check_mix(noisy, clean, b, n, want, h):
    """h: the reference's responses; an utterance that ends before anything arrives (every h[..., :n] exactly zero) is zero"""
    nref, cref, _ = want
    silent = bool(np.all(h[..., :n] == 0))
    got_n, got_c = noisy[b].cpu().numpy(), clean[b, 0].cpu().numpy()
    assert np.all(got_n[:, n:] == 0) and np.all(got_c[n:] == 0), "the output is not zero past the utterance's length"
    ratios = [_ratio(got_n[m, :n], nref[m], silent) for m in range(nref.shape[0])] + [_ratio(got_c[:n], cref, silent)]
    return max(ratios)


@pytest.mark.parametrize("order", [0, 3])                             # K below one partition of 512, and above
@pytest.mark.parametrize("L", [1, 512, 513, 777, BLOCK, BLOCK + 1, 3 * BLOCK + 229])   # (512: one partition)
def test_mixtures_against_the_definition(dev, L, order):
    from eabnet_amd import simulate as sim
    sc = _cached(("mix", order), lambda: _scene((5.0, 4.0, 2.7), order, 3, 3, 50 + order))
    K = sim.rir_length(sc.room_dim, order, 16000)
    assert (K < sim.PARTITION) if order == 0 else (K > sim.PARTITION)
    x = _cached(("x", 3 * BLOCK + 229), lambda: _sources(3, 3 * BLOCK + 229, 60))[:, :L]
    want = _cached(("mixref", order, L), lambda: ref.simulate(sc, x.astype(np.float64), _href(("mix", order), sc)))
    noisy, clean = sim.simulate_rooms(torch.from_numpy(np.ascontiguousarray(x))[None].to(dev), [sc])
    assert noisy.shape == (1, 3, L) and clean.shape == (1, 1, L)
    worst = _check_mix(noisy, clean, 0, L, want, _href(("mix", order), sc))
    assert L > 1 or np.all(_href(("mix", order), sc)[..., :1] == 0)      # (one sample: nothing has arrived yet)
    print(f"mixture L = {L}, O = {order} (K = {K}): max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR


def _unequal_batch():
    def make():
        scenes = _batch_scenes()
        lens = [777, BLOCK + 1, 3 * BLOCK + 229]
        L = max(lens)
        xs = np.full((3, 3, L), NAN, dtype=np.float32)
        for b, (sc, n) in enumerate(zip(scenes, lens)):
            xs[b, :sc.n_sources, :n] = _sources(sc.n_sources, n, 70 + b)
        xs[2, 1, 2000:9000] = 0.0
        xs[2, 2, :lens[2]] = 0.0                                       # an all-zero noise: its gain of ~1e29 meets zero spectra
        want = [ref.simulate(sc, xs[b, :sc.n_sources, :n].astype(np.float64), _href(f"b{b}", sc))
                for b, (sc, n) in enumerate(zip(scenes, lens))]
        return scenes, lens, xs, want
    return _cached("unequal", make)


def test_unequal_lengths_in_one_batch_and_the_same_bits_alone(dev):
    from eabnet_amd import simulate as sim
    scenes, lens, xs, want = _unequal_batch()
    x = torch.from_numpy(xs).to(dev)
    noisy, clean = sim.simulate_rooms(x, scenes, lengths=lens)
    worst = max(_check_mix(noisy, clean, b, lens[b], want[b], _href(f"b{b}", scenes[b])) for b in range(3))
    print(f"mixtures of a batch with lengths {lens}: max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR
    # a second call: the same bits
    noisy2, clean2 = sim.simulate_rooms(x, scenes, lengths=lens)
    assert torch.equal(noisy.view(torch.int32), noisy2.view(torch.int32)) and torch.equal(clean.view(torch.int32), clean2.view(torch.int32))
    hb, kb = sim.image_source_rirs(scenes, dev)
    gb = sim.mix_gains(x, scenes, lengths=lens)
    for b, (sc, n) in enumerate(zip(scenes, lens)):
        S = sc.n_sources
        alone = x[b:b + 1, :S, :n].contiguous()
        n1, c1 = sim.simulate_rooms(alone, [sc])
        assert torch.equal(n1.view(torch.int32), noisy[b:b + 1, :, :n].view(torch.int32)), f"utterance {b}: noisy differs alone"
        assert torch.equal(c1.view(torch.int32), clean[b:b + 1, :, :n].view(torch.int32)), f"utterance {b}: clean differs alone"
        h1, k1 = sim.image_source_rirs([sc], dev)
        assert k1 == [kb[b]] and torch.equal(h1[0].view(torch.int32), hb[b, :S, :, :k1[0]].view(torch.int32))
        g1 = sim.mix_gains(alone, [sc])
        assert torch.equal(g1[0].view(torch.int64), gb[b, :S].view(torch.int64))


def test_room_simulator_feeds_a_training_step(dev):
    """RoomSimulator on its side stream -> prepare_data -> EaBNet forward, loss, backward: device tensors all the way"""
    import eabnet_amd
    from eabnet_amd import simulate as sim
    with open(os.path.join(ROOT, "tests", "golden", "mcse_dataset_settings_v3.json")) as f:
        settings = json.load(f)
    settings["room"]["rt60"] = [0.08, 0.15]                            # (small orders: the test stays quick)
    simu = eabnet_amd.RoomSimulator(settings, max_batch=2, seed=3, rir_method="ism")
    scenes = simu.sample(2)
    B, L = 2, 8000
    gen = torch.Generator(device="cpu").manual_seed(5)
    sources = (0.1 * torch.randn(B, simu.n_sources, L, generator=gen)).to(dev)
    for b, sc in enumerate(scenes):
        sources[b, sc.n_sources:] = NAN
    noisy, clean = simu.simulate(sources, scenes)
    simu.wait()
    assert noisy.device == dev and clean.device == dev and noisy.shape == (B, 8, L) and clean.shape == (B, 1, L)
    n2, c2 = eabnet_amd.simulate_rooms(sources, scenes)
    assert torch.equal(noisy, n2) and torch.equal(clean, c2)
    assert bool(torch.isfinite(noisy).all()) and bool(torch.isfinite(clean).all())
    # the mixture sits at its dBFS
    for b, sc in enumerate(scenes):
        want = ref.dry_gains(list(sources[b, :sc.n_sources].cpu().numpy().astype(np.float64)), list(sc.snr), sc.dBFS, 16000.0)
        got = eabnet_amd.mix_gains(sources[b:b + 1], [sc]).cpu().numpy()[0, :sc.n_sources]
        assert float(np.abs(got / want - 1.0).max()) <= BAR
    args = type("A", (), dict(mics=8, sr=16000, wav_len=L / 16000, win_size=0.020, win_shift=0.010, fft_num=320))
    net = eabnet_amd.EaBNet(M=8, p=1, q=1).to(dev).train()
    spec, target = eabnet_amd.prepare_data(noisy, clean, dev, args)
    est = net(spec)
    assert est.requires_grad and net.training_backend == "hip"
    loss = eabnet_amd.com_mag_mse_loss(est, target, [spec.shape[1]] * B)
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    # the next batch goes to the other output slot: the first one's tensors are untouched
    keep = noisy.clone()
    n3, _ = simu.simulate(sources * 0.5, scenes)
    simu.wait()
    assert n3.data_ptr() != noisy.data_ptr() and torch.equal(noisy, keep)
