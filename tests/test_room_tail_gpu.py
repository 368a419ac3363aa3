"""The response model "ism_tail" on the MI355X: eab_room_rirs_tail_f32 against the float64 restatement
(tests/room_tail_ref.py), mixtures through simulate_rooms against tests/room_ref.py's mixing with those responses, their bits
alone, in a batch and in a second call, the padding, and RoomSimulator on the shipped settings.

Bar for every value check: max|got - ref| / max|ref| <= 1e-4 per response and per output channel (4.18's bar).  The measured
ratio is printed.  SEGMENT = 4096 samples of a response per workgroup."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import room_ref as ref
import room_tail_ref as tref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _scene(Lr, rt60, S, M, seed, **tail):
    """a room by its rt60 (absorption and order by Sabine), S sources, M microphones within 5 cm per axis of a centre"""
    from eabnet_amd import simulate as sim
    rng = np.random.default_rng(seed)
    Lr = np.asarray(Lr, dtype=np.float64)
    a, order = ref.inverse_sabine(rt60, list(Lr))
    centre = Lr * rng.uniform(0.3, 0.7, 3)
    mics = centre + rng.uniform(-0.05, 0.05, (M, 3))
    src = Lr * rng.uniform(0.05, 0.95, (S, 3))
    kw = dict(tail_start=0.02, tail_density=2.0, tail_seed=int(rng.integers(0, 1 << 53)))
    kw.update(tail)
    return sim.Scene(room_dim=Lr, absorption=a, max_order=order, fs=16000, sources=src, mics=mics, ref_mic=M - 1,
                     snr=list(rng.uniform(-5.0, 10.0, S - 1)), dBFS=-22.0, rir_method="ism_tail", **kw)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _small(density=2.0, **kw):
    """(4, 3.5, 2.6) m at rt60 0.25 s: O = 32, K = 6241, two segments"""
    return _cached(("small", density, tuple(sorted(kw.items()))), lambda: _scene((4.0, 3.5, 2.6), 0.25, 2, 3, 101, tail_density=density, **kw))


def _batch_scenes():
    """three rooms: K = 6241, 2466 and 4751 (two segments, one, two), S = 2, 1 and 3"""
    return _cached("batch", lambda: [_small(), _scene((3.0, 3.0, 2.5), 0.12, 1, 3, 102), _scene((5.0, 4.0, 2.7), 0.15, 3, 3, 103, tail_density=1.3)])


def _href(key, sc, cut=None):
    return _cached(("h", key, cut), lambda: tref.scene_rirs(sc, cut=cut))


def _ratio(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def _tail_windows(got, want, sc, W=512):
    """The bar above is held by the direct path, 30 to 80 dB above the late tail, so the tail is also held window by window:
    in every W samples from the first that carry the tail at full density (k_mix + 81) on,
        max|got - ref| <= 1e-4 max|ref over the window| + 2^-41 81 (nu + 1).
    The first term is the bar applied to the window; the second is what the accumulation may add on its own: a sample
    receives about 81 nu taps of the tail (and a few of the early part), each rounded to within 2^-41 when it becomes an
    integer of 2^-40.  Returns the largest share of that bound any window uses (0 without a tail)."""
    _, _, J, nu = tref.tail_counts(sc)
    if J == 0:
        return 0.0
    first = int(sc.tail_start * float(sc.fs)) + tref.TAPS
    share = 0.0
    for k in range(first, want.shape[-1], W):
        err = np.abs(got[..., k:k + W].astype(np.float64) - want[..., k:k + W]).max(-1)
        share = max(share, float((err / (1e-4 * np.abs(want[..., k:k + W]).max(-1) + 2.0 ** -41 * 81 * (nu + 1))).max()))
    return share


def _check_rirs(h, ks, scenes, keys, cut=None):
    worst = 0.0
    for b, (sc, key) in enumerate(zip(scenes, keys)):
        want = _href(key, sc, cut)
        S, M1, K = want.shape
        assert K == ks[b]
        got = h[b].cpu().numpy()
        assert np.all(np.isfinite(got))
        for s in range(S):
            for m in range(M1):
                worst = max(worst, _ratio(got[s, m, :K], want[s, m]))
        frac = _tail_windows(got[:S, :M1 - 1, :K], want[:, :M1 - 1], sc)
        print(f"scene {b}: the tail's windows use {frac:.3f} of their bound")
        assert frac <= 1.0, f"scene {b}: a window of the tail is off by {frac:.2f} of its bound"
        assert np.all(got[:S, :, K:] == 0) and np.all(got[S:] == 0), "a response is not zero past its length or its sources"
    return worst


@pytest.mark.parametrize("density", [0.05, 2.0, 0.0])
def test_responses_against_the_restatement(dev, density):
    """two segments of 4096 samples; at 0.05 images per sample the pulses stand apart (about one in 20 samples against 81
    taps: pairs overlap, no crowd hides a wrong one), at 0 the early part is alone"""
    from eabnet_amd import simulate as sim
    sc = _small(density)
    K = sim.rir_length(sc.room_dim, sc.max_order, 16000)
    assert (sc.max_order, K) == (32, 6241)
    k0 = tref.tail_pulses(sc, 0, sc.mics[0])[0]
    if density > 0:
        assert ((k0 < sim.SEGMENT) & (k0 + 80 >= sim.SEGMENT)).any(), "no tail pulse crosses the segment boundary"
        assert len(k0) == int(np.ceil(density * (K - 81 - 320)))
    else:
        assert len(k0) == 0
    n_early = len(tref.early_pulses(sc, 0, sc.mics[0])[0])
    assert 0 < n_early < len(ref.images(sc.room_dim, 32, sc.sources[0])[0])
    h, ks = sim.image_source_rirs([sc], dev)
    assert h.shape == (1, 2, 4, K) and h.dtype == torch.float32 and ks == [K]
    worst = _check_rirs(h, ks, [sc], [("small", density)])
    print(f"responses at {density} images per sample ({n_early} early images, {len(k0)} in the tail): "
          f"max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR
    if density == 0:                                                   # nothing after the early part's last pulse
        last = max(int(tref.early_pulses(sc, s, sc.mics[m])[1].max()) for s in range(2) for m in range(3))
        assert bool((h[0, :, :3, last + 81:] == 0).all()) and last + 81 < K


def test_responses_at_the_default_settings_over_four_segments(dev):
    """(6, 5, 3) m at rt60 0.4 s, the first room of the model's validation, tail_start 0.05 s and 2 images per sample as
    RoomSimulator hands them out: O = 45, K = 12,958, the early sphere of 17 m and 24,154 virtual images per source"""
    from eabnet_amd import simulate as sim
    sc = _cached("default", lambda: _scene((6.0, 5.0, 3.0), 0.4, 1, 2, 106, tail_start=0.05))
    assert (sc.max_order, sim.rir_length(sc.room_dim, 45, 16000), tref.tail_counts(sc)[2]) == (45, 12958, 24154)
    h, ks = sim.image_source_rirs([sc], dev)
    worst = _check_rirs(h, ks, [sc], ["default"])
    n_early = len(tref.early_pulses(sc, 0, sc.mics[0])[0])
    print(f"responses at the defaults (K = {ks[0]}, {n_early} early images): max|got - ref| / max|ref| = {worst:.2e}")
    assert n_early > 100 and worst <= BAR


def test_a_tail_that_starts_after_the_response_leaves_the_whole_image_set(dev):
    """tail_start past K - 81: n_slots <= 0, no tail, and r_mix beyond the farthest image: the response is that of "ism" """
    from eabnet_amd import simulate as sim
    sc = _cached("late", lambda: _scene((4.0, 3.5, 2.6), 0.25, 1, 2, 104, tail_start=(6241 - 81) / 16000.0 + 0.002))
    assert tref.tail_counts(sc)[1] <= 0 and tref.tail_counts(sc)[2] == 0
    h, ks = sim.image_source_rirs([sc], dev)
    worst = _check_rirs(h, ks, [sc], ["late"])
    plain = copy.copy(sc)
    plain.rir_method = "ism"
    assert np.abs(_href("late", sc) - _cached("late-ism", lambda: ref.scene_rirs(plain))).max() == 0.0
    print(f"responses without a tail (n_slots = {tref.tail_counts(sc)[1]}): max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR


def test_pulses_cut_at_the_end_of_the_response(dev):
    """the last virtual images reach the centre at K - 81, a microphone 0.3 m off it up to 14 samples later: their pulses are
    cut at K; and max_rir_seconds cuts through the middle of the tail, where the response is the head of the uncut one"""
    from eabnet_amd import simulate as sim

    def make():
        sc = copy.copy(_small())
        sc.mics = tref.centre(sc)[None, :] + np.array([[-0.3, 0.0, 0.0], [0.3, 0.0, 0.0]])
        sc.ref_mic = 1
        return sc
    sc = _cached("wide", make)
    K = 6241
    sim.check_scene(sc)
    k0 = np.concatenate([tref.tail_pulses(sc, s, sc.mics[m])[0] for s in range(2) for m in range(2)])
    assert ((k0 < K) & (k0 + 75 >= K)).sum() >= 5, "too few pulses of the tail lose taps at the end"
    full, ks = sim.image_source_rirs([sc], dev)
    worst = _check_rirs(full, ks, [sc], ["wide"])
    print(f"responses with pulses cut at K = {K}: max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR
    cut, kc = sim.image_source_rirs([sc], dev, max_rir_seconds=0.2)
    assert kc == [3200] and torch.equal(cut.view(torch.int32), full[..., :3200].contiguous().view(torch.int32))
    k0 = tref.tail_pulses(sc, 0, sc.mics[0])[0]
    assert ((k0 < 3200) & (k0 + 80 >= 3200)).any() and (k0 >= 3200).any()
    worst = _check_rirs(cut, kc, [sc], ["wide"], cut=3200)
    print(f"responses cut at 3200 of {K} samples: max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR


def test_responses_of_a_batch_of_three_rooms(dev):
    """different K and S in one launch (the microphones' number is the batch's: 4.18); scene 1 has one source in a table of three
    rows, and every scene's rows are zero past its own K"""
    from eabnet_amd import simulate as sim
    scenes = _batch_scenes()
    h, ks = sim.image_source_rirs(scenes, dev)
    assert h.shape == (3, 3, 4, max(ks)) and len(set(ks)) == 3 and [sc.n_sources for sc in scenes] == [2, 1, 3]
    worst = _check_rirs(h, ks, scenes, [("small", 2.0), "b1", "b2"])
    print(f"responses of a batch (K = {ks}, S = 2, 1, 3): max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR


def test_one_microphone_is_its_own_centre(dev):
    from eabnet_amd import simulate as sim
    sc = _cached("mono", lambda: _scene((5.0, 4.0, 2.7), 0.15, 2, 1, 105))
    assert np.array_equal(tref.centre(sc), sc.mics[0])
    t, pos, _, _, _ = tref.tail_images(sc, 1)
    assert np.abs(np.linalg.norm(pos - sc.mics[0], axis=1) - 343.0 * t).max() < 1e-9      # d = c t_j: every image arrives at t_j
    h, ks = sim.image_source_rirs([sc], dev)
    assert h.shape[2] == 2
    worst = _check_rirs(h, ks, [sc], ["mono"])
    print(f"responses at M = 1: max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR


def _sources(S, L, seed):
    rng = np.random.default_rng(seed)
    x = (0.1 * rng.standard_normal((S, L))).astype(np.float32)
    x *= (1.0 + np.sin(np.arange(L) / 300.0)).astype(np.float32)       # (not stationary)
    return x


def _unequal_batch():
    def make():
        scenes = _batch_scenes()
        lens = [777, 4097, 9000]
        L = max(lens)
        xs = np.full((3, 3, L), NAN, dtype=np.float32)                 # NaN in the rows a scene does not have and past its length
        for b, (sc, n) in enumerate(zip(scenes, lens)):
            xs[b, :sc.n_sources, :n] = _sources(sc.n_sources, n, 170 + b)
        keys = [("small", 2.0), "b1", "b2"]
        want = [ref.simulate(sc, xs[b, :sc.n_sources, :n].astype(np.float64), h=_href(key, sc))
                for b, (sc, n, key) in enumerate(zip(scenes, lens, keys))]
        return scenes, lens, xs, want
    return _cached("unequal", make)


def _mix_ratio(noisy, clean, b, n, want):
    nref, cref, _ = want
    got_n, got_c = noisy[b].cpu().numpy(), clean[b, 0].cpu().numpy()
    return max([_ratio(got_n[m, :n], nref[m]) for m in range(nref.shape[0])] + [_ratio(got_c[:n], cref)])


def test_mixtures_of_unequal_lengths_against_the_definition(dev):
    from eabnet_amd import simulate as sim
    scenes, lens, xs, want = _unequal_batch()
    noisy, clean = sim.simulate_rooms(torch.from_numpy(xs).to(dev), scenes, lengths=lens)
    assert noisy.shape == (3, 3, 9000) and clean.shape == (3, 1, 9000)
    worst = max(_mix_ratio(noisy, clean, b, lens[b], want[b]) for b in range(3))
    print(f"mixtures of a batch with lengths {lens}: max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR


def test_padding_is_never_read_and_the_output_is_zero_past_each_length(dev):
    """the rows s >= S_b and the samples from lens[b] on hold NaN: one read of them would show in the sums"""
    from eabnet_amd import simulate as sim
    scenes, lens, xs, _ = _unequal_batch()
    assert np.isnan(xs[1, 1:]).all() and np.isnan(xs[0, 2]).all() and np.isnan(xs[0, :, 777:]).all()
    noisy, clean = sim.simulate_rooms(torch.from_numpy(xs).to(dev), scenes, lengths=lens)
    assert bool(torch.isfinite(noisy).all()) and bool(torch.isfinite(clean).all())
    for b, n in enumerate(lens):
        assert bool((noisy[b, :, n:] == 0).all()) and bool((clean[b, :, n:] == 0).all()), f"utterance {b} is not zero from {n} on"
        first = sim.first_arrival(scenes[b])
        assert bool((noisy[b, :, :first] == 0).all()) and bool(noisy[b, :, :n].abs().max() > 0)
    h, ks = sim.image_source_rirs(scenes, dev, sources=4)              # a table with a row no scene has
    assert h.shape[1] == 4 and bool((h[:, 3] == 0).all()) and bool((h[1, 1:] == 0).all())


def test_the_same_bits_alone_in_a_batch_and_in_a_second_call(dev):
    from eabnet_amd import simulate as sim
    scenes, lens, xs, _ = _unequal_batch()
    x = torch.from_numpy(xs).to(dev)
    noisy, clean = sim.simulate_rooms(x, scenes, lengths=lens)
    noisy2, clean2 = sim.simulate_rooms(x, scenes, lengths=lens)
    assert torch.equal(noisy.view(torch.int32), noisy2.view(torch.int32)) and torch.equal(clean.view(torch.int32), clean2.view(torch.int32))
    hb, kb = sim.image_source_rirs(scenes, dev)
    hb2, _ = sim.image_source_rirs(scenes, dev)
    assert torch.equal(hb.view(torch.int32), hb2.view(torch.int32))
    for b, (sc, n) in enumerate(zip(scenes, lens)):
        S = sc.n_sources
        n1, c1 = sim.simulate_rooms(x[b:b + 1, :S, :n].contiguous(), [sc])
        assert torch.equal(n1.view(torch.int32), noisy[b:b + 1, :, :n].contiguous().view(torch.int32)), f"utterance {b}: noisy differs alone"
        assert torch.equal(c1.view(torch.int32), clean[b:b + 1, :, :n].contiguous().view(torch.int32)), f"utterance {b}: clean differs alone"
        h1, k1 = sim.image_source_rirs([sc], dev)
        assert k1 == [kb[b]] and torch.equal(h1[0].view(torch.int32), hb[b, :S, :, :k1[0]].contiguous().view(torch.int32))


def test_room_simulator_on_the_shipped_settings(dev):
    """RoomSimulator(settings, rir_method="ism_tail") on the settings file as shipped (it asks for "hybrid"): scenes, mixtures
    on the side stream, the same bits as simulate_rooms, and the reference microphone's channel and the clean target of the
    first utterance against the restatement"""
    import eabnet_amd
    from eabnet_amd import simulate as sim
    with open(os.path.join(ROOT, "tests", "golden", "mcse_dataset_settings_v3.json")) as f:
        settings = json.load(f)
    assert settings["audio"]["rir_method"] == "hybrid"
    simu = eabnet_amd.RoomSimulator(settings, max_batch=2, seed=3, rir_method="ism_tail")
    scenes = simu.sample(2)
    assert all(sc.rir_method == "ism_tail" and (sc.tail_start, sc.tail_density) == (0.05, 2.0) for sc in scenes)
    B, L = 2, 8000
    gen = torch.Generator(device="cpu").manual_seed(6)
    sources = (0.1 * torch.randn(B, simu.n_sources, L, generator=gen)).to(dev)
    for b, sc in enumerate(scenes):
        sources[b, sc.n_sources:] = NAN
    noisy, clean = simu.simulate(sources, scenes)
    simu.wait()
    assert noisy.device == dev and noisy.shape == (B, 8, L) and clean.shape == (B, 1, L)
    assert bool(torch.isfinite(noisy).all()) and bool(torch.isfinite(clean).all())
    n2, c2 = eabnet_amd.simulate_rooms(sources, scenes)
    assert torch.equal(noisy, n2) and torch.equal(clean, c2)
    # one channel against the restatement: the responses of every source to the reference microphone, cut at the utterance
    sc = scenes[0]
    S = sc.n_sources
    K = sim.rir_length(sc.room_dim, sc.max_order, 16000)
    assert K < L and sc.max_order == 28 and S == 6
    h = np.zeros((S, 2, K))
    for s in range(S):                                                 # (the centre and the images are those of the eight microphones)
        h[s, 0] = tref.rir(sc, s, sc.ref_mic, K)
        h[s, 1] = ref.rir(sc.room_dim, 1.0, 0, 16000.0, sc.sources[s], sc.mics[sc.ref_mic], K)
    one = copy.copy(sc)                                                # the mixing of room_ref with that one microphone
    one.mics, one.ref_mic = sc.mics[sc.ref_mic:sc.ref_mic + 1], 0
    nref, cref, _ = ref.simulate(one, sources[0, :S].cpu().numpy().astype(np.float64), h=h)
    worst = max(_ratio(noisy[0, sc.ref_mic].cpu().numpy(), nref[0]), _ratio(clean[0, 0].cpu().numpy(), cref))
    print(f"RoomSimulator, shipped settings (O = {sc.max_order}, K = {K}, S = {S}): max|got - ref| / max|ref| = {worst:.2e}")
    assert worst <= BAR
