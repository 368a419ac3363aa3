"""The response model "ism_tail"  without a GPU: the float64 restatement (tests/room_tail_ref.py) against
hand-computed values and its own rules, eabnet_amd.simulate's new fields and refusals, and the model itself against the exact
image-source response it stands for (tests/room_ref.py)."""
import copy
import json
import math
import os

import numpy as np
import pytest

import room_ref as ref
import room_tail_ref as tref
from eabnet_amd import simulate as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _settings():
    with open(os.path.join(ROOT, "tests", "golden", "mcse_dataset_settings_v3.json")) as f:
        return json.load(f)


def _scene(**kw):
    base = dict(room_dim=(4.0, 3.0, 2.5), absorption=0.3, max_order=14, fs=16000, sources=np.array([[1.0, 1.0, 1.2], [3.0, 2.0, 1.4]]),
                mics=np.array([[2.0, 1.5, 1.1], [2.05, 1.5, 1.1]]), ref_mic=0, snr=[5.0], dBFS=-25.0, rir_method="ism_tail",
                tail_start=0.02, tail_density=2.0, tail_seed=1234567)
    base.update(kw)
    return sim.Scene(**base)


def test_generator_on_hand_computed_words():
    """tail_seed = 0, s = 0, d = 0: the counters j = 0, 1, 2 give GOLDEN, 2 GOLDEN, 3 GOLDEN, whose mix is the published
    SplitMix64 sequence of seed 0; a second counter with every field set, worked out with Python's integers"""
    assert [int(w) for w in tref.words(0, 0, 0, [0, 1, 2])] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    mask = (1 << 64) - 1
    z = (12345 + tref.GOLDEN * (1 + (((4 * 3 + 2) << 32) | 77))) & mask
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & mask
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & mask
    z ^= z >> 31
    assert z == 0xD6F22EE06E3C1044 and int(tref.words(12345, 3, 2, [77])[0]) == z
    U = tref.uniforms(12345, 3, [77])
    assert U.shape == (4, 1) and U[2, 0] == (z >> 11) * 2.0 ** -53 and np.all((U >= 0) & (U < 1))
    # the largest seed, the last source, the last uniform: no overflow into another field
    assert int(tref.words((1 << 53) - 1, 7, 3, [(1 << 28) - 1])[0]) != int(tref.words((1 << 53) - 1, 7, 3, [0])[0])


def test_tail_counts_arrival_times_and_positions():
    sc = _scene()
    K = sim.rir_length(sc.room_dim, sc.max_order, sc.fs)
    k_mix, n_slots, J, nu = tref.tail_counts(sc)
    assert k_mix == 320 and n_slots == K - 81 - 320 and J == 2 * n_slots and nu == 2.0
    odd = _scene(tail_density=0.3, tail_start=0.0201)
    k_mix, n_slots, J, nu = tref.tail_counts(odd)
    assert k_mix == 321 and J == math.ceil(0.3 * n_slots) and nu == J / n_slots and 0.3 <= nu < 0.3 + 1.0 / n_slots
    for case in (sc, odd):
        t, pos, u, walls, sign = tref.tail_images(case, 1)
        J = tref.tail_counts(case)[2]
        assert len(t) == J and np.all(np.diff(t) > 0), "t_j rises with j"
        assert t[0] >= case.tail_start and t[-1] < case.tail_start + tref.tail_counts(case)[1] / 16000.0 * (1 + 1e-12)
        far = np.linalg.norm(pos - tref.centre(case), axis=1)
        assert np.all(far >= 343.0 * case.tail_start * (1 - 1e-12)), "a virtual image lies inside r_mix"
        assert np.abs(far - 343.0 * t).max() < 1e-9 and np.abs(np.linalg.norm(u, axis=1) - 1.0).max() < 1e-12
        assert set(sign) == {-1.0, 1.0} and abs(sign.mean()) < 4.0 / math.sqrt(J)
        assert abs(u.mean(0)).max() < 4.0 / math.sqrt(J)                # directions uniform on the sphere: mean 0, variance 1/3 per axis
        assert np.all(walls >= 343.0 * t / max(case.room_dim) * (1 - 1e-12))
    # the images of two sources differ, those of one source do not depend on the microphone
    assert not np.array_equal(tref.tail_images(sc, 0)[0], tref.tail_images(sc, 1)[0])
    assert np.array_equal(tref.centre(sc), np.array([2.025, 1.5, 1.1]))


def test_one_tail_pulse_by_hand():
    """image j = 5 of source 1, every factor of rule 2 spelled out with math.*"""
    sc = _scene(tail_density=0.05)
    k_mix, n_slots, J, nu = tref.tail_counts(sc)
    U = tref.uniforms(sc.tail_seed, 1, [5])[:, 0]
    t = 0.02 + (5 + U[0]) / (nu * 16000.0)
    z, phi = 2.0 * U[1] - 1.0, 2.0 * math.pi * U[2]
    u = np.array([math.sqrt(1 - z * z) * math.cos(phi), math.sqrt(1 - z * z) * math.sin(phi), z])
    p = np.array([2.025, 1.5, 1.1]) + 343.0 * t * u
    d = float(np.linalg.norm(p - sc.mics[1]))
    walls = 343.0 * t * (abs(u[0]) / 4.0 + abs(u[1]) / 3.0 + abs(u[2]) / 2.5)
    g = (-1.0 if U[3] < 0.5 else 1.0) * math.sqrt(4 * math.pi * 343.0 ** 3 * t * t / (30.0 * 16000.0 * nu)) * 0.7 ** (0.5 * walls) / (4 * math.pi * d)
    k0, f, gg = tref.tail_pulses(sc, 1, sc.mics[1])
    assert k0[5] == int(d * 16000.0 / 343.0) and abs(f[5] - (d * 16000.0 / 343.0 - k0[5])) < 1e-9 and abs(gg[5] / g - 1.0) < 1e-12
    # the level: g^2 nu is the energy per sample of the exact model's pulse train, c / (4 pi V fs) at no absorption
    assert abs(g * g * nu / (343.0 / (4 * math.pi * 30.0 * 16000.0) * 0.7 ** walls) * (d / (343.0 * t)) ** 2 - 1.0) < 1e-12


def test_no_tail_at_density_zero_and_in_a_dead_room():
    sc = _scene()
    K = sim.rir_length(sc.room_dim, sc.max_order, sc.fs)
    early = tref.rir(sc, 0, 1, tail=False)
    n, k0, _, _ = tref.early_pulses(sc, 0, sc.mics[1])
    all_n = ref.images(sc.room_dim, sc.max_order, sc.sources[0])[0]
    assert 0 < len(n) < len(all_n) and np.abs(early).max() > 0
    # the early set is the same for both microphones, and holds the direct image
    assert np.array_equal(n, tref.early_pulses(sc, 0, sc.mics[0])[0]) and (np.abs(n).sum(1) == 0).any()
    for quiet in (_scene(tail_density=0.0), _scene(absorption=1.0), _scene(tail_start=(K - 81) / 16000.0 + 1e-9)):
        assert tref.tail_counts(quiet)[2] == 0 and len(tref.tail_pulses(quiet, 0, quiet.mics[1])[0]) == 0
    assert np.array_equal(tref.rir(_scene(tail_density=0.0), 0, 1), early)
    dead = tref.rir(_scene(absorption=1.0), 0, 1)                      # the direct image alone
    assert np.array_equal(dead, ref.rir(sc.room_dim, 1.0, 0, 16000.0, sc.sources[0], sc.mics[1], K))
    full = tref.rir(sc, 0, 1)
    assert full.shape == (K,) and np.array_equal(full[:200], early[:200]) and not np.array_equal(full, early)
    # a cut response is the head of the whole one: the tail's images are those of the scene's own length
    assert np.array_equal(tref.rir(sc, 0, 1, cut=1500), full[:1500])
    h = tref.scene_rirs(sc)
    assert h.shape == (2, 3, K) and np.array_equal(h[0, 1], full)
    assert np.array_equal(h[1, 2], ref.rir(sc.room_dim, 1.0, 0, 16000.0, sc.sources[1], sc.mics[0], K))


def test_refusals_and_what_stays_as_it_was():
    import torch
    sim.check_scene(_scene())
    bad = {
        "tail too close": _scene(tail_start=(1.0 + 0.024) / 343.0),    # r_mix = 1.024 m, the array's radius is 0.025 m
        "negative density": _scene(tail_density=-0.5),
        "density nan": _scene(tail_density=float("nan")),
        "density inf": _scene(tail_density=float("inf")),
        "density 65": _scene(tail_density=65.0),
        "seed 2^53": _scene(tail_seed=1 << 53),
        "seed -1": _scene(tail_seed=-1),
        "seed 1.5": _scene(tail_seed=1.5),
        "hybrid": _scene(rir_method="hybrid"),
    }
    for name, sc in bad.items():
        with pytest.raises(ValueError):
            sim.check_scene(sc)
        with pytest.raises(ValueError):                                # before the device is asked for
            sim.image_source_rirs([sc], "cpu")
        with pytest.raises(ValueError):
            sim.simulate_rooms(torch.zeros(1, 2, 100), [sc])
    sim.check_scene(_scene(tail_start=(1.0 + 0.026) / 343.0))
    sim.check_scene(_scene(tail_density=64.0, tail_seed=(1 << 53) - 1))
    sim.check_scene(_scene(rir_method="ism", tail_density=-1.0))       # "ism" does not look at the tail's fields
    with pytest.raises(ValueError, match="rir_method"):                # two methods in one batch
        sim.image_source_rirs([_scene(), _scene(rir_method="ism")], "cpu")
    from eabnet_amd import _lib
    with pytest.raises(_lib.EabError, match="no CPU fallback"):        # a valid call without the GPU
        sim.image_source_rirs([_scene()], "cpu")
    with pytest.raises(ValueError, match="hybrid"):
        sim.RoomSimulator(_settings())                                 # the shipped settings still ask for "hybrid"
    with pytest.raises(ValueError):
        sim.RoomSimulator(_settings(), rir_method="ism_tail", tail_density=100.0)
    simu = sim.RoomSimulator(_settings(), rir_method="ism_tail", tail_start=0.04, tail_density=1.5, seed=9)
    scenes = simu.sample(3)
    assert all(sc.rir_method == "ism_tail" and sc.tail_start == 0.04 and sc.tail_density == 1.5 for sc in scenes)
    assert len({sc.tail_seed for sc in scenes}) == 3
    for sc in scenes:
        sim.check_scene(sc)


def test_sample_scene_draws_the_seed_last_and_only_for_the_tail():
    st = _settings()
    for seed in range(20):
        r_ism, r_tail = np.random.default_rng(seed), np.random.default_rng(seed)
        a = sim.sample_scene(st, r_ism, rir_method="ism")
        b = sim.sample_scene(st, r_tail, rir_method="ism_tail")
        for name in ("room_dim", "sources", "mics"):
            assert np.array_equal(getattr(a, name), getattr(b, name))
        assert (a.absorption, a.max_order, a.rt60, a.dBFS, list(a.snr)) == (b.absorption, b.max_order, b.rt60, b.dBFS, list(b.snr))
        assert a.tail_seed == 0 and 0 <= b.tail_seed < 1 << 53
        assert b.tail_seed == int(r_ism.integers(0, 1 << 53)), "the seed is not the draw after the scene's last"
        assert r_ism.random() == r_tail.random()
        assert (b.tail_start, b.tail_density) == (0.05, 2.0)
        sim.check_scene(b)
    # the "ism" scene of seed 7, as recorded before the tail's draw existed
    a = sim.sample_scene(st, np.random.default_rng(7), rir_method="ism")
    assert (a.rt60, a.dBFS, a.max_order) == (0.44815074277746997, -34.121159840772336, 53)
    assert np.abs(np.asarray(a.room_dim) - np.array([7.37566827, 9.28049661, 2.88784285])).max() < 1e-8


def test_scene_record_and_entry_point():
    import ctypes as C
    from eabnet_amd import _lib
    sc = _scene()
    K = sim.rir_length(sc.room_dim, sc.max_order, sc.fs)
    r = sim._scene_record(sc)
    assert list(r[136:144]) == [1234567.0, 0.02, 2.0, float(K), float(K), 0.0, 0.0, 0.0]
    assert sim._scene_record(sc, 800)[140] == 800.0 and sim._scene_record(sc, 800)[139] == float(K)
    plain = copy.copy(sc)
    plain.rir_method = "ism"
    assert np.array_equal(r[:136], sim._scene_record(plain)[:136]) and not sim._scene_record(plain)[136:].any()
    # the first arrival: never later than the tail's nearest image can be
    near = _scene(tail_start=1.1 / 343.0)                              # the tail from 1.1 m on, the sources 1.12 m and more away
    assert sim.first_arrival(near) == int((1.1 - 0.025) * 16000 / 343.0) - 1 == 49 and sim.first_arrival(plain) == 50
    assert sim.first_arrival(sc) == sim.first_arrival(plain)           # (here the sources are nearer than the tail)
    lib = _lib.load()
    one = C.c_void_p(16)                                               # (never dereferenced: the shapes are refused first)
    assert lib.eab_room_rirs_tail_f32(None, 1, 1, 1, 100, 16000.0, None, None) == 1
    assert lib.eab_room_rirs_tail_f32(one, 1, 9, 1, 100, 16000.0, one, None) == 1     # S > 8
    assert lib.eab_room_rirs_tail_f32(one, 1, 1, 33, 100, 16000.0, one, None) == 1    # M > 32
    assert lib.eab_room_rirs_tail_f32(one, 1, 1, 1, 0, 16000.0, one, None) == 1
    assert lib.eab_abi_version() == 10


# the two rooms the model was derived on; the worst deviation measured over the five seeds below was 1.10 dB in the first and
# 1.90 dB in the second (DESIGN.md 4.23 has every window).  The bar is that worst case plus 1 dB for the scatter from window
# to window at about 1,300 pulses per window; a tail at the Eyring rate misses by 6 to 18 dB over the same windows.
VALIDATION_BAR_DB = 2.9
VALIDATION_SEEDS = [17 + 1000003 * k for k in range(5)]


@pytest.mark.parametrize("Lr, rt60, src, ctr", [((6.0, 5.0, 3.0), 0.4, (1.7, 3.4, 1.6), (3.9, 2.1, 1.3)),
                                                ((10.0, 10.0, 3.0), 0.6, (2.3, 7.1, 1.7), (6.2, 4.4, 1.2))])
def test_the_tail_carries_the_energy_of_the_exact_response(Lr, rt60, src, ctr):
    """energy in 40 ms windows from tail_start + 10 ms to O min(Lr) / (sqrt(3) c), where the order-O image set is still
    complete, against the exact response minus its 161-sample moving average (the slow drift the model leaves out)"""
    assert VALIDATION_BAR_DB <= 4.0
    a, order = ref.inverse_sabine(rt60, list(Lr))
    mics = np.array(ctr)[None, :] + np.array([[-0.025, 0.0, 0.0], [0.025, 0.0, 0.0]])
    sc = sim.Scene(room_dim=Lr, absorption=a, max_order=order, fs=16000, sources=np.array([src]), mics=mics, rir_method="ism_tail")
    sim.check_scene(sc)
    K = ref.rir_length(list(Lr), order, 16000.0)
    exact = ref.rir(Lr, a, order, 16000.0, np.array(src), mics[0], K)
    exact = exact - np.convolve(exact, np.ones(161) / 161.0, mode="same")
    W = 640
    lo, hi = int((sc.tail_start + 0.01) * 16000), int(order * min(Lr) / (math.sqrt(3.0) * 343.0) * 16000)
    starts = list(range(lo, hi - W + 1, W))
    assert len(starts) >= 4
    worst = 0.0
    for seed in VALIDATION_SEEDS:
        sc.tail_seed = seed
        h = tref.rir(sc, 0, 0, K)
        dev = [10.0 * math.log10(float((h[k:k + W] ** 2).sum() / (exact[k:k + W] ** 2).sum())) for k in starts]
        print(f"room {Lr}, seed {seed}: dB per window " + " ".join(f"{d:+.2f}" for d in dev))
        worst = max(worst, max(abs(d) for d in dev))
    print(f"room {Lr}: worst deviation {worst:.2f} dB over {len(VALIDATION_SEEDS)} seeds and {len(starts)} windows")
    assert worst <= VALIDATION_BAR_DB
