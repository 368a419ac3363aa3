"""The room simulation's host side without a GPU: the float64 reference (tests/room_ref.py) against hand-computed values and
mirror geometry, eabnet_amd.simulate's inverse_sabine / rir_length / sample_scene / refusals, and the C entry points' argument
checks."""
import copy
import json
import math
import os

import numpy as np
import pytest

import room_ref as ref
from eabnet_amd import simulate as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _settings():
    with open(os.path.join(ROOT, "tests", "golden", "mcse_dataset_settings_v3.json")) as f:
        return json.load(f)


def _scene(**kw):
    base = dict(room_dim=(4.0, 3.0, 2.5), absorption=0.3, max_order=2, fs=16000, sources=np.array([[1.0, 1.0, 1.2], [3.0, 2.0, 1.4]]),
                mics=np.array([[2.0, 1.5, 1.1], [2.05, 1.5, 1.1]]), ref_mic=0, snr=[5.0], dBFS=-25.0)
    base.update(kw)
    return sim.Scene(**base)


@pytest.mark.parametrize("fn", [sim.inverse_sabine, ref.inverse_sabine])
def test_inverse_sabine_on_hand_computed_values(fn):
    # V = 22.5, A = 48: a = 24 ln10 22.5 / (343 48 0.3) = 1243.40 / 4939.2;  O = ceil(343 0.3 / 2.5 - 1) = ceil(40.16)
    a, order = fn(0.3, (3.0, 3.0, 2.5))
    assert abs(a - 0.252) < 5e-4 and order == 41
    # V = 300, A = 320: a = 16578.6 / 76832;  O = ceil(343 0.7 / 3 - 1) = ceil(79.03)
    a, order = fn(0.7, (10.0, 10.0, 3.0))
    assert abs(a - 0.216) < 5e-4 and order == 80
    with pytest.raises(ValueError):
        fn(0.05, (10.0, 10.0, 3.0))                                    # a = 3.02 > 1


def test_rir_length_bounds_every_image_and_is_tight_at_a_vertex():
    rng = np.random.default_rng(5)
    for _ in range(20):
        Lr = rng.uniform(2.0, 10.0, 3)
        order = int(rng.integers(0, 7))
        src, mic = Lr * rng.random(3), Lr * rng.random(3)
        _, k0, _, _ = ref.image_pulses(Lr, 0.2, order, 16000.0, src, mic)
        K = sim.rir_length(Lr, order, 16000)
        assert K == ref.rir_length(list(Lr), order, 16000.0)
        assert k0.max() + ref.TAPS <= K
    # the source in one corner, the microphone in the opposite one: the image n = (O, 0, 0) of an even O lies (O + 1) Lx away
    Lr, order = (5.0, 3.0, 2.5), 4
    _, k0, _, _ = ref.image_pulses(Lr, 0.2, order, 16000.0, Lr, (0.0, 0.0, 0.0))
    assert k0.max() + ref.TAPS == sim.rir_length(Lr, order, 16000)


def test_order_zero_is_one_pulse_at_the_right_delay():
    # fs = 34300, d = 1 m: tau = 100 exactly, so the pulse is g at 100 + 40 and sinc's zeros elsewhere
    h = ref.rir((4.0, 3.0, 2.5), 0.3, 0, 34300.0, (1.0, 1.0, 1.0), (2.0, 1.0, 1.0), 400)
    assert abs(h[140] - 1.0 / (4.0 * math.pi)) < 1e-15
    h[140] = 0.0
    assert np.abs(h).max() < 1e-16
    # a fractional delay: the 81 taps by the formula, nothing outside them
    src, mic, fs = np.array([1.0, 1.0, 1.0]), np.array([2.3, 1.7, 1.4]), 16000.0
    diff = mic - src
    d = math.sqrt(diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2])
    tau = d * fs / 343.0
    k0, f = int(tau), tau - int(tau)
    h = ref.rir((4.0, 3.0, 2.5), 0.3, 0, fs, src, mic, 400)
    want = np.zeros(400)
    for i in range(81):
        x = i - 40 - f
        want[k0 + i] = 1.0 / (4.0 * math.pi * d) * (0.5 - 0.5 * math.cos(2.0 * math.pi * i / 80.0)) * math.sin(math.pi * x) / (math.pi * x)
    assert np.abs(h - want).max() < 1e-15                              # (taps <= 0.05; the sines' arguments round at 1e-14)
    assert int(np.abs(h).argmax()) in (k0 + 40, k0 + 41)


def test_order_one_each_of_the_seven_images_against_mirror_geometry():
    Lr, a, fs = np.array([4.0, 3.0, 2.5]), 0.36, 16000.0
    src, mic = np.array([1.1, 0.7, 1.9]), np.array([2.9, 2.2, 0.6])
    n, pos = ref.images(Lr, 1, src)
    assert len(n) == 7
    _, k0, f, g = ref.image_pulses(Lr, a, 1, fs, src, mic)
    total = np.zeros(600)
    seen = set()
    for k in range(7):
        want = src.copy()
        walls = 0
        for ax in range(3):
            if n[k, ax] == 1:
                want[ax] = 2.0 * Lr[ax] - src[ax]                     # mirrored in the wall at L
                walls += 1
            elif n[k, ax] == -1:
                want[ax] = -src[ax]                                    # mirrored in the wall at 0
                walls += 1
        assert walls == (0 if not n[k].any() else 1)
        seen.add(tuple(n[k]))
        assert np.abs(pos[k] - want).max() < 1e-12
        d = float(np.linalg.norm(want - mic))
        assert abs(g[k] - math.sqrt(1.0 - a) ** walls / (4.0 * math.pi * d)) < 1e-15
        assert k0[k] == int(d * fs / 343.0) and abs(f[k] - (d * fs / 343.0 - k0[k])) < 1e-9
        one = ref.add_pulses(np.zeros(600), k0[k:k + 1], f[k:k + 1], g[k:k + 1])
        peak = int(np.abs(one).argmax())
        assert peak in (k0[k] + 40, k0[k] + 41) and np.all(one[:k0[k]] == 0) and np.all(one[k0[k] + 81:] == 0)
        total += one
    assert len(seen) == 7
    assert np.abs(total - ref.rir(Lr, a, 1, fs, src, mic, 600)).max() < 1e-15


def test_sample_scene_honours_every_constraint_of_the_settings():
    st = _settings()
    arr, tgt, noi, room = st["mic_array"], st["target"], st["noise"], st["room"]
    counts = set()
    for seed in range(200):
        sc = sim.sample_scene(st, np.random.default_rng(seed), clean_name=f"c{seed}", rir_method="ism")
        Lr = np.asarray(sc.room_dim)
        assert np.all(Lr >= room["min_dim"]) and np.all(Lr <= room["max_dim"])
        target, centre = sc.sources[0], sc.meta["array_centre"]
        for p, rule in ((target, tgt), (centre, arr)):
            d = rule["min_dist_to_wall"]
            assert d <= p[0] <= Lr[0] - d and d <= p[1] <= Lr[1] - d and rule["h"][0] <= p[2] <= rule["h"][1]
        dist = np.linalg.norm(target - centre)
        assert tgt["dist_to_mic_array"][0] <= dist <= tgt["dist_to_mic_array"][1]
        # the array: congruent to the settings', level, centred, its direction (microphone 5 -> microphone 0) at the target
        flat = np.array([[m["x"], m["y"]] for m in arr["mics"]])
        assert sc.mics.shape == (8, 3) and np.abs(sc.mics[:, 2] - centre[2]).max() < 1e-12
        assert np.abs(sc.mics[:, :2].mean(0) - centre[:2]).max() < 1e-12
        want = np.linalg.norm(flat[:, None] - flat[None], axis=-1)
        assert np.abs(np.linalg.norm(sc.mics[:, None, :2] - sc.mics[None, :, :2], axis=-1) - want).max() < 1e-12
        axis = (sc.mics[0, :2] - sc.mics[5, :2]) / 0.09
        to_target = (target[:2] - centre[:2]) / np.linalg.norm(target[:2] - centre[:2])
        assert np.abs(axis - to_target).max() < 1e-9
        # orientation kept (a rotation, not a reflection): microphone 0 is to the left of the direction
        off = sc.mics[0, :2] - centre[:2]
        assert to_target[0] * off[1] - to_target[1] * off[0] > 0
        n = sc.n_sources - 1
        counts.add(n)
        assert noi["n"][0] <= n <= noi["n"][1] and len(sc.snr) == n
        for p, snr in zip(sc.sources[1:], sc.snr):
            assert 0 <= p[0] <= Lr[0] and 0 <= p[1] <= Lr[1] and noi["h"][0] <= p[2] <= noi["h"][1]
            assert np.linalg.norm(p - centre) >= noi["min_dist_to_mic_array"]
            v1, v2 = target - centre, p - centre
            ang = math.degrees(math.acos(np.dot(v1, v2) / (np.linalg.norm(v1) * np.linalg.norm(v2))))
            assert ang >= noi["min_doa_diff_wrt_target"]
            assert noi["SNR"][0] <= snr <= noi["SNR"][1]
        assert room["rt60"][0] <= sc.rt60 <= room["rt60"][1]
        assert (sc.absorption, sc.max_order) == ref.inverse_sabine(sc.rt60, list(Lr)) and sc.absorption <= 1.0
        assert st["noisy_dBFS"][0] <= sc.dBFS <= st["noisy_dBFS"][1]
        assert sc.fs == 16000 and sc.ref_mic == 0 and sc.clean_name == f"c{seed}" and sc.rir_method == "ism"
        sim.check_scene(sc)
    assert counts == {3, 4, 5}
    assert sim.sample_scene(st, np.random.default_rng(0)).rir_method == "hybrid"      # the settings' own method is kept
    a = sim.sample_scene(st, np.random.default_rng(7), rir_method="ism")
    b = sim.sample_scene(st, np.random.default_rng(7), rir_method="ism")
    assert np.array_equal(a.sources, b.sources) and np.array_equal(a.mics, b.mics) and a.rt60 == b.rt60


def test_refusals_happen_on_the_host():
    import torch
    from eabnet_amd import _lib
    sim.check_scene(_scene())
    bad = {
        "source outside": _scene(sources=np.array([[1.0, 1.0, 1.2], [4.5, 2.0, 1.4]])),
        "source below": _scene(sources=np.array([[1.0, -0.1, 1.2], [3.0, 2.0, 1.4]])),
        "microphone outside": _scene(mics=np.array([[2.0, 1.5, 1.1], [2.0, 1.5, 2.6]])),
        "too close": _scene(sources=np.array([[2.0, 1.55, 1.15], [3.0, 2.0, 1.4]])),
        "absorption": _scene(absorption=1.2),
        "nine sources": _scene(sources=np.tile(np.array([[1.0, 1.0, 1.2]]), (9, 1)), snr=[0.0] * 8),
        "33 microphones": _scene(mics=np.tile(np.array([[2.0, 1.5, 1.1]]), (33, 1))),
        "hybrid": _scene(rir_method="hybrid"),
    }
    for name, sc in bad.items():
        with pytest.raises(ValueError):
            sim.check_scene(sc)
        with pytest.raises(ValueError):                                # before the device is asked for
            sim.image_source_rirs([sc], "cpu")
        with pytest.raises(ValueError):
            sim.simulate_rooms(torch.zeros(1, sc.n_sources, 100), [sc])
        with pytest.raises(ValueError):
            sim.mix_gains(torch.zeros(1, sc.n_sources, 100), [sc])
    with pytest.raises(ValueError, match="hybrid"):
        sim.RoomSimulator(_settings())                                 # the shipped settings ask for "hybrid"
    assert sim.RoomSimulator(_settings(), rir_method="ism").n_sources == 6
    many = copy.deepcopy(_settings())
    many["noise"]["n"] = [3, 8]
    with pytest.raises(ValueError, match="S = 9"):
        sim.RoomSimulator(many, rir_method="ism")
    with pytest.raises(ValueError):                                    # fewer rows than the scene has sources
        sim.simulate_rooms(torch.zeros(1, 1, 100), [_scene()])
    with pytest.raises(ValueError):                                    # mixed sample rates
        sim.image_source_rirs([_scene(), _scene(fs=8000)], "cpu")
    # a valid call without the GPU: no fallback
    with pytest.raises(_lib.EabError, match="no CPU fallback"):
        sim.simulate_rooms(torch.zeros(1, 2, 100), [_scene()])
    with pytest.raises(_lib.EabError, match="no CPU fallback"):
        sim.image_source_rirs([_scene()], "cpu")


def test_entry_points_check_their_arguments_before_any_launch():
    import ctypes as C
    from eabnet_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(16)                                               # (never dereferenced: the shapes are refused first)
    assert lib.eab_room_rirs_f32(None, 1, 1, 1, 100, 16000.0, None, None) == 1
    assert lib.eab_room_rirs_f32(one, 1, 9, 1, 100, 16000.0, one, None) == 1          # S > 8
    assert lib.eab_room_rirs_f32(one, 1, 1, 33, 100, 16000.0, one, None) == 1         # M > 32
    assert lib.eab_room_rirs_f32(one, 1, 1, 1, 0, 16000.0, one, None) == 1
    assert lib.eab_room_gains_f32(None, 1, 1, 100, None, None, 16000.0, None, 1, None, None) == 1
    assert lib.eab_room_gains_f32(one, 1, 1, 3201, one, one, 16000.0, one, 2, one, None) == 1    # three windows, room for two
    assert lib.eab_room_workspace_bytes(1, 9, 1, 100, 100) == -1
    # 2 rows of source blocks + 1 channel pair x 1 partition, 1024 complex each
    assert lib.eab_room_workspace_bytes(1, 1, 1, 1000, 400) == 8 * 1024 * (2 + 1)
    assert lib.eab_room_convolve_f32(one, 1, 1, 1000, one, one, one, one, one, 1, 400, one, one, 8, one, one, None) == 1


def test_scene_record_layout():
    sc = _scene()
    r = sim._scene_record(sc)
    assert r.shape == (sim.SCENE_DOUBLES,) and list(r[:8]) == [4.0, 3.0, 2.5, 0.3, 2.0, 2.0, 0.0, -25.0]
    assert r[9] == 5.0 and list(r[16:22]) == [1.0, 1.0, 1.2, 3.0, 2.0, 1.4] and list(r[40:46]) == [2.0, 1.5, 1.1, 2.05, 1.5, 1.1]
    assert sim.response_lengths([sc], max_rir_seconds=0.01) == [160] and sim.response_lengths([sc]) == [sim.rir_length(sc.room_dim, 2, 16000)]


def test_python_mirrors_the_kernel_constants():
    """the sizes eabnet_amd/simulate.py allocates by are the #defines of csrc/room.hip"""
    import re
    src = open(os.path.join(ROOT, "eabnet_amd", "csrc", "room.hip")).read()
    d = {n: int(v, 0) for n, v in re.findall(r"^#define\s+ROOM_(\w+)\s+(\d+)\b", src, flags=re.M)}
    assert re.search(r"^#define\s+ROOM_NQ\s+\(ROOM_GRAM \+ ROOM_MAX_SRC\)", src, flags=re.M)
    assert sim.GAIN_SUMS == d["GRAM"] + d["MAX_SRC"] == 44
    assert (sim.SEGMENT, sim.PARTITION, sim.NFFT, sim.TAPS, sim.SCENE_DOUBLES) == (d["SEG"], d["PART"], d["NFFT"], d["TAPS"], d["SCENE"])
    assert (sim.MAX_SOURCES, sim.MAX_MICS, sim.MAX_ORDER) == (d["MAX_SRC"], d["MAX_MIC"], d["MAX_ORDER"])


def test_room_simulator_checks_before_it_touches_the_device():
    import torch
    simu = sim.RoomSimulator(_settings(), rir_method="ism")
    with pytest.raises(ValueError):
        simu.simulate(torch.zeros(2, 100), [_scene()])                 # not (B, S, L)
    with pytest.raises(ValueError):
        simu.simulate(torch.zeros(1, 2, 100), [])
    with pytest.raises(ValueError):
        simu.simulate(torch.zeros(1, 2, 100), [_scene(rir_method="hybrid")])
