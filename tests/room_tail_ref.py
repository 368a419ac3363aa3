"""The response model "ism_tail" of DESIGN.md 4.23 in float64 numpy: the reference of tests/test_room_tail_ref.py and
tests/test_room_tail_gpu.py, written from the definition (not from eabnet_amd/simulate.py or csrc/room.hip).  The early part
is room_ref's image set cut at r_mix = c tail_start about the mean of the microphone positions, the tail a train of virtual
images recomputed from a counter-based generator.  A scene is any object with the fields of eabnet_amd.simulate.Scene."""
import math

import numpy as np

import room_ref as ref

C = ref.C
TAPS = ref.TAPS
GOLDEN = 0x9E3779B97F4A7C15


def mix(z):
    """the finaliser of the generator on uint64 arrays (arithmetic modulo 2^64)"""
    z = np.array(z, dtype=np.uint64, ndmin=1)
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def words(seed, s, d, j):
    """mix(seed + GOLDEN (1 + (((4 s + d) << 32) | j))) for an array of image indices j"""
    j = np.array(j, dtype=np.uint64, ndmin=1)
    with np.errstate(over="ignore"):
        counter = (np.uint64((4 * s + d) << 32) | j) + np.uint64(1)
        return mix(np.uint64(seed) + np.uint64(GOLDEN) * counter)


def uniforms(seed, s, j):
    """(4, len(j)): U0..U3 in [0, 1) of the images j of source s"""
    return np.stack([(words(seed, s, d, j) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 for d in range(4)])


def centre(sc):
    mic = np.asarray(sc.mics, dtype=np.float64)
    total = np.zeros(3)
    for r in mic:                                                      # in index order
        total = total + r
    return total / len(mic)


def tail_counts(sc, K=None):
    """(k_mix, n_slots, J, nu) of a scene whose own response length is K"""
    K = ref.rir_length(list(sc.room_dim), sc.max_order, float(sc.fs)) if K is None else K
    k_mix = int(math.floor(sc.tail_start * float(sc.fs)))
    n_slots = K - TAPS - k_mix
    if n_slots > 0 and sc.absorption < 1.0 and sc.tail_density > 0:
        J = int(math.ceil(sc.tail_density * n_slots))
        return k_mix, n_slots, J, J / n_slots
    return k_mix, n_slots, 0, 0.0


def tail_images(sc, s, K=None):
    """the virtual images of source s: (t (J,), position (J, 3), direction (J, 3), reflections (J,), sign (J,))"""
    _, _, J, nu = tail_counts(sc, K)
    if J == 0:
        return np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0)
    fs = float(sc.fs)
    U = uniforms(sc.tail_seed, s, np.arange(J))
    t = sc.tail_start + (np.arange(J) + U[0]) / (nu * fs)
    z = 2.0 * U[1] - 1.0
    phi = 2.0 * np.pi * U[2]
    u = np.stack([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z], 1)
    sign = np.where(U[3] < 0.5, -1.0, 1.0)
    pos = centre(sc)[None, :] + (C * t)[:, None] * u
    walls = C * t * (np.abs(u) / np.asarray(sc.room_dim, dtype=np.float64)[None, :]).sum(1)
    return t, pos, u, walls, sign


def tail_pulses(sc, s, mic, K=None):
    """(k0, f, g) of the tail of source s at the position mic"""
    _, _, J, nu = tail_counts(sc, K)
    t, pos, _, walls, sign = tail_images(sc, s, K)
    if J == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0)
    fs = float(sc.fs)
    Lr = [float(v) for v in sc.room_dim]
    V = Lr[0] * Lr[1] * Lr[2]
    diff = pos - np.asarray(mic, dtype=np.float64)
    d = np.sqrt(diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2])
    g = sign * np.sqrt(4.0 * np.pi * C ** 3 * t * t / (V * fs * nu)) * np.exp(0.5 * walls * math.log(1.0 - sc.absorption)) / (4.0 * np.pi * d)
    tau = d * fs / C
    k0 = np.floor(tau).astype(np.int64)
    return k0, tau - k0, g


def early_pulses(sc, s, mic):
    """(n, k0, f, g) of the images of source s closer than r_mix to the centre of the array, at the position mic"""
    src = np.asarray(sc.sources, dtype=np.float64)[s]
    n, pos = ref.images(sc.room_dim, sc.max_order, src)
    e = pos - centre(sc)
    keep = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]) < C * sc.tail_start
    n, k0, f, g = ref.image_pulses(sc.room_dim, sc.absorption, sc.max_order, float(sc.fs), src, mic)
    return n[keep], k0[keep], f[keep], g[keep]


def rir(sc, s, m, K=None, cut=None, tail=True, early=True):
    """the response of source s at microphone m: K its own length (it fixes the tail), cut the sample it is cut at"""
    K = ref.rir_length(list(sc.room_dim), sc.max_order, float(sc.fs)) if K is None else K
    h = np.zeros(K if cut is None else cut, dtype=np.float64)
    mic = np.asarray(sc.mics, dtype=np.float64)[m]
    if early:
        _, k0, f, g = early_pulses(sc, s, mic)
        ref.add_pulses(h, k0, f, g)
    if tail:
        k0, f, g = tail_pulses(sc, s, mic, K)
        inside = k0 < len(h)
        ref.add_pulses(h, k0[inside], f[inside], g[inside])
    return h


def scene_rirs(sc, K=None, cut=None):
    """(S, M + 1, K or cut): row M the free-field response of the reference microphone, the direct image alone"""
    K = ref.rir_length(list(sc.room_dim), sc.max_order, float(sc.fs)) if K is None else K
    n = K if cut is None else cut
    src, mic = np.asarray(sc.sources, dtype=np.float64), np.asarray(sc.mics, dtype=np.float64)
    h = np.zeros((len(src), len(mic) + 1, n))
    for s in range(len(src)):
        for m in range(len(mic)):
            h[s, m] = rir(sc, s, m, K, cut)
        h[s, len(mic)] = ref.rir(sc.room_dim, 1.0, 0, float(sc.fs), src[s], mic[sc.ref_mic], n)
    return h
