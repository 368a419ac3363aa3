"""Training mixtures on the device: shoebox image-source rooms, what the reference's ``McseDatasetOnline`` makes per sample on
the host with pyroomacoustics (dataset/mcse_dataset.py:52-289 -> dataset/audio_util.py:6-88, ``rir_method == "ism"``), for a
padded batch in six launches of csrc/room.hip.

The definition (equality with pyroomacoustics is NOT verified, the library is not a dependency).  A scene has a
room Lr = (Lx, Ly, Lz), an energy absorption a in (0, 1], an order O, a rate fs, c = 343 m/s, sources s_0 (target), s_1.. (noises)
and microphones r_m.  Response h[s][m]: one image per integer triple n with |nx|+|ny|+|nz| <= O, per axis at n L + s for even n
and (n + 1) L - s for odd n; with d = |image - r_m|, g = (1 - a)^((|nx|+|ny|+|nz|)/2) / (4 pi d), tau = d fs / c,
k0 = floor(tau), f = tau - k0:

    h[k0 + i] += g (0.5 - 0.5 cos(2 pi i / 80)) sinc(i - 40 - f),        i = 0..80

(the 40-sample delay of the fractional-delay filter is kept).  h_free is the image n = 0 alone.  The dry gains are those of
``mix_scaler``: peak-normalised sources, the noises scaled to their SNR against the target by their active rms (windows of
int(fs/10) samples above -50 dB), the mixture scaled to dBFS.  Then

    noisy[m][t] = sum_s gain_s (x_s * h[s][m])[t],        clean[t] = gain_0 (x_0 * h_free[0][ref])[t],        t < L_b.

``rir_method="ism_tail"`` keeps of these images the ones closer than c tail_start to the centre of the array and
replaces the rest by a sampled tail: tail_density virtual images per sample with random directions and signs, recomputed on the
device from tail_seed; what it approximates is the ``"ism"`` response above, at about a tenth of its pulses.

The ``"hybrid"`` method of the reference's settings files (stochastic ray tracing, air absorption) is refused.  Reading,
cropping and resampling the source files stays with the caller (``eabnet_amd.resample``).  ``sample_scene`` is host code; the
rest runs on the device and has no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import model as _m

SOUND_SPEED = 343.0
TAPS = 81                                     # ROOM_TAPS of csrc/room.hip
MAX_SOURCES = 8                               # ROOM_MAX_SRC
MAX_MICS = 32                                 # ROOM_MAX_MIC
MAX_ORDER = 255                               # ROOM_MAX_ORDER
SCENE_DOUBLES = 144                           # ROOM_SCENE
SEGMENT = 4096                                # ROOM_SEG: samples of a response one workgroup holds in LDS
PARTITION = 512                               # ROOM_PART
NFFT = 1024                                   # ROOM_NFFT
GAIN_SUMS = 44                                # ROOM_NQ: doubles per window of the gains' scratch (36 Gram entries, 8 peaks)
MIN_SOURCE_MIC_DISTANCE = 0.1
RIR_METHODS = ("ism", "ism_tail")
MAX_TAIL_DENSITY = 64.0                       # ROOM_MAX_DENSITY
MIN_TAIL_DISTANCE = 1.0                       # metres between the array and the nearest virtual image of the tail
_TWIDDLES: Dict[str, torch.Tensor] = {}


def inverse_sabine(rt60: float, room_dim) -> Tuple[float, int]:
    """(energy absorption a, image order O) of a shoebox with reverberation time rt60 by Sabine's formula;
    ValueError when the room is too large for it (a > 1)."""
    Lx, Ly, Lz = (float(v) for v in room_dim)
    if not (rt60 > 0.0 and min(Lx, Ly, Lz) > 0.0):
        raise ValueError(f"rt60 and the room's dimensions must be positive, got {rt60} and {(Lx, Ly, Lz)}")
    V = Lx * Ly * Lz
    A = 2.0 * (Lx * Ly + Ly * Lz + Lx * Lz)
    a = 24.0 * math.log(10.0) * V / (SOUND_SPEED * A * rt60)
    if a > 1.0:
        raise ValueError(f"a room of {(Lx, Ly, Lz)} m cannot have rt60 = {rt60} s: absorption {a:.3f} > 1")
    return a, int(math.ceil(SOUND_SPEED * rt60 / min(Lx, Ly, Lz) - 1.0))


def rir_length(room_dim, max_order: int, fs) -> int:
    """samples of a response: an upper bound of the last index any image of order <= max_order writes, plus one (the farthest
    image lies (O + 1) L along one axis and L along the others)"""
    Lr = [float(v) for v in room_dim]
    far = 0.0
    for ax in range(3):
        d2 = sum(((max_order + 1) * Lr[k]) ** 2 if k == ax else Lr[k] ** 2 for k in range(3))
        far = max(far, math.sqrt(d2))
    return int(math.floor(float(fs) / SOUND_SPEED * far)) + TAPS


@dataclass
class Scene:
    """one utterance's room: plain fields.  sources[0] is the target, sources[1:] the noises with snr[j - 1] dB each."""
    room_dim: Sequence[float]
    absorption: float
    max_order: int
    fs: int
    sources: np.ndarray                       # (S, 3)
    mics: np.ndarray                          # (M, 3)
    ref_mic: int = 0
    snr: Sequence[float] = ()                 # (S - 1,)
    dBFS: float = -25.0
    rir_method: str = "ism"
    rt60: Optional[float] = None
    clean_name: Optional[str] = None
    meta: dict = field(default_factory=dict)
    tail_start: float = 0.05                  # "ism_tail": seconds from which the sampled tail stands for the images
    tail_density: float = 2.0                 # "ism_tail": virtual images per sample; 0: no tail
    tail_seed: int = 0                        # "ism_tail": an integer in [0, 2^53)

    @property
    def n_sources(self) -> int:
        return int(np.asarray(self.sources).shape[0])

    @property
    def n_mics(self) -> int:
        return int(np.asarray(self.mics).shape[0])


def check_scene(sc: Scene) -> None:
    """the refusals of the module: ValueError on the host, before anything is launched"""
    if sc.rir_method not in RIR_METHODS:
        raise ValueError(f"rir_method {sc.rir_method!r} is not supported: only the image-source model 'ism' and its variant with a "
                         "sampled tail 'ism_tail' are (the 'hybrid' method adds stochastic ray tracing and air absorption)")
    Lr = np.asarray(sc.room_dim, dtype=np.float64)
    src = np.asarray(sc.sources, dtype=np.float64)
    mic = np.asarray(sc.mics, dtype=np.float64)
    if Lr.shape != (3,) or not np.all(np.isfinite(Lr)) or not np.all(Lr > 0):
        raise ValueError(f"room_dim must be three positive lengths, got {sc.room_dim}")
    if src.ndim != 2 or src.shape[1] != 3 or mic.ndim != 2 or mic.shape[1] != 3:
        raise ValueError(f"sources and mics must be (S, 3) and (M, 3), got {src.shape} and {mic.shape}")
    S, M = src.shape[0], mic.shape[0]
    if not 1 <= S <= MAX_SOURCES:
        raise ValueError(f"a scene has 1 to {MAX_SOURCES} sources, got S = {S}")
    if not 1 <= M <= MAX_MICS:
        raise ValueError(f"a scene has 1 to {MAX_MICS} microphones, got M = {M}")
    if not (0.0 < sc.absorption <= 1.0):
        raise ValueError(f"the energy absorption must lie in (0, 1], got a = {sc.absorption}")
    if isinstance(sc.max_order, bool) or int(sc.max_order) != sc.max_order or not 0 <= sc.max_order <= MAX_ORDER:
        raise ValueError(f"max_order must be an integer in [0, {MAX_ORDER}], got {sc.max_order}")
    if not (float(sc.fs) >= 10.0 and float(sc.fs) <= 1.0e7):
        raise ValueError(f"fs must lie in [10, 1e7], got {sc.fs}")
    if not 0 <= int(sc.ref_mic) < M:
        raise ValueError(f"ref_mic must lie in [0, {M}), got {sc.ref_mic}")
    if len(sc.snr) != S - 1:
        raise ValueError(f"a scene of {S} sources needs {S - 1} SNRs, got {len(sc.snr)}")
    if not (np.all(np.isfinite(src)) and np.all(np.isfinite(mic)) and np.all(np.isfinite(np.asarray(sc.snr, dtype=np.float64)))
            and math.isfinite(float(sc.dBFS))):
        raise ValueError("positions, SNRs and dBFS must be finite")
    if np.any(src < 0) or np.any(src > Lr):
        raise ValueError(f"a source lies outside the room {tuple(Lr)}: {src[np.any((src < 0) | (src > Lr), axis=1)][0]}")
    if np.any(mic < 0) or np.any(mic > Lr):
        raise ValueError(f"a microphone lies outside the room {tuple(Lr)}: {mic[np.any((mic < 0) | (mic > Lr), axis=1)][0]}")
    dist = np.sqrt(((src[:, None, :] - mic[None, :, :]) ** 2).sum(-1))
    if dist.min() < MIN_SOURCE_MIC_DISTANCE:
        s, m = np.unravel_index(int(dist.argmin()), dist.shape)
        raise ValueError(f"source {s} lies {dist.min():.3f} m from microphone {m}: closer than {MIN_SOURCE_MIC_DISTANCE} m")
    if sc.rir_method == "ism_tail":
        _check_tail(sc.tail_start, sc.tail_density)
        seed = sc.tail_seed
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 53:
            raise ValueError(f"tail_seed must be an integer in [0, 2^53) (a double holds it exactly), got {seed!r}")
        radius = array_radius(mic)
        if SOUND_SPEED * float(sc.tail_start) < MIN_TAIL_DISTANCE + radius:
            raise ValueError(f"the tail would start too close to the array: c tail_start = {SOUND_SPEED * float(sc.tail_start):.3f} m is "
                             f"below {MIN_TAIL_DISTANCE} m plus the array's radius of {radius:.3f} m")


def _check_tail(tail_start, tail_density) -> None:
    if not (math.isfinite(float(tail_start)) and float(tail_start) > 0.0):
        raise ValueError(f"tail_start must be a positive number of seconds, got {tail_start}")
    if not (math.isfinite(float(tail_density)) and float(tail_density) >= 0.0):
        raise ValueError(f"tail_density must be finite and not negative, got {tail_density}")
    if float(tail_density) > MAX_TAIL_DENSITY:
        raise ValueError(f"tail_density is at most {MAX_TAIL_DENSITY:g} virtual images per sample, got {tail_density}")


def array_radius(mics) -> float:
    """the largest distance of a microphone from the mean of the microphone positions"""
    mic = np.asarray(mics, dtype=np.float64)
    return float(np.sqrt(((mic - mic.mean(0)) ** 2).sum(-1)).max())


def _angle_deg(v1, v2) -> float:
    c = float(np.dot(v1, v2) / (np.linalg.norm(v1) * np.linalg.norm(v2)))
    return math.degrees(math.acos(max(-1.0, min(1.0, c))))


def _uniform(rng: np.random.Generator, bounds) -> float:
    return float(bounds[0] + (bounds[1] - bounds[0]) * rng.random())


def sample_scene(settings: dict, rng: np.random.Generator, clean_name: Optional[str] = None, rir_method: Optional[str] = None,
                 max_tries: int = 100000, tail_start: float = 0.05, tail_density: float = 2.0) -> Scene:
    """one random scene by the rules of a settings dictionary (the reference's mcse_dataset_settings*.json): room between
    min_dim and max_dim; target and array centre at their heights, away from the walls, at a distance inside
    target.dist_to_mic_array (drawn again together otherwise); the array rotated about the vertical so that its direction
    points at the target; noise.n[0]..n[1] noises anywhere in the room at their heights, at least min_dist_to_mic_array from
    the array's centre and min_doa_diff_wrt_target degrees off the target as seen from it (each drawn again otherwise); one SNR
    per noise; an rt60 that the room can have (drawn again otherwise); dBFS.  rir_method overrides the settings' own; for
    "ism_tail" the scene gets tail_start and tail_density and, as the generator's last draw, its tail_seed (no other method
    draws it: their scenes of a given seed do not change)."""
    room = settings["room"]
    lo, hi = np.asarray(room["min_dim"], dtype=np.float64), np.asarray(room["max_dim"], dtype=np.float64)
    room_dim = lo + (hi - lo) * rng.random(3)
    arr, tgt, noi = settings["mic_array"], settings["target"], settings["noise"]
    if not tgt.get("fixed_doa", True):
        raise ValueError("target.fixed_doa = false is not supported (nor is it by the reference)")
    for _ in range(max_tries):
        d = tgt["min_dist_to_wall"]
        p_target = np.array([_uniform(rng, (d, room_dim[0] - d)), _uniform(rng, (d, room_dim[1] - d)), _uniform(rng, tgt["h"])])
        d = arr["min_dist_to_wall"]
        centre = np.array([_uniform(rng, (d, room_dim[0] - d)), _uniform(rng, (d, room_dim[1] - d)), _uniform(rng, arr["h"])])
        dist = float(np.linalg.norm(p_target - centre))
        if tgt["dist_to_mic_array"][0] <= dist <= tgt["dist_to_mic_array"][1]:
            break
    else:
        raise ValueError("no target / array position satisfies the settings")
    # rotate the array about the vertical: its direction towards the target
    p2 = np.array([[m["x"], m["y"]] for m in arr["mics"]], dtype=np.float64).T          # (2, M)
    v = np.array([arr["direction"]["x"], arr["direction"]["y"]], dtype=np.float64)
    w = p_target[:2] - centre[:2]
    ang = math.radians(_angle_deg(v, w))
    if v[0] * w[1] - v[1] * w[0] < 0:
        ang = -ang
    R = np.array([[math.cos(ang), -math.sin(ang)], [math.sin(ang), math.cos(ang)]])
    mics = np.concatenate([R @ p2, np.zeros((1, p2.shape[1]))], 0).T + centre[None, :]     # (M, 3)
    n_noises = int(rng.integers(noi["n"][0], noi["n"][1] + 1))
    snr = [_uniform(rng, noi["SNR"]) for _ in range(n_noises)]
    sources = [p_target]
    for _ in range(n_noises):
        for _ in range(max_tries):
            p = np.array([_uniform(rng, (0.0, room_dim[0])), _uniform(rng, (0.0, room_dim[1])), _uniform(rng, noi["h"])])
            if float(np.linalg.norm(p - centre)) < noi["min_dist_to_mic_array"]:
                continue
            if _angle_deg(p_target - centre, p - centre) < noi["min_doa_diff_wrt_target"]:
                continue
            break
        else:
            raise ValueError("no noise position satisfies the settings")
        sources.append(p)
    for _ in range(max_tries):
        rt60 = _uniform(rng, room["rt60"])
        try:
            a, order = inverse_sabine(rt60, room_dim)
        except ValueError:
            continue                                                  # the room is too large for this rt60
        break
    else:
        raise ValueError("no rt60 of the settings fits the room")
    sc = Scene(room_dim=room_dim, absorption=a, max_order=order, fs=settings["audio"]["fs"], sources=np.stack(sources), mics=mics,
               ref_mic=int(arr["ref_mic"]), snr=snr, dBFS=_uniform(rng, settings["noisy_dBFS"]),
               rir_method=rir_method if rir_method is not None else settings["audio"]["rir_method"], rt60=rt60,
               clean_name=clean_name, meta={"array_centre": centre})
    if sc.rir_method == "ism_tail":
        sc.tail_start, sc.tail_density = float(tail_start), float(tail_density)
        sc.tail_seed = int(rng.integers(0, 1 << 53))
    return sc


# -------------------------------------------------------------------------------------------------------------------------------
# the device side
def _scene_record(sc: Scene, k: Optional[int] = None) -> np.ndarray:
    """the SCENE_DOUBLES doubles csrc/room.hip reads for one scene; k: the sample its responses are cut at ("ism_tail" alone
    reads it; default: the scene's own response length)"""
    r = np.zeros(SCENE_DOUBLES, dtype=np.float64)
    r[0:3] = np.asarray(sc.room_dim, dtype=np.float64)
    r[3], r[4], r[5], r[6], r[7] = sc.absorption, sc.max_order, sc.n_sources, sc.ref_mic, sc.dBFS
    r[9:9 + sc.n_sources - 1] = np.asarray(sc.snr, dtype=np.float64)
    r[16:16 + 3 * sc.n_sources] = np.asarray(sc.sources, dtype=np.float64).reshape(-1)
    r[40:40 + 3 * sc.n_mics] = np.asarray(sc.mics, dtype=np.float64).reshape(-1)
    if sc.rir_method == "ism_tail":
        own = rir_length(sc.room_dim, sc.max_order, sc.fs)
        r[136:141] = sc.tail_seed, sc.tail_start, sc.tail_density, own, own if k is None else k
    return r


def _check_batch(scenes: Sequence[Scene], S_max: Optional[int] = None) -> Tuple[float, int, int]:
    """(fs, M, S_max) of a batch of checked scenes"""
    if len(scenes) < 1 or len(scenes) > 4096:
        raise ValueError(f"a batch has 1 to 4096 scenes, got {len(scenes)}")
    for sc in scenes:
        check_scene(sc)
    fs, M = float(scenes[0].fs), scenes[0].n_mics
    if any(float(sc.fs) != fs or sc.n_mics != M for sc in scenes):
        raise ValueError("the scenes of one batch share the sample rate and the number of microphones")
    if any(sc.rir_method != scenes[0].rir_method for sc in scenes):
        raise ValueError("the scenes of one batch share the rir_method: one launch makes all their responses")
    most = max(sc.n_sources for sc in scenes)
    if S_max is None:
        S_max = most
    if most > S_max:
        raise ValueError(f"a scene has {most} sources, the batch's tensor has {S_max} rows")
    if S_max > MAX_SOURCES:
        raise ValueError(f"a batch has at most {MAX_SOURCES} source rows, got S = {S_max}")
    return fs, M, S_max


def response_lengths(scenes: Sequence[Scene], max_rir_seconds: Optional[float] = None) -> List[int]:
    """samples of every scene's responses: rir_length, or the cap of max_rir_seconds where that is shorter"""
    ks = [rir_length(sc.room_dim, sc.max_order, sc.fs) for sc in scenes]
    if max_rir_seconds is not None:
        if not max_rir_seconds > 0:
            raise ValueError(f"max_rir_seconds must be positive, got {max_rir_seconds}")
        ks = [min(k, max(1, int(max_rir_seconds * float(sc.fs)))) for k, sc in zip(ks, scenes)]
    return ks


def first_arrival(sc: Scene) -> int:
    """a sample index before which nothing of the scene reaches a microphone: one below the delay of its shortest path.  The
    mixing kernel writes exact zeros before it, where a transform would leave its rounding (about 1e-9 of the block's peak); the
    definition's value there is zero, so this is a property of this implementation, not part of the contract."""
    src, mic = np.asarray(sc.sources, dtype=np.float64), np.asarray(sc.mics, dtype=np.float64)
    d = np.sqrt(((src[:, None, :] - mic[None, :, :]) ** 2).sum(-1)).min()
    if sc.rir_method == "ism_tail":                                   # the tail's images lie c tail_start or more from the centre
        d = min(d, SOUND_SPEED * float(sc.tail_start) - array_radius(mic))
    return max(0, int(math.floor(d * float(sc.fs) / SOUND_SPEED)) - 1)


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _to_device(a: np.ndarray, device: torch.device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(device, non_blocking=True)


def _twiddles(device: torch.device) -> torch.Tensor:
    key = str(device)
    hit = _TWIDDLES.get(key)
    if hit is None:
        ang = -2.0 * np.pi * np.arange(NFFT, dtype=np.float64) / NFFT
        hit = _TWIDDLES[key] = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)).to(device)
    return hit


def _need_cuda(device: torch.device, what: str) -> None:
    if device.type != "cuda":
        raise _lib.EabError(f"{what} needs a CUDA (ROCm) device; there is no CPU fallback by design.")


def _check_sources(sources: torch.Tensor, scenes: Sequence[Scene], lengths):
    if not isinstance(sources, torch.Tensor) or sources.ndim != 3:
        raise ValueError("sources must be a (B, S, L) tensor")
    B, S_max, L = sources.shape
    if B != len(scenes):
        raise ValueError(f"{B} rows of sources for {len(scenes)} scenes")
    if L < 1 or L > 1 << 28:
        raise ValueError(f"the sources must have 1 to 2^28 samples, got {L}")
    fs, M, S_max = _check_batch(scenes, S_max)
    lens = [L] * B if lengths is None else _m.check_lengths(lengths, B, L, lo=1, unit="the samples of a row", integral=True)
    _need_cuda(sources.device, "simulate_rooms")
    if sources.dtype != torch.float32 or not sources.is_contiguous():
        sources = sources.to(torch.float32).contiguous()
    return sources, fs, M, lens


def _launch_rirs(records: torch.Tensor, B: int, S_max: int, M: int, K: int, fs: float, h: torch.Tensor, method: str = "ism") -> None:
    name = {"ism": "eab_room_rirs_f32", "ism_tail": "eab_room_rirs_tail_f32"}[method]
    _lib.check(getattr(_lib.load(), name)(records.data_ptr(), B, S_max, M, K, fs, h.data_ptr(), _stream()), name)


def _launch_gains(x: torch.Tensor, lens: torch.Tensor, records: torch.Tensor, fs: float, partial: torch.Tensor, nwin: int,
                  gains: torch.Tensor) -> None:
    B, S_max, L = x.shape
    _lib.check(_lib.load().eab_room_gains_f32(x.data_ptr(), B, S_max, L, lens.data_ptr(), records.data_ptr(), fs, partial.data_ptr(),
                                              nwin, gains.data_ptr(), _stream()), "eab_room_gains_f32")


def _windows(L: int, fs: float) -> int:
    W = int(fs / 10.0)
    return (L + W - 1) // W


def image_source_rirs(scenes: Sequence[Scene], device, max_rir_seconds: Optional[float] = None, sources: Optional[int] = None):
    """(h, lengths): h (B, S, M + 1, K) fp32 on ``device``, h[b, s, m] the response from source s to microphone m and
    h[b, s, M] the free-field response to the reference microphone; K the longest of the scenes' own response lengths
    ``lengths`` (rows are zero past them, and for s >= S_b).  max_rir_seconds (a deviation, off by default): responses are cut
    at that many seconds; images that arrive later are dropped.  sources: rows S of the table (default: the most of any scene).
    The scenes' rir_method picks the model: "ism", or "ism_tail" (the tail's images are those of the uncut response)."""
    device = torch.device(device)
    fs, M, S_max = _check_batch(scenes, sources)
    _need_cuda(device, "image_source_rirs")
    ks = response_lengths(scenes, max_rir_seconds)
    K, B = max(ks), len(scenes)
    with torch.cuda.device(device):
        records = _to_device(np.stack([_scene_record(sc, k) for sc, k in zip(scenes, ks)]), device)
        h = torch.empty((B, S_max, M + 1, K), dtype=torch.float32, device=device)
        _launch_rirs(records, B, S_max, M, K, fs, h, scenes[0].rir_method)
    return h, ks


def mix_gains(sources: torch.Tensor, scenes: Sequence[Scene], lengths=None) -> torch.Tensor:
    """(B, S) float64 on the device: the factor of every dry source in its utterance's mixture (zeros for s >= S_b)"""
    sources, fs, M, lens = _check_sources(sources, scenes, lengths)
    B, S_max, L = sources.shape
    with torch.cuda.device(sources.device):
        records = _to_device(np.stack([_scene_record(sc) for sc in scenes]), sources.device)
        nwin = _windows(L, fs)
        partial = torch.empty((B, nwin, GAIN_SUMS), dtype=torch.float64, device=sources.device)
        gains = torch.empty((B, S_max), dtype=torch.float64, device=sources.device)
        _launch_gains(sources, _m._device_lengths(lens, sources.device), records, fs, partial, nwin, gains)
    return gains


class _Buffers:
    """the device buffers of one batch shape; grown, never shrunk"""

    def __init__(self):
        self.t: Dict[str, torch.Tensor] = {}

    def get(self, name: str, numel: int, dtype: torch.dtype, device: torch.device) -> torch.Tensor:
        cur = self.t.get(name)
        if cur is None or cur.numel() < numel or cur.device != device:
            cur = self.t[name] = torch.empty(max(numel, 1), dtype=dtype, device=device)
        return cur[:numel]


def _simulate(sources: torch.Tensor, scenes: Sequence[Scene], lengths, max_rir_seconds, buf: _Buffers, out=None):
    sources, fs, M, lens = _check_sources(sources, scenes, lengths)
    B, S_max, L = sources.shape
    dev = sources.device
    ks = response_lengths(scenes, max_rir_seconds)
    K = max(ks)
    lib = _lib.load()
    work_bytes = lib.eab_room_workspace_bytes(B, S_max, M, L, K)
    if work_bytes < 0:
        raise ValueError(f"simulate_rooms: shape (B, S, M, L, K) = {(B, S_max, M, L, K)} is out of the kernels' range")
    with torch.cuda.device(dev):
        records = _to_device(np.stack([_scene_record(sc, k) for sc, k in zip(scenes, ks)]), dev)
        dlens = _m._device_lengths(lens, dev)
        klen = _to_device(np.asarray([[k, first_arrival(sc)] for k, sc in zip(ks, scenes)], dtype=np.int32), dev)
        nwin = _windows(L, fs)
        partial = buf.get("partial", B * nwin * GAIN_SUMS, torch.float64, dev)
        gains = buf.get("gains", B * S_max, torch.float64, dev)
        h = buf.get("h", B * S_max * (M + 1) * K, torch.float32, dev)
        work = buf.get("work", (work_bytes + 7) // 8, torch.float64, dev)
        if out is None:
            noisy = torch.empty((B, M, L), dtype=torch.float32, device=dev)
            clean = torch.empty((B, 1, L), dtype=torch.float32, device=dev)
        else:
            noisy, clean = out
        _launch_gains(sources, dlens, records, fs, partial, nwin, gains)
        _launch_rirs(records, B, S_max, M, K, fs, h, scenes[0].rir_method)
        _lib.check(lib.eab_room_convolve_f32(sources.data_ptr(), B, S_max, L, dlens.data_ptr(), records.data_ptr(), klen.data_ptr(),
                                             gains.data_ptr(), h.data_ptr(), M, K, _twiddles(dev).data_ptr(), work.data_ptr(),
                                             work_bytes, noisy.data_ptr(), clean.data_ptr(), _stream()), "eab_room_convolve_f32")
    return noisy, clean


def simulate_rooms(sources: torch.Tensor, scenes: Sequence[Scene], lengths=None, max_rir_seconds: Optional[float] = None):
    """sources (B, S, L) fp32 on the device (row 0 the target, rows 1.. the noises of each scene; rows at and past a scene's
    own source count and samples at and past ``lengths[b]`` are never read) -> noisy (B, M, L), clean (B, 1, L): the tensors
    ``prepare_data(x, target, device, args)`` takes.  Zero from lengths[b] on, and before the first arrival.  Six launches, no host synchronisation; an
    utterance has the same bits alone, in any batch and in a second call."""
    return _simulate(sources, scenes, lengths, max_rir_seconds, _Buffers())


class RoomSimulator:
    """``sim = RoomSimulator(settings); scenes = sim.sample(B); noisy, clean = sim.simulate(sources, scenes)``: scenes drawn from
    a settings dictionary and mixtures made on a side stream with buffers the simulator owns, so that the next batch can be made
    while a training step runs.  ``simulate`` orders the side stream after the caller's current stream (the sources are ready),
    enqueues the six launches there and returns at once; ``wait()`` orders the caller's current stream after them, without a
    host synchronisation.  Two output slots alternate: the tensors of a call stay untouched until the call after the next."""

    def __init__(self, settings: dict, max_batch: int = 6, seed: int = 0, rir_method: Optional[str] = None,
                 max_rir_seconds: Optional[float] = None, tail_start: float = 0.05, tail_density: float = 2.0):
        self.settings = settings
        self.rir_method = rir_method if rir_method is not None else settings["audio"]["rir_method"]
        if self.rir_method not in RIR_METHODS:
            raise ValueError(f"rir_method {self.rir_method!r} is not supported: only the image-source model 'ism' and its variant "
                             "with a sampled tail 'ism_tail' are; pass rir_method='ism' or rir_method='ism_tail' to use a settings "
                             "file written for 'hybrid'")
        _check_tail(tail_start, tail_density)
        self.tail_start, self.tail_density = float(tail_start), float(tail_density)
        if len(settings["mic_array"]["mics"]) > MAX_MICS:
            raise ValueError(f"a scene has at most {MAX_MICS} microphones, got M = {len(settings['mic_array']['mics'])}")
        if settings["noise"]["n"][1] + 1 > MAX_SOURCES:
            raise ValueError(f"a scene has at most {MAX_SOURCES} sources, the settings ask for up to S = {settings['noise']['n'][1] + 1}")
        if max_batch < 1:
            raise ValueError(f"max_batch must be positive, got {max_batch}")
        self.max_batch = int(max_batch)
        self.max_rir_seconds = max_rir_seconds
        self.rng = np.random.default_rng(seed)
        self.n_sources = int(settings["noise"]["n"][1]) + 1              # rows of the sources tensor that fit every scene
        self._buf = _Buffers()
        self._out = [_Buffers(), _Buffers()]
        self._slot = 0
        self._stream: Optional[torch.cuda.Stream] = None
        self._done: Optional[torch.cuda.Event] = None

    def sample(self, n: int, clean_names: Optional[Sequence[str]] = None) -> List[Scene]:
        if not 1 <= n <= self.max_batch:
            raise ValueError(f"a batch has 1 to max_batch = {self.max_batch} scenes, got {n}")
        return [sample_scene(self.settings, self.rng, None if clean_names is None else clean_names[i], rir_method=self.rir_method,
                             tail_start=self.tail_start, tail_density=self.tail_density) for i in range(n)]

    def simulate(self, sources: torch.Tensor, scenes: Sequence[Scene], lengths=None):
        if len(scenes) > self.max_batch:
            raise ValueError(f"a batch has at most max_batch = {self.max_batch} scenes, got {len(scenes)}")
        sources, _, M, _ = _check_sources(sources, scenes, lengths)
        dev = sources.device
        with torch.cuda.device(dev):
            if self._stream is None or self._stream.device != dev:
                self._stream = torch.cuda.Stream(device=dev)
            self._stream.wait_stream(torch.cuda.current_stream())
            B, _, L = sources.shape
            slot = self._out[self._slot]
            self._slot ^= 1
            with torch.cuda.stream(self._stream):                      # (the slots too: allocated, written and freed on this stream)
                out = (slot.get("noisy", B * M * L, torch.float32, dev).view(B, M, L),
                       slot.get("clean", B * L, torch.float32, dev).view(B, 1, L))
                noisy, clean = _simulate(sources, scenes, lengths, self.max_rir_seconds, self._buf, out)
                sources.record_stream(self._stream)
                self._done = torch.cuda.Event()
                self._done.record(self._stream)
        return noisy, clean

    def wait(self) -> None:
        """order the caller's current stream after the last ``simulate``"""
        if self._done is not None:
            torch.cuda.current_stream().wait_event(self._done)
