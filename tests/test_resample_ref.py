"""Resampling without a device: the float64 definition (tests/resample_ref.py) against scipy's upfirdn, the polyphase bank of
``eabnet_amd.resample.filter_bank`` against the definition, the new entry point in the header, the binding and the library, and
the unchanged defaults of the three tools."""
import ctypes
import importlib
import inspect
import os

import numpy as np
import pytest
import torch

import eabnet_amd
import resample_ref as ref

rs = importlib.import_module("eabnet_amd.resample")       # (eabnet_amd.resample, the attribute, is the function)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(48000, 16000), (44100, 16000), (16000, 48000), (8000, 16000), (22050, 16000), (32000, 16000)]
LENGTHS = [1, 20, 163, 2085]
EPS = 2.0 ** -24


@pytest.mark.parametrize("orig,new", PAIRS)
def test_definition_equals_upfirdn(orig, new):
    pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(orig + new)
    for L in LENGTHS:
        x = rng.standard_normal(L)
        y = ref.ref_resample(x, orig, new)
        want = ref.upfirdn_resample(x, orig, new)
        assert y.shape == want.shape == (ref.out_length(L, orig, new),)
        err = np.abs(y - want).max()
        print(f"{orig}->{new} L={L}: max |ref - upfirdn| {err:.2e}")
        assert err <= 1e-12


@pytest.mark.parametrize("orig,new,n,K", [(48000, 16000, 1, 37), (44100, 16000, 160, 34), (22050, 16000, 320, 17),
                                          (16000, 48000, 3, 13), (11025, 16000, 640, 13), (96000, 16000, 1, 73)])
def test_bank_sizes(orig, new, n, K):
    tab, first, o, n_, K_ = rs.filter_bank(orig, new)
    assert (n_, K_) == (n, K) and tab.shape == (n, K) and tab.dtype == np.float64
    assert first.shape == (n,) and first.dtype == np.int32
    assert o * new == n * orig
    # what the kernel's tiling relies on
    assert (np.diff(first) >= 0).all() and first[-1] - first[0] <= o


@pytest.mark.parametrize("window", ["hann", "kaiser"])
@pytest.mark.parametrize("orig,new", PAIRS + [(16000, 44100), (11025, 16000)])
def test_bank_is_the_prototype_cut_into_phases(orig, new, window):
    tab, first, o, n, K = rs.filter_bank(orig, new, window)
    base = 0.99 * min(o, n)
    p = np.arange(n)[:, None]
    m = first.astype(np.int64)[:, None] + np.arange(-2, K + 2)[None, :]            # two taps on either side of every run
    want = ref.h((m * n - p * o) / float(o * n), o, n, window)
    assert np.abs(want[:, 2:K + 2] - tab).max() <= 1e-15
    assert (want[:, :2] == 0.0).all(), "a tap before first[p] lies inside the support"
    # the taps the bank drops: outside the support they are zero by definition; the ones a clamp of u to +-lw would keep (as
    # torchaudio's kernel does) have the value of the prototype AT the clamp, (base/o) sinc(lw) w(lw): cos^2(pi/2) ~ 4e-33 for
    # the hann window; 1/I0(beta) ~ 4e-6 for the kaiser window, times sinc(6) ~ 4e-17
    at_clamp = abs((base / o) * np.sinc(6.0) * ref.window_value(np.float64(6.0), 6.0, window))
    print(f"{orig}->{new} {window}: tap at the clamp {at_clamp:.2e}")
    assert at_clamp < (1e-30 if window == "hann" else 1e-20)
    for pp in range(n):
        run = np.nonzero(np.abs(base * ((m[pp] * n - pp * o) / float(o * n))) < 6)[0]
        assert run[0] == 2 and (np.diff(run) == 1).all() and len(run) <= K
    gain = tab.sum()
    print(f"{orig}->{new} {window}: n={n} K={K} sum={gain:.6f}")
    assert abs(gain - n) <= 1e-3 * n


def _fp32_bank_apply(x32, orig, new, window="hann"):
    """the bank's taps in fp32, accumulated in ascending k in fp32 (unfused), as a numpy loop"""
    tab, first, o, n, K = rs.filter_bank(orig, new, window)
    t32 = tab.astype(np.float32)
    L = len(x32)
    n_out = rs.resampled_length(L, orig, new)
    i = np.arange(n_out)
    q, p = i // n, i % n
    acc = np.zeros(n_out, dtype=np.float32)
    for k in range(K):
        j = q * o + first[p] + k
        xv = np.where((j >= 0) & (j < L), x32[np.clip(j, 0, L - 1)], np.float32(0)).astype(np.float32)
        acc = (acc + t32[p, k] * xv).astype(np.float32)
    return acc, K


@pytest.mark.parametrize("orig,new", PAIRS)
def test_bank_in_fp32_stays_inside_the_bound(orig, new):
    rng = np.random.default_rng(7)
    worst = 0.0
    for L in LENGTHS:
        x32 = rng.standard_normal(L).astype(np.float32)
        got, K = _fp32_bank_apply(x32, orig, new)
        y, ya = ref.ref_resample(x32, orig, new), ref.ref_abs(x32, orig, new)
        bound = (2 * K + 2) * EPS * ya
        assert got.shape == y.shape
        ok = bound > 0
        assert (np.abs(got - y)[~ok] == 0).all()
        worst = max(worst, float((np.abs(got - y)[ok] / bound[ok]).max()) if ok.any() else 0.0)
        assert (np.abs(got - y) <= bound).all()
    print(f"{orig}->{new}: largest err / bound {worst:.3f}")


def test_kaiser_window_against_numpy_i0():
    lw, beta = 6.0, 14.769656459379492
    u = np.linspace(-5.999, 5.999, 1001)
    want = np.i0(beta * np.sqrt(1.0 - (u / lw) ** 2)) / np.i0(beta)
    base = 0.99
    got = rs.prototype(u / base, 3, 1, "kaiser") / ((base / 3) * np.sinc(u))
    keep = np.abs(np.sinc(u)) > 1e-3
    assert np.abs(got[keep] - want[keep]).max() <= 1e-12
    assert rs.KAISER_BETA == beta
    with pytest.raises(ValueError, match="window"):
        rs.filter_bank(48000, 16000, "boxcar")


def test_resampled_length():
    assert rs.resampled_length(0, 48000, 16000) == 0
    assert [rs.resampled_length(L, 48000, 16000) for L in (1, 2, 3, 4, 48000)] == [1, 1, 1, 2, 16000]
    assert rs.resampled_length(44100, 44100, 16000) == 16000 and rs.resampled_length(44101, 44100, 16000) == 16001
    assert rs.resampled_length(163, 16000, 44100) == -(-441 * 163 // 160)
    assert rs.resampled_length(777, 16000, 16000) == 777
    for L in (1, 20, 163, 2085):
        for orig, new in PAIRS:
            assert rs.resampled_length(L, orig, new) == ref.out_length(L, orig, new)
    assert eabnet_amd.resampled_length is rs.resampled_length and eabnet_amd.filter_bank is rs.filter_bank


def test_refusals_on_the_host():
    with pytest.raises(ValueError, match="44101 -> 16000"):
        rs.filter_bank(44101, 16000)                          # n = 16000 phases: far over the LDS cap
    with pytest.raises(ValueError, match="LDS"):
        rs.filter_bank(16000, 44101)
    with pytest.raises(ValueError, match="positive integers"):
        rs.filter_bank(0, 16000)
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback by design"):
        eabnet_amd.resample(torch.zeros(2, 100), 48000, 16000)
    with pytest.raises(ValueError, match="mic_order"):
        eabnet_amd.resample(torch.zeros(2, 100), 48000, 16000, mic_order=[0, 2])
    with pytest.raises(ValueError, match="lengths"):
        eabnet_amd.resample(torch.zeros(2, 3, 100), 48000, 16000, lengths=[50, 101])


def test_streaming_push_size_must_be_whole():
    model = eabnet_amd.EaBNet(M=2)
    with pytest.raises(ValueError, match="whole number"):
        eabnet_amd.StreamingEnhancer(model, 1, 1.0, 1, sample_rate=22050)       # 160 * 441 / 320 = 220.5 samples per push
    with pytest.raises(ValueError, match="whole number"):
        eabnet_amd.StreamingEnhancer(model, 1, 1.0, 3, sample_rate=11025)       # 480 * 441 / 640 = 330.75


def test_entry_point_is_declared_bound_and_exported():
    from eabnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "eabnet_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert "eab_resample_f32(" in header and "eab_resample_f32" in _lib.EXPORTS and hasattr(lib, "eab_resample_f32")
    assert _lib.ABI_VERSION == 10 and "#define EAB_ABI_VERSION 10" in header, "only an entry point was added: the ABI stays 10"
    assert _lib.load().eab_abi_version() == 10
    assert "resample.hip" in open(os.path.join(ROOT, "eabnet_amd", "csrc", "Makefile")).read()


def test_argument_validation_happens_before_any_launch():
    from eabnet_amd import _lib
    f = _lib.load().eab_resample_f32
    buf = (ctypes.c_float * 64)()                             # host memory stands in: a refused call launches and reads nothing
    p = ctypes.addressof(buf)

    def call(x=p, cols=8, rows=1, rpu=1, y=p, n_out=3, tab=p, first=p, o=3, n=1, K=37, io=0, oo=0, vh=-1):
        return f(x, 8, cols, None, None, rows, rpu, y, 8, n_out, tab, first, o, n, K, io, oo, vh, None)

    assert call(x=None) == 1 and call(y=None) == 1 and call(tab=None) == 1 and call(first=None) == 1
    assert call(o=0) == 1 and call(n=0) == 1 and call(K=0) == 1
    assert call(n=160, K=103) == 1                            # 16480 floats of bank
    assert call(rows=-1) == 1 and call(cols=-1) == 1 and call(n_out=-1) == 1 and call(rpu=0) == 1
    assert call(io=-1) == 1 and call(oo=-1) == 1
    assert call(o=64, K=770) == 1                             # 64 input samples per output: the span of a tile exceeds LDS
    assert call(rows=0) == 0 and call(n_out=0) == 0           # nothing to do is no error (and launches nothing)


def test_defaults_of_the_tools_are_unchanged():
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()][1:]

    e = params(eabnet_amd.Enhancer.__init__)
    assert [n for n, _ in e] == ["model", "max_batch", "fft_num", "hop", "window", "length_buckets", "sample_rate", "mic_order",
                                 "output_rate"]
    assert [d for _, d in e][1:] == [16, 320, 160, None, "auto", 16000, None, None]
    s = params(eabnet_amd.Scorer.__init__)
    assert [n for n, _ in s] == ["model", "max_batch", "fft_num", "hop", "window", "length_buckets", "ref_mic", "sample_rate",
                                 "mic_order"]
    assert [d for _, d in s][1:] == [16, 320, 160, None, "auto", 0, 16000, None]
    t = params(eabnet_amd.StreamingEnhancer.__init__)
    assert [n for n, _ in t] == ["model", "B", "seconds", "chunk", "sr", "fft_num", "hop", "endless", "sample_rate", "mic_order"]
    assert [d for _, d in t][3:] == [1, 16000, 320, 160, False, None, None]
    r = [(p.name, p.default) for p in inspect.signature(eabnet_amd.resample).parameters.values()]
    assert r == [("wav", inspect.Parameter.empty), ("orig_freq", inspect.Parameter.empty), ("new_freq", inspect.Parameter.empty),
                 ("lengths", None), ("mic_order", None), ("window", "hann"), ("lowpass_filter_width", 6), ("rolloff", 0.99)]
