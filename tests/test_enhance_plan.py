"""Batched enhancement, host side (no GPU): the grouping rule ``plan_batches``, the validation of ``lengths=`` in the front and
back end, the re-planning of a batch whose program exceeds the arena budget, and the two new C-ABI entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

import eabnet_amd
from eabnet_amd import Enhancer, plan_batches
from eabnet_amd import model as mdl
from eabnet_amd.enhance import Batch, batch_sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = mdl.AUTO_BUCKETS


def bench_frames(files=50):
    """the seeded file lengths of tools/bench_varlen.py (2 .. 10 s at 16 kHz, hop 160)"""
    seconds = np.random.default_rng(1234).uniform(2.0, 10.0, size=files)
    return [1 + int(s * 16000) // 160 for s in seconds]


def check_plan(frames, caps, max_batch, plan):
    sizes = batch_sizes(max_batch)
    seen = [i for b in plan for i in b.indices]
    assert sorted(seen) == list(range(len(frames))), "every file exactly once"
    for b in plan:
        longest = max(frames[i] for i in b.indices)
        assert frames[b.indices[0]] == longest, "slot 0 holds the longest member"
        assert 1 <= len(b.indices) <= max_batch
        if b.cap is None:
            assert longest > max(caps) and len(b.indices) == 1 and b.batch_size == 1
            continue
        assert b.cap == min(c for c in caps if c >= longest), "the smallest cap that holds the longest member"
        assert b.batch_size == min(s for s in sizes if s >= len(b.indices)), "the smallest allowed batch size that holds the group"
        assert b.dummies == b.batch_size - len(b.indices) >= 0
    # outputs map back to input order: writing each batch's results to its indices fills every position once
    out = [None] * len(frames)
    for b in plan:
        for slot, i in enumerate(b.indices):
            assert out[i] is None
            out[i] = (id(b), slot)
    assert all(o is not None for o in out)


@pytest.mark.parametrize("name,frames,max_batch", [
    ("bench", bench_frames(), 16), ("bench_mb8", bench_frames(), 8), ("equal", [301] * 21, 16), ("single", [137], 16),
    ("max_batch_1", bench_frames(9), 1), ("above_caps", [100, 9000, 8192, 20000, 64, 65], 4), ("ties", [64, 64, 65, 64, 65], 2)])
def test_plan_invariants(name, frames, max_batch):
    check_plan(frames, CAPS, max_batch, plan_batches(frames, CAPS, max_batch))


def test_plan_of_the_50_bench_lengths():
    """four groups of 16, 16, 16 and 2 files in the caps 1024, 1024, 512, 256 at batch sizes 16, 16, 16, 4 (two dummies); the
    frames padded up to each group's longest member stay at or below 0.26 of its valid frames"""
    frames = bench_frames()
    plan = plan_batches(frames, CAPS, 16)
    assert [(len(b.indices), b.cap, b.batch_size, b.dummies) for b in plan] == \
        [(16, 1024, 16, 0), (16, 1024, 16, 0), (16, 512, 16, 0), (2, 256, 4, 2)]
    ratios = []
    for b in plan:
        valid = sum(frames[i] for i in b.indices)
        ratios.append((frames[b.indices[0]] * len(b.indices) - valid) / valid)
    assert [round(r, 2) for r in ratios] == [0.08, 0.25, 0.26, 0.10]
    assert max(ratios) <= 0.26
    order = [i for b in plan for i in b.indices]
    assert [frames[i] for i in order] == sorted(frames, reverse=True), "longest first, neighbours in length share a batch"


def test_plan_batch_sizes_and_refusals():
    assert batch_sizes(16) == (16, 4, 1) and batch_sizes(4) == (4, 1) and batch_sizes(3) == (3, 1) and batch_sizes(1) == (1,)
    assert plan_batches([], CAPS, 16) == []
    assert plan_batches([70, 300], (64, 128), 4) == [Batch((1,), None, 1), Batch((0,), 128, 1)]
    with pytest.raises(ValueError):
        plan_batches([10], CAPS, 0)
    with pytest.raises(ValueError):
        plan_batches([0], CAPS, 4)
    with pytest.raises(ValueError):
        plan_batches([10], CAPS, 4, sizes=(2, 1))


def test_a_batch_above_the_arena_budget_is_planned_again_at_the_next_size():
    """Enhancer._fit_plan with the device question (_fits) answered by a stub: (cap 1024, B 16) does not fit, so the 32 files of
    the two 1024-frame groups run in groups of 4; everything else keeps the plan of plan_batches"""
    frames = bench_frames()
    enh = Enhancer(eabnet_amd.EaBNet(M=2), max_batch=16)
    asked = []
    enh._fits = lambda cap, size, F, device: asked.append((cap, size)) or not (cap == 1024 and size == 16)
    plan = enh._fit_plan(frames, CAPS, 161, None)
    assert sorted(i for b in plan for i in b.indices) == list(range(50))
    assert all(b.batch_size == 4 and len(b.indices) == 4 for b in plan[:8])
    assert [(len(b.indices), b.cap, b.batch_size) for b in plan[8:]] == [(16, 512, 16), (2, 256, 4)]
    for b in plan[:8]:
        assert b.cap == mdl.bucket_for(frames[b.indices[0]], CAPS)
    assert [frames[i] for b in plan for i in b.indices] == sorted(frames, reverse=True)
    assert (1024, 16) in asked and (1024, 4) in asked
    # nothing fits: every file alone (batch size 1 is never refused)
    enh._fits = lambda cap, size, F, device: False
    plan = enh._fit_plan(frames[:5], CAPS, 161, None)
    assert [(len(b.indices), b.batch_size) for b in plan] == [(1, 1)] * 5


@pytest.mark.parametrize("lengths", [[400.5, 800], [400], [400, 800, 800], [160, 800], [400, 801], torch.tensor([400.0, 800.0]),
                                     torch.tensor([[400, 800]]), torch.tensor([True, False]), [True, 800], ["400", 800]])
def test_stft_lengths_validation_comes_before_the_device(lengths):
    """host tensors: the ValueError fires before the 'needs a CUDA tensor' refusal"""
    with pytest.raises(ValueError):
        eabnet_amd.stft_compress(torch.zeros(2, 4, 800), 320, 160, torch.hann_window(320), lengths=lengths)


@pytest.mark.parametrize("lengths", [[1, 9], [2, 10], [2.5, 9], [9], torch.tensor([2.0, 9.0]), torch.tensor([2, 9, 9])])
def test_istft_lengths_validation_comes_before_the_device(lengths):
    with pytest.raises(ValueError):
        eabnet_amd.istft(torch.zeros(2, 2, 9, 161), 320, 160, torch.hann_window(320), lengths=lengths)


def test_valid_lengths_reach_the_device_check_and_none_is_todays_path():
    for kw in ({}, {"lengths": None}, {"lengths": [161, 800]}, {"lengths": torch.tensor([400, 800])}):
        with pytest.raises(eabnet_amd._lib.EabError):
            eabnet_amd.stft_compress(torch.zeros(2, 4, 800), 320, 160, torch.hann_window(320), **kw)
    for kw in ({}, {"lengths": [2, 9]}, {"lengths": np.array([5, 6])}):
        with pytest.raises(eabnet_amd._lib.EabError):
            eabnet_amd.istft(torch.zeros(2, 2, 9, 161), 320, 160, torch.hann_window(320), **kw)
    # the networks' forward keeps its own validation (whole numbers were never required of a sequence there)
    assert mdl.check_lengths([3.0, 4], 2, 10) == [3, 4]


def test_enhancer_refusals_without_a_device():
    net = eabnet_amd.EaBNet(M=2).eval()
    with pytest.raises(TypeError):
        Enhancer(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError):
        Enhancer(net, max_batch=0)
    enh = Enhancer(net)
    assert enh.sizes == (16, 4, 1) and enh.last_plan is None
    assert enh([]) == [] and enh.last_plan["batches"] == []
    with pytest.raises(ValueError):
        enh([torch.zeros(2, 160)])                         # not longer than fft_num / 2
    with pytest.raises(ValueError):
        enh([torch.zeros(2, 4000), torch.zeros(3, 4000)])  # one microphone count per call
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        enh([torch.zeros(2, 4000)])                        # the model is on the CPU
    with pytest.raises(RuntimeError, match="eval"):
        Enhancer(eabnet_amd.EaBNet(M=2).train())([torch.zeros(2, 4000)])
    assert net.length_buckets is None


def test_new_entry_points_are_declared_bound_and_exported():
    from eabnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "eabnet_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("eab_stft_compress_lens_f32", "eab_istft_lens_f32"):
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 10 and "#define EAB_ABI_VERSION 10" in header
    lib = _lib.load()
    # argument checks happen on the host, before any launch
    assert lib.eab_stft_compress_lens_f32(None, None, None, None, None, 1, 1, 1000, 320, 160, 0, None) == 1
    assert lib.eab_istft_lens_f32(None, None, None, None, None, 1, 9, 320, 160, None) == 1
