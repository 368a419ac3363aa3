"""The multi-resolution STFT loss without a GPU: the float64 restatement of tests/mrstft_ref.py against ``torch.stft`` under float64
autograd (so the GPU tests may use the restatement at any shape), the conditions the GPU tests' inputs must satisfy, and every
refusal of ``mr_stft_loss`` and of its C entry points -- raised before a device is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import mrstft_ref as M

CASES = [(M.SMALL, 33), (M.SMALL, 129), (M.SMALL, 257), (M.DEFAULT, 1025), (M.DEFAULT, 4099)]


@pytest.mark.parametrize("res,n", CASES, ids=[f"{'small' if r is M.SMALL else 'default'}-{n}" for r, n in CASES])
@pytest.mark.parametrize("floor", [1e-7, M.GRAD_FLOOR])
def test_restatement_matches_torch_stft_under_float64_autograd(res, n, floor):
    e, s = M.make_signals(n, M.SEEDS[n])
    loss, grad = M.loss_and_grad(e, s, res, 0.7, 1.3, floor)
    leaf = torch.from_numpy(e).double().requires_grad_(True)
    want = M.torch_loss(leaf[None], torch.from_numpy(s).double()[None], None, res, 0.7, 1.3, floor)[0]
    (wgrad,) = torch.autograd.grad(want, leaf)
    assert abs(loss - float(want.detach())) <= 1e-12 * abs(loss)
    assert np.abs(grad - wgrad.numpy()).max() <= 1e-10 * np.abs(grad).max()


def test_restatement_with_lengths_reads_nothing_past_them():
    lens = [257, 33, 129]
    est, clean = torch.full((3, 300), float("nan"), dtype=torch.float64), torch.full((3, 280), float("nan"), dtype=torch.float64)
    pairs = [M.make_signals(n, M.SEEDS[n]) for n in lens]
    for b, (e, s) in enumerate(pairs):
        est[b, :lens[b]], clean[b, :lens[b]] = torch.from_numpy(e).double(), torch.from_numpy(s).double()
    leaf = est.clone().requires_grad_(True)
    want = M.torch_loss(leaf, clean, lens, M.SMALL, floor=M.GRAD_FLOOR)
    (wgrad,) = torch.autograd.grad(want.sum(), leaf)
    for b, (e, s) in enumerate(pairs):
        loss, grad = M.loss_and_grad(e, s, M.SMALL, floor=M.GRAD_FLOOR)
        assert abs(loss - float(want[b].detach())) <= 1e-12 * abs(loss)
        assert np.abs(grad - wgrad[b, :lens[b]].numpy()).max() <= 1e-10 * np.abs(grad).max()
        assert (wgrad[b, lens[b]:] == 0).all()


@pytest.mark.parametrize("n", sorted(M.SEEDS))
def test_inputs_of_the_gpu_tests_are_well_conditioned(n):
    """floor = 0.02: no bin power within 1e-5 relative of the floor (fp32 rounds a power to about 1e-6).  Default floor, default
    resolutions: the fp32 torch restatement itself -- the yardstick of the GPU test -- is at most 1e-4 off on the gradient."""
    res = M.SMALL if n < 1025 else M.DEFAULT
    e, s = M.make_signals(n, M.SEEDS[n])
    margin = M.floor_margin(e, s, res, M.GRAD_FLOOR)
    v2, g2 = M.fp32_restatement_error(e, s, res, M.GRAD_FLOOR)
    v7, g7 = M.fp32_restatement_error(e, s, res, 1e-7)
    print(f"n {n}: floor margin {margin:.1e}; fp32 torch restatement on the CPU: value {v2:.1e}, gradient {g2:.1e} at floor 0.02; "
          f"value {v7:.1e}, gradient {g7:.1e} at floor 1e-7")
    assert margin > 1e-5
    assert v2 <= 1e-6 and v7 <= 1e-6
    assert g7 <= 1e-4


def test_the_silent_stretch_input_is_silent_where_the_gpu_test_expects_zeros():
    e, s = M.make_signals(12517, M.SEEDS[12517])
    e[M.SILENT[0]:M.SILENT[1]] = 0.0
    s[M.SILENT[0]:M.SILENT[1]] = 0.0
    loss, grad = M.loss_and_grad(e, s, M.DEFAULT)
    zero = M.silent_samples(12517, M.DEFAULT, M.SILENT)
    assert np.isfinite(loss) and np.isfinite(grad).all()
    assert zero.sum() > 1000 and (grad[zero] == 0).all() and (grad[~zero] != 0).mean() > 0.99


def test_refusals_come_before_any_device_is_touched():
    import eabnet_amd
    from eabnet_amd import mr_stft_loss
    assert "mr_stft_loss" in eabnet_amd.__all__
    est, clean = torch.zeros(2, 1100), torch.ones(2, 1100)
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        mr_stft_loss(est, clean)
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        mr_stft_loss(est.requires_grad_(True), clean[:, None], lengths=[1025, 1100])
    est = est.detach()
    with pytest.raises(TypeError):
        mr_stft_loss(est.double(), clean)
    with pytest.raises(TypeError):
        mr_stft_loss(est, clean.half())
    with pytest.raises(NotImplementedError):
        mr_stft_loss(est, torch.ones(2, 1100, requires_grad=True))
    for kw in ({"reduction": "max"}, {"floor": 0.0}, {"floor": -1.0}, {"floor": float("nan")}, {"factor_sc": -1.0},
               {"factor_mag": float("inf")}, {"factor_sc": float("nan")}, {"resolutions": ()},
               {"resolutions": ((64, 16, 48),) * 9},                  # more than 8
               {"resolutions": ((63, 16, 48),)},                      # odd n_fft
               {"resolutions": ((6, 2, 6),)}, {"resolutions": ((4096, 1024, 4096),)},
               {"resolutions": ((48, 12, 48),)},                      # 24 = 2^3 3
               {"resolutions": ((64, 0, 48),)}, {"resolutions": ((64, 65, 48),)}, {"resolutions": ((64, 16, 65),)},
               {"resolutions": ((64, 16, 0),)},
               {"resolutions": ((64, 4, 48),)},                       # twelve windows over a sample
               {"resolutions": ((64, 16),)}, {"resolutions": ((64.0, 16, 48),)},
               {"lengths": [1100, 1101]}, {"lengths": [1100, 1024]},  # past the row; not more than max n_fft / 2
               {"lengths": [1100]}, {"lengths": [1100, 1050.5]}, {"lengths": torch.tensor([1100.0, 1100.0])}):
        with pytest.raises(ValueError):
            mr_stft_loss(est, clean, **kw)
    with pytest.raises(ValueError, match="2\\^a 5\\^b"):
        mr_stft_loss(est, clean, resolutions=((48, 12, 48),))
    with pytest.raises(ValueError, match="reflect"):
        mr_stft_loss(est[:, :1024], clean)                            # rows of max n_fft / 2 samples
    with pytest.raises(ValueError):
        mr_stft_loss(est, clean[:1])
    with pytest.raises(ValueError):
        mr_stft_loss(est[0], clean[0])
    # what the default passes: five windows over a sample although ceil(n_fft / hop) = 9
    assert eabnet_amd.wave.check_resolutions(M.DEFAULT) == M.DEFAULT and eabnet_amd.wave.check_resolutions(M.SMALL) == M.SMALL


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    from eabnet_amd import _lib
    lib = _lib.load()
    one = C.addressof(C.c_double(0.0))

    def res(*triples):
        return (C.c_int32 * (3 * len(triples)))(*[v for t in triples for v in t])

    ok = res(*M.SMALL)
    assert lib.eab_mrstft_workspace_bytes(ok, 3, 2, 300, 0) == 2 * (5 + 8 + 4) * 3 * 8       # 19, 31, 13 frames in groups of four
    assert lib.eab_mrstft_workspace_bytes(ok, 3, 2, 300, 1) == 2 * (19 * 48 + 31 * 40 + 13 * 49) * 4
    assert lib.eab_mrstft_workspace_bytes(res(*M.DEFAULT), 3, 1, 1025, 0) > 0
    for bad in (res((48, 12, 48)), res((63, 16, 48)), res((64, 4, 48)), res((64, 65, 48)), res((64, 16, 65)), res((4096, 512, 4096))):
        assert lib.eab_mrstft_workspace_bytes(bad, 1, 2, 300, 0) == -1
    assert lib.eab_mrstft_workspace_bytes(ok, 3, 2, 32, 0) == -1                              # cap = max n_fft / 2
    assert lib.eab_mrstft_workspace_bytes(ok, 0, 2, 300, 0) == -1 and lib.eab_mrstft_workspace_bytes(None, 3, 2, 300, 0) == -1
    assert lib.eab_mrstft_workspace_bytes(res(*([(64, 16, 48)] * 9)), 9, 2, 300, 0) == -1
    fwd = lambda **k: lib.eab_mrstft_loss_f32(k.get("est", one), 300, k.get("cap", 300), one, 300, 300, one, k.get("B", 2),  # noqa: E731
                                              k.get("res", ok), k.get("R", 3), one, k.get("f", 1.0), 1.0, k.get("floor", 1e-7), one,
                                              k.get("bytes", 1 << 20), one, one, one, None)
    assert fwd(est=None) == 1 and fwd(B=0) == 1 and fwd(cap=301) == 1 and fwd(R=9) == 1 and fwd(res=res((48, 12, 48)), R=1) == 1
    assert fwd(f=-1.0) == 1 and fwd(f=float("nan")) == 1 and fwd(floor=0.0) == 1 and fwd(bytes=815) == 1 and fwd(cap=32) == 1
    bwd = lambda **k: lib.eab_mrstft_loss_bwd_f32(one, 300, 300, one, 300, 300, k.get("lens", one), k.get("B", 2), ok, k.get("R", 3), one,  # noqa: E731
                                                  k.get("floor", 0.02), one, one, k.get("gs", 1), 1.0, one, k.get("bytes", 1 << 20), one,
                                                  k.get("stride", 300), None)
    assert bwd(lens=None) == 1 and bwd(B=0) == 1 and bwd(R=0) == 1 and bwd(floor=-1.0) == 1 and bwd(gs=-1) == 1
    assert bwd(bytes=22311) == 1 and bwd(stride=299) == 1
