"""Per-utterance lengths on the MI355X: a padded batch with ``lengths=`` against one-at-a-time exact-shape calls, the
length-bucketed program cache, the two-stage model and the three precisions.  Small shapes (M 4, B <= 3, T <= 300)."""
import argparse

import numpy as np
import pytest
import torch

import paramgen
from util import torch_params

pytestmark = pytest.mark.gpu

LENS = [200, 137, 61]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _net(dev, seed=3, precision="f32", **kw):
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=4, **kw)
    net.load_state_dict(torch_params(4, seed, **kw), strict=True)
    net = net.to(dev).eval()
    net.precision = precision
    return net


def _input(B, T, seed=11):
    return torch.from_numpy(paramgen.make_spec_input(B, T, 161, 4, seed))


def _one_at_a_time(net, x, lens):
    """exact-shape calls on x[b:b+1, :len[b]] -> list of (2, len, F)"""
    out = []
    with torch.no_grad():
        for b, n in enumerate(lens):
            out.append(net(x[b:b + 1, :n].contiguous())[0])
    return out


def _check(y, refs, lens, tol, exact=False, what=""):
    for b, n in enumerate(lens):
        ref = refs[b]
        got = y[b, :, :n]
        if exact:
            assert torch.equal(got, ref), f"{what} utterance {b}: max diff {float((got - ref).abs().max()):.3e}"
        else:
            err = float((got - ref).abs().max() / ref.abs().max())
            assert err <= tol, f"{what} utterance {b} (len {n}): {err:.3e} > {tol:.1e}"
        assert torch.equal(y[b, :, n:], torch.zeros_like(y[b, :, n:])), f"{what} utterance {b}: padding frames not zero"


def test_default_configuration_mixed_lengths_vs_exact_shape_and_oracle(dev):
    """IN, U2, LSTM, MIMO, causal: B = 3 with mixed lengths against one-at-a-time exact-shape calls (the InstanceNorm partials
    of the padded program merge in a different tile set: 1e-5 of the output's range), one utterance against the oracle."""
    from oracle import eabnet_oracle as orc
    net = _net(dev)
    x = _input(3, max(LENS))
    with torch.no_grad():
        y = net(x.to(dev), lengths=LENS).cpu()
    assert y.shape == (3, 2, max(LENS), 161)
    _check(y, [r.cpu() for r in _one_at_a_time(net, x.to(dev), LENS)], LENS, 1e-5, what="IN")
    P = torch_params(4, 3)
    n = LENS[2]
    want = orc.eabnet_forward(P, x[2:3, :n], fast_lstm=True)[0]
    err = float((y[2, :, :n] - want).abs().max() / want.abs().max())
    assert err < 1e-4, f"utterance 2 vs oracle: {err:.3e}"


@pytest.mark.parametrize("norm", ["BN", "cLN"])
def test_bn_eval_and_cln_equal_the_exact_shape_calls_bit_for_bit(dev, norm, monkeypatch):
    """No data-dependent statistic over time: the padded program computes every valid frame exactly as the exact-shape
    program does -- provided both run the same kernels.  Kernel and tile choices follow (B, T) by design (the small-tile and
    the wide-tile convolution kernels sum in different orders), so they are pinned to one choice here."""
    monkeypatch.setenv("EAB_ST", "0")
    monkeypatch.setenv("EAB_BM", "64")
    net = _net(dev, seed=5, norm_type=norm)
    x = _input(3, max(LENS), seed=12).to(dev)
    with torch.no_grad():
        y = net(x, lengths=LENS)
    _check(y, _one_at_a_time(net, x, LENS), LENS, 0.0, exact=True, what=norm)


def test_nan_in_the_padding_stays_out_of_the_valid_frames(dev):
    net = _net(dev, seed=7)
    x = _input(3, max(LENS), seed=13).to(dev)
    for b, n in enumerate(LENS):
        x[b, n:] = 0.0
    xn = x.clone()
    for b, n in enumerate(LENS):
        xn[b, n:] = float("nan")
    with torch.no_grad():
        y0 = net(x, lengths=LENS)
        y1 = net(xn, lengths=LENS)
    assert torch.equal(y0, y1), "NaN in the padding reached the output (valid frames or the zero padding)"


def test_length_buckets_serve_six_lengths_from_one_lowering(dev, monkeypatch):
    from eabnet_amd import program as prg
    net = _net(dev, seed=9)
    Ts = [257, 300, 280, 311, 399, 512]
    x = _input(2, max(Ts), seed=14).to(dev)
    with torch.no_grad():
        refs = [net(x[:, :T].contiguous()) for T in Ts]
    calls = []
    real = prg.lower
    monkeypatch.setattr(prg, "lower", lambda *a, **k: calls.append(a[3]) or real(*a, **k))
    net.length_buckets = "auto"
    with torch.no_grad():
        outs = [net(x[:, :T].contiguous()) for T in Ts]
    assert calls == [512], f"lower() calls: {calls}"
    for T, y, ref in zip(Ts, outs, refs):
        assert y.shape == ref.shape == (2, 2, T, 161)
        err = float((y - ref).abs().max() / ref.abs().max())
        assert err <= 1e-5, f"T = {T}: {err:.3e}"
    (key, nbytes), = net.varlen_arena_bytes().items()
    assert key[:2] == (2, 512) and nbytes > 0
    net.length_buckets = None
    with torch.no_grad():
        assert torch.equal(net(x[:, :Ts[0]].contiguous()), refs[0])    # back on the exact-shape path


def _two_stage_args():
    return argparse.Namespace(
        k1=(2, 3), k2=(1, 3), c=64, M=4, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=1, q=1, is_causal=True, is_u2=True,
        bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="IN", ref_mic=0, freeze_eabnet=False,
        gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=1,
        gagnet_q=2, gagnet_dilas=[1, 2], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=True,
        gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="IN")


def test_two_stage_model_with_lengths_vs_one_at_a_time(dev):
    import eabnet_amd
    torch.manual_seed(0)
    net = eabnet_amd.make_eabnet_with_postnet(_two_stage_args()).to(dev).eval()
    with torch.no_grad():
        for p in net.parameters():                       # off the default initialisation, deterministic
            p.add_(0.02 * torch.randn_like(p))
    lens = [150, 97]
    x = _input(2, max(lens), seed=15).to(dev)
    with torch.no_grad():
        out = net(x, lengths=lens)
        for b, n in enumerate(lens):
            ref = net(x[b:b + 1, :n].contiguous())
            for key in ("esti0_stft", "esti_stft"):
                got, want = out[key][b, :, :n], ref[key][0]
                err = float((got - want).abs().max() / want.abs().max())
                assert err <= 1e-5, f"{key} utterance {b}: {err:.3e}"
                assert torch.equal(out[key][b, :, n:], torch.zeros_like(out[key][b, :, n:]))
            for j, est in enumerate(out["esti1_stft_list"]):
                want = ref["esti1_stft_list"][j][0]
                err = float((est[b, :, :, :n] - want).abs().max() / want.abs().max())
                assert err <= 1e-5, f"stage {j} utterance {b}: {err:.3e}"


@pytest.mark.parametrize("precision,tol", [("f16x3", 1e-4), ("bf16", 5e-2)])
def test_reduced_precisions_with_lengths_vs_exact_shape(dev, precision, tol):
    net = _net(dev, seed=4, precision=precision)
    lens = [180, 75]
    x = _input(2, max(lens), seed=16).to(dev)
    with torch.no_grad():
        y = net(x, lengths=lens)
    _check(y, _one_at_a_time(net, x, lens), lens, tol, what=precision)


def test_refusals_on_the_device(dev):
    net = _net(dev)
    x = _input(1, 40).to(dev)
    with pytest.raises(NotImplementedError, match="lengths"):
        net(x, lengths=[20])                              # parameters require grad, grad enabled: a training call
    bn = _net(dev, norm_type="BN").train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="lengths"):
        bn(x, lengths=[20])
    nc = _net(dev, is_causal=False)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="is_causal=True"):
        nc(x, lengths=[20])
    nc.length_buckets = "auto"                            # quietly the exact-shape path
    with torch.no_grad():
        ref = nc(x)
        assert not nc._varlen_bound and ref.shape == (1, 2, 40, 161)
    with torch.no_grad(), pytest.raises(ValueError):
        net(x, lengths=[41])
