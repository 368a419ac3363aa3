"""Streams of any length on the MI355X: ``stream_begin(..., endless=True)`` keeps a resident window of T_max frames and
moves the rows later steps can still read to its front when it reaches the end (eab_shift_rows_f32).  The frames it returns
are, bit for bit, those of the plain stream and of one offline call on everything pushed since reset().  The window and the
long programs pick the same kernels for every shape used here (tests/test_endless_lowering.py), which is why equality of
bits may be demanded."""
import ctypes as C
import re

import pytest
import torch

import paramgen
from util import TOL_HIP, assert_close, torch_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _model(M, seed, dev, **kw):
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=M, **kw)
    net.load_state_dict(torch_params(M, seed, **kw), strict=True)
    return net.to(dev).eval()


def _run(st, x, chunk):
    return torch.cat([st.step(x[:, t:t + chunk]) for t in range(0, x.shape[1], chunk)], dim=2)


def test_shift_rows_moves_exactly_the_listed_rows(dev):
    """the entry point on its own: three tensors (16-byte rows, 8-byte rows of an odd microphone count, more rows asked
    for than H), two utterances; everything outside the destination rows stays as it was"""
    from eabnet_amd import _lib
    lib = _lib.load()
    B, T, H, src = 2, 23, 5, 19
    shapes = [(64, 5), (322, 1), (8, 9)]                       # (floats per row, rows)
    tens = [torch.randn(B, T, row, device=dev) for row, _ in shapes]
    want = []
    for t, (row, rows) in zip(tens, shapes):
        h = min(rows, H)
        w = t.clone()
        w[:, H - h:H] = t[:, src - h:src]
        want.append(w)
    descs = (_lib.ShiftDesc * 3)()
    for d, t, (row, rows) in zip(descs, tens, shapes):
        d.ptr, d.row_floats, d.rows = t.data_ptr(), row, rows
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    rc = lib.eab_shift_rows_f32(table.data_ptr(), 3, B, T, src, H, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for t, w in zip(tens, want):
        assert torch.equal(t, w)


@pytest.mark.parametrize("chunk", [1, 4])
@pytest.mark.parametrize("norm,precision", [("BN", "f32"), ("cLN", "f32"), ("BN", "bf16")])
def test_endless_equals_plain_stream_and_offline(dev, norm, precision, chunk):
    """B = 2, M = 4, p = q = 2 (history 8), the smallest window, more than ten windows and (chunk 4) a short final chunk.
    cLN: the count of the cumulative statistics is carried with the sums, not taken from the row index."""
    B, M = 2, 4
    net = _model(M, 3100, dev, norm_type=norm, p=2, q=2)
    net.precision = precision
    window = 2 * 8 + chunk
    N = 10 * window + 3
    assert N % chunk == (0 if chunk == 1 else 3)
    x = torch.from_numpy(paramgen.make_spec_input(B, N, 161, M, 3101)).to(dev)
    st = net.stream_begin(B, T_max=window, chunk=chunk, endless=True)
    assert st.endless and st.history == 8 and st.T_max == window
    got = _run(st, x, chunk)
    assert st.pos <= window
    plain = _run(net.stream_begin(B, T_max=N, chunk=chunk), x, chunk)
    assert got.shape == plain.shape == (B, 2, N, 161)
    assert torch.isfinite(got).all()
    differ = (got != plain).any(dim=3).any(dim=1).any(dim=0).nonzero().flatten().tolist()
    assert not differ, f"{norm} {precision} chunk {chunk}: frames that differ from the plain stream: {differ[:8]} ..."
    assert torch.equal(got, plain)
    if precision == "f32":
        with torch.no_grad():
            off = net(x)
        assert torch.equal(got, off)
    if chunk == 4:                                   # the short final chunk closed the stream, as it does the plain one
        with pytest.raises(RuntimeError, match="reset"):
            st.step(x[:, :chunk])


def test_default_depth_equals_plain_stream_and_matches_the_oracle(dev):
    """p = 6, q = 3: the S-TCM of dilation 32 reads 128 frames back; window 2 * 128 + 1, 700 frames"""
    from oracle import eabnet_oracle as orc
    kw = dict(norm_type="BN")
    M, N = 4, 700
    net = _model(M, 3110, dev, **kw)
    x = torch.from_numpy(paramgen.make_spec_input(1, N, 161, M, 3111))
    xd = x.to(dev)
    st = net.stream_begin(1, T_max=257, chunk=1, endless=True)
    assert st.history == 128
    got = _run(st, xd, 1)
    plain = _run(net.stream_begin(1, T_max=N, chunk=1), xd, 1)
    assert torch.equal(got, plain)
    with torch.no_grad():
        ref = orc.eabnet_forward(torch_params(M, 3110, **kw), x, fast_lstm=True, **kw)
    m, l2 = assert_close(got[:, :, -50:].cpu().numpy(), ref[:, :, -50:].numpy(), TOL_HIP, "last 50 frames of the endless stream vs oracle")
    print(f"endless stream, frames 650..699 vs oracle: max-rel {m:.2e}, l2-rel {l2:.2e}")


def _two_stage(dev):
    import argparse
    import eabnet_amd
    M = 4
    args = argparse.Namespace(
        k1=(2, 3), k2=(1, 3), c=64, M=M, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=1, q=1, is_causal=True, is_u2=True,
        bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="BN", ref_mic=0, freeze_eabnet=False,
        gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=1,
        gagnet_q=1, gagnet_dilas=[1, 2], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=True,
        gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="BN",
        mics=M, sr=16000, wav_len=4.0, win_size=0.020, win_shift=0.010, fft_num=320)
    net = eabnet_amd.make_eabnet_with_postnet(args)
    specs = {**{"eabnet." + k: s for k, s in net.eabnet._specs.items()}, **{"postnet." + k: s for k, s in net.postnet._specs.items()}}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in paramgen.make_params(specs, 3120).items()}, strict=True)
    return net.to(dev).eval()


@pytest.mark.parametrize("chunk", [1, 2])
def test_two_stage_stream_and_wave_enhancer(dev, chunk):
    """EaBNetWithPostNet: both stages move their own rows (history 4 each, window 2 * 4 + chunk, 31 frames = more than three
    windows); all three outputs equal the plain stream, and the enhanced wave equals the offline wave chain."""
    import eabnet_amd
    net = _two_stage(dev)
    M, B, L = 4, 2, 160 * 30
    wav = torch.from_numpy(paramgen.make_wave(B, M, L, 3121)).to(dev)
    win = torch.hann_window(320)
    with torch.no_grad():
        spec = eabnet_amd.stft_compress(wav, 320, 160, win)                     # (B, 31, F, M, 2)
        off_wave = eabnet_amd.istft(net(spec)["esti_stft"], 320, 160, win)
    T = spec.shape[1]
    window = 2 * 4 + chunk
    assert T >= 3 * window
    st = net.stream_begin(B, T_max=window, chunk=chunk, endless=True)
    assert (st.first.history, st.second.history) == (4, 4) and st.first.endless and st.second.endless
    plain = net.stream_begin(B, T_max=T, chunk=chunk)
    assert not plain.first.endless
    a = [st.step(spec[:, t:t + chunk]) for t in range(0, T, chunk)]
    b = [plain.step(spec[:, t:t + chunk]) for t in range(0, T, chunk)]
    for key, dim in (("esti0_stft", 2), ("esti_stft", 2)):
        assert torch.equal(torch.cat([o[key] for o in a], dim=dim), torch.cat([o[key] for o in b], dim=dim)), key
    assert torch.equal(torch.cat([o["esti1_stft_list"][0] for o in a], dim=3), torch.cat([o["esti1_stft_list"][0] for o in b], dim=3))
    # waves in, waves out: `seconds` is the window
    enh = eabnet_amd.StreamingEnhancer(net, B=B, seconds=(window - 0.5) * 160 / 16000, chunk=chunk, endless=True)
    assert enh.T_max == window and enh.stream.first.endless
    step = chunk * 160
    got = torch.cat([enh.push(wav[:, :, s:s + step], last=s + step >= L) for s in range(0, L, step)], dim=1)
    assert got.shape == off_wave.shape == (B, L)
    assert torch.equal(got, off_wave)


def test_reset_after_several_rebases_starts_a_fresh_stream(dev):
    B, M, chunk = 2, 4, 1
    net = _model(M, 3130, dev, norm_type="cLN", p=2, q=2)
    x1 = torch.from_numpy(paramgen.make_spec_input(B, 60, 161, M, 3131)).to(dev)
    x2 = torch.from_numpy(paramgen.make_spec_input(B, 40, 161, M, 3132)).to(dev)
    st = net.stream_begin(B, T_max=17, chunk=chunk, endless=True)
    _run(st, x1, chunk)                               # 60 frames in a window of 17: several moves
    st.reset()
    assert st.pos == 0
    second = _run(st, x2, chunk)
    fresh = _run(net.stream_begin(B, T_max=17, chunk=chunk, endless=True), x2, chunk)
    assert torch.equal(second, fresh)
    assert torch.equal(second, _run(net.stream_begin(B, T_max=40, chunk=chunk), x2, chunk))


def test_window_below_the_minimum_is_refused_before_anything_is_bound(dev, monkeypatch):
    from eabnet_amd import model
    net = _model(4, 3140, dev, norm_type="BN", p=2, q=2)
    made = []
    monkeypatch.setattr(model, "_Bound", lambda *a, **k: made.append(a) or pytest.fail("a program was bound"))
    for chunk, minimum in ((1, 17), (4, 20)):
        with pytest.raises(ValueError, match=rf"at least {minimum}\b") as e:
            net.stream_begin(2, T_max=minimum - 1, chunk=chunk, endless=True)
        assert re.search(r"\b8 frames back", str(e.value))
    assert not made
    big = _model(4, 3141, dev, norm_type="BN")
    with pytest.raises(ValueError, match=r"at least 257\b"):
        big.stream_begin(1, T_max=256, endless=True)
