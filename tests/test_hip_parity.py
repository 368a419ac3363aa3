"""Parity of the HIP path with the oracle / reference fixtures, on a real
MI355X, through the C ABI.  Tolerance: 1e-4 relative fp32 (BASELINE.json
north_star; both max-abs/max and L2-rel, tests/util.py); STFT frame indexing
bit-exact."""
import ctypes as C

import os

import numpy as np
import pytest
import torch

import paramgen
from util import TOL_HIP, assert_close, assert_compressed_close, load, rel_errs, torch_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()                                   # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _model(M, seed, dev, **kw):
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=M, **kw)
    net.load_state_dict(torch_params(M, seed, **kw), strict=True)
    return net.to(dev).eval()


def test_side_streams_overlap_with_the_launch_stream(dev):
    """graphs.side_streams: the streams a program's parallel lanes replay on are picked so that they really run beside the launch
    stream (HIP maps streams onto a few hardware queues in creation order; two streams on one queue run back to back -- the
    post-filter's streamed hop was 2.64 instead of 2.11 ms whenever that happened)."""
    from eabnet_amd import graphs
    if int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) < 3:
        pytest.skip("three streams cannot overlap on fewer than three hardware queues (the lanes still replay correctly: "
                    "profiles/r04_scarce_queues.txt)")
    for _ in range(5):                                   # shift the creation-order lottery a little
        torch.cuda.Stream(device=dev)
    main = torch.cuda.current_stream(dev)
    sides = graphs.side_streams(dev, 2)
    assert len(sides) == 2 and len({s.cuda_stream for s in sides} | {main.cuda_stream}) == 3
    assert graphs.side_streams(dev, 2) == sides, "one set per (device, launch stream) for the whole process"
    alone = min(graphs._overlap(main, main, dev) for _ in range(3)) / 2.0
    pairs = [(main, sides[0]), (main, sides[1]), (sides[0], sides[1])]
    took = [min(graphs._overlap(a, b, dev) for _ in range(3)) for a, b in pairs]
    print(f"spin kernel alone {alone * 1e3:.3f} ms; pairs on (launch, side0), (launch, side1), (side0, side1): "
          + ", ".join(f"{t * 1e3:.3f}" for t in took) + " ms")
    assert all(t < 1.5 * alone for t in took), (alone, took)


# ------------------------------------------------------------------ front end
@pytest.mark.parametrize("B,M,L,n_fft,hop", [(1, 3, 2085, 320, 160), (2, 1, 161, 320, 160), (1, 8, 64000, 320, 160),
                                             (2, 11, 64000, 320, 160), (1, 16, 8004, 320, 160), (2, 5, 4096, 256, 64),
                                             (1, 9, 1003, 256, 64)])
def test_stft_frame_indexing_bit_exact(dev, B, M, L, n_fft, hop):
    """north_star: "bit-exact for STFT frame indexing" (train_distributed.py:83, torch.stft centre / reflect framing).
    eab_stft_frames_f32 runs the PRODUCT kernel (stft_fft_kernel, the instance eab_stft_compress_f32 picks for these sizes)
    compiled to store the rows it gathered instead of transforming them, so both of its gather paths are what is compared:
    the four-samples-per-load path of interior frames (L and n_fft multiples of 4: 64000, 8004, 4096) and the reflected scalar
    path (first / last frame of every utterance; every frame when L % 4 != 0: 2085, 161, 1003); M > 8 takes a second pass
    over the microphones, M = 11 / 9 / 5 / 3 leave a partial pass."""
    from eabnet_amd import _lib
    from oracle import eabnet_oracle as orc
    lib = _lib.load()
    wav = torch.from_numpy(paramgen.make_wave(B, M, L, 40 + M))
    T = 1 + L // hop
    d_w = wav.to(dev)
    frames = torch.full((B, M, T, n_fft), float("nan"), device=dev)
    _lib.check(lib.eab_stft_frames_f32(d_w.data_ptr(), frames.data_ptr(), B, M, L, n_fft, hop, None))
    torch.cuda.synchronize()
    want = orc.stft_frames(wav.reshape(B * M, L), n_fft, hop).reshape(B, M, T, n_fft)
    assert torch.equal(frames.cpu(), want)


@pytest.mark.parametrize("name", ["stft_B1_M2_L1600.npz", "stft_B2_M8_L4000.npz", "stft_B1_M3_L2085.npz",
                                  "stft_zero_mic.npz"])
def test_stft_compress_vs_reference_fixtures(dev, name):
    import eabnet_amd
    g = load(name)
    B, T, F, M, _ = g["noisy"].shape
    L = 1600 if "zero" in name else int(name.split("_L")[1].split(".")[0])
    x = torch.from_numpy(paramgen.make_wave(B, M, L, int(g["seed"])))
    if "zero" in name:
        x[:, 1] = 0.0
    args = type("A", (), dict(mics=M, sr=16000, wav_len=L / 16000, win_size=0.020, win_shift=0.010, fft_num=320))
    noisy, tgt = eabnet_amd.prepare_data(x, x[:, :1], dev, args)
    assert noisy.shape == (B, T, F, M, 2) and tgt.shape == (B, 2, T, F)
    assert_compressed_close(noisy.cpu().numpy(), g["noisy"], TOL_HIP, "noisy")
    if "target" in g.files:
        assert_compressed_close(np.moveaxis(tgt.cpu().numpy(), 1, -1), np.moveaxis(g["target"], 1, -1), TOL_HIP, "target")
    if "zero" in name:
        assert torch.count_nonzero(noisy[..., 1, :]) == 0        # 0 -> exactly 0, no NaN from rsqrt(0)


def test_stft_compress_sixteen_mics_vs_oracle(dev):
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    x = torch.from_numpy(paramgen.make_wave(2, 16, 3200, 41))
    got = eabnet_amd.stft_compress(x.to(dev), 320, 160, torch.hann_window(320)).cpu()
    want, _ = orc.prepare_data_oracle(x, None)
    assert_compressed_close(got.numpy(), want.numpy(), TOL_HIP)


@pytest.mark.parametrize("B,T", [(1, 2), (2, 9), (3, 40)])
def test_istft_vs_reference_fixtures(dev, B, T):
    import eabnet_amd
    g = load(f"istft_B{B}_T{T}.npz")
    esti = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 1, int(g["seed"]))[..., 0, :]).permute(0, 3, 1, 2)
    wav = eabnet_amd.istft(esti.to(dev), 320, 160, torch.hann_window(320))          # non-contiguous input on purpose
    assert wav.shape == (B, 160 * (T - 1))
    assert_close(wav.cpu().numpy(), g["wav"], 1e-5, "istft")


def test_istft_full_size_vs_oracle_and_properties(dev):
    """C2 size (16 x 401 frames): against the oracle, linearity, and 'a frame only reaches the two
    segments it overlaps' (locality of the overlap-add)."""
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    B, T = 16, 401
    win = torch.hann_window(320)
    a = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 1, 50)[..., 0, :]).permute(0, 3, 1, 2).contiguous()
    b = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 1, 51)[..., 0, :]).permute(0, 3, 1, 2).contiguous()
    ya, yb = eabnet_amd.istft(a.to(dev), 320, 160, win), eabnet_amd.istft(b.to(dev), 320, 160, win)
    assert ya.shape == (B, 64000)
    assert_close(ya.cpu().numpy(), orc.istft_oracle(a).numpy(), 1e-5, "istft C2")
    yab = eabnet_amd.istft((2.0 * a - 0.5 * b).to(dev), 320, 160, win)
    assert_close(yab.cpu().numpy(), (2.0 * ya - 0.5 * yb).cpu().numpy(), 1e-5, "linearity")
    c = a.clone()
    c[:, :, 200] += 1.0                                   # perturb one frame
    yc = eabnet_amd.istft(c.to(dev), 320, 160, win)
    changed = (yc != ya).any(0).nonzero().flatten()
    assert changed.min() >= 160 * 199 and changed.max() < 160 * 201
    with pytest.raises(NotImplementedError):              # more than 8 frames over a sample (other hops, dividing fft_num or
        eabnet_amd.istft(a.to(dev), 320, 39, win)         # not: test_istft_other_hops_and_windows_vs_torch)


def test_filter_sum_vs_oracle_and_linearity(dev):
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    g = np.random.default_rng(5)
    for (B, T, F, M) in ((2, 7, 161, 8), (1, 3, 5, 1), (1, 4, 161, 9)):
        w = torch.from_numpy(g.standard_normal((B, T, F, M, 2)).astype(np.float32))
        x = torch.from_numpy(g.standard_normal((B, T, F, M, 2)).astype(np.float32))
        y = eabnet_amd.filter_and_sum(w.to(dev), x.to(dev)).cpu()
        assert_close(y.numpy(), orc.filter_and_sum(w, x).numpy(), 1e-5)
        y2 = eabnet_amd.filter_and_sum((2 * w).to(dev), x.to(dev)).cpu()
        assert_close(y2.numpy(), 2 * y.numpy(), 1e-6)


# ------------------------------------------------------------------ op by op
def _op_errors(op, prev, got, want):
    """Errors of ONE op on the elements it CHANGED (bit comparison of the emulator's arena before and after the op; an
    element the op rewrites with identical bits, such as an in-place accumulate of zero, is not in the set -- it is still
    under the whole-arena assertion), each normalised by the reference's maximum over THOSE elements:
    [(what, error, exact)] -- exact entries must be 0.

    Named exceptions to "one maximum per op", each judged component by component instead (a mixed maximum would hide them):
      * the Welford partials (n, mean, M2, 0) a ConvOp writes for the next InstanceNorm (stats, f2_stats): n and the pad
        must be exact; M2 is normalised by the largest M2 of the op's partials; mean by max(|mean|, sqrt(M2 / n)) of the
        op's partials -- a mean is a difference of sums that is legitimately near zero, its natural scale is the spread
        of the values it averages (the in-kernel merge multiplies it by 1/std, never by 1/mean).
      * the (cumulative mean, rstd) pairs of ClnStatsOp: rstd by its own maximum, the mean by max(|mean|, 1 / rstd), for the
        same reason.
    The outputs proper of a ConvOp (dst, dst_acc, f2_dst), of LstmOp and of BfwOp have no exception."""
    from eabnet_amd import program as prg
    ch = want.view(np.int32) != prev.view(np.int32)
    out = []

    def rel(name, g, w, scale):
        if w.size:
            out.append((name, float(np.abs(g.astype(np.float64) - w).max() / scale) if scale > 0 else float(np.abs(g - w).max()), scale <= 0))
    parts = []
    if op.kind == prg.OP_CONV:
        parts = [(op.stats, (op.B, op.stat_tiles, op.nsets, op.Cout, 4), "stats"),
                 (op.f2_stats, (op.B, op.f2_stat_tiles, op.f2_nsets, op.f2_N, 4), "f2_stats")]
    elif op.kind == prg.OP_CLN_STATS:
        parts = [(op.mr, (op.B, op.T, 2), "mr")]
        for ref, n in ((op.sums, op.B * op.T * 4), (op.state, op.B * 4)):      # fp64 scratch: compared as doubles by the caller
            if ref is not None:
                ch[ref.off:ref.off + n] = False
    for ref, shape, name in parts:
        if ref is None or ref.arena != "a":
            continue
        sl = slice(ref.off, ref.off + int(np.prod(shape)))
        m = ch[sl].reshape(shape).copy()
        g, w = got[sl].reshape(shape), want[sl].reshape(shape).astype(np.float64)
        ch[sl] = False
        if not m.any():
            continue
        if name == "mr":
            sel = m[..., 0] | m[..., 1]
            mean, rstd = w[..., 0][sel], w[..., 1][sel]
            rel("mr.mean", g[..., 0][sel], mean, float(np.maximum(np.abs(mean), 1.0 / rstd).max()))
            rel("mr.rstd", g[..., 1][sel], rstd, float(np.abs(rstd).max()))
            continue
        sel = m.any(-1)
        n, mean, M2 = w[..., 0][sel], w[..., 1][sel], w[..., 2][sel]
        out.append((name + ".n", float(np.abs(g[..., 0][sel] - n).max() + np.abs(g[..., 3][sel]).max()), True))
        live = n > 0
        if live.any():
            rel(name + ".mean", g[..., 1][sel][live], mean[live],
                float(np.maximum(np.abs(mean[live]), np.sqrt(M2[live] / n[live])).max()))
            rel(name + ".M2", g[..., 2][sel][live], M2[live], float(M2[live].max()))
    if ch.any():
        w = want[ch].astype(np.float64)
        rel("output", got[ch], w, float(np.abs(w).max()))
    return out


def _assert_op(k, op, prev, got, want, lim):
    worst = 0.0
    for what, err, exact in _op_errors(op, prev, got, want):
        assert err == 0.0 if exact else err < lim, (f"op {k} {op.name} (kind {op.kind}) {what}: deviates by {err:.3e} relative to the "
                                                    f"maximum over the elements the op wrote (limit {lim:.0e})")
        worst = max(worst, 0.0 if exact else err)
    return worst


@pytest.mark.parametrize("M,B,T,pq,precision", [(8, 1, 12, (6, 3), "f32"), (9, 2, 21, (2, 1), "f32"),
                                                 (16, 1, 9, (1, 1), "f32"), (8, 2, 21, (2, 1), "f16x3"),
                                                 (9, 1, 12, (1, 1), "f16x3"), (8, 2, 21, (2, 1), "bf16")])
def test_every_op_matches_the_emulator(dev, M, B, T, pq, precision):
    """Run the device program one op at a time next to the numpy interpreter of
    the same program (tests/emulator.py, itself pinned to the reference fixtures
    on CPU) and compare the WHOLE workspace after each op: the first diverging
    kernel is named."""
    from eabnet_amd import program as prg
    from eabnet_amd.model import _Bound
    from eabnet_amd.spec import NetConfig, param_specs
    from emulator import Emulator
    p, q = pq
    cfg = NetConfig(M=M, p=p, q=q)
    P = paramgen.make_params(param_specs(cfg), 50 + M)
    x = paramgen.make_spec_input(B, T, 161, M, 60 + M)
    prog = prg.lower(cfg, P, B, T, 161, dump_bfw=True, precision=precision)
    emu = Emulator(prog, x)
    bound = _Bound(prog, dev)
    bound.acts.fill_(float("nan"))
    bound.reset_counters()
    xin = torch.from_numpy(x).to(dev)
    out = torch.full((B, 2, T, 161), float("nan"), device=dev)
    bound.bind(xin.data_ptr(), out.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    worst = worst_op = 0.0
    for k, op in enumerate(prog.ops):
        bound.run(stream, k, 1)
        torch.cuda.synchronize()
        prev = emu.arena["a"].copy()
        emu.step(op)
        got = bound.acts.cpu().numpy()
        want = emu.arena["a"]
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"op {k} {op.name}: wrote a different set of elements"
        m = ~np.isnan(want)
        scale = max(np.abs(want[m]).max(), 1e-20) if m.any() else 1.0
        # compare only what this op may have touched: cheap global check, tight tolerance per op
        err = np.abs(got[m] - want[m]).max() / scale if m.any() else 0.0
        # bf16: an operand one ulp(fp32) apart on the two sides can round to different bf16 values (2^-9 relative)
        lim = 2e-4 if precision != "bf16" else 2e-3
        assert err < lim, f"op {k} {op.name} (kind {op.kind}): workspace deviates by {err:.3e} (relative to max)"
        # ... and per op: the same limit on the elements THIS op wrote, relative to their own maximum (the arena maximum is
        # hundreds of times the LSTM outputs, the beam-forming weights and the norm tables)
        worst_op = max(worst_op, _assert_op(k, op, prev, got, want, lim))
        # keep both sides in lockstep so that errors do not compound across ops
        emu.arena["a"][:] = got
        worst = max(worst, err)
    print(f"worst deviation relative to the arena maximum {worst:.2e}, relative to the op's own maximum {worst_op:.2e}")
    got_out = out.cpu().numpy()
    assert not np.isnan(got_out).any()
    assert_close(got_out, emu.arena["out"].reshape(got_out.shape), TOL_HIP if precision != "bf16" else 2e-3, "out")


# ------------------------------------------------------------------ end to end
def test_e2e_taps_fixture(dev):
    g = load("e2e_M8_B1_T12_taps.npz")
    net = _model(8, int(g["param_seed"]), dev)
    net.dump_bfw = True
    x = torch.from_numpy(paramgen.make_spec_input(1, 12, 161, 8, int(g["input_seed"]))).to(dev)
    with torch.no_grad():
        y = net(x)
    bound = net._last[0]
    names = {"en.0": "en.meta_unet_list.0", "en.3": "en.meta_unet_list.3", "en.4": "en.last_conv",
             "de.0": "de.meta_unet_list.0", "de.3": "de.meta_unet_list.3", "de.4": "de.last_conv"}
    for ref_name, mine in names.items():
        got = bound.view(bound.prog.taps[mine]).permute(0, 3, 1, 2).cpu().numpy()
        assert_close(got, g["tap/" + ref_name], TOL_HIP, ref_name)
    # S-TCM output: reference layout (B, 256, T) with channel c*4+f; here [B][T][f*64+c]
    t0 = bound.view(bound.prog.taps["stcns.0.0"]).reshape(1, 12, 4, 64).permute(0, 3, 2, 1).reshape(1, 256, 12)
    assert_close(t0.cpu().numpy(), g["tap/stcns.0.0"], TOL_HIP, "stcns.0.0")
    for nm in ("rnn1", "rnn2"):
        h = bound.view(bound.prog.taps[f"bf_map.{nm}"]).permute(0, 2, 1, 3).reshape(161, 12, 64)
        assert_close(h.cpu().numpy(), g["tap/" + nm], TOL_HIP, nm)
    assert_close(bound.view(bound.prog.taps["bf_w"]).reshape(1, 12, 161, 8, 2).cpu().numpy(), g["tap/bf_w"], TOL_HIP, "bf_w")
    assert_close(y.cpu().numpy(), g["out"], TOL_HIP, "out")


@pytest.mark.parametrize("M,name,B,T", [(8, "e2e_M8_B2_T20.npz", 2, 20), (9, "e2e_M9_B1_T10.npz", 1, 10),
                                        (1, "e2e_M1_B1_T10.npz", 1, 10)])
def test_e2e_fixtures(dev, M, name, B, T):
    import eabnet_amd
    g = load(name)
    net = _model(M, int(g["param_seed"]), dev)
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, int(g["input_seed"]))).to(dev)
    with torch.no_grad():
        y = net(x)
        if M == 1:
            assert torch.equal(net(x[..., 0, :]), y)                 # 4-D input path (EaBNet.py:93-94)
    assert y.shape == (B, 2, T, 161) and y.dtype == torch.float32
    assert_close(y.cpu().numpy(), g["out"], TOL_HIP)
    if "loss_ragged" in g.files:
        label = torch.from_numpy(paramgen.make_spec_input(2, 20, 161, 1, int(g["label_seed"]))[..., 0, :]).permute(0, 3, 1, 2).to(dev)
        assert abs(float(eabnet_amd.com_mag_mse_loss(y, label, [20, 13])) - float(g["loss_ragged"])) < 1e-4 * float(g["loss_ragged"])


def test_c1_full_size_wave_to_output(dev):
    """BASELINE config C1: one 4-s 8-mic utterance, wave -> STFT -> EaBNet."""
    import eabnet_amd
    g = load("c1_M8_T401.npz")
    net = _model(8, int(g["param_seed"]), dev)
    wav = torch.from_numpy(paramgen.make_wave(1, 8, 64000, int(g["wave_seed"])))
    args = type("A", (), dict(mics=8, sr=16000, wav_len=4.0, win_size=0.020, win_shift=0.010, fft_num=320))
    with torch.no_grad():
        ns, ts = eabnet_amd.prepare_data(wav, wav[:, :1], dev, args)
        y = net(ns)
    assert ns.shape == (1, 401, 161, 8, 2)
    assert_compressed_close(ns[:, g["stft_probe_t"].tolist()].cpu().numpy(), g["stft_probe"], TOL_HIP)
    assert abs(float(torch.linalg.vector_norm(ns.double())) - float(g["stft_l2"])) < 1e-5 * float(g["stft_l2"])
    assert abs(float(torch.linalg.vector_norm(ts.double())) - float(g["target_l2"])) < 1e-5 * float(g["target_l2"])
    m, l2 = assert_close(y.cpu().numpy(), g["out"], TOL_HIP)
    print(f"C1 parity: max-rel {m:.2e}, l2-rel {l2:.2e}")


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_c2_batch16_properties(dev, precision):
    """BASELINE config C2/C3 size (16 x 4 s x 8 mics).  The oracle needs minutes at
    this size, so use what the path guarantees: utterances are independent (IN /
    LN / LSTM are per sample), so (a) slot 0 carries the C1 fixture input and must
    reproduce the reference output, (b) a duplicated utterance gives bit-identical
    rows, (c) results do not depend on what else is in the batch."""
    import eabnet_amd
    g = load("c1_M8_T401.npz")
    net = _model(8, int(g["param_seed"]), dev)
    net.precision = precision
    wav = torch.from_numpy(paramgen.make_wave(16, 8, 64000, 77))
    wav[0] = torch.from_numpy(paramgen.make_wave(1, 8, 64000, int(g["wave_seed"])))[0]
    wav[5] = wav[0]
    with torch.no_grad():
        ns = eabnet_amd.stft_compress(wav.to(dev), 320, 160, torch.hann_window(320))
        y = net(ns)
        y3 = net(ns[3:4].contiguous())
    assert y.shape == (16, 2, 401, 161) and torch.isfinite(y).all()
    assert_close(y[0:1].cpu().numpy(), g["out"], TOL_HIP, "slot 0 vs reference fixture")
    assert torch.equal(y[0], y[5]), "identical utterances must give bit-identical outputs"
    assert_close(y[3:4].cpu().numpy(), y3.cpu().numpy(), 1e-5, "batch independence")


def _variants():
    import json
    import os
    from util import GOLDEN
    with open(os.path.join(GOLDEN, "keys_variants.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("name", sorted(_variants()))
def test_constructor_variants_vs_reference_fixtures(dev, name, precision):
    """Every non-default constructor branch of the reference (EaBNet.py:68-85) on the HIP program,
    against outputs of the reference built with the same keywords."""
    e = _variants()[name]
    g = load(f"var_{name}.npz")
    net = _model(e["M"], int(g["param_seed"]), dev, **e["kwargs"])
    net.precision = precision
    x = torch.from_numpy(paramgen.make_spec_input(2, 20, 161, e["M"], int(g["input_seed"]))).to(dev)
    with torch.no_grad():
        y = net(x)
    assert tuple(y.shape) == tuple(g["out"].shape)
    assert_close(y.cpu().numpy(), g["out"], TOL_HIP, name)


@pytest.mark.parametrize("kw", [dict(norm_type="BN"), dict(intra_connect="add", is_causal=False),
                                dict(is_u2=False, norm_type="BN", bf_type="cnn", is_causal=False)],
                         ids=["bn", "add_noncausal", "unet_bn_cnn_noncausal"])
def test_constructor_variants_moderate_size_vs_oracle(dev, kw):
    """Same branches at a size with several 128-row tiles per utterance, the patch pipeline without
    a statistics epilogue (BN) and S-TCM look-ahead taps longer than a tile (dilation 32, T = 150)."""
    from oracle import eabnet_oracle as orc
    M, B, T = 8, 2, 150
    net = _model(M, 410, dev, **kw)
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, 411))
    with torch.no_grad():
        ref = orc.eabnet_forward(torch_params(M, 410, **kw), x, fast_lstm=True, **kw).numpy()
        for precision in ("f32", "f16x3"):
            net.precision = precision
            assert_close(net(x.to(dev)).cpu().numpy(), ref, TOL_HIP, f"{kw} {precision}")


@pytest.mark.parametrize("name,M,B,T", [("e2e_M8_B2_T20.npz", 8, 2, 20), ("e2e_M9_B1_T10.npz", 9, 1, 10)])
def test_f16x3_e2e_fixtures(dev, name, M, B, T):
    """precision='f16x3' (fp16 hi+lo split on the f16 matrix cores) against the SAME reference
    fixtures and the SAME 1e-4 bar as the exact-fp32 path."""
    g = load(name)
    net = _model(M, int(g["param_seed"]), dev)
    net.precision = "f16x3"
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, int(g["input_seed"]))).to(dev)
    with torch.no_grad():
        y = net(x)
    m, l2 = assert_close(y.cpu().numpy(), g["out"], TOL_HIP)
    print(f"f16x3 {name}: max-rel {m:.2e}, l2-rel {l2:.2e}")


def test_f16x3_c1_full_size(dev):
    import eabnet_amd
    g = load("c1_M8_T401.npz")
    net = _model(8, int(g["param_seed"]), dev)
    net.precision = "f16x3"
    wav = torch.from_numpy(paramgen.make_wave(1, 8, 64000, int(g["wave_seed"])))
    with torch.no_grad():
        ns = eabnet_amd.stft_compress(wav.to(dev), 320, 160, torch.hann_window(320))
        y = net(ns)
        net.precision = "f32"
        y32 = net(ns)
    m, l2 = assert_close(y.cpu().numpy(), g["out"], TOL_HIP)
    m2, _ = rel_errs(y.cpu().numpy(), y32.cpu().numpy())
    print(f"f16x3 C1: max-rel {m:.2e}, l2-rel {l2:.2e} vs reference; {m2:.2e} vs the f32 mode")


def test_moderate_size_vs_oracle(dev):
    """B=2, T=130, 4 mics against the oracle run on the host cores."""
    from oracle import eabnet_oracle as orc
    P = torch_params(4, 91)
    net = _model(4, 91, dev)
    x = torch.from_numpy(paramgen.make_spec_input(2, 130, 161, 4, 92))
    with torch.no_grad():
        y = net(x.to(dev)).cpu()
        ref = orc.eabnet_forward(P, x, fast_lstm=True)
    assert_close(y.numpy(), ref.numpy(), TOL_HIP)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_c5_shape_16_mics_8_seconds_vs_oracle(dev, precision):
    """BASELINE configs[4] shape (16-mic array, 8-s utterance, T = 801), wave -> output, against the
    oracle on the host cores.  (The streaming / bf16 aspects of that config are later rows.)"""
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    P = torch_params(16, 123)
    net = _model(16, 123, dev)
    net.precision = precision
    wav = torch.from_numpy(paramgen.make_wave(1, 16, 128000, 124))
    with torch.no_grad():
        ns = eabnet_amd.stft_compress(wav.to(dev), 320, 160, torch.hann_window(320))
        y = net(ns).cpu()
        ns_ref, _ = orc.prepare_data_oracle(wav, None)
        ref = orc.eabnet_forward(P, ns_ref, fast_lstm=True)
    assert ns.shape == (1, 801, 161, 16, 2)
    assert_compressed_close(ns.cpu().numpy(), ns_ref.numpy(), TOL_HIP)
    m, l2 = assert_close(y.numpy(), ref.numpy(), TOL_HIP)
    print(f"C5 shape {precision}: max-rel {m:.2e}, l2-rel {l2:.2e}")


@pytest.mark.parametrize("L", [161, 319, 480, 800])
def test_shortest_utterances(dev, L):
    """torch.stft(center=True, reflect) needs L > n_fft/2 = 160: L = 161 is the shortest legal wave
    (T = 2 frames).  InstanceNorm over 2-4 frames divides by a vanishing variance, so the reference
    ALGORITHM is ill-conditioned there: its own fp32 and fp64 evaluations differ by 5e-2 at T = 2
    (5.7e-5 at T = 4, 3.5e-6 at T = 11).  The bar is therefore: against the fp64 evaluation, the HIP
    path may not be worse than max(1e-4, 3 x the fp32 reference arithmetic's own error)."""
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    P = torch_params(2, 130)
    net = _model(2, 130, dev)
    wav = torch.from_numpy(paramgen.make_wave(1, 2, L, 131))
    with torch.no_grad():
        ns = eabnet_amd.stft_compress(wav.to(dev), 320, 160, torch.hann_window(320))
        y = net(ns).cpu()
        ns_ref, _ = orc.prepare_data_oracle(wav, None)
        ref32 = orc.eabnet_forward(P, ns_ref)
        ref64 = orc.eabnet_forward({k: v.double() for k, v in P.items()}, ns_ref.double())
    assert y.shape == (1, 2, 1 + L // 160, 161) and torch.isfinite(y).all()
    assert_compressed_close(ns.cpu().numpy(), ns_ref.numpy(), TOL_HIP)
    e_ref = max(rel_errs(ref32.numpy(), ref64.numpy()))
    e_hip = max(rel_errs(y.numpy(), ref64.numpy()))
    assert e_hip <= max(TOL_HIP, 3.0 * e_ref), f"T={1 + L // 160}: HIP {e_hip:.2e} vs fp32 reference arithmetic {e_ref:.2e}"


def test_long_utterance_12_seconds(dev):
    """T = 1201 frames: many tiles per utterance, large per-utterance tensors (offset arithmetic)."""
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    P = torch_params(4, 170)
    net = _model(4, 170, dev)
    wav = torch.from_numpy(paramgen.make_wave(1, 4, 192000, 171))
    with torch.no_grad():
        ns = eabnet_amd.stft_compress(wav.to(dev), 320, 160, torch.hann_window(320))
        y = net(ns).cpu()
        ns_ref, _ = orc.prepare_data_oracle(wav, None)
        ref = orc.eabnet_forward(P, ns_ref, fast_lstm=True)
    assert y.shape == (1, 2, 1201, 161)
    assert_close(y.numpy(), ref.numpy(), TOL_HIP)


def test_input_forms_odd_batch_noncontiguous_float64(dev):
    """forward accepts what the reference accepts: any batch size, non-contiguous views, other float
    dtypes (converted to fp32 for the HIP program, result cast back)."""
    from oracle import eabnet_oracle as orc
    P = torch_params(2, 180)
    net = _model(2, 180, dev)
    x = torch.from_numpy(paramgen.make_spec_input(3, 17, 161, 2, 181))
    with torch.no_grad():
        ref = orc.eabnet_forward(P, x)
        y = net(x.to(dev))
        big = torch.zeros(3, 17, 161, 2, 4)
        big[..., ::2] = x
        y_nc = net(big.to(dev)[..., ::2])                       # strided view
        y64 = net(x.double().to(dev))
    assert_close(y.cpu().numpy(), ref.numpy(), TOL_HIP)
    assert torch.equal(y_nc, y)
    assert y64.dtype == torch.float64 and torch.equal(y64.float(), y)


def test_too_short_wave_is_rejected(dev):
    import eabnet_amd
    from eabnet_amd import _lib
    with pytest.raises(_lib.EabError):
        eabnet_amd.stft_compress(torch.zeros(1, 1, 160, device=dev), 320, 160, torch.hann_window(320))


def test_graph_replay_equals_direct_launches(dev):
    """hipGraph replay of the op program (default) and ~250 direct launches give bit-identical
    outputs; changing the input between replays is honoured (static buffers are refreshed)."""
    net = _model(4, 97, dev)
    x1 = torch.from_numpy(paramgen.make_spec_input(2, 23, 161, 4, 98)).to(dev)
    x2 = torch.from_numpy(paramgen.make_spec_input(2, 23, 161, 4, 99)).to(dev)
    with torch.no_grad():
        net.use_graph = True
        a1, a2, a1b = net(x1).clone(), net(x2).clone(), net(x1).clone()
        assert net._last[0].graph is not None, "graph capture did not engage"
        net.use_graph = False
        b1, b2 = net(x1), net(x2)
    assert torch.equal(a1, b1) and torch.equal(a2, b2) and torch.equal(a1, a1b)
    assert not torch.equal(a1, a2)


def test_graph_replay_on_idle_stream_full_length(dev):
    """Regression: at T = 401 a hipMemsetAsync node inside the captured program was not ordered against
    its neighbours when the graph was replayed on an IDLE stream (the S-TCN running sum was not
    re-zeroed).  Replays separated by synchronisations must equal direct launches bit for bit."""
    net = _model(8, 100, dev)
    x = torch.from_numpy(paramgen.make_spec_input(2, 401, 161, 8, 141)).to(dev)
    with torch.no_grad():
        net.use_graph = False
        ref = net(x).clone()
        torch.cuda.synchronize()
        net.use_graph = True
        for i in range(4):
            y = net(x)
            torch.cuda.synchronize()
            assert net._last[0].graph is not None
            assert torch.equal(y, ref), f"replay {i} deviates from direct launches"


def test_weights_are_repacked_after_update(dev):
    net = _model(2, 95, dev)
    x = torch.from_numpy(paramgen.make_spec_input(1, 8, 161, 2, 96)).to(dev)
    with torch.no_grad():
        y0 = net(x).clone()
        net.get_parameter("bf_map.w_dnn.2.bias").add_(1.0)
        y1 = net(x)
    assert not torch.allclose(y0, y1)


def test_training_forward_matches_hip_inference_and_steps(dev):
    """Differentiable forward (the HIP training programs, eabnet_amd/train.py) == HIP inference forward within the parity
    bar, and one optimiser step of the reference's loop (train_distributed.py:218-230) runs."""
    import eabnet_amd
    net = _model(4, 150, dev)
    x = torch.from_numpy(paramgen.make_spec_input(2, 30, 161, 4, 151)).to(dev)
    label = torch.from_numpy(paramgen.make_spec_input(2, 30, 161, 1, 152)[..., 0, :]).permute(0, 3, 1, 2).to(dev)
    with torch.no_grad():
        y_hip = net(x)
    net.train()
    y_tr = net(x)                                   # grad enabled, parameters require grad
    assert y_tr.requires_grad and net.training_backend == "hip"
    assert_close(y_tr.detach().cpu().numpy(), y_hip.cpu().numpy(), TOL_HIP)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    loss = eabnet_amd.com_mag_mse_loss(y_tr, label, [30, 30])
    loss.backward()
    torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
    opt.step()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    with torch.no_grad():                           # updated weights are re-packed for the HIP program
        y2 = net.eval()(x)
    assert not torch.equal(y2, y_hip) and torch.isfinite(y2).all()


def test_differentiable_calls_outside_the_training_programs_are_refused(dev):
    """One backend: what the HIP training programs do not cover raises instead of running anywhere else -- a gradient
    w.r.t. the input spectrogram, BatchNorm in eval mode under autograd, CPU tensors -- for both networks."""
    import eabnet_amd
    from eabnet_amd import _lib
    net = _model(2, 153, dev).train()
    x = torch.from_numpy(paramgen.make_spec_input(1, 12, 161, 2, 154)).to(dev)
    with pytest.raises(NotImplementedError, match="input requires grad"):
        net(x.clone().requires_grad_(True))
    with pytest.raises(_lib.EabError, match="no CPU fallback"):
        net(x.cpu())
    bn = _model(2, 155, dev, norm_type="BN")        # .eval()
    with pytest.raises(NotImplementedError, match="eval mode"):
        bn(x)
    with torch.no_grad():
        assert torch.isfinite(bn(x)).all()          # inference is what eval mode is for
    gag = eabnet_amd.GaGNet(p=1, q=1, dilas=(1, 2)).to(dev).train()
    a = _planar(1, 12, 156).to(dev)
    with pytest.raises(NotImplementedError, match="requires grad"):
        gag(a, a.clone().requires_grad_(True))
    with pytest.raises(_lib.EabError, match="no CPU fallback"):
        gag(a.cpu(), a.cpu())
    assert not hasattr(net, "use_hip_training")


# ------------------------------------------------------------------ post-filter
def _gag_variants():
    import json
    import os
    from util import GOLDEN
    with open(os.path.join(GOLDEN, "keys_gagnet.json")) as f:
        return json.load(f)


def _gag_model(kw, seed, dev):
    import eabnet_amd
    net = eabnet_amd.GaGNet(**kw)
    P = {k: torch.from_numpy(v) for k, v in paramgen.make_params(eabnet_amd.gag_param_specs(net.cfg), seed).items()}
    net.load_state_dict(P, strict=True)
    return net.to(dev).eval(), P


def _planar(B, T, seed):
    return torch.from_numpy(paramgen.make_spec_input(B, T, 161, 1, seed)[..., 0, :]).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("name", sorted(_gag_variants()))
def test_gagnet_vs_reference_fixtures(dev, name, precision):
    e = _gag_variants()[name]
    g = load(f"gag_{name}.npz")
    net, _ = _gag_model(e["kwargs"], int(g["param_seed"]), dev)
    net.precision = precision
    with torch.no_grad():
        outs = net(_planar(2, 14, int(g["inpt_seed"])).to(dev), _planar(2, 14, int(g["pre_seed"])).to(dev))
    assert len(outs) == net.q
    for j, o in enumerate(outs):
        assert tuple(o.shape) == tuple(g[f"out{j}"].shape)
        assert_close(o.cpu().numpy(), g[f"out{j}"], TOL_HIP, f"{name} stage {j}")


def test_gagnet_c1_size_vs_oracle_and_replay(dev):
    """4-s utterances (T = 401) x 2: several tiles per utterance in every S-TCM, dilation-9 taps crossing
    tile borders; graph replay == direct launches bit for bit; a second call with new inputs re-uses the
    captured graph."""
    from oracle import eabnet_oracle as orc
    net, P = _gag_model({}, 530, dev)
    a, b = _planar(2, 401, 531), _planar(2, 401, 532)
    with torch.no_grad():
        ref = orc.gagnet_forward(P, a, b)
        ref64 = orc.gagnet_forward({k: v.double() for k, v in P.items()}, a.double(), b.double())
        outs = net(a.to(dev), b.to(dev))
        net.use_graph = False
        direct = net(a.to(dev), b.to(dev))
        net.use_graph = True
        again = net(b.to(dev), a.to(dev))
        ref_again = orc.gagnet_forward(P, b, a)
    for j in range(net.q):
        # bar: 1e-4, or 3x the reference's own fp32 rounding error where the net is worse conditioned
        floor = rel_errs(ref[j].numpy(), ref64[j].numpy())[0]
        assert_close(outs[j].cpu().numpy(), ref[j].numpy(), max(TOL_HIP, 3 * floor), f"stage {j}")
        assert torch.equal(outs[j], direct[j])
        assert_close(again[j].cpu().numpy(), ref_again[j].numpy(), max(TOL_HIP, 3 * floor), f"swapped stage {j}")


def _postnet_args(M, **over):
    import argparse
    d = dict(k1=(2, 3), k2=(1, 3), c=64, M=M, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=6, q=3, is_causal=True, is_u2=True,
             bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="IN", ref_mic=0, freeze_eabnet=False,
             gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=2,
             gagnet_q=3, gagnet_dilas=[1, 2, 5, 9], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=True,
             gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="IN",
             mics=M, sr=16000, wav_len=4.0, win_size=0.020, win_shift=0.010, fft_num=320)
    d.update(over)
    return argparse.Namespace(**d)


def test_two_stage_wrapper_vs_reference_fixture(dev):
    """EaBNetWithPostNet on the HIP programs against the reference's two classes composed as
    EaBNet.py:138-148 does.  Stage-wise: the beam-former estimate at 1e-4 against the fixture; the
    post-filter at 1e-4 against the reference semantics ON THE SAME INPUT (the oracle fed with the
    HIP estimate) -- its ~100x amplification of input differences (see test_oracle_golden) would
    otherwise turn the beam-former's 2e-6 into 2e-4; the end-to-end figure is checked at 1e-3."""
    import eabnet_amd
    from eabnet_amd.spec import GagConfig, gag_param_specs
    from oracle import eabnet_oracle as orc
    g = load("postnet_M4_T12.npz")
    net = eabnet_amd.make_eabnet_with_postnet(_postnet_args(4, ref_mic=int(g["ref_mic"])))
    Pe = torch_params(4, int(g["eab_seed"]))
    Pg = {k: torch.from_numpy(v) for k, v in paramgen.make_params(gag_param_specs(GagConfig()), int(g["gag_seed"])).items()}
    net.load_state_dict({**{"eabnet." + k: v for k, v in Pe.items()}, **{"postnet." + k: v for k, v in Pg.items()}}, strict=True)
    net = net.to(dev).eval()
    noisy = torch.from_numpy(paramgen.make_spec_input(1, 12, 161, 4, int(g["input_seed"])))
    with torch.no_grad():
        out = net(noisy.to(dev))
        esti0 = out["esti0_stft"].cpu()
        ref_stages = orc.gagnet_forward(Pg, noisy[..., int(g["ref_mic"]), :].permute(0, 3, 1, 2), esti0)
    assert_close(esti0.numpy(), g["esti0"], TOL_HIP, "esti0")
    for j, o in enumerate(out["esti1_stft_list"]):
        assert_close(o.cpu().numpy(), ref_stages[j].numpy(), TOL_HIP, f"post-filter stage {j} on the same input")
    assert out["esti_stft"].shape == (1, 2, 12, 161)
    assert_close(out["esti_stft"].cpu().numpy(), g["esti"], 1e-3, "end to end")
    assert torch.equal(out["esti_stft"], out["esti1_stft_list"][-1].permute(0, 1, 3, 2))


def test_enhance_pipeline_wave_to_wave(dev):
    """enhance.py:45-62 end to end on the device: wave -> prepare_data -> EaBNetWithPostNet -> istft,
    against the oracle chain fed stage by stage with the device's own intermediate results."""
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    M, L = 8, 16000
    args = _postnet_args(M, p=2, q=1, gagnet_p=1, gagnet_q=2, wav_len=1.0)
    net = eabnet_amd.make_eabnet_with_postnet(args)
    sd = net.state_dict()
    specs = {**{"eabnet." + k: s for k, s in net.eabnet._specs.items()}, **{"postnet." + k: s for k, s in net.postnet._specs.items()}}
    P = {k: torch.from_numpy(v) for k, v in paramgen.make_params(specs, 540).items()}
    assert list(P) == list(sd)
    net.load_state_dict(P, strict=True)
    net = net.to(dev).eval()
    wav = torch.from_numpy(paramgen.make_wave(1, M, L, 541))
    with torch.no_grad():
        noisy, _ = eabnet_amd.prepare_data(wav, wav[:, :1], dev, args)
        out = net(noisy)
        enhanced = eabnet_amd.istft(out["esti_stft"], 320, 160, torch.hann_window(320))
        assert enhanced.shape == (1, L)
        n_cpu = noisy.cpu()
        Pe = {k[7:]: v for k, v in P.items() if k.startswith("eabnet.")}
        Pg = {k[8:]: v for k, v in P.items() if k.startswith("postnet.")}
        assert_close(out["esti0_stft"].cpu().numpy(), orc.eabnet_forward(Pe, n_cpu, p=2, q=1, fast_lstm=True).numpy(), TOL_HIP, "esti0")
        stages = orc.gagnet_forward(Pg, n_cpu[..., 0, :].permute(0, 3, 1, 2), out["esti0_stft"].cpu(), p=1, q=2)
        assert_close(out["esti_stft"].cpu().numpy(), stages[-1].permute(0, 1, 3, 2).numpy(), TOL_HIP, "esti")
        assert_close(enhanced.cpu().numpy(), orc.istft_oracle(out["esti_stft"].cpu()).numpy(), 1e-5, "wave")


def test_config4_two_stage_ddp_bf16_training_step(dev):
    """BASELINE config 4 on one rank: train_distributed.py's loop (:181-230) -- the two-stage model with the
    beam-former frozen, DistributedDataParallel over the RCCL backend, bf16 autocast, stage-wise loss,
    gradient clipping, Adam -- then inference with the updated post-filter on the HIP program."""
    import os
    import torch.distributed as dist
    import eabnet_amd
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_free_port())        # (a fixed port can collide on a shared box)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        args = _postnet_args(4, p=1, q=1, gagnet_p=1, gagnet_q=2, gagnet_dilas=[1, 2], freeze_eabnet=True)
        torch.manual_seed(3)
        net = eabnet_amd.make_eabnet_with_postnet(args).to(dev).train()
        ddp = torch.nn.parallel.DistributedDataParallel(net, device_ids=[dev.index])
        opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=5e-4)
        x = torch.from_numpy(paramgen.make_spec_input(2, 24, 161, 4, 170)).to(dev)
        label = torch.from_numpy(paramgen.make_spec_input(2, 24, 161, 1, 171)[..., 0, :]).permute(0, 3, 2, 1).contiguous().to(dev)
        before = {k: v.clone() for k, v in net.postnet.state_dict().items()}
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = ddp(x)
            loss = eabnet_amd.stagewise_com_mag_mse_loss([o.float() for o in out["esti1_stft_list"]], label, [24, 24])
        assert out["esti0_stft"].dtype == torch.float32 and not out["esti0_stft"].requires_grad   # frozen stage: HIP program
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
        assert torch.isfinite(loss)
        assert all(p.grad is None for p in net.eabnet.parameters())
        assert any(not torch.equal(before[k], v) for k, v in net.postnet.state_dict().items())
        with torch.no_grad():
            y = net.eval()(x)["esti_stft"]
        assert y.shape == (2, 2, 24, 161) and torch.isfinite(y).all()
    finally:
        dist.destroy_process_group()


def test_two_stage_training_reduces_the_loss(dev):
    """train_distributed.py's loop (:214-230) on one fixed batch: 40 Adam steps of the two-stage model, both stages on the HIP
    training programs (hipGraph replay, weights re-packed from the updated parameters every step), must fit the batch --
    every stage's loss goes down, in fp32 and with bf16 products."""
    import eabnet_amd
    args = _postnet_args(4, p=1, q=1, gagnet_p=1, gagnet_q=2, gagnet_dilas=[1, 2])
    x = torch.from_numpy(paramgen.make_spec_input(2, 30, 161, 4, 190)).to(dev)
    label = torch.from_numpy(paramgen.make_spec_input(2, 30, 161, 1, 191)[..., 0, :]).permute(0, 3, 1, 2).contiguous().to(dev)
    for prec in ("f32", "bf16"):
        torch.manual_seed(7)
        net = eabnet_amd.make_eabnet_with_postnet(args).to(dev).train()
        net.eabnet.precision = net.postnet.precision = prec
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        hist = []
        for _ in range(40):
            opt.zero_grad(set_to_none=True)
            losses = eabnet_amd.eabnet_with_postnet_loss(net(x), label, [30, 30])
            losses["final"].backward()
            torch.nn.utils.clip_grad_norm_(net.parameters(), 5.0)
            opt.step()
            hist.append((float(losses["eabnet"].detach()), float(losses["postnet"].detach())))
        assert getattr(net.eabnet, "_train_bound", None) and getattr(net.postnet, "_train_bound", None)
        assert all(np.isfinite(h).all() for h in hist)
        print(f"{prec}: beam-former loss {hist[0][0]:.4f} -> {hist[-1][0]:.4f}, post-filter loss {hist[0][1]:.4f} -> {hist[-1][1]:.4f}")
        assert hist[-1][0] < 0.8 * hist[0][0] and hist[-1][1] < 0.8 * hist[0][1], (prec, hist[0], hist[-1])


def test_two_stage_training_step_with_flat_allreduce(dev):
    """BASELINE configs[3] as train_distributed.py:181-230 drives it: both stages trained, eabnet_with_postnet_loss, one flat
    RCCL all-reduce per stage (single-rank group here): forward and backward of BOTH stages on the HIP training programs, and
    the synchronised gradients equal those of an unsynchronised step."""
    import os
    import torch.distributed as dist
    import eabnet_amd
    from eabnet_amd import train as tr
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_free_port())        # (a fixed port can collide on a shared box)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        args = _postnet_args(4, p=1, q=1, gagnet_p=1, gagnet_q=2, gagnet_dilas=[1, 2])
        x = torch.from_numpy(paramgen.make_spec_input(2, 24, 161, 4, 180)).to(dev)
        label = torch.from_numpy(paramgen.make_spec_input(2, 24, 161, 1, 181)[..., 0, :]).permute(0, 3, 1, 2).contiguous().to(dev)
        grads = {}
        for mode in ("plain", "flat"):
            torch.manual_seed(5)
            net = eabnet_amd.make_eabnet_with_postnet(args).to(dev).train()
            if mode == "flat":
                tr.broadcast_parameters(net)
                tr.enable_flat_allreduce(net.eabnet)
                tr.enable_flat_allreduce(net.postnet)
            out = net(x)
            loss = eabnet_amd.eabnet_with_postnet_loss(out, label, [24, 24])["final"]
            loss.backward()
            assert getattr(net.eabnet, "_train_bound", None) and getattr(net.postnet, "_train_bound", None), \
                "both stages must train on the HIP programs"
            assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
            grads[mode] = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone()
            opt = torch.optim.Adam(net.parameters(), lr=5e-4)
            torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
            opt.step()
            with torch.no_grad():
                y = net.eval()(x)["esti_stft"]
            assert y.shape == (2, 2, 24, 161) and torch.isfinite(y).all()
        rel = float((grads["flat"] - grads["plain"]).norm() / grads["plain"].norm())
        assert rel <= 1e-5, rel                      # (atomics order in the weight gradients)
    finally:
        dist.destroy_process_group()


def test_branch_programs_replay_across_a_process_group_lifetime(dev):
    """The crashing combination of round 3 (hip::Graph::UpdateStreams <- hipGraphLaunch): a post-filter program with parallel
    branches captured BEFORE a process group exists, replayed while it is alive (and after it is gone).  The branches replay
    as separate single-stream hipGraphs now (eabnet_amd/graphs.py), which never enter the runtime's stream assignment; the
    results stay bit-identical to direct single-stream launches, for inference and for a training step."""
    import os
    import torch.distributed as dist
    import eabnet_amd
    from eabnet_amd import graphs
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    torch.manual_seed(11)
    net = eabnet_amd.GaGNet(p=1, q=2, dilas=(1, 2)).to(dev).eval()
    mk = lambda seed: torch.from_numpy(np.ascontiguousarray(                       # noqa: E731
        paramgen.make_spec_input(2, 24, 161, 1, seed)[..., 0, :].transpose(0, 3, 1, 2))).to(dev)
    a, b = mk(801), mk(802)
    with torch.no_grad():
        y0 = [t.clone() for t in net(a, b)]                                        # captured here: no process group yet
    bound = net._last[0]
    assert isinstance(bound.graph, graphs.LaneGraphs) and bound.graph.n_graphs > 1, "branches must be separate graphs"
    assert all(e[0] != graphs.RUN or e[1] in (0, 1, 2) for e in bound.graph.plan)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        t = torch.ones(4, device=dev)
        dist.all_reduce(t)                                                         # the communicator (and its streams) exist
        with torch.no_grad():
            for _ in range(3):
                y1 = net(a, b)
        assert net._last[0] is bound, "the program captured before init_process_group is the one replayed"
        assert all(torch.equal(u, v) for u, v in zip(y0, y1))
        # training programs of the same network: captured while the group is alive, replayed after it is gone
        net.train()
        out = net(a, b)
        sum(o.square().mean() for o in out).backward()
        g_alive = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone()
        assert net.training_backend == "hip" and torch.isfinite(g_alive).all()
    finally:
        dist.destroy_process_group()
    for p in net.parameters():
        p.grad = None
    out = net(a, b)
    sum(o.square().mean() for o in out).backward()
    g_after = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    rel = float((g_after - g_alive).norm() / g_alive.norm())
    assert rel <= 1e-5, rel                                                        # (atomics order in the weight gradients)
    with torch.no_grad():
        y2 = net.eval()(a, b)
    assert all(torch.equal(u, v) for u, v in zip(y0, y2))
    # single-stream reference: the same program without branches
    os.environ["EAB_GRAPH_BRANCHES"] = "0"
    try:
        ref = eabnet_amd.GaGNet(p=1, q=2, dilas=(1, 2)).to(dev).eval()
        ref.load_state_dict(net.state_dict())
        with torch.no_grad():
            y3 = ref(a, b)
        assert ref._last[0].graph.n_graphs == 1
    finally:
        del os.environ["EAB_GRAPH_BRANCHES"]
    assert all(torch.equal(u, v) for u, v in zip(y0, y3))


def _free_port() -> int:
    from eabnet_amd import dist as ed
    return ed.free_port()


# ------------------------------------------------------------------ streaming (BASELINE config 5)
@pytest.mark.parametrize("chunk,use_graph", [(1, True), (7, True), (16, False)])
def test_streaming_equals_offline_bit_for_bit(dev, chunk, use_graph):
    """Frame-synchronous inference with BatchNorm (eval) norms: feeding the utterance chunk by chunk
    (kernels windowed through the device-side frame position, LSTM state carried) returns exactly the
    frames of one offline call, which is pinned to the reference by the var_bn fixture.  T = 45 makes
    the last chunk short for chunk 7 and 16."""
    net = _model(4, 201, dev, norm_type="BN")              # parameters of the var_bn fixture
    net.use_graph = use_graph
    B, T = 2, 45
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 4, 600)).to(dev)
    with torch.no_grad():
        off = net(x)
    st = net.stream_begin(B, T_max=48, chunk=chunk)
    outs = [st.step(x[:, t:t + chunk]) for t in range(0, T, chunk)]
    y = torch.cat(outs, dim=2)
    assert y.shape == off.shape
    assert torch.equal(y, off)
    if T % chunk:
        with pytest.raises(RuntimeError):
            st.step(x[:, :chunk])
    st.reset()                                              # second utterance on the same stream object
    x2 = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 4, 601)).to(dev)
    with torch.no_grad():
        off2 = net(x2)
    y2 = torch.cat([st.step(x2[:, t:t + chunk]) for t in range(0, T, chunk)], dim=2)
    assert torch.equal(y2, off2)


@pytest.mark.parametrize("k1,chunk", [((3, 3), 1), ((5, 3), 4), ((1, 3), 2)])
def test_streaming_with_longer_gated_kernels_equals_offline(dev, k1, chunk):
    """k1 = (k_t, 3) with k_t != 2 (the gated convolutions reach k_t - 1 frames back; k_t = 1: none, and ".conv.weight" keys;
    reference fixtures var_k1_33 / var_k1_53_bn_add / var_k1_13 pin the offline path): a frame-synchronous run returns the frames
    of the offline call bit for bit."""
    net = _model(4, 620, dev, norm_type="BN", k1=k1, p=2, q=2)
    B, T = 2, 23
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 4, 621)).to(dev)
    with torch.no_grad():
        off = net(x)
    st = net.stream_begin(B, T_max=24, chunk=chunk)
    y = torch.cat([st.step(x[:, t:t + chunk]) for t in range(0, T, chunk)], dim=2)
    assert torch.equal(y, off)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_streaming_s_tcn_runs_as_one_chain_launch(dev, precision, monkeypatch):
    """A frame-synchronous step (BatchNorm norms, chunk <= 16) runs the 1-D convolutions of the whole S-TCN as ONE launch
    (conv_st_chain_kernel: one workgroup per utterance walks the descriptors; runtime.fuse_step, bound in model._Bound.bind):
    the chain must engage, cover every S-TCN launch, and give the bits of the separate launches (EAB_ST_CHAIN=0) and of the offline call."""
    from eabnet_amd import program as prg
    B, T, chunk = 2, 32, 8
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 4, 610)).to(dev)

    def run(chain: bool):
        monkeypatch.setenv("EAB_ST_CHAIN", "1" if chain else "0")
        net = _model(4, 201, dev, norm_type="BN", p=3, q=2)
        net.precision = precision
        with torch.no_grad():
            off = net(x)
        st = net.stream_begin(B, T_max=T, chunk=chunk)
        y = torch.cat([st.step(x[:, t:t + chunk]) for t in range(0, T, chunk)], dim=2)
        return off, y, st.bound
    off1, y1, b1 = run(True)
    off0, y0, b0 = run(False)
    assert b1.chains and not b0.chains, "the chain launch did not engage"
    stcn = [k for k, o in enumerate(b1.prog.ops) if o.kind == prg.OP_CONV and o.name.startswith("stcns.")]
    (first, cnt, *_), = b1.chains
    assert first == stcn[0] and cnt == len(stcn) and b1.n_exec == len(b1.prog.ops) - cnt + 1
    assert torch.equal(y1, y0) and torch.equal(y1, off1) and torch.equal(off1, off0)


def test_streaming_cln_units_run_as_one_step_launch(dev, monkeypatch):
    """cLN, one frame per step: every (statistics, apply) pair of the program runs as ONE launch (eab_cln_step_f32;
    runtime.fuse_step), EAB_CLN_STEP=0 keeps the separate launches, and both give the frames of the offline call bit for bit.
    Two utterances: the step kernel runs one workgroup per utterance; twelve frames: the running sums carry something."""
    from eabnet_amd import program as prg
    B, T = 2, 12
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 4, 611)).to(dev)

    def run(fuse: bool):
        monkeypatch.setenv("EAB_CLN_STEP", "1" if fuse else "0")
        net = _model(4, 1240, dev, norm_type="cLN", p=2, q=2)
        with torch.no_grad():
            off = net(x)
        st = net.stream_begin(B, T_max=T, chunk=1)
        y = torch.cat([st.step(x[:, t:t + 1]) for t in range(T)], dim=2)
        return off, y, st.bound
    off1, y1, b1 = run(True)
    off0, y0, b0 = run(False)
    n_stats = sum(op.kind == prg.OP_CLN_STATS for op in b1.prog.ops)
    assert n_stats > 0 and sum(op.kind == prg.OP_CLN_STEP for op, _, _ in b1.fused) == n_stats
    assert len(b1.exec_ops) == len(b1.prog.ops) - n_stats
    assert b0.fused is None and b0.exec_ops is None, "EAB_CLN_STEP=0 runs the program's own array"
    assert torch.equal(y1, y0) and torch.equal(y1, off1) and torch.equal(off1, off0)


def test_rebinding_a_streaming_program_refreshes_the_fused_step(dev):
    """bind() to other boundary buffers re-encodes the fused array and the chain's descriptor table with the per-op array: the
    same step on a second set of buffers writes the same bits there and leaves the first output alone."""
    from eabnet_amd import program as prg
    from eabnet_amd.model import _Bound
    B, T, chunk = 2, 8, 4
    net = _model(4, 201, dev, norm_type="BN", p=2, q=2)
    prog = prg.lower(net.cfg, net._numpy_params(), B, T, 161, chunk=chunk)
    bound = _Bound(prog, dev)
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 4, 612)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for _ in range(2):
        xin, out = x.clone(), torch.full((B, 2, T, 161), float("nan"), device=dev)
        assert bound.bind(xin.data_ptr(), out.data_ptr())
        assert bound.chains, "the chain launch did not engage"
        bound.t_pos.fill_(0)                                # position 0 reads no state
        bound.run(stream)
        torch.cuda.synchronize()
        outs.append((xin, out, out.clone()))
    (_, out1, first1), (_, out2, _) = outs
    assert torch.isfinite(out2[:, :, :chunk]).all() and torch.isnan(out2[:, :, chunk:]).all()
    assert torch.equal(out2[:, :, :chunk], out1[:, :, :chunk])
    assert torch.equal(out1.view(torch.int32), first1.view(torch.int32)), "the second run wrote into the first binding's output"


def test_streaming_variants_and_refusals(dev):
    """cnn head + plain U-Net encoder stream too; InstanceNorm / non-causal / f16x3 are refused."""
    kw = dict(is_u2=False, norm_type="BN", bf_type="cnn")
    net = _model(4, 207, dev, **kw)
    x = torch.from_numpy(paramgen.make_spec_input(1, 21, 161, 4, 602)).to(dev)
    with torch.no_grad():
        off = net(x)
    st = net.stream_begin(1, T_max=21, chunk=3)
    assert torch.equal(torch.cat([st.step(x[:, t:t + 3]) for t in range(0, 21, 3)], dim=2), off)
    with pytest.raises(ValueError):
        st.step(x[:, :3])                                   # past T_max
    with pytest.raises(NotImplementedError):
        _model(4, 1, dev).stream_begin(1, 8)                # InstanceNorm looks at the whole utterance
    with pytest.raises(NotImplementedError):
        _model(4, 1, dev, norm_type="BN", is_causal=False).stream_begin(1, 8)
    net.precision = "f16x3"
    with pytest.raises(NotImplementedError):
        net.stream_begin(1, 8)


def test_post_filter_and_two_stage_streaming_bit_exact(dev):
    """GaGNet / EaBNetWithPostNet with BatchNorm norms: chunked streaming == offline, bit for bit."""
    import eabnet_amd
    args = _postnet_args(4, p=2, q=1, gagnet_p=1, gagnet_q=2, norm_type="BN", gagnet_norm_type="BN")
    net = eabnet_amd.make_eabnet_with_postnet(args)
    specs = {**{"eabnet." + k: s for k, s in net.eabnet._specs.items()}, **{"postnet." + k: s for k, s in net.postnet._specs.items()}}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in paramgen.make_params(specs, 560).items()}, strict=True)
    net = net.to(dev).eval()
    B, T, chunk = 2, 23, 4
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 4, 561)).to(dev)
    with torch.no_grad():
        off = net(x)
    st = net.stream_begin(B, T_max=24, chunk=chunk)
    outs = [st.step(x[:, t:t + chunk]) for t in range(0, T, chunk)]
    assert torch.equal(torch.cat([o["esti0_stft"] for o in outs], dim=2), off["esti0_stft"])
    assert torch.equal(torch.cat([o["esti_stft"] for o in outs], dim=2), off["esti_stft"])
    for j in range(2):
        assert torch.equal(torch.cat([o["esti1_stft_list"][j] for o in outs], dim=3), off["esti1_stft_list"][j])
    with pytest.raises(NotImplementedError):
        eabnet_amd.GaGNet().to(dev).eval().stream_begin(1, 8)          # InstanceNorm post-filter


@pytest.mark.parametrize("chunk", [1, 5])
def test_wave_to_wave_streaming_enhancer_bit_exact(dev, chunk):
    """enhance.py as a real-time loop: pushing `chunk` hops of samples at a time through STFT windows, the
    streamed two-stage model and ISTFT windows returns exactly the offline enhanced wave."""
    import eabnet_amd
    M, L = 4, 160 * 30
    args = _postnet_args(M, p=1, q=1, gagnet_p=1, gagnet_q=1, gagnet_dilas=[1, 2], norm_type="BN", gagnet_norm_type="BN")
    net = eabnet_amd.make_eabnet_with_postnet(args)
    specs = {**{"eabnet." + k: s for k, s in net.eabnet._specs.items()}, **{"postnet." + k: s for k, s in net.postnet._specs.items()}}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in paramgen.make_params(specs, 570).items()}, strict=True)
    net = net.to(dev).eval()
    wav = torch.from_numpy(paramgen.make_wave(2, M, L, 571)).to(dev)
    win = torch.hann_window(320)
    with torch.no_grad():
        off = eabnet_amd.istft(net(eabnet_amd.stft_compress(wav, 320, 160, win))["esti_stft"], 320, 160, win)
    enh = eabnet_amd.StreamingEnhancer(net, B=2, seconds=L / 16000, chunk=chunk)
    step = chunk * 160
    pieces = []
    for a in range(0, L, step):
        pieces.append(enh.push(wav[:, :, a:a + step], last=a + step >= L))
    got = torch.cat(pieces, dim=1)
    assert got.shape == off.shape == (2, L)
    assert torch.equal(got, off)


# ------------------------------------------------------------------ structural properties
def test_causality_with_batchnorm_norms(dev):
    """norm_type='BN' (eval) + is_causal: frames before t0 do not depend on the input from t0 on -- bit for bit
    (the property streaming rests on); with InstanceNorm they do, through the utterance statistics."""
    B, T, t0 = 2, 70, 41
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 4, 700)).to(dev)
    x2 = x.clone()
    x2[:, t0:] = torch.from_numpy(paramgen.make_spec_input(B, T - t0, 161, 4, 701)).to(dev)
    net = _model(4, 702, dev, norm_type="BN")
    with torch.no_grad():
        y, y2 = net(x), net(x2)
    assert torch.equal(y[:, :, :t0], y2[:, :, :t0]) and not torch.equal(y[:, :, t0:], y2[:, :, t0:])
    net_in = _model(4, 702, dev)
    with torch.no_grad():
        z, z2 = net_in(x), net_in(x2)
    assert not torch.equal(z[:, :, :t0], z2[:, :, :t0])


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_batch_permutation_equivariance(dev, precision):
    """Utterances never interact: permuting the batch permutes the outputs bit for bit (tiles never
    straddle utterances, statistics are per utterance, the LSTM state is per sequence)."""
    net = _model(4, 710, dev, p=2, q=2)
    net.precision = precision
    x = torch.from_numpy(paramgen.make_spec_input(5, 37, 161, 4, 711)).to(dev)
    perm = torch.tensor([3, 0, 4, 2, 1], device=dev)
    with torch.no_grad():
        assert torch.equal(net(x[perm]), net(x)[perm])
        assert torch.equal(net(x[1:2]), net(x)[1:2])         # and a batch of one is the same utterance alone


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_configurations_vs_oracle(dev, seed):
    """A seeded sweep over the constructor space (M, p, q, kd1, norm, skips, head, encoder) and over (B, T)."""
    from oracle import eabnet_oracle as orc
    rng = np.random.default_rng(4200 + seed)
    kw = dict(M=int(rng.integers(1, 7)), p=int(rng.integers(1, 4)), q=int(rng.integers(1, 3)), kd1=int(rng.choice([3, 5])),
              norm_type=str(rng.choice(["IN", "BN"])), intra_connect=str(rng.choice(["cat", "add"])),
              bf_type=str(rng.choice(["lstm", "cnn"])), is_u2=bool(rng.integers(0, 2)), is_causal=bool(rng.integers(0, 2)))
    B, T = int(rng.integers(1, 4)), int(rng.integers(3, 90))
    M = kw.pop("M")
    net = _model(M, 4300 + seed, dev, **kw)
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, 4400 + seed))
    okw = {k: v for k, v in kw.items() if k not in ("p", "q", "kd1")}
    with torch.no_grad():
        P = torch_params(M, 4300 + seed, **kw)
        ref = orc.eabnet_forward(P, x, p=kw["p"], q=kw["q"], kd=kw["kd1"], fast_lstm=True, **okw)
        ref64 = orc.eabnet_forward({k: v.double() if v.dtype == torch.float32 else v for k, v in P.items()}, x.double(),
                                   p=kw["p"], q=kw["q"], kd=kw["kd1"], **okw)
        floor = rel_errs(ref.numpy(), ref64.numpy())[0]
        for precision in ("f32", "f16x3"):
            net.precision = precision
            y = net(x.to(dev))
            assert_close(y.cpu().numpy(), ref.numpy(), max(TOL_HIP, 3 * floor), f"{kw} B={B} T={T} {precision}")


# ------------------------------------------------------------------ fused losses (first piece)
def test_fused_loss_value_vs_reference_fixtures(dev):
    """com_mag_mse_loss on the device (one fused pass) against the values the reference's own function
    returned (full and ragged frame lists), and the stage-wise loss against GaGNet.py's."""
    import eabnet_amd
    g = load("e2e_M8_B2_T20.npz")
    esti = torch.from_numpy(g["out"]).to(dev)
    label = torch.from_numpy(paramgen.make_spec_input(2, 20, 161, 1, int(g["label_seed"]))[..., 0, :]).permute(0, 3, 1, 2).to(dev)
    for frames, key in (([20, 20], "loss_full"), ([20, 13], "loss_ragged")):
        v = float(eabnet_amd.com_mag_mse_loss(esti, label, frames))
        assert abs(v - float(g[key])) <= 1e-5 * abs(float(g[key])), (v, float(g[key]))
    gg = load("gag_default.npz")
    outs = [torch.from_numpy(gg[f"out{j}"]).to(dev) for j in range(3)]
    lab = torch.from_numpy(paramgen.make_spec_input(2, 14, 161, 1, 800)[..., 0, :]).permute(0, 3, 2, 1).contiguous().to(dev)
    v = float(eabnet_amd.stagewise_com_mag_mse_loss(outs, lab, [14, 9]))
    assert abs(v - float(gg["stage_loss"])) <= 1e-5 * float(gg["stage_loss"])


def test_fused_loss_gradient_vs_autograd(dev):
    """d loss / d esti from the fused kernel == autograd through the reference's tensor expressions
    (ragged masks, bf16-rounded inputs, an exactly-zero bin), and it composes with upstream autograd."""
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    torch.manual_seed(5)
    e0 = torch.randn(3, 2, 17, 161, device=dev)
    e0[1, :, 4, 7] = 0.0
    lab = torch.randn(3, 2, 17, 161, device=dev)
    frames = [17, 9, 12]
    w = torch.randn(3, 2, 17, 161, device=dev, requires_grad=True)
    loss = eabnet_amd.com_mag_mse_loss(e0 * w, lab, frames)            # upstream op: grads flow through
    loss.backward()
    e_ref = (e0 * w.detach()).cpu().double().requires_grad_(True)
    ref = orc.com_mag_mse_loss(e_ref, lab.cpu().double(), frames)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-5 * float(ref.detach())
    gref = (e_ref.grad * e0.cpu().double())
    gref[torch.isnan(gref)] = 0.0                                      # |e| = 0: the kernel's subgradient is 0
    assert_close(w.grad.cpu().numpy(), gref.numpy(), 1e-5, "d loss / d w")


@pytest.mark.parametrize("depth,front", [(2, False), (3, True)])
def test_pipeline_executor_is_bit_identical_and_ordered(dev, depth, front):
    """eabnet_amd.Pipeline: several batches in flight on separate streams / captured programs return, in
    submission order, exactly what net(x) returns for each batch (different inputs per batch; also after a
    weight update and for the wave front end)."""
    import eabnet_amd
    net = _model(4, 230, dev, p=2, q=1)
    win = torch.hann_window(320)
    if front:
        batches = [torch.from_numpy(paramgen.make_wave(2, 4, 4000, 240 + i)).to(dev) for i in range(5)]
        ref_in = [eabnet_amd.stft_compress(w, 320, 160, win) for w in batches]
    else:
        batches = [torch.from_numpy(paramgen.make_spec_input(2, 19, 161, 4, 240 + i)).to(dev) for i in range(5)]
        ref_in = batches
    with torch.no_grad():
        want = [net(x).clone() for x in ref_in]
    pipe = eabnet_amd.Pipeline(net, depth=depth, front_end=(320, 160, win) if front else None)
    assert pipe.calibrate(batches[0], tries=2, steps=3) > 0.0     # stream choice never changes results
    got = list(pipe.map(batches))
    assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
    with pytest.raises(RuntimeError):
        pipe.collect()
    with torch.no_grad():                                   # parameters change -> every slot re-packs
        net.get_parameter("bf_map.w_dnn.2.bias").add_(0.5)
        want2 = net(ref_in[0]).clone()
    assert not torch.equal(want2, want[0])
    pipe.submit(batches[0])
    assert torch.equal(pipe.collect(), want2)
    if not front:                                           # shapes may change from batch to batch; direct launches too
        net.use_graph = False
        odd = [torch.from_numpy(paramgen.make_spec_input(1 + i % 2, 9 + 3 * i, 161, 4, 290 + i)).to(dev) for i in range(4)]
        with torch.no_grad():
            want3 = [net(x).clone() for x in odd]
        assert all(torch.equal(g, w) for g, w in zip(pipe.map(odd), want3))


@pytest.mark.parametrize("mode", ["front_end", "prepare"])
def test_pipeline_takes_host_waves_and_overlaps_their_upload(dev, mode):
    """Host input pipelining (train_distributed.py:76-77 are two blocking .to(device) calls per step): Pipeline.submit takes
    the waves in HOST memory -- pageable or pinned --, stages them through the pinned ring on the copy stream and runs the
    front end on the slot's stream; results are bit-identical to the blocking calls, in order, and the caller may overwrite its
    buffers as soon as submit returns (more batches than ring slots, so slots are re-used while earlier batches are in flight)."""
    import eabnet_amd
    net = _model(4, 231, dev, p=1, q=1)
    args = type("A", (), dict(mics=4, sr=16000, wav_len=0.5, win_size=0.020, win_shift=0.010, fft_num=320))
    win = torch.hann_window(320)
    waves = [torch.from_numpy(paramgen.make_wave(2, 4, 8000, 700 + i)) for i in range(9)]
    want = []
    with torch.no_grad():
        for w in waves:
            noisy, tgt = eabnet_amd.prepare_data(w, w[:, :1], dev, args)
            want.append((net(noisy).clone(), tgt.clone()))
    pipe = (eabnet_amd.Pipeline(net, depth=3, prepare=args) if mode == "prepare"
            else eabnet_amd.Pipeline(net, depth=3, front_end=(320, 160, win)))
    got = []
    for i, w in enumerate(waves):
        if pipe.outstanding == pipe.depth:
            got.append(pipe.collect())
        buf = w.clone().pin_memory() if i % 2 else w.clone()          # pinned and pageable sources alternate
        tgt = buf[:, :1].clone()
        if mode == "prepare":
            pipe.submit(buf, tgt)
        else:
            pipe.submit(buf)
        buf.fill_(1e6)                                               # the caller recycles its buffers immediately
        tgt.fill_(-1e6)
    while pipe.outstanding:
        got.append(pipe.collect())
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for g, (y, t) in zip(got, want):
        if mode == "prepare":
            assert torch.equal(g[0], y) and torch.equal(g[1], t)
        else:
            assert torch.equal(g, y)
    with pytest.raises(eabnet_amd._lib.EabError):                    # host tensors only where a front end takes them
        eabnet_amd.Pipeline(net, depth=2).submit(torch.zeros(1, 10, 161, 4, 2))


def test_pipeline_executor_two_stage_model(dev):
    """The same executor over EaBNetWithPostNet (dictionary outputs, two programs per replica) and over GaGNet
    (two inputs), f16x3 knob set after construction."""
    import eabnet_amd
    net = eabnet_amd.make_eabnet_with_postnet(_postnet_args(4, p=1, q=1, gagnet_p=1, gagnet_q=2, gagnet_dilas=[1, 2]))
    specs = {**{"eabnet." + k: s for k, s in net.eabnet._specs.items()}, **{"postnet." + k: s for k, s in net.postnet._specs.items()}}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in paramgen.make_params(specs, 250).items()}, strict=True)
    net = net.to(dev).eval()
    pipe = eabnet_amd.Pipeline(net, depth=2)
    net.eabnet.precision = net.postnet.precision = "f16x3"
    xs = [torch.from_numpy(paramgen.make_spec_input(1, 15, 161, 4, 260 + i)).to(dev) for i in range(4)]
    with torch.no_grad():
        want = [{k: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for k, v in net(x).items()} for x in xs]
    for got, w in zip(pipe.map(xs), want):
        assert torch.equal(got["esti_stft"], w["esti_stft"]) and torch.equal(got["esti0_stft"], w["esti0_stft"])
        assert all(torch.equal(a, b) for a, b in zip(got["esti1_stft_list"], w["esti1_stft_list"]))
    gp = eabnet_amd.Pipeline(net.postnet, depth=2)
    pairs = [(_planar(1, 15, 270 + i).to(dev), _planar(1, 15, 280 + i).to(dev)) for i in range(3)]
    with torch.no_grad():
        wg = [[t.clone() for t in net.postnet(a, b)] for a, b in pairs]
    for got, w in zip(gp.map(pairs), wg):
        assert all(torch.equal(a, b) for a, b in zip(got, w))



# ------------------------------------------------------------------ C2 size: nothing stale is ever read
def _c2_batch(dev):
    g = load("c1_M8_T401.npz")
    wav = torch.from_numpy(paramgen.make_wave(16, 8, 64000, 78))
    wav[0] = torch.from_numpy(paramgen.make_wave(1, 8, 64000, int(g["wave_seed"])))[0]
    wav[9] = wav[0]
    return g, wav.to(dev)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_c2_size_nan_poisoned_workspace(dev, precision):
    """B = 16, T = 401 (the bench's shape): with the activation arena, the static boundary buffers and the output
    NaN-filled before a run, the result is finite and bit-identical -- every kernel (tile tails, halo cells,
    statistics partials, LSTM windows) reads only what this run wrote.  Graph replay and direct launches."""
    import eabnet_amd
    g, wav = _c2_batch(dev)
    net = _model(8, int(g["param_seed"]), dev)
    net.precision = precision
    with torch.no_grad():
        ns = eabnet_amd.stft_compress(wav, 320, 160, torch.hann_window(320))
        ref = net(ns).clone()
        bound = net._last[0]
        assert bound.graph is not None
        for _ in range(2):
            bound.acts.fill_(float("nan"))
            bound.reset_counters()
            bound.static_out.fill_(float("nan"))
            bound.static_in.fill_(float("nan"))
            y = net(ns)
            assert torch.isfinite(y).all() and torch.equal(y, ref)
        net.use_graph = False
        y0 = net(ns).clone()
        b2 = net._last[0]
        b2.acts.fill_(float("nan"))
        b2.reset_counters()
        y1 = net(ns)
        assert torch.isfinite(y1).all() and torch.equal(y1, y0) and torch.equal(y0, ref)
    assert_close(ref[0:1].cpu().numpy(), g["out"], TOL_HIP, "slot 0 vs reference fixture")
    assert torch.equal(ref[0], ref[9])


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_c2_size_pipelined_equals_direct_after_other_precision(dev, precision):
    """The round-1 failure mode: a Pipeline of the OTHER precision ran first and was dropped (its arenas went back
    to the allocator, the process-wide slot streams stay), then this precision runs pipelined with two batches in
    flight for many steps, a DIFFERENT batch each step (with one repeated batch a stale read returns the right
    values) -- every collected result must equal the direct call bit for bit.  Root causes found with this test:
    two cross-wave LDS races in lstm64_h3_kernel, and packed-fp32 VALU results going wrong next to another wave's
    f16 MFMAs (csrc/Makefile: -packed-fp32-ops; tools/diag_corun.py isolates kernel pairs)."""
    import eabnet_amd
    g, wav0 = _c2_batch(dev)
    wavs = [wav0] + [torch.from_numpy(paramgen.make_wave(16, 8, 64000, 79 + i)).to(dev) for i in range(2)]
    win = torch.hann_window(320)
    net = _model(8, int(g["param_seed"]), dev)
    other = "f16x3" if precision == "f32" else "f32"
    with torch.no_grad():
        net.precision = other
        p0 = eabnet_amd.Pipeline(net, depth=2, front_end=(320, 160, win))
        p0.calibrate(wav0, tries=2, steps=3)
        for _ in range(3):
            p0.submit(wav0)
            p0.collect()
        p0 = None
        net.precision = precision
        wants = [net(eabnet_amd.stft_compress(w, 320, 160, win)).clone() for w in wavs]
        for use_graph in (True, False):
            net.use_graph = use_graph
            pipe = eabnet_amd.Pipeline(net, depth=2, front_end=(320, 160, win))
            got = []
            for k in range(14):
                if pipe.outstanding == 2:
                    got.append(pipe.collect())
                pipe.submit(wavs[k % 3])
            while pipe.outstanding:
                got.append(pipe.collect())
            torch.cuda.synchronize()
            bad = [(k, int((y != wants[k % 3]).sum())) for k, y in enumerate(got) if not torch.equal(y, wants[k % 3])]
            assert not bad, f"graph={use_graph}: pipelined results (index, wrong values) {bad} of {len(got)} differ from the direct call"
    assert_close(wants[0][0:1].cpu().numpy(), g["out"], TOL_HIP, "slot 0 vs reference fixture")


def test_kernels_are_unaffected_by_co_running_kernels(dev):
    """Kernel pairs on two streams (own programs, own arenas): the victim's output must be bit-identical to its
    solo run while the aggressor loops beside it.  Pairs = every kernel class against the two f16-MFMA-dense
    kernels that exposed the packed-fp32 fault (lstm64_h3_kernel, the f16x3 patch convolution)."""
    from eabnet_amd import program as prg
    from eabnet_amd.model import _Bound
    from eabnet_amd.spec import NetConfig, param_specs
    B, T, M = 16, 401, 8
    cfg = NetConfig(M=M)
    P = paramgen.make_params(param_specs(cfg), 5)

    def make(seed):
        prog = prg.lower(cfg, P, B, T, 161, precision="f16x3")
        bound = _Bound(prog, dev)
        x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, seed)).to(dev)
        out = torch.empty(B, 2, T, 161, device=dev)
        bound.bind(x.data_ptr(), out.data_ptr())
        bound.run(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return bound, x, out

    def region(bound, out, op):
        if op.kind == prg.OP_CONV:
            return bound.acts[op.dst.off:op.dst.off + op.B * op.T * op.Fout * op.Cout]
        if op.kind == prg.OP_LSTM64:
            return bound.acts[op.h_out.off:op.h_out.off + op.B * op.T * op.F * 64]
        if op.kind == prg.OP_NORM_ACT:
            return bound.acts[op.out.off:op.out.off + op.B * op.P * op.C]
        return out.view(-1)

    A, Bq = make(11), make(12)                   # keep the bound inputs / outputs alive: the programs hold raw pointers
    (ba, _, oa), (bb, _, _) = A, Bq
    idx = {op.name: k for k, op in enumerate(ba.prog.ops)}
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    reps = 6
    for v in ("bf_map.w_dnn+fs", "bf_map.rnn2", "de.last_conv.ph0", "en.meta_unet_list.1.enco.0.conv", "de.last_conv",
              "stcns.0.tcm_list.0.lr_conv"):
        for a in ("bf_map.rnn2", "de.last_conv.ph0"):
            reg = region(ba, oa, ba.prog.ops[idx[v]])
            n = min(reg.numel(), 1 << 23)
            ref = reg[:n].clone()
            snaps = torch.empty(reps, n, device=dev)
            torch.cuda.synchronize()
            with torch.cuda.stream(s2):
                for _ in range(reps * 6):
                    bb.run(s2.cuda_stream, idx[a], 1)
            with torch.cuda.stream(s1):
                for r in range(reps):
                    ba.run(s1.cuda_stream, idx[v], 1)
                    snaps[r].copy_(reg[:n])
            torch.cuda.synchronize()
            bad = [(r, int((snaps[r] != ref).sum())) for r in range(reps) if not torch.equal(snaps[r], ref)]
            assert not bad, f"{v} next to {a}: runs (index, wrong values) {bad}"


# ------------------------------------------------------------------ BASELINE configs[4] as stated: streaming at M = 16, T = 801
@pytest.mark.parametrize("chunk", [1, 16])
def test_streaming_config5_size_equals_offline_and_oracle(dev, chunk):
    """16 microphones, 8-s utterance (T = 801), BatchNorm norms: the streamed frames equal one offline call bit
    for bit (chunk 1 = 801 replays; chunk 16 ends in a short chunk), and the offline call matches the oracle."""
    from oracle import eabnet_oracle as orc
    kw = dict(norm_type="BN")
    M, T = 16, 801
    net = _model(M, 1230, dev, **kw)
    x = torch.from_numpy(paramgen.make_spec_input(1, T, 161, M, 1231))
    xd = x.to(dev)
    with torch.no_grad():
        off = net(xd)
    st = net.stream_begin(1, T_max=T, chunk=chunk)
    y = torch.cat([st.step(xd[:, t:t + chunk]) for t in range(0, T, chunk)], dim=2)
    assert torch.equal(y, off)
    if chunk == 16:
        with torch.no_grad():
            ref = orc.eabnet_forward(torch_params(M, 1230, **kw), x, fast_lstm=True, **kw)
        assert_close(off.cpu().numpy(), ref.numpy(), TOL_HIP, "offline BN vs oracle")


def test_two_stage_loss_vs_reference_fixture(dev):
    """eabnet_with_postnet_loss (EaBNet.py:642-650) on the device against the value the reference's own
    function returned on the two-stage fixture's outputs."""
    import eabnet_amd
    g, gl = load("postnet_M4_T12.npz"), load("loss_postnet.npz")
    output = {"esti0_stft": torch.from_numpy(g["esti0"]).to(dev),
              "esti1_stft_list": [torch.from_numpy(g[f"stage{j}"]).to(dev) for j in range(3)]}
    label = torch.from_numpy(paramgen.make_spec_input(1, 12, 161, 1, int(gl["label_seed"]))[..., 0, :]).permute(0, 3, 1, 2).contiguous().to(dev)
    l = eabnet_amd.eabnet_with_postnet_loss(output, label, [12])
    for k in ("eabnet", "postnet", "final"):
        assert abs(float(l[k]) - float(gl[f"full/{k}"])) <= 1e-5 * abs(float(gl[f"full/{k}"])), k


# ------------------------------------------------------------------ training on the HIP programs
def _oracle_grads(P, x, label, frames, dtype=torch.float64, **kw):
    """autograd through the oracle in `dtype`: loss value, d loss / d activation at the oracle's named taps and
    d loss / d parameter for every parameter (all returned in fp64)"""
    from oracle import eabnet_oracle as orc
    Pd = {k: v.to(dtype).requires_grad_(True) for k, v in P.items()}
    taps = {}
    y = orc.eabnet_forward(Pd, x.to(dtype), taps=taps, **kw)
    taps = {k: v for k, v in taps.items() if torch.is_tensor(v) and v.requires_grad}
    for v in taps.values():
        v.retain_grad()
    loss = orc.com_mag_mse_loss(y, label.to(dtype), frames)
    loss.backward()
    return (float(loss.detach()), {k: v.grad.double() for k, v in taps.items() if v.grad is not None},
            {k: v.grad.double() for k, v in Pd.items()})


def _grad_errors(got: dict, ref: dict):
    """global l2-rel over all tensors; per-tensor max-abs error relative to that tensor's largest entry (tensors whose
    whole gradient is below 1e-6 of the largest gradient entry anywhere -- biases in front of an InstanceNorm -- are
    left to the global measure)"""
    num = sum(float(((got[k] - ref[k]) ** 2).sum()) for k in ref)
    den = sum(float((ref[k] ** 2).sum()) for k in ref)
    gmax = max(float(v.abs().max()) for v in ref.values())
    per = {k: float((got[k] - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref if float(ref[k].abs().max()) > 1e-6 * gmax}
    return (num / den) ** 0.5, per


@pytest.mark.parametrize("M,B,T,pq,smooth", [(4, 2, 30, (2, 2), True), (8, 1, 70, (6, 3), True), (4, 2, 30, (2, 2), False),
                                             (8, 1, 70, (6, 3), False), (9, 2, 24, (2, 2), True),       # M = 9: the reference's default
                                             (1, 1, 17, (1, 1), True), (16, 2, 19, (1, 2), True),      # one microphone; config 5's 16
                                             (8, 2, 301, (6, 3), True)])    # three seconds: ~190 row tiles per utterance and layer, split-K
def test_hip_training_gradients_vs_oracle_autograd(dev, M, B, T, pq, smooth):     # weight gradients, the LSTM's long recurrence
    _check_training_gradients(dev, M, B, T, pq, smooth)


@pytest.mark.parametrize("smooth", [True, False])
def test_hip_training_gradients_add_skips_vs_oracle_autograd(dev, smooth):
    """the same for intra_connect="add" (Skip_connect, EaBNet.py:499-500): the HIP training programs materialise the sum"""
    _check_training_gradients(dev, 4, 2, 30, (2, 2), smooth, intra_connect="add")


def test_hip_training_gradients_cnn_head_vs_oracle_autograd(dev):
    """bf_type="cnn" (pointwise head, EaBNet.py:80-81,111-113) on the HIP training programs"""
    _check_training_gradients(dev, 4, 2, 30, (2, 2), True, bf_type="cnn", taps=("bf_w", "de.4", "de.0", "stcns", "en.4", "en.0"))


@pytest.mark.parametrize("M,B,T,pq", [(4, 3, 22, (2, 2)), (8, 2, 40, (6, 3))])
def test_hip_training_batchnorm_train_mode_vs_oracle_autograd(dev, M, B, T, pq):
    """norm_type="BN" with the module in train mode (NormSwitch BN branch, EaBNet.py:677-681 = nn.BatchNorm{1,2}d: batch
    statistics over (B, T[, F]), momentum-0.1 update of the running buffers with the unbiased variance) on the HIP training
    programs: output, every parameter gradient and the updated buffers against fp64 autograd through the oracle.
    PReLU slopes are 1 (smooth network, see _check_training_gradients): the bar is 1e-4 per tensor."""
    import eabnet_amd
    from eabnet_amd.spec import NetConfig, param_specs
    from oracle import eabnet_oracle as orc
    p, q = pq
    kw = dict(p=p, q=q, norm_type="BN")
    P = torch_params(M, 930 + M, **kw)
    specs = param_specs(NetConfig(M=M, **kw))
    for k, sp in specs.items():
        if sp.kind == "prelu":
            P[k] = torch.ones_like(P[k])
    net = eabnet_amd.EaBNet(M=M, **kw)
    net.load_state_dict(P, strict=True)
    net = net.to(dev).train()
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, 940))
    label = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 1, 941)[..., 0, :]).permute(0, 3, 1, 2).contiguous()
    frames = [T] * B
    y = net(x.to(dev))
    assert y.requires_grad and net.training_backend == "hip" and getattr(net, "_train_bound", None), "the HIP path did not engage"
    loss = eabnet_amd.com_mag_mse_loss(y, label.to(dev), frames)
    loss.backward()
    # oracle: fp64, train-mode BatchNorm
    is_param = {k for k, sp in specs.items() if not sp.kind.startswith("bn_")}
    Pd = {k: (v.double().requires_grad_(True) if k in is_param else v.double()) for k, v in P.items()}
    Pd["__bn_updates__"] = {}
    y_ref = orc.eabnet_forward(Pd, x.double(), bn_train=True, **kw)
    ref_loss = orc.com_mag_mse_loss(y_ref, label.double(), frames)
    ref_loss.backward()
    assert_close(y.detach().cpu().numpy(), y_ref.detach().numpy(), 1e-5, "train-mode BatchNorm forward")
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    ref = {k: Pd[k].grad for k in is_param}
    got = {k: net.get_parameter(k).grad.cpu().double() for k in ref}
    assert all(torch.isfinite(g).all() for g in got.values())
    total, per = _grad_errors(got, ref)
    bad = sorted(((e, k) for k, e in per.items() if e > 1e-4), reverse=True)
    print(f"BatchNorm train mode: parameter gradients global l2-rel {total:.2e}, worst tensor {max(per.values()):.2e}")
    assert total <= 1e-4 and not bad, f"global l2-rel {total:.3e}; tensors over 1e-4: {bad[:8]}"
    # running buffers after one step
    upd = Pd["__bn_updates__"]
    assert len(upd) == sum(1 for sp in specs.values() if sp.kind == "bn_mean")
    for k, (rm, rv) in upd.items():
        np.testing.assert_allclose(net.get_buffer(f"{k}.norm.running_mean").cpu().numpy(), rm.numpy(), rtol=2e-5, atol=1e-6, err_msg=k)
        np.testing.assert_allclose(net.get_buffer(f"{k}.norm.running_var").cpu().numpy(), rv.numpy(), rtol=2e-5, atol=1e-6, err_msg=k)
        assert int(net.get_buffer(f"{k}.norm.num_batches_tracked")) == int(P[f"{k}.norm.num_batches_tracked"]) + 1
    # eval mode under autograd is refused (one backend: the training programs implement BatchNorm's train mode)
    net.eval()
    with pytest.raises(NotImplementedError, match="eval mode"):
        net(x.to(dev))


def _train_variants():
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", "keys_variants.json")) as f:
        return {k: v for k, v in json.load(f).items()}


@pytest.mark.parametrize("name", sorted(_train_variants()))
def test_hip_training_of_every_constructor_variant_vs_oracle_autograd(dev, name):
    """Every constructor branch of tests/golden/keys_variants.json (plain U-Net, cnn / miso heads, add skips, BatchNorm --
    in train mode, as the reference's trainer runs it --, non-causal S-TCMs and their combinations) trains on the HIP
    programs: output, loss and every parameter gradient against fp64 autograd through the oracle (smooth network: PReLU
    slopes 1, bar 1e-4 per tensor).  cLN (cumulative LayerNorm: reverse prefix-scan backward, csrc/cln.hip) included."""
    import eabnet_amd
    from eabnet_amd.spec import NetConfig, param_specs
    from oracle import eabnet_oracle as orc
    e = _train_variants()[name]
    kw, M = dict(e["kwargs"], p=2, q=2), e["M"]
    # (B, T) = (3, 21) puts one pre-activation of the head's ReLU (EaBNet.py:594) within fp32 rounding of zero for the "unet"
    # entry: the one flipped derivative is a 1e-3 gradient error on its own (tools/diag_variant_grads.py) -- see
    # _check_training_gradients on smooth instances
    B, T = 3, 20
    P = torch_params(M, 980, **kw)
    specs = param_specs(NetConfig(M=M, **kw))
    for k, sp in specs.items():
        if sp.kind == "prelu":
            P[k] = torch.ones_like(P[k])
    net = eabnet_amd.EaBNet(M=M, **kw)
    net.load_state_dict(P, strict=True)
    net = net.to(dev).train()
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, 981))
    y = net(x.to(dev))
    assert y.requires_grad and net.training_backend == "hip" and getattr(net, "_train_bound", None), "the HIP path did not engage"
    label = torch.from_numpy(np.random.default_rng(982).standard_normal(tuple(y.shape)).astype(np.float32))
    loss = ((y - label.to(dev)) ** 2).mean()
    loss.backward()
    is_param = {k for k, sp in specs.items() if not sp.kind.startswith("bn_")}
    Pd = {k: (v.double().requires_grad_(True) if k in is_param else v.double()) for k, v in P.items()}
    y_ref = orc.eabnet_forward(Pd, x.double(), bn_train=kw.get("norm_type") == "BN", **kw)
    assert tuple(y_ref.shape) == tuple(y.shape)
    ref_loss = ((y_ref - label.double()) ** 2).mean()
    ref_loss.backward()
    assert_close(y.detach().cpu().numpy(), y_ref.detach().numpy(), 1e-5, f"{name}: training forward")
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-5 * abs(float(ref_loss.detach()))
    ref = {k: Pd[k].grad for k in is_param}
    got = {k: net.get_parameter(k).grad.cpu().double() for k in ref}
    assert all(torch.isfinite(g).all() for g in got.values())
    total, per = _grad_errors(got, ref)
    bad = sorted(((err, k) for k, err in per.items() if err > 1e-4), reverse=True)
    print(f"{name}: parameter gradients global l2-rel {total:.2e}, worst tensor {max(per.values()):.2e}")
    assert total <= 1e-4 and not bad, f"global l2-rel {total:.3e}; tensors over 1e-4: {bad[:8]}"


def _check_training_gradients(dev, M, B, T, pq, smooth, taps=None, **extra):
    """net(x) under autograd runs the two HIP training programs (eabnet_amd/train.py): the forward equals the
    inference program's output, and loss.backward() gives every parameter the gradient fp64 autograd through the
    oracle gives.

    smooth=True: every PReLU slope is 1 (those activations have no kink; the one ReLU of the beam-former head, EaBNet.py:594,
    keeps its own: the instances here have no pre-activation within fp32 rounding of zero -- M = 16, B = 3, T = 19 has exactly
    one of 587,328, tools/diag_train_taps.py, and is therefore not in the list), so the gradient is a smooth function of the
    activations and fp32 rounding of the forward cannot flip a derivative: every parameter tensor must agree with fp64
    autograd to 1e-4 (relative to its largest entry) and so must the activation gradients at the oracle's taps.
    smooth=False (random slopes): the reference's OWN fp32 autograd deviates from its fp64 autograd by ~1e-3 on this
    network (PReLU derivative flips amplified through the InstanceNorm chain; measured below with the oracle in
    fp32) -- the HIP gradient must stay within 4x that floor, and exact at the head where no flip has happened yet."""
    import eabnet_amd
    from eabnet_amd.spec import NetConfig, param_specs
    p, q = pq
    kw = dict(p=p, q=q, **extra)
    P = torch_params(M, 910 + M, **kw)
    if smooth:
        for k, sp in param_specs(NetConfig(M=M, **kw)).items():
            if sp.kind == "prelu":
                P[k] = torch.ones_like(P[k])
    net = eabnet_amd.EaBNet(M=M, **kw)
    net.load_state_dict(P, strict=True)
    net = net.to(dev).eval()
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, 920))
    label = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 1, 921)[..., 0, :]).permute(0, 3, 1, 2).contiguous()
    frames = [T] * B
    with torch.no_grad():
        y_inf = net(x.to(dev))
    net.train()
    y = net(x.to(dev))
    assert y.requires_grad and getattr(net, "_train_bound", None), "the HIP training path did not engage"
    assert_close(y.detach().cpu().numpy(), y_inf.cpu().numpy(), 1e-5, "training forward vs inference program")
    loss = eabnet_amd.com_mag_mse_loss(y, label.to(dev), frames)
    loss.backward()
    ref_loss, ref_taps, ref = _oracle_grads(P, x, label, frames, **kw)
    assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss)
    got = {k: net.get_parameter(k).grad.cpu().double() for k in ref}
    assert all(torch.isfinite(g).all() for g in got.values())
    total, per = _grad_errors(got, ref)
    # activation gradients at the oracle's taps (backward order): localises a deviation to a stage
    bound = next(iter(net._train_bound.values()))
    acts = {}
    for name in (taps or ("bf_w", "de.4", "de.3", "de.2", "de.1", "de.0", "stcns", "en.4", "en.3", "en.2", "en.1", "en.0")):
        r, Fv, Cv = bound.prog.grad_taps[name]
        g_ = bound.acts[r.off:r.off + B * T * Fv * Cv].view(B, T, Fv, Cv).cpu().double()
        want = ref_taps[name]
        want = want.reshape(B, T, Fv, -1) if name == "bf_w" else want.permute(0, 2, 3, 1)      # (B,C,T,F) -> (B,T,F,C)
        acts[name] = rel_errs(g_[..., :want.shape[-1]].numpy(), want.numpy())[1]
    print(f"smooth={smooth}: parameter gradients global l2-rel {total:.2e}, worst tensor {max(per.values()):.2e}; activation "
          f"gradients l2-rel {[(n, f'{e:.1e}') for n, e in acts.items()]}")
    if smooth:
        bad = sorted(((e, k) for k, e in per.items() if e > 1e-4), reverse=True)
        act_bar = {n: 1e-4 for n in acts}
        if B * T >= 512:
            # Long utterances: a weight gradient is a sum over B * T * F positions and the LSTM's reverse pass a recurrence over
            # T steps; fp32 accumulation of that many terms leaves more than 1e-4 whatever the arithmetic -- the reference's own
            # fp32 autograd (the oracle in fp32) is the yardstick, per tensor and per tap: not worse than 3 x its error.
            _, taps32, g32 = _oracle_grads(P, x, label, frames, dtype=torch.float32, **kw)
            floor, per32 = _grad_errors(g32, ref)
            acts32 = {n: rel_errs(taps32[n].double().numpy(), ref_taps[n].numpy())[1] for n in acts}
            print(f"fp32 reference arithmetic: global l2-rel {floor:.2e}, worst tensor {max(per32.values()):.2e}; activation "
                  f"gradients l2-rel {[(n, f'{e:.1e}') for n, e in acts32.items()]}")
            bad = [(e, k) for e, k in bad if e > 3.0 * per32.get(k, 0.0)]
            act_bar = {n: max(1e-4, 3.0 * acts32[n]) for n in acts}
            assert total <= max(1e-4, 3.0 * floor)
        assert total <= 1e-4 and not bad, f"global l2-rel {total:.3e}; tensors over 1e-4: {bad[:8]}"
        assert all(acts[n] <= act_bar[n] for n in acts), (acts, act_bar)
    else:
        _, taps32, g32 = _oracle_grads(P, x, label, frames, dtype=torch.float32, **kw)
        floor, _ = _grad_errors(g32, ref)
        print(f"   reference fp32 autograd vs fp64: global l2-rel {floor:.2e}")
        assert total <= max(1e-4, 4.0 * floor), f"global l2-rel {total:.3e} vs the reference's own fp32 floor {floor:.3e}"
        assert acts["bf_w"] <= 1e-4 and acts["de.4"] <= max(1e-4, 4.0 * floor)


@pytest.mark.parametrize("smooth", [True, False])
def test_hip_training_of_the_post_filter_vs_oracle_autograd(dev, smooth):
    """GaGNet(inpt, pre_x) under autograd runs the two HIP training programs of eabnet_amd/train_gag.py: the forward equals
    the inference program's output and loss.backward() (stage-wise loss, GaGNet.py:601-619) gives every parameter the
    gradient fp64 autograd through the oracle gives.  smooth / non-smooth as in the beam-former's test above."""
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    kw = dict(p=1, q=2, dilas=[1, 2])
    net, P = _gag_model(kw, 960, dev)
    if smooth:
        for k, sp in eabnet_amd.gag_param_specs(net.cfg).items():
            if sp.kind == "prelu":
                P[k] = torch.ones_like(P[k])
        net.load_state_dict(P, strict=True)
    B, T = 2, 26
    inpt, pre_x = _planar(B, T, 961), _planar(B, T, 962)
    label = _planar(B, T, 963).permute(0, 1, 3, 2).contiguous()              # (B,2,F,T)
    frames = [T] * B
    with torch.no_grad():
        y_inf = net(inpt.to(dev), pre_x.to(dev))
    net.train()
    outs = net(inpt.to(dev), pre_x.to(dev))
    assert outs[0].requires_grad and getattr(net, "_train_bound", None), "the HIP training path did not engage"
    for a, b in zip(outs, y_inf):
        assert_close(a.detach().cpu().numpy(), b.cpu().numpy(), 1e-5, "training forward vs inference program")
    loss = eabnet_amd.stagewise_com_mag_mse_loss(outs, label.to(dev), frames)
    loss.backward()

    def oracle_grads(dtype):
        Pd = {k: v.to(dtype).requires_grad_(True) for k, v in P.items()}
        lo = orc.stagewise_com_mag_mse_loss(orc.gagnet_forward(Pd, inpt.to(dtype), pre_x.to(dtype), kd1=3, **kw), label.to(dtype), frames)
        lo.backward()
        return float(lo.detach()), {k: v.grad.double() for k, v in Pd.items()}
    ref_loss, ref = oracle_grads(torch.float64)
    assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss)
    got = {k: net.get_parameter(k).grad.cpu().double() for k in ref}
    assert all(torch.isfinite(g).all() for g in got.values())
    total, per = _grad_errors(got, ref)
    print(f"post-filter, smooth={smooth}: parameter gradients global l2-rel {total:.2e}, worst tensor {max(per.values()):.2e}")
    if smooth:
        bad = sorted(((e, k) for k, e in per.items() if e > 1e-4), reverse=True)
        assert total <= 1e-4 and not bad, f"global l2-rel {total:.3e}; tensors over 1e-4: {bad[:8]}"
    else:
        _, g32 = oracle_grads(torch.float32)
        floor, _ = _grad_errors(g32, ref)
        print(f"   reference fp32 autograd vs fp64: global l2-rel {floor:.2e}")
        assert total <= max(1e-4, 4.0 * floor), f"global l2-rel {total:.3e} vs the reference's own fp32 floor {floor:.3e}"


def test_hip_training_of_the_post_filter_batchnorm_train_mode_vs_oracle_autograd(dev):
    """the post-filter with norm_type="BN" in train mode (GaGNet.py's NormSwitch BN branch = nn.BatchNorm{1,2}d) on the HIP
    training programs: outputs, parameter gradients and the updated running buffers against fp64 autograd through the oracle"""
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    kw = dict(p=1, q=2, dilas=[1, 2], norm_type="BN")
    net, P = _gag_model(kw, 970, dev)
    specs = eabnet_amd.gag_param_specs(net.cfg)
    for k, sp in specs.items():
        if sp.kind == "prelu":
            P[k] = torch.ones_like(P[k])
    net.load_state_dict(P, strict=True)
    B, T = 3, 22
    inpt, pre_x = _planar(B, T, 971), _planar(B, T, 972)
    label = _planar(B, T, 973).permute(0, 1, 3, 2).contiguous()              # (B,2,F,T)
    frames = [T] * B
    net.train()
    outs = net(inpt.to(dev), pre_x.to(dev))
    assert outs[0].requires_grad and net.training_backend == "hip" and getattr(net, "_train_bound", None)
    loss = eabnet_amd.stagewise_com_mag_mse_loss(outs, label.to(dev), frames)
    loss.backward()
    is_param = {k for k, sp in specs.items() if not sp.kind.startswith("bn_")}
    Pd = {k: (v.double().requires_grad_(True) if k in is_param else v.double()) for k, v in P.items()}
    Pd["__bn_updates__"] = {}
    ref_outs = orc.gagnet_forward(Pd, inpt.double(), pre_x.double(), kd1=3, bn_train=True, **kw)
    lo = orc.stagewise_com_mag_mse_loss(ref_outs, label.double(), frames)
    lo.backward()
    for a, b in zip(outs, ref_outs):
        assert_close(a.detach().cpu().numpy(), b.detach().numpy(), 1e-5, "train-mode BatchNorm forward (post-filter)")
    assert abs(float(loss) - float(lo)) <= 1e-5 * abs(float(lo))
    ref = {k: Pd[k].grad for k in is_param}
    got = {k: net.get_parameter(k).grad.cpu().double() for k in ref}
    total, per = _grad_errors(got, ref)
    bad = sorted(((e, k) for k, e in per.items() if e > 1e-4), reverse=True)
    print(f"post-filter, BatchNorm train mode: parameter gradients global l2-rel {total:.2e}, worst tensor {max(per.values()):.2e}")
    assert total <= 1e-4 and not bad, f"global l2-rel {total:.3e}; tensors over 1e-4: {bad[:8]}"
    upd = Pd["__bn_updates__"]
    assert len(upd) == sum(1 for sp in specs.values() if sp.kind == "bn_mean")
    for k, (rm, rv) in upd.items():
        np.testing.assert_allclose(net.get_buffer(f"{k}.norm.running_mean").cpu().numpy(), rm.numpy(), rtol=2e-5, atol=1e-6, err_msg=k)
        np.testing.assert_allclose(net.get_buffer(f"{k}.norm.running_var").cpu().numpy(), rv.numpy(), rtol=2e-5, atol=1e-6, err_msg=k)


@pytest.mark.parametrize("name", sorted(_gag_variants()))
def test_hip_training_of_every_post_filter_variant_vs_oracle_autograd(dev, name):
    """Every GaGNet constructor variant of tests/golden/keys_gagnet.json (BatchNorm -- train mode --, squeezed gaze block, tanh /
    relu gain, plain U-Net encoder, add skips, non-causal S-TCMs) trains on the HIP programs: stage outputs, loss and parameter
    gradients against fp64 autograd through the oracle (smooth network, 1e-4 per tensor)."""
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    kw = dict(_gag_variants()[name]["kwargs"])
    if name == "default":
        kw.update(p=1, q=2, dilas=[1, 2])                # (the full-size default is covered by the tests above)
    net, P = _gag_model(kw, 990, dev)
    specs = eabnet_amd.gag_param_specs(net.cfg)
    for k, sp in specs.items():
        if sp.kind == "prelu":
            P[k] = torch.ones_like(P[k])
    net.load_state_dict(P, strict=True)
    B, T = 3, 20
    inpt, pre_x = _planar(B, T, 991), _planar(B, T, 992)
    label = _planar(B, T, 993).permute(0, 1, 3, 2).contiguous()              # (B,2,F,T)
    frames = [T] * B
    net.train()
    outs = net(inpt.to(dev), pre_x.to(dev))
    assert outs[0].requires_grad and net.training_backend == "hip" and getattr(net, "_train_bound", None)
    loss = eabnet_amd.stagewise_com_mag_mse_loss(outs, label.to(dev), frames)
    loss.backward()
    is_param = {k for k, sp in specs.items() if not sp.kind.startswith("bn_")}
    Pd = {k: (v.double().requires_grad_(True) if k in is_param else v.double()) for k, v in P.items()}
    okw = {k: v for k, v in kw.items() if k not in ("kd1",)}
    ref_outs = orc.gagnet_forward(Pd, inpt.double(), pre_x.double(), kd1=kw.get("kd1", 3), bn_train=kw.get("norm_type") == "BN", **okw)
    lo = orc.stagewise_com_mag_mse_loss(ref_outs, label.double(), frames)
    lo.backward()
    for a, b in zip(outs, ref_outs):
        assert_close(a.detach().cpu().numpy(), b.detach().numpy(), 1e-5, f"{name}: training forward (post-filter)")
    assert abs(float(loss.detach()) - float(lo.detach())) <= 1e-5 * abs(float(lo.detach()))
    ref = {k: Pd[k].grad for k in is_param}
    got = {k: net.get_parameter(k).grad.cpu().double() for k in ref}
    assert all(torch.isfinite(g).all() for g in got.values())
    total, per = _grad_errors(got, ref)
    bad = sorted(((err, k) for k, err in per.items() if err > 1e-4), reverse=True)
    print(f"post-filter {name}: parameter gradients global l2-rel {total:.2e}, worst tensor {max(per.values()):.2e}")
    assert total <= 1e-4 and not bad, f"global l2-rel {total:.3e}; tensors over 1e-4: {bad[:8]}"


def test_hip_training_step_matches_operator_path(dev):
    """One optimiser step of the reference's loop (train_distributed.py:218-230: forward, loss, backward, clip, Adam)
    on the HIP training programs against the same step on the PyTorch-ROCm operator comparator (tests/operator_path.py): same
    loss, same clipped-gradient norm, and the updated model gives the same inference output."""
    import copy
    import eabnet_amd
    from operator_path import OperatorPath
    net = _model(4, 930, dev, p=2, q=1)
    ref = OperatorPath(copy.deepcopy(net))
    x = torch.from_numpy(paramgen.make_spec_input(2, 24, 161, 4, 931)).to(dev)
    label = torch.from_numpy(paramgen.make_spec_input(2, 24, 161, 1, 932)[..., 0, :]).permute(0, 3, 1, 2).contiguous().to(dev)
    out = []
    for m in (net, ref):
        m.train()
        opt = torch.optim.Adam(m.parameters(), lr=5e-4)
        opt.zero_grad()
        loss = eabnet_amd.com_mag_mse_loss(m(x), label, [24, 24])
        loss.backward()
        gn = torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        with torch.no_grad():
            out.append((float(loss), float(gn), m.eval()(x).clone()))
    assert abs(out[0][0] - out[1][0]) <= 1e-4 * abs(out[1][0])
    assert abs(out[0][1] - out[1][1]) <= 2e-3 * abs(out[1][1])              # MIOpen's fp32 convolutions are the looser side
    assert_close(out[0][2].cpu().numpy(), out[1][2].cpu().numpy(), 2e-3, "inference after one step")


def test_config3_full_size_three_adam_steps_vs_operator_path(dev):
    """BASELINE configs[3] at ITS OWN size (train_distributed.py:273,279: per-GPU batch 6 x 6 s x 8 mics, T = 601): three
    steps of the reference's loop (prepare_data, forward, com_mag_mse_loss, backward, clip_grad_norm_(1.0), Adam(5e-4)) on the
    HIP training programs against the same three steps on the PyTorch-ROCm operator path, same initial parameters and batch.
    Loss of every step within 1e-4 relative; the global gradient of the first step (same parameters on both sides) within
    4 x the fp32-vs-fp64 floor the small-size oracle test measures for the reference arithmetic itself (1e-3)."""
    import argparse
    import copy
    import eabnet_amd
    torch.manual_seed(0)
    B, M, L = 6, 8, 96000
    net = eabnet_amd.EaBNet(M=M).to(dev)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("norm.weight"):
                p.copy_(torch.empty(p.shape).uniform_(0.5, 1.5, generator=g))
            elif n.endswith("norm.bias"):
                p.copy_(torch.empty(p.shape).uniform_(-0.3, 0.3, generator=g))
    from operator_path import OperatorPath
    ref = OperatorPath(copy.deepcopy(net))
    args = argparse.Namespace(mics=M, sr=16000, wav_len=6.0, win_size=0.020, win_shift=0.010, fft_num=320)
    wav = (0.05 * torch.randn(B, M, L, generator=g)).to(dev)
    tgt = (0.05 * torch.randn(B, 1, L, generator=g)).to(dev)
    T = 1 + L // 160
    losses, grads = [], []
    for m in (net, ref):
        m.train()
        opt = torch.optim.Adam(m.parameters(), lr=5e-4)
        ls = []
        for k in range(3):
            opt.zero_grad(set_to_none=True)
            noisy, target = eabnet_amd.prepare_data(wav, tgt, dev, args)
            assert noisy.shape == (B, T, 161, M, 2)
            loss = eabnet_amd.com_mag_mse_loss(m(noisy), target, [T] * B)
            loss.backward()
            if k == 0:
                grads.append(torch.cat([p.grad.reshape(-1) for p in m.parameters()]).double().cpu())
            torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
            opt.step()
            ls.append(float(loss))
        losses.append(ls)
        torch.cuda.empty_cache()
    assert net.training_backend == "hip" and ref.net.training_backend is None
    for a, b in zip(*losses):
        assert abs(a - b) <= 1e-4 * abs(b), losses
    assert all(np.isfinite(losses[0])) and bool(torch.isfinite(grads[0]).all())
    rel = float(torch.linalg.vector_norm(grads[0] - grads[1]) / torch.linalg.vector_norm(grads[1]))
    assert rel <= 4e-3, f"global gradient l2-rel {rel:.2e} (HIP programs vs operator path, first step)"


# ------------------------------------------------------------------ bf16 mode (BASELINE configs[3]/[4])
BF16_BOUND = 5e-2      # stated L2 bound of the bf16 mode against the fp32 reference; measured 1.3-2.3e-2
# worst single element (max-abs/max): 2-5e-2 measured; on the 10-frame fixture (InstanceNorm over ten frames) the numpy
# emulator of the same program already shows 4.0-4.5e-2 whatever the kernels' summation order, the device 5.1e-2
BF16_BOUND_MAX = 8e-2


@pytest.mark.parametrize("name,M,B,T", [("e2e_M8_B2_T20.npz", 8, 2, 20), ("e2e_M9_B1_T10.npz", 9, 1, 10)])
def test_bf16_mode_vs_reference_fixtures(dev, name, M, B, T):
    """precision='bf16' (operands rounded to bf16 on the bf16 matrix cores, fp32 accumulate / norms / activations -- the
    arithmetic autocast(bfloat16) gives the reference) cannot meet the 1e-4 bar; its error against the fp32 reference
    fixtures is bounded at BF16_BOUND and printed."""
    g = load(name)
    net = _model(M, int(g["param_seed"]), dev)
    net.precision = "bf16"
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, int(g["input_seed"]))).to(dev)
    with torch.no_grad():
        y = net(x)
    m, l2 = assert_close(y.cpu().numpy(), g["out"], BF16_BOUND, "bf16 vs fp32 reference", tol_max=BF16_BOUND_MAX)
    print(f"bf16 {name}: max-rel {m:.2e}, l2-rel {l2:.2e}")


def test_bf16_c1_full_size_and_streaming_config5(dev):
    """bf16 at the C1 size against the reference fixture, and BASELINE configs[4] as stated: 16 microphones, 8 s,
    BatchNorm norms, streaming in bf16 -- streamed frames equal the offline bf16 call bit for bit, and the offline
    call stays within BF16_BOUND of the oracle."""
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    g = load("c1_M8_T401.npz")
    net = _model(8, int(g["param_seed"]), dev)
    net.precision = "bf16"
    wav = torch.from_numpy(paramgen.make_wave(1, 8, 64000, int(g["wave_seed"])))
    with torch.no_grad():
        y = net(eabnet_amd.stft_compress(wav.to(dev), 320, 160, torch.hann_window(320)))
    m, l2 = assert_close(y.cpu().numpy(), g["out"], BF16_BOUND, "bf16 C1")
    print(f"bf16 C1: max-rel {m:.2e}, l2-rel {l2:.2e}")
    kw = dict(norm_type="BN")
    M, T = 16, 801
    net = _model(M, 1230, dev, **kw)
    net.precision = "bf16"
    x = torch.from_numpy(paramgen.make_spec_input(1, T, 161, M, 1231))
    xd = x.to(dev)
    with torch.no_grad():
        off = net(xd)
        ref = orc.eabnet_forward(torch_params(M, 1230, **kw), x, fast_lstm=True, **kw)
    m, l2 = assert_close(off.cpu().numpy(), ref.numpy(), BF16_BOUND, "bf16 offline BN vs oracle")
    print(f"bf16 config-5 shape: max-rel {m:.2e}, l2-rel {l2:.2e}")
    for chunk in (1, 16):
        st = net.stream_begin(1, T_max=T, chunk=chunk)
        ys = torch.cat([st.step(xd[:, t:t + chunk]) for t in range(0, T, chunk)], dim=2)
        assert torch.equal(ys, off), f"bf16 streaming chunk {chunk} differs from the offline bf16 call"


@pytest.mark.parametrize("M,B,T,pq", [(8, 1, 70, (6, 3)), (4, 2, 30, (2, 2))])
def test_bf16_training_gradients_vs_fp64_oracle_and_the_references_own_bf16_mode(dev, M, B, T, pq):
    """bf16 products in the training programs (precision="bf16": forward, dgrad and wgrad contractions on the bf16 matrix cores,
    fp32 accumulation, storage, norms and LSTM) at network level: every parameter gradient against fp64 autograd through the
    oracle, next to what the REFERENCE's bf16 mode does on the same model and batch -- torch.autocast(bfloat16), which is what
    BASELINE configs[3]/[4] mean, run through the PyTorch-ROCm operator path.  The HIP gradient must be clearly closer to
    fp64 than the autocast gradient (<= 0.6 x its global l2-rel error; measured 0.31 x) and inside 1e-1 globally, with
    every parameter tensor pointing the same way as fp64 (cosine >= 0.99 for tensors above the noise floor).
    Smooth network (PReLU slopes 1) so that activation-derivative flips do not mask the rounding being measured."""
    import eabnet_amd
    from eabnet_amd.spec import NetConfig, param_specs
    p, q = pq
    kw = dict(p=p, q=q)
    P = torch_params(M, 1010 + M, **kw)
    for k, sp in param_specs(NetConfig(M=M, **kw)).items():
        if sp.kind == "prelu":
            P[k] = torch.ones_like(P[k])
    x = torch.from_numpy(paramgen.make_spec_input(B, T, 161, M, 1011))
    label = torch.from_numpy(paramgen.make_spec_input(B, T, 161, 1, 1012)[..., 0, :]).permute(0, 3, 1, 2).contiguous()
    frames = [T] * B
    _, _, ref = _oracle_grads(P, x, label, frames, **kw)

    def grads_of(hip: bool):
        net = eabnet_amd.EaBNet(M=M, **kw)
        net.load_state_dict(P, strict=True)
        net = net.to(dev).train()
        if hip:
            net.precision = "bf16"
            y = net(x.to(dev))
            assert net.training_backend == "hip"
        else:
            from operator_path import forward_autograd
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = forward_autograd(net, x.to(dev))
            assert net.training_backend is None
        eabnet_amd.com_mag_mse_loss(y.float(), label.to(dev), frames).backward()
        return {k: net.get_parameter(k).grad.detach().cpu().double() for k in ref}
    g_hip, g_ac = grads_of(True), grads_of(False)
    e_hip, per_hip = _grad_errors(g_hip, ref)
    e_ac, _ = _grad_errors(g_ac, ref)
    gmax = max(float(v.abs().max()) for v in ref.values())
    cos = {k: float(torch.nn.functional.cosine_similarity(g_hip[k].reshape(-1), ref[k].reshape(-1), dim=0))
           for k in ref if float(ref[k].abs().max()) > 1e-3 * gmax}
    print(f"bf16 training gradients vs fp64 oracle: HIP programs l2-rel {e_hip:.2e} (worst tensor {max(per_hip.values()):.2e}, "
          f"min cosine {min(cos.values()):.4f}); torch.autocast(bf16) operator path {e_ac:.2e}")
    assert all(torch.isfinite(g).all() for g in g_hip.values())
    # measured: 2.7e-2 / 6.1e-2 (HIP) against 8.6e-2 / 2.0e-1 (autocast: it also stores activations in bf16)
    assert e_hip <= 1e-1 and e_hip <= 0.6 * e_ac, (e_hip, e_ac)
    assert min(cos.values()) >= 0.99, sorted((c, k) for k, c in cos.items())[:5]


def test_bf16_storage_changes_the_bytes_not_the_numbers(dev, monkeypatch):
    """bf16 training programs store the tensors that only bf16 contractions read as bf16 (train.assign_bf16_storage).  Those
    kernels round their operands to bf16 anyway, so against the same program with everything stored in fp32 (EAB_BF16_STORE=0)
    the forward output must be bit-identical and the gradients equal up to the order of the fp32 atomics (and the bias
    gradients, which sum the stored -- rounded -- convolution-output gradients)."""
    import eabnet_amd
    x = torch.from_numpy(paramgen.make_spec_input(2, 40, 161, 4, 1101)).to(dev)
    label = torch.from_numpy(paramgen.make_spec_input(2, 40, 161, 1, 1102)[..., 0, :]).permute(0, 3, 1, 2).contiguous().to(dev)
    res = {}
    for run, store in (("0", "0"), ("0b", "0"), ("1", "1")):          # "0b": the fp32-stored program again = the run-to-run floor
        monkeypatch.setenv("EAB_BF16_STORE", store)
        net = _model(4, 1100, dev, p=2, q=1).train()
        net.precision = "bf16"
        y = net(x)
        eabnet_amd.com_mag_mse_loss(y, label, [40, 40]).backward()
        bound = next(iter(net._train_bound.values()))
        n_bf = sum(1 for op in bound.prog.fwd + bound.prog.bwd if getattr(op, "src_bf16", 0) or getattr(op, "bf16_mask", 0))
        assert (n_bf > 50) == (store == "1"), n_bf
        res[run] = (y.detach().clone(), {k: p.grad.detach().double().clone() for k, p in net.named_parameters()})
    assert torch.equal(res["0"][0], res["1"][0]), "forward output must not change"

    def diffs(a, b):
        gmax = max(float(g.norm()) for g in a.values())
        glob = float(torch.cat([(a[k] - b[k]).reshape(-1) for k in a]).norm() / torch.cat([g.reshape(-1) for g in a.values()]).norm())
        per = {k: float((a[k] - b[k]).norm() / a[k].norm()) for k in a if float(a[k].norm()) > 1e-4 * gmax}
        return glob, per
    floor_g, floor = diffs(res["0"][1], res["0b"][1])
    got_g, got = diffs(res["0"][1], res["1"][1])
    worst = sorted(((got[k], floor[k], k) for k in got), reverse=True)[:8]
    print(f"bf16 storage on/off: global gradient l2-rel {got_g:.2e} (run-to-run floor of the fp32-stored program {floor_g:.2e}); "
          f"worst tensors (diff, floor, name): {worst}")
    # (a bias in front of an InstanceNorm has a zero gradient -- the norm removes the mean -- so its evaluations are unrelated
    # rounding noise: tensors below 1e-4 of the largest one are left out.)  Weights: the same products, only the order of the
    # fp32 atomics differs -> within a few times the program's own run-to-run floor; biases of gated / head convolutions are
    # column sums of the stored (rounded) gradient instead of the unrounded one
    assert got_g <= max(5.0 * floor_g, 5e-3), (got_g, floor_g)
    for k, r in got.items():
        assert r <= max(5.0 * floor[k], 2e-2 if k.endswith("bias") else 1e-4), (k, r, floor[k])


def test_config4_ddp_training_on_the_hip_programs(dev):
    """BASELINE configs[3] on one rank: train_distributed.py's step (:218-230) for the beam-former stage with forward and
    backward on the HIP training programs, (a) under torch DistributedDataParallel over the RCCL backend (one 64 MB
    bucket, gradient_as_bucket_view, static_graph -- SURVEY §5) and (b) with the built-in flat gradient all-reduce; both
    give the gradients of a plain (unsynchronised) step, fp32 and bf16 products both train."""
    import os
    import torch.distributed as dist
    import eabnet_amd
    from eabnet_amd import train as tr
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_free_port())        # (a fixed port can collide on a shared box)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        x = torch.from_numpy(paramgen.make_spec_input(2, 24, 161, 4, 170)).to(dev)
        label = torch.from_numpy(paramgen.make_spec_input(2, 24, 161, 1, 171)[..., 0, :]).permute(0, 3, 1, 2).contiguous().to(dev)
        grads = {}
        for mode in ("plain", "ddp", "flat"):
            net = _model(4, 940, dev, p=2, q=1).train()
            model = net
            if mode == "ddp":
                model = torch.nn.parallel.DistributedDataParallel(net, device_ids=[dev.index], bucket_cap_mb=64,
                                                                  gradient_as_bucket_view=True, static_graph=True)
            elif mode == "flat":
                tr.broadcast_parameters(net)
                tr.enable_flat_allreduce(net)
            opt = torch.optim.Adam(net.parameters(), lr=5e-4)
            loss = eabnet_amd.com_mag_mse_loss(model(x), label, [24, 24])
            loss.backward()
            assert getattr(net, "_train_bound", None), "the HIP training path did not engage"
            grads[mode] = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone()
            torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
            opt.step()
            assert torch.isfinite(loss)
        assert_close(grads["ddp"].cpu().numpy(), grads["plain"].cpu().numpy(), 1e-5, "DDP gradients")          # (wgrad accumulates with atomics: order varies)
        assert_close(grads["flat"].cpu().numpy(), grads["plain"].cpu().numpy(), 1e-5, "flat all-reduce gradients")
        net = _model(4, 940, dev, p=2, q=1).train()
        net.precision = "bf16"
        loss_b = eabnet_amd.com_mag_mse_loss(net(x), label, [24, 24])
        loss_b.backward()
        gb = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
        assert torch.isfinite(gb).all()
        m, l2 = rel_errs(gb.cpu().numpy(), grads["plain"].cpu().numpy())
        cos = float(torch.nn.functional.cosine_similarity(gb, grads["plain"], dim=0))
        print(f"bf16 training gradients vs fp32: max-rel {m:.2e}, l2-rel {l2:.2e}, cosine {cos:.4f}")
        # bf16 products (2^-9 relative per operand) through ~60 normalised layers on a 24-frame utterance: a direction
        # check, not a parity claim (the bf16 mode is outside the 1e-4 bar by construction)
        assert cos > 0.9
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------ cumulative LayerNorm (second half)
def test_cln_every_op_matches_the_emulator_and_streams(dev):
    """norm_type="cLN" (the reference's CumulativeLayerNorm classes behind the fixed NormSwitch constructor): every op of
    the device program against the numpy interpreter, the output against the reference fixture (var_cln.npz), and the
    property the norm exists for: streaming (running sums as the only norm state) equals the offline call bit for bit --
    also at BASELINE configs[4] size (16 microphones, 8 s) in fp32 and bf16."""
    from eabnet_amd import program as prg
    from eabnet_amd.model import _Bound
    from eabnet_amd.spec import NetConfig, param_specs
    from emulator import Emulator
    g = load("var_cln.npz")
    cfg = NetConfig(M=4, norm_type="cLN")
    P = paramgen.make_params(param_specs(cfg), int(g["param_seed"]))
    x = paramgen.make_spec_input(2, 20, 161, 4, int(g["input_seed"]))
    prog = prg.lower(cfg, P, 2, 20, 161)
    emu = Emulator(prog, x)
    bound = _Bound(prog, dev)
    bound.acts.fill_(float("nan"))
    xin = torch.from_numpy(x).to(dev)
    out = torch.full((2, 2, 20, 161), float("nan"), device=dev)
    bound.bind(xin.data_ptr(), out.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    for k, op in enumerate(prog.ops):
        bound.run(stream, k, 1)
        torch.cuda.synchronize()
        prev = emu.arena["a"].copy()
        emu.step(op)
        got, want = bound.acts.cpu().numpy(), emu.arena["a"]
        if op.kind == prg.OP_CLN_STATS:        # fp64 scratch: compare as doubles where the emulator wrote them
            gd, wd = got[op.sums.off:op.sums.off + 2 * 20 * 4].view(np.float64), want[op.sums.off:op.sums.off + 2 * 20 * 4].view(np.float64)
            assert np.allclose(gd, wd, rtol=1e-5), f"op {k} {op.name}: frame sums"
            want[op.sums.off:op.sums.off + 2 * 20 * 4] = got[op.sums.off:op.sums.off + 2 * 20 * 4]
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"op {k} {op.name}: wrote a different set of elements"
        m = ~np.isnan(want)
        err = np.abs(got[m] - want[m]).max() / max(np.abs(want[m]).max(), 1e-20)
        assert err < 2e-4, f"op {k} {op.name} (kind {op.kind}): workspace deviates by {err:.3e}"
        _assert_op(k, op, prev, got, want, 2e-4)         # per op, relative to the maximum over what the op wrote
        emu.arena["a"][:] = got
    assert_close(out.cpu().numpy(), g["out"], TOL_HIP, "cLN vs reference fixture")
    # streaming == offline, small and at config-5 size
    for M, T, chunks, precs in ((4, 20, (1, 3), ("f32",)), (16, 801, (1, 16), ("f32", "bf16"))):
        net = _model(M, int(g["param_seed"]) if M == 4 else 1240, dev, norm_type="cLN")
        xs = torch.from_numpy(paramgen.make_spec_input(1, T, 161, M, 1241)).to(dev)
        for prec in precs:
            net.precision = prec
            with torch.no_grad():
                off = net(xs)
            assert torch.isfinite(off).all()
            for chunk in chunks:
                st = net.stream_begin(1, T_max=T, chunk=chunk)
                ys = torch.cat([st.step(xs[:, t:t + chunk]) for t in range(0, T, chunk)], dim=2)
                assert torch.equal(ys, off), f"cLN streaming M={M} T={T} chunk={chunk} {prec}"
    # causality: frames before t0 do not depend on the input from t0 on
    x2 = xs.clone()
    x2[:, 500:] = 0.0
    with torch.no_grad():
        assert torch.equal(net(x2)[:, :, :500], off[:, :, :500])


def test_prepare_data_with_a_window_shorter_than_the_fft(dev):
    """prepare_data with win_size != fft_num (the reference accepts any win_length <= n_fft, train_distributed.py:83)."""
    import eabnet_amd
    from oracle import eabnet_oracle as orc
    x = torch.from_numpy(paramgen.make_wave(2, 4, 3200, 43))
    args = type("A", (), dict(mics=4, sr=16000, wav_len=0.2, win_size=0.0125, win_shift=0.010, fft_num=320))   # 200-sample window
    noisy, tgt = eabnet_amd.prepare_data(x, x[:, :1], dev, args)
    want_n, want_t = orc.prepare_data_oracle(x, x[:, :1], 320, 160, 200)
    assert_compressed_close(noisy.cpu().numpy(), want_n.numpy(), TOL_HIP, "noisy")
    assert_compressed_close(np.moveaxis(tgt.cpu().numpy(), 1, -1), np.moveaxis(want_t.numpy(), 1, -1), TOL_HIP, "target")
    with pytest.raises(RuntimeError):
        eabnet_amd.prepare_data(x, x[:, :1], dev, type("A", (), dict(mics=4, sr=16000, wav_len=0.2, win_size=0.03, win_shift=0.010, fft_num=320)))


@pytest.mark.parametrize("stage", [True, False])
def test_prepare_data_is_done_with_a_pinned_source_when_it_returns(dev, stage):
    """A caller may refill its (pinned) batch buffer as soon as prepare_data returns -- the reference's x.to(device) is
    synchronous for exactly this case (train_distributed.py:76-77).  Both host paths: staged through the ring's own pinned
    slot (default) and the direct read of the caller's pinned buffer, which must not return before the read has finished."""
    import eabnet_amd
    from eabnet_amd import model as mdl
    args = type("A", (), dict(mics=8, sr=16000, wav_len=4.0, win_size=0.020, win_shift=0.010, fft_num=320))
    src = torch.from_numpy(paramgen.make_wave(4, 8, 64000, 77))
    want_n, want_t = eabnet_amd.prepare_data(src.clone(), src[:, :1].clone(), dev, args)
    want_n, want_t = want_n.clone(), want_t.clone()
    saved = mdl._HostStager.always_stage
    mdl._HostStager.always_stage = stage
    try:
        for _ in range(4):                                   # several slots of the ring
            x = src.clone().pin_memory()
            t = src[:, :1].clone().contiguous().pin_memory()
            noisy, tgt = eabnet_amd.prepare_data(x, t, dev, args)
            x.fill_(1e6)                                     # the caller recycles its buffers immediately
            t.fill_(-1e6)
            torch.cuda.synchronize()
            assert torch.equal(noisy, want_n) and torch.equal(tgt, want_t)
    finally:
        mdl._HostStager.always_stage = saved


def test_istft_refuses_a_window_that_violates_nola(dev):
    """torch.istft raises when the squared-window overlap-add has a gap (window overlap add min); the HIP back end would divide
    by zero there, so the wrapper checks the same condition on the host and raises too -- for a short zero-padded window with
    a large hop and for a Hann window without overlap."""
    import eabnet_amd
    x = torch.randn(1, 2, 12, 161, device=dev)
    for wl, what in ((160, "NOLA"), (100, "win_shift <= win_length")):   # a gap in the envelope; a hop beyond the window
        with pytest.raises(RuntimeError, match=what):
            eabnet_amd.istft(x, 320, 160, torch.hann_window(wl))
        with pytest.raises(RuntimeError):
            torch.istft(torch.view_as_complex(x.permute(0, 3, 2, 1).contiguous()).cpu(), 320, 160, wl, torch.hann_window(wl))
    with pytest.raises(RuntimeError, match="NOLA"):
        eabnet_amd.istft(torch.randn(1, 2, 12, 129, device=dev), 256, 256, torch.hann_window(256))
    assert torch.isfinite(eabnet_amd.istft(x, 320, 160, torch.hann_window(320))).all()


@pytest.mark.parametrize("n_fft,hop,win", [(320, 80, 320), (256, 64, 256), (512, 128, 400), (320, 40, 320), (320, 160, 200), (256, 256, 256),
                                           (320, 100, 320), (320, 96, 320), (320, 130, 320), (320, 200, 320), (320, 41, 320),
                                           (512, 150, 400), (256, 77, 200), (320, 159, 320), (320, 161, 320), (320, 319, 320)])
def test_istft_other_hops_and_windows_vs_torch(dev, n_fft, hop, win):
    """The back end for any hop (dividing fft_num or not, up to 8 overlapping frames) and any win_length <= fft_num, against
    torch.istft called as enhance.py:59-62 calls it (the reference only ever passes 320/160/320; test.py / enhance.py take
    the three numbers from args).  Rectangular window for the hop == n_fft case (a Hann window has no valid envelope there)."""
    import eabnet_amd
    torch.manual_seed(n_fft + hop)
    B, T, F = 2, 37, n_fft // 2 + 1                   # several workgroups per utterance
    esti = torch.randn(B, 2, T, F)
    # a window without zeros where a Hann window has no valid envelope (no or nearly no overlap)
    window = torch.ones(win) if hop == n_fft else (torch.hamming_window(win) if hop * 2 > win else torch.hann_window(win))
    want = torch.istft(torch.view_as_complex(esti.permute(0, 3, 2, 1).contiguous()), n_fft, hop, win, window)
    got = eabnet_amd.istft(esti.to(dev), n_fft, hop, window)
    assert got.shape == want.shape == (B, hop * (T - 1))
    assert_close(got.cpu().numpy(), want.numpy(), 1e-5, f"istft {n_fft}/{hop}/{win}")
