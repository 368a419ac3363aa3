"""Every convolution kernel variant the benchmark shapes select, ONE LAUNCH AT A TIME, against the float64 reference of
that launch (tests/conv_ref.py) on a real MI355X.

Per benchmark shape (conv_ref.bench_shapes, read from bench.py) the program is lowered and bound once; per variant key
(conv_ref.variant_key) the op with the most ragged last tile -- and the deepest one, if it is another -- runs alone on a
NaN-poisoned arena whose read regions hold seeded random data.  Only two distinct utterances fill the batch (slot b carries
utterance b % 2): the float64 reference is computed for two slots, every other slot must be bit-identical to its twin, so all
16 slots are checked for the CPU cost of two.  Asserted per launch: the set of changed elements of the whole arena is exactly
the launch's output set; dst / f2_dst / dst_acc meet the derived per-element limit AND the statistical criterion (L2 error at
most 8 x that of the fp32 CPU evaluation, both against float64); the Welford partials have exact counts and mean / M2 within
their limits; the fused-finalisation tables match and the arrival counters are re-armed."""
import time

import numpy as np
import pytest
import torch

import conv_ref as cr
from eabnet_amd import program as prg

pytestmark = pytest.mark.gpu

NAN_SRC_FIELDS = ("src0", "src1")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _tile_slots(a: np.ndarray, idx) -> np.ndarray:
    return np.ascontiguousarray(a[list(idx)])


def _run_launch(bound, prog, k, xin, out, dev, utt_of_slot, lens_of_slot, nref):
    """one op alone; returns (worst err/limit, L2 ratio).  utt_of_slot[b]: which of the two utterances slot b carries;
    lens_of_slot: per-slot frame counts or None; the slots repeat with period nref (slot b is the twin of slot b % nref)."""
    op = prog.ops[k]
    B = op.B
    rng = np.random.default_rng(4000 + k)
    inputs = cr.random_inputs(op, rng, 2)
    arenas = {"a": bound.acts, "in": xin.view(-1)}
    field_of = {ref: f for f, ref, _, _, _ in cr.regions(op)}
    bound.acts.fill_(float("nan"))
    xin.fill_(float("nan"))
    out.fill_(float("nan"))
    bound.reset_counters()
    ref_inputs = {}
    for ref, a in inputs.items():
        a = _tile_slots(a, utt_of_slot[:nref])                        # (nref, ...): what the reference sees
        if lens_of_slot is not None and field_of[ref] in NAN_SRC_FIELDS:
            for b in range(nref):                                     # padding frames: never read (eab_time_window.lens)
                a[b, lens_of_slot[b]:] = np.nan
        ref_inputs[ref] = a
        n = a[0].size
        view = arenas[ref.arena][ref.off:ref.off + B * n].view(B, n)
        h = torch.from_numpy(a.reshape(nref, n)).to(dev)
        for b in range(nref):
            view[b::nref] = h[b]
    lop, arena = cr.cut_out(op, prog.weights, ref_inputs)
    lens = None if lens_of_slot is None else list(lens_of_slot[:nref])
    outs = cr.conv_ref(lop, arena, lens)
    yard_arena = cr.conv_f32(lop, arena)
    before = bound.acts.clone()
    bound.run(torch.cuda.current_stream().cuda_stream, k, 1)
    torch.cuda.synchronize()
    changed = bound.acts.view(torch.int32) != before.view(torch.int32)
    what = f"op {k} {op.name} [{cr.key_str(cr.variant_key(op))}]"
    full_ref = {f: r for f, r, _, _, _ in cr.regions(op)}            # the program's own Refs (lop's point into the cut-out)
    got, yard = {}, {}
    for name, o in outs.items():
        ref = full_ref[name]
        assert ref.arena == "a", f"{what}: {name} lies outside the activation arena"
        n = int(np.prod(o.shape[1:]))
        sl = slice(ref.off, ref.off + B * n)
        idx = [b % nref for b in range(B)]
        may = torch.from_numpy(_tile_slots(o.may.reshape(nref, n), idx)).to(dev)
        must = torch.from_numpy(_tile_slots(o.must.reshape(nref, n), idx)).to(dev)
        ch = changed[sl].view(B, n)
        assert not (ch & ~may).any(), f"{what}: {name} changed outside the elements the launch writes"
        if name not in ("dst_acc", "fz_counter"):           # (a running sum or a counter may legitimately keep its bits)
            assert not (must & ~ch).any(), f"{what}: {name} has elements the launch should have written and did not"
        bits = bound.acts[sl].view(torch.int32).view(B, n)
        for b in range(nref, B):
            assert not ((bits[b] != bits[b % nref]) & must[b]).any(), f"{what}: {name} of slot {b} differs from its twin {b % nref}"
        got[name] = bound.acts[sl].view(B, n)[:nref].cpu().numpy().reshape(o.shape)
        yard[name] = cr.read(yard_arena, o.ref, o.shape)
        changed[sl] = False
    assert not changed.any(), f"{what}: {int(changed.sum())} elements changed outside the launch's output regions"
    assert torch.isnan(out).all(), f"{what}: the network output was touched"
    return cr.check(outs, got, yard, what, got_is_region=True)


def _walk(dev, shape, varlen=False, lens_pattern=None, only=None, tag=""):
    from eabnet_amd.model import _Bound
    t0 = time.time()
    prog = cr.lower_shape(shape, varlen=varlen)
    bound = _Bound(prog, dev)
    B, T, M = shape["B"], shape["T"], shape["M"]
    if "gag" in shape:                        # post-filter: two planar inputs, one planar output per stage
        xin = torch.empty((2, B, 2, T, 161), device=dev)
        out = torch.empty((prog.cfg.q, B, 2, T, 161), device=dev)
        bound.bind(xin[0].data_ptr(), out.data_ptr(), xin[1].data_ptr())
    else:
        xin = torch.empty((B, T, 161, M, 2), device=dev)
        out = torch.empty((B, 2, T, 161), device=dev)
        bound.bind(xin.data_ptr(), out.data_ptr())
    if lens_pattern is None:
        nref = min(2, B)
        utt, lens_of_slot = [b % 2 for b in range(B)], None
    else:                                     # slot b: utterance b % 2, length lens_pattern[(b // 2) % len]; period 2 * len
        nref = 2 * len(lens_pattern)
        assert B >= nref
        utt = [b % 2 for b in range(B)]
        lens_of_slot = [lens_pattern[(b // 2) % len(lens_pattern)] for b in range(B)]
        bound.lens.copy_(torch.tensor(lens_of_slot, dtype=torch.int32))
    chosen = cr.chosen_ops(prog)
    if only is not None:
        chosen = [(key, k) for key, k in chosen if only(prog.ops[k])]
        assert chosen
    keys = set()
    for key, k in chosen:
        worst, l2 = _run_launch(bound, prog, k, xin, out, dev, utt, lens_of_slot, nref)
        keys.add(key)
        print(f"VARIANT {cr.shape_str(shape)}{' varlen' if varlen else ''}{tag} | {cr.key_str(key)} | {prog.ops[k].name} | err/limit {worst:.3f} | "
              f"L2 ratio {'-' if l2 is None else format(l2, '.2f')}")
    if only is None:
        assert keys == set(cr.variants_of(prog)), "a variant of this program was not run"
    print(f"{len(chosen)} launches of {len(keys)} variants in {time.time() - t0:.1f} s")


@pytest.mark.parametrize("index", range(len(cr.bench_shapes())))
def test_every_conv_variant_of_a_benchmark_shape_matches_float64(dev, index):
    _walk(dev, cr.bench_shapes()[index])


def test_conv_variants_with_per_utterance_lengths(dev):
    """varlen lowering of the headline shape: the full length, a single frame, and a length that ends inside a tile
    (250 frames: 250 * No is no multiple of 64 or 128 for No = 1, 4, 9, 19, 39, 79, 161).  Rows below each length obey the same
    limits, the statistics count only those rows, the padding frames of the sources hold NaN."""
    shape = cr.bench_shapes()[0]
    _walk(dev, shape, varlen=True, lens_pattern=[shape["T"], 1, 250])


def test_conv_variants_with_fused_finalisation(dev, monkeypatch):
    """EAB_FUSE_FIN=1 (off by default): the workgroup that writes the last partial merges them all (fz_*).  The counter is
    primed as if the other launches feeding the norm had arrived; afterwards the tables match and the counter is zero."""
    import eabnet_amd
    import paramgen
    from util import assert_close, torch_params
    x = torch.from_numpy(paramgen.make_spec_input(2, 70, 161, 8, 5)).to(dev)

    def forward():
        net = eabnet_amd.EaBNet(M=8)
        net.load_state_dict(torch_params(8, 3), strict=True)
        with torch.no_grad():
            return net.to(dev).eval()(x).cpu().numpy()
    plain = forward()
    monkeypatch.setenv("EAB_FUSE_FIN", "1")
    _walk(dev, cr.bench_shapes()[3], only=lambda op: op.fz_counter is not None, tag=" EAB_FUSE_FIN=1")
    # regression: the knob used to fuse the finalisation into launches whose kernels refuse it (small-tile kernel, phase-pair
    # form), and the program failed at its first run; now those norms keep their finalize launch and the network agrees
    assert_close(forward(), plain, 1e-5, "EAB_FUSE_FIN=1 against the default lowering")


# ----------------------------------------------------------------------------------------------------------------------
# the inference LSTM kernels through the C ABI (eab_lstm64_prec_f32, eab_lstm64_bf16, eab_lstm64_stream_f32 for lens)
# ----------------------------------------------------------------------------------------------------------------------
# fp32 runs 4-sequence workgroups up to S = B*F = 2048 sequences and 16-sequence workgroups above (csrc/lstm.hip); the
# reduced precisions always run the 16-sequence kernel of csrc/lstm_h3.hip.  Sequence counts on both sides of the switch,
# not multiples of 4 / 16, and S % 16 = 13 at the shape of 13 utterances:
LSTM_SHAPES = [(23, 89), (16, 128), (3, 683), (13, 161), (3, 7)]          # S = 2047, 2048, 2049, 2093, 21
GUARD = 4096


def _rn16(a):
    return a.astype(np.float16).astype(np.float32)


def _lstm_ref(x, wcat, bias, precision):
    """The recurrence in float64 with the operand roundings of the precision (tests/emulator.py Emulator.lstm states them):
    f32 none; bf16: [x_t | h_{t-1}] and W to bf16, h_t leaves exact; f16x3: W = hi + lo (nearest), [x_t | h_{t-1}] = hi + lo
    (toward zero), and h_t is carried AND stored as fp16 hi + lo (nearest).  x (S, T, 64) float64 (already normalised)."""
    from emulator import bf16_round, split_f16x3
    S, T, _ = x.shape
    W = wcat.float().numpy()
    if precision == prg.PREC_BF16:
        W = bf16_round(W)
    elif precision == prg.PREC_F16X3:
        Wh = _rn16(W)
        W = Wh.astype(np.float64) + _rn16(W - Wh).astype(np.float64)
    W, b = torch.from_numpy(np.asarray(W, np.float64)), bias.double()

    def operand(a):         # (S, 128) float64 -> what the matrix cores multiply
        a32 = a.float().numpy()
        if precision == prg.PREC_BF16:
            return torch.from_numpy(bf16_round(a32).astype(np.float64))
        if precision == prg.PREC_F16X3:
            hi, lo = split_f16x3(a32)
            return torch.from_numpy(hi.astype(np.float64) + lo.astype(np.float64))
        return a
    h, c = torch.zeros(S, 64, dtype=torch.float64), torch.zeros(S, 64, dtype=torch.float64)
    hs = []
    for t in range(T):
        pre = operand(torch.cat((x[:, t], h), 1)) @ W.T + b
        i, f, g, o = torch.sigmoid(pre[:, :64]), torch.sigmoid(pre[:, 64:128]), torch.tanh(pre[:, 128:192]), torch.sigmoid(pre[:, 192:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        if precision == prg.PREC_F16X3:
            h32 = h.float().numpy()
            hh = _rn16(h32)
            h = torch.from_numpy(hh.astype(np.float64) + _rn16(h32 - hh).astype(np.float64))
        hs.append(h)
    return torch.stack(hs, 1)


def _lstm_case(B, F, T, ln, seed):
    g = torch.Generator().manual_seed(seed)
    lstm = torch.nn.LSTM(64, 64, batch_first=True).double()
    norm = torch.nn.LayerNorm(64).double()
    with torch.no_grad():
        for p in lstm.parameters():
            p.copy_(torch.empty_like(p).uniform_(-0.125, 0.125, generator=g))
        norm.weight.copy_(torch.empty(64, dtype=torch.float64).uniform_(0.5, 1.5, generator=g))
        norm.bias.copy_(torch.empty(64, dtype=torch.float64).uniform_(-0.3, 0.3, generator=g))
    S = B * F
    x = torch.randn(S, T, 64, generator=g, dtype=torch.float64).float().double()     # what the device holds, exactly
    wcat = torch.cat((lstm.weight_ih_l0, lstm.weight_hh_l0), 1).detach().float().double()
    bias = (lstm.bias_ih_l0 + lstm.bias_hh_l0).detach().float().double()
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(wcat[:, :64]); lstm.weight_hh_l0.copy_(wcat[:, 64:])       # noqa: E702
        lstm.bias_ih_l0.copy_(bias); lstm.bias_hh_l0.zero_()                                # noqa: E702
        norm.weight.copy_(norm.weight.float().double()); norm.bias.copy_(norm.bias.float().double())   # noqa: E702
        xn = norm(x) if ln else x
        h64, _ = lstm(xn)
        l32, n32 = torch.nn.LSTM(64, 64, batch_first=True), torch.nn.LayerNorm(64)
        l32.load_state_dict({k: v.float() for k, v in lstm.state_dict().items()})
        n32.load_state_dict({k: v.float() for k, v in norm.state_dict().items()})
        h32, _ = l32(n32(x.float()) if ln else x.float())
    return dict(S=S, x=x, xn=xn, wcat=wcat, bias=bias, norm=norm, h64=h64, err32=float((h32.double() - h64).abs().max()))


def _run_lstm(lib, case, B, F, T, ln, precision, lens=None, entry="prec"):
    import ctypes as C
    from eabnet_amd import _lib
    dev = "cuda:0"
    to_btf = lambda t: t.view(B, F, T, 64).permute(0, 2, 1, 3).contiguous()      # noqa: E731
    xd = to_btf(case["x"]).float()
    if lens is not None:
        for b in range(B):
            xd[b, lens[b]:] = float("nan")                   # padding frames: never read
    xd = xd.to(dev)
    wd, bd = case["wcat"].float().to(dev), case["bias"].float().to(dev)
    gd, be = case["norm"].weight.detach().float().to(dev), case["norm"].bias.detach().float().to(dev)
    n = B * T * F * 64
    buf = torch.full((n + GUARD,), float("nan"), device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lg, lb = (gd.data_ptr(), be.data_ptr()) if ln else (None, None)
    if lens is not None:
        ld = torch.tensor(lens, dtype=torch.int32, device=dev)
        win = _lib.TimeWindow(None, 0, ld.data_ptr())
        code = lib.eab_lstm64_stream_f32(xd.data_ptr(), lg, lb, 1e-5, wd.data_ptr(), bd.data_ptr(), buf.data_ptr(), None, B, T, F,
                                         precision, win, st)
    elif entry == "bf16":
        code = lib.eab_lstm64_bf16(xd.data_ptr(), lg, lb, 1e-5, wd.data_ptr(), bd.data_ptr(), buf.data_ptr(), B, T, F, st)
    else:
        code = lib.eab_lstm64_prec_f32(xd.data_ptr(), lg, lb, 1e-5, wd.data_ptr(), bd.data_ptr(), buf.data_ptr(), B, T, F, precision, st)
    _lib.check(code, "eab_lstm64")
    torch.cuda.synchronize()
    assert torch.isnan(buf[n:]).all(), "the kernel wrote behind h_out"
    return buf[:n].view(B, T, F, 64).cpu().double().permute(0, 2, 1, 3).reshape(B * F, T, 64)


def _lstm_limits(case, T, precision, got, ref, what):
    """fp32: 1e-5 absolute for T <= 40 (outputs are bounded by 1; the bar tests/test_hip_train_ops.py sets for single kernels),
    4 x the error of torch's fp32 CPU LSTM against the same float64 result for T = 401 (the recurrence accumulates rounding
    over time on both sides alike).  f16x3: the same two limits, against the reference that carries the rounded operands and
    the rounded state.  bf16: state
    and operands rounded in the reference; a value on the other side of a bf16 rounding boundary of h_{t-1} moves the next
    step by 2^-9 of one operand, so the bound is the one the training kernel's test states (2e-3 L2, 1e-2 max)."""
    err = float((got - ref).abs().max())
    if precision == prg.PREC_BF16:
        m = float((got - ref).abs().max() / ref.abs().max())
        l2 = float((got - ref).norm() / ref.norm())
        print(f"LSTM {what}: bf16 max-rel {m:.2e} (bound 1e-2), L2 {l2:.2e} (bound 2e-3)")
        assert m <= 1e-2 and l2 <= 2e-3, what
        exact = float((got - case["h64"]).norm() / case["h64"].norm())
        assert 1e-4 < exact < 2e-2, f"{what}: {exact} -- really bf16 products, and no worse than bf16"
        return
    lim = 1e-5 if T <= 40 else 4 * case["err32"]
    print(f"LSTM {what}: max abs error {err:.2e}, limit {lim:.2e} (torch fp32 on the CPU: {case['err32']:.2e})")
    assert err <= lim, f"{what}: max abs error {err:.3e} > {lim:.3e}"


def _rounded_ref(case, ln, precision):
    """float64 nn.LSTM for fp32; for the reduced precisions the recurrence on the rounded operands (once per case).  The
    normalised input the device rounds is its own fp32 LayerNorm output: the fp32 CPU LayerNorm stands in for it."""
    if precision == prg.PREC_F32:
        return case["h64"]
    if precision not in case:
        xn = torch.nn.functional.layer_norm(case["x"].float(), (64,), case["norm"].weight.detach().float(),
                                            case["norm"].bias.detach().float(), 1e-5).double() if ln else case["x"]
        case[precision] = _lstm_ref(xn, case["wcat"], case["bias"], precision)
    return case[precision]


@pytest.fixture(scope="module")
def lib(dev):
    from eabnet_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("B,F", LSTM_SHAPES)
def test_inference_lstm_kernels_vs_float64(lib, B, F, ln):
    for T in (1, 2, 40):
        case = _lstm_case(B, F, T, ln, 100 + T)
        # the hand-written recurrence IS nn.LSTM in float64
        assert float((_lstm_ref(case["xn"], case["wcat"], case["bias"], prg.PREC_F32) - case["h64"]).abs().max()) < 1e-13
        for precision, entry in ((prg.PREC_F32, "prec"), (prg.PREC_F16X3, "prec"), (prg.PREC_BF16, "bf16"), (prg.PREC_BF16, "prec")):
            got = _run_lstm(lib, case, B, F, T, ln, precision, entry=entry)
            _lstm_limits(case, T, precision, got, _rounded_ref(case, ln, precision),
                         f"S={B * F} (B={B}, F={F}) T={T} ln={ln} prec={precision} via {entry}")


@pytest.mark.parametrize("B,F,ln", [(13, 161, True), (23, 89, False)])
def test_inference_lstm_kernels_full_length_vs_float64(lib, B, F, ln):
    T = 401
    case = _lstm_case(B, F, T, ln, 7)
    for precision in (prg.PREC_F32, prg.PREC_F16X3, prg.PREC_BF16):
        got = _run_lstm(lib, case, B, F, T, ln, precision)
        _lstm_limits(case, T, precision, got, _rounded_ref(case, ln, precision), f"S={B * F} T=401 ln={ln} prec={precision}")


@pytest.mark.parametrize("B,F", [(13, 161), (3, 7)])
def test_inference_lstm_with_per_utterance_lengths(lib, B, F):
    """eab_time_window.lens: frames below each length equal the full-length result (the recurrence is causal); the padding
    frames of the input hold NaN and are never read"""
    T = 40
    case = _lstm_case(B, F, T, True, 21)
    lens = [T, 1, 17] + [1 + (7 * b) % T for b in range(3, B)]
    for precision in (prg.PREC_F32, prg.PREC_F16X3, prg.PREC_BF16):
        got = _run_lstm(lib, case, B, F, T, True, precision, lens=lens[:B])
        full = _run_lstm(lib, case, B, F, T, True, precision)
        for b in range(B):
            rows = slice(b * F, (b + 1) * F)
            assert torch.equal(got[rows, :lens[b]], full[rows, :lens[b]]), f"utterance {b} below its length, precision {precision}"
            assert torch.isfinite(got[rows, :lens[b]]).all()
        if precision == prg.PREC_F32:
            below = torch.arange(T)[None, :] < torch.tensor(lens[:B]).repeat_interleave(F)[:, None]         # (S, T)
            _lstm_limits(case, T, precision, got[below], case["h64"][below], f"lens S={B * F}")
