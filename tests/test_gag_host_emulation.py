"""The kernels of csrc/gag.hip -- the pack, the gain / residual tail and its backward under per-utterance lengths
(eab_gag_crm_bwd_lens_f32) -- compiled for the HOST against tests/hip_host_shim (one thread per lane) into a
stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process: the same source the GPU runs,
on arrays allocated at exactly their size, with NaN behind every length of every input and a sentinel in every output, judged
against the masked float64 reference (tests/train_buckets_ref.py) with train_ref.check.  No GPU needed; the compiler is the one that
builds the library; nothing sanitized is loaded into Python."""
import struct

import numpy as np
import pytest

import host_emulation
import train_buckets_ref as bref
import train_ref as tref
from eabnet_amd import program as prg

B, T, F = 3, 24, 161
LENS = (24, 13, 5)
LD, LIN = 384, 192              # train_gag.PRE_LD, program.GAG_LIN_LD
SENTINEL = np.float32(7.25)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_emulation.build(tmp_path_factory, "gag", "gag.hip")


def _inputs(seed, lens):
    """every input of the three launches; NaN in every frame behind a length"""
    rng = np.random.default_rng(seed)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)                 # noqa: E731
    h = dict(inpt=f32(B, 2, T, F), pre_x=f32(B, 2, T, F), pre=f32(B, T, LD), g=f32(B, T, LIN), r=f32(B, T, LIN), i=f32(B, T, LIN),
             dplanar=f32(B, 2, T, F), dpre_out=f32(B, T, LD), acc_in=f32(B, T, LD))
    for b, n in enumerate(lens):
        for k, v in h.items():
            if v.shape[1] == 2:
                v[b, :, n:] = np.nan
            else:
                v[b, n:] = np.nan
    return h


ORDER = ("inpt", "pre_x", "pre", "g", "r", "i", "dplanar", "dpre_out", "acc_in")
OUTS = (("enc_in", (B, T, F, 4)), ("pre", (B, T, LD)), ("pre_out", (B, T, LD)), ("planar", (B, 2, T, F)), ("dg", (B, T, LIN)),
        ("dr", (B, T, LIN)), ("di", (B, T, LIN)), ("dpre", (B, T, LD)))


def _run(program, tmp_path, h, act, lens):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("7i", B, T, F, LD, LIN, act, int(lens is not None)))
        f.write(struct.pack(f"{B}i", *(lens if lens is not None else [T] * B)))
        for k in ORDER:
            f.write(np.ascontiguousarray(h[k], np.float32).tobytes())
    host_emulation.run(program, src, dst)
    raw, o, got = open(dst, "rb").read(), 0, {}
    for name, shape in OUTS:
        n = int(np.prod(shape))
        got[name] = np.frombuffer(raw, np.float32, n, o).reshape(shape)
        o += 4 * n
    assert o == len(raw)
    return got


@pytest.mark.parametrize("act", [prg.ACT_SIGMOID, prg.ACT_TANH, prg.ACT_RELU], ids=["sigmoid", "tanh", "relu"])
def test_pack_crm_and_the_masked_crm_backward_on_the_host(program, tmp_path, act):
    h = _inputs(300 + act, LENS)
    got = _run(program, tmp_path, h, act, LENS)
    refs = []
    for dt in (np.float64, np.float32):
        o = {"pack": bref.gag_pack([B, T, F, LD], h, LENS, dt), "crm": bref.gag_crm([B, T, F, LD, LIN, act], h, LENS, dt),
             "bwd": bref.gag_crm_bwd([B, T, F, LD, LIN, act], dict(h, dpre=True), LENS, dt)}
        refs.append(o)
    o64, o32 = refs
    for group, names in (("pack", {"enc_in": "enc_in", "pre": "pre"}), ("crm", {"pre_out": "pre_out", "planar": "planar"}),
                         ("bwd", {k: k for k in ("dg", "dr", "di", "dpre")})):
        g = {ref: got[out] for ref, out in names.items()}
        for ref, o in o64[group].items():
            assert (g[ref][~o.must] == SENTINEL).all(), f"{group} {ref}: a padding frame was written"
            assert np.isfinite(g[ref][o.must]).all(), f"{group} {ref}: NaN from behind a length reached a written element"
        worst, l2 = tref.check(o64[group], g, {k: o.val for k, o in o32[group].items()}, f"host {group}")
        print(f"HOST gag {group} act={act} | err/limit {worst:.3f} | L2 ratio {'-' if l2 is None else format(l2, '.2f')}")
    # the stage output's padding is zeros, written by selection
    for b, n in enumerate(LENS):
        assert (got["planar"][b, :, n:] == 0).all() and (got["pre_out"][b, n:] == 0).all()


def test_without_lengths_every_frame_is_computed_on_the_host(program, tmp_path):
    h = _inputs(400, [T] * B)
    got = _run(program, tmp_path, h, prg.ACT_SIGMOID, None)
    full = _run(program, tmp_path, h, prg.ACT_SIGMOID, [T] * B)
    for k in got:
        assert got[k].tobytes() == full[k].tobytes(), f"{k}: full lengths != lens == NULL"
        assert not (got[k][..., :1] == SENTINEL).any(), k
    o64 = bref.gag_crm_bwd([B, T, F, LD, LIN, prg.ACT_SIGMOID], dict(h, dpre=True), [T] * B)
    tref.check(o64, {k: got[k] for k in o64}, None, "host crm backward, lens == NULL")
