"""Training of the GaGNet post-filter on the hand-written kernels (SURVEY §8 rows N1 x N3).

The reference trains the two-stage model with autograd (train_distributed.py:181,218-230: EaBNetWithPostNet, the post-filter
fed esti0.detach(), EaBNet.py:142).  Here GaGNet.forward (GaGNet.py:76-90) and its backward are two static op programs behind
one torch.autograd.Function, built with the machinery of eabnet_amd/train.py (TrainLowering: tape of late-binding closures,
gradient Slots, index images for parameter packing, deferred + batched weight gradients).  What is specific to GaGNet:

  * inputs inpt, pre_x (B,2,T,F) planar -> gag_pack (enc_in [B][T][F][4], pre [B][T][384]); neither needs a gradient;
  * U2-encoder = the same blocks as EaBNet's (TrainLowering.unet_module / conv2d_fwd), 4 input channels;
  * a GlanceGazeModule (GaGNet.py:93-133): two gated 1x1 in-convs on cat(feat, pre) = ONE two-source gated convolution each
    (N = 512, GLU epilogue with factor dump), three chains of p*|dilas| single-branch S-TCMs (GaGNet.py:303-327), three
    linears d_feat -> 161 (rows padded to 192), the gain/residual tail y = pre * act(g) + (r, i) (eab_gag_crm_f32) whose
    backward is eab_gag_crm_bwd_f32;
  * the q stage outputs live in the 'out' arena [q][B][2][T][F]; their gradients arrive in 'dout' (same shape).

`pre` rows are 384 floats here (the inference program uses 324): the gradient w.r.t. pre is a dgrad convolution whose output
channel count must be a multiple of 64."""
from __future__ import annotations

from typing import Callable, Tuple

import numpy as np

from . import program as prg
from . import train as tr
from .program import Geometry, Ref, glu_row_order, pack_taps, tcm_taps
from .spec import GagConfig, gag_param_specs
from .train import GenOp, TVar, TrainLowering, TrainProgram, _split64

PRE_LD = 384            # floats per (b, t) row of the interleaved previous estimate: 2*161 padded to a multiple of 64
LIN_LD = prg.GAG_LIN_LD


def supported(cfg: GagConfig) -> bool:
    return (cfg.intra_connect in ("cat", "add") and cfg.norm_type in ("IN", "BN") and cfg.cin == 2 and 2 * cfg.freq <= PRE_LD)


class GagTrainLowering(TrainLowering):
    spec_fn = staticmethod(gag_param_specs)
    supports = staticmethod(supported)

    # ---- blocks ------------------------------------------------------------------------------------------------
    def gated_in(self, pfx: str, feat: TVar, pre: TVar, feat_perm: np.ndarray) -> TVar:
        """in_conv_main(cat) * sigmoid(in_conv_gate(cat)) (GaGNet.py:191,251): one gated two-source 1x1 convolution"""
        cfg = self.cfg
        D, Fq = cfg.d_feat, cfg.freq
        w = np.concatenate([self.idx(f"{pfx}.in_conv_main.weight"), self.idx(f"{pfx}.in_conv_gate.0.weight")], axis=0)[:, :, 0]
        cols = np.arange(2 * Fq)
        cols_pre = D + (cols % 2) * Fq + cols // 2                  # memory channel f*2+ri <- reference ri*F+f
        wk = np.full((2 * D, D + PRE_LD), -1, dtype=np.int64)
        wk[:, :D] = w[:, feat_perm]
        wk[:, D:D + 2 * Fq] = w[:, cols_pre]
        order = glu_row_order(2 * D)
        wk = wk[order]
        one = Geometry.pointwise(1)
        wimg = pack_taps(wk[:, :, None], one.taps)
        bimg = np.concatenate([self.idx(f"{pfx}.in_conv_main.bias"), self.idx(f"{pfx}.in_conv_gate.0.bias")])[order]
        out = self.act(1, D)
        rows = self.B * self.T
        dump = self.alloc(rows * 2 * D)
        self.conv_op(f"{pfx}.in_conv", [feat, pre], self.wadd(f"{pfx}.in_conv.w", wimg), self.wadd(f"{pfx}.in_conv.b", bimg), one,
                     N=2 * D, epi=prg.EPI_GLU, dst=out.ref, bm=64, glu_dump=dump)

        def back():
            dz = self.alloc(rows * 2 * D)
            self.bwd.append(GenOp(tr.OP_GLU_BWD, [self.grad_of(out), dump, dz], list(_split64(rows)) + [2 * D], name=f"{pfx}.in_conv.glu_bwd"))
            self.wgrad_op(f"{pfx}.in_conv.wgrad", dz, [feat, pre], one, wimg, N=2 * D, dbias=self.gadd([bimg]))
            c_lo = 0
            for s in (feat, pre):
                if s.needs_grad:
                    img = pack_taps(np.ascontiguousarray(wk[:, c_lo:c_lo + s.C].T)[:, :, None], one.taps)      # (C_s, 2D, 1)
                    self.dgrad(f"{pfx}.in_conv.dgrad{c_lo}", s, dz, [(self.wadd(f"{pfx}.in_conv.wd{c_lo}", img), one)], N=2 * D)
                c_lo += s.C
        self.tape.append(back)
        return out

    def tcm1(self, pre: str, x: TVar, dilation: int) -> TVar:
        """GaGNet's single-branch SqueezedTCM (GaGNet.py:303-327): in_conv -> PReLU/norm/dilated conv -> PReLU/norm/out_conv
        + residual"""
        cfg = self.cfg
        one, gd = Geometry.pointwise(1), Geometry.temporal(tcm_taps(cfg.kd1, dilation, cfg.is_causal))
        y, back_in = self.conv1d(f"{pre}.in_conv", x, self.idx(f"{pre}.in_conv.weight"), None, one, epi=prg.EPI_LINEAR, wname=f"{pre}.in_conv")
        self.tape.append(lambda: back_in(self.grad_of(y)))
        yd = self.in1d(f"{pre}.d", y, f"{pre}.d_conv.1", f"{pre}.d_conv.0")
        z, back_d = self.conv1d(f"{pre}.d_conv", yd, self.idx(f"{pre}.d_conv.3.weight"), None, gd, epi=prg.EPI_LINEAR, wname=f"{pre}.d_conv")
        self.tape.append(lambda: back_d(self.grad_of(z)))
        zo = self.in1d(f"{pre}.out", z, f"{pre}.out_conv.1", f"{pre}.out_conv.0")
        out, back_out = self.conv1d(f"{pre}.out_conv", zo, self.idx(f"{pre}.out_conv.2.weight"), None, one, epi=prg.EPI_ADD, aux=x,
                                    wname=f"{pre}.out_conv")

        def back():
            d = self.grad_of(out)
            self.contribute(x, d)                                            # residual
            back_out(d)
        self.tape.append(back)
        return out

    def chain(self, pre: str, x: TVar) -> TVar:
        for j in range(self.cfg.p):
            for k, d in enumerate(self.cfg.dilas):
                x = self.tcm1(f"{pre}.{j}.tcns.{k}", x, d)
        return x

    def linear(self, key: str, x: TVar) -> Tuple[TVar, Callable[[Ref], None]]:
        """Conv1d(d_feat -> 161, 1) (GaGNet.py:176,241), rows padded to LIN_LD (padded rows: zero weights, gradient discarded)"""
        D, Fq = self.cfg.d_feat, self.cfg.freq
        w = np.full((LIN_LD, D, 1), -1, dtype=np.int64)
        b = np.full(LIN_LD, -1, dtype=np.int64)
        w[:Fq], b[:Fq] = self.idx(f"{key}.weight"), self.idx(f"{key}.bias")
        return self.conv1d(key, x, w, b, Geometry.pointwise(1), epi=prg.EPI_LINEAR, wname=key)

    # ---- whole network -----------------------------------------------------------------------------------------
    def build(self) -> TrainProgram:
        cfg, B, T, F = self.cfg, self.B, self.T, self.F
        assert F == cfg.freq
        c = cfg.c
        enc_in = TVar(self.alloc(B * T * F * 4), F, 4, tr.Slot(), needs_grad=False)
        pre = TVar(self.alloc(B * T * PRE_LD), 1, PRE_LD, tr.Slot(), needs_grad=False)
        self.fwd.append(prg.GagPackOp(inpt=Ref("in"), pre_x=Ref("in2"), enc_in=enc_in.ref, pre=pre.ref, B=B, T=T, F=F, pre_ld=PRE_LD,
                                      name="pack"))
        x = enc_in
        if cfg.is_u2:
            for i in range(4):
                x = self.unet_module(f"en.meta_unet_list.{i}", [x], 4 - i, False)
            x = self.conv2d_fwd("en.last_conv", [x], "en.last_conv.0.conv.1", True, "en.last_conv.1", "en.last_conv.2")
        else:
            for i in range(5):                          # GaGNet's UNet_Encoder (GaGNet.py:417-452): every layer normed
                q = f"en.unet_list.{i}"
                x = self.conv2d_fwd(q, [x], f"{q}.0.conv.1", True, f"{q}.1", f"{q}.2")
        assert x.F * x.C == cfg.d_feat
        k = np.arange(cfg.d_feat)
        feat_perm = (k % c) * x.F + k // c                 # memory channel f*64+c <- reference c*4+f (GaGNet.py:83-84)
        feat = x.view(1, cfg.d_feat)
        self.gtaps["feat"] = feat
        act = {"sigmoid": prg.ACT_SIGMOID, "tanh": prg.ACT_TANH, "relu": prg.ACT_RELU}[cfg.acti_type]
        n_stage = B * 2 * T * F
        for gi in range(cfg.q):
            gl, gz = f"gags.{gi}.glance_block", f"gags.{gi}.gaze_block"
            xg0 = self.gated_in(gl, feat, pre, feat_perm)
            xz = self.gated_in(gz, feat, pre, feat_perm)
            # The glance chain and the two gaze chains only meet again in the tail; each of their launches fills a fraction
            # of the chip (57 workgroups at 6 x 6 s), so they run as three parallel branches, forward and backward.  The gaze
            # chains both read xz: each gets its own gradient slot, summed after the backward join (two lanes must not
            # accumulate into one buffer).
            xz_r, xz_i = TVar(xz.ref, xz.F, xz.C, tr.Slot()), TVar(xz.ref, xz.F, xz.C, tr.Slot())

            def join_back(xz=xz, xz_r=xz_r, xz_i=xz_i):
                self.mark("bwd", "join", [1, 2])
                self.contribute(xz, self.grad_of(xz_r))
                if not cfg.is_squeezed:
                    self.contribute(xz, self.grad_of(xz_i))
            self.tape.append(join_back)                 # replayed after the chains' closures, before the gated in-convs'
            self.mark("fwd", "fork", [1, 2])
            gain, back_g = self.linear(f"{gl}.linear_g.0", self.chain(f"{gl}.tcn_g", xg0))
            self.cur_lane = 1
            if cfg.is_squeezed:                         # one chain feeds both linear maps (GaGNet.py:236-237,255)
                ri = self.chain(f"{gz}.tcm_ri", xz_r)
                lr, back_r = self.linear(f"{gz}.linear_r", ri)
                li, back_i = self.linear(f"{gz}.linear_i", ri)
            else:
                lr, back_r = self.linear(f"{gz}.linear_r", self.chain(f"{gz}.tcm_r", xz_r))
                self.cur_lane = 2
                li, back_i = self.linear(f"{gz}.linear_i", self.chain(f"{gz}.tcm_i", xz_i))
            self.cur_lane = 0
            self.mark("fwd", "join", [1, 2])
            nxt = TVar(self.alloc(B * T * PRE_LD), 1, PRE_LD, tr.Slot(), needs_grad=gi + 1 < cfg.q)
            self.fwd.append(prg.GagCrmOp(pre=pre.ref, g=gain.ref, r=lr.ref, i=li.ref, pre_out=nxt.ref, planar=Ref("out", gi * n_stage),
                                         B=B, T=T, F=F, act=act, pre_ld=PRE_LD, name=f"gags.{gi}.crm"))

            def back(gi=gi, pre=pre, gain=gain, nxt=nxt, back_g=back_g, back_r=back_r, back_i=back_i):
                n = B * T * LIN_LD
                dg, dr, di = self.alloc(n), self.alloc(n), self.alloc(n)
                dst, aux = self.grad_target(pre) if pre.needs_grad else (None, None)
                self.bwd.append(GenOp(prg.OP_GAG_CRM_BWD, [pre.ref, gain.ref, Ref("dout", gi * n_stage), nxt.slot.ref, aux, dg, dr, di, dst],
                                      [B, T, F, PRE_LD, LIN_LD, act], name=f"gags.{gi}.crm_bwd"))
                self.mark("bwd", "fork", [1, 2])
                back_g(dg)
                self.cur_lane = 1
                back_r(dr)
                self.cur_lane = 1 if cfg.is_squeezed else 2
                back_i(di)
                self.cur_lane = 0
            self.tape.append(back)
            pre = nxt
        for fn in reversed(self.tape):
            fn()
        prog = self.finish()
        prog.out_shape = (cfg.q, B, 2, T, F)
        prog.has_in2 = True
        return prog


def lower_train(cfg: GagConfig, B: int, T: int, F: int = 161, precision: str = "f32", varlen: bool = False,
                bucket: bool = False, lstm_bound: bool = True) -> TrainProgram:
    """varlen / bucket: the same op list with every op that sums across rows flagged for per-utterance lengths (train.flag_varlen,
    DESIGN §4.27: the convolutions, in1d, the norm backward, the weight gradients, and the pack / CRM / CRM backward of this
    file, which skip padding frames); T is the padded width, with bucket a cap.  The three parallel lanes read one lengths
    array.  Configurations outside is_causal=True / norm_type='IN' are refused with train.varlen_unsupported_reason."""
    if (varlen or bucket) and tr.varlen_unsupported_reason(cfg):
        raise NotImplementedError("training with per-utterance lengths: " + tr.varlen_unsupported_reason(cfg))
    prog = GagTrainLowering(cfg, B, T, F, precision).build()
    return tr.flag_varlen(prog, bucket, lstm_bound) if (varlen or bucket) else prog      # (lstm_bound: the post-filter has no LSTM)
