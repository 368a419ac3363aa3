"""float64 reference of the post-filter's tail under per-utterance lengths  (TEST INFRASTRUCTURE; numpy only).

As tests/train_varlen_ref.py does for the beam-former's ops, nothing here re-derives an op: every function cuts utterance b's first
lens[b] frames out of the padded batch, calls the UNMASKED reference of tests/train_ref.py on that slice as a batch of one and
puts the results back.  What a masked kernel must leave alone or write as zeros is said by the `must` set and the value:

    op              valid frames                padding frames (t >= lens[b])
    GAG_PACK        enc_in, pre of the slice    not written (must False)
    GAG_CRM         pre_out, planar of the slice  zeros, written (limit 0)
    GAG_CRM_BWD     dg, dr, di, dpre of the slice  not written (must False)

The padding frames of the INPUTS never enter: a test fills them with NaN.  dtype float32 gives train_ref's yardstick."""
from __future__ import annotations

from typing import Dict

import numpy as np

import train_ref as tref
from train_varlen_ref import _lens_ok, _out


def _planar(a, b, n):
    """frames [0, n) of utterance b of a planar (B, 2, T, F) tensor, as a batch of one"""
    return np.asarray(a)[b:b + 1, :, :n]


def gag_pack(i, A, lens, dtype=np.float64) -> Dict[str, tref.Out]:
    B, T, F, ld = i[:4]
    lens = _lens_ok(lens, B, T)
    shapes = {"enc_in": (B, T, F, 4), "pre": (B, T, ld)}
    val = {k: np.zeros(s, dtype) for k, s in shapes.items()}
    must = {k: np.zeros(s, bool) for k, s in shapes.items()}
    for b, n in enumerate(lens):
        res, _ = tref.run_ref("GAG_PACK", [1, n, F, ld], [], dict(inpt=_planar(A["inpt"], b, n), pre_x=_planar(A["pre_x"], b, n)), dtype)
        for k in shapes:
            val[k][b, :n], must[k][b, :n] = res[k][0][0], True
    return {k: _out(k, val[k], np.zeros(shapes[k]), must[k]) for k in shapes}


def gag_crm(i, A, lens, dtype=np.float64) -> Dict[str, tref.Out]:
    B, T, F, ld, lin_ld, act = i[:6]
    lens = _lens_ok(lens, B, T)
    nxt, Ln = np.zeros((B, T, ld), dtype), np.zeros((B, T, ld))                 # the padding frames: exact zeros (limit 0)
    pl, Lp = np.zeros((B, 2, T, F), dtype), np.zeros((B, 2, T, F))
    for b, n in enumerate(lens):
        Ab = {k: np.asarray(A[k])[b:b + 1, :n] for k in ("pre", "g", "r", "i")}
        res, _ = tref.run_ref("GAG_CRM", [1, n, F, ld, lin_ld, act], [], Ab, dtype)
        nxt[b, :n], Ln[b, :n] = res["pre_out"][0][0], res["pre_out"][1][0]
        pl[b, :, :n], Lp[b, :, :n] = res["planar"][0][0], res["planar"][1][0]
    return {"pre_out": _out("pre_out", nxt, Ln, np.ones(nxt.shape, bool)), "planar": _out("planar", pl, Lp, np.ones(pl.shape, bool))}


def gag_crm_bwd(i, A, lens, dtype=np.float64) -> Dict[str, tref.Out]:
    """A: pre, g, dplanar and / or dpre_out, optionally acc_in; the key 'dpre' asks for that output"""
    B, T, F, ld, lin_ld, act = i[:6]
    lens = _lens_ok(lens, B, T)
    shapes = {"dg": (B, T, lin_ld), "dr": (B, T, lin_ld), "di": (B, T, lin_ld)}
    if "dpre" in A:
        shapes["dpre"] = (B, T, ld)
    val = {k: np.zeros(s, dtype) for k, s in shapes.items()}
    lim = {k: np.zeros(s) for k, s in shapes.items()}
    must = {k: np.zeros(s, bool) for k, s in shapes.items()}
    for b, n in enumerate(lens):
        Ab = {k: np.asarray(A[k])[b:b + 1, :n] for k in ("pre", "g", "dpre_out", "acc_in") if A.get(k) is not None}
        if A.get("dplanar") is not None:
            Ab["dplanar"] = _planar(A["dplanar"], b, n)
        if "dpre" in A:
            Ab["dpre"] = True
        res, _ = tref.run_ref("GAG_CRM_BWD", [1, n, F, ld, lin_ld, act], [], Ab, dtype)
        for k in shapes:
            val[k][b, :n], lim[k][b, :n], must[k][b, :n] = res[k][0][0], res[k][1][0], True
    return {k: _out(k, val[k], lim[k], must[k]) for k in shapes}
