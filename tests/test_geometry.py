"""program.Geometry on its own (CPU): the constructors against the literal numbers the lowerings' call sites used to carry,
Geometry.adjoint against the dot-product identity, and pack_taps on an index image against pack_taps on the weights."""
import itertools

import numpy as np
import pytest

from eabnet_amd.program import Geometry, pack_taps, tcm_taps

G = Geometry


@pytest.mark.parametrize("Fin, Fout", [(161, 80), (79, 39), (4, 1)])
def test_strided(Fin, Fout):
    assert G.strided(Fin, 2, 3) == G(Fin, Fout, Fout, 1, 0, 2, (-1, -1, -1, 0, 0, 0), (0, 1, 2, 0, 1, 2), (0, 1, 2, 3, 4, 5))
    assert G.strided(Fin, 1, 3) == G(Fin, Fout, Fout, 1, 0, 2, (0, 0, 0), (0, 1, 2), (0, 1, 2))
    assert G.strided(Fin, 2, 3).ntaps == 6 and G.strided(Fin, 2, 3).kpad(4) == 96 and G.strided(Fin, 1, 3).kpad(2 * 64) == 384


@pytest.mark.parametrize("Fin, Fout, No", [(161, 323, (162, 161)), (79, 159, (80, 79)), (4, 9, (5, 4))])
def test_transposed(Fin, Fout, No):
    assert G.transposed(Fin, 2, 3) == (G(Fin, Fout, No[0], 2, 0, 1, (0, 0, -1, -1), (0, -1, 0, -1), (0, 2, 3, 5)),
                                       G(Fin, Fout, No[1], 2, 1, 1, (0, -1), (0, 0), (1, 4)))
    assert G.transposed(Fin, 1, 3) == (G(Fin, Fout, No[0], 2, 0, 1, (0, 0), (0, -1), (0, 2)),
                                       G(Fin, Fout, No[1], 2, 1, 1, (0,), (0,), (1,)))


def test_pointwise_and_temporal():
    assert G.pointwise(161) == G(161, 161, 161, 1, 0, 1, (0,), (0,), (0,))
    assert G.pointwise(161, dt=-1) == G(161, 161, 161, 1, 0, 1, (-1,), (0,), (0,))
    assert G.pointwise(1) == G.temporal([0]) == G(1, 1, 1, 1, 0, 1, (0,), (0,), (0,))
    assert G.temporal([-4, -2, 0]) == G(1, 1, 1, 1, 0, 1, (-4, -2, 0), (0, 0, 0), (0, 1, 2))
    assert G.pointwise(161).kpad(64) == 64 and G.pointwise(1).kpad(256 + 324) == 592 and G.temporal([-4, -2, 0]).kpad(64) == 192


def test_tcm_taps():
    assert tcm_taps(5, 2, True) == [-8, -6, -4, -2, 0] and tcm_taps(5, 2, False) == [-4, -2, 0, 2, 4]
    assert tcm_taps(3, 1, True) == [-2, -1, 0] and tcm_taps(3, 1, False) == [-1, 0, 1]
    assert tcm_taps(3, 16, True) == [-32, -16, 0] and tcm_taps(2, 1, False) == [0, 1] and tcm_taps(1, 4, True) == [0]


def test_adjoint_literals():
    """the data-gradient launches the training closures used to write out by hand"""
    assert G.adjoint(G.strided(161, 2, 3)) == [G(80, 161, 81, 2, 0, 1, (1, 1, 0, 0), (0, -1, 0, -1), (0, 2, 3, 5)),
                                               G(80, 161, 80, 2, 1, 1, (1, 0), (0, 0), (1, 4))]
    assert G.adjoint(G.strided(4, 1, 3)) == [G(1, 4, 2, 2, 0, 1, (0, 0), (0, -1), (0, 2)), G(1, 4, 2, 2, 1, 1, (0,), (0,), (1,))]
    assert G.adjoint(G.transposed(79, 2, 3)) == [G(159, 79, 79, 1, 0, 2, (0, 0, 0, 1, 1, 1), (0, 1, 2, 0, 1, 2), (0, 1, 2, 3, 4, 5))]
    assert G.adjoint(G.pointwise(161)) == [G.pointwise(161)]
    assert G.adjoint(G.temporal([-8, -4, 0])) == [G.temporal([8, 4, 0])]
    assert G.adjoint(G.strided(1, 1, 1)) == [G(1, 1, 1, 2, 0, 1, (0,), (0,), (0,))]       # no column, no tap of parity 1: no launch


def gather(x, w, g):
    """out[t][ostride*o + ophase] += w[:, :, taps[j]] @ x[t + dt[j]][istride*o + ioff[j]]: x [T][Fin][C], w [N][C][all taps]"""
    T, Fin, _ = x.shape
    assert Fin == g.Fin
    out = np.zeros((T, g.Fout, w.shape[0]))
    for t, o, j in itertools.product(range(T), range(g.No), range(g.ntaps)):
        ts, fi = t + g.dt[j], g.istride * o + g.ioff[j]
        if 0 <= ts < T and 0 <= fi < Fin:
            out[t, g.ostride * o + g.ophase] += w[:, :, g.taps[j]] @ x[ts, fi]          # (an output column past Fout raises)
    return out


@pytest.mark.parametrize("form", ["strided", "transposed"])
@pytest.mark.parametrize("sources", [1, 2])
@pytest.mark.parametrize("Fin", [4, 5, 8])
@pytest.mark.parametrize("kt, kf", [(1, 3), (2, 3), (2, 5)])
def test_adjoint_is_the_adjoint(form, sources, Fin, kt, kf):
    """<conv(x; W), y> == <x, sum of the adjoint launches (y; W^T)>, exactly: all operands are small integers.  Two
    sources: x is their concatenation, each source gets the adjoint launches with its own slice of W^T."""
    T, N, Cs = 3, 3, [2, 3][:sources]
    rng = np.random.default_rng(kt * 100 + kf * 10 + Fin)
    geoms = G.transposed(Fin, kt, kf) if form == "transposed" else (G.strided(Fin, kt, kf),)
    xs = [rng.integers(-3, 4, (T, Fin, C)).astype(np.float64) for C in Cs]
    w = rng.integers(-3, 4, (N, sum(Cs), kt * kf)).astype(np.float64)
    y = rng.integers(-3, 4, (T, geoms[0].Fout, N)).astype(np.float64)
    out = sum(gather(np.concatenate(xs, axis=2), w, g) for g in geoms)
    if len(geoms) == 2:                   # the phases write disjoint output columns, together all of them
        a, b = (np.abs(gather(np.ones_like(np.concatenate(xs, axis=2)), np.ones_like(w), g)).sum(axis=(0, 2)) > 0 for g in geoms)
        assert not (a & b).any() and (a | b).all()
    adj = G.adjoint(geoms)
    assert len(adj) == (1 if form == "transposed" else 2) and all((g.Fin, g.Fout) == (geoms[0].Fout, Fin) for g in adj)
    lhs, rhs, c_lo = float((out * y).sum()), 0.0, 0
    for x in xs:
        wt = np.ascontiguousarray(w[:, c_lo:c_lo + x.shape[2]].transpose(1, 0, 2))
        rhs += float((x * sum(gather(y, wt, g) for g in adj)).sum())
        c_lo += x.shape[2]
    assert lhs == rhs and (lhs != 0.0 or geoms[0].Fout == 0)          # ((2, 5) on 4 columns has no output column)


@pytest.mark.parametrize("C", [4, 16, 21])
def test_pack_taps_of_an_index_image_is_the_image_of_pack_taps(C):
    N, K, taps = 5, 6, (0, 2, 3, 5)
    w = np.random.default_rng(C).standard_normal((N, C, K)).astype(np.float32)
    idx = np.arange(w.size, dtype=np.int64).reshape(w.shape)
    wp, img = pack_taps(w, taps), pack_taps(idx, taps)
    assert wp.dtype == np.float32 and img.dtype == np.int64 and wp.shape == img.shape == (N, len(taps) * ((C + 15) // 16) * 16)
    assert ((img == -1) == (np.arange(img.shape[1]) % (((C + 15) // 16) * 16) >= C)).all()
    assert np.array_equal(np.where(img >= 0, w.reshape(-1)[np.maximum(img, 0)], np.float32(0)), wp)
    assert np.array_equal(pack_taps(idx.astype(np.int32), taps), img) and pack_taps(idx.astype(np.int32), taps).dtype == np.int32
