"""float64 restatement of the end of the training step (eabnet_amd.FlatAdam, csrc/optim.hip): the clip factor of
``clip_grad_norm_`` and one step of ``torch.optim.Adam`` (no amsgrad, maximize False), and the error bounds an fp32 implementation
of it must keep.  numpy only.

Bounds, with eps32 = 2^-23, every reference quantity in float64 and g_c = c g (+ weight_decay p):
    |m' - m'_ref| <= 4 eps32 (|m| + |g_c|)
    |v' - v'_ref| <= 4 eps32 (|v| + g_c^2)
    |p' - p'_ref| <= 32 eps32 (|p| + (lr / (1 - beta1^t)) (|m| + |g_c|) / (sqrt(v'_ref) / sqrt(1 - beta2^t) + eps))
    norm: relative error <= 2^-31 up to 2^22 elements, n 2^-53 beyond
They count fp32 roundings per output (the scalars are rounded to fp32 once, each operation once); the bound of p uses |m| + |g_c|
and not |m'|, so that a cancelling m' cannot break it."""
import numpy as np

EPS32 = 2.0 ** -23
NORM_REL = 2.0 ** -31
M_UNITS, V_UNITS, P_UNITS = 4.0, 4.0, 32.0


def norm_rel_bound(n: int) -> float:
    return NORM_REL if n <= 2 ** 22 else n * 2.0 ** -53


def grad_norm(grads) -> float:
    """sqrt of the sum of squares of every element of every array, float64"""
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads)))


def clip_coef(grads, max_norm) -> float:
    """c = min(1, max_norm / (norm + 1e-6)), NaN kept; no clipping (1) for max_norm None or <= 0"""
    if max_norm is None or max_norm <= 0:
        return 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.float64(max_norm) / (np.float64(grad_norm(grads)) + 1e-6)
    return float(r) if (r < 1.0 or np.isnan(r)) else 1.0


def adam_step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, c=1.0):
    """(p', m', v') after step t (1-based) from (p, m, v) with the raw gradient g; everything float64"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    gc = c * g + (weight_decay * p if weight_decay != 0 else 0.0)
    m1 = m + (gc - m) * (1.0 - b1)
    v1 = b2 * v + (1.0 - b2) * gc * gc
    denom = np.sqrt(v1) / np.sqrt(1.0 - b2 ** t) + eps
    p1 = p - (lr / (1.0 - b1 ** t)) * m1 / denom
    return p1, m1, v1


def bounds(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, c=1.0):
    """the three absolute bounds (arrays) at the reference point"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    gc = c * g + (weight_decay * p if weight_decay != 0 else 0.0)
    _, _, v1 = adam_step(p, g, m, v, t, lr, betas, eps, weight_decay, c)
    bm = M_UNITS * EPS32 * (np.abs(m) + np.abs(gc))
    bv = V_UNITS * EPS32 * (np.abs(v) + gc * gc)
    bp = P_UNITS * EPS32 * (np.abs(p) + (lr / (1.0 - b1 ** t)) * (np.abs(m) + np.abs(gc)) / (np.sqrt(v1) / np.sqrt(1.0 - b2 ** t) + eps))
    return bp, bm, bv


def check(got, p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, c=1.0):
    """got = (p', m', v') of an implementation.  Returns the largest error of each in units of eps32 times its bound's scale, i.e.
    (units_p, units_m, units_v); within the bounds iff units_p <= 32, units_m <= 4, units_v <= 4."""
    ref = adam_step(p, g, m, v, t, lr, betas, eps, weight_decay, c)
    bnd = bounds(p, g, m, v, t, lr, betas, eps, weight_decay, c)
    units = []
    for a, r, b, u in zip(got, ref, bnd, (P_UNITS, M_UNITS, V_UNITS)):
        err = np.abs(np.asarray(a, np.float64).reshape(-1) - r.reshape(-1))
        scale = b.reshape(-1) / u
        ok = scale > 0
        worst = float((err[ok] / scale[ok]).max()) if ok.any() else 0.0
        if (err[~ok] > 0).any():
            worst = float("inf")
        units.append(worst)
    return tuple(units)


def assert_within(got, *args, what="", **kw):
    up, um, uv = check(got, *args, **kw)
    print(f"{what}: p {up:.2f} / {P_UNITS:g}, m {um:.2f} / {M_UNITS:g}, v {uv:.2f} / {V_UNITS:g} units of 2^-23")
    assert up <= P_UNITS and um <= M_UNITS and uv <= V_UNITS, (what, up, um, uv)


def make_case(n: int, seed: int, scale: float = 1.0, with_state: bool = True, sign_of_p: bool = False):
    """seeded fp32 (p, g, m, v): non-zero gradients log-uniform in magnitude over [1e-2, 1] * scale with random signs (inside
    1e-8 .. 1e3 for scale in 1e-6 .. 1e3), every seventh element (3, 10, ..) exactly zero; m of the gradient's size, v of its square.
    sign_of_p: every gradient takes its parameter's sign, so that g + weight_decay p adds magnitudes.  The bounds are relative to
    |g_c|; an implementation that forms the two terms in fp32 (torch does) has an error of eps32 (|g| + |wd p|) in g_c, which is
    within them only where the terms do not cancel.  csrc/optim.hip forms g_c in fp64 and is tested with random signs."""
    r = np.random.default_rng(seed)
    p = r.standard_normal(n).astype(np.float32)
    mag = 10.0 ** r.uniform(-2.0, 0.0, n) * scale
    g = (mag * r.choice([-1.0, 1.0], n)).astype(np.float32)
    if sign_of_p:
        g = np.copysign(g, p).astype(np.float32)
    g[3::7] = 0.0
    if with_state:
        m = (0.3 * mag * r.standard_normal(n)).astype(np.float32)
        v = ((mag * r.uniform(0.2, 1.5, n)) ** 2).astype(np.float32)
    else:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    return p, g, m, v
