"""The contract of the fused clip + Adam step on the CPU: tests/optim_ref.py against torch.optim.Adam itself, and
everything of eabnet_amd.FlatAdam that needs no device -- the flat buffers, torch.optim.Adam's checkpoint format in both
directions, the refusal to step on CPU tensors, and the argument checks of the two entry points (nothing is launched)."""
import ctypes

import numpy as np
import pytest
import torch

import optim_ref as R

SIZES5 = (18, 1, 1025, 7, 64)


def _torch_adam_step(p, g, m, v, t, lr, wd):
    """one torch.optim.Adam(foreach=False) step number t from injected state"""
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=lr, weight_decay=wd, foreach=False)
    opt.state[tp] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
    tp.grad = torch.from_numpy(g.copy())
    opt.step()
    s = opt.state[tp]
    assert int(s["step"]) == t
    return tp.detach().numpy(), s["exp_avg"].numpy(), s["exp_avg_sq"].numpy()


@pytest.mark.parametrize("n,t,scale,wd", [(1025, 1, 1.0, 0.0), (70_001, 2, 1e-6, 1e-2), (70_001, 7, 1e3, 1e-2),
                                          (300_007, 1000, 1.0, 0.0), (2_838_610, 7, 1e-3, 1e-2)])
def test_torch_adam_single_steps_stay_within_the_bounds(n, t, scale, wd):
    p, g, m, v = R.make_case(n, 11 + t, scale, with_state=t > 1, sign_of_p=wd != 0)          # (torch forms g + wd p in fp32)
    nz = np.abs(g[g != 0])
    assert nz.min() >= 1e-8 and nz.max() <= 1e3 and (g[3::7] == 0).all()
    got = _torch_adam_step(p, g, m, v, t, 5e-4, wd)
    R.assert_within(got, p, g, m, v, t, 5e-4, weight_decay=wd, what=f"torch.optim.Adam n {n} t {t} scale {scale:g} wd {wd:g}")


def test_clip_factor_of_one_is_no_clipping():
    p, g, m, v = R.make_case(1025, 3, 1e-2)
    norm = R.grad_norm([g])
    assert norm < 1.0 and R.clip_coef([g], 1.0) == 1.0 and R.clip_coef([g], None) == 1.0
    a = R.adam_step(p, g, m, v, 3, 5e-4, c=R.clip_coef([g], 1.0))
    b = R.adam_step(p, g, m, v, 3, 5e-4)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = R.clip_coef([g, g], 0.25 * norm)
    assert abs(c - 0.25 * norm / (np.sqrt(2.0) * norm + 1e-6)) < 1e-15
    bad = g.copy()
    bad[5] = np.nan
    assert np.isnan(R.clip_coef([bad], 1.0)) and R.clip_coef([bad], None) == 1.0


def _five(seed=0):
    r = np.random.default_rng(seed)
    out = []
    for n in SIZES5:
        t = torch.from_numpy(r.standard_normal(n).astype(np.float32))
        out.append(torch.nn.Parameter(t.reshape(8, 8) if n == 64 else t))
    return out


def test_flat_adam_parameters_become_slices_of_one_buffer():
    import eabnet_amd
    ps = _five()
    frozen = torch.nn.Parameter(torch.ones(3), requires_grad=False)
    before = [p.detach().clone() for p in ps]
    ptr_frozen = frozen.data_ptr()
    opt = eabnet_amd.FlatAdam(ps[:2] + [frozen] + ps[2:], lr=1e-3)
    assert isinstance(opt, torch.optim.Optimizer)
    base = ps[0].data_ptr()
    off = 0
    for p, b in zip(ps, before):
        assert p.data_ptr() == base + 4 * off and torch.equal(p.detach(), b) and p.shape == b.shape and p.requires_grad
        off += p.numel()
    assert frozen.data_ptr() == ptr_frozen and frozen not in opt.state
    for p in ps:
        s = opt.state[p]
        assert set(s) == {"step", "exp_avg", "exp_avg_sq"} and s["exp_avg"].shape == p.shape and s["exp_avg_sq"].shape == p.shape
    assert opt.state[ps[1]]["exp_avg"].data_ptr() == opt.state[ps[0]]["exp_avg"].data_ptr() + 4 * SIZES5[0]
    for bad in ("amsgrad", "maximize", "capturable", "foreach", "fused"):
        with pytest.raises(TypeError):
            eabnet_amd.FlatAdam(_five(), **{bad: True})


def test_flat_adam_state_dict_has_torch_adams_keys_and_shapes():
    import eabnet_amd
    ps, qs = _five(), _five()
    ref = torch.optim.Adam(qs, lr=1e-3)
    for q in qs:
        q.grad = torch.ones_like(q)
    ref.step()
    a, b = eabnet_amd.FlatAdam(ps, lr=1e-3).state_dict(), ref.state_dict()
    assert set(a) == set(b) and len(a["param_groups"]) == 1
    assert set(a["param_groups"][0]) == set(b["param_groups"][0]) and a["param_groups"][0]["params"] == b["param_groups"][0]["params"]
    assert set(a["state"]) == set(b["state"])
    for k in b["state"]:
        assert set(a["state"][k]) == set(b["state"][k])
        for name in ("exp_avg", "exp_avg_sq", "step"):
            assert a["state"][k][name].shape == b["state"][k][name].shape and a["state"][k][name].dtype == b["state"][k][name].dtype


def test_torch_adam_state_loads_into_flat_adam_and_back():
    import eabnet_amd
    qs = _five(1)
    ref = torch.optim.Adam(qs, lr=2e-3, betas=(0.8, 0.99), weight_decay=1e-2)
    r = np.random.default_rng(5)
    for _ in range(3):
        for q in qs:
            q.grad = torch.from_numpy(r.standard_normal(tuple(q.shape)).astype(np.float32))
        ref.step()
    sd = ref.state_dict()
    ps = _five(1)
    opt = eabnet_amd.FlatAdam(ps, lr=5e-4)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert g["lr"] == 2e-3 and tuple(g["betas"]) == (0.8, 0.99) and g["weight_decay"] == 1e-2
    m0 = opt.state[ps[0]]["exp_avg"]
    off = 0
    for p, q in zip(ps, qs):                                  # the moments are views of the flat buffers again, with torch's values
        s = opt.state[p]
        assert s["exp_avg"].data_ptr() == m0.data_ptr() + 4 * off
        assert torch.equal(s["exp_avg"], ref.state[q]["exp_avg"]) and torch.equal(s["exp_avg_sq"], ref.state[q]["exp_avg_sq"])
        off += p.numel()
    back = opt.state_dict()
    for k in sd["state"]:
        assert int(back["state"][k]["step"]) == 3 == int(sd["state"][k]["step"])
        assert torch.equal(back["state"][k]["exp_avg"], sd["state"][k]["exp_avg"])
        assert torch.equal(back["state"][k]["exp_avg_sq"], sd["state"][k]["exp_avg_sq"])
    fresh = torch.optim.Adam(_five(1), lr=1.0)
    fresh.load_state_dict(back)                               # and torch.optim.Adam takes FlatAdam's state dict, then steps
    fs, rs = fresh.state_dict(), ref.state_dict()
    for k in rs["state"]:
        assert all(torch.equal(fs["state"][k][n], rs["state"][k][n]) for n in ("exp_avg", "exp_avg_sq"))
        assert int(fs["state"][k]["step"]) == 3
    assert fresh.param_groups[0]["lr"] == 2e-3
    for q in fresh.param_groups[0]["params"]:
        q.grad = torch.ones_like(q)
    fresh.step()
    assert all(int(fresh.state[q]["step"]) == 4 for q in fresh.param_groups[0]["params"])


def test_flat_adam_step_on_cpu_tensors_is_refused():
    import eabnet_amd
    ps = _five()
    opt = eabnet_amd.FlatAdam(ps, max_grad_norm=1.0)
    assert opt.step() is None                                 # no gradient anywhere: nothing to do, as in torch
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        opt.step()
    ps[2].grad = None
    with pytest.raises(RuntimeError, match="parameter 2"):
        opt.step()


def test_a_refused_state_dict_changes_nothing():
    import eabnet_amd
    ps = _five(2)
    opt = eabnet_amd.FlatAdam(ps, lr=5e-4)
    good = opt.state_dict()
    views = [opt.state[p]["exp_avg"].data_ptr() for p in ps]
    uneven = {"state": {i: {k: v.clone() for k, v in s.items()} for i, s in good["state"].items()}, "param_groups": good["param_groups"]}
    uneven["state"][3]["step"] = torch.tensor(5.0)
    partial = {"state": {i: s for i, s in good["state"].items() if i != 1}, "param_groups": good["param_groups"]}
    amsgrad = {"state": good["state"], "param_groups": [dict(good["param_groups"][0], amsgrad=True)]}
    for bad, what in ((uneven, "different steps"), (partial, "some parameters"), (amsgrad, "amsgrad")):
        with pytest.raises(ValueError, match=what):
            opt.load_state_dict(bad)
        assert [opt.state[p]["exp_avg"].data_ptr() for p in ps] == views and not opt.param_groups[0]["amsgrad"]


def test_load_state_dict_assign_true_leaves_the_optimizer_with_the_old_parameters():
    """nn.Module.load_state_dict(assign=True) puts NEW Parameter objects into the module, which no optimizer sees (torch's
    neither): the old ones get no gradient any more, so the group rests and its step count stays.  A new optimizer is needed."""
    import eabnet_amd
    net = torch.nn.Linear(5, 3)
    opt = eabnet_amd.FlatAdam(net.parameters(), lr=5e-4)
    old = list(net.parameters())
    net.load_state_dict({k: v.clone() for k, v in net.state_dict().items()}, assign=True)
    new = list(net.parameters())
    assert all(a is not b for a, b in zip(old, new))
    net(torch.ones(2, 5)).sum().backward()
    assert all(q.grad is not None for q in new) and all(q.grad is None for q in old)
    assert opt.step() is None and opt.last_path is None                   # nothing stepped, on any device
    assert all(int(s["step"]) == 0 for s in opt.state_dict()["state"].values())
    again = eabnet_amd.FlatAdam(net.parameters(), lr=5e-4)                # the way on: the new parameters move into flat buffers
    assert new[1].data_ptr() == new[0].data_ptr() + 4 * new[0].numel() and again.state[new[0]]["exp_avg"].shape == new[0].shape


def test_optim_entry_points_validate_before_any_launch():
    from eabnet_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    out = (ctypes.c_double * 4)()
    a = ctypes.addressof(buf)
    o = ctypes.addressof(out)
    seg = lambda n=16, grad=a, param=a: _lib.OptimSegment(param, grad, a, a, n)          # noqa: E731
    table = lambda *s: (_lib.OptimSegment * len(s))(*s)                                  # noqa: E731
    adam = lambda t, n, partial=o, npartial=1: lib.eab_adam_clip_f32(t, n, partial, npartial, 1.0, 1e-3, 0.9, 0.999, 1.0, 1e-8, 0.0,  # noqa: E731
                                                                     o, None)
    assert lib.eab_grad_sumsq_f64(None, 1, o, 1, None) == 1
    assert lib.eab_grad_sumsq_f64(table(seg()), 1, None, 1, None) == 1
    assert lib.eab_grad_sumsq_f64(table(seg(grad=None)), 1, o, 1, None) == 1
    assert lib.eab_grad_sumsq_f64(table(seg(n=-1)), 1, o, 1, None) == 1
    assert lib.eab_grad_sumsq_f64(table(seg()), 0, o, 1, None) == 1
    assert lib.eab_grad_sumsq_f64(table(*[seg()] * 9), 9, o, 4, None) == 1
    assert lib.eab_grad_sumsq_f64(table(seg()), 1, o, 0, None) == 1                      # partial buffer too small
    assert adam(None, 1) == 1
    assert adam(table(seg(param=None)), 1) == 1
    assert adam(table(seg(grad=None)), 1) == 1
    assert adam(table(seg(n=-1)), 1) == 1
    assert adam(table(*[seg()] * 9), 9) == 1
    assert adam(table(seg()), 1, partial=None) == 1
    assert adam(table(seg()), 1, npartial=-1) == 1
