"""The C-ABI library loads on a machine without a GPU and exports every symbol
include/eabnet_hip.h declares (no compute calls here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "eabnet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(eab_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from eabnet_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/eabnet_hip.h but not exported"
    assert sorted(_lib.EXPORTS) == names, "ctypes binding and header disagree on the entry points"


def test_python_mirrors_every_header_constant():
    """Every EAB_(OP|EPI|XF|PREC|KORDER|ACT)_* #define of the header, and the limits and flag words beside them, has a Python
    mirror of the same name (without the EAB_ prefix) and value: the op kinds and enums in program.py, the ABI version in
    _lib.py.  No two op kinds share a value."""
    from eabnet_amd import _lib, program
    src = open(os.path.join(ROOT, "include", "eabnet_hip.h")).read()
    defines = {n: int(v, 0) for n, v in re.findall(r"^#define\s+EAB_(\w+)\s+(0[xX][0-9a-fA-F]+|\d+)\b", src, flags=re.M)}
    names = [n for n in defines if re.match(r"(OP|EPI|XF|PREC|KORDER|ACT)_", n)]
    assert len(names) >= 50
    for n in names + ["MAX_TAPS", "NB_SUMS_ZEROED", "NB_SUM_COPIES", "STORE_BF16"]:
        assert getattr(program, n, None) == defines[n], f"program.{n} != EAB_{n} = {defines[n]}"
    assert _lib.ABI_VERSION == defines["ABI_VERSION"] and _lib.MAX_TAPS == defines["MAX_TAPS"]
    kinds = [defines[n] for n in names if n.startswith("OP_")]
    assert len(set(kinds)) == len(kinds), "two EAB_OP_* share a value"


def test_binding_handshake_and_error_strings():
    from eabnet_amd import _lib
    lib = _lib.load()                      # checks ABI version + struct sizes
    assert lib.eab_abi_version() == _lib.ABI_VERSION
    assert b"invalid argument" in lib.eab_error_string(1)
    assert lib.eab_conv_tiles(401, 79, 128) == (401 * 79 + 127) // 128
    assert lib.eab_conv_tiles(401, 79, 100) == -1


def test_argument_validation_happens_before_any_launch():
    """Null pointers / bad shapes are rejected on the host (EAB_EINVAL) -- safe to
    call without a GPU because nothing is launched."""
    from eabnet_amd import _lib
    lib = _lib.load()
    assert lib.eab_filter_sum_f32(None, None, None, 1, 1, 1, 1, None) == 1
    assert lib.eab_stft_compress_f32(None, None, None, None, 1, 1, 1000, 320, 160, 0, None) == 1
    d = _lib.ConvDesc()
    assert lib.eab_conv_f32(ctypes.byref(d), None) == 1
    assert lib.eab_run_program(None, 0, None) == 1
    with pytest.raises(_lib.EabError):
        _lib.check(1, "x")


def test_product_path_refuses_cpu_tensors():
    import torch
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=2)
    with torch.no_grad(), pytest.raises(eabnet_amd._lib.EabError):
        net(torch.zeros(1, 4, 161, 2, 2))
    with pytest.raises(eabnet_amd._lib.EabError):
        eabnet_amd.filter_and_sum(torch.zeros(1, 1, 1, 1, 2), torch.zeros(1, 1, 1, 1, 2))


def test_differentiable_calls_have_no_cpu_or_operator_fallback():
    """One backend: a differentiable call on CPU tensors is refused like an inference call (the PyTorch-operator evaluation
    that used to serve it is test infrastructure now, tests/operator_path.py), and the package does not import it."""
    import torch
    import eabnet_amd
    net = eabnet_amd.EaBNet(M=2, p=1, q=1)
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        net(torch.zeros(1, 4, 161, 2, 2))                # grad enabled, parameters require grad
    gag = eabnet_amd.GaGNet(p=1, q=1, dilas=(1,))
    with pytest.raises(eabnet_amd._lib.EabError, match="no CPU fallback"):
        gag(torch.zeros(1, 2, 4, 161), torch.zeros(1, 2, 4, 161))
    assert not hasattr(net, "use_hip_training")
    import re
    pkg = os.path.join(ROOT, "eabnet_amd")
    assert not os.path.exists(os.path.join(pkg, "autograd_path.py"))
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            bad = re.findall(r"^\s*(?:from|import)\s+\S*(?:autograd_path|operator_path|oracle)\b.*$", src, re.M)
            assert not bad, (fn, bad)


def test_operator_comparator_matches_oracle_on_cpu():
    """tests/operator_path.py (the PyTorch-operator comparator of the GPU training tests and of bench.py's in-run check)
    against the oracle; runs on CPU because it is plain PyTorch."""
    import torch
    import paramgen
    import eabnet_amd
    from operator_path import OperatorPath
    from eabnet_amd.spec import NetConfig, param_specs
    from oracle import eabnet_oracle as orc
    cfg = NetConfig(M=3, p=2, q=2)
    P = {k: torch.from_numpy(v) for k, v in paramgen.make_params(param_specs(cfg), 160).items()}
    net = eabnet_amd.EaBNet(M=3, p=2, q=2)
    net.load_state_dict(P, strict=True)
    x = torch.from_numpy(paramgen.make_spec_input(2, 9, 161, 3, 161))
    y = OperatorPath(net)(x)                             # grad enabled -> the comparator's operators
    assert y.requires_grad
    with torch.no_grad():
        ref = orc.eabnet_forward(P, x, p=2, q=2)
    assert float((y.detach() - ref).abs().max() / ref.abs().max()) < 1e-5
    y.square().mean().backward()
    assert all(p.grad is not None for p in net.parameters())


def test_state_dict_round_trip_with_reference_keys():
    import json
    import torch
    import eabnet_amd
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "keys_M8.json")))
    net = eabnet_amd.EaBNet(M=8)
    sd = net.state_dict()
    assert list(sd.keys()) == [k for k, _ in ref]
    assert all(tuple(sd[k].shape) == tuple(s) for k, s in ref)
    assert eabnet_amd.numParams(net) == 2_835_920
    other = eabnet_amd.EaBNet(M=8)
    other.load_state_dict({k: torch.randn_like(v) for k, v in sd.items()}, strict=True)
    # wrapper prefix used by EaBNetWithPostNet (reference EaBNet.py:130)
    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.eabnet = eabnet_amd.EaBNet(M=8)
    assert all(k.startswith("eabnet.") for k in Wrap().state_dict())
    # reference default is M=9
    assert eabnet_amd.EaBNet().M == 9


def _variants():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "keys_variants.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(_variants()))
def test_constructor_variants_keep_reference_keys_and_train(name):
    """Every constructor branch: the module's state dict (parameters AND BatchNorm buffers, in the
    reference's order), and the operator comparator (tests/operator_path.py) against the reference's output."""
    import numpy as np
    from operator_path import OperatorPath
    import torch
    import paramgen
    import eabnet_amd
    from eabnet_amd.spec import NetConfig, param_specs
    e = _variants()[name]
    g = np.load(os.path.join(ROOT, "tests", "golden", f"var_{name}.npz"))
    net = eabnet_amd.EaBNet(M=e["M"], **e["kwargs"])
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == e["keys"]
    specs = param_specs(NetConfig(M=e["M"], **e["kwargs"]))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in paramgen.make_params(specs, int(g["param_seed"])).items()},
                        strict=True)
    net.eval()
    x = torch.from_numpy(paramgen.make_spec_input(2, 20, 161, e["M"], int(g["input_seed"])))
    y = OperatorPath(net)(x)
    ref = torch.from_numpy(g["out"])
    assert y.shape == ref.shape and y.requires_grad
    assert float((y.detach() - ref).abs().max() / ref.abs().max()) < 1e-5
    y.square().mean().backward()
    assert all(p.grad is not None for p in net.parameters())


def test_batchnorm_training_mode_updates_running_statistics():
    """The comparator's norm_type='BN' in train mode follows nn.BatchNorm: batch statistics, momentum-0.1 update of
    the buffers, step counter; this holds under no_grad too.  (The HIP programs' train mode is pinned on the GPU by
    tests/golden/bn_train.npz and test_hip_training_batchnorm_train_mode_vs_oracle_autograd.)"""
    import torch
    import eabnet_amd
    from operator_path import OperatorPath
    net = eabnet_amd.EaBNet(M=2, p=1, q=1, norm_type="BN").train()
    key = "en.meta_unet_list.0.in_conv.1.norm"
    before = net.state_dict()[f"{key}.running_mean"].clone()
    with torch.no_grad():
        OperatorPath(net)(torch.randn(2, 6, 161, 2, 2))
    sd = net.state_dict()
    assert int(sd[f"{key}.num_batches_tracked"]) == 1
    assert not torch.equal(sd[f"{key}.running_mean"], before)
    assert eabnet_amd.numParams(net) == sum(p.numel() for p in net.parameters())


def _gag_variants():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "keys_gagnet.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(_gag_variants()))
def test_gagnet_module_keys_and_training_path(name):
    """eabnet_amd.GaGNet: the reference's state-dict inventory, and the operator comparator against
    the reference's stage outputs (CPU, plain PyTorch)."""
    import numpy as np
    from operator_path import OperatorPath
    import torch
    import paramgen
    import eabnet_amd
    e = _gag_variants()[name]
    g = np.load(os.path.join(ROOT, "tests", "golden", f"gag_{name}.npz"))
    net = eabnet_amd.GaGNet(**e["kwargs"])
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == e["keys"]
    net.load_state_dict({k: torch.from_numpy(v) for k, v in
                         paramgen.make_params(eabnet_amd.gag_param_specs(net.cfg), int(g["param_seed"])).items()}, strict=True)
    net.eval()
    mk = lambda seed: torch.from_numpy(paramgen.make_spec_input(2, 14, 161, 1, seed)[..., 0, :]).permute(0, 3, 1, 2)  # noqa: E731
    outs = OperatorPath(net)(mk(int(g["inpt_seed"])), mk(int(g["pre_seed"])))
    assert len(outs) == net.q and outs[-1].requires_grad
    for j, o in enumerate(outs):
        ref = torch.from_numpy(g[f"out{j}"])
        assert o.shape == ref.shape
        # same ATen operators as the reference, but on permuted-view inputs: summation orders differ in
        # the last bit and the post-filter amplifies that ~40x per the conditioning noted in DESIGN.md
        assert float((o.detach() - ref).abs().max() / ref.abs().max()) < 5e-5
    label = torch.zeros_like(outs[-1])
    eabnet_amd.stagewise_com_mag_mse_loss(outs, label.detach(), [14, 9]).backward()
    assert all(p.grad is not None for p in net.parameters())
    if name == "default":
        assert eabnet_amd.numParams(net) == 5_950_697
        with torch.no_grad(), pytest.raises(eabnet_amd._lib.EabError):
            net(mk(1), mk(2))                         # inference without the GPU: no fallback


def test_two_stage_wrapper_keys_and_output_dictionary(monkeypatch):
    """EaBNetWithPostNet (EaBNet.py:127-155): ``eabnet.`` / ``postnet.`` prefixes, freeze switch and the
    output dictionary; the reference's factory moves the post-filter to the GPU, patched out here."""
    import argparse
    import torch
    import eabnet_amd
    monkeypatch.setattr(eabnet_amd.GaGNet, "cuda", lambda self, *a, **k: self)
    args = argparse.Namespace(
        k1=(2, 3), k2=(1, 3), c=64, M=3, embed_dim=64, kd1=5, cd1=64, d_feat=256, p=1, q=1, is_causal=True, is_u2=True,
        bf_type="lstm", topo_type="mimo", intra_connect="cat", norm_type="IN", ref_mic=1, freeze_eabnet=False,
        gagnet_k1=(2, 3), gagnet_k2=(1, 3), gagnet_c=64, gagnet_kd1=3, gagnet_cd1=64, gagnet_d_feat=256, gagnet_p=1,
        gagnet_q=2, gagnet_dilas=[1, 2], gagnet_fft_num=320, gagnet_is_u2=True, gagnet_is_causal=True,
        gagnet_is_squeezed=False, gagnet_acti_type="sigmoid", gagnet_intra_connect="cat", gagnet_norm_type="IN")
    net = eabnet_amd.make_eabnet_with_postnet(args)
    keys = list(net.state_dict())
    assert all(k.startswith(("eabnet.", "postnet.")) for k in keys)
    assert [k[7:] for k in keys if k.startswith("eabnet.")] == list(eabnet_amd.EaBNet(M=3, p=1, q=1).state_dict())
    from operator_path import OperatorPath
    out = OperatorPath(net)(torch.randn(1, 6, 161, 3, 2))      # parameters require grad -> the comparator's operators (CPU is fine)
    assert set(out) == {"esti0_stft", "esti1_stft_list", "esti_stft"}
    assert out["esti0_stft"].shape == (1, 2, 6, 161) and out["esti_stft"].shape == (1, 2, 6, 161)
    assert len(out["esti1_stft_list"]) == 2 and out["esti1_stft_list"][0].shape == (1, 2, 161, 6)
    out["esti_stft"].sum().backward()
    assert all(p.grad is None for p in net.eabnet.parameters())        # the post-filter sees esti0.detach()
    net.freeze_eabnet()
    assert not any(p.requires_grad for p in net.eabnet.parameters())
    with pytest.raises(eabnet_amd._lib.EabError):      # the module itself: HIP programs only, no CPU fallback
        net(torch.randn(1, 6, 161, 3, 2))


def test_param_fingerprint_sees_every_kind_of_weight_change():
    """The packed-weight cache key (model._param_fingerprint) must change for an in-place update, a ``.data =``
    re-assignment of a MIDDLE tensor, ``load_state_dict(assign=True)`` and a dtype round trip of one
    submodule -- and replicas (eabnet_amd.Pipeline) must see the same changes."""
    import torch
    import eabnet_amd
    from eabnet_amd.model import _replica
    net = eabnet_amd.EaBNet(M=2, p=1, q=1)
    rep = _replica(net)
    names = [n for n, _ in net.named_parameters()]
    mid = names[len(names) // 2]
    seen = {net._param_fingerprint()}

    def changed():
        fp, fr = net._param_fingerprint(), rep._param_fingerprint()
        assert fp == fr, "replica and model disagree"
        new = fp not in seen
        seen.add(fp)
        return new

    assert not changed()
    with torch.no_grad():
        net.get_parameter(mid).mul_(1.5)                              # in place
    assert changed()
    p = net.get_parameter(mid)
    p.data = p.data.clone()                                           # re-assignment, version counter untouched
    assert changed()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(sd, strict=True, assign=True)                 # new Parameter objects in every slot
    assert changed()
    net.stcns.double().float()                                        # dtype round trip of one submodule
    assert changed()
    assert not changed()


def test_two_stage_loss_matches_reference_value():
    """eabnet_with_postnet_loss (reference EaBNet.py:642-650) on CPU tensors against the reference's own value."""
    import numpy as np
    import torch
    import eabnet_amd
    import paramgen
    gd = os.path.join(ROOT, "tests", "golden")
    g, gl = np.load(os.path.join(gd, "postnet_M4_T12.npz")), np.load(os.path.join(gd, "loss_postnet.npz"))
    output = {"esti0_stft": torch.from_numpy(g["esti0"]), "esti1_stft_list": [torch.from_numpy(g[f"stage{j}"]) for j in range(3)]}
    label = torch.from_numpy(paramgen.make_spec_input(1, 12, 161, 1, int(gl["label_seed"]))[..., 0, :]).permute(0, 3, 1, 2).contiguous()
    l = eabnet_amd.eabnet_with_postnet_loss(output, label, [12])
    assert set(l) == {"eabnet", "postnet", "final"}
    for k in l:
        assert abs(float(l[k]) - float(gl[f"full/{k}"])) <= 1e-5 * abs(float(gl[f"full/{k}"])), k
