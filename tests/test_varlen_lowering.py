"""Per-utterance lengths and length buckets, host side (no GPU): the bucket choice, the validation of ``lengths=``, the
refusals that are decided before anything reaches the device, and the ``varlen`` flag of the lowering."""
import numpy as np
import pytest
import torch

import paramgen
from eabnet_amd import model as mdl
from eabnet_amd import program as prg
from eabnet_amd.spec import NetConfig, param_specs


def test_auto_buckets_are_powers_of_two_from_64_to_8192():
    assert mdl.AUTO_BUCKETS == (64, 128, 256, 512, 1024, 2048, 4096, 8192)


@pytest.mark.parametrize("T,cap", [(1, 64), (64, 64), (65, 128), (301, 512), (1024, 1024), (1025, 2048), (8192, 8192),
                                   (8193, None)])
def test_bucket_is_the_smallest_cap_not_below_T(T, cap):
    assert mdl.bucket_for(T, mdl.AUTO_BUCKETS) == cap


def test_bucket_choice_of_an_explicit_tuple():
    net = mdl.EaBNet(M=2)
    net.length_buckets = (100, 300)
    assert net._bucket_caps() == (100, 300)
    assert [mdl.bucket_for(T, net._bucket_caps()) for T in (1, 100, 101, 300, 301)] == [100, 100, 300, 300, None]
    # a call of T frames runs in its bucket with every utterance T frames long
    with torch.no_grad():
        assert net._varlen_call(137, 2, None, needs_graph=False) == (300, 137)
        assert net._varlen_call(301, 2, None, needs_graph=False) is None          # above the largest cap: exact shape
        assert net._varlen_call(137, 2, [5, 137], needs_graph=False) == (300, [5, 137])
    net.length_buckets = None
    assert net._varlen_call(137, 2, None, needs_graph=False) is None              # default: today's path
    assert net._varlen_call(137, 2, [5, 137], needs_graph=False) == (137, [5, 137])


@pytest.mark.parametrize("bad", ["linear", (64, 64), (128, 64), (0, 64), ()])
def test_malformed_buckets_are_refused(bad):
    net = mdl.EaBNet(M=2)
    net.length_buckets = bad
    with pytest.raises(ValueError):
        net._bucket_caps()


def test_non_causal_configuration_with_buckets_takes_the_exact_shape_path():
    net = mdl.EaBNet(M=2, is_causal=False)
    net.length_buckets = "auto"
    assert net._varlen_call(100, 1, None, needs_graph=False) is None


@pytest.mark.parametrize("lengths", [[0, 5], [5, 11], [5], [5, 5, 5], torch.tensor([0, 3]), torch.tensor([3, 3, 3]),
                                     torch.tensor([2.0, 3.0])])
def test_lengths_validation_raises_value_error(lengths):
    with pytest.raises(ValueError):
        mdl.check_lengths(lengths, 2, 10)
    net = mdl.EaBNet(M=2).eval()
    with torch.no_grad(), pytest.raises(ValueError):
        net(torch.zeros(2, 10, 161, 2, 2), lengths=lengths)                    # checked before anything reaches the device


def test_lengths_validation_accepts_sequences_and_integer_tensors():
    assert mdl.check_lengths([1, 10], 2, 10) == [1, 10]
    assert mdl.check_lengths(torch.tensor([4, 7], dtype=torch.int64), 2, 10) == [4, 7]
    assert mdl.check_lengths(np.array([3, 2], dtype=np.int32), 2, 10) == [3, 2]


def test_lengths_on_a_non_causal_configuration_are_refused_with_the_reason():
    net = mdl.EaBNet(M=2, is_causal=False).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="is_causal=True"):
        net(torch.zeros(1, 10, 161, 2, 2), lengths=[4])


def test_lengths_under_autograd_are_refused():
    net = mdl.EaBNet(M=2)
    with pytest.raises(NotImplementedError, match="lengths"):
        net(torch.zeros(1, 10, 161, 2, 2), lengths=[4])
    bn = mdl.EaBNet(M=2, norm_type="BN").train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="lengths"):
        bn(torch.zeros(1, 10, 161, 2, 2), lengths=[4])                         # BatchNorm in train mode


def test_gagnet_lengths_validation_and_refusal():
    gag = mdl.GaGNet(p=1, q=1, dilas=(1,)).eval()
    x = torch.zeros(2, 2, 10, 161)
    with torch.no_grad(), pytest.raises(ValueError):
        gag(x, x, lengths=[3, 0])
    gnc = mdl.GaGNet(p=1, q=1, dilas=(1,), is_causal=False).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="is_causal=True"):
        gnc(x, x, lengths=[3, 3])


def test_varlen_lowering_flag_and_refusals():
    cfg = NetConfig(M=2, p=1, q=1)
    params = paramgen.make_params({k: v for k, v in param_specs(cfg).items() if v.kind != "bn_count"}, 0)
    prog = prg.lower(cfg, params, 2, 40, varlen=True)
    assert prog.varlen and prog.T == 40 and prog.chunk == 0
    exact = prg.lower(cfg, params, 2, 40)
    assert not exact.varlen
    assert [type(o) for o in prog.ops] == [type(o) for o in exact.ops]     # same op list: only the binding adds the lengths
    with pytest.raises(NotImplementedError, match="is_causal"):
        prg.lower(NetConfig(M=2, p=1, q=1, is_causal=False),
                  paramgen.make_params({k: v for k, v in param_specs(NetConfig(M=2, p=1, q=1, is_causal=False)).items()
                                        if v.kind != "bn_count"}, 0), 1, 40, varlen=True)
    cfg_bn = NetConfig(M=2, p=1, q=1, norm_type="BN")
    params_bn = paramgen.make_params({k: v for k, v in param_specs(cfg_bn).items() if v.kind != "bn_count"}, 0)
    with pytest.raises(NotImplementedError, match="offline"):
        prg.lower(cfg_bn, params_bn, 1, 40, chunk=1, varlen=True)


def test_pipeline_replicas_do_not_share_bucketed_programs():
    net = mdl.EaBNet(M=2)
    net.length_buckets = "auto"
    rep = mdl._replica(net)
    assert rep.length_buckets is None and rep._varlen_bound is not net._varlen_bound
