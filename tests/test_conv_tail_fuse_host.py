"""Host side of K27 (`component_visualization/_bn_fuse.py`): the graph of an owner whose residual tail normalises the output of
a 64 -> 256 channel pointwise convolution — what its generated code calls, which convolutions are and are not taken, the
single-consumer rules, and what gates the graph."""
import pytest
import torch
import torch.nn as nn

import synth
from semanticlens_amd import _native as N
from semanticlens_amd.component_visualization import _bn_fuse, aggregators
from semanticlens_amd.component_visualization.activation_caching import ActMaxCache


def _plan_of(block):
    plan = _bn_fuse._Plan(block)
    by_owner = {ref(): i for i, (ref, _, _) in enumerate(plan.parents)}
    return plan, by_owner


def test_an_identity_bottleneck_gets_a_graph_without_conv3():
    block = synth.Bottleneck(256, 64).eval()
    plan, by_owner = _plan_of(block)
    gm, gates = plan.convs[by_owner[block]]
    code = gm.code
    print(code)
    assert len(gates) == 1 and isinstance(gates[0], _bn_fuse._FusedConv)
    assert gates[0].conv is block.conv3 and gates[0].single.site.bn is block.bn3 and gates[0].single.bn_first
    # conv3, bn3, the add and the relu are one call on conv3's input and the identity
    assert "self.conv3" not in code and "self.bn" not in code and "self.relu" not in code
    assert code.count("self._sl_fused_") == 3 and "self._sl_fused_2(_sl_fused_1, x)" in code
    assert "self.conv1(x)" in code and "self.conv2(_sl_fused_0)" in code
    # the graphs of K16 / K19 are what they were
    assert "self._sl_fused_2(conv3, x)" in plan.parents[by_owner[block]][1].code and plan.duals == {}


def test_a_bottleneck_with_a_pointwise_downsample_gets_one_call_for_both_convolutions():
    block = synth.Bottleneck(64, 64).eval()  # downsample = Sequential(conv 64 -> 256, bn)
    plan, by_owner = _plan_of(block)
    gm, gates = plan.convs[by_owner[block]]
    code = gm.code
    print(code)
    assert len(gates) == 1 and isinstance(gates[0], _bn_fuse._FusedConvDual)
    fused = gates[0]
    assert fused.conv is block.conv3 and fused.shortcut_conv is block.downsample[0]
    assert fused.dual.shortcut.bn is block.downsample[1] and fused.dual.single.site.bn is block.bn3
    assert "self.conv3" not in code and "self.downsample" not in code and "self.bn" not in code and "self.relu" not in code
    assert code.count("self._sl_fused_") == 3 and "self._sl_fused_2(_sl_fused_1, x)" in code
    # K19's graph still calls both convolutions as modules
    dual = plan.duals[by_owner[block]][0].code
    assert 'getattr(self.downsample, "0")(x)' in dual and "self._sl_fused_2(conv3, downsample_0)" in dual


def test_resnet50_has_three_such_owners_and_resnet18_none():
    p50 = _bn_fuse._Plan(synth.resnet50())
    owners = sorted(type(p50.parents[i][0]()).__name__ for i in p50.convs)
    kinds = sorted(type(g).__name__ for _, gates in p50.convs.values() for g in gates)
    assert owners == ["Bottleneck"] * 3 and kinds == ["_FusedConv", "_FusedConv", "_FusedConvDual"]
    assert len(p50.duals) == 4  # as before
    assert _bn_fuse._Plan(synth.resnet18()).convs == {}


class _Tail(nn.Module):
    def __init__(self, conv, mode="plain", shortcut=None):
        super().__init__()
        self.conv, self.bn, self.relu, self.mode = conv, nn.BatchNorm2d(conv.out_channels), nn.ReLU(), mode
        if shortcut is not None:
            self.shortcut = shortcut

    def forward(self, x, idt):
        c = self.conv(x)
        out = self.bn(c)
        if self.mode == "conv_read_twice":
            return self.relu(out + idt) + c
        if self.mode == "identity_left":
            return self.relu(idt + out)
        if self.mode == "no_add":
            return self.relu(out)
        return self.relu(out + idt)


def _convs(block):
    return _bn_fuse._Plan(block.eval()).convs


def test_convolutions_that_are_and_are_not_taken():
    assert len(_convs(_Tail(nn.Conv2d(64, 256, 1, bias=False)))) == 1
    assert len(_convs(_Tail(nn.Conv2d(64, 256, (1, 1), stride=(1, 1), padding=0, bias=False)))) == 1
    for name, conv in (("stride 2", nn.Conv2d(64, 256, 1, stride=2, bias=False)),
                       ("bias", nn.Conv2d(64, 256, 1)),
                       ("groups", nn.Conv2d(64, 256, 1, groups=2, bias=False)),
                       ("3x3", nn.Conv2d(64, 256, 3, padding=1, bias=False)),
                       ("padding", nn.Conv2d(64, 256, 1, padding=1, bias=False)),
                       ("dilation", nn.Conv2d(64, 256, 1, dilation=2, bias=False)),
                       ("64 -> 128", nn.Conv2d(64, 128, 1, bias=False)),
                       ("128 -> 256", nn.Conv2d(128, 256, 1, bias=False)),
                       ("256 -> 64", nn.Conv2d(256, 64, 1, bias=False)),
                       ("circular", nn.Conv2d(64, 256, 1, bias=False, padding_mode="circular"))):
        block = _Tail(conv)
        assert _convs(block) == {}, name
        assert len(_bn_fuse._Plan(block).parents) == 1, name  # K16's tail is still there

    class OwnForward(nn.Conv2d):
        def forward(self, x):
            return super().forward(x) * 2

    assert _convs(_Tail(OwnForward(64, 256, 1, bias=False))) == {}


def test_single_consumer_rules_and_operand_order():
    conv = lambda: nn.Conv2d(64, 256, 1, bias=False)  # noqa: E731
    assert _convs(_Tail(conv(), "conv_read_twice")) == {}  # the convolution's output has a second reader
    assert _convs(_Tail(conv(), "no_add")) == {}  # bn -> relu alone: not a residual tail
    (gm, gates), = _convs(_Tail(conv(), "identity_left")).values()
    assert gates[0].single.bn_first is False and "self._sl_fused_0(x, idt)" in gm.code
    (gm, gates), = _convs(_Tail(conv())).values()
    assert gates[0].single.bn_first is True and "self._sl_fused_0(x, idt)" in gm.code


def test_a_shortcut_that_is_not_conv_bn_keeps_its_k19_tail_beside_the_fused_convolution():
    class Block(nn.Module):
        def __init__(self, shortcut):
            super().__init__()
            self.conv, self.bn, self.relu, self.shortcut = nn.Conv2d(64, 256, 1, bias=False), nn.BatchNorm2d(256), nn.ReLU(), shortcut

        def forward(self, x):
            return self.relu(self.bn(self.conv(x)) + self.shortcut(x))

    for shortcut in (nn.Sequential(nn.AvgPool2d(1), nn.Conv2d(64, 256, 1, bias=False), nn.BatchNorm2d(256)),  # three children
                     nn.Sequential(nn.Conv2d(64, 256, 1), nn.BatchNorm2d(256))):  # a bias
        block = Block(shortcut).eval()
        plan = _bn_fuse._Plan(block)
        assert len(plan.duals) == 1 and plan.convs == {}  # the tail is K19's, and K19's takes no convolution on one side only


def test_the_graph_is_gated_by_hooks_the_switches_and_the_module_and_results_do_not_change(monkeypatch):
    block = synth.Bottleneck(256, 64).eval()
    for bn in (block.bn1, block.bn2, block.bn3):
        bn.running_mean.normal_(), bn.running_var.uniform_(0.5, 2.0)
    x = torch.randn(2, 256, 5, 5)
    with torch.no_grad():
        want = block(x)
    plan = _bn_fuse._Plan(block)
    fused = plan.convs[0][1][0]
    assert fused.ready()
    for hooked in (block.conv3, block.bn3, block.relu):
        handle = hooked.register_forward_hook(lambda m, i, o: None)
        assert not fused.ready()
        handle.remove()
    handle = block.conv3.register_forward_pre_hook(lambda m, i: None)
    assert not fused.ready()
    handle.remove()
    monkeypatch.setenv("SEMANTICLENS_AMD_FUSE_CONV", "0")
    assert not fused.ready() and _bn_fuse.enabled()
    monkeypatch.delenv("SEMANTICLENS_AMD_FUSE_CONV")
    monkeypatch.setenv("SEMANTICLENS_AMD_FUSE_BN", "0")
    assert not fused.ready()
    monkeypatch.delenv("SEMANTICLENS_AMD_FUSE_BN")
    block.conv3.stride = (2, 2)  # the user changed the module after the trace
    assert not fused.ready()
    block.conv3.stride = (1, 1)
    fused.dropped = True
    assert not fused.ready()
    fused.dropped = False
    assert fused.ready()
    # on the CPU no call is eligible: the graph calls conv3 as a module, once, and its norm and activation behind it
    calls = []
    handle = block.bn3.register_forward_pre_hook(lambda m, i: calls.append(tuple(i[0].shape)))
    cache = ActMaxCache([], aggregators.aggregate_conv_max, 3)
    with torch.no_grad():
        got_direct = plan.convs[0][0].forward(x)
        with cache.hook_context(block):
            got = block(x)
    handle.remove()
    assert torch.equal(got, want) and torch.equal(got_direct, want) and calls == [(2, 256, 5, 5)] * 2


def test_the_wrappers_are_declared_and_refuse_other_shapes():
    for name in ("sl_conv1x1_64_256", "sl_conv1x1_bn_add_relu", "sl_conv1x1_bn_add_conv1x1_bn_relu"):
        assert name in N.SIGNATURES and hasattr(N.lib(), name)
    assert (N.CONV_TAIL_IN, N.CONV_TAIL_OUT, N.CONV_TAIL_SPLITS) == (64, 256, 7)


def test_a_new_input_shape_or_cudnn_flag_is_proven_anew(monkeypatch):
    """What a site has proven holds for one input shape and one setting of the cudnn flags: MIOpen picks its solver by them."""
    import torch.nn.functional as F

    block = synth.Bottleneck(256, 64).eval()
    block.bn3.running_mean.normal_(), block.bn3.running_var.uniform_(0.5, 2.0)
    fused = _bn_fuse._Plan(block).convs[0][1][0]
    proofs, launches = [], []
    conv2d = F.conv2d

    def counted_conv2d(x, w, *a, **k):  # only the proof calls F.conv2d directly here
        proofs.append(tuple(x.shape))
        return conv2d(x, w, *a, **k)

    def kernel(x, w, bn, other):  # stands in for the device kernel: the unfused sequence on the host
        launches.append(tuple(x.shape))
        return torch.relu_(F.batch_norm(conv2d(x, w), *bn[:4], False, 0.0, bn[4]) + other)

    monkeypatch.setattr(F, "conv2d", counted_conv2d)
    monkeypatch.setattr(N, "conv1x1_bn_add_relu", kernel)
    small = (torch.randn(2, 64, 4, 4), torch.randn(2, 256, 4, 4))
    large = (torch.randn(3, 64, 4, 4), torch.randn(3, 256, 4, 4))
    saved = torch.backends.cudnn.benchmark
    try:
        with torch.no_grad():
            fused.run(*small)
            fused.run(*small)
            assert proofs == [(2, 64, 4, 4)] and len(launches) == 2 and len(fused.verified) == 1
            fused.run(*large)  # another batch size: another solver may serve it
            fused.run(*large)
            assert proofs == [(2, 64, 4, 4), (3, 64, 4, 4)] and len(fused.verified) == 2
            torch.backends.cudnn.benchmark = not saved
            fused.run(*small)
            fused.run(*small)
            assert proofs == [(2, 64, 4, 4), (3, 64, 4, 4), (2, 64, 4, 4)] and len(fused.verified) == 3
            torch.backends.cudnn.benchmark = saved
            fused.run(*small)  # what was proven under the first setting still stands
            assert len(proofs) == 3 and len(launches) == 7 and not fused.dropped
            # a kernel that does not reproduce the sequence loses the site, and the caller gets the reference
            monkeypatch.setattr(N, "conv1x1_bn_add_relu", lambda x, w, bn, other: kernel(x, w, bn, other) + 1)
            other = (torch.randn(1, 64, 4, 4), torch.randn(1, 256, 4, 4))
            with pytest.warns(RuntimeWarning, match="did not reproduce"):
                got = fused.run(*other)
            want = torch.relu_(F.batch_norm(conv2d(other[0], block.conv3.weight), block.bn3.running_mean, block.bn3.running_var,
                                            block.bn3.weight, block.bn3.bias, False, 0.0, block.bn3.eps) + other[1])
            assert fused.dropped and not fused.ready() and torch.equal(got, want)
    finally:
        torch.backends.cudnn.benchmark = saved
