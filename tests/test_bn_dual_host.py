"""Host side of K19 (`component_visualization/_bn_fuse.py`): the second graph of an owner whose residual add takes the output of
a shortcut `nn.Sequential` that ends in a BatchNorm2d — what its generated code calls and in which order, and which shortcuts
are left alone."""
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


def test_bottleneck_with_a_downsample_gets_a_second_graph():
    block = synth.Bottleneck(64, 64).eval()  # cin != planes * 4: downsample = Sequential(conv, bn)
    plan, by_owner = _plan_of(block)
    single = plan.parents[by_owner[block]][1].code
    gm, fused = plan.duals[by_owner[block]]
    code = gm.code
    print(code)
    assert len(fused) == 1 and fused[0].shortcut.bn is block.downsample[1] and fused[0].single.site.bn is block.bn3
    # the shortcut's conv is called as a module where the Sequential was: before conv1
    assert 'getattr(self.downsample, "0")(x)' in code
    assert code.index("self.downsample") < code.index("self.conv1(")
    # one fused tail with two tensor arguments: conv3's output (the add's left operand) and the shortcut conv's
    assert code.count("self._sl_fused_") == 3 and "self._sl_fused_2(conv3, downsample_0)" in code
    # no call of the Sequential as a whole or of its BatchNorm, nor of any norm or activation of the block
    assert "self.downsample(" not in code and 'getattr(self.downsample, "1")' not in code
    assert "self.bn" not in code and "self.relu" not in code
    # the first graph is the one every pull request before this one built
    assert "self.downsample(x)" in single and "self._sl_fused_2(conv3, downsample)" in single
    assert single.index("self.downsample(x)") < single.index("self.conv1(")


def test_a_block_without_a_downsample_is_rewritten_as_before():
    block = synth.Bottleneck(256, 64).eval()
    assert block.downsample is None
    plan, by_owner = _plan_of(block)
    assert plan.duals == {}
    code = plan.parents[by_owner[block]][1].code
    assert code.count("self._sl_fused_") == 3 and "self._sl_fused_2(conv3, x)" in code


def test_resnets_and_the_clip_bottleneck_need_no_special_case():
    p50, p18 = _bn_fuse._Plan(synth.resnet50()), _bn_fuse._Plan(synth.resnet18())
    assert len(p50.duals) == 4 and len(p18.duals) == 3  # the first block of every stage whose shape changes
    clip = synth.ClipBottleneck(64, 64, stride=2).eval()  # Sequential(AvgPool2d, Conv2d, BatchNorm2d), act3(out + downsample(x))
    plan, by_owner = _plan_of(clip)
    code = plan.duals[by_owner[clip]][0].code
    print(code)
    pool, conv = code.index('getattr(self.downsample, "-1")(x)'), code.index('getattr(self.downsample, "0")(')
    assert pool < conv < code.index("self._sl_fused_2(conv3, ")
    assert 'getattr(self.downsample, "1")' not in code and "self.downsample(" not in code


class _Block(nn.Module):
    def __init__(self, shortcut, mode="plain"):
        super().__init__()
        self.bn, self.relu, self.shortcut, self.mode = nn.BatchNorm2d(4), nn.ReLU(), shortcut, mode

    def forward(self, x):
        idt = self.shortcut(x)
        out = self.bn(x)
        if self.mode == "second_consumer":
            return self.relu(out + idt) + idt
        if self.mode == "into_shortcut":
            idt += out
            return self.relu(idt)
        if self.mode == "shortcut_left":
            return self.relu(idt + out)
        return self.relu(out + idt)


class _OwnForward(nn.Sequential):
    def forward(self, x):
        return super().forward(x) * 2


def _shortcut(cls=nn.Sequential):
    return cls(nn.Identity(), nn.BatchNorm2d(4))


def test_shortcuts_that_are_left_alone():
    for block in (_Block(_shortcut(), "second_consumer"),  # the shortcut's output has a second consumer
                  _Block(_shortcut(_OwnForward)),  # a Sequential subclass with its own forward
                  _Block(nn.Sequential(nn.BatchNorm2d(4))),  # nothing in front of the norm
                  _Block(nn.Sequential(nn.BatchNorm2d(4), nn.Identity()))):  # does not end in the norm
        plan = _bn_fuse._Plan(block.eval())
        assert len(plan.parents) == 1 and plan.duals == {}, block.mode
    # `idt += out` writes into the shortcut's output: no tail at all, as before
    assert _bn_fuse._Plan(_Block(_shortcut(), "into_shortcut").eval()).parents == []
    # either operand order of an out-of-place add is taken, and the tail remembers which operand is the left one
    for mode, bn_first in (("plain", True), ("shortcut_left", False)):
        plan = _bn_fuse._Plan(_Block(_shortcut(), mode).eval())
        (gm, fused), = plan.duals.values()
        assert fused[0].single.bn_first is bn_first and "self._sl_fused_0(x, shortcut_0)" in gm.code


def test_the_owner_takes_the_second_graph_only_while_nothing_hooks_the_pair_and_results_do_not_change():
    block = _Block(_shortcut()).eval()
    for bn in (block.bn, block.shortcut[1]):
        bn.running_mean.normal_(), bn.running_var.uniform_(0.5, 2.0)
    x = torch.randn(2, 4, 3, 3)
    with torch.no_grad():
        want = block(x)
    plan = _bn_fuse._Plan(block)
    fused = plan.duals[0][1][0]
    assert fused.ready()
    for hooked in (block.shortcut, block.shortcut[1], block.bn, block.relu):
        handle = hooked.register_forward_hook(lambda m, i, o: None)
        assert not fused.ready()
        handle.remove()
    handle = nn.modules.module.register_module_forward_pre_hook(lambda m, i: None)
    assert not fused.ready()
    handle.remove()
    old = block.shortcut[0]
    block.shortcut[0] = nn.Identity()  # a child that is not the traced object
    assert not fused.ready()
    block.shortcut[0] = old
    assert fused.ready()
    # on the CPU nothing is eligible: the second graph runs the shortcut's leading child, its norm and the tail's modules
    calls = []
    handle = block.shortcut[0].register_forward_hook(lambda m, i, o: calls.append(m))
    cache = ActMaxCache([], aggregators.aggregate_conv_max, 3)
    with torch.no_grad(), cache.hook_context(block):
        assert "forward" in block.__dict__
        got = block(x)
    handle.remove()
    assert torch.equal(got, want) and calls == [old] and "forward" not in block.__dict__


def test_the_wrapper_carries_its_channel_cap_and_is_declared():
    assert N.BN_DUAL_MAX_CHANNELS == 2048 and N.BN_DUAL_MAX_CHANNELS <= N.BN_MAX_CHANNELS
    assert "sl_batchnorm_infer_add_bn_relu" in N.SIGNATURES and hasattr(N.lib(), "sl_batchnorm_infer_add_bn_relu")
