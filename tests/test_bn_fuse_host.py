"""Host side of K16 (`component_visualization/_bn_fuse.py`): which forwards `ActMaxCache.hook_context` swaps, that they are
gone afterwards, and that a model nothing is eligible on (a CPU model here) computes exactly what it did."""
import gc
import weakref

import pytest
import torch
import torch.nn as nn

import synth
from semanticlens_amd.component_visualization import _bn_fuse, aggregators
from semanticlens_amd.component_visualization.activation_caching import ActCache, ActMaxCache


def _snapshot(model):
    return {name: (id(m), m.__dict__.get("forward"), tuple(id(p) for p in m.parameters(recurse=False)), len(m._forward_hooks))
            for name, m in model.named_modules()}


def test_plan_of_resnet50_and_resnet18():
    m50, m18 = synth.resnet50(), synth.resnet18()
    p50, p18 = _bn_fuse._Plan(m50), _bn_fuse._Plan(m18)
    assert len(p50.sites) == 53 and len(p18.sites) == 20
    assert len(p50.parents) == 17 and len(p18.parents) == 9  # the blocks and the stem's owner; a downsample (conv, bn) has no pattern
    code = dict((ref(), gm.code) for ref, gm, _ in p50.parents)[m50.layer2[1]]
    assert code.count("self._sl_fused_") == 3 and "self.bn" not in code and "self.relu" not in code
    assert "self._sl_fused_2(conv3, x)" in code  # relu(bn3(conv3) + identity) is one call


def test_forwards_are_swapped_inside_the_context_only_and_results_do_not_change():
    model = synth.resnet18()
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        want = model(x)
    before = _snapshot(model)
    cache = ActMaxCache([], aggregators.aggregate_conv_max, 3)
    with torch.no_grad(), cache.hook_context(model):
        assert "forward" in model.layer1[0].__dict__ and "forward" in model.bn1.__dict__ and "forward" in model.__dict__
        assert "forward" not in model.layer1[0].conv1.__dict__
        got = model(x)  # nothing is eligible on the CPU: the modules run as written
    assert torch.equal(got, want) and _snapshot(model) == before
    with pytest.raises(KeyError):
        with cache.hook_context(model):
            raise KeyError("inside")
    assert _snapshot(model) == before
    with ActCache([]).hook_context(model):  # the plain activation cache never substitutes
        assert "forward" not in model.bn1.__dict__


def test_plan_is_kept_per_model_weakly_and_rebuilt_when_the_modules_change():
    model = synth.resnet18()
    _bn_fuse.substitute(model)()
    plan = _bn_fuse._PLANS[model]
    _bn_fuse.substitute(model)()
    assert _bn_fuse._PLANS[model] is plan
    model.layer1[0].bn1 = nn.BatchNorm2d(64).eval()
    _bn_fuse.substitute(model)()
    assert _bn_fuse._PLANS[model] is not plan
    ref = weakref.ref(model)
    del model, plan
    gc.collect()
    assert ref() is None


def test_switch_user_forwards_and_untraceable_modules(monkeypatch):
    class Branchy(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.bn, self.relu = nn.Conv2d(3, 4, 1), nn.BatchNorm2d(4), nn.ReLU()

        def forward(self, x):
            y = self.bn(self.conv(x))
            if y.sum() > 0:  # control flow on a value: not traceable
                y = y * 1
            return self.relu(y)

    model = Branchy().eval()
    undo = _bn_fuse.substitute(model)
    assert "forward" in model.bn.__dict__ and "forward" not in model.__dict__
    with torch.no_grad():
        assert model(torch.randn(1, 3, 2, 2)).shape == (1, 4, 2, 2)
    undo()
    assert "forward" not in model.bn.__dict__

    mine = lambda x: x  # noqa: E731
    model.bn.forward = mine  # a forward the user installed is neither replaced nor removed
    _bn_fuse.substitute(model)()
    assert model.bn.__dict__["forward"] is mine

    monkeypatch.setenv("SEMANTICLENS_AMD_FUSE_BN", "0")
    assert _bn_fuse.substitute(synth.resnet18()) is None


def test_only_single_use_patterns_are_fused():
    class TwoUses(nn.Module):
        def __init__(self):
            super().__init__()
            self.bn, self.relu = nn.BatchNorm2d(4), nn.ReLU()

        def forward(self, x):
            y = self.bn(x)
            return self.relu(y) + y  # the BatchNorm output has a second consumer

    class AddAlpha(nn.Module):
        def __init__(self):
            super().__init__()
            self.bn, self.relu = nn.BatchNorm2d(4), nn.ReLU()

        def forward(self, x, idt):
            return self.relu(torch.add(self.bn(x), idt, alpha=2))

    for model in (TwoUses().eval(), AddAlpha().eval()):
        assert _bn_fuse._Plan(model).parents == []


def test_an_owner_leaves_the_traced_forward_when_its_mode_changes_and_iadd_into_the_other_operand_is_not_fused():
    class Moody(nn.Module):
        def __init__(self):
            super().__init__()
            self.bn, self.relu = nn.BatchNorm2d(4), nn.ReLU()

        def forward(self, x):
            y = self.relu(self.bn(x))
            return y + 1 if self.training else y

    model = Moody().eval()
    x = torch.randn(3, 4, 2, 2)
    undo = _bn_fuse.substitute(model)
    with torch.no_grad():
        assert "forward" in model.__dict__ and torch.equal(model(x), torch.relu(model.bn(x)))
        model.train()  # the trace holds the eval branch: the owner's own forward runs
        assert torch.equal(model(x), Moody.forward(model, x)) and (model(x) >= 1).all()
    undo()

    class IntoOther(nn.Module):
        def __init__(self):
            super().__init__()
            self.bn, self.relu = nn.BatchNorm2d(4), nn.ReLU()

        def forward(self, x, idt):
            idt += self.bn(x)
            return self.relu(idt)

    assert _bn_fuse._Plan(IntoOther().eval()).parents == []

    class InPlaceElsewhere(nn.Module):
        def __init__(self):
            super().__init__()
            self.bn, self.relu = nn.BatchNorm2d(4), nn.ReLU()

        def forward(self, x, acc):
            acc += 1  # the caller's tensor: the traced forward must still write into it
            out = self.bn(x)
            out += acc
            return self.relu(out)

    model = InPlaceElsewhere().eval()
    plan = _bn_fuse._Plan(model)
    assert len(plan.parents) == 1 and "acc += 1" in plan.parents[0][1].code
    undo = _bn_fuse.substitute(model)
    acc, acc2 = torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2)
    with torch.no_grad():
        got = model(x[:1], acc)
        undo()
        assert torch.equal(got, model(x[:1], acc2)) and torch.equal(acc, acc2) and acc.eq(1).all()
