"""Host side of K18 (`component_visualization/_bn_fuse.py`): the graph a stem-like owner is rewritten to, which spellings of the
max-pool are matched, and that the pool's parameters are read when the fused call runs, not when it was traced.  Nothing is
eligible on the CPU, so every forward here also checks that the fallback chain computes what the modules compute."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import synth
from semanticlens_amd.component_visualization import _bn_fuse


class Stem(nn.Module):
    def __init__(self, pool=None):
        super().__init__()
        self.conv1, self.bn1, self.relu = nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(inplace=True)
        self.maxpool = pool if pool is not None else nn.MaxPool2d(3, 2, 1)

    def forward(self, x):
        return self.maxpool(self.relu(self.bn1(self.conv1(x))))


def _only_parent(model):
    plan = _bn_fuse._Plan(model)
    assert len(plan.parents) == 1
    return plan, plan.parents[0][1]


def _fused(gm):
    return [m for name, m in gm.named_children() if name.startswith("_sl_fused_")]


def test_one_fused_node_replaces_bn_relu_and_pool():
    model = Stem().eval()
    _, gm = _only_parent(model)
    calls = [n for n in gm.graph.nodes if n.op in ("call_module", "call_function", "call_method")]
    assert [n.target for n in calls] == ["conv1", "_sl_fused_0"]
    assert "self.bn1" not in gm.code and "self.relu" not in gm.code and "self.maxpool" not in gm.code
    (fused,) = _fused(gm)
    assert isinstance(fused, _bn_fuse._FusedPool) and fused.pool is model.maxpool and fused.inner.site.bn is model.bn1
    x = torch.randn(2, 3, 9, 11)
    with torch.no_grad():
        want = model(x)
        undo = _bn_fuse.substitute(model)
        got = model(x)
        undo()
    assert torch.equal(got, want) and "forward" not in model.__dict__


def test_the_resnet_stems_are_matched():
    for model in (synth.resnet50(), synth.resnet18()):
        plan = _bn_fuse._Plan(model)
        code = dict((ref(), gm) for ref, gm, _ in plan.parents)[model]
        assert any(isinstance(m, _bn_fuse._FusedPool) and m.pool is model.maxpool for m in _fused(code))
        assert "self.maxpool" not in code.code


def test_functional_spellings():
    class Functional(nn.Module):
        def __init__(self, how):
            super().__init__()
            self.bn, self.relu, self.how = nn.BatchNorm2d(4), nn.ReLU(), how

        def forward(self, x):
            y = self.relu(self.bn(x))
            if self.how == "positional":
                return F.max_pool2d(y, 3, 2, 1)
            if self.how == "keywords":
                return F.max_pool2d(y, kernel_size=(3, 2), stride=(2, 1), padding=(1, 0))
            if self.how == "default_stride":
                return F.max_pool2d(y, 2)
            return F.max_pool2d(y, (y.shape[2] // 2, 2))  # a kernel size computed from the input: not literal

    x = torch.randn(2, 4, 8, 8)
    expected = {"positional": ((3, 3), (2, 2), (1, 1)), "keywords": ((3, 2), (2, 1), (1, 0)), "default_stride": ((2, 2), (2, 2), (0, 0))}
    for how, params in expected.items():
        model = Functional(how).eval()
        _, gm = _only_parent(model)
        (fused,) = _fused(gm)
        assert isinstance(fused, _bn_fuse._FusedPool) and _bn_fuse._pool_params(**fused.pool) == params, how
        assert "max_pool2d" not in gm.code
        with torch.no_grad():
            assert torch.equal(gm(x), model(x))

    _, gm = _only_parent(Functional("computed").eval())
    (fused,) = _fused(gm)
    assert type(fused) is _bn_fuse._Fused and "max_pool2d" in gm.code  # bn + relu only; the pool stays in the graph


def test_a_second_consumer_of_the_relu_keeps_the_pool_outside():
    class TwoUses(nn.Module):
        def __init__(self):
            super().__init__()
            self.bn, self.relu, self.pool = nn.BatchNorm2d(4), nn.ReLU(), nn.MaxPool2d(2, 2)

        def forward(self, x):
            y = self.relu(self.bn(x))
            return self.pool(y), y

    model = TwoUses().eval()
    _, gm = _only_parent(model)
    (fused,) = _fused(gm)
    assert type(fused) is _bn_fuse._Fused and "self.pool(" in gm.code
    x = torch.randn(1, 4, 6, 6)
    with torch.no_grad():
        got, want = gm(x), model(x)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_other_pools_are_not_matched():
    class MyPool(nn.MaxPool2d):
        def forward(self, x):
            return super().forward(x) * 2

    for pool in (MyPool(2), nn.AvgPool2d(2), nn.MaxPool1d(2)):
        _, gm = _only_parent(Stem(pool).eval())
        (fused,) = _fused(gm)
        assert type(fused) is _bn_fuse._Fused and "self.maxpool(" in gm.code


def test_pool_parameters_are_read_at_call_time(monkeypatch):
    model = Stem().eval()
    _, gm = _only_parent(model)
    (fused,) = _fused(gm)
    seen = []
    real = _bn_fuse._pool_params
    monkeypatch.setattr(_bn_fuse, "_pool_params", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    x = torch.randn(1, 3, 12, 12)
    with torch.no_grad():
        gm(x)
        model.maxpool.kernel_size, model.maxpool.stride, model.maxpool.padding = 2, (2, 1), 0
        got = gm(x)
        assert got.shape == (1, 8, 6, 11) and torch.equal(got, model(x))  # the pool as it is now
        model.maxpool.ceil_mode = True
        gm(x)
        model.maxpool.ceil_mode, model.maxpool.kernel_size = False, 5
        gm(x)
        model.maxpool.kernel_size, model.maxpool.dilation = 3, 2
        gm(x)
        model.maxpool.dilation, model.maxpool.padding = 1, 2  # padding above half the kernel (PyTorch refuses it itself)
        assert real(3, 2, 2) is None
    assert seen == [((3, 3), (2, 2), (1, 1)), ((2, 2), (2, 1), (0, 0)), None, None, None]


def test_pool_params_normalisation():
    p = _bn_fuse._pool_params
    assert p(3, None, 1) is None and p(2) == ((2, 2), (2, 2), (0, 0)) and p((3, 2), (2, 1), (1, 0)) == ((3, 2), (2, 1), (1, 0))  # (stride defaults to the kernel size: 3 is not supported)
    assert p(2, [], 1) == ((2, 2), (2, 2), (1, 1))
    for bad in (dict(kernel_size=4), dict(kernel_size=3, stride=3), dict(kernel_size=2, padding=2), dict(kernel_size=3, dilation=2),
                dict(kernel_size=3, ceil_mode=True), dict(kernel_size=3, return_indices=True), dict(kernel_size=(3, 3, 3)),
                dict(kernel_size=3, padding=-1), dict(kernel_size=1, stride=1)):
        assert p(**bad) is None, bad
