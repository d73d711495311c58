"""K16 on the device: the fused inference BatchNorm kernels against PyTorch's unfused sequence, BIT FOR BIT (int32 views, zero
mismatches), the whole ResNets under `ActMaxCache.hook_context`, and every condition under which the fusion steps aside (counted
through the `SL_PROF_BATCHNORM` launch counter)."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import synth
from semanticlens_amd import _native as N
from semanticlens_amd.component_visualization import aggregators
from semanticlens_amd.component_visualization.activation_caching import ActMaxCache

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# every (C, H, W) a BatchNorm2d of ResNet-50 sees at 224 x 224
RESNET50_BN_SHAPES = [(64, 112, 112), (64, 56, 56), (256, 56, 56), (128, 56, 56), (128, 28, 28), (512, 28, 28), (256, 28, 28),
                      (256, 14, 14), (1024, 14, 14), (512, 14, 14), (512, 7, 7), (2048, 7, 7)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _mismatches(got, want):
    return int((_bits(got) != _bits(want)).sum().item())


def _inputs(B, C, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, C, H, W, device=DEV, generator=g) * 4
    res = torch.randn(B, C, H, W, device=DEV, generator=g)
    mean = torch.randn(C, device=DEV, generator=g)
    var = torch.exp(torch.empty(C, device=DEV).uniform_(-7.0, 3.0, generator=g))
    var[::7] = torch.exp(torch.empty(C, device=DEV).uniform_(-40.0, -20.0, generator=g))[::7]  # very small variances
    var[3 % C] = 0.0
    weight = torch.randn(C, device=DEV, generator=g)
    weight[1::4] = -weight[1::4].abs()
    weight[2::8] = 0.0
    bias = torch.randn(C, device=DEV, generator=g)
    bias[::6] = 0.0
    bias[3::6] = -0.0
    flat = x.view(-1)
    flat[0::101] = float("nan")
    flat[1::101] = float("inf")
    flat[2::101] = -float("inf")
    flat[3::101] = -0.0
    flat[4::101] = 0.0
    x[:, 5 % C] = mean[5 % C]  # normalises to exactly 0 (x scale, then + bias: -0.0, 0.0 and signed-zero sums)
    res.view(-1)[7::103] = float("nan")
    res.view(-1)[8::103] = -0.0
    return x, res, mean, var, weight, bias


@pytest.mark.parametrize("B", [256, 3])
@pytest.mark.parametrize("shape", RESNET50_BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_equal_pytorch_bit_for_bit(shape, B):
    C, H, W = shape
    x, res, mean, var, weight, bias = _inputs(B, C, H, W, seed=C * H + B)
    eps = 1e-5
    want = F.batch_norm(x, mean, var, weight, bias, False, 0.0, eps)
    got = N.batchnorm_infer(x, mean, var, weight, bias, eps)
    bad = {"plain": _mismatches(got, want)}
    got = N.batchnorm_infer(x, mean, var, weight, bias, eps, relu=True)
    bad["relu"] = _mismatches(got, torch.relu_(want.clone()))
    got = N.batchnorm_infer(x, mean, var, weight, bias, eps, residual=res)
    bad["add_relu"] = _mismatches(got, torch.relu_(want + res))
    cancel = torch.nan_to_num(-want, nan=1.0, posinf=1.0, neginf=-1.0)  # y + residual == 0 exactly: the sign of the sum
    got = N.batchnorm_infer(x, mean, var, weight, bias, eps, residual=cancel)
    bad["add_relu_cancel"] = _mismatches(got, torch.relu_(want + cancel))
    print(shape, B, bad)
    assert all(v == 0 for v in bad.values()), bad


def test_variance_sweep_and_cache_policies():
    """2^20 random variances x inputs per eps, and every cache policy (`bn_policy`) writes the same bits."""
    C, B, H, W = 4096, 4, 8, 8
    for seed, (lo, hi), eps in ((0, (-7.0, 5.0), 1e-5), (1, (-30.0, -9.0), 1e-5), (2, (-14.0, 9.0), 1e-3), (3, (-18.0, 4.0), 1e-12)):
        g = torch.Generator(device=DEV).manual_seed(seed)
        x = torch.randn(B, C, H, W, device=DEV, generator=g) * 3
        mean, weight, bias = (torch.randn(C, device=DEV, generator=g) for _ in range(3))
        var = torch.exp(torch.empty(C, device=DEV).uniform_(lo, hi, generator=g))
        want = F.batch_norm(x, mean, var, weight, bias, False, 0.0, eps)
        try:
            for policy in (0, 1, 2, 3):
                N.set_option("bn_policy", policy)
                bad = _mismatches(N.batchnorm_infer(x, mean, var, weight, bias, eps), want)
                print("sweep", seed, eps, "policy", policy, "mismatches", bad)
                assert bad == 0
        finally:
            N.set_option("bn_policy", 0)


def test_argument_checks():
    x = torch.zeros(1, 4, 2, 2, device=DEV)
    p = torch.zeros(4, device=DEV)
    with pytest.raises(ValueError, match="16-byte aligned"):
        N.batchnorm_infer(x.view(-1)[1:13].view(1, 3, 2, 2), p, p, p, p, 1e-5)
    big = torch.zeros(1, 4097, 1, 1, device=DEV)
    with pytest.raises(ValueError, match="channels exceed"):
        N.batchnorm_infer(big, p, p, p, p, 1e-5)


# ------------------------------------------------------------------------------------------------ whole model
def _launches():
    return N.prof_read(N.SL_PROF_BATCHNORM)[1]


@pytest.fixture
def prof():
    N.prof_enable(True)
    N.prof_reset()
    yield
    N.prof_reset()
    N.prof_enable(False)


def _run(model, x, fused, layers=("layer1", "layer2", "layer3", "layer4")):
    taps = {}
    handles = [model.get_submodule(n).register_forward_hook(lambda m, i, o, n=n: taps.__setitem__(n, o.clone())) for n in layers]
    try:
        with torch.no_grad():
            if fused:
                cache = ActMaxCache(["layer2", "layer3", "layer4"], aggregators.aggregate_conv_max, 5)
                with cache.hook_context(model):
                    taps["logits"] = model(x)
            else:
                taps["logits"] = model(x)
    finally:
        for h in handles:
            h.remove()
    return taps


def _identity(model):
    return ([(n, id(m), m.__dict__.get("forward")) for n, m in model.named_modules()],
            [(n, id(p), p._version) for n, p in model.named_parameters()], [(n, id(b)) for n, b in model.named_buffers()])


@pytest.mark.parametrize("arch,n_bn", [("resnet50", 53), ("resnet18", 20)])
def test_whole_model_is_bit_identical_and_untouched(arch, n_bn, prof):
    model = getattr(synth, arch)().to(DEV)
    x = synth.normalize_u8(synth.synth_images_u8(torch.arange(256, device=DEV)), synth.IMAGENET_MEAN, synth.IMAGENET_STD)
    before = _identity(model)
    want = _run(model, x, fused=False)
    assert _launches() == 0
    got = _run(model, x, fused=True)
    assert _launches() == n_bn  # every BatchNorm2d of the forward ran on the library's kernel, once
    assert _identity(model) == before
    for name in want:
        assert _mismatches(got[name], want[name]) == 0, name
    N.prof_reset()
    got = _run(model, x, fused=True)  # a second visualizer over the same model: the verified plan is reused
    assert _launches() == n_bn
    for name in want:
        assert _mismatches(got[name], want[name]) == 0, name
    with pytest.raises(ZeroDivisionError):
        with ActMaxCache(["layer4"], aggregators.aggregate_conv_max, 5).hook_context(model):
            1 / 0
    assert _identity(model) == before


# ------------------------------------------------------------------------------------------------ stepping aside
class _TinyBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.bn1, self.bn2, self.relu = nn.BatchNorm2d(c), nn.BatchNorm2d(c), nn.ReLU(inplace=True)

    def forward(self, x):
        out = self.relu(self.bn1(x))
        out = self.bn2(out)
        return self.relu(out + x)


class _TinyNet(nn.Module):
    """A residual net of norms and activations only (5 BatchNorm2d).  MIOpen's convolutions for small odd shapes do not reproduce
    themselves from call to call on this stack (atomics), so the stepping-aside cases, which compare whole forwards bit for bit,
    run on a model whose every kernel is deterministic; the convolutional ResNets are covered at B = 256 above."""

    def __init__(self, c=32):
        super().__init__()
        self.bn1, self.relu, self.pool = nn.BatchNorm2d(c), nn.ReLU(inplace=True), nn.AvgPool2d(2)
        self.layer1, self.layer2 = _TinyBlock(c), _TinyBlock(c)

    def forward(self, x):
        return self.layer2(self.pool(self.layer1(self.relu(self.bn1(x)))))


def _small(seed=0):
    g = torch.Generator().manual_seed(seed)
    model = _TinyNet().eval()
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(32, generator=g))
            m.running_var.copy_(torch.rand(32, generator=g) + 0.1)
            m.weight.data.copy_(torch.randn(32, generator=g))
            m.bias.data.copy_(torch.randn(32, generator=g))
    return model.to(DEV), torch.randn(8, 32, 28, 28, generator=g).to(DEV)


def _plain(model, x, grad=False):
    """The model as the user runs it; two calls must agree before they count as the expectation."""
    with torch.set_grad_enabled(grad):
        first, second = model(x), model(x)
    assert _mismatches(first, second) == 0, "the unfused model does not reproduce itself"
    return first


def _under_context(model, x, grad=False):
    cache = ActMaxCache([], aggregators.aggregate_conv_max, 5)
    with torch.set_grad_enabled(grad), cache.hook_context(model):
        return model(x)


def test_small_model_is_fused_by_default(prof):
    model, x = _small()
    want = _plain(model, x)
    got = _under_context(model, x)
    assert _launches() == 5 and _mismatches(got, want) == 0


def test_train_mode_is_left_alone(prof):
    model, x = _small()
    model.train()
    twin, once = copy.deepcopy(model), copy.deepcopy(model)
    want = _plain(twin, x)  # (batch statistics: the output does not depend on how often the running ones were updated)
    got = _under_context(model, x)
    assert _launches() == 0 and _mismatches(got, want) == 0
    with torch.no_grad():
        once(x)
    assert torch.equal(model.bn1.running_mean, once.bn1.running_mean) and torch.equal(model.bn1.running_var, once.bn1.running_var)


def test_channels_last_and_half_models_are_left_alone(prof):
    model, x = _small()
    model = model.to(memory_format=torch.channels_last)
    x = x.contiguous(memory_format=torch.channels_last)
    want = _plain(model, x)
    got = _under_context(model, x)
    assert _launches() == 0 and torch.equal(got, want)
    model, x = _small()
    model, x = model.half(), x.half()
    want = _plain(model, x)
    got = _under_context(model, x)
    assert _launches() == 0 and torch.equal(got, want)


def test_grad_mode_is_left_alone(prof):
    model, x = _small()
    want = _plain(model, x, grad=True)
    got = _under_context(model, x, grad=True)
    assert _launches() == 0 and got.requires_grad and _mismatches(got, want) == 0
    got.sum().backward()  # the relevance path sees the user's own modules
    assert model.bn1.weight.grad is not None


def test_env_switch_off(prof, monkeypatch):
    monkeypatch.setenv("SEMANTICLENS_AMD_FUSE_BN", "0")
    model, x = _small()
    want = _plain(model, x)
    got = _under_context(model, x)
    assert _launches() == 0 and "forward" not in model.bn1.__dict__ and _mismatches(got, want) == 0


def test_user_hooks_on_norm_and_activation_still_see_their_outputs(prof):
    model = nn.Sequential(nn.Identity(), nn.BatchNorm2d(16), nn.ReLU(inplace=True)).to(DEV).eval()
    wrapper = nn.Sequential(model)  # the pattern's owner is `model`
    x = torch.randn(4, 16, 32, 32, device=DEV)
    with torch.no_grad():
        want_bn = model[1](model[0](x))
        want = torch.relu(want_bn)
    # no hooks: one fused launch
    got = _under_context(wrapper, x)
    assert _launches() == 1 and _mismatches(got, want) == 0
    for hooked, expect in ((model[1], want_bn), (model[2], want)):
        N.prof_reset()
        seen = []
        handle = hooked.register_forward_hook(lambda m, i, o: seen.append(o.clone()))
        try:
            got = _under_context(wrapper, x)
        finally:
            handle.remove()
        # the BatchNorm alone ran on the kernel (its own call, hooks fire); the ReLU ran as the user's module
        assert _launches() == 1 and len(seen) == 1
        assert _mismatches(seen[0], expect) == 0 and _mismatches(got, want) == 0
    # a hooked layer that IS the activation is collected as before
    N.prof_reset()
    cache = ActMaxCache(["0.2"], aggregators.aggregate_conv_max, 3)
    with torch.no_grad(), cache.hook_context(wrapper):
        wrapper(x)
    assert _launches() == 1 and cache["0.2"].sample_ids.shape == (16, 3)


def test_untraceable_module_still_runs_with_the_plain_kernel(prof):
    class Branchy(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.bn, self.relu = nn.Identity(), nn.BatchNorm2d(8), nn.ReLU(inplace=True)

        def forward(self, x):
            y = self.bn(self.conv(x))
            if y.sum() > -1e30:  # control flow on a value
                y = y * 1
            return self.relu(y)

    model = Branchy().to(DEV).eval()
    x = torch.randn(2, 8, 16, 16, device=DEV)
    want = _plain(model, x)
    got = _under_context(model, x)
    assert _launches() == 1 and _mismatches(got, want) == 0
