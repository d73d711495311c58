"""K18 on the device: the fused BatchNorm + ReLU + max-pool kernel against PyTorch's unfused sequence, BIT FOR BIT (int32 views,
zero mismatches), the graph rewrite on a conv-free model under `ActMaxCache.hook_context`, and every condition under which the
pooled form steps aside (counted through the `SL_PROF_BATCHNORM` launch counter and a counter on `F.max_pool2d`)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from semanticlens_amd import _native as N
from semanticlens_amd.component_visualization import aggregators
from semanticlens_amd.component_visualization.activation_caching import ActMaxCache

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the last two planes are larger than a block stages at once (64 KiB): bands of rows, 16-byte and element-wise
SHAPES = [(3, 5, 7, 9), (2, 3, 8, 8), (1, 1, 1, 1), (2, 4, 1, 13), (3, 64, 16, 16), (2, 64, 112, 112), (1, 7, 30, 52),
          (1, 2, 40, 512), (1, 2, 70, 250)]
POOLS = [((3, 3), (2, 2), (1, 1)), ((2, 2), (2, 2), (0, 0)), ((3, 3), (1, 1), (1, 1)), ((3, 3), (2, 2), (0, 0)),
         ((3, 2), (2, 1), (1, 0)), ((2, 3), (1, 2), (1, 1))]
EPS = (1e-5, 1e-3, 1e-12)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _mismatches(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return int((_bits(got) != _bits(want)).sum().item())


def _inputs(B, C, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, C, H, W, device=DEV, generator=g) * 4
    mean = torch.randn(C, device=DEV, generator=g)
    var = torch.exp(torch.empty(C, device=DEV).uniform_(-7.0, 3.0, generator=g))
    var[::7] = torch.exp(torch.empty(C, device=DEV).uniform_(-40.0, -20.0, generator=g))[::7]  # 4e-18 .. 2e-9
    var[0] = 1e-17
    weight = torch.randn(C, device=DEV, generator=g)
    weight[1::4] = -weight[1::4].abs()
    weight[2::8] = 0.0  # with a negative bias every window of the channel is all negative: +0.0
    bias = torch.randn(C, device=DEV, generator=g)
    bias[2::8] = -bias[2::8].abs() - 0.5
    bias[3::6] = -0.0
    flat = x.view(-1)
    n = flat.numel()
    flat[1::23] = float("inf")
    flat[2::23] = -float("inf")
    flat[3::23] = -0.0
    x[:, 4 % C] = -x[:, 4 % C].abs() * weight[4 % C].sign() - 50.0 * weight[4 % C].sign()  # far below the mean: all negative
    # NaNs with distinct payloads, in runs of two and in pairs one row apart, so that windows hold two of them
    bits = flat.view(torch.int32)
    for start, step in ((0, 29), (1, 29), (W, 31), (5, 7 * W + 3)):
        idx = torch.arange(min(start, n), n, step, device=DEV)
        bits[idx] = 0x7FC00001 + (idx % 0x3FFFF).to(torch.int32) * 3
    return x, mean, var, weight, bias


def _reference(x, mean, var, weight, bias, eps, pool):
    k, s, p = pool
    return F.max_pool2d(torch.relu_(F.batch_norm(x, mean, var, weight, bias, False, 0.0, eps)), k, s, p)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_pytorch_bit_for_bit(shape):
    B, C, H, W = shape
    x, mean, var, weight, bias = _inputs(B, C, H, W, seed=C * H + W)
    bad, ran = {}, 0
    before = N.get_option("bn_policy")
    try:
        for n, pool in enumerate(POOLS):
            (kh, kw), _, (ph, pw) = pool
            eps = EPS[n % len(EPS)]
            if H + 2 * ph < kh or W + 2 * pw < kw:  # no output at all: PyTorch refuses it, and so does the library
                with pytest.raises(ValueError, match="smaller than the pooling window"):
                    N.batchnorm_infer_relu_maxpool(x, mean, var, weight, bias, eps, *pool)
                continue
            want = _reference(x, mean, var, weight, bias, eps, pool)
            for policy in (0, 1, 2, 3):
                N.set_option("bn_policy", policy)
                bad[(pool, policy)] = _mismatches(N.batchnorm_infer_relu_maxpool(x, mean, var, weight, bias, eps, *pool), want)
            ran += 1
    finally:
        N.set_option("bn_policy", before)
    print(shape, "pools compared:", ran, "mismatches:", {k: v for k, v in bad.items() if v})
    assert ran >= (1 if shape == (1, 1, 1, 1) else 4) and all(v == 0 for v in bad.values()), bad


def test_the_data_exercises_what_it_claims():
    """Windows with two distinct NaNs (the later one wins), all-negative windows giving +0.0, infinities on both sides."""
    x, mean, var, weight, bias = _inputs(3, 64, 16, 16, seed=1)
    y = torch.relu_(F.batch_norm(x, mean, var, weight, bias, False, 0.0, 1e-5))
    want = F.max_pool2d(y, 3, 2, 1)
    got = N.batchnorm_infer_relu_maxpool(x, mean, var, weight, bias, 1e-5, (3, 3), (2, 2), (1, 1))
    assert _mismatches(got, want) == 0
    nans = F.avg_pool2d(y.isnan().float(), 3, 2, 1, divisor_override=1)  # NaNs per window
    # the planted payloads survive the BatchNorm; not every NaN keeps a pattern of its own (inf x 0 yields the default NaN)
    assert int((nans >= 2).sum()) > 20 and _bits(y)[y.isnan()].unique().numel() > int(y.isnan().sum()) * 3 // 4
    assert int(((_bits(want) == 0) & (F.max_pool2d(torch.nan_to_num(y, nan=1.0), 3, 2, 1) == 0)).sum()) > 100  # +0.0 windows
    assert bool(want.isposinf().any()) and float(var.min()) <= 1e-17 and bool((x == float("-inf")).any())


def test_argument_checks():
    x = torch.zeros(1, 4, 8, 8, device=DEV)
    p = torch.zeros(4, device=DEV)
    ok = ((3, 3), (2, 2), (1, 1))
    for k, s, pad, what in (((4, 3), (2, 2), (1, 1), "kernel size"), ((3, 1), (2, 2), (1, 0), "kernel size"),
                            ((3, 3), (3, 2), (1, 1), "stride"), ((3, 3), (2, 0), (1, 1), "stride"),
                            ((3, 3), (2, 2), (2, 1), "padding"), ((2, 2), (2, 2), (0, 2), "padding"),
                            ((3, 3), (2, 2), (-1, 0), "padding")):
        with pytest.raises(ValueError, match=what):
            N.batchnorm_infer_relu_maxpool(x, p, p, p, p, 1e-5, k, s, pad)
    with pytest.raises(ValueError, match="16-byte aligned"):
        N.batchnorm_infer_relu_maxpool(torch.zeros(260, device=DEV)[1:257].view(1, 4, 8, 8), p, p, p, p, 1e-5, *ok)
    big = torch.zeros(1, 4097, 2, 2, device=DEV)
    with pytest.raises(ValueError, match="channels exceed"):
        N.batchnorm_infer_relu_maxpool(big, p, p, p, p, 1e-5, *ok)
    empty = N.batchnorm_infer_relu_maxpool(torch.zeros(0, 4, 8, 8, device=DEV), p, p, p, p, 1e-5, *ok)
    assert empty.shape == (0, 4, 4, 4) and empty.dtype is torch.float32


# ------------------------------------------------------------------------------------------------ the rewrite
def _launches():
    return N.prof_read(N.SL_PROF_BATCHNORM)[1]


@pytest.fixture
def prof():
    N.prof_enable(True)
    N.prof_reset()
    yield
    N.prof_reset()
    N.prof_enable(False)


@pytest.fixture
def pool_calls(monkeypatch):
    calls = []
    real = F.max_pool2d

    def counted(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(F, "max_pool2d", counted)
    return calls


class _Block(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.bn1, self.bn2, self.relu = nn.BatchNorm2d(c), nn.BatchNorm2d(c), nn.ReLU(inplace=True)

    def forward(self, x):
        out = self.relu(self.bn1(x))
        out = self.bn2(out)
        return self.relu(out + x)


class _StemNet(nn.Module):
    """bn -> relu -> max-pool -> two residual blocks, no convolution (MIOpen's small convolutions do not reproduce themselves
    from call to call, and these tests compare whole forwards bit for bit): 5 BatchNorm2d."""

    def __init__(self, pool=None, c=32, second_consumer=False):
        super().__init__()
        self.bn1, self.relu = nn.BatchNorm2d(c), nn.ReLU(inplace=True)
        self.maxpool = pool if pool is not None else nn.MaxPool2d(3, 2, 1)
        self.layer1, self.layer2 = _Block(c), _Block(c)
        self.second_consumer = second_consumer

    def forward(self, x):
        y = self.relu(self.bn1(x))
        z = self.maxpool(y)
        if self.maxpool.return_indices:
            z = z[0]
        z = self.layer2(self.layer1(z))
        return z + y.amax() if self.second_consumer else z


def _small(pool=None, seed=0, **kwargs):
    g = torch.Generator().manual_seed(seed)
    model = _StemNet(pool, **kwargs).eval()
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(32, generator=g))
            m.running_var.copy_(torch.rand(32, generator=g) + 0.1)
            m.weight.data.copy_(torch.randn(32, generator=g))
            m.bias.data.copy_(torch.randn(32, generator=g))
    return model.to(DEV), torch.randn(8, 32, 28, 28, generator=g).to(DEV)


def _plain(model, x, grad=False):
    with torch.set_grad_enabled(grad):
        first, second = model(x), model(x)
    assert _mismatches(first, second) == 0, "the unfused model does not reproduce itself"
    return first


def _under_context(model, x, grad=False, forwards=1):
    cache = ActMaxCache([], aggregators.aggregate_conv_max, 5)
    with torch.set_grad_enabled(grad), cache.hook_context(model):
        for _ in range(forwards):
            out = model(x)
    return out


def _identity(model):
    return ([(n, id(m), m.__dict__.get("forward")) for n, m in model.named_modules()],
            [(n, id(p), p._version) for n, p in model.named_parameters()], [(n, id(b)) for n, b in model.named_buffers()])


def test_stem_is_fused_and_bit_identical(prof, pool_calls):
    model, x = _small()
    before = _identity(model)
    want = _plain(model, x)
    assert _launches() == 0
    del pool_calls[:]
    got = _under_context(model, x)
    assert _launches() == 5 and _mismatches(got, want) == 0  # one launch per BatchNorm2d; the first call's proof may pool
    assert len(pool_calls) <= 1
    N.prof_reset()
    del pool_calls[:]
    got = _under_context(model, x)  # the second forward: no pooling outside the fused kernel
    assert _launches() == 5 and _mismatches(got, want) == 0 and pool_calls == []
    assert _identity(model) == before


def test_a_taller_input_that_is_pooled_in_bands_is_proven_again(prof, pool_calls):
    model, x = _small()
    tall = torch.randn(1, 32, 40, 512, device=DEV)  # 80 KiB planes: the banded launch
    want, want_tall = _plain(model, x), _plain(model, tall)
    cache = ActMaxCache([], aggregators.aggregate_conv_max, 5)
    counts = []
    with torch.no_grad(), cache.hook_context(model):
        for inp, ref in ((x, want), (x, want), (tall, want_tall), (tall, want_tall)):
            del pool_calls[:]
            assert _mismatches(model(inp), ref) == 0
            counts.append(len(pool_calls))
    assert counts == [1, 0, 1, 0]  # the reference pools once per proof: per launch form, not per site


def _step_aside(model, x, pool_calls, hooked=None, expect=None):
    want = _plain(model, x)
    N.prof_reset()
    seen = []
    handle = hooked.register_forward_hook(lambda m, i, o: seen.append((o[0] if isinstance(o, tuple) else o).clone())) if hooked else None
    try:
        _under_context(model, x)  # (a first forward, so that no proof is pending in the counted one)
        N.prof_reset()
        del pool_calls[:], seen[:]
        got = _under_context(model, x)
    finally:
        if handle is not None:
            handle.remove()
    assert _mismatches(got, want) == 0
    assert _launches() == 5  # every BatchNorm2d still ran on the library's kernel, the stem's without the pool
    assert len(pool_calls) == 1  # the user's pool ran
    if hooked is not None:
        assert len(seen) == 1 and _mismatches(seen[0], expect) == 0


@pytest.mark.parametrize("which", ["maxpool", "relu", "bn1"])
def test_a_hook_on_the_pool_the_activation_or_the_norm_sees_its_output(which, prof, pool_calls):
    model, x = _small()
    with torch.no_grad():
        bn = model.bn1(x)
        relu = torch.relu(bn)
        expect = {"bn1": bn, "relu": relu, "maxpool": model.maxpool(relu)}[which]
    _step_aside(model, x, pool_calls, hooked=getattr(model, which), expect=expect)


@pytest.mark.parametrize("pool", [nn.MaxPool2d(3, 2, 1, ceil_mode=True), nn.MaxPool2d(3, 2, 1, return_indices=True),
                                  nn.MaxPool2d(3, 2, 1, dilation=2), nn.MaxPool2d(5, 2, 2)],
                         ids=["ceil_mode", "return_indices", "dilation", "kernel_size_5"])
def test_pools_the_kernel_does_not_take_run_as_modules(pool, prof, pool_calls):
    model, x = _small(pool)
    _step_aside(model, x, pool_calls)


def test_a_second_consumer_of_the_relu_keeps_the_pool(prof, pool_calls):
    model, x = _small(second_consumer=True)
    _step_aside(model, x, pool_calls)


def test_train_grad_channels_last_and_half_are_left_alone(prof):
    model, x = _small()
    want = _plain(model, x, grad=True)
    got = _under_context(model, x, grad=True)
    assert _launches() == 0 and got.requires_grad and _mismatches(got, want) == 0
    model.train()
    got = _under_context(model, x)
    assert _launches() == 0 and got.shape == want.shape
    model, x = _small()
    model, x = model.to(memory_format=torch.channels_last), x.contiguous(memory_format=torch.channels_last)
    want = _plain(model, x)
    assert torch.equal(_under_context(model, x), want) and _launches() == 0
    model, x = _small()
    model, x = model.half(), x.half()
    want = _plain(model, x)
    assert torch.equal(_under_context(model, x), want) and _launches() == 0


def test_env_switch_off(prof, monkeypatch):
    monkeypatch.setenv("SEMANTICLENS_AMD_FUSE_BN", "0")
    model, x = _small()
    want = _plain(model, x)
    cache = ActMaxCache([], aggregators.aggregate_conv_max, 5)
    with torch.no_grad(), cache.hook_context(model):
        assert "forward" not in model.__dict__ and "forward" not in model.bn1.__dict__
        got = model(x)
    assert _launches() == 0 and _mismatches(got, want) == 0
