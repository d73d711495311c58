"""K19 on the device: `relu(bn_a(xa) + bn_b(xb))` in one kernel against PyTorch's unfused sequence, BIT FOR BIT (int32 views, zero
mismatches, no tolerance), and the rewrite that takes a shortcut Sequential's BatchNorm into the residual tail: a conv-free
residual net under `ActMaxCache.hook_context`, the hooks that switch a pair back to the two-kernel path, and the channel cap."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from semanticlens_amd import _native as N
from semanticlens_amd.component_visualization import _bn_fuse, aggregators
from semanticlens_amd.component_visualization.activation_caching import ActMaxCache

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = N.BN_DUAL_MAX_CHANNELS
SHAPES = [
    (3, 5, 7, 7),  # unaligned, pieces cross planes, total % 4 == 3
    (3, 7, 2, 6),  # aligned, runs of 64 pieces cross planes and channels wrap
    (2, 3, 56, 56),  # runs inside one plane, several blocks
    (1, 1, 1, 1),
    (2, CAP, 2, 2),  # the entry point's channel cap, HW = 4
    (64, 2048, 7, 7),  # the benchmark's last stage: two 32 KiB tables, more work than resident blocks (the blocks loop)
]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _mismatches(got, want):
    return int((_bits(got) != _bits(want)).sum().item())


def _params(C, g, eps):
    mean = torch.randn(C, device=DEV, generator=g)
    var = torch.exp(torch.empty(C, device=DEV).uniform_(-39.1, 9.2, generator=g))  # 1e-17 ... 1e4, log-uniform
    weight = torch.randn(C, device=DEV, generator=g)
    weight[1::4] = -weight[1::4].abs()
    weight[2::8] = 0.0
    weight[6::8] = -0.0
    bias = torch.randn(C, device=DEV, generator=g)
    return [mean, var, weight, bias, eps]


def _inputs(B, C, H, W, seed):
    """Two tensors and two BatchNorms (eps 1e-5 and 1e-3).  Where x equals its channel's mean the BatchNorm value is the bias
    exactly, so channel 0 (opposite biases) sums to +0.0 there and channel 1 (negative weights, biases -0.0) to -0.0."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    xa = torch.randn(B, C, H, W, device=DEV, generator=g) * 4
    xb = torch.randn(B, C, H, W, device=DEV, generator=g) * 2
    pa, pb = _params(C, g, 1e-5), _params(C, g, 1e-3)
    pb[3][0] = -pa[3][0]
    if C > 1:
        for p in (pa, pb):
            p[2][1], p[3][1] = -1.5, -0.0
    fa, fb, ia, ib = xa.view(-1), xb.view(-1), xa.view(-1).view(torch.int32), xb.view(-1).view(torch.int32)
    ia[0::29], ib[1::29] = 0x7FC00123, 0x7FC00456  # NaN in one operand only, distinct payloads
    ia[2::29], ib[2::29] = 0x7FC00AAA, 0x7FC00BBB  # NaN in both operands of one add
    ia[9::29], ib[9::29] = 0xFFC00001 - (1 << 32), 0x7FC00002  # ... of either sign
    fa[3::29], fb[4::29] = float("inf"), -float("inf")
    fa[5::29], fb[5::29] = float("inf"), float("inf")  # inf - inf for the channels whose weights differ in sign
    fa[6::29], fb[7::29] = -0.0, 0.0
    for start in (8, 10):  # x == mean
        idx = torch.arange(xa.numel(), device=DEV)[start::29]
        ch = (idx // (H * W)) % C
        fa[idx], fb[idx] = pa[0][ch], pb[0][ch]
    return xa, pa, xb, pb


def _want(xa, pa, xb, pb):
    return torch.relu_(F.batch_norm(xa, *pa[:4], False, 0.0, pa[4]) + F.batch_norm(xb, *pb[:4], False, 0.0, pb[4]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_pytorch_bit_for_bit_in_both_operand_orders_under_every_policy(shape):
    xa, pa, xb, pb = _inputs(*shape, seed=sum(shape))
    bad = {}
    try:
        for order, args in (("ab", (xa, pa, xb, pb)), ("ba", (xb, pb, xa, pa))):
            want = _want(*args)
            for policy in (0, 1, 2, 3):
                N.set_option("bn_policy", policy)
                bad[(order, policy)] = _mismatches(N.batchnorm_infer_add_bn_relu(*args), want)
    finally:
        N.set_option("bn_policy", 0)
    print(shape, bad)
    assert all(v == 0 for v in bad.values()), bad


def test_special_values_reach_the_add():
    """The inputs above do produce what they are meant to: both zeros of a cancelling sum, and NaNs of both operands."""
    xa, pa, xb, pb = _inputs(3, 7, 2, 6, seed=18)
    ya, yb = F.batch_norm(xa, *pa[:4], False, 0.0, pa[4]), F.batch_norm(xb, *pb[:4], False, 0.0, pb[4])
    total = _bits(ya + yb).view(-1)
    both_nan = (ya.isnan() & yb.isnan()).view(-1)
    assert int((total == 0).sum()) > 0 and int((total == -(1 << 31)).sum()) > 0  # +0.0 and -0.0
    assert int(both_nan.sum()) > 0 and int((_bits(ya).view(-1)[both_nan] != _bits(yb).view(-1)[both_nan]).sum()) > 0


def test_argument_checks_and_the_channel_cap():
    xa, pa, xb, pb = _inputs(1, CAP + 1, 2, 2, seed=5)
    with pytest.raises(ValueError, match="channels exceed"):
        N.batchnorm_infer_add_bn_relu(xa, pa, xb, pb)
    x = torch.zeros(1, 4, 2, 2, device=DEV)
    p = [torch.zeros(4, device=DEV)] * 4 + [1e-5]
    with pytest.raises(ValueError, match="one shape"):
        N.batchnorm_infer_add_bn_relu(x, p, torch.zeros(1, 4, 2, 3, device=DEV), p)
    with pytest.raises(ValueError, match="16-byte aligned"):
        N.batchnorm_infer_add_bn_relu(x, p, torch.zeros(20, device=DEV)[1:17].view(1, 4, 2, 2), p)
    with pytest.raises(ValueError, match="per-channel"):
        N.batchnorm_infer_add_bn_relu(x, p, x, [torch.zeros(3, device=DEV)] * 4 + [1e-5])
    empty = torch.zeros(0, 4, 2, 2, device=DEV)
    assert N.batchnorm_infer_add_bn_relu(empty, p, empty, p).shape == (0, 4, 2, 2)


# ------------------------------------------------------------------------------------------------ the rewrite
class _Block(nn.Module):
    """A residual block of norms and activations whose shortcut is a Sequential that ends in a BatchNorm2d.  No convolution:
    MIOpen's small convolutions do not reproduce themselves from call to call on this stack."""

    def __init__(self, c, into_shortcut=False):
        super().__init__()
        self.bn1, self.bn2, self.relu = nn.BatchNorm2d(c), nn.BatchNorm2d(c), nn.ReLU(inplace=True)
        self.downsample = nn.Sequential(nn.AvgPool2d(1), nn.BatchNorm2d(c))
        self.into_shortcut = into_shortcut

    def forward(self, x):
        idt = self.downsample(x)
        out = self.relu(self.bn1(x))
        out = self.bn2(out)
        if self.into_shortcut:
            idt += out
            return self.relu(idt)
        out += idt
        return self.relu(out)


class _Net(nn.Module):
    """7 BatchNorm2d; layer1 at 14 x 14 (aligned), layer2 at 7 x 7 (16-byte pieces cross planes)."""

    def __init__(self, c, into_shortcut=False):
        super().__init__()
        self.bn1, self.relu, self.pool = nn.BatchNorm2d(c), nn.ReLU(inplace=True), nn.AvgPool2d(2)
        self.layer1, self.layer2 = _Block(c), _Block(c, into_shortcut)

    def forward(self, x):
        return self.layer2(self.pool(self.layer1(self.relu(self.bn1(x)))))


N_BN = 7


def _net(c=32, hw=14, seed=0, **kwargs):
    g = torch.Generator().manual_seed(seed)
    model = _Net(c, **kwargs).eval()
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(c, generator=g))
            m.running_var.copy_(torch.rand(c, generator=g) + 0.1)
            m.weight.data.copy_(torch.randn(c, generator=g))
            m.bias.data.copy_(torch.randn(c, generator=g))
    model.layer1.downsample[1].eps = 1e-3
    return model.to(DEV), torch.randn(4, c, hw, hw, generator=g).to(DEV)


def _plain(model, x):
    with torch.no_grad():
        first, second = model(x), model(x)
    assert _mismatches(first, second) == 0, "the unfused model does not reproduce itself"
    return first


def _under_context(model, x):
    cache = ActMaxCache([], aggregators.aggregate_conv_max, 5)
    with torch.no_grad(), cache.hook_context(model):
        return model(x)


def _identity(model):
    return ([(n, id(m), m.__dict__.get("forward")) for n, m in model.named_modules()],
            [(n, id(p), p._version) for n, p in model.named_parameters()], [(n, id(b)) for n, b in model.named_buffers()])


@pytest.fixture
def prof():
    N.prof_enable(True)
    N.prof_reset()
    yield
    N.prof_reset()
    N.prof_enable(False)


def _slot():
    """(BatchNorm2d evaluations, algorithmic bytes) of the profile slot since the last reset."""
    _, launches, work = N.prof_read(N.SL_PROF_BATCHNORM)
    return launches, work


def _bytes(model, x, two_kernel=()):
    """What the slot's bytes must be: bn + relu is 2 passes, a tail 3, and a pair on the two-kernel path adds the shortcut norm's 2."""
    t1, t2 = x.numel() * 4, x.numel()
    return 2 * t1 + (5 + 2 * ("layer1" in two_kernel)) * t1 + (5 + 2 * ("layer2" in two_kernel)) * t2


def test_residual_net_is_bit_identical_counted_and_untouched(prof):
    model, x = _net()
    before = _identity(model)
    want = _plain(model, x)
    assert _slot()[0] == 0
    got = _under_context(model, x)  # with the proofs
    assert _mismatches(got, want) == 0 and _slot() == (N_BN, _bytes(model, x)) and _identity(model) == before
    N.prof_reset()
    got = _under_context(model, x)  # the verified plan
    assert _mismatches(got, want) == 0 and _slot() == (N_BN, _bytes(model, x)) and _identity(model) == before
    assert all(f.verified and not f.dropped for _, fused in _bn_fuse._PLANS[model].duals.values() for f in fused)


@pytest.mark.parametrize("where,two_kernel", [("layer1.downsample", True), ("layer1.downsample.1", True), ("layer1.downsample.0", False)])
def test_hooks_on_the_shortcut_fire_once_with_the_unfused_tensors(where, two_kernel, prof):
    model, x = _net()
    want_seen, seen = [], []
    target = model.get_submodule(where)
    handle = target.register_forward_hook(lambda m, i, o: want_seen.append((i[0].clone(), o.clone())))
    want = _plain(model, x)
    handle.remove()
    handle = target.register_forward_hook(lambda m, i, o: seen.append((i[0].clone(), o.clone())))
    try:
        got = _under_context(model, x)
    finally:
        handle.remove()
    assert len(seen) == 1 and _mismatches(seen[0][0], want_seen[0][0]) == 0 and _mismatches(seen[0][1], want_seen[0][1]) == 0
    assert _mismatches(got, want) == 0
    assert _slot() == (N_BN, _bytes(model, x, two_kernel=("layer1",) if two_kernel else ()))


def test_iadd_into_the_shortcut_output_is_not_fused(prof):
    model, x = _net(into_shortcut=True)
    before = _identity(model)
    want = _plain(model, x)
    got = _under_context(model, x)
    plan = _bn_fuse._PLANS[model]
    owners = [plan.parents[i][0]() for i in plan.duals]
    assert owners == [model.layer1]
    # layer2: bn1 + relu fused, bn2 and the shortcut's norm plain, add and relu as the user wrote them
    t1, t2 = x.numel() * 4, x.numel()
    assert _slot() == (N_BN, 2 * t1 + 5 * t1 + 6 * t2)
    assert _mismatches(got, want) == 0 and _identity(model) == before


def test_above_the_channel_cap_the_rewrite_gives_the_two_kernel_result(prof):
    model, x = _net(c=CAP + 1, hw=4)  # (2 x 2 after the pool: a 1 x 1 plane also counts as channels_last and is left alone)
    want = _plain(model, x)
    got = _under_context(model, x)
    assert _mismatches(got, want) == 0
    assert _slot() == (N_BN, _bytes(model, x, two_kernel=("layer1", "layer2")))
