"""K27 on the device: the convolution + residual-tail kernels against the raw product followed by the K16 / K19 kernels, BIT FOR
BIT; the product against float64 within the bound of a 64-term fma chain; independence of where a pixel sits; further trips of
the persistent loop; and a stack of layer1's blocks under `hook_context`, whether its sites prove or are dropped."""
import warnings

import pytest
import torch
import torch.nn as nn

import synth
from semanticlens_amd import _native as N
from semanticlens_amd.component_visualization import _bn_fuse, aggregators
from semanticlens_amd.component_visualization.activation_caching import ActMaxCache

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (images, H, W).  A wave takes 32 pixels: 7 x 7 ends in a ragged tile and is not a multiple of 4 (no 16-byte pieces), 8 x 8 is
# whole tiles that end with the image, 9 x 9 is both ragged and unaligned, 56 x 56 is the headline's plane
SHAPES = [(1, 7, 7), (3, 7, 7), (1, 8, 8), (3, 8, 8), (1, 9, 9), (3, 9, 9), (2, 56, 56)]
GAMMA_66 = 66 * 2.0**-24 / (1 - 66 * 2.0**-24)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _mismatches(got, want):
    return int((_bits(got) != _bits(want)).sum().item())


def _bn(gen, special=True):
    C = 256
    mean = torch.randn(C, device=DEV, generator=gen)
    var = torch.exp(torch.empty(C, device=DEV).uniform_(-7.0, 3.0, generator=gen))
    weight = torch.randn(C, device=DEV, generator=gen)
    bias = torch.randn(C, device=DEV, generator=gen)
    if special:
        var[::7] = torch.exp(torch.empty(C, device=DEV).uniform_(-40.0, -20.0, generator=gen))[::7]  # very small variances
        var[3], var[19], var[35] = 0.0, float("inf"), float("nan")
        weight[1::4] = -weight[1::4].abs()
        weight[2::8], weight[10], weight[26], weight[42], weight[58] = 0.0, -0.0, float("inf"), -float("inf"), float("nan")
        bias[::6], bias[3::6] = 0.0, -0.0
        bias[9], bias[21], bias[33] = float("inf"), -float("inf"), float("nan")
        mean[4], mean[20], mean[36] = float("nan"), float("inf"), -float("inf")
    return [mean, var, weight, bias, 1e-5]


def _operands(n, h, w, seed, special=True):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    xa, xb = (torch.randn(n, 64, h, w, device=DEV, generator=gen) * 2 for _ in range(2))
    xa.view(-1)[5::37] = 0.0  # what a ReLU in front leaves
    wa, wb = (torch.randn(256, 64, 1, 1, device=DEV, generator=gen) * 0.125 for _ in range(2))
    idt = torch.randn(n, 256, h, w, device=DEV, generator=gen)
    if special:
        flat = idt.view(-1)
        flat[0::101], flat[1::101], flat[2::101] = float("nan"), float("inf"), -float("inf")
        flat[3::101], flat[4::101] = -0.0, 0.0
    return xa, wa, _bn(gen, special), xb, wb, _bn(gen, special), idt


@pytest.fixture(scope="module")
def cases():
    """Per shape: the operands and the raw products under the split the tails take (computed once, left unchanged)."""
    out = {}
    for i, (n, h, w) in enumerate(SHAPES):
        xa, wa, pa, xb, wb, pb, idt = _operands(n, h, w, seed=100 + i)
        out[(n, h, w)] = dict(xa=xa, wa=wa, pa=pa, xb=xb, wb=wb, pb=pb, idt=idt, ca=N.conv1x1_64_256(xa, wa, 0),
                              cb=N.conv1x1_64_256(xb, wb, 0))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_forms_equal_the_product_followed_by_the_tail_kernels(cases, shape):
    c = cases[shape]
    bad = {}
    got = N.conv1x1_bn_add_relu(c["xa"], c["wa"], c["pa"], c["idt"])
    bad["add_relu"] = _mismatches(got, N.batchnorm_infer(c["ca"], *c["pa"], residual=c["idt"]))
    plain = N.batchnorm_infer(c["ca"], *c["pa"])
    cancel = torch.nan_to_num(-plain, nan=1.0, posinf=1.0, neginf=-1.0)  # bn + identity == 0 exactly: the sign of the sum
    got = N.conv1x1_bn_add_relu(c["xa"], c["wa"], c["pa"], cancel)
    bad["add_relu_cancel"] = _mismatches(got, N.batchnorm_infer(c["ca"], *c["pa"], residual=cancel))
    got = N.conv1x1_bn_add_conv1x1_bn_relu(c["xa"], c["wa"], c["pa"], c["xb"], c["wb"], c["pb"])
    bad["dual"] = _mismatches(got, N.batchnorm_infer_add_bn_relu(c["ca"], c["pa"], c["cb"], c["pb"]))
    got = N.conv1x1_bn_add_conv1x1_bn_relu(c["xb"], c["wb"], c["pb"], c["xa"], c["wa"], c["pa"])  # the other operand order
    bad["dual_swapped"] = _mismatches(got, N.batchnorm_infer_add_bn_relu(c["cb"], c["pb"], c["ca"], c["pa"]))
    print(shape, bad)
    assert all(v == 0 for v in bad.values()), bad


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_product_is_within_the_fma_chain_bound_of_float64(cases, shape):
    c = cases[shape]
    x, w = c["xa"].double(), c["wa"].view(256, 64).double()
    ref = torch.einsum("oc,nchw->nohw", w, x)
    bound = GAMMA_66 * torch.einsum("oc,nchw->nohw", w.abs(), x.abs())
    for split in range(N.CONV_TAIL_SPLITS):
        got = c["ca"] if split == 0 else N.conv1x1_64_256(c["xa"], c["wa"], split)
        excess = ((got.double() - ref).abs() - bound).max().item()
        print(shape, "split", split, "max (|got - ref| - bound)", excess, "max bound", bound.max().item())
        assert excess <= 0.0, (split, excess)


def test_a_pixel_gives_the_same_bits_wherever_it_sits():
    gen = torch.Generator(device=DEV).manual_seed(7)
    col = torch.randn(64, device=DEV, generator=gen)
    w = torch.randn(256, 64, 1, 1, device=DEV, generator=gen) * 0.125
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    seen = []
    # (images, H, W, image, pixel): first lane of a tile, inside a ragged last tile, the last pixel of an image, an unaligned
    # plane, and a grid at its cap, where the pixel belongs to a wave's later trip
    for n, h, wd, img, px in ((1, 8, 8, 0, 0), (3, 9, 9, 2, 77), (2, 56, 56, 1, 3135), (3, 7, 7, 1, 48), (cus * 16 + 5, 8, 8, cus * 16 + 4, 37)):
        x = torch.randn(n, 64, h, wd, device=DEV, generator=gen)
        x.view(n, 64, -1)[img, :, px] = col
        for split in (0, 4):
            y = N.conv1x1_64_256(x, w, split)
            seen.append((split, _bits(y).view(n, 256, -1)[img, :, px].clone()))
    for split, bits in seen[2:]:
        assert torch.equal(bits, seen[split // 4][1]), "the product of one pixel depends on where the pixel sits"
    assert not torch.equal(seen[0][1], seen[1][1])  # (the two splits do differ: the comparison sees what it should)


def test_later_trips_of_the_persistent_loop():
    """More (image, tile) pairs than the capped grid has waves: every wave takes a second trip, then up to five."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = cus * 2 * 8  # waves of the capped grid: two blocks of eight waves per CU (one block for the two-product form)
    xa, wa, pa, xb, wb, pb, idt = _operands(3, 8, 8, seed=11, special=False)
    small = (N.conv1x1_64_256(xa, wa, 0), N.conv1x1_bn_add_relu(xa, wa, pa, idt),
             N.conv1x1_bn_add_conv1x1_bn_relu(xa, wa, pa, xb, wb, pb))
    assert 3 * 2 <= cap  # the small problem is one trip
    for n in (cap + 1, 2 * cap + 1):
        reps = -(-n // 3)
        big = [t.repeat(reps, 1, 1, 1)[:n].contiguous() for t in (xa, xb, idt)]
        got = (N.conv1x1_64_256(big[0], wa, 0), N.conv1x1_bn_add_relu(big[0], wa, pa, big[2]),
               N.conv1x1_bn_add_conv1x1_bn_relu(big[0], wa, pa, big[1], wb, pb))
        for name, g, s in zip(("product", "add_relu", "dual"), got, small):
            bad = _mismatches(g, s.repeat(reps, 1, 1, 1)[:n])
            print("images", n, name, "mismatches", bad)
            assert bad == 0, (n, name)
        del big, got


def test_argument_checks():
    x, w = torch.zeros(1, 64, 2, 2, device=DEV), torch.zeros(256, 64, 1, 1, device=DEV)
    with pytest.raises(ValueError, match="expected"):
        N.conv1x1_64_256(torch.zeros(1, 32, 2, 2, device=DEV), w, 0)
    with pytest.raises(ValueError, match="expected"):
        N.conv1x1_64_256(x, torch.zeros(128, 64, 1, 1, device=DEV), 0)
    with pytest.raises(ValueError, match="split"):
        N.conv1x1_64_256(x, w, 7)
    with pytest.raises(ValueError, match="permutation"):
        N.conv1x1_64_256(x, w, 0, torch.zeros(64, dtype=torch.int32, device=DEV))
    assert N.conv1x1_64_256(torch.zeros(0, 64, 2, 2, device=DEV), w, 0).shape == (0, 256, 2, 2)


# ------------------------------------------------------------------------------------------------ a stack of layer1's blocks
def _stack(seed=0):
    torch.manual_seed(seed)
    model = nn.Sequential(synth.Bottleneck(64, 64), synth.Bottleneck(256, 64), synth.Bottleneck(256, 64))
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2), m.running_var.uniform_(0.5, 2.0), m.weight.data.normal_(1, 0.2), m.bias.data.normal_(0, 0.2)
    return model.to(DEV).eval()


def _run(model, x, hooked):
    with torch.no_grad():
        if not hooked:
            return model(x)
        cache = ActMaxCache(["2"], aggregators.aggregate_conv_max, 3)
        with cache.hook_context(model):
            return model(x)


class _Calls:
    """Counts the calls of the two fused entry points; `spoil` makes them return something else, so that no site proves."""

    def __init__(self, monkeypatch, spoil=False):
        self.n = {"single": 0, "dual": 0}
        one, two = N.conv1x1_bn_add_relu, N.conv1x1_bn_add_conv1x1_bn_relu

        def single(*a):
            self.n["single"] += 1
            return one(*a) + 1 if spoil else one(*a)

        def dual(*a):
            self.n["dual"] += 1
            return two(*a) + 1 if spoil else two(*a)

        monkeypatch.setattr(N, "conv1x1_bn_add_relu", single)
        monkeypatch.setattr(N, "conv1x1_bn_add_conv1x1_bn_relu", dual)


def _gates(model):
    plan = _bn_fuse._PLANS[model]
    return [g for _, gates in plan.convs.values() for g in gates]


def test_stack_is_bit_identical_whether_its_sites_prove_or_not(monkeypatch):
    model = _stack()
    x = torch.randn(3, 64, 56, 56, device=DEV)
    want = _run(model, x, hooked=False)
    calls = _Calls(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # a site that does not prove says so; that is MIOpen's choice here
        first = _run(model, x, hooked=True)
        second = _run(model, x, hooked=True)
    gates = _gates(model)
    proven = sum(bool(g.verified) for g in gates)
    print("sites:", len(gates), "proven:", proven, "dropped:", sum(g.dropped for g in gates), "calls:", calls.n)
    assert len(gates) == 3 and calls.n["single"] + calls.n["dual"] == 3 + proven  # a dropped site is not tried again
    assert _mismatches(first, want) == 0 and _mismatches(second, want) == 0
    assert all("forward" not in m.__dict__ for m in model.modules())


def test_stack_is_bit_identical_when_every_site_is_dropped(monkeypatch):
    model = _stack(seed=1)
    x = torch.randn(3, 64, 56, 56, device=DEV)
    want = _run(model, x, hooked=False)
    calls = _Calls(monkeypatch, spoil=True)
    with pytest.warns(RuntimeWarning, match="did not reproduce"):
        first = _run(model, x, hooked=True)
    gates = _gates(model)
    assert len(gates) == 3 and all(g.dropped and not g.verified for g in gates) and calls.n == {"single": 2, "dual": 1}
    second = _run(model, x, hooked=True)  # one level down now: the K16 / K19 graphs
    assert calls.n == {"single": 2, "dual": 1}
    assert _mismatches(first, want) == 0 and _mismatches(second, want) == 0


def test_a_hooked_convolution_keeps_the_k16_path_and_its_hook_fires_once(monkeypatch):
    model = _stack(seed=2)
    x = torch.randn(3, 64, 56, 56, device=DEV)
    want = _run(model, x, hooked=False)
    calls = _Calls(monkeypatch)
    fired = []
    handle = model[1].conv3.register_forward_hook(lambda m, i, o: fired.append(o.clone()))
    N.prof_enable(True)
    N.prof_reset()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            got = _run(model, x, hooked=True)
        launches = N.prof_read(N.SL_PROF_BATCHNORM)[1]
    finally:
        handle.remove()
        N.prof_reset()
        N.prof_enable(False)
    assert len(fired) == 1 and calls.n["single"] == 1 and calls.n["dual"] == 1  # blocks 0 and 2 fused, block 1 not
    assert _mismatches(got, want) == 0
    assert launches >= 10  # every BatchNorm2d of the stack still ran on the library's kernels (proofs launch none)
    with torch.no_grad():  # what the hook saw is conv3's output
        b = model[1]
        assert _mismatches(fired[0], b.conv3(b.relu(b.bn2(b.conv2(b.relu(b.bn1(b.conv1(model[0](x))))))))) == 0


@pytest.mark.parametrize("switch", ["SEMANTICLENS_AMD_FUSE_CONV", "SEMANTICLENS_AMD_FUSE_BN"])
def test_switches(monkeypatch, switch):
    model = _stack(seed=3)
    x = torch.randn(3, 64, 56, 56, device=DEV)
    want = _run(model, x, hooked=False)
    calls = _Calls(monkeypatch)
    monkeypatch.setenv(switch, "0")
    N.prof_enable(True)
    N.prof_reset()
    try:
        got = _run(model, x, hooked=True)
        launches = N.prof_read(N.SL_PROF_BATCHNORM)[1]
    finally:
        N.prof_reset()
        N.prof_enable(False)
    assert calls.n == {"single": 0, "dual": 0} and _mismatches(got, want) == 0
    assert (launches == 0) if switch.endswith("FUSE_BN") else (launches >= 10)  # FUSE_CONV=0 leaves K16 / K19 at work
