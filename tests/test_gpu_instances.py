"""K7 / K11: every built instance of the clarity and encoder kernel families against float64.

The kernels here are template families whose instance is picked from the shape (`clarity_multi_kernel<PPL>` by the width,
`attention_*_kernel<D, MAXW>` by head size and sequence length, `LinearEpi<ACT, RES, REMAP, SPLIT>` by the epilogue, the
LayerNorm kernel by width and alignment) and whose grid changes regime with the device's CU count.  Each case below is the
smallest shape that reaches one instance or one regime that the rest of the suite does not launch on its own; every
reference is float64 computed from the same fp32 inputs, and the bounds are the ones the suite already holds these entry
points to.  The CU count is read from the device, so the grid thresholds follow the part the suite runs on."""
import functools
import math

import numpy as np
import pytest
import torch

import oracle
from semanticlens_amd import _native as N
from semanticlens_amd import scores

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def rel_err(a, b):
    """max |a - b| over max |b| (the measure of test_gpu_native_clip.py), taken in float64"""
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def poison(numel: int, dtype=torch.float32):
    """Leave a NaN-filled block of this size in the allocator's cache: an output element that a kernel skips then reads NaN
    instead of an earlier call's (right) answer."""
    torch.full((numel,), float("nan"), dtype=dtype, device=DEV)  # freed at once: the next allocation of this size gets it


# ---- 1. clarity: PPL instances and grid regimes ------------------------------------------------------------------------------
def clarity64(V: torch.Tensor) -> torch.Tensor:
    """scores.hip:29-31 in float64: rows normalised with eps 1e-12, mean over n, ((|m|^2) - 1/n) / (n - 1) * n."""
    V = V.double()
    n = V.shape[-2]
    m = (V / V.norm(dim=-1, keepdim=True).clamp_min(1e-12)).mean(-2)
    return ((m * m).sum(-1) - 1.0 / n) / (n - 1) * n


def assert_clarity(got: torch.Tensor, V: torch.Tensor, tag):
    want = clarity64(V)
    assert got.shape == want.shape and got.dtype == torch.float32, tag
    err = (got.double() - want).abs().max().item() if want.numel() else 0.0
    assert err <= 1e-5, (tag, err)  # NaN (a skipped component) fails too
    return err


def test_float64_clarity_restatement_matches_the_oracle():
    rng = np.random.RandomState(5)
    V = (rng.randn(7, 3, 768) * rng.rand(7, 1, 1) * 3).astype(np.float32)
    V[2, 1] = 0.0
    want = oracle.clarity(V)
    np.testing.assert_allclose(clarity64(torch.from_numpy(V)).numpy(), want, rtol=0, atol=1e-5)


@pytest.mark.parametrize("D", [640, 768, 1024, 1536, 1792])
def test_clarity_pieces_per_lane_3_4_6_7(D):
    """`clarity_multi_kernel<PPL>`, PPL = ceil(D / 256) = 3, 3, 4, 6, 7: the widths of CLIP ViT-L/14, RN50 and ViT-H embeddings
    (the rest of the suite runs PPL 1, 2, 5, 8).  One zero-norm row (F.normalize's eps path) and one component whose rows
    differ by 1e3 in scale."""
    g = torch.Generator(device=DEV).manual_seed(D)
    V = torch.randn(5, 3, D, device=DEV, generator=g)
    V[1, 0] = 0.0
    V[2, 1] *= 1e3
    V[2, 2] *= 1e-3
    V[4] *= 37.0
    errs = [assert_clarity(scores.clarity_score(V), V, ("clarity_score", D)), assert_clarity(N.clarity(V), V, ("clarity", D)),
            assert_clarity(N.clarity_multi([V])[0], V, ("clarity_multi", D))]
    print(f"clarity D={D} PPL={(D // 4 + 63) // 64}: max |got - float64| = {max(errs):.3g}")


def angle_components(C: int, D: int, seed: int) -> torch.Tensor:
    """(C, 2, D): component c holds two rows at an angle drawn for c (and of c-dependent lengths), so its clarity is the
    cosine of that angle: a component that is read twice, skipped or written to another slot shows."""
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(D, 2, generator=g, dtype=torch.float64))
    u, w = q[:, 0], q[:, 1]
    theta = torch.rand(C, generator=g, dtype=torch.float64) * math.pi
    c = torch.arange(C, dtype=torch.float64)
    V = torch.empty(C, 2, D, dtype=torch.float64)
    V[:, 0] = u * (1.0 + (c % 7))[:, None]
    V[:, 1] = (torch.cos(theta)[:, None] * u + torch.sin(theta)[:, None] * w) * (0.5 + (c % 5))[:, None]
    return V.float().to(DEV)


@pytest.mark.parametrize("D", [8, 6])
@pytest.mark.parametrize("mult,extra", [(8, 0), (8, 1), (16, 0), (16, 1)])
def test_clarity_grid_regimes(D, mult, extra):
    """C on both sides of 8 CUs (one workgroup per component -> resident grid that strides over the components, where the
    layer cursor advances and the LDS sums are reused) and of 16 CUs (-> one workgroup per component again), for the one-pass
    kernel (D = 8) and for the two-pass kernel's own grid stride (D = 6)."""
    C = mult * cus() + extra
    V = angle_components(C, D, seed=C + D)
    poison(C)
    err = assert_clarity(N.clarity(V), V, (C, D))
    print(f"clarity C={C} ({mult} CUs + {extra}) D={D}: max |got - float64| = {err:.3g}")


def test_clarity_multi_grid_stride_crosses_a_layer_boundary_and_an_empty_layer():
    n_cu = cus()
    Cs = (8 * n_cu - 3, 0, 9)  # 8 CUs + 6 components in all: the resident grid's second visit starts in the last layer
    Vs = [angle_components(C, 8, seed=40 + i) if C else torch.empty(0, 2, 8, device=DEV) for i, C in enumerate(Cs)]
    for C in Cs:
        poison(C)
    got = N.clarity_multi(Vs)
    assert got is not None and len(got) == 3
    for i, (o, V) in enumerate(zip(got, Vs)):
        assert_clarity(o, V, ("layer", i))
    assert got[1].shape == (0,)


def test_clarity_slab_one_float_past_a_16_byte_boundary():
    """A slab that is not 16-byte aligned leaves the float4 kernel for the two-pass one (scores.hip: `fast`): same values."""
    C, n, D = 4, 3, 768
    g = torch.Generator(device=DEV).manual_seed(3)
    buf = torch.randn(C * n * D + 4, device=DEV, generator=g)
    V_off = buf[1:1 + C * n * D].view(C, n, D)
    V = V_off.clone()
    assert V.data_ptr() % 16 == 0 and V_off.data_ptr() % 16 == 4 and V_off.is_contiguous()
    aligned, off = N.clarity(V), N.clarity(V_off)
    assert_clarity(aligned, V, "aligned")
    assert_clarity(off, V, "offset")
    assert (aligned - off).abs().max().item() <= 1e-5
    assert_clarity(N.clarity_multi([V, V_off])[1], V, "multi, second layer offset")


# ---- 2. attention instances ---------------------------------------------------------------------------------------------------
def attention64(qkv, B, T, H, D, causal):
    q, k, v = (qkv.double().reshape(B, T, 3, H, D)[:, :, i].permute(0, 2, 1, 3) for i in range(3))  # (B, H, T, D)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(D)
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device=s.device).triu_(1), float("-inf"))
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * T, H * D)


def check_attention(D, T, causal, bf16x3, bound):
    B, H = 2, 2
    g = torch.Generator(device=DEV).manual_seed(1000 * D + T)
    qkv = torch.randn(B * T, 3 * H * D, device=DEV, generator=g)
    want = attention64(qkv, B, T, H, D, causal)
    poison(B * T * H * D)
    got = N.attention(qkv, B, T, H, D, causal, bf16x3=bf16x3)
    err = (got.double() - want).abs().max().item()
    tol = bound * max(1.0, want.abs().max().item())
    print(f"attention {'bf16x3' if bf16x3 else 'fp32'} D={D} T={T} causal={causal}: max |got - float64| = {err:.3g} (bound {tol:.3g})")
    assert err < tol, (D, T, causal, err)
    sp = N.Split(B * T, H * D, DEV)
    N.attention(qkv, B, T, H, D, causal, out_split=sp, bf16x3=bf16x3)
    assert (sp.hi.float() + sp.lo.float() - got).abs().max().item() <= 2.0 ** -16 * got.abs().max().item() + 1e-9


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D,T", [(32, 161), (88, 257), (80, 100), (96, 128), (104, 161), (72, 161)])
def test_attention_bf16x3_instances(D, T, causal):
    """`attention_bf16x3_kernel<D, MAXW>`, MAXW = 8 iff more than four query tiles and D <= 96: <32, 8>, <88, 8> (ViT-g/14's own
    shape), <80, 4>, <96, 4>, <104, 4> over two key chunks and <72, 8> outside a tower."""
    check_attention(D, T, causal, True, 2e-5)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D,T", [(32, 257), (72, 193), (88, 193), (104, 129)])
def test_attention_fp32_second_key_chunk(D, T, causal):
    """`attention_mfma_kernel<D>` past one LDS chunk of keys (256 / 192 / 128 keys for D <= 64 / <= 96 / above) for the four
    head sizes the rest of the suite runs inside one chunk."""
    check_attention(D, T, causal, False, 2e-6)


# ---- 4. (before 3: its bound is part of 3's) the activations, pointwise --------------------------------------------------------
def gelu64(z):
    return 0.5 * z * torch.special.erfc(-z * math.sqrt(0.5))  # = 0.5 z (1 + erf(z / sqrt 2)) without the cancellation at z << 0


def gelu_tanh64(z):
    return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def quickgelu64(z):
    return z * torch.sigmoid(1.702 * z)


ACTS = {
    "gelu": (N.SL_ACT_GELU, gelu64, torch.nn.functional.gelu),
    "gelu_tanh": (N.SL_ACT_GELU_TANH, gelu_tanh64, lambda x: torch.nn.functional.gelu(x, approximate="tanh")),
    "quickgelu": (N.SL_ACT_QUICKGELU, quickgelu64, lambda x: x * torch.sigmoid(1.702 * x)),
}
SPECIALS = [0.0, 1e-30, 20.0, 60.0, 1e4, float("inf")]
SATURATED = [60.0, 1e4, float("inf")]  # every activation has reached x, +-0 or NaN in fp32


def activation_grid() -> torch.Tensor:
    return torch.linspace(-12.0, 12.0, 8192, dtype=torch.float64).float().to(DEV)


@functools.lru_cache(maxsize=None)
def torch_fp32_error(name: str) -> float:
    """max |torch's fp32 op on the GPU - float64| over the 8 192-point grid on [-12, 12]"""
    _, f64, f32 = ACTS[name]
    x = activation_grid()
    return (f32(x).double() - f64(x.double())).abs().max().item()


def activation_bound(name: str, z64: torch.Tensor) -> torch.Tensor:
    """Pointwise absolute bound at (finite) float64 arguments `z64`.  GELU on [-8, 8]: the kernel's own claim (encoder_epilogue.hpp,
    `erf_as`), 4.7e-7, and one fp32 rounding of the result.  Elsewhere: four times torch's own fp32 distance from float64 on the
    grid (the kernels have two 1-ulp approximate instructions and two roundings that torch's op has not), never below
    2^-22 max(1, |want|)."""
    want = ACTS[name][1](z64)
    b = torch.maximum(torch.full_like(want, 4.0 * torch_fp32_error(name)), 2.0 ** -22 * want.abs().clamp_min(1.0))
    if name == "gelu":
        b = torch.where(z64.abs() <= 8.0, 4.7e-7 + 2.0 ** -24 * want.abs(), b)
    return b


def pointwise(x: torch.Tensor, act: int) -> torch.Tensor:
    """act(x) through `sl_linear`: K = 1, w = 1, no bias, fp32-input matrix cores (exact products): no GEMM rounding"""
    return N.linear(x.reshape(-1, 1).contiguous(), torch.ones(1, 1, device=DEV), act=act).reshape(-1)


def activation_points() -> torch.Tensor:
    sp = torch.tensor([s * v for v in SPECIALS for s in (1.0, -1.0)], dtype=torch.float32, device=DEV)
    return torch.cat([activation_grid(), sp])


def test_pointwise_identity_is_exact():
    x = activation_points()
    got = pointwise(x, N.SL_ACT_NONE)
    assert torch.equal(got, x)  # values (inf included); -0 == +0 here
    nz = x != 0
    assert torch.equal(got[nz].view(torch.int32), x[nz].view(torch.int32))  # the accumulator's + 0 turns -0 into +0, nothing else moves


@pytest.mark.parametrize("name", list(ACTS))
def test_pointwise_activation_against_float64(name):
    code, f64, f32 = ACTS[name]
    x = activation_points()
    got = pointwise(x, code)
    fin = torch.isfinite(x)
    z = x[fin].double()
    err = (got[fin].double() - f64(z)).abs()
    bound = activation_bound(name, z)
    ngrid = 8192
    line = f"{name}: max |fp32 - float64| on [-12, 12]: torch {torch_fp32_error(name):.3g}, kernel {err[:ngrid].max().item():.3g}"
    if name == "gelu":
        line += f"; kernel on [-8, 8] {err[:ngrid][z[:ngrid].abs() <= 8.0].max().item():.3g} (claim 4.7e-7)"
    print(line)
    worst = (err - bound).argmax()
    assert bool((err <= bound).all()), (name, z[worst].item(), err[worst].item(), bound[worst].item())
    # non-finite and saturated inputs: torch's fp32 result, exactly (NaN where torch has NaN; the sign of a zero is free)
    sat = torch.tensor([s * v for v in SATURATED for s in (1.0, -1.0)], dtype=torch.float32, device=DEV)
    got_s, want_s = pointwise(sat, code), f32(sat)
    same = (got_s == want_s) | (got_s.isnan() & want_s.isnan())
    assert bool(same.all()), (name, sat.tolist(), got_s.tolist(), want_s.tolist())


# ---- 3. linear epilogue combinations ------------------------------------------------------------------------------------------
def linear_case(M, Nn, K):
    g = torch.Generator(device=DEV).manual_seed(M * 7 + Nn * 3 + K)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(Nn, K, device=DEV, generator=g)
    b = torch.randn(Nn, device=DEV, generator=g)
    r = torch.randn(M, Nn, device=DEV, generator=g)
    return x, w, b, r, x.double() @ w.double().T + b.double()


def under_both_tiles(option: str, run):
    """`run()` under option = 0 (the dispatcher's rule: a 128 x 128 kernel at these sizes) and = 8 (the 8-phase kernel and its
    batched `fetch` / `store_fetched` epilogue, where the shape allows it); options are read per dispatch."""
    outs = []
    try:
        for tile in (0, 8):
            N.set_option(option, tile)
            outs.append(run())
    finally:
        N.set_option(option, 0)
    return outs


# (321, 130, 64) is there beside the two ragged shapes because the fp32 8-phase kernel takes whole 128-byte rows only (K % 32 == 0)
@pytest.mark.parametrize("M,Nn,K", [(70, 33, 100), (321, 130, 40), (321, 130, 64)])
@pytest.mark.parametrize("name", list(ACTS))
def test_linear_activation_with_residual(name, M, Nn, K):
    """`LinearEpi<ACT, true, false, false>` of sl_linear: act(x w^T + b) + residual, out of place and with residual = out."""
    code, f64, _ = ACTS[name]
    x, w, b, r, z = linear_case(M, Nn, K)
    want = f64(z) + r.double()

    def run():
        poison(M * Nn)
        out = N.linear(x, w, b, act=code, residual=r)
        inplace = r.clone()
        N.linear(x, w, b, act=code, residual=inplace, out=inplace)
        return out, inplace

    (o0, i0), (o8, i8) = under_both_tiles("f32_tile", run)
    assert torch.equal(o0, o8) and torch.equal(i0, i8), "tile variants differ"
    assert torch.equal(o0, i0), "in place differs from out of place"
    e = rel_err(o0, want)
    print(f"linear {name} + residual ({M}, {Nn}, {K}): rel_err {e:.3g}")
    assert e < 1e-5


def linear3_tolerance(name, z, K):
    """test_linear3_random_shapes_against_fp64's bound on the product (8 2^-16 sqrt(K) + 1e-6 for unit-variance operands),
    carried through an activation of slope < 1.2, plus the pointwise bound of the activation itself"""
    return 1.2 * (8 * 2.0 ** -16 * K ** 0.5 + 1e-6) + activation_bound(name, z)


@pytest.mark.parametrize("M,Nn,K", [(70, 33, 100), (321, 130, 40)])
@pytest.mark.parametrize("name", list(ACTS))
def test_linear3_activation_with_residual(name, M, Nn, K):
    """`LinearEpi<ACT, true, false, false>` of sl_linear_bf16x3 through the 128 x 128 and the 8-phase kernel."""
    code, f64, _ = ACTS[name]
    x, w, b, r, z = linear_case(M, Nn, K)
    want = f64(z) + r.double()
    sx, sw = N.Split.of(x), N.Split.of(w)

    def run():
        poison(M * Nn)
        out = N.linear3(sx, sw, b, act=code, residual=r)
        inplace = r.clone()
        N.linear3(sx, sw, b, act=code, residual=inplace, out=inplace)
        return out, inplace

    (o0, i0), (o8, i8) = under_both_tiles("g3_tile", run)
    assert torch.equal(o0, o8) and torch.equal(i0, i8), "tile variants differ"
    assert torch.equal(o0, i0), "in place differs from out of place"
    err = (o0.double() - want).abs()
    tol = linear3_tolerance(name, z, K) + 2.0 ** -24 * want.abs()  # the residual add rounds once more
    print(f"linear3 {name} + residual ({M}, {Nn}, {K}): max |got - float64| = {err.max().item():.3g}, min bound {tol.min().item():.3g}")
    assert bool((err < tol).all()), (err - tol).max().item()


@pytest.mark.parametrize("M,Nn,K", [(70, 33, 100), (321, 130, 40)])
@pytest.mark.parametrize("name", ["gelu_tanh", "quickgelu"])
def test_linear3_activation_to_split_output(name, M, Nn, K):
    """`LinearEpi<2 or 3, false, false, true>`: the activated result leaves as a split (hi, lo) matrix."""
    code, f64, _ = ACTS[name]
    x, w, b, _, z = linear_case(M, Nn, K)
    want = f64(z)
    sx, sw = N.Split.of(x), N.Split.of(w)

    def run():
        return N.linear3(sx, sw, b, act=code, out_split=N.Split(M, Nn, DEV))

    s0, s8 = under_both_tiles("g3_tile", run)
    assert torch.equal(s0.buf, s8.buf), "tile variants differ"
    err = ((s0.hi.float() + s0.lo.float()).double() - want).abs()
    tol = linear3_tolerance(name, z, K) + 2.0 ** -16 * want.abs().max().item()  # hi + lo carries a value to 2^-16 (test_primitives_against_torch)
    print(f"linear3 {name} -> split ({M}, {Nn}, {K}): max |got - float64| = {err.max().item():.3g}, min bound {tol.min().item():.3g}")
    assert bool((err < tol).all()), (err - tol).max().item()
    if s0.kp != Nn:  # the padding of a split output stays zero (the next GEMM reads it)
        assert s0.buf.view(M, s0.kp // 32, 2, 32)[:, -1, :, Nn % 32:].float().abs().max().item() == 0.0


# ---- 5. LayerNorm paths -------------------------------------------------------------------------------------------------------
def layernorm64(x, gam, bet):
    return torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), gam.double(), bet.double(), 1e-5)


def ln_inputs(rows, cols, seed, row_stride=None, offset=0):
    """(rows, cols) view of row- and column-dependent values, with the given row stride, `offset` floats past an aligned base"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ld = row_stride or cols
    buf = torch.randn(rows * ld + 4, device=DEV, generator=g)
    x = buf[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    r = torch.arange(rows, device=DEV, dtype=torch.float32)[:, None]
    x.mul_(1.0 + (r % 13)).add_(r % 7 - 3.0)
    gam, bet = torch.randn(cols, device=DEV, generator=g), torch.randn(cols, device=DEV, generator=g)
    return x, gam, bet, ld


def check_layernorm(x, gam, bet, ld):
    rows, cols = x.shape
    want = layernorm64(x, gam, bet)
    poison(rows * cols)
    got = N.layernorm(x, gam, bet, 1e-5, rows=rows, x_row_stride=ld)
    sp = N.layernorm(x, gam, bet, 1e-5, rows=rows, x_row_stride=ld, out_split=N.Split(rows, cols, DEV))
    e, es = rel_err(got, want), rel_err(sp.hi.float() + sp.lo.float(), want)
    print(f"layernorm rows={rows} cols={cols} stride={ld} base%16={x.data_ptr() % 16}: rel_err {e:.3g}, split {es:.3g}")
    assert e < 1e-5 and es < 1e-5
    return got, sp


@pytest.mark.parametrize("cols", [2052, 4096])
def test_layernorm_three_pass_kernel_past_2048_columns(cols):
    check_layernorm(*ln_inputs(9, cols, seed=cols))


def test_layernorm_rows_that_fail_the_16_byte_rule():
    """cols = 768 would take the register kernel; a row stride of 769 floats, or a base one float past a 16-byte boundary, sends
    it to the three-pass kernel (J = 0) instead: same values as the aligned call within the bound."""
    x, gam, bet, ld = ln_inputs(9, 768, seed=1, row_stride=769)
    assert x.stride(0) == 769 and x.data_ptr() % 16 == 0
    check_layernorm(x, gam, bet, ld)
    x, gam, bet, ld = ln_inputs(9, 768, seed=2, offset=1)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    got, _ = check_layernorm(x, gam, bet, ld)
    assert rel_err(N.layernorm(x.clone(), gam, bet, 1e-5), got) < 1e-5


@pytest.mark.parametrize("cols", [8, 1028])
def test_layernorm_grid_stride_walk(cols):
    """rows = 32 CUs + 5: the waves of the first five workgroups take a second row (J = 4 at 8 columns; J = 8 at 1028, where
    gamma / beta sit in LDS across rows).  Besides the float64 bound, every row equals the same row normalised without a walk,
    bit for bit: a stale gamma / beta or a skipped row that a max-norm bound would hide."""
    head = 32 * cus()
    rows = head + 5
    x, gam, bet, ld = ln_inputs(rows, cols, seed=cols)
    got, sp = check_layernorm(x, gam, bet, ld)
    first = N.layernorm(x[:head], gam, bet, 1e-5)
    first_sp = N.layernorm(x[:head], gam, bet, 1e-5, out_split=N.Split(head, cols, DEV))
    assert torch.equal(got[:head], first) and torch.equal(sp.buf[:head], first_sp.buf)
    for r in (0, head - 1, *range(head, rows)):
        alone = N.layernorm(x[r:r + 1], gam, bet, 1e-5)
        alone_sp = N.layernorm(x[r:r + 1], gam, bet, 1e-5, out_split=N.Split(1, cols, DEV))
        assert torch.equal(got[r:r + 1], alone) and torch.equal(sp.buf[r:r + 1], alone_sp.buf), r


# ---- 6. attention pool --------------------------------------------------------------------------------------------------------
def pool64(q, kv, B, T, H, hd):
    W = H * hd
    k = kv[:, :W].double().reshape(B, T, H, hd).permute(0, 2, 1, 3)
    v = kv[:, W:].double().reshape(B, T, H, hd).permute(0, 2, 1, 3)
    s = (q.double().reshape(B, H, 1, hd) @ k.transpose(-1, -2)) / math.sqrt(hd)
    return (torch.softmax(s, -1) @ v).reshape(B, W), s


@pytest.mark.parametrize("hd", [4, 128])
@pytest.mark.parametrize("T", [1, 64, 65])
def test_attention_pool_small(T, hd):
    """One key per lane at most (T <= 64), a lane with two keys (65), a single key; the smallest and the largest head."""
    B, H = 2, 3
    W = H * hd
    g = torch.Generator(device=DEV).manual_seed(T * 131 + hd)
    kv = torch.randn(B * T, 2 * W, device=DEV, generator=g)
    q = torch.randn(B, W, device=DEV, generator=g)
    want, _ = pool64(q, kv, B, T, H, hd)
    e = rel_err(N.attention_pool_q(q, kv, B, T, H, hd), want)
    want1, _ = pool64(q[:1].expand(B, W), kv, B, T, H, hd)
    e1 = rel_err(N.attention_pool(q[0].contiguous(), kv, B, T, H, hd), want1)
    print(f"attention_pool T={T} hd={hd}: rel_err per-image query {e:.3g}, shared query {e1:.3g}")
    assert e < 1e-5 and e1 < 1e-5


def test_attention_pool_logits_near_300():
    """Queries scaled until the largest |logit| is 300 (a CLIP-ResNet trunk's range): the double-accumulated score and the
    library exponentials of `attention_pool_kernel` exist for this."""
    B, T, H, hd = 2, 65, 3, 128
    W = H * hd
    g = torch.Generator(device=DEV).manual_seed(300)
    kv = torch.randn(B * T, 2 * W, device=DEV, generator=g)
    q = torch.randn(B, W, device=DEV, generator=g)
    _, s = pool64(q, kv, B, T, H, hd)
    q = (q * (300.0 / s.abs().max().item())).contiguous()
    want, s = pool64(q, kv, B, T, H, hd)
    assert 299.0 < s.abs().max().item() < 301.0 and s.min().item() < -100.0 and s.max().item() > 100.0
    e = rel_err(N.attention_pool_q(q, kv, B, T, H, hd), want)
    print(f"attention_pool logits in [{s.min().item():.0f}, {s.max().item():.0f}]: rel_err {e:.3g}")
    assert e < 1e-5
