"""K6 / K8 / K10: every operand-preparation branch of the cosine path against float64.

`cosine_matrix_nt` / `cosine_matrix_multi` (csrc/cosine.hip) prepare their operands on one of several bodies picked from the
width, the alignment and the layer count (`norm_split_rows_kernel`: registers, float4 loop, scalar; `row_inv_norm_kernel` +
`split_bf16_kernel` behind 32 layers; the fp32 GEMM's vectorised and scalar loads and its K tail), and the tile-variant tests
of test_gpu_parity.py compare GEMM kernels that all read the SAME prepared operands.  Each case below is the smallest shape
that reaches one of those bodies (or one grid-stride loop of the score kernels around them) and holds it to a float64
reference computed on the device from the same fp32 inputs.  The CU count is read from the device.

Input recipe `hard_rows(M, N, K, seed)`, used by every cosine case that does not say otherwise:
  * x ~ N(0, 1), (M, K);  y[j] = x[j % M] + 1e-3 N(0, 1), (N, K): near-parallel pairs on and off the diagonal, where the
    split-bf16 arithmetic is biased to one side (the dropped lo * lo terms all share a sign);
  * y[N - 1] = -x[(N - 1) % M] and y[1] = 3 x[1]: cosines within the bound of -1 and of 1;
  * x[2] keeps only its first K // 2 coordinates and y[3] only the others: disjoint supports, the cosine is exactly 0 in
    either arithmetic (K >= 2);
  * then every row of x and of y is scaled by its own 10 ** randint(-12, 12): rows up to 24 decades apart;
  * last x[M - 1] = 0 and y[0] = 0: their whole output row and column are exactly 0.
  So the last row of x (zero) and of y (the negated row) are special rows: the edge tiles, which clamp the rows past the
  matrix edge onto the last row, read them.  A special row that the shape has no room for is left out.

Bound on a cosine: 1e-5 absolute against float64 in both arithmetic modes, the bound the suite holds everywhere else.  A CPU
emulation of both arithmetics on this recipe (sequential fp32 sums; hi * hi + hi * lo + lo * hi on bf16 halves; K in {65, 2048,
2052, 4100, 8200}) stayed at or below 5.2e-6 (split-bf16) and 2.9e-6 (fp32).  Every case prints what it observed; on an MI355X
(256 CUs) the largest over all cases were 5.6e-6 (split-bf16: `cosine_nt(x, x)` at K = 65) and 3.1e-6 (fp32: K = 4100), the
aligned-against-unaligned gap 1.46e-6 (split-bf16, K = 68; 0 elsewhere), the row-wise branch 2.5e-7."""
import contextlib

import numpy as np
import pytest
import torch

import oracle
from semanticlens_amd import _native as N
from semanticlens_amd import scores

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-5
MODES = ("bf16x3", "f32")
WORST = {m: 0.0 for m in MODES}  # the largest cosine error seen so far per mode, printed with every case


def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def poison(numel: int, dtype=torch.float32):
    """Leave a NaN-filled block of this size in the allocator's cache (test_gpu_instances.py): an output element that a kernel
    skips then reads NaN instead of an earlier call's (right) answer."""
    torch.full((max(int(numel), 1),), float("nan"), dtype=dtype, device=DEV)


@contextlib.contextmanager
def gemm_mode(mode):
    N.set_gemm_mode(mode)
    try:
        yield
    finally:
        N.set_gemm_mode(None)


def one_float_past(t: torch.Tensor) -> torch.Tensor:
    """A contiguous copy of `t` that starts one float past a 16-byte boundary (test_clarity_slab_one_float_past_a_16_byte_boundary)."""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---- references (float64, from the same fp32 inputs) ---------------------------------------------------------------------------
def unit64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def cos64(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """normalize(x) @ normalize(y).T in float64, F.normalize's eps = 1e-12 on each norm"""
    return unit64(x) @ unit64(y).T


def rowwise64(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """F.cosine_similarity(x, y, dim=-1) as `rowwise_cosine_kernel` states it: eps = 1e-8 on each norm"""
    x, y = x.double(), y.double()
    return (x * y).sum(-1) / (x.norm(dim=-1).clamp_min(1e-8) * y.norm(dim=-1).clamp_min(1e-8))


def redundancy64(V: torch.Tensor) -> torch.Tensor:
    """mean_i max_j (cos - 2 I) over the last two axes"""
    u = unit64(V)
    s = u @ u.transpose(-1, -2)
    s.diagonal(dim1=-2, dim2=-1).sub_(2.0)
    return s.max(-1).values.mean(-1)


def template_mean64(E: torch.Tensor, E0: torch.Tensor, Q: int) -> torch.Tensor:
    T, D = E0.shape
    return (E.double().view(Q, T, D) - E0.double()).mean(1)


def test_float64_restatements_match_the_oracle():
    rng = np.random.RandomState(7)
    x = (rng.randn(9, 33) * 10.0 ** rng.randint(-3, 4, (9, 1))).astype(np.float32)
    y = (rng.randn(5, 33) * 10.0 ** rng.randint(-3, 4, (5, 1))).astype(np.float32)
    x[4] = 0.0
    tx, ty = torch.from_numpy(x), torch.from_numpy(y)
    np.testing.assert_allclose(cos64(tx, ty).numpy(), oracle.similarity(x, y), rtol=0, atol=1e-6)
    y9 = (x + 0.1 * rng.randn(9, 33)).astype(np.float32)
    np.testing.assert_allclose(rowwise64(tx, torch.from_numpy(y9)).numpy(), oracle.similarity(x, y9), rtol=0, atol=1e-6)
    y33 = rng.randn(33, 6).astype(np.float32)  # branch 1: no transpose
    np.testing.assert_allclose((unit64(tx) @ unit64(torch.from_numpy(y33))).numpy(), oracle.similarity(x, y33), rtol=0, atol=1e-6)
    V = rng.randn(2, 7, 33).astype(np.float32)
    V[1, 3] = V[1, 5]
    V[0, 2] = 0.0
    np.testing.assert_allclose(redundancy64(torch.from_numpy(V)).numpy(), oracle.redundancy(V), rtol=0, atol=1e-6)
    E, E0 = rng.randn(3 * 4, 5).astype(np.float32), rng.randn(4, 5).astype(np.float32)
    np.testing.assert_allclose(template_mean64(torch.from_numpy(E), torch.from_numpy(E0), 3).numpy(), oracle.template_mean(E, E0, 3),
                               rtol=0, atol=1e-6)


# ---- the input recipe ----------------------------------------------------------------------------------------------------------
def decades(n: int, g: torch.Generator) -> torch.Tensor:
    """(n, 1) factors 10 ** randint(-12, 12), both ends included"""
    return 10.0 ** torch.randint(-12, 13, (n, 1), device=DEV, generator=g).float()


def hard_rows(M: int, Nn: int, K: int, seed: int):
    """The recipe of the module docstring: x (M, K), y (Nn, K) and the places of the special rows."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(M, K, device=DEV, generator=g)
    y = x[torch.arange(Nn, device=DEV) % M] + 1e-3 * torch.randn(Nn, K, device=DEV, generator=g)
    sp = {}
    zx, zy = (M - 1 if M >= 2 else None), (0 if Nn >= 2 else None)
    if Nn >= 3 and (Nn - 1) % M != zx:
        y[Nn - 1] = -x[(Nn - 1) % M]
        sp["neg"] = ((Nn - 1) % M, Nn - 1)
    if Nn >= 4 and 1 % M != zx:
        y[1] = 3.0 * x[1 % M]
        sp["pos"] = (1 % M, 1)
    if K >= 2 and M >= 4 and Nn >= 5:
        x[2, K // 2:] = 0.0
        y[3, :K // 2] = 0.0
        sp["disjoint"] = (2, 3)
    x *= decades(M, g)
    y *= decades(Nn, g)
    if zx is not None:
        x[zx] = 0.0
    if zy is not None:
        y[zy] = 0.0
    sp["zero_x"], sp["zero_y"] = zx, zy
    return x, y, sp


def assert_cosine(got: torch.Tensor, x: torch.Tensor, y: torch.Tensor, sp: dict, mode: str, tag) -> float:
    """`got` against cos64(x, y) within BOUND, and the special rows of `hard_rows`; a NaN (a skipped element) fails."""
    want = cos64(x, y)
    assert got.shape == want.shape and got.dtype == torch.float32, tag
    err = (got.double() - want).abs().max().item()
    WORST[mode] = max(WORST[mode], err) if err == err else float("nan")
    print(f"cosine {tag} mode={mode}: max |got - float64| = {err:.3g}  (largest so far: bf16x3 {WORST['bf16x3']:.3g}, f32 {WORST['f32']:.3g})")
    assert err <= BOUND, (tag, mode, err)
    if sp.get("zero_x") is not None:
        assert got[sp["zero_x"]].abs().max().item() == 0.0, (tag, mode, "zero row of x")
    if sp.get("zero_y") is not None:
        assert got[:, sp["zero_y"]].abs().max().item() == 0.0, (tag, mode, "zero row of y")
    if "disjoint" in sp:
        assert got[sp["disjoint"]].item() == 0.0, (tag, mode, "disjoint supports")
    if "neg" in sp:
        assert abs(got[sp["neg"]].item() + 1.0) <= BOUND, (tag, mode, "-x row")
    if "pos" in sp:
        assert abs(got[sp["pos"]].item() - 1.0) <= BOUND, (tag, mode, "3 x row")
    return err


# ---- A. operand preparation and K tails ----------------------------------------------------------------------------------------
M_A, N_A = 130, 67  # neither a tile multiple: one 128-row tile and a clamped remainder of x, one partial tile of y


@pytest.mark.parametrize("K", [64, 65, 68, 99, 2044, 2048, 2052, 4100])
@pytest.mark.parametrize("mode", MODES)
def test_similarity_widths_of_every_preparation_body(mode, K):
    """bf16x3, `norm_split_rows_kernel`: 64 / 68 / 2044 / 2048 the register body (smallest width, padded last line, all eight
    pieces full), 2052 / 4100 the float4 loop, 65 / 99 the scalar body.  f32: `row_inv_norm_kernel`, then `gemm_nt_kernel<true>`
    (K % 4 == 0; 68 / 2044 / 2052 / 4100 with a K tail) or `<false>` (65, 99: full tiles and a tail)."""
    x, y, sp = hard_rows(M_A, N_A, K, seed=K)
    poison(M_A * N_A)
    with gemm_mode(mode):
        got = N.similarity(x, y)
    assert_cosine(got, x, y, sp, mode, (M_A, N_A, K))


@pytest.mark.parametrize("K", [1, 31, 32, 33, 36, 73])
def test_fp32_gemm_k_tails(K):
    """The fp32 GEMM alone (below K = 64 either mode takes it; f32 is set all the same): 1 / 31 `Scalar128` with no full k-tile,
    32 exactly one full tile of `Vec128`, 33 `Scalar128` with one full tile and a tail of one, 36 the `Vec128` tail, 73
    `Scalar128` with two full tiles and a tail."""
    x, y, sp = hard_rows(M_A, N_A, K, seed=100 + K)
    poison(M_A * N_A)
    with gemm_mode("f32"):
        got = N.similarity(x, y)
    assert_cosine(got, x, y, sp, "f32", (M_A, N_A, K))


ALIGN_GAP = 2e-6  # aligned against unaligned: the two bodies sum the squares in different orders, a last-bit step of the inverse norm


@pytest.mark.parametrize("which", ["x", "y", "both"])
@pytest.mark.parametrize("K", [68, 2052])
@pytest.mark.parametrize("mode", MODES)
def test_similarity_operand_one_float_past_a_16_byte_boundary(mode, K, which):
    """K % 4 == 0 with an unaligned base: bf16x3 leaves the register body (68) / the float4 loop (2052) for the scalar body, f32
    leaves `Vec128` for `Scalar128`."""
    x, y, sp = hard_rows(M_A, N_A, K, seed=200 + K)
    xo = one_float_past(x) if which in ("x", "both") else x
    yo = one_float_past(y) if which in ("y", "both") else y
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    with gemm_mode(mode):
        poison(M_A * N_A)
        aligned = N.similarity(x, y)
        poison(M_A * N_A)
        off = N.similarity(xo, yo)
    assert_cosine(aligned, x, y, sp, mode, (K, "aligned"))
    assert_cosine(off, x, y, sp, mode, (K, which, "one float past"))
    gap = (aligned - off).abs().max().item()
    print(f"aligned against unaligned {which} K={K} mode={mode}: max gap {gap:.3g}")
    assert gap <= ALIGN_GAP, (mode, K, which, gap)


@pytest.mark.parametrize("K", [65, 2052])
@pytest.mark.parametrize("mode", MODES)
def test_cosine_nt_same_operand(mode, K):
    """`cosine_matrix_nt` with B == A: one preparation launch, the GEMM reads one operand on both sides."""
    x, _, _ = hard_rows(M_A, N_A, K, seed=300 + K)
    out = torch.full((M_A, M_A), float("nan"), device=DEV)
    with gemm_mode(mode):
        N.cosine_nt(x, x, out)
    want = cos64(x, x)
    err = (out.double() - want).abs().max().item()
    WORST[mode] = max(WORST[mode], err) if err == err else float("nan")
    print(f"cosine_nt(x, x) K={K} mode={mode}: max |got - float64| = {err:.3g}")
    assert err <= BOUND, (mode, K, err)
    d = out.diagonal()
    assert (d[:M_A - 1] - 1.0).abs().max().item() <= BOUND and d[M_A - 1].item() == 0.0
    assert out[M_A - 1].abs().max().item() == 0.0 and out[:, M_A - 1].abs().max().item() == 0.0


@pytest.mark.parametrize("K", [65, 68, 2052])
def test_split_padding_is_written_on_every_call(K):
    """bf16x3: the split operands are padded to a multiple of 32 columns (96, 96, 2080) and the GEMM reads the padding.  The
    workspace holds NaN bytes before each of two calls: a padding element that a preparation body leaves unwritten would be a
    NaN in every cosine of its row; the two results are bit-equal."""
    x, y, sp = hard_rows(M_A, N_A, K, seed=400 + K)
    ws = torch.empty(int(N.lib().sl_cosine_nt_ws_bytes(M_A, N_A, K)), dtype=torch.uint8, device=DEV)
    outs = []
    with gemm_mode("bf16x3"):
        for _ in range(2):
            ws.fill_(0xFF)  # bf16 0xFFFF and fp32 0xFFFFFFFF are NaNs
            out = torch.full((M_A, N_A), float("nan"), device=DEV)
            outs.append(N.cosine_nt(x, y, out, ws=ws))
    assert_cosine(outs[0], x, y, sp, "bf16x3", (K, "poisoned workspace"))
    assert torch.equal(outs[0], outs[1])


# ---- B. NaN isolation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rx,ry", [(129, 3), (0, 66)])
@pytest.mark.parametrize("mode", MODES)
def test_a_nan_row_stays_in_its_own_row_and_column(mode, rx, ry):
    """Gaussian rows (routing, not accuracy).  (129, 3): the NaN sits in the last row of x, the row that the edge tile's clamped
    loads repeat for rows 130..255; (0, 66): in the first row of x and the last of y."""
    g = torch.Generator(device=DEV).manual_seed(500 + rx)
    x, y = torch.randn(M_A, 68, device=DEV, generator=g), torch.randn(N_A, 68, device=DEV, generator=g)
    want = cos64(x, y)
    x[rx, 5] = float("nan")
    y[ry, 7] = float("nan")
    poison(M_A * N_A)
    with gemm_mode(mode):
        got = N.similarity(x, y)
    hit = torch.zeros(M_A, N_A, dtype=torch.bool, device=DEV)
    hit[rx] = True
    hit[:, ry] = True
    assert bool(got[hit].isnan().all()), (mode, "a cosine of the NaN row or column is a number")
    assert bool(torch.isfinite(got[~hit]).all()), (mode, "NaN outside its row and column")
    err = (got.double() - want)[~hit].abs().max().item()
    assert err <= BOUND, (mode, err)


# ---- C. similarity_multi -------------------------------------------------------------------------------------------------------
LAYERS = (3, 1, 70, 5, 0, 2)


def check_multi(mode, Q, K, sizes, seed, unaligned=(), bitwise=True):
    x, y, sp = hard_rows(Q, sum(sizes), K, seed)
    ys = [part.clone() for part in y.split(list(sizes))]
    for i in unaligned:
        ys[i] = one_float_past(ys[i])
    assert all(t.data_ptr() % 16 == (4 if i in unaligned else 0) for i, t in enumerate(ys) if t.numel())
    with gemm_mode(mode):
        for s in sizes:
            poison(Q * s)
        outs = N.similarity_multi(x, ys)
        assert outs is not None and len(outs) == len(ys)
        for i, (o, t) in enumerate(zip(outs, ys)):
            assert o.shape == (Q, t.shape[0]), i
            if bitwise and t.shape[0]:
                assert torch.equal(o, N.similarity(x, t)), (mode, i, "fused differs from layer by layer")
    assert_cosine(torch.cat(outs, 1), x, y, sp, mode, (Q, K, f"{len(sizes)} layers"))


@pytest.mark.parametrize("K,extra,unaligned", [(64, 2, ()), (64, 3, ()), (99, 2, ()), (68, 2, (2, 5)), (68, 3, (2, 5))])
@pytest.mark.parametrize("mode", MODES)
def test_multi_layer_cursor_jumps_whole_layers_in_one_grid_stride(mode, K, extra, unaligned):
    """Q = 32 CUs + 2 or + 3 query rows against layers of (3, 1, 70, 5, 0, 2) rows.  bf16x3, one launch for the query and all
    layers (`norm_split_rows_kernel` over Q + 81 rows with 32 CUs waves): the second row of wave w is row 32 CUs + w, which for
    w = 2.. lies 1 to 5 layers past the query the wave started in.  One launch needs the query's split rows to end on a
    256-byte boundary: 128 Q (Kp / 32) bytes, so always at K = 64 (Kp = 64) and K = 99 (Kp = 128), and at K = 68 (Kp = 96) for
    an even Q only — (68, 3) is the two-launch route, whose layer launch walks the same cursor without a stride.  K = 99 is the
    scalar body under the moving cursor, K = 68 with layers 2 and 5 one float past a 16-byte boundary mixes the register and the
    scalar body in one launch.  f32: the per-layer loop.  Fused results equal `similarity` layer by layer, bit for bit."""
    check_multi(mode, 32 * cus() + extra, K, LAYERS, seed=600 + K + extra, unaligned=unaligned)


@pytest.mark.parametrize("mode", MODES)
def test_multi_layer_cursor_of_the_gathering_fp32_route(mode):
    """f32: the layers are gathered into one fp32 operand for the 256 x 256 kernel when all of them together fill half the chip
    and none does alone (`norm_rows_kernel<true>`: the same cursor).  34 query rows; a first layer of 32 CUs - 2 rows, then
    (3, 1, 70, 5, 0, 2) and a last layer that takes the sum just past (CUs / 2 - 1) x 256 rows: the last two waves' second rows lie
    six layers further.  bf16x3 walks the same layers behind the query in one launch."""
    n = cus()
    first = 32 * n - 2
    last = ((n + 1) // 2 - 1) * 256 + 9 - first - sum(LAYERS)
    assert 0 < last <= ((n + 1) // 2 - 1) * 256
    check_multi(mode, 34, 64, (first, *LAYERS, last), seed=650)


@pytest.mark.parametrize("L", [32, 33])
@pytest.mark.parametrize("mode", MODES)
def test_multi_32_and_33_layers(mode, L):
    """32 layers: the query does not fit as a 33rd row source, two preparation launches, still bit-equal to layer by layer.
    33 layers: the unfused route, whose inverse norms come from `row_inv_norm_kernel` and whose split operands from
    `split_bf16_kernel` with a row scale (float64 bound only: the inverse norm may differ in the last bit)."""
    check_multi(mode, 34, 64, tuple(1 + (i % 5) for i in range(L)), seed=700 + L, bitwise=(L == 32))


# ---- D. branch 0: row-wise cosine ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1, 63, 65, 130])
def test_rowwise_cosine_grid_stride(cols):
    """x.shape == y.shape: one wave per row, 32 CUs waves, rows = 32 CUs + 5 so that the waves of the first two workgroups take a
    second row.  Paired rows (y = x + 1e-3 noise, one sign flip, one 3 x, rows scaled over 24 decades, zero rows).  Bound 1e-6:
    one fp32 dot product and two norms of at most 130 terms."""
    rows = 32 * cus() + 5
    g = torch.Generator(device=DEV).manual_seed(800 + cols)
    x = torch.randn(rows, cols, device=DEV, generator=g)
    y = x + 1e-3 * torch.randn(rows, cols, device=DEV, generator=g)
    y[1] = -x[1]
    y[rows - 2] = 3.0 * x[rows - 2]
    sx, sy = decades(rows, g), decades(rows, g)
    sx[1], sy[1], sx[rows - 2], sy[rows - 2] = 1e-3, 1e9, 1e7, 1e-2  # the +-1 rows keep their norms clear of eps
    x *= sx
    y *= sy
    x[rows - 1] = 0.0  # one side zero, in the grid-stride tail
    x[2] = 0.0
    y[2] = 0.0
    want = rowwise64(x, y)
    assert abs(want[1].item() + 1.0) <= 1e-9 and abs(want[rows - 2].item() - 1.0) <= 1e-9  # the construction, not the kernel
    poison(rows)
    got = N.similarity(x, y)
    assert got.shape == (rows,) and got.dtype == torch.float32
    err = (got.double() - want).abs().max().item()
    print(f"row-wise cosine rows={rows} cols={cols}: max |got - float64| = {err:.3g}")
    assert err <= 1e-6, (cols, err)
    assert got[rows - 1].item() == 0.0 and got[2].item() == 0.0
    assert abs(got[1].item() + 1.0) <= 1e-6 and abs(got[rows - 2].item() - 1.0) <= 1e-6


# ---- E. branch 1: no transpose -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xs,ys", [((4100, 3), (3, 4100)), ((2, 4097), (4097, 4100))])
def test_no_transpose_branch_grid_strides(xs, ys):
    """x.shape[1] == y.shape[0]: normalize(x) @ normalize(y).  (4100, 3) x (3, 4100) has 16 810 000 outputs, more than the 65 535 x
    256 threads of `gemm_nn_kernel`'s grid; (2, 4097) x (4097, 4100) has 16 797 700 elements of y, more than `scale_rows_kernel`'s.
    Gaussian rows scaled over 24 decades, one zero row on each side."""
    g = torch.Generator(device=DEV).manual_seed(900 + xs[0])
    x = torch.randn(*xs, device=DEV, generator=g) * decades(xs[0], g)
    y = torch.randn(*ys, device=DEV, generator=g) * decades(ys[0], g)
    x[xs[0] - 1] = 0.0
    y[1] = 0.0
    want = unit64(x) @ unit64(y)
    poison(xs[0] * ys[1])
    got = N.similarity(x, y)
    assert got.shape == want.shape and got.dtype == torch.float32
    err = (got.double() - want).abs().max().item()
    print(f"no-transpose branch {xs} x {ys}: max |got - float64| = {err:.3g}")
    assert err <= BOUND, (xs, ys, err)
    assert got[xs[0] - 1].abs().max().item() == 0.0


# ---- F. K8: redundancy ---------------------------------------------------------------------------------------------------------
def assert_redundancy(V: torch.Tensor, mode: str, tag) -> torch.Tensor:
    want = redundancy64(V)
    C, D = V.shape[-2:]
    poison(int(N.lib().sl_redundancy_ws_bytes(1, C, D)) // 4)
    poison(want.numel())
    with gemm_mode(mode):
        got = N.redundancy(V)
    assert got.shape == want.shape and got.dtype == torch.float32, tag
    err = (got.double() - want).abs().max().item()
    print(f"redundancy {tag} mode={mode}: max |got - float64| = {err:.3g}")
    assert err <= BOUND, (tag, mode, err)
    return got


@pytest.mark.parametrize("shape", [(3, 67, 65), (3, 66, 68)])
@pytest.mark.parametrize("mode", MODES)
def test_redundancy_slabs(mode, shape):
    """(3, 67, 65): slabs 1 and 2 start 67 x 65 floats apart, one and two floats past a 16-byte boundary, and take the scalar
    bodies; (3, 66, 68): aligned slabs, partial tiles.  Rows scaled over 24 decades, one zero row, one duplicated row per slab;
    the last slab holds 33 pairs of equal rows (and, at 67 rows, the zero row), so every row maximum there is a cosine of 1."""
    Bt, C, D = shape
    g = torch.Generator(device=DEV).manual_seed(C * D)
    V = torch.randn(Bt, C, D, device=DEV, generator=g)
    V[:, 5] = V[:, 9]
    V[Bt - 1, 33:66] = V[Bt - 1, :33]
    V *= decades(Bt * C, g).view(Bt, C, 1)
    V[:, C - 1] = 0.0
    assert V.data_ptr() % 16 == 0 and (C * D % 4 == 0 or V[1].data_ptr() % 16 != 0)
    got = assert_redundancy(V, mode, shape)
    if C == 67:  # 66 rows at a maximum of 1, the zero row at 0 (at C = 66 the zero row took the place of one of a pair)
        assert abs(got[Bt - 1].item() - 66.0 / 67.0) <= BOUND


@pytest.mark.parametrize("D", [7, 65])
@pytest.mark.parametrize("mode", MODES)
def test_redundancy_one_and_two_components(mode, D):
    """C = 1: the only entry is the diagonal, cos(v, v) - 2: exactly -1 for a row with one non-zero coordinate (its cosine with
    itself is exact in either arithmetic), within the bound of -1 for any row.  C = 2: the cosine of the two rows; two equal rows
    give a row maximum within the bound of 1."""
    g = torch.Generator(device=DEV).manual_seed(D)
    axis = torch.zeros(1, D, device=DEV)
    axis[0, D // 2] = -8.0
    assert assert_redundancy(axis, mode, (1, D, "axis")).item() == -1.0
    v = torch.randn(4, 1, D, device=DEV, generator=g) * decades(4, g).view(4, 1, 1)
    assert (assert_redundancy(v, mode, (4, 1, D)) + 1.0).abs().max().item() <= BOUND
    pair = torch.randn(3, 2, D, device=DEV, generator=g) * decades(6, g).view(3, 2, 1)
    pair[1, 1] = pair[1, 0]
    got = assert_redundancy(pair, mode, (3, 2, D))
    assert abs(got[1].item() - 1.0) <= BOUND


@pytest.mark.parametrize("mode", MODES)
def test_redundancy_rowmax_grid_stride(mode):
    """C = 32 CUs + 5 rows of 64: the waves of `rowmax_offdiag_kernel`'s first two workgroups take a second row.  Each of the last
    five rows is a near-copy of an earlier row (row maximum near 1 where a Gaussian row's is near 0.5): a dropped row moves the
    mean by about 0.5 / C = 6e-5 at 256 CUs, six times the bound."""
    C = 32 * cus() + 5
    g = torch.Generator(device=DEV).manual_seed(64)
    V = torch.randn(C, 64, device=DEV, generator=g)
    for i in range(5):
        V[C - 5 + i] = 2.0 * V[7 * i + 1] + 1e-3 * torch.randn(64, device=DEV, generator=g)
    assert_redundancy(V, mode, (C, 64))


# ---- G. K10: template mean -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,T,D", [(3, 1, 5), (7, 80, 33), (8200, 2, 2052)])
def test_template_mean(Q, T, D):
    """out[q] = mean_t (E[q T + t] - E0[t]).  (8200, 2, 2052): Q D = 16 826 400 outputs, more than the 65 535 x 256 threads of the
    grid.  Column 0 of E is E0's column 0 times 1 + 1e-6 N(0, 1): the differences cancel to about 1e-6 of the operands.  Bound
    (T + 5) 2^-24 max(|E|, |E0|): T rounded differences, T partial sums of magnitude at most 2 M t (their rounding, divided by
    T, is at most M T 2^-24), one division."""
    g = torch.Generator(device=DEV).manual_seed(Q + T + D)
    E0 = torch.randn(T, D, device=DEV, generator=g) * 3.0
    E = torch.randn(Q * T, D, device=DEV, generator=g) * 3.0
    E[:, 0] = E0[:, 0].repeat(Q) * (1.0 + 1e-6 * torch.randn(Q * T, device=DEV, generator=g))
    want = template_mean64(E, E0, Q)
    poison(Q * D)
    got = N.template_mean(E, E0, Q)
    assert got.shape == (Q, D) and got.dtype == torch.float32
    err = (got.double() - want).abs().max().item()
    bound = (T + 5) * 2.0 ** -24 * max(E.abs().max().item(), E0.abs().max().item())
    print(f"template_mean ({Q}, {T}, {D}): max |got - float64| = {err:.3g} (bound {bound:.3g}); cancelling column "
          f"{(got[:, 0].double() - want[:, 0]).abs().max().item():.3g} of values up to {want[:, 0].abs().max().item():.3g}")
    assert err <= bound, (Q, T, D, err, bound)


# ---- H. empty operands ---------------------------------------------------------------------------------------------------------
EMPTY_SHAPES = [(a, b) for a in (0, 3, 5) for b in (0, 3, 5)]


@pytest.mark.parametrize("device", ["cuda:0", "cpu"])
def test_similarity_score_of_empty_operands_is_torchs(device):
    """Every pair of shapes over {0, 3, 5}^2 x {0, 3, 5}^2 with a zero in it: `similarity_score` returns what the reference's
    torch expressions return on the host (`oracle.similarity_torch`) — shape, dtype, device and values: an empty result, or zeros
    where the contraction is over nothing — or raises the reference's ValueError where no branch accepts the shapes."""
    seen = set()
    for xs in EMPTY_SHAPES:
        for ys in EMPTY_SHAPES:
            if 0 not in xs + ys:
                continue
            x, y = torch.randn(*xs), torch.randn(*ys)
            try:
                want = oracle.similarity_torch(x, y)
            except ValueError:
                with pytest.raises(ValueError, match="same shape"):
                    scores.similarity_score(x.to(device), y.to(device))
                continue
            poison(max(want.numel(), 1))
            got = scores.similarity_score(x.to(device), y.to(device))
            assert got.shape == want.shape and got.dtype == want.dtype and got.device == torch.device(device), (xs, ys)
            assert torch.equal(got.cpu(), want), (xs, ys, got)
            branch = 0 if xs == ys else (1 if xs[1] == ys[0] else 2)
            seen.add((branch, want.numel() == 0))
    assert seen == {(b, e) for b in (0, 1, 2) for e in (False, True)}  # all three branches, empty and all-zero results
