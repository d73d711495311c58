"""K13 and K14 at the edges of their tiling (DESIGN.md §K13 "Edge geometries", §K14 "Upsample ratios"): one row per
horizontal LDS tile, the widest accepted plane, kernel_size 255 and 1, vertical tiles that start below row 0, planes wider
than the workgroup, one-column strips, long channel sums, non-integer and downsampling bilinear ratios, the (B, C) layer
form, out-of-range pairs, and sl_condition_init with more than one element per thread.  The checkers are those of
test_gpu_render.py plus a separable float64 blur; every threshold is derived in the docstring of the test that uses it and
every measured error is printed (run with -s), never asserted against itself."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from semanticlens_amd import _native as N
from test_gpu_render import _condition_cpu, blur_cpu, gaussian_taps, make_heats, norm_cpu, run_k13, square_box
from test_gpu_render import test_pixels_match_the_checker_within_one_lsb as pixels_match_the_checker  # render_checker, imgify, pillow_stroke

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP = 2.0 ** -24  # the unit roundoff of fp32

# H, W, kernel_size, Cin: what each row reaches is tabulated in DESIGN.md §K13
GEOMETRIES = [(5, 8200, 3, 1), (2, 16382, 3, 1), (131, 130, 255, 3), (128, 128, 255, 1), (300, 65, 3, 67), (257, 64, 1, 1),
              (40, 1100, 31, 3)]


def tiling(H, W, k):
    """(r, output rows per vertical tile, rows per horizontal tile) of blur_plane."""
    r = k // 2
    return r, 256 - 2 * r, 16384 // (W + 2 * r)


def blur_cpu_sep(heat, k):
    """blur_cpu as two float64 passes, 1 x k then k x 1, with the fp32 taps cast to double: the same sum in another
    order, fast enough at k = 255."""
    g = gaussian_taps(k).double()
    r = k // 2
    p = F.pad(heat.double()[:, None], (r, r, r, r), mode="reflect")
    return F.conv2d(F.conv2d(p, g[None, None, None, :]), g[None, None, :, None])[:, 0]


def full_box(H, W):
    return square_box(np.full((H, W), np.nan, np.float32), 0.01)  # nothing exceeds crop_th: the full image, made square


def check_boxes(heat, want, box, crop_th, H, W):
    """The existing rule: the box is square_box of the GPU's own heat exactly, and the reference's box wherever moving
    crop_th by 1e-5 cannot move it; at least half of the images are compared the second way."""
    compared = 0
    for i in range(heat.shape[0]):
        assert square_box(heat[i].numpy(), crop_th) == tuple(box[i]), i
        w = want[i].numpy()
        if square_box(w, crop_th - 1e-5) == square_box(w, crop_th + 1e-5):
            assert square_box(w, crop_th) == tuple(box[i]), i
            compared += 1
    assert 2 * compared >= heat.shape[0], compared


def test_separable_checker_equals_the_2d_checker():
    """The two passes against the 2-D float64 convolution with the outer product of the same taps: 1e-13 of the maximum
    (summation order only).  blur_cpu itself is not that close to either: it forms the outer product in fp32, as
    torchvision does, so each 2-D tap carries a rounding of up to 2**-25 of itself (measured: 1.1e-8 of the maximum at
    (37, 10, 7)).  The taps sum to 1, hence |blur_cpu - blur_cpu_sep| <= 2**-25 * max|heat|, asserted with 2**-24."""
    for H, W, k in ((37, 10, 7), (26, 26, 51)):
        heat = make_heats(3, H, W, seed=H)
        g, r = gaussian_taps(k).double(), k // 2
        exact = F.conv2d(F.pad(heat.double()[:, None], (r, r, r, r), mode="reflect"), (g[:, None] * g[None, :])[None, None])[:, 0]
        sep = blur_cpu_sep(heat, k)
        assert (exact - sep).abs().max().item() <= 1e-13 * exact.abs().max().item()
        d = (blur_cpu(heat, k) - sep).abs().max().item()
        print(f"blur_cpu - blur_cpu_sep at ({H}, {W}, {k}): {d:.3g}")
        assert d <= ULP * heat.abs().max().item()


# ------------------------------------------------------------------------------------------------ K13: impulses
@functools.lru_cache(maxsize=None)
def impulse_case(H, W, k):
    r, TH, rpt = tiling(H, W, k)
    ys = sorted({y for y in (0, H - 1, TH - 1, TH, rpt - 1, rpt, H // 2) if 0 <= y < H})
    xs = sorted({x for x in (0, W - 1, 63, 64, W // 2) if 0 <= x < W})
    rel = torch.zeros(2, 1, H, W)
    for iy, y in enumerate(ys):
        for ix, x in enumerate(xs):
            n = iy * len(xs) + ix
            rel[0, 0, y, x] = 1 + n % 4
            if (iy + 2 * ix) % 3:  # the second image: another subset, other values
                rel[1, 0, y, x] = 1 + (3 * n + 1) % 4
    b = blur_cpu_sep(rel[:, 0], k)
    return rel, b / b.amax((1, 2), keepdim=True)


@pytest.mark.parametrize("H,W,k,Cin", GEOMETRIES)
def test_impulses_land_where_the_checker_puts_them(H, W, k, Cin):
    """Positive integer impulses on every tile seam, B = 2, Cin = 1, CROP.  A wrong row, column, halo row or strip width
    moves a blurred impulse by a whole pixel, i.e. by far more than rounding.

    Where the reference is exactly 0 (no impulse inside the window) the kernel sums taps times 0: exactly 0.  Elsewhere
    |got - want| <= 32 * 2**-24 * want: every term is positive, so nothing cancels and each rounding is relative to the
    result.  The tap arguments are bit-equal to torchvision's fp32 sequence (integers / fp32 sigma); two expf
    implementations differ by about 2 ulp per tap; then come two products, at most four adds of non-zero terms, one divide
    and the max (a few ulp), and the common 1 / sum(pdf) factor cancels in b / max b.  A numpy transcription of the tile
    loops with the checker's taps stays at or below 5 ulp at every geometry; 32 leaves room for the expf difference only."""
    rel, want = impulse_case(H, W, k)
    heat, box, flags, _ = run_k13(rel, torch.zeros(2, 3, H, W), "crop", k, crop_th=0.5)
    got = heat.double()
    zero = want == 0
    assert zero.any() or k == 255  # k = 255 covers these planes entirely
    assert torch.equal(got[zero], torch.zeros_like(got[zero]))
    rerr = ((got - want).abs()[~zero] / want[~zero]).max().item()
    print(f"K13 impulses H={H} W={W} k={k}: max relative error {rerr / ULP:.2f} ulp (bound 32)")
    assert bool(((got - want).abs() <= 32 * ULP * want).all()), rerr / ULP
    check_boxes(heat, want, box, 0.5, H, W)
    if W > 1024:  # a wide flat plane: the square box is shifted to row 0 and passes H, reported unclamped
        assert square_box(want[0].numpy(), 0.5)[1] > H and box[0][1] > H
    assert np.all(flags & 1)


# ------------------------------------------------------------------------------------------------ K13: dense planes
@functools.lru_cache(maxsize=None)
def dense_case(H, W, k, Cin):
    """4 relevance-like images as in test_gpu_render's blur test plus one all-zero image; the float64 blur of their
    channel sums, A = max|sum| and mx = max|blur| per image."""
    seed = H + W + k + {(131, 130, 255, 3): 3, (128, 128, 255, 1): 2}.get((H, W, k, Cin), 0)  # k = 255 averages a plane away: mx >= 0.05 A
    g = torch.Generator().manual_seed(seed + 6 * H)
    base = make_heats(4, H, W, seed=seed)
    rel = base[:, None] * torch.rand(4, Cin, 1, 1, generator=g) + 0.05 * torch.randn(4, Cin, H, W, generator=g)
    rel = torch.cat([rel, torch.zeros(1, Cin, H, W)])
    s = rel.double().sum(1)
    b = blur_cpu_sep(s, k).abs()
    return rel, b, s.abs().amax((1, 2)), b.amax((1, 2))


@pytest.mark.parametrize("H,W,k,Cin", GEOMETRIES)
@pytest.mark.parametrize("style", ["crop", "opaque"])
def test_dense_planes_match_the_separable_checker(H, W, k, Cin, style):
    """Reference: rel.double().sum(1) -> blur_cpu_sep -> |.| / max.  With A = max|rel.double().sum(1)| and mx the maximum
    of the float64 blur (per image), the normalised heat may differ by 2 * E / mx + 2**-22, E = 2**-24 * (2k + Cin + 8) * A:
    a sequential fp32 sum of Cin channels is within (Cin - 1) ulp of A, each of the two sequential k-term dot products with
    taps that sum to 1 adds at most (k + 1) ulp of A, the taps themselves carry a few ulp; an absolute error E on the blur
    and on its maximum moves |b| / max|b| by at most 2 * E / mx, and the divide and the fp32 store add 2**-22 at most.
    The bound is only meaningful while the blur keeps a fair share of the plane's magnitude: mx >= 0.05 * A is asserted on
    the reference (the seeds give 0.115 .. 1.0)."""
    rel, b, A, mx = dense_case(H, W, k, Cin)
    assert bool((mx[:4] >= 0.05 * A[:4]).all()), (mx / A).tolist()
    img = torch.rand(5, 3, H, W, generator=torch.Generator().manual_seed(1))
    heat, box, flags, _ = run_k13(rel, img, style, k)
    if style == "crop":  # the all-zero image: 0 / 0
        assert torch.isnan(heat[4]).all()
    else:
        assert torch.equal(heat[4], torch.zeros(H, W))
    assert tuple(box[4]) == full_box(H, W)
    want = b[:4] / (mx[:4, None, None] + (0.0 if style == "crop" else 1e-8))
    tol = 2 * ULP * (2 * k + Cin + 8) * A[:4] / mx[:4] + 2.0 ** -22
    err = (heat[:4].double() - want).abs().amax((1, 2))
    print(f"K13 dense H={H} W={W} k={k} Cin={Cin} {style}: max error {err.max().item():.3g} (bounds {tol.min().item():.3g} .. "
          f"{tol.max().item():.3g}), mx/A {(mx[:4] / A[:4]).min().item():.3f} .. {(mx[:4] / A[:4]).max().item():.3f}")
    assert bool((err <= tol).all()), (err.tolist(), tol.tolist())
    if k == 1 and style == "crop":  # taps [1]: no arithmetic but the divide
        assert Cin == 1 and torch.equal(heat[:4], norm_cpu(rel[:4].sum(1), 0))
    check_boxes(heat[:4], want, box[:4], 0.01, H, W)
    if style == "crop":
        assert np.all(flags[:4] & 1)


# ------------------------------------------------------------------------------------------------ K13: pixels
@pytest.mark.parametrize("H,W,k", [g[:3] for g in (GEOMETRIES[2], GEOMETRIES[4], GEOMETRIES[6])])
@pytest.mark.parametrize("style,rf", [("crop", False), ("opaque", True), ("opaque", False), ("lighten", True), ("lighten", False)])
def test_pixels_match_the_checker_at_tile_edges(H, W, k, style, rf):
    """test_gpu_render's pixel test (render_checker within 1 LSB, the stroke footprint against the 4-neighbour rule
    exactly, one constant image) at k = 255, at a plane taller than one vertical tile and at one wider than the workgroup."""
    pixels_match_the_checker(H, W, k, style, rf)


# ------------------------------------------------------------------------------------------------ K14: upsample ratios
def ref_heat(maps, size):
    return F.interpolate(maps.double()[:, None], size=size, mode="bilinear", align_corners=False)[:, 0].clamp_min(0)


def check_k14(act, rows, chans, maps, size, k, crop_th, **kw):
    """|heat - interpolate in float64| <= 2**-24 * (6 * (gh + gw) + 8) * max|map| per pair: the fp32 source coordinate
    scale * (dst + 0.5) - 0.5 carries at most 3 ulp of its magnitude (scale, product, subtraction), i.e. 3 * 2**-24 * g
    grid cells along an axis of g cells; a coordinate error moves the lerp by that times a neighbour difference of at most
    2 * max|map|; the lerp's own arithmetic adds a few ulp of max|map|.  (1e-6 * max in test_gpu_crop_db.py holds for
    integer ratios, whose coordinates are exact.)  Boxes: K13's CROP style and sl_heat_boxes on the same heat, bit for bit,
    with and without the heat written."""
    gh, gw = maps.shape[1:]
    heat, box = N.activation_heat_boxes(act.to(DEV), rows, chans, size, kernel_size=k, crop_th=crop_th, want_heat=True, **kw)
    want = ref_heat(maps, size)
    amax = maps.double().abs().amax((1, 2))
    err = (heat.cpu().double() - want).abs().amax((1, 2))
    tol = ULP * (6 * (gh + gw) + 8) * amax
    print(f"K14 ({gh}, {gw}) -> {tuple(size)}: max error / max|map| {(err.max() / amax.max()).item():.3g} (bound {ULP * (6 * (gh + gw) + 8):.3g})")
    assert bool((err <= tol).all()), (err / amax).tolist()
    _, box13, _, _ = N.render_heatmaps(heat[:, None], torch.zeros(len(rows), 3, *size, device=DEV), "crop", kernel_size=k, crop_th=crop_th)
    assert torch.equal(box, box13)
    assert torch.equal(N.heat_boxes(heat, kernel_size=k, crop_th=crop_th), box)
    none, box2 = N.activation_heat_boxes(act.to(DEV), rows, chans, size, kernel_size=k, crop_th=crop_th, **kw)
    assert none is None and torch.equal(box2, box)
    return heat, box


@pytest.mark.parametrize("hw,size", [((7, 7), (100, 100)), ((13, 9), (120, 200)), ((37, 37), (518, 518)), ((56, 56), (32, 48)),
                                     ((3, 5), (26, 27)), ((1, 5), (30, 64))])
def test_conv_heat_at_non_integer_and_downsampling_ratios(hw, size):
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    act = torch.randn(3, 5, *hw, generator=g)
    rows, chans = torch.tensor([0, 2, 1, 2]), torch.tensor([4, 0, 3, 1])
    check_k14(act, rows, chans, act[rows, chans], size, 51, 0.01)


def test_two_dimensional_layer_gives_constant_planes():
    """(B, C): a 1 x 1 grid.  Both neighbours of every pixel are the one value a, so the plane is max(a, 0) exactly.

    This test found that the plane was not constant: UpsampledActHeat blended the cell with itself, as ATen's fp32 kernel
    does, h0 * (w0 * a + w1 * a) + h1 * (w0 * a + w1 * a) with rounded weights, up to 3 ulp off a on 1 - 2 % of the pixels
    (F.interpolate in fp32 shows the same).  No box moved, but the heat of a (B, C) layer was not the activation.  The
    kernel now skips the blend along an axis of one cell; grids with two or more cells per axis are computed as before."""
    g = torch.Generator().manual_seed(4)
    act = torch.randn(6, 7, generator=g)
    rows, chans = torch.tensor([0, 1, 2, 3, 5, 4]), torch.tensor([6, 2, 0, 3, 1, 5])
    act[rows[:3], chans[:3]] = act[rows[:3], chans[:3]].abs() + 0.1  # three positive values with full mantissas
    act[3, 3], act[5, 1] = 0.0, -1.5
    heat, box = check_k14(act, rows, chans, act[rows, chans][:, None, None], (40, 40), 21, 0.01)
    want = act[rows, chans].clamp_min(0)[:, None, None].expand(6, 40, 40)
    assert torch.equal(heat.cpu(), want)
    assert bool((want[:, 0, 0] > 0).sum() >= 3)
    for j in range(6):  # a constant plane blurs to a constant plane: everything above crop_th, or nothing (a zero plane)
        norm = np.full((40, 40), 1.0 if want[j, 0, 0] > 0 else np.nan, np.float32)
        assert tuple(box[j].tolist()) == square_box(norm, 0.01)


def test_token_heat_with_prefix_and_trailing_tokens():
    g = torch.Generator().manual_seed(6)
    act = torch.randn(3, 2 + 3 * 5 + 1, 6, generator=g)  # T = 18: two prefix tokens, a 3 x 5 grid, one trailing token
    act[:, :2], act[:, 17] = 1e3, -1e3  # reading a prefix or the trailing token would show
    rows, chans = torch.tensor([0, 1, 2, 1]), torch.tensor([5, 0, 3, 5])
    maps = act[rows, 2:17, :][torch.arange(4), :, chans].reshape(4, 3, 5)
    check_k14(act, rows, chans, maps, (30, 44), 21, 0.05, token_grid=(3, 5), prefix_tokens=2)


def test_out_of_range_pairs_give_an_all_zero_map():
    """Device-resident rows / channels skip the wrapper's host check; the header promises an all-zero map for a pair out of
    range: heat 0, the full-image square box, the other pairs of the batch untouched."""
    g = torch.Generator().manual_seed(8)
    act = torch.randn(3, 4, 6, 5, generator=g).to(DEV)
    rows, chans = torch.tensor([0, 3 + 5, 1, 2, 2]), torch.tensor([1, 2, 3, -1, 0])
    size = (36, 50)
    heat, box = N.activation_heat_boxes(act, rows.to(DEV), chans.to(DEV), size, kernel_size=11, crop_th=0.05, want_heat=True)
    ok = torch.tensor([0, 2, 4])
    heat_ok, box_ok = N.activation_heat_boxes(act, rows[ok], chans[ok], size, kernel_size=11, crop_th=0.05, want_heat=True)
    assert torch.equal(heat[ok.to(DEV)], heat_ok) and torch.equal(box[ok.to(DEV)], box_ok)
    assert bool((heat_ok.amax((1, 2)) > 0).all())
    for j in (1, 3):
        assert torch.equal(heat[j].cpu(), torch.zeros(size)) and tuple(box[j].tolist()) == full_box(*size)
    _, box2 = N.activation_heat_boxes(act, rows.to(DEV), chans.to(DEV), size, kernel_size=11, crop_th=0.05)
    assert torch.equal(box2, box)


# ------------------------------------------------------------------------------------------------ sl_condition_init
def plant(ch, same_thread=None, cross_thread=None, flat=None, nan_wins=None, first_nan=None, signed_zero=None):
    """`ch[slot]` is a (S,) view of one (row, channel) of the layer; positions s and s + 1024 belong to one thread."""
    if same_thread is not None:
        ch[same_thread][5] = ch[same_thread][5 + 1024] = 99.0  # equal maxima in one thread: the earlier one
    if cross_thread is not None:
        ch[cross_thread][7] = ch[cross_thread][1030] = 99.0  # thread 6 holds s = 1030, thread 7 the earlier s = 7
    if flat is not None:
        ch[flat].fill_(3.0)  # every thread's candidate ties: s = 0
    if nan_wins is not None:
        s = 2000 if ch[nan_wins].shape[0] > 2000 else 1400
        ch[nan_wins][3], ch[nan_wins][s] = 99.0, float("nan")  # NaN is the largest value, whatever comes before it
    if first_nan is not None:
        ch[first_nan][8] = ch[first_nan][1031] = float("nan")  # two NaNs: the first, held by the later thread
    if signed_zero is not None:
        ch[signed_zero].fill_(-2.0)
        ch[signed_zero][9], ch[signed_zero][1032] = -0.0, 0.0  # -0.0 == +0.0: the first index, its sign kept


@pytest.mark.parametrize("rf", [True, False])
def test_condition_init_with_more_than_one_element_per_thread(rf):
    """S = 2400 and 1500: each of the 1024 threads scans two or three positions, then the tree reduction settles ties across
    threads.  Bit equality with torch.argmax's rule (first index among equals, NaN largest) on int32 views."""
    g = torch.Generator().manual_seed(12)
    conv = torch.randint(-5, 6, (3, 4, 40, 60), generator=g).float()
    plant({(i, c): conv[i, c].view(-1) for i in range(3) for c in range(4)}, same_thread=(0, 0), cross_thread=(1, 0), flat=(2, 0),
          nan_wins=(0, 1), first_nan=(1, 1), signed_zero=(2, 1))
    tokens = torch.randint(-5, 6, (2, 1500, 8), generator=g).float()
    plant({(i, c): tokens[i, :, c] for i in range(2) for c in range(8)}, same_thread=(0, 0), cross_thread=(1, 0), flat=(0, 1),
          nan_wins=(1, 1), first_nan=(0, 2), signed_zero=(1, 2))
    cases = [(conv, False), (conv.to(memory_format=torch.channels_last), False), (tokens, True)]
    for a, tok in cases:
        C = a.shape[2] if tok else a.shape[1]
        for c in range(C):
            ch = [c] * a.shape[0]
            want = _condition_cpu(a.contiguous(), ch, rf, tok)
            got = N.condition_init(a.to(DEV), ch, rf).cpu().contiguous()
            assert got.shape == want.shape
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (tok, c)
            if rf:  # the checker itself: one position per row, the planted one
                assert int((want.view(torch.int32) != 0).sum()) <= a.shape[0]
    if rf:
        want = _condition_cpu(conv, [0, 0, 0], True, False).view(3, 4, -1)
        assert want[0, 0, 5] == 99 and want[1, 0, 7] == 99 and want[2, 0, 0] == 3
        want = _condition_cpu(conv, [1, 1, 1], True, False).view(3, 4, -1)
        assert torch.isnan(want[0, 1, 2000]) and torch.isnan(want[1, 1, 8]) and not torch.isnan(want[1, 1, 1031])
        assert want[2, 1].view(torch.int32)[9] == -2 ** 31  # -0.0
