"""K12 (device preprocessing) at output sizes S that are not multiples of 4: the case table, held on the host.

Both passes of ``csrc/preprocess.hip`` change code path on ``S % 4`` (packed quad store / ``float4`` store / 12-byte
store against their scalar forms, ``ncol < 4`` in the last column group).  This file defines the table of sizes and
source shapes once (``tests/test_gpu_preprocess_edges.py`` imports it) and checks, without a GPU,

1. that the CPU oracle, the reference of the GPU file, equals Pillow + torch arithmetic on the whole table, bit for bit
   (12 sizes x 17 shapes x 2 modes x 2 filters = 816 cases);
2. that the table reaches every class of work the kernels distinguish, one assertion per class (``CLASSES``), with a
   restatement of ``precompute_coeffs``' per-index bounds that is itself held to the plan's KH / KV / TOP / LEFT;
3. the planners' refusals at their exact limits and the ROI plan columns at odd S.

Which shape serves which class.  Named is the first witness in table order, all of them ``shortest`` / ``bicubic``; most
classes recur at every S, because a shape's tap counts follow its ratio to S.

    horizontal pass, per kept output column (taps = source columns read), source height h
      taps < 4 (scalar multiply loop)          S=1 (1, 1): 1 tap; every upscale near an edge, e.g. (1, 1) at any S
      taps >= 4, taps % 4 == 0 (no tail)       S=1 (1, 9): 9 -> 9 is the identity, 4 taps
      taps >= 4, taps % 4 == 1 (tail of 1)     S=1 (5, 5): 5 taps
      taps >= 4, taps % 4 == 2 (tail of 2)     S=1 (13, 200): 200 -> 15 columns
      taps >= 4, taps % 4 == 3 (tail of 3)     S=1 (4, 7): 7 taps
      h % 4 == 0, 1, 2, 3 (rows of last group) (4, 7), (1, 1), (2, 3), (3, 2); also (200, 13), (257, 63), (S, S) ...
      h < 4 (every thread a partial one)       (1, 1), (1, 9), (2, 3), (3, 2)
    vertical pass, per kept output row (taps = intermediate rows read)
      taps % 4 == 0, 1, 2, 3 (unroll-4 loop)   S=1 (9, 1): 4; (1, 1): 1; (2, 3): 2; (3, 2): 3
      ncol == 1, 2, 3 (last column group)      S % 4 == 1: S in {1, 5, 9, 13, 37}; 2: {2, 6, 30, 50}; 3: {3, 7, 67}
      full quads at S % 4 != 0 (unaligned)     every S >= 5 of the table, S=5 first
    centre crop, int(round(d / 2.0)) with d = resized - S odd
      floor(d / 2) even (the half rounds down) d = 1: (S, S + 1) and (S + 1, S) at every S, S=1 (1, 2) first
      floor(d / 2) odd  (the half rounds up)   S=1 (257, 63): 257 -> 4 rows, d = 3

``test_table_reaches_class`` asserts each class on its own; ``coverage()`` maps every class to its first witness.
"""
import functools
import math

import numpy as np
import pytest

import oracle
from semanticlens_amd import _native as N

SIZES = (1, 2, 3, 5, 6, 7, 9, 13, 30, 37, 50, 67)
MODES = ("shortest", "squash")
INTERPS = ("bicubic", "bilinear")
# plan columns (csrc/preprocess.hip)
P_OFF, P_H, P_W, P_OH, P_OW, P_TOP, P_LEFT, P_KH, P_KV, P_ROW_BYTES = 0, 1, 2, 3, 4, 5, 6, 7, 8, 12


def SHAPES(S):
    return ((1, 1), (1, 9), (9, 1), (2, 3), (3, 2), (5, 5), (7, 4), (4, 7), (S, S), (S, S + 1), (S + 1, S), (S + 3, 2 * S + 1),
            (13, 200), (200, 13), (3 * S + 2, 4 * S + 1), (129, 131), (257, 63))


def CASES():
    for S in SIZES:
        for mode in MODES:
            for interp in INTERPS:
                for h, w in SHAPES(S):
                    yield S, h, w, mode, interp


@functools.lru_cache(maxsize=None)
def image(h, w):
    """Seeded (h, w, 3) uint8 source: random bytes, about 30 % of the pixels (255, 0, 255) so clip8 saturates both ways."""
    rng = np.random.default_rng([12, h, w])
    arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    arr[rng.random((h, w)) < 0.3] = (255, 0, 255)
    arr.setflags(write=False)
    return arr


# ---- restatement of the plan and of Resample.c precompute_coeffs' bounds -----------------------------------------------
def resized_size(h, w, S, mode):
    if mode == "squash":
        return S, S
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(S * long / short)
    return (new_long, S) if w <= h else (S, new_long)


def crop_offset(size, S):
    return int(round((size - S) / 2.0))  # Python rounds half to even, like torchvision's CenterCrop


def axis_bounds(in_size, out_size, crop0, S, interp):
    """(ksize, [(first source index, tap count) for the S kept output indices]) of one axis."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = (2.0 if interp == "bicubic" else 1.0) * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = []
    for j in range(S):
        center = (j + crop0 + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        bounds.append((xmin, xmax - xmin))
    return ksize, bounds


def case_geometry(S, h, w, mode, interp):
    oh, ow = resized_size(h, w, S, mode)
    top, left = crop_offset(oh, S), crop_offset(ow, S)
    kh, hb = axis_bounds(w, ow, left, S, interp)
    kv, vb = axis_bounds(h, oh, top, S, interp)
    return dict(oh=oh, ow=ow, top=top, left=left, kh=kh, kv=kv, hb=hb, vb=vb)


CLASSES = (
    "h_taps_lt4", "h_taps_ge4_mod0", "h_taps_ge4_mod1", "h_taps_ge4_mod2", "h_taps_ge4_mod3",
    "h_rows_mod0", "h_rows_mod1", "h_rows_mod2", "h_rows_mod3", "h_rows_lt4",
    "v_taps_mod0", "v_taps_mod1", "v_taps_mod2", "v_taps_mod3",
    "v_ncol1", "v_ncol2", "v_ncol3", "v_full_quad_unaligned",
    "crop_half_floor_even", "crop_half_floor_odd",
)


def case_classes(S, h, w, geo):
    out = set()
    for _, n in geo["hb"]:
        out.add("h_taps_lt4" if n < 4 else f"h_taps_ge4_mod{n % 4}")
    out.add(f"h_rows_mod{h % 4}")
    if h < 4:
        out.add("h_rows_lt4")
    for _, n in geo["vb"]:
        out.add(f"v_taps_mod{n % 4}")
    if S % 4:
        out.add(f"v_ncol{S % 4}")
        if S > 4:
            out.add("v_full_quad_unaligned")
    for d in (geo["oh"] - S, geo["ow"] - S):
        if d % 2:
            out.add("crop_half_floor_even" if (d // 2) % 2 == 0 else "crop_half_floor_odd")
    return out


@functools.lru_cache(maxsize=None)
def coverage():
    """class -> first (S, h, w, mode, interp) of the table that supplies it"""
    seen = {}
    for case in CASES():
        S, h, w, mode, interp = case
        for c in case_classes(S, h, w, case_geometry(*case)):
            seen.setdefault(c, case)
    return seen


# ---- 1. the oracle is Pillow at these sizes ----------------------------------------------------------------------------
def test_oracle_equals_pillow_on_the_whole_table():
    pytest.importorskip("PIL")
    from golden import make_golden_preprocess as G  # the Pillow + torch recipe that made tests/golden/preprocess.npz

    n = 0
    for S, h, w, mode, interp in CASES():
        img = image(h, w)
        want_u8, want_f = G.transform(img, S, mode, interp)
        u8, f = oracle.preprocess(img, S, G.MEAN, G.STD, mode, interp)
        assert np.array_equal(u8, want_u8), f"bytes differ from Pillow: S={S} {h}x{w} {mode} {interp}"
        assert np.array_equal(f, want_f), f"floats differ from torch: S={S} {h}x{w} {mode} {interp}"
        n += 1
    assert n == 816


# ---- 2. the table reaches every branch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("interp", INTERPS)
def test_restated_bounds_agree_with_the_plan(mode, interp):
    for S in SIZES:
        shapes = SHAPES(S)
        plan, _ = N.preprocess_plan(shapes, S, mode, interp)
        for (h, w), row in zip(shapes, plan.tolist()):
            geo = case_geometry(S, h, w, mode, interp)
            where = f"S={S} {h}x{w} {mode} {interp}"
            assert (row[P_H], row[P_W], row[P_OH], row[P_OW]) == (h, w, geo["oh"], geo["ow"]), where
            assert (row[P_TOP], row[P_LEFT]) == (geo["top"], geo["left"]), where
            assert (row[P_KH], row[P_KV]) == (geo["kh"], geo["kv"]), where
            # every kept index has at least one tap, inside the source and inside the coefficient row
            assert all(0 <= x0 and 1 <= n <= geo["kh"] and x0 + n <= w for x0, n in geo["hb"]), where
            assert all(0 <= y0 and 1 <= n <= geo["kv"] and y0 + n <= h for y0, n in geo["vb"]), where


@pytest.mark.parametrize("cls", CLASSES)
def test_table_reaches_class(cls):
    assert cls in coverage(), f"no case of the table supplies {cls}: add the smallest shape that does"


def test_classes_are_all_known():
    assert set(coverage()) <= set(CLASSES)


# ---- 3. refusals at the exact limits, ROI plan columns at odd S -------------------------------------------------------
def test_plan_accepts_the_largest_side_and_refuses_the_next():
    big = 2**24 - 1
    for hw in ((big, 1), (1, big), (big, 3)):
        plan, info = N.preprocess_plan([hw], 5)
        assert plan[0, P_H].item() == hw[0] and plan[0, P_W].item() == hw[1]
        assert info["max_h"] == hw[0] and info["pixel_bytes"] == 3 * hw[0] * hw[1]
        rplan, _ = N.preprocess_plan_rois([hw], [(0, 1, 0, 1)], [0], 5)
        assert rplan[0, P_ROW_BYTES].item() == 3 * hw[1]
    for hw in ((big + 1, 1), (1, big + 1)):
        with pytest.raises(ValueError, match="has size"):
            N.preprocess_plan([hw], 5)
        with pytest.raises(ValueError, match="has size"):
            N.preprocess_plan_rois([hw], [(0, 1, 0, 1)], [0], 5)


def test_plan_refuses_size_zero():
    with pytest.raises(ValueError, match="bad shape"):
        N.preprocess_plan([(8, 8)], 0)
    with pytest.raises(ValueError, match="bad shape"):
        N.preprocess_plan_rois([(8, 8)], [(0, 4, 0, 4)], [0], 0)


def test_roi_plan_refuses_empty_boxes_and_bad_indices_at_odd_size():
    hw = [(40, 30), (25, 60)]
    for box in ((10, 10, 0, 5), (0, 5, 30, 40), (40, 45, 0, 5), (-3, 0, 0, 5), (0, 5, 7, 7), (12, 9, 0, 5)):
        with pytest.raises(ValueError, match="is empty"):
            N.preprocess_plan_rois(hw, [box], [0], 5)
    for n in (2, -1):  # index == N, and below 0
        with pytest.raises(ValueError, match="refers to image"):
            N.preprocess_plan_rois(hw, [(0, 5, 0, 5)], [n], 5)
    N.preprocess_plan_rois(hw, [(0, 5, 0, 5)], [1], 5)  # N - 1 is the last valid index


@pytest.mark.parametrize("S", [5, 37])
def test_roi_plan_row_stride_and_offset_at_odd_size(S):
    hw = [(40, 30), (25, 61)]
    boxes = [(3, 17, 5, 9), (39, 40, 0, 30), (0, 11, 7, 16), (-4, 60, 3, 99), (24, 25, 60, 61)]
    index = [0, 0, 1, 1, 1]
    plan, info = N.preprocess_plan_rois(hw, boxes, index, S)
    base = [0, 40 * 30 * 3]
    for row, (r1, r2, c1, c2), n in zip(plan.tolist(), boxes, index):
        h, w = hw[n]
        r1, r2, c1, c2 = max(r1, 0), min(r2, h), max(c1, 0), min(c2, w)
        assert row[P_ROW_BYTES] == 3 * w
        assert row[P_OFF] == base[n] + (r1 * w + c1) * 3
        assert (row[P_H], row[P_W]) == (r2 - r1, c2 - c1)
        geo = case_geometry(S, r2 - r1, c2 - c1, "shortest", "bicubic")
        assert (row[P_OH], row[P_OW], row[P_TOP], row[P_LEFT], row[P_KH], row[P_KV]) == (
            geo["oh"], geo["ow"], geo["top"], geo["left"], geo["kh"], geo["kv"])
    assert info["pixel_bytes"] == 3 * (40 * 30 + 25 * 61) and info["max_h"] == 25
