"""K12 on the device at output sizes that are not multiples of 4 (the scalar-store branch of the horizontal pass, the
``ncol < 4`` and unaligned full-quad branches of the vertical pass, S < 4), bit for bit against the CPU oracle, which
``tests/test_preprocess_edges_host.py`` holds to Pillow on the same table.  No tolerances: every comparison is equality."""
import functools

import numpy as np
import pytest
import torch

import oracle
from semanticlens_amd import _native as N
from semanticlens_amd.foundation_models import DevicePreprocess
from semanticlens_amd.foundation_models.preprocess import OPENAI_DATASET_MEAN as MEAN, OPENAI_DATASET_STD as STD
from test_preprocess_edges_host import INTERPS, MODES, SHAPES, SIZES, image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _expected(S, h, w, mode, interp):
    u8, f = oracle.preprocess(image(h, w), S, MEAN, STD, mode, interp)
    u8.setflags(write=False)
    f.setflags(write=False)
    return u8, f


def _run(imgs, S, mode="shortest", interp="bicubic", want_u8=True, want_f32=True, max_h_factor=1):
    pp = DevicePreprocess(S, MEAN, STD, mode, interp, device=DEV)
    buf, plan, info = pp.pack(imgs)
    info = dict(info, max_h=info["max_h"] * max_h_factor)
    f, u8 = N.preprocess(buf.to(DEV), plan, info, S, pp.mean, pp.std, interp, want_u8=want_u8, want_f32=want_f32)
    torch.cuda.synchronize()
    return (None if f is None else f.cpu().numpy()), (None if u8 is None else u8.cpu().numpy())


# ---- 1. the whole table, one ragged batch per (S, mode, filter) --------------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", SIZES)
def test_table_ragged_batch_equals_oracle(S, mode, interp):
    shapes = SHAPES(S)
    f, u8 = _run([image(h, w) for h, w in shapes], S, mode, interp)
    assert f.shape == (len(shapes), 3, S, S) and u8.shape == (len(shapes), S, S, 3)
    for b, (h, w) in enumerate(shapes):
        eu8, ef = _expected(S, h, w, mode, interp)
        assert np.array_equal(u8[b], eu8), f"bytes: S={S} image {b} {h}x{w} {mode} {interp}"
        assert np.array_equal(f[b], ef), f"floats: S={S} image {b} {h}x{w} {mode} {interp}"


# ---- 2. an image's result does not depend on its neighbours in the batch -----------------------------------------------
@pytest.mark.parametrize("S", [5, 37])
def test_batch_independence_at_odd_sizes(S):
    imgs = [image(h, w) for h, w in SHAPES(S)]
    f_all, u_all = _run(imgs, S)
    f_rev, u_rev = _run(imgs[::-1], S)
    for b, (h, w) in enumerate(SHAPES(S)):
        f_one, u_one = _run([imgs[b]], S)
        r = len(imgs) - 1 - b
        assert np.array_equal(u_one[0], u_all[b]) and np.array_equal(f_one[0], f_all[b]), f"alone vs batch: S={S} {h}x{w}"
        assert np.array_equal(u_rev[r], u_all[b]) and np.array_equal(f_rev[r], f_all[b]), f"reversed vs batch: S={S} {h}x{w}"
        eu8, ef = _expected(S, h, w, "shortest", "bicubic")
        assert np.array_equal(u_all[b], eu8) and np.array_equal(f_all[b], ef), f"batch vs oracle: S={S} {h}x{w}"


# ---- 3. sizes real towers use -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,mode,interp", [(299, "shortest", "bicubic"), (378, "shortest", "bicubic"), (518, "shortest", "bicubic"),
                                           (299, "squash", "bilinear")])
def test_real_sizes_off_the_multiple_of_four(S, mode, interp):
    shapes = [(500, 375), (375, 500), (97, 640)]
    f, u8 = _run([image(h, w) for h, w in shapes], S, mode, interp)
    for b, (h, w) in enumerate(shapes):
        eu8, ef = _expected(S, h, w, mode, interp)
        assert np.array_equal(u8[b], eu8), f"bytes: S={S} {h}x{w} {mode} {interp}"
        assert np.array_equal(f[b], ef), f"floats: S={S} {h}x{w} {mode} {interp}"


# ---- 4. either output alone ----------------------------------------------------------------------------------------------
def test_output_selection_at_odd_size():
    imgs = [image(h, w) for h, w in SHAPES(7)]
    f, u8 = _run(imgs, 7)
    f_only, none_u8 = _run(imgs, 7, want_u8=False, want_f32=True)
    none_f, u8_only = _run(imgs, 7, want_u8=True, want_f32=False)
    assert none_u8 is None and none_f is None
    assert np.array_equal(f_only, f) and np.array_equal(u8_only, u8)
    for b, (h, w) in enumerate(SHAPES(7)):
        eu8, ef = _expected(7, h, w, "shortest", "bicubic")
        assert np.array_equal(u8[b], eu8) and np.array_equal(f[b], ef), f"{h}x{w}"


# ---- 5. sub-rectangles at odd sizes ---------------------------------------------------------------------------------------
def _roi_cases():
    imgs = [image(h, w) for h, w in ((50, 37), (33, 64), (96, 80))]
    boxes, index = [], []
    for n, im in enumerate(imgs):
        h, w = im.shape[:2]
        for b in ((0, h, 0, w), (0, 5, 0, w), (h - 5, h, 0, w), (0, h, 0, 1), (0, h, w - 1, w), (3, 4, 0, w), (7, 8, 9, 10),
                  (-4, h + 9, 2, w + 20), (h // 3, h // 2 + 7, w // 4, w - 3), (h - 1, h + 5, w - 2, w + 30),
                  (2, 9, 5, 9),          # width exactly 4: one full tap group, no tail
                  (h - 1, h, 0, w),      # height exactly 1, the image's last row
                  (0, 11, 5, 14)):       # starts at byte column 15 of row 0: an odd address in all three images
            boxes.append(b)
            index.append(n)
    return imgs, boxes, index


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [5, 37])
def test_roi_at_odd_sizes_is_the_oracle_on_the_slice(S, mode, interp):
    imgs, boxes, index = _roi_cases()
    pp = DevicePreprocess(S, MEAN, STD, mode, interp, device=DEV)
    got = pp.crops(imgs, boxes, index).cpu().numpy()
    assert got.shape == (len(boxes), 3, S, S)
    for j, ((r1, r2, c1, c2), n) in enumerate(zip(boxes, index)):
        h, w = imgs[n].shape[:2]
        sl = imgs[n][max(r1, 0):min(r2, h), max(c1, 0):min(c2, w)]
        _, want = oracle.preprocess(sl, S, MEAN, STD, mode, interp)
        assert np.array_equal(got[j], want), f"S={S} image {n} box {(r1, r2, c1, c2)} {mode} {interp}"


# ---- 6. grey input, device tensor batch ------------------------------------------------------------------------------------
def test_grey_input_equals_its_replication():
    pp = DevicePreprocess(6, MEAN, STD, device=DEV)
    grey = image(23, 17)[:, :, 1].copy()
    rgb = np.repeat(grey[:, :, None], 3, axis=2)
    got = pp([grey, rgb, torch.from_numpy(grey)]).cpu().numpy()
    _, want = oracle.preprocess(rgb, 6, MEAN, STD)
    for b in range(3):
        assert np.array_equal(got[b], want), b


def test_device_tensor_batch_equals_the_list_path():
    h, w, S = 45, 61, 30
    imgs = [np.ascontiguousarray(image(h + 5 * b, w + 3)[b:b + h, 1:1 + w]) for b in range(5)]
    pp = DevicePreprocess(S, MEAN, STD, device=DEV)
    from_list = pp(imgs).cpu().numpy()
    batch = torch.from_numpy(np.stack(imgs))
    from_device = pp(batch.to(DEV)).cpu().numpy()
    from_host = pp(batch).cpu().numpy()
    assert np.array_equal(from_device, from_list) and np.array_equal(from_host, from_list)
    for b, im in enumerate(imgs):
        assert np.array_equal(from_list[b], oracle.preprocess(im, S, MEAN, STD)[1]), b


# ---- 7. the pinned staging slots are reused only after their upload -------------------------------------------------------
def test_staging_reuse_without_synchronisation():
    S = 13
    groups = [SHAPES(S)[11:17], SHAPES(S)[0:6], SHAPES(S)[6:12]]  # the largest first, so that its buffer serves the third
    pp = DevicePreprocess(S, MEAN, STD, device=DEV)
    outs, slots = [], []
    for g in groups:  # no synchronisation in between: the third call rewrites the pinned memory the first call uploaded from
        outs.append(pp([image(h, w) for h, w in g]))
        slots.append((pp._slot, pp._staging[pp._slot].data_ptr()))
    assert slots[0] == slots[2] and slots[1][0] != slots[0][0]
    for g, out in zip(groups, outs):
        out = out.cpu().numpy()
        for b, (h, w) in enumerate(g):
            assert np.array_equal(out[b], _expected(S, h, w, "shortest", "bicubic")[1]), f"{h}x{w}"


# ---- 8. a declared height above the tallest image only adds threads that return -------------------------------------------
def test_declared_height_larger_than_needed():
    imgs = [image(h, w) for h, w in SHAPES(7)]
    f, u8 = _run(imgs, 7)
    f4, u84 = _run(imgs, 7, max_h_factor=4)
    assert np.array_equal(f4, f) and np.array_equal(u84, u8)


# ---- 9. refusals of the launch call: each returns before any kernel is launched -------------------------------------------
def _tiny():
    plan, info = N.preprocess_plan([(4, 4)], 4)
    return torch.zeros(48, dtype=torch.uint8, device=DEV), plan, info


def test_launch_refuses_more_than_65535_images():
    plan, info = N.preprocess_plan([(1, 1)] * 65536, 1)
    pixels = torch.zeros(3 * 65536, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="at most 65535 images"):
        N.preprocess(pixels, plan, info, 1, MEAN, STD)
    f, _ = N.preprocess(pixels[:-3], plan[:-1], info, 1, MEAN, STD)  # 65535 is the last accepted count
    want = oracle.preprocess(np.zeros((1, 1, 3), np.uint8), 1, MEAN, STD)[1]
    assert np.array_equal(f.cpu().numpy(), np.broadcast_to(want, (65535, 3, 1, 1)))


def test_launch_refuses_a_bad_workspace_split():
    pixels, plan, info = _tiny()
    with pytest.raises(ValueError, match="bad workspace split"):
        N.preprocess(pixels, plan, dict(info, coef_bytes=info["coef_bytes"] + 8, ws_bytes=info["ws_bytes"] + 16), 4, MEAN, STD)
    with pytest.raises(ValueError, match="bad workspace split"):
        N.preprocess(pixels, plan, dict(info, coef_bytes=info["ws_bytes"] + 16), 4, MEAN, STD)
    with pytest.raises(ValueError, match="bad workspace split"):
        N.preprocess(pixels, plan, dict(info, coef_bytes=-16), 4, MEAN, STD)


def test_launch_refuses_a_call_without_outputs():
    pixels, plan, info = _tiny()
    with pytest.raises(ValueError, match="null pointer"):
        N.preprocess(pixels, plan, info, 4, MEAN, STD, want_u8=False, want_f32=False)


def test_launch_refuses_an_image_too_tall_for_the_grid():
    plan, info = N.preprocess_plan([(32, 32)], 32)
    pixels = torch.zeros(32 * 32 * 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="image too tall"):
        N.preprocess(pixels, plan, dict(info, max_h=2**28), 32, MEAN, STD)
    torch.cuda.synchronize()
    f, _ = N.preprocess(pixels, plan, info, 32, MEAN, STD)  # the refusal left nothing behind: the next call is exact
    assert np.array_equal(f.cpu().numpy()[0], oracle.preprocess(np.zeros((32, 32, 3), np.uint8), 32, MEAN, STD)[1])
