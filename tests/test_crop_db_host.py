"""CPU-only tests (-m "not gpu") of the cropped concept DB (K14): the box-scaling rule, token-grid inference, argument
validation before any launch, the cache file names and the header / binding agreement of the new entry points."""
import numpy as np
import pytest
import torch

from helpers import FakeVLM, TensorPairDataset, make_int_conv_model
from semanticlens_amd import Lens
from semanticlens_amd import _native as N
from semanticlens_amd.component_visualization import ActivationComponentVisualizer
from semanticlens_amd.component_visualization.crop_db import crop_item, infer_token_grid, item_hw, scale_box

FAKE = 1  # a non-null pointer that is never dereferenced: validation runs before any launch


def test_k14_entry_points_are_declared_and_bound():
    for name in ("sl_activation_heat_boxes", "sl_heat_boxes", "sl_preprocess_plan_rois"):
        assert name in N.SIGNATURES
        assert hasattr(N.lib(), name)


def test_scale_box_is_the_identity_at_equal_sizes():
    for box in ((0, 224, 0, 224), (10, 60, 3, 53), (100, 250, 180, 330), (0, 1, 5, 6)):
        r1, r2, c1, c2 = box
        assert scale_box(box, (224, 224), (224, 224)) == (r1, min(r2, 224), c1, min(c2, 224))


def test_scale_box_floor_ceil_and_clamp():
    # r1' = floor(r1 h / H), r2' = ceil(min(r2, H) h / H)
    assert scale_box((10, 50, 20, 70), (224, 224), (448, 112)) == (20, 100, 10, 35)
    assert scale_box((1, 3, 1, 3), (224, 224), (100, 100)) == (0, 2, 0, 2)  # floor(100/224)=0, ceil(300/224)=2
    assert scale_box((7, 9, 0, 1), (224, 224), (500, 375)) == (15, 21, 0, 2)
    # past the edge: the high ends clamp to the model input first, then to the image
    assert scale_box((180, 260, 190, 270), (224, 224), (112, 112)) == (90, 112, 95, 112)
    # non-square model input
    assert scale_box((0, 192, 64, 128), (192, 256), (96, 512)) == (0, 96, 128, 256)


def test_scale_box_empty_extent_grows_to_one_pixel():
    assert scale_box((5, 5, 0, 10), (224, 224), (224, 224)) == (5, 6, 0, 10)
    assert scale_box((0, 10, 223, 223), (224, 224), (224, 224)) == (0, 10, 223, 224)
    assert scale_box((224, 224, 0, 4), (224, 224), (224, 224)) == (223, 224, 0, 4)


def test_token_grid_inference():
    assert infer_token_grid(196) == (14, 14, 0)
    assert infer_token_grid(197) == (14, 14, 1)
    assert infer_token_grid(50) == (7, 7, 1)
    assert infer_token_grid(49) == (7, 7, 0)
    assert infer_token_grid(1) == (1, 1, 0)
    assert infer_token_grid(200, token_grid=(14, 14)) == (14, 14, 4)
    assert infer_token_grid(200, token_grid=(14, 14), prefix_tokens=2) == (14, 14, 2)
    assert infer_token_grid(198, prefix_tokens=2) == (14, 14, 2)
    with pytest.raises(ValueError, match="token_grid.*prefix_tokens"):
        infer_token_grid(200)
    with pytest.raises(ValueError, match="does not fit"):
        infer_token_grid(100, token_grid=(10, 11))
    with pytest.raises(ValueError, match="not a square grid"):
        infer_token_grid(199, prefix_tokens=1)


def test_host_crop_forms():
    arr = np.arange(6 * 5 * 3, dtype=np.uint8).reshape(6, 5, 3)
    assert item_hw(arr) == (6, 5)
    assert np.array_equal(crop_item(arr, (1, 4, 2, 5)), arr[1:4, 2:5])
    t = torch.arange(3 * 6 * 5, dtype=torch.float32).reshape(3, 6, 5)
    assert item_hw(t) == (6, 5)
    assert torch.equal(crop_item(t, (1, 4, 2, 5)), t[:, 1:4, 2:5])
    from PIL import Image

    pil = Image.fromarray(arr)
    assert item_hw(pil) == (6, 5)
    assert np.array_equal(np.asarray(crop_item(pil, (1, 4, 2, 5))), arr[1:4, 2:5])


def _boxes(P=2, B=2, C=3, S=16, prefix=0, gh=4, gw=4, H=32, W=32, k=5, crop_th=0.01, act=FAKE, rows=FAKE, chans=FAKE, box=FAKE,
           ws=FAKE, ws_bytes=1 << 30):
    return N.lib().sl_activation_heat_boxes(act, B, C, S, S * C, S, 1, prefix, gh, gw, rows, chans, P, H, W, k, crop_th, None, box, ws,
                                            ws_bytes, None)


def test_activation_heat_boxes_rejects_bad_arguments_without_a_device():
    lib = N.lib()
    for kw in ({"act": None}, {"rows": None}, {"chans": None}, {"box": None}, {"ws": None}):
        assert _boxes(**kw) == -1
        assert lib.sl_last_error() == b"sl_activation_heat_boxes: null pointer"
    assert _boxes(k=4) == -1 and b"kernel_size must be an odd positive integer, got 4" in lib.sl_last_error()
    assert _boxes(k=0) == -1
    assert _boxes(H=2, k=5) == -1 and b"kernel_size // 2 = 2 must be smaller than H and W" in lib.sl_last_error()
    assert _boxes(k=257, H=300, W=300) == -3 and b"exceeds the supported maximum" in lib.sl_last_error()
    # the limits themselves, for both entry points: W + kernel_size - 1 = 16384 fills the LDS tile; kernel_size 255 needs 128 x 128
    assert _boxes(H=2, W=16382, k=3, P=0) == 0 and lib.sl_heat_boxes(FAKE, 0, 2, 16382, 3, 0.01, FAKE, FAKE, 0, None) == 0
    assert _boxes(H=2, W=16383, k=3) == -3 and b"exceeds the supported maximum" in lib.sl_last_error()
    assert lib.sl_heat_boxes(FAKE, 2, 2, 16383, 3, 0.01, FAKE, FAKE, 1 << 30, None) == -3
    assert b"sl_heat_boxes: kernel_size 3 with W 16383 exceeds the supported maximum" in lib.sl_last_error()
    assert _boxes(H=128, W=128, k=255, P=0) == 0 and lib.sl_heat_boxes(FAKE, 0, 128, 128, 255, 0.01, FAKE, FAKE, 0, None) == 0
    assert _boxes(H=127, W=128, k=255) == -1 and b"kernel_size // 2 = 127 must be smaller than H and W" in lib.sl_last_error()
    assert lib.sl_heat_boxes(FAKE, 2, 127, 128, 255, 0.01, FAKE, FAKE, 1 << 30, None) == -1
    for crop_th in (-0.1, 1.0, float("nan")):
        assert _boxes(crop_th=crop_th) == -1 and lib.sl_last_error() == b"'crop_th' must be between [0, 1)"
    assert _boxes(prefix=1) == -1 and b"does not fit S = 16" in lib.sl_last_error()
    assert _boxes(gh=5) == -1
    assert _boxes(ws_bytes=16) == -1 and b"workspace too small" in lib.sl_last_error()
    assert _boxes(P=0) == 0  # valid, nothing to launch
    assert lib.sl_heat_boxes(FAKE, 2, 32, 32, 6, 0.01, FAKE, FAKE, 1 << 30, None) == -1
    assert lib.sl_heat_boxes(FAKE, 2, 32, 32, 5, 1.5, FAKE, FAKE, 1 << 30, None) == -1
    assert lib.sl_heat_boxes(None, 2, 32, 32, 5, 0.01, FAKE, FAKE, 1 << 30, None) == -1
    assert lib.sl_heat_boxes(FAKE, 0, 32, 32, 5, 0.01, FAKE, FAKE, 0, None) == 0


def test_python_crop_arguments_are_checked_first():
    for ks in (0, 4, 50, 257, 3.0, True):
        with pytest.raises(ValueError, match="kernel_size"):
            N.check_crop_args(0.01, ks)
    for th in (-0.01, 1.0, 2):
        with pytest.raises(ValueError, match="crop_th"):
            N.check_crop_args(th, 51)
    with pytest.raises(ValueError, match="smaller than H and W"):
        N.check_crop_args(0.01, 51, 16, 224)
    N.check_crop_args(0.0, 1, 1, 1)


def test_preprocess_plan_rois_reads_only_the_box():
    hw = [(40, 30), (20, 50)]
    boxes = [(0, 40, 0, 30), (5, 17, 10, 42), (-3, 100, -1, 7)]
    plan, info = N.preprocess_plan_rois(hw, boxes, [0, 1, 0], 16, "shortest", "bicubic")
    full, _ = N.preprocess_plan([(40, 30)], 16, "shortest", "bicubic")
    assert torch.equal(plan[0, :12], full[0, :12]) and plan[0, 12] == 30 * 3  # the row stride slot
    assert info["pixel_bytes"] == 40 * 30 * 3 + 20 * 50 * 3
    p = plan[1]
    assert p[0] == 40 * 30 * 3 + (5 * 50 + 10) * 3 and (p[1], p[2]) == (12, 32) and p[12] == 150
    p = plan[2]  # clamped to (0, 40, 0, 7)
    assert p[0] == 0 and (p[1], p[2]) == (40, 7)
    # the K12 plan is unchanged: slot 12 stays 0
    assert int(full[0, 12]) == 0
    with pytest.raises(ValueError, match="empty"):
        N.preprocess_plan_rois(hw, [(10, 10, 0, 5)], [0], 16)
    with pytest.raises(ValueError, match="empty"):
        N.preprocess_plan_rois(hw, [(0, 5, 30, 40)], [0], 16)
    with pytest.raises(ValueError, match="refers to image 2"):
        N.preprocess_plan_rois(hw, [(0, 5, 0, 5)], [2], 16)


def _cv(tmp_path):
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 4, (12, 3, 12, 12), generator=g).float()
    ds = TensorPairDataset(x, name="ds")
    model = make_int_conv_model()
    model.name = "m"
    return ActivationComponentVisualizer(model, ds, ds, ["2"], num_samples=3, device="cpu", cache_dir=str(tmp_path))


def test_concept_db_cache_file_names(tmp_path):
    cv = _cv(tmp_path)
    lens = Lens(FakeVLM(img_numel=3 * 12 * 12), device="cpu")
    plain = lens._concept_db_path(cv)
    assert plain.name == "concept_db-" + "-".join(v for k, v in cv.metadata.items() if k not in ("dataset", "model")) + ".safetensors"
    assert lens._concept_db_path(cv, crop=False, crop_th=0.3, kernel_size=7) == plain
    assert lens._concept_db_path(cv, crop=True).name == plain.stem + "-crop-th0.01-k51.safetensors"
    assert lens._concept_db_path(cv, crop=True, crop_th=0.25, kernel_size=7).name == plain.stem + "-crop-th0.25-k7.safetensors"
    assert lens._concept_db_path(cv, crop=True, crop_th=0.0, kernel_size=1).name == plain.stem + "-crop-th0-k1.safetensors"


def test_crop_arguments_are_refused_before_any_work(tmp_path):
    cv = _cv(tmp_path)
    lens = Lens(FakeVLM(img_numel=3 * 12 * 12), device="cpu")
    with pytest.raises(ValueError, match="kernel_size"):
        lens.compute_concept_db(cv, crop=True, kernel_size=4)
    with pytest.raises(ValueError, match="crop_th"):
        lens.compute_concept_db(cv, crop=True, crop_th=1.0)
    with pytest.raises(ValueError, match="kernel_size"):
        cv._compute_concept_db(lens.fm, crop=True, kernel_size=256)
    assert not any(cv.storage_dir.rglob("*.safetensors"))  # nothing ran, nothing was written
