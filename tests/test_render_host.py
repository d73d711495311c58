"""CPU-only tests (-m "not gpu") of the K13 surface: argument validation of sl_render_heatmaps / sl_condition_init without a
device, the reference's ValueError texts of utils.render, and the two forms of RelevanceComponentVisualizer.get_max_reference."""
import ctypes
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import TensorDataset

from semanticlens_amd import _native as N
from semanticlens_amd.component_visualization import RelevanceComponentVisualizer
from semanticlens_amd.utils import crop_and_mask_images, vis_lighten_img_border, vis_opaque_img_border

FAKE = 1  # a non-null pointer that is never dereferenced: validation runs before any launch


def _render(B=2, Cin=3, H=32, W=32, k=51, vis_th=0.02, crop_th=0.01, alpha=0.4, style=0, rf=1, rel=FAKE, img=FAKE, box=FAKE,
            flags=FAKE, rgb=FAKE, ws=FAKE, ws_bytes=1 << 30):
    return N.lib().sl_render_heatmaps(rel, B, Cin, H, W, img, k, vis_th, crop_th, alpha, style, rf, None, box, flags, rgb, ws,
                                      ws_bytes, None)


def test_render_entry_points_are_declared():
    for name in ("sl_render_heatmaps", "sl_render_ws_bytes", "sl_condition_init"):
        assert name in N.SIGNATURES
        assert hasattr(N.lib(), name)
    assert N.lib().sl_render_ws_bytes(256, 224, 224) == 256 * 2 * 224 * 224 * 4


def test_render_rejects_bad_arguments_without_a_device():
    lib = N.lib()
    for kw in ({"rel": None}, {"img": None}, {"box": None}, {"flags": None}, {"rgb": None}, {"ws": None}):
        assert _render(**kw) == -1
        assert lib.sl_last_error() == b"sl_render_heatmaps: null pointer"
    assert _render(k=50) == -1
    assert b"kernel_size must be an odd positive integer, got 50" in lib.sl_last_error()
    assert _render(k=0) == -1
    # torch's reflect pad needs pad < dim: 26 x 26 is the smallest plane kernel_size 51 accepts
    assert _render(H=25, W=40) == -1
    assert b"kernel_size // 2 = 25 must be smaller than H and W (25 x 40)" in lib.sl_last_error()
    assert _render(H=40, W=25) == -1
    assert _render(H=26, W=26, B=0) == 0  # valid, nothing to launch
    assert _render(H=10, W=37, k=7, B=0) == 0
    for alpha in (-0.1, 1.01):
        assert _render(alpha=alpha) == -1 and lib.sl_last_error() == b"'alpha' must be between [0, 1]"
    assert _render(alpha=1.0, B=0) == 0 and _render(alpha=0.0, B=0) == 0
    for vis_th in (-0.01, 1.0, float("nan")):
        assert _render(vis_th=vis_th) == -1 and lib.sl_last_error() == b"'vis_th' must be between [0, 1)"
    for crop_th in (-0.5, 1.0):
        assert _render(crop_th=crop_th) == -1 and lib.sl_last_error() == b"'crop_th' must be between [0, 1)"
    assert _render(style=3) == -1 and b"unknown style 3" in lib.sl_last_error()
    assert _render(ws_bytes=16) == -1 and b"workspace too small" in lib.sl_last_error()
    assert _render(k=257, H=300, W=300) == -3 and b"exceeds the supported maximum" in lib.sl_last_error()
    # the limits themselves: W + kernel_size - 1 = 16384 fills the LDS tile; kernel_size 255 needs a 128 x 128 plane
    assert _render(H=2, W=16382, k=3, B=0) == 0
    assert _render(H=2, W=16383, k=3) == -3 and b"exceeds the supported maximum" in lib.sl_last_error()
    assert _render(H=128, W=128, k=255, B=0) == 0
    assert _render(H=127, W=128, k=255) == -1 and b"kernel_size // 2 = 127 must be smaller than H and W (127 x 128)" in lib.sl_last_error()


def test_condition_init_rejects_bad_arguments_without_a_device():
    lib = N.lib()
    assert lib.sl_condition_init(None, 2, 3, 4, 12, 4, 1, FAKE, 1, FAKE, 12, 4, 1, None) == -1
    assert lib.sl_last_error() == b"sl_condition_init: null pointer"
    assert lib.sl_condition_init(FAKE, 2, 3, 4, 12, 4, 1, None, 1, FAKE, 12, 4, 1, None) == -1
    assert lib.sl_condition_init(FAKE, 2, 3, 4, 12, 4, 1, FAKE, 1, None, 12, 4, 1, None) == -1
    assert lib.sl_condition_init(FAKE, 2, 0, 4, 12, 4, 1, FAKE, 1, FAKE, 12, 4, 1, None) == -1
    assert b"bad shape" in lib.sl_last_error()
    assert lib.sl_condition_init(FAKE, 0, 3, 4, 12, 4, 1, FAKE, 1, FAKE, 12, 4, 1, None) == 0


@pytest.mark.parametrize("fn", [crop_and_mask_images, vis_opaque_img_border, vis_lighten_img_border])
def test_render_functions_raise_the_reference_texts_before_touching_a_device(fn):
    x, h = torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8)
    with pytest.raises(ValueError, match=r"^'alpha' must be between \[0, 1\]$"):
        fn(x, h, alpha=1.5)
    with pytest.raises(ValueError, match=r"^'alpha' must be between \[0, 1\]$"):
        fn(x, h, alpha=-0.5, vis_th=2.0)  # alpha is checked first, as in the reference
    with pytest.raises(ValueError, match=r"^'vis_th' must be between \[0, 1\)$"):
        fn(x, h, vis_th=1.0)
    with pytest.raises(ValueError, match=r"^'crop_th' must be between \[0, 1\)$"):
        fn(x, h, crop_th=-0.1)


def test_render_function_defaults_follow_the_reference():
    import inspect

    want = {crop_and_mask_images: False, vis_opaque_img_border: True, vis_lighten_img_border: False}
    for fn, rf in want.items():
        p = inspect.signature(fn).parameters
        assert list(p) == ["data_batch", "heatmaps", "rf", "alpha", "vis_th", "crop_th", "kernel_size"]
        assert (p["rf"].default, p["alpha"].default, p["vis_th"].default, p["crop_th"].default, p["kernel_size"].default) == (
            rf, 0.4, 0.02, 0.01, 51)


def test_lighten_with_nothing_to_render_raises_the_reference_assertion():
    with pytest.raises(AssertionError, match="No masking or cropping was applied"):
        vis_lighten_img_border(torch.zeros(0, 3, 8, 8), torch.zeros(0, 8, 8))
    assert crop_and_mask_images(torch.zeros(0, 3, 8, 8), torch.zeros(0, 8, 8)) == []


@pytest.fixture
def relevance_cv():
    model = nn.Sequential(nn.Conv2d(3, 4, 3), nn.ReLU(), nn.Flatten(), nn.LazyLinear(2))
    model.name = "mock_model"
    ds = TensorDataset(torch.randn(4, 3, 8, 8), torch.zeros(4))
    ds.name = "mock_dataset"
    return RelevanceComponentVisualizer(model, ds, ds, ["0"], num_samples=3, cache_dir=None)


def test_get_max_reference_dispatches_both_forms(relevance_cv):
    cv = relevance_cv
    assert cv.plot_fn is crop_and_mask_images and cv.denormalize is None
    assert "plot_fn" not in cv.metadata and "denormalize" not in cv.metadata
    with mock.patch.object(RelevanceComponentVisualizer, "_max_reference_ids", return_value="ids") as ids, \
            mock.patch.object(RelevanceComponentVisualizer, "_max_reference_images", return_value="images") as imgs:
        # the package's own forms: a layer name first
        assert cv.get_max_reference("0") == "ids"
        assert cv.get_max_reference("0", mode="activation") == "ids"
        assert cv.get_max_reference("0", "activation") == "ids"
        assert cv.get_max_reference(layer_name="0") == "ids"
        assert cv.get_act_max_sample_ids("0") == "ids"
        assert imgs.call_count == 0 and ids.call_count == 5
        # the reference's form: an int or a list of ints first
        for args, kwargs in (((0, "0", 3), {}), (([0, 2], "0", 3), {"batch_size": 4}), ((np.int64(1), "0", 2), {}),
                             ((), {"concept_ids": [1], "layer_name": "0", "n_ref": 2}), ((torch.tensor([0, 1]), "0", 1), {})):
            assert cv.get_max_reference(*args, **kwargs) == "images"
        assert imgs.call_count == 5 and ids.call_count == 5


def test_get_max_reference_ids_path_is_unchanged(relevance_cv):
    with pytest.raises(ValueError, match="not found in model layers"):
        relevance_cv.get_max_reference("2")
    with pytest.raises(ValueError, match="not found in model layers"):
        relevance_cv.get_max_reference("2", mode="activation")


def test_compute_heatmaps_refuses_before_running(relevance_cv):
    with pytest.raises(ValueError, match="mode must be"):
        relevance_cv.compute_heatmaps([0], "0", 2, mode="bogus")
    with pytest.raises(RuntimeError, match="call run"):
        relevance_cv.compute_heatmaps([0], "0", 2)


def test_callable_attribution_cannot_be_conditioned():
    from semanticlens_amd.component_visualization.lrp import conditional_input_relevance

    model = nn.Sequential(nn.Conv2d(3, 2, 3))
    with pytest.raises(NotImplementedError, match="layer relevance only"):
        conditional_input_relevance(model, model[0], torch.zeros(1, 3, 5, 5), [0], composite=lambda *a: None)
