"""Reference-sample rendering (reference: ``utils/render.py``) on K13.

The reference renders each image on the host: torchvision's ``gaussian_blur`` (a full 2-D convolution), crp's crop range,
zennit's ``imgify`` and a per-pixel Python loop of Pillow ellipses (``mystroke``).  Here one kernel launch renders the
whole batch on the device (``sl_render_heatmaps``, rules in DESIGN.md §K13); the only host step is slicing each canvas to
its box and ``Image.fromarray``.  Same signatures, defaults and error texts as the reference:

* ``crop_and_mask_images`` (``render.py:270-341``): crop to the square box of the blurred, normalised heat, no composite;
* ``vis_opaque_img_border`` (``:146-222``): darken below ``vis_th`` (x ``alpha``), crop when ``rf``, black stroke;
* ``vis_lighten_img_border`` (``:36-143``): lighten below ``vis_th`` toward white, crop when ``rf``, black stroke; raises
  ``AssertionError`` when no image of the batch has a masked pixel.

``data_batch`` (B, 3, H, W) display-space images and ``heatmaps`` (B, H, W) may be tensors on any device (or sequences of
per-image tensors); they are moved to the HIP device for the kernel.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch
from PIL import Image

from semanticlens_amd import _native as N

__all__ = ["crop_and_mask_images", "vis_opaque_img_border", "vis_lighten_img_border"]

_NOTHING_MASKED = ("No masking or cropping was applied to any image in the batch. "
                   "This may indicate that the visibility threshold (vis_th) is too high "
                   "or that there's an issue with the heatmaps.")


def _validate(alpha, vis_th, crop_th):
    # the reference's checks and texts, in its order (render.py:92-97)
    if alpha > 1 or alpha < 0:
        raise ValueError("'alpha' must be between [0, 1]")
    if vis_th >= 1 or vis_th < 0:
        raise ValueError("'vis_th' must be between [0, 1)")
    if crop_th >= 1 or crop_th < 0:
        raise ValueError("'crop_th' must be between [0, 1)")


def _as_batch(x) -> torch.Tensor:
    if torch.is_tensor(x):
        return x
    return torch.stack([torch.as_tensor(t) for t in x]) if len(x) else torch.empty(0)


def _render(style, data_batch, heatmaps, rf, alpha, vis_th, crop_th, kernel_size):
    _validate(alpha, vis_th, crop_th)
    imgs, heat = _as_batch(data_batch), _as_batch(heatmaps)
    if len(imgs) == 0:
        return [], 0
    if imgs.ndim != 4 or imgs.shape[1] != 3 or heat.ndim != 3 or heat.shape[0] != imgs.shape[0] or heat.shape[1:] != imgs.shape[2:]:
        raise ValueError(f"expected data_batch (B, 3, H, W) and heatmaps (B, H, W), got {tuple(imgs.shape)} and {tuple(heat.shape)}")
    dev = heat.device if heat.is_cuda else (imgs.device if imgs.is_cuda else N.default_device())
    imgs = imgs.detach().to(dev, torch.float32)
    heat = heat.detach().to(dev, torch.float32).unsqueeze(1)
    _, box, flags, rgb = N.render_heatmaps(heat, imgs, style, kernel_size, vis_th, crop_th, alpha, rf)
    box, flags, rgb = box.cpu().numpy(), flags.cpu().numpy(), rgb.cpu().numpy()
    H, W = imgs.shape[2:]
    out = []
    for i in range(len(rgb)):
        h, w = H, W
        if flags[i] & 1:
            r1, r2, c1, c2 = (int(v) for v in box[i])
            h, w = max(min(r2, H) - r1, 0), max(min(c2, W) - c1, 0)
        if h == 0 or w == 0:  # the reference's imgify fails on an empty crop as well
            raise ValueError(f"the crop box of image {i} is empty: {tuple(int(v) for v in box[i])}")
        out.append(Image.fromarray(np.ascontiguousarray(rgb[i, :h, :w])))
    return out, int((flags & 2).any())


@torch.no_grad()
def crop_and_mask_images(data_batch, heatmaps, rf=False, alpha=0.4, vis_th=0.02, crop_th=0.01, kernel_size=51):
    """Each image cropped to the square box of its blurred heatmap (``rf`` is unused, as in the reference) -> list of RGB
    ``PIL.Image``."""
    return _render("crop", data_batch, heatmaps, rf, alpha, vis_th, crop_th, kernel_size)[0]


@torch.no_grad()
def vis_opaque_img_border(data_batch, heatmaps, rf=True, alpha=0.4, vis_th=0.02, crop_th=0.01, kernel_size=51):
    """Pixels below ``max * vis_th`` of the blurred heatmap darkened (x ``alpha``), the masked region outlined in black,
    cropped to the square box when ``rf`` -> list of RGB ``PIL.Image`` (shapes differ when cropped)."""
    return _render("opaque", data_batch, heatmaps, rf, alpha, vis_th, crop_th, kernel_size)[0]


@torch.no_grad()
def vis_lighten_img_border(data_batch, heatmaps, rf=False, alpha=0.4, vis_th=0.02, crop_th=0.01, kernel_size=51):
    """Pixels below ``max * vis_th`` of the blurred heatmap lightened toward white (``alpha``), the masked region outlined
    in black, cropped when ``rf`` -> list of RGB ``PIL.Image``.  ``AssertionError`` when no image has a masked pixel."""
    imgs, any_masked = _render("lighten", data_batch, heatmaps, rf, alpha, vis_th, crop_th, kernel_size)
    if not any_masked:
        raise AssertionError(_NOTHING_MASKED)
    return imgs
