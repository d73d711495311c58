"""Utilities (reference: utils/__init__.py:16-24).  ``to_transforms_compose`` (a torchvision preset converter) is not
provided: torchvision is not a dependency."""
from semanticlens_amd.utils.helper import get_denormalization_transform, get_fallback_name
from semanticlens_amd.utils.log_setup import setup_colored_logging
from semanticlens_amd.utils.render import crop_and_mask_images, vis_lighten_img_border, vis_opaque_img_border

__all__ = ["get_fallback_name", "get_denormalization_transform", "setup_colored_logging", "crop_and_mask_images",
           "vis_opaque_img_border", "vis_lighten_img_border"]
