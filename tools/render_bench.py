"""K13 measurements (GPU only), one JSON line per measurement:

* ``k13``: sl_render_heatmaps at B=256, 224 x 224, kernel_size 51, relevance (B, 3, H, W), per style; us per batch and
  algorithmic bytes (relevance + images read, canvas written) / time against the measured device copy ceiling;
* ``reference_way``: the same work the reference's way — torchvision's blur as F.conv2d with the 2-D kernel on the device
  (timed over the batch), then per image on the host the normalisation, crop box, composite, imgify and the Pillow
  stroke loop (timed on ``--host-images`` images and scaled to the batch);
* ``compute_heatmaps``: 64 channels x 20 references of ResNet-50 ``layer4`` at 224 x 224 in batches of 32: the LRP
  (epsilon_plus_flat) forward + conditional backward and K13 (crop style) timed separately.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image, ImageDraw, ImageFilter

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import synth  # noqa: E402
from semanticlens_amd import _native as N  # noqa: E402
from semanticlens_amd.component_visualization.lrp import conditional_input_relevance  # noqa: E402

DEV = "cuda:0"


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def copy_ceiling():
    src = torch.empty(1 << 28, dtype=torch.float32, device=DEV)  # 1 GiB
    dst = torch.empty_like(src)
    ms = timed(lambda: dst.copy_(src), 10)
    return 2 * src.numel() * 4 / ms / 1e6  # GB/s, read + write


def host_chain(heat_blurred, img, style, alpha=0.4, vis_th=0.02, crop_th=0.01):
    """The reference's per-image host steps after the blur (numpy + Pillow), for timing only."""
    a = np.abs(heat_blurred)
    norm = a / (a.max() + (0 if style == "crop" else 1e-8))
    rows, cols = np.nonzero(norm > crop_th)
    H, W = norm.shape
    r1, r2, c1, c2 = (rows.min(), rows.max(), cols.min(), cols.max()) if len(rows) else (0, H, 0, W)
    dr, dc = r2 - r1, c2 - c1
    if dr > dc:
        c1, c2 = max(c1 - (dr - dc) // 2, 0), c2 + (dr - dc) // 2
    elif dc > dr:
        r1, r2 = max(r1 - (dc - dr) // 2, 0), r2 + (dc - dr) // 2
    mask = norm > vis_th
    if style == "crop" or (img[:, r1:r2, c1:c2].sum() != 0 and mask[r1:r2, c1:c2].sum() != 0):
        img, mask = img[:, r1:r2, c1:c2], mask[r1:r2, c1:c2]
    if style != "crop":
        img = img * mask + img * ~mask * alpha
    x = img.transpose(1, 2, 0)
    u8 = ((x - x.min()) / (x.max() - x.min()) * 255).clip(0, 255).astype(np.uint8)
    out = Image.fromarray(u8).convert("RGBA")
    if style == "crop":
        return out.convert("RGB")
    arr = np.array(out)
    arr[..., 3] = mask * 255
    top = Image.fromarray(arr)
    edge = top.filter(ImageFilter.FIND_EDGES).load()
    stroke = Image.new("RGBA", top.size, (0, 0, 0, 0))
    draw = ImageDraw.Draw(stroke)
    for xx in range(top.size[0]):  # the reference's per-pixel loop
        for yy in range(top.size[1]):
            if edge[xx, yy][3] > 0:
                draw.ellipse((xx - 1, yy - 1, xx + 1, yy + 1), fill=(0, 0, 0, 180))
    stroke.paste(top, (0, 0), top)
    out.paste(stroke, (0, 0), stroke)
    return out.convert("RGB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-images", type=int, default=8)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--refs", type=int, default=20)
    ap.add_argument("--skip", default="", help="comma list of sections to skip: k13,reference,heatmaps")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    B, S, k = args.batch, args.size, 51
    g = torch.Generator(device=DEV).manual_seed(0)
    rel = torch.randn(B, 3, S, S, device=DEV, generator=g)
    img = torch.rand(B, 3, S, S, device=DEV, generator=g)
    if "k13" not in skip:
        ceiling = copy_ceiling()
        print(json.dumps({"what": "copy_ceiling", "GBps": round(ceiling, 1)}), flush=True)
        nbytes = rel.numel() * 4 + img.numel() * 4 + B * S * S * 3
        for style, rf in (("crop", False), ("opaque", True), ("lighten", False)):
            ms = timed(lambda: N.render_heatmaps(rel, img, style, k, 0.02, 0.01, 0.4, rf), args.iters)
            print(json.dumps({"what": "k13", "style": style, "B": B, "H": S, "W": S, "kernel_size": k, "us_per_batch": round(ms * 1e3, 1),
                              "alg_bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1), "of_copy_ceiling": round(nbytes / ms / 1e6 / ceiling, 4)}),
                  flush=True)
    if "reference" not in skip:
        sigma = 0.15 * k + 0.35
        x = torch.linspace(-(k - 1) * 0.5, (k - 1) * 0.5, k)
        g1 = torch.exp(-0.5 * (x / sigma).pow(2))
        g1 = g1 / g1.sum()
        k2 = torch.mm(g1[:, None], g1[None, :]).to(DEV)[None, None]
        heat = rel.sum(1, keepdim=True)
        blur = lambda: F.conv2d(F.pad(heat, (k // 2,) * 4, mode="reflect"), k2)  # noqa: E731
        ms_blur = timed(blur, max(args.iters // 4, 2))
        bl = blur()[:, 0].cpu().numpy()
        im = img.cpu().numpy()
        for style in ("crop", "opaque"):
            t0 = time.perf_counter()
            for i in range(args.host_images):
                host_chain(bl[i], im[i], style)
            per_img = (time.perf_counter() - t0) / args.host_images
            print(json.dumps({"what": "reference_way", "style": style, "B": B, "device_conv2d_blur_ms": round(ms_blur, 3),
                              "host_ms_per_image": round(per_img * 1e3, 2), "host_images_timed": args.host_images,
                              "batch_ms_estimate": round(ms_blur + per_img * 1e3 * B, 1)}), flush=True)
    if "heatmaps" not in skip:
        model = synth.resnet50().to(DEV)
        module = model.layer4
        n_pairs, bs = args.channels * args.refs, 32
        imgs = torch.randn(bs, 3, S, S, device=DEV, generator=g)
        chans = [c for c in range(args.channels) for _ in range(args.refs)]
        t_lrp = t_k13 = 0.0
        for warm in (True, False):
            t_lrp = t_k13 = 0.0
            for s in range(0, n_pairs if not warm else bs, bs):
                ch = chans[s:s + bs]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = conditional_input_relevance(model, module, imgs[:len(ch)], ch, rf=True, composite="epsilon_plus_flat")
                h = r.sum(1)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                N.render_heatmaps(h[:, None], imgs[:len(ch)].clamp(0, 1), "crop", k, 0.02, 0.01, 0.4, False)
                torch.cuda.synchronize()
                t_lrp += t1 - t0
                t_k13 += time.perf_counter() - t1
        print(json.dumps({"what": "compute_heatmaps", "model": "resnet50 layer4", "pairs": n_pairs, "batch_size": bs, "H": S,
                          "lrp_fwd_bwd_s": round(t_lrp, 3), "k13_s": round(t_k13, 4), "total_s": round(t_lrp + t_k13, 3),
                          "k13_share": round(t_k13 / (t_lrp + t_k13), 4)}), flush=True)


if __name__ == "__main__":
    main()
