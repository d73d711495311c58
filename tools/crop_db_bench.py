"""K14 / cropped concept-DB measurements (GPU only), one JSON line per measurement:

* ``k14``: sl_activation_heat_boxes at P = 256 pairs of a 14 x 14 map, 224 x 224, kernel_size 51, against K13
  (sl_render_heatmaps, crop style) on the same heat; sl_heat_boxes on that heat;
* ``roi_preprocess``: DevicePreprocess.crops of 256 pairs over 64 unique 224 x 224 images;
* ``crop_db``: the cropped concept DB of synth ResNet-50 ``layer2``-``layer4``, k = 20, after ``run()``, through synth
  CLIP ViT-B/32 behind NativeClip with device preprocessing.  Wall time of the whole build (no extra synchronisation),
  then a second build with each stage synchronised and timed: K14 (in the forward hooks), ROI preprocessing, encode;
  what remains is the forward of the referenced samples plus host work (sample loading, box scaling, planning).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import synth  # noqa: E402
from semanticlens_amd import _native as N  # noqa: E402
from semanticlens_amd.component_visualization import ActivationComponentVisualizer, aggregators  # noqa: E402
from semanticlens_amd.component_visualization import crop_db  # noqa: E402
from semanticlens_amd.foundation_models import DevicePreprocess  # noqa: E402
from semanticlens_amd.foundation_models.native_clip import NativeClip  # noqa: E402

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


class _Tensors(torch.utils.data.Dataset):
    def __init__(self, x, name, hwc=False):
        self.x, self.name, self.hwc = x, name, hwc

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i].numpy() if self.hwc else (self.x[i], 0)


def bench_kernels(iters):
    S, P, k = 224, 256, 51
    g = torch.Generator(device=DEV).manual_seed(0)
    act = torch.randn(P, 64, 14, 14, device=DEV, generator=g)
    rows = torch.arange(P)
    chans = torch.randint(0, 64, (P,), generator=torch.Generator().manual_seed(0))
    heat, _ = N.activation_heat_boxes(act, rows, chans, (S, S), k, 0.01, want_heat=True)
    img = torch.rand(P, 3, S, S, device=DEV, generator=g)
    ms14 = timed(lambda: N.activation_heat_boxes(act, rows.to(DEV), chans.to(DEV), (S, S), k, 0.01), iters)
    ms14h = timed(lambda: N.activation_heat_boxes(act, rows.to(DEV), chans.to(DEV), (S, S), k, 0.01, want_heat=True), iters)
    msh = timed(lambda: N.heat_boxes(heat, k, 0.01), iters)
    ms13 = timed(lambda: N.render_heatmaps(heat[:, None], img, "crop", k, 0.02, 0.01, 0.4, False), iters)
    print(json.dumps({"what": "k14", "P": P, "map": "14x14", "H": S, "W": S, "kernel_size": k,
                      "activation_heat_boxes_us": round(ms14 * 1e3, 1), "with_heat_us": round(ms14h * 1e3, 1),
                      "heat_boxes_us": round(msh * 1e3, 1), "k13_crop_us": round(ms13 * 1e3, 1),
                      "k14_over_k13": round(ms14 / ms13, 3)}), flush=True)
    u8 = synth.synth_images_u8(torch.arange(64, device=DEV), S).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    items = list(u8)
    rng = np.random.default_rng(0)
    idx = rng.integers(0, 64, P)
    r1 = rng.integers(0, 150, P)
    c1 = rng.integers(0, 150, P)
    side = rng.integers(20, 74, P)
    boxes = np.stack([r1, r1 + side, c1, c1 + side], 1).astype(np.int32)
    pp = DevicePreprocess(S, device=DEV)
    ms = timed(lambda: pp.crops(items, boxes, idx), iters)
    print(json.dumps({"what": "roi_preprocess", "pairs": P, "unique_images": 64, "size": S, "ms": round(ms, 3),
                      "pairs_per_s": round(P / ms * 1e3, 1)}), flush=True)


def bench_crop_db(n, k, batch_size):
    u8 = synth.synth_images_u8(torch.arange(n, device=DEV), 224)
    x = synth.normalize_u8(u8, synth.IMAGENET_MEAN, synth.IMAGENET_STD).cpu()
    hwc = u8.permute(0, 2, 3, 1).contiguous().cpu()
    model = synth.resnet50().to(DEV).eval()
    layers = ["layer2", "layer3", "layer4"]
    cv = ActivationComponentVisualizer(model, _Tensors(x, f"synth-{n}"), _Tensors(hwc, f"synth-fm-{n}", hwc=True), layers, num_samples=k,
                                       aggregate_fn=aggregators.aggregate_conv_max, device=DEV)
    t0 = time.perf_counter()
    cv.run(batch_size=256)
    torch.cuda.synchronize()
    t_run = time.perf_counter() - t0
    fm = NativeClip(synth.SyntheticClip(device=DEV), preprocess=DevicePreprocess(224, synth.CLIP_MEAN, synth.CLIP_STD))
    refs = {name: cv.get_max_reference(name) for name in layers}
    pairs = sum(int((r >= 0).sum()) for r in refs.values())
    uniq = int(torch.unique(torch.cat([r.reshape(-1) for r in refs.values()])).numel())
    cv._compute_concept_db(fm, batch_size=batch_size, crop=True, kernel_size=51, crop_th=0.01)  # warm-up (kernels, allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    db = cv._compute_concept_db(fm, batch_size=batch_size, crop=True, kernel_size=51, crop_th=0.01, keep_on_device=True)
    torch.cuda.synchronize()
    t_total = time.perf_counter() - t0
    # second build with each stage synchronised and timed
    acc = {"k14": 0.0, "roi_preprocess": 0.0, "encode": 0.0}

    def wrap(fn, key):
        def inner(*a, **kw):
            torch.cuda.synchronize()
            s = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            acc[key] += time.perf_counter() - s
            return out

        return inner

    orig_k14, orig_crops, orig_enc = N.activation_heat_boxes, DevicePreprocess.crops, fm.encode_image
    N.activation_heat_boxes = wrap(orig_k14, "k14")
    DevicePreprocess.crops = wrap(orig_crops, "roi_preprocess")
    fm.encode_image = wrap(orig_enc, "encode")
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cv._compute_concept_db(fm, batch_size=batch_size, crop=True, kernel_size=51, crop_th=0.01, keep_on_device=True)
        torch.cuda.synchronize()
        t_staged = time.perf_counter() - t0
    finally:
        N.activation_heat_boxes, DevicePreprocess.crops = orig_k14, orig_crops
        del fm.encode_image
    rest = t_staged - sum(acc.values())
    print(json.dumps({"what": "crop_db", "model": "resnet50 layer2-4", "fm": "synth clip vit-b/32 (NativeClip, device preprocess)",
                      "dataset": n, "k": k, "batch_size": batch_size, "forward_chunk": crop_db.FORWARD_CHUNK, "pairs": pairs,
                      "unique_samples": uniq, "run_s": round(t_run, 3), "crop_db_s": round(t_total, 3),
                      "pairs_per_s": round(pairs / t_total, 1), "staged_s": round(t_staged, 3),
                      "stages_s": {"forward_and_host": round(rest, 3), **{kk: round(v, 3) for kk, v in acc.items()}},
                      "k14_and_roi_share": round((acc["k14"] + acc["roi_preprocess"]) / t_staged, 4),
                      "shape": {name: list(t.shape) for name, t in db.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip", default="", help="comma list of sections to skip: kernels,db")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    if "kernels" not in skip:
        bench_kernels(args.iters)
    if "db" not in skip:
        bench_crop_db(args.dataset, args.k, args.batch_size)


if __name__ == "__main__":
    main()
