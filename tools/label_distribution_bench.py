"""K25 measurement: the streaming softmax statistics (``sl_softmax_merge``) against K20 (``sl_mutualmax_merge``) on the same
tile, the split-row regime, and ``probe_softmax`` against ``probe_topk`` end to end.

Kernel part.  One fp32 tile of 8 192 rows by 32 768 and by 2 048 columns, uniform values in [-1, 1], logit scale 100.
``sl_softmax_merge`` and ``sl_mutualmax_merge`` — K20 as it stands, which reads the same bytes — on the same tile in the same
process, alternating.  Times are the library's per-dispatch event times (``sl_prof_*``, the dispatch's own begin / end
timestamps), the mean over ``--launches`` launches per block; ``--blocks`` blocks give the median and the spread.  The bar is the
one K22 and K24 were held to: at most 1.10 of K20's time.  Rates are tile bytes over time.

Split rows.  4 rows of 524 288 columns: the tile launch and the fold of the partial states, both in K25's family (two dispatches
per merge).

End to end.  ``lens.probe_softmax`` against ``lens.probe_topk`` (what ``label_components`` runs) at k = 5 on the two shapes of
DESIGN.md §K17's table, 100 000 word vectors: HIP-event time of whole calls, alternating, and the GEMM / K17 / K25 split from
the library's events in a pass of its own.  ``--scale`` divides the sizes for a rehearsal; a figure taken below the default size
is a figure of overheads.

    python tools/label_distribution_bench.py [--out profiles/k25_label_distribution_bench.txt]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from semanticlens_amd import _native as N  # noqa: E402
from semanticlens_amd import lens as L  # noqa: E402

COPY_CEILING = 6.29e12
SCALE = 100.0
SHAPES = {"rn50_clip": (3584, 512), "so400m_siglip": (30000, 1152)}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def dispatch_ms(fn, launches: int, family: int, per_call: int = 1) -> float:
    """Mean time per call of ``launches`` calls of ``fn`` under the library's events (``per_call`` dispatches each)."""
    N.prof_enable(True)
    N.prof_reset()
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    ms, n, _ = N.prof_read(family)
    N.prof_enable(False)
    assert n == launches * per_call, (n, launches, per_call)
    return ms / launches


def median(xs):
    return sorted(xs)[len(xs) // 2]


def kernel_part(say, dev, R: int, B: int, launches: int, blocks: int):
    tile = torch.rand(R, B, device=dev) * 2 - 1
    nbytes = R * B * 4
    row_state = torch.zeros(R, dtype=torch.int64, device=dev)
    col_state = torch.zeros(B, dtype=torch.int64, device=dev)
    sm = N.softmax_new(R, dev)
    split = int(N.lib().sl_softmax_merge_ws_bytes(R, B)) > 0
    ws = torch.empty(max(int(N.lib().sl_softmax_merge_ws_bytes(R, B)), 1), dtype=torch.uint8, device=dev)
    variants = {
        "k20": (lambda: N.mutualmax_merge(row_state, col_state, tile), N.SL_PROF_TOPK, 1),
        "k25": (lambda: N.softmax_merge(sm, tile, SCALE, ws), N.SL_PROF_SOFTMAX, 2 if split else 1),
    }
    for fn, _, _ in variants.values():  # warm-up: code objects; K20's states reach their final values
        fn(), fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(blocks):
        for name, (fn, family, per_call) in variants.items():
            times[name].append(dispatch_ms(fn, launches, family, per_call))
    k20, k25 = median(times["k20"]), median(times["k25"])
    say(json.dumps({
        "part": "kernel", "tile": [R, B], "tile_MB": round(nbytes / 1e6, 1), "split_rows": split, "launches_per_block": launches,
        "blocks": blocks, "logit_scale": SCALE,
        "k20_us_median": round(k20 * 1e3, 2), "k20_us_blocks": [round(t * 1e3, 2) for t in times["k20"]],
        "k20_TBps": round(nbytes / (k20 * 1e-3) / 1e12, 3),
        "k25_us_median": round(k25 * 1e3, 2), "k25_us_blocks": [round(t * 1e3, 2) for t in times["k25"]],
        "k25_TBps": round(nbytes / (k25 * 1e-3) / 1e12, 3),
        "k25_fraction_of_copy_ceiling": round(nbytes / (k25 * 1e-3) / COPY_CEILING, 3),
        "k25_over_k20": round(k25 / k20, 3), "bar": 1.10,
    }))


def profiled(fn):
    N.prof_enable(True)
    N.prof_reset()
    fn()
    torch.cuda.synchronize()
    out = {name: N.prof_read(family) for name, family in (("gemm", N.SL_PROF_GEMM), ("k17", N.SL_PROF_TOPK), ("k25", N.SL_PROF_SOFTMAX))}
    N.prof_enable(False)
    return out


def end_to_end(say, dev, name: str, C: int, D: int, V: int, k: int, reps: int):
    g = torch.Generator(device="cpu").manual_seed(0)
    db = torch.randn(C, D, generator=g).to(dev)
    words = torch.randn(V, D, generator=g).to(dev)
    old = lambda: L.probe_topk(words, db, k)
    new = lambda: L.probe_softmax(words, db, k, logit_scale=SCALE)
    old(), new()
    torch.cuda.synchronize()
    t_old, t_new = [], []
    for _ in range(reps):
        ms, (ov, oi) = event_ms(old)
        t_old.append(ms)
        ms, (nv, ni, probs, lz, h) = event_ms(new)
        t_new.append(ms)
    p = profiled(new)
    cols = N.topk_chunk_rows(C, V)
    new_ms = median(t_new)
    say(json.dumps({
        "part": "end_to_end", "shape": name, "C": C, "D": D, "V": V, "k": k, "logit_scale": SCALE, "gemm_mode": "bf16x3 (default)",
        "tile_cols": cols, "tiles": -(-V // cols),
        "probe_topk_ms_median": round(median(t_old), 3), "probe_topk_ms_all": [round(t, 3) for t in t_old],
        "probe_softmax_ms_median": round(new_ms, 3), "probe_softmax_ms_all": [round(t, 3) for t in t_new],
        "probe_softmax_over_probe_topk": round(new_ms / median(t_old), 3),
        "gemm_ms": round(p["gemm"][0], 3), "k17_ms": round(p["k17"][0], 3), "k17_launches": p["k17"][1],
        "k25_ms": round(p["k25"][0], 3), "k25_launches": p["k25"][1], "k25_share_of_call": round(p["k25"][0] / new_ms, 4),
        "k25_TBps": round(C * V * 4 / (p["k25"][0] * 1e-3) / 1e12, 3) if p["k25"][0] else None,
        "values_and_ids_bit_equal": bool(torch.equal(ov.view(torch.int32), nv.view(torch.int32)) and torch.equal(oi, ni)),
        "mean_top1_prob": round(float(probs[:, 0].mean()), 4), "mean_effective_labels": round(float(h.exp().mean()), 1),
    }))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--part", choices=("all", "kernel", "end_to_end"), default="all")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = N.default_device()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    s = args.scale
    if args.part in ("all", "kernel"):
        for R, B in ((8192 // s, 32768 // s), (8192 // s, 2048 // s), (4, 524288 // s)):
            kernel_part(say, dev, R, B, args.launches, args.blocks)
            torch.cuda.empty_cache()
    if args.part in ("all", "end_to_end"):
        for name, (C, D) in SHAPES.items():
            end_to_end(say, dev, name, C // s, D, 100000 // s, 5, args.reps)
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
