"""K26 measurement: the rank count (``sl_rank_merge``) against K25 (``sl_softmax_merge``) on the same tile, the split-row
regime, and ``probe_rank`` against ``probe_topk`` end to end.

Kernel part.  One fp32 tile of 8 192 rows by 32 768 and by 2 048 columns, uniform values in [-1, 1]; the keys are the values of
random columns of the tile, T = 1, 4 and 16 per row.  ``sl_rank_merge`` and ``sl_softmax_merge`` (logit scale 100) — K25 as it
stands, which reads the same bytes — on the same tile in the same process, alternating.  Times are the library's per-dispatch
event times (``sl_prof_*``, the dispatch's own begin / end timestamps), the mean over ``--launches`` launches per block;
``--blocks`` blocks give the median and the spread.  The bar, for T = 1 only, is the one K24 and K25 were held to: at most 1.10
of the neighbour's time.  Rates are tile bytes over time.

Split rows.  4 rows of 524 288 columns: K26 is one dispatch whose waves add their partial counts with integer atomics, K25 two
(the tile launch and the fold of the partial states).

End to end.  ``lens.probe_rank`` with one target per component against ``lens.probe_topk`` at k = 5 (what ``label_components``
runs) on 100 000 word vectors of width 512 against 3 584 components: HIP-event time of whole calls, alternating, and the split
into the key pass (``rank_keys``: its GEMM), the GEMM of the walk and K26 from the library's events in passes of their own.
``--scale`` divides the sizes for a rehearsal; a figure taken below the default size is a figure of overheads.

    python tools/label_rank_bench.py [--out profiles/k26_label_rank_bench.txt]
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
    sm = N.softmax_new(R, dev)
    k25_split = int(N.lib().sl_softmax_merge_ws_bytes(R, B)) > 0
    ws = torch.empty(max(int(N.lib().sl_softmax_merge_ws_bytes(R, B)), 1), dtype=torch.uint8, device=dev)
    variants = {"k25": (lambda: N.softmax_merge(sm, tile, SCALE, ws), N.SL_PROF_SOFTMAX, 2 if k25_split else 1)}
    g = torch.Generator(device="cpu").manual_seed(R + B)
    for T in (1, 4, 16):
        ids = torch.randint(0, B, (R, T), generator=g).to(dev)
        keys = torch.gather(tile, 1, ids).contiguous()
        counts = torch.zeros((R, T), dtype=torch.int64, device=dev)
        variants[f"k26_T{T}"] = (lambda c=counts, k=keys, i=ids: N.rank_merge(c, tile, k, i), N.SL_PROF_TOPK, 1)
    for fn, _, _ in variants.values():  # warm-up: code objects
        fn(), fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(blocks):
        for name, (fn, family, per_call) in variants.items():
            times[name].append(dispatch_ms(fn, launches, family, per_call))
    k25 = median(times["k25"])
    rec = {
        "part": "kernel", "tile": [R, B], "tile_MB": round(nbytes / 1e6, 1), "k26_waves_per_row": int(N.lib().sl_rank_merge_splits(R, B)),
        "k25_split_rows": k25_split, "launches_per_block": launches, "blocks": blocks,
        "k25_us_median": round(k25 * 1e3, 2), "k25_us_blocks": [round(t * 1e3, 2) for t in times["k25"]],
        "k25_TBps": round(nbytes / (k25 * 1e-3) / 1e12, 3),
    }
    for T in (1, 4, 16):
        t = median(times[f"k26_T{T}"])
        rec.update({
            f"k26_T{T}_us_median": round(t * 1e3, 2), f"k26_T{T}_us_blocks": [round(x * 1e3, 2) for x in times[f"k26_T{T}"]],
            f"k26_T{T}_TBps": round(nbytes / (t * 1e-3) / 1e12, 3),
            f"k26_T{T}_fraction_of_copy_ceiling": round(nbytes / (t * 1e-3) / COPY_CEILING, 3),
            f"k26_T{T}_over_k25": round(t / k25, 3),
        })
    rec["bar_T1"] = 1.10
    say(json.dumps(rec))


def profiled(fn):
    N.prof_enable(True)
    N.prof_reset()
    out = fn()
    torch.cuda.synchronize()
    fams = {name: N.prof_read(family) for name, family in (("gemm", N.SL_PROF_GEMM), ("topk", N.SL_PROF_TOPK))}
    N.prof_enable(False)
    return fams, out


def end_to_end(say, dev, C: int, D: int, V: int, k: int, reps: int):
    g = torch.Generator(device="cpu").manual_seed(0)
    db = torch.randn(C, D, generator=g).to(dev)
    words = torch.randn(V, D, generator=g).to(dev)
    targets = torch.randint(0, V, (C, 1), generator=g)
    old = lambda: L.probe_topk(words, db, k)
    new = lambda: L.probe_rank(words, db, targets)
    old(), new()
    torch.cuda.synchronize()
    t_old, t_new = [], []
    for _ in range(reps):
        ms, (ov, oi) = event_ms(old)
        t_old.append(ms)
        ms, r = event_ms(new)
        t_new.append(ms)
    tg = targets.to(dev)
    p_keys, key_vals = profiled(lambda: N.rank_keys(db, words, targets))
    p_walk, _ = profiled(lambda: N.rank_probe(db, words, key_vals, tg))
    # a target inside the top k is listed at its rank; one outside it is listed nowhere
    listed = (oi == tg).int().argmax(dim=1)
    inside = (oi == tg).any(dim=1)
    agree = bool(((r.rank[:, 0] == listed) | ~inside).all() and ((r.rank[:, 0] >= k) | inside).all())
    cols = N.topk_chunk_rows(C, V)
    new_ms = median(t_new)
    say(json.dumps({
        "part": "end_to_end", "C": C, "D": D, "V": V, "targets_per_component": 1, "k_of_probe_topk": k, "gemm_mode": "bf16x3 (default)",
        "tile_cols": cols, "tiles": -(-V // cols),
        "probe_topk_ms_median": round(median(t_old), 3), "probe_topk_ms_all": [round(t, 3) for t in t_old],
        "probe_rank_ms_median": round(new_ms, 3), "probe_rank_ms_all": [round(t, 3) for t in t_new],
        "probe_rank_over_probe_topk": round(new_ms / median(t_old), 3),
        "key_pass_gemm_ms": round(p_keys["gemm"][0], 3), "key_pass_gemm_launches": p_keys["gemm"][1],
        "walk_gemm_ms": round(p_walk["gemm"][0], 3), "k26_ms": round(p_walk["topk"][0], 3), "k26_launches": p_walk["topk"][1],
        "k26_share_of_call": round(p_walk["topk"][0] / new_ms, 4),
        "k26_TBps": round(C * V * 4 / (p_walk["topk"][0] * 1e-3) / 1e12, 3) if p_walk["topk"][0] else None,
        "ranks_agree_with_probe_topk_ids": agree, "targets_inside_top_k": int(inside.sum()),
        "mean_rank": round(float(r.rank.double().mean()), 1), "mrr": round(r.mrr(), 6),
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
        end_to_end(say, dev, 3584 // s, 512, 100000 // s, 5, args.reps)
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
