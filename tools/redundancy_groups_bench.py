"""K24 measurement: the threshold-union merge (``sl_threshold_union_merge``) against K20 (``sl_mutualmax_merge``) on the same tile,
and ``redundancy_groups`` end to end against ``mutual_probe(x, x)``.

Kernel part.  One fp32 tile of 8 192 rows by 32 768 and by 2 048 columns, uniform values in [-1, 1), with ids that put the whole
tile right of the diagonal (rows 0.., columns 8 192..), so that both kernels read the same bytes.  K20 as it stands and K24 with
a threshold nothing reaches (2.0) alternate in the same process; times are the library's per-dispatch event times
(``sl_prof_*``), the mean over ``--launches`` launches per block; ``--blocks`` blocks give the median and the spread.  The bar:
K24 with no element at or above the threshold takes at most 1.10 x K20's time.

Then, without a bar, K24 at thresholds that 1e-6, 1e-4, 1e-2 and all of the elements reach (threshold = 1 - 2 f).  "fresh": every
launch starts from the empty forest, so every edge's unite does its work; "steady": the forest of the previous launch is kept, so
every unite finds its two ends joined already and only the degree atomics change memory.  The last fraction is the degenerate
dense case — one group, every degree the other side's size — which is bound by the atomics, not by the read.

End to end.  ``scores.redundancy_groups`` on 98 304 x 768 random unit rows at threshold 0.9 (no edge) against
``_native.mutual_probe(x, x)``, the route to "who duplicates whom" before K24: HIP-event times of whole calls, and the GEMM /
selection split from the library's events in a pass of its own.  ``--scale`` divides the sizes for a rehearsal; a figure taken
below the default size is a figure of overheads.

    python tools/redundancy_groups_bench.py [--out profiles/k24_redundancy_groups_bench.txt]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from semanticlens_amd import _native as N  # noqa: E402
from semanticlens_amd import scores as S  # noqa: E402

COPY_CEILING = 6.29e12
FRACTIONS = (1e-6, 1e-4, 1e-2, 1.0)
BAR = 1.10


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def dispatch_ms(fn, launches: int, before=None) -> float:
    """Mean per-dispatch time of ``launches`` calls of ``fn`` under the library's events (family SL_PROF_TOPK); ``before`` runs
    ahead of every call, outside the events."""
    total = 0.0
    for _ in range(launches):
        if before is not None:
            before()
        N.prof_enable(True)
        N.prof_reset()
        fn()
        torch.cuda.synchronize()
        ms, n, _ = N.prof_read(N.SL_PROF_TOPK)
        N.prof_enable(False)
        assert n == 1
        total += ms
    return total / launches


def profiled(fn):
    N.prof_enable(True)
    N.prof_reset()
    fn()
    torch.cuda.synchronize()
    s_ms, s_n, s_bytes = N.prof_read(N.SL_PROF_TOPK)
    g_ms, g_n, g_flops = N.prof_read(N.SL_PROF_GEMM)
    N.prof_enable(False)
    return g_ms, g_n, g_flops, s_ms, s_n, s_bytes


def median(xs):
    return sorted(xs)[len(xs) // 2]


def kernel_part(say, dev, R: int, B: int, launches: int, blocks: int):
    tile = torch.rand(R, B, device=dev) * 2 - 1
    nbytes = R * B * 4
    n = R + B
    row_state = torch.zeros(R, dtype=torch.int64, device=dev)
    col_state = torch.zeros(B, dtype=torch.int64, device=dev)
    parent, degree, status = N.unionfind_new(n, dev)
    k20 = lambda: N.mutualmax_merge(row_state, col_state, tile)
    k24 = lambda: N.threshold_union_merge(parent, degree, status, tile, 2.0, 0, R)
    for fn in (k20, k24):  # warm-up: code objects, and K20's states reach their final values
        fn(), fn()
    torch.cuda.synchronize()
    times = {"k20": [], "k24": []}
    for _ in range(blocks):
        times["k20"].append(dispatch_ms(k20, launches))
        times["k24"].append(dispatch_ms(k24, launches))
    t20, t24 = median(times["k20"]), median(times["k24"])
    assert int(degree.sum()) == 0 and int(status.item()) == 0
    say(json.dumps({
        "part": "kernel", "tile": [R, B], "tile_MB": round(nbytes / 1e6, 1), "launches_per_block": launches, "blocks": blocks,
        "hit_fraction": 0.0, "k20_us_median": round(t20 * 1e3, 2), "k20_us_blocks": [round(t * 1e3, 2) for t in times["k20"]],
        "k24_us_median": round(t24 * 1e3, 2), "k24_us_blocks": [round(t * 1e3, 2) for t in times["k24"]],
        "k24_over_k20": round(t24 / t20, 3), "bar": BAR, "bar_met": bool(t24 <= BAR * t20),
        "k20_TBps": round(nbytes / (t20 * 1e-3) / 1e12, 3), "k24_TBps": round(nbytes / (t24 * 1e-3) / 1e12, 3),
        "k24_fraction_of_copy_ceiling": round(nbytes / (t24 * 1e-3) / COPY_CEILING, 3),
    }))
    for f in FRACTIONS:
        threshold = 1.0 - 2.0 * f
        few = launches if f < 1.0 else 2  # the dense case takes milliseconds per launch
        merge = lambda: N.threshold_union_merge(parent, degree, status, tile, threshold, 0, R)
        reset = lambda: N.lib().sl_unionfind_init(N._ptr(parent), N._ptr(degree), N._ptr(status), n, N._stream(parent))
        fresh = [dispatch_ms(merge, few, before=reset) for _ in range(blocks)]
        reset(), merge()
        edges, max_degree = int(degree.sum()) // 2, int(degree.max())
        N.unionfind_flatten(parent, status)
        groups = int((parent == torch.arange(n, device=dev, dtype=torch.int32)).sum())
        steady = [dispatch_ms(merge, few) for _ in range(blocks)]
        assert int(status.item()) == 0
        say(json.dumps({
            "part": "kernel", "tile": [R, B], "hit_fraction": f, "threshold": threshold, "edges": edges, "groups_of": n, "groups": groups,
            "max_degree": max_degree,
            "launches_per_block": few, "k24_fresh_us_median": round(median(fresh) * 1e3, 2),
            "k24_fresh_us_blocks": [round(t * 1e3, 2) for t in fresh], "k24_steady_us_median": round(median(steady) * 1e3, 2),
            "k24_steady_us_blocks": [round(t * 1e3, 2) for t in steady],
            "fresh_over_k20": round(median(fresh) / t20, 3), "steady_over_k20": round(median(steady) / t20, 3),
            "fresh_Medges_per_s": round(edges / (median(fresh) * 1e-3) / 1e6, 1),
        }))


def end_to_end(say, dev, C: int, D: int, reps: int):
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.nn.functional.normalize(torch.randn(C, D, generator=g), dim=1).to(dev)
    new = lambda: S.redundancy_groups(x, threshold=0.9)
    old = lambda: N.mutual_probe(x, x)
    new(), old()
    torch.cuda.synchronize()
    t_new, t_old = [], []
    for _ in range(reps):
        ms, groups = event_ms(new)
        t_new.append(ms)
        ms, _ = event_ms(old)
        t_old.append(ms)
    ng_ms, ng_n, ng_flops, ns_ms, ns_n, ns_bytes = profiled(new)
    og_ms, og_n, og_flops, os_ms, os_n, os_bytes = profiled(old)
    rows, cols = N.tile_plan(C, C)
    say(json.dumps({
        "part": "end_to_end", "C": C, "D": D, "threshold": 0.9, "gemm_mode": "bf16x3 (default)", "tile": [rows, cols],
        "tiles": len(list(N.upper_tile_walk(C, rows, cols))), "n_groups": groups.n_groups, "redundant": int(groups.redundant.sum()),
        "redundancy_groups_ms_median": round(median(t_new), 2), "redundancy_groups_ms_all": [round(t, 2) for t in t_new],
        "mutual_probe_ms_median": round(median(t_old), 2), "mutual_probe_ms_all": [round(t, 2) for t in t_old],
        "mutual_probe_over_redundancy_groups": round(median(t_old) / median(t_new), 3),
        "new_gemm_ms": round(ng_ms, 2), "new_gemm_launches": ng_n, "new_gemm_TFLOP": round(ng_flops / 1e12, 2),
        "new_select_ms": round(ns_ms, 2), "new_select_launches": ns_n, "new_select_TBps": round(ns_bytes / (ns_ms * 1e-3) / 1e12, 3) if ns_ms else None,
        "old_gemm_ms": round(og_ms, 2), "old_gemm_launches": og_n, "old_gemm_TFLOP": round(og_flops / 1e12, 2),
        "old_select_ms": round(os_ms, 2), "old_select_launches": os_n, "old_select_TBps": round(os_bytes / (os_ms * 1e-3) / 1e12, 3) if os_ms else None,
    }))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
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
        for B in (32768 // s, 2048 // s):
            kernel_part(say, dev, 8192 // s, B, args.launches, args.blocks)
            torch.cuda.empty_cache()
    if args.part in ("all", "end_to_end"):
        end_to_end(say, dev, 98304 // s, 768, args.reps)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
