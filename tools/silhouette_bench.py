"""K23 measurement: what choosing every component's facet count costs, on the 2 048 x 20 x 512 concept-DB layer that
tools/scores_bench.py and tools/facets_bench.py time.

* ``sl_silhouette`` for ``m = 1`` and ``m = 5`` label sets (both metrics), next to one fixed-k ``polysemanticity_score`` (a K9
  run: the same Gram matrices plus the k-means) on the same tensor, the calls alternating.  The kernel calls are timed as
  windows of ``--inner`` back-to-back launches between two HIP events.
* ``polysemanticity_facets(n_clusters="auto", max_clusters=6)`` end to end, next to the five fixed-k
  ``polysemanticity_facets`` calls (k = 2..6) whose clusterings it contains, each timed alone in the same process on the same
  commit, and their sum.

Times are HIP-event times after warm-up; medians of ``--reps`` windows, every window listed.  ``--size`` shrinks the component
count for a rehearsal; a figure taken below the default size is a figure of overheads.

    python tools/silhouette_bench.py [--out profiles/k23_silhouette_bench.txt]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPE = (2048, 20, 512)
MAX_CLUSTERS = 6


def median(xs):
    return sorted(xs)[len(xs) // 2]


def window_ms(torch, fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(torch, fns: dict, reps: int, warmup: int, inner: int) -> dict:
    """All window times (ms per call) of each function, the functions taking turns."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(window_ms(torch, fn, inner))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20, help="launches per timed window of the kernel calls")
    ap.add_argument("--size", type=int, default=0, help="cap on the component count (0: the full shape)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import torch

    from semanticlens_amd import _native as N
    from semanticlens_amd import scores

    lines = []

    def say(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        lines.append(s)

    dev = N.default_device()
    C, n, D = SHAPE
    C = min(C, args.size) if args.size else C
    V = torch.randn(C, n, D, generator=torch.Generator().manual_seed(0)).to(dev)
    ks = list(range(2, MAX_CLUSTERS + 1))
    fixed = {k: scores.polysemanticity_facets(V, n_clusters=k) for k in ks}
    labels = torch.stack([fixed[k].labels for k in ks])  # (5, C, n)
    m = len(ks)
    lib, ptr, stream = N.lib(), N._ptr, N._stream(V)
    nbytes = int(lib.sl_silhouette_ws_bytes(C, n, D))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    mean = torch.empty((m, C), dtype=torch.float64, device=dev)

    def sil(sets, metric):
        return lambda: lib.sl_silhouette(ptr(V), C, n, D, ptr(labels), sets, MAX_CLUSTERS, metric, None, ptr(mean), ptr(ws), nbytes, stream)

    calls = {"silhouette_m1_euclidean": sil(1, 0), "silhouette_m5_euclidean": sil(m, 0), "silhouette_m1_cosine": sil(1, 1),
             "silhouette_m5_cosine": sil(m, 1)}
    t = alternate(torch, calls, args.reps, args.warmup, args.inner)
    t.update(alternate(torch, {"polysemanticity_score_k2": lambda: scores.polysemanticity_score(V, n_clusters=2),
                               "polysemanticity_score_k3": lambda: scores.polysemanticity_score(V, n_clusters=3)}, args.reps, args.warmup, 1))
    v_bytes, h_bytes = C * n * D * 4, C * n * n * 8
    say({"what": "sl_silhouette (Gram + silhouette kernels, mean only) next to one K9 run on the same tensor", "shape": [C, n, D],
         "inner": args.inner, "V_MB": round(v_bytes / 1e6, 2), "H_MB": round(h_bytes / 1e6, 2),
         **{f"{name}_us": round(median(x) * 1e3, 1) for name, x in t.items()},
         "m5_over_m1_euclidean": round(median(t["silhouette_m5_euclidean"]) / median(t["silhouette_m1_euclidean"]), 3),
         "m1_over_k9_k2": round(median(t["silhouette_m1_euclidean"]) / median(t["polysemanticity_score_k2"]), 3),
         "m1_V_read_TBps": round(v_bytes / (median(t["silhouette_m1_euclidean"]) * 1e-3) / 1e12, 3),
         **{f"{name}_us_all": [round(v * 1e3, 1) for v in x] for name, x in t.items()}})

    calls = {f"facets_k{k}": (lambda k=k: scores.polysemanticity_facets(V, n_clusters=k)) for k in ks}
    for metric in ("euclidean", "cosine"):
        calls[f"facets_auto_{metric}"] = lambda metric=metric: scores.polysemanticity_facets(V, "auto", max_clusters=MAX_CLUSTERS, metric=metric)
    t = alternate(torch, calls, args.reps, args.warmup, 1)
    parts = sum(median(t[f"facets_k{k}"]) for k in ks)
    auto = scores.polysemanticity_facets(V, "auto", max_clusters=MAX_CLUSTERS)
    say({"what": "polysemanticity_facets(n_clusters='auto', max_clusters=6) end to end against the sum of its five fixed-k calls",
         "shape": [C, n, D], **{f"{name}_ms": round(median(x), 3) for name, x in t.items()}, "sum_of_fixed_k_ms": round(parts, 3),
         "auto_euclidean_over_sum": round(median(t["facets_auto_euclidean"]) / parts, 4),
         "auto_cosine_over_sum": round(median(t["facets_auto_cosine"]) / parts, 4),
         "n_facets_histogram": torch.bincount(auto.n_facets.long(), minlength=MAX_CLUSTERS + 1).tolist(),
         **{f"{name}_ms_all": [round(v, 3) for v in x] for name, x in t.items()}})
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
