"""K21 measurement: what exporting K9's labels and reducing the facets costs, at two concept-DB layers of 20 samples x 512:
1 536 components (a configs[4]-sized layer) and 2 048 (the layer tools/scores_bench.py times).

* ``sl_facet_stats`` against ``sl_clarity`` on the same tensor in the same process, the two alternating: both read the same
  C*n*D*4 bytes once; bytes alone allow 1 + kc/n.  A kernel of tens of microseconds is timed as a window of ``--inner``
  back-to-back launches between two HIP events.
* ``polysemanticity_facets`` end to end against ``polysemanticity_score``, alternating.
* ``polysemanticity_score`` on this tree and on a tree of the parent commit (``--parent-tree``: a checkout with its library
  built), each in a child process of its own because the two libraries export the same names; the children alternate,
  ``--rounds`` times each, and every child's median is listed so that the run-to-run spread can be read next to the difference.

Times are HIP-event times after warm-up; medians of ``--reps`` windows.  ``--size`` shrinks the component counts for a rehearsal;
a figure taken below the default sizes is a figure of overheads.

``--kc`` sets ``n_clusters`` (2 with at most 128 samples: K9's LDS variant; anything else: its workspace variant) and ``--shape
C,n,D`` replaces the two layers by one shape, for all three measurements.

    python tools/facets_bench.py [--parent-tree DIR] [--kc K] [--shape C,n,D] [--out profiles/k21_facets_bench.txt]
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1536, 20, 512), (2048, 20, 512)]


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
    """Median and all window times (ms per call) of each function, the functions taking turns."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(window_ms(torch, fn, inner))
    return times


def shapes(args):
    """The shapes to time: ``--shape`` alone when given, else the two layers; ``--size`` caps the component counts."""
    todo = [tuple(int(x) for x in args.shape.split(","))] if args.shape else SHAPES
    return [(min(C, args.size) if args.size else C, n, D) for C, n, D in todo]


def child(args):
    """``polysemanticity_score`` of the package found in ``--tree``: one JSON line per shape."""
    sys.path.insert(0, str(Path(args.tree).resolve()))
    import torch

    from semanticlens_amd import _native as N
    from semanticlens_amd import scores

    dev = N.default_device()
    for C, n, D in shapes(args):
        V = torch.randn(C, n, D, generator=torch.Generator().manual_seed(0)).to(dev)
        t = alternate(torch, {"score": lambda: scores.polysemanticity_score(V, n_clusters=args.kc)}, args.reps, args.warmup, 1)["score"]
        digest = float(scores.polysemanticity_score(V, n_clusters=args.kc).sum())
        print(json.dumps({"shape": [C, n, D], "ms_median": round(median(t), 3), "ms_all": [round(x, 3) for x in t], "score_sum": digest}),
              flush=True)


def run_child(tree, args):
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--tree", str(tree), "--reps", str(args.reps), "--warmup",
           str(args.warmup), "--size", str(args.size), "--kc", str(args.kc)] + (["--shape", args.shape] if args.shape else [])
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return [json.loads(line) for line in out.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=50, help="launches per timed window of the two kernels")
    ap.add_argument("--rounds", type=int, default=3, help="child processes per tree for the parent comparison")
    ap.add_argument("--size", type=int, default=0, help="cap on the component counts (0: the full shapes)")
    ap.add_argument("--kc", type=int, default=2, help="n_clusters (2: K9's LDS kernel up to 128 samples; else its general kernel)")
    ap.add_argument("--shape", default=None, help="C,n,D: time this shape instead of the two layers")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=str(ROOT), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []

    def say(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        lines.append(s)

    # the parent comparison first: its children must not share the device with this process's allocations
    if args.parent_tree:
        runs = {"this": [], "parent": []}
        for _ in range(args.rounds):
            for name, tree in (("parent", args.parent_tree), ("this", ROOT)):
                runs[name].append(run_child(tree, args))
        for i, shape in enumerate(shapes(args)):
            meds = {name: [r[i]["ms_median"] for r in rs] for name, rs in runs.items()}
            sums = {r[i]["score_sum"] for rs in runs.values() for r in rs}
            say({"what": "polysemanticity_score, this tree against the parent tree", "shape": shape, "kc": args.kc,
                 "this_ms_medians_per_process": meds["this"], "parent_ms_medians_per_process": meds["parent"],
                 "this_ms": median(meds["this"]), "parent_ms": median(meds["parent"]),
                 "this_over_parent": round(median(meds["this"]) / median(meds["parent"]), 4),
                 "spread_this": round(max(meds["this"]) / min(meds["this"]), 4),
                 "spread_parent": round(max(meds["parent"]) / min(meds["parent"]), 4), "scores_identical": len(sums) == 1})

    sys.path.insert(0, str(ROOT))
    import torch

    from semanticlens_amd import _native as N
    from semanticlens_amd import scores

    dev = N.default_device()
    kc = args.kc
    for C, n, D in shapes(args):
        V = torch.randn(C, n, D, generator=torch.Generator().manual_seed(0)).to(dev)
        f = scores.polysemanticity_facets(V, n_clusters=kc)
        labels = f.labels
        centres = torch.empty((C, kc, D), dtype=torch.float32, device=dev)
        counts = torch.empty((C, kc), dtype=torch.int32, device=dev)
        clar = torch.empty((C, kc), dtype=torch.float32, device=dev)
        out = torch.empty((C,), dtype=torch.float32, device=dev)
        lib, ptr, stream = N.lib(), N._ptr, N._stream(V)
        kernels = {
            "clarity": lambda: lib.sl_clarity(ptr(V), C, n, D, ptr(out), stream),
            "facet_stats": lambda: lib.sl_facet_stats(ptr(V), C, n, D, ptr(labels), kc, ptr(centres), ptr(counts), ptr(clar), stream),
        }
        t = alternate(torch, kernels, args.reps, args.warmup, args.inner)
        nbytes = C * n * D * 4
        mc, mf = median(t["clarity"]), median(t["facet_stats"])
        say({"what": "sl_facet_stats against sl_clarity", "shape": [C, n, D], "kc": kc, "inner": args.inner,
             "clarity_us": round(mc * 1e3, 2), "facet_stats_us": round(mf * 1e3, 2), "ratio": round(mf / mc, 3),
             "bytes_allow": round(1 + kc / n, 3), "clarity_TBps": round(nbytes / (mc * 1e-3) / 1e12, 3),
             "facet_stats_TBps": round(nbytes * (1 + kc / n) / (mf * 1e-3) / 1e12, 3),
             "clarity_us_all": [round(x * 1e3, 2) for x in t["clarity"]], "facet_stats_us_all": [round(x * 1e3, 2) for x in t["facet_stats"]]})
        calls = {"score": lambda: scores.polysemanticity_score(V, n_clusters=kc), "facets": lambda: scores.polysemanticity_facets(V, n_clusters=kc)}
        t = alternate(torch, calls, args.reps, args.warmup, 1)
        ms, mf = median(t["score"]), median(t["facets"])
        say({"what": "polysemanticity_facets against polysemanticity_score, end to end", "shape": [C, n, D], "kc": kc,
             "score_ms": round(ms, 3), "facets_ms": round(mf, 3), "ratio": round(mf / ms, 4),
             "score_ms_all": [round(x, 3) for x in t["score"]], "facets_ms_all": [round(x, 3) for x in t["facets"]],
             "score_bit_equal": bool(torch.equal(f.score, scores.polysemanticity_score(V, n_clusters=kc)))})
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
