"""K22 measurement: per-set column maxima (``sl_segmax_merge``) against K20 (``sl_mutualmax_merge``) on the same tile, and the
audit path end to end.

Kernel part.  One fp32 tile of 8 192 rows by 32 768 and by 2 048 columns, uniform values.  ``sl_segmax_merge`` with the rows cut
into runs of 1, 4, 16, 64 and 8 192 (one set) consecutive rows per segment, and ``sl_mutualmax_merge`` — K20 as it stands, which
reads the same bytes and issues one column flush per row block plus one atomic per row — on the same tile in the same process,
the variants alternating.  Times are the library's per-dispatch event times (``sl_prof_*``, the dispatch's own begin / end
timestamps), the mean over ``--launches`` launches per block; ``--blocks`` blocks give the median and the spread.  The states
persist from launch to launch, so from the second launch on an atomic max finds its own value: the atomics are issued, the
memory side has nothing to change.  Rates are tile bytes over time.

End to end.  ``lens.probe_setmax`` for 40 000 x 768 prompt vectors in 2 000 sets of 20 against 98 304 components: HIP-event time
of whole calls, and the GEMM / selection split from the library's events in a pass of its own.  Against 2 048 components, where
the (prompts, components) matrix fits, the same call against ``_native.similarity`` followed by ``torch.scatter_reduce(amax)``
(which returns no argmax).  ``--scale`` divides the sizes for a rehearsal; a figure taken below the default size is a figure of
overheads.

    python tools/audit_bench.py [--out profiles/k22_audit_bench.txt]
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
RUNS = (1, 4, 16, 64, 8192)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def dispatch_ms(fn, launches: int) -> float:
    """Mean per-dispatch time of ``launches`` calls of ``fn`` under the library's events (family SL_PROF_TOPK)."""
    N.prof_enable(True)
    N.prof_reset()
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    ms, n, _ = N.prof_read(N.SL_PROF_TOPK)
    N.prof_enable(False)
    assert n == launches
    return ms / n


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
    variants = {}
    row_state = torch.zeros(R, dtype=torch.int64, device=dev)
    col_state = torch.zeros(B, dtype=torch.int64, device=dev)
    variants["k20"] = lambda: N.mutualmax_merge(row_state, col_state, tile)
    keep = []
    for run in RUNS:
        run = min(run, R)
        seg = (torch.arange(R, device=dev) // run).to(torch.int32)
        state = torch.zeros((-(-R // run), B), dtype=torch.int64, device=dev)
        keep.append((seg, state))
        variants[f"k22_run{run}"] = (lambda s=state, g=seg: N.segmax_merge(s, tile, g))
    for fn in variants.values():  # warm-up: code objects, and the states reach their final values
        fn(), fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(blocks):
        for name, fn in variants.items():
            times[name].append(dispatch_ms(fn, launches))
    k20 = median(times["k20"])
    say(json.dumps({
        "part": "kernel", "tile": [R, B], "tile_MB": round(nbytes / 1e6, 1), "launches_per_block": launches, "blocks": blocks,
        "k20_us_median": round(k20 * 1e3, 2), "k20_us_blocks": [round(t * 1e3, 2) for t in times["k20"]],
        "k20_spread_max_over_min": round(max(times["k20"]) / min(times["k20"]), 3),
        "k20_TBps": round(nbytes / (k20 * 1e-3) / 1e12, 3),
    }))
    for name, ts in times.items():
        if name == "k20":
            continue
        med = median(ts)
        run = int(name.split("run")[1])
        say(json.dumps({
            "part": "kernel", "tile": [R, B], "run_length": run, "segments": -(-R // run),
            "k22_us_median": round(med * 1e3, 2), "k22_us_blocks": [round(t * 1e3, 2) for t in ts],
            "k22_over_k20": round(med / k20, 3), "k22_TBps": round(nbytes / (med * 1e-3) / 1e12, 3),
            "k22_fraction_of_copy_ceiling": round(nbytes / (med * 1e-3) / COPY_CEILING, 3),
            "atomic_bytes_over_tile_bytes": round(8 * -(-64 // min(run, 64)) / (4 * 64), 3),  # computed: 8 B per column per run per 64-row block
        }))


def end_to_end(say, dev, P: int, G: int, D: int, C: int, reps: int, with_matrix: bool):
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(P, D, generator=g).to(dev)
    y = torch.randn(C, D, generator=g).to(dev)
    offsets = [round(i * P / G) for i in range(G + 1)]
    new = lambda: L.probe_setmax(x, offsets, y)
    new()
    torch.cuda.synchronize()
    t_new = []
    for _ in range(reps):
        ms, (vals, ids) = event_ms(new)
        t_new.append(ms)
    g_ms, g_n, g_flops, s_ms, s_n, s_bytes = profiled(new)
    rows = N.topk_chunk_rows(C, P)
    line = {
        "part": "end_to_end", "prompts": P, "sets": G, "D": D, "components": C, "gemm_mode": "bf16x3 (default)",
        "tile_rows": rows, "tiles": -(-P // rows),
        "probe_setmax_ms_median": round(median(t_new), 2), "probe_setmax_ms_all": [round(t, 2) for t in t_new],
        "gemm_ms": round(g_ms, 2), "gemm_launches": g_n, "gemm_TFLOPs": round(g_flops / (g_ms * 1e-3) / 1e12, 1) if g_ms else None,
        "select_ms": round(s_ms, 2), "select_launches": s_n, "select_TBps": round(s_bytes / (s_ms * 1e-3) / 1e12, 3) if s_ms else None,
    }
    if with_matrix:
        seg = torch.repeat_interleave(torch.arange(G), torch.tensor([b - a for a, b in zip(offsets, offsets[1:])])).to(dev)

        def old():
            sim = N.similarity(x, y)
            out = torch.full((G, C), float("-inf"), device=dev)
            return out.scatter_reduce(0, seg[:, None].expand(P, C), sim, "amax")

        old()
        torch.cuda.synchronize()
        t_old = []
        for _ in range(reps):
            ms, _ = event_ms(new)
            ms_old, amax = event_ms(old)
            t_old.append(ms_old)
        line.update({
            "matrix_then_scatter_reduce_ms_median": round(median(t_old), 2), "matrix_then_scatter_reduce_ms_all": [round(t, 2) for t in t_old],
            "matrix_path_over_probe_setmax": round(median(t_old) / median(t_new), 3),
            "max_abs_value_difference": float((amax - vals).abs().max()),
        })
    say(json.dumps(line))


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
        end_to_end(say, dev, 40000 // s, 2000 // s, 768, 98304 // s, args.reps, with_matrix=False)
        torch.cuda.empty_cache()
        end_to_end(say, dev, 40000 // s, 2000 // s, 768, 2048 // s, args.reps, with_matrix=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
