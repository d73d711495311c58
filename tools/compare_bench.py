"""K20 measurement: comparing two concept DBs, one cosine pass with mutual maxima against what the parent commit offers.

Two single-layer DBs of C = 98 304 random unit rows at D = 768 (24 blocks x 4 096 components of a ViT-L, under a CLIP ViT-L/14's
text width), in both GEMM modes.

* new: ``lens.compare_concept_dbs(a, b)`` — per tile one cosine GEMM (K6) into one reused buffer and one K20 launch that takes
  the row maxima (A -> B) and the column maxima (B -> A) out of the same read.
* square: ``_native.mutual_probe`` over square tiles of the same bytes (not what the API does; it prices the per-tile operand
  preparation of the full-width tiling).
* parent: ``probe_topk(a, b, 1, per="query")`` plus ``probe_topk(b, a, 1, per="query")`` — the formulation available before K20:
  the GEMM twice over the same products, every tile read by K17 at k = 1.

Times are HIP-event times of whole calls after warm-up, the two paths alternating.  The GEMM / selection split comes from the
library's per-dispatch events in a pass of its own (``sl_prof_*``: SL_PROF_GEMM and SL_PROF_TOPK, the family K17 and K20 share);
the selection's bytes are the tile bytes the library logs for the family, its ceiling the 6.29 TB/s float4 copy rate the project
uses.  ``--size`` shrinks the DBs for a rehearsal; a figure taken below the default size is a figure of overheads.

    python tools/compare_bench.py [--reps 3] [--out profiles/k20_compare_bench.txt]
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
C, D = 98_304, 768


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def profiled(fn):
    """One call under the library's per-dispatch events: (GEMM ms, GEMM flops, selection ms, launches, bytes)."""
    N.prof_enable(True)
    N.prof_reset()
    fn()
    torch.cuda.synchronize()
    s_ms, s_n, s_bytes = N.prof_read(N.SL_PROF_TOPK)
    g_ms, _, g_flops = N.prof_read(N.SL_PROF_GEMM)
    N.prof_enable(False)
    return g_ms, g_flops, s_ms, s_n, s_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, default=C)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = N.default_device()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cpu").manual_seed(0)
    a = torch.nn.functional.normalize(torch.randn(args.size, D, generator=g), dim=1).to(dev)
    b = torch.nn.functional.normalize(torch.randn(args.size, D, generator=g), dim=1).to(dev)
    new = lambda: L.compare_concept_dbs(a, b)
    old = lambda: (L.probe_topk(a, b, 1, per="query"), L.probe_topk(b, a, 1, per="query"))
    for mode in ("bf16x3", "f32"):
        N.set_gemm_mode(mode)
        try:
            for _ in range(args.warmup):
                new(), old()
            torch.cuda.synchronize()
            t_new, t_old = [], []
            for _ in range(args.reps):
                ms, cmp = event_ms(new)
                t_new.append(ms)
                ms, (fwd, rev) = event_ms(old)
                t_old.append(ms)
            vals_a, ids_a, vals_b, ids_b = cmp.pair()
            same = min(float((ids_a == fwd[2][:, 0]).float().mean()), float((ids_b == rev[2][:, 0]).float().mean()))
            max_dv = max(float((vals_a - fwd[0][:, 0]).abs().max()), float((vals_b - rev[0][:, 0]).abs().max()))
            set_ab = cmp.set_similarity_ab
            del cmp, fwd, rev
            # the same pass over square tiles of the same bytes: each call of the GEMM entry point prepares both operands, and a
            # square tile prepares sqrt(tile) rows of each where a full-width tile prepares all of B ("Driver")
            side = min(args.size, int((N.TOPK_TILE_BYTES // 4) ** 0.5))
            square = lambda: N.mutual_probe(a, b, side, side)
            square()
            t_sq = [event_ms(square)[0] for _ in range(args.reps)]
            ng_ms, ng_flops, ns_ms, ns_n, ns_bytes = profiled(new)
            og_ms, og_flops, os_ms, os_n, os_bytes = profiled(old)
        finally:
            N.set_gemm_mode(None)
        med_new, med_old = sorted(t_new)[len(t_new) // 2], sorted(t_old)[len(t_old) // 2]
        rate = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 1e12, 3) if ms else None
        say(json.dumps({
            "gemm_mode": mode, "C_a": args.size, "C_b": args.size, "D": D,
            "tile_rows": N.topk_chunk_rows(args.size, args.size), "tiles": -(-args.size // N.topk_chunk_rows(args.size, args.size)),
            "new_ms_median": round(med_new, 2), "new_ms_all": [round(t, 2) for t in t_new],
            "parent_ms_median": round(med_old, 2), "parent_ms_all": [round(t, 2) for t in t_old],
            "parent_over_new": round(med_old / med_new, 3),
            "square_tile_side": side, "square_tiles_ms_median": round(sorted(t_sq)[len(t_sq) // 2], 2),
            "new_gemm_ms": round(ng_ms, 2), "new_gemm_TFLOPs": round(ng_flops / (ng_ms * 1e-3) / 1e12, 1) if ng_ms else None,
            "new_select_ms": round(ns_ms, 2), "new_select_launches": ns_n, "new_select_TBps": rate(ns_bytes, ns_ms),
            "new_select_fraction_of_copy_ceiling": round(ns_bytes / (ns_ms * 1e-3) / COPY_CEILING, 3) if ns_ms else None,
            "parent_gemm_ms": round(og_ms, 2), "parent_gemm_TFLOPs": round(og_flops / (og_ms * 1e-3) / 1e12, 1) if og_ms else None,
            "parent_select_ms": round(os_ms, 2), "parent_select_launches": os_n, "parent_select_TBps": rate(os_bytes, os_ms),
            "ids_equal_fraction": round(same, 6), "max_abs_value_difference": max_dv, "set_similarity_ab": round(set_ab, 6),
        }))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
