"""K17 measurement: labelling every component out of a large vocabulary, new path against what the parent commit offers.

Synthetic embeddings, V = 100 000 words against C = 3 584 components at D = 512 (ResNet-50 layer2-4 under CLIP ViT-B) and
C = 30 000 at D = 1 152 (a ViT-so400m's blocks under SigLIP), k = 5 and k = 100.

* new: ``_native.topk_probe`` — the cosine GEMM (K6) tile by tile into one reused buffer, each tile folded by K17.
* torch: the same tiles through ``similarity_score``, ``torch.topk`` per tile, ``torch.cat`` + ``torch.topk`` merge on the device
  (what a user can write on the parent commit without holding the V x C matrix).

Times are HIP-event times of whole calls after warm-up, the two paths alternating; K17's own time comes from the library's
per-dispatch events in a separate pass (``sl_prof_*``), its bytes are what the library logs for the family (the tile bytes
R * B * 4 per launch; where few rows are split over several waves, which none of these shapes is, the partial lists too), and the
ceiling is the 6.29 TB/s float4 copy rate the project uses.  ``--once SHAPE`` runs one new-path call per k and nothing else (for a kernel trace).

    python tools/label_bench.py [--reps 5] [--out profiles/k17_label_bench.txt]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from semanticlens_amd import _native as N  # noqa: E402
from semanticlens_amd.scores import similarity_score  # noqa: E402

COPY_CEILING = 6.29e12
SHAPES = {"rn50_clip": (3584, 512), "so400m_siglip": (30000, 1152)}
V = 100_000


def torch_composition(db, vocab, k, step):
    vals = ids = None
    for start in range(0, vocab.shape[0], step):
        sim = similarity_score(db, vocab[start : start + step])  # (C, chunk)
        v, i = torch.topk(sim, min(k, sim.shape[1]), dim=1)
        i = i + start
        if vals is None:
            vals, ids = v, i
        else:
            cv, ci = torch.cat([vals, v], dim=1), torch.cat([ids, i], dim=1)
            vals, pos = torch.topk(cv, min(k, cv.shape[1]), dim=1)
            ids = torch.gather(ci, 1, pos)
    return vals, ids


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", default=None, choices=list(SHAPES))
    ap.add_argument("--vocab", type=int, default=V)
    args = ap.parse_args()
    dev = N.default_device()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cpu").manual_seed(0)
    for name, (C, D) in SHAPES.items():
        if args.once and name != args.once:
            continue
        db = torch.randn(C, D, generator=g).to(dev)
        vocab = torch.randn(args.vocab, D, generator=g).to(dev)
        step = N.topk_chunk_rows(C, args.vocab)
        tiles = -(-args.vocab // step)
        if args.once:
            for k in (5, 100):
                N.topk_probe(db, vocab, k)
                torch.cuda.synchronize()
            return
        for k in (5, 100):
            new = lambda: N.topk_probe(db, vocab, k)
            old = lambda: torch_composition(db, vocab, k, step)
            for _ in range(args.warmup):
                new(), old()
            torch.cuda.synchronize()
            t_new, t_old = [], []
            for _ in range(args.reps):
                ms, (nv, ni) = event_ms(new)
                t_new.append(ms)
                ms, (ov, oi) = event_ms(old)
                t_old.append(ms)
            same_ids = float((ni == oi).float().mean())
            max_dv = float((nv - ov).abs().max())
            # K17 and GEMM device time inside the new path (the library's per-dispatch events; a pass of its own)
            N.prof_enable(True)
            N.prof_reset()
            new()
            torch.cuda.synchronize()
            k_ms, k_n, k_bytes = N.prof_read(N.SL_PROF_TOPK)
            g_ms, g_n, g_flops = N.prof_read(N.SL_PROF_GEMM)
            N.prof_enable(False)
            med_new, med_old = sorted(t_new)[len(t_new) // 2], sorted(t_old)[len(t_old) // 2]
            rec = {
                "shape": name, "C": C, "D": D, "V": args.vocab, "k": k, "tile_cols": step, "tiles": tiles,
                "new_ms_median": round(med_new, 3), "new_ms_all": [round(t, 3) for t in t_new],
                "torch_ms_median": round(med_old, 3), "torch_ms_all": [round(t, 3) for t in t_old],
                "torch_over_new": round(med_old / med_new, 3),
                "k17_ms": round(k_ms, 3), "k17_launches": k_n, "k17_share_of_new": round(k_ms / med_new, 4),
                "k17_TBps": round(k_bytes / (k_ms * 1e-3) / 1e12, 3) if k_ms else None,
                "k17_fraction_of_copy_ceiling": round(k_bytes / (k_ms * 1e-3) / COPY_CEILING, 3) if k_ms else None,
                "gemm_ms": round(g_ms, 3), "gemm_TFLOPs": round(g_flops / (g_ms * 1e-3) / 1e12, 1) if g_ms else None,
                "ids_equal_fraction": round(same_ids, 6), "max_abs_value_difference": max_dv,
            }
            say(json.dumps(rec))
        del db, vocab
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
