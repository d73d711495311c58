"""K28 measurement: the pursuit step (``sl_omp_step``) against the row gather K5 (``sl_gather_rows``) of the same rows, and
``probe_decompose`` against the vocabulary passes it is made of.

Kernel part.  C = 8 192 and 98 304 components of width 768 against 100 000 word vectors; a state with t chosen words per component
(random distinct ids, their Cholesky factor and right-hand side built by running steps 0 .. t - 1 with hand-fed candidates), then
step t timed: t + 1 = 1, 4, 8, 16 rows per component.  The baseline is ``N.gather_rows`` of the same ``(C, t + 1)`` ids from the same
table, alternating with it in the same process.  The gather reads each row once and writes it once: 2 (t + 1) row-sized streams;
the step reads each row twice (the second time from L2) and x twice, and writes one row: 2 (t + 1) + 3 streams, and the tool
reports its rate over all of them.  The bar the kernel was given is a ratio of 1.5 to the gather.  Every timed step runs on a fresh copy of the state (a step changes it); the copies are
made outside the timed dispatches.  Times are the library's per-dispatch event times (``sl_prof_*``), the mean over ``--launches``
launches per block; ``--blocks`` blocks give the median and the spread.

End to end.  ``lens.probe_decompose(n_terms=8)`` of 98 304 x 768 components over 100 000 words against eight ``probe_topk(k = 1)``
calls on the same operands (the passes without the steps, at the smallest k): HIP-event time of whole calls, alternating, and
K28's share of the call from the library's events in a pass of its own.
``--scale`` divides the sizes for a rehearsal; a figure taken below the default size is a figure of overheads.

    python tools/decompose_bench.py [--out profiles/k28_decompose_bench.txt]
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

SL_PROF_GATHER = 3  # include/semanticlens_amd.h
BAR = 1.5


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def prof_block(calls, family: int) -> float:
    """Mean dispatch time of ``calls`` (a list of thunks, one dispatch of ``family`` each) under the library's events."""
    N.prof_enable(True)
    N.prof_reset()
    for call in calls:
        call()
    torch.cuda.synchronize()
    ms, n, _ = N.prof_read(family)
    N.prof_enable(False)
    assert n == len(calls), (n, len(calls))
    return ms / len(calls)


def clone_state(st: N.OmpState) -> N.OmpState:
    return N.OmpState(*(part.clone() for part in st))


def kernel_part(say, dev, C: int, V: int, D: int, rows: int, launches: int, blocks: int):
    g = torch.Generator(device="cpu").manual_seed(C + rows)
    x = torch.randn(C, D, generator=g).to(dev)
    w = torch.randn(V, D, generator=g).to(dev)
    s = max(rows, 1)
    # `rows` distinct random words per component
    ids = torch.stack([torch.randperm(V, generator=g)[:rows] for _ in range(min(C, 256))]).repeat(-(-C // 256), 1)[:C]
    ids = ((ids + torch.arange(C)[:, None]) % V).to(dev)  # a shift per component keeps them distinct and spreads the rows
    ids = ids[:, :rows].contiguous()  # every step is offered all of them and takes the first it has not chosen: ids[:, t]
    vals = torch.full((C, rows), 0.5, device=dev)
    st = N.omp_new(x, s)
    for t in range(rows - 1):
        N.omp_step(st, x, w, vals, ids, t, 0.0)
    assert int(st.n_terms.min()) == rows - 1 and int(st.finished.sum()) == 0
    t = rows - 1
    flat = ids.reshape(-1).contiguous()
    gather = lambda: N.gather_rows(w, flat, check=False)
    copies = [clone_state(st) for _ in range(launches)]
    step_on = lambda c: N.omp_step(c, x, w, vals, ids, t, 0.0)
    step_on(clone_state(st)), gather(), gather()
    torch.cuda.synchronize()
    t_step, t_gather = [], []
    for _ in range(blocks):
        for c, src in zip(copies, [st] * launches):  # reset the copies outside the timed dispatches
            for a, b in zip(c, src):
                a.copy_(b)
        torch.cuda.synchronize()
        t_step.append(prof_block([lambda c=c: step_on(c) for c in copies], N.SL_PROF_TOPK))
        t_gather.append(prof_block([gather] * launches, SL_PROF_GATHER))
    done = copies[0]
    assert int(done.n_terms.min()) == rows and bool(torch.isfinite(done.coefs).all())
    ms, mg = median(t_step), median(t_gather)
    row_bytes = C * rows * D * 4
    say(json.dumps({
        "part": "kernel", "C": C, "V": V, "D": D, "rows_per_component": rows, "launches_per_block": launches, "blocks": blocks,
        "row_MB": round(row_bytes / 1e6, 1),
        "k28_step_us_median": round(ms * 1e3, 2), "k28_step_us_blocks": [round(v * 1e3, 2) for v in t_step],
        "k5_gather_us_median": round(mg * 1e3, 2), "k5_gather_us_blocks": [round(v * 1e3, 2) for v in t_gather],
        "k28_over_k5": round(ms / mg, 3), "bar": BAR, "within_bar": bool(ms / mg <= BAR),
        "k28_row_reads_TBps": round(2 * row_bytes / (ms * 1e-3) / 1e12, 3),
        "k28_all_bytes_TBps": round((2 * row_bytes + 3 * C * D * 4) / (ms * 1e-3) / 1e12, 3),
        "k5_TBps": round(2 * row_bytes / (mg * 1e-3) / 1e12, 3),
    }))


def end_to_end(say, dev, C: int, D: int, V: int, s: int, reps: int):
    g = torch.Generator(device="cpu").manual_seed(0)
    db = torch.randn(C, D, generator=g).to(dev)
    words = torch.randn(V, D, generator=g).to(dev)

    def passes():
        for _ in range(s):
            L.probe_topk(words, db, 1)

    new = lambda: L.probe_decompose(words, db, n_terms=s)
    passes(), new()
    torch.cuda.synchronize()
    t_old, t_new = [], []
    for _ in range(reps):
        t_old.append(event_ms(passes)[0])
        ms, dec = event_ms(new)
        t_new.append(ms)
    N.prof_enable(True)
    N.prof_reset()
    new()
    torch.cuda.synchronize()
    gemm, topk = N.prof_read(N.SL_PROF_GEMM), N.prof_read(N.SL_PROF_TOPK)
    N.prof_reset()
    passes()
    torch.cuda.synchronize()
    topk_passes = N.prof_read(N.SL_PROF_TOPK)
    N.prof_enable(False)
    # SL_PROF_TOPK holds K17's merges and K28's init and steps; the K17 part alone, at its k = t + 1, in a pass of its own
    N.prof_enable(True)
    N.prof_reset()
    st = N.omp_new(db, s)
    vals, ids = N.topk_probe(db, words, s)
    torch.cuda.synchronize()
    N.prof_reset()
    for t in range(s):
        N.omp_step(st, db, words, vals, ids, t, 0.0)
    torch.cuda.synchronize()
    k28 = N.prof_read(N.SL_PROF_TOPK)
    N.prof_enable(False)
    new_ms = median(t_new)
    say(json.dumps({
        "part": "end_to_end", "C": C, "D": D, "V": V, "n_terms": s, "gemm_mode": "bf16x3 (default)",
        "eight_probe_topk_k1_ms_median": round(median(t_old), 3), "eight_probe_topk_k1_ms_all": [round(t, 3) for t in t_old],
        "probe_decompose_ms_median": round(new_ms, 3), "probe_decompose_ms_all": [round(t, 3) for t in t_new],
        "probe_decompose_over_passes": round(new_ms / median(t_old), 3),
        "gemm_ms": round(gemm[0], 3), "gemm_launches": gemm[1],
        "k17_plus_k28_ms": round(topk[0], 3), "k17_plus_k28_launches": topk[1],
        "k17_ms_of_the_k1_passes": round(topk_passes[0], 3),
        "k28_steps_ms": round(k28[0], 3), "k28_step_launches": k28[1],
        "k28_steps_ms_each": round(k28[0] / max(k28[1], 1), 3),
        "k28_share_of_call": round(k28[0] / new_ms, 4),
        "terms_used_mean": round(float(dec.n_terms.double().mean()), 2), "explained_mean": round(float(dec.explained[:, -1].mean()), 4),
    }))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=5)
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

    sc = args.scale
    if args.part in ("all", "kernel"):
        for C in (8192 // sc, 98304 // sc):
            for rows in (1, 4, 8, 16):
                kernel_part(say, dev, C, 100000 // sc, 768, rows, args.launches, args.blocks)
                torch.cuda.empty_cache()
    if args.part in ("all", "end_to_end"):
        end_to_end(say, dev, 98304 // sc, 768, 100000 // sc, 8, args.reps)
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
