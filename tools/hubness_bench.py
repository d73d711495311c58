"""K29 measurement: ``sl_topk_merge_biased`` against K17 (``sl_topk_merge``) on the same tile, K17 on this tree against another
build of the library, and ``probe_csls`` against the three ``probe_topk`` calls it contains.

Kernel part.  One fp32 tile of 8 192 rows by 32 768 and by 2 048 columns, uniform values in [-1, 1], k = 5; for K29 row and column
biases uniform in [0, 0.25].  Both states are first warmed by a tile whose values (and scores) lie above everything the timed tile
holds, so the timed launches run the steady state of a long vocabulary walk: every candidate is tested against the threshold and
none is inserted.  ``sl_topk_merge_biased`` and ``sl_topk_merge`` on the same tile in the same process, alternating.  Times are the
library's per-dispatch event times (``sl_prof_*``), the mean over ``--launches`` launches per block; ``--blocks`` blocks give the
median and the spread.  The bar is the one K24, K25 and K26 were held to: at most 1.10 of the yardstick's time.

K17 itself.  With ``--parent-lib PATH`` (a ``libsemanticlens_hip.so`` built from the parent commit) ``sl_topk_merge`` of both
libraries on those tiles, loaded side by side and alternating block by block: medians, the spread of each over its blocks, and
the difference.

Whole call.  ``lens.probe_csls(k = 5, neighbours = 10)`` against the sum of ``probe_topk`` of components against words at k = 10,
words against components at k = 10 and components against words at k = 5, on the two shapes of DESIGN.md §K17's table over
100 000 word vectors: HIP-event time of whole calls, alternating.  K29's share: the top-k family's event time of the whole call
minus that of its two K17 passes run alone.  ``--scale`` divides the sizes for a rehearsal; a figure taken below the default size
is a figure of overheads.

    python tools/hubness_bench.py [--parent-lib PATH] [--out profiles/k29_hubness_bench.txt]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from semanticlens_amd import _native as N  # noqa: E402
from semanticlens_amd import lens as L  # noqa: E402

COPY_CEILING = 6.29e12
SHAPES = {"rn50_clip": (3584, 512), "so400m_siglip": (30000, 1152)}
K, NEIGHBOURS = 5, 10


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def prof_read(lib, family: int):
    ms, n, nbytes = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    lib.sl_prof_read(family, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(nbytes))
    return ms.value, n.value


def dispatch_ms(lib, fn, launches: int) -> float:
    """Mean top-k family time per call of ``launches`` calls of ``fn`` under ``lib``'s events (one dispatch each)."""
    lib.sl_prof_enable(1)
    lib.sl_prof_reset()
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    ms, n = prof_read(lib, N.SL_PROF_TOPK)
    lib.sl_prof_enable(0)
    assert n == launches, (n, launches)
    return ms / launches


def median(xs):
    return sorted(xs)[len(xs) // 2]


def us(xs):
    return [round(t * 1e3, 2) for t in xs]


def load_other(path: str):
    """Another build of the library beside this tree's, with the few entry points the K17 comparison calls"""
    other = ctypes.CDLL(path)
    for name in ("sl_topk_merge", "sl_prof_enable", "sl_prof_reset", "sl_prof_read"):
        fn = getattr(other, name)
        fn.restype, fn.argtypes = N.SIGNATURES[name]
    return other


def kernel_part(say, dev, R: int, B: int, launches: int, blocks: int, other):
    g = torch.Generator(device="cpu").manual_seed(R + B)
    tile = (torch.rand(R, B, generator=g) * 2 - 1).to(dev)
    rb = (torch.rand(R, generator=g) * 0.25).to(dev)
    cb = (torch.rand(B, generator=g) * 0.25).to(dev)
    nbytes = R * B * 4
    assert int(N.lib().sl_topk_merge_ws_bytes(R, K, B)) == 0  # one wave per row: one dispatch per merge
    states = {name: N.topk_new(R, K, dev) for name in ("k17", "k29", "k17_parent")}
    for sv, si in states.values():  # the previous tile: K distinct values above every cosine and every score of the timed tile
        N.topk_merge(sv, si, 4.0 + torch.rand(R, 64, device=dev), 0)
    p, stream = N._ptr, N._stream(tile)

    def merge(lib, name):
        sv, si = states[name]
        return lambda: lib.sl_topk_merge(p(sv), p(si), R, K, p(tile), B, B, 64, None, 0, stream)

    variants = {"k17": (N.lib(), merge(N.lib(), "k17")),
                "k29": (N.lib(), lambda: N.topk_merge_biased(*states["k29"], tile, rb, cb, 64))}
    if other is not None:
        variants["k17_parent"] = (other, merge(other, "k17_parent"))
    before = {name: (sv.clone(), si.clone()) for name, (sv, si) in states.items()}
    for _, fn in variants.values():  # warm-up: code objects
        fn(), fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(blocks):
        for name, (lib, fn) in variants.items():
            times[name].append(dispatch_ms(lib, fn, launches))
    steady = all(torch.equal(sv, before[name][0]) and torch.equal(si, before[name][1]) for name, (sv, si) in states.items())
    k17, k29 = median(times["k17"]), median(times["k29"])
    line = {
        "part": "kernel", "tile": [R, B], "tile_MB": round(nbytes / 1e6, 1), "k": K, "launches_per_block": launches, "blocks": blocks,
        "no_candidate_inserted": steady,
        "k17_us_median": round(k17 * 1e3, 2), "k17_us_blocks": us(times["k17"]), "k17_TBps": round(nbytes / (k17 * 1e-3) / 1e12, 3),
        "k29_us_median": round(k29 * 1e3, 2), "k29_us_blocks": us(times["k29"]), "k29_TBps": round(nbytes / (k29 * 1e-3) / 1e12, 3),
        "k29_fraction_of_copy_ceiling": round(nbytes / (k29 * 1e-3) / COPY_CEILING, 3),
        "k29_over_k17": round(k29 / k17, 3), "bar": 1.10,
    }
    if other is not None:
        par = median(times["k17_parent"])
        line.update({
            "k17_parent_us_median": round(par * 1e3, 2), "k17_parent_us_blocks": us(times["k17_parent"]),
            "k17_spread_us": round((max(times["k17"]) - min(times["k17"])) * 1e3, 2),
            "k17_parent_spread_us": round((max(times["k17_parent"]) - min(times["k17_parent"])) * 1e3, 2),
            "k17_minus_parent_us": round((k17 - par) * 1e3, 2), "k17_over_parent": round(k17 / par, 4),
        })
    say(json.dumps(line))


def topk_family_ms(fn) -> float:
    N.prof_enable(True)
    N.prof_reset()
    fn()
    torch.cuda.synchronize()
    ms = N.prof_read(N.SL_PROF_TOPK)[0]
    N.prof_enable(False)
    return ms


def whole_call(say, dev, name: str, C: int, D: int, V: int, reps: int):
    g = torch.Generator(device="cpu").manual_seed(0)
    db = torch.randn(C, D, generator=g).to(dev)
    words = torch.randn(V, D, generator=g).to(dev)
    densities = lambda: (L.probe_topk(words, db, NEIGHBOURS), L.probe_topk(db, words, NEIGHBOURS))
    three = lambda: (densities(), L.probe_topk(words, db, K))
    csls = lambda: L.probe_csls(words, db, k=K, neighbours=NEIGHBOURS)
    three(), csls()
    torch.cuda.synchronize()
    t_three, t_csls = [], []
    for _ in range(reps):
        t_three.append(event_ms(three)[0])
        ms, hl = event_ms(csls)
        t_csls.append(ms)
    k29_ms = topk_family_ms(csls) - topk_family_ms(densities)
    (rv, ri), (qv, qi) = densities()
    plain = L.probe_topk(words, db, K)[1]
    csls_ms = median(t_csls)
    say(json.dumps({
        "part": "whole_call", "shape": name, "C": C, "D": D, "V": V, "k": K, "neighbours": NEIGHBOURS, "gemm_mode": "bf16x3 (default)",
        "three_probe_topk_ms_median": round(median(t_three), 3), "three_probe_topk_ms_all": [round(t, 3) for t in t_three],
        "probe_csls_ms_median": round(csls_ms, 3), "probe_csls_ms_all": [round(t, 3) for t in t_csls],
        "probe_csls_over_three_probe_topk": round(csls_ms / median(t_three), 3), "bar": 1.10,
        "k29_ms": round(k29_ms, 3), "k29_share_of_call": round(k29_ms / csls_ms, 4),
        "k29_TBps": round(C * V * 4 / (k29_ms * 1e-3) / 1e12, 3) if k29_ms > 0 else None,
        "densities_bit_equal_to_probe_topk_means": bool(
            torch.equal(hl.component_density, N.topk_density(rv, ri)) and torch.equal(hl.label_density, N.topk_density(qv, qi))),
        "top1_changed_fraction": round(float((hl.ids[:, 0] != plain[:, 0]).float().mean()), 4),
    }))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--part", choices=("all", "kernel", "whole_call"), default="all")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = N.default_device()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    s = args.scale
    if args.part in ("all", "kernel"):
        other = load_other(args.parent_lib) if args.parent_lib else None
        for R, B in ((8192 // s, 32768 // s), (8192 // s, 2048 // s)):
            kernel_part(say, dev, R, B, args.launches, args.blocks, other)
            torch.cuda.empty_cache()
    if args.part in ("all", "whole_call"):
        for name, (C, D) in SHAPES.items():
            whole_call(say, dev, name, C // s, D, 100000 // s, args.reps)
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
