"""Standalone timing of the K18 kernel: `sl_batchnorm_infer_relu_maxpool` against the pair it replaces, the
K16 `bn + relu` kernel and `F.max_pool2d` on that kernel's output, under each `bn_policy`.

Event-timed, 12 launches after 3 warm-ups, rotating over more than 600 MB of distinct input buffers so that nothing is served
from the Infinity Cache; no other stream.  µs per call (median, minimum) and GB/s of algorithmic bytes against the 6.29 TB/s
copy ceiling.

  python tools/bn_pool_bench.py [--out profiles/k18_standalone_timing.txt]
"""
import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semanticlens_amd import _native as N  # noqa: E402

COPY_GBS = 6290.0
POOL = ((3, 3), (2, 2), (1, 1))
SHAPES = ((256, 64, 112, 112), (256, 64, 56, 56))


def timed(fn, bufs, warm=3, reps=12):
    for i in range(warm):
        fn(bufs[i % len(bufs)])
    torch.cuda.synchronize()
    events = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(bufs[(i + warm) % len(bufs)])
        b.record()
        events.append((a, b))
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in events)
    return us[len(us) // 2], us[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for shape in SHAPES:
        B, C, H, W = shape
        in_bytes = B * C * H * W * 4
        out_bytes = in_bytes // 4
        xs = [torch.randn(shape, device=dev) for _ in range(max(2, -(-700_000_000 // in_bytes)))]
        mean, w, b = (torch.randn(C, device=dev) for _ in range(3))
        var = torch.rand(C, device=dev) + 0.1
        say(f"== {shape}: input {in_bytes / 1e6:.0f} MB, pooled output {out_bytes / 1e6:.0f} MB, {len(xs)} rotating inputs")
        ys = [N.batchnorm_infer(x, mean, var, w, b, 1e-5, relu=True) for x in xs[:2]]
        before = N.get_option("bn_policy")
        try:
            for pol in (1, 2, 3):
                N.set_option("bn_policy", pol)
                med, low = timed(lambda x: N.batchnorm_infer_relu_maxpool(x, mean, var, w, b, 1e-5, *POOL), xs)
                gbs = (in_bytes + out_bytes) / med / 1e3
                say(f"  pol{pol} bn+relu+maxpool {med:.0f} us (min {low:.0f}) {gbs:.0f} GB/s = {gbs / COPY_GBS:.2f} of copy")
                med, low = timed(lambda x: N.batchnorm_infer(x, mean, var, w, b, 1e-5, relu=True), xs)
                say(f"  pol{pol} bn+relu alone   {med:.0f} us (min {low:.0f}) {2 * in_bytes / med / 1e3:.0f} GB/s")
        finally:
            N.set_option("bn_policy", before)
        med, low = timed(lambda y: F.max_pool2d(y, *POOL), ys)
        say(f"  F.max_pool2d on the bn+relu output {med:.0f} us (min {low:.0f})")
        got = N.batchnorm_infer_relu_maxpool(xs[0], mean, var, w, b, 1e-5, *POOL)
        bad = int((got.view(torch.int32) != F.max_pool2d(ys[0], *POOL).view(torch.int32)).sum())
        say(f"  elements that differ from the unfused result: {bad}")
        del xs, ys
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
