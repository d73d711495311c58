"""Standalone timing of the K19 kernel: `sl_batchnorm_infer_add_bn_relu` against the pair it replaces, the plain
K16 kernel on the shortcut's tensor followed by the K16 `add + relu` tail, at the four shapes of ResNet-50's stage-opening blocks
under each `bn_policy`.

Event-timed, 12 calls after 3 warm-ups, rotating over more than 600 MB of distinct input buffers so that nothing is served
from the Infinity Cache; no other stream.  µs per call (median, minimum) and GB/s of algorithmic bytes (three passes for the one
kernel, five for the pair) against the 6.29 TB/s copy ceiling.

  python tools/bn_dual_bench.py [--out profiles/k19_standalone_timing.txt]
"""
import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semanticlens_amd import _native as N  # noqa: E402

COPY_GBS = 6290.0
SHAPES = ((256, 256, 56, 56), (256, 512, 28, 28), (256, 1024, 14, 14), (256, 2048, 7, 7))


def timed(fn, bufs, warm=3, reps=12):
    for i in range(warm):
        fn(*bufs[i % len(bufs)])
    torch.cuda.synchronize()
    events = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(*bufs[(i + warm) % len(bufs)])
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
        C = shape[1]
        nbytes = shape[0] * C * shape[2] * shape[3] * 4
        pairs = [(torch.randn(shape, device=dev), torch.randn(shape, device=dev)) for _ in range(max(2, -(-350_000_000 // nbytes)))]
        pa, pb = ([*(torch.randn(C, device=dev) for _ in range(2)), torch.randn(C, device=dev), torch.randn(C, device=dev), 1e-5]
                  for _ in range(2))
        for p in (pa, pb):
            p[1] = torch.rand(C, device=dev) + 0.1

        def one(xa, xb):
            return N.batchnorm_infer_add_bn_relu(xa, pa, xb, pb)

        def pair(xa, xb):
            idt = N.batchnorm_infer(xb, *pb)
            return N.batchnorm_infer(xa, *pa, residual=idt)

        say(f"== {shape}: {nbytes / 1e6:.0f} MB per tensor, {len(pairs)} rotating pairs of inputs")
        before = N.get_option("bn_policy")
        try:
            for pol in (0, 1, 2, 3):
                N.set_option("bn_policy", pol)
                med, low = timed(one, pairs)
                gbs = 3 * nbytes / med / 1e3
                say(f"  pol{pol} bn+bn+add+relu  {med:.0f} us (min {low:.0f}) {gbs:.0f} GB/s = {gbs / COPY_GBS:.2f} of copy")
                med, low = timed(pair, pairs)
                say(f"  pol{pol} plain, then tail {med:.0f} us (min {low:.0f}) {5 * nbytes / med / 1e3:.0f} GB/s")
        finally:
            N.set_option("bn_policy", before)
        xa, xb = pairs[0]
        want = torch.relu_(F.batch_norm(xa, *pa[:4], False, 0.0, pa[4]) + F.batch_norm(xb, *pb[:4], False, 0.0, pb[4]))
        bad = int((one(xa, xb).view(torch.int32) != want.view(torch.int32)).sum())
        say(f"  elements that differ from the unfused result: {bad}")
        del pairs, want
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
