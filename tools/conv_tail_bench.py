"""Standalone timing of the K27 kernels at layer1's shape, (256, 64, 56, 56) -> 256 channels: each fused call
against what it replaces, `F.conv2d` (MIOpen, find-db pinned as in bench.py) followed by the K16 / K19 tail kernel.

Event-timed, 12 calls after 3 warm-ups, rotating over more than 600 MB of distinct input buffers so that nothing is served
from the Infinity Cache; no other stream.  µs per call (median, minimum) and GB/s of the fused form's algorithmic bytes.

  python tools/conv_tail_bench.py [--out profiles/k27_standalone_timing.txt]
"""
import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from semanticlens_amd import _native as N  # noqa: E402

SHAPE = (256, 64, 56, 56)


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


def bn_params(dev):
    return [torch.randn(256, device=dev), torch.rand(256, device=dev) + 0.1, torch.randn(256, device=dev),
            torch.randn(256, device=dev), 1e-5]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bench.pin_conv_algorithms()
    torch.backends.cudnn.benchmark = False
    dev = "cuda:0"
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    B, _, H, W = SHAPE
    out_shape = (B, 256, H, W)
    in_b, out_b = B * 64 * H * W * 4, B * 256 * H * W * 4
    wa, wb = (torch.randn(256, 64, 1, 1, device=dev) * 0.125 for _ in range(2))
    pa, pb = bn_params(dev), bn_params(dev)
    # three sets of (x, identity, second x): 206 + 822 + 206 MB each
    sets = [(torch.randn(SHAPE, device=dev), torch.randn(out_shape, device=dev), torch.randn(SHAPE, device=dev)) for _ in range(3)]
    say(f"== {SHAPE} -> 256 channels: {in_b / 1e6:.0f} MB in, {out_b / 1e6:.0f} MB out, {len(sets)} rotating sets of inputs")

    def report(name, fn, nbytes=None):
        med, low = timed(fn, sets)
        rate = f" {nbytes / med / 1e3:.0f} GB/s" if nbytes else ""
        say(f"  {name:<46} {med:.0f} us (min {low:.0f}){rate}")
        return med

    say("identity block (layer1.1, layer1.2): relu(bn3(conv3(x)) + identity)")
    fused = report("conv1x1_bn_add_relu", lambda x, idt, xb: N.conv1x1_bn_add_relu(x, wa, pa, idt), in_b + 2 * out_b)
    unfused = report("F.conv2d, then batchnorm_infer(residual)",
                     lambda x, idt, xb: N.batchnorm_infer(F.conv2d(x, wa), *pa, residual=idt))
    report("  F.conv2d alone", lambda x, idt, xb: F.conv2d(x, wa), in_b + out_b)
    report("  the product alone (sl_conv1x1_64_256)", lambda x, idt, xb: N.conv1x1_64_256(x, wa, 0), in_b + out_b)
    conv = F.conv2d(sets[0][0], wa)
    report("  batchnorm_infer(residual) alone", lambda x, idt, xb: N.batchnorm_infer(conv, *pa, residual=idt))
    del conv
    say(f"  saved per call: {unfused - fused:.0f} us ({unfused / fused:.2f}x)")

    say("first block (layer1.0): relu(bn3(conv3(x)) + downsample.1(downsample.0(x0)))")
    fused2 = report("conv1x1_bn_add_conv1x1_bn_relu", lambda x, idt, xb: N.conv1x1_bn_add_conv1x1_bn_relu(x, wa, pa, xb, wb, pb),
                    2 * in_b + out_b)
    unfused2 = report("two F.conv2d, then batchnorm_infer_add_bn_relu",
                      lambda x, idt, xb: N.batchnorm_infer_add_bn_relu(F.conv2d(x, wa), pa, F.conv2d(xb, wb), pb))
    say(f"  saved per call: {unfused2 - fused2:.0f} us ({unfused2 / fused2:.2f}x)")
    say(f"per batch of the headline (two identity blocks, one first block): {2 * (unfused - fused) + unfused2 - fused2:.0f} us")

    x, idt, xb = sets[0]
    conv = F.conv2d(x, wa)
    want = torch.relu_(F.batch_norm(conv, *pa[:4], False, 0.0, pa[4]) + idt)
    bad = int((N.conv1x1_bn_add_relu(x, wa, pa, idt).view(torch.int32) != want.view(torch.int32)).sum())
    want = torch.relu_(F.batch_norm(conv, *pa[:4], False, 0.0, pa[4]) + F.batch_norm(F.conv2d(xb, wb), *pb[:4], False, 0.0, pb[4]))
    bad2 = int((N.conv1x1_bn_add_conv1x1_bn_relu(x, wa, pa, xb, wb, pb).view(torch.int32) != want.view(torch.int32)).sum())
    say(f"elements that differ from the unfused result: {bad} (identity block), {bad2} (first block)")
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
