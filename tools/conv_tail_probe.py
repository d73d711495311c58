"""Step 0 of K27: which partial-sum arithmetic reproduces, bit for bit, what `F.conv2d` computes for layer1's
64 -> 256 channel pointwise convolutions at the headline's shape, (256, 64, 56, 56).

MIOpen serves these from `GemmFwd1x1_0_1`, a strided-batched fp32 GEMM of rocBLAS/Tensile (`MI16x16x4x1` kernels in the committed
traces).  `sl_conv1x1_64_256` accumulates with the same instruction; what is unknown is how the GEMM kernel cuts K = 64 among
wave groups (LocalSplitU 1, 2 or 4), in which granules, how the partial sums are added, and whether its local reads hand an MFMA
step adjacent k (vector width 1) or every second / fourth one (width 2 / 4).  Every combination is one candidate here:

  L   chains (wave groups that each sum a part of K)
  G   MFMA steps (of four k) a chain takes before the next chain's turn; 16 / L is one contiguous run per chain
  vw  local-read vector width: a step takes k {b + vw g + e} for slot g, e the step's index within a block of vw steps
  add how L = 4 partial sums are combined: in order, or pairwise

The MIOpen find-db is pinned the way `bench.pin_conv_algorithms` does, so MIOpen picks the benchmark's solver.  Per input
(three seeds: unit normal, a post-ReLU distribution with exact zeros, wide dynamic range) the table counts the elements whose
int32 patterns differ from `F.conv2d`'s, of 205,520,896.

  python tools/conv_tail_probe.py [--batch 256] [--out profiles/k27_step0_probe.txt]
"""
import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from semanticlens_amd import _native as N  # noqa: E402

SPLIT_OF = {(1, "-"): 0, (2, "-"): 1, (4, "in order"): 3, (4, "pairwise"): 4}  # the kernels whose chains are contiguous step runs


def k_order(L: int, G: int, vw: int):
    """k of (step, slot) for chains that take granules of G steps in turn, each chain's k handed to its steps vw-strided."""
    chains = [[] for _ in range(L)]
    for q in range(16 // G):
        chains[q % L] += list(range(4 * G * q, 4 * G * (q + 1)))
    slots = []
    for kk in chains:
        for blk in range(0, len(kk), 4 * vw):
            for e in range(vw):
                slots += [kk[blk + vw * g + e] for g in range(4)]
    return slots


def candidates():
    for vw in (1, 2, 4):
        yield 1, 16, vw, "-"
        for G in (1, 2, 4, 8):
            yield 2, G, vw, "-"
        for G in (1, 2, 4):
            for add in ("in order", "pairwise"):
                yield 4, G, vw, add


def inputs(seed: int, batch: int, dev):
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((batch, 64, 56, 56), device=dev, generator=gen)
    w = torch.randn((256, 64, 1, 1), device=dev, generator=gen) * 0.125
    if seed % 3 == 1:
        x = torch.relu_(x)  # what conv3 sees behind bn2 + relu: half the operands are exact zeros
    elif seed % 3 == 2:
        x = x * torch.exp2(torch.randint(-12, 12, (1, 64, 1, 1), device=dev, generator=gen).float())
    return x, w


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bench.pin_conv_algorithms()  # before the first convolution of this process
    torch.backends.cudnn.benchmark = False
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    # the kernel itself first: a small problem against float64, so that a table of mismatches is about arithmetic and not a bug
    x, w = inputs(0, 2, dev)
    ref64 = torch.einsum("oc,nchw->nohw", w.view(256, 64).double(), x.double())
    bound = 66 * 2.0**-24 * torch.einsum("oc,nchw->nohw", w.view(256, 64).double().abs(), x.double().abs())
    for split in range(N.CONV_TAIL_SPLITS):
        got = N.conv1x1_64_256(x, w, split)
        if not bool(((got.double() - ref64).abs() <= bound).all()):
            say(f"split {split}: outside the fma-chain bound of float64; nothing below would mean anything")
            return 1
    say("all splits within gamma_66 * sum |w x| of float64 at (2, 64, 56, 56)")

    say(f"{'L':>2} {'G':>2} {'vw':>2} {'add':<9}" + "".join(f" {'seed ' + str(s):>12}" for s in args.seeds))
    rows, refs = [], []
    for seed in args.seeds:
        x, w = inputs(seed, args.batch, dev)
        refs.append((x, w, F.conv2d(x, w).view(torch.int32)))
    for L, G, vw, add in candidates():
        order = torch.tensor(k_order(L, G, vw), dtype=torch.int32, device=dev)
        counts = []
        for x, w, ref in refs:
            got = N.conv1x1_64_256(x, w, SPLIT_OF[(L, add)], order)
            counts.append(int((got.view(torch.int32) != ref).sum()))
            del got
        rows.append(((L, G, vw, add), counts))
        say(f"{L:>2} {G:>2} {vw:>2} {add:<9}" + "".join(f" {c:>12}" for c in counts))
    # the kernels that deal steps to chains themselves must agree with the G = 1 orders above (a check of the probe)
    for split, key in ((2, (2, 1, 1, "-")), (5, (4, 1, 1, "in order")), (6, (4, 1, 1, "pairwise"))):
        x, w, ref = refs[0]
        same = int((N.conv1x1_64_256(x, w, split).view(torch.int32) != ref).sum()) == dict(rows)[key][0]
        say(f"split {split} (steps dealt in the kernel) counts as L, G, vw, add = {key}: {same}")
    proven = [key for key, counts in rows if not any(counts)]
    say(f"elements per input: {refs[0][2].numel()}; candidates with no mismatch on any input: {proven if proven else 'none'}")
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
