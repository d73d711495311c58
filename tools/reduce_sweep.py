"""K1 / K2 sweep for comparing two builds of libsemanticlens_hip.so bit for bit (select one with SEMANTICLENS_AMD_LIB).

  python tools/reduce_sweep.py run OUT.npz      every call's (cand, out_f32), fixed seeds, in call order
  python tools/reduce_sweep.py compare A.npz B.npz [TRACE_A.csv TRACE_B.csv]

Covers fp32 / fp16 / bf16; NCHW, channels_last, tokens and transposed tokens; all aggregators; planted NaN, +-inf, -0.0;
S = 1..1100 with row counts of every divisibility the ladders test; one input of >= 8 MiB per rowreduce_dma call site (the
shapes of tests/test_gpu_parity.py); colreduce_nw forced to 4 / 8 / 16; tables of tensors; inputs above nt_min_bytes.
"""
import csv
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def site_shapes():
    sys.path.insert(0, str(ROOT / "tests"))
    from test_gpu_parity import DMA_SITES_F32, DMA_SITES_HALF  # one list: the test's

    return DMA_SITES_F32, DMA_SITES_HALF


def run(out_path):
    import torch

    from semanticlens_amd import _native as N

    dev = "cuda:0"
    saved = []

    def keep(*ts):
        for t in ts:
            saved.append(t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy().ravel().astype(np.int32))

    def conv(x, code):
        B, C = x.shape[:2]
        cand = torch.empty((B, C), dtype=torch.bfloat16, device=dev)
        out = torch.empty((B, C), dtype=torch.float32, device=dev)
        N.reduce_conv(x, code, cand, out)
        keep(cand, out)

    def tokens(x, code, pos=0):
        B, T, F = x.shape
        cand = torch.empty((B, F), dtype=torch.bfloat16, device=dev)
        out = torch.empty((B, F), dtype=torch.float32, device=dev)
        N.reduce_tokens(x, code, pos, cand, out)
        keep(cand, out)

    g = torch.Generator().manual_seed(1234)
    n = 64 << 20
    base = torch.randn(n, generator=g)
    idx = torch.arange(0, n, 997)
    base[idx[0::4]] = float("nan")
    base[idx[1::4]] = float("inf")
    base[idx[2::4]] = -float("inf")
    base[idx[3::4]] = -0.0
    bufs = {dt: base.to(dt).to(dev) for dt in (torch.float32, torch.float16, torch.bfloat16)}
    convs = (N.SL_CONV_MAX, N.SL_CONV_MEAN, N.SL_CONV_SUM)
    toks = (N.SL_TOK_MEAN, N.SL_TOK_ABSMEAN, N.SL_TOK_MAX, N.SL_TOK_ABSMAX)
    # S = 1..1100, rows of every divisibility the ladders test (R % 16 == 0, 8, 4, 2, odd), at an offset that moves with S
    for dt, buf in bufs.items():
        for S in range(1, 1101):
            for C in (16, 24, 20, 18, 17) if S % 7 == 0 or S <= 64 else ((16, 24, 20, 18, 17)[S % 5],):
                x = buf[S * 16:S * 16 + 2 * C * S].view(2, C, S, 1)
                conv(x, convs[S % 2])
                if S % 3 == 0:
                    tokens(x.view(2, C, S).transpose(1, 2), toks[S % 4])  # transposed tokens: the token axis contiguous
    # one >= 8 MiB input per rowreduce_dma site, every aggregator (abs ops through the transposed-token entry)
    f32_sites, half_sites = site_shapes()
    for dt, sites in ((torch.float32, f32_sites), (torch.float16, half_sites), (torch.bfloat16, half_sites)):
        for _, (B, C, H, W) in sites:
            x = bufs[dt][4096:4096 + B * C * H * W].view(B, C, H, W)
            for code in convs:
                conv(x, code)
            for code in (N.SL_TOK_ABSMAX, N.SL_TOK_ABSMEAN):
                tokens(x.view(B, C, H * W).transpose(1, 2), code)
    # component axis contiguous: tokens and channels_last, every aggregator and the single-token pick, forced wave counts
    for nw in (0, 4, 8, 16):
        N.set_option("colreduce_nw", nw)
        for dt, buf in bufs.items():
            for B, T, F in ((8, 197, 768), (4, 50, 260), (3, 33, 1000), (2, 257, 1024), (2, 300, 96), (5, 7, 12)):
                x = buf[64:64 + B * T * F].view(B, T, F)
                for code in toks:
                    tokens(x, code)
                tokens(x, N.SL_TOK_TOKEN, -1)
            for B, C, H, W in ((4, 64, 7, 7), (2, 96, 14, 14), (3, 260, 5, 3)):
                x = buf[128:128 + B * C * H * W].view(B, H, W, C).permute(0, 3, 1, 2)  # channels_last
                for code in convs:
                    conv(x, code)
            xs = [buf[k * 1000003:k * 1000003 + 4 * 197 * 768].view(4, 197, 768) for k in range(3)]
            for code in toks:
                cand = torch.empty((3, 4, 768), dtype=torch.bfloat16, device=dev)
                N.reduce_multi("tokens", xs, code, 0, cand)
                keep(cand)
    N.set_option("colreduce_nw", 0)
    # above nt_min_bytes: the tail split, with the thresholds lowered (32 MiB inputs) and with the defaults (411 MB)
    for nt_min, tail in ((16 << 20, 8 << 20), (16 << 20, 0), (0, 0), (None, None)):
        N.set_reduce_policy(nt_min, tail)
        for dt, buf in bufs.items():
            es = buf.element_size()
            for B, C, H, W in ((64, 2048, 7, 7), (64, 1024, 14, 14), (16, 512, 28, 28), (8, 256, 64, 64), (8, 256, 61, 67)):
                k = (32 << 20) // (es * C * H * W * B) + 1
                x = buf[:k * B * C * H * W].view(k * B, C, H, W)
                conv(x, N.SL_CONV_MAX)
                conv(x, N.SL_CONV_MEAN)
            x = buf[:(40 << 20) // es // 768 // 197 * 197 * 768].view(-1, 197, 768)
            tokens(x, N.SL_TOK_MAX)
            tokens(x, N.SL_TOK_MEAN)
    big = torch.randn(256, 512, 28, 28, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    conv(big, N.SL_CONV_MAX)
    conv(big, N.SL_CONV_MEAN)
    torch.cuda.synchronize()
    np.savez(out_path, n=np.array([len(saved)]), sizes=np.array([len(a) for a in saved]), data=np.concatenate(saved))
    print(f"sweep: {len(saved)} arrays saved to {out_path}")


def kernels(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows if "reduce" in r["Kernel_Name"] and ("sl::" in r["Kernel_Name"] or "_ZN2sl" in r["Kernel_Name"])]
    # rowreduce_fast lost a kernel parameter; nothing else in any signature changed (demangled and mangled spelling)
    names = [re.sub(r"(rowreduce_fast_kernel<[^>]*>\(.*float\*), int, long\)", r"\1, long)", k) for k in names]
    return [re.sub(r"(rowreduce_fast_kernelI\w+EEvPKflifPtPf)il$", r"\1l", k) for k in names]


def compare(a, b, ta=None, tb=None):
    A, B = np.load(a), np.load(b)
    same_layout = np.array_equal(A["sizes"], B["sizes"])
    mism = -1
    if same_layout:
        ends = np.cumsum(A["sizes"])
        diff = A["data"] != B["data"]
        mism = int(sum(diff[e - s:e].any() for s, e in zip(A["sizes"], ends)))
    print(f"arrays compared: {int(A['n'][0])} vs {int(B['n'][0])}; same layout: {same_layout}; arrays with a differing bit: {mism}")
    if ta:
        ka, kb = kernels(ta), kernels(tb)
        fam = lambda k: re.search(r"(\w+_kernel)", k).group(1)
        print(f"reduce kernel launches: {len(ka)} vs {len(kb)}; ordered kernel-name lists identical: {ka == kb}")
        for i, (x, y) in enumerate(zip(ka, kb)):
            if x != y:
                print(f"  first difference at launch {i}:\n    {x}\n    {y}")
                break
        inst = sorted(set(kb))
        print(f"distinct reduce instances hit: {len(set(ka))} vs {len(inst)}")
        count = {}
        for k in inst:
            count[fam(k)] = count.get(fam(k), 0) + 1
        for f, c in sorted(count.items()):
            print(f"  {f}: {c} instances hit")
    return 0 if mism == 0 and (not ta or ka == kb) else 1


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        sys.exit(compare(*sys.argv[2:]))
