"""Target of a counter run on the K18 kernel alone: three launches of `sl_batchnorm_infer_relu_maxpool` at the
benchmark's shape, each on a fresh 822 MB input (larger than the Infinity Cache).

  rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT -- python tools/bn_pool_pmc_target.py
  python tools/prof_summarize.py pmc OUT profiles/k18_pmc_fetch.csv       # HBM read bytes = 2 x FETCH_SIZE x 1024
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semanticlens_amd import _native as N  # noqa: E402

dev = "cuda:0"
B, C, H, W = 256, 64, 112, 112
mean, w, b = (torch.randn(C, device=dev) for _ in range(3))
var = torch.rand(C, device=dev) + 0.1
for _ in range(3):
    x = torch.randn(B, C, H, W, device=dev)
    y = N.batchnorm_infer_relu_maxpool(x, mean, var, w, b, 1e-5, (3, 3), (2, 2), (1, 1))
    torch.cuda.synchronize()
    del x, y
