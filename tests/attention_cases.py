"""Attention inputs whose softmax is NOT that of `torch.randn`: one head's q, k, v for a named logit pattern, their float64
reference, a derived per-element error bound, and a host restatement of the two kernels' arithmetic
(`attention_mfma_kernel<D>` and `attention_bf16x3_kernel<D, MAXW>`, semanticlens_amd/csrc/encoder_attention.hip).  A helper, not a test:
tests/test_attention_bound_host.py holds every case to its description and the emulation to half the bound without a GPU,
tests/test_gpu_attention_values.py runs the kernels on the same inputs, docs/ATTENTION_VALUES.md is the table.

Logits are built through two reserved dimensions of the head (s_ij = q_i . k_j / sqrt(D)):

  q[:, 1] = sqrt(D),     k[:, 1] = c_j      a bias c_j per key
  q[:, 0] = a_i sqrt(D), k[:, 0] = b_j      a rank-one term a_i b_j

the other dimensions are 0.3 randn (logit noise of about 0.1), v is randn.  Patterns (L = the size of the planted logit):

  sink         c_0 = L                          the maximum is fixed by key 0; later tiles add e^-L
  last         c_{T-1} = L                      the accumulators are wiped at the last key tile (one valid key if T % 32 == 1)
  stairs       c_j = L (j // 32)                the maximum rises by L at every key tile
  stairs_down  c_j = -L (j // 32)               every later tile adds underflowed terms only
  mixed        b_1 = -L, b_{T-2} = L, a_i = +1 (i even), -1 (i odd): even rows peak at key T - 2, odd rows at key 1
  diag         q = k = sqrt(L sqrt(D)) x unit vectors (orthonormal inside every run of D rows): s_ii = L, s_ij = L cos
  uniform      q = 0                            all logits 0
  bigv         sink, with row T // 2 of v scaled by 1e4
  scaled       randn q, k, v, q scaled until the largest |logit| in float64 is L
"""
from __future__ import annotations

import math

import torch

SHAPES = ((64, 33), (32, 257), (96, 193), (128, 161))  # (D, T): see tests/test_gpu_attention_values.py
STRUCTURAL = ("sink", "last", "stairs", "stairs_down", "mixed", "diag", "bigv")
PATTERN_CASES = tuple((p, L) for p in STRUCTURAL for L in (40, 120)) + (("uniform", 0),) + tuple(("scaled", L) for L in (30, 100, 300))
B, H = 2, 2  # every GPU case is one call with four heads, each built from its own seed
GAP_EXACT = 105.0  # a key this far below the row's maximum has a probability below 2^-150 (104 = 150 ln 2) in either arithmetic

U = 2.0 ** -24      # unit roundoff of fp32
W3 = 3 * 2.0 ** -18  # split-bf16 x3: hi + lo leaves 2^-18 of either operand, the dropped lo * lo is 2^-18 of the product


def head_seed(pattern: str, L: int, D: int, T: int, head: int) -> int:
    return 1_000_000 * (1 + STRUCTURAL.index(pattern) if pattern in STRUCTURAL else 9 + len(pattern)) + 10_000 * L + 10 * (D + T) + head


def build(pattern: str, T: int, D: int, L: float, seed: int):
    """fp32 q, k, v of shape (T, D) for one head"""
    g = torch.Generator().manual_seed(seed)
    rd = math.sqrt(D)
    v = torch.randn(T, D, generator=g, dtype=torch.float64)
    if pattern == "scaled":
        q = torch.randn(T, D, generator=g, dtype=torch.float64)
        k = torch.randn(T, D, generator=g, dtype=torch.float64).float().double()
        q = q * (L / ((q @ k.T) / rd).abs().max())
        return q.float(), k.float(), v.float()
    if pattern == "uniform":
        k = torch.randn(T, D, generator=g, dtype=torch.float64)
        return torch.zeros(T, D), k.float(), v.float()
    if pattern == "diag":
        runs = [torch.linalg.qr(torch.randn(D, D, generator=g, dtype=torch.float64))[0].T for _ in range(0, T, D)]
        u = torch.cat(runs)[:T]
        qk = (math.sqrt(L * rd) * u).float()
        return qk, qk.clone(), v.float()
    q = 0.3 * torch.randn(T, D, generator=g, dtype=torch.float64)
    k = 0.3 * torch.randn(T, D, generator=g, dtype=torch.float64)
    a, b, c = torch.zeros(T, dtype=torch.float64), torch.zeros(T, dtype=torch.float64), torch.zeros(T, dtype=torch.float64)
    j = torch.arange(T)
    if pattern in ("sink", "bigv"):
        c[0] = L
    elif pattern == "last":
        c[T - 1] = L
    elif pattern == "stairs":
        c = (L * (j // 32)).double()
    elif pattern == "stairs_down":
        c = (-L * (j // 32)).double()
    elif pattern == "mixed":
        assert T >= 4
        b[1], b[T - 2] = -L, L
        a = torch.where(j % 2 == 0, 1.0, -1.0).double()
    else:
        raise ValueError(pattern)
    q[:, 0], k[:, 0] = a * rd, b
    q[:, 1], k[:, 1] = rd, c
    if pattern == "bigv":
        v[T // 2] *= 1e4
    return q.float(), k.float(), v.float()


def _mask(T: int, causal: bool) -> torch.Tensor:
    return torch.ones(T, T, dtype=torch.bool).triu_(1) if causal else torch.zeros(T, T, dtype=torch.bool)


def reference(q, k, v, causal: bool):
    """float64 (out, s, p) of softmax(q k^T / sqrt(D)) v from the fp32 inputs; masked logits are -inf"""
    T, D = q.shape
    s = (q.double() @ k.double().T) / math.sqrt(D)
    s = s.masked_fill(_mask(T, causal), float("-inf"))
    p = torch.softmax(s, -1)
    return p @ v.double(), s, p


def bound(q, k, v, causal: bool, p, bf16x3: bool) -> torch.Tensor:
    """(T, D) bound on |kernel - reference|.  A rounded score is off by at most delta_i = ((D + 4) u + w) max_j A_ij, where
    A_ij = sum_d |q_id| |k_jd| / sqrt(D): D products and additions, the pre-scaling of q, the subtraction of the maximum and the
    argument of the exponential in fp32, and w per split product.  Moving every logit of a row by at most delta moves a
    normalised probability by a factor inside e^(+-2 delta).  The second term is the P V product over T keys (T u), the rescales
    and exponentials (8 u) and the split of P and V (w), on sum_j p_ij |v_jd|."""
    T, D = q.shape
    w = W3 if bf16x3 else 0.0
    A = (q.double().abs() @ k.double().abs().T) / math.sqrt(D)
    A = A.masked_fill(_mask(T, causal), 0.0)
    delta = ((D + 4) * U + w) * A.max(1).values
    return (torch.expm1(2 * delta)[:, None] + (T + 8) * U + w) * (p @ v.double().abs())


def exact_rows(s) -> torch.Tensor:
    """(rows, their dominant key): rows in which every key but one sits GAP_EXACT or more below the maximum, so that both
    kernels see the probabilities (1, 0, ..., 0) and the output row is that key's v row"""
    top = s.max(1)
    others = s.clone()
    others[torch.arange(s.shape[0]), top.indices] = float("-inf")
    rows = torch.nonzero(top.values - others.max(1).values >= GAP_EXACT).reshape(-1)
    return rows, top.indices[rows]


# ---- the kernels' arithmetic on the host ---------------------------------------------------------------------------------------
def _split(x: torch.Tensor):
    """fp32 -> (hi, lo): bf16 values (round to nearest even, as the kernel's casts) held in fp32"""
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


_LOG2E = torch.tensor(1.44269502e+00, dtype=torch.float32)
_LOG2E_LO = torch.tensor(1.92596299e-08, dtype=torch.float32)
_LN2 = torch.tensor(6.93147182e-01, dtype=torch.float32)


def exp_neg(x: torch.Tensor) -> torch.Tensor:
    """`exp_neg` of encoder_attention.hip on fp32 `x`: the clamp at -104, 2^(x log2 e) with the product's rounding error and the low part
    of the constant folded back in.  The fused multiply-adds are taken in float64 and rounded once; the hardware exp2 is the
    float64 one rounded to fp32, with results below 2^-126 flushed to 0 as the instruction does."""
    x = x.clamp_min(-104.0)
    t = x * _LOG2E
    d = (x.double() * _LOG2E.double() - t.double()).float()
    d = (x.double() * _LOG2E_LO.double() + d.double()).float()
    r = torch.exp2(t.double()).float()
    r = torch.where(t < -126.0, torch.zeros_like(r), r)
    return (r.double() * (d * _LN2).double() + r.double()).float()


def emulate(q, k, v, causal: bool, bf16x3: bool) -> torch.Tensor:
    """(T, D) fp32: what the kernel computes, restated from its comments.  q is pre-scaled by float32(1 / sqrt(D)); a wave owns 32
    query rows (rows past T repeat row T - 1 under their own index, as the kernel's padded lanes do) and walks 32-key tiles
    (all of them, or up to its own under `causal`) with the running maximum m, alpha = exp(m - mn), l = l alpha + sum p and
    o = o alpha + p v in fp32.  `bf16x3`: q', K, P and V are split into bf16 hi + lo and every product is lo * hi + hi * lo +
    hi * hi in that order per 16-wide k-step, the exponential is `exp_neg`, and the rescale of o is skipped for a wave whose 32
    maxima all stood still.  The order of the additions inside one k-step is torch's, not the matrix core's."""
    T, D = q.shape
    Tp = (T + 31) // 32 * 32
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=torch.float64).float()
    qi = torch.arange(Tp)
    qs = q[qi.clamp_max(T - 1)] * scale
    kp, vp = torch.zeros(Tp, D), torch.zeros(Tp, D)
    kp[:T], vp[:T] = k, v
    if bf16x3:
        qh, ql = _split(qs)
        kh, kl = _split(kp)
        vh, vl = _split(vp)
    ex = exp_neg if bf16x3 else torch.exp
    o = torch.zeros(Tp, D)
    m = torch.full((Tp,), float("-inf"))
    l = torch.zeros(Tp)
    for kt in range(Tp // 32):
        ks = slice(32 * kt, 32 * kt + 32)
        takes = (qi // 32 >= kt) if causal else torch.ones(Tp, dtype=torch.bool)  # the waves whose key loop reaches this tile
        if bf16x3:
            st = torch.zeros(Tp, 32)
            for d0 in range(0, D, 16):
                ds = slice(d0, d0 + 16)
                st = st + qh[:, ds] @ kl[ks, ds].T
                st = st + ql[:, ds] @ kh[ks, ds].T
                st = st + qh[:, ds] @ kh[ks, ds].T
        else:
            st = qs @ kp[ks].T
        key = torch.arange(32 * kt, 32 * kt + 32)
        masked = (key >= T)[None, :] | ((key[None, :] > qi[:, None]) if causal else False)
        st = st.masked_fill(masked, float("-inf"))
        mn = torch.maximum(m, st.max(1).values)
        mn = torch.where(takes, mn, torch.zeros_like(mn))  # rows that skip the tile: keep -inf - -inf out of the arithmetic
        alpha = ex(torch.where(takes, m - mn, torch.zeros_like(m)))
        p = ex(st - mn[:, None])
        l_new = l * alpha + p.sum(1)
        if bf16x3:
            still = (mn == m).reshape(-1, 32).all(1).repeat_interleave(32)  # `if (!__all(mn == m))`
            o_new = torch.where(still[:, None], o, o * alpha[:, None])
            for s2 in range(2):
                k16 = slice(32 * kt + 16 * s2, 32 * kt + 16 * s2 + 16)
                ph, pl = _split(p[:, 16 * s2:16 * s2 + 16])
                o_new = o_new + ph @ vl[k16]
                o_new = o_new + pl @ vh[k16]
                o_new = o_new + ph @ vh[k16]
        else:
            o_new = o * alpha[:, None] + p @ vp[ks]
        o = torch.where(takes[:, None], o_new, o)
        l = torch.where(takes, l_new, l)
        m = torch.where(takes, mn, m)
    return (o * (1.0 / l)[:, None])[:T]


# ---- four heads in the entry point's layout -----------------------------------------------------------------------------------
def pack(heads, T: int, D: int) -> torch.Tensor:
    """B * H (q, k, v) triples -> the (B * T, 3 * H * D) qkv matrix of `sl_attention`; head (b, h) is heads[b * H + h]"""
    qkv = torch.empty(B, T, 3, H, D)
    for i, (q, k, v) in enumerate(heads):
        qkv[i // H, :, 0, i % H], qkv[i // H, :, 1, i % H], qkv[i // H, :, 2, i % H] = q, k, v
    return qkv.reshape(B * T, 3 * H * D)


def unpack(out: torch.Tensor, T: int, D: int):
    """the (B * T, H * D) output -> a list of B * H (T, D) heads"""
    o = out.reshape(B, T, H, D)
    return [o[i // H, :, i % H] for i in range(B * H)]


def case_heads(pattern: str, L: int, D: int, T: int):
    return [build(pattern, T, D, L, head_seed(pattern, L, D, T, i)) for i in range(B * H)]
