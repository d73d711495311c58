"""K11: `attention_mfma_kernel<D>` (`sl_attention`) and `attention_bf16x3_kernel<D, MAXW>` (`sl_attention_bf16x3`) against float64
where the softmax is peaked and the logits are large.  Every other attention test feeds the kernels `torch.randn` (logits of
order 1, a largest probability near 0.01, a running maximum that settles in the first key tile); the cases of
tests/attention_cases.py pin the maximum to the first key, the last valid key or the causal diagonal, raise it by 40 or 120 at
every key tile (alpha = e^-40, alpha = 0 and every argument below the -104 clamp of `exp_neg`), split a wave into lanes that
have settled and lanes that still rise, and scale random logits to 30, 100 and 300.  The flat bars of the suite do not hold
there (tests/test_attention_bound_host.py), so each output element is held to `attention_cases.bound`, derived from the
float64 quantities of its own row.  docs/ATTENTION_VALUES.md has the patterns, the derivation and the measured ratios.

Shapes (D, T), every T one key past a tile: (64, 33) one wave; (32, 257) MAXW = 8, two rounds, three key chunks in bf16x3;
(96, 193) MAXW = 8 with two waves per SIMD, two chunks in both kernels; (128, 161) MAXW = 4, 128-key chunks in both."""
from functools import lru_cache

import pytest
import torch

import attention_cases as AC
from semanticlens_amd import _native as N
from test_gpu_instances import check_attention, poison

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNELS = [pytest.param(False, id="fp32"), pytest.param(True, id="bf16x3")]
CAUSAL = [pytest.param(False, id="full"), pytest.param(True, id="causal")]


@lru_cache(maxsize=None)
def case(pattern, L, D, T):
    heads = AC.case_heads(pattern, L, D, T)
    return heads, AC.pack(heads, T, D).to(DEV)


@lru_cache(maxsize=None)
def references(pattern, L, D, T, causal):
    return [AC.reference(q, k, v, causal) for q, k, v in case(pattern, L, D, T)[0]]


def run(qkv, D, T, causal, bf16x3):
    poison(AC.B * T * AC.H * D)
    return N.attention(qkv, AC.B, T, AC.H, D, causal, bf16x3=bf16x3)


def check_split_form(qkv, got, D, T, causal, bf16x3):
    sp = N.Split(AC.B * T, AC.H * D, DEV)
    N.attention(qkv, AC.B, T, AC.H, D, causal, out_split=sp, bf16x3=bf16x3)
    assert (sp.hi.float() + sp.lo.float() - got).abs().max().item() <= 2.0 ** -16 * got.abs().max().item() + 1e-9


def check_values(pattern, L, D, T, causal, bf16x3):
    """every head of the case: finite, within the bound element by element, exact where the probabilities are (1, 0, ..., 0).
    Returns (largest |got - float64| / bound, largest |got - float64|)."""
    heads, qkv = case(pattern, L, D, T)
    got_dev = run(qkv, D, T, causal, bf16x3)
    assert bool(torch.isfinite(got_dev).all()), "non-finite output"
    worst, worst_err, exact = 0.0, 0.0, 0
    for h, (got, (q, k, v), (want, s, p)) in enumerate(zip(AC.unpack(got_dev.cpu(), T, D), heads, references(pattern, L, D, T, causal))):
        err = (got.double() - want).abs()
        bnd = AC.bound(q, k, v, causal, p, bf16x3)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
        i = ratio.argmax().item()
        worst, worst_err = max(worst, ratio.reshape(-1)[i].item()), max(worst_err, err.max().item())
        assert bool((err <= bnd).all()), f"head {h} row {i // D} dim {i % D}: |got - float64| = {err.reshape(-1)[i].item():.3g}, bound {bnd.reshape(-1)[i].item():.3g}"
        rows, keys = AC.exact_rows(s)
        exact += len(rows)
        if causal:
            assert rows[0].item() == 0 and keys[0].item() == 0
        if bf16x3:  # 1 * (v_hi + v_lo): the split of v is the whole error
            off = ((got[rows] - v[keys]).abs() - 2.0 ** -17 * v[keys].abs()).max(1).values
            assert bool((off <= 0).all()), f"head {h} row {rows[off.argmax()].item()} is not its dominant v row to 2^-17"
        else:
            same = (got[rows] == v[keys]).all(1)
            assert bool(same.all()), f"head {h} row {rows[(~same).nonzero()[0, 0]].item()} is not its dominant v row bit for bit"
    if L == 120 and pattern in ("sink", "last", "bigv"):
        assert exact >= (AC.B * AC.H * (2 if pattern == "last" and causal else T))
    if L == 120 and pattern == "diag" and (causal or T <= D):
        assert exact >= AC.B * AC.H * min(T, D)
    check_split_form(qkv, got_dev, D, T, causal, bf16x3)
    return worst, worst_err


@pytest.mark.parametrize("bf16x3", KERNELS)
@pytest.mark.parametrize("causal", CAUSAL)
@pytest.mark.parametrize("pattern,L", AC.PATTERN_CASES, ids=[f"{p}{L}" for p, L in AC.PATTERN_CASES])
@pytest.mark.parametrize("D,T", AC.SHAPES)
def test_attention_values_within_the_derived_bound(D, T, pattern, L, causal, bf16x3):
    worst, err = check_values(pattern, L, D, T, causal, bf16x3)
    print(f"attention values {'bf16x3' if bf16x3 else 'fp32'} {pattern} L={L} D={D} T={T} causal={causal}: "
          f"worst |got - float64| / bound = {worst:.3f} (max |got - float64| = {err:.3g})")


@pytest.mark.parametrize("causal", CAUSAL)
@pytest.mark.parametrize("D,T", AC.SHAPES + ((64, 161),))
def test_scaled_logits_table(D, T, causal):
    """`scaled` at L = 1, 30, 100, 300 through both kernels and through an explicit fp32 softmax(q k^T / sqrt(D)) v of torch on
    the device: max |out - float64| over the four heads.  The kernels are held to the bound; torch's figure is printed
    beside them, not asserted.  (64, 161) is the shape of the emulation table in docs/ATTENTION_VALUES.md."""
    for L in (1, 30, 100, 300):
        heads, _ = case("scaled", L, D, T)
        _, e32 = check_values("scaled", L, D, T, causal, False)
        _, e3 = check_values("scaled", L, D, T, causal, True)
        et = 0.0
        mask = torch.ones(T, T, dtype=torch.bool, device=DEV).triu_(1)
        for (q, k, v), (want, _, _) in zip(heads, references("scaled", L, D, T, causal)):
            qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
            s = (qd @ kd.T) * (D ** -0.5)
            if causal:
                s = s.masked_fill(mask, float("-inf"))
            et = max(et, ((torch.softmax(s, -1) @ vd).cpu().double() - want).abs().max().item())
        print(f"scaled table D={D} T={T} causal={causal} largest |logit| {L}: max |out - float64| fp32 kernel {e32:.2e}, "
              f"bf16x3 kernel {e3:.2e}, torch fp32 {et:.2e}")


@pytest.mark.parametrize("bf16x3", KERNELS)
@pytest.mark.parametrize("causal", CAUSAL)
@pytest.mark.parametrize("D,T", AC.SHAPES)
def test_a_head_does_not_depend_on_the_other_heads_of_the_call(D, T, causal, bf16x3):
    """`stairs` at L = 120 (every accumulator wiped at every key tile) beside three heads of the same pattern, then beside three
    `bigv` heads (a settled maximum and a 1e4 value row): the head's rows keep every bit, in each of the four slots."""
    mine, qkv = case("stairs", 120, D, T)
    base = AC.unpack(run(qkv, D, T, causal, bf16x3), T, D)
    others, _ = case("bigv", 40, D, T)
    for slot in range(AC.B * AC.H):
        mixed = list(others)
        mixed[slot] = mine[slot]
        got = AC.unpack(run(AC.pack(mixed, T, D).to(DEV), D, T, causal, bf16x3), T, D)
        assert torch.equal(got[slot], base[slot]), slot


@pytest.mark.parametrize("bf16x3", KERNELS)
@pytest.mark.parametrize("causal", CAUSAL)
@pytest.mark.parametrize("L", [40, 120])
@pytest.mark.parametrize("D,T", AC.SHAPES)
def test_wiped_accumulators_carry_nothing_over(D, T, L, causal, bf16x3):
    """`stairs`: a second call returns the same bits, and so does the same head placed in another slot of the call (another
    workgroup, after another head's rounds): nothing of m, l or o survives a round or a call."""
    heads, qkv = case("stairs", L, D, T)
    first = run(qkv, D, T, causal, bf16x3)
    assert torch.equal(run(qkv, D, T, causal, bf16x3), first)
    swapped = [heads[2], heads[3], heads[0], heads[1]]
    got = AC.unpack(run(AC.pack(swapped, T, D).to(DEV), D, T, causal, bf16x3), T, D)
    want = AC.unpack(first, T, D)
    for slot in range(4):
        assert torch.equal(got[slot], want[(slot + 2) % 4]), slot


@pytest.mark.parametrize("bf16x3", KERNELS)
@pytest.mark.parametrize("causal", CAUSAL)
@pytest.mark.parametrize("T", [1, 32])
@pytest.mark.parametrize("D", [64, 128])
def test_attention_single_key_and_one_full_tile(D, T, causal, bf16x3):
    """T = 1 (a single key) and T = 32 (a full tile without a padded key) on randn inputs against the suite's flat bars and
    float64; the rest of the suite runs these lengths at D = 64 without a mask only, against torch's fp32."""
    check_attention(D, T, causal, bf16x3, 2e-5 if bf16x3 else 2e-6)
