"""The attention value cases on the host (no GPU): every case of tests/test_gpu_attention_values.py is what its name says,
the restated arithmetic of both kernels stays within HALF the derived bound on it, and the suite's flat bars do not hold at
large logits.  docs/ATTENTION_VALUES.md has the table."""
import math
from functools import lru_cache

import pytest
import torch

import attention_cases as AC

CASES = [(D, T, causal, pattern, L) for D, T in AC.SHAPES for causal in (False, True) for pattern, L in AC.PATTERN_CASES]
IDS = [f"{p}{L}-D{D}-T{T}-{'causal' if c else 'full'}" for D, T, c, p, L in CASES]


@lru_cache(maxsize=None)
def heads(pattern, L, D, T):
    return AC.case_heads(pattern, L, D, T)


@lru_cache(maxsize=None)
def references(pattern, L, D, T, causal):
    return [AC.reference(q, k, v, causal) for q, k, v in heads(pattern, L, D, T)]


def tile_maxima(s, T):
    """per row, the maximum over each 32-key tile that has an unmasked key"""
    return [s[:, t0:t0 + 32].max(1).values for t0 in range(0, T, 32)]


@pytest.mark.parametrize("D,T,causal,pattern,L", CASES, ids=IDS)
def test_the_case_is_what_it_says(D, T, causal, pattern, L):
    assert T % 32 == 1 and T > 32  # every shape: a last key tile with one valid key and 31 padded ones
    vis = ~AC._mask(T, causal)
    for (q, k, v), (want, s, p) in zip(heads(pattern, L, D, T), references(pattern, L, D, T, causal)):
        assert q.dtype == k.dtype == v.dtype == torch.float32 and q.shape == k.shape == v.shape == (T, D)
        assert torch.isfinite(want).all() and (p.sum(1) - 1).abs().max().item() < 1e-12
        fin = s[vis]
        rows, keys = AC.exact_rows(s)
        if causal:
            assert rows[0].item() == 0 and keys[0].item() == 0  # row 0 has a single key
        if pattern in ("sink", "bigv"):
            assert L - 1 < s[:, 0].min().item() and s[:, 0].max().item() < L + 1 and fin.min().item() > -1
            assert s[:, 1:][vis[:, 1:]].abs().max().item() < 1
            assert (s.argmax(1) == 0).all()
            assert rows.numel() == (T if L == 120 else int(causal))
            if pattern == "bigv":
                assert v[T // 2].abs().max().item() > 1e4 and p[:, T // 2].max().item() < 1e-15
        elif pattern == "last":
            assert abs(s[T - 1, T - 1].item() - L) < 1 and s[:, :T - 1][vis[:, :T - 1]].abs().max().item() < 1
            assert 1 - p[T - 1, T - 1].item() < T * math.exp(2 - L)
            if L == 120:  # every row that sees the last key is (0, ..., 0, 1); under `causal` that is the last row alone
                assert rows.tolist() == ([0, T - 1] if causal else list(range(T)))
                assert keys[-1].item() == T - 1
        elif pattern in ("stairs", "stairs_down"):
            tm = tile_maxima(s, T)
            for t in range(1, len(tm)):
                seen = torch.isfinite(tm[t])  # rows whose causal mask leaves a key of tile t
                rise = (tm[t] - tm[t - 1])[seen]
                assert seen.any() and (rise * (1 if pattern == "stairs" else -1) - L).abs().max().item() < 1, t
            assert abs(fin.abs().max().item() - L * ((T - 1) // 32)) < 1
        elif pattern == "mixed":
            i = torch.arange(T)
            peak = s.argmax(1)
            sees_last = vis[:, T - 2]
            assert (peak[(i % 2 == 0) & sees_last] == T - 2).all() and ((i % 2 == 0) & sees_last).any()
            assert (peak[(i % 2 == 1)] == 1).all()
            assert abs(fin.max().item() - L) < 1 and abs(fin.min().item() + L) < 1
        elif pattern == "diag":
            assert (s.argmax(1) == torch.arange(T)).all()
            assert (s.diagonal() - L).abs().max().item() < 1e-3 * L
            # the run of D rows a row belongs to is orthonormal: those logits vanish against L
            run = (torch.arange(T)[:, None] // D) == (torch.arange(T)[None, :] // D)
            off = run & vis & ~torch.eye(T, dtype=torch.bool)
            assert s[off].abs().max().item() < 1e-3
            if L == 120:  # no set of 257 unit vectors in 32 dimensions keeps every cosine below 1 - 105 / 120: exact rows are
                want_rows = min(T, D) if (causal or T <= D) else 0  # those that see only their own orthonormal run
                assert rows.numel() >= want_rows and (keys == rows).all()
                assert rows[:want_rows].tolist() == list(range(want_rows))
        elif pattern == "uniform":
            assert fin.abs().max().item() == 0.0
            assert (p[vis] - (1.0 / vis.sum(1, keepdim=True).double()).expand(T, T)[vis]).abs().max().item() < 1e-15
        elif pattern == "scaled":
            full = AC.reference(q, k, v, False)[1]
            assert abs(full.abs().max().item() / L - 1) < 0.01
        else:
            raise AssertionError(pattern)


@pytest.mark.parametrize("bf16x3", [False, True], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("D,T,causal,pattern,L", CASES, ids=IDS)
def test_the_restated_arithmetic_stays_within_half_the_bound(D, T, causal, pattern, L, bf16x3):
    worst = 0.0
    for (q, k, v), (want, s, p) in zip(heads(pattern, L, D, T), references(pattern, L, D, T, causal)):
        got = AC.emulate(q, k, v, causal, bf16x3)
        assert torch.isfinite(got).all()
        err = (got.double() - want).abs()
        bnd = AC.bound(q, k, v, causal, p, bf16x3)
        ratio = err / bnd
        ratio[(err == 0) & (bnd == 0)] = 0.0
        i = ratio.argmax()
        worst = max(worst, ratio.reshape(-1)[i].item())
        assert bool((err <= 0.5 * bnd).all()), (i.item() // D, i.item() % D, err.reshape(-1)[i].item(), bnd.reshape(-1)[i].item())
        rows, keys = AC.exact_rows(s)  # the exact statements of the GPU file, on the emulation
        tol = 2.0 ** -17 * v[keys].abs() if bf16x3 else torch.zeros(len(rows), D)
        assert bool(((got[rows] - v[keys]).abs() <= tol).all())
    print(f"emulation {'bf16x3' if bf16x3 else 'fp32'} {pattern} L={L} D={D} T={T} causal={causal}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("L", [30, 100, 300])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D,T", AC.SHAPES)
def test_the_flat_bars_do_not_hold_at_large_logits(D, T, causal, L):
    """Why tests/test_gpu_attention_values.py has a bound of its own: on `scaled` inputs from L = 30 on, the correct
    split-bf16 arithmetic is further from float64 than 2e-5 max(1, max |want|), the bar the suite holds the bf16x3 kernel to
    on randn inputs (the largest error over the case's four heads against the bar of the head it falls in)."""
    over = []
    for (q, k, v), (want, _, _) in zip(heads("scaled", L, D, T), references("scaled", L, D, T, causal)):
        err = (AC.emulate(q, k, v, causal, True).double() - want).abs().max().item()
        over.append(err / (2e-5 * max(1.0, want.abs().max().item())))
    print(f"scaled L={L} D={D} T={T} causal={causal}: bf16x3 emulation at {max(over):.2f} of the flat bar (per head: {[round(o, 2) for o in over]})")
    assert max(over) > 1.0, over
