"""Every grid-stride kernel past its grid cap: the second, the ragged last and a third trip (docs/GRID_CAPS.md is the audit).

The launchers of `semanticlens_amd/csrc` clamp their grids (8 or 16 workgroups per CU, `4 x CUs x per_cu` one-wave items, a
fixed 4 096 or 65 535 blocks) and walk the rest of the work in a grid-stride loop.  The rest of the suite picks its shapes for
tile edges, alignment and special values, almost all of them small enough for one trip per workgroup.  Each test below restates
one site's cap from the device's CU count, asserts that its call crosses it, ends the work inside a trip (cap + a few items)
and, where the memory allows, repeats it with 2 x cap + 1 items so that a third trip exists.  The value of item i depends on i
(a trip that reads item i - grid again shows), the outputs hold NaN (or another wrong value) before the call (a skipped item
shows), and every item is compared, not a prefix.

References: data movement and the init kernels bit for bit against numpy / torch indexing; the one-add kernels against the
same fp32 add on the host; the Gram matrices against V V^T in `np.longdouble` with the bound D 2^-53 sum_d |a_d b_d| per entry
(the products of two fp32 values are exact in fp64 and both kernels add them one at a time); K9, K23, K25, K26, K17 and K10
against the references and bounds of their own test files."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import oracle
from semanticlens_amd import _native as N
from semanticlens_amd import scores
from test_gpu_cosine_paths import assert_cosine, gemm_mode, hard_rows
from test_gpu_label_distribution import reference as softmax_reference
from test_gpu_label_distribution import softmax_bound
from test_gpu_label_rank import SENTINEL, ref_counts
from test_gpu_parity import assert_polysemanticity_matches
from test_gpu_silhouette import TOL as SIL_TOL
from test_gpu_silhouette import sk_samples
from test_gpu_topk import assert_state_equal, ref_topk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def nan_block(numel: int, dtype=torch.float32):
    """Leave a NaN-filled block of this size in the allocator's cache (test_gpu_instances.py: `poison`): an output that the
    entry point allocates itself and a kernel then skips reads NaN, not an earlier call's (right) answer."""
    torch.full((max(int(numel), 1),), NAN, dtype=dtype, device=DEV)


def past(cap: int, unit: int = 1, few: int = 3):
    """The two item counts of a site, in units of `unit` items: just past the cap, ending inside the second trip, and at least
    2 x cap + 1, so that a third trip exists."""
    return (cap // unit + few, (2 * cap) // unit + few)


def ibits(t: torch.Tensor) -> torch.Tensor:
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ---- the caps, restated from the launchers ---------------------------------------------------------------------------------------
def cap_blocks8() -> int:  # `blocks > 8 x CUs`: kmeans.hip, silhouette.hip, gather.hip (wave kernel)
    return 8 * cus()


def cap_stride256() -> int:  # common.hpp: stride_grid_256, 8 x CUs workgroups of 256 threads, one item per thread
    return 8 * cus() * 256


def cap_grid_for() -> int:  # encoder.hip: grid_for, gather.hip (element kernel), gemm_bf16x3.hpp (launch_split): 16 x CUs x 256
    return 16 * cus() * 256


def cap_wave_grid(per_cu: int = 32) -> int:  # rowseg_tile.hpp: wave_grid, 4 x CUs x per_cu one-wave items
    return 4 * cus() * per_cu


def topk_per_cu(k: int) -> int:  # topk.hip: wave_grid(items, k) over lds_bytes(k) = 12 bytes x pow2_entries(k)
    entries = 256
    while entries < k + 128:  # the state and at least kMinBuf = 128 entries behind it
        entries *= 2
    return max(1, min(32, 160 * 1024 // (entries * 12)))


# ---- 1. K5: both gather kernels and the sharded form -----------------------------------------------------------------------------
N_ROWS = 101  # prime: the period of the ids is coprime to every grid size


def gather_table(D: int):
    e = (np.arange(N_ROWS * D, dtype=np.float32) * 0.5 - 7.0).reshape(N_ROWS, D)  # every element its own value
    return e, torch.from_numpy(e).to(DEV)


def gather_ids(n_ids: int) -> np.ndarray:
    i = np.arange(n_ids, dtype=np.int64)
    ids = (i * 37 + i // N_ROWS) % N_ROWS  # depends on i, period coprime to the grid
    return np.where(i % 3 == 0, ids - N_ROWS, ids)  # every third id negative: it wraps


@pytest.mark.parametrize("D,rpw", [(4, 8), (260, 4), (772, 2), (1796, 1)])
def test_gather_wave_kernel_past_its_grid(D, rpw):
    """`gather_rows_wave_kernel<RPW, PPL>` (gather.hip:94): 8 CUs workgroups x 4 waves x RPW rows per trip, one width class per
    RPW value.  cap + RPW + 1 ids: the last trip holds one full row group and one row of the next."""
    cap = cap_blocks8() * 4 * rpw
    e, emb = gather_table(D)
    for n_ids in (cap + rpw + 1, 2 * cap + 1):
        assert n_ids > cap and n_ids >= 64 and D % 4 == 0 and D <= 2048
        ids = gather_ids(n_ids)
        nan_block(n_ids * D)
        got = N.gather_rows(emb, torch.from_numpy(ids)).cpu().numpy()
        assert np.array_equal(got, e[ids]), (D, n_ids)
        del got
    bad = gather_ids(cap + rpw + 1)
    bad[-1] = N_ROWS  # out of range, in the last trip
    with pytest.raises(IndexError):
        N.gather_rows(emb, torch.from_numpy(bad))
    bad[-1] = -N_ROWS - 1
    with pytest.raises(IndexError):
        N.gather_rows(emb, torch.from_numpy(bad))


def test_gather_sharded_form_past_its_grid():
    D, rpw = 260, 4
    cap = cap_blocks8() * 4 * rpw
    n_ids = cap + rpw + 1
    assert n_ids > cap
    e, emb = gather_table(D)
    ids = gather_ids(n_ids)
    want = e[ids]
    src = np.where(ids < 0, ids + N_ROWS, ids)
    total = np.zeros_like(want)
    for lo, hi in ((0, 40), (40, 41), (41, N_ROWS)):
        nan_block(n_ids * D)
        part = N.gather_rows_shard(emb[lo:hi].contiguous(), torch.from_numpy(ids), lo, N_ROWS).cpu().numpy()
        mine = (src >= lo) & (src < hi)
        assert np.array_equal(part[mine], want[mine]) and not part[~mine].any(), (lo, hi)
        total += part
    assert np.array_equal(total, want)
    bad = ids.copy()
    bad[-1] = N_ROWS
    with pytest.raises(IndexError):
        N.gather_rows_shard(emb[:40].contiguous(), torch.from_numpy(bad), 0, N_ROWS)


@pytest.mark.parametrize("D", [30, 2052])
def test_gather_element_kernel_past_its_grid(D):
    """`gather_rows_kernel<VEC4>` (gather.hip:123): 16 CUs x 256 elements per trip; D = 30 is the scalar instance (items are
    floats), D = 2052 the float4 one (rows longer than the wave kernel takes; items are 16-byte pieces)."""
    cap = cap_grid_for()
    per_row = D // 4 if D % 4 == 0 else D
    e, emb = gather_table(D)
    for n_ids in past(cap, per_row, few=2):
        assert n_ids * per_row > cap and (D % 4 != 0 or D > 2048)
        ids = gather_ids(n_ids)
        nan_block(n_ids * D)
        got = N.gather_rows(emb, torch.from_numpy(ids)).cpu().numpy()
        assert np.array_equal(got, e[ids]), (D, n_ids)
        del got
    bad = gather_ids(cap // per_row + 2)
    bad[-1] = N_ROWS
    with pytest.raises(IndexError):
        N.gather_rows(emb, torch.from_numpy(bad))


# ---- 2. K11: the encoder's element kernels ---------------------------------------------------------------------------------------
def patches(img: torch.Tensor, P: int) -> torch.Tensor:
    B, C, Hi, Wi = img.shape
    gh, gw = Hi // P, Wi // P
    return img.reshape(B, C, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, C * P * P).contiguous()


@pytest.mark.parametrize("P,Hi,Wi", [(4, 8, 12), (2, 4, 6)])
def test_patchify_past_its_grid(P, Hi, Wi):
    """`patchify_kernel` (P = 4: items are float4) and `patchify_scalar_kernel` (P = 2: floats), encoder.hip:206 `grid_for`:
    fp32 output and the split-bf16 output, bit for bit against reshape / permute."""
    C, cap = 3, cap_grid_for()
    per_image = C * Hi * Wi // (4 if P % 4 == 0 else 1)
    for B in past(cap, per_image, few=2):
        items = B * per_image
        assert items > cap and items % (16 * cus() * 256) != 0
        img = (torch.arange(B * C * Hi * Wi, dtype=torch.float32, device=DEV) * 0.25 - 3.0).reshape(B, C, Hi, Wi)
        want = patches(img, P)
        out = torch.full_like(want, NAN)
        N.patchify(img, P, out=out)
        assert torch.equal(out, want), (P, B)
        sp = N.Split(want.shape[0], want.shape[1], DEV)
        sp.buf.fill_(NAN)
        N.patchify(img, P, out_split=sp)
        hi = want.bfloat16()
        lo = (want - hi.float()).bfloat16()
        assert torch.equal(ibits(sp.hi.contiguous()), ibits(hi)) and torch.equal(ibits(sp.lo.contiguous()), ibits(lo)), (P, B)
        del img, want, out, sp, hi, lo


def test_broadcast_row_past_its_grid():
    """`broadcast_row_kernel`: out[g * stride + c] = v[c] + add[c]; 7 columns (coprime to the grid), a row stride of 10 whose
    three trailing floats must stay as they were."""
    n, stride, cap = 7, 10, cap_grid_for()
    v = torch.arange(n, dtype=torch.float32, device=DEV) * 1.25 + 0.1
    add = torch.arange(n, dtype=torch.float32, device=DEV) * -0.3 + 1e-3
    for G in past(cap, n, few=2):
        assert G * n > cap
        for a in (add, None):
            out = torch.full((G, stride), NAN, device=DEV)
            N.broadcast_row(v, a, G, stride, out)
            want = (v.cpu() + a.cpu()) if a is not None else (v.cpu() + 0.0)
            got = out.cpu()
            assert torch.equal(got[:, :n], want.expand(G, n)), G
            assert bool(got[:, n:].isnan().all()), "wrote between the rows"


def test_embed_tokens_past_its_grid():
    """`embed_tokens_kernel`: out[b, t] = table[clamp(ids[b, t])] + pos[t]; ids from -3 to vocab + 2."""
    vocab, W, T, cap = 11, 6, 5, cap_grid_for()
    table = (torch.arange(vocab * W, dtype=torch.float32) * 0.37 - 2.0).reshape(vocab, W)
    pos = (torch.arange(T * W, dtype=torch.float32) * -0.011 + 0.5).reshape(T, W)
    for B in past(cap, T * W, few=2):
        assert B * T * W > cap
        i = torch.arange(B * T, dtype=torch.int64)
        ids = ((i * 7 + i // 17) % 17 - 3).reshape(B, T)
        assert int(ids.min()) < 0 and int(ids.max()) >= vocab
        want = (table[ids.clamp(0, vocab - 1)] + pos).reshape(B * T, W)  # the same fp32 add, on the host
        out = torch.full((B * T, W), NAN, device=DEV)
        N.embed_tokens(table.to(DEV), ids.to(DEV), pos.to(DEV), out=out)
        assert torch.equal(out.cpu(), want), B


@pytest.mark.parametrize("S", [255, 256, 639])
def test_tokens_from_map_at_the_raised_lds_limit(S):
    """`sl_tokens_from_map` raises its dynamic LDS limit when the 64 x (S + 1) fp32 tile passes 64 KiB (S >= 256) up to the
    160 KiB of S = 639; C = 70 leaves a partial last channel block.  The contract of
    test_tokens_from_map_and_per_image_query_pool_primitives: plain tokens bit-equal, the mean token within 2e-6."""
    B, C = 2, 70
    assert (64 * (S + 1) * 4 > 64 * 1024) == (S >= 256) and 64 * (S + 1) * 4 <= 160 * 1024
    g = torch.Generator(device=DEV).manual_seed(S)
    fmap = torch.randn(B, C, S, device=DEV, generator=g)
    pos = torch.randn(S + 1, C, device=DEV, generator=g)
    out = torch.full((B, S + 1, C), NAN, device=DEV)
    got = N.tokens_from_map(fmap.reshape(B, C, S, 1), pos, out=out)
    x = fmap.permute(0, 2, 1)
    want = torch.cat([x.mean(1, keepdim=True), x], 1) + pos
    assert torch.equal(got[:, 1:], want[:, 1:])
    assert torch.allclose(got, want, rtol=0, atol=2e-6)
    if S == 639:
        with pytest.raises(ValueError):
            N.tokens_from_map(torch.zeros(B, C, 640, 1, device=DEV), torch.zeros(641, C, device=DEV))


# ---- 3. the init and finish kernels of `stride_grid_256`, and `actmax_init_kernel` -----------------------------------------------
def test_init_kernels_past_their_grids():
    """`softmax_init_kernel`, `topk_init_kernel`, `unionfind_init_kernel` (stride_grid_256: 2 048 CUs items) and
    `actmax_init_kernel` (4 096 blocks of 256 whatever the device): every entry is the empty one, bit for bit."""
    cap = cap_stride256()
    for n in past(cap, few=5):
        assert n > cap
        nan_block(n * 4, torch.float64)
        sm = N.softmax_new(n, DEV)
        want = torch.tensor([-np.inf, 0.0, 0.0, 0.0], dtype=torch.float64, device=DEV)
        assert torch.equal(ibits(sm), ibits(want.expand(n, 4).contiguous())), n
        del sm
        a, b = (torch.full((n,), -5, dtype=torch.int32, device=DEV) for _ in range(2))
        del a, b
        parent, degree, status = N.unionfind_new(n, DEV)
        assert torch.equal(parent, torch.arange(n, dtype=torch.int32, device=DEV)) and not bool(degree.any()) and int(status) == 0
        del parent, degree
    for R in past(cap, 5, few=2):
        assert R * 5 > cap
        vals = torch.full((R, 5), NAN, device=DEV)
        ids = torch.full((R, 5), 7, dtype=torch.int64, device=DEV)
        N.topk_init(vals, ids)
        assert bool((vals == -np.inf).all()) and bool((ids == -1).all()), R
    cap = 4096 * 256
    for C in past(cap, 20, few=2):
        assert C * 20 > cap
        vals = torch.full((C, 20), 1.0, dtype=torch.bfloat16, device=DEV)
        ids = torch.full((C, 20), 7, dtype=torch.int64, device=DEV)
        N.actmax_init(vals, ids)
        assert bool((ibits(vals) == -0x8000).all()) and bool((ids == -1).all()), C  # -0.0 and -1


def order_key(v: np.ndarray) -> np.ndarray:
    """packed_best.hpp: f32_order_key for finite non-negative values"""
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) | np.uint32(0x80000000)


def test_finish_kernels_past_their_grid():
    """`mutualmax_finish_kernel`, `group_min_finish_kernel` and `unionfind_flatten_kernel` (stride_grid_256) on states packed by
    the test: entry i decodes to a value and an id of its own."""
    cap = cap_stride256()
    for n in past(cap, few=5):
        assert n > cap
        i = np.arange(n, dtype=np.int64)
        # K20: (order key << 32) | (2^32 - 1 - id); every seventh entry empty
        v = (i % 1009).astype(np.float32) * 0.5 + 0.25
        ids = (i * 3 + 11) % (1 << 20)
        packed = (order_key(v).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ids.astype(np.uint64))
        empty = i % 7 == 3
        packed[empty] = 0
        nan_block(n)
        nan_block(n, torch.float64)
        gv, gi = N.mutualmax_finish(torch.from_numpy(packed.view(np.int64)).to(DEV))
        assert np.array_equal(gv.cpu().numpy(), np.where(empty, -np.inf, v).astype(np.float32)), n
        assert np.array_equal(gi.cpu().numpy(), np.where(empty, -1, ids)), n
        # K24 cohesion: the value at state[labels[i]]; NaN for the empty key and for a label outside [0, n)
        labels = ((i * 7919 + 13) % n).astype(np.int32)
        labels[5::1013] = -1
        state = order_key(i.astype(np.float32) * 0.5 + 1.0).view(np.int32).copy()
        state[3::11] = -1
        nan_block(n)
        got = N.group_min_finish(torch.from_numpy(state).to(DEV), torch.from_numpy(labels).to(DEV)).cpu().numpy()
        lab = np.where(labels < 0, 0, labels)
        want = np.where((labels < 0) | (state[lab] == -1), np.nan, lab.astype(np.float32) * 0.5 + 1.0).astype(np.float32)
        assert np.array_equal(got, want, equal_nan=True), n
        # K24 forest: chains of three (parent[i] = i - 1 inside a chain): every entry ends at its chain's first id
        parent = np.where(i % 3 == 0, i, i - 1).astype(np.int32)
        dp = torch.from_numpy(parent).to(DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        N.unionfind_flatten(dp, status)
        assert np.array_equal(dp.cpu().numpy(), (i - i % 3).astype(np.int32)) and int(status) == 0, n


# ---- 4. the row-segment grid: K25, K26, K17 --------------------------------------------------------------------------------------
def rows_of_8(R: int, seed: int, n: int = 8) -> np.ndarray:
    """(R, n) fp32 in [-1, 1), the values of a row distinct: the order in a row is unambiguous"""
    rng = np.random.default_rng(seed)
    base = rng.permutation(4096)[:n].astype(np.float32) / 2048.0 - 1.0  # distinct, spaced by 2^-11
    v = base[None, :] + rng.uniform(0.0, 2.0 ** -12, size=(R, n)).astype(np.float32)
    return np.take_along_axis(v, rng.random((R, n)).argsort(1), 1).astype(np.float32)


def test_softmax_merge_and_finish_past_their_grids():
    """`softmax_tile_kernel` (softmax.hip:196, wave_grid: 128 CUs rows) and `softmax_finish_kernel` (stride_grid_256 over R x k
    probabilities): three tiles of 8 columns, k = 17, so that R x k passes 2 048 CUs as well."""
    cap, k, scale = cap_wave_grid(32), 17, 100.0
    for R in past(cap):
        assert R > cap and R * k > (R // cap) * cap_stride256() and N.lib().sl_softmax_merge_ws_bytes(R, 8) == 0
        vals = torch.from_numpy(rows_of_8(R, seed=R, n=24)).to(DEV)
        nan_block(R * 4, torch.float64)
        sm = N.softmax_new(R, DEV)
        sv, si = N.topk_new(R, k, DEV)
        for t in (2, 0, 1):
            tile = vals[:, 8 * t:8 * t + 8].contiguous()
            N.softmax_merge(sm, tile, scale)
            N.topk_merge(sv, si, tile, 8 * t)
        assert bool((sm[:, 3] == 24).all())
        nan_block(R * k)
        nan_block(R, torch.float64)
        probs, lz, h = N.softmax_finish(sm, scale, sv)
        want_lz, want_h, want_p = softmax_reference(vals, scale)
        b_lz, b_p, b_h = softmax_bound(scale, float(vals.max() - vals.min()), 24)
        p_ref = torch.gather(want_p, 1, si)
        big = p_ref > 1e-30
        e_lz, e_h = float((lz - want_lz).abs().max()), float((h - want_h).abs().max())
        e_p = float(((probs.double() - p_ref).abs() / p_ref)[big].max())
        print(f"softmax R={R}: log_z {e_lz:.2e} / {b_lz:.2e}, probs {e_p:.2e} / {b_p:.2e}, entropy {e_h:.2e} / {b_h:.2e}")
        assert not bool(torch.isnan(lz).any() | torch.isnan(h).any() | torch.isnan(probs).any())
        assert e_lz <= b_lz + 4 * 2.0 ** -53 * float(want_lz.abs().max()) and e_p <= b_p and e_h <= b_h
        assert float(probs[~big].max() if bool((~big).any()) else 0.0) <= 1e-29


def test_rank_merge_past_its_grid():
    """`rank_tile_kernel` (rank.hip:114, wave_grid: 128 CUs rows): exact against `ref_counts`."""
    cap = cap_wave_grid(32)
    for R in past(cap):
        assert R > cap and int(N.lib().sl_rank_merge_splits(R, 8)) == 1
        vals = rows_of_8(R, seed=R + 1)
        r = np.arange(R)
        # slot 0: a column's own value; slot 1: another column's value at an id behind the tile; slot 2: unused
        key_ids = np.stack([5 + r % 8, 5 + 8 + r % 3, np.full(R, -1)], 1).astype(np.int64)
        key_vals = np.stack([vals[r, r % 8], vals[r, (3 * r + 1) % 8], np.zeros(R)], 1).astype(np.float32)
        want = ref_counts(vals, 5, key_vals, key_ids, np.full((R, 3), SENTINEL, dtype=np.int64))
        counts = torch.full((R, 3), SENTINEL, dtype=torch.int64, device=DEV)
        N.rank_merge(counts, torch.from_numpy(vals).to(DEV), torch.from_numpy(key_vals).to(DEV), torch.from_numpy(key_ids).to(DEV), 5)
        assert np.array_equal(counts.cpu().numpy(), want), R
        # among 8 distinct values a column has 0 to 7 before it; the key behind the tile also has the column it copies before it
        assert (want[:, 2] == SENTINEL).all() and (want[:, 0] - SENTINEL).max() == 7 and (want[:, 1] - SENTINEL).max() == 8


@pytest.mark.parametrize("k", [5, 1024])
def test_topk_merge_past_its_grid(k):
    """`topk_tile_kernel` (topk.hip:263) and `topk_lists_kernel` (topk.hip:290, `topk_merge_states`), wave_grid with
    per_cu = min(32, 160 KiB / LDS bytes of k): 128 CUs rows at k = 5 (256 entries of 12 bytes), 24 CUs at k = 1 024 (2 048
    entries: six workgroups per CU).  Exact against `ref_topk`."""
    cap = cap_wave_grid(topk_per_cu(k))
    assert topk_per_cu(5) == 32 and topk_per_cu(1024) == 6
    for R in past(cap):
        assert R > cap and N.lib().sl_topk_merge_ws_bytes(R, k, 8) == 0
        vals = rows_of_8(R, seed=R + k, n=16)
        ids = 11 + np.arange(16, dtype=np.int64)
        want = ref_topk(vals, ids, k)
        sv = torch.full((R, k), NAN, device=DEV)
        si = torch.full((R, k), 7, dtype=torch.int64, device=DEV)
        N.topk_init(sv, si)
        N.topk_merge(sv, si, torch.from_numpy(np.ascontiguousarray(vals[:, 8:])).to(DEV), 11 + 8)
        N.topk_merge(sv, si, torch.from_numpy(np.ascontiguousarray(vals[:, :8])).to(DEV), 11)
        assert_state_equal((sv.cpu().numpy(), si.cpu().numpy()), want)
        del sv, si
        # the same entries as explicit (value, id) lists, an empty slot among them
        av, ai = N.topk_new(R, k, DEV)
        ov = np.concatenate([vals, np.full((R, 1), 9.0, dtype=np.float32)], 1)
        oi = np.concatenate([np.broadcast_to(ids, (R, 16)), np.full((R, 1), -1, dtype=np.int64)], 1)
        N.topk_merge_states(av, ai, torch.from_numpy(ov).to(DEV), torch.from_numpy(oi).to(DEV))
        assert_state_equal((av.cpu().numpy(), ai.cpu().numpy()), want)
        del av, ai, want


# ---- 5. the Gram matrices of K9 and K23 ------------------------------------------------------------------------------------------
GRAM = {"staged": 0.0, "general": 0.0, "entries": 0, "duplicates": 0}  # the largest |H - reference| / bound per kernel so far


def gram_input(C: int, n: int, D: int, seed: int) -> np.ndarray:
    """Gaussian rows scaled per component over six decades, row n - 1 a copy of row 1 (n >= 3) and row 0 of component 0 zero"""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((C, n, D)).astype(np.float32)
    V *= (10.0 ** rng.integers(-3, 4, size=(C, 1, 1))).astype(np.float32)
    V[:, n - 1] = V[:, 1]
    V[0, 0] = 0.0
    return V


def owned_ws(nbytes: int):
    """A workspace the test owns, every byte 0xFF (a NaN in any format), and the offset of its first 256-byte boundary"""
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    return ws, (-ws.data_ptr()) % 256


def gram_of(ws: torch.Tensor, off: int, C: int, n: int) -> np.ndarray:
    torch.cuda.synchronize()
    return ws[off:off + C * n * n * 8].view(torch.float64).view(C, n, n).cpu().numpy()


def gram_via_k9(V: np.ndarray, general: bool) -> np.ndarray:
    """H as `sl_poly2means_labels` (gram_kernel, kmeans.hip:662) or `sl_polykmeans_labels` (gram_general_kernel) leaves it"""
    C, n, D = V.shape
    lib, p = N.lib(), N._ptr
    Vd = torch.from_numpy(V).to(DEV)
    first, rand = scores.kmeans_draws(n, 2, 123, 2)
    first, rand = np.ascontiguousarray(first, dtype=np.int32), np.ascontiguousarray(rand, dtype=np.float64)
    score = torch.empty((C,), dtype=torch.float64, device=DEV)
    mc = torch.empty((C,), dtype=torch.int32, device=DEV)
    lab = torch.empty((C, n), dtype=torch.int32, device=DEV)
    nbytes = int(lib.sl_polykmeans_ws_bytes(C, n, D, 2, len(first)) if general else lib.sl_poly2means_ws_bytes(C, n, D))
    ws, off = owned_ws(nbytes)
    tail = (first.ctypes.data_as(N._vp), len(first), rand.ctypes.data_as(N._vp), 1, p(score), p(mc), p(lab), p(ws), nbytes, N._stream(Vd))
    rc = lib.sl_polykmeans_labels(p(Vd), C, n, D, 2, *tail) if general else lib.sl_poly2means_labels(p(Vd), C, n, D, *tail)
    torch.cuda.synchronize()
    assert rc == 0, lib.sl_last_error()
    return gram_of(ws, off, C, n)


def gram_via_k23(V: np.ndarray) -> np.ndarray:
    """H as `sl_silhouette` leaves it: gram_kernel (silhouette.hip:161) up to n = 128, gram_general_kernel above"""
    C, n, D = V.shape
    lib, p = N.lib(), N._ptr
    Vd = torch.from_numpy(V).to(DEV)
    labels = (torch.arange(C * n, dtype=torch.int32, device=DEV) % 2).view(1, C, n).contiguous()
    mean = torch.empty((1, C), dtype=torch.float64, device=DEV)
    nbytes = int(lib.sl_silhouette_ws_bytes(C, n, D))
    ws, off = owned_ws(nbytes)
    rc = lib.sl_silhouette(p(Vd), C, n, D, p(labels), 1, 2, 0, None, p(mean), p(ws), nbytes, N._stream(Vd))
    torch.cuda.synchronize()
    assert rc == 0, lib.sl_last_error()
    return gram_of(ws, off, C, n)


def assert_gram(H: np.ndarray, V: np.ndarray, kernel: str, tag):
    """|H - V V^T| <= D 2^-53 sum_d |a_d b_d| per entry against np.longdouble; H symmetric bit for bit; the duplicated rows'
    entries H[1][1], H[1][n-1], H[n-1][n-1] bit-equal (K9's "distance == 0" in Gram space rests on it)."""
    C, n, D = V.shape
    assert H.shape == (C, n, n) and not np.isnan(H).any(), (tag, "an entry was left unwritten")
    L = V.astype(np.longdouble)
    ref = np.einsum("cid,cjd->cij", L, L)
    bound = D * np.longdouble(2.0) ** -53 * np.einsum("cid,cjd->cij", np.abs(L), np.abs(L))
    err = np.abs(H.astype(np.longdouble) - ref)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    GRAM[kernel] = max(GRAM[kernel], ratio)
    GRAM["entries"] += H.size
    sym = np.array_equal(H.view(np.int64), np.ascontiguousarray(H.transpose(0, 2, 1)).view(np.int64))
    j = n - 1
    dup = [np.array_equal(H[:, 1, 1].view(np.int64), H[:, a, b].view(np.int64)) for a, b in ((1, j), (j, 1), (j, j))]
    GRAM["duplicates"] += C
    print(f"gram {kernel} {tag}: max |H - reference| / bound = {ratio:.3g} (largest so far: staged {GRAM['staged']:.3g}, general "
          f"{GRAM['general']:.3g}; {GRAM['entries']} entries), symmetric {sym}, duplicated rows bit-equal {all(dup)} "
          f"({GRAM['duplicates']} components so far)")
    assert (err <= bound).all(), (tag, kernel, ratio)
    assert sym, (tag, kernel, "H[i][j] and H[j][i] differ")
    assert all(dup), (tag, kernel, "the entries of two equal rows differ", dup)
    assert not H[0, 0].any() and not H[0, :, 0].any(), (tag, "the zero row")


@pytest.mark.parametrize("site", ["k9", "k23"])
def test_gram_kernel_past_its_grid(site):
    """`gram_kernel` (gram.hpp:20) from both launch sites, 8 CUs components per trip: C = cap + 3 and 2 cap + 1 at n = 4, D = 3."""
    cap = cap_blocks8()
    for C in past(cap):
        assert C > cap
        V = gram_input(C, 4, 3, seed=C)
        H = gram_via_k9(V, general=False) if site == "k9" else gram_via_k23(V)
        assert_gram(H, V, "staged", (site, C, 4, 3))


@pytest.mark.parametrize("D", [94, 95, 96, 191])
def test_gram_kernel_chunk_edge_at_128_samples(D):
    """n = 128 stages Dc = 48 KiB / (4 n) - 1 = 95 features at a time: one chunk that is not full, one full, a chunk of one
    feature behind a full one, two full ones and a chunk of one."""
    V = gram_input(3, 128, D, seed=D)
    assert_gram(gram_via_k9(V, general=False), V, "staged", ("k9", 3, 128, D))
    assert_gram(gram_via_k23(V), V, "staged", ("k23", 3, 128, D))


@pytest.mark.parametrize("D", [1, 7])
def test_gram_general_kernel_behind_the_switch(D):
    """n = 129 is the first n of `gram_general_kernel`; its 129^2 = 16 641 pairs also pass the 64 x 256 threads its grid.x is
    clamped to (kmeans.hip:688, silhouette.hip:166), and n = 182 (33 124 pairs) makes a third trip.  n = 128 at the same D is
    the other side of the switch."""
    for n, trips in ((129, 2), (182, 3)):
        assert n * n > (trips - 1) * 64 * 256
        V = gram_input(2, n, D, seed=n + D)
        assert_gram(gram_via_k9(V, general=True), V, "general", ("k9", 2, n, D))
        assert_gram(gram_via_k23(V), V, "general", ("k23", 2, n, D))
    V = gram_input(2, 128, D, seed=128 + D)
    assert_gram(gram_via_k9(V, general=False), V, "staged", ("k9", 2, 128, D))
    assert_gram(gram_via_k23(V), V, "staged", ("k23", 2, 128, D))


def test_k9_past_the_gram_grid(monkeypatch):
    """K9 (k = 2, LDS variant) with C = 8 CUs + 37 components of n = 6, D = 8, well separated blobs: one launch against launches
    of at most 4 CUs components, bit for bit on scores and labels; components [cap, C) against scikit-learn."""
    cap = cap_blocks8()
    C, n, D = cap + 37, 6, 8
    assert C > cap
    rng = np.random.RandomState(C + n + D)
    V = rng.randn(C, n, D).astype(np.float32)
    centers = rng.randn(C, 2, D).astype(np.float32) * 2
    assign = rng.randint(0, 2, size=(C, n))
    assign[:, :2], assign[:, 2:4] = 0, 1  # two samples of each blob at least: no blob of one sample, so no fallback row
    V = centers[np.arange(C)[:, None], assign] + 0.5 * V  # the "blobs" recipe of test_polysemanticity_vs_sklearn_oracle
    Vd = torch.from_numpy(V).to(DEV)
    first, rand = scores.kmeans_draws(n, 10, 123, 2)

    def run():
        nan_block(C, torch.float64)
        lab = torch.full((C, n), -1, dtype=torch.int32, device=DEV)
        return N.poly2means(Vd, first, rand, True, n_clusters=2, labels=lab), lab

    monkeypatch.delenv("SL_POLY_WS_GB", raising=False)
    whole, whole_lab = run()
    monkeypatch.setattr(N, "POLYK_MAX_COMPONENTS", cap // 2)
    parts, parts_lab = run()
    monkeypatch.undo()
    assert torch.equal(ibits(whole), ibits(parts)) and torch.equal(whole_lab, parts_lab)
    assert bool(((whole_lab == 0) | (whole_lab == 1)).all())
    tail = V[cap:]
    _, fallback = oracle.polysemanticity(tail, n_clusters=2, return_fallback=True)
    assert not fallback.any(), "the seed gives a fallback row: choose another"
    assert_polysemanticity_matches(whole.cpu().numpy()[cap:], tail, "past the cap")


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_silhouette_past_the_gram_grid(monkeypatch, metric):
    """K23 with C = 8 CUs + 5 components of n = 4, D = 3 under m = 2 label sets: one launch against chunked launches bit for
    bit; components [cap, C) against scikit-learn's float64 silhouette_samples."""
    cap = cap_blocks8()
    C, n, D = cap + 5, 4, 3
    assert C > cap
    rng = np.random.RandomState(C)
    V = rng.randn(C, n, D).astype(np.float32)
    patterns = np.array([[0, 0, 1, 1], [0, 1, 0, 1], [0, 1, 1, 0], [0, 1, 2, 2], [2, 0, 2, 1], [1, 1, 2, 0]], dtype=np.int32)
    c = np.arange(C)
    labels = np.stack([patterns[c % 6], patterns[(c // 6 + 1) % 6]])  # (2, C, n): depends on c
    Vd, ld = torch.from_numpy(V).to(DEV), torch.from_numpy(labels).to(DEV)
    monkeypatch.delenv("SL_POLY_WS_GB", raising=False)
    nan_block(2 * C * n, torch.float64)
    nan_block(2 * C, torch.float64)
    whole = N.silhouette(Vd, ld, 3, metric)
    monkeypatch.setattr(N, "POLYK_MAX_COMPONENTS", cap // 2)
    chunked = N.silhouette(Vd, ld, 3, metric)
    monkeypatch.undo()
    for a, b in zip(whole, chunked):
        assert a.shape == b.shape and torch.equal(ibits(a), ibits(b))
    samples, mean = whole[0].cpu().numpy(), whole[1].cpu().numpy()
    assert not np.isnan(samples).any() and not np.isnan(mean).any()
    want = np.stack([[sk_samples(V[cc], labels[s, cc], metric) for cc in range(cap, C)] for s in range(2)])
    err_s = np.abs(samples[:, cap:] - want).max()
    err_m = np.abs(mean[:, cap:] - want.mean(-1)).max()
    print(f"K23 past the cap, {metric}: max sample error {err_s:.2e}, max mean error {err_m:.2e}")
    assert err_s <= SIL_TOL and err_m <= SIL_TOL


# ---- 6. K10 and the cosine path's operand preparation ----------------------------------------------------------------------------
def test_template_mean_past_its_grid():
    """`template_mean_kernel` (scores.hip:299): 65 535 blocks of 256 whatever the device; T = 1, D = 8, Q D = cap + 24 and
    2 cap + 24.  The float64 reference and the bound (T + 5) 2^-24 max(|E|, |E0|) of test_gpu_cosine_paths.py::test_template_mean,
    the reference taken in four row blocks to keep the float64 copies small."""
    cap, T, D = 65535 * 256, 1, 8
    for Q in past(cap, D):
        assert Q * D > cap
        g = torch.Generator(device=DEV).manual_seed(Q)
        E0 = torch.randn(T, D, device=DEV, generator=g) * 3.0
        E = torch.randn(Q * T, D, device=DEV, generator=g) * 3.0
        E[:, 0] = E0[0, 0] * (1.0 + 1e-6 * torch.randn(Q, device=DEV, generator=g))
        bound = (T + 5) * 2.0 ** -24 * max(E.abs().max().item(), E0.abs().max().item())
        nan_block(Q * D)
        got = N.template_mean(E, E0, Q)
        assert got.shape == (Q, D) and got.dtype == torch.float32
        err = 0.0
        for lo in range(0, Q, (Q + 3) // 4):
            hi = min(Q, lo + (Q + 3) // 4)
            want = (E[lo:hi].double().view(hi - lo, T, D) - E0.double()).mean(1)
            e = (got[lo:hi].double() - want).abs().max().item()
            err = max(err, e) if e == e else NAN
        print(f"template_mean ({Q}, {T}, {D}): max |got - float64| = {err:.3g} (bound {bound:.3g})")
        assert err <= bound, (Q, err, bound)
        del E, got, want


def test_split_bf16_past_its_grid():
    """`split_bf16_kernel` (gemm_bf16x3.hpp:337, 16 CUs x 256 elements of the padded matrix per trip), the one operand
    preparation launch of the cosine path that no other test carries past its cap.  Directly (`Split.of`, K = 4 padded to 32
    columns, with and without a row scale): hi = bf16(v), lo = bf16(v - hi), the padding zero, bit for bit.  Through the cosine
    path: 33 layers take the unfused route, whose query goes through `row_inv_norm_kernel` and this kernel with a row scale;
    Q x 64 elements pass the cap, and the cosines meet the float64 bound of test_gpu_cosine_paths.py."""
    cap = cap_grid_for()
    for R in past(cap, 32):
        assert R * 32 > cap
        g = torch.Generator(device=DEV).manual_seed(R)
        x = torch.randn(R, 4, device=DEV, generator=g) * (1.0 + torch.arange(R, device=DEV, dtype=torch.float32)[:, None] % 97)
        scale = 0.5 + torch.rand(R, device=DEV, generator=g)
        for s in (None, scale):
            v = x if s is None else x * s[:, None]
            nan_block(R * 64, torch.bfloat16)
            sp = N.Split.of(x, s)
            hi = v.bfloat16()
            lo = (v - hi.float()).bfloat16()
            assert torch.equal(ibits(sp.hi.contiguous()), ibits(hi)) and torch.equal(ibits(sp.lo.contiguous()), ibits(lo)), R
            full = sp.buf.view(R, 2, 32)
            assert not bool(full[:, :, 4:].view(torch.int16).any()), "the padding is not zero"
    Q, K = cap // 64 + 3, 64
    sizes = tuple(1 + (i % 5) for i in range(33))
    assert Q * K > cap and len(sizes) > 32
    x, y, sp = hard_rows(Q, sum(sizes), K, seed=33)
    ys = [part.clone() for part in y.split(list(sizes))]
    with gemm_mode("bf16x3"):
        for s in sizes:
            nan_block(Q * s)
        outs = N.similarity_multi(x, ys)
    assert outs is not None and len(outs) == 33
    assert_cosine(torch.cat(outs, 1), x, y, sp, "bf16x3", (Q, K, "33 layers"))


# ---- 7. K1 / K2 / K3: reduce kernels whose grids `grid_blocks` clamps, and the fused BatchNorm + pool ---------------------------
def test_abs_norm_rows_past_its_grid():
    """`abs_norm_rows_kernel` (reduce.hip:292): one workgroup per row, 8 CUs workgroups, the row sum through LDS that the next row
    reuses.  Integer data: the sum is exact in any order, so the result equals the oracle's bit for bit."""
    cap = cap_blocks8()
    for B in past(cap):
        assert B > cap
        rng = np.random.default_rng(B)
        x = rng.integers(-6, 7, size=(B, 5)).astype(np.float32) * (1 + np.arange(B, dtype=np.float32)[:, None] % 13)
        x[7] = 0.0
        got = N.abs_norm_rows(torch.from_numpy(x).to(DEV)).cpu().numpy()
        assert np.array_equal(got, oracle.abs_norm_rows(x)), B


def test_generic_reduce_past_its_grid():
    """`generic_reduce_kernel` (reduce.hip:88, 16 CUs x 256 outputs per trip) takes what no other kernel does, here an fp32 tensor
    one float past a 16-byte boundary.  max equals torch.amax bit for bit; the sum of integer data is exact."""
    cap = cap_grid_for()
    C = 257
    for B in past(cap, C, few=2):
        assert B * C > cap
        buf = torch.empty(B * C * 3 + 4, device=DEV)
        x = buf[1:1 + B * C * 3].view(B, C, 1, 3)
        g = torch.Generator(device=DEV).manual_seed(B)
        x.copy_(torch.randint(-50, 51, (B, C, 1, 3), device=DEV, generator=g).float())
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
        for code, want in ((N.SL_CONV_MAX, x.amax((2, 3))), (N.SL_CONV_SUM, x.double().sum((2, 3)).float())):
            out = torch.full((B, C), NAN, device=DEV)
            cand = torch.full((B, C), NAN, dtype=torch.bfloat16, device=DEV)
            N.reduce_conv(x, code, cand, out)
            assert torch.equal(out, want) and torch.equal(ibits(cand), ibits(want.bfloat16())), (B, code)
        del buf, x, out, cand, want


@pytest.mark.parametrize("dt,F", [(torch.float32, 8), (torch.float16, 16), (torch.bfloat16, 12)])
def test_token_reduce_past_its_grid(dt, F):
    """`colreduce2_kernel` (reduce_col.hip:231) and, for a half-precision width that is no multiple of eight, the column kernel
    behind it (reduce_col.hip:304): tasks are (batch, chunk of features) pairs, 8 CUs workgroups.  (B, 3, F) tokens with one
    chunk per batch, B = cap + 3 and 2 cap + 3: max and absmax over the tokens, exact."""
    cap = cap_blocks8()
    for B in past(cap):
        assert B > cap
        g = torch.Generator(device=DEV).manual_seed(B + F)
        x = (torch.randn(B, 3, F, device=DEV, generator=g) * 4).to(dt)
        for code, want in ((N.SL_TOK_MAX, x.float().amax(1)), (N.SL_TOK_ABSMAX, x.float().abs().amax(1))):
            out = torch.full((B, F), NAN, device=DEV)
            cand = torch.full((B, F), NAN, dtype=torch.bfloat16, device=DEV)
            N.reduce_tokens(x, code, 0, cand, out)
            assert torch.equal(out, want) and torch.equal(ibits(cand), ibits(want.bfloat16())), (dt, B, code)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("rows", ["odd", "sixteens"])
def test_row_reduce_of_one_element_rows_past_its_grid(dt, rows):
    """The row kernels (reduce_row.hip:260 for rows that do not group into tasks, :271 for those that do; reduce_row_half.hip:132
    and reduce_dma.hpp:234 in half precision and from 8 MiB on) give a workgroup 4 x U x 64 / G rows per trip, at most 512.  With
    H = W = 1 a row is one element, so 4 096 CUs + a few rows pass the cap of every instance in 4 MiB, and max is the identity."""
    cap = 8 * cus() * 512
    for R in (cap + 3, 2 * cap + 3) if rows == "odd" else (cap + 16, 2 * cap + 16):
        assert R > cap and (R % 2 == 1) == (rows == "odd")
        B = 1 if rows == "odd" else 16
        g = torch.Generator(device=DEV).manual_seed(R)
        x = (torch.randn(B, R // B, 1, 1, device=DEV, generator=g) * 4).to(dt)
        out = torch.full((B, R // B), NAN, device=DEV)
        cand = torch.full((B, R // B), NAN, dtype=torch.bfloat16, device=DEV)
        N.reduce_conv(x, N.SL_CONV_MAX, cand, out)
        want = x.float().view(B, R // B)
        assert torch.equal(out, want) and torch.equal(ibits(cand), ibits(want.bfloat16())), (dt, R)


def test_bn_relu_maxpool_past_its_grid():
    """`sl_batchnorm_infer_relu_maxpool` (batchnorm.hip:458): planes x bands work items over 8 workgroups per CU for small planes.
    (1, 8 CUs + 3, 8, 8) and (2, 8 CUs + 1, 8, 8) with the inputs, the reference and the bit-for-bit contract of
    test_gpu_bn_pool.py."""
    from test_gpu_bn_pool import _inputs, _mismatches, _reference

    cap = cap_blocks8()
    pool = ((3, 3), (2, 2), (1, 1))
    for B, C in ((1, cap + 3), (2, cap + 1)):
        assert B * C > B * cap and C <= N.BN_MAX_CHANNELS and 8 * 8 * 4 * 8 <= 160 * 1024
        x, mean, var, weight, bias = _inputs(B, C, 8, 8, seed=C)
        want = _reference(x, mean, var, weight, bias, 1e-5, pool)
        nan_block(want.numel())
        got = N.batchnorm_infer_relu_maxpool(x, mean, var, weight, bias, 1e-5, *pool)
        assert _mismatches(got, want) == 0, (B, C)
