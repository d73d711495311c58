"""K20 on the device: the mutual-max kernel against a numpy lexsort (ids exact, values bit for bit after the two mappings the
packing makes), the tiled cosine + mutual-max driver against the float64 cosine, the compare API, and the memory bound.

``TOL`` is the project's bound for cosine values (1e-4).  Where ids are compared exactly the inputs are constructed so that the
float64 cosine of the best match leads the runner-up by more than 4 * TOL in both directions, and that is asserted first."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from semanticlens_amd import _native as N
from semanticlens_amd import lens as L

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda"
MAX_ID = (1 << 32) - 2
CANONICAL_NAN = np.uint32(0x7FC00000)


# ---------------------------------------------------------------------------------------------------------------------
# kernel, exact
# ---------------------------------------------------------------------------------------------------------------------
def special_matrix(R: int, n: int, seed: int) -> np.ndarray:
    """Heavy exact ties, +-0.0, +-inf, NaN, mixed with a few distinct values (the recipe of test_gpu_topk.special_matrix)."""
    rng = np.random.default_rng(seed)
    pool = np.array([-np.inf, -1.0, -0.0, 0.0, 0.5, 0.5, 1.0, np.inf, np.nan, 0.25, -0.25, 1e-30, -1e-30], dtype=np.float32)
    v = pool[rng.integers(0, len(pool), size=(R, n))]
    mix = rng.random((R, n)) < 0.3
    v[mix] = rng.standard_normal(int(mix.sum())).astype(np.float32).round(1)  # one decimal: still many ties
    return v


def ref_best(vals: np.ndarray, id_base: int):
    """numpy reference per row: the first entry of a lexsort on (is-NaN descending, value descending, id ascending)."""
    R, n = vals.shape
    ids = id_base + np.arange(n, dtype=np.int64)
    out_v = np.empty(R, dtype=np.float32)
    out_i = np.empty(R, dtype=np.int64)
    for r in range(R):
        v = vals[r]
        nan = np.isnan(v)
        key = np.where(nan, 0.0, v).astype(np.float64) + 0.0  # -0.0 and +0.0 compare equal
        best = np.lexsort((ids, -key, ~nan))[0]
        out_v[r], out_i[r] = v[best], ids[best]
    return out_v, out_i


def canonical_bits(v: np.ndarray) -> np.ndarray:
    """Bit patterns after -0.0 -> +0.0 and NaN -> the canonical quiet NaN (what the packed state keeps of a value)."""
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).copy()
    bits[bits == np.uint32(0x80000000)] = 0
    bits[np.isnan(v)] = CANONICAL_NAN
    return bits


def run_tiles(vals: np.ndarray, n_tiles: int, row_base: int, col_base: int, seed: int, unaligned: bool):
    """Fold ``vals`` into fresh states as ``n_tiles`` tiles, cut along rows and along columns, in shuffled order; returns the
    raw states and their decoded forms."""
    R, B = vals.shape
    if n_tiles == 64 and min(R, B) > 1:
        grid_r, grid_c = 8, 8  # (3, 5) leaves some of the 64 empty: they are skipped
    else:  # one cut direction: along the longer side
        grid_r, grid_c = (n_tiles, 1) if R >= B else (1, n_tiles)
    rcuts = np.linspace(0, R, grid_r + 1).astype(np.int64)
    ccuts = np.linspace(0, B, grid_c + 1).astype(np.int64)
    row_state = torch.zeros(R, dtype=torch.int64, device=DEV)
    col_state = torch.zeros(B, dtype=torch.int64, device=DEV)
    full = torch.from_numpy(vals).to(DEV)
    for t in np.random.default_rng(seed).permutation(grid_r * grid_c):
        ra, rb = int(rcuts[t // grid_c]), int(rcuts[t // grid_c + 1])
        ca, cb = int(ccuts[t % grid_c]), int(ccuts[t % grid_c + 1])
        if rb == ra or cb == ca:
            continue
        if unaligned:  # a view that starts 4 bytes past a 16-byte boundary, with a row stride that is not a multiple of 4
            w = cb - ca
            buf = torch.full((rb - ra, w + 3 + (w % 2 == 1)), float("nan"), dtype=torch.float32, device=DEV)
            assert buf.stride(0) % 2 == 1
            buf[:, 1 : 1 + w] = full[ra:rb, ca:cb]
            tile = buf[:, 1 : 1 + w]
            assert tile.data_ptr() % 16 == 4
        else:
            tile = full[ra:rb, ca:cb].contiguous()
        N.mutualmax_merge(row_state[ra:rb], col_state[ca:cb], tile, row_base + ra, col_base + ca)
    rv, ri = N.mutualmax_finish(row_state)
    cv, ci = N.mutualmax_finish(col_state)
    torch.cuda.synchronize()
    return (row_state.cpu().numpy(), col_state.cpu().numpy()), tuple(t.cpu().numpy() for t in (rv, ri, cv, ci))


@pytest.mark.parametrize("R,B", [(1, 1), (3, 5), (65, 257), (300, 4099), (4099, 300), (1, 70001), (70001, 1)])
def test_kernel_exact_against_lexsort(R, B):
    vals = special_matrix(R, B, seed=R * 1000 + B)
    row_base, col_base = MAX_ID - R - 3, MAX_ID + 1 - B  # the last column has the largest id a state can hold
    want_rv, want_ri = ref_best(vals, col_base)
    want_cv, want_ci = ref_best(np.ascontiguousarray(vals.T), row_base)
    first = None
    for n_tiles in (1, 7, 64):
        states, (rv, ri, cv, ci) = run_tiles(vals, n_tiles, row_base, col_base, seed=n_tiles, unaligned=(n_tiles == 7))
        assert np.array_equal(ri, want_ri), f"{n_tiles} tiles: row ids differ in {int((ri != want_ri).sum())} entries"
        assert np.array_equal(ci, want_ci), f"{n_tiles} tiles: column ids differ in {int((ci != want_ci).sum())} entries"
        assert np.array_equal(canonical_bits(rv), canonical_bits(want_rv)), f"{n_tiles} tiles: row value bit patterns differ"
        assert np.array_equal(canonical_bits(cv), canonical_bits(want_cv)), f"{n_tiles} tiles: column value bit patterns differ"
        assert np.array_equal(rv.view(np.uint32), canonical_bits(rv))  # what comes back IS canonical
        if first is None:
            first = states
        assert np.array_equal(states[0], first[0]) and np.array_equal(states[1], first[1])  # the cut and its order do not show


def test_all_nan_column_and_untouched_entries():
    R, B = 70, 1030
    vals = special_matrix(R, B, seed=5)
    vals[:, 17] = np.nan
    vals[3, :] = np.nan
    row_state = torch.zeros(R + 9, dtype=torch.int64, device=DEV)
    col_state = torch.zeros(B + 5, dtype=torch.int64, device=DEV)
    N.mutualmax_merge(row_state[4 : 4 + R], col_state[2 : 2 + B], torch.from_numpy(vals).to(DEV), 100, 200)
    rv, ri = (t.cpu().numpy() for t in N.mutualmax_finish(row_state))
    cv, ci = (t.cpu().numpy() for t in N.mutualmax_finish(col_state))
    for v, i, lo, n in ((rv, ri, 4, R), (cv, ci, 2, B)):  # what no merge touched is empty
        outside = np.r_[0:lo, lo + n : len(v)]
        assert np.isneginf(v[outside]).all() and (i[outside] == -1).all()
        assert (i[lo : lo + n] >= 0).all()
    assert cv[2 + 17].view(np.uint32) == CANONICAL_NAN and ci[2 + 17] == 100  # all NaN: ties go to the smallest row id
    assert rv[4 + 3].view(np.uint32) == CANONICAL_NAN and ri[4 + 3] == 200
    want_rv, want_ri = ref_best(vals, 200)
    assert np.array_equal(ri[4 : 4 + R], want_ri)
    empty = N.mutualmax_finish(torch.zeros(5, dtype=torch.int64, device=DEV))
    assert torch.isneginf(empty[0]).all() and (empty[1] == -1).all()
    none = N.mutualmax_finish(torch.zeros(0, dtype=torch.int64, device=DEV))
    assert none[0].shape == (0,) and none[1].dtype == torch.int64


def test_merge_refuses_ids_out_of_range_and_wrong_states():
    tile = torch.zeros(4, 8, device=DEV)
    rs, cs = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="2\\^32 - 2"):
        N.mutualmax_merge(rs, cs, tile, MAX_ID - 2, 0)
    with pytest.raises(ValueError, match="does not fit"):
        N.mutualmax_merge(cs, rs, tile)
    with pytest.raises(ValueError, match="int64"):
        N.mutualmax_merge(rs.float(), cs, tile)
    assert (rs == 0).all() and (cs == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# driver: tiled cosine + mutual max against the float64 cosine
# ---------------------------------------------------------------------------------------------------------------------
def unit64(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)


def planted_pairs(Ca: int, Cb: int, D: int, seed: int):
    """``a`` random; the first min(Ca, Cb) rows of ``a`` each get a near-copy (noise 0.05 per coordinate: cosine about 0.9988) at
    a random row of ``b``.  Every other row of either side gets a graded copy of a row of the other side with noise ORTHOGONAL
    to it (cosine 1 / sqrt(1 + 0.6^2) = 0.857 to that row — far above the random level 1 / sqrt(D), far below the near-copies'),
    so that every row and every column has a clear best match.  Returns a, b and the float64 argmax / max in both directions
    after asserting the gap precondition."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((Ca, D))
    b = rng.standard_normal((Cb, D))
    n = min(Ca, Cb)
    spots = rng.choice(Cb, size=n, replace=False)
    b[spots] = a[:n] + 0.05 * rng.standard_normal((n, D))

    def graded_copy(src):
        noise = rng.standard_normal(D)
        noise -= (noise @ src) / (src @ src) * src
        return (src + 0.6 * np.linalg.norm(src) * noise / np.linalg.norm(noise)) * rng.uniform(0.5, 2.0)

    for j in np.setdiff1d(np.arange(Cb), spots):
        b[j] = graded_copy(a[rng.integers(0, Ca)])
    for i in range(n, Ca):
        a[i] = graded_copy(b[rng.integers(0, Cb)])
    a, b = a.astype(np.float32), b.astype(np.float32)
    cos = unit64(a) @ unit64(b).T
    want = []
    for c in (cos, cos.T):
        top2 = np.sort(np.partition(c, -2, axis=1)[:, -2:], axis=1)
        gap = top2[:, 1] - top2[:, 0]
        assert gap.min() > 4 * TOL, f"construction: smallest float64 gap {gap.min():.3e} is not above 4 * TOL"
        want.append((c.argmax(axis=1), c.max(axis=1)))
    return a, b, want


PLANTED = {}


def planted_case(Ca, Cb, D):
    if (Ca, Cb, D) not in PLANTED:  # the float64 reference once per shape, shared by the cases that use it and left unchanged
        PLANTED[(Ca, Cb, D)] = planted_pairs(Ca, Cb, D, seed=Ca + D)
    return PLANTED[(Ca, Cb, D)]


# chunk_rows forces several row tiles everywhere; the chunk_cols case also cuts the columns (4097 = 3 x 1500 - 403)
@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("Ca,Cb,D,chunk_rows,chunk_cols", [(512, 4097, 512, 100, None), (512, 4097, 512, 129, 1500),
                                                           (3000, 1000, 1152, 701, None)])
def test_driver_ids_exact_under_gap_construction(mode, Ca, Cb, D, chunk_rows, chunk_cols):
    a, b, ((want_ai, want_av), (want_bi, want_bv)) = planted_case(Ca, Cb, D)
    N.set_gemm_mode(mode)
    try:
        (av, ai), (bv, bi) = N.mutual_probe(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), chunk_rows, chunk_cols)
    finally:
        N.set_gemm_mode(None)
    assert tuple(av.shape) == (Ca,) and tuple(bi.shape) == (Cb,) and ai.dtype == torch.int64 and bv.dtype == torch.float32
    assert np.array_equal(ai.cpu().numpy(), want_ai)
    assert np.array_equal(bi.cpu().numpy(), want_bi)
    err_a, err_b = np.abs(av.cpu().numpy() - want_av).max(), np.abs(bv.cpu().numpy() - want_bv).max()
    print(f"max |value - float64 cosine|: a -> b {err_a:.3e}, b -> a {err_b:.3e}")
    assert err_a <= TOL and err_b <= TOL


def check_best(rows: np.ndarray, cols: np.ndarray, vals: np.ndarray, ids: np.ndarray, block: int = 512):
    """Every returned value within TOL of the float64 cosine of its own (row, id); ids in range; no unreturned candidate above the
    returned one's float64 cosine by more than 2 * TOL.  No row is exempted."""
    assert ids.min() >= 0 and ids.max() < cols.shape[0]
    rh, ch = unit64(rows), unit64(cols)
    worst_val = worst_miss = 0.0
    for s in range(0, rows.shape[0], block):
        cos = rh[s : s + block] @ ch.T
        own = np.take_along_axis(cos, ids[s : s + block, None], axis=1)[:, 0]
        worst_val = max(worst_val, float(np.abs(own - vals[s : s + block]).max()))
        worst_miss = max(worst_miss, float((cos.max(axis=1) - own).max()))
    print(f"max |value - float64 cosine| = {worst_val:.3e}; max (best candidate - returned) = {worst_miss:.3e}")
    assert worst_val <= TOL
    assert worst_miss <= 2 * TOL


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_driver_values_on_random_data(mode):
    rng = np.random.default_rng(21)
    a = rng.standard_normal((1500, 768)).astype(np.float32)
    b = rng.standard_normal((2301, 768)).astype(np.float32)
    N.set_gemm_mode(mode)
    try:
        (av, ai), (bv, bi) = N.mutual_probe(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), chunk_rows=400)
    finally:
        N.set_gemm_mode(None)
    check_best(a, b, av.cpu().numpy(), ai.cpu().numpy())
    check_best(b, a, bv.cpu().numpy(), bi.cpu().numpy())


def test_driver_empty_operand():
    x = torch.randn(5, 16, device=DEV)
    (xv, xi), (yv, yi) = N.mutual_probe(x, torch.zeros(0, 16, device=DEV))
    assert torch.isneginf(xv).all() and (xi == -1).all() and tuple(xv.shape) == (5,)
    assert tuple(yv.shape) == (0,) and tuple(yi.shape) == (0,)


# ---------------------------------------------------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------------------------------------------------
def api_dbs(seed: int = 4, D: int = 256):
    """A = {a0: 300, a1: 500, a2: 200}, B = {b0: 400, b1: 500}; b1 is a shuffled noisy copy of a1 (cosine about 0.9988 to its
    original), everything else is random (cosines around 1 / sqrt(D) = 0.06)."""
    rng = np.random.default_rng(seed)
    A = {f"a{i}": rng.standard_normal((n, D)).astype(np.float32) for i, n in enumerate((300, 500, 200))}
    perm = rng.permutation(500)
    B = {"b0": rng.standard_normal((400, D)).astype(np.float32),
         "b1": (A["a1"][perm] + 0.05 * rng.standard_normal((500, D))).astype(np.float32)}
    return A, B, perm


def test_api_dict_dbs_against_float64():
    A, B, perm = api_dbs()
    lens = L.Lens(_NoModel(), device=DEV)
    cmp = lens.compare_concept_dbs({k: torch.from_numpy(v).to(DEV) for k, v in A.items()},
                                   {k: torch.from_numpy(v).to(DEV) for k, v in B.items()}, chunk_rows=128)
    assert isinstance(cmp, L.ConceptDBComparison)
    assert cmp.layers_a == ["a0", "a1", "a2"] and cmp.layers_b == ["b0", "b1"]
    cos = {(i, j): unit64(a) @ unit64(b).T for i, a in enumerate(A.values()) for j, b in enumerate(B.values())}
    want_ab = np.array([[cos[(i, j)].max(axis=1).mean() for j in range(2)] for i in range(3)])
    want_ba = np.array([[cos[(i, j)].max(axis=0).mean() for i in range(3)] for j in range(2)])
    ab, ba = cmp.layer_similarity_ab, cmp.layer_similarity_ba
    assert tuple(ab.shape) == (3, 2) and tuple(ba.shape) == (2, 3) and ab.dtype == torch.float32 and ab.is_cuda
    assert np.abs(ab.cpu().numpy() - want_ab).max() <= TOL
    assert np.abs(ba.cpu().numpy() - want_ba).max() <= TOL
    all_cos = np.block([[cos[(i, j)] for j in range(2)] for i in range(3)])
    assert abs(cmp.set_similarity_ab - all_cos.max(axis=1).mean()) <= TOL
    assert abs(cmp.set_similarity_ba - all_cos.max(axis=0).mean()) <= TOL
    assert isinstance(cmp.set_similarity_ab, float)
    # the planted layer: a1[perm[j]] <-> b1[j], decoded exactly in both directions, and mutual
    inv = np.argsort(perm)
    v, layer, comp = (t.cpu().numpy() for t in cmp.best_in_b["a1"])
    assert (layer == 1).all() and np.array_equal(comp, inv)
    assert np.abs(v - cos[(1, 1)][np.arange(500), inv]).max() <= TOL
    v, layer, comp = (t.cpu().numpy() for t in cmp.best_in_a["b1"])
    assert (layer == 1).all() and np.array_equal(comp, perm)
    mutual = cmp.mutual()
    assert list(mutual) == ["a0", "a1", "a2"] and mutual["a1"].dtype == torch.bool
    assert mutual["a1"].all() and tuple(mutual["a0"].shape) == (300,)
    # the unplanted layers decode within range, against the float64 best of the whole other DB
    starts_b = np.array([0, 400])
    for i, name in enumerate(A):
        v, layer, comp = (t.cpu().numpy() for t in cmp.best_in_b[name])
        assert ((layer >= 0) & (layer < 2)).all() and (comp < np.array([400, 500])[layer]).all()
        row_cos = np.concatenate([cos[(i, 0)], cos[(i, 1)]], axis=1)
        own = row_cos[np.arange(len(v)), starts_b[layer] + comp]
        assert np.abs(own - v).max() <= TOL and (row_cos.max(axis=1) - own).max() <= 2 * TOL


class _NoModel:
    """compare_concept_dbs needs no foundation model; Lens only stores one."""

    device = DEV
    name = "none"

    def to(self, device):
        return self


def test_pair_equals_probe_topk_k1():
    A, B, perm = api_dbs()
    a, b = torch.from_numpy(A["a1"]).to(DEV), torch.from_numpy(B["b1"]).to(DEV)
    cos = unit64(A["a1"]) @ unit64(B["b1"]).T
    for c in (cos, cos.T):  # the gap precondition for exact ids, in both directions
        top2 = np.sort(np.partition(c, -2, axis=1)[:, -2:], axis=1)
        assert (top2[:, 1] - top2[:, 0]).min() > 4 * TOL
    vals_a, ids_a, vals_b, ids_b = L.compare_concept_dbs(a, b).pair(None, None)
    pv, player, pcomp, names = L.probe_topk(a, b, 1, per="query")
    assert names == [None] and (player == 0).all()
    assert torch.equal(ids_a, pcomp[:, 0])
    assert (vals_a - pv[:, 0]).abs().max().item() <= TOL
    rv, rlayer, rcomp, _ = L.probe_topk(b, a, 1, per="query")
    assert torch.equal(ids_b, rcomp[:, 0])
    assert (vals_b - rv[:, 0]).abs().max().item() <= TOL


def test_tensor_db_against_dict_db():
    A, B, perm = api_dbs()
    a = torch.from_numpy(A["a1"]).to(DEV)
    cmp = L.compare_concept_dbs(a, {k: torch.from_numpy(v).to(DEV) for k, v in B.items()})
    assert cmp.layers_a == [None] and cmp.layers_b == ["b0", "b1"]
    assert tuple(cmp.layer_similarity_ab.shape) == (1, 2) and tuple(cmp.layer_similarity_ba.shape) == (2, 1)
    v, layer, comp = cmp.best_in_b[None]
    assert (layer == 1).all() and np.array_equal(comp.cpu().numpy(), np.argsort(perm))
    assert cmp.mutual()[None].all()
    rev = L.compare_concept_dbs({k: torch.from_numpy(v) for k, v in B.items()}, a)  # a CPU DB A: results come back to the CPU
    assert rev.layers_b == [None] and not rev.layer_similarity_ab.is_cuda
    assert np.array_equal(rev.best_in_a[None][2].numpy(), np.argsort(perm))
    assert torch.allclose(rev.layer_similarity_ab, cmp.layer_similarity_ba.cpu(), atol=TOL, rtol=0)


# ---------------------------------------------------------------------------------------------------------------------
# memory
# ---------------------------------------------------------------------------------------------------------------------
def test_memory_at_full_size():
    """C_a = C_b = 32 768 at D = 256 (the full matrix would be 4 GiB): the rise of the allocator's peak over the call stays below
    tile (128 MiB) + states + 64 MiB; the embeddings are resident before the call."""
    C, D = 32768, 256
    g = torch.Generator(device="cpu").manual_seed(2)
    a = torch.randn(C, D, generator=g).to(DEV)
    b = torch.randn(C, D, generator=g).to(DEV)
    b[:64] = a[100:164] * 2.0  # a few exact counterparts, checked below
    states = 2 * C * (8 + 4 + 8)  # packed entries and their decoded (value, id) forms, both directions
    bound = (128 << 20) + states + (64 << 20)
    L.compare_concept_dbs(a[:256], b[:128])  # code objects loaded before the measured call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    cmp = L.compare_concept_dbs(a, b)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB, full matrix {C * C * 4 / 2**20:.0f} MiB")
    assert rise < bound
    vals_a, ids_a, vals_b, ids_b = cmp.pair()
    assert torch.equal(ids_b[:64].cpu(), torch.arange(100, 164)) and torch.equal(ids_a[100:164].cpu(), torch.arange(64))
    assert (vals_b[:64] - 1).abs().max().item() <= TOL
    assert cmp.mutual()[None][100:164].all()
