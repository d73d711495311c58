"""K24 on the device: the threshold-union kernel against a numpy union-find (labels and degrees exact), the forest under
contention, the tiled cosine + union driver against the float64 cosine under a gap construction, the API and the memory bound.

``TOL`` is the project's bound for cosine values (1e-4).  Where groups are compared exactly the inputs are constructed so that
no float64 cosine lies within 4 * TOL of the threshold, and that is asserted first."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import semanticlens_amd
from semanticlens_amd import _native as N
from semanticlens_amd import lens as L
from semanticlens_amd import scores as S

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def ref_groups(n: int, a: np.ndarray, b: np.ndarray):
    """numpy union-find over the edge list (a[k], b[k]) on n ids: (labels = the smallest id of every group, degrees)."""
    labels = np.arange(n, dtype=np.int64)
    while len(a):
        low = np.minimum(labels[a], labels[b])
        nxt = labels.copy()
        np.minimum.at(nxt, a, low)
        np.minimum.at(nxt, b, low)
        nxt = nxt[nxt]  # every label points at an id of its group that is not above it: follow it
        if np.array_equal(nxt, labels):
            break
        labels = nxt
    degree = np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
    return labels, degree.astype(np.int32)


def tile_edges(vals: np.ndarray, threshold: float, row_base: int, col_base: int):
    """The edges of a tile: row id < column id and value >= threshold (false for a NaN)."""
    with np.errstate(invalid="ignore"):
        r, c = np.nonzero(vals >= np.float32(threshold))
    rid, cid = r + row_base, c + col_base
    keep = rid < cid
    return rid[keep], cid[keep]


def special_matrix(R: int, n: int, seed: int) -> np.ndarray:
    """Heavy exact ties, +-0.0, +-inf, NaN, mixed with a few distinct values (the recipe of test_gpu_compare.special_matrix)."""
    rng = np.random.default_rng(seed)
    pool = np.array([-np.inf, -1.0, -0.0, 0.0, 0.5, 0.5, 1.0, np.inf, np.nan, 0.25, -0.25, 1e-30, -1e-30], dtype=np.float32)
    v = pool[rng.integers(0, len(pool), size=(R, n))]
    mix = rng.random((R, n)) < 0.3
    v[mix] = rng.standard_normal(int(mix.sum())).astype(np.float32).round(1)  # one decimal: still many ties
    return v


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel, exact, no GEMM
# ---------------------------------------------------------------------------------------------------------------------
def run_tiles(vals: np.ndarray, n: int, threshold: float, n_tiles: int, row_base: int, col_base: int, seed: int, unaligned: bool):
    """Fold ``vals`` into a fresh forest as ``n_tiles`` tiles, cut along rows and along columns, in shuffled order, with a
    flatten after every tile; returns (labels, degree, status)."""
    R, B = vals.shape
    if n_tiles == 64 and min(R, B) > 1:
        grid_r, grid_c = 8, 8  # (3, 5) leaves some of the 64 empty: they are skipped
    else:  # one cut direction: along the longer side
        grid_r, grid_c = (n_tiles, 1) if R >= B else (1, n_tiles)
    rcuts = np.linspace(0, R, grid_r + 1).astype(np.int64)
    ccuts = np.linspace(0, B, grid_c + 1).astype(np.int64)
    parent, degree, status = N.unionfind_new(n, DEV)
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
        N.threshold_union_merge(parent, degree, status, tile, threshold, row_base + ra, col_base + ca)
        N.unionfind_flatten(parent, status)
    torch.cuda.synchronize()
    return parent.cpu().numpy(), degree.cpu().numpy(), int(status.item())


def id_bases(R: int, B: int):
    """(name, row_id_base, col_id_base): a diagonal tile, one wholly above the diagonal, one wholly below it, a straddling one."""
    straddle = (B // 3, 0) if B >= R else (0, R // 3)
    return [("diagonal", 5, 5), ("above", 0, R + 2), ("below", B + 1, 0), ("straddling", *straddle)]


@pytest.mark.parametrize("R,B", [(1, 1), (3, 5), (65, 257), (300, 4099), (4099, 300), (1, 70001)])
def test_kernel_exact_against_numpy_union_find(R, B):
    threshold = 0.5  # the pool's ties sit exactly on it
    vals = special_matrix(R, B, seed=R * 1000 + B)
    for name, row_base, col_base in id_bases(R, B):
        n = max(row_base + R, col_base + B) + 3
        rid, cid = tile_edges(vals, threshold, row_base, col_base)
        want_labels, want_degree = ref_groups(n, rid, cid)
        if name == "below":
            assert len(rid) == 0 and np.array_equal(want_labels, np.arange(n))  # nothing may change
        for n_tiles in (1, 7, 64):
            labels, degree, status = run_tiles(vals, n, threshold, n_tiles, row_base, col_base, seed=n_tiles, unaligned=(n_tiles == 7))
            what = f"{name}, {n_tiles} tiles, {len(rid)} edges"
            assert status == 0, what
            assert np.array_equal(degree, want_degree), f"{what}: degrees differ in {int((degree != want_degree).sum())} entries"
            assert np.array_equal(labels, want_labels), f"{what}: labels differ in {int((labels != want_labels).sum())} entries"


# ---------------------------------------------------------------------------------------------------------------------
# 2. contention
# ---------------------------------------------------------------------------------------------------------------------
def test_all_ones_is_one_group_and_all_nan_is_none():
    n = 1031
    for fill, want_label, want_degree in ((1.0, np.zeros(n, dtype=np.int64), n - 1), (float("nan"), np.arange(n), 0)):
        parent, degree, status = N.unionfind_new(n, DEV)
        tile = torch.full((n, n), fill, dtype=torch.float32, device=DEV)
        N.threshold_union_merge(parent, degree, status, tile, 0.5, 0, 0)
        N.unionfind_flatten(parent, status)
        assert int(status.item()) == 0
        assert np.array_equal(parent.cpu().numpy(), want_label)
        assert (degree == want_degree).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. driver under a gap construction
# ---------------------------------------------------------------------------------------------------------------------
RHO = 0.95
THRESHOLD = 0.88  # edges at distance 1 (0.95) and 2 (0.9025) only: distance 3 is 0.857
CHAINS = [2, 3, 4, 7, 33, 2, 2, 5, 20] + [2] * 50


def unit64(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)


def planted_chains(C: int, D: int, seed: int):
    """Gaussian rows with chains x_{t+1} = rho x_t + sqrt(1 - rho^2) u_t planted at shuffled positions under random positive
    scales, u_t orthonormal to everything before it in the chain: cos(x_s, x_t) = rho^|t - s|.  Returns x (float32), the chains'
    positions, and the float64 reference (labels, degree) after asserting the gap precondition."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((C, D))
    spots = rng.permutation(C)[: sum(CHAINS)]
    chains, at = [], 0
    for length in CHAINS:
        q, _ = np.linalg.qr(rng.standard_normal((D, length)))
        rows = [q[:, 0]]
        for t in range(1, length):
            rows.append(RHO * rows[-1] + np.sqrt(1 - RHO * RHO) * q[:, t])
        pos = spots[at : at + length]
        x[pos] = np.stack(rows) * rng.uniform(0.5, 2.0, size=(length, 1))
        chains.append(pos)
        at += length
    x = x.astype(np.float32)
    xh = unit64(x)
    cos = xh @ xh.T
    np.fill_diagonal(cos, -2.0)
    nearest = np.abs(cos - THRESHOLD).min()
    assert nearest > 4 * TOL, f"construction: a float64 cosine lies {nearest:.3e} from the threshold, not above 4 * TOL"
    a, b = np.nonzero(np.triu(cos >= THRESHOLD, 1))
    assert len(a) == 179
    labels, degree = ref_groups(C, a, b)
    return x, chains, labels, degree


PLANTED = {}


def planted_case(C, D):
    if (C, D) not in PLANTED:  # the float64 reference once per shape, shared by the cases that use it and left unchanged
        PLANTED[(C, D)] = planted_chains(C, D, seed=C + D)
    return PLANTED[(C, D)]


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("C,D", [(4097, 512), (3000, 1152), (1031, 64)])
def test_driver_groups_exact_under_gap_construction(mode, C, D):
    x, chains, want_labels, want_degree = planted_case(C, D)
    xd = torch.from_numpy(x).to(DEV)
    N.set_gemm_mode(mode)
    try:
        for chunk_rows, chunk_cols in ((100, None), (129, 1500), (701, None), (None, None)):
            labels, degree, coh = N.redundancy_probe(xd, THRESHOLD, chunk_rows, chunk_cols, cohesion=True)
            what = f"chunks ({chunk_rows}, {chunk_cols})"
            assert labels.dtype == torch.int64 and degree.dtype == torch.int32 and coh.dtype == torch.float32
            labels, degree, coh = labels.cpu().numpy(), degree.cpu().numpy(), coh.cpu().numpy()
            assert np.array_equal(degree, want_degree), what
            assert np.array_equal(labels, want_labels), what
            for pos in chains:
                assert (labels[pos] == pos.min()).all(), f"{what}: a group's label is not its smallest id"
                want = RHO ** (len(pos) - 1)  # the chain's two ends
                err = np.abs(coh[pos] - want).max()
                assert err <= TOL, f"{what}: cohesion of a {len(pos)}-chain off by {err:.3e} from {want:.5f}"
            single = want_degree == 0
            assert np.isnan(coh[single]).all() and not np.isnan(coh[~single]).any(), what
    finally:
        N.set_gemm_mode(None)
    assert abs(RHO ** 32 - 0.19371) < 1e-5 and len(chains[4]) == 33


# ---------------------------------------------------------------------------------------------------------------------
# 4. a clique of near-copies
# ---------------------------------------------------------------------------------------------------------------------
def clique_db(n_rows: int = 2000, n_clique: int = 300, D: int = 512, seed: int = 3):
    """``n_clique`` copies of one row with noise 0.05 per coordinate (cosine about 0.9975 to each other) at shuffled positions
    among Gaussian rows (cosines around 1 / sqrt(D))."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_rows, D))
    pos = np.sort(rng.permutation(n_rows)[:n_clique])
    x[pos] = rng.standard_normal(D) + 0.05 * rng.standard_normal((n_clique, D))
    return x.astype(np.float32), pos


def test_clique_of_near_copies():
    x, pos = clique_db()
    cos = unit64(x) @ unit64(x).T
    np.fill_diagonal(cos, -2.0)
    assert np.abs(cos - 0.9).min() > 4 * TOL
    g = S.redundancy_groups(torch.from_numpy(x).to(DEV), threshold=0.9, chunk_rows=300)
    assert isinstance(g, S.RedundancyGroups) and g.cohesion is None and g.labels.is_cuda
    inside = np.zeros(len(x), dtype=bool)
    inside[pos] = True
    labels, degree = g.labels.cpu().numpy(), g.degree.cpu().numpy()
    assert (labels[inside] == pos[0]).all() and (degree[inside] == 299).all()
    assert np.array_equal(labels[~inside], np.nonzero(~inside)[0]) and (degree[~inside] == 0).all()
    assert g.n_groups == 1701 and int((g.sizes == 300).sum()) == 300 and int((g.sizes == 1).sum()) == 1700
    assert np.array_equal(g.members(int(pos[17])).cpu().numpy(), pos)
    reps = g.representatives().cpu().numpy()  # every degree in the clique is 299: the tie goes to its smallest id
    assert np.array_equal(reps, np.nonzero(~inside | (np.arange(len(x)) == pos[0]))[0])
    assert tuple(g.prune(torch.from_numpy(x)).shape) == (1701, 512)


# ---------------------------------------------------------------------------------------------------------------------
# 5. API
# ---------------------------------------------------------------------------------------------------------------------
class _NoModel:
    """eval_redundancy_groups needs no foundation model; Lens only stores one."""

    device = DEV
    name = "none"

    def to(self, device):
        return self


def test_api_dict_db_lens_and_package_export():
    x, pos = clique_db(600, 40, 128, seed=8)
    y, _ = clique_db(300, 7, 128, seed=9)
    db = {"l1": torch.from_numpy(x).to(DEV), "l2": torch.from_numpy(y)}  # l2 on the host: its results come back to the host
    out = L.Lens(_NoModel(), device=DEV).eval_redundancy_groups(db, threshold=0.9, cohesion=True)
    assert list(out) == ["l1", "l2"] and all(isinstance(g, S.RedundancyGroups) for g in out.values())
    assert out["l1"].labels.is_cuda and not out["l2"].labels.is_cuda and not out["l2"].cohesion.is_cuda
    assert out["l1"].n_groups == 561 and out["l2"].n_groups == 294
    single = semanticlens_amd.redundancy_groups(db["l1"], threshold=0.9, cohesion=True)
    assert torch.equal(single.labels, out["l1"].labels) and torch.equal(single.degree, out["l1"].degree)
    assert torch.equal(single.cohesion.isnan(), ~single.redundant)
    assert float(single.cohesion[single.redundant].min()) > 0.99


def test_nan_row_and_zero_row_are_singletons():
    x, pos = clique_db(500, 30, 64, seed=11)
    x[pos[3], 5] = np.nan
    x[pos[4], 7] = np.inf
    x[pos[5]] = 0.0
    g = S.redundancy_groups(torch.from_numpy(x).to(DEV), threshold=0.9)
    for p in pos[3:6]:
        assert int(g.labels[p]) == p and int(g.degree[p]) == 0
    rest = np.delete(pos, [3, 4, 5])
    assert (g.labels[rest] == int(rest[0])).all() and (g.degree[rest] == 26).all()
    # a negative threshold: a zero row has cosine 0 to every finite row, which is an edge; the NaN rows still have none
    g = S.redundancy_groups(torch.from_numpy(x).to(DEV), threshold=-0.5)
    assert int(g.degree[pos[5]]) == 497 and int(g.degree[pos[3]]) == 0 and int(g.degree[pos[4]]) == 0


def test_empty_and_single_component():
    for C in (0, 1):
        g = S.redundancy_groups(torch.randn(C, 16, device=DEV), threshold=0.5, cohesion=True)
        assert tuple(g.labels.shape) == (C,) and g.labels.dtype == torch.int64 and g.degree.dtype == torch.int32
        assert g.n_groups == C and not g.redundant.any() and g.cohesion.isnan().all() and g.labels.is_cuda
        assert g.labels.tolist() == list(range(C))


def test_redundant_share_equals_the_best_off_diagonal_cosines():
    """``redundant.float().mean()`` is the share of components whose best cosine to ANOTHER component reaches the threshold;
    those best cosines come from K20 (what ``mutual_probe(x, x)`` folds) over the matrix with its diagonal masked."""
    x, pos = clique_db(700, 50, 96, seed=13)
    xd = torch.from_numpy(x).to(DEV)
    cos = N.cosine_nt(xd, xd, torch.empty(700, 700, device=DEV))
    cos.fill_diagonal_(float("-inf"))
    row_state = torch.zeros(700, dtype=torch.int64, device=DEV)
    col_state = torch.zeros(700, dtype=torch.int64, device=DEV)
    N.mutualmax_merge(row_state, col_state, cos)
    best, _ = N.mutualmax_finish(row_state)
    assert ((best - 0.9).abs() > 4 * TOL).all()
    g = S.redundancy_groups(xd, threshold=0.9)
    assert float(g.redundant.float().mean()) == float((best >= 0.9).float().mean())
    assert int(g.redundant.sum()) == 50
    assert torch.equal(g.redundant, best >= 0.9)


# ---------------------------------------------------------------------------------------------------------------------
# 6. memory
# ---------------------------------------------------------------------------------------------------------------------
def test_memory_stays_under_a_quarter_of_the_matrix():
    """C = 20 000 at D = 64, chunk_rows = 256: the full matrix would be 1.6 GB; the rise of the allocator's peak over the call
    stays under a quarter of it (the tile is 20 MB).  The embeddings are resident before the call."""
    C, D = 20000, 64
    g = torch.Generator(device="cpu").manual_seed(2)
    x = torch.randn(C, D, generator=g).to(DEV)
    x[5000:5064] = x[100:164] * 2.0  # a few exact copies, checked below
    S.redundancy_groups(x[:256], threshold=0.95, cohesion=True)  # code objects loaded before the measured call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    groups = S.redundancy_groups(x, threshold=0.95, chunk_rows=256, cohesion=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    bound = C * C * 4 // 4
    print(f"peak rise {rise / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB, full matrix {C * C * 4 / 2**20:.0f} MiB")
    assert rise < bound
    assert torch.equal(groups.labels[5000:5064].cpu(), torch.arange(100, 164)) and (groups.degree[100:164] == 1).all()
    assert groups.n_groups == C - 64 and (groups.cohesion[100:164] - 1).abs().max().item() <= TOL
