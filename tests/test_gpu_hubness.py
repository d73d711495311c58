"""K29 on the device: ``sl_topk_merge_biased`` bit for bit against CPU torch's fp32 score followed by a restatement of K17's total
order; ``csls_probe`` in both GEMM modes against the float64 CSLS of the fp32 inputs; the planted hubs the feature is for; and
``label_components_csls`` over the suite's fake text tower.

Bounds of the float64 comparison, with the suite's cosine tolerance ``TOL = 1e-4`` (DESIGN.md §K29 derives them): a density is the
mean of the ``m`` largest cosines, which is 1-Lipschitz in the sup norm, plus one fp32 rounding: ``TOL + 2^-24``.  A score errs by
``2 dc + dr + dq`` plus two fp32 roundings at magnitude below 4: ``4 TOL + 2^-22``; sorted values are 1-Lipschitz too, so the bound
holds position by position as well as id by id.  The recovered cosine: ``TOL`` plus the recovery's ``2^-23 + 2^-25 < 2e-7``.  Ids are
compared wherever the float64 score stands more than ``8 TOL`` (twice a score's error) from both of its neighbours in the
reference's top-(k + 1); at most 20 % of the positions may be left out of that comparison."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from helpers import FakeVLM
from semanticlens_amd import _native as N
from semanticlens_amd import lens as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def ref_scores(c: np.ndarray, rb: np.ndarray, cb: np.ndarray) -> np.ndarray:
    """The score in CPU torch, fp32, two roundings"""
    return ((2 * torch.from_numpy(c) - torch.from_numpy(rb)[:, None]) - torch.from_numpy(cb)[None, :]).numpy()


def ref_topk(scores: np.ndarray, ids: np.ndarray, k: int):
    """K17's total order restated: NaN first, then the larger value, -0.0 == +0.0, equal keys by the smaller id; unused slots
    (-inf, -1)."""
    R, n = scores.shape
    nan = np.isnan(scores)
    key = np.where(nan, 0.0, scores).astype(np.float64) + 0.0
    order = np.lexsort((np.broadcast_to(ids, (R, n)), -key, ~nan), axis=1)[:, :k]
    out_v = np.full((R, k), -np.inf, dtype=np.float32)
    out_i = np.full((R, k), -1, dtype=np.int64)
    out_v[:, : order.shape[1]] = np.take_along_axis(scores, order, 1)
    out_i[:, : order.shape[1]] = ids[order]
    return out_v, out_i


def assert_state_equal(got, want, what=""):
    """ids equal; values equal bit for bit, a NaN for a NaN (the sign and payload of a NaN are not part of the rule: x86 makes
    ``inf - inf`` the negative quiet NaN, the device the positive one)."""
    gv, gi = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in got)
    wv, wi = want
    assert np.array_equal(gi, wi), f"{what}: ids differ in {int((gi != wi).sum())} slots"
    nan = np.isnan(wv)
    assert np.array_equal(np.isnan(gv), nan), f"{what}: NaNs differ"
    assert np.array_equal(gv.view(np.uint32)[~nan], wv.view(np.uint32)[~nan]), f"{what}: value bit patterns differ"


def place(a: np.ndarray, off: int = 0, pad: int = 0) -> torch.Tensor:
    """``a`` on the device as a view that starts ``off`` elements past a 16-byte boundary; a matrix gets a row stride of
    ``columns + pad``.  Everything around it is NaN."""
    if a.ndim == 1:
        buf = torch.full((a.shape[0] + off + 4,), NAN, dtype=torch.float32, device=DEV)
        view = buf[off : off + a.shape[0]]
    else:
        R, B = a.shape
        ld = B + pad
        buf = torch.full((R * ld + off + 4,), NAN, dtype=torch.float32, device=DEV)
        view = buf[off : off + R * ld].view(R, ld)[:, :B]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * (off % 4)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


def special_case(R: int, B: int, seed: int):
    """Tile and biases in multiples of 1/8 (many scores tie exactly), with NaN, +-inf and -0.0 sprinkled over the tile and the
    column biases, row biases of +inf, NaN and -inf in rows 1, 2, 3, and a +inf cosine under the +inf row bias (inf - inf)."""
    rng = np.random.default_rng(seed)
    pool = np.array([np.nan, np.inf, -np.inf, -0.0], dtype=np.float32)
    c = (rng.integers(-8, 9, size=(R, B)) / 8).astype(np.float32)
    rb = (rng.integers(-8, 9, size=R) / 8).astype(np.float32)
    cb = (rng.integers(-8, 9, size=B) / 8).astype(np.float32)
    mask = rng.random((R, B)) < 0.05
    c[mask] = pool[rng.integers(0, 4, size=int(mask.sum()))]
    mask = rng.random(B) < 0.04
    cb[mask] = pool[rng.integers(0, 4, size=int(mask.sum()))]
    if R >= 4:
        rb[1], rb[2], rb[3] = np.inf, np.nan, -np.inf
        c[1, 0] = np.inf
        if not np.isfinite(cb[0]):
            cb[0] = 0.25
    return c, rb, cb


def fold(c, rb, cb, k, pieces=None, id_base=0, tile_off=0, pad=0, cb_off=0, rb_off=0, state=None):
    """Fold column pieces ``[(a, b), ...]`` of the tile into a state (a fresh one by default), each as a tile and a slice of the
    column biases of their own, placed at the given offsets."""
    R, B = c.shape
    sv, si = state if state is not None else N.topk_new(R, k, DEV)
    rbd = place(rb, rb_off)
    for a, b in pieces or [(0, B)]:
        N.topk_merge_biased(sv, si, place(c[:, a:b], tile_off, pad), rbd, place(cb[a:b], cb_off), id_base + a)
    return sv, si


@pytest.mark.parametrize("B", [1, 3, 4, 5, 1023, 1024, 1025, 2051])
def test_kernel_exact_at_every_alignment(B):
    """R = 7 rows at every chunk edge (one wave per row up to B = 2 047; B = 2 051 is two segments per row); the tile 0..3 elements
    past a 16-byte boundary with ld > B, the column biases 0..3 elements past one, independently; k below and above B."""
    R = 7
    c, rb, cb = special_case(R, B, seed=B)
    scores = ref_scores(c, rb, cb)
    assert np.isnan(scores[1, 0]) and not np.isnan(c[1, 0]) and not np.isnan(cb[0])  # inf - inf
    assert np.isnan(scores[2]).all() and (B < 1023 or np.isnan(cb).any() and np.isinf(cb).any() and np.isnan(c).any())
    id_base = (1 << 40) - 3
    ids = id_base + np.arange(B, dtype=np.int64)
    for k in (1, 5, 130, 1024):
        want = ref_topk(scores, ids, k)
        if B < k:
            assert (want[1][:, B:] == -1).all()
        offsets = [(t, q) for t in range(4) for q in range(4)] if k in (5, 130) else [(1, 2), (0, 0)]
        for tile_off, cb_off in offsets:
            got = fold(c, rb, cb, k, id_base=id_base, tile_off=tile_off, pad=3 if tile_off else 0, cb_off=cb_off, rb_off=cb_off ^ 1)
            assert_state_equal(got, want, f"B={B} k={k} tile+{tile_off} bias+{cb_off}")


@pytest.mark.parametrize("R,B", [(3, 4096), (1, 10000)])
def test_kernel_exact_on_split_rows(R, B):
    """Few rows of many columns: S >= 2 segments per row, whose partial selections (scores) go through the workspace and the
    list fold.  Segment starts are not chunk starts: a lane's piece straddles lo and hi."""
    c, rb, cb = special_case(R, B, seed=R + B)
    if R < 4:
        c[0, 5], rb[0] = np.inf, np.inf
    scores = ref_scores(c, rb, cb)
    assert np.isnan(scores[0, 5]) or R >= 4
    ids = 11 + np.arange(B, dtype=np.int64)
    for k in (5, 130, 1024):
        assert N.lib().sl_topk_merge_ws_bytes(R, k, B) > 0
        want = ref_topk(scores, ids, k)
        for tile_off, cb_off in ((0, 0), (1, 3), (2, 0), (3, 1)):
            got = fold(c, rb, cb, k, id_base=11, tile_off=tile_off, pad=5 if tile_off else 0, cb_off=cb_off)
            assert_state_equal(got, want, f"R={R} B={B} k={k} tile+{tile_off} bias+{cb_off}")


@pytest.mark.parametrize("k", [5, 130])
def test_state_does_not_depend_on_the_cut_into_tiles(k):
    R, B = 5, 2051
    c, rb, cb = special_case(R, B, seed=k)
    id_base = (1 << 40) - 5
    want = ref_topk(ref_scores(c, rb, cb), id_base + np.arange(B, dtype=np.int64), k)
    for n_pieces in (1, 3, 7):
        cuts = np.linspace(0, B, n_pieces + 1).astype(np.int64)
        pieces = [(int(cuts[t]), int(cuts[t + 1])) for t in np.random.default_rng(n_pieces).permutation(n_pieces)]
        got = fold(c, rb, cb, k, pieces, id_base=id_base, tile_off=n_pieces % 4, pad=1, cb_off=(n_pieces + 1) % 4)
        assert_state_equal(got, want, f"{n_pieces} pieces")


def test_zero_biases_give_k17s_ids_and_twice_its_values():
    R, B, k = 6, 1500, 20
    c, _, _ = special_case(R, B, seed=1)
    zr, zc = np.zeros(R, dtype=np.float32), np.zeros(B, dtype=np.float32)
    tile = place(c, 1, 2)
    pv, pi = N.topk_new(R, k, DEV)
    N.topk_merge(pv, pi, tile, 7)
    bv, bi = fold(c, zr, zc, k, id_base=7, tile_off=1, pad=2)
    assert (c.view(np.uint32) == 0x80000000).any() and np.isinf(c).any()
    assert_state_equal((bv, bi), ((2 * pv).cpu().numpy(), pi.cpu().numpy()))


def test_a_biased_state_merges_with_merge_states():
    R, B, k = 5, 1800, 40
    c, rb, cb = special_case(R, B, seed=2)
    want = ref_topk(ref_scores(c, rb, cb), np.arange(B, dtype=np.int64), k)
    h = 777
    av, ai = fold(c, rb, cb, k, [(0, h)])
    bv, bi = fold(c, rb, cb, k, [(h, B)], cb_off=1)
    N.topk_merge_states(av, ai, bv, bi)
    assert_state_equal((av, ai), want)
    assert_state_equal(fold(c, rb, cb, k, [(h, B), (0, h)]), want)


def test_kernel_past_its_grid():
    """``topk_tile_kernel<true>`` on K17's grid, ``rowseg::wave_grid``: 4 x CUs x 32 one-wave items at k = 5 (256 LDS entries of 12
    bytes: 32 workgroups per CU).  R = cap + 1 and 2 cap + 1 rows of 8 columns, the row bias a function of the row: every row."""
    cap = 4 * torch.cuda.get_device_properties(0).multi_processor_count * 32
    k, B = 5, 8
    for R in (cap + 1, 2 * cap + 1):
        assert R > cap and N.lib().sl_topk_merge_ws_bytes(R, k, B) == 0
        rng = np.random.default_rng(R)
        c = (rng.integers(-64, 65, size=(R, B)) / 64).astype(np.float32)
        rb = ((np.arange(R) % 97) / 32 - 1.5).astype(np.float32)
        cb = (rng.permutation(B) / 16).astype(np.float32)
        want = ref_topk(ref_scores(c, rb, cb), 3 + np.arange(B, dtype=np.int64), k)
        sv = torch.full((R, k), NAN, device=DEV)
        si = torch.full((R, k), 7, dtype=torch.int64, device=DEV)
        N.topk_init(sv, si)
        assert_state_equal(fold(c, rb, cb, k, id_base=3, state=(sv, si)), want, f"R={R}")
        del sv, si


def test_refusals_launch_nothing():
    R, B, k = 3, 4096, 5
    c, rb, cb = special_case(R, B, seed=3)
    tile, rbd, cbd = place(c), place(rb), place(cb)
    sv, si = N.topk_new(R, k, DEV)
    lib, p = N.lib(), N._ptr
    nbytes = int(lib.sl_topk_merge_ws_bytes(R, k, B))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    args = lambda rbp, cbp, wsp, wsn: (p(sv), p(si), R, k, p(tile), B, B, 0, rbp, cbp, wsp, wsn, N._stream(sv))
    assert lib.sl_topk_merge_biased(*args(None, p(cbd), p(ws), nbytes)) == -1 and b"null bias" in lib.sl_last_error()
    assert lib.sl_topk_merge_biased(*args(p(rbd), None, p(ws), nbytes)) == -1 and b"null bias" in lib.sl_last_error()
    assert lib.sl_topk_merge_biased(*args(p(rbd), p(cbd), p(ws), nbytes - 1)) == -1 and b"workspace too small" in lib.sl_last_error()
    assert lib.sl_topk_merge_biased(*args(p(rbd), p(cbd), None, nbytes)) == -1 and b"workspace too small" in lib.sl_last_error()
    for bad_rb, bad_cb in ((rbd[:2], cbd), (rbd, cbd[:-1]), (rbd.double(), cbd), (rbd, cbd.cpu()), (rbd, cbd.view(2, -1)),
                           (rbd, place(np.repeat(cb, 2))[::2])):
        with pytest.raises(ValueError):
            N.topk_merge_biased(sv, si, tile, bad_rb, bad_cb)
    with pytest.raises(ValueError):
        N.topk_merge_biased(sv, si, tile[:2], rbd[:2], cbd)  # a tile that does not fit the state
    torch.cuda.synchronize()
    assert bool((si == -1).all()) and bool((sv == -INF).all()), "a refused call wrote to the state"
    N.topk_merge_biased(sv, si, tile, rbd, cbd, 0, ws)
    assert_state_equal((sv, si), ref_topk(ref_scores(c, rb, cb), np.arange(B, dtype=np.int64), k))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the probe against float64
# ---------------------------------------------------------------------------------------------------------------------
PROBE_CASES = [(48, 132, 32, 10, 5), (130, 1030, 36, 10, 5), (7, 5000, 20, 16, 8), (300, 9, 12, 10, 3)]
DENSITY_BOUND = TOL + 2.0 ** -24
SCORE_BOUND = 4 * TOL + 2.0 ** -22
COSINE_BOUND = TOL + 2e-7


def unit64(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.float64)
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def csls64(x: np.ndarray, w: np.ndarray, m: int):
    """float64 cosines of the fp32 inputs, the mean of the m largest per side (of those present), the score"""
    cos = unit64(x) @ unit64(w).T
    r = -np.sort(-cos, axis=1)[:, :m].mean(1)
    q = -np.sort(-cos, axis=0)[:m].mean(0)
    return cos, r, q, 2 * cos - r[:, None] - q[None, :]


@functools.lru_cache(maxsize=None)
def probe_case(case):
    C, V, D, m, k = case
    rng = np.random.default_rng(C + V)
    mu = rng.standard_normal(D)
    x = (rng.standard_normal((C, D)) + 0.7 * mu).astype(np.float32)
    w = (rng.standard_normal((V, D)) + 0.3 * mu).astype(np.float32)
    cos, r, q, s = csls64(x, w, m)
    order = np.argsort(-s, axis=1, kind="stable")[:, : k + 1]
    top = np.take_along_axis(s, order, 1)  # (C, k + 1), best first
    gap = np.abs(np.diff(top, axis=1))  # gap[:, p] between positions p and p + 1
    before = np.concatenate([np.full((C, 1), np.inf), gap[:, : k - 1]], 1)
    decidable = (before > 8 * TOL) & (gap[:, :k] > 8 * TOL)
    for a in (x, w, cos, r, q, s, order, top, decidable):
        a.setflags(write=False)
    return x, w, cos, r, q, s, order[:, :k], top[:, :k], decidable


def check_probe(case, mode, chunk_rows):
    C, V, D, m, k = case
    x, w, cos, r, q, s, order, top, decidable = probe_case(case)
    left_out = 1.0 - decidable.mean()
    N.set_gemm_mode(mode)
    try:
        gv, gi, gr, gq = N.csls_probe(torch.tensor(x, device=DEV), torch.tensor(w, device=DEV), k, m, chunk_rows)
    finally:
        N.set_gemm_mode(None)
    assert gv.dtype == torch.float32 and gi.dtype == torch.int64 and gr.dtype == torch.float32 and gq.dtype == torch.float32
    assert tuple(gv.shape) == (C, k) and tuple(gi.shape) == (C, k) and tuple(gr.shape) == (C,) and tuple(gq.shape) == (V,) and gv.is_cuda
    hl = L.HubnessLabels(gv, gi, gr, gq, m)
    vals, ids, rr, qq, cosine = (t.cpu().numpy() for t in (gv, gi, gr, gq, hl.cosine))
    assert ids.min() >= 0 and ids.max() < V
    assert (np.sort(ids, 1)[:, 1:] != np.sort(ids, 1)[:, :-1]).all(), "an id is returned twice in a row"
    rows = np.arange(C)[:, None]
    e_r, e_q = np.abs(rr - r).max(), np.abs(qq - q).max()
    e_pos = np.abs(vals - top).max()
    e_own = np.abs(vals - s[rows, ids]).max()
    e_cos = np.abs(cosine - cos[rows, ids]).max()
    print(f"{case} {mode} chunk_rows={chunk_rows}: |r - f64| {e_r:.2e}, |q - f64| {e_q:.2e} (bound {DENSITY_BOUND:.2e}); score by "
          f"position {e_pos:.2e}, by id {e_own:.2e} (bound {SCORE_BOUND:.2e}); cosine {e_cos:.2e} (bound {COSINE_BOUND:.2e}); "
          f"{left_out:.1%} of the positions left out of the id comparison")
    assert e_r <= DENSITY_BOUND and e_q <= DENSITY_BOUND
    assert e_pos <= SCORE_BOUND and e_own <= SCORE_BOUND
    assert e_cos <= COSINE_BOUND
    assert left_out <= 0.20
    assert np.array_equal(ids[decidable], order[decidable])
    return gv, gi, gr, gq


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("case", PROBE_CASES)
def test_csls_probe_against_float64(case, mode):
    check_probe(case, mode, None)


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_csls_probe_over_several_tiles(mode):
    """chunk_rows = 257: five tiles per pass, the column biases' slices start 1, 2, 3 and 0 elements past a 16-byte boundary"""
    check_probe(PROBE_CASES[1], mode, 257)


def test_csls_probe_of_an_empty_side():
    x, w = torch.randn(6, 8, device=DEV), torch.randn(9, 8, device=DEV)
    vals, ids, r, q = N.csls_probe(x[:0], w, 3, 4)
    assert tuple(vals.shape) == (0, 3) and tuple(ids.shape) == (0, 3) and tuple(r.shape) == (0,) and bool(q.isnan().all()) and q.shape[0] == 9
    vals, ids, r, q = N.csls_probe(x, w[:0], 3, 4)
    assert bool((vals == -INF).all()) and bool((ids == -1).all()) and tuple(vals.shape) == (6, 3)
    assert bool(r.isnan().all()) and r.shape[0] == 6 and tuple(q.shape) == (0,)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the planted hubs: what the feature is for
# ---------------------------------------------------------------------------------------------------------------------
def normalize(a: np.ndarray) -> np.ndarray:
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


@pytest.mark.parametrize("seed", [0, 1])
def test_planted_words_beat_the_hubs(seed):
    C, D, m = 48, 32, 10
    rng = np.random.default_rng(seed)
    mu = normalize(rng.standard_normal(D))
    e = normalize(rng.standard_normal((C, D)))
    comps = normalize(mu + e).astype(np.float32)
    hubs = normalize(mu + 0.5 * rng.standard_normal((4, D)) / np.sqrt(D))
    planted = normalize(e + 0.45 * rng.standard_normal((C, D)) / np.sqrt(D))
    distractors = normalize(rng.standard_normal((80, D)))
    vocab = np.concatenate([hubs, planted, distractors]).astype(np.float32)
    cos, r, q, s = csls64(comps, vocab, m)
    plain_top = cos.argmax(1)
    hub_rows = plain_top < 4
    top2 = -np.sort(-s, axis=1)[:, :2]
    margin = (top2[:, 0] - top2[:, 1]).min()
    print(f"seed {seed}: plain top-1 is a hub for {hub_rows.mean():.0%} of the components; CSLS top-1 margin {margin:.3f}")
    assert hub_rows.mean() >= 0.5
    assert np.array_equal(s.argmax(1), 4 + np.arange(C))
    assert margin >= 0.02
    # a precondition of the comparison below, not of the feature: where a hub leads, it leads every other word by more than the
    # two cosines' errors, so the device's plain top-1 is a hub there too
    assert (cos[:, :4].max(1) - cos[:, 4:].max(1))[hub_rows].min() > 2 * TOL

    xd, wd = torch.from_numpy(comps).to(DEV), torch.from_numpy(vocab).to(DEV)
    _, plain_ids = L.probe_topk(wd, xd, k=1)
    assert bool((plain_ids[:, 0].cpu()[torch.from_numpy(hub_rows)] < 4).all())
    hl = L.probe_csls(wd, xd, k=1, neighbours=m)
    assert isinstance(hl, L.HubnessLabels) and hl.neighbours == m
    assert torch.equal(hl.ids[:, 0].cpu(), 4 + torch.arange(C))
    assert set(hl.hubs(4)[1].tolist()) == {0, 1, 2, 3}


# ---------------------------------------------------------------------------------------------------------------------
# 4. label_components_csls over the suite's fake text tower
# ---------------------------------------------------------------------------------------------------------------------
LETTERS = "abcdefghijklmnopqrstuvwxyz"
TEMPLATES = ["a photo of {}", "{} texture", "an image showing {}."]
FIELDS = ("values", "ids", "component_density", "label_density")


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same(a: L.HubnessLabels, b: L.HubnessLabels) -> bool:
    return a.neighbours == b.neighbours and all(torch.equal(bits(getattr(a, f)), bits(getattr(b, f))) for f in FIELDS)


@pytest.mark.parametrize("templates", [None, TEMPLATES])
def test_label_components_csls_equals_probe_csls_bit_for_bit(templates):
    rng = np.random.default_rng(11)
    words = []
    while len(words) < 40:
        word = "".join(LETTERS[i] for i in rng.integers(0, 26, size=int(rng.integers(3, 9))))
        if word not in words:
            words.append(word)
    V = len(words)
    fm = FakeVLM(dim=16, ctx=24).to(DEV)
    emb = L._embed_words(fm, words, templates, None)
    g = torch.Generator().manual_seed(3)
    db = {"a": emb[:30] + 0.3 * torch.randn(30, 16, generator=g).to(DEV) * emb.abs().mean(),
          "b": torch.randn(12, 16, generator=g)}  # layer b lives on the host
    want = L.probe_csls(emb, db, k=5, neighbours=4)
    assert set(want) == {"a", "b"} and want["a"].ids.is_cuda and not want["b"].ids.is_cuda and not want["b"].label_density.is_cuda
    assert tuple(want["a"].label_density.shape) == (V,) and tuple(want["b"].label_density.shape) == (V,)
    assert not torch.equal(want["a"].label_density.cpu(), want["b"].label_density)  # q is taken over each layer's own components
    assert tuple(want["a"].values.shape) == (30, 5) and tuple(want["b"].component_density.shape) == (12,)
    for chunk_size in (7, V):
        got = L.label_components_csls(fm, words, db, k=5, neighbours=4, templates=templates, chunk_size=chunk_size)
        assert list(got) == ["a", "b"]
        for name in db:
            assert same(got[name], want[name]), f"layer {name}, chunk_size={chunk_size}"
            assert got[name].ids.device == db[name].device and got[name].label_density.device == db[name].device
    again = L.label_components_csls(fm, words, db, k=5, neighbours=4, templates=templates, chunk_size=7)
    assert all(same(again[name], want[name]) for name in db)  # the same call twice: the same bits
    one = L.Lens(fm, device=DEV).label_components_csls(words, db["a"], 5, 4, templates, None, 7)
    assert isinstance(one, L.HubnessLabels) and same(one, want["a"])
    cosine = one.cosine
    plain_vals, plain_ids = L.probe_topk(emb, db["a"], k=V)
    lookup = torch.zeros(30, V, device=DEV).scatter_(1, plain_ids, plain_vals)  # the cosine K17 saw for every (component, word)
    assert float((cosine - lookup.gather(1, one.ids)).abs().max()) <= 2e-7  # the recovery alone: the same GEMM gave both
