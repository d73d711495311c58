"""K17 on the device: the streaming fp32 top-k kernel against a numpy lexsort (bit patterns and ids, exact), the tiled
cosine + top-k path against the float64 cosine, and the describe / search API over the suite's fake text tower.

``TOL`` is the project's bound for cosine values (1e-4).  Where ids are compared exactly the inputs are constructed so that the
float64 gaps between consecutive top-(k+1) cosines exceed 4 * TOL, and that precondition is asserted first."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from helpers import FakeVLM
from semanticlens_amd import _native as N
from semanticlens_amd import lens as L

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------------
# kernel, exact
# ---------------------------------------------------------------------------------------------------------------------
def ref_topk(vals: np.ndarray, ids: np.ndarray, k: int):
    """numpy reference: per row a lexsort on (is-NaN descending, value descending, id ascending); empty slots (-inf, -1)."""
    R, n = vals.shape
    out_v = np.full((R, k), -np.inf, dtype=np.float32)
    out_i = np.full((R, k), -1, dtype=np.int64)
    for r in range(R):
        v = vals[r]
        nan = np.isnan(v)
        key = np.where(nan, 0.0, v).astype(np.float64) + 0.0  # -0.0 and +0.0 compare equal
        order = np.lexsort((ids, -key, ~nan))[:k]
        out_v[r, : len(order)] = v[order]
        out_i[r, : len(order)] = ids[order]
    return out_v, out_i


def special_matrix(R: int, n: int, seed: int) -> np.ndarray:
    """Heavy exact ties, +-0.0, +-inf, NaN, mixed with a few distinct values."""
    rng = np.random.default_rng(seed)
    pool = np.array([-np.inf, -1.0, -0.0, 0.0, 0.5, 0.5, 1.0, np.inf, np.nan, 0.25, -0.25, 1e-30, -1e-30], dtype=np.float32)
    v = pool[rng.integers(0, len(pool), size=(R, n))]
    mix = rng.random((R, n)) < 0.3
    v[mix] = rng.standard_normal(int(mix.sum())).astype(np.float32).round(1)  # one decimal: still many ties
    return v


def run_tiles(vals: np.ndarray, k: int, n_tiles: int, id_base: int, seed: int, unaligned: bool):
    """Fold ``vals`` into a fresh state as ``n_tiles`` column tiles in shuffled order."""
    R, n = vals.shape
    sv, si = N.topk_new(R, k, DEV)
    cuts = np.linspace(0, n, n_tiles + 1).astype(np.int64)
    order = np.random.default_rng(seed).permutation(n_tiles)
    for t in order:
        a, b = int(cuts[t]), int(cuts[t + 1])
        if b == a:
            continue
        if unaligned:  # a view that starts 4 bytes past a 16-byte boundary, with a row stride that is not a multiple of 4
            buf = torch.full((R, (b - a) + 3), float("nan"), dtype=torch.float32, device=DEV)
            buf[:, 1 : 1 + (b - a)] = torch.from_numpy(vals[:, a:b]).to(DEV)
            tile = buf[:, 1 : 1 + (b - a)]
        else:
            tile = torch.from_numpy(np.ascontiguousarray(vals[:, a:b])).to(DEV)
        N.topk_merge(sv, si, tile, id_base + a)
    torch.cuda.synchronize()
    return sv.cpu().numpy(), si.cpu().numpy()


def assert_state_equal(got, want):
    gv, gi = got
    wv, wi = want
    assert np.array_equal(gi, wi), f"ids differ in {int((gi != wi).sum())} slots"
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), "value bit patterns differ"


@pytest.mark.parametrize("R,k,n", [(1, 1, 5003), (3, 5, 4099), (3584, 5, 301), (3, 100, 3001), (1, 1024, 5003), (3, 1024, 1501),
                                   (3584, 100, 257), (1, 5, 70001)])
def test_kernel_exact_against_lexsort(R, k, n):
    vals = special_matrix(R, n, seed=R * 1000 + k)
    id_base = (1 << 40) - 5
    ids = id_base + np.arange(n, dtype=np.int64)
    want = ref_topk(vals, ids, k)
    first = None
    for n_tiles in (1, 7, 64):
        got = run_tiles(vals, k, n_tiles, id_base, seed=n_tiles, unaligned=(n_tiles == 7))
        assert_state_equal(got, want)
        if first is None:
            first = got
        assert_state_equal(got, first)  # the cut into tiles and their order do not show


@pytest.mark.parametrize("R,k,n", [(3, 5, 3), (1, 100, 64), (3584, 1024, 9), (3, 1, 1)])
def test_kernel_fewer_than_k_leaves_empty_slots(R, k, n):
    vals = special_matrix(R, n, seed=k)
    vals[:, 0] = -np.inf  # a real -inf beats an empty slot
    ids = np.arange(n, dtype=np.int64)
    want = ref_topk(vals, ids, k)
    if n < k:
        assert (want[1][:, n:] == -1).all() and np.isneginf(want[0][:, n:]).all()
    assert_state_equal(run_tiles(vals, k, 2 if n > 1 else 1, 0, seed=0, unaligned=True), want)


@pytest.mark.parametrize("R,k,n", [(3, 5, 2001), (3584, 100, 150), (1, 1024, 4000)])
def test_merge_states_of_two_halves_equals_one_pass(R, k, n):
    vals = special_matrix(R, n, seed=n)
    ids = np.arange(n, dtype=np.int64)
    want = ref_topk(vals, ids, k)
    h = n // 2
    av, ai = N.topk_new(R, k, DEV)
    bv, bi = N.topk_new(R, k, DEV)
    N.topk_merge(av, ai, torch.from_numpy(np.ascontiguousarray(vals[:, :h])).to(DEV), 0)
    N.topk_merge(bv, bi, torch.from_numpy(np.ascontiguousarray(vals[:, h:])).to(DEV), h)
    N.topk_merge_states(av, ai, bv, bi)
    assert_state_equal((av.cpu().numpy(), ai.cpu().numpy()), want)


# ---------------------------------------------------------------------------------------------------------------------
# end to end: tiled cosine + top-k against the float64 cosine
# ---------------------------------------------------------------------------------------------------------------------
def unit64(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)


def check_values(rows: np.ndarray, cols: np.ndarray, vals, ids, block: int = 512):
    """Every returned value within TOL of the float64 cosine of its own (row, id); ids in range and distinct per row; no
    unreturned candidate above the row's smallest returned float64 cosine by more than 2 * TOL.  No row is exempted.
    ``vals`` / ``ids``: one result, or lists of results over the same inputs (each held to the same bounds; the float64
    cosine is computed once)."""
    results = list(zip(vals, ids)) if isinstance(vals, (list, tuple)) else [(vals, ids)]
    V = cols.shape[0]
    for _, i in results:
        assert i.min() >= 0 and i.max() < V
        assert (np.sort(i, axis=1)[:, 1:] != np.sort(i, axis=1)[:, :-1]).all(), "an id is returned twice in a row"
    rh, ch = unit64(rows), unit64(cols)
    worst_val, worst_miss = [0.0] * len(results), [0.0] * len(results)
    for a in range(0, rows.shape[0], block):
        cos = rh[a : a + block] @ ch.T
        for n, (v, i) in enumerate(results):
            own = np.take_along_axis(cos, i[a : a + block], axis=1)
            worst_val[n] = max(worst_val[n], float(np.abs(own - v[a : a + block]).max()))
            np.put_along_axis(cos, i[a : a + block], -np.inf, axis=1)
            worst_miss[n] = max(worst_miss[n], float((cos.max(axis=1) - own.min(axis=1)).max()))
            np.put_along_axis(cos, i[a : a + block], own, axis=1)
    for n in range(len(results)):
        print(f"max |value - float64 cosine| = {worst_val[n]:.3e}; max (best unreturned - smallest returned) = {worst_miss[n]:.3e}")
        assert worst_val[n] <= TOL
        assert worst_miss[n] <= 2 * TOL


def random_planted(C: int, V: int, D: int, seed: int):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((C, D)).astype(np.float32)
    cols = rng.standard_normal((V, D)).astype(np.float32)
    planted = rng.choice(V, size=min(V, C), replace=False)  # a near-copy of a component somewhere in the vocabulary
    cols[planted] = rows[: len(planted)] + 0.05 * rng.standard_normal((len(planted), D)).astype(np.float32)
    return rows, cols


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("C,V,D,k", [(1000, 20000, 768, 5), (3000, 8192, 1152, 100), (512, 4097, 512, 1)])
def test_values_against_float64(mode, C, V, D, k):
    rows, cols = random_planted(C, V, D, seed=C + D)
    N.set_gemm_mode(mode)
    try:
        vals, ids = L.probe_topk(torch.from_numpy(cols).to(DEV), torch.from_numpy(rows).to(DEV), k, chunk_rows=3001)
    finally:
        N.set_gemm_mode(None)
    check_values(rows, cols, vals.cpu().numpy(), ids.cpu().numpy())


def test_values_and_memory_at_full_size():
    """V = 65 536 against C = 8 192 (the full matrix would be 2 GiB), in both GEMM modes: values as above, and the rise of the
    allocator's peak over each call stays below tile + states + 64 MiB (no chunk of embeddings is allocated inside the call:
    they are passed in).  One test for both modes, so that the float64 cosine is computed once."""
    C, V, D, k = 8192, 65536, 512, 5
    rows, cols = random_planted(C, V, D, seed=11)
    x = torch.from_numpy(rows).to(DEV)
    y = torch.from_numpy(cols).to(DEV)
    chunk = N.topk_chunk_rows(C, V)
    assert C * chunk * 4 <= 128 << 20
    # the embeddings are resident before the call, so the allowance is the tile, the states and the slack alone
    bound = C * chunk * 4 + C * k * 12 + (64 << 20)
    got_vals, got_ids = [], []
    for mode in ("bf16x3", "f32"):
        N.set_gemm_mode(mode)
        try:
            L.probe_topk(y[:256], x[:128], k)  # code objects loaded before the measured call
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            vals, ids = L.probe_topk(y, x, k)
            torch.cuda.synchronize()
            rise = torch.cuda.max_memory_allocated() - before
        finally:
            N.set_gemm_mode(None)
        print(f"{mode}: peak rise {rise / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB, full matrix {C * V * 4 / 2**20:.0f} MiB")
        assert rise < bound
        got_vals.append(vals.cpu().numpy())
        got_ids.append(ids.cpu().numpy())
        del vals, ids
    check_values(rows, cols, got_vals, got_ids)


# ---------------------------------------------------------------------------------------------------------------------
# end to end: ids, exact, under a gap construction
# ---------------------------------------------------------------------------------------------------------------------
def graded(C: int, V: int, D: int, grades: int, seed: int):
    """Vocabulary rows = each component's vector plus graded noise ORTHOGONAL to it: grade j of component c has the cosine
    1 / sqrt(1 + (0.1 (j + 1))^2) to it (0.995, 0.981, 0.958, ... — consecutive gaps above 0.01 up to grade 21), the rest of the
    vocabulary is random (cosines around 1 / sqrt(D)); rows are shuffled."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((C, D))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    cols = rng.standard_normal((V, D))
    assert C * grades <= V
    for c in range(C):
        for j in range(grades):
            n = rng.standard_normal(D)
            n -= (n @ rows[c]) * rows[c]
            n /= np.linalg.norm(n)
            cols[c * grades + j] = (rows[c] + 0.1 * (j + 1) * n) * rng.uniform(0.5, 2.0)
    cols = cols[rng.permutation(V)]
    return rows.astype(np.float32), cols.astype(np.float32)


def float64_topk(rows: np.ndarray, cols: np.ndarray, k: int):
    """ids (R, k) of the float64 argsort, after asserting the gap precondition on the top k + 1."""
    cos = unit64(rows) @ unit64(cols).T
    order = np.argsort(-cos, axis=1, kind="stable")[:, : k + 1]
    top = np.take_along_axis(cos, order, axis=1)
    gaps = top[:, :-1] - top[:, 1:]
    assert gaps.min() > 4 * TOL, f"construction: smallest float64 gap {gaps.min():.3e} is not above 4 * TOL"
    return order[:, :k], top[:, :k]


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("k", [1, 5, 20])
@pytest.mark.parametrize("C,V,D", [(512, 16384, 512), (300, 8000, 1152)])
def test_ids_exact_under_gap_construction(mode, k, C, V, D):
    rows, cols = graded(C, V, D, grades=21, seed=D + C)
    want_ids, want_vals = float64_topk(rows, cols, k)
    N.set_gemm_mode(mode)
    try:
        vals, ids = L.probe_topk(torch.from_numpy(cols).to(DEV), torch.from_numpy(rows).to(DEV), k, chunk_rows=2500)
    finally:
        N.set_gemm_mode(None)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.abs(vals.cpu().numpy() - want_vals).max() <= TOL


def test_search_across_layers_decodes_layer_and_component():
    D, k = 512, 5
    sizes = {"layer2": 300, "layer3": 700, "layer4": 1500}
    total = sum(sizes.values())
    queries, comps = graded(6, total, D, grades=8, seed=3)  # 6 queries, each with 8 graded components somewhere
    want_ids, want_vals = float64_topk(queries, comps, k)
    db, off = {}, 0
    for name, n in sizes.items():
        db[name] = torch.from_numpy(comps[off : off + n]).to(DEV)
        off += n
    vals, layer_index, component, names = L.probe_topk(torch.from_numpy(queries).to(DEV), db, k, per="query")
    assert names == list(sizes)
    starts = np.cumsum([0] + list(sizes.values()))[:-1]
    got = starts[layer_index.cpu().numpy()] + component.cpu().numpy()
    assert np.array_equal(got, want_ids)
    assert (component.cpu().numpy() < np.array(list(sizes.values()))[layer_index.cpu().numpy()]).all()
    assert np.abs(vals.cpu().numpy() - want_vals).max() <= TOL
    assert len(set(layer_index.cpu().numpy().ravel().tolist())) > 1  # the planted components do span layers


@pytest.mark.parametrize("Q", [7, 512])
def test_no_transpose_trap_512_by_512(Q):
    """512-d queries against a 512-component layer (similarity_score would multiply without the transpose; with Q = 512 it would
    even take the row-wise branch): (C, k) results that agree with the float64 normalize(x) @ normalize(y).T."""
    rows, cols = random_planted(512, Q, 512, seed=Q)
    k = 3
    vals, ids = L.probe_topk(torch.from_numpy(cols).to(DEV), torch.from_numpy(rows).to(DEV), k)
    assert tuple(vals.shape) == (512, k) and tuple(ids.shape) == (512, k)
    check_values(rows, cols, vals.cpu().numpy(), ids.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# API over the suite's fake text tower
# ---------------------------------------------------------------------------------------------------------------------
LETTERS = "abcdefghijklmnopqrstuvwxyz"
TEMPLATES = ["a photo of {}", "{} texture", "an image showing {}."]


def make_vocabulary(V: int, seed: int) -> list[str]:
    rng = np.random.default_rng(seed)
    words, seen = [], set()
    while len(words) < V:
        w = "".join(LETTERS[i] for i in rng.integers(0, 26, size=int(rng.integers(3, 12))))
        key = "".join(sorted(w))  # FakeVLM embeds the character histogram: anagrams would tie exactly
        if key not in seen:
            seen.add(key)
            words.append(w)
    return words


def word_embeddings64(fm: FakeVLM, words: list[str], templates) -> np.ndarray:
    """float64 per-word embeddings computed in the test: mean over the word's own templates minus the empty template."""
    cpu = FakeVLM(dim=fm.dim, ctx=fm.ctx)
    enc = lambda texts: cpu.encode_text(cpu.tokenize(texts)).numpy().astype(np.float64)
    if not templates:
        return enc(words)
    empty = enc([t.format("") for t in templates])
    return np.stack([np.mean(enc([t.format(w) for t in templates]) - empty, axis=0) for w in words])


def api_case(templates, seed: int, V: int = 1200, C: int = 12, k: int = 3, dim: int = 64):
    """A vocabulary and a DB whose float64 top-(k+1) gaps exceed 4 * TOL (asserted by float64_topk); the DB rows are noisy copies
    of a few words' embeddings, so every component has a clear best label."""
    fm = FakeVLM(dim=dim, ctx=40)
    words = make_vocabulary(V, seed)
    emb = word_embeddings64(fm, words, templates)
    rng = np.random.default_rng(seed + 1)
    db = emb[rng.choice(V, size=C, replace=False)] + 0.5 * rng.standard_normal((C, dim)) * np.abs(emb).mean()
    return fm.to(DEV), words, emb, db.astype(np.float32)


@pytest.mark.parametrize("templates,seed", [(None, 0), (TEMPLATES, 0)])
def test_label_components_chunking_and_float64(templates, seed):
    k = 3
    fm, words, emb, db = api_case(templates, seed)
    want_ids, want_vals = float64_topk(db, emb, k)
    results = []
    for chunk_size in (len(words), 1000, 37):
        vals, ids = L.label_components(fm, words, torch.from_numpy(db).to(DEV), k=k, templates=templates, chunk_size=chunk_size,
                                       batch_size=256)
        assert vals.dtype == torch.float32 and ids.dtype == torch.int64 and vals.is_cuda
        results.append((vals.cpu().numpy(), ids.cpu().numpy()))
    for vals, ids in results:
        assert np.array_equal(ids, want_ids)
        assert np.array_equal(ids, results[0][1])
        assert np.abs(vals - results[0][0]).max() <= TOL
        assert np.abs(vals - want_vals).max() <= TOL


def test_embed_words_is_the_per_word_template_mean():
    fm, words, emb, _ = api_case(TEMPLATES, 0, V=50)
    got = L._embed_words(fm, words, TEMPLATES, batch_size=16).cpu().numpy()
    assert np.abs(got - emb).max() <= 1e-4 * np.abs(emb).max()
    plain = L._embed_words(fm, words, None, None).cpu().numpy()
    assert np.array_equal(plain, torch.cat([fm.encode_text(fm.tokenize([w])) for w in words]).cpu().numpy())


def test_label_components_dict_equals_per_layer():
    fm, words, emb, db = api_case(None, 0)
    layers = {"a": torch.from_numpy(db[:5]).to(DEV), "b": torch.from_numpy(db[5:]).to(DEV)}
    both = L.Lens(fm, device=DEV).label_components(words, layers, k=3, chunk_size=500)
    assert list(both) == ["a", "b"]
    for name, layer in layers.items():
        vals, ids = L.label_components(fm, words, layer, k=3, chunk_size=500)
        assert torch.equal(both[name][1], ids)
        assert torch.equal(both[name][0], vals)


def test_search_components_text_queries():
    k = 4
    fm, words, emb, _ = api_case(TEMPLATES, 0, V=40)
    queries = words[:5]
    rng = np.random.default_rng(5)
    total, dim = 900, emb.shape[1]
    comps = rng.standard_normal((total, dim)) * np.abs(emb).mean()
    spots = iter(rng.choice(total, size=5 * (k + 1), replace=False))
    for q in range(5):  # graded copies of each query's embedding, scattered over the layers
        for j in range(k + 1):
            n = rng.standard_normal(dim)
            n -= (n @ emb[q]) / (emb[q] @ emb[q]) * emb[q]
            comps[next(spots)] = emb[q] + 0.15 * (j + 1) * n / np.linalg.norm(n) * np.linalg.norm(emb[q])
    comps = comps.astype(np.float32)
    want_ids, want_vals = float64_topk(emb[:5], comps, k)
    sizes = [200, 300, 400]
    db, off = {}, 0
    for i, n in enumerate(sizes):
        db[f"l{i}"] = torch.from_numpy(comps[off : off + n]).to(DEV)
        off += n
    vals, layer_index, component, names = L.Lens(fm, device=DEV).search_components(queries, db, k=k, templates=TEMPLATES)
    assert names == ["l0", "l1", "l2"]
    starts = np.array([0, 200, 500])
    assert np.array_equal(starts[layer_index.cpu().numpy()] + component.cpu().numpy(), want_ids)
    assert np.abs(vals.cpu().numpy() - want_vals).max() <= TOL


def test_search_components_image_query():
    """Several images are averaged on the host (a CPU probe vector reaches probe_topk): one result row that equals the float64
    top-k of the mean image embedding over the concatenated layers."""
    k = 4
    rng = np.random.default_rng(9)
    images = [torch.from_numpy(rng.integers(0, 4, size=(3, 16, 16)).astype(np.float32)) for _ in range(3)]
    cpu = FakeVLM(dim=64)
    probe = cpu.encode_image(cpu.preprocess(images)).numpy().astype(np.float64).mean(0, keepdims=True)
    total, dim = 600, 64
    comps = rng.standard_normal((total, dim)) * np.abs(probe).mean()
    for j, spot in enumerate(rng.choice(total, size=k + 1, replace=False)):  # graded copies of the probe vector
        n = rng.standard_normal(dim)
        n -= (n @ probe[0]) / (probe[0] @ probe[0]) * probe[0]
        comps[spot] = probe[0] + 0.15 * (j + 1) * n / np.linalg.norm(n) * np.linalg.norm(probe[0])
    comps = comps.astype(np.float32)
    want_ids, want_vals = float64_topk(probe, comps, k)
    fm = FakeVLM(dim=64).to(DEV)
    db = {"a": torch.from_numpy(comps[:250]).to(DEV), "b": torch.from_numpy(comps[250:]).to(DEV)}
    vals, layer_index, component, names = L.Lens(fm, device=DEV).search_components_image(images, db, k=k)
    assert names == ["a", "b"] and tuple(vals.shape) == (1, k)
    starts = np.array([0, 250])
    assert np.array_equal(starts[layer_index.cpu().numpy()] + component.cpu().numpy(), want_ids)
    assert np.abs(vals.cpu().numpy() - want_vals).max() <= TOL
