"""K26 on the GPU: ``sl_rank_merge`` against a numpy restatement of csrc/rank_order.hpp's ``orders_before`` on the same fp32
tiles (equality of int64 counts), rows split over waves, and ``probe_rank`` / ``label_rank`` against the float64 cosine.

The counts are integers, so the kernel tests ask for equality.  End to end the cosine GEMM's rounding can move a target among
candidates within ``TOL`` of it: one test builds data in which no candidate is that close and asks for the exact rank, the others
ask for the interval of ranks float64 allows."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from helpers import FakeVLM
from semanticlens_amd import _native as N
from semanticlens_amd import lens as L

pytestmark = pytest.mark.gpu
TOL = 1e-4  # the suite's bound for a cosine
DEV = "cuda"
SPECIALS = np.array([np.nan, np.inf, 0.5, 0.25, 0.0, -0.0, -1.0, -np.inf], dtype=np.float32)
SENTINEL = 1_000_000_007


# ---------------------------------------------------------------------------------------------------------------------
# kernel, exact
# ---------------------------------------------------------------------------------------------------------------------
def order_key(v: np.ndarray) -> np.ndarray:
    """csrc/packed_best.hpp: f32_order_key, on an fp32 array."""
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    key = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000))
    key = np.where(bits == np.uint32(0x80000000), np.uint32(0x80000000), key)
    return np.where((bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def ref_counts(vals: np.ndarray, id_base: int, key_vals: np.ndarray, key_ids: np.ndarray, start: np.ndarray) -> np.ndarray:
    """``start`` plus, in every slot with a key id >= 0, the number of columns that order before the key (csrc/rank_order.hpp:
    ``orders_before``); the other slots as they were."""
    ck = order_key(vals)[:, None, :]
    cid = (id_base + np.arange(vals.shape[1], dtype=np.int64))[None, None, :]
    k, kid = order_key(key_vals)[:, :, None], key_ids[:, :, None]
    before = (cid != kid) & ((ck > k) | ((ck == k) & (cid < kid)))
    return start + np.where(key_ids >= 0, before.sum(-1), 0)


def fold_tiles(vals: np.ndarray, id_base: int, key_vals: np.ndarray, key_ids: np.ndarray, n_tiles: int, seed: int | None,
               unaligned: bool) -> np.ndarray:
    """The matrix folded as ``n_tiles`` column tiles into counts that start at ``SENTINEL``, in shuffled order (``seed=None``: in
    order).  ``unaligned``: views that start 4 bytes past a 16-byte boundary, with a row stride that is no multiple of 4 and NaN
    around them (``test_gpu_label_distribution.run_tiles``' view)."""
    R, n = vals.shape
    dv = torch.from_numpy(vals).to(DEV)
    counts = torch.full(key_ids.shape, SENTINEL, dtype=torch.int64, device=DEV)
    kv, ki = torch.from_numpy(key_vals).to(DEV), torch.from_numpy(key_ids).to(DEV)
    cuts = np.linspace(0, n, n_tiles + 1).astype(np.int64)
    order = np.arange(n_tiles) if seed is None else np.random.default_rng(seed).permutation(n_tiles)
    for t in order:
        a, b = int(cuts[t]), int(cuts[t + 1])
        if b == a:
            continue
        if unaligned:
            buf = torch.full((R, (b - a) + 3), float("nan"), dtype=torch.float32, device=DEV)
            buf[:, 1 : 1 + (b - a)] = dv[:, a:b]
            tile = buf[:, 1 : 1 + (b - a)]
            assert tile.data_ptr() % 16 == 4
        else:
            tile = dv[:, a:b].contiguous()
        N.rank_merge(counts, tile, kv, ki, id_base + a)
    return counts.cpu().numpy()


def make_keys(vals: np.ndarray, T: int, id_base: int, rng) -> tuple[np.ndarray, np.ndarray]:
    """``(R, T)`` keys: ids before, inside and after the tile, every special value as a key value, a slot in three unused.  A key
    inside the tile carries its own column's value in every other case and another value otherwise (its own column must not be
    counted either way)."""
    R, n = vals.shape
    key_vals = np.empty((R, T), dtype=np.float32)
    key_ids = np.empty((R, T), dtype=np.int64)
    for r in range(R):
        for t in range(T):
            where = (r + t) % 4
            col = int(rng.integers(0, n))
            if where == 0 and id_base > 0:
                key_ids[r, t] = id_base - 1 - int(rng.integers(0, 3))
            elif where == 1:
                key_ids[r, t] = id_base + n + int(rng.integers(0, 3))
            else:
                key_ids[r, t] = id_base + col
            own = where >= 2 and (r + t) % 8 < 4
            key_vals[r, t] = vals[r, col] if own else SPECIALS[(3 * r + t) % len(SPECIALS)]
            if T > 1 and (2 * r + t) % 3 == 1:
                key_ids[r, t] = -1
    return key_vals, key_ids


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("B", [1, 5, 1023, 1024, 1025, 4099])
def test_kernel_exact_against_numpy(B, unaligned):
    R = 3
    for T in (1, 2, 3, 16):
        for id_base in (0, 2**31 + 5, 2**40):
            rng = np.random.default_rng(1000 * B + 10 * T + (id_base % 7))
            vals = SPECIALS[rng.integers(0, len(SPECIALS), size=(R, B))]
            key_vals, key_ids = make_keys(vals, T, id_base, rng)
            want = ref_counts(vals, id_base, key_vals, key_ids, np.full((R, T), SENTINEL, dtype=np.int64))
            assert (want[key_ids < 0] == SENTINEL).all()
            what = f"B={B} T={T} id_base={id_base} unaligned={unaligned}"
            one = fold_tiles(vals, id_base, key_vals, key_ids, 1, None, unaligned)
            assert one.dtype == np.int64 and np.array_equal(one, want), f"one tile, {what}"
            n_tiles = min(3, B)
            assert np.array_equal(fold_tiles(vals, id_base, key_vals, key_ids, n_tiles, None, unaligned), want), f"in order, {what}"
            assert np.array_equal(fold_tiles(vals, id_base, key_vals, key_ids, n_tiles, B + T, unaligned), want), f"shuffled, {what}"


def test_every_special_value_as_key_and_candidate():
    """One row holding every special value, ranked against each of them at every id inside, before and after: ties everywhere."""
    vals = np.tile(SPECIALS, 3)[None, :].copy()
    n = vals.shape[1]
    for id_base in (0, 2**31 + 5):
        ids = [id_base + c for c in range(n)] + [id_base + n] + ([id_base - 1] if id_base else [])
        for key_id in ids:
            for start in range(0, len(SPECIALS), 16):
                kv = SPECIALS[None, start : start + 16].copy()
                ki = np.full(kv.shape, key_id, dtype=np.int64)
                want = ref_counts(vals, id_base, kv, ki, np.full(kv.shape, SENTINEL, dtype=np.int64))
                assert np.array_equal(fold_tiles(vals, id_base, kv, ki, 1, None, False), want), (id_base, key_id)


def test_merge_refuses_bad_arguments():
    tile = torch.zeros((3, 8), dtype=torch.float32, device=DEV)
    counts = torch.zeros((3, 2), dtype=torch.int64, device=DEV)
    kv = torch.zeros((3, 2), dtype=torch.float32, device=DEV)
    ki = torch.zeros((3, 2), dtype=torch.int64, device=DEV)
    N.rank_merge(counts, tile, kv, ki)
    with pytest.raises(ValueError):
        N.rank_merge(counts, tile.double(), kv, ki)
    with pytest.raises(ValueError):
        N.rank_merge(counts, tile[:2], kv, ki)
    with pytest.raises(ValueError):
        N.rank_merge(counts.int(), tile, kv, ki)
    with pytest.raises(ValueError):
        N.rank_merge(counts, tile, kv[:, :1], ki)
    with pytest.raises(ValueError):
        N.rank_merge(torch.zeros((3, 17), dtype=torch.int64, device=DEV), tile, torch.zeros((3, 17), device=DEV),
                     torch.zeros((3, 17), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="id_base"):
        N.rank_merge(counts, tile, kv, ki, id_base=-1)


# ---------------------------------------------------------------------------------------------------------------------
# rows split over waves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2])
def test_split_rows_exact(R):
    lib = N.lib()
    B = 300_000
    while int(lib.sl_rank_merge_splits(R, B)) == 1 and B < 1 << 26:  # a card with so many CUs that this B is not split
        B *= 2
    assert int(lib.sl_rank_merge_splits(R, B)) > 1
    assert int(lib.sl_rank_merge_splits(4096, 4096)) == 1
    rng = np.random.default_rng(R)
    vals = np.round(rng.standard_normal((R, B)), 3).astype(np.float32)  # three decimals: thousands of ties per value
    rows, cols, base = np.arange(R), rng.integers(0, B, size=(R, 3)), 7
    # slots: a column's own value; another value at a column; behind the tile; unused; a NaN key (no candidate is NaN: rank 0)
    key_ids = np.stack([base + cols[:, 0], base + cols[:, 1], np.full(R, base + B + 5), np.full(R, -1), base + cols[:, 2]], axis=1)
    key_vals = np.stack([vals[rows, cols[:, 0]], np.full(R, 0.125), np.zeros(R), np.zeros(R), np.full(R, np.nan)], axis=1)
    key_ids, key_vals = key_ids.astype(np.int64), key_vals.astype(np.float32)
    want = ref_counts(vals, 7, key_vals, key_ids, np.full(key_ids.shape, SENTINEL, dtype=np.int64))
    assert np.array_equal(fold_tiles(vals, 7, key_vals, key_ids, 1, None, False), want)
    assert np.array_equal(fold_tiles(vals, 7, key_vals, key_ids, 1, None, True), want)
    assert (want[:, 3] == SENTINEL).all() and (want[:, 4] == SENTINEL).all() and (want[:, :3] > SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# end to end against the float64 cosine
# ---------------------------------------------------------------------------------------------------------------------
def unit64(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)


def graded(C: int, V: int, D: int, grades: int, seed: int):
    """``test_gpu_topk.graded``: vocabulary rows = each component's vector plus graded noise ORTHOGONAL to it: grade j of component
    c has the cosine 1 / sqrt(1 + (0.1 (j + 1))^2) to it (consecutive gaps above 0.01 up to grade 21), the rest of the vocabulary is
    random (cosines around 1 / sqrt(D)); rows are shuffled."""
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


def random_planted(C: int, V: int, D: int, seed: int):
    """``test_gpu_topk.random_planted``."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((C, D)).astype(np.float32)
    cols = rng.standard_normal((V, D)).astype(np.float32)
    planted = rng.choice(V, size=min(V, C), replace=False)  # a near-copy of a component somewhere in the vocabulary
    cols[planted] = rows[: len(planted)] + 0.05 * rng.standard_normal((len(planted), D)).astype(np.float32)
    return rows, cols


def rank_interval(cos: np.ndarray, targets: np.ndarray):
    """Per (row, slot), from float64 alone: ``(t, lo, hi)`` with t the target's cosine, lo = #(cos > t + 2 TOL) and
    hi = #(cos >= t - 2 TOL) - 1.  The GPU's cosines are within TOL of these, so a candidate more than 2 TOL above the target is
    before it whatever the rounding, and one more than 2 TOL below is behind it."""
    t = np.take_along_axis(cos, targets, axis=1)
    lo = (cos[:, None, :] > (t + 2 * TOL)[:, :, None]).sum(-1)
    hi = (cos[:, None, :] >= (t - 2 * TOL)[:, :, None]).sum(-1) - 1
    return t, lo, hi


_GRADED = {}


def graded_case():
    """(rows, cols, float64 ranks' targets (C,)) of graded(512, 16384, 512, 21), with the gap precondition asserted; once."""
    if not _GRADED:
        C, V, D = 512, 16384, 512
        rows, cols = graded(C, V, D, grades=21, seed=D + C)
        cos = unit64(rows) @ unit64(cols).T
        order = np.argsort(-cos, axis=1, kind="stable")
        grade = np.arange(C) % 20
        targets = order[np.arange(C), grade]  # grade j of a component is its j-th best word
        t = cos[np.arange(C), targets]
        others = np.abs(cos - t[:, None])
        others[np.arange(C), targets] = np.inf
        assert others.min() > 4 * TOL, f"construction: a cosine lies {others.min():.3e} from a target's, not above 4 * TOL"
        _GRADED.update(rows=rows, cols=cols, targets=targets, t=t, grade=grade)
    return _GRADED


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_rank_exact_under_gap_construction(mode):
    case = graded_case()
    grade = case["grade"]
    N.set_gemm_mode(mode)
    try:
        r = L.probe_rank(torch.from_numpy(case["cols"]).to(DEV), torch.from_numpy(case["rows"]).to(DEV), case["targets"].tolist(),
                         chunk_rows=2500)
    finally:
        N.set_gemm_mode(None)
    assert isinstance(r, L.LabelRanks) and r.rank.dtype == torch.int64 and tuple(r.rank.shape) == (512, 1) and r.n_labels == 16384
    assert r.prob is None and r.log_z is None
    assert np.array_equal(r.rank[:, 0].cpu().numpy(), grade)
    assert np.array_equal(r.targets[:, 0].cpu().numpy(), case["targets"])
    err = np.abs(r.value[:, 0].cpu().numpy().astype(np.float64) - case["t"]).max()
    print(f"{mode}: max |value - float64 cosine| = {err:.3e}")
    assert err <= TOL
    assert np.array_equal(r.best().cpu().numpy(), grade)
    assert np.array_equal(r.hit(5).cpu().numpy(), grade < 5)
    assert r.n_evaluated == 512
    assert r.topk_accuracy(5) == float((grade < 5).sum()) / 512
    assert abs(r.mrr() - float(np.mean(1.0 / (grade + 1.0)))) <= 1e-12


_PLANTED = {}


def planted_case():
    if not _PLANTED:
        rows, cols = random_planted(1000, 20000, 768, seed=1768)
        targets = np.random.default_rng(5).integers(0, 20000, size=(1000, 2))
        t, lo, hi = rank_interval(unit64(rows) @ unit64(cols).T, targets)
        _PLANTED.update(rows=rows, cols=cols, targets=targets, t=t, lo=lo, hi=hi)
    return _PLANTED


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_rank_inside_the_float64_interval(mode):
    case = planted_case()
    N.set_gemm_mode(mode)
    try:
        r = L.probe_rank(torch.from_numpy(case["cols"]).to(DEV), torch.from_numpy(case["rows"]).to(DEV), case["targets"].tolist(),
                         chunk_rows=3001)
    finally:
        N.set_gemm_mode(None)
    rank = r.rank.cpu().numpy()
    print(f"{mode}: widest float64 interval {int((case['hi'] - case['lo']).max())} ranks; "
          f"max |value - float64 cosine| = {np.abs(r.value.cpu().numpy() - case['t']).max():.3e}")
    assert (rank >= case["lo"]).all() and (rank <= case["hi"]).all()
    assert np.abs(r.value.cpu().numpy().astype(np.float64) - case["t"]).max() <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# label_rank over the suite's fake text tower
# ---------------------------------------------------------------------------------------------------------------------
LETTERS = "abcdefghijklmnopqrstuvwxyz"
TEMPLATES = ["a photo of {}", "{} texture", "an image showing {}."]


def make_vocabulary(V: int, seed: int) -> list[str]:
    rng = np.random.default_rng(seed)
    words, seen = [], set()
    while len(words) < V:
        w = "".join(LETTERS[i] for i in rng.integers(0, 26, size=int(rng.integers(3, 12))))
        if w not in seen:
            seen.add(w)
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


_CASES = {}


def api_case(templates):
    """(fm, words, float64 cosines (C, V), db, targets (C, 2)) for a (200, 16) DB and 1 200 words; once per template setting.
    The fake text tower is linear in a prompt's characters, so a template only shows where the prompt is cut: at 24 tokens the
    longest template cuts words of 7 letters and more."""
    key = bool(templates)
    if key not in _CASES:
        fm = FakeVLM(dim=16, ctx=24)
        words = make_vocabulary(1200, seed=3)
        emb = word_embeddings64(fm, words, templates)
        db = np.random.default_rng(4).standard_normal((200, 16)).astype(np.float32)
        targets = np.random.default_rng(6).integers(0, len(words), size=(200, 2))
        _CASES[key] = (words, unit64(db) @ unit64(emb).T, db, targets)
    words, cos, db, targets = _CASES[key]
    return FakeVLM(dim=16, ctx=24).to(DEV), words, cos, torch.from_numpy(db).to(DEV), targets


@pytest.mark.parametrize("templates", [None, TEMPLATES])
def test_label_rank_words_indices_chunking_and_float64(templates):
    fm, words, cos, db, targets = api_case(templates)
    t, lo, hi = rank_interval(cos, targets)
    by_index = targets.tolist()
    by_word = [[words[i] for i in row] for row in by_index]
    by_word[3] = words[targets[3, 0]]  # a bare word and a bare index are one-target rows
    by_index[3] = int(targets[3, 0])
    by_word[5] = by_index[5] = None
    used = np.ones(targets.shape, dtype=bool)
    used[3, 1] = False
    used[5] = False
    for chunk_size in (64, None):
        r = L.label_rank(fm, words, db, by_index, templates=templates, chunk_size=chunk_size, batch_size=512)
        w = L.label_rank(fm, words, db, by_word, templates=templates, chunk_size=chunk_size, batch_size=512)
        for field in ("rank", "targets"):
            assert torch.equal(getattr(r, field), getattr(w, field)), field
        assert torch.equal(r.value.view(torch.int32), w.value.view(torch.int32))
        assert r.rank.is_cuda and r.rank.dtype == torch.int64 and r.value.dtype == torch.float32 and r.n_labels == len(words)
        rank, value = r.rank.cpu().numpy(), r.value.cpu().numpy()
        assert (r.targets.cpu().numpy()[used] == targets[used]).all() and (r.targets.cpu().numpy()[~used] == -1).all()
        assert (rank[~used] == -1).all() and np.isnan(value[~used]).all()
        assert (rank[used] >= lo[used]).all() and (rank[used] <= hi[used]).all(), f"chunk_size={chunk_size}"
        assert np.abs(value[used].astype(np.float64) - t[used]).max() <= TOL
        assert r.n_evaluated == 199 and r.best()[5] == -1 and not r.hit(len(words))[5]
    if templates:  # the templates are applied: without them the same words have other cosines
        plain = L.label_rank(fm, words, db, by_index, chunk_size=None)
        assert np.abs(plain.value.cpu().numpy()[used] - value[used]).max() > 100 * TOL


def test_label_rank_dict_returns_the_named_layers_only():
    fm, words, _, db, targets = api_case(None)
    layers = {"a": db[:120], "b": db[120:]}
    tb = targets[120:].tolist()
    got = L.Lens(fm, device=DEV).label_rank(words, layers, {"b": tb}, chunk_size=500)
    assert list(got) == ["b"]
    one = L.label_rank(fm, words, layers["b"], tb, chunk_size=500)
    assert torch.equal(got["b"].rank, one.rank) and torch.equal(got["b"].value, one.value)
    both = L.label_rank(fm, words, layers, {"b": tb, "a": targets[:120, 0].tolist()}, chunk_size=500)
    assert list(both) == ["a", "b"] and torch.equal(both["b"].rank, one.rank) and tuple(both["a"].rank.shape) == (120, 1)


def test_label_rank_prob_and_log_z():
    """``prob`` is float32: a probability float64 puts below float32's smallest normal number cannot carry a relative bound in
    that format and is only asked to stay below it; every other one is held to 1e-4 relative.  Each component's best label is a
    target next to the random one, so that probabilities near 1 are among those checked."""
    scale, tiny = 100.0, float(np.finfo(np.float32).tiny)
    fm, words, cos, db, targets = api_case(TEMPLATES)
    targets = np.concatenate([targets[:, :1], cos.argmax(axis=1)[:, None]], axis=1)
    r = L.label_rank(fm, words, db, targets.tolist(), templates=TEMPLATES, chunk_size=500, batch_size=512, logit_scale=scale)
    dist = L.label_distribution(fm, words, db, k=1, logit_scale=scale, templates=TEMPLATES, chunk_size=500, batch_size=512)
    assert r.logit_scale == scale and r.log_z.dtype == torch.float64 and r.prob.dtype == torch.float32
    assert torch.equal(r.log_z, dist.log_z)
    logits = torch.from_numpy(scale * cos)
    want = (torch.gather(logits, 1, torch.from_numpy(targets)) - torch.logsumexp(logits, 1)[:, None]).exp()
    got = r.prob.cpu().double()
    normal = want >= tiny
    rel = ((got - want).abs() / want)[normal].max()
    print(f"max relative error of prob against float64: {float(rel):.3e} over {int(normal.sum())} of {normal.numel()} probabilities; "
          f"largest {float(want.max()):.3f}")
    assert int(normal.sum()) >= normal.numel() // 2 and float(want.max()) > 0.5
    assert float(rel) <= 1e-4
    assert (got[~normal] <= tiny).all()
    without = L.label_rank(fm, words, db, targets.tolist(), templates=TEMPLATES, chunk_size=500, batch_size=512)
    assert torch.equal(without.rank, r.rank) and without.prob is None and without.log_z is None


def test_nan_target_ranks_first_and_is_left_out_of_the_metrics():
    fm, words, _, db, targets = api_case(None)
    db = db[:40].clone()
    db[7, 3] = float("nan")
    r = L.label_rank(fm, words, db, targets[:40, 0].tolist(), chunk_size=300)
    assert int(r.rank[7, 0]) == int(targets[7, 0])  # every cosine of the row is NaN: ties, by the smaller id
    assert math.isnan(float(r.value[7, 0])) and int(r.best()[7]) == -1 and r.n_evaluated == 39
