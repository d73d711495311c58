"""K22 on the device: the per-segment column-max kernel against a numpy lexsort (ids exact, values bit for bit after the two
mappings the packing makes, raw states bit-identical across cuts), the tiled cosine + per-set max driver against the float64
cosine, the audit API over the suite's fake text tower, and the memory bound.

``TOL`` is the project's bound for cosine values (1e-4).  The driver and API checks hold for EVERY (set, component): the returned
id lies in the set, the returned value is within TOL of the float64 cosine of its own pair, and no member of the set is above it
by more than 2 * TOL.  Id equality with the float64 argmax is asserted wherever the float64 top-two gap inside the set exceeds
4 * TOL (or the set has one member); the share of the other pairs is asserted to be at most 5 %."""
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
MAX_ID = (1 << 32) - 2
CANONICAL_NAN = np.uint32(0x7FC00000)
MAX_EXEMPT_SHARE = 0.05


# ---------------------------------------------------------------------------------------------------------------------
# kernel, exact
# ---------------------------------------------------------------------------------------------------------------------
def special_matrix(R: int, n: int, seed: int) -> np.ndarray:
    """Heavy exact ties, +-0.0, +-inf, NaN, mixed with a few distinct values (the recipe of test_gpu_compare.special_matrix)."""
    rng = np.random.default_rng(seed)
    pool = np.array([-np.inf, -1.0, -0.0, 0.0, 0.5, 0.5, 1.0, np.inf, np.nan, 0.25, -0.25, 1e-30, -1e-30], dtype=np.float32)
    v = pool[rng.integers(0, len(pool), size=(R, n))]
    mix = rng.random((R, n)) < 0.3
    v[mix] = rng.standard_normal(int(mix.sum())).astype(np.float32).round(1)  # one decimal: still many ties
    return v


def canonical_bits(v: np.ndarray) -> np.ndarray:
    """Bit patterns after -0.0 -> +0.0 and NaN -> the canonical quiet NaN (what the packed state keeps of a value)."""
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).copy()
    bits[bits == np.uint32(0x80000000)] = 0
    bits[np.isnan(v)] = CANONICAL_NAN
    return bits


def run_segments(R: int, G: int, max_run: int, n_empty: int, seed: int) -> np.ndarray:
    """Row segments as runs: 70 % of the run lengths from [1, min(8, max_run)], the rest from [1, max_run], the first two being 1
    and max_run.  The first runs walk through a permutation of the segments that may own rows (all but ``n_empty`` of them),
    later runs draw from those at random, so a segment's rows need not be adjacent."""
    rng = np.random.default_rng(seed)
    allowed = np.sort(rng.permutation(G)[: G - n_empty])
    order = rng.permutation(allowed)
    seg = np.empty(R, dtype=np.int32)
    r = k = 0
    while r < R:
        if k < 2:
            n = (1, max_run)[k]
        else:
            n = int(rng.integers(1, (min(8, max_run) if rng.random() < 0.7 else max_run) + 1))
        seg[r : r + n] = order[k] if k < len(order) else allowed[rng.integers(0, len(allowed))]
        r, k = r + n, k + 1
    return seg


def interleaved_segments(R: int, G: int) -> np.ndarray:
    """No runs at all: row r belongs to segment r mod G; every 50th row to none (-1), and one row names a segment past the end."""
    seg = (np.arange(R) % G).astype(np.int32)
    seg[::50] = -1
    if R > 75:
        seg[75] = G
    return seg


def ref_segbest(vals: np.ndarray, seg: np.ndarray, G: int, row_base: int):
    """numpy reference per (segment, column): the first entry of a lexsort on (is-NaN descending, value descending with +-0 equal,
    id ascending) — one lexsort of the flattened tile with (segment, column) as its leading key."""
    R, B = vals.shape
    out_v = np.full((G, B), -np.inf, dtype=np.float32)
    out_i = np.full((G, B), -1, dtype=np.int64)
    keep = np.nonzero((seg >= 0) & (seg < G))[0]
    rows = np.repeat(keep, B)
    cols = np.tile(np.arange(B, dtype=np.int64), len(keep))
    flat = vals[keep].ravel()
    nan = np.isnan(flat)
    key = np.where(nan, 0.0, flat).astype(np.float64) + 0.0  # -0.0 and +0.0 compare equal
    group = seg[rows].astype(np.int64) * B + cols
    order = np.lexsort((rows, -key, ~nan, group))
    sorted_group = group[order]
    pick = order[np.r_[True, sorted_group[1:] != sorted_group[:-1]]]
    out_v.ravel()[group[pick]] = flat[pick]
    out_i.ravel()[group[pick]] = row_base + rows[pick]
    return out_v, out_i


PAD = 5  # state columns beyond B: state_ld > B, and nothing may be written there


def run_tiles(vals: np.ndarray, seg: np.ndarray, G: int, n_tiles: int, row_base: int, seed: int, unaligned: bool):
    """Fold ``vals`` into a fresh ``(G, B + PAD)`` state as ``n_tiles`` tiles, cut along rows and along columns, in shuffled
    order; returns the raw state and its decoded form."""
    R, B = vals.shape
    if n_tiles == 64 and min(R, B) > 1:
        grid_r, grid_c = 8, 8  # (5, 3) leaves some of the 64 empty: they are skipped
    else:  # one cut direction: along the longer side
        grid_r, grid_c = (n_tiles, 1) if R >= B else (1, n_tiles)
    rcuts = np.linspace(0, R, grid_r + 1).astype(np.int64)
    ccuts = np.linspace(0, B, grid_c + 1).astype(np.int64)
    state = torch.zeros((G, B + PAD), dtype=torch.int64, device=DEV)
    full = torch.from_numpy(vals).to(DEV)
    seg_d = torch.from_numpy(seg).to(DEV)
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
        N.segmax_merge(state[:, ca:cb], tile, seg_d[ra:rb], row_base + ra)
    v, i = N.setmax_finish(state)
    torch.cuda.synchronize()
    return state.cpu().numpy(), v.cpu().numpy(), i.cpu().numpy()


KERNEL_CASES = [
    # R, B, G, segments
    (1, 1, 1, lambda: np.zeros(1, dtype=np.int32)),
    (5, 3, 2, lambda: run_segments(5, 2, 3, 0, seed=1)),
    (70, 257, 9, lambda: run_segments(70, 9, 8, 0, seed=2)),
    (300, 4099, 40, lambda: run_segments(300, 40, 8, 0, seed=3)),
    (4099, 300, 300, lambda: run_segments(4099, 300, 64, 5, seed=4)),  # run lengths 1 .. 64; five segments own no row
    (2000, 1030, 3, lambda: interleaved_segments(2000, 3)),
]


@pytest.mark.parametrize("R,B,G,make_seg", KERNEL_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in KERNEL_CASES])
def test_kernel_exact_against_lexsort(R, B, G, make_seg):
    vals = special_matrix(R, B, seed=R * 1000 + B)
    seg = make_seg()
    assert seg.shape == (R,) and seg.dtype == np.int32
    owners = np.unique(seg[(seg >= 0) & (seg < G)])
    if (R, B, G) == (4099, 300, 300):
        runs = np.diff(np.r_[0, np.nonzero(np.diff(seg))[0] + 1, R])
        assert runs.min() == 1 and runs.max() == 64 and len(owners) == G - 5
    row_base = MAX_ID + 1 - R  # the last row has the largest id a state can hold
    want_v, want_i = ref_segbest(vals, seg, G, row_base)
    rowless = np.setdiff1d(np.arange(G), owners)
    first = None
    for n_tiles in (1, 7, 64):
        state, v, i = run_tiles(vals, seg, G, n_tiles, row_base, seed=n_tiles, unaligned=(n_tiles == 7))
        assert np.array_equal(i[:, :B], want_i), f"{n_tiles} tiles: ids differ in {int((i[:, :B] != want_i).sum())} entries"
        assert np.array_equal(canonical_bits(v[:, :B]), canonical_bits(want_v)), f"{n_tiles} tiles: value bit patterns differ"
        assert np.array_equal(v.view(np.uint32), canonical_bits(v))  # what comes back IS canonical
        # a segment without rows, and the state columns beyond B, are untouched and decode as empty
        assert (state[rowless] == 0).all() and (state[:, B:] == 0).all()
        assert np.isneginf(v[rowless]).all() and (i[rowless] == -1).all()
        assert np.isneginf(v[:, B:]).all() and (i[:, B:] == -1).all()
        assert (i[owners][:, :B] >= row_base).all()
        if first is None:
            first = state
        assert np.array_equal(state, first)  # the cut and its order do not show


def test_merge_refusals_leave_the_state_untouched():
    tile = torch.ones(4, 8, device=DEV)
    seg = torch.zeros(4, dtype=torch.int32, device=DEV)
    state = torch.zeros(3, 8, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="int64"):
        N.segmax_merge(state.to(torch.float64), tile, seg)
    with pytest.raises(ValueError, match="int64"):
        N.segmax_merge(state.to(torch.int32), tile, seg)
    with pytest.raises(ValueError, match="the state must be"):
        N.segmax_merge(state[:, :7], tile, seg)
    with pytest.raises(ValueError, match="the state must be"):
        N.segmax_merge(state[0], tile, seg)
    with pytest.raises(ValueError, match="the state must be"):
        N.segmax_merge(state.cpu(), tile, seg)
    with pytest.raises(ValueError, match="unit column stride"):
        N.segmax_merge(torch.zeros(8, 3, dtype=torch.int64, device=DEV).t(), tile, seg)
    with pytest.raises(ValueError, match="segment table"):
        N.segmax_merge(state, tile, seg[:3])
    with pytest.raises(ValueError, match="segment table"):
        N.segmax_merge(state, tile, seg.to(torch.int64))
    with pytest.raises(ValueError, match="segment table"):
        N.segmax_merge(state, tile, seg.cpu())
    with pytest.raises(ValueError, match="float32"):
        N.segmax_merge(state, tile.double(), seg)
    with pytest.raises(ValueError, match="2\\^32 - 2"):
        N.segmax_merge(state, tile, seg, MAX_ID - 2)
    with pytest.raises(ValueError, match="2\\^32 - 2"):
        N.segmax_merge(state, tile, seg, -1)
    torch.cuda.synchronize()
    assert (state == 0).all()
    N.segmax_merge(state, tile, seg, MAX_ID - 3)  # the same call with ids in range writes segment 0 only
    v, i = N.setmax_finish(state)
    assert (v[0] == 1).all() and (i[0] == MAX_ID - 3).all() and (state[1:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# driver: tiled cosine + per-set max against the float64 cosine
# ---------------------------------------------------------------------------------------------------------------------
def unit64(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)


def offsets_of(sizes) -> list[int]:
    return [0] + [int(s) for s in np.cumsum(sizes)]


def check_setmax(cos: np.ndarray, offsets: list[int], vals: np.ndarray, ids: np.ndarray, what: str = ""):
    """``cos``: the float64 (P, C) cosines.  Every (g, c) is held to the three value checks; ids equal the float64 argmax wherever
    the float64 top-two gap inside the set exceeds 4 * TOL or the set has one member; the other pairs' share is at most 5 %."""
    G, C = len(offsets) - 1, cos.shape[1]
    assert vals.shape == (G, C) and ids.shape == (G, C)
    worst_val = worst_miss = 0.0
    exempt = wrong = 0
    cols = np.arange(C)
    for g, (a, b) in enumerate(zip(offsets, offsets[1:])):
        assert b > a
        assert (ids[g] >= a).all() and (ids[g] < b).all(), f"set {g}: an id outside the set's rows [{a}, {b})"
        sub = cos[a:b]
        own = cos[ids[g], cols]
        worst_val = max(worst_val, float(np.abs(own - vals[g]).max()))
        worst_miss = max(worst_miss, float((sub.max(axis=0) - own).max()))
        if b - a == 1:
            clear = np.ones(C, dtype=bool)
        else:
            top2 = np.sort(np.partition(sub, -2, axis=0)[-2:], axis=0)
            clear = (top2[1] - top2[0]) > 4 * TOL
        exempt += int((~clear).sum())
        wrong += int((ids[g][clear] != a + sub.argmax(axis=0)[clear]).sum())
    share = exempt / (G * C)
    print(f"{what}max |value - float64 cosine| = {worst_val:.3e}; max (best member - returned) = {worst_miss:.3e}; "
          f"ids off the float64 argmax where the gap is clear: {wrong}; exempt share {share:.4f}")
    assert worst_val <= TOL
    assert worst_miss <= 2 * TOL
    assert wrong == 0
    assert share <= MAX_EXEMPT_SHARE
    return share


DRIVER_CASES = {
    # name: (C, D, set sizes, seed, chunk_rows, chunk_cols)
    "700x256": (700, 256, [1, 1, 2, 5, 17, 64, 130, 3, 300, 77], 0, 97, None),
    "3000x1152": (3000, 1152, [1, 2, 40, 257, 9, 600, 91], 1, 333, 1100),
}
DRIVER_DATA = {}


def driver_case(name):
    if name not in DRIVER_DATA:  # the float64 reference once per case, shared by both GEMM modes and left unchanged
        C, D, sizes, seed, chunk_rows, chunk_cols = DRIVER_CASES[name]
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((sum(sizes), D)).astype(np.float32)  # the prompts are drawn before the DB
        y = rng.standard_normal((C, D)).astype(np.float32)
        DRIVER_DATA[name] = (x, y, offsets_of(sizes), unit64(x) @ unit64(y).T, chunk_rows, chunk_cols)
    return DRIVER_DATA[name]


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", list(DRIVER_CASES))
def test_driver_against_float64(mode, name):
    x, y, offsets, cos, chunk_rows, chunk_cols = driver_case(name)
    N.set_gemm_mode(mode)
    try:
        state = N.setmax_probe(torch.from_numpy(x).to(DEV), offsets, torch.from_numpy(y).to(DEV), chunk_rows, chunk_cols)
        vals, ids = N.setmax_finish(state)
    finally:
        N.set_gemm_mode(None)
    assert state.dtype == torch.int64 and tuple(state.shape) == (len(offsets) - 1, y.shape[0])
    assert vals.dtype == torch.float32 and ids.dtype == torch.int64 and vals.is_cuda
    check_setmax(cos, offsets, vals.cpu().numpy(), ids.cpu().numpy(), what=f"{name} {mode}: ")


def test_continuation_over_a_cut_inside_a_set():
    x, y, offsets, cos, chunk_rows, _ = driver_case("700x256")
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    whole = N.setmax_probe(xd, offsets, yd, chunk_rows)
    P, h = x.shape[0], 300
    assert any(a < h < b for a, b in zip(offsets, offsets[1:]))  # the cut falls inside a set
    clip = lambda lo, hi: [min(max(o, lo), hi) - lo for o in offsets]
    state = N.setmax_probe(xd[:h], clip(0, h), yd, chunk_rows)
    again = N.setmax_probe(xd[h:], clip(h, P), yd, chunk_rows, id_base=h, state=state)
    assert again is state
    assert torch.equal(state, whole)
    # the other order, and a chunk in which most sets are empty, give the same bits too
    state = N.setmax_probe(xd[h:], clip(h, P), yd, chunk_rows, id_base=h)
    N.setmax_probe(xd[:h], clip(0, h), yd, 41, 333, state=state)
    assert torch.equal(state, whole)


def test_empty_sets_and_empty_operands():
    x = torch.randn(6, 16, device=DEV)
    y = torch.randn(5, 16, device=DEV)
    vals, ids = N.setmax_finish(N.setmax_probe(x, [0, 0, 4, 4, 6], y))
    assert tuple(vals.shape) == (4, 5)
    assert torch.isneginf(vals[[0, 2]]).all() and (ids[[0, 2]] == -1).all()
    assert ((ids[1] >= 0) & (ids[1] < 4)).all() and ((ids[3] >= 4) & (ids[3] < 6)).all()
    vals, ids = L.probe_setmax(x[:0], [0, 0], y)
    assert tuple(vals.shape) == (1, 5) and torch.isneginf(vals).all() and (ids == -1).all()
    vals, ids = L.probe_setmax(x, [0, 6], y[:0])
    assert tuple(vals.shape) == (1, 0) and ids.dtype == torch.int64


def test_single_prompt_sets_against_k17():
    """Sets of one prompt each make the state the whole (P, C) cosine matrix: its row and column maxima against K17's k = 1."""
    x, y, _, cos, _, _ = driver_case("700x256")
    xd, yd = torch.from_numpy(x[:200]).to(DEV), torch.from_numpy(y).to(DEV)
    vals, ids = L.probe_setmax(xd, list(range(201)), yd, chunk_rows=64)
    assert torch.equal(ids, torch.arange(200, device=DEV)[:, None].expand(200, 700))
    assert np.abs(vals.cpu().numpy() - cos[:200]).max() <= TOL
    qv, _, qcomp, _ = L.probe_topk(xd, yd, 1, per="query")
    assert (vals.amax(dim=1) - qv[:, 0]).abs().max().item() <= TOL
    assert (vals.gather(1, qcomp) - qv).abs().max().item() <= TOL
    cv, cid = L.probe_topk(xd, yd, 1, per="component")
    assert (vals.amax(dim=0) - cv[:, 0]).abs().max().item() <= TOL
    assert (vals.gather(0, cid.t()) - cv.t()).abs().max().item() <= TOL


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_one_set_equals_mutual_probe_columns_bit_for_bit(mode):
    x, y, _, _, _, _ = driver_case("3000x1152")
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    N.set_gemm_mode(mode)
    try:
        (_, _), (want_v, want_i) = N.mutual_probe(xd, yd, 333, 1100)
        vals, ids = N.setmax_finish(N.setmax_probe(xd, [0, x.shape[0]], yd, 333, 1100))
    finally:
        N.set_gemm_mode(None)
    assert torch.equal(ids[0], want_i)
    assert torch.equal(vals[0].view(torch.int32), want_v.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# API over the suite's fake text tower
# ---------------------------------------------------------------------------------------------------------------------
LETTERS = "abcdefghijklmnopqrstuvwxyz"
TEMPLATES = ["a photo of {}", "{} texture", "an image showing {}."]
SET_SIZES = {"ox/valid": 3, "ox/parts": 60, "plough/valid": 1, "cart/valid": 17, "ox/spurious": 200, "plough/spurious": 2,
             "cart/spurious": 120, "background": 40}
VALID = ["ox/valid", "ox/parts", "plough/valid", "cart/valid"]
SPURIOUS = ["ox/spurious", "plough/spurious", "cart/spurious", "background"]
N_PLANTED = 12  # components planted on a word of a valid set, and as many on a word of a spurious set


def make_vocabulary(V: int, seed: int) -> list[str]:
    """The recipe of test_gpu_topk.make_vocabulary: random words, no two of them anagrams of each other."""
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
    """float64 per-word embeddings computed in the test: mean over the word's own templates minus the empty template (the recipe
    of test_gpu_topk.word_embeddings64)."""
    cpu = FakeVLM(dim=fm.dim, ctx=fm.ctx)
    enc = lambda texts: cpu.encode_text(cpu.tokenize(texts)).numpy().astype(np.float64)
    if not templates:
        return enc(words)
    empty = enc([t.format("") for t in templates])
    return np.stack([np.mean(enc([t.format(w) for t in templates]) - empty, axis=0) for w in words])


API_DATA = {}


def api_case(templated: bool):
    """8 named sets of 1 to 200 words, their float64 embeddings, and a DB of 2 * N_PLANTED components: the first N_PLANTED are
    noisy copies (cosine about 0.98) of words of valid sets, the others of words of spurious sets.  Returns the float64 cosines
    too, after asserting that every component's float64 margin has the planted sign by more than 4 * TOL."""
    if templated not in API_DATA:
        templates = TEMPLATES if templated else None
        fm = FakeVLM(dim=64, ctx=40)
        words = make_vocabulary(sum(SET_SIZES.values()), seed=11)
        sets, start = {}, 0
        for name, n in SET_SIZES.items():
            sets[name] = words[start : start + n]
            start += n
        offsets = offsets_of(list(SET_SIZES.values()))
        emb = word_embeddings64(fm, words, templates)
        rng = np.random.default_rng(12)
        names = list(SET_SIZES)
        rows_of = lambda group: np.concatenate([np.arange(offsets[names.index(n)], offsets[names.index(n) + 1]) for n in group])
        on = np.r_[rng.choice(rows_of(VALID), N_PLANTED, replace=False), rng.choice(rows_of(SPURIOUS), N_PLANTED, replace=False)]
        db = (emb[on] + 0.2 * rng.standard_normal((2 * N_PLANTED, 64)) * emb.std()).astype(np.float32)
        cos = unit64(emb) @ unit64(db).T
        best = lambda group: np.max([cos[offsets[names.index(n)] : offsets[names.index(n) + 1]].max(axis=0) for n in group], axis=0)
        margin = best(SPURIOUS) - best(VALID)
        assert (margin[:N_PLANTED] < -4 * TOL).all() and (margin[N_PLANTED:] > 4 * TOL).all(), "construction: a margin is unclear"
        API_DATA[templated] = (sets, words, offsets, db, cos, margin, templates)
    return API_DATA[templated]


@pytest.mark.parametrize("templated", [False, True], ids=["plain", "templates"])
def test_audit_chunking_and_float64(templated):
    sets, words, offsets, db, cos, margin, templates = api_case(templated)
    fm = FakeVLM(dim=64, ctx=40).to(DEV)
    dbd = torch.from_numpy(db).to(DEV)
    audits = [L.audit_concepts(fm, sets, dbd, templates=templates, batch_size=256, chunk_size=chunk) for chunk in (None, 100, 7)]
    first = audits[0]
    assert isinstance(first, L.ConceptAudit)
    assert first.sets == list(SET_SIZES) and first.prompts == words and first.set_offsets == offsets and first.layers == [None]
    assert tuple(first.alignment[None].shape) == (8, 2 * N_PLANTED) and first.alignment[None].dtype == torch.float32
    assert first.best_prompt[None].dtype == torch.int64 and first.alignment[None].is_cuda
    G = len(offsets) - 1
    clear = np.ones((G, db.shape[0]), dtype=bool)
    for g, (a, b) in enumerate(zip(offsets, offsets[1:])):
        if b - a > 1:
            top2 = np.sort(np.partition(cos[a:b], -2, axis=0)[-2:], axis=0)
            clear[g] = (top2[1] - top2[0]) > 4 * TOL
    v0, i0 = first.alignment[None].cpu().numpy(), first.best_prompt[None].cpu().numpy()
    for chunk, audit in zip(("all", 100, 7), audits):
        v, i = audit.alignment[None].cpu().numpy(), audit.best_prompt[None].cpu().numpy()
        check_setmax(cos, offsets, v, i, what=f"chunk_size {chunk}: ")
        assert np.array_equal(i[clear], i0[clear])
        assert np.abs(v - v0).max() <= TOL
    # margin, flag, rank and describe on the device, against float64
    m = first.margin(valid=VALID, spurious=SPURIOUS)[None]
    assert m.is_cuda and np.abs(m.cpu().numpy() - margin).max() <= 2 * TOL  # a difference of two values, each within TOL
    flagged = first.flag(valid=VALID, spurious=SPURIOUS)[None].cpu().numpy()
    assert np.array_equal(flagged, np.arange(2 * N_PLANTED) >= N_PLANTED)  # exactly the components planted on a spurious word
    vals, layer, comp = first.rank(valid=VALID, spurious=SPURIOUS, k=5)
    assert (layer == 0).all() and set(comp.tolist()) <= set(range(N_PLANTED, 2 * N_PLANTED))
    assert np.abs(vals.cpu().numpy() - np.sort(margin)[::-1][:5]).max() <= 2 * TOL
    described = first.describe(None, N_PLANTED)
    assert [name for name, _, _ in described] == list(SET_SIZES)
    for g, (name, value, prompt) in enumerate(described):
        assert prompt == words[i0[g, N_PLANTED]] and prompt in sets[name] and abs(value - v0[g, N_PLANTED]) == 0


def test_audit_dict_db_lens_method_and_cpu_db():
    sets, words, offsets, db, cos, margin, _ = api_case(False)
    fm = FakeVLM(dim=64, ctx=40).to(DEV)
    layers = {"a": torch.from_numpy(db[:9]).to(DEV), "b": torch.from_numpy(db[9:]).to(DEV)}
    both = L.Lens(fm, device=DEV).audit_concepts(sets, layers, chunk_size=100)
    assert both.layers == ["a", "b"] and list(both.alignment) == ["a", "b"]
    for name, layer in layers.items():
        one = L.audit_concepts(fm, sets, layer, chunk_size=100)
        assert torch.equal(both.alignment[name], one.alignment[None])
        assert torch.equal(both.best_prompt[name], one.best_prompt[None])
    flagged = both.flag(valid=VALID, spurious=SPURIOUS)
    assert not flagged["a"].any() and np.array_equal(flagged["b"].cpu().numpy(), np.arange(9, 2 * N_PLANTED) >= N_PLANTED)
    vals, layer, comp = both.rank(valid=VALID, spurious=SPURIOUS, k=1000)
    assert tuple(vals.shape) == (2 * N_PLANTED,) and (layer[:N_PLANTED] == 1).all() and (comp[:N_PLANTED] >= N_PLANTED - 9).all()
    # the vector-level entry on the same embeddings, and a DB on the host: results come back to the host
    emb = L._embed_words(fm, words, None, None)
    pv, pi = L.probe_setmax(emb, offsets, layers["a"])
    assert torch.equal(pv, both.alignment["a"]) and torch.equal(pi, both.best_prompt["a"])
    host = L.probe_setmax(emb, offsets, {"a": layers["a"].cpu()}, chunk_rows=50)
    assert not host["a"][0].is_cuda and torch.equal(host["a"][1], pi.cpu())
    with pytest.raises(ValueError, match="does not match"):
        L.audit_concepts(fm, sets, torch.zeros(4, 32, device=DEV))  # the width is known once the first chunk is embedded


# ---------------------------------------------------------------------------------------------------------------------
# memory
# ---------------------------------------------------------------------------------------------------------------------
def test_memory_at_full_size():
    """P = 20 000 vectors in G = 200 sets against C = 32 768 components at D = 64 (the full matrix would be 2.6 GB): the rise of
    the allocator's peak over the call stays below tile + states + GEMM workspace + 32 MB, which is below a quarter of the
    matrix; the embeddings are resident before the call."""
    P, G, C, D = 20000, 200, 32768, 64
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(P, D, generator=g).to(DEV)
    y = torch.randn(C, D, generator=g).to(DEV)
    y[:64] = x[10000:10064] * 2.0  # a few exact counterparts, checked below
    offsets = list(range(0, P + 1, P // G))
    rows = N.topk_chunk_rows(C, P)
    ws_bytes = int(N.lib().sl_cosine_nt_ws_bytes(rows, C, D))
    bound = N.TOPK_TILE_BYTES + 20 * G * C + ws_bytes + (32 << 20)
    matrix = P * C * 4
    assert bound < matrix // 4
    L.probe_setmax(x[:300], [0, 100, 300], y[:128])  # code objects loaded before the measured call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    vals, ids = L.probe_setmax(x, offsets, y)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB, full matrix {matrix / 2**20:.0f} MiB")
    assert rise <= bound
    assert tuple(vals.shape) == (G, C)
    lo = torch.arange(G, device=DEV)[:, None] * (P // G)
    assert ((ids >= lo) & (ids < lo + P // G)).all()
    assert torch.equal(ids[100, :64].cpu(), torch.arange(10000, 10064))  # prompts 10 000 .. 10 063 lie in set 100
    assert (vals[100, :64] - 1).abs().max().item() <= TOL
