"""K25 on the GPU: the streaming softmax statistics (``sl_softmax_*``) against float64 torch on the same fp32 tiles, their
special values, ``finish``, and ``label_distribution`` / ``probe_softmax`` over the suite's fake text tower.

The tolerance is DESIGN.md §K25's, derived from the kernel's arithmetic and restated in ``softmax_bound``; no constant in it comes
from a run of the kernel."""
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
U = 2.0 ** -24


def softmax_bound(scale: float, gap: float, n: int) -> tuple[float, float, float]:
    """``(log_z absolute, probs relative, entropy absolute)`` bounds of DESIGN.md §K25 for ``n`` candidates whose largest and
    smallest differ by ``gap``, in units of u = 2^-24.  With G = scale * gap (the logit gap), L = ln max(n, 8),
    D1 = min(G, L) >= E_p|d| and D2 = min(G, 2 L) min(G, L) + 4 L^2 / max(n, 8) >= E_p d^2:
        log_z    (3 D1 + 18) u       3 u |d| on every exponent, 2 u for v_exp_f32, 15 u for a 16-term fp32 sum, 1 u for all fp64 steps
        probs    log_z's + 2 u       the rounding of the fp32 result and of the fp64 exponent
        entropy  log_z's + (21 D1 + 3 D2) u"""
    G, lg, nn = scale * gap, math.log(max(n, 8)), max(n, 8)
    d1 = min(G, lg)
    d2 = min(G, 2 * lg) * d1 + 4 * lg * lg / nn
    lz = (3 * d1 + 18) * U
    return lz, lz + 2 * U, lz + (21 * d1 + 3 * d2) * U


def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def is_split(R: int, B: int) -> bool:
    return int(N.lib().sl_softmax_merge_ws_bytes(R, B)) > 0


# ---------------------------------------------------------------------------------------------------------------------
# kernel against float64
# ---------------------------------------------------------------------------------------------------------------------
def planted(R: int, n: int, seed: int) -> torch.Tensor:
    """Uniform in [-1, 1] with a cluster of near-maxima per row, on the device."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, size=(R, n)).astype(np.float32)
    m = min(n, 12)
    cols = rng.integers(0, n, size=(R, m))
    v[np.arange(R)[:, None], cols] = (0.999 - rng.uniform(0.0, 1e-3, size=(R, m))).astype(np.float32)
    return torch.from_numpy(v).to(DEV)


def run_tiles(vals: torch.Tensor, scale: float, n_tiles: int, seed: int | None, unaligned: bool, k: int | None = None):
    """Fold the device matrix ``vals`` into fresh states as ``n_tiles`` column tiles, in shuffled order (``seed=None``: in order).
    ``unaligned``: views that start 4 bytes past a 16-byte boundary, with a row stride that is no multiple of 4 and NaN around them."""
    R, n = vals.shape
    sm = N.softmax_new(R, DEV)
    sv, si = N.topk_new(R, k, DEV) if k else (None, None)
    cuts = np.linspace(0, n, n_tiles + 1).astype(np.int64)
    order = np.arange(n_tiles) if seed is None else np.random.default_rng(seed).permutation(n_tiles)
    for t in order:
        a, b = int(cuts[t]), int(cuts[t + 1])
        if b == a:
            continue
        if unaligned:
            buf = torch.full((R, (b - a) + 3), float("nan"), dtype=torch.float32, device=DEV)
            buf[:, 1 : 1 + (b - a)] = vals[:, a:b]
            tile = buf[:, 1 : 1 + (b - a)]
            assert tile.data_ptr() % 16 == 4
        else:
            tile = vals[:, a:b].contiguous()
        if k:
            N.topk_merge(sv, si, tile, a)
        N.softmax_merge(sm, tile, scale)
    return sm, sv, si


def reference(vals: torch.Tensor, scale: float):
    """float64 torch on the same fp32 tile: ``(log_z, entropy, probs)``."""
    logits = float(scale) * vals.double()
    lz = torch.logsumexp(logits, dim=1)
    p = torch.softmax(logits, dim=1)
    ent = -(p * torch.where(p > 0, (logits - lz[:, None]), torch.zeros_like(p))).sum(1)
    return lz, ent, p


def edge() -> int:
    return 8 * cus()  # rows from which on a tile is never split (csrc/softmax.hip: splits)


SHAPES = [(1, 1), (3, 5), (3, 4099), (1, 70001), (3584, 301), (3584, 257),
          # the launcher's boundaries: a row is split over waves iff B >= 2048 and R < 8 * CUs
          (3, 2047), (3, 2048), ("edge-1", 2048), ("edge", 2048)]


@pytest.mark.parametrize("R,n", SHAPES)
def test_kernel_against_float64(R, n):
    R = edge() - 1 if R == "edge-1" else edge() if R == "edge" else R
    assert is_split(R, n) == (n >= 2048 and R < edge())
    vals = planted(R, n, seed=R + n)
    gap = float(vals.max() - vals.min())
    k = min(5, n)
    for scale in (1.0, 100.0, 1000.0):
        want_lz, want_h, want_p = reference(vals, scale)
        b_lz, b_p, b_h = softmax_bound(scale, gap, n)
        if scale <= 100:
            assert max(b_lz, b_p, b_h) <= TOL
        for n_tiles in (1, 7, 64):
            sm, sv, si = run_tiles(vals, scale, n_tiles, seed=n_tiles, unaligned=(n_tiles == 7), k=k)
            again, _, _ = run_tiles(vals, scale, n_tiles, seed=n_tiles, unaligned=(n_tiles == 7))
            assert torch.equal(sm.view(torch.int64), again.view(torch.int64)), "the same tiling twice is not bit-equal"
            assert (sm[:, 3] == n).all()
            probs, lz, h = N.softmax_finish(sm, scale, sv)
            assert not torch.isnan(lz).any() and not torch.isnan(h).any() and not torch.isnan(probs).any()  # the NaN padding never shows
            p_ref = torch.gather(want_p, 1, si)
            big = p_ref > 1e-30
            e_lz = float((lz - want_lz).abs().max())
            e_h = float((h - want_h).abs().max())
            e_p = float(((probs.double() - p_ref).abs() / p_ref)[big].max()) if big.any() else 0.0
            assert float(probs[~big].max() if (~big).any() else 0.0) <= 1e-29
            print(f"({R}, {n}) scale {scale:g} tiles {n_tiles}: log_z {e_lz:.2e} / {b_lz:.2e}, probs {e_p:.2e} / {b_p:.2e}, "
                  f"entropy {e_h:.2e} / {b_h:.2e}")
            assert e_lz <= b_lz + 4 * 2.0 ** -53 * float(want_lz.abs().max())  # the reference's own rounding of a sum near `scale`
            assert e_p <= b_p
            assert e_h <= b_h


# ---------------------------------------------------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3000, 3 * 4096])  # three tiles of 1000 (one wave per row) and of 4096 (split rows)
@pytest.mark.parametrize("where", [0, 1, 2])  # the tile the special value arrives in: first, middle, last
def test_special_values_follow_float64_torch(n, where):
    rng = np.random.default_rng(n + where)
    v = rng.uniform(-1.0, 1.0, size=(5, n)).astype(np.float32)
    spot = where * (n // 3) + int(rng.integers(0, n // 3))
    v[0, rng.random(n) < 0.5] = -np.inf  # {-inf, finite}
    v[0, spot] = -np.inf
    v[1, spot] = np.nan
    v[2, spot] = np.inf
    v[3, :] = -np.inf
    v[4, spot] = np.inf  # +inf and a NaN: the NaN wins
    v[4, (spot + n // 2) % n] = np.nan
    vals = torch.from_numpy(v).to(DEV)
    assert is_split(5, n // 3) == (n // 3 >= 2048)
    scale, k = 100.0, 4
    want_lz, want_h, want_p = reference(vals, scale)
    assert math.isinf(float(want_lz[2])) and torch.isnan(want_p[2]).all() and float(want_lz[3]) == -math.inf  # what torch does
    assert torch.isnan(want_lz[[1, 4]]).all() and torch.isnan(want_p[3]).all()
    b_lz, b_p, b_h = softmax_bound(scale, 2.0, n)
    for seed in (None, 1, 2):  # in order, and two shuffles
        sm, sv, si = run_tiles(vals, scale, 3, seed=seed, unaligned=(seed == 1), k=k)
        probs, lz, h = N.softmax_finish(sm, scale, sv)
        assert abs(float(lz[0] - want_lz[0])) <= b_lz and abs(float(h[0] - want_h[0])) <= b_h
        p0 = want_p[0][si[0]]
        assert float(((probs[0].double() - p0).abs() / p0).max()) <= b_p
        for r in (1, 4):
            assert math.isnan(float(lz[r])) and math.isnan(float(h[r])) and torch.isnan(probs[r]).all()
        assert float(lz[2]) == math.inf and math.isnan(float(h[2])) and torch.isnan(probs[2]).all()
        assert float(lz[3]) == -math.inf and math.isnan(float(h[3])) and torch.isnan(probs[3]).all()
        assert (sm[:, 3] == n).all()


def test_never_merged_state_and_empty_slots():
    sm = N.softmax_new(3, DEV)
    sv, _ = N.topk_new(3, 4, DEV)
    probs, lz, h = N.softmax_finish(sm, 100.0, sv)
    assert (lz == -math.inf).all() and torch.isnan(h).all() and (probs == 0).all()
    # all -inf candidates, fewer than k: the real candidates are NaN, the empty slots stay 0
    tile = torch.full((3, 2), -math.inf, dtype=torch.float32, device=DEV)
    si = torch.empty((3, 4), dtype=torch.int64, device=DEV)
    N.topk_init(sv, si)
    N.topk_merge(sv, si, tile, 0)
    N.softmax_merge(sm, tile, 100.0)
    probs, lz, h = N.softmax_finish(sm, 100.0, sv)
    assert (lz == -math.inf).all() and torch.isnan(h).all()
    assert torch.isnan(probs[:, :2]).all() and (probs[:, 2:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# finish and argument checks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,n,k", [(3, 5, 8), (70, 301, 5), (1, 1, 3)])
def test_finish_probs_empty_slots_and_null_values(R, n, k):
    scale = 100.0
    vals = planted(R, n, seed=n)
    sm, sv, si = run_tiles(vals, scale, 2 if n > 1 else 1, seed=0, unaligned=True, k=k)
    probs, lz, h = N.softmax_finish(sm, scale, sv)
    _, b_p, _ = softmax_bound(scale, 2.0, n)
    m = min(n, k)
    want = torch.exp(scale * sv[:, :m].double() - lz[:, None])
    big = want > 1e-30  # below that fp32 has no relative precision left (denormals)
    assert big[:, 0].all() and float(((probs[:, :m].double() - want).abs() / want)[big].max()) <= b_p
    assert float(probs[:, :m][~big].max() if (~big).any() else 0.0) <= 1e-29
    assert (probs[:, m:] == 0).all() and (si[:, m:] == -1).all()
    none, lz2, h2 = N.softmax_finish(sm, scale)  # d_vals = NULL: the statistics alone
    assert none is None and torch.equal(lz2, lz) and torch.equal(h2, h)
    assert probs.dtype == torch.float32 and lz.dtype == torch.float64 and h.dtype == torch.float64


def test_merge_refuses_bad_arguments():
    sm = N.softmax_new(2, DEV)
    tile = torch.zeros((2, 8), dtype=torch.float32, device=DEV)
    lib = N.lib()
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert lib.sl_softmax_merge(sm.data_ptr(), 2, tile.data_ptr(), 8, 8, bad, None, 0, None) == -1
        assert b"logit scale" in lib.sl_last_error()
    assert lib.sl_softmax_merge(sm.data_ptr(), 2, tile.data_ptr(), 4, 8, 1.0, None, 0, None) == -1  # ld < B
    assert lib.sl_softmax_merge(sm.data_ptr(), 2, tile.data_ptr(), 8, 0, 1.0, None, 0, None) == -1  # B < 1
    assert lib.sl_softmax_merge(sm.data_ptr(), 2, tile.data_ptr() + 2, 8, 4, 1.0, None, 0, None) == -1  # not 4-byte aligned
    assert lib.sl_softmax_merge(None, 0, None, 8, 8, 1.0, None, 0, None) == 0  # R == 0: a no-op
    with pytest.raises(ValueError):
        N.softmax_merge(sm, tile[:1], 1.0)
    torch.cuda.synchronize()
    assert torch.equal(sm.cpu(), torch.tensor([[-math.inf, 0.0, 0.0, 0.0]] * 2, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------
# API over the suite's fake text tower
# ---------------------------------------------------------------------------------------------------------------------
LETTERS = "abcdefghijklmnopqrstuvwxyz"
TEMPLATES = ["a photo of {}", "{} texture", "an image showing {}."]
SCALE = 10.0  # keeps logit_scale * TOL meaningful


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


def unit64(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)


_CASES = {}


def api_case(templates):
    """(fm, words, float64 cosines (C, V), db) for a (300, 16) DB and 2 000 words; computed once per template setting."""
    key = bool(templates)
    if key not in _CASES:
        fm = FakeVLM(dim=16, ctx=40)
        words = make_vocabulary(2000, seed=3)
        emb = word_embeddings64(fm, words, templates)
        db = np.random.default_rng(4).standard_normal((300, 16)).astype(np.float32)
        _CASES[key] = (words, unit64(db) @ unit64(emb).T, db)
    words, cos, db = _CASES[key]
    return FakeVLM(dim=16, ctx=40).to(DEV), words, cos, torch.from_numpy(db).to(DEV)


@pytest.mark.parametrize("templates", [None, TEMPLATES])
def test_label_distribution_chunking_and_float64(templates):
    k = 5
    fm, words, cos, db = api_case(templates)
    logits = torch.from_numpy(SCALE * cos)
    want_lz = torch.logsumexp(logits, 1)
    want_p = torch.softmax(logits, 1)
    want_h = -(want_p * (logits - want_lz[:, None])).sum(1)
    b_lz, b_p, b_h = softmax_bound(SCALE, 2.0, len(words))
    results = []
    for chunk_size in (None, 97, 2000):
        vals, ids = L.label_components(fm, words, db, k=k, templates=templates, chunk_size=chunk_size, batch_size=512)
        dist = L.label_distribution(fm, words, db, k=k, logit_scale=SCALE, templates=templates, chunk_size=chunk_size, batch_size=512)
        assert isinstance(dist, L.LabelDistribution) and dist.n_labels == len(words) and dist.logit_scale == SCALE
        assert torch.equal(dist.ids, ids) and torch.equal(dist.values.view(torch.int32), vals.view(torch.int32))
        assert dist.probs.dtype == torch.float32 and dist.log_z.dtype == torch.float64 and dist.entropy.dtype == torch.float64
        assert dist.probs.is_cuda and tuple(dist.probs.shape) == (300, k) and tuple(dist.log_z.shape) == (300,)
        results.append(dist)
        p_ref = torch.gather(want_p, 1, dist.ids.cpu())
        assert float((dist.log_z.cpu() - want_lz).abs().max()) <= SCALE * TOL + b_lz
        assert float(((dist.probs.cpu().double() - p_ref).abs() / p_ref).max()) <= SCALE * TOL + b_p
        assert float((dist.entropy.cpu() - want_h).abs().max()) <= SCALE * TOL + b_h
        assert torch.allclose(dist.effective_labels, dist.entropy.exp()) and dist.confident(0.0).all()
    first = results[0]
    for dist in results[1:]:  # the same cosines cut differently: within the kernel's bound of each other (both sides carry it)
        assert torch.equal(dist.ids, first.ids)
        assert float((dist.log_z - first.log_z).abs().max()) <= 2 * b_lz
        assert float(((dist.probs.double() - first.probs.double()).abs() / first.probs.double()).max()) <= 2 * b_p
        assert float((dist.entropy - first.entropy).abs().max()) <= 2 * b_h


def test_label_distribution_dict_equals_per_layer():
    fm, words, _, db = api_case(None)
    layers = {"a": db[:120], "b": db[120:]}
    both = L.Lens(fm, device=DEV).label_distribution(words, layers, k=3, logit_scale=SCALE, chunk_size=500)
    assert list(both) == ["a", "b"]
    for name, layer in layers.items():
        one = L.label_distribution(fm, words, layer, k=3, logit_scale=SCALE, chunk_size=500)
        for field in ("values", "ids", "probs", "log_z", "entropy"):
            assert torch.equal(getattr(both[name], field), getattr(one, field)), field


def test_nan_row_and_full_vocabulary_sum():
    fm, words, _, db = api_case(None)
    words = words[:1000]
    db = db[:40].clone()
    db[7, 3] = float("nan")
    dist = L.label_distribution(fm, words, db, k=len(words), logit_scale=SCALE, chunk_size=300)
    bad = torch.zeros(40, dtype=torch.bool, device=DEV)
    bad[7] = True
    assert torch.isnan(dist.probs[7]).all() and math.isnan(float(dist.log_z[7])) and math.isnan(float(dist.entropy[7]))
    assert not torch.isnan(dist.probs[~bad]).any() and not torch.isnan(dist.log_z[~bad]).any() and not torch.isnan(dist.entropy[~bad]).any()
    assert not dist.confident(0.0)[7] and dist.confident(0.0)[~bad].all()
    _, b_p, _ = softmax_bound(SCALE, 2.0, len(words))
    total = dist.probs[~bad].double().sum(1)
    assert float((total - 1.0).abs().max()) <= b_p  # every probability carries at most b_p relative, and they sum to 1
    # an all-zero row (an empty facet): cosine 0 to everything, a uniform distribution
    zero = torch.zeros((1, 16), dtype=torch.float32, device=DEV)
    uni = L.label_distribution(fm, words, zero, k=3, logit_scale=SCALE)
    _, u_p, u_h = softmax_bound(SCALE, 0.0, len(words))
    assert float((uni.entropy - math.log(len(words))).abs().max()) <= u_h
    assert float((uni.effective_labels - len(words)).abs().max()) <= len(words) * 2 * u_h
    assert float((uni.probs.double() * len(words) - 1.0).abs().max()) <= u_p


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_probe_softmax_both_gemm_modes(mode):
    C, V, D, k = 512, 4097, 512, 5
    rng = np.random.default_rng(C + D)
    rows = rng.standard_normal((C, D)).astype(np.float32)
    cols = rng.standard_normal((V, D)).astype(np.float32)
    cols[:C] = rows + 0.05 * rng.standard_normal((C, D)).astype(np.float32)
    x, y = torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV)
    N.set_gemm_mode(mode)
    try:
        vals, ids, probs, lz, h = L.probe_softmax(y, x, k, logit_scale=SCALE, chunk_rows=1001)
        tv, ti = L.probe_topk(y, x, k, chunk_rows=1001)
    finally:
        N.set_gemm_mode(None)
    assert torch.equal(ids, ti) and torch.equal(vals.view(torch.int32), tv.view(torch.int32))
    logits = torch.from_numpy(SCALE * (unit64(rows) @ unit64(cols).T))
    want_lz = torch.logsumexp(logits, 1)
    want_p = torch.softmax(logits, 1)
    want_h = -(want_p * (logits - want_lz[:, None])).sum(1)
    b_lz, b_p, b_h = softmax_bound(SCALE, 2.0, V)
    p_ref = torch.gather(want_p, 1, ids.cpu())
    assert float((lz.cpu() - want_lz).abs().max()) <= SCALE * TOL + b_lz
    assert float(((probs.cpu().double() - p_ref).abs() / p_ref).max()) <= SCALE * TOL + b_p
    assert float((h.cpu() - want_h).abs().max()) <= SCALE * TOL + b_h


def test_memory_at_full_size():
    """V = 65 536 against C = 8 192 (the full matrix would be 2 GiB): the rise of the allocator's peak over the call stays below
    tile + states + 64 MiB, the allowance K17's full-size test uses."""
    C, V, D, k = 8192, 65536, 512, 5
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn((C, D), generator=g, device=DEV)
    y = torch.randn((V, D), generator=g, device=DEV)
    chunk = N.topk_chunk_rows(C, V)
    bound = C * chunk * 4 + C * k * 12 + C * 32 + (64 << 20)  # the tile, both states, the slack
    L.probe_softmax(y[:256], x[:128], k)  # code objects loaded before the measured call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    vals, ids, probs, lz, h = L.probe_softmax(y, x, k)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB, full matrix {C * V * 4 / 2**20:.0f} MiB")
    assert rise < bound
    assert not torch.isnan(lz).any() and float((probs.double().sum(1)).max()) <= 1.0 + 1e-4
    assert float(h.min()) > 0 and float(h.max()) <= math.log(V) + 1e-9
