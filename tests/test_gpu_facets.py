"""K21 on the device: per-facet statistics against numpy float64, the exported labels against scikit-learn itself, degenerate
input, chunking, and the describe / search API over facets.

Bounds: counts and labels are exact.  A facet centre is an fp32 sum of at most n terms and one division, so
``|got - want| <= n * 2**-23 * max|V[c]|`` elementwise (derived, not measured).  Clarity: the project's K7 tolerance (1e-5,
tests/test_gpu_parity.py) against ``oracle.clarity`` of the facet's rows."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import oracle
from helpers import FakeVLM
from semanticlens_amd import _native as N
from semanticlens_amd import lens as L
from semanticlens_amd import scores

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4  # the project's bound for cosine values (tests/test_gpu_topk.py)


# ---------------------------------------------------------------------------------------------------------------------
# references in numpy float64
# ---------------------------------------------------------------------------------------------------------------------
def stats64(V: np.ndarray, labels: np.ndarray, kc: int):
    """counts (C, kc), centres (C, kc, D) in float64, clarity (C, kc) through ``oracle.clarity`` (NaN below two rows)."""
    C, n, D = V.shape
    V64 = V.astype(np.float64)
    counts = np.zeros((C, kc), dtype=np.int64)
    centres = np.zeros((C, kc, D), dtype=np.float64)
    clarity = np.full((C, kc), np.nan, dtype=np.float64)
    for j in range(kc):
        mask = labels == j
        counts[:, j] = mask.sum(1)
        centres[:, j] = (V64 * mask[..., None]).sum(1) / np.maximum(counts[:, j], 1)[:, None]
        for c in np.nonzero(counts[:, j] >= 2)[0]:
            clarity[c, j] = oracle.clarity(V[c][mask[c]][None])[0]
    return counts, centres, clarity


def assert_stats(V: np.ndarray, labels: np.ndarray, kc: int, centres, counts, clarity, tag=""):
    """The contract of ``sl_facet_stats`` for device results against ``stats64``."""
    C, n, D = V.shape
    want_counts, want_centres, want_clarity = stats64(V, labels, kc)
    counts, centres, clarity = counts.cpu().numpy(), centres.cpu().numpy(), clarity.cpu().numpy()
    assert counts.dtype == np.int32 and centres.dtype == np.float32 and clarity.dtype == np.float32
    assert counts.shape == (C, kc) and centres.shape == (C, kc, D) and clarity.shape == (C, kc)
    assert np.array_equal(counts, want_counts), tag
    bound = n * 2.0**-23 * np.abs(V).reshape(C, -1).max(1).astype(np.float64)
    err = np.abs(centres.astype(np.float64) - want_centres).reshape(C, -1).max(1)
    live = np.isfinite(want_clarity)
    cerr = np.abs(clarity[live] - want_clarity[live]).max() if live.any() else 0.0
    print(f"K21 {tag}: max centre error / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}, max clarity error {cerr:.2e}, "
          f"{int((want_counts == 0).sum())} empty and {int((want_counts == 1).sum())} singleton facets")
    assert np.all(err <= bound), (tag, np.nonzero(err > bound)[0][:10])
    assert np.array_equal(np.isnan(clarity), want_counts < 2), tag  # NaN exactly where a facet has fewer than two rows
    assert cerr <= 1e-5, tag
    assert np.all(centres[want_counts == 0] == 0.0), tag


# ---------------------------------------------------------------------------------------------------------------------
# (a) sl_facet_stats with made-up labels
# ---------------------------------------------------------------------------------------------------------------------
# (C, n, D, kc).  D: 4 and 256 are one 16-byte piece per lane (256 its last width), 260 two, 1152 five (the row kernel for
# kc = 2, the column kernel for kc = 3), 7 and 30 are no multiple of four and 2052 is past the row kernel: the column kernel.
# C = 5000 is more than the grid (8 workgroups per CU): the grid-stride loop of both kernels.
STATS_CASES = [
    (1, 2, 4, 2), (5000, 2, 4, 2), (5000, 2, 7, 3), (37, 3, 4, 3), (37, 3, 7, 2), (37, 5, 256, 16), (37, 5, 30, 2), (1, 5, 30, 16),
    (37, 33, 256, 2), (37, 33, 260, 3), (37, 33, 260, 2), (37, 33, 7, 3), (300, 33, 256, 1), (37, 100, 1152, 2),
    (37, 100, 1152, 3), (37, 100, 2052, 2), (1, 100, 2052, 3), (300, 33, 30, 3), (37, 100, 260, 16),
]


def stats_case(C, n, D, kc):
    rng = np.random.RandomState(C + 7 * n + 13 * D + 17 * kc)
    V = rng.randn(C, n, D).astype(np.float32)
    labels = rng.randint(-1, kc + 1, size=(C, n)).astype(np.int32)  # -1 and kc: both kinds of out-of-range label
    if C >= 4:
        labels[0][labels[0] == kc - 1] = -1                     # a cluster forced empty
        labels[1][labels[1] == 0] = kc                          # a cluster forced to a single row
        labels[1][n - 1] = 0
        V[2] = 0.0                                              # F.normalize's epsilon path
        V[3] *= np.logspace(-3, 3, n, dtype=np.float32)[:, None]  # per-row scales 1e-3 .. 1e3
    return V, labels


@pytest.mark.parametrize("C,n,D,kc", STATS_CASES)
def test_facet_stats_against_float64(C, n, D, kc):
    V, labels = stats_case(C, n, D, kc)
    Vd, ld = torch.from_numpy(V).to(DEV), torch.from_numpy(labels).to(DEV)
    centres, counts, clarity = N.facet_stats(Vd, ld, kc)
    assert centres.is_cuda and counts.is_cuda and clarity.is_cuda
    assert_stats(V, labels, kc, centres, counts, clarity, f"C={C} n={n} D={D} kc={kc}")
    again = N.facet_stats(Vd, ld, kc)
    for a, b in zip((centres, counts, clarity), again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # bit-equal, NaN included
    no_clarity = N.facet_stats(Vd, ld, kc, clarity=False)
    assert no_clarity[2] is None
    assert torch.equal(no_clarity[0], centres) and torch.equal(no_clarity[1], counts)


def test_facet_stats_unaligned_slab_takes_the_general_path():
    """A slab that does not start on 16 bytes cannot be read in 16-byte pieces: same contract."""
    V, labels = stats_case(37, 33, 256, 2)
    flat = torch.empty(V.size + 1, dtype=torch.float32, device=DEV)
    Vd = flat[1:].view(V.shape)
    Vd.copy_(torch.from_numpy(V))
    assert Vd.data_ptr() % 16 == 4 and Vd.is_contiguous()
    centres, counts, clarity = N.facet_stats(Vd, torch.from_numpy(labels).to(DEV), 2)
    assert_stats(V, labels, 2, centres, counts, clarity, "unaligned")


# ---------------------------------------------------------------------------------------------------------------------
# (b) labels against scikit-learn
# ---------------------------------------------------------------------------------------------------------------------
def poly_input(C, n, D, k, kind):
    """The generators of tests/test_gpu_parity.py's scikit-learn comparisons."""
    rng = np.random.RandomState(C + n + D + k)
    V = rng.randn(C, n, D).astype(np.float32)
    if kind == "blobs":
        cen = rng.randn(C, k, D).astype(np.float32) * 2
        V = cen[np.arange(C)[:, None], rng.randint(0, k, size=(C, n))] + 0.4 * V
    elif kind == "weak":  # barely separated blobs: many competing local optima across the 10 inits
        cen = rng.randn(C, 2, D).astype(np.float32) * 0.15
        V = cen[np.arange(C)[:, None], rng.randint(0, 2, size=(C, n))] + V
    elif kind == "dup":
        V[:, n // 2:] = V[:, : n - n // 2]
        V[:, :3] = V[:, :1]
    return V


@functools.lru_cache(maxsize=None)
def sklearn_fit(C, n, D, k, kind):
    """Computed once per case and left unchanged: (V, labels_ (C, n), cluster_centers_ (C, k, D) float64)."""
    from sklearn.cluster import KMeans

    V = poly_input(C, n, D, k, kind)
    fits = [KMeans(n_clusters=k, n_init=10, random_state=123).fit(e.astype(np.float64)) for e in V]
    return V, np.stack([f.labels_ for f in fits]).astype(np.int32), np.stack([f.cluster_centers_ for f in fits])


SKLEARN_CASES = [(64, 20, 512, 2, "random"), (64, 20, 512, 2, "blobs"), (64, 20, 512, 2, "weak"), (48, 33, 100, 3, "blobs"),
                 (32, 150, 32, 2, "blobs"), (48, 12, 16, 5, "random"), (16, 200, 24, 3, "random")]


@pytest.mark.parametrize("C,n,D,k,kind", SKLEARN_CASES)
def test_labels_against_sklearn(C, n, D, k, kind):
    V, want_labels, want_centres = sklearn_fit(C, n, D, k, kind)
    # what the comparison rests on: scikit-learn's centres ARE the means by its labels, and no facet is empty
    by_labels = np.stack([[V[c].astype(np.float64)[want_labels[c] == j].mean(0) for j in range(k)] for c in range(C)])
    assert np.abs(by_labels - want_centres).max() <= 1e-14 * max(1.0, np.abs(want_centres).max())
    Vd = torch.from_numpy(V).to(DEV)
    f = scores.polysemanticity_facets(Vd, n_clusters=k)
    assert f.labels.dtype == torch.int32 and f.score.dtype == torch.float64 and f.labels.is_cuda
    got = f.labels.cpu().numpy()
    bad = np.nonzero((got != want_labels).any(1))[0]
    assert bad.size == 0, ("labels_ differ from scikit-learn's for components", bad[:10])
    want_counts = np.stack([np.bincount(row, minlength=k) for row in want_labels])
    assert np.array_equal(f.counts.cpu().numpy(), want_counts)
    bound = n * 2.0**-23 * np.abs(V).reshape(C, -1).max(1).astype(np.float64)
    err = np.abs(f.centers.cpu().numpy().astype(np.float64) - want_centres).reshape(C, -1).max(1)
    print(f"K21 {kind} k={k}: max centre error / bound {np.max(err / bound):.3f}, {int((want_counts == 1).sum())} singleton facets")
    assert np.all(err <= bound)
    assert_stats(V, want_labels, k, f.centers, f.counts, f.clarity, f"{kind} k={k}")
    for replace in (True, False):
        score = scores.polysemanticity_score(Vd, n_clusters=k, replace_empty_clusters=replace)
        ff = f if replace else scores.polysemanticity_facets(Vd, n_clusters=k, replace_empty_clusters=False)
        assert torch.equal(ff.score, score)
        assert torch.equal(ff.labels, f.labels)


# ---------------------------------------------------------------------------------------------------------------------
# (c) degenerate input
# ---------------------------------------------------------------------------------------------------------------------
def check_self_consistent(V: np.ndarray, f: scores.Facets, k: int, tag: str):
    C, n, D = V.shape
    labels = f.labels.cpu().numpy()
    assert labels.min() >= 0 and labels.max() < k
    assert np.array_equal(f.counts.cpu().numpy(), np.stack([np.bincount(row, minlength=k) for row in labels]))
    assert_stats(V, labels, k, f.centers, f.counts, f.clarity, tag)


def test_duplicated_points_are_self_consistent():
    """Equal points make scikit-learn's labels a matter of tie order: no comparison with it.  Every component has an empty facet
    and a singleton facet there; whatever labels come back, the other fields must be the statistics of THOSE labels."""
    C, n, D, k = 48, 8, 4, 6
    V = poly_input(C, n, D, k, "dup")
    Vd = torch.from_numpy(V).to(DEV)
    for replace in (True, False):
        f = scores.polysemanticity_facets(Vd, n_clusters=k, replace_empty_clusters=replace)
        check_self_consistent(V, f, k, f"dup replace={replace}")
        assert torch.equal(f.score, scores.polysemanticity_score(Vd, n_clusters=k, replace_empty_clusters=replace))
        counts = f.counts.cpu().numpy()
        assert (counts == 0).any(), "the input was built to leave facets empty"
        assert np.all(f.centers.cpu().numpy()[counts == 0] == 0.0)
        assert np.all(np.isnan(f.clarity.cpu().numpy()[counts < 2]))


# ---------------------------------------------------------------------------------------------------------------------
# (d) chunking
# ---------------------------------------------------------------------------------------------------------------------
FIELDS = ("score", "labels", "counts", "centers", "clarity")


def assert_facets_bit_equal(a: scores.Facets, b: scores.Facets):
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape, name
        as_int = torch.int64 if x.element_size() == 8 else torch.int32
        assert torch.equal(x.view(as_int), y.view(as_int)), name  # bit-equal, NaN included


@pytest.mark.parametrize("k", [2, 3])
def test_chunked_components_equal_one_launch(monkeypatch, k):
    rng = np.random.RandomState(5)
    V = torch.from_numpy(rng.randn(150, 12, 16).astype(np.float32)).to(DEV)
    V[:20, 1:] = V[:20, :1]  # all-duplicate components: empty facets in the chunks too
    monkeypatch.delenv("SL_POLY_WS_GB", raising=False)
    whole = scores.polysemanticity_facets(V, n_clusters=k)
    monkeypatch.setenv("SL_POLY_WS_GB", "1e-4")  # ~100 KB: a handful of components per launch
    monkeypatch.setattr(N, "POLYK_MAX_COMPONENTS", 7)
    assert_facets_bit_equal(scores.polysemanticity_facets(V, n_clusters=k), whole)


@pytest.mark.parametrize("k", [2, 3])
def test_no_components(k):
    f = scores.polysemanticity_facets(torch.zeros(0, 12, 16, device=DEV), n_clusters=k)
    assert tuple(f.score.shape) == (0,) and f.score.dtype == torch.float64
    assert tuple(f.labels.shape) == (0, 12) and f.labels.dtype == torch.int32
    assert tuple(f.counts.shape) == (0, k) and f.counts.dtype == torch.int32
    assert tuple(f.centers.shape) == (0, k, 16) and f.centers.dtype == torch.float32
    assert tuple(f.clarity.shape) == (0, k) and f.clarity.dtype == torch.float32
    assert tuple(f.aggregated().shape) == (0, 16)


def test_host_tensors_in_host_tensors_out():
    V = torch.from_numpy(poly_input(8, 20, 32, 2, "blobs"))
    f = scores.polysemanticity_facets(V)
    assert all(not getattr(f, name).is_cuda for name in FIELDS)
    assert_facets_bit_equal(f, scores.Facets(*(getattr(scores.polysemanticity_facets(V.to(DEV)), name).cpu() for name in FIELDS)))
    with pytest.raises(ValueError):  # scikit-learn: n_samples should be >= n_clusters
        scores.polysemanticity_facets(V[:, :2].to(DEV), n_clusters=3)


# ---------------------------------------------------------------------------------------------------------------------
# (e) API
# ---------------------------------------------------------------------------------------------------------------------
LETTERS = "abcdefghijklmnopqrstuvwxyz"


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


def test_eval_facets_on_a_dict_keeps_the_key_order():
    fm = FakeVLM(dim=16).to(DEV)
    db = {"z": torch.from_numpy(poly_input(6, 20, 16, 2, "blobs")).to(DEV), "a": torch.from_numpy(poly_input(4, 20, 16, 3, "blobs")).to(DEV)}
    lens = L.Lens(fm, device=DEV)
    out = lens.eval_facets(db, n_clusters=3)
    assert list(out) == ["z", "a"]
    for name, V in db.items():
        assert isinstance(out[name], scores.Facets) and out[name].n_clusters == 3
        assert_facets_bit_equal(out[name], scores.polysemanticity_facets(V, n_clusters=3))
    single = lens.eval_facets(db["z"])
    assert isinstance(single, scores.Facets) and single.n_clusters == 2


def test_label_facets_is_label_components_on_aggregated():
    """Exactly ``label_components`` on ``aggregated()``, reshaped, except the ``-inf`` / ``-1`` slots of empty facets (built through
    the duplicated-points input)."""
    k = 3
    fm = FakeVLM(dim=4, ctx=40).to(DEV)
    words = make_vocabulary(60, 3)
    f = scores.polysemanticity_facets(torch.from_numpy(poly_input(48, 8, 4, 6, "dup")).to(DEV), n_clusters=6)
    g = scores.polysemanticity_facets(torch.from_numpy(poly_input(10, 20, 4, 2, "blobs")).to(DEV), n_clusters=2)
    empty = f.counts == 0
    assert empty.any() and not (g.counts == 0).any()
    vals, ids = L.label_facets(fm, words, f, k=k)
    assert tuple(vals.shape) == (48, 6, k) and tuple(ids.shape) == (48, 6, k)
    assert vals.dtype == torch.float32 and ids.dtype == torch.int64 and vals.is_cuda
    want_vals, want_ids = L.label_components(fm, words, f.aggregated(), k=k)
    want_vals, want_ids = want_vals.reshape(48, 6, k), want_ids.reshape(48, 6, k)
    assert torch.equal(vals[~empty], want_vals[~empty]) and torch.equal(ids[~empty], want_ids[~empty])
    assert torch.all(vals[empty] == float("-inf")) and torch.all(ids[empty] == -1)
    both = L.Lens(fm, device=DEV).label_facets(words, {"f": f, "g": g}, k=k, chunk_size=25)
    assert list(both) == ["f", "g"]
    assert torch.equal(both["f"][1], ids)
    gv, gi = L.label_components(fm, words, g.aggregated(), k=k, chunk_size=25)
    assert torch.equal(both["g"][0], gv.reshape(10, 2, k)) and torch.equal(both["g"][1], gi.reshape(10, 2, k))


def test_facets_end_to_end_labels_and_search():
    """Component c's 20 samples are 10 noisy copies of word a_c's text embedding and 10 of word b_c's: its two facets are
    labelled {a_c, b_c}, and searching for a_c finds that component and that facet first."""
    C, n, dim = 12, 20, 64
    cpu = FakeVLM(dim=dim, ctx=40)
    words = make_vocabulary(200, 11)
    emb = cpu.encode_text(cpu.tokenize(words)).numpy().astype(np.float64)
    rng = np.random.default_rng(12)
    picks = rng.choice(len(words), size=2 * C, replace=False).reshape(C, 2)
    which = np.stack([rng.permutation(np.repeat([0, 1], n // 2)) for _ in range(C)])  # (C, n): a_c or b_c, interleaved
    V = emb[picks[np.arange(C)[:, None], which]] + 0.02 * np.abs(emb).mean() * rng.standard_normal((C, n, dim))
    V = V.astype(np.float32)
    # precondition, in float64: every facet centre's best and second-best vocabulary cosines differ by more than 4 * TOL
    unit = emb / np.linalg.norm(emb, axis=1, keepdims=True)
    for c in range(C):
        for side in (0, 1):
            centre = V[c][which[c] == side].astype(np.float64).mean(0)
            cos = np.sort(unit @ (centre / np.linalg.norm(centre)))[::-1]
            assert cos[0] - cos[1] > 4 * TOL, f"construction: top-2 gap {cos[0] - cos[1]:.3e} is not above 4 * TOL"
            assert np.argmax(unit @ centre) == picks[c, side]
    fm = FakeVLM(dim=dim, ctx=40).to(DEV)
    lens = L.Lens(fm, device=DEV)
    facets = lens.eval_facets({"layer": torch.from_numpy(V).to(DEV)})
    f = facets["layer"]
    labels = f.labels.cpu().numpy()
    for c in range(C):  # the clustering separates the two words (either numbering)
        assert np.array_equal(labels[c], which[c]) or np.array_equal(labels[c], 1 - which[c])
    vals, ids = lens.label_facets(words, facets, k=2)["layer"]
    top1 = ids[:, :, 0].cpu().numpy()
    for c in range(C):
        assert set(top1[c]) == set(picks[c]), (c, top1[c], picks[c])
    queries = [words[i] for i in picks[:, 0]]
    svals, layer_index, component, facet, names = lens.search_facets(queries, facets, k=3)
    assert names == ["layer"] and tuple(svals.shape) == (C, 3)
    assert torch.all(layer_index[:, 0] == 0)
    assert component[:, 0].cpu().tolist() == list(range(C))
    want_facet = [int(np.nonzero(top1[c] == picks[c, 0])[0][0]) for c in range(C)]
    assert facet[:, 0].cpu().tolist() == want_facet
    # the facet's reference samples: the README's last line
    for c in range(C):
        members = np.nonzero(f.members(want_facet[c])[c].cpu().numpy())[0]
        assert np.array_equal(members, np.nonzero(which[c] == 0)[0])
