"""K23 on the device: ``sl_silhouette`` against scikit-learn's ``silhouette_samples`` (both metrics), its independence of m, of
the component chunking and of where the tensors live, the edge semantics, and ``polysemanticity_facets(n_clusters="auto")``:
the selection rule against scikit-learn's silhouettes of the device's own labels, its consistency with the fixed-k path, and
``label_facets`` / ``search_facets`` over the result.

Bound for silhouette values: 1e-6 absolute.  A float64 numpy restatement of the Gram-matrix distances is within 3.4e-8 of
scikit-learn on these shapes (worst: the duplicated rows, whose Gram difference is rounding where scikit-learn's is not zero),
the cosine metric within 3e-14; the remaining factor of 30 is for the kernel's summation order."""
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
TOL = 1e-6
METRICS = ("euclidean", "cosine")


def planted(seed, C, n, D, noise):  # component c has 1 + c % 5 planted directions
    rs = np.random.RandomState(seed)
    V = np.empty((C, n, D), np.float32)
    for c in range(C):
        kt = 1 + c % 5
        cen = rs.randn(kt, D)
        cen /= np.linalg.norm(cen, axis=1, keepdims=True)
        V[c] = cen[np.arange(n) % kt] + noise * rs.randn(n, D) / np.sqrt(D)
    return V


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def sk_samples(Vc: np.ndarray, labels: np.ndarray, metric: str) -> np.ndarray:
    """scikit-learn's silhouette_samples of one component in float64 over the samples with a label >= 0; NaN elsewhere."""
    from sklearn.metrics import silhouette_samples

    keep = labels >= 0
    out = np.full(labels.shape, np.nan)
    out[keep] = silhouette_samples(Vc[keep].astype(np.float64), labels[keep], metric=metric)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against scikit-learn
# ---------------------------------------------------------------------------------------------------------------------
# odd D, a D above one LDS stage of the Gram kernel, n on both sides of the 128 limit of the one-wave path, the n limit itself
KERNEL_SHAPES = [(6, 5, 3), (6, 20, 64), (6, 24, 513), (6, 67, 130), (6, 130, 48), (2, 1024, 16)]


@functools.lru_cache(maxsize=None)
def kernel_case(C, n, D):
    """Computed once per shape and left unchanged: V with one duplicated row, scikit-learn's k-means labels (3, C, n) for
    k = 2, 3, min(6, n - 1), and the expected samples per metric."""
    from sklearn.cluster import KMeans

    V = planted(C + 7 * n + 13 * D, C, n, D, 0.4)
    V[1, n - 1] = V[1, 0]  # one row copied over another
    ks = (2, 3, min(6, n - 1))
    labels = np.stack([[KMeans(k, n_init=10, random_state=123).fit(V[c].astype(np.float64)).labels_ for c in range(C)] for k in ks])
    labels = labels.astype(np.int32)
    want = {metric: np.stack([[sk_samples(V[c], labels[s, c], metric) for c in range(C)] for s in range(len(ks))]) for metric in METRICS}
    return V, ks, labels, want


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("C,n,D", KERNEL_SHAPES)
def test_kernel_against_sklearn(C, n, D, metric):
    V, ks, labels, want = kernel_case(C, n, D)
    Vd, ld = torch.from_numpy(V).to(DEV), torch.from_numpy(labels).to(DEV)
    samples, mean = N.silhouette(Vd, ld, max(ks), metric)  # one m = 3 call
    assert samples.is_cuda and mean.is_cuda and samples.dtype == torch.float64 and mean.dtype == torch.float64
    assert tuple(samples.shape) == (3, C, n) and tuple(mean.shape) == (3, C)
    err_s = np.abs(samples.cpu().numpy() - want[metric]).max()
    err_m = np.abs(mean.cpu().numpy() - want[metric].mean(-1)).max()
    print(f"K23 C={C} n={n} D={D} {metric}: max sample error {err_s:.2e}, max mean error {err_m:.2e}")
    assert err_s <= TOL and err_m <= TOL
    # the scores wrappers: any label in [0, 16) is a cluster
    assert torch.equal(bits(scores.silhouette_samples(Vd, ld, metric)), bits(samples))
    assert torch.equal(bits(scores.silhouette_score(Vd, ld, metric)), bits(mean))
    # ---- 2. independence of m: bit-equal to three m = 1 calls, in both label layouts ----
    for s in range(3):
        one_s, one_m = N.silhouette(Vd, ld[s], max(ks), metric)
        assert tuple(one_s.shape) == (C, n) and tuple(one_m.shape) == (C,)
        assert torch.equal(bits(one_s), bits(samples[s])) and torch.equal(bits(one_m), bits(mean[s]))
    none_s, only_m = N.silhouette(Vd, ld, max(ks), metric, samples=False)
    assert none_s is None and torch.equal(bits(only_m), bits(mean))


# ---------------------------------------------------------------------------------------------------------------------
# 2. independence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [12, 130])
def test_chunked_components_equal_one_launch(monkeypatch, n):
    rng = np.random.RandomState(5)
    C, D = 23, 16
    V = torch.from_numpy(rng.randn(C, n, D).astype(np.float32)).to(DEV)
    labels = torch.from_numpy(rng.randint(-1, 4, size=(3, C, n)).astype(np.int32)).to(DEV)
    monkeypatch.delenv("SL_POLY_WS_GB", raising=False)
    whole = N.silhouette(V, labels, 4, "euclidean")
    monkeypatch.setenv("SL_POLY_WS_GB", "1e-3")  # ~1 MB: 7 components per launch at n = 130
    monkeypatch.setattr(N, "POLYK_MAX_COMPONENTS", 7)
    chunked = N.silhouette(V, labels, 4, "euclidean")
    for a, b in zip(whole, chunked):
        assert a.shape == b.shape and torch.equal(bits(a), bits(b))  # bit-equal, NaN included
    assert torch.equal(bits(N.silhouette(V, labels[1], 4, "euclidean")[1]), bits(whole[1][1]))


def test_host_tensors_in_host_tensors_out():
    V, ks, labels, _ = kernel_case(6, 20, 64)
    Vh, lh = torch.from_numpy(V), torch.from_numpy(labels)
    s, m = scores.silhouette_samples(Vh, lh), scores.silhouette_score(Vh, lh, metric="cosine")
    assert not s.is_cuda and not m.is_cuda
    assert torch.equal(bits(s), bits(scores.silhouette_samples(Vh.to(DEV), lh.to(DEV)).cpu()))
    assert torch.equal(bits(m), bits(scores.silhouette_score(Vh.to(DEV), lh.to(DEV), metric="cosine").cpu()))
    f = scores.polysemanticity_facets(Vh, "auto")
    for name in ("score", "labels", "counts", "centers", "clarity", "n_facets", "silhouette"):
        assert not getattr(f, name).is_cuda, name


def test_no_components():
    V = torch.zeros(0, 12, 16, device=DEV)
    s, m = N.silhouette(V, torch.zeros(3, 0, 12, dtype=torch.int32, device=DEV), 4)
    assert tuple(s.shape) == (3, 0, 12) and tuple(m.shape) == (3, 0) and s.dtype == torch.float64 and m.dtype == torch.float64
    assert tuple(scores.silhouette_score(V, torch.zeros(0, 12, dtype=torch.int32, device=DEV)).shape) == (0,)
    f = scores.polysemanticity_facets(V, "auto", max_clusters=5)
    assert tuple(f.score.shape) == (0,) and tuple(f.labels.shape) == (0, 12) and tuple(f.counts.shape) == (0, 5)
    assert tuple(f.centers.shape) == (0, 5, 16) and tuple(f.clarity.shape) == (0, 5)
    assert tuple(f.n_facets.shape) == (0,) and f.n_facets.dtype == torch.int32
    assert tuple(f.silhouette.shape) == (0, 4) and f.silhouette.dtype == torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# 3. edge semantics
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [20, 130])
def test_edge_semantics(n, metric):
    C, D = 5, 32
    V = planted(3, C, n, D, 0.4)
    V[4] = V[4, :1]  # component 4: every row equal
    rng = np.random.RandomState(n)
    labels = rng.randint(0, 3, size=(C, n)).astype(np.int32)
    labels[0, 7] = 5                                  # component 0: a singleton cluster (ids need not be consecutive)
    labels[1, rng.rand(n) < 0.3] = -1                 # component 1: masked samples, both kinds of out-of-range label
    labels[1, 2] = 6
    labels[2] = 1                                     # component 2: one non-empty cluster ...
    labels[3] = np.where(np.arange(n) % 4 == 0, -1, 2)  # ... and one non-empty cluster beside masked samples
    samples, mean = N.silhouette(torch.from_numpy(V).to(DEV), torch.from_numpy(labels).to(DEV), 6, metric)
    samples, mean = samples.cpu().numpy(), mean.cpu().numpy()
    # a singleton cluster gives s = 0; the rest as scikit-learn
    assert samples[0, 7] == 0.0
    want0 = sk_samples(V[0], labels[0], metric)
    assert want0[7] == 0.0 and np.abs(samples[0] - want0).max() <= TOL and abs(mean[0] - want0.mean()) <= TOL
    # masked samples: scikit-learn on the remaining samples, NaN at the masked positions
    masked = labels[1].copy()
    masked[masked >= 6] = -1
    want1 = sk_samples(V[1], masked, metric)
    out = masked < 0
    assert out.sum() >= 2 and np.all(np.isnan(samples[1][out])) and not np.isnan(samples[1][~out]).any()
    assert np.abs(samples[1][~out] - want1[~out]).max() <= TOL and abs(mean[1] - want1[~out].mean()) <= TOL
    # fewer than two non-empty clusters: the silhouette is not defined
    assert np.isnan(mean[2]) and np.isnan(mean[3])
    assert np.all(np.isnan(samples[2])) and np.all(np.isnan(samples[3]))
    # every row equal: every distance is the same, s = 0 (euclidean: exactly, max(a, b) == 0; cosine: 1 - h / (sqrt h)^2 is one
    # rounding off zero for every pair alike)
    assert not np.isnan(samples[4]).any()
    if metric == "euclidean":
        assert np.all(samples[4] == 0.0) and mean[4] == 0.0
    else:
        assert np.abs(samples[4]).max() <= 1e-12 and abs(mean[4]) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 4. selection
# ---------------------------------------------------------------------------------------------------------------------
SEL = dict(C=60, n=24, D=64, max_clusters=6, min_silhouette=0.25)


@functools.lru_cache(maxsize=None)
def selection_input():
    return planted(23, SEL["C"], SEL["n"], SEL["D"], 0.4)


def select(sil: np.ndarray, min_silhouette: float):
    """The rule on a (C, K - 1) array of mean silhouettes: (n_facets, top-two gap, distance of the best to the threshold)."""
    key = np.where(np.isnan(sil), -np.inf, sil)
    best = key.argmax(1)  # the first maximum: ties go to the smaller k
    top = key.max(1)
    srt = np.sort(key, axis=1)
    n_facets = np.where(top >= min_silhouette, best + 2, 1)
    return n_facets, srt[:, -1] - srt[:, -2], np.abs(top - min_silhouette)


@functools.lru_cache(maxsize=None)
def device_fixed_k():
    """The fixed-k results the selection is made of, computed once: {k: Facets} for k = 2..6."""
    Vd = torch.from_numpy(selection_input()).to(DEV)
    return {k: scores.polysemanticity_facets(Vd, n_clusters=k) for k in range(2, SEL["max_clusters"] + 1)}


@functools.lru_cache(maxsize=None)
def device_auto(metric):
    Vd = torch.from_numpy(selection_input()).to(DEV)
    return scores.polysemanticity_facets(Vd, "auto", max_clusters=SEL["max_clusters"], metric=metric)


def sk_mean_silhouettes(labels_by_k: dict, metric: str) -> np.ndarray:
    from sklearn.metrics import silhouette_score

    V = selection_input().astype(np.float64)
    return np.stack([[silhouette_score(V[c], labels_by_k[k][c], metric=metric) for k in sorted(labels_by_k)] for c in range(len(V))])


@pytest.mark.parametrize("metric", METRICS)
def test_selection_against_sklearn_on_the_device_labels(metric):
    C = SEL["C"]
    f = device_auto(metric)
    assert f.n_facets.dtype == torch.int32 and tuple(f.n_facets.shape) == (C,)
    assert f.silhouette.dtype == torch.float64 and tuple(f.silhouette.shape) == (C, SEL["max_clusters"] - 1)
    labels_by_k = {k: g.labels.cpu().numpy() for k, g in device_fixed_k().items()}
    want = sk_mean_silhouettes(labels_by_k, metric)
    got = f.silhouette.cpu().numpy()
    print(f"K23 selection {metric}: max silhouette error {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= TOL
    want_facets, gap, margin = select(want, SEL["min_silhouette"])
    skip = (gap < 1e-4) | (margin < 1e-4)
    assert skip.sum() <= 3, f"{int(skip.sum())} of {C} components sit on a near-tie"
    n_facets = f.n_facets.cpu().numpy()
    assert np.array_equal(n_facets[~skip], want_facets[~skip])
    planted_count = 1 + np.arange(C) % 5
    hits = int((n_facets == planted_count).sum())
    print(f"K23 selection {metric}: planted count recovered for {hits} of {C}, smallest top-two gap {gap.min():.2e}, "
          f"smallest distance to the threshold {margin.min():.2e}")
    assert hits >= 58


def test_selection_cpu_reference_pipeline():
    """scikit-learn k-means plus silhouette on the same input: no near-tie to skip, the planted count for 60 of 60."""
    from sklearn.cluster import KMeans

    V = selection_input().astype(np.float64)
    labels_by_k = {k: np.stack([KMeans(k, n_init=10, random_state=123).fit(Vc).labels_ for Vc in V]) for k in range(2, 7)}
    for metric, min_gap in (("euclidean", 1.07e-3), ("cosine", 7.7e-4)):
        n_facets, gap, margin = select(sk_mean_silhouettes(labels_by_k, metric), SEL["min_silhouette"])
        assert not ((gap < 1e-4) | (margin < 1e-4)).any()
        assert gap.min() >= min_gap * 0.99 and margin.min() >= 0.15
        assert np.array_equal(n_facets, 1 + np.arange(SEL["C"]) % 5)


# ---------------------------------------------------------------------------------------------------------------------
# 5. consistency with the fixed-k path
# ---------------------------------------------------------------------------------------------------------------------
def assert_facet_rows(V: np.ndarray, rows: np.ndarray, centre: np.ndarray, clarity: float, tag):
    """The tolerances of test_gpu_facets.py::test_facet_stats_against_float64 for one facet given by its sample indices."""
    n = V.shape[0]
    want = V[rows].astype(np.float64).mean(0)
    assert np.abs(centre.astype(np.float64) - want).max() <= n * 2.0**-23 * np.abs(V).max(), tag
    if rows.size >= 2:
        assert abs(clarity - oracle.clarity(V[rows][None])[0]) <= 1e-5, tag
    else:
        assert np.isnan(clarity), tag


@pytest.mark.parametrize("metric", METRICS)
def test_auto_is_consistent_with_the_fixed_k_path(metric):
    V = selection_input()
    C, n, kc = SEL["C"], SEL["n"], SEL["max_clusters"]
    f = device_auto(metric)
    n_facets = f.n_facets.cpu().numpy()
    assert set(n_facets) == {1, 2, 3, 4, 5}  # every branch below is taken
    labels, counts = f.labels.cpu().numpy(), f.counts.cpu().numpy()
    centers, clarity, score = f.centers.cpu().numpy(), f.clarity.cpu().numpy(), f.score.cpu().numpy()
    assert tuple(counts.shape) == (C, kc) and tuple(centers.shape) == (C, kc, V.shape[2]) and tuple(clarity.shape) == (C, kc)
    assert f.n_clusters == kc and tuple(f.aggregated().shape) == (C * kc, V.shape[2])
    sil = f.silhouette.cpu().numpy()
    for k, g in device_fixed_k().items():
        assert g.n_facets is None and g.silhouette is None  # an integer n_clusters: the fields stay None
        mine = np.nonzero(n_facets == k)[0]
        idx = torch.from_numpy(mine).to(DEV)
        assert torch.equal(f.labels[idx], g.labels[idx])
        assert torch.equal(bits(f.score[idx]), bits(g.score[idx]))
        assert torch.equal(f.counts[idx][:, :k], g.counts[idx])
        for c in mine:
            for j in range(k):
                assert_facet_rows(V[c], np.nonzero(labels[c] == j)[0], centers[c, j], clarity[c, j], (c, j))
            assert np.all(counts[c, k:] == 0) and np.all(centers[c, k:] == 0.0) and np.all(np.isnan(clarity[c, k:]))
    single = np.nonzero(n_facets == 1)[0]
    want_clarity = scores.clarity_score(torch.from_numpy(V[single]).to(DEV)).cpu().numpy()
    for c, wc in zip(single, want_clarity):
        assert np.all(labels[c] == 0) and counts[c, 0] == n and np.all(counts[c, 1:] == 0) and score[c] == 0.0
        assert_facet_rows(V[c], np.arange(n), centers[c, 0], clarity[c, 0], (c, 0))
        assert abs(clarity[c, 0] - wc) <= 1e-5
        assert np.all(centers[c, 1:] == 0.0) and np.all(np.isnan(clarity[c, 1:]))
        assert not (np.nan_to_num(sil[c], nan=-np.inf) >= SEL["min_silhouette"]).any()


def test_auto_caps_the_candidates_at_n_minus_one():
    """n = 4: K = 3 candidates k = 2, 3; the columns of k = 4..6 stay NaN and the tensors keep max_clusters slots."""
    V = torch.from_numpy(planted(4, 7, 4, 8, 0.1)).to(DEV)
    f = scores.polysemanticity_facets(V, "auto", max_clusters=6)
    sil = f.silhouette.cpu().numpy()
    assert tuple(sil.shape) == (7, 5) and np.all(np.isnan(sil[:, 2:]))
    assert tuple(f.counts.shape) == (7, 6) and int(f.n_facets.max()) <= 3 and int(f.n_facets.min()) >= 1
    assert torch.equal(f.counts.sum(1), torch.full((7,), 4, dtype=torch.int64, device=DEV))
    lens_f = L.Lens(FakeVLM(dim=8).to(DEV), device=DEV).eval_facets({"a": V}, n_clusters="auto", max_clusters=6)["a"]
    assert torch.equal(lens_f.n_facets, f.n_facets) and torch.equal(lens_f.labels, f.labels)


# ---------------------------------------------------------------------------------------------------------------------
# 6. downstream
# ---------------------------------------------------------------------------------------------------------------------
def test_label_and_search_facets_on_auto_facets():
    dim = SEL["D"]
    fm = FakeVLM(dim=dim, ctx=40).to(DEV)
    f = device_auto("euclidean")
    C, kc = f.counts.shape
    used = f.counts > 0
    assert torch.equal(used.sum(1).to(torch.int32), f.n_facets)  # K9 left no chosen facet empty on this input
    words = ["cat", "dog", "stripes", "wheel", "grass", "sky", "water", "fur", "metal", "wood", "text", "face"]
    vals, ids = L.label_facets(fm, words, f, k=3)
    assert tuple(vals.shape) == (C, kc, 3)
    assert torch.all(vals[~used] == float("-inf")) and torch.all(ids[~used] == -1)
    want_vals, want_ids = L.label_components(fm, words, f.aggregated(), k=3)  # the same centre rows
    assert torch.equal(vals[used], want_vals.reshape(C, kc, 3)[used]) and torch.equal(ids[used], want_ids.reshape(C, kc, 3)[used])
    k = 40
    svals, layer_index, component, facet, names = L.search_facets(fm, words[:4], {"layer": f}, k=k)
    assert names == ["layer"] and tuple(svals.shape) == (4, k)
    found = component >= 0
    assert found.all()  # 180 facets in use, 40 asked for
    assert torch.all(facet[found] < f.n_facets.to(facet.device)[component[found]].to(facet.dtype))  # an unused facet is never found
    everything = L.search_facets(fm, words[:1], f, k=N.TOPK_MAX_K)
    n_used = int(used.sum())
    if N.TOPK_MAX_K >= n_used:  # every facet in use is found, then the slots are empty
        assert int((everything[2] >= 0).sum()) == n_used
