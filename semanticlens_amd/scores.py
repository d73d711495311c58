"""Concept-quality scores (reference: semanticlens/scores.py:18-185) on HIP kernels.

Same names, arguments and shape conventions as the reference — including the shape-dependent
branches of ``similarity_score`` (scores.py:119-128).  Inputs may live on the host or the
device; results come back on the input's device, as with the reference.  There is no CPU
implementation behind these functions: without a HIP device they raise.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass

import numpy as np
import torch

from semanticlens_amd import _native as N

logger = logging.getLogger(__name__)


@torch.inference_mode()
def clarity_score(V):
    """Mean off-diagonal cosine among each component's samples.  V (..., n_samples, D) -> (...).

    Reference: scores.py:18-47 — ``((mean_j normalize(v_j))**2).sum(-1) - 1/n) / (n-1) * n``.  Kernel K7.
    """
    return N.clarity(V).to(V.device)


@torch.inference_mode()
def redundancy_score(cones):
    """Mean over components of the max cosine to any *other* component.  (..., C, D) -> (...).

    Reference: scores.py:50-81 (diagonal removed by ``- 2 * eye``).  Kernel K8 = K6's MFMA GEMM + row max.
    """
    return N.redundancy(cones).to(cones.device)


@torch.inference_mode()
def similarity_score(x, y):
    """Cosine similarity with the reference's shape branches (scores.py:84-128):

    * ``x.shape == y.shape``        -> row-wise cosine, shape ``(n,)``
    * ``x.shape[1] == y.shape[0]``  -> ``normalize(x) @ normalize(y)`` (no transpose)
    * ``x.shape[1] == y.shape[1]``  -> ``normalize(x) @ normalize(y).T``  (the probing GEMM, K6)
    * otherwise ``ValueError("x and y must have the same shape")``
    """
    return N.similarity(x, y).to(x.device)


def kmeans_draws(n_samples: int, n_init: int, random_state: int, n_clusters: int = 2):
    """The random draws scikit-learn's ``KMeans(n_clusters, n_init, random_state)`` consumes, per init.

    ``KMeans.fit`` seeds one ``RandomState(random_state)`` and, for each of the ``n_init`` k-means++ seedings, draws
    ``choice(n_samples, p=uniform)`` for the first centre and, for every further centre,
    ``uniform(size=2 + int(log(n_clusters)))`` for its candidates (sklearn/cluster/_kmeans.py ``_kmeans_plusplus``).
    None of it depends on the data, so the host produces the draws and the device kernel consumes them.
    Returns ``first (n_init,) int32`` and ``rand (n_init, n_clusters - 1, trials) float64``.
    """
    rs = np.random.RandomState(random_state)
    weights = np.ones(n_samples, dtype=np.float64)  # KMeans' sample_weight takes X's dtype: float64 (see oracle)
    p = weights / weights.sum()
    trials = 2 + int(np.log(n_clusters))
    first = np.empty(n_init, dtype=np.int32)
    rand = np.empty((n_init, max(n_clusters - 1, 1), trials), dtype=np.float64)
    for i in range(n_init):
        first[i] = rs.choice(n_samples, p=p)
        for c in range(n_clusters - 1):
            rand[i, c] = rs.uniform(size=trials)
    return first, rand


@torch.inference_mode()
def polysemanticity_score(V, replace_empty_clusters=True, random_state=123, n_clusters=2):
    """``1 - clarity_score(centres)`` of a k-means clustering of each component's samples (``n_clusters`` = 2 by default:
    ``1 - cos(centre_1, centre_2)``).

    Reference: scores.py:131-185 (scikit-learn ``KMeans(n_clusters, n_init=10, random_state=123)`` per component in a
    Python loop).  Kernel K9 restates that procedure per component on the device for ``n_clusters`` up to 16 and up to
    1024 samples per component; rows whose smallest cluster has fewer than 2 samples use the reference's fallback.
    ``n_samples < n_clusters`` raises ``ValueError`` as scikit-learn does.
    """
    first, rand = kmeans_draws(V.shape[-2], 10, random_state, n_clusters)
    return N.poly2means(V, first, rand, replace_empty_clusters, n_clusters=n_clusters).to(V.device)


@dataclass
class Facets:
    """What ``polysemanticity_facets`` returns: the clustering each component's polysemanticity score comes from, split into
    its ``kc = n_clusters`` facets.  Every tensor lives on the input's device.

    * ``score (C,)`` float64: bit-equal to ``polysemanticity_score`` with the same arguments.
    * ``labels (C, n)`` int32: scikit-learn's ``labels_`` (reference scores.py:167), aligned with the sample axis of
      ``concept_db[layer]`` and so with ``ActMax.sample_ids``; facet ``j`` is the ``j``-th seeded centre.
    * ``counts (C, kc)`` int32: facet sizes.
    * ``centers (C, kc, D)`` float32: the mean embedding of a facet's samples — what ``concept_db.mean(1)`` is for the whole
      component, and what the reference reads as ``cluster_centers_`` (scores.py:168).  Zeros for an empty facet.
    * ``clarity (C, kc)`` float32: ``clarity_score`` within the facet; NaN for fewer than two samples.

    With ``n_clusters="auto"`` (kernel K23) every component has its own number of facets, ``kc = max_clusters`` is the fixed
    width of the tensors above and the facets a component does not use are empty (count 0, zero centre, NaN clarity), which
    ``label_facets`` and ``search_facets`` skip.  Two more fields, ``None`` after a fixed-``n_clusters`` call:

    * ``n_facets (C,)`` int32: the chosen facet count, 1 for a component without substantial cluster structure; ``score`` is
      the polysemanticity at that count, 0.0 where it is 1.
    * ``silhouette (C, max_clusters - 1)`` float64: column ``k - 2`` is the mean silhouette of the ``k``-facet clustering;
      NaN for a ``k`` that was not tried (``k >= n``) or whose clustering has fewer than two non-empty clusters."""

    score: torch.Tensor
    labels: torch.Tensor
    counts: torch.Tensor
    centers: torch.Tensor
    clarity: torch.Tensor
    n_facets: torch.Tensor | None = None
    silhouette: torch.Tensor | None = None

    @property
    def n_clusters(self) -> int:
        return int(self.centers.shape[1])

    def aggregated(self) -> torch.Tensor:
        """``(C * kc, D)``: row ``c * kc + j`` is facet ``j`` of component ``c`` — an aggregated concept DB of facets."""
        return self.centers.reshape(-1, self.centers.shape[-1])

    def members(self, j: int) -> torch.Tensor:
        """``(C, n)`` bool: the samples of facet ``j``."""
        if not 0 <= j < self.n_clusters:
            raise IndexError(f"facet {j} not in [0, {self.n_clusters})")
        return self.labels == j

    def decode(self, rows: torch.Tensor):
        """Rows of ``aggregated()`` -> ``(component, facet)`` = ``(row // kc, row % kc)``; a negative row (an empty slot) gives
        ``(-1, -1)``."""
        kc = self.n_clusters
        empty = rows < 0
        return (torch.div(rows, kc, rounding_mode="floor").masked_fill(empty, -1), (rows % kc).masked_fill(empty, -1))


@dataclass
class RedundancyGroups:
    """What ``redundancy_groups`` returns: which components of a layer duplicate each other.  A group is a connected component of
    the graph "cosine >= threshold" over the layer's aggregated concept DB — the quantity ``redundancy_score`` averages, kept
    per pair.  Every tensor lives on the DB's device.

    * ``labels (C,)`` int64: the SMALLEST component id of the component's group; a singleton labels itself.
    * ``degree (C,)`` int32: how many OTHER components have a cosine at or above the threshold to this one.
    * ``cohesion (C,)`` float32 or ``None``: the smallest pairwise cosine inside the component's group, NaN for a singleton.
      Connected components chain — two members of one group may be far below the threshold to each other — and this is where
      it shows; it costs a second pass over the cosine tiles, so it is computed only on request."""

    labels: torch.Tensor
    degree: torch.Tensor
    cohesion: torch.Tensor | None = None

    @property
    def redundant(self) -> torch.Tensor:
        """``(C,)`` bool: the component has at least one near-duplicate."""
        return self.degree > 0

    @property
    def sizes(self) -> torch.Tensor:
        """``(C,)`` int64: the size of each component's group."""
        return torch.bincount(self.labels, minlength=self.labels.shape[0])[self.labels]

    @property
    def n_groups(self) -> int:
        """How many distinct concepts the layer holds at this threshold."""
        return int((self.labels == torch.arange(self.labels.shape[0], device=self.labels.device)).sum())

    def members(self, i: int) -> torch.Tensor:
        """The ids of the group of component ``i``, ascending."""
        return torch.nonzero(self.labels == self.labels[i]).flatten()

    def representatives(self, by: str = "degree") -> torch.Tensor:
        """One id per group, ascending by label.  ``by="degree"``: the member of largest degree (ties: the smaller id), the
        component closest to the most others; ``by="label"``: the label itself."""
        if by not in ("degree", "label"):
            raise ValueError(f"by={by!r}: \"degree\" or \"label\"")
        C = self.labels.shape[0]
        ids = torch.arange(C, device=self.labels.device)
        roots = ids[self.labels == ids]
        if by == "label":
            return roots
        key = self.degree.to(torch.int64) * C + (C - 1 - ids)  # larger degree first, then the smaller id
        best = torch.zeros(C, dtype=torch.int64, device=self.labels.device).scatter_reduce(0, self.labels, key, "amax")
        return C - 1 - best[roots] % C

    def prune(self, db: torch.Tensor) -> torch.Tensor:
        """``db[representatives()]``: one row per group."""
        return db[self.representatives().to(db.device)]


@torch.inference_mode()
def redundancy_groups(cones, threshold=0.9, cohesion=False, chunk_rows=None, chunk_cols=None) -> RedundancyGroups:
    """Which components ``redundancy_score`` (reference scores.py:51-81) counts as duplicates of each other: the groups of the
    ``(C, D)`` aggregated concept DB ``cones`` under "cosine >= threshold" (``RedundancyGroups``).  A NaN cosine is never an
    edge (a component with a NaN or infinite coordinate is a singleton of degree 0), a zero row has cosine 0 to everything, a
    tie at exactly ``threshold`` is an edge, the diagonal is not.  Deterministic: no ``k``, no random start.

    Kernel K24 folds each tile of the cosine GEMM's upper triangle into a union-find forest and the degrees
    (``_native.redundancy_probe``); the ``(C, C)`` matrix never exists.  ``cohesion=True`` adds a second pass."""
    threshold = N.check_threshold(threshold)
    if cones.ndim != 2:
        raise ValueError("redundancy_groups expects a (n_components, n_features) tensor")
    labels, degree, coh = N.redundancy_probe(cones, threshold, chunk_rows, chunk_cols, cohesion)
    return RedundancyGroups(labels.to(cones.device), degree.to(cones.device), None if coh is None else coh.to(cones.device))


@torch.inference_mode()
def silhouette_samples(V, labels, metric="euclidean"):
    """scikit-learn's ``silhouette_samples`` for every component: ``V (C, n, D)``, ``labels (C, n)`` or ``(m, C, n)`` int32 ->
    float64 shaped like ``labels``.  Labels are cluster ids in ``[0, 16)``; any other value (``-1``) takes the sample out: its
    value is NaN and it enters nobody's distances.  Fewer than two non-empty clusters give NaN.  Kernel K23."""
    return N.silhouette(V, labels, N.SIL_MAX_CLUSTERS, metric)[0].to(V.device)


@torch.inference_mode()
def silhouette_score(V, labels, metric="euclidean"):
    """scikit-learn's ``silhouette_score`` for every component: the mean of ``silhouette_samples`` over the samples that are in,
    float64 ``(C,)`` or ``(m, C)``; NaN where fewer than two clusters are non-empty.  Kernel K23."""
    return N.silhouette(V, labels, N.SIL_MAX_CLUSTERS, metric, samples=False)[1].to(V.device)


@torch.inference_mode()
def polysemanticity_facets(V, n_clusters=2, random_state=123, replace_empty_clusters=True, max_clusters=6, min_silhouette=0.25,
                           metric="euclidean") -> Facets:
    """``polysemanticity_score`` together with the clustering it scores: per component the ``n_clusters`` facets' labels,
    sizes, mean embeddings and clarity (``Facets``).

    Kernel K9 exports the ``labels_`` of the scikit-learn run it replays (reference scores.py:167-168); kernel K21 reduces
    every facet's raw and normalised rows in one read of ``V``.  Same limits and ``ValueError``s as
    ``polysemanticity_score``.

    ``n_clusters="auto"`` chooses every component's facet count: the ``k`` in ``2..min(max_clusters, n - 1)`` whose clustering
    has the largest mean silhouette (kernel K23, ``metric`` "euclidean" or "cosine"; ties go to the smaller ``k``) if that
    silhouette reaches ``min_silhouette``, otherwise one facet (0.25 is Kaufman and Rousseeuw's "no substantial structure"
    line).  The tensors then have ``max_clusters`` facet slots, see ``Facets``.  ``max_clusters``, ``min_silhouette`` and
    ``metric`` are read only then."""
    if V.ndim != 3:
        raise ValueError("polysemanticity_facets expects a (n_components, n_samples, n_features) tensor")
    if isinstance(n_clusters, str):
        if n_clusters != "auto":
            raise ValueError(f"n_clusters={n_clusters!r}: an integer or \"auto\"")
        return _facets_auto(V, max_clusters, min_silhouette, metric, random_state, replace_empty_clusters)
    if n_clusters < 2:
        raise ValueError(f"n_clusters={n_clusters} must be at least 2")
    if n_clusters > N.POLYK_MAX_CLUSTERS:
        raise ValueError(f"n_clusters={n_clusters} exceeds the device kernel's maximum of {N.POLYK_MAX_CLUSTERS}")
    first, rand = kmeans_draws(V.shape[-2], 10, random_state, n_clusters)
    Vd = N._f32c(V)
    C, n, D = Vd.shape
    dev = Vd.device
    labels = torch.empty((C, n), dtype=torch.int32, device=dev)
    centers = torch.empty((C, n_clusters, D), dtype=torch.float32, device=dev)
    counts = torch.empty((C, n_clusters), dtype=torch.int32, device=dev)
    clarity = torch.empty((C, n_clusters), dtype=torch.float32, device=dev)
    score = N.poly2means(Vd, first, rand, replace_empty_clusters, n_clusters=n_clusters, labels=labels,
                         stats=(centers, counts, clarity))
    return Facets(*(t.to(V.device) for t in (score, labels, counts, centers, clarity)))


def _facets_auto(V, max_clusters, min_silhouette, metric, random_state, replace_empty_clusters) -> Facets:
    """``polysemanticity_facets(V, "auto")``: K9 once per candidate ``k``, one K23 call over the stacked labels, the selection in
    torch on the device, one K21 call at ``kc = max_clusters``."""
    n = V.shape[1]
    if isinstance(max_clusters, bool) or not isinstance(max_clusters, int) or not 2 <= max_clusters <= N.SIL_MAX_CLUSTERS:
        raise ValueError(f"max_clusters={max_clusters!r} not in [2, {N.SIL_MAX_CLUSTERS}]")
    if n < 3:
        raise ValueError(f"n_samples={n}: choosing a facet count needs at least 3 samples per component (candidates k = 2..n - 1)")
    N.check_silhouette_metric(metric)
    K = min(max_clusters, n - 1)
    Vd = N._f32c(V)
    C, n, D = Vd.shape
    dev = Vd.device
    labels = torch.empty((K - 1, C, n), dtype=torch.int32, device=dev)
    score = torch.empty((K - 1, C), dtype=torch.float64, device=dev)
    for k in range(2, K + 1):
        first, rand = kmeans_draws(n, 10, random_state, k)
        score[k - 2] = N.poly2means(Vd, first, rand, replace_empty_clusters, n_clusters=k, labels=labels[k - 2])
    sil = N.silhouette(Vd, labels, K, metric, samples=False)[1]  # (K - 1, C)
    key = sil.masked_fill(sil.isnan(), float("-inf"))
    top = key.max(0).values
    ks = torch.arange(K - 1, device=dev)[:, None]
    best = torch.where(key == top, ks, K - 1).min(0).values  # the smallest k among the best
    single = ~(top >= min_silhouette)
    n_facets = (best + 2).masked_fill(single, 1).to(torch.int32)
    chosen = labels.gather(0, best[None, :, None].expand(1, C, n))[0].masked_fill(single[:, None], 0)
    chosen_score = score.gather(0, best[None])[0].masked_fill(single, 0.0)
    centers, counts, clarity = N.facet_stats(Vd, chosen, max_clusters)
    silhouette = torch.full((C, max_clusters - 1), float("nan"), dtype=torch.float64, device=dev)
    silhouette[:, :K - 1] = sil.T
    return Facets(*(t.to(V.device) for t in (chosen_score, chosen, counts, centers, clarity, n_facets, silhouette)))
