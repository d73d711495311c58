"""K9 on the host: a float64 numpy walk of `kmeans_component` (semanticlens_amd/csrc/kmeans.hip) in Gram space that counts the
branches it takes, the input families chosen for those branches, and their scikit-learn reference.  A helper, not a test:
tests/test_k9_walk_host.py pins the census of every family without a GPU, tests/test_gpu_k9_branches.py runs the kernels
on the same inputs, docs/K9_BRANCHES.md is the table.

The walk follows the kernel step by step (centring and tol, k-means++ with the draws of `scores.kmeans_draws`, Lloyd with the
E-step, `relocate_empty`, `subset_stats`, the shift and both stop rules, the final E-step, best of n_init with
`same_clustering`, `min_count`); only the order of additions inside a sum is numpy's.  Census keys:

  stop_strict / stop_tol / stop_cap      how a Lloyd run ended (labels unchanged / shift <= tol / 300 iterations)
  stop_tol_positive                      ... by shift <= tol with tol > 0 and shift > 0
  tol_final_estep_changes_labels         the E-step after a run that did not end strictly changed a label
  chosen_label_ne_member                 the chosen run's labels differ from the member sets its centres come from
  best_better_but_same                   a run with a smaller inertia was not taken: `same_clustering`
  seed_trial_<t>_wins                    candidate t of a k-means++ step had the smallest potential
  seed_clamp                             a candidate index of n was clamped to n - 1
  reloc_<1|2|3plus>_empty                `relocate_empty` entered with that many empty clusters
  reloc_early_return / reloc_moves_a_point   ... and returned at far == 0 / moved points
  chosen_run_relocated                   the chosen run is one in which a relocation moved a point
  closing_empty_cluster, fallback        the chosen member sets leave a cluster empty; min_count < 2
  iters_max                              the longest Lloyd run (a maximum, not a count)
  min_margin                             the smallest relative margin of a decision, by the rule of
                                         tools/k9_postmortem.py:near_tie (a minimum, not a count)
"""
from __future__ import annotations

import warnings
from collections import Counter
from functools import lru_cache

import numpy as np

from semanticlens_amd.scores import kmeans_draws

NEAR_TIE = 1e-12  # the project's near-tie rule (tools/k9_postmortem.py): below it a decision may fall either way


def walk(X, k, n_init=10, random_state=123, draws=None, runs=None):
    """(labels (n,), min_count, Counter) of `kmeans_component` on one component X (n, D).  `draws`: (first, rand) in place of
    `kmeans_draws(n, n_init, random_state, k)`; `runs`: a list that receives (seeds, a relocation moved a point) per run."""
    X = np.asarray(X, np.float64)
    n, D = X.shape
    cen, margin = Counter(), [np.inf]

    def note(kind, m):
        if np.isfinite(m) and not (kind == "best" and m == 0.0):
            margin[0] = min(margin[0], abs(float(m)))

    # centre_gram
    H = X @ X.T
    r = H.sum(1) / n
    mu = r.sum() / n
    G = H - r[:, None] - r[None, :] + mu
    gd = np.diag(G).copy()
    tol = (np.diag(H) - 2.0 * r + mu).sum() / (n * D) * 1e-4
    first, rand = kmeans_draws(n, n_init, random_state, k) if draws is None else draws
    idx = np.arange(n)

    def dist_to(cc):
        return np.maximum(gd + gd[cc] - 2.0 * G[:, cc], 0.0)

    def dpart(s, cnt, W):  # (k, n): squared distance to every centre without the G_ii term; an empty cluster is never nearest
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(cnt[:, None] > 0, W[:, None] - 2.0 * s / cnt[:, None], np.inf)

    def estep(s, cnt, W):
        dp = dpart(s, cnt, W)
        if k > 1:
            two = np.partition(dp + gd[None, :], 1, axis=0)[:2]
            ok = np.isfinite(two[1])
            if ok.any():
                note("assign", ((two[1][ok] - two[0][ok]) / np.maximum(two[1][ok], 1e-300)).min())
        return dp.argmin(0), dp

    def subset_stats(member):
        M = np.zeros((n, k))
        M[idx, member] = 1.0
        so = (G @ M).T
        c = M.sum(0)
        t = (so * M.T).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            return so, c, np.where(c > 0, t / (c * c), 0.0)

    best = None
    for init in range(len(first)):
        # _kmeans_plusplus
        seed = [int(first[init])]
        closest = dist_to(seed[0])
        pot = closest.sum()
        for cc in range(1, k):
            v = rand[init, cc - 1] * pot
            cs = np.cumsum(closest)
            cand = np.searchsorted(cs, v, side="left")
            cen["seed_clamp"] += int((cand >= n).sum())
            cand = np.minimum(cand, n - 1)
            mn = np.minimum(closest[None, :], np.stack([dist_to(int(c)) for c in cand]))
            pots = mn.sum(1)
            b = int(np.argmin(pots))
            cen[f"seed_trial_{b}_wins"] += 1
            if pot > 0:
                note("search", np.abs(cs[None, :] - v[:, None]).min() / pot)
                others = pots[cand != cand[b]]
                if others.size:
                    note("cand", (others.min() - pots[b]) / max(pots[b], 1e-300))
            seed.append(int(cand[b]))
            closest, pot = mn[b], pots[b]
        # _kmeans_single_lloyd
        cnt, W, s = np.ones(k), gd[seed].copy(), G[seed, :].copy()
        label_old = np.full(n, -1)
        strict, stop, moved = False, "stop_cap", False
        for it in range(300):
            label, dp = estep(s, cnt, W)
            member = label.copy()
            count = np.bincount(label, minlength=k)
            empty = np.nonzero(count == 0)[0]
            if empty.size:  # relocate_empty
                cen["reloc_%s_empty" % (empty.size if empty.size < 3 else "3plus")] += 1
                dist = gd + dp[label, idx]
                if max(dist.max(), 0.0) > 0.0:
                    cen["reloc_moves_a_point"] += 1
                    moved = True
                    for j in empty:
                        far = int(np.argmax(dist))
                        member[far] = j
                        dist[far] = -np.inf
                else:
                    cen["reloc_early_return"] += 1
            sn, ncnt, nW = subset_stats(member)
            M = np.zeros((k, n))
            M[member, idx] = 1.0
            x = (s * M).sum(1)
            both = (cnt > 0) & (ncnt > 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                shift = np.where(both, W + nW - 2.0 * x / (cnt * ncnt), 0.0).sum()
            s, cnt, W = sn, ncnt, nW
            if np.array_equal(label, label_old):
                strict, stop = True, "stop_strict"
                break
            if shift <= tol:
                stop = "stop_tol"
                cen["stop_tol_positive"] += int(tol > 0 and shift > 0)
                break
            label_old = label
        cen[stop] += 1
        if runs is not None:
            runs.append((tuple(seed), moved))
        cen["iters_max"] = max(cen["iters_max"], it + 1)
        if not strict:
            new, dp = estep(s, cnt, W)
            cen["tol_final_estep_changes_labels"] += int(not np.array_equal(new, label))
            label = new
        else:
            dp = dpart(s, cnt, W)
        inertia = (gd + dp[label, idx]).sum()
        # best of n_init
        take = best is None
        if best is not None:
            note("best", (inertia - best[0]) / best[0] if best[0] else np.inf)
            if inertia < best[0]:
                take = not same_clustering(label, best[1], k)
                cen["best_better_but_same"] += int(not take)
        if take:
            best = (inertia, label, member, moved)
    _, label, member, moved = best
    cen["chosen_run_relocated"] += int(moved)
    cen["chosen_label_ne_member"] += int(not np.array_equal(label, member))
    cen["closing_empty_cluster"] += int((np.bincount(member, minlength=k) == 0).any())
    min_count = int(np.bincount(label, minlength=k).min())
    cen["fallback"] += int(min_count < 2)
    cen["min_margin"] = margin[0]
    return label.astype(np.int32), min_count, cen


def same_clustering(a, b, k):
    """`same_clustering` of kmeans.hip (_is_same_clustering): every label of `a` maps to a single label of `b`."""
    m = np.full(k, -1)
    for x, y in zip(a, b):
        if m[x] == -1:
            m[x] = y
        elif m[x] != y:
            return False
    return True


def census(V, k):
    """The walk over every component of V (C, n, D): labels (C, n), min_count (C,), the summed census (iters_max: the maximum,
    min_margin: per component, as an array)."""
    labels, mcs, total, margins, iters = [], [], Counter(), [], 0
    for X in V:
        lab, mc, cen = walk(X, k)
        labels.append(lab)
        mcs.append(mc)
        margins.append(cen.pop("min_margin"))
        iters = max(iters, cen.pop("iters_max"))
        total.update(cen)
    total["iters_max"] = iters
    return np.stack(labels), np.asarray(mcs), total, np.asarray(margins)


def sklearn_fit(V, k):
    """KMeans(k, n_init=10, random_state=123) on every component in float64: `labels_` (C, n) int32 and 1 - clarity of
    `cluster_centers_` in float64 (C,), which is what polysemanticity_score returns without the fallback (scores.py:168-172).
    The centres are those of the last M-step, not the means of `labels_`: the two differ after a stop by tolerance."""
    from sklearn.cluster import KMeans

    lab, raw = np.empty(V.shape[:2], np.int32), np.empty(len(V))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # ConvergenceWarning: fewer distinct points than clusters, on purpose
        for c, X in enumerate(V):
            fit = KMeans(n_clusters=k, n_init=10, random_state=123).fit(X.astype(np.float64))
            lab[c] = fit.labels_
            cn = fit.cluster_centers_ / np.maximum(np.linalg.norm(fit.cluster_centers_, axis=-1, keepdims=True), 1e-12)
            raw[c] = 1.0 - ((cn.mean(0) ** 2).sum() - 1.0 / k) / (k - 1) * k
    return lab, raw


def sklearn_labels(V, k):
    return sklearn_fit(V, k)[0]


# ---- the input families ---------------------------------------------------------------------------------------------------------
# name -> generator (`make`), seed, shape (C, n, D), k, and `floor`: census key -> the least count the family's walk must hold
# (tests/test_k9_walk_host.py).  The floors are the host's measurements (docs/K9_BRANCHES.md) rounded down: a seed that loses
# the branch fails there.  `asserted` False: labels are measured on the device, not asserted.
FAMILIES: dict[str, dict] = {}


def _family(name, gen, seed, shape, k, floor, hi=None, asserted=True, pick=None):
    FAMILIES[name] = dict(gen=gen, seed=seed, shape=shape, k=k, hi=hi, floor=floor, asserted=asserted, pick=pick)


def _wins(least, trials):
    return {f"seed_trial_{t}_wins": least for t in range(trials)}


# uniform, n at and near the workspace variant's limit: stops by tolerance, a final E-step that changes labels, a chosen run
# whose labels are not its member sets, a better run that is the same clustering, long runs, three and four seeding trials
_family("uniform_1024_k2", "uniform", 0, (6, 1024, 2), 2,
        {"stop_tol_positive": 50, "tol_final_estep_changes_labels": 35, "chosen_label_ne_member": 3, "best_better_but_same": 2})
_family("uniform_1024_k5", "uniform", 0, (4, 1024, 3), 5,
        {"stop_tol_positive": 15, "tol_final_estep_changes_labels": 8, "chosen_label_ne_member": 1, "iters_max": 34, **_wins(40, 3)})
_family("uniform_1024_k16", "uniform", 0, (4, 1024, 8), 16, {"iters_max": 34, **_wins(100, 4)})
_family("uniform_300_k16", "uniform", 0, (4, 300, 2), 16, _wins(100, 4))
_family("uniform_512_k8", "uniform", 0, (4, 512, 2), 8, {"iters_max": 34, **_wins(50, 4)})
# the LDS variant's edges: one wave and one past it, the two n whose LDS state is above 64 KiB, the workspace variant's first n
for _n in (64, 65, 127, 128, 129):
    _family(f"lds_edge_{_n}", "uniform", _n, (6, _n, 2), 2, {"stop_strict": 50, **_wins(15, 2)})
# heavy tails: the variance, and so tol, is the outliers'; runs stop by tol > 0 in the LDS variant
_family("cauchy_12", "cauchy", 0, (200, 12, 1), 2, {"stop_tol_positive": 60, "fallback": 100})
_family("cauchy_40", "cauchy", 0, (200, 40, 1), 2, {"stop_tol_positive": 120, "fallback": 100})
_family("cauchy_128", "cauchy", 0, (100, 128, 1), 2, {"stop_tol_positive": 100, "fallback": 50})
# the LDS variant with a chosen run whose labels are not its member sets: the first three seeds, found among 60 000
_family("student_t_128", "student_t", None, (16, 128, 1), 2,
        {"chosen_label_ne_member": 3, "tol_final_estep_changes_labels": 3, "best_better_but_same": 5},
        pick=(14217, 15559, 39452) + tuple(range(13)))
# integers, n a power of two (means and sums over copies are exact on both sides), fewer distinct points than clusters
_family("int_8_k6", "int", 0, (150, 8, 2), 6, hi=2, floor={"reloc_2_empty": 500, "reloc_3plus_empty": 500, "reloc_early_return": 1500,
                                                        "closing_empty_cluster": 150, "fallback": 150})
_family("int_16_k5", "int", 0, (150, 16, 1), 5, hi=4, floor={"reloc_1_empty": 1000, "reloc_2_empty": 50, "reloc_early_return": 1500,
                                                         "closing_empty_cluster": 150, "fallback": 150})
_family("int_32_k12", "int", 0, (100, 32, 2), 12, hi=3, floor={"reloc_3plus_empty": 1000, "reloc_early_return": 1000,
                                                           "seed_trial_3_wins": 300, "closing_empty_cluster": 100})
_family("int_64_k16", "int", 0, (60, 64, 3), 16, hi=2, floor={"reloc_3plus_empty": 600, "reloc_early_return": 600,
                                                          "seed_trial_3_wins": 200, "closing_empty_cluster": 60})
# a relocation that moves a point (`_islands_stream`): the first 24 of the 34 such components among the stream's 200 000
ISLANDS = (4484, 10434, 10638, 10754, 14526, 52981, 66494, 68911, 76720, 78660, 87010, 91517, 97581, 103689, 113889, 122518, 131902,
           134183, 134960, 135001, 137066, 142942, 146390, 151282)
_family("islands_14_k3", "picked", 7, (len(ISLANDS), 14, 1), 3, {"reloc_moves_a_point": 24, "reloc_1_empty": 24, "fallback": 24},
        pick=ISLANDS)
# copies of 3, 5, 6 and 7, n no power of two (`_dupes`)
_family("dupes_21_k8", "dupes", 0, (100, 21, 2), 8, {"reloc_3plus_empty": 1000, "reloc_early_return": 1000, "fallback": 100},
        asserted=False)


def make(name):
    """The family's input V (C, n, D) float32."""
    f = FAMILIES[name]
    rng = np.random.RandomState(f["seed"])
    if f["gen"] == "uniform":
        return rng.rand(*f["shape"]).astype(np.float32)
    if f["gen"] == "cauchy":
        return rng.standard_cauchy(f["shape"]).astype(np.float32)
    if f["gen"] == "int":
        return rng.randint(0, f["hi"], size=f["shape"]).astype(np.float32)
    if f["gen"] == "dupes":
        return _dupes(rng, *f["shape"], f["k"])
    if f["gen"] == "student_t":  # one seed per component: the components were found one by one (docs/K9_BRANCHES.md)
        C, n, D = f["shape"]
        assert len(f["pick"]) == C
        return np.stack([np.random.RandomState(c).standard_t(3, (n, D)) for c in f["pick"]]).astype(np.float32)
    if f["gen"] == "picked":  # components picked out of a seeded stream: the branch is too rare to meet by seed alone
        V = _islands_stream(rng, *f["shape"][1:])[np.asarray(f["pick"])]
        assert V.shape == f["shape"]
        return V
    raise KeyError(f["gen"])


STREAM = 200_000  # components in the stream that the `picked` family indexes


def _islands_stream(rng, n, D):
    """1-D, for k = 3: a lone point at -a, c copies of -b, a lone point at 0, a lone point at p, c copies of p + b', a lone
    point at p + e (n = 2 c + 4), jittered by 0.03, in random order.  When the three lone points -a, 0, p + e are the seeds, the
    middle cluster is {0, p} with its centre at p / 2, the outer centres move onto the copies, 0 and p both leave for them and
    the middle cluster is empty in the second iteration with every point off its centre: `relocate_empty` moves a point.
    Few orders seed it so under the fixed draws (about 1 in 8 000); `pick` lists them."""
    assert D == 1 and n % 2 == 0 and n > 4
    c = (n - 4) // 2
    a, b, p, b2, e = (rng.uniform(lo, hi, size=STREAM) for lo, hi in ((2.2, 4), (1.2, 1.9), (3.5, 4.5), (1.2, 1.9), (4, 6)))
    pts = np.concatenate([-a[:, None], np.repeat(-b[:, None], c, 1), 0 * a[:, None], p[:, None], np.repeat((p + b2)[:, None], c, 1),
                          (p + e)[:, None]], axis=1)
    pts = pts + 0.03 * rng.randn(STREAM, n)
    order = np.argsort(rng.rand(STREAM, n), axis=1)
    return np.take_along_axis(pts, order, axis=1).astype(np.float32)[:, :, None]


def _dupes(rng, C, n, D, k):
    """Fewer distinct integer points than clusters, in copies of 3, 5, 6 and 7, n no power of two, the copies shuffled: the mean
    of c copies of a centred, inexact value rounds.  The kernel still sees exact zeros (two copies have bit-equal Gram rows), returns
    early from the relocation and stops after one iteration; scikit-learn counts an empty cluster's parked centre in its shift,
    runs a second iteration and relocates copies on distances of about 1e-32 (docs/K9_BRANCHES.md)."""
    mult = np.array([3, 5, 6, 7])
    assert n == mult.sum() and n & (n - 1) and len(mult) < k
    V = np.empty((C, n, D), np.float32)
    for c in range(C):
        while True:
            pts = rng.randint(0, 5, size=(len(mult), D))
            if len({tuple(p) for p in pts}) == len(mult):
                break
        V[c] = np.repeat(pts, rng.permutation(mult), axis=0)[rng.permutation(n)]
    return V


@lru_cache(maxsize=None)
def reference(name):
    """(V, scikit-learn's labels, its score without the fallback) of a family, computed once per process and shared: the
    arrays are read-only."""
    V = make(name)
    lab, raw = sklearn_fit(V, FAMILIES[name]["k"])
    for a in (V, lab, raw):
        a.setflags(write=False)
    return V, lab, raw


def relocating_run(X, k):
    """(draws of that run alone, its seeds) for the first of the ten runs on X in which a relocation moves a point."""
    runs = []
    walk(X, k, runs=runs)
    init = next(i for i, (_, moved) in enumerate(runs) if moved)
    first, rand = kmeans_draws(len(X), 10, 123, k)
    return (first[init:init + 1].copy(), rand[init:init + 1].copy()), runs[init][0]


def sklearn_from_seeds(X, seeds):
    """scikit-learn's Lloyd run from the given seed points alone (KMeans(init=X[seeds], n_init=1)): `labels_` and 1 - clarity
    of `cluster_centers_`."""
    from sklearn.cluster import KMeans

    X = np.asarray(X, np.float64)
    k = len(seeds)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fit = KMeans(n_clusters=k, init=X[list(seeds)].copy(), n_init=1).fit(X)
    cn = fit.cluster_centers_ / np.maximum(np.linalg.norm(fit.cluster_centers_, axis=-1, keepdims=True), 1e-12)
    return fit.labels_.astype(np.int32), 1.0 - ((cn.mean(0) ** 2).sum() - 1.0 / k) / (k - 1) * k
