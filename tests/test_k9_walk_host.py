"""K9 host side (no GPU): the float64 walk of `kmeans_component` (tests/k9_walk.py) on every input family of
tests/test_gpu_k9_branches.py.  Per family: the walk's labels and min_count equal scikit-learn's for every component, and the
walk's census holds the branch the family was chosen for at least as often as `floor` states.  This pins the inputs: a change
of a seed, a shape or a generator that loses the branch fails here, before any kernel runs."""
from __future__ import annotations

import numpy as np
import pytest

import k9_walk as K


@pytest.mark.parametrize("name", list(K.FAMILIES))
def test_family_reaches_its_branches_and_the_walk_equals_sklearn(name):
    f = K.FAMILIES[name]
    k = f["k"]
    V, sk, _ = K.reference(name)
    lab, mc, cen, margins = K.census(V, k)
    differ = (lab != sk).any(axis=1)
    print(f"K9 walk {name}: shape {V.shape}, k = {k}: labels equal scikit-learn's on {int((~differ).sum())} of {len(V)}; "
          f"smallest margin {margins.min():.3g}; census {dict(sorted(cen.items()))}")
    for key, least in f["floor"].items():
        assert cen[key] >= least, (name, key, cen[key], "the family no longer reaches the branch it is there for")
    assert cen["stop_strict"] + cen["stop_tol"] + cen["stop_cap"] == 10 * len(V)
    if not f["asserted"]:
        return  # the duplicate family: labels are measured on the device, not asserted (docs/K9_BRANCHES.md)
    # a component may be left out only on a near-tie, at most 1 in 100 per family
    assert (margins[differ] < K.NEAR_TIE).all(), (name, "the walk differs from scikit-learn off a near-tie", np.nonzero(differ)[0][:10])
    assert int(differ.sum()) <= len(V) // 100, (name, int(differ.sum()))
    want_mc = np.array([np.bincount(l, minlength=k).min() for l in sk])
    assert np.array_equal(mc[~differ], want_mc[~differ])


def test_walk_on_a_hand_checked_component():
    """Two well separated pairs on a line: every run ends on unchanged labels with the pairs as clusters; the census counts
    ten runs, and cluster 0 is the cluster of the first seed."""
    X = np.array([[0.0], [1.0], [10.0], [11.0]], np.float32)
    lab, mc, cen = K.walk(X, 2)
    assert lab[0] == lab[1] != lab[2] == lab[3] and mc == 2
    assert cen["stop_strict"] == 10 and cen["stop_tol"] == 0 and cen["stop_cap"] == 0
    assert cen["seed_trial_0_wins"] + cen["seed_trial_1_wins"] == 10 and cen["fallback"] == 0
    assert np.array_equal(lab, K.sklearn_labels(X[None], 2)[0])
    # all points equal: one empty cluster, the early return, a stop at shift == 0 == tol, the fallback
    lab, mc, cen = K.walk(np.ones((5, 2), np.float32), 2)
    assert not lab.any() and mc == 0
    assert cen["reloc_1_empty"] == 10 and cen["reloc_early_return"] == 10 and cen["reloc_moves_a_point"] == 0
    assert cen["stop_tol"] == 10 and cen["stop_tol_positive"] == 0 and cen["closing_empty_cluster"] == 1 and cen["fallback"] == 1


def test_same_clustering_is_one_sided():
    """`same_clustering` of kmeans.hip: every label of the run maps to a single label of the best run, not the reverse."""
    assert K.same_clustering([0, 0, 1, 1], [1, 1, 0, 0], 2)
    assert K.same_clustering([0, 1, 2, 2], [0, 0, 1, 1], 3)      # a refinement maps to single labels
    assert not K.same_clustering([0, 0, 1, 1], [0, 1, 2, 2], 3)  # label 0 would map to two


def test_relocating_run_alone_equals_sklearn():
    """Of an island component's ten runs the one whose relocation moves a point is never the chosen one, so the ten-run result
    shows the relocation only through that run's inertia.  The run alone (n_init = 1, its own draws) against scikit-learn's
    Lloyd from the same seed points: the labels are equal, and the relocation did move a point."""
    V, _, _ = K.reference("islands_14_k3")
    for X in V:
        draws, seeds = K.relocating_run(X, 3)
        lab, _, cen = K.walk(X, 3, draws=draws)
        assert cen["reloc_moves_a_point"] == 1 and cen["chosen_run_relocated"] == 1 and cen["min_margin"] > K.NEAR_TIE
        assert np.array_equal(lab, K.sklearn_from_seeds(X, seeds)[0])
