"""K9 (csrc/kmeans.hip) against scikit-learn on inputs chosen for the branches they reach.

tests/k9_walk.py holds the input families and a float64 walk of `kmeans_component` that counts branches;
tests/test_k9_walk_host.py pins, without a GPU, that each family still reaches the branch it is there for and that the walk
picks scikit-learn's clustering on it.  Here the kernels run on the same inputs: labels equal scikit-learn's `labels_`
exactly, scores within the bounds of tests/test_gpu_parity.py (1e-9 where the score comes from the centres, 1e-6 on fallback
rows; the reference is `oracle.polysemanticity`), `min_count` equals the smallest label count, with `replace_empty_clusters`
True and False, and at k = 2 and n <= 128 in both storage variants, whose labels and `min_count` are bit-equal.
docs/K9_BRANCHES.md is the table of branches, families and tests."""
import warnings
from functools import lru_cache

import numpy as np
import pytest
import torch

import k9_walk as K
import oracle
from semanticlens_amd import _native as N
from semanticlens_amd import scores

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ASSERTED = [name for name, f in K.FAMILIES.items() if f["asserted"]]
MEASURED = [name for name, f in K.FAMILIES.items() if not f["asserted"]]


@lru_cache(maxsize=None)
def _oracle(name):
    """`oracle.polysemanticity` of a family (score, fallback rows), once per process."""
    V = K.reference(name)[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # ConvergenceWarning: fewer distinct points than clusters, on purpose
        return oracle.polysemanticity(V, n_clusters=K.FAMILIES[name]["k"], return_fallback=True)


def _entry_point(V, k, first, rand, replace, workspace):
    """(score, min_count, labels) straight from `sl_poly2means_labels` (LDS variant) or `sl_polykmeans_labels` (workspace
    variant): `_native.poly2means` does not hand out the min_count the kernel decides the fallback by."""
    C, n, D = V.shape
    lib, p = N.lib(), N._ptr
    first, rand = np.ascontiguousarray(first, dtype=np.int32), np.ascontiguousarray(rand, dtype=np.float64)
    score = torch.empty((C,), dtype=torch.float64, device=DEV)
    mc = torch.empty((C,), dtype=torch.int32, device=DEV)
    lab = torch.full((C, n), -1, dtype=torch.int32, device=DEV)
    nbytes = int(lib.sl_polykmeans_ws_bytes(C, n, D, k, len(first)) if workspace else lib.sl_poly2means_ws_bytes(C, n, D))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    tail = (first.ctypes.data_as(N._vp), len(first), rand.ctypes.data_as(N._vp), int(replace), p(score), p(mc), p(lab), p(ws), nbytes,
            N._stream(V))
    rc = lib.sl_polykmeans_labels(p(V), C, n, D, k, *tail) if workspace else lib.sl_poly2means_labels(p(V), C, n, D, *tail)
    torch.cuda.synchronize()
    assert rc == 0, N.lib().sl_last_error().decode()
    return score, mc, lab


def _device(monkeypatch, V, k, replace, workspace):
    """(score, min_count, labels) as numpy of one storage variant, through `_native.poly2means` as dispatched (the workspace
    variant forced by POLY2_MAX_N = 0 where the LDS variant would take the call) and from the variant's entry point: equal bits."""
    C, n, _ = V.shape
    first, rand = scores.kmeans_draws(n, 10, 123, k)
    with monkeypatch.context() as m:
        if workspace:
            m.setattr(N, "POLY2_MAX_N", 0)
        assert (k != 2 or n > N.POLY2_MAX_N) == workspace
        lab = torch.full((C, n), -1, dtype=torch.int32, device=DEV)
        score = N.poly2means(V, first, rand, replace, n_clusters=k, labels=lab)
    s2, mc, l2 = _entry_point(V, k, first, rand, replace, workspace)
    assert torch.equal(score, s2) and torch.equal(lab, l2), "the dispatch did not reach this variant's entry point"
    return score.cpu().numpy(), mc.cpu().numpy(), lab.cpu().numpy()


def _variants(n, k):
    return (("lds", False), ("workspace", True)) if k == 2 and n <= N.POLY2_MAX_N else (("workspace", True),)


@pytest.mark.parametrize("name", ASSERTED)
def test_family_against_sklearn(monkeypatch, name):
    """Labels, scores and min_count of every storage variant that takes the family, against scikit-learn.  A component may be
    left out only where its device labels differ AND the walk's smallest relative decision margin on it is below 1e-12 (the
    near-tie rule of tools/k9_postmortem.py), at most 1 in 100 per family.  Measured on an MI355X: no component of any family
    left out, every label equal."""
    f = K.FAMILIES[name]
    k = f["k"]
    Vh, sk, raw = K.reference(name)
    C, n, _ = Vh.shape
    want, fallback = _oracle(name)
    want_mc = np.array([np.bincount(l, minlength=k).min() for l in sk])
    assert np.array_equal(fallback, want_mc < 2)
    np.testing.assert_allclose(raw[~fallback], want[~fallback], rtol=0, atol=1e-12)  # two statements of one reference
    V = torch.from_numpy(Vh.copy()).to(DEV)
    got = {}
    for replace in (True, False):
        for variant, workspace in _variants(n, k):
            s, mc, lab = _device(monkeypatch, V, k, replace, workspace)
            got[variant, replace] = (mc, lab)
            differ = np.nonzero((lab != sk).any(axis=1))[0]
            tie = np.array([K.walk(Vh[c], k)[2]["min_margin"] < K.NEAR_TIE for c in differ], dtype=bool)
            print(f"K9 {name} {variant} replace={replace}: {C} components, labels differ on {differ.size} "
                  f"({int(tie.sum())} of them near-ties), {int(fallback.sum())} fallback rows")
            assert tie.all(), (name, variant, "labels differ from scikit-learn's for components", differ[~tie][:10])
            assert differ.size <= C // 100, (name, variant, "more than 1 in 100 components are near-ties", differ[:10])
            keep = np.ones(C, bool)
            keep[differ] = False
            assert np.array_equal(mc[keep], want_mc[keep]), (name, variant, "min_count")
            # replace=False: every row is scored from the centres; the reference's fallback rows then come from the same fits
            ref, loose = (want, fallback) if replace else (np.where(fallback, raw, want), np.zeros(C, bool))
            diff = np.abs(s - ref)
            print(f"   max |score - reference|: centre rows {diff[keep & ~loose].max() if (keep & ~loose).any() else 0:.2e}, "
                  f"fallback rows {diff[keep & loose].max() if (keep & loose).any() else 0:.2e}")
            bad = np.nonzero(keep & ~loose & ~(diff <= 1e-9))[0]
            assert bad.size == 0, (name, variant, replace, "centre scores differ", bad[:10], diff[bad[:10]])
            bad = np.nonzero(keep & loose & ~(diff <= 1e-6))[0]
            assert bad.size == 0, (name, variant, replace, "fallback scores differ", bad[:10], diff[bad[:10]])
        if len(_variants(n, k)) == 2:  # one procedure over two storage variants: the same decisions, bit for bit
            (ma, la), (mb, lb) = got["lds", replace], got["workspace", replace]
            assert np.array_equal(la, lb), (name, "labels differ between the storage variants")
            assert np.array_equal(ma, mb), (name, "min_count differs between the storage variants")
    (ma, la), (mb, lb) = got["workspace", True], got["workspace", False]
    assert np.array_equal(la, lb) and np.array_equal(ma, mb), "replace_empty_clusters changed the clustering"


@pytest.mark.parametrize("name", MEASURED)
def test_duplicates_off_a_power_of_two_fall_back_like_sklearn(monkeypatch, name):
    """Fewer distinct points than clusters, in 3, 5, 6 and 7 copies, n no power of two.  The kernel sees exact zeros between copies,
    returns early from the relocation and stops after one iteration with the empty clusters parked on the biggest one;
    scikit-learn counts the parked centres in its shift, runs a second iteration, and there relocates copies on distances of about
    1e-32 that rounding in feature space left (docs/K9_BRANCHES.md).  Labels and the centre score may therefore differ.  The
    fallback score does not depend on the clustering and both sides fall back on every component: that one is held to 1e-6.  The
    other two are counted and printed.  Measured on an MI355X: labels differ on 1 of 100 components, replace=False scores by more
    than 1e-9 on 46, largest replace=True difference 1.2e-7."""
    f = K.FAMILIES[name]
    k = f["k"]
    Vh, sk, raw = K.reference(name)
    C, n, _ = Vh.shape
    want, fallback = _oracle(name)
    assert fallback.all()
    V = torch.from_numpy(Vh.copy()).to(DEV)
    for variant, workspace in _variants(n, k):
        s, mc, lab = _device(monkeypatch, V, k, True, workspace)
        s_raw, _, lab_raw = _device(monkeypatch, V, k, False, workspace)
        assert np.array_equal(lab, lab_raw)
        print(f"K9 {name} {variant}: {C} components; device labels differ from scikit-learn's on "
              f"{int((lab != sk).any(axis=1).sum())}, replace=False scores differ by more than 1e-9 on "
              f"{int((np.abs(s_raw - raw) > 1e-9).sum())}, max |replace=True score - reference| {np.abs(s - want).max():.2e}")
        assert (mc < 2).all()
        np.testing.assert_allclose(s, want, rtol=0, atol=1e-6)


def test_relocating_run_alone_against_sklearn():
    """`relocate_empty` moving a point, seen directly.  Of an island component's ten runs the relocating one is never chosen, so
    above it shows only through its inertia.  Here that run is the only one (n_init = 1, its own draws, straight through the
    entry point) and the reference is scikit-learn's Lloyd from the same seed points: labels equal, the centre score within
    1e-9, min_count equal."""
    Vh, _, _ = K.reference("islands_14_k3")
    V = torch.from_numpy(Vh.copy()).to(DEV)
    worst = 0.0
    for c, X in enumerate(Vh):
        (first, rand), seeds = K.relocating_run(X, 3)
        sk, raw = K.sklearn_from_seeds(X, seeds)
        s, mc, lab = _entry_point(V[c:c + 1], 3, first, rand, False, True)
        assert np.array_equal(lab.cpu().numpy()[0], sk), (c, "labels differ from scikit-learn's")
        assert int(mc) == np.bincount(sk, minlength=3).min()
        worst = max(worst, abs(float(s) - raw))
    print(f"K9 islands, the relocating run alone: {len(Vh)} components, max |score - reference| {worst:.2e}")
    assert worst <= 1e-9
