"""K21 host side (no GPU): the label-export and facet-statistics ABI is declared, ``sl_facet_stats`` refuses bad arguments
before any launch, the ``Facets`` helpers are right on hand-made CPU tensors, and ``label_facets`` / ``search_facets`` check
their arguments before they touch a device."""
from __future__ import annotations

import math
import re
from pathlib import Path

import pytest
import torch

import semanticlens_amd
from semanticlens_amd import _native as N
from semanticlens_amd import lens as L
from semanticlens_amd import scores as S

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("sl_poly2means_labels", "sl_polykmeans_labels", "sl_facet_stats")


def _err():
    return N.lib().sl_last_error().decode()


def test_facet_symbols_declared():
    header = (ROOT / "include" / "semanticlens_amd.h").read_text()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in the header"
        assert name in N.SIGNATURES, f"{name} is not in _native.SIGNATURES"
        assert hasattr(N.lib(), name)
    # one more pointer than the calls without labels
    assert len(N.SIGNATURES["sl_poly2means_labels"][1]) == len(N.SIGNATURES["sl_poly2means"][1]) + 1
    assert len(N.SIGNATURES["sl_polykmeans_labels"][1]) == len(N.SIGNATURES["sl_polykmeans"][1]) + 1
    assert re.search(r"^SRCS :=.*\bfacets\.hip\b", (ROOT / "semanticlens_amd" / "csrc" / "Makefile").read_text(), re.M)
    assert N.lib().sl_abi_version() == 1  # the change is additive
    assert callable(N.facet_stats)


def test_api_exists():
    for name in ("Facets", "polysemanticity_facets", "label_facets", "search_facets"):
        assert name in semanticlens_amd.__all__ and hasattr(semanticlens_amd, name)
    assert semanticlens_amd.label_facets is L.label_facets and semanticlens_amd.search_facets is L.search_facets
    assert semanticlens_amd.Facets is S.Facets
    for method in ("eval_facets", "label_facets", "search_facets"):
        assert callable(getattr(L.Lens, method))


def test_facet_stats_argument_errors_before_launch():
    stats = N.lib().sl_facet_stats
    # (V, C, n, D, labels, n_clusters, centres, counts, clarity, stream)
    assert stats(None, 3, 5, 8, None, 2, None, None, None, None) == -1
    assert "null pointer" in _err()
    buf = torch.zeros(3 * 5 * 8)  # host memory: never dereferenced, the call must fail on the pointers that ARE null
    p = buf.data_ptr()
    assert stats(p, 3, 5, 8, None, 2, p, p, None, None) == -1  # labels
    assert "null pointer" in _err()
    assert stats(p, 3, 5, 8, p, 2, None, p, None, None) == -1  # centres
    assert "null pointer" in _err()
    assert stats(p, 3, 5, 8, p, 2, p, None, None, None) == -1  # counts
    assert "null pointer" in _err()
    assert stats(None, 3, 5, 8, p, 2, p, p, p, None) == -1  # V
    assert "null pointer" in _err()
    assert stats(p, 3, 5, 8, p, 0, p, p, p, None) == -1
    assert "n_clusters=0" in _err()
    assert stats(p, 3, 5, 8, p, 17, p, p, p, None) == -1
    assert "n_clusters=17" in _err()
    assert stats(p, 3, 1025, 8, p, 2, p, p, p, None) == -1
    assert "1025" in _err()
    assert stats(p, -1, 5, 8, p, 2, p, p, p, None) == -1
    assert "negative" in _err()
    assert stats(p, 3, -5, 8, p, 2, p, p, p, None) == -1
    assert "negative" in _err()
    assert stats(p, 3, 5, -8, p, 2, p, p, p, None) == -1
    assert "negative" in _err()
    assert stats(None, 0, 5, 8, None, 2, None, None, None, None) == 0  # C == 0: success, no launch


def test_label_entry_points_refuse_a_null_label_pointer():
    lib = N.lib()
    buf = torch.zeros(64)
    p = buf.data_ptr()
    assert lib.sl_poly2means_labels(p, 2, 4, 4, p, 10, p, 1, p, None, None, p, 1 << 20, None) == -1
    assert "null label pointer" in _err()
    assert lib.sl_polykmeans_labels(p, 2, 4, 4, 3, p, 10, p, 1, p, None, None, p, 1 << 20, None) == -1
    assert "null label pointer" in _err()
    assert lib.sl_poly2means_labels(None, 0, 4, 4, None, 10, None, 1, None, None, None, None, 0, None) == 0
    assert lib.sl_polykmeans_labels(None, 0, 4, 4, 3, None, 10, None, 1, None, None, None, None, 0, None) == 0


def test_facet_stats_wrapper_argument_errors_without_a_device():
    with pytest.raises(ValueError, match="labels"):
        N.facet_stats(torch.zeros(2, 3, 4), torch.zeros(2, 4, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="n_clusters=17"):
        N.facet_stats(torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.int32), 17)
    with pytest.raises(ValueError, match="n_clusters=0"):
        N.facet_stats(torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.int32), 0)
    with pytest.raises(ValueError, match="n_samples=1025"):
        N.facet_stats(torch.zeros(1, 1025, 4), torch.zeros(1, 1025, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="n_components"):
        S.polysemanticity_facets(torch.zeros(3, 4))
    with pytest.raises(ValueError, match="n_clusters=17"):
        S.polysemanticity_facets(torch.zeros(2, 20, 4), n_clusters=17)
    with pytest.raises(ValueError, match="n_clusters=1"):
        S.polysemanticity_facets(torch.zeros(2, 20, 4), n_clusters=1)


def _hand_made(kc: int = 2, D: int = 4, empty: bool = True) -> S.Facets:
    """Three components of five samples; with ``empty``, component 1 has an empty facet 0 (zero centre, NaN clarity)."""
    labels = torch.tensor([[0, 1, 1, 0, 1], [1, 1, 1, 1, 1], [kc - 1, 0, 0, 0, 0]], dtype=torch.int32)
    if not empty:
        labels[1, 0] = 0
    counts = torch.stack([(labels == j).sum(1) for j in range(kc)], dim=1).to(torch.int32)
    centers = torch.arange(3 * kc * D, dtype=torch.float32).reshape(3, kc, D) + 1
    centers[counts == 0] = 0
    clarity = torch.full((3, kc), 0.5)
    clarity[counts < 2] = math.nan
    return S.Facets(score=torch.zeros(3, dtype=torch.float64), labels=labels, counts=counts, centers=centers, clarity=clarity)


def test_facets_helpers_on_hand_made_tensors():
    f = _hand_made(kc=3, D=4)
    assert f.n_clusters == 3
    agg = f.aggregated()
    assert tuple(agg.shape) == (9, 4)
    for c in range(3):
        for j in range(3):
            assert torch.equal(agg[c * 3 + j], f.centers[c, j])
    m = f.members(1)
    assert m.dtype == torch.bool and tuple(m.shape) == (3, 5)
    assert m.tolist() == [[False, True, True, False, True], [True] * 5, [False] * 5]
    assert f.members(2).tolist()[2] == [True, False, False, False, False]
    with pytest.raises(IndexError):
        f.members(3)
    comp, facet = f.decode(torch.tensor([[0, 4, 8], [5, -1, 2]]))
    assert comp.tolist() == [[0, 1, 2], [1, -1, 0]]
    assert facet.tolist() == [[0, 1, 2], [2, -1, 2]]
    rows = torch.arange(9)
    comp, facet = f.decode(rows)
    assert torch.equal(comp, rows // 3) and torch.equal(facet, rows % 3)


def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(N, "_f32c", no_device)
    monkeypatch.setattr(N, "topk_probe", no_device)


class _NoTower:
    device = "cpu"

    def tokenize(self, *a):
        raise AssertionError("the text tower ran before the arguments were checked")

    encode_text = tokenize


def test_label_facets_argument_errors_without_a_device(monkeypatch):
    _no_device(monkeypatch)
    f = _hand_made()
    fm = _NoTower()
    for bad_k in (0, -1, N.TOPK_MAX_K + 1, 2.5, "3"):
        with pytest.raises(ValueError, match="k"):
            L.label_facets(fm, ["cat"], f, k=bad_k)
    for bad_vocabulary in ([], "cat", None):
        with pytest.raises(ValueError, match="vocabulary"):
            L.label_facets(fm, bad_vocabulary, f)
    with pytest.raises(ValueError, match="widths differ"):
        L.label_facets(fm, ["cat"], {"a": f, "b": _hand_made(D=8)})
    with pytest.raises(ValueError, match="chunk_size"):
        L.label_facets(fm, ["cat"], f, chunk_size=0)
    with pytest.raises(ValueError, match="Facets"):
        L.label_facets(fm, ["cat"], torch.zeros(4, 4))
    with pytest.raises(ValueError, match="Facets"):
        L.label_facets(fm, ["cat"], {"a": torch.zeros(4, 4)})


def test_search_facets_argument_errors_without_a_device(monkeypatch):
    _no_device(monkeypatch)
    f = _hand_made()
    fm = _NoTower()
    for bad_k in (0, N.TOPK_MAX_K + 1, 1.5):
        with pytest.raises(ValueError, match="k"):
            L.search_facets(fm, "cat", f, k=bad_k)
    with pytest.raises(ValueError, match="at least one query"):
        L.search_facets(fm, [], f)
    with pytest.raises(ValueError, match="widths differ"):
        L.search_facets(fm, "cat", {"a": f, "b": _hand_made(D=8)})
    with pytest.raises(ValueError, match="Facets"):
        L.search_facets(fm, "cat", [f])


def test_search_facets_maps_kept_rows_back(monkeypatch):
    """Empty facets are dropped before the probe; the rows ``search_components`` returns index the KEPT rows of each layer and
    must come back as (component, facet) of the full ``aggregated()``.  The probe is replaced by a hand-made answer."""
    fa, fb = _hand_made(kc=2), _hand_made(kc=3, empty=False)
    # layer a: aggregated rows 0..5, row 2 (component 1, facet 0) is empty -> kept rows [0, 1, 3, 4, 5]
    # layer b (kc = 3): counts [[2, 3, 0], [1, 4, 0], [4, 0, 1]] -> kept rows [0, 1, 3, 4, 6, 8]
    seen = {}

    def fake_search(fm, query, db, k, templates):
        seen["sizes"] = [v.shape[0] for v in db.values()]
        seen["rows_a"] = db[0].clone()
        vals = torch.tensor([[0.9, 0.8, 0.7, -math.inf]])
        layer = torch.tensor([[0, 1, 1, -1]])
        row = torch.tensor([[2, 5, 1, -1]])
        return vals, layer, row, list(db)

    monkeypatch.setattr(L, "search_components", fake_search)
    vals, layer, comp, facet, names = L.search_facets(object(), "q", {"a": fa, "b": fb}, k=4)
    assert seen["sizes"] == [5, 6]
    assert torch.equal(seen["rows_a"], fa.aggregated()[torch.tensor([0, 1, 3, 4, 5])])
    assert names == ["a", "b"]
    assert layer.tolist() == [[0, 1, 1, -1]]
    # a: kept row 2 -> original row 3 = (1, 1); b: kept row 5 -> original 8 = (2, 2); kept row 1 -> original 1 = (0, 1)
    assert comp.tolist() == [[1, 2, 0, -1]]
    assert facet.tolist() == [[1, 2, 1, -1]]
    assert vals[0, 3] == -math.inf
