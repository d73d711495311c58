"""K20 host side (no GPU): the sl_mutualmax_* ABI is declared, argument errors come back before any launch, ``compare_concept_dbs``
checks its arguments before it touches a device, and the result object's across-layer decode and ``mutual()`` are right on
hand-made per-pair results (CPU tensors)."""
from __future__ import annotations

import re
from pathlib import Path

import pytest
import torch

import semanticlens_amd
from semanticlens_amd import _native as N
from semanticlens_amd import lens as L

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("sl_mutualmax_merge", "sl_mutualmax_finish")
MAX_ID = (1 << 32) - 2


def _err():
    return N.lib().sl_last_error().decode()


def test_mutualmax_symbols_declared():
    header = (ROOT / "include" / "semanticlens_amd.h").read_text()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in the header"
        assert name in N.SIGNATURES, f"{name} is not in _native.SIGNATURES"
        assert hasattr(N.lib(), name)
    assert "mutualmax.hip" in (ROOT / "semanticlens_amd" / "csrc" / "Makefile").read_text()
    for fn in ("mutualmax_merge", "mutualmax_finish", "mutual_probe"):
        assert callable(getattr(N, fn))
    assert N.MUTUALMAX_MAX_ID == MAX_ID


def test_mutualmax_merge_argument_errors_before_launch():
    merge = N.lib().sl_mutualmax_merge
    # (row_state, col_state, R, B, cand, ld, row_id_base, col_id_base, stream)
    assert merge(None, None, -1, 8, None, 8, 0, 0, None) == -1
    assert "negative" in _err()
    assert merge(None, None, 4, -8, None, 8, 0, 0, None) == -1
    assert "negative" in _err()
    assert merge(None, None, 4, 8, None, 7, 0, 0, None) == -1
    assert "row stride" in _err()
    assert merge(None, None, 4, 8, None, 8, -1, 0, None) == -1
    assert "row ids" in _err() and "2^32 - 2" in _err()
    assert merge(None, None, 4, 8, None, 8, 0, -1, None) == -1
    assert "column ids" in _err()
    assert merge(None, None, 4, 8, None, 8, MAX_ID - 2, 0, None) == -1  # the last row would have the id 2^32 - 1
    assert "row ids" in _err()
    assert merge(None, None, 4, 8, None, 8, 0, MAX_ID - 6, None) == -1
    assert "column ids" in _err()
    assert merge(None, None, 4, 8, None, 8, 1 << 40, 0, None) == -1
    assert merge(None, None, 4, 8, None, 8, MAX_ID - 3, MAX_ID - 7, None) == -1  # ids in range: now the null pointers are refused
    assert "null state" in _err()
    assert merge(None, None, 4, 8, None, 8, 0, 0, None) == -1
    assert "null state" in _err()


def test_mutualmax_zero_sizes_are_no_ops():
    lib = N.lib()
    assert lib.sl_mutualmax_merge(None, None, 0, 8, None, 8, 0, 0, None) == 0
    assert lib.sl_mutualmax_merge(None, None, 4, 0, None, 0, 0, 0, None) == 0
    assert lib.sl_mutualmax_merge(None, None, 0, 0, None, 0, MAX_ID, MAX_ID, None) == 0
    assert lib.sl_mutualmax_finish(None, 0, None, None, None) == 0


def test_mutualmax_finish_argument_errors():
    lib = N.lib()
    assert lib.sl_mutualmax_finish(None, -1, None, None, None) == -1
    assert "negative" in _err()
    assert lib.sl_mutualmax_finish(None, 5, None, None, None) == -1
    assert "null pointer" in _err()


def test_api_exists():
    assert callable(L.compare_concept_dbs) and callable(L.Lens.compare_concept_dbs)
    assert semanticlens_amd.compare_concept_dbs is L.compare_concept_dbs
    assert "compare_concept_dbs" in semanticlens_amd.__all__


def test_compare_argument_errors_without_a_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(N, "_f32c", no_device)
    monkeypatch.setattr(N, "mutual_probe", no_device)
    db = torch.zeros(4, 16)
    with pytest.raises(ValueError, match="does not match"):
        L.compare_concept_dbs(db, torch.zeros(4, 8))
    with pytest.raises(ValueError, match="does not match"):
        L.compare_concept_dbs({"l1": db}, {"m1": torch.zeros(3, 8), "m2": torch.zeros(5, 8)})
    with pytest.raises(ValueError, match="widths differ"):
        L.compare_concept_dbs(db, {"m1": torch.zeros(3, 16), "m2": torch.zeros(5, 8)})
    with pytest.raises(ValueError, match="2-D"):
        L.compare_concept_dbs(torch.zeros(4, 3, 16), db)
    with pytest.raises(ValueError, match="2-D"):
        L.compare_concept_dbs(db, {"m1": torch.zeros(2, 3, 16)})
    with pytest.raises(ValueError, match="2-D"):
        L.compare_concept_dbs({"l1": db, "l2": torch.zeros(16)}, db)
    with pytest.raises(ValueError, match="DB A is empty"):
        L.compare_concept_dbs({}, db)
    with pytest.raises(ValueError, match="DB B is empty"):
        L.compare_concept_dbs(db, torch.zeros(0, 16))
    with pytest.raises(ValueError, match="DB A is empty"):
        L.compare_concept_dbs({"l1": db, "l2": torch.zeros(0, 16)}, db)


def test_mutual_probe_argument_errors_without_a_device():
    with pytest.raises(ValueError, match="2-D"):
        N.mutual_probe(torch.zeros(4), torch.zeros(4, 4))
    with pytest.raises(ValueError, match="widths differ"):
        N.mutual_probe(torch.zeros(4, 8), torch.zeros(4, 4))
    with pytest.raises(ValueError, match="chunk_rows"):
        N.mutual_probe(torch.zeros(4, 4), torch.zeros(4, 4), chunk_rows=0)
    with pytest.raises(ValueError, match="chunk_cols"):
        N.mutual_probe(torch.zeros(4, 4), torch.zeros(4, 4), chunk_cols=-2)


def _hand_made():
    """A = {"a0": 3, "a1": 2 components}, B = {"b0": 2, "b1": 4}.  Per-pair results written by hand; the across-layer bests are
    what the order (larger value, then the earlier layer, then the smaller component) makes of them."""
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    i = lambda v: torch.tensor(v, dtype=torch.int64)
    pairs = {
        # (vals_a, ids_a into the B layer, vals_b, ids_b into the A layer)
        (0, 0): (t([0.9, 0.2, 0.5]), i([1, 0, 1]), t([0.2, 0.9]), i([1, 0])),
        (0, 1): (t([0.4, 0.8, 0.5]), i([3, 2, 0]), t([0.5, 0.1, 0.8, 0.4]), i([2, 0, 1, 0])),
        (1, 0): (t([0.3, 0.1]), i([0, 0]), t([0.3, 0.05]), i([0, 1])),
        (1, 1): (t([0.7, 0.6]), i([1, 3]), t([0.0, 0.7, 0.2, 0.6]), i([0, 0, 1, 1])),
    }
    # A -> B over B's global ids (b0: 0..1, b1: 2..5): a0/0 -> b0/1 (0.9); a0/1 -> b1/2 (0.8); a0/2: 0.5 in both layers -> the
    # earlier layer, b0/1; a1/0 -> b1/1 (0.7); a1/1 -> b1/3 (0.6)
    best_ab = [(t([0.9, 0.8, 0.5]), i([1, 4, 1])), (t([0.7, 0.6]), i([3, 5]))]
    # B -> A over A's global ids (a0: 0..2, a1: 3..4): b0/0 -> a1/0 (0.3); b0/1 -> a0/0 (0.9); b1/0 -> a0/2 (0.5);
    # b1/1 -> a1/0 (0.7); b1/2 -> a0/1 (0.8); b1/3 -> a1/1 (0.6)
    best_ba = [(t([0.3, 0.9]), i([3, 0])), (t([0.5, 0.7, 0.8, 0.6]), i([2, 3, 1, 4]))]
    return L.ConceptDBComparison(layers_a=["a0", "a1"], layers_b=["b0", "b1"], sizes_a=[3, 2], sizes_b=[2, 4], pairs=pairs,
                                 best_ab=best_ab, best_ba=best_ba)


def test_decode_across_layers_on_hand_made_results():
    cmp = _hand_made()
    v, layer, comp = cmp.best_in_b["a0"]
    assert v.tolist() == pytest.approx([0.9, 0.8, 0.5])
    assert layer.tolist() == [0, 1, 0] and comp.tolist() == [1, 2, 1]
    v, layer, comp = cmp.best_in_b["a1"]
    assert layer.tolist() == [1, 1] and comp.tolist() == [1, 3]
    v, layer, comp = cmp.best_in_a["b0"]
    assert layer.tolist() == [1, 0] and comp.tolist() == [0, 0]
    v, layer, comp = cmp.best_in_a["b1"]
    assert v.tolist() == pytest.approx([0.5, 0.7, 0.8, 0.6])
    assert layer.tolist() == [0, 1, 0, 1] and comp.tolist() == [2, 0, 1, 1]
    assert cmp.pair("a1", "b0")[1].tolist() == [0, 0]
    with pytest.raises(ValueError):
        cmp.pair("a1", "nope")


def test_mutual_on_hand_made_results():
    cmp = _hand_made()
    m = cmp.mutual()
    assert list(m) == ["a0", "a1"]
    assert m["a0"].dtype == torch.bool
    # a0/0 <-> b0/1 and a0/1 <-> b1/2 are mutual; a0/2 -> b0/1, whose best is a0/0: not mutual; a1/0 <-> b1/1, a1/1 <-> b1/3
    assert m["a0"].tolist() == [True, True, False]
    assert m["a1"].tolist() == [True, True]


def test_similarities_on_hand_made_results():
    cmp = _hand_made()
    ab, ba = cmp.layer_similarity_ab, cmp.layer_similarity_ba
    assert tuple(ab.shape) == (2, 2) and tuple(ba.shape) == (2, 2) and ab.dtype == torch.float32
    assert torch.allclose(ab, torch.tensor([[(0.9 + 0.2 + 0.5) / 3, (0.4 + 0.8 + 0.5) / 3], [0.2, 0.65]]), atol=1e-6)
    assert torch.allclose(ba, torch.tensor([[0.55, 0.175], [(0.5 + 0.1 + 0.8 + 0.4) / 4, (0.0 + 0.7 + 0.2 + 0.6) / 4]]), atol=1e-6)
    assert cmp.set_similarity_ab == pytest.approx((0.9 + 0.8 + 0.5 + 0.7 + 0.6) / 5)
    assert cmp.set_similarity_ba == pytest.approx((0.3 + 0.9 + 0.5 + 0.7 + 0.8 + 0.6) / 6)


def test_empty_entries_and_nan_in_hand_made_results():
    """An empty entry (-inf, -1) decodes to layer -1 / component -1 and is never mutual; a NaN value propagates into the means."""
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    i = lambda v: torch.tensor(v, dtype=torch.int64)
    cmp = L.ConceptDBComparison(
        layers_a=[None], layers_b=[None], sizes_a=[2], sizes_b=[2],
        pairs={(0, 0): (t([float("nan"), 0.5]), i([0, 1]), t([float("nan"), 0.5]), i([0, 1]))},
        best_ab=[(t([float("-inf"), 0.5]), i([-1, 1]))], best_ba=[(t([float("nan"), 0.5]), i([0, 1]))])
    v, layer, comp = cmp.best_in_b[None]
    assert layer.tolist() == [-1, 0] and comp.tolist() == [-1, 1]
    assert cmp.mutual()[None].tolist() == [False, True]
    assert torch.isnan(cmp.layer_similarity_ab).all()
    assert cmp.pair()[0].shape == (2,)
