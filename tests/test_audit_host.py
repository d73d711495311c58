"""K22 host side (no GPU): the sl_segmax_merge ABI is declared and its argument errors come back before any launch,
``audit_concepts`` and ``setmax_probe`` check their arguments before they touch a device or the text tower, and ``ConceptAudit``'s
``margin`` / ``flag`` / ``rank`` / ``describe`` are right on hand-made alignments (CPU tensors)."""
from __future__ import annotations

import re
from pathlib import Path

import pytest
import torch

import semanticlens_amd
from helpers import FakeVLM
from semanticlens_amd import _native as N
from semanticlens_amd import lens as L

ROOT = Path(__file__).resolve().parent.parent
MAX_ID = (1 << 32) - 2
NAN = float("nan")


def _err():
    return N.lib().sl_last_error().decode()


def test_segmax_symbol_declared():
    header = (ROOT / "include" / "semanticlens_amd.h").read_text()
    assert re.search(r"\bsl_segmax_merge\s*\(", header), "sl_segmax_merge is not declared in the header"
    assert "sl_segmax_merge" in N.SIGNATURES and hasattr(N.lib(), "sl_segmax_merge")
    assert "segmax.hip" in (ROOT / "semanticlens_amd" / "csrc" / "Makefile").read_text()
    for fn in ("segmax_merge", "setmax_probe", "setmax_finish"):
        assert callable(getattr(N, fn))


def test_segmax_merge_argument_errors_before_launch():
    merge = N.lib().sl_segmax_merge
    # (state, state_ld, G, R, B, cand, ld, row_seg, row_id_base, stream); 8 and 16 stand for non-null, suitably aligned pointers:
    # every call below is refused before a pointer is followed
    assert merge(None, 8, 2, -1, 8, None, 8, None, 0, None) == -1
    assert "negative" in _err()
    assert merge(None, 8, -2, 4, 8, None, 8, None, 0, None) == -1
    assert "negative" in _err()
    assert merge(None, 8, 2, 4, 8, None, 7, None, 0, None) == -1
    assert "row stride" in _err()
    assert merge(None, 7, 2, 4, 8, None, 8, None, 0, None) == -1
    assert "state stride" in _err()
    assert merge(None, 8, 2, 4, 8, None, 8, None, -1, None) == -1
    assert "row ids" in _err() and "2^32 - 2" in _err()
    assert merge(None, 8, 2, 4, 8, None, 8, None, MAX_ID - 2, None) == -1  # the last row would have the id 2^32 - 1
    assert "row ids" in _err()
    assert merge(None, 8, 2, 4, 8, None, 8, None, 1 << 40, None) == -1
    assert "row ids" in _err()
    assert merge(None, 8, 2, 4, 8, 16, 8, 16, MAX_ID - 3, None) == -1  # ids in range: now the null pointers are refused
    assert "null state" in _err()
    assert merge(16, 8, 2, 4, 8, None, 8, 16, 0, None) == -1
    assert "null candidate tile" in _err()
    assert merge(16, 8, 2, 4, 8, 16, 8, None, 0, None) == -1
    assert "null segment table" in _err()
    assert merge(16, 8, 2, 4, 8, 18, 8, 16, 0, None) == -1
    assert "4-byte aligned" in _err()
    assert merge(16, 8, 2, 4, 8, 16, 8, 18, 0, None) == -1
    assert "4-byte aligned" in _err()
    assert merge(20, 8, 2, 4, 8, 16, 8, 16, 0, None) == -1
    assert "8-byte aligned" in _err()
    assert merge(16, 1, 2, 1 << 40, 1, 16, 1, 16, 0, None) == -1  # the row-id range is checked before the workgroup limit
    assert "row ids" in _err()


def test_segmax_zero_sizes_are_no_ops():
    merge = N.lib().sl_segmax_merge
    assert merge(None, 8, 2, 0, 8, None, 8, None, 0, None) == 0
    assert merge(None, 0, 2, 4, 0, None, 0, None, 0, None) == 0
    assert merge(None, 8, 0, 4, 8, None, 8, None, 0, None) == 0
    assert merge(None, 0, 0, 0, 0, None, 0, None, MAX_ID, None) == 0


def test_api_exists():
    assert callable(L.audit_concepts) and callable(L.Lens.audit_concepts) and callable(L.probe_setmax)
    for name in ("audit_concepts", "ConceptAudit", "probe_setmax"):
        assert getattr(semanticlens_amd, name) is getattr(L, name)
        assert name in semanticlens_amd.__all__


def test_audit_argument_errors_without_a_device_or_the_text_tower(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(N, "_f32c", no_device)
    monkeypatch.setattr(N, "setmax_probe", no_device)
    fm = FakeVLM(dim=16)
    db = torch.zeros(4, 16)
    good = {"ox/valid": ["ox", "horns"], "ox/spurious": ["grass"]}
    with pytest.raises(ValueError, match="non-empty mapping"):
        L.audit_concepts(fm, [["ox"], ["grass"]], db)
    with pytest.raises(ValueError, match="non-empty mapping"):
        L.audit_concepts(fm, "ox", db)
    with pytest.raises(ValueError, match="non-empty mapping"):
        L.audit_concepts(fm, {}, db)
    with pytest.raises(ValueError, match="'ox/spurious' must be a non-empty list"):
        L.audit_concepts(fm, {"ox/valid": ["ox"], "ox/spurious": []}, db)
    with pytest.raises(ValueError, match="non-empty list"):
        L.audit_concepts(fm, {"ox/valid": "ox"}, db)  # a bare string is not a list of prompts
    with pytest.raises(ValueError, match="not a string"):
        L.audit_concepts(fm, {"ox/valid": ["ox", 3]}, db)
    with pytest.raises(ValueError, match="chunk_size"):
        L.audit_concepts(fm, good, db, chunk_size=0)
    with pytest.raises(ValueError, match="2-D"):
        L.audit_concepts(fm, good, torch.zeros(4, 3, 16))
    with pytest.raises(ValueError, match="2-D"):
        L.Lens(fm, device="cpu").audit_concepts(good, {"l1": db, "l2": torch.zeros(2, 3, 16)})
    with pytest.raises(ValueError, match="widths differ"):
        L.audit_concepts(fm, good, {"l1": db, "l2": torch.zeros(4, 8)})
    assert fm.calls["encode_text"] == 0


def test_setmax_probe_argument_errors_without_a_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(N, "_f32c", no_device)
    x, y = torch.zeros(6, 4), torch.zeros(3, 4)
    with pytest.raises(ValueError, match="non-decreasing"):
        N.setmax_probe(x, [0, 4, 2, 6], y)
    with pytest.raises(ValueError, match="end at the number of prompt rows"):
        N.setmax_probe(x, [0, 2, 5], y)
    with pytest.raises(ValueError, match="start at 0"):
        N.setmax_probe(x, [1, 2, 6], y)
    with pytest.raises(ValueError, match="start at 0"):
        N.setmax_probe(x, [], y)
    with pytest.raises(ValueError, match="integers"):
        N.setmax_probe(x, [0, 2.5, 6], y)
    with pytest.raises(ValueError, match="2-D"):
        N.setmax_probe(torch.zeros(6), [0, 6], y)
    with pytest.raises(ValueError, match="widths differ"):
        N.setmax_probe(x, [0, 6], torch.zeros(3, 5))
    with pytest.raises(ValueError, match="chunk_rows"):
        N.setmax_probe(x, [0, 6], y, chunk_rows=0)
    with pytest.raises(ValueError, match="chunk_cols"):
        N.setmax_probe(x, [0, 6], y, chunk_cols=-1)
    with pytest.raises(ValueError, match="prompt ids"):
        N.setmax_probe(x, [0, 6], y, id_base=MAX_ID - 4)
    with pytest.raises(ValueError, match="state must be"):
        N.setmax_probe(x, [0, 2, 6], y, state=torch.zeros(3, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="non-decreasing"):
        L.probe_setmax(x, [0, 4, 2, 6], y)
    with pytest.raises(ValueError, match="does not match"):
        L.probe_setmax(x, [0, 6], torch.zeros(3, 5))
    assert N.check_set_offsets((0, 0, 6, 6), 6) == [0, 0, 6, 6]  # empty sets are fine here


# ---------------------------------------------------------------------------------------------------------------------
# ConceptAudit on hand-made alignments
# ---------------------------------------------------------------------------------------------------------------------
def _hand_made():
    """Two layers ("l0": 4 components, "l1": 3), four sets: two valid ("v0", "v1") and two spurious ("s0", "s1")."""
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    alignment = {
        #            c0    c1    c2    c3
        "l0": t([[0.50, 0.10, 0.25, 0.30],    # v0
                 [0.25, 0.40, 0.10, NAN],     # v1
                 [0.75, 0.20, 0.20, 0.50],    # s0
                 [0.10, 0.30, 0.75, 0.10]]),  # s1
        "l1": t([[0.25, 0.50, 0.00],
                 [0.25, 0.10, 0.25],
                 [0.50, 0.25, 0.75],
                 [0.00, 0.20, 0.10]]),
    }
    best = {"l0": torch.tensor([[0, 1, 0, 1], [2, 2, 3, 2], [4, 5, 4, 4], [6, 6, 7, 6]]),
            "l1": torch.tensor([[1, 1, 0], [3, 2, 2], [5, 5, 4], [7, 6, 6]])}
    return L.ConceptAudit(sets=["v0", "v1", "s0", "s1"], prompts=["ox", "horns", "hooves", "yoke", "grass", "cart", "fence", "mud"],
                          set_offsets=[0, 2, 4, 6, 8], layers=["l0", "l1"], alignment=alignment, best_prompt=best)


def test_margin_over_several_sets():
    a = _hand_made()
    m = a.margin(valid=["v0", "v1"], spurious=["s0", "s1"])
    assert list(m) == ["l0", "l1"] and m["l0"].dtype == torch.float32
    # l0: spurious best [0.75, 0.30, 0.75, 0.50], valid best [0.50, 0.40, 0.25, NaN]
    assert m["l0"][:3].tolist() == pytest.approx([0.25, -0.10, 0.50])
    assert torch.isnan(m["l0"][3])  # amax propagates the NaN
    assert m["l1"].tolist() == pytest.approx([0.25, -0.25, 0.50])
    one = a.margin(valid="v0", spurious="s1")  # one name instead of a list
    assert one["l0"].tolist() == pytest.approx([-0.40, 0.20, 0.50, -0.20])
    assert one["l1"].tolist() == pytest.approx([-0.25, -0.30, 0.10])


def test_unknown_set_name_is_a_key_error():
    a = _hand_made()
    with pytest.raises(KeyError, match="nope"):
        a.margin(valid="v0", spurious="nope")
    with pytest.raises(KeyError, match="v7"):
        a.flag(valid=["v0", "v7"], spurious="s0")
    with pytest.raises(KeyError, match="nope"):
        a.rank(valid="nope", spurious="s0")


def test_flag_margin_min_alignment_and_nan():
    a = _hand_made()
    f = a.flag(valid=["v0", "v1"], spurious=["s0", "s1"])
    assert f["l0"].dtype == torch.bool
    assert f["l0"].tolist() == [True, False, True, False]  # c3's margin is NaN: not flagged
    assert f["l1"].tolist() == [True, False, True]
    f = a.flag(valid=["v0", "v1"], spurious=["s0", "s1"], margin=0.25)  # strictly above
    assert f["l0"].tolist() == [False, False, True, False] and f["l1"].tolist() == [False, False, True]
    f = a.flag(valid=["v0", "v1"], spurious=["s0", "s1"], min_alignment=0.75)
    assert f["l0"].tolist() == [True, False, True, False] and f["l1"].tolist() == [False, False, True]
    f = a.flag(valid="v0", spurious="s0", min_alignment=0.5)  # c3: margin 0.2, spurious alignment exactly 0.5 (>=)
    assert f["l0"].tolist() == [True, False, False, True]
    a.alignment["l0"][2, 0] = NAN  # a NaN spurious alignment flags nothing either
    assert a.flag(valid="v0", spurious="s0", min_alignment=0.0)["l0"].tolist() == [False, True, False, True]


def test_rank_order_ties_nan_and_clipping():
    a = _hand_made()
    vals, layer, comp = a.rank(valid=["v0", "v1"], spurious=["s0", "s1"], k=4)
    # margins l0 [0.25, -0.10, 0.50, NaN], l1 [0.25, -0.25, 0.50]: NaN first, then 0.50 (l0/2 before l1/2), then 0.25 (l0/0 ...)
    assert torch.isnan(vals[0]) and vals[1:].tolist() == pytest.approx([0.5, 0.5, 0.25])
    assert layer.tolist() == [0, 0, 1, 0] and comp.tolist() == [3, 2, 2, 0]
    assert layer.dtype == torch.int64 and comp.dtype == torch.int64
    vals, layer, comp = a.rank(valid=["v0", "v1"], spurious=["s0", "s1"], k=100)  # clipped to the 7 components
    assert tuple(vals.shape) == (7,)
    assert layer.tolist() == [0, 0, 1, 0, 1, 0, 1] and comp.tolist() == [3, 2, 2, 0, 0, 1, 1]
    with pytest.raises(ValueError, match="at least 1"):
        a.rank(valid="v0", spurious="s0", k=0)


def test_rank_importance_tensor_and_dict():
    a = _hand_made()
    # a dict: l1 weighted, l0 missing (counts as 1); l1's margins [0.25, -0.25, 0.50] * [4, -2, 0.25] = [1.0, 0.5, 0.125]
    vals, layer, comp = a.rank(valid=["v0", "v1"], spurious=["s0", "s1"], k=4, importance={"l1": torch.tensor([4.0, -2.0, 0.25])})
    assert torch.isnan(vals[0]) and vals[1:].tolist() == pytest.approx([1.0, 0.5, 0.5])
    assert layer.tolist() == [0, 1, 0, 1] and comp.tolist() == [3, 0, 2, 1]  # the 0.5 tie: the earlier layer first
    single = L.ConceptAudit(sets=a.sets, prompts=a.prompts, set_offsets=a.set_offsets, layers=[None],
                            alignment={None: a.alignment["l1"]}, best_prompt={None: a.best_prompt["l1"]})
    vals, layer, comp = single.rank(valid=["v0", "v1"], spurious=["s0", "s1"], k=2, importance=torch.tensor([1.0, -4.0, 1.0]))
    assert vals.tolist() == pytest.approx([1.0, 0.5]) and layer.tolist() == [0, 0] and comp.tolist() == [1, 2]
    with pytest.raises(ValueError, match="importance"):
        single.rank(valid="v0", spurious="s0", importance=torch.ones(5))


def test_describe_is_a_host_list():
    a = _hand_made()
    d = a.describe("l0", 2)
    assert [name for name, _, _ in d] == ["v0", "v1", "s0", "s1"]
    assert [v for _, v, _ in d] == pytest.approx([0.25, 0.1, 0.2, 0.75])
    assert [p for _, _, p in d] == ["ox", "yoke", "grass", "mud"]
    assert all(isinstance(v, float) for _, v, _ in d)
    a.best_prompt["l1"][1, 0] = -1  # an empty entry has no prompt
    assert a.describe("l1", 0)[1][2] is None
