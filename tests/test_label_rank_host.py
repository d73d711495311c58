"""K26 without a GPU: the order rule of csrc/rank_order.hpp as a host program, the entry point's argument checks,
``check_rank_targets``, the argument checks of ``label_rank`` / ``probe_rank`` before the text tower or a device is touched, and
``LabelRanks``' helpers on CPU tensors."""
from __future__ import annotations

import math
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import semanticlens_amd
from helpers import FakeVLM
from semanticlens_amd import _native as N
from semanticlens_amd import lens as L

ROOT = Path(__file__).resolve().parent.parent


def test_order_rule_on_the_host(tmp_path):
    """csrc/rank_order.hpp compiled with g++: ``orders_before`` on a table (NaN against NaN, +-0, +-inf, equal values on both sides
    of the id, the key's own id, ids above 2^32) and the kernel's 32-bit column form against it (tests/native/rank_order_check.cpp)."""
    exe = tmp_path / "rank_order_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe),
                    str(ROOT / "tests" / "native" / "rank_order_check.cpp")], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout


def test_entry_point_checks_arguments_without_a_device():
    lib = N.lib()
    assert N.RANK_MAX_TARGETS == 16
    assert lib.sl_rank_merge(None, 3, 1, 8, 4, 4, 0, 8, 8, None) == -1 and lib.sl_last_error().startswith(b"sl_rank_merge: null")
    for where in range(4):  # each of the four pointers
        ptrs = [8, 8, 8, 8]
        ptrs[where] = None
        assert lib.sl_rank_merge(ptrs[0], 3, 2, ptrs[1], 4, 4, 0, ptrs[2], ptrs[3], None) == -1
        assert b"null" in lib.sl_last_error()
    for T in (0, 17, -1):
        assert lib.sl_rank_merge(8, 3, T, 8, 4, 4, 0, 8, 8, None) == -1 and b"not in [1, 16]" in lib.sl_last_error()
    assert lib.sl_rank_merge(8, 3, 1, 8, 3, 4, 0, 8, 8, None) == -1 and b"row stride" in lib.sl_last_error()
    assert lib.sl_rank_merge(8, 3, 1, 8, 4, 0, 0, 8, 8, None) == -1 and b"at least one column" in lib.sl_last_error()
    assert lib.sl_rank_merge(8, 3, 1, 8, 4, 4, -1, 8, 8, None) == -1 and b"id_base" in lib.sl_last_error()
    assert lib.sl_rank_merge(8, -1, 1, 8, 4, 4, 0, 8, 8, None) == -1
    assert lib.sl_rank_merge(4, 3, 1, 8, 4, 4, 0, 8, 8, None) == -1 and b"8-byte aligned" in lib.sl_last_error()
    assert lib.sl_rank_merge(8, 3, 1, 6, 4, 4, 0, 8, 8, None) == -1 and b"4-byte aligned" in lib.sl_last_error()
    assert lib.sl_rank_merge(None, 0, 1, None, 4, 4, 0, None, None, None) == 0  # R == 0: a no-op


def test_check_rank_targets():
    got = N.check_rank_targets([1, None, [2, 0, -1], -1, [], np.int64(4), (3,)], 7, 5)
    assert got.dtype == torch.int64 and not got.is_cuda
    assert got.tolist() == [[1, -1, -1], [-1, -1, -1], [2, 0, -1], [-1, -1, -1], [-1, -1, -1], [4, -1, -1], [3, -1, -1]]
    assert N.check_rank_targets([None, None], 2, 5).tolist() == [[-1], [-1]]  # T is at least 1
    assert N.check_rank_targets(torch.tensor([[0, 4], [-1, 2]]), 2, 5).tolist() == [[0, 4], [-1, 2]]
    assert N.check_rank_targets(np.array([3, 1]), 2, 5).tolist() == [[3], [1]]
    assert tuple(N.check_rank_targets([list(range(16))], 1, 16).shape) == (1, 16)
    assert tuple(N.check_rank_targets([], 0, 5).shape) == (0, 1)
    for bad in ([5], [-2], [[0, 5]], [1.5], ["1"], [True], [[None, 2.0]], [list(range(17))], [0, 1], 3, "0", None, [[[0]]]):
        with pytest.raises(ValueError):
            N.check_rank_targets(bad, 1, 5)


class _FakeLens:
    def __init__(self, fm):
        self.fm = fm


VOCAB = ["cat", "dog", "fish", "dog"]


@pytest.mark.parametrize("kwargs", [
    dict(targets=None), dict(targets=3), dict(targets="cat"), dict(targets=[0] * 6), dict(targets=[0] * 8),  # not one entry per component
    dict(targets={"a": [0] * 7}),                                                    # a dict for a tensor DB
    dict(targets=["cat", "bird"] + [None] * 5),                                      # an unknown word
    dict(targets=[[0] * 17] + [None] * 6),                                           # more than 16 targets
    dict(targets=[4] + [None] * 6), dict(targets=[-2] + [None] * 6), dict(targets=[1.5] + [None] * 6),
    dict(chunk_size=0), dict(chunk_size=-4),
    dict(logit_scale=0), dict(logit_scale=-100.0), dict(logit_scale=math.inf), dict(logit_scale=math.nan), dict(logit_scale="100"),
    dict(vocabulary=[]), dict(vocabulary="word"),
])
def test_label_rank_refuses_bad_arguments_before_anything_runs(kwargs):
    fm = FakeVLM(dim=16)
    args = dict(vocabulary=VOCAB, targets=["cat", 1, ["dog", 2], None, None, None, None], chunk_size=None, logit_scale=None)
    args.update(kwargs)
    db = torch.randn(7, 16)  # a CPU tensor: moving it would need a device
    for call in (lambda: L.label_rank(fm, args["vocabulary"], db, args["targets"], templates=["a {}"], chunk_size=args["chunk_size"],
                                      logit_scale=args["logit_scale"]),
                 lambda: L.Lens.label_rank(_FakeLens(fm), args["vocabulary"], db, args["targets"], ["a {}"], None, args["chunk_size"],
                                           args["logit_scale"])):
        with pytest.raises(ValueError):
            call()
    assert fm.calls == {"encode_text": 0, "encode_image": 0}


def test_label_rank_dict_db_targets():
    fm = FakeVLM(dim=16)
    db = {"a": torch.randn(3, 16), "b": torch.randn(2, 16)}
    for bad in ({"c": [0, 0]}, {"a": [0, 0, 0], "c": [0, 0]}, [0, 0, 0], {"a": [0, 0]}, {"b": ["cat", "bird"]}):
        with pytest.raises(ValueError):
            L.label_rank(fm, VOCAB, db, bad)
        with pytest.raises(ValueError):
            L.probe_rank(torch.randn(4, 16), db, bad)
    with pytest.raises(ValueError, match="unknown layers"):
        L.label_rank(fm, VOCAB, db, {"c": [0, 0]})
    assert fm.calls == {"encode_text": 0, "encode_image": 0}


def test_words_resolve_to_their_first_occurrence():
    index = {}
    got = L._resolve_targets(["dog", ["fish", "dog", 3], None], 3, len(VOCAB), VOCAB, index)
    assert got.tolist() == [[1, -1, -1], [2, 1, 3], [-1, -1, -1]]


def test_probe_rank_refuses_bad_arguments():
    q, db = torch.randn(5, 16), torch.randn(7, 16)
    good = [0, 1, [2, 3], None, None, None, 4]
    for bad in (dict(chunk_rows=0), dict(logit_scale=0.0), dict(logit_scale=math.nan), dict(targets=[5] + [None] * 6),
                dict(targets=["cat"] + [None] * 6), dict(targets=[list(range(5)) * 4] + [None] * 6), dict(targets=good[:6])):
        args = dict(targets=good, chunk_rows=None, logit_scale=None)
        args.update(bad)
        with pytest.raises(ValueError):
            L.probe_rank(q, db, **args)
    with pytest.raises(ValueError):
        L.probe_rank(torch.randn(5, 8), db, good)  # widths differ
    with pytest.raises(ValueError):
        L.probe_rank(q, {"a": db, "b": torch.randn(3, 8)}, {"a": good})


def test_names_are_exported():
    for name in ("label_rank", "probe_rank", "LabelRanks"):
        assert name in semanticlens_amd.__all__
    assert semanticlens_amd.label_rank is L.label_rank and semanticlens_amd.probe_rank is L.probe_rank
    assert semanticlens_amd.LabelRanks is L.LabelRanks and callable(L.Lens.label_rank)
    assert "sl_rank_merge" in N.SIGNATURES and "sl_rank_merge_splits" in N.SIGNATURES


def test_label_ranks_helpers_on_cpu_tensors():
    nan = math.nan
    r = semanticlens_amd.LabelRanks(
        rank=torch.tensor([[7, 2], [-1, -1], [0, -1], [4, 0], [0, 9]]),          # two synonyms | no target | a NaN target | ...
        value=torch.tensor([[0.1, 0.2], [nan, nan], [nan, nan], [0.3, nan], [0.9, 0.1]]),
        targets=torch.tensor([[0, 9], [-1, -1], [1, -1], [5, 6], [2, 3]]), prob=None, log_z=None, n_labels=10)
    assert r.best().dtype == torch.int64 and r.best().tolist() == [2, -1, -1, 4, 0]  # row 3: its rank-0 target is NaN and left out
    assert r.hit(1).tolist() == [False, False, False, False, True]
    assert r.hit(3).tolist() == [True, False, False, False, True]
    assert r.hit(5).tolist() == [True, False, False, True, True]
    assert r.n_evaluated == 3
    assert r.topk_accuracy(1) == 1 / 3 and r.topk_accuracy(3) == 2 / 3 and r.topk_accuracy(10) == 1.0
    assert abs(r.mrr() - (1 / 3 + 1 / 5 + 1.0) / 3) < 1e-15
    assert r.logit_scale is None
    none = semanticlens_amd.LabelRanks(rank=torch.tensor([[-1]]), value=torch.tensor([[nan]]), targets=torch.tensor([[-1]]), prob=None,
                                       log_z=None, n_labels=10)
    assert none.n_evaluated == 0 and math.isnan(none.topk_accuracy(5)) and math.isnan(none.mrr()) and none.best().tolist() == [-1]
