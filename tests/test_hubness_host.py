"""K29 without a GPU: the entry point and its refusals, the score rule of csrc/biased_score.hpp as a host program under both
contraction settings against numpy's fp32 arithmetic, the argument checks of ``label_components_csls`` / ``probe_csls`` before the
text tower or a device is touched, and ``HubnessLabels`` on CPU tensors."""
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


def test_names_are_exported():
    header = (ROOT / "include" / "semanticlens_amd.h").read_text()
    assert "int sl_topk_merge_biased(float* d_vals, int64_t* d_ids, int64_t R, int64_t k, const float* d_cand" in header
    assert "sl_topk_merge_biased" in N.SIGNATURES and callable(N.lib().sl_topk_merge_biased)
    assert N.lib().sl_abi_version() == 1
    for name in ("label_components_csls", "probe_csls", "HubnessLabels"):
        assert name in semanticlens_amd.__all__
    assert semanticlens_amd.probe_csls is L.probe_csls and semanticlens_amd.label_components_csls is L.label_components_csls
    assert semanticlens_amd.HubnessLabels is L.HubnessLabels and callable(L.Lens.label_components_csls)
    makefile = (ROOT / "semanticlens_amd" / "csrc" / "Makefile").read_text()
    hdrs = next(line for line in makefile.splitlines() if line.startswith("HDRS"))
    assert "biased_score.hpp" in hdrs.split()


def test_score_rule_on_the_host_under_both_contraction_settings(tmp_path):
    """csrc/biased_score.hpp compiled with g++ with and without contraction (tests/native/biased_score_check.cpp prints the bits of
    the score for every triple of its operand table: +-0.0, +-inf, NaN, denormals, cancellations): the two builds agree line by
    line, and every line equals ``np.float32(np.float32(2 * c - r) - q)``."""
    outputs = []
    for flag in ("-ffp-contract=off", "-ffp-contract=fast"):
        exe = tmp_path / f"biased_score_check{flag[-4:].strip('=')}"
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", flag, "-o", str(exe),
                        str(ROOT / "tests" / "native" / "biased_score_check.cpp")], check=True)
        res = subprocess.run([str(exe)], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        outputs.append(res.stdout)
    assert outputs[0] == outputs[1], "the contracted and the two-step form differ"
    table = np.array([[int(word, 16) for word in line.split()] for line in outputs[0].splitlines()], dtype=np.uint32)
    assert table.shape[1] == 4 and table.shape[0] >= 20 ** 3
    c, r, q = (table[:, i].copy().view(np.float32) for i in range(3))
    for needed in (0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x00000001, 0x007FFFFF):
        assert (table[:, 0] == needed).any() and (table[:, 1] == needed).any() and (table[:, 2] == needed).any()
    with np.errstate(invalid="ignore", over="ignore"):
        want = ((np.float32(2.0) * c - r).astype(np.float32) - q).astype(np.float32)
    got = table[:, 3].copy().view(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)  # a NaN's payload and sign are not part of the rule
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    inf_minus_inf = (table[:, 0] == 0x7F800000) & (table[:, 1] == 0x7F800000)
    assert inf_minus_inf.any() and nan[inf_minus_inf].all()


def _merge(lib, **over):
    """``sl_topk_merge_biased`` with made-up, well-aligned pointers (never followed: every call here is refused before a launch,
    or is a no-op)."""
    a = dict(vals=16, ids=16, R=3, k=5, cand=16, ld=8, B=8, id_base=0, row_bias=16, col_bias=16, ws=None, ws_bytes=0)
    assert set(over) <= set(a)
    a.update(over)
    return lib.sl_topk_merge_biased(a["vals"], a["ids"], a["R"], a["k"], a["cand"], a["ld"], a["B"], a["id_base"], a["row_bias"],
                                    a["col_bias"], a["ws"], a["ws_bytes"], None)


def test_entry_point_refuses_in_k17s_order_without_a_device():
    lib = N.lib()
    err = lib.sl_last_error
    for k in (0, 1025, -1):
        assert _merge(lib, k=k, B=0, cand=None, row_bias=None) == -1 and b"not in [1, 1024]" in err()  # the state comes first
    assert _merge(lib, R=-1) == -1 and b"negative row count" in err()
    assert _merge(lib, B=0, id_base=-1, row_bias=None) == -1 and b"at least one column" in err()  # then the tile's shape
    assert _merge(lib, ld=7, id_base=-1) == -1 and b"row stride" in err()
    assert _merge(lib, id_base=-1, vals=None) == -1 and b"id_base" in err()  # then the ids
    assert _merge(lib, id_base=(1 << 62) - 7) == -1 and b"id_base" in err()
    assert _merge(lib, R=0, vals=None, ids=None, cand=None, row_bias=None, col_bias=None) == 0  # R == 0: a no-op before any pointer
    assert _merge(lib, vals=None, row_bias=None) == -1 and b"null state" in err()  # then the pointers
    assert _merge(lib, cand=None, row_bias=None) == -1 and b"null candidate tile" in err()
    assert _merge(lib, cand=18) == -1 and b"4-byte aligned" in err()
    for name in ("row_bias", "col_bias"):
        assert _merge(lib, **{name: None}) == -1 and b"sl_topk_merge_biased: null bias vector" in err(), name
        assert _merge(lib, **{name: 18}) == -1 and b"bias vector is not 4-byte aligned" in err(), name
    # the unbiased entry point keeps its texts
    assert lib.sl_topk_merge(None, None, 3, 5, 16, 8, 8, 0, None, 0, None) == -1 and err() == b"sl_topk_merge: null state"


def test_argument_helpers():
    assert N.check_neighbours(1) == 1 and N.check_neighbours(np.int64(1024)) == 1024 and N.check_neighbours(10) == 10
    for bad in (0, 1025, -1, 2.5, "3", None):
        with pytest.raises(ValueError):
            N.check_neighbours(bad)
    inf, nan = math.inf, math.nan
    vals = torch.tensor([[0.5, 0.25, -inf], [1.0, -inf, -inf], [-inf, -inf, -inf], [nan, 0.5, 0.25], [-inf, -inf, -inf]])
    ids = torch.tensor([[4, 1, -1], [0, -1, -1], [-1, -1, -1], [2, 0, 1], [3, 1, -1]])  # the last row: two real -inf candidates
    got = N.topk_density(vals, ids)
    assert got.dtype == torch.float32 and tuple(got.shape) == (5,)
    assert got[:2].tolist() == [0.375, 1.0] and math.isnan(got[2]) and math.isnan(got[3]) and got[4] == -inf
    third = torch.tensor([[1 / 3, 1 / 3 + 2 ** -24, 1.0]], dtype=torch.float32)
    want = np.float32(third.double().sum().item() / 3)  # the float64 mean, rounded once
    assert N.topk_density(third, torch.tensor([[0, 1, 2]])).item() == want
    assert tuple(N.topk_density(torch.empty(0, 4), torch.empty(0, 4, dtype=torch.int64)).shape) == (0,)


class _FakeLens:
    def __init__(self, fm):
        self.fm = fm


VOCAB = ["cat", "dog", "fish", "dog"]


@pytest.mark.parametrize("kwargs", [
    dict(neighbours=0), dict(neighbours=1025), dict(neighbours=2.5), dict(neighbours="3"),
    dict(k=0), dict(k=1025), dict(k=1.5), dict(k="5"),
    dict(chunk_rows=0), dict(chunk_size=0), dict(chunk_size=-4),
    dict(vocabulary=[]), dict(vocabulary="word"),
])
def test_label_components_csls_refuses_bad_arguments_before_anything_runs(kwargs):
    fm = FakeVLM(dim=16)
    args = dict(vocabulary=VOCAB, k=5, neighbours=10, chunk_rows=None, chunk_size=None)
    args.update(kwargs)
    db = torch.randn(7, 16)  # a CPU tensor: moving it would need a device
    for call in (lambda: L.label_components_csls(fm, args["vocabulary"], db, k=args["k"], neighbours=args["neighbours"],
                                                 templates=["a {}"], chunk_size=args["chunk_size"], chunk_rows=args["chunk_rows"]),
                 lambda: L.Lens.label_components_csls(_FakeLens(fm), args["vocabulary"], db, args["k"], args["neighbours"], ["a {}"],
                                                      None, args["chunk_size"], args["chunk_rows"])):
        with pytest.raises(ValueError):
            call()
    assert fm.calls == {"encode_text": 0, "encode_image": 0}


def test_label_components_csls_refuses_a_bad_db_before_anything_runs():
    fm = FakeVLM(dim=16)
    for bad in (torch.randn(16), {"a": torch.randn(3, 16), "b": torch.randn(2, 8)}, {"a": {"b": torch.randn(3, 16)}}):
        with pytest.raises(ValueError):
            L.label_components_csls(fm, VOCAB, bad)
    assert fm.calls == {"encode_text": 0, "encode_image": 0}


def test_probe_csls_refuses_bad_arguments():
    w, db = torch.randn(5, 16), torch.randn(7, 16)
    for bad in (dict(neighbours=0), dict(neighbours=1025), dict(neighbours=2.5), dict(neighbours="3"), dict(k=0), dict(k=1025),
                dict(k=2.5), dict(chunk_rows=0)):
        with pytest.raises(ValueError):
            L.probe_csls(w, db, **bad)
    with pytest.raises(ValueError):
        L.probe_csls(torch.randn(5, 8), db)  # widths differ
    with pytest.raises(ValueError):
        L.probe_csls(torch.randn(0, 16), db)  # no words
    with pytest.raises(ValueError):
        L.probe_csls(torch.randn(16), db)
    with pytest.raises(ValueError):
        L.probe_csls({"a": w}, db)  # a dict where the word vectors belong
    with pytest.raises(ValueError):
        L.probe_csls(w, {"a": db, "b": torch.randn(3, 8)})
    for bad in (dict(neighbours=0), dict(k=0), dict(chunk_rows=0)):
        with pytest.raises(ValueError):
            N.csls_probe(db, w, **{"k": 5, **bad})
    with pytest.raises(ValueError):
        N.csls_probe(db, torch.randn(5, 8), 5)


def test_hubness_labels_on_cpu_tensors():
    inf, nan = math.inf, math.nan
    r = torch.tensor([0.5, 0.25, 0.75], dtype=torch.float32)
    q = torch.tensor([0.125, 0.875, 0.5, 0.875, nan], dtype=torch.float32)
    ids = torch.tensor([[2, 0, -1], [1, 3, 4], [-1, -1, -1]])
    cos = torch.tensor([[0.75, 0.5, 0.0], [0.875, 0.8125, 0.25], [0.0, 0.0, 0.0]], dtype=torch.float32)
    values = (2 * cos - r[:, None]) - q[ids.clamp(min=0)]  # exact: every operand is a multiple of 1/16
    values[ids < 0] = -inf
    hl = semanticlens_amd.HubnessLabels(values=values, ids=ids, component_density=r, label_density=q, neighbours=10)
    got = hl.cosine
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3)
    assert got[0, :2].tolist() == [0.75, 0.5] and got[1, :2].tolist() == [0.875, 0.8125]
    assert math.isnan(got[1, 2])  # a NaN density: the score was NaN, and so is what is recovered from it
    assert torch.isnan(got[ids < 0]).all() and int(torch.isnan(got).sum()) == 5  # unused slots
    # the recovery in float64, rounded once: a score that is not exactly 2 c - r - q comes back within 2^-23 + 2^-25
    c = np.float32(0.3333333)
    score = np.float32(np.float32(2 * c - np.float32(0.1)) - np.float32(0.7))
    one = semanticlens_amd.HubnessLabels(torch.tensor([[score]]), torch.tensor([[0]]), torch.tensor([0.1]), torch.tensor([0.7]), 3)
    want = np.float32((np.float64(score) + np.float64(np.float32(0.1)) + np.float64(np.float32(0.7))) / 2)
    assert one.cosine.item() == want and abs(float(want) - float(c)) <= 2.0 ** -23 + 2.0 ** -25
    # the hubs: largest density first, NaN before every number, equal densities by the smaller id
    hv, hi = hl.hubs(4)
    assert hi.tolist() == [4, 1, 3, 2] and math.isnan(hv[0]) and hv[1:].tolist() == [0.875, 0.875, 0.5]
    assert hl.hubs()[1].tolist() == [4, 1, 3, 2, 0] and hl.hubs(0)[1].tolist() == []
    with pytest.raises(ValueError):
        hl.hubs(-1)
