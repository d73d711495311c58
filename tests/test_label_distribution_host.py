"""K25 without a GPU: the combine rule of csrc/softmax_state.hpp as a host program, ``check_logit_scale``, the argument checks of
``label_distribution`` / ``probe_softmax`` before the text tower or a device is touched, and ``LabelDistribution``'s helpers on
CPU tensors."""
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


def test_combine_rule_on_the_host(tmp_path):
    """csrc/softmax_state.hpp compiled with g++: the empty state is the identity, 10 000 random logits in shuffled groupings agree
    with a long double log-sum-exp and entropy within the derived bound, and NaN, +inf and "nothing above -inf" survive every
    merge order (tests/native/softmax_state_check.cpp)."""
    exe = tmp_path / "softmax_state_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe),
                    str(ROOT / "tests" / "native" / "softmax_state_check.cpp")], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout


def test_check_logit_scale():
    assert N.check_logit_scale(100) == 100.0 and isinstance(N.check_logit_scale(100), float)
    assert N.check_logit_scale(np.float32(2.5)) == 2.5
    for bad in (0, 0.0, -1, -100.0, math.inf, -math.inf, math.nan, "100", b"100", None, [100.0], 1e39, 1e-39):
        with pytest.raises(ValueError):
            N.check_logit_scale(bad)


def test_entry_points_check_arguments_without_a_device():
    lib = N.lib()
    assert lib.sl_softmax_init(None, 3, None) == -1 and lib.sl_last_error() == b"sl_softmax_init: null state"
    assert lib.sl_softmax_init(None, 0, None) == 0  # R == 0: a no-op
    assert lib.sl_softmax_init(None, -1, None) == -1
    for bad in (0.0, -2.0, math.inf, math.nan):
        assert lib.sl_softmax_merge(8, 2, 8, 4, 4, bad, None, 0, None) == -1
        assert b"logit scale" in lib.sl_last_error()
        assert lib.sl_softmax_finish(8, 2, bad, None, 0, None, 8, 8, None) == -1
    assert lib.sl_softmax_merge(8, 2, 8, 4, 0, 1.0, None, 0, None) == -1 and b"at least one column" in lib.sl_last_error()
    assert lib.sl_softmax_merge(8, 2, 8, 3, 4, 1.0, None, 0, None) == -1 and b"row stride" in lib.sl_last_error()
    assert lib.sl_softmax_merge(8, 2, None, 4, 4, 1.0, None, 0, None) == -1 and b"null candidate tile" in lib.sl_last_error()
    assert lib.sl_softmax_merge(8, 2, 6, 4, 4, 1.0, None, 0, None) == -1 and b"4-byte aligned" in lib.sl_last_error()
    assert lib.sl_softmax_merge(4, 2, 8, 4, 4, 1.0, None, 0, None) == -1 and b"8-byte aligned" in lib.sl_last_error()
    assert lib.sl_softmax_merge(None, 0, None, 4, 4, 1.0, None, 0, None) == 0
    assert lib.sl_softmax_finish(8, 2, 1.0, 8, 0, 8, 8, 8, None) == -1 and b"k = 0" in lib.sl_last_error()
    assert lib.sl_softmax_finish(8, 2, 1.0, 8, 1025, 8, 8, 8, None) == -1
    assert lib.sl_softmax_finish(8, 2, 1.0, None, 0, None, None, 8, None) == -1 and b"null log_z" in lib.sl_last_error()
    assert lib.sl_softmax_finish(8, 2, 1.0, 8, 3, None, 8, 8, None) == -1
    assert lib.sl_softmax_finish(None, 0, 1.0, None, 0, None, None, None, None) == 0
    assert lib.sl_softmax_merge_ws_bytes(0, 100) == 0 and lib.sl_softmax_merge_ws_bytes(5, 0) == 0
    assert lib.sl_softmax_merge_ws_bytes(100000, 341) == 0  # many rows of few columns: never split


@pytest.mark.parametrize("kwargs", [dict(k=0), dict(k=1025), dict(k=2.5), dict(k="3"), dict(vocabulary=[]), dict(vocabulary="word"),
                                    dict(chunk_size=0), dict(chunk_size=-4), dict(logit_scale=0), dict(logit_scale=-100.0),
                                    dict(logit_scale=math.inf), dict(logit_scale=math.nan), dict(logit_scale="100")])
def test_label_distribution_refuses_bad_arguments_before_anything_runs(kwargs):
    fm = FakeVLM(dim=16)
    args = dict(vocabulary=["cat", "dog", "fish"], k=2, logit_scale=100.0, chunk_size=None)
    args.update(kwargs)
    db = torch.randn(7, 16)  # a CPU tensor: moving it would need a device
    for call in (lambda: L.label_distribution(fm, args["vocabulary"], db, k=args["k"], logit_scale=args["logit_scale"],
                                              chunk_size=args["chunk_size"], templates=["a {}"]),
                 lambda: L.Lens.label_distribution(_FakeLens(fm), args["vocabulary"], {"a": db}, args["k"], args["logit_scale"],
                                                   ["a {}"], None, args["chunk_size"])):
        with pytest.raises(ValueError):
            call()
    assert fm.calls == {"encode_text": 0, "encode_image": 0}


class _FakeLens:
    def __init__(self, fm):
        self.fm = fm


def test_probe_softmax_refuses_bad_arguments():
    q, db = torch.randn(5, 16), torch.randn(7, 16)
    for bad in (dict(k=0), dict(logit_scale=0.0), dict(logit_scale=math.nan), dict(chunk_rows=0)):
        args = dict(k=2, logit_scale=100.0, chunk_rows=None)
        args.update(bad)
        with pytest.raises(ValueError):
            L.probe_softmax(q, db, **args)
    with pytest.raises(ValueError):
        L.probe_softmax(torch.randn(5, 8), db, 2)  # widths differ
    with pytest.raises(ValueError):
        L.probe_softmax(q, {"a": db, "b": torch.randn(3, 8)}, 2)


def test_label_distribution_helpers_on_cpu_tensors():
    nan = math.nan
    dist = semanticlens_amd.LabelDistribution(
        values=torch.tensor([[0.3, 0.2], [0.3, 0.29], [nan, nan]]), ids=torch.tensor([[4, 1], [0, 2], [3, 5]]),
        probs=torch.tensor([[0.9, 0.05], [0.5, 0.2], [nan, nan]]), log_z=torch.tensor([1.0, 2.0, nan], dtype=torch.float64),
        entropy=torch.tensor([0.0, math.log(3.0), nan], dtype=torch.float64), n_labels=10, logit_scale=100.0)
    eff = dist.effective_labels
    assert eff.dtype == torch.float64 and float(eff[0]) == 1.0 and abs(float(eff[1]) - 3.0) < 1e-12 and math.isnan(float(eff[2]))
    assert dist.confident().tolist() == [True, True, False]  # the default 0.5 is inclusive; a NaN row is never confident
    assert dist.confident(min_prob=0.6).tolist() == [True, False, False]
    assert dist.confident(min_prob=0.0).tolist() == [True, True, False]
    assert semanticlens_amd.label_distribution is L.label_distribution and semanticlens_amd.probe_softmax is L.probe_softmax
