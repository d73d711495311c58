"""K28 without a GPU: the rules of csrc/omp_state.hpp as a host program, the entry points' argument checks, the argument checks of
``decompose_components`` / ``probe_decompose`` before the text tower or a device is touched, and ``Decomposition.terms`` on CPU tensors."""
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


def test_state_rules_on_the_host(tmp_path):
    """csrc/omp_state.hpp compiled with g++: the Cholesky append and solve against a long double solve of the normal equations for
    random Gram matrices of unit vectors, t = 1..16, and every branch of the rule that picks a step's candidate on a table
    (tests/native/omp_state_check.cpp)."""
    exe = tmp_path / "omp_state_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe),
                    str(ROOT / "tests" / "native" / "omp_state_check.cpp")], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout


def _step(lib, **over):
    """``sl_omp_step`` with made-up, well-aligned pointers (never followed: every call here is refused before a launch)."""
    a = dict(x=16, C=3, D=8, w=16, V=5, cand_vals=16, cand_ids=16, k_cand=2, t=1, s=4, min_correlation=0.0, ids=16, chol=16, rhs=16,
             coefs=16, corr=16, explained=16, n_terms=16, finished=16, residual=16, last=16)
    assert set(over) <= set(a)
    a.update(over)
    return lib.sl_omp_step(a["x"], a["C"], a["D"], a["w"], a["V"], a["cand_vals"], a["cand_ids"], a["k_cand"], a["t"], a["s"],
                           a["min_correlation"], a["ids"], a["chol"], a["rhs"], a["coefs"], a["corr"], a["explained"], a["n_terms"],
                           a["finished"], a["residual"], a["last"], None)


def test_entry_points_check_arguments_without_a_device():
    lib = N.lib()
    assert N.OMP_MAX_TERMS == 16 and N.OMP_MIN_PIVOT == 1e-10 and N.OMP_RESIDUAL_DONE == 1e-8
    pointers = ("x", "w", "cand_vals", "cand_ids", "ids", "chol", "rhs", "coefs", "corr", "explained", "n_terms", "finished", "residual",
                "last")
    for name in pointers:
        assert _step(lib, **{name: None}) == -1 and lib.sl_last_error().startswith(b"sl_omp_step: null"), name
    for s in (0, 17, -1):
        assert _step(lib, s=s, t=0) == -1 and b"not in [1, 16]" in lib.sl_last_error()
    for t in (-1, 4, 5):
        assert _step(lib, t=t, k_cand=8) == -1 and b"not in [0, s" in lib.sl_last_error()
    assert _step(lib, t=2, k_cand=2) == -1 and b"at least t + 1 candidates" in lib.sl_last_error()
    assert _step(lib, k_cand=0, t=0) == -1 and b"at least t + 1 candidates" in lib.sl_last_error()
    for D in (0, -3):
        assert _step(lib, D=D) == -1 and b"at least one coordinate" in lib.sl_last_error()
    for bad in (-0.1, 1.0, math.nan, math.inf):
        assert _step(lib, min_correlation=bad) == -1 and b"min_correlation" in lib.sl_last_error()
    assert _step(lib, C=-1) == -1 and b"negative" in lib.sl_last_error()
    assert _step(lib, V=0) == -1 and b"empty vocabulary" in lib.sl_last_error()
    for name in ("cand_ids", "ids", "chol", "rhs", "coefs", "explained"):
        assert _step(lib, **{name: 12}) == -1 and b"8-byte aligned" in lib.sl_last_error(), name
    for name in ("x", "w", "cand_vals", "corr", "n_terms", "finished", "residual", "last"):
        assert _step(lib, **{name: 18}) == -1 and b"4-byte aligned" in lib.sl_last_error(), name
    assert _step(lib, C=0, **{name: None for name in pointers}) == 0  # C == 0: a no-op

    def init(x=16, C=3, D=8, s=4, ids=16, coefs=16, corr=16, explained=16, n_terms=16, finished=16, residual=16, last=16):
        return lib.sl_omp_init(x, C, D, s, ids, coefs, corr, explained, n_terms, finished, residual, last, None)

    for name in ("x", "ids", "coefs", "corr", "explained", "n_terms", "finished", "residual", "last"):
        assert init(**{name: None}) == -1 and lib.sl_last_error().startswith(b"sl_omp_init: null"), name
    assert init(s=0) == -1 and init(s=17) == -1 and b"not in [1, 16]" in lib.sl_last_error()
    assert init(D=0) == -1 and b"at least one coordinate" in lib.sl_last_error()
    assert init(C=-1) == -1
    assert init(ids=12) == -1 and b"8-byte aligned" in lib.sl_last_error()
    assert init(residual=18) == -1 and b"4-byte aligned" in lib.sl_last_error()
    assert lib.sl_omp_init(None, 0, 8, 4, None, None, None, None, None, None, None, None, None) == 0


def test_argument_helpers():
    assert N.check_omp_terms(1) == 1 and N.check_omp_terms(np.int64(16)) == 16
    for bad in (0, 17, -1, 1.5, "4", None, True):
        with pytest.raises(ValueError):
            N.check_omp_terms(bad)
    assert N.check_min_correlation(0) == 0.0 and N.check_min_correlation(0.25) == 0.25 and N.check_min_correlation(np.float32(0.5)) == 0.5
    for bad in (-0.1, 1.0, 1.5, math.nan, math.inf, -math.inf, "0.1", None, True):
        with pytest.raises(ValueError):
            N.check_min_correlation(bad)


class _FakeLens:
    def __init__(self, fm):
        self.fm = fm


VOCAB = ["cat", "dog", "fish", "dog"]


@pytest.mark.parametrize("kwargs", [
    dict(n_terms=0), dict(n_terms=17), dict(n_terms=1.5), dict(n_terms="4"),
    dict(min_correlation=-0.1), dict(min_correlation=1.0), dict(min_correlation=math.nan), dict(min_correlation=math.inf),
    dict(chunk_rows=0), dict(chunk_size=0), dict(chunk_size=-4),
    dict(vocabulary=[]), dict(vocabulary="word"),
])
def test_decompose_components_refuses_bad_arguments_before_anything_runs(kwargs):
    fm = FakeVLM(dim=16)
    args = dict(vocabulary=VOCAB, n_terms=4, min_correlation=0.0, chunk_rows=None, chunk_size=None)
    args.update(kwargs)
    db = torch.randn(7, 16)  # a CPU tensor: moving it would need a device
    for call in (lambda: L.decompose_components(fm, args["vocabulary"], db, n_terms=args["n_terms"], templates=["a {}"],
                                                chunk_size=args["chunk_size"], min_correlation=args["min_correlation"],
                                                chunk_rows=args["chunk_rows"]),
                 lambda: L.Lens.decompose_components(_FakeLens(fm), args["vocabulary"], db, args["n_terms"], ["a {}"], None,
                                                     args["chunk_size"], args["min_correlation"], args["chunk_rows"])):
        with pytest.raises(ValueError):
            call()
    assert fm.calls == {"encode_text": 0, "encode_image": 0}


def test_decompose_components_refuses_a_bad_db_before_anything_runs():
    fm = FakeVLM(dim=16)
    for bad in (torch.randn(16), {"a": torch.randn(3, 16), "b": torch.randn(2, 8)}, {"a": {"b": torch.randn(3, 16)}}):
        with pytest.raises(ValueError):
            L.decompose_components(fm, VOCAB, bad)
    assert fm.calls == {"encode_text": 0, "encode_image": 0}


def test_probe_decompose_refuses_bad_arguments():
    w, db = torch.randn(5, 16), torch.randn(7, 16)
    for bad in (dict(n_terms=0), dict(n_terms=17), dict(n_terms=1.5), dict(n_terms="4"), dict(min_correlation=-0.1),
                dict(min_correlation=1.0), dict(min_correlation=math.nan), dict(min_correlation=math.inf), dict(chunk_rows=0)):
        with pytest.raises(ValueError):
            L.probe_decompose(w, db, **bad)
    with pytest.raises(ValueError):
        L.probe_decompose(torch.randn(5, 8), db)  # widths differ
    with pytest.raises(ValueError):
        L.probe_decompose(torch.randn(0, 16), db)  # no words
    with pytest.raises(ValueError):
        L.probe_decompose(torch.randn(16), db)
    with pytest.raises(ValueError):
        L.probe_decompose({"a": w}, db)  # a dict where the word vectors belong
    with pytest.raises(ValueError):
        L.probe_decompose(w, {"a": db, "b": torch.randn(3, 8)})
    with pytest.raises(ValueError):
        N.decompose_probe(w, torch.randn(0, 16), 2)  # (x, w): an empty vocabulary, refused before a device is asked for


def test_names_are_exported():
    for name in ("decompose_components", "probe_decompose", "Decomposition"):
        assert name in semanticlens_amd.__all__
    assert semanticlens_amd.decompose_components is L.decompose_components and semanticlens_amd.probe_decompose is L.probe_decompose
    assert semanticlens_amd.Decomposition is L.Decomposition and callable(L.Lens.decompose_components)
    assert "sl_omp_init" in N.SIGNATURES and "sl_omp_step" in N.SIGNATURES
    assert N.lib().sl_abi_version() == 1
    makefile = (ROOT / "semanticlens_amd" / "csrc" / "Makefile").read_text()
    srcs = next(line for line in makefile.splitlines() if line.startswith("SRCS"))
    hdrs = next(line for line in makefile.splitlines() if line.startswith("HDRS"))
    assert "omp.hip" in srcs.split() and "omp_state.hpp" in hdrs.split()


def test_decomposition_terms_on_cpu_tensors():
    nan = math.nan
    dec = semanticlens_amd.Decomposition(
        ids=torch.tensor([[2, 0, -1], [1, -1, -1], [-1, -1, -1]]),
        coefs=torch.tensor([[0.75, 0.5, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64),
        correlation=torch.tensor([[0.8, 0.4, nan], [1.0, nan, nan], [nan, nan, nan]]),
        explained=torch.tensor([[0.64, 0.9, 0.9], [1.0, 1.0, 1.0], [nan, nan, nan]], dtype=torch.float64),
        n_terms=torch.tensor([2, 1, 0], dtype=torch.int32), residual=torch.zeros(3, 4))
    vocab = ["cat", "dog", "fish"]
    assert dec.terms(0, vocab) == [("fish", 0.75, 0.64), ("cat", 0.5, 0.9)]
    assert dec.terms(1, vocab) == [("dog", 1.0, 1.0)]
    assert dec.terms(2, vocab) == []
