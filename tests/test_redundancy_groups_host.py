"""K24 host side (no GPU): the new sl_* entry points are declared with the argument counts the binding uses, argument errors come
back before any launch, csrc/unionfind.hpp holds its rule under eight host threads, ``upper_tile_walk`` covers every pair of
the upper triangle once, the ``RedundancyGroups`` helpers are right on hand-written CPU tensors, and the public calls check their
arguments before they touch a device."""
from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import pytest
import torch

import semanticlens_amd
from semanticlens_amd import _native as N
from semanticlens_amd import lens as L
from semanticlens_amd import scores as S

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("sl_unionfind_init", "sl_threshold_union_merge", "sl_unionfind_flatten", "sl_group_min_merge", "sl_group_min_finish")


def _err():
    return N.lib().sl_last_error().decode()


def test_abi_surface():
    header = (ROOT / "include" / "semanticlens_amd.h").read_text()
    for name in NAMES:
        decl = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", header)
        assert decl, f"{name} is not declared in the header"
        assert name in N.SIGNATURES, f"{name} is not in _native.SIGNATURES"
        assert len(N.SIGNATURES[name][1]) == len(decl.group(1).split(",")), f"{name}: argument counts differ"
        assert hasattr(N.lib(), name)
    assert "reference scores.py:51-81" in header
    assert N.lib().sl_abi_version() == 1
    makefile = (ROOT / "semanticlens_amd" / "csrc" / "Makefile").read_text()
    assert "redgroups.hip" in makefile and "unionfind.hpp" in makefile


def test_merge_argument_errors_before_launch():
    merge = N.lib().sl_threshold_union_merge
    # (parent, degree, status, n, cand, ld, R, B, row_id_base, col_id_base, threshold, stream)
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert merge(None, None, None, 100, None, 8, 4, 8, 0, 0, bad, None) == -1
        assert "not finite" in _err()
    assert merge(None, None, None, -1, None, 8, 4, 8, 0, 0, 0.5, None) == -1
    assert merge(None, None, None, 1 << 31, None, 8, 4, 8, 0, 0, 0.5, None) == -1
    assert "2^31 - 1" in _err()
    assert merge(None, None, None, 100, None, 8, -4, 8, 0, 0, 0.5, None) == -1
    assert "negative" in _err()
    assert merge(None, None, None, 100, None, 7, 4, 8, 0, 0, 0.5, None) == -1
    assert "row stride" in _err()
    assert merge(None, None, None, 100, None, 8, 4, 8, 97, 0, 0.5, None) == -1
    assert "row ids" in _err()
    assert merge(None, None, None, 100, None, 8, 4, 8, -1, 0, 0.5, None) == -1
    assert "row ids" in _err()
    assert merge(None, None, None, 100, None, 8, 4, 8, 0, 93, 0.5, None) == -1
    assert "column ids" in _err()
    assert merge(None, None, None, 100, None, 8, 4, 8, 0, 0, 0.5, None) == -1
    assert "null candidate" in _err()
    # wholly below the diagonal, or empty: a no-op before the state is looked at
    assert merge(None, None, None, 100, ctypes_ptr(16), 8, 4, 8, 50, 0, 0.5, None) == 0
    assert merge(None, None, None, 100, ctypes_ptr(16), 8, 4, 8, 7, 0, 0.5, None) == 0  # last column id 7 == first row id
    assert merge(None, None, None, 100, None, 8, 0, 8, 0, 0, 0.5, None) == 0
    assert merge(None, None, None, 100, ctypes_ptr(16), 8, 4, 8, 6, 0, 0.5, None) == -1  # one element above the diagonal
    assert "null state" in _err()
    assert merge(None, None, None, 100, ctypes_ptr(18), 8, 4, 8, 0, 0, 0.5, None) == -1
    assert "4-byte aligned" in _err()


def ctypes_ptr(address: int):
    """A non-null pointer value for calls that must return before they use it."""
    return ctypes.c_void_p(address)


def test_other_entry_points_argument_errors():
    lib = N.lib()
    assert lib.sl_unionfind_init(None, None, None, 4, None) == -1
    assert "null state" in _err()
    assert lib.sl_unionfind_init(None, None, None, -1, None) == -1
    assert lib.sl_unionfind_flatten(None, 0, None, None) == 0
    assert lib.sl_unionfind_flatten(None, 5, None, None) == -1
    assert "null state" in _err()
    assert lib.sl_unionfind_flatten(None, 1 << 31, None, None) == -1
    assert lib.sl_group_min_merge(None, None, 100, None, 8, 4, 8, 0, 93, None) == -1
    assert "column ids" in _err()
    assert lib.sl_group_min_merge(None, None, 100, ctypes_ptr(16), 8, 4, 8, 50, 0, None) == 0
    assert lib.sl_group_min_merge(None, None, 100, ctypes_ptr(16), 8, 4, 8, 0, 0, None) == -1
    assert "null state" in _err()
    assert lib.sl_group_min_finish(None, None, 0, None, None) == 0
    assert lib.sl_group_min_finish(None, None, 3, None, None) == -1
    assert "null pointer" in _err()


def test_unionfind_header_on_the_host(tmp_path):
    """csrc/unionfind.hpp over std::atomic<int32_t>: eight threads unite a sparse random graph on 10 000 ids, a 1 000-clique, a
    5 000-chain in reverse order and an empty list; after a flatten the labels equal a sequential union-find's and
    parent[x] <= x held after every phase (tests/native/unionfind_check.cpp)."""
    exe = tmp_path / "unionfind_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-o", str(exe),
                    str(ROOT / "tests" / "native" / "unionfind_check.cpp")], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "failures=0" in res.stdout


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 1031])
@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (64, 1024), "n", (129, 1500)])
def test_upper_tile_walk(n, shape):
    rows, cols = (n, n) if shape == "n" else shape
    seen = torch.zeros((n, n), dtype=torch.int32)
    for r0, nr, c0, nc in N.upper_tile_walk(n, rows, cols):
        assert 0 <= r0 and 1 <= nr <= rows and r0 + nr <= n
        assert 0 <= c0 and 1 <= nc <= -(-cols // 4) * 4 and c0 + nc <= n
        assert c0 % 4 == 0, "a rectangle starts off a multiple of 4"
        assert c0 + nc - 1 > r0, "a rectangle lies wholly below the diagonal"
        seen[r0 : r0 + nr, c0 : c0 + nc] += 1
    upper = torch.triu(torch.ones((n, n), dtype=torch.bool), diagonal=1)
    assert (seen[upper] == 1).all(), "a pair i < j is not covered exactly once"
    assert int(seen.max()) <= 1


def _hand_made():
    """Ten components: {0, 3, 4, 8} (a path 0 - 3 - 4 - 8 plus 0 - 4), {1, 6} and {5, 7, 9} (a triangle); 2 is alone."""
    labels = torch.tensor([0, 1, 2, 0, 0, 5, 1, 5, 0, 5], dtype=torch.int64)
    degree = torch.tensor([2, 1, 0, 2, 3, 2, 1, 2, 1, 2], dtype=torch.int32)
    return S.RedundancyGroups(labels=labels, degree=degree)


def test_groups_helpers_on_hand_made_results():
    g = _hand_made()
    assert g.cohesion is None
    assert g.sizes.tolist() == [4, 2, 1, 4, 4, 3, 2, 3, 4, 3] and g.sizes.dtype == torch.int64
    assert g.n_groups == 4 and isinstance(g.n_groups, int)
    assert g.redundant.tolist() == [True, True, False, True, True, True, True, True, True, True] and g.redundant.dtype == torch.bool
    assert g.members(4).tolist() == [0, 3, 4, 8] and g.members(0).tolist() == [0, 3, 4, 8]
    assert g.members(2).tolist() == [2] and g.members(9).tolist() == [5, 7, 9] and g.members(6).tolist() == [1, 6]
    # by degree: group 0 -> 4 (degree 3); group 1 -> a tie between 1 and 6, the smaller id; 2; group 5 -> a three-way tie, 5
    assert g.representatives().tolist() == [4, 1, 2, 5]
    assert g.representatives(by="degree").tolist() == [4, 1, 2, 5]
    assert g.representatives(by="label").tolist() == [0, 1, 2, 5]
    with pytest.raises(ValueError, match="by="):
        g.representatives(by="size")
    db = torch.arange(10, dtype=torch.float32)[:, None] * torch.ones(1, 3)
    assert g.prune(db).tolist() == [[4.0] * 3, [1.0] * 3, [2.0] * 3, [5.0] * 3]


def test_groups_helpers_on_trivial_results():
    empty = S.RedundancyGroups(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    assert empty.n_groups == 0 and empty.sizes.shape == (0,) and empty.representatives().shape == (0,)
    assert empty.prune(torch.zeros(0, 4)).shape == (0, 4)
    one = S.RedundancyGroups(torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.tensor([float("nan")]))
    assert one.n_groups == 1 and one.sizes.tolist() == [1] and one.representatives().tolist() == [0] and one.members(0).tolist() == [0]
    assert not one.redundant.any()


def test_api_exists():
    assert semanticlens_amd.redundancy_groups is S.redundancy_groups
    assert semanticlens_amd.RedundancyGroups is S.RedundancyGroups
    assert "redundancy_groups" in semanticlens_amd.__all__ and "RedundancyGroups" in semanticlens_amd.__all__
    assert callable(L.Lens.eval_redundancy_groups) and callable(N.redundancy_probe)


def test_argument_errors_without_a_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(N, "_f32c", no_device)
    monkeypatch.setattr(N, "unionfind_new", no_device)
    db = torch.zeros(4, 16)
    for bad in (float("nan"), float("inf"), float("-inf"), "high", None):
        with pytest.raises(ValueError, match="finite"):
            S.redundancy_groups(db, threshold=bad)
        with pytest.raises(ValueError, match="finite"):
            N.redundancy_probe(db, bad)
    with pytest.raises(ValueError, match="n_components"):
        S.redundancy_groups(torch.zeros(4, 3, 16))
    with pytest.raises(ValueError, match="2-D"):
        N.redundancy_probe(torch.zeros(16), 0.5)
    with pytest.raises(ValueError, match="chunk_rows"):
        S.redundancy_groups(db, chunk_rows=0)
    with pytest.raises(ValueError, match="chunk_cols"):
        S.redundancy_groups(db, chunk_cols=-3)
    with pytest.raises(ValueError, match="finite"):
        L.Lens.__new__(L.Lens).eval_redundancy_groups({"l1": db}, threshold=float("nan"))  # needs no foundation model


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the error raised where there is no HIP device")
def test_no_cpu_fallback():
    with pytest.raises(N.NativeLibraryError, match="HIP device"):
        S.redundancy_groups(torch.zeros(4, 16), threshold=0.5)
