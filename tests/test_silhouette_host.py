"""K23 host side (no GPU): the silhouette ABI is declared, ``sl_silhouette`` refuses bad arguments before any launch,
``_native.silhouette``, the ``scores`` functions and ``polysemanticity_facets(n_clusters="auto")`` raise ``ValueError`` for
what the host can see without touching a device, and a ``Facets`` built without the new fields still works."""
from __future__ import annotations

import re
from pathlib import Path

import pytest
import torch

import semanticlens_amd
from semanticlens_amd import _native as N
from semanticlens_amd import lens as L
from semanticlens_amd import scores as S

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("sl_silhouette_ws_bytes", "sl_silhouette")


def _err():
    return N.lib().sl_last_error().decode()


def test_silhouette_symbols_declared():
    header = (ROOT / "include" / "semanticlens_amd.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)  # prototypes only
    for name in NAMES:
        proto = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", header)
        assert proto, f"{name} is not declared in the header"
        assert name in N.SIGNATURES, f"{name} is not in _native.SIGNATURES"
        assert len(proto.group(1).split(",")) == len(N.SIGNATURES[name][1]), f"{name}: argument counts differ"
        assert hasattr(N.lib(), name)
    assert re.search(r"^SRCS :=.*\bsilhouette\.hip\b", (ROOT / "semanticlens_amd" / "csrc" / "Makefile").read_text(), re.M)
    assert N.lib().sl_abi_version() == 1  # the change is additive
    assert callable(N.silhouette)
    for name in ("silhouette_samples", "silhouette_score"):
        assert name in semanticlens_amd.__all__ and getattr(semanticlens_amd, name) is getattr(S, name)


def test_sl_silhouette_argument_errors_before_launch():
    sil = N.lib().sl_silhouette
    buf = torch.zeros(1 << 16)  # host memory: never dereferenced, every call must fail on its arguments
    p, big = buf.data_ptr(), 1 << 30
    # (V, C, n, D, labels, m, n_clusters, metric, samples, mean, ws, ws_bytes, stream)
    assert sil(None, 3, 5, 8, p, 1, 2, 0, p, p, p, big, None) == -1  # V
    assert "null pointer" in _err()
    assert sil(p, 3, 5, 8, None, 1, 2, 0, p, p, p, big, None) == -1  # labels
    assert "null pointer" in _err()
    assert sil(p, 3, 5, 8, p, 1, 2, 0, p, None, p, big, None) == -1  # mean (samples may be null, mean may not)
    assert "null pointer" in _err()
    assert sil(p, 3, 5, 8, p, 1, 2, 0, None, p, None, big, None) == -1  # workspace
    assert "workspace" in _err()
    need = N.lib().sl_silhouette_ws_bytes(3, 5, 8)
    assert need >= 3 * 5 * 5 * 8
    assert sil(p, 3, 5, 8, p, 1, 2, 0, None, p, p, need - 1, None) == -1
    assert "workspace" in _err() and str(need - 1) in _err()
    assert sil(p, 3, 1025, 8, p, 1, 2, 0, p, p, p, big, None) == -1
    assert "n_samples=1025" in _err()
    assert sil(p, 3, 1, 8, p, 1, 2, 0, p, p, p, big, None) == -1
    assert "n_samples=1" in _err()
    assert sil(p, 3, 5, 0, p, 1, 2, 0, p, p, p, big, None) == -1
    assert "D=0" in _err()
    for m in (0, 16):
        assert sil(p, 3, 5, 8, p, m, 2, 0, p, p, p, big, None) == -1
        assert f"m={m}" in _err()
    for k in (1, 17):
        assert sil(p, 3, 5, 8, p, 1, k, 0, p, p, p, big, None) == -1
        assert f"n_clusters={k}" in _err()
    for metric in (-1, 2):
        assert sil(p, 3, 5, 8, p, 1, 2, metric, p, p, p, big, None) == -1
        assert f"metric={metric}" in _err()
    assert sil(p, 65536, 5, 8, p, 1, 2, 0, p, p, p, big, None) == -1
    assert "65536" in _err()
    assert sil(p, -1, 5, 8, p, 1, 2, 0, p, p, p, big, None) == -1
    assert "negative" in _err()
    assert sil(None, 0, 5, 8, None, 1, 2, 0, None, None, None, 0, None) == 0  # C == 0: success, no launch


def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(N, "_f32c", no_device)
    monkeypatch.setattr(N, "to_device", no_device)


def test_native_silhouette_argument_errors_without_a_device(monkeypatch):
    _no_device(monkeypatch)
    V = torch.zeros(2, 5, 4)
    lab = torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match="n_samples=1025"):
        N.silhouette(torch.zeros(1, 1025, 4), torch.zeros(1, 1025, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="n_samples=1"):
        N.silhouette(torch.zeros(2, 1, 4), torch.zeros(2, 1, dtype=torch.int32), 2)
    for k in (1, 17, 2.0, True):
        with pytest.raises(ValueError, match="n_clusters"):
            N.silhouette(V, lab, k)
    with pytest.raises(ValueError, match="m=16"):
        N.silhouette(V, torch.zeros(16, 2, 5, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="labels"):  # shape: samples do not match
        N.silhouette(V, torch.zeros(2, 4, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="labels"):  # shape: components do not match
        N.silhouette(V, torch.zeros(3, 3, 5, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="labels"):  # shape: one axis too many
        N.silhouette(V, torch.zeros(1, 1, 2, 5, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="labels"):  # V is not (C, n, D)
        N.silhouette(torch.zeros(5, 4), lab, 2)
    for dtype in (torch.int64, torch.float32):
        with pytest.raises(ValueError, match="int32"):
            N.silhouette(V, lab.to(dtype), 2)
    for metric in ("manhattan", "", None, 0):
        with pytest.raises(ValueError, match="metric"):
            N.silhouette(V, lab, 2, metric=metric)
    with pytest.raises(ValueError, match="D=0"):
        N.silhouette(torch.zeros(2, 5, 0), lab, 2)


def test_scores_argument_errors_without_a_device(monkeypatch):
    _no_device(monkeypatch)
    V = torch.zeros(2, 5, 4)
    lab = torch.zeros(2, 5, dtype=torch.int32)
    for fn in (S.silhouette_samples, S.silhouette_score):
        with pytest.raises(ValueError, match="metric"):
            fn(V, lab, metric="l1")
        with pytest.raises(ValueError, match="int32"):
            fn(V, lab.long())
        with pytest.raises(ValueError, match="labels"):
            fn(V, lab[:, :4])
        with pytest.raises(ValueError, match="n_samples=1025"):
            fn(torch.zeros(1, 1025, 4), torch.zeros(1, 1025, dtype=torch.int32))
        with pytest.raises(ValueError, match="m=16"):
            fn(V, torch.zeros(16, 2, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="n_samples=2"):
        S.polysemanticity_facets(torch.zeros(2, 2, 4), n_clusters="auto")
    for bad in (1, 17, 0, 2.5):
        with pytest.raises(ValueError, match="max_clusters"):
            S.polysemanticity_facets(V, n_clusters="auto", max_clusters=bad)
    with pytest.raises(ValueError, match="metric"):
        S.polysemanticity_facets(V, n_clusters="auto", metric="l1")
    with pytest.raises(ValueError, match="auto"):
        S.polysemanticity_facets(V, n_clusters="automatic")
    with pytest.raises(ValueError, match="n_components"):
        S.polysemanticity_facets(torch.zeros(3, 4), n_clusters="auto")
    with pytest.raises(ValueError, match="max_clusters"):  # Lens.eval_facets forwards "auto" and the keywords
        L.Lens.eval_facets(L.Lens.__new__(L.Lens), V, n_clusters="auto", max_clusters=17)


def test_hand_made_facets_without_the_new_fields():
    labels = torch.tensor([[0, 1, 1, 0, 1], [1, 1, 1, 1, 1]], dtype=torch.int32)
    counts = torch.tensor([[2, 3], [0, 5]], dtype=torch.int32)
    f = S.Facets(score=torch.zeros(2, dtype=torch.float64), labels=labels, counts=counts, centers=torch.ones(2, 2, 4),
                 clarity=torch.full((2, 2), 0.5))
    assert f.n_facets is None and f.silhouette is None
    assert f.n_clusters == 2 and tuple(f.aggregated().shape) == (4, 4)
    assert f.members(1).tolist() == [[False, True, True, False, True], [True] * 5]
    comp, facet = f.decode(torch.tensor([3, -1, 0]))
    assert comp.tolist() == [1, -1, 0] and facet.tolist() == [1, -1, 0]
    positional = S.Facets(f.score, f.labels, f.counts, f.centers, f.clarity)
    assert positional.n_facets is None and positional.silhouette is None
    g = S.Facets(f.score, f.labels, f.counts, f.centers, f.clarity, n_facets=torch.tensor([2, 1], dtype=torch.int32),
                 silhouette=torch.zeros(2, 1, dtype=torch.float64))
    assert g.n_facets.tolist() == [2, 1] and g.n_clusters == 2
