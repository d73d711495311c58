"""K9 bit-equality check: this tree's k-means (csrc/kmeans.hip) against a tree of another commit (``--parent-tree``: a checkout
with its library built).  Each tree runs in a child process of its own, because the two libraries export the same names.

A child clusters every case below through ``_native.poly2means(..., labels=...)`` (score, labels) and once more through the entry
point that call dispatches to (score, labels, min_count: ``poly2means`` does not hand the count out), checks that the two agree,
and dumps the arrays.  The parent process compares the dumps with ``np.array_equal(..., equal_nan=True)``.

One named exception: an all-duplicate component (every sample the same) at k = 2, n <= 128, ``replace_empty_clusters=False``.
The LDS kernel used to move a point into the empty cluster there where scikit-learn's relocation returns early; labels and
min_count must still be equal and both scores within 1e-9 of 0.  These components are listed separately; the set is found from
the inputs, not from the outputs.

    python tools/k9_ab.py --parent-tree DIR [--out profiles/k9_unify_ab.txt]
"""
from __future__ import annotations

import argparse
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def cases():
    """(C, n, D, k, n_init, kind, replace_empty_clusters), C <= 64."""
    out = []
    for n in (2, 3, 63, 64, 65, 127, 128, 129, 150):  # k = 2: lane-stride edges, the LDS limit, the general kernel at k = 2
        C = 32 if n <= 65 else 12
        for kind in ("random", "dup"):
            for rep in (True, False):
                out.append((C, n, 16, 2, 10, kind, rep))
    for n in (20, 64, 128, 150):
        for kind in ("blobs", "weak", "alldup"):
            for rep in (True, False):
                out.append((24 if n <= 64 else 12, n, 32, 2, 10, kind, rep))
    for k in (3, 7, 8, 16):  # between 7 and 8 the trial count goes from 3 to 4
        for n in (k, 20, 40):
            for kind in ("random", "blobs", "dup"):
                for rep in (True, False):
                    out.append((24, n, 16, k, 10, kind, rep))
    for k in (2, 3):
        out.append((32, 20, 1, k, 10, "random", True))    # D = 1
        out.append((1, 20, 16, k, 10, "blobs", True))     # C = 1
        out.append((16, 12, 16, k, 10, "alldup", False))
        for n_init in (1, 32):
            out.append((32, 20, 16, k, n_init, "weak", True))
    out.append((16, 20, 16, 16, 32, "random", True))      # the largest set of draws: 32 x 15 x 4
    out.append((64, 20, 64, 2, 10, "random", True))
    return out


def make(case, seed):
    C, n, D, k, _, kind, _ = case
    rng = np.random.RandomState(seed)
    V = rng.randn(C, n, D).astype(np.float32)
    if kind == "blobs":
        cen = rng.randn(C, k, D).astype(np.float32) * 2
        V = cen[np.arange(C)[:, None], rng.randint(0, k, size=(C, n))] + 0.4 * V
    elif kind == "weak":  # barely separated blobs: many competing local optima across the inits
        cen = rng.randn(C, 2, D).astype(np.float32) * 0.15
        V = cen[np.arange(C)[:, None], rng.randint(0, 2, size=(C, n))] + V
    elif kind == "dup":  # as tests/test_gpu_parity.py: empty clusters and fallback rows occur
        V[:, n // 2:] = V[:, : n - n // 2]
        V[:, :3] = V[:, :1]
    elif kind == "alldup":  # the first half of the components: every sample the same
        V[: (C + 1) // 2, 1:] = V[: (C + 1) // 2, :1]
    return np.ascontiguousarray(V)


def child(args):
    sys.path.insert(0, str(Path(args.tree).resolve()))
    import torch

    from semanticlens_amd import _native as N
    from semanticlens_amd import scores

    dev = N.default_device()
    dump = {}
    for idx, case in enumerate(cases()):
        C, n, D, k, n_init, _, rep = case
        V = torch.from_numpy(make(case, idx)).to(dev)
        first, rand = scores.kmeans_draws(n, n_init, 123, k)
        labels = torch.full((C, n), -7, dtype=torch.int32, device=dev)
        score = N.poly2means(V, first, rand, rep, n_clusters=k, labels=labels)
        # the entry point poly2means dispatched to, for the min_count it keeps to itself
        first, rand = np.ascontiguousarray(first, dtype=np.int32), np.ascontiguousarray(rand, dtype=np.float64)
        s2 = torch.empty((C,), dtype=torch.float64, device=dev)
        mc = torch.full((C,), -7, dtype=torch.int32, device=dev)
        l2 = torch.full((C, n), -7, dtype=torch.int32, device=dev)
        general = k != 2 or n > N.POLY2_MAX_N
        lib, p = N.lib(), N._ptr
        nbytes = int(lib.sl_polykmeans_ws_bytes(C, n, D, k, n_init) if general else lib.sl_poly2means_ws_bytes(C, n, D))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        tail = (first.ctypes.data_as(N._vp), n_init, rand.ctypes.data_as(N._vp), int(rep), p(s2), p(mc), p(l2), p(ws), nbytes, N._stream(V))
        with N._on(dev):
            rc = lib.sl_polykmeans_labels(p(V), C, n, D, k, *tail) if general else lib.sl_poly2means_labels(p(V), C, n, D, *tail)
        torch.cuda.synchronize()
        assert rc == 0, (case, rc)
        score, labels, s2, mc, l2 = (t.cpu().numpy() for t in (score, labels, s2, mc, l2))
        assert np.array_equal(score, s2, equal_nan=True) and np.array_equal(labels, l2), f"case {idx} {case}: poly2means and its entry point differ"
        dump[f"score{idx}"], dump[f"min_count{idx}"], dump[f"labels{idx}"] = score, mc, labels
    np.savez(args.dump, **dump)


def run_child(tree, path):
    subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--tree", str(tree), "--dump", str(path)], check=True,
                   timeout=900)
    return np.load(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=str(ROOT), help=argparse.SUPPRESS)
    ap.add_argument("--dump", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_tree:
        ap.error("--parent-tree is required")
    with tempfile.TemporaryDirectory() as tmp:
        old = run_child(args.parent_tree, Path(tmp) / "parent.npz")
        new = run_child(ROOT, Path(tmp) / "this.npz")
    lines, bad = [], 0
    n_comp = n_exc = n_exc_moved = 0
    for idx, case in enumerate(cases()):
        C, n, D, k, n_init, kind, rep = case
        V = make(case, idx)
        alldup = np.all(V == V[:, :1], axis=(1, 2))
        exc = alldup & (k == 2 and n <= 128 and not rep)  # the named exception, from the inputs alone
        so, sn = old[f"score{idx}"], new[f"score{idx}"]
        ok = all(np.array_equal(old[f"{w}{idx}"][~exc], new[f"{w}{idx}"][~exc], equal_nan=True) for w in ("score", "min_count", "labels"))
        ok_exc = (np.array_equal(old[f"labels{idx}"][exc], new[f"labels{idx}"][exc]) and
                  np.array_equal(old[f"min_count{idx}"][exc], new[f"min_count{idx}"][exc]) and
                  bool(np.all(np.abs(so[exc]) <= 1e-9)) and bool(np.all(np.abs(sn[exc]) <= 1e-9)))
        n_comp += C
        n_exc += int(exc.sum())
        moved = int((so[exc] != sn[exc]).sum())
        n_exc_moved += moved
        bad += (not ok) + (not ok_exc)
        line = (f"case {idx:3d} C={C:2d} n={n:3d} D={D:2d} k={k:2d} n_init={n_init:2d} {kind:6s} replace={int(rep)}: "
                f"{'bit-equal' if ok else 'DIFFERENT'} ({int((~exc).sum())} components, {int(alldup.sum())} all-duplicate)")
        if exc.any():
            line += (f"; exception: components {np.flatnonzero(exc).tolist()}, labels and min_count {'equal' if ok_exc else 'NOT EQUAL / score off 0'}, "
                     f"max |score| parent {np.abs(so[exc]).max():.3g} this {np.abs(sn[exc]).max():.3g}, {moved} scores moved")
        lines.append(line)
    head = [f"K9 unification, bit-equality against the parent tree: {len(cases())} cases, {n_comp} components",
            f"score, min_count and labels bit-equal outside the exception: {'yes' if bad == 0 else 'NO'}",
            f"exception (all-duplicate, k = 2, n <= 128, replace_empty_clusters=False): {n_exc} components, labels and min_count equal, "
            f"both scores within 1e-9 of 0; {n_exc_moved} of their scores differ in bits"]
    text = "\n".join(head + lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
