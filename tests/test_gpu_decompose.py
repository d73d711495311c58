"""K28 on the GPU: ``sl_omp_init`` / ``sl_omp_step`` with hand-fed candidates against a numpy float64 restatement that solves every
least-squares problem with ``np.linalg.lstsq`` on the same fp32 rows, the step kernel past its grid cap, ``probe_decompose`` against
float64 greedy matching pursuit in both GEMM arithmetics, and ``decompose_components`` over the suite's fake text tower.

Bounds.  ids, ``n_terms`` and the finished flags are integers: equality.  ``coefs`` and ``explained``: 1e-12 absolute — two float64
methods on this data (lstsq against the normal equations by Cholesky) differ by at most 3.6e-15 at Gram condition numbers up to 15,
a reordered float64 dot of length 130 adds about 1.4e-14 times that condition number, and 1e-12 leaves a factor of about 5 over the
product.  The residual: ``2^-23 max|r| + 1e-12``, the fp32 rounding of the stored value.  The reference keeps the margins of its own
decisions (pivots against 1e-10, ``|r|^2`` against 1e-8) and the tests assert that none of them is within a factor 10 of its
constant, so a difference of rounding cannot flip a branch.

Measured on one MI355X: kernel against lstsq, worst ``|coefs|`` error 8.0e-15, ``|explained|`` error 5.6e-16, residual 0.497 of its bound;
end to end on decidable components, ``|correlation - float64|`` 3.0e-6 (bf16x3) and 5.4e-7 (f32), ``|coefs|`` 3.7e-15."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from helpers import FakeVLM
from semanticlens_amd import _native as N
from semanticlens_amd import lens as L

pytestmark = pytest.mark.gpu
TOL = 1e-4  # the suite's bound for a cosine
DEV = "cuda"
MIN_PIVOT, RESIDUAL_DONE = 1e-10, 1e-8  # csrc/omp_state.hpp
F64_BOUND = 1e-12
FIELDS = ("ids", "chol", "rhs", "coefs", "corr", "explained", "n_terms", "last")
SENTINEL = dict(ids=-7, chol=2.25, rhs=-1.75, coefs=123.25, corr=-3.5, explained=-9.5, n_terms=77, last=5.5)


# ---------------------------------------------------------------------------------------------------------------------
# the reference: csrc/omp_state.hpp's rules and the kernel's outputs, restated in float64 with lstsq
# ---------------------------------------------------------------------------------------------------------------------
class Ref:
    def __init__(self, x: np.ndarray, w: np.ndarray, s: int):
        C, D = x.shape
        self.s, self.V = s, w.shape[0]
        x64, w64 = x.astype(np.float64), w.astype(np.float64)
        with np.errstate(all="ignore"):
            sx = (x64 * x64).sum(1)
            valid = np.isfinite(sx) & (sx > 0)
            self.xh = np.where(valid[:, None], x64 / np.sqrt(np.where(valid, sx, 1.0))[:, None], 0.0)
            self.wh = w64 / np.sqrt((w64 * w64).sum(1))[:, None]
        self.ids = np.full((C, s), -1, dtype=np.int64)
        self.chol = np.zeros((C, s * (s + 1) // 2))  # compared only where a sentinel was written: the factor is the kernel's own
        self.rhs = np.zeros((C, s))
        self.coefs = np.zeros((C, s))
        self.corr = np.full((C, s), np.nan, dtype=np.float32)
        self.explained = np.where(valid[:, None], 0.0, np.nan) * np.ones((1, s))
        self.n_terms = np.zeros(C, dtype=np.int32)
        self.finished = (~valid).astype(np.int32)
        self.work = self.xh.copy()
        self.last = np.full((C, D), np.nan)
        self.last_defined = ~valid
        self.frozen = np.zeros(C, dtype=bool)  # rows that carry the sentinel pattern: compared whole, chol and rhs included
        self.reasons = {}                      # component -> why it stopped
        self.skipped_chosen = 0                # candidates passed over because they were chosen already
        self.equal_to_min_correlation = 0
        self.pivots, self.r2s = [], []         # every decision's figure, for the margins
        self.step_r2 = [[] for _ in range(C)]

    def _stop(self, c: int, t: int, why: str):
        self.last[c], self.last_defined[c] = self.work[c], True
        self.work[c] = 0.0
        self.finished[c] = 1
        self.explained[c, t:] = self.explained[c, t - 1] if t > 0 else 0.0
        self.reasons[c] = why

    def step(self, cand_vals: np.ndarray, cand_ids: np.ndarray, t: int, min_correlation: float):
        s = self.s
        for c in range(self.ids.shape[0]):
            if self.finished[c]:
                continue
            chosen = self.ids[c, :t].tolist()
            slot = None
            for j in range(cand_ids.shape[1]):
                i = int(cand_ids[c, j])
                if i < 0 or i >= self.V:
                    continue
                if i in chosen:
                    self.skipped_chosen += 1
                    continue
                slot = j
                break
            if slot is None:
                self._stop(c, t, "none")
                continue
            v, i = cand_vals[c, slot], int(cand_ids[c, slot])
            if np.isnan(v):
                self._stop(c, t, "nan")
                continue
            if float(v) <= min_correlation:
                self.equal_to_min_correlation += float(v) == min_correlation
                self._stop(c, t, "correlation")
                continue
            A = self.wh[chosen].T  # (D, t)
            with np.errstate(all="ignore"):
                d = self.wh[i] - (A @ np.linalg.lstsq(A, self.wh[i], rcond=None)[0] if t else 0.0)
                d2 = float(d @ d)
            self.pivots.append(d2)
            if not d2 >= MIN_PIVOT:
                self._stop(c, t, "pivot")
                continue
            A = self.wh[chosen + [i]].T
            a = np.linalg.lstsq(A, self.xh[c], rcond=None)[0]
            r = self.xh[c] - A @ a
            r2 = float(r @ r)
            self.r2s.append(r2)
            self.step_r2[c].append(r2)
            self.ids[c, t], self.corr[c, t], self.n_terms[c] = i, v, t + 1
            self.coefs[c, : t + 1] = a
            self.explained[c, t] = 1.0 - r2
            if t == s - 1:
                self.last[c], self.last_defined[c] = r, True
            else:
                self.work[c] = r
            if r2 <= RESIDUAL_DONE:
                if t != s - 1:
                    self.last[c], self.last_defined[c] = r, True
                self.work[c] = 0.0
                self.finished[c] = 1
                self.explained[c, t + 1:] = 1.0 - r2
                self.reasons[c] = "residual"

    def margins_hold(self):
        """No decision of the reference lies within a factor 10 of its constant."""
        assert all(p < MIN_PIVOT / 10 or p > MIN_PIVOT * 10 for p in self.pivots), sorted(self.pivots)[:3]
        assert all(r < RESIDUAL_DONE / 10 or r > RESIDUAL_DONE * 10 for r in self.r2s), sorted(self.r2s)[:3]


def cosines(ref: Ref) -> np.ndarray:
    """float64 cosines of the working residuals to every word; a zero row has cosine 0 to everything."""
    n = np.sqrt((ref.work * ref.work).sum(1))
    return (ref.work / np.where(n > 0, n, 1.0)[:, None]) @ ref.wh.T


def best_candidates(cos: np.ndarray, k: int):
    order = np.argsort(-cos, axis=1, kind="stable")[:, :k]
    vals, ids = np.take_along_axis(cos, order, axis=1).astype(np.float32), order.astype(np.int64)
    if k > cos.shape[1]:  # K17's empty slots
        pad = k - cos.shape[1]
        vals = np.concatenate([vals, np.full((cos.shape[0], pad), -np.inf, dtype=np.float32)], axis=1)
        ids = np.concatenate([ids, np.full((cos.shape[0], pad), -1, dtype=np.int64)], axis=1)
    return vals, ids


class Worst:
    def __init__(self):
        self.coefs = self.explained = self.residual = 0.0


def close64(got: np.ndarray, want: np.ndarray, what: str) -> float:
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN in other places"
    err = float(np.nanmax(np.abs(got - want), initial=0.0))
    assert err <= F64_BOUND, f"{what}: {err:.3e} above {F64_BOUND:.0e}"
    return err


def residual_close(got: np.ndarray, want: np.ndarray, what: str) -> float:
    """fp32 rows against float64 rows: 2^-23 max|r| + 1e-12 per row; returns the worst error in units of the bound."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN in other places"
    bound = 2.0 ** -23 * np.nanmax(np.abs(want), axis=1, initial=0.0)[:, None] + 1e-12
    ratio = np.nan_to_num(np.abs(got.astype(np.float64) - want) / bound)
    assert ratio.max(initial=0.0) <= 1.0, f"{what}: {ratio.max():.3f} of the bound"
    return float(ratio.max(initial=0.0))


def compare(st: N.OmpState, ref: Ref, what: str, worst: Worst):
    got = {name: getattr(st, name).cpu().numpy() for name in st._fields}
    assert np.array_equal(got["ids"], ref.ids), f"{what}: ids"
    assert np.array_equal(got["n_terms"], ref.n_terms), f"{what}: n_terms"
    assert np.array_equal(got["finished"], ref.finished), f"{what}: finished flags"
    assert np.array_equal(got["corr"], ref.corr, equal_nan=True), f"{what}: correlation"
    worst.coefs = max(worst.coefs, close64(got["coefs"], ref.coefs, f"{what}: coefs"))
    worst.explained = max(worst.explained, close64(got["explained"], ref.explained, f"{what}: explained"))
    worst.residual = max(worst.residual, residual_close(got["residual"], ref.work, f"{what}: working residual"))
    assert not got["residual"][ref.finished == 1].any(), f"{what}: a finished component's working row is not zero"
    rows = ref.last_defined
    worst.residual = max(worst.residual, residual_close(got["last"][rows], ref.last[rows], f"{what}: reported residual"))
    for name in ("chol", "rhs"):  # a frozen row's factor and right-hand side carry the sentinel too
        assert np.array_equal(got[name][ref.frozen], getattr(ref, name)[ref.frozen]), f"{what}: {name} of a finished component moved"


def plant_sentinels(st: N.OmpState, ref: Ref):
    """Every finished component that does not carry the pattern yet gets it, on the device and in the reference: what a later step
    writes there shows in the next comparison."""
    new = (ref.finished == 1) & ~ref.frozen
    if not new.any():
        return
    rows = torch.from_numpy(np.flatnonzero(new)).to(DEV)
    for name in FIELDS:
        getattr(st, name)[rows] = SENTINEL[name]
        getattr(ref, name)[new] = SENTINEL[name]
    ref.last_defined |= new
    ref.frozen |= new


def run_pursuit(x: np.ndarray, w: np.ndarray, s: int, min_correlation: float, k_extra: int, edit=None, w_dev=None, sentinels=True):
    """Init and ``s`` steps with candidates taken from the reference's own float64 cosines (``edit(t, vals, ids, ref)`` may rewrite them),
    every output compared after every step."""
    ref, worst = Ref(x, w, s), Worst()
    xd = torch.from_numpy(x).to(DEV)
    wd = torch.from_numpy(w).to(DEV) if w_dev is None else w_dev
    st = N.omp_new(xd, s)
    compare(st, ref, "init", worst)
    for t in range(s):
        if sentinels:
            plant_sentinels(st, ref)
        vals, ids = best_candidates(cosines(ref), t + 1 + k_extra)
        if edit is not None:
            edit(t, vals, ids, ref)
        ref.step(vals, ids, t, min_correlation)
        N.omp_step(st, xd, wd, torch.from_numpy(vals).to(DEV), torch.from_numpy(ids).to(DEV), t, min_correlation)
        compare(st, ref, f"step {t}", worst)
    ref.margins_hold()
    return st, ref, worst


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel, hand-fed candidates
# ---------------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [(96, 500, 64, 4, False), (96, 500, 64, 4, True), (64, 300, 36, 16, False), (70, 257, 130, 6, False), (5, 40, 4, 3, False),
                (3, 9, 1, 1, False)]
MIN_CORRELATION = 0.125


def special_inputs(x: np.ndarray, w: np.ndarray):
    """Components 4..8 and the duplicate word the branches need (see ``special_edit``)."""
    w[7] = w[5]                                              # an exact duplicate vocabulary row under another id
    unit = lambda v: v.astype(np.float64) / np.linalg.norm(v.astype(np.float64))
    x[4] = (0.8 * unit(w[5]) + 0.3 * unit(w[20])).astype(np.float32)
    x[5] = (0.6 * unit(w[30]) + 0.8 * unit(w[31])).astype(np.float32)  # exactly two words: |r|^2 <= 1e-8 after two terms
    x[6] = 0.0
    x[7, 3] = np.inf
    x[8, 2] = np.nan


def special_edit(t: int, vals: np.ndarray, ids: np.ndarray, ref: Ref):
    """Candidate lists (k = t + 2) that reach each branch of the rule."""
    V = ref.V
    if t == 0:
        vals[4, 0], ids[4, 0] = 0.9, 5                      # component 4 takes word 5 ...
        ids[9, :] = -1                                      # component 9: only empty slots
        vals[10, 1], ids[10, 1] = vals[10, 0], ids[10, 0]   # component 10: an id >= V first, then its best word
        vals[10, 0], ids[10, 0] = 0.99, V + 3
        vals[11, 1], ids[11, 1] = vals[11, 0], ids[11, 0]   # component 11: an id of -1 first
        vals[11, 0], ids[11, 0] = 0.99, -1
        vals[12, 1], ids[12, 1] = vals[12, 0], ids[12, 0]   # component 12: an id far past V (never an index)
        vals[12, 0], ids[12, 0] = 0.99, 2**40
    if t == 1:
        vals[1, 1], ids[1, 1] = vals[1, 0], ids[1, 0]       # component 1: its first candidate is already chosen
        vals[1, 0], ids[1, 0] = 0.9, ref.ids[1, 0]
        vals[2, 0] = np.float32(MIN_CORRELATION)            # component 2: a value exactly equal to min_correlation
        vals[3, 0] = np.nan                                 # component 3: a NaN value
        vals[4, 0], ids[4, 0] = 0.5, 7                      # ... and is offered its duplicate, word 7: pivot 0


@pytest.mark.parametrize("C,V,D,s,misaligned", KERNEL_CASES)
def test_kernel_against_lstsq_after_every_step(C, V, D, s, misaligned):
    rng = np.random.default_rng(1000 * C + D)
    w = rng.standard_normal((V, D)).astype(np.float32)
    x = rng.standard_normal((C, D)).astype(np.float32)
    special = C >= 16
    if special:
        special_inputs(x, w)
    w_dev = None
    if misaligned:  # a view of the vocabulary that starts 4 bytes past a 16-byte boundary, NaN around it
        buf = torch.full((V * D + 8,), float("nan"), dtype=torch.float32, device=DEV)
        buf[1 : 1 + V * D] = torch.from_numpy(w).to(DEV).reshape(-1)
        w_dev = buf[1 : 1 + V * D].view(V, D)
        assert w_dev.data_ptr() % 16 == 4 and w_dev.is_contiguous()
    st, ref, worst = run_pursuit(x, w, s, MIN_CORRELATION, 1, special_edit if special else None, w_dev)
    print(f"({C}, {V}, {D}, {s}) misaligned={misaligned}: worst |coefs - lstsq| = {worst.coefs:.3e}, |explained - lstsq| = "
          f"{worst.explained:.3e}, residual {worst.residual:.3f} of its bound; stops {sorted(set(ref.reasons.values()))}")
    if special:  # the reference reached every branch
        assert ref.skipped_chosen >= 1
        assert ref.reasons[2] == "correlation" and ref.equal_to_min_correlation >= 1
        assert ref.reasons[3] == "nan"
        assert ref.reasons[4] == "pivot" and min(ref.pivots) < 1e-20
        assert ref.reasons[5] == "residual"
        assert ref.reasons[9] == "none"
        assert {"none", "nan", "correlation", "pivot", "residual"} <= set(ref.reasons.values())
        assert ref.frozen[[2, 3, 4, 5, 6, 7, 8, 9]].all()  # finished before the last step: they carried the pattern through later steps
        assert ref.finished[[6, 7, 8]].all() and 6 not in ref.reasons  # zero row, inf and NaN coordinates: finished by init
        assert (~ref.frozen).any() and ref.n_terms[~ref.frozen].max() == s
    # sentinels aside, the same pursuit gives the state whose pattern-free outputs the API hands out
    free, _, _ = run_pursuit(x, w, s, MIN_CORRELATION, 1, special_edit if special else None, w_dev, sentinels=False)
    if special:
        n = free.n_terms.cpu().numpy()
        assert n[1] >= 2 and n[[2, 3, 4]].tolist() == [1, 1, 1] and n[5] == 2 and n[[6, 7, 8, 9]].tolist() == [0, 0, 0, 0]
        assert n[[10, 11, 12]].min() >= 1
        assert np.isnan(free.explained.cpu().numpy()[[6, 7, 8]]).all() and np.isnan(free.last.cpu().numpy()[[6, 7, 8]]).all()
        assert (free.ids.cpu().numpy()[[6, 7, 8, 9]] == -1).all() and (free.coefs.cpu().numpy()[[6, 7, 8, 9]] == 0).all()


def test_step_refuses_states_and_candidates_that_do_not_fit():
    x = torch.randn(6, 8, device=DEV)
    w = torch.randn(9, 8, device=DEV)
    st = N.omp_new(x, 3)
    vals, ids = torch.zeros(6, 1, device=DEV), torch.zeros(6, 1, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        N.omp_step(st, x, w, vals, ids, 1)               # step 1 needs two candidates
    with pytest.raises(ValueError):
        N.omp_step(st, x, w, vals[:5], ids[:5], 0)       # another row count
    with pytest.raises(ValueError):
        N.omp_step(st, x, w, vals, ids.int(), 0)         # ids of another type
    with pytest.raises(ValueError):
        N.omp_step(st, x, w[:, :4].contiguous(), vals, ids, 0)  # another width
    with pytest.raises(ValueError):
        N.omp_step(st, x, torch.randn(8, 9, device=DEV).t(), vals, ids, 0)  # a vocabulary that is not contiguous
    with pytest.raises(ValueError):
        N.omp_step(st, x.double(), w, vals, ids, 0)
    with pytest.raises(ValueError):
        N.omp_step(st._replace(coefs=st.coefs[:, :2]), x, w, vals, ids, 0)  # a state of another s
    with pytest.raises(ValueError):
        N.omp_step(st, x, w, vals, ids, 3)               # t outside [0, s)


# ---------------------------------------------------------------------------------------------------------------------
# 2. past the grid cap
# ---------------------------------------------------------------------------------------------------------------------
def test_step_kernel_past_its_grid():
    """omp.hip: ``rowseg::wave_grid(C, CUs, 4)`` one-wave items in workgroups of four waves: 16 x CUs components per trip.  C = cap + 1
    ends the second trip after one component, 2 x cap + 1 the third; every component against the reference."""
    cap = 4 * torch.cuda.get_device_properties(0).multi_processor_count * 4
    D, V, s = 4, 16, 2
    w = np.random.default_rng(28).standard_normal((V, D)).astype(np.float32)
    for C in (cap + 1, 2 * cap + 1):
        assert C > cap
        x = np.random.default_rng(C).standard_normal((C, D)).astype(np.float32)
        _, ref, worst = run_pursuit(x, w, s, 0.0, 0, sentinels=False)
        assert (ref.n_terms == 2).sum() > C // 2
        print(f"C = {C}: worst |coefs - lstsq| = {worst.coefs:.3e}, residual {worst.residual:.3f} of its bound")


# ---------------------------------------------------------------------------------------------------------------------
# 3. probe_decompose against float64 greedy matching pursuit
# ---------------------------------------------------------------------------------------------------------------------
E2E_CASES = [(96, 500, 64, 4, 3, 0.05), (96, 1000, 64, 8, 3, 0.05), (64, 300, 36, 16, 5, 0.1), (70, 257, 130, 6, 2, 0.0)]
_E2E = {}


def planted_inputs(C: int, V: int, D: int, planted: int, noise: float):
    rng = np.random.default_rng(7)
    w = rng.standard_normal((V, D)).astype(np.float32)
    w[1] = w[0] + np.float32(0.3) * rng.standard_normal(D).astype(np.float32)
    wh = w.astype(np.float64) / np.linalg.norm(w.astype(np.float64), axis=1, keepdims=True)
    x = np.empty((C, D), dtype=np.float32)
    for c in range(C):
        words = rng.choice(V, size=planted, replace=False)
        weights = rng.uniform(0.4, 1.0, size=planted)
        x[c] = (weights @ wh[words] + noise * rng.standard_normal(D) / np.sqrt(D)).astype(np.float32)
    return x, w


def e2e_case(case):
    """The float64 pursuit of a case and which of its components are decidable; computed once."""
    if case not in _E2E:
        C, V, D, s, planted, noise = case
        x, w = planted_inputs(C, V, D, planted, noise)
        ref = Ref(x, w, s)
        decidable = ref.finished == 0
        for t in range(s):
            cos = cosines(ref)
            vals, ids = best_candidates(cos, t + 1)
            open_ = np.flatnonzero(ref.finished == 0)
            ref.step(vals, ids, t, 0.0)
            for c in open_:
                admissible = np.delete(cos[c], ref.ids[c, :t])
                top = np.sort(admissible)[-2:]
                if len(top) == 2 and top[1] - top[0] <= 2 * TOL:  # either cosine may move by TOL
                    decidable[c] = False
                if abs(top[-1] - 0.0) <= TOL:                     # the chosen (or refused) cosine against min_correlation
                    decidable[c] = False
        for c in range(C):
            if any(RESIDUAL_DONE / 10 <= r <= RESIDUAL_DONE * 10 for r in ref.step_r2[c]):
                decidable[c] = False
        assert all(p > 10 * MIN_PIVOT for p in ref.pivots)
        _E2E[case] = (x, w, ref, decidable)
    return _E2E[case]


def check_invariants(dec: L.Decomposition, w: np.ndarray, what: str):
    ids, n = dec.ids.cpu().numpy(), dec.n_terms.cpu().numpy()
    explained, residual = dec.explained.cpu().numpy(), dec.residual.cpu().numpy().astype(np.float64)
    wh = w.astype(np.float64) / np.linalg.norm(w.astype(np.float64), axis=1, keepdims=True)
    assert (np.diff(explained, axis=1) >= 0).all() and explained.min() >= 0 and explained.max() <= 1 + 1e-12, f"{what}: explained"
    for c in range(ids.shape[0]):
        chosen = ids[c, : n[c]]
        assert (chosen >= 0).all() and len(set(chosen.tolist())) == n[c] and (ids[c, n[c]:] == -1).all(), f"{what}: ids of {c}"
        assert np.abs(wh[chosen] @ residual[c]).max(initial=0.0) <= 1e-6, f"{what}: the residual of {c} is not orthogonal to its words"
        if n[c]:
            assert abs(explained[c, n[c] - 1] - (1.0 - residual[c] @ residual[c])) <= 1e-6, f"{what}: explained of {c}"


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("case", E2E_CASES)
def test_probe_decompose_against_float64_pursuit(case, mode):
    C, V, D, s, _, _ = case
    x, w, ref, decidable = e2e_case(case)
    print(f"{case}: {int(decidable.sum())} / {C} decidable; terms used {np.bincount(ref.n_terms, minlength=s + 1).tolist()}")
    assert decidable.sum() >= 0.9 * C
    N.set_gemm_mode(mode)
    try:
        dec = L.probe_decompose(torch.from_numpy(w).to(DEV), torch.from_numpy(x).to(DEV), n_terms=s)
    finally:
        N.set_gemm_mode(None)
    assert isinstance(dec, L.Decomposition) and dec.ids.dtype == torch.int64 and dec.coefs.dtype == torch.float64
    assert dec.correlation.dtype == torch.float32 and dec.explained.dtype == torch.float64 and dec.n_terms.dtype == torch.int32
    assert dec.residual.dtype == torch.float32 and tuple(dec.residual.shape) == (C, D) and tuple(dec.ids.shape) == (C, s) and dec.ids.is_cuda
    check_invariants(dec, w, f"{case} {mode}")
    d = decidable
    assert np.array_equal(dec.ids.cpu().numpy()[d], ref.ids[d]) and np.array_equal(dec.n_terms.cpu().numpy()[d], ref.n_terms[d])
    corr, used = dec.correlation.cpu().numpy()[d], ref.ids[d] >= 0
    assert np.isnan(corr[~used]).all()
    err_corr = np.abs(corr[used].astype(np.float64) - ref.corr[d][used]).max()
    err_coefs = np.abs(dec.coefs.cpu().numpy()[d] - ref.coefs[d]).max()
    err_expl = np.abs(dec.explained.cpu().numpy()[d] - ref.explained[d]).max()
    print(f"{mode}: max |correlation - float64| = {err_corr:.3e}, |coefs - lstsq| = {err_coefs:.3e}, |explained - lstsq| = {err_expl:.3e}")
    assert err_corr <= TOL and err_coefs <= F64_BOUND and err_expl <= F64_BOUND
    if case[5] == 0.0:
        assert (ref.n_terms == 2).all() and set(ref.reasons.values()) == {"residual"}  # exactly two words each


# ---------------------------------------------------------------------------------------------------------------------
# 4. tiling
# ---------------------------------------------------------------------------------------------------------------------
def test_tiling_does_not_change_the_decidable_components():
    case = E2E_CASES[0]
    x, w, ref, decidable = e2e_case(case)
    V, s = case[1], case[3]
    xd, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
    whole = L.probe_decompose(wd, xd, n_terms=s, chunk_rows=V)
    tiled = L.probe_decompose(wd, xd, n_terms=s, chunk_rows=97)
    d = torch.from_numpy(decidable).to(DEV)
    assert torch.equal(whole.ids[d], tiled.ids[d]) and torch.equal(whole.n_terms[d], tiled.n_terms[d])
    assert np.array_equal(tiled.ids[d].cpu().numpy(), ref.ids[decidable])
    check_invariants(tiled, w, "chunk_rows=97")


# ---------------------------------------------------------------------------------------------------------------------
# 5. decompose_components over the suite's fake text tower
# ---------------------------------------------------------------------------------------------------------------------
LETTERS = "abcdefghijklmnopqrstuvwxyz"
TEMPLATES = ["a photo of {}", "{} texture", "an image showing {}."]


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same(a: L.Decomposition, b: L.Decomposition) -> bool:
    return all(torch.equal(bits(getattr(a, f)), bits(getattr(b, f))) for f in ("ids", "coefs", "correlation", "explained", "n_terms", "residual"))


@pytest.mark.parametrize("templates", [None, TEMPLATES])
def test_decompose_components_equals_probe_decompose_bit_for_bit(templates):
    rng = np.random.default_rng(11)
    words = []
    while len(words) < 39:
        word = "".join(LETTERS[i] for i in rng.integers(0, 26, size=int(rng.integers(3, 9))))
        if word not in words:
            words.append(word)
    words.insert(20, words[4])  # 40 words, one of them twice: a duplicate row of the vocabulary
    fm = FakeVLM(dim=16, ctx=24).to(DEV)
    emb = L._embed_words(fm, words, templates, None)
    assert torch.equal(emb[20], emb[4])
    g = torch.Generator().manual_seed(3)
    mix = torch.rand(30, 40, generator=g) * (torch.rand(30, 40, generator=g) < 0.08)
    db = {"a": (mix.to(DEV) @ emb + 0.05 * torch.randn(30, 16, generator=g).to(DEV) * emb.abs().mean()),
          "b": torch.randn(12, 16, generator=g)}  # layer b lives on the host
    db["a"][0] = emb[4]  # component 0 IS the duplicated word: one term spans it, and the residual rule stops it there
    want = L.probe_decompose(emb, db, n_terms=3)
    assert set(want) == {"a", "b"} and want["a"].ids.is_cuda and not want["b"].ids.is_cuda and not want["b"].residual.is_cuda
    assert int(want["a"].n_terms[0]) == 1 and int(want["a"].ids[0, 0]) in (4, 20)
    for chunk_size in (7, None):
        got = L.decompose_components(fm, words, db, n_terms=3, templates=templates, chunk_size=chunk_size)
        assert list(got) == ["a", "b"]
        for name in db:
            assert same(got[name], want[name]), f"layer {name}, chunk_size={chunk_size}"
            assert got[name].ids.device == db[name].device and got[name].residual.device == db[name].device
    one = L.Lens(fm, device=DEV).decompose_components(words, db["a"], 3, templates, None, 7)
    assert isinstance(one, L.Decomposition) and same(one, want["a"])
    terms = one.terms(0, words)
    assert len(terms) == 1 and terms[0][0] == words[4] and abs(terms[0][2] - float(one.explained[0, 0])) == 0.0
    bad = emb.clone()
    bad[3, 2] = float("inf")
    with pytest.raises(ValueError, match="NaN or an infinite"):
        L.probe_decompose(bad, db["a"], n_terms=2)
