"""References of the recycled GCR solve (vasp_amd/csrc/fsi_krylov.hip) and of its kept store, plain numpy, no device.

The solve's safety nets - the FP64 verdict on b - A x, the restart, the fall-back from FP32 storage - turn a wiring error
of the device code into slowness, so the tests (tests/test_gcr_solve_reference.py on the CPU, tests/test_gpu_gcr_solve.py on a
live context) state properties that hold whatever path the iteration takes:

check_store     the exact facts of a store as kernel_shim.ctx_krylov_info / ctx_krylov_columns fetch it;
true_residual   b - A x in np.longdouble from the context's own CSR arrays, with the a-priori bound of an FP64 product;
gcr_twin        a host twin of the FP64 path, for what a property cannot say: how many iterations a case should take.
"""
from __future__ import annotations

import numpy as np

import kernel_shim as ks

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)          # 2^-52, twice the unit round-off u
# | |KQh[k]|^2 - 1 |, see check_store: 64 eps for the FP64 sum of squares, 3 eps for the square root, the reciprocal and the
# scaling (u each, doubled by the square), one more for the second-order terms
WINDOW_NORM_BOUND = 68 * EPS


class Csr:
    """a square CSR matrix as the context holds it (rowptr int64 [n + 1], cols, vals float64)"""

    def __init__(self, rowptr, cols, vals):
        self.rowptr = np.asarray(rowptr, dtype=np.int64)
        self.cols = np.asarray(cols, dtype=np.int64)
        self.vals = np.asarray(vals, dtype=np.float64)
        self.n = len(self.rowptr) - 1
        self.row_nnz = np.diff(self.rowptr)
        self._first = np.minimum(self.rowptr[:-1], max(len(self.vals) - 1, 0))
        self._abs = None

    @classmethod
    def from_dense(cls, M):
        M = np.asarray(M, dtype=np.float64)
        mask = M != 0.0
        rowptr = np.concatenate(([0], np.cumsum(mask.sum(axis=1))))
        return cls(rowptr, np.nonzero(mask)[1], M[mask])

    def _rows(self, terms):
        if len(terms) == 0:
            return np.zeros(self.n, dtype=terms.dtype)
        y = np.add.reduceat(terms, self._first)
        y[self.row_nnz == 0] = 0
        return y

    def dot(self, x, dtype=np.float64):
        """A x, every product and every row sum in `dtype`"""
        return self._rows(self.vals.astype(dtype) * np.asarray(x, dtype=dtype)[self.cols])

    def absdot(self, x):
        """|A| |x| in float64"""
        if self._abs is None:
            self._abs = np.abs(self.vals)
        return self._rows(self._abs * np.abs(np.asarray(x, dtype=np.float64))[self.cols])


def true_residual(A: Csr, b, x):
    """(r, bound): r = b - A x in np.longdouble, and the 2-norm of the a-priori bound of an FP64 evaluation of the same
    expression against it.  A row of L entries is L products and L additions (the subtraction from b among them), each
    rounded once: the error of row i is at most (L_i + 2) eps (|A| |x| + |b|)_i with eps = 2^-52 (twice the unit round-off, which
    covers the second-order terms and any summation order), and the largest row stands for all of them:
        bound = | (max row nnz + 2) eps (|A| |x| + |b|) |_2.
    | |r_fp64| - |r| | <= |r_fp64 - r| <= bound, so a device residual norm may differ from |r| by the bound and no more."""
    b64, x64 = np.asarray(b, dtype=np.float64), np.asarray(x, dtype=np.float64)
    r = b64.astype(LD) - A.dot(x64, LD)
    vec = (int(A.row_nnz.max()) + 2) * EPS * (A.absdot(x64) + np.abs(b64))
    return r, float(np.linalg.norm(vec))


def norm(v):
    return float(np.sqrt(np.sum(np.asarray(v, dtype=LD) ** 2)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def check_store(info, Q, Z, Qh=None):
    """The exact facts of a kept store; raises AssertionError naming the first one that does not hold.

    info: cap, hw, made, free (the free list), born [cap], hot_slots [GCR_WINDOW], kry_fp32, ndof (kernel_shim.ctx_krylov_info,
    or gcr_twin's); Q [hw][ldq] float32 or float64 as stored, Z [hw][ldz], Qh [GCR_WINDOW][ldq] float64 (FP32 store only).

    * hw <= cap; kept = hw - len(free) = count(born >= 0); no slot at or above hw holds a direction; the free list is exactly
      the slots below hw without one, each once;
    * the born indices are distinct and below made;
    * a free slot below hw was retired, and retirement zeroes its KQ and KZ column over the whole stride: all-zero bits;
    * every window entry is -1 or a live slot, no slot twice;
    * the protect rule of GcrStore::retire: a direction born before cap - gcr_ring(cap) is never retired, so every index below
      min(made, cap - gcr_ring(cap)) is present (made restarts at 0 with a reset, so this holds across restarts too);
    * FP32 store, every window column k in use: KQ[hot_slots[k]] equals float32(KQh[k]) bit for bit on the ndof rows
      (gcr_update rounds one FP64 value q_i = w_i / |w'| into both), and | |KQh[k]|^2 - 1 | <= WINDOW_NORM_BOUND.
      Derivation of the constant: |w'|^2 is the update kernel's FP64 sum of squares, relative error 64 eps (the rule of
      tests/test_gpu_gcr_kernels.py, all terms positive); the host takes its square root (u = eps / 2), forms 1 / |w'| (u), the
      kernel multiplies every entry by it (u).  The last three enter |q|^2 squared, 2u = eps each: 64 eps + 3 eps, and one eps
      for the products of these terms.  The check's own sum is formed in np.longdouble.
    """
    cap, hw, made, n = info["cap"], info["hw"], info["made"], info["ndof"]
    born, free, hot = list(info["born"]), list(info["free"]), list(info["hot_slots"])
    fp32 = bool(info["kry_fp32"])
    assert 0 <= hw <= cap, f"hw {hw} outside [0, cap {cap}]"
    assert len(born) == cap and len(hot) == ks.GCR_WINDOW
    live = [s for s in range(cap) if born[s] >= 0]
    assert all(s < hw for s in live), f"a direction lives at or above hw {hw}: slots {[s for s in live if s >= hw]}"
    kept = hw - len(free)
    assert kept == len(live), f"kept: hw - len(free) = {kept}, but {len(live)} slots hold a direction"
    assert sorted(free) == [s for s in range(hw) if born[s] < 0], f"free list {sorted(free)} is not the empty slots below hw"
    ages = [born[s] for s in live]
    assert len(set(ages)) == len(ages), "born: an index appears twice"
    assert all(a < made for a in ages), f"born: index {max(ages, default=-1)} is not below made {made}"
    assert Q.shape[0] == hw and Z.shape[0] == hw, (Q.shape, Z.shape, hw)
    assert Q.dtype == (np.float32 if fp32 else np.float64), f"Q fetched as {Q.dtype} from a store with kry_fp32 = {int(fp32)}"
    for s in free:
        nq, nz = int(np.count_nonzero(_bits(Q[s]))), int(np.count_nonzero(_bits(Z[s])))
        assert nq == 0, f"free slot {s}: {nq} entries of its KQ column are not zero bits"
        assert nz == 0, f"free slot {s}: {nz} entries of its KZ column are not zero bits"
    used = [s for s in hot if s >= 0]
    assert all(s < hw and born[s] >= 0 for s in used), f"window: entries {[s for s in used if not (s < hw and born[s] >= 0)]} are not live slots"
    assert len(set(used)) == len(used), "window: a slot appears twice"
    protect = cap - ks.gcr_ring(cap)
    missing = sorted(set(range(min(made, protect))) - set(ages))
    assert not missing, f"protect rule: directions {missing[:8]} born before {protect} are gone"
    if fp32:
        assert Qh is not None, "an FP32 store has a window"
        for k, s in enumerate(hot):
            if s < 0:
                continue
            diff = int(np.count_nonzero(_bits(Q[s, :n]) != _bits(Qh[k, :n].astype(np.float32))))
            assert diff == 0, f"window column {k} (slot {s}): {diff} entries of KQ differ from float32(KQh) in their bits"
            dev = abs(float(np.sum(Qh[k, :n].astype(LD) ** 2) - 1))
            assert dev <= WINDOW_NORM_BOUND, f"window column {k} (slot {s}): | |q|^2 - 1 | = {dev:.3e} > {WINDOW_NORM_BOUND:.3e}"


def _dots(Qm, w, dots):
    """Q_k . w for the rows of Qm: every product rounded to float64, accumulated in float64 (a BLAS product) or in np.longdouble"""
    if dots == "float64":
        return Qm @ w
    assert dots == "longdouble", dots
    return (Qm * w).astype(LD).sum(axis=1).astype(np.float64)


def gcr_twin(A: Csr, M, b, rtol, max_it, cap, escape, dots="longdouble", track_pairs=False, resume=None):
    """Right-preconditioned flexible GCR with kept pairs (Q = A P orthonormal), the host twin of solve_gcr's FP64 path.

    FP64 columns; per cycle the entry projection r -= Q (Q^T r), x += P (Q^T r); per iteration z = M(src), w = A z, classical
    Gram-Schmidt twice against the live columns, q = w' / |w'|, p = (z - sum_j h_j p_j) / |w'| kept explicit, alpha = q . r, r by
    recurrence, and the escape rule of gcr_store (alpha^2 <= escape |r|^2: the next direction is made from q), which changes the
    iterates.  Slots, retirement and the ring are GcrStoreRef's, a cycle ends by gcr_cycle_end_ref, after every cycle the true
    residual is formed (true_residual, rounded to float64) and the restart rule is judge_fp64_cycle's.  M: any callable.
    `dots`: "longdouble" or "float64" accumulation of every inner product and norm - two host references whose spread is what
    summation order alone is worth.  resume: an earlier result, whose kept pairs this solve starts with (the same matrix and M).

    Returns a dict: x, iters, relres (of the true residual), restarts, cycles, store (GcrStoreRef), Q, P [cap][n], info (what
    check_store takes), and with track_pairs pair_bound [cap]: an a-priori bound of |A p_k - q_k|_2 per slot, from
        A p_k - q_k = (fl(A z) - A z - sum_j h_j (A p_j - q_j) + roundings of w' and p) / |w'|:
    E_k = (sum_j |h_j| E_j + (L + 6 m + 6) eps (| |A| |z| | + sum_j |h_j| (| |A| |p_j| | + 1))) / |w'|, L the longest row, m the live
    columns (two roundings per column and entry in each of the two passes over w' and in p, the sum of the two passes'
    coefficients, the division)."""
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    if resume is None:
        store = ks.GcrStoreRef(cap)
        Q, P = np.zeros((cap, n)), np.zeros((cap, n))
        pair_bound, ap_norm = np.zeros(cap), np.zeros(cap)
    else:
        assert resume["store"].cap == cap
        store, Q, P, pair_bound, ap_norm = (resume[k] for k in ("store", "Q", "P", "pair_bound", "ap_norm"))
    L = int(A.row_nnz.max())
    nrm = (lambda v: float(np.sqrt(np.sum(v.astype(LD) ** 2)))) if dots == "longdouble" else (lambda v: float(np.sqrt(v @ v)))
    x, r = np.zeros(n), b.copy()
    bnorm = nrm(b)
    out = {"iters": 0, "restarts": 0, "cycles": 0, "arnoldi_steps": 0}
    if bnorm == 0.0:
        rnorm = 0.0
    iters = stalls = 0
    rstart = rnorm = bnorm
    for cyc in range(8):
        if bnorm == 0.0 or iters >= max_it:
            break
        out["cycles"] += 1
        target = rtol * bnorm
        store.clear_window()
        live = [j for j in range(store.hw) if store.born[j] >= 0]
        r_entry = nrm(r)
        if live:
            h = _dots(Q[live], r, dots)
            r = r - h @ Q[live]
            x = x + h @ P[live]
        rnorm = nrm(r)
        src, best, since_gain = r, rnorm, 0
        stagnated = stalled = False
        while rnorm > target and iters < max_it:
            end = ks.gcr_cycle_end_ref(since_gain, False, rnorm, target, r_entry, store.full())
            if end:
                stagnated, stalled = end == 1, end == 2
                break
            z = np.asarray(M(src), dtype=np.float64)
            w = A.dot(z)
            if store.full():
                for s in store.retire(ks.gcr_retire_batch(cap)):
                    Q[s] = 0.0
                    P[s] = 0.0
                store.window_drop_retired()
            slot, _ = store.take()
            live = [j for j in range(store.hw) if store.born[j] >= 0]
            htot = np.zeros(len(live))
            for _pass in range(2):
                if live:
                    h = _dots(Q[live], w, dots)
                    w = w - h @ Q[live]
                    htot += h
            wn = nrm(w)
            if not (wn > 0.0 and np.isfinite(wn)):
                raise ArithmeticError(f"gcr_twin: breakdown, |w'| = {wn} at iteration {iters}")
            q = w / wn
            p = (z - htot @ P[live]) / wn if live else z / wn
            alpha = float(_dots(q[None, :], r, dots)[0])
            r = r - alpha * q
            x = x + alpha * p
            src = r
            if alpha * alpha <= escape * rnorm * rnorm:
                src = q
                out["arnoldi_steps"] += 1
            if track_pairs:
                ha = np.abs(htot)
                pair_bound[slot] = (ha @ pair_bound[live] + (L + 6 * len(live) + 6) * EPS
                                    * (float(np.linalg.norm(A.absdot(z))) + ha @ (ap_norm[live] + 1.0))) / wn
                ap_norm[slot] = float(np.linalg.norm(A.absdot(p)))
            Q[slot], P[slot] = q, p
            store.set_born(slot)
            iters += 1
            rnorm = nrm(r)
            if rnorm < 0.9 * best:
                best, since_gain = rnorm, 0
            else:
                since_gain += 1
        # the answer of every cycle is judged on b - A x (judge_fp64_cycle, with the verdict always due)
        r = true_residual(A, b, x)[0].astype(np.float64)
        rnorm = nrm(r)
        if rnorm <= rtol * bnorm:
            break
        if rtol <= 1e-9 and rnorm <= 100.0 * rtol * bnorm and (stagnated or cyc >= 1):
            break
        if iters >= max_it:
            break
        if stalled or not rnorm < 0.5 * rstart:
            if stalls >= 2:
                break
            stalls += 1
            out["restarts"] += 1
            store.reset()
            Q[:], P[:] = 0.0, 0.0
            pair_bound[:], ap_norm[:] = 0.0, 0.0
        rstart = rnorm
    info = {"cap": cap, "hw": store.hw, "made": store.made, "free": list(store.free), "born": list(store.born),
            "hot_slots": list(store.hot), "kry_fp32": 0, "ndof": n}
    out.update(x=x, iters=iters, relres=(norm(true_residual(A, b, x)[0]) / bnorm if bnorm > 0.0 else 0.0), store=store, Q=Q, P=P,
               info=info, pair_bound=pair_bound, ap_norm=ap_norm)
    return out
