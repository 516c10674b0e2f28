"""The references of tests/gcr_solve.py on the CPU, so that a failure of tests/test_gpu_gcr_solve.py is one of the device code, not
of its reference: the twin solves a synthetic system and leaves a consistent store at a capacity that rotates hard (8), one that
rotates (40) and one that never fills (600); check_store and true_residual reject each planted defect."""
import numpy as np
import pytest

import gcr_solve as gs
import kernel_shim as ks

N = 301                      # odd, and no multiple of 4: the sizes at which the device pads its columns
RTOL = 1e-10
ESCAPE = 1e-3                # FsiTuning.gcr_escape's default


@pytest.fixture(scope="module")
def system():
    """A nonsymmetric, well conditioned sparse matrix and M = A^-1 (I + E), |E|_2 about 1.7: GCR needs about a hundred
    iterations to 1e-10, so a store of 8 turns its ring of 4 thirty times and a store of 40 its ring of 20 three times."""
    rng = np.random.default_rng(5)
    A = np.diag(1.0 + 3.0 * rng.random(N)) + 0.3 * rng.standard_normal((N, N)) * (rng.random((N, N)) < 0.05)
    M = np.linalg.inv(A) @ (np.eye(N) + 0.85 * rng.standard_normal((N, N)) / np.sqrt(N))
    return A, gs.Csr.from_dense(A), M, rng.standard_normal(N)


@pytest.fixture(scope="module")
def twins(system):
    A, csr, M, b = system
    return {(cap, dots): gs.gcr_twin(csr, lambda v: M @ v, b, RTOL, 4000, cap, ESCAPE, dots, track_pairs=True)
            for cap in (8, 40, 600) for dots in ("longdouble", "float64")}


def columns(o):
    hw = o["store"].hw
    return o["Q"][:hw].copy(), o["P"][:hw].copy()


@pytest.mark.parametrize("dots", ["longdouble", "float64"])
@pytest.mark.parametrize("cap", [8, 40, 600])
def test_twin_converges_and_leaves_a_consistent_store(cap, dots, system, twins):
    A, csr, M, b = system
    o = twins[cap, dots]
    r, bound = gs.true_residual(csr, b, o["x"])
    assert gs.norm(r) <= RTOL * gs.norm(b), (gs.norm(r) / gs.norm(b), o["iters"])
    assert o["relres"] == gs.norm(r) / gs.norm(b)
    assert o["restarts"] == 0 and o["cycles"] == 1 and o["store"].made == o["iters"]
    if cap < 600:
        assert o["store"].made > 2 * cap and o["store"].hw == cap          # the store has rotated
    else:
        assert o["store"].hw == o["iters"] < cap
    Q, P = columns(o)
    gs.check_store(o["info"], Q, P)
    # the pairs are pairs, each within the bound the twin carried along, and the columns are orthonormal: classical
    # Gram-Schmidt twice leaves |q_i . q_j - delta_ij| at a small multiple of n eps whatever the cancellation
    live = [s for s in range(o["store"].hw) if o["store"].born[s] >= 0]
    for s in live:
        assert np.linalg.norm(A @ P[s] - Q[s]) <= o["pair_bound"][s], (s, o["store"].born[s])
    G = Q[live] @ Q[live].T - np.eye(len(live))
    assert np.abs(G).max() <= 8 * N * gs.EPS, np.abs(G).max()
    print(f"twin cap {cap} {dots}: {o['iters']} iterations, relres {o['relres']:.3e}, kept {len(live)}, "
          f"max |A p - q| / bound {max(np.linalg.norm(A @ P[s] - Q[s]) / o['pair_bound'][s] for s in live):.3f}")


def test_twin_recycles_its_store(system):
    """a second solve with the pairs of the first: the projection alone answers the same right-hand side"""
    A, csr, M, b = system
    o = gs.gcr_twin(csr, lambda v: M @ v, b, 1e-8, 4000, 600, ESCAPE)
    live = list(range(o["store"].hw))
    h = o["Q"][live] @ b
    x = h @ o["P"][live]
    assert gs.norm(gs.true_residual(csr, b, x)[0]) <= 1e-8 * gs.norm(b)


def rotated_with_a_free_slot(twins):
    """the store of capacity 40 after its rotation, with free slots (had the solve ended on a full store: one more batch retired,
    as gcr_make_room does)"""
    o = twins[40, "longdouble"]
    info = dict(o["info"])
    store = ks.GcrStoreRef(40)
    store.born, store.free, store.hw, store.made = list(info["born"]), list(info["free"]), info["hw"], info["made"]
    Q, P = columns(o)
    if not store.free:
        assert store.full()
        for s in store.retire(ks.gcr_retire_batch(40)):
            Q[s] = 0.0
            P[s] = 0.0
    info.update(born=list(store.born), free=list(store.free))
    return info, Q, P


def test_check_store_rejects_a_nonzero_entry_in_a_free_column(twins):
    info, Q, P = rotated_with_a_free_slot(twins)
    gs.check_store(info, Q, P)
    assert len(info["free"]) >= 4
    for which, pos in ((Q, N - 1), (P, 0), (Q, 0)):
        saved = which[info["free"][3], pos]
        which[info["free"][3], pos] = 5e-324                 # one bit
        with pytest.raises(AssertionError, match="free slot"):
            gs.check_store(info, Q, P)
        which[info["free"][3], pos] = saved
    Q[info["free"][0], 7] = -0.0                             # the sign bit alone: not what a memset leaves
    with pytest.raises(AssertionError, match="free slot"):
        gs.check_store(info, Q, P)


def test_check_store_rejects_a_born_duplicate_and_a_wrong_count(twins):
    info, Q, P = rotated_with_a_free_slot(twins)
    live = [s for s in range(info["hw"]) if info["born"][s] >= 0]
    bad = dict(info, born=list(info["born"]))
    bad["born"][live[-1]] = bad["born"][live[-2]]
    with pytest.raises(AssertionError, match="born"):
        gs.check_store(bad, Q, P)
    bad = dict(info, born=list(info["born"]))
    bad["born"][live[-1]] = info["made"]                     # an index that has not been made yet
    with pytest.raises(AssertionError, match="below made"):
        gs.check_store(bad, Q, P)
    bad = dict(info, free=info["free"][:-1])                 # a retired slot that is not on the free list
    with pytest.raises(AssertionError, match="kept|free list"):
        gs.check_store(bad, Q, P)
    bad = dict(info, hot_slots=[info["free"][0]] + [-1] * (ks.GCR_WINDOW - 1))
    with pytest.raises(AssertionError, match="window"):
        gs.check_store(bad, Q, P)


def test_check_store_rejects_a_missing_protected_direction(twins):
    info, Q, P = rotated_with_a_free_slot(twins)
    protect = 40 - ks.gcr_ring(40)
    assert sorted(b for b in info["born"] if 0 <= b < protect) == list(range(protect))
    slot = info["born"].index(protect - 1)
    # retired as retire() would have retired it had the protect rule been off by one: column zeroed, slot on the free list
    bad = dict(info, born=list(info["born"]), free=info["free"] + [slot])
    bad["born"][slot] = -1
    Q[slot] = 0.0
    P[slot] = 0.0
    with pytest.raises(AssertionError, match="protect rule"):
        gs.check_store(bad, Q, P)


def fp32_store(rng, n=N, cap=40, hw=37, first=3):
    """an FP32 store as a cycle of 34 iterations leaves it: every q = w / |w'| with |w'|^2 an FP64 sum of squares, rounded once
    into KQ and kept in the window, which has wrapped (34 > 32)"""
    ldq = (n + 3) & ~3
    Q, Qh, Z = np.zeros((hw, ldq), dtype=np.float32), np.zeros((ks.GCR_WINDOW, ldq)), np.zeros((hw, n + 1))
    store = ks.GcrStoreRef(cap)
    for s in range(hw):
        slot, _ = store.take()
        w = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3)
        q = w * (1.0 / np.sqrt(w @ w))
        Q[slot, :n] = q.astype(np.float32)
        Z[slot, :n] = rng.standard_normal(n)
        if s >= first:
            Qh[store.window_put(slot), :n] = q
        store.set_born(slot)
    info = {"cap": cap, "hw": hw, "made": store.made, "free": [], "born": list(store.born), "hot_slots": list(store.hot),
            "kry_fp32": 1, "ndof": n}
    assert store.window_cols() == ks.GCR_WINDOW and store.hot_next == (hw - first) % ks.GCR_WINDOW
    return info, Q, Z, Qh


def test_check_store_rejects_a_window_column_whose_fp32_image_differs_in_one_bit():
    info, Q, Z, Qh = fp32_store(np.random.default_rng(11))
    gs.check_store(info, Q, Z, Qh)
    k = 17
    s = info["hot_slots"][k]
    for pos in (0, N - 1, 123):
        saved = Q[s, pos]
        Q[s, pos] = np.nextafter(saved, np.float32(2.0))     # the last bit of one entry
        with pytest.raises(AssertionError, match=f"window column {k}"):
            gs.check_store(info, Q, Z, Qh)
        Q[s, pos] = saved
    # the window's column against a neighbour's slot (an offset of one column in KQh)
    bad = dict(info, hot_slots=info["hot_slots"][1:] + info["hot_slots"][:1])
    with pytest.raises(AssertionError, match="window column"):
        gs.check_store(bad, Q, Z, Qh)
    # a column that is not a unit vector: scaled by 1 + 2^-44, far inside FP32 rounding, so its image may well be the same
    Qh[k] *= 1.0 + 2.0 ** -44
    Q[s] = Qh[k].astype(np.float32)
    with pytest.raises(AssertionError, match=r"\|q\|\^2 - 1"):
        gs.check_store(info, Q, Z, Qh)
    with pytest.raises(AssertionError, match="fetched as"):
        gs.check_store(dict(info, kry_fp32=0), Q, Z, Qh)


def test_true_residual_rejects_one_entry_moved_by_1e_6(system):
    A, csr, M, b = system
    x = np.linalg.solve(A, b)
    r, bound = gs.true_residual(csr, b, x)
    ref = b.astype(gs.LD) - A.astype(gs.LD) @ x.astype(gs.LD)
    assert gs.norm(r - ref) <= 4 * np.finfo(gs.LD).eps * csr.row_nnz.max() * gs.norm(csr.absdot(x) + np.abs(b))
    assert gs.norm(r) <= 8 * bound                      # a backward stable solve's residual is a small multiple of the bound
    r64 = b - csr.dot(x)                                # the FP64 evaluation the bound is stated for
    assert gs.norm(r64.astype(gs.LD) - r) <= bound
    bn = gs.norm(b)
    for i in (0, N // 2, N - 1):
        y = x.copy()
        y[i] *= 1.0 + 1e-6
        ry, by = gs.true_residual(csr, b, y)
        assert abs(gs.norm(ry) - gs.norm(r)) > 1e3 * (bound + by), (i, gs.norm(ry), bound)
        assert gs.norm(ry) / bn > 1e-10                 # and a solve that claims 1e-10 with this x is caught
