"""The monolithic multicolour ILU(0) path (precond = 1 of include/vaspfsi.h) one launch function at a time on an MI355X:
launch_ilu0_levels (k_ilu0_level) and launch_sptrsv_levels (k_sptrsv_level<false / true>) through libfsi_kernel_shim.so.

The factor is held to the DEFINITION of ILU(0), not to another factorisation: with non-zero pivots the unit-lower L and upper U on
the pattern of A are the unique pair with (L U)_ij = a_ij at every pattern position, and the device's factor must satisfy that
identity entry by entry within the componentwise backward error of Doolittle elimination, (n_ij + 2) eps S_ij
(ks.ilu0_identity: extended precision, valid for any order of the updates, with or without FMA contraction).  The triangular
solves are held row by row to their own equations (ks.sptrsv_residuals) with bounds that hold for any order of the wave's sum.
tests/test_kernel_references.py shows on the CPU that a plain FP64 IKJ factor passes the identity and that a dropped update, the
unfactored pivot of a row of the same group and an update applied to the neighbouring column each fail it, so a kernel with a
missed update, a stale hand-off between the rows of a node or a wrong column match cannot pass here.

Every test prints the largest error / bound it saw; none of the bounds is tuned on the kernels' output."""
import time

import numpy as np
import pytest

import kernel_shim as ks

pytestmark = pytest.mark.gpu

NAN = float("nan")
MIXED = [(40, 6), (33, 6), (1, 6), (0, 6), (25, 1), (17, 1)]          # an empty level must be skipped
LENGTHS = [(40, 6), (200, 6), (30, 1), (20, 1)]
N_LENGTHS = 40 * 6 + 200 * 6 + 50
# rows of 1024 entries (MAXROW) with the diagonal first (first level, nlow = 0) and last (last level, nlow = 1023), the diagonal
# alone, and lengths around the lane count and two strips of it
HEAVY = [3, N_LENGTHS - 5, 250, 251, 252, 253, 1447]
HEAVY_LEN = [1024, 1024, 1, 63, 64, 65, 129]


def levels_of(m):
    return len(m["first"]), m["first"], m["ngroups"], m["group_rows"]


def factor(m, vals=None):
    """launch_ilu0_levels on the matrix: (LU, counters[1]); the other counters must come back zero and the tail untouched"""
    nnz = len(m["cols"])
    LU = ks.out(nnz, np.float64, NAN)
    LU[:nnz] = m["vals"] if vals is None else vals
    counters = np.full(4, 77, dtype=np.int32)          # the launch function zeroes all four first
    ks.call("shim_ilu0", m["n"], *levels_of(m), m["rowptr"], m["cols"], m["diagpos"], LU, counters)
    assert ks.tail_untouched(LU, nnz, NAN), "written past the end of LU"
    assert counters[0] == 0 and counters[2] == 0 and counters[3] == 0
    return LU[:nnz].copy(), int(counters[1])


def solve(m, LU, rhs):
    """launch_sptrsv_levels: (y, x) of L y = rhs, U x = y"""
    n = m["n"]
    y, x = ks.out(n, np.float64, NAN), ks.out(n, np.float64, NAN)
    ks.call("shim_sptrsv", n, *levels_of(m), m["rowptr"], m["cols"], m["diagpos"], np.ascontiguousarray(LU), rhs, y, x)
    assert ks.tail_untouched(y, n, NAN) and ks.tail_untouched(x, n, NAN)
    return y[:n].copy(), x[:n].copy()


def identity_ratio(m, LU, what, skip_rows=()):
    err, bound = ks.ilu0_identity(m["rowptr"], m["cols"], m["diagpos"], m["vals"], LU)
    for r in skip_rows:
        err[m["rowptr"][r]:m["rowptr"][r + 1]] = 0
    r = ks.worst_ratio(err, bound)
    print(f"{what}: ILU(0) identity, largest error / bound {r:.3f} over {len(err)} entries")
    return r


def solve_ratios(m, LU, rhs, y, x, what):
    ef, bf, eb, bb = ks.sptrsv_residuals(m["rowptr"], m["cols"], m["diagpos"], LU, rhs, y, x)
    rf, rb = ks.worst_ratio(ef, bf), ks.worst_ratio(eb, bb)
    print(f"{what}: forward sweep largest error / bound {rf:.3f}, backward sweep {rb:.3f}")
    return rf, rb


MATRICES = {
    "mixed-symmetric": lambda: ks.level_matrix(MIXED, np.random.default_rng(21), symmetric=True),
    "mixed-unsymmetric": lambda: ks.level_matrix(MIXED, np.random.default_rng(22), symmetric=False),
    # a third of the strictly lower entries exactly 0.0: the kernel skips the update of such an entry (l != 0)
    "zero-lower-entries": lambda: ks.level_matrix(MIXED, np.random.default_rng(23), symmetric=False, zero_lower=0.33),
    # a node's d / v rows: row rr of a group needs the factored rows 0 .. rr - 1 of its own group, handed over through global memory
    "node-coupling": lambda: ks.level_matrix([(12, 6), (5, 6), (7, 1)], np.random.default_rng(24), row_len=12),
    "own-group-only": lambda: ks.level_matrix([(9, 6), (4, 1), (6, 6)], np.random.default_rng(25), own_group_only=True),
    "row-lengths": lambda: ks.level_matrix(LENGTHS, np.random.default_rng(26), heavy=HEAVY, heavy_len=HEAVY_LEN, diag_first=[3],
                                           diag_last=[N_LENGTHS - 5]),
}


@pytest.fixture(scope="module")
def factored():
    """every synthetic matrix with its device factor, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            m = MATRICES[name]()
            assert ks.level_violations(list(zip(m["ngroups"], m["group_rows"])), m["rowptr"], m["cols"]) == 0
            cache[name] = (m,) + factor(m)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(MATRICES))
def test_ilu0_factor_satisfies_the_ilu0_identity(factored, name):
    m, LU, flags = factored(name)
    assert flags == 0
    if name == "row-lengths":
        L = np.diff(m["rowptr"])
        assert [int(L[r]) for r in HEAVY] == HEAVY_LEN and L.max() == ks.ILU_MAXROW
        assert m["diagpos"][3] == m["rowptr"][3] and m["diagpos"][N_LENGTHS - 5] == m["rowptr"][N_LENGTHS - 4] - 1
    if name == "zero-lower-entries":
        row = np.repeat(np.arange(m["n"]), np.diff(m["rowptr"]))
        assert np.count_nonzero((m["vals"] == 0.0) & (m["cols"] < row)) > 100
    assert identity_ratio(m, LU, name) <= 1.0


def test_ilu0_of_uncoupled_groups_is_the_exact_lu_of_each_block(factored):
    """Groups coupled ONLY to themselves: ILU(0) drops nothing, so the factor of each 6 x 6 block is its LU factorisation without
    pivoting (the blocks are diagonally dominant, cond < 100).  Reference: Doolittle elimination in extended precision.  Bound, to
    first order (Higham, Accuracy and Stability, theorem 9.15, Barrlund): |dU|_F / |U|_F and |dL|_F / |L|_F <= chi |dA|_F / |A|_F
    with chi = |L^-1|_2 |U^-1|_2 |A|_2 and |dA| <= 8 eps |L||U| the backward error of a 6 x 6 elimination; twice that here for the
    higher-order terms."""
    m, LU, flags = factored("own-group-only")
    assert flags == 0
    import scipy.sparse as sp
    n = m["n"]
    A = sp.csr_matrix((m["vals"], m["cols"], m["rowptr"]), shape=(n, n)).toarray()
    F = sp.csr_matrix((LU, m["cols"], m["rowptr"]), shape=(n, n)).toarray()
    worst = 0.0
    for g in np.unique(m["group_of"]):
        sel = m["group_of"] == g
        B, k = A[np.ix_(sel, sel)].astype(np.longdouble), int(sel.sum())
        assert np.linalg.cond(B.astype(np.float64)) < 100
        W = B.copy()
        for c in range(k):                                      # Doolittle, no pivoting
            W[c + 1:, c] /= W[c, c]
            W[c + 1:, c + 1:] -= np.outer(W[c + 1:, c], W[c, c + 1:])
        Lr, Ur = (np.tril(W, -1) + np.eye(k)).astype(np.float64), np.triu(W).astype(np.float64)
        Fg = F[np.ix_(sel, sel)]
        chi = np.linalg.norm(np.linalg.inv(Lr), 2) * np.linalg.norm(np.linalg.inv(Ur), 2) * np.linalg.norm(B.astype(np.float64), 2)
        rel = 8 * ks.EPS64 * np.linalg.norm(np.abs(Lr) @ np.abs(Ur)) / np.linalg.norm(B.astype(np.float64))
        for got, ref in ((np.triu(Fg), Ur), (np.tril(Fg, -1) + np.eye(k), Lr)):
            err, bound = np.linalg.norm(got - ref), 2 * chi * rel * np.linalg.norm(ref)
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
    print(f"own-group-only: factor against the exact LU of each block, largest error / bound {worst:.3f}")
    assert worst <= 1.0


def test_ilu0_grid_stride_over_more_groups_than_workgroups():
    """One level of 16384 + 129 groups of six rows (the launch is capped at 16384 workgroups, so 129 of them take a second group)
    and a second level that depends on it.  99 318 rows are too many for the extended-precision row loops: the identity is
    evaluated with scipy's FP64 sparse products (ks.ilu0_identity_f64), whose own rounding is of the size of the bound, so the
    error is held to TWICE the bound here."""
    m = ks.level_matrix([(16384 + 129, 6), (40, 6)], np.random.default_rng(27), symmetric=False, row_len=8)
    assert 7.5 <= np.diff(m["rowptr"]).mean() <= 8.5
    LU, flags = factor(m)
    assert flags == 0
    err, bound = ks.ilu0_identity_f64(m["rowptr"], m["cols"], m["diagpos"], m["vals"], LU)
    r = ks.worst_ratio(err, 2 * bound)
    print(f"grid stride: ILU(0) identity in FP64, largest error / (2 x bound) {r:.3f} over {len(err)} entries")
    assert r <= 1.0
    assert not np.array_equal(LU[m["rowptr"][6 * 16384]:], m["vals"][m["rowptr"][6 * 16384]:])      # the second pass did factor its rows


def test_ilu0_error_flags():
    """What the kernel refuses in code (no fault involved): a row longer than its LDS tile is left as it is and flagged 1; a pivot
    that is exactly zero or not finite is flagged 2 and stored as 1.0."""
    # a row of 1025 entries that no other row depends on
    r = 1460
    m = ks.level_matrix(LENGTHS, np.random.default_rng(28), heavy=[r], heavy_len=[1025], isolated=[r])
    assert m["rowptr"][r + 1] - m["rowptr"][r] == ks.ILU_MAXROW + 1
    LU, flags = factor(m)
    assert flags == 1
    s, e = m["rowptr"][r], m["rowptr"][r + 1]
    assert LU[s:e].tobytes() == m["vals"][s:e].tobytes()                       # bit for bit as given
    assert identity_ratio(m, LU, "row of 1025 entries (every other row)", skip_rows=[r]) <= 1.0
    # [[1, 1], [1, 1]] as one group of two rows: the second pivot cancels to exactly zero
    two = dict(n=2, first=np.zeros(1, dtype=np.int64), ngroups=np.ones(1, dtype=np.int64), group_rows=np.full(1, 2, dtype=np.int32),
               rowptr=np.array([0, 2, 4], dtype=np.int64), cols=np.array([0, 1, 0, 1], dtype=np.int32),
               diagpos=np.array([0, 3], dtype=np.int64), vals=np.ones(4))
    LU, flags = factor(two)
    assert flags == 2
    np.testing.assert_array_equal(LU, [1.0, 1.0, 1.0, 1.0])                  # l = 1, and the stored pivot 1.0 in place of 0
    # a NaN diagonal
    d3 = dict(n=3, first=np.zeros(1, dtype=np.int64), ngroups=np.full(1, 3, dtype=np.int64), group_rows=np.ones(1, dtype=np.int32),
              rowptr=np.arange(4, dtype=np.int64), cols=np.arange(3, dtype=np.int32), diagpos=np.arange(3, dtype=np.int64),
              vals=np.array([2.0, NAN, -3.0]))
    LU, flags = factor(d3)
    assert flags == 2
    np.testing.assert_array_equal(LU, [2.0, 1.0, -3.0])


# ---- triangular solves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["device-factor", "random-values"])
@pytest.mark.parametrize("name", list(MATRICES))
def test_sptrsv_rows_satisfy_their_equations(factored, name, which):
    """L y = rhs and U x = y row by row, with the device's own factor and with random values in its place (the matrix's entries:
    random in [-1, 1] under a dominant diagonal, so that the substitution does not overflow)"""
    m, LU, _ = factored(name)
    if which == "random-values":
        LU = m["vals"]
    n = m["n"]
    row = np.repeat(np.arange(n), np.diff(m["rowptr"]))
    low, up = np.bincount(row[m["cols"] < row], minlength=n), np.bincount(row[m["cols"] > row], minlength=n)
    assert np.any(low == 0) and np.any(up == 0)                                # rows with an empty lower / upper part
    if name in ("node-coupling", "mixed-symmetric"):                           # rows of a group depend on each other in both sweeps
        same = m["group_of"][row] == m["group_of"][m["cols"]]
        assert np.any(same & (m["cols"] < row)) and np.any(same & (m["cols"] > row))
    rhs = np.random.default_rng(31).standard_normal(n)
    y, x = solve(m, LU, rhs)
    rf, rb = solve_ratios(m, LU, rhs, y, x, f"{name}, {which}")
    assert rf <= 1.0 and rb <= 1.0


def test_sptrsv_grid_stride_over_more_groups_than_waves():
    """One level of 32768 + 70 groups of one row: the launch is capped at 8192 workgroups of four waves, so 70 waves take a second
    row; a second level couples the rows."""
    m = ks.level_matrix([(32768 + 70, 1), (500, 1)], np.random.default_rng(32), symmetric=True, row_len=6)
    rhs = np.random.default_rng(33).standard_normal(m["n"])
    y, x = solve(m, m["vals"], rhs)
    rf, rb = solve_ratios(m, m["vals"], rhs, y, x, "grid stride")
    assert rf <= 1.0 and rb <= 1.0


def test_sptrsv_of_uncoupled_groups_solves_each_block(factored):
    """On the block diagonal matrix the two sweeps with the device's factor solve every block: x against numpy.linalg.solve of
    the block, within 16 eps cond(block) |x| (blocks built with cond < 100)."""
    m, LU, _ = factored("own-group-only")
    import scipy.sparse as sp
    n = m["n"]
    A = sp.csr_matrix((m["vals"], m["cols"], m["rowptr"]), shape=(n, n)).toarray()
    rhs = np.random.default_rng(34).standard_normal(n)
    _, x = solve(m, LU, rhs)
    worst = 0.0
    for g in np.unique(m["group_of"]):
        sel = m["group_of"] == g
        B = A[np.ix_(sel, sel)]
        cond = np.linalg.cond(B)
        assert cond < 100
        ref = np.linalg.solve(B, rhs[sel])
        worst = max(worst, np.abs(x[sel] - ref).max() / (16 * ks.EPS64 * cond * np.abs(ref).max()))
    print(f"own-group-only: x against the solve of each block, largest error / bound {worst:.3f}")
    assert worst <= 1.0


# ---- the real matrix --------------------------------------------------------------------------------------------------------------
def test_ilu0_path_on_the_cylinder_jacobian(cylinder_case, monkeypatch):
    """The context's own matrix (cylinder fixture, FSI_ORDER=colour, precond = 1, Jacobian at the golden states 0 and 1 as in
    test_bicgstab_and_ilu0_solve_match_sparse_lu): (i) the multicolour ordering obeys the contract of the level kernels, (ii) the
    factor refresh_preconditioner left in the context satisfies the ILU(0) identity on the row-equilibrated Jacobian (penalty rows
    of 1e7, condition number ~1e12: the bound is scale-free; FP64 products, so twice the bound as in the grid-stride test), (iii)
    the context's preconditioner application is the two sweeps with that factor, and they satisfy their equations."""
    from conftest import GOLDEN
    from test_gpu_parity import boundary_data
    from vasp_amd.capi import HipBackend
    monkeypatch.setenv("FSI_ORDER", "colour")
    hb = HipBackend(cylinder_case[1], lin_solver=0, precond=1)
    try:
        gold = np.load(GOLDEN / "cylinder_tight.npz")["states"]
        g, P = boundary_data(cylinder_case, 3e-3)
        hb.set_state("n", gold[1].copy()); hb.set_state("n-1", gold[0].copy()); hb.set_dirichlet_values(g); hb.set_interface_pressure(P)
        hb.assemble_residual()
        hb.assemble_jacobian()                                                  # refreshes the preconditioner: the factor
        info = ks.ctx_info(hb.ctx)
        N2, V, n = info["N2"], info["V"], hb.ndof
        lv = ks.ctx_levels(hb.ctx)
        rowptr, cols, diagpos = (ks.ctx_array(hb.ctx, k) for k in ("rowptr", "cols", "diagpos"))
        A, LU = ks.ctx_array(hb.ctx, "A"), ks.ctx_array(hb.ctx, "LU")
        # (i) the colouring contract
        assert len(lv) % 2 == 0 and len(lv) >= 2
        nxt = 0
        for k, (first, ngroups, group_rows) in enumerate(lv):
            assert first == nxt and ngroups >= 0                                # the levels tile 0 .. n without gaps
            assert group_rows == (6 if k < len(lv) // 2 else 1)                 # d / v levels, then pressure levels
            nxt = first + ngroups * group_rows
            if k == len(lv) // 2 - 1:
                assert nxt == 6 * N2
        assert nxt == n == 6 * N2 + V
        levels = [(ng, gr) for _, ng, gr in lv]
        assert ks.level_violations(levels, rowptr, cols) == 0, "a row references another group of its own colour: number_nodes"
        np.testing.assert_array_equal(cols[diagpos], np.arange(n))              # every row has its diagonal entry
        assert np.diff(rowptr).max() <= ks.ILU_MAXROW
        # (ii) the factor
        assert not np.array_equal(A, LU)
        t0 = time.time()
        err, bound = ks.ilu0_identity_f64(rowptr, cols, diagpos, A, LU)
        r = ks.worst_ratio(err, 2 * bound)
        print(f"cylinder ({n} rows, {len(cols)} entries, {len(lv)} levels): ILU(0) identity in FP64, largest error / (2 x bound) {r:.3f} "
              f"({time.time() - t0:.1f} s on the host)")
        assert r <= 1.0
        # (iii) the preconditioner application: fsi_apply_preconditioner permutes to the solver's order, scales by rowscale, runs the
        # two sweeps and permutes back; the same sweeps through the shim give the same bits, and satisfy their equations
        u2s, rs = ks.ctx_array(hb.ctx, "user2solver").astype(np.int64), ks.ctx_array(hb.ctx, "rowscale")
        res = np.random.default_rng(41).standard_normal(n)
        z = hb.apply_preconditioner(res)
        rhs = np.zeros(n)
        rhs[u2s] = res
        rhs *= rs
        m = dict(n=n, first=np.array([l[0] for l in lv], dtype=np.int64), ngroups=np.array([l[1] for l in lv], dtype=np.int64),
                 group_rows=np.array([l[2] for l in lv], dtype=np.int32), rowptr=rowptr, cols=cols, diagpos=diagpos)
        y, x = solve(m, LU, rhs)
        assert z.tobytes() == x[u2s].tobytes()
        rf, rb = solve_ratios(m, LU, rhs, y, x, "cylinder")
        assert rf <= 1.0 and rb <= 1.0
    finally:
        hb.close()
