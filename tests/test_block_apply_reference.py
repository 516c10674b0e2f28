"""The host restatement of one block-preconditioner application (tests/block_apply.py) against what it restates and against
mathematics, without a GPU: the Chebyshev schedules meet their bounds, a chain without its last sweep hands its consumer the
full chain's result, the restarted tail chain of a two-level cycle is a fresh chain on the corrected residual, the composed
stages invert a block system whose factorisation is exact, and the map of ctx->blk is the one of BlockApply's constructor.
A failure of tests/test_gpu_block_application.py is then one of the library and not of its reference."""
import re
from pathlib import Path

import numpy as np
import pytest

import block_apply as ba
import kernel_shim as ks

LD, F32, F64 = np.longdouble, np.float32, np.float64


def spd_rows(n, seed, kappa_like=50.0):
    """an SPD matrix on a banded graph, as Rows and dense, with its Jacobi-scaled spectrum's ends"""
    rng = np.random.default_rng(seed)
    ptr, cols = ks.local_graph(n, rng, reach=6, max_deg=6)
    row = np.repeat(np.arange(n), np.diff(ptr))
    M = np.zeros((n, n))
    M[row, cols] = rng.uniform(-1, 0, len(cols))
    M = 0.5 * (M + M.T)
    np.fill_diagonal(M, 0.0)
    np.fill_diagonal(M, np.abs(M).sum(axis=1) * (1.0 + 1.0 / kappa_like) + 0.05)
    import scipy.sparse as sp
    lam = np.linalg.eigvalsh(M / np.sqrt(np.outer(np.diag(M), np.diag(M))))
    return ba.rows_of_csr(sp.csr_matrix(M)), M, lam.min(), lam.max()


@pytest.mark.parametrize("fourth", [0, 1])
def test_coefficients_are_the_library_s(fourth):
    n = 24
    c1, c2, init = np.zeros(2 * n), np.zeros(2 * n), np.zeros(1)
    ks.call("shim_cheb_coefficients", 1.7, 35.0, fourth, n, c1, c2, init)
    i0, a, b = ba.coefficients(1.7, 35.0, bool(fourth), n)
    assert i0 == init[0]
    assert np.array_equal(np.concatenate([a, b]), np.stack([c1, c2], axis=1))


@pytest.mark.parametrize("k", [1, 2, 5, 12, 30])
def test_classic_schedule_meets_the_chebyshev_bound(k):
    """On [lmax / kappa, lmax] containing the Jacobi-scaled spectrum, k directions reduce the error in the energy norm by
    2 rho^k / (1 + rho^2k), rho = (sqrt(kappa) - 1) / (sqrt(kappa) + 1)."""
    A, M, lo, hi = spd_rows(120, 3)
    lmax, kappa = 1.02 * hi, 1.05 * hi / lo
    rng = np.random.default_rng(k)
    xstar = rng.standard_normal(120)
    b = M @ xstar
    x = ba.run_chain(A, ba.over(np.diag(M)), ba.Schedule(lmax, kappa), b, k, LD).astype(F64)
    en = lambda e: np.sqrt(e @ M @ e)      # noqa: E731
    rho = (np.sqrt(kappa) - 1) / (np.sqrt(kappa) + 1)
    bound = 2 * rho ** k / (1 + rho ** (2 * k))
    assert en(x - xstar) <= bound * en(xstar) * (1 + 1e-9), (en(x - xstar) / en(xstar), bound)
    assert en(x - xstar) >= 1e-3 * bound * en(xstar) or k > 12      # and it is this polynomial, not a better solver


@pytest.mark.parametrize("k", [1, 2, 3, 7, 16])
def test_fourth_kind_schedule_is_its_polynomial(k):
    """On a diagonal matrix the residual after k directions is W_k(1 - 2 lam / lmax) / (2 k + 1) times the first one, W_k the
    Chebyshev polynomial of the 4th kind, W_k(cos t) = sin((k + 1/2) t) / sin(t / 2)  (Lottes 2022)."""
    lmax = 2.3
    lam = np.linspace(0.01, 1.0, 97) * lmax
    import scipy.sparse as sp
    A = ba.rows_of_csr(sp.diags(lam).tocsr())
    b = np.ones(len(lam))
    x = ba.run_chain(A, ba.identity, ba.Schedule(lmax, 1e9, True), b, k, LD)
    res = (b - lam * x).astype(F64)
    t = np.arccos(1 - 2 * lam / lmax)
    want = np.sin((k + 0.5) * t) / np.sin(0.5 * t) / (2 * k + 1)
    assert np.abs(res - want).max() <= 1e-12, np.abs(res - want).max()


@pytest.mark.parametrize("fourth", [False, True])
def test_dropped_last_sweep_is_the_full_chain_to_the_bit(fourth):
    """x + d of a chain run one sweep short is what the full chain's last sweep stores, in float32 to the bit"""
    A, M, lo, hi = spd_rows(90, 5)
    rng = np.random.default_rng(1)
    b = rng.standard_normal(90).astype(F32)
    for its in (1, 2, 9):
        short = ba.run_chain(A, ba.over(np.diag(M)), ba.Schedule(1.1 * hi, 30.0, fourth), b, its, F32, coef=F32)
        full = ba.Chain(A, ba.over(np.diag(M)), ba.Schedule(1.1 * hi, 30.0, fourth), b, F32, coef=F32)
        full.sweeps(its)                               # every sweep launched: the last one's x += d
        assert short.dtype == F32 and np.array_equal(short.view(np.uint32), full.x.view(np.uint32)), its
    assert not np.any(ba.run_chain(A, ba.over(np.diag(M)), ba.Schedule(1.1 * hi, 30.0), b, 0, F32))      # no sweep: x = 0
    # the deliberate error of the GPU test is visible: one sweep short and the last direction not added
    assert not np.array_equal(ba.run_chain(A, ba.over(np.diag(M)), ba.Schedule(1.1 * hi, 30.0), b, 9, F32, short=True), short)


@pytest.mark.parametrize("post", [0, 1, 6])
@pytest.mark.parametrize("fourth", [False, True])
def test_restarted_tail_is_a_fresh_chain_on_the_corrected_residual(post, fourth):
    """pre sweeps, a correction e as the next direction, the restarted tail: equal to 'x += e, r = b - A x, a fresh chain of post
    sweeps from r' to rounding"""
    n, pre = 80, 4
    A, M, lo, hi = spd_rows(n, 9)
    rng = np.random.default_rng(2)
    b = rng.standard_normal(n)
    B = ba.over(np.diag(M))
    lmax, alpha = 1.1 * hi, 8.0
    W = rng.standard_normal((n, 7))
    coarse = lambda r: (W @ np.linalg.solve(W.T @ M @ W, W.T @ r.astype(F64))).astype(r.dtype)      # noqa: E731
    got, r_pre = ba.two_level(A, B, ba.Schedule(lmax, alpha, fourth), b, pre, post, coarse, F64)
    ch = ba.Chain(A, B, ba.Schedule(lmax, alpha, fourth), b, F64)
    ch.sweeps(pre)
    assert np.array_equal(ch.r, r_pre)
    x1 = ch.x + coarse(ch.r)
    want = x1 + ba.run_chain(A, B, ba.Schedule(lmax, alpha, fourth), b - M @ x1, post, F64)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    # a tail that goes on with the old recurrence is another vector
    cont, _ = ba.two_level(A, B, ba.Schedule(lmax, alpha, fourth), b, pre, post, coarse, F64, restarts=False)
    assert post == 0 or np.abs(cont - want).max() > 1e-6 * np.abs(want).max()


def test_rows_sum_in_both_orders_and_every_type():
    rng = np.random.default_rng(4)
    N2 = 37
    g = ks.mono_graph(N2, 9, rng)
    db = rng.standard_normal(3 * len(g[1]))
    A = ba.rows_of_db(N2, g[0], g[1], db)
    x = rng.standard_normal(3 * N2)
    want = A.dense() @ x
    for dt, tol in ((F32, 1e-5), (F64, 1e-14), (LD, 1e-14)):
        for rev in (False, True):
            y = A(x.astype(dt), rev)
            assert y.dtype == dt and np.abs(y.astype(F64) - want).max() <= tol * np.abs(want).max()
    assert not np.array_equal(A(x.astype(F32)), A(x.astype(F32), True))      # the order is really another one
    # identity rows and the 3x3 block form against their dense matrices
    flag = rng.random(3 * N2) < 0.2
    S = ba.rows_of_scalar(N2, g[0], g[1], rng.standard_normal(len(g[1])), flag)
    assert np.allclose(S(x), S.dense() @ x) and np.array_equal(S(x)[flag], x[flag])
    v9 = rng.standard_normal(9 * len(g[1]))
    Bk = ba.rows_of_blocks(N2, g[0], g[1], v9)
    ref = np.zeros(3 * N2)
    for i in range(N2):
        for b in range(g[0][i], g[0][i + 1]):
            ref[3 * i:3 * i + 3] += v9[9 * b:9 * b + 9].reshape(3, 3) @ x[3 * g[1][b]:3 * g[1][b] + 3]
    assert np.allclose(Bk(x), ref)


@pytest.mark.parametrize("two_chains", [False, True])
def test_composition_inverts_the_block_system(two_chains):
    """About 200 nodes, a diagonal Avv, exact inner solves, and a coupling for which the factorisation is exact: the composed
    stages invert the assembled matrix to FP64 rounding in the longdouble run.  Then one block at a time runs its real chain
    with many sweeps, and the answer is the same."""
    D, M = ba.synthetic_data(two_chains=two_chains)
    rng = np.random.default_rng(7)
    r = rng.standard_normal(M.shape[0]) * np.where(np.arange(M.shape[0]) % 6 < 3, 1e2, 1.0)
    want = np.linalg.solve(M, r)
    z = ba.application(D, r, LD)["z"].astype(F64)
    cond = np.linalg.cond(M)
    assert np.abs(z - want).max() <= 64 * np.finfo(F64).eps * cond * np.abs(want).max(), np.abs(z - want).max()
    assert np.linalg.norm(M @ z - r) <= 1e-11 * np.linalg.norm(r)
    for block in ("solid", "fluid", "schur", "disp"):
        Dc, _ = ba.synthetic_data(two_chains=two_chains, exact=tuple(b for b in ("solid", "fluid", "schur", "disp") if b != block))
        zc = ba.application(Dc, r, LD)["z"].astype(F64)
        assert np.linalg.norm(zc - want) <= 1e-9 * np.linalg.norm(want), (block, np.linalg.norm(zc - want) / np.linalg.norm(want))
    # the two forms differ where they should: Gauss-Seidel against Jacobi coupling needs fluid rows with solid columns, which a
    # diagonal Avv has none of; the displacement block's velocity is the one thing that differs
    o = ba.application(D, r, LD)
    v = o["xs"] if two_chains else o["dv"]
    assert np.array_equal(o["td"], o["rd0"] - D["adv"]["A"](v.astype(LD)))
    # user order and back
    ru = rng.standard_normal(M.shape[0])
    rs = ba.to_solver(D, ru)
    assert np.array_equal(rs[D["user2solver"]], D["rowscale"][D["user2solver"]] * ru) and np.array_equal(ba.to_user(D, rs), rs[D["user2solver"]])


@pytest.mark.parametrize("N2,V", [(6, 2), (549, 121)])
def test_map_of_blk_is_the_constructor_s(N2, V):
    """the offsets of blk_map against the numbers in BlockApply's constructor and F32Work (vasp_amd/csrc/fsi_precond.hip), for an
    even and an odd N2 (an odd one leaves IW off a 16-byte boundary)"""
    src = (Path(ba.__file__).resolve().parents[1] / "vasp_amd" / "csrc" / "fsi_precond.hip").read_text()
    ctor = src[src.index("explicit BlockApply("):src.index("// the stages, in the order")]
    n3 = 3 * N2
    want = {"rd": 0}
    for name, k in re.findall(r"(\w+) = W \+ (?:(\d+) \* )?n3", ctor):
        want[name] = int(k or 1) * n3
    assert re.search(r"\brd = W;", ctor)
    for name, k in re.findall(r"(\w+) = IW \+ (\d+) \* n3", ctor):
        want[name] = want["IW"] + int(k) * n3
    m = ba.blk_map(N2, V)
    assert set(want) == {"rd", "rv", "rp", "vs", "tp", "dp", "dv", "td", "dd", "IW", "w3", "xs", "xf"}
    for name, off in want.items():
        assert m[name][0] == off, name
    assert m["xs"][0] == m["IW"][0] + 4 * n3 and m["xf"][0] == m["IW"][0] + 5 * n3
    assert m["schur"] == (m["rp"][0] + V, 3 * V) and m["schur"][0] + 3 * V <= m["vs"][0] or 4 * V > n3
    assert m["w3"][0] + n3 <= 20 * n3 + 16                               # the allocation of fsi_setup.hip
    assert "r = F; d = F + n; t = F + 2 * n; x = F + 3 * n; rhs = F + 4 * n;" in src and "+ 15) & ~uintptr_t(15)" in src
    fw = ba.f32_work(m["IW"][0], 4 * N2)
    start = fw["r"][0]
    assert (4 * start) % 16 == 0 and 0 <= 4 * start - 8 * m["IW"][0] < 16
    assert ba.disp_f32_result(N2, V) == (start + 12 * N2, 4 * N2)
    assert fw["rhs"][0] + 4 * N2 <= 2 * m["xs"][0]                       # the FP32 sweeps' five vectors end below xs
    fb = ba.f32_work(m["IW"][0] + 6 * n3, 4 * N2)                        # the fluid sweeps of the two-chain form: IW[6 n3, 10 n3)
    assert fb["r"][0] >= 2 * (m["xf"][0] + n3) and fb["rhs"][0] + 4 * N2 <= 2 * (m["IW"][0] + 10 * n3)
    blk = np.arange(20 * n3 + 16, dtype=F64)
    assert np.array_equal(ba.blk_vector(blk, N2, V, "tp"), np.arange(4 * n3, 4 * n3 + V))
