"""The boundary terms of every Newton step and the small vector launchers of the default path, one launch function at a time on an
MI355X through libfsi_kernel_shim.so: launch_robin_residual, launch_add_at, launch_add_indexed, launch_bc_rhs, launch_bc_set;
launch_fill, copy, axpy, axpby, scale, mul, div, negate, gather, scatter, gather3, scatter3, round_to_f32; launch_f32_ripple4 and
launch_f32_sumsq (the helpers that make the coarse levels' power iteration reproducible).

Sizes: n in {0, 1, 255, 256, 257, 4096 * 256 + 257}; the last is past the cap of 4096 workgroups of grid_for / gridn, so the
grid-stride loop runs a second pass.  Launchers that move values are held to the reference bit for bit; the arithmetic ones to
one rounding of the reference in extended precision whether or not the compiler contracts a multiply-add (for y + a x:
eps (|y| + |a x|)).  Every output starts as a sentinel: entries outside the index set or past the end must keep it.  n = 0 must
return without a HIP error (an empty grid is an invalid launch) and write nothing."""
import numpy as np
import pytest

import kernel_shim as ks

pytestmark = pytest.mark.gpu

CAP = 4096 * 256                       # threads of the largest grid grid_for (fsi_solver.hip) and gridn (fsi_block.hip) launch
SIZES = [0, 1, 255, 256, 257, CAP + 257]
SENT = -7.0e77
EPS = ks.EPS64
LD = np.longdouble


def vec(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    if got.tobytes() != ref.tobytes():
        u = np.uint64 if got.dtype.itemsize == 8 else np.uint32
        bad = np.flatnonzero(got.view(u) != ref.view(u))
        raise AssertionError(f"{what}: {len(bad)} entries differ in their bits, first at {bad[0]}: {got[bad[0]]!r} for {ref[bad[0]]!r}")


def within(got, ref, bound, what):
    """|got - ref| <= bound entry by entry in extended precision (ref and bound are np.longdouble); prints the largest ratio"""
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD))
    r = ks.worst_ratio(err, bound)
    print(f"{what}: largest error / bound {r:.3f}")
    if not r <= 1.0:
        i = int(np.flatnonzero(~(err <= np.asarray(bound, dtype=LD)))[0])
        raise AssertionError(f"{what}: entry {i}: got {np.asarray(got)[i]!r}, reference {np.asarray(ref)[i]!r}, error {float(err[i]):.3e} > "
                             f"bound {float(np.asarray(bound)[i]):.3e}")


def subset(n, nt, seed):
    """n distinct targets among nt > n, in random order"""
    return np.random.default_rng(seed).permutation(nt)[:n].astype(np.int32)


# ---- bitwise launchers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_fill_copy_negate(n):
    x = ks.out(n, np.float64, SENT)
    ks.call("shim_fill", n, 0.1, x)
    same_bits(x[:n], np.full(n, 0.1), "fill")
    s = vec(n, 1)
    d, b = ks.out(n, np.float64, SENT), ks.out(n, np.float64, SENT)
    ks.call("shim_copy", n, s, d)
    ks.call("shim_negate", n, s, b)
    same_bits(d[:n], s, "copy")
    same_bits(b[:n], -s, "negate")
    assert all(ks.tail_untouched(a, n, SENT) for a in (x, d, b))


@pytest.mark.parametrize("n", SIZES)
def test_gather_scatter(n):
    ns = n + 37
    s = vec(ns, 2)
    idx = np.random.default_rng(3).integers(0, ns, n).astype(np.int32)          # a gather may repeat an index
    d = ks.out(n, np.float64, SENT)
    ks.call("shim_gather", n, s, ns, idx, d)
    same_bits(d[:n], s[idx], "gather")
    assert ks.tail_untouched(d, n, SENT)
    tgt = subset(n, ns, 4)                                                        # distinct targets, a strict subset
    src, full = vec(n, 5), np.full(ns, SENT)
    ks.call("shim_scatter", n, src, tgt, full, ns)
    ref = np.full(ns, SENT)
    ref[tgt] = src
    same_bits(full, ref, "scatter")


@pytest.mark.parametrize("nS", [0, 1, 85, 86, CAP // 3 + 90])                    # 3 nS around 256 and past the cap
def test_gather3_scatter3(nS):
    nnodes = nS + 11
    snode = subset(nS, nnodes, 6)
    full = vec(3 * nnodes, 7)
    comp = ks.out(3 * nS, np.float64, SENT)
    ks.call("shim_gather3", nS, nnodes, snode, full, comp)
    ref = full.reshape(-1, 3)[snode].reshape(-1)
    same_bits(comp[:3 * nS], ref, "gather3")
    assert ks.tail_untouched(comp, 3 * nS, SENT)
    back = np.full(3 * nnodes, SENT)
    src = vec(3 * nS, 8)
    ks.call("shim_scatter3", nS, nnodes, snode, src, back)
    refb = np.full((nnodes, 3), SENT)
    refb[snode] = src.reshape(-1, 3)
    same_bits(back, refb.reshape(-1), "scatter3")


@pytest.mark.parametrize("n", SIZES)
def test_bc_set(n):
    nu = n + 19
    bc, g = subset(n, nu, 9), vec(n, 10)
    U = np.full(nu, SENT)
    ks.call("shim_bc_set", n, bc, g, U, nu)
    ref = np.full(nu, SENT)
    ref[bc] = g
    same_bits(U, ref, "bc_set")


@pytest.mark.parametrize("n", SIZES)
def test_round_to_f32(n):
    a = vec(n, 11) * 10.0 ** np.random.default_rng(12).integers(-30, 30, n)
    if n > 8:
        a[:8] = [0.0, -0.0, 1 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, 1e-46, 3.5e38, -1e39, 1.401298464324817e-45]   # ties, under- / overflow
    b = ks.out(n, np.float32, np.float32(-7.25))
    ks.call("shim_round_to_f32", n, a, b)
    with np.errstate(over="ignore", under="ignore"):
        ref = a.astype(np.float32)                                                # round to nearest even, as the device's conversion
    same_bits(b[:n], ref, "round_to_f32")
    assert ks.tail_untouched(b, n, np.float32(-7.25))


# ---- one rounding of the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_axpy_axpby_scale_mul_div(n):
    x, y0, a, b = vec(n, 13), vec(n, 14), 0.7310585786300049, -1.3
    xl, yl = x.astype(LD), y0.astype(LD)
    y = ks.out(n, np.float64, SENT)
    y[:n] = y0
    ks.call("shim_axpy", n, a, x, y)
    within(y[:n], yl + LD(a) * xl, EPS * (np.abs(yl) + np.abs(LD(a) * xl)), "axpy")
    z = ks.out(n, np.float64, SENT)
    ks.call("shim_axpby", n, a, x, b, y0, z)
    within(z[:n], LD(a) * xl + LD(b) * yl, EPS * (np.abs(LD(a) * xl) + np.abs(LD(b) * yl)), "axpby")
    sc = ks.out(n, np.float64, SENT)
    sc[:n] = y0
    ks.call("shim_scale", n, a, sc)
    within(sc[:n], LD(a) * yl, EPS * np.abs(LD(a) * yl), "scale")
    mu, dv = ks.out(n, np.float64, SENT), ks.out(n, np.float64, SENT)
    ks.call("shim_mul", n, x, y0, mu)
    within(mu[:n], xl * yl, EPS * np.abs(xl * yl), "mul")
    den = np.where(np.abs(y0) < 1e-3, 1.0, y0)
    ks.call("shim_div", n, x, den, dv)
    within(dv[:n], xl / den.astype(LD), EPS * np.abs(xl / den.astype(LD)), "div")
    assert all(ks.tail_untouched(o, n, SENT) for o in (y, z, sc, mu, dv))


@pytest.mark.parametrize("n", SIZES)
def test_add_indexed_add_at_bc_rhs(n):
    nt = n + 23
    base = vec(nt, 15)
    # interface pressure load: y[idx] += a coef
    idx, coef, a = subset(n, nt, 16), vec(n, 17), -133.322
    y = base.copy()
    ks.call("shim_add_indexed", n, idx, coef, a, y, nt)
    ref = base.astype(LD)
    ref[idx] += LD(a) * coef.astype(LD)
    bound = np.zeros(nt, dtype=LD)
    bound[idx] = EPS * (np.abs(base[idx].astype(LD)) + np.abs(LD(a) * coef.astype(LD)))
    within(y, ref, bound, "add_indexed")
    out_of_set = np.setdiff1d(np.arange(nt), idx)
    same_bits(y[out_of_set], base[out_of_set], "add_indexed outside the index set")
    # Robin rows of A_pre: vals[pos] += th0 v
    pos, v, th0 = subset(n, nt, 18).astype(np.int64), vec(n, 19) * 1e7, 0.51
    vals = base.copy()
    ks.call("shim_add_at", n, pos, v, th0, vals, nt)
    ref = base.astype(LD)
    ref[pos] += LD(th0) * v.astype(LD)
    bound = np.zeros(nt, dtype=LD)
    bound[pos] = EPS * (np.abs(base[pos].astype(LD)) + np.abs(LD(th0) * v.astype(LD)))
    within(vals, ref, bound, "add_at")
    same_bits(np.delete(vals, pos), np.delete(base, pos), "add_at outside the positions")
    # Dirichlet rows of the right-hand side: b[bc] = g - U[bc]
    bc, g, U = subset(n, nt, 20), vec(n, 21), vec(nt, 22)
    b = base.copy()
    ks.call("shim_bc_rhs", n, bc, g, U, b, nt)
    ref = base.astype(LD)
    ref[bc] = g.astype(LD) - U[bc].astype(LD)
    bound = np.zeros(nt, dtype=LD)
    bound[bc] = EPS * (np.abs(g.astype(LD)) + np.abs(U[bc].astype(LD)))
    within(b, ref, bound, "bc_rhs")
    same_bits(np.delete(b, bc), np.delete(base, bc), "bc_rhs outside the Dirichlet rows")


def test_add_at_single_position_is_the_diagonal_shift():
    """launch_add_at's second use (fsi_newton.hip): n = 1, one diagonal entry shifted"""
    vals = vec(50, 23)
    base = vals.copy()
    pos, v = np.array([31], dtype=np.int64), np.array([2.5e-3])
    ks.call("shim_add_at", 1, pos, v, 1.0, vals, 50)
    assert vals[31] == base[31] + 2.5e-3                                         # a = 1: one exactly rounded addition
    same_bits(np.delete(vals, 31), np.delete(base, 31), "the other entries")


@pytest.mark.parametrize("nrows", [0, 1, 257, CAP + 257])
def test_robin_residual(nrows):
    """F[urow[k]] += sum_i val_i (th0 U[col_i] + th1 U1[col_i]) over 1 .. 12 entries per row (and some rows of none), one thread per
    distinct row.  Bound per row with L entries: (L + 3) eps (|F_before| + sum |val| (|th0 U| + |th1 U1|)): two roundings and a
    multiplication per term, L additions of the row's sum and the one into F, in any order and with or without FMAs."""
    rng = np.random.default_rng(24)
    nu = nrows + 41
    th0, th1 = 0.51, 0.49
    urow = subset(nrows, nu, 25)
    L = rng.integers(1, 13, nrows)
    if nrows > 8:
        L[[2, nrows - 1]] = 0                                                    # rows of length 0 leave F unchanged
        L[[0, 5]] = [12, 1]
    ptr = np.concatenate([[0], np.cumsum(L)]).astype(np.int32)
    ne = int(ptr[-1])
    col, val = rng.integers(0, nu, ne).astype(np.int32), rng.standard_normal(ne) * 1e3
    U, U1, F0 = vec(nu, 26), vec(nu, 27), vec(nu, 28)
    F = F0.copy()
    ks.call("shim_robin_residual", nrows, urow, ptr, col, val, th0, th1, U, U1, F, nu)
    t0, t1 = LD(th0) * U[col].astype(LD), LD(th1) * U1[col].astype(LD)
    s = ks._row_sums(ptr.astype(np.int64), val.astype(LD) * (t0 + t1))
    S = ks._row_sums(ptr.astype(np.int64), np.abs(val.astype(LD)) * (np.abs(t0) + np.abs(t1)))
    ref = F0.astype(LD)
    ref[urow] += s
    bound = np.zeros(nu, dtype=LD)
    bound[urow] = (L + 3) * EPS * (np.abs(F0[urow].astype(LD)) + S)
    within(F, ref, bound, f"robin_residual, {nrows} rows")
    untouched = np.setdiff1d(np.arange(nu), urow[L > 0])
    same_bits(F[untouched], F0[untouched], "rows outside urow and rows of length 0")


# ---- the helpers of the coarse levels' power iteration -----------------------------------------------------------------------------
@pytest.mark.parametrize("nnodes", [0, 1, 255, 100_003, CAP + 257])                # gridn's cap is 4096 workgroups of 256
def test_f32_ripple4(nnodes):
    x = ks.out(4 * nnodes, np.float32, np.float32(-7.25))
    ks.call("shim_f32_ripple4", nnodes, x)
    same_bits(x[:4 * nnodes], ks.f32_ripple4(nnodes), "f32_ripple4")
    assert np.all(x[3:4 * nnodes:4] == 0.0)                                      # every fourth lane exactly zero
    assert ks.tail_untouched(x, 4 * nnodes, np.float32(-7.25))


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 400_001])
def test_f32_sumsq(n):
    """One workgroup of 1024 threads, each summing n / 1024 squares (exact products of FP32 values in FP64), then a tree of ten
    levels: (n / 1024 + 12) eps sum x^2.  Same bits on every call."""
    x = np.random.default_rng(29).standard_normal(n).astype(np.float32)
    a, b = ks.out(1, np.float64, SENT), ks.out(1, np.float64, SENT)
    ks.call("shim_f32_sumsq", n, x, a)
    ks.call("shim_f32_sumsq", n, x, b)
    ref = np.sum(x.astype(LD) ** 2)
    within(a[:1], np.array([ref]), np.array([(n / 1024 + 12) * EPS * ref]), f"f32_sumsq, n = {n}")
    assert a[0].tobytes() == b[0].tobytes()
    assert ks.tail_untouched(a, 1, SENT) and ks.tail_untouched(b, 1, SENT)


def test_empty_launches_return_clean():
    """n = 0 through every launcher of this file and through launch_spmv: no HIP error (ks.call raises on hipGetLastError) and
    nothing written.  The other launchers' n = 0 cases are in the parametrised tests above."""
    e64, e32i, e64i = np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64)
    y = np.full(3, SENT)
    ks.call("shim_spmv", 0, np.zeros(1, dtype=np.int64), e32i, e64, y[:0].copy(), 0, y, 0)
    same_bits(y, np.full(3, SENT), "spmv of no rows")
    F = np.full(5, SENT)
    ks.call("shim_robin_residual", 0, e32i, np.zeros(1, dtype=np.int32), e32i, e64, 0.51, 0.49, F.copy(), F.copy(), F, 5)
    ks.call("shim_add_at", 0, e64i, e64, 0.5, F, 5)
    ks.call("shim_add_indexed", 0, e32i, e64, 0.5, F, 5)
    ks.call("shim_bc_rhs", 0, e32i, e64, F.copy(), F, 5)
    ks.call("shim_bc_set", 0, e32i, e64, F, 5)
    same_bits(F, np.full(5, SENT), "boundary terms of no rows")
