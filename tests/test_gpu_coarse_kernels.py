"""The two-level (P2 -> P1) coarse levels and the diagonal scalings of the block preconditioner (vasp_amd/csrc/fsi_block.hip), one
launch at a time through the test shim, against the numpy contracts of tests/kernel_shim.py, and on live contexts against the
hierarchy and Galerkin products restated from the mesh and the assembled Jacobian.

Bitwise, where a kernel does not accumulate: k_mg_d0, k_mg_coarse_finish (cc, cflag, dcinv4, identity rows, the row-sum bound:
an FP32 sum of fabsf terms in entry order), k_sbmg_flags, the identity rows / cflag / untouched blocks of k_sbmg_coarse_finish,
k_sb_dinv, k_dinv_f32, k_diag_inverse (correctly rounded divisions), binv12 == float(binv9), k_gather3_f32 / k_scatter3_f32
(entries outside snode untouched), the zeroed x / d2 and the gathered r of k_solid_cycle_init, bd == rc of k_sbmg_restrict.

Bounded, where it accumulates (L = the number of contributions to the entry, sum |terms| in FP64):
    k_mg_rap                  (L + 8) eps64 sum |terms|
    k_sbmg_rap                (L + 10) 2^-24 sum |terms|
    k_mg_restrict             (L + 10) 2^-24 |dcinv| sum |terms|
    k_sbmg_restrict           (L + 10) 2^-24 sum |terms|
    k_mg_prolong / k_sbmg_prolong, bmul products    2 2^-24 sum |terms|
    k_sb_binv (FP64)          16 eps64 |A^-1| |A| |A^-1|  elementwise, reference: the adjugate in extended precision
    k_sbmg_coarse_finish      16 2^-24 |A^-1| |A| |A^-1|  elementwise (FP32 cofactors)
    its row-sum bound         (3 L + 8) 2^-24 sum |B^-1| |C_e|, with the kernel's own B^-1
Against the assembled Jacobian the references gain the Jacobian's own 2 eps64 per entry: (L + 12) eps64 for the displacement
level, 16 u |A^-1||A||A^-1| for the solid blocks.

Non-symmetric fine operators and 3x3 blocks throughout, so that a transposed product or inverse fails; coarse rows of more than
64 and 128 entries (the RAP kernels' chunk loop), nc past the RAP kernels' 65 536 waves and past the restrictions' 262 144 / 131 072
lane groups; Dirichlet rows, a vertex without a free child, mixed component flags, a missing pair, singular and indefinite
diagonal blocks.  The RAP kernels report a missing pair only in rows of <= 64 entries (see k_mg_rap); that is all this asserts."""
import numpy as np
import pytest
import scipy.sparse as sp

import kernel_shim as ks

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
EPS = np.finfo(np.float64).eps
check = ks.check


# ---- synthetic levels --------------------------------------------------------------------------------------------------------
def level(nc, nmid, seed, heavy=(), deg=6):
    """A random hierarchy: nc vertices and nmid edge midpoints (two distinct parents, weights 1/2) at random fine positions, a
    fine graph (diagonal + up to deg neighbours within a window, vectorised), the full coarse pattern (ascending, with the
    diagonal).  Vertex v gets heavy[v] extra midpoints, each joined to a different vertex: its coarse row grows past 64 / 128."""
    rng = np.random.default_rng(seed)
    nm = nmid + sum(heavy)
    N2 = nc + nm
    perm = rng.permutation(N2)
    vpos = np.sort(perm[:nc])                  # fine index of coarse node i (cfine), ascending as in the library
    mpos = perm[nc:]
    par = np.zeros((N2, 2), dtype=np.int32)
    pw = np.zeros((N2, 2), dtype=np.float32)
    par[vpos, 0] = par[vpos, 1] = np.arange(nc)
    pw[vpos, 0] = 1.0
    a = rng.integers(0, nc, nm)
    b = (a + 1 + rng.integers(0, min(nc - 1, 40), nm)) % nc
    k = nmid
    for v, h in enumerate(heavy):
        a[k:k + h] = v
        b[k:k + h] = (v + 1 + rng.permutation(nc - 1)[:h]) % nc
        k += h
    par[mpos, 0], par[mpos, 1] = a, b
    pw[mpos] = 0.5
    nadj_ptr, nadj = ks.mono_graph(N2, 0, rng, reach=30, max_deg=deg)[:2]
    chptr, child, chw = ks.children(par, pw, nc)
    G = sp.csr_matrix((np.ones(len(nadj)), nadj, nadj_ptr), shape=(N2, N2))
    P = ks.prolongation(par, pw, nc)
    Pat = (abs(P).T @ G @ abs(P) + sp.eye(nc)).tocsr()
    Pat.sort_indices()
    return dict(N2=N2, nc=nc, par=par.ravel(), pw=pw.ravel(), nadj_ptr=nadj_ptr, nadj=nadj, chptr=chptr, child=child, chw=chw,
                cptr=Pat.indptr.astype(np.int64), ccol=Pat.indices.astype(np.int32), cfine=vpos.astype(np.int32), P=P, rng=rng)


def vec4(rng, n):
    v = np.zeros((n, 4), dtype=np.float32)
    v[:, :3] = rng.standard_normal((n, 3)).astype(np.float32)
    return v.ravel()


def run_mg_rap(L, db, rowscale, rowflag, cptr=None, ccol=None):
    cptr = L["cptr"] if cptr is None else cptr
    ccol = L["ccol"] if ccol is None else ccol
    Ac = np.full(int(cptr[-1]), np.nan)
    flags = np.array([5, 1, 9, 0], dtype=np.int32)        # pre-filled: the kernel may only OR bit 64 into flags[1]
    ks.call("shim_mg_rap", L["nc"], L["N2"], L["chptr"], L["child"], L["chw"], L["nadj_ptr"], L["nadj"], db, rowscale, rowflag,
            L["par"], L["pw"], cptr, ccol, Ac, flags)
    return Ac, flags


@pytest.mark.parametrize("nc,nmid,heavy", [(300, 500, (150, 12)), (70001, 90000, ())])
def test_displacement_level(nc, nmid, heavy):
    L = level(nc, nmid, seed=nc, heavy=heavy)
    rng, N2 = L["rng"], L["N2"]
    nnz = len(L["nadj"])
    lens = np.diff(L["cptr"])
    if heavy:
        assert lens.max() > 128 and ((lens > 64) & (lens <= 128)).any(), "the chunk loop of k_mg_rap is not reached"
    db = rng.standard_normal(3 * nnz)
    row = np.repeat(np.arange(N2), np.diff(L["nadj_ptr"]))
    db[3 * np.flatnonzero(L["nadj"] == row)] = rng.uniform(5.0, 9.0, N2)       # positive diagonals
    rowscale = rng.uniform(0.5, 2.0, 6 * N2)
    rowflag = np.zeros(3 * N2, dtype=np.uint8)
    dir_rows = rng.choice(N2, N2 // 20, replace=False)
    rowflag[3 * dir_rows[:, None] + np.arange(3)] = 1
    # a vertex without a free child: the vertex and every midpoint it parents are Dirichlet rows
    lonely = 3
    kids = L["child"][L["chptr"][lonely]:L["chptr"][lonely + 1]]
    rowflag[3 * kids.astype(np.int64)[:, None] + np.arange(3)] = 1

    # k_mg_d0
    d0 = np.full(N2, np.nan, dtype=np.float32)
    flags = np.array([3, 2, 0, 0], dtype=np.int32)
    ks.call("shim_mg_d0", N2, L["nadj_ptr"], L["nadj"], db, rowscale, rowflag, d0, flags)
    d0_ref, mixed = ks.mg_d0(N2, L["nadj_ptr"], L["nadj"], db, rowscale, rowflag)
    np.testing.assert_array_equal(d0, d0_ref)
    assert not mixed and list(flags) == [3, 2, 0, 0]
    rf2 = rowflag.copy()
    rf2[3 * 7 + 1] ^= 1                                                           # node 7: one component Dirichlet
    flags = np.array([3, 2, 0, 0], dtype=np.int32)
    ks.call("shim_mg_d0", N2, L["nadj_ptr"], L["nadj"], db, rowscale, rf2, d0, flags)
    assert list(flags) == [3, 2 | 32, 0, 0]

    # k_mg_rap: bounded against the contract, the same bits twice, no missing pair on the full pattern
    Ac, flags = run_mg_rap(L, db, rowscale, rowflag)
    ref, S, Lc, missed = ks.mg_rap(nc, L["chptr"], L["child"], L["chw"], L["nadj_ptr"], L["nadj"], db, rowscale, rowflag,
                                   L["par"], L["pw"], L["cptr"], L["ccol"])
    assert not missed and list(flags) == [5, 1, 9, 0]
    check(Ac, ref, (Lc + 8) * EPS * S, "mg_rap against the contract")
    assert (Ac[np.repeat(np.arange(nc), lens) == lonely] == 0).all()
    # and against P^T A0 P of the matrix itself (non-symmetric: a transposed product misses)
    A0 = sp.csr_matrix((db[0::3] * (1.0 / rowscale[6 * row]), L["nadj"], L["nadj_ptr"]), shape=(N2, N2))
    G = ks.galerkin(L["P"], A0, rowflag[0::3] == 0)
    crow = np.repeat(np.arange(nc), lens)
    check(Ac, np.asarray(G[crow, L["ccol"]]).ravel(), 2 * (Lc + 8) * EPS * S, "mg_rap against P^T A0 P")
    assert abs(G - G.T).max() > 1e-3 * abs(G).max()
    Ac2, _ = run_mg_rap(L, db, rowscale, rowflag)
    np.testing.assert_array_equal(Ac2, Ac)
    # a missing pair in a row of <= 64 entries sets bit 64
    short = np.flatnonzero((lens <= 64) & (lens > 1) & (np.arange(nc) != lonely))
    i = int(short[np.argmax(lens[short])])
    e = int(L["cptr"][i] + np.flatnonzero((L["ccol"][L["cptr"][i]:L["cptr"][i + 1]] != i) &
                                          (S[L["cptr"][i]:L["cptr"][i + 1]] > 0))[0])
    cptr2 = L["cptr"].copy()
    cptr2[i + 1:] -= 1
    _, flags = run_mg_rap(L, db, rowscale, rowflag, cptr2, np.delete(L["ccol"], e))
    assert flags[1] == 1 | 64

    # k_mg_coarse_finish on the kernel's own Ac, with a diagonal <= 0, a row without a diagonal and the lonely vertex
    Acf = Ac.copy()
    dg = {k: int(np.flatnonzero((crow == k) & (L["ccol"] == k))[0]) for k in (10, 11, 12)}
    Acf[dg[10]] = -abs(Acf[dg[10]])
    Acf[dg[11]] = 0.0
    ccolf = L["ccol"].copy()
    absent = np.setdiff1d(np.arange(nc), ccolf[L["cptr"][12]:L["cptr"][13]])[0]
    ccolf[dg[12]] = absent                                                      # row 12 loses its diagonal
    cc = np.full(len(Acf), np.nan, dtype=np.float32)
    cflag = np.full(3 * nc, 7, dtype=np.uint8)
    dcinv4 = np.full(4 * nc, np.nan, dtype=np.float32)
    rowmax = np.array([np.float32(0.5).view(np.int32)], dtype=np.int32)
    ks.call("shim_mg_coarse_finish", nc, N2, L["cptr"], ccolf, Acf, L["cfine"], rowflag, cc, cflag, dcinv4, rowmax)
    cc_r, cflag_r, dcinv_r, rowmax_r = ks.mg_coarse_finish(nc, L["cptr"], ccolf, Acf, L["cfine"], rowflag)
    np.testing.assert_array_equal(cc, cc_r)
    np.testing.assert_array_equal(cflag, cflag_r)
    np.testing.assert_array_equal(dcinv4, dcinv_r)
    assert rowmax.view(np.float32)[0] == rowmax_r
    assert cflag_r[3 * np.array([10, 11, 12, lonely])].all()

    # k_mg_restrict (4 lanes per vertex) with and without the coarse Chebyshev start
    r4 = vec4(rng, N2)
    rc4 = np.full(4 * nc, np.nan, dtype=np.float32)
    ks.call("shim_mg_restrict", nc, N2, L["chptr"], L["child"], L["chw"], d0_ref, r4, dcinv_r, rc4, 0.0, None, None, None)
    val, bnd = ks.mg_restrict(nc, L["chptr"], L["child"], L["chw"], d0_ref, r4, dcinv_r)
    rc = rc4.reshape(-1, 4)
    check(rc[:, :3], val, bnd, "mg_restrict")
    assert (rc[:, 3] == 0).all() and (rc[cflag_r[0::3] == 1, :3] == 0).all()
    cx, cr, cd = (np.full(4 * nc, np.nan, dtype=np.float32) for _ in range(3))
    rc4b = np.full(4 * nc, np.nan, dtype=np.float32)
    inv_theta = np.float32(0.37)
    ks.call("shim_mg_restrict", nc, N2, L["chptr"], L["child"], L["chw"], d0_ref, r4, dcinv_r, rc4b, float(inv_theta), cx, cr, cd)
    np.testing.assert_array_equal(rc4b, rc4)
    np.testing.assert_array_equal(cx, 0)
    np.testing.assert_array_equal(cr, rc4)
    np.testing.assert_array_equal(cd, (rc4 * inv_theta).astype(np.float32))

    # k_mg_prolong
    xc4 = vec4(rng, nc)
    e4 = np.full(4 * N2, np.nan, dtype=np.float32)
    ks.call("shim_mg_prolong", N2, nc, L["par"], L["pw"], d0_ref, xc4, e4)
    val, bnd = ks.mg_prolong(L["par"], L["pw"], d0_ref != 0, xc4)
    e = e4.reshape(-1, 4)
    check(e[:, :3], val, bnd, "mg_prolong")
    assert (e[:, 3] == 0).all() and (e[d0_ref == 0] == 0).all()


@pytest.mark.parametrize("kind", ["mg", "sbmg"])
def test_restriction_strides_past_the_grid_cap(kind):
    """nc = 270 001: the 4- and 8-lane groups of the restrictions stride past gridn's 4096 workgroups"""
    nc, nmid = 270001, 300000
    rng = np.random.default_rng(9)
    N2 = nc + nmid
    par = np.zeros((N2, 2), dtype=np.int32)
    pw = np.zeros((N2, 2), dtype=np.float32)
    par[:nc, 0] = par[:nc, 1] = np.arange(nc)
    pw[:nc, 0] = 1.0
    a = rng.integers(0, nc, nmid)
    par[nc:, 0], par[nc:, 1] = a, (a + 1 + rng.integers(0, 50, nmid)) % nc
    pw[nc:] = 0.5
    chptr, child, chw = ks.children(par, pw, nc)
    r4 = vec4(rng, N2)
    rc4 = np.full(4 * nc, np.nan, dtype=np.float32)
    if kind == "mg":
        d0 = rng.uniform(0.5, 2.0, N2).astype(np.float32)
        d0[::17] = 0
        dcinv4 = vec4(rng, nc)
        ks.call("shim_mg_restrict", nc, N2, chptr, child, chw, d0, r4, dcinv4, rc4, 0.0, None, None, None)
        val, bnd = ks.mg_restrict(nc, chptr, child, chw, d0, r4, dcinv4)
    else:
        snode = np.arange(N2, dtype=np.int32)
        rowscale = rng.uniform(0.5, 2.0, 6 * N2)
        flag = (rng.random(N2) < 0.05).astype(np.uint8)
        cflag = (rng.random(nc) < 0.05).astype(np.uint8)
        ks.call("shim_sbmg_restrict", nc, N2, N2, chptr, child, chw, snode, rowscale, flag, cflag, r4, rc4, None, None, 0)
        val, bnd = ks.sbmg_restrict(nc, chptr, child, chw, snode, rowscale, flag, cflag, r4)
    rc = rc4.reshape(-1, 4)
    check(rc[:, :3], val, bnd, f"{kind}_restrict at nc = {nc}")
    assert (rc[:, 3] == 0).all()


def block_level(L, seed):
    """3x3 values on a level's fine graph (non-symmetric blocks, dominant diagonal blocks), snode into a longer node list"""
    rng = np.random.default_rng(seed)
    nS = L["N2"]
    nb = len(L["nadj"])
    vals = (0.3 * rng.standard_normal((nb, 3, 3))).astype(np.float32)
    row = np.repeat(np.arange(nS), np.diff(L["nadj_ptr"]))
    dg = np.flatnonzero(L["nadj"] == row)
    vals[dg] += (np.diag([6.0, 7.0, 8.0]) + rng.standard_normal((len(dg), 3, 3))).astype(np.float32)
    N2 = nS + 11
    snode = np.sort(rng.choice(N2, nS, replace=False)).astype(np.int32)
    rowscale = rng.uniform(0.5, 2.0, 6 * N2)
    return vals.ravel(), snode, rowscale, N2, rng


@pytest.mark.parametrize("nc,nmid,heavy", [(300, 500, (150, 12)), (70001, 90000, ())])
def test_solid_level(nc, nmid, heavy):
    L = level(nc, nmid, seed=nc + 1, heavy=heavy, deg=5)
    nS = L["N2"]
    vals, snode, rowscale, N2, rng = block_level(L, nc)
    sb_ptr, sb_col = L["nadj_ptr"], L["nadj"]
    # k_sbmg_flags: flagged = a row of the node holds its diagonal alone
    v = vals.reshape(-1, 3, 3)
    for i, c in ((5, 0), (6, 2), (nS - 1, 1)):
        v[sb_ptr[i]:sb_ptr[i + 1], c, :] = 0
        d = sb_ptr[i] + int(np.flatnonzero(sb_col[sb_ptr[i]:sb_ptr[i + 1]] == i)[0])
        v[d, c, c] = 3.0
    lonely = 4                                          # a vertex without a free child: flag every child
    kids = L["child"][L["chptr"][lonely]:L["chptr"][lonely + 1]].astype(np.int64)
    for k in kids:
        v[sb_ptr[k]:sb_ptr[k + 1]] = 0
        d = sb_ptr[k] + int(np.flatnonzero(sb_col[sb_ptr[k]:sb_ptr[k + 1]] == k)[0])
        v[d] = np.eye(3)
    flag = np.full(nS, 9, dtype=np.uint8)
    ks.call("shim_sbmg_flags", nS, sb_ptr, sb_col, vals, flag)
    flag_r = ks.sbmg_flags(nS, sb_ptr, sb_col, vals)
    np.testing.assert_array_equal(flag, flag_r)
    assert flag[[5, 6, nS - 1]].all() and flag[kids].all()

    # k_sbmg_rap
    def rap(cptr, ccol):
        cv = np.full(9 * int(cptr[-1]), np.nan, dtype=np.float32)
        fl = np.array([5, 1, 9, 0], dtype=np.int32)
        ks.call("shim_sbmg_rap", nc, nS, N2, L["chptr"], L["child"], L["chw"], sb_ptr, sb_col, vals, snode, rowscale, flag,
                L["par"], L["pw"], cptr, ccol, cv, fl)
        return cv, fl
    cv, fl = rap(L["cptr"], L["ccol"])
    ref, S, Lc, missed = ks.sbmg_rap(nc, L["chptr"], L["child"], L["chw"], sb_ptr, sb_col, vals, snode, rowscale, flag,
                                     L["par"], L["pw"], L["cptr"], L["ccol"])
    assert not missed and list(fl) == [5, 1, 9, 0]
    check(cv.reshape(-1, 9), ref, (Lc[:, None] + 10) * U32 * S, "sbmg_rap against the contract")
    cv2, _ = rap(L["cptr"], L["ccol"])
    np.testing.assert_array_equal(cv2, cv)
    lens = np.diff(L["cptr"])
    short = np.flatnonzero((lens <= 64) & (lens > 1) & (np.arange(nc) != lonely))
    i = int(short[np.argmax(lens[short])])
    seg = slice(L["cptr"][i], L["cptr"][i + 1])
    e = int(L["cptr"][i] + np.flatnonzero((L["ccol"][seg] != i) & (S[seg].sum(axis=1) > 0))[0])
    cptr2 = L["cptr"].copy()
    cptr2[i + 1:] -= 1
    assert rap(cptr2, np.delete(L["ccol"], e))[1][1] == 1 | 64

    # k_sbmg_coarse_finish on the kernel's own blocks, with det = 0, det < 0, a00 <= 0 and a missing diagonal block
    cvf = cv.copy().reshape(-1, 3, 3)
    crow = np.repeat(np.arange(nc), lens)
    dgi = {k: int(np.flatnonzero((crow == k) & (L["ccol"] == k))[0]) for k in (10, 11, 12, 13)}
    cvf[dgi[10]] = [[1, 2, 0], [0, 0, 0], [0.5, 0, 1]]
    cvf[dgi[11]] = [[1, 0.2, 0], [0, 1, 0], [0.1, 0, -1]]
    cvf[dgi[12]] = [[-1, 0, 0.1], [0, -1, 0], [0, 0.3, 1]]
    ccolf = L["ccol"].copy()
    ccolf[dgi[13]] = np.setdiff1d(np.arange(nc), L["ccol"][crow == 13])[0]
    cvf = cvf.ravel()
    cvk = cvf.copy()
    cb = np.full(12 * nc, np.nan, dtype=np.float32)
    cflag = np.full(nc, 7, dtype=np.uint8)
    rowmax = np.array([np.float32(0.5).view(np.int32)], dtype=np.int32)
    ks.call("shim_sbmg_coarse_finish", nc, nS, L["cptr"], ccolf, cvk, L["cfine"], flag, cb, cflag, rowmax)
    ident, after, inv, a = ks.sbmg_coarse_finish(nc, L["cptr"], ccolf, cvf, L["cfine"], flag)
    assert ident[[10, 11, 12, 13, lonely]].all() and not ident.all()
    np.testing.assert_array_equal(cflag, ident.astype(np.uint8))
    np.testing.assert_array_equal(cvk, after)
    b = cb.reshape(-1, 3, 4)
    assert (b[:, :, 3] == 0).all()
    np.testing.assert_array_equal(b[ident, :, :3], np.tile(np.eye(3, dtype=np.float32), (int(ident.sum()), 1, 1)))
    check(b[~ident, :, :3], np.asarray(inv[~ident], dtype=np.float64), ks.inverse_bound(a[~ident], inv[~ident], U32),
          "sbmg_coarse_finish block inverse")
    rm, rb = ks.sbmg_rowmax(nc, L["cptr"], cvk, cb, ident)
    check(rowmax.view(np.float32), [rm], [rb], "sbmg_coarse_finish row-sum bound")

    # k_sbmg_restrict, plain and with the exact solve's FP64 right-hand side at a permuted position
    r4 = vec4(rng, nS)
    bpos = rng.permutation(nc).astype(np.int32)
    rc4 = np.full(4 * nc, np.nan, dtype=np.float32)
    ks.call("shim_sbmg_restrict", nc, nS, N2, L["chptr"], L["child"], L["chw"], snode, rowscale, flag, cflag, r4, rc4, None, None, 0)
    val, bnd = ks.sbmg_restrict(nc, L["chptr"], L["child"], L["chw"], snode, rowscale, flag, cflag, r4)
    rc = rc4.reshape(-1, 4)
    check(rc[:, :3], val, bnd, "sbmg_restrict")
    assert (rc[:, 3] == 0).all() and (rc[ident] == 0).all()
    rc4b = np.full(4 * nc, np.nan, dtype=np.float32)
    bd = np.full(3 * nc + 3, -7.0)
    ks.call("shim_sbmg_restrict", nc, nS, N2, L["chptr"], L["child"], L["chw"], snode, rowscale, flag, cflag, r4, rc4b, bpos, bd,
            len(bd))
    np.testing.assert_array_equal(rc4b, rc4)
    np.testing.assert_array_equal(bd[:3 * nc].reshape(-1, 3)[bpos], rc[:, :3].astype(np.float64))
    np.testing.assert_array_equal(bd[3 * nc:], -7.0)

    # k_sbmg_prolong, from xc4 and from the exact solve's FP64 answer at permuted positions
    xc4 = vec4(rng, nc)
    e4 = np.full(4 * nS, np.nan, dtype=np.float32)
    ks.call("shim_sbmg_prolong", nS, nc, L["par"], L["pw"], flag, xc4, e4, None, None, 0)
    val, bnd = ks.mg_prolong(L["par"], L["pw"], flag == 0, xc4)
    e = e4.reshape(-1, 4)
    check(e[:, :3], val, bnd, "sbmg_prolong")
    assert (e[:, 3] == 0).all() and (e[flag != 0] == 0).all()
    xd = np.zeros(3 * nc)
    xd.reshape(-1, 3)[bpos] = rng.standard_normal((nc, 3))
    e4b = np.full(4 * nS, np.nan, dtype=np.float32)
    ks.call("shim_sbmg_prolong", nS, nc, L["par"], L["pw"], flag, None, e4b, bpos, xd, len(xd))
    x_from = np.zeros((nc, 4), dtype=np.float32)
    x_from[:, :3] = xd.reshape(-1, 3)[bpos].astype(np.float32)
    val, bnd = ks.mg_prolong(L["par"], L["pw"], flag == 0, x_from.ravel())
    check(e4b.reshape(-1, 4)[:, :3], val, bnd, "sbmg_prolong from bpos / xd")


# ---- the diagonal scalings and the solid cycle's entry / exit ---------------------------------------------------------------
def csr_rows(rng, n3, width=12):
    """rows of a CSR value array: row k at a random offset, its entries random, diagpos3 somewhere inside, and for the block
    inverse the 3x3 block of node r at diagpos3[3 r + c] - c (non-symmetric, dominant)"""
    N2 = n3 // 3
    base = width * rng.permutation(n3).astype(np.int64)
    A = rng.standard_normal(width * n3)
    off = rng.integers(0, width - 3, N2)
    c = np.arange(3)
    diagpos3 = (base.reshape(-1, 3) + off[:, None] + c).ravel()
    blk = rng.standard_normal((N2, 3, 3)) + np.diag([5.0, 6.0, 7.0])
    A[(base.reshape(-1, 3) + off[:, None])[:, :, None] + c] = blk
    return A, diagpos3, blk


def test_diagonal_scalings():
    rng = np.random.default_rng(12)
    N2 = 5003
    A, diagpos3, blk = csr_rows(rng, 3 * N2)
    A[diagpos3[[3, 100]]] = [-2.5, 1e-30]                 # a negative and a tiny diagonal
    snode = np.sort(rng.choice(N2, 3001, replace=False)).astype(np.int32)
    nS = len(snode)
    blk = A[(diagpos3.reshape(-1, 3) - np.arange(3))[:, :, None] + np.arange(3)]
    # k_sb_binv
    b12 = np.full(12 * nS, np.nan, dtype=np.float32)
    b9 = np.full(9 * nS, np.nan)
    ks.call("shim_sb_binv", nS, N2, snode, diagpos3, A, len(A), b12, b9)
    inv, _ = ks.inv3(blk[snode])
    check(b9.reshape(-1, 3, 3), np.asarray(inv, dtype=np.float64), ks.inverse_bound(blk[snode], inv, EPS), "sb_binv")
    np.testing.assert_array_equal(b12.reshape(-1, 3, 4)[:, :, :3], b9.reshape(-1, 3, 3).astype(np.float32))
    assert (b12.reshape(-1, 3, 4)[:, :, 3] == 0).all()
    # k_sb_dinv, k_dinv_f32 (with and without mask), k_diag_inverse: correctly rounded divisions
    sd = np.full(4 * nS, np.nan, dtype=np.float32)
    ks.call("shim_sb_dinv", nS, N2, snode, diagpos3, A, len(A), sd)
    ref = np.zeros((nS, 4), dtype=np.float32)
    ref[:, :3] = (1.0 / A[diagpos3.reshape(-1, 3)[snode]]).astype(np.float32)
    np.testing.assert_array_equal(sd, ref.ravel())
    mask = rng.choice([0.0, 1.0, 0.7], 3 * N2)
    for m in (None, mask):
        di = np.full(4 * N2, np.nan, dtype=np.float32)
        ks.call("shim_dinv_f32", N2, m, diagpos3, A, len(A), di)
        ref = np.zeros((N2, 4), dtype=np.float32)
        ref[:, :3] = (((1.0 if m is None else m) / A[diagpos3]).astype(np.float32)).reshape(-1, 3)
        np.testing.assert_array_equal(di, ref.ravel())
    dinv = np.full(3 * N2, np.nan)
    ks.call("shim_diag_inverse", 3 * N2, diagpos3, A, len(A), dinv)
    np.testing.assert_array_equal(dinv, 1.0 / A[diagpos3])
    # k_block_scale_d: y = B y per node, B read row-major (a transposed block misses)
    y = rng.standard_normal(3 * nS)
    yk = y.copy()
    ks.call("shim_block_scale_d", nS, b9, yk)
    B = b9.reshape(-1, 3, 3)
    check(yk.reshape(-1, 3), np.einsum("ncj,nj->nc", B, y.reshape(-1, 3)),
          4 * EPS * np.einsum("ncj,nj->nc", np.abs(B), np.abs(y.reshape(-1, 3))), "block_scale_d")
    # k_gather3_f32 / k_scatter3_f32 / k_solid_cycle_init
    full = rng.standard_normal(3 * N2)
    comp = np.full(4 * nS, np.nan, dtype=np.float32)
    ks.call("shim_gather3_f32", nS, 3 * N2, snode, full, comp)
    g = np.zeros((nS, 4), dtype=np.float32)
    g[:, :3] = full.reshape(-1, 3)[snode].astype(np.float32)
    np.testing.assert_array_equal(comp, g.ravel())
    back = np.full(3 * N2, -3.0)
    src = vec4(rng, nS)
    src.reshape(-1, 4)[:, 3] = 99.0                      # the pad is not scattered
    ks.call("shim_scatter3_f32", nS, 3 * N2, snode, src, back)
    ref = np.full((N2, 3), -3.0)
    ref[snode] = src.reshape(-1, 4)[:, :3].astype(np.float64)
    np.testing.assert_array_equal(back, ref.ravel())
    x, r, d, d2 = (np.full(4 * nS, np.nan, dtype=np.float32) for _ in range(4))
    scale = np.float32(0.41)
    ks.call("shim_solid_cycle_init", nS, 3 * N2, snode, full, b12, float(scale), x, r, d, d2)
    np.testing.assert_array_equal(x, 0)
    np.testing.assert_array_equal(d2, 0)
    np.testing.assert_array_equal(r, g.ravel())
    bb = b12.reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    z = np.einsum("ncj,nj->nc", bb, g[:, :3].astype(np.float64)) * float(scale)
    zb = 4 * U32 * np.einsum("ncj,nj->nc", np.abs(bb), np.abs(g[:, :3].astype(np.float64))) * float(scale)
    dd = d.reshape(-1, 4)
    check(dd[:, :3], z, zb, "solid_cycle_init direction")
    assert (dd[:, 3] == 0).all()


# ---- live contexts --------------------------------------------------------------------------------------------------------------
TUNING = dict(dd_mg=1, solid_mg=1, scalar_dd=1, sweeps_fp32=1, solid_fp32=1, solid_block_jacobi=1, solid_fused=1,
              solid_coarse_exact=1)


def make_ctx(case, seed):
    from vasp_amd.capi import HipBackend
    from test_gpu_parity import boundary_data, random_state
    ns, desc = case[0], case[1]
    hb = HipBackend(desc, tuning=dict(TUNING))
    g, P = boundary_data(case, 1e-3)
    hb.set_dirichlet_values(g)
    hb.set_interface_pressure(P)
    refresh(hb, case, seed)
    return hb


def refresh(hb, case, seed):
    from test_gpu_parity import random_state
    U, U1 = random_state(case[0]["mesh"], hb.ndof, seed=seed)
    hb.set_state("n", U)
    hb.set_state("n-1", U1)
    hb.assemble_residual()
    hb.assemble_jacobian()
    hb.apply_preconditioner(np.random.default_rng(0).standard_normal(hb.ndof))      # forces the preconditioner's refresh


@pytest.fixture(scope="module", params=["fixture", "generated"])
def live(request, stenosis_case, tmp_path_factory):
    from conftest import prepare_case
    if request.param == "fixture":
        case = stenosis_case
    else:
        from vasp_amd.meshgen import write_mesh
        tmp = tmp_path_factory.mktemp("coarsegen")
        write_mesh(tmp / "s.h5", 12000)
        case = prepare_case("offset_stenosis", tmp / "s.h5", tmp / "run", dt="0.001", T="0.002")
    hb = make_ctx(case, 3)
    yield request.param, case, hb
    hb.close()


class Live:
    """what the checks read from a context: its arrays, the hierarchy restated from the mesh and the blocks of its Jacobian"""

    def __init__(self, hb, case):
        self.hb = hb
        self.info = ks.ctx_info(hb.ctx)
        self.A = lambda name: ks.ctx_array(hb.ctx, name)      # noqa: E731
        N2, V = self.info["N2"], self.info["V"]
        self.N2, self.V = N2, V
        s2u = self.A("solver2user").astype(np.int64)
        self.rank2node = s2u[6 * np.arange(N2)] // 3
        self.tn = np.asarray(case[1]["tet_nodes"])[hb.cell_order]
        self.rs = self.A("rowscale")
        self.M = hb.matrix().tocsr()                           # user layout, unscaled
        self.snode = self.A("snode").astype(np.int64)

    def A0(self):
        """displacement block, component 0, rank order, unscaled"""
        d = 3 * self.rank2node
        return self.M[d][:, d].tocsr()

    def Avv_t(self, nodes_rank):
        """Avv~ = Avv + ktheta Avd (solid displacement columns) on the given ranks, 3 x 3 blocks, user rows, unscaled"""
        N2 = self.N2
        nd = self.rank2node[nodes_rank]
        vrows = (3 * N2 + 3 * nd[:, None] + np.arange(3)).ravel()
        drows = (3 * nd[:, None] + np.arange(3)).ravel()
        solid = np.repeat(self.A("node_solid")[nodes_rank] != 0, 3)
        K = sp.diags(ks.ctx_ktheta(self.hb.ctx) * solid.astype(np.float64))
        Mv = self.M[vrows]
        return (Mv[:, vrows] + Mv[:, drows] @ K).tocsr(), (abs(Mv[:, vrows]) + abs(Mv[:, drows]) @ K).tocsr()


def check_hierarchy(lv):
    h = ks.p1_hierarchy(lv.tn, lv.V, lv.rank2node)
    for k in ("par", "pw", "chptr", "child", "chw", "cptr", "ccol", "cfine"):
        np.testing.assert_array_equal(lv.A("mg_" + k), h[k], err_msg=f"mg_{k}")
    assert lv.info["mg_nc"] == h["nc"] and lv.info["mg_cnnz"] == len(h["ccol"])
    hs = ks.p1_hierarchy(lv.tn, lv.V, lv.rank2node, lv.snode)
    assert hs is not None
    for k in ("par", "pw", "chptr", "child", "chw", "cptr", "ccol", "cfine"):
        np.testing.assert_array_equal(lv.A("sbmg_" + k), hs[k], err_msg=f"sbmg_{k}")
    assert lv.info["sbmg_nc"] == hs["nc"] and lv.info["sbmg_nblk"] == len(hs["ccol"])
    return h, hs


def check_displacement_level(lv, h):
    A, N2, nc = lv.A, lv.N2, h["nc"]
    nadj_ptr, nadj, db, rowflag = A("nadj_ptr"), A("nadj"), A("dd_db"), A("dd_rowflag")
    d0, mixed = ks.mg_d0(N2, nadj_ptr, nadj, db, lv.rs, rowflag)
    assert not mixed
    np.testing.assert_array_equal(A("mg_d0"), d0)
    Ac = A("mg_Ac")
    ref, S, L, missed = ks.mg_rap(nc, h["chptr"], h["child"], h["chw"], nadj_ptr, nadj, db, lv.rs, rowflag, h["par"], h["pw"],
                                  h["cptr"], h["ccol"])
    assert not missed
    check(Ac, ref, (L + 8) * EPS * S, "mg_Ac against the contract")
    P = ks.prolongation(h["par"], h["pw"], nc)
    G = ks.galerkin(P, lv.A0(), rowflag[0::3] == 0)
    crow = np.repeat(np.arange(nc), np.diff(h["cptr"]))
    check(Ac, np.asarray(G[crow, h["ccol"]]).ravel(), (L + 12) * EPS * S, "mg_Ac against P^T A0 P of the Jacobian")
    cc, cflag, dcinv4, rowmax = ks.mg_coarse_finish(nc, h["cptr"], h["ccol"], Ac, h["cfine"], rowflag)
    np.testing.assert_array_equal(A("mg_cc"), cc)
    np.testing.assert_array_equal(A("mg_cflag"), cflag)
    np.testing.assert_array_equal(A("mg_dcinv4"), dcinv4)
    assert ks.ctx_coarse(lv.hb.ctx)["mg_gersh"] == float(rowmax)
    return cc, cflag, dcinv4, d0


def solid_raw(lv, hs):
    """the solid level's Galerkin blocks before the finish: one k_sbmg_rap launch on the context's own arrays"""
    A = lv.A
    cv = np.zeros(9 * len(hs["ccol"]), dtype=np.float32)
    fl = np.zeros(4, dtype=np.int32)
    ks.call("shim_sbmg_rap", hs["nc"], lv.info["nS"], lv.N2, hs["chptr"], hs["child"], hs["chw"], A("sb_ptr"), A("sb_col"),
            A("sb_vals"), A("snode"), lv.rs, A("sbmg_flag"), hs["par"], hs["pw"], hs["cptr"], hs["ccol"], cv, fl)
    assert fl[1] == 0
    return cv


def check_solid_level(lv, hs):
    A, nc, nS = lv.A, hs["nc"], lv.info["nS"]
    sb_ptr, sb_col, sb_vals, flag = A("sb_ptr"), A("sb_col"), A("sb_vals"), A("sbmg_flag")
    np.testing.assert_array_equal(flag, ks.sbmg_flags(nS, sb_ptr, sb_col, sb_vals))
    raw = solid_raw(lv, hs)
    ref, S, L, missed = ks.sbmg_rap(nc, hs["chptr"], hs["child"], hs["chw"], sb_ptr, sb_col, sb_vals, lv.snode, lv.rs, flag,
                                    hs["par"], hs["pw"], hs["cptr"], hs["ccol"])
    assert not missed
    check(raw.reshape(-1, 9), ref, (L[:, None] + 10) * U32 * S, "sbmg raw blocks against the contract")
    At, _ = lv.Avv_t(lv.snode)
    Ps = sp.kron(ks.prolongation(hs["par"], hs["pw"], nc), sp.eye(3)).tocsr()
    G = ks.galerkin(Ps, At, np.repeat(flag == 0, 3))
    crow = np.repeat(np.arange(nc), np.diff(hs["cptr"]))
    gref = np.stack([np.asarray(G[3 * crow + c, 3 * hs["ccol"] + t]).ravel() for c in range(3) for t in range(3)], axis=1)
    check(raw.reshape(-1, 9), gref, (L[:, None] + 12) * U32 * S, "sbmg blocks against P_s^T Avv~ P_s of the Jacobian")
    ident, after, inv, a = ks.sbmg_coarse_finish(nc, hs["cptr"], hs["ccol"], raw, hs["cfine"], flag)
    np.testing.assert_array_equal(A("sbmg_cvals"), after)
    np.testing.assert_array_equal(A("sbmg_cflag"), ident.astype(np.uint8))
    b = A("sbmg_cbinv12").reshape(-1, 3, 4)
    np.testing.assert_array_equal(b[ident, :, :3], np.tile(np.eye(3, dtype=np.float32), (int(ident.sum()), 1, 1)))
    check(b[~ident, :, :3], np.asarray(inv[~ident], dtype=np.float64), ks.inverse_bound(a[~ident], inv[~ident], U32),
          "sbmg_cbinv12")
    rm, rb = ks.sbmg_rowmax(nc, hs["cptr"], after, A("sbmg_cbinv12"), ident)
    check([ks.ctx_coarse(lv.hb.ctx)["sbmg_gersh"]], [rm], [rb], "sbmg_gersh")
    return after, ident, S, L


def test_live_hierarchy_and_coarse_operators(live):
    which, case, hb = live
    lv = Live(hb, case)
    assert lv.info["mg_ready"] and lv.info["sbmg_ready"] and lv.info["bcr_ready"], lv.info
    h, hs = check_hierarchy(lv)
    check_displacement_level(lv, h)
    check_solid_level(lv, hs)
    cb = ks.ctx_coarse(hb.ctx)
    assert all(np.isfinite(v) and v > 0 for v in cb.values()), cb


def test_live_galerkin_consistency(live):
    """prolong, then the scaled fine residual of P y, then restrict: cc y (displacement level) and cvals y (solid level)"""
    which, case, hb = live
    lv = Live(hb, case)
    h, hs = check_hierarchy(lv)
    A, N2 = lv.A, lv.N2
    rng = np.random.default_rng(21)
    # displacement level; y holds small integers, so that P y (weights 1 and 1/2) is exact in FP32
    nc = h["nc"]
    cc, cflag, dcinv4, d0 = check_displacement_level(lv, h)
    y = np.zeros((nc, 4), dtype=np.float32)
    y[:, :3] = rng.integers(-512, 513, (nc, 3))
    y[cflag[0::3] == 1] = 0
    e4 = np.full(4 * N2, np.nan, dtype=np.float32)
    ks.call("shim_mg_prolong", N2, nc, h["par"], h["pw"], d0, y.ravel(), e4)
    e = e4.reshape(-1, 4)[:, :3].astype(np.float64)
    P = ks.prolongation(h["par"], h["pw"], nc)
    Py = P @ y[:, :3].astype(np.float64)
    np.testing.assert_array_equal(e, np.where((d0 != 0)[:, None], Py, 0.0))
    nadj_ptr, nadj, db = A("nadj_ptr"), A("nadj"), A("dd_db")
    row = np.repeat(np.arange(N2), np.diff(nadj_ptr))
    A0 = sp.csr_matrix((db[0::3] * (1.0 / lv.rs[6 * row]), nadj, nadj_ptr), shape=(N2, N2))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where((d0 != 0)[:, None], (A0 @ e) / d0.astype(np.float64)[:, None], 0.0)
    r4 = np.zeros((N2, 4), dtype=np.float32)
    r4[:, :3] = r
    rc4 = np.full(4 * nc, np.nan, dtype=np.float32)
    ks.call("shim_mg_restrict", nc, N2, h["chptr"], h["child"], h["chw"], d0, r4.ravel(), dcinv4, rc4, 0.0, None, None, None)
    C = sp.csr_matrix((cc.astype(np.float64), h["ccol"], h["cptr"]), shape=(nc, nc))
    Cabs = sp.csr_matrix((np.abs(cc.astype(np.float64)), h["ccol"], h["cptr"]), shape=(nc, nc))
    _, bnd = ks.mg_restrict(nc, h["chptr"], h["child"], h["chw"], d0, r4.ravel(), dcinv4)
    yy = y[:, :3].astype(np.float64)
    L = np.diff(h["cptr"])[:, None]
    check(rc4.reshape(-1, 4)[:, :3], C @ yy, 2 * bnd + (L + 12) * U32 * (Cabs @ np.abs(yy)),
          "displacement level: restrict(scaled residual of P y) against cc y")
    # solid level: r = the row-scaled block rows (sb_vals) applied to P y; restrict gives P^T (r / rowscale) = cvals y
    nS, nc = lv.info["nS"], hs["nc"]
    cvals, ident, S, Lc = check_solid_level(lv, hs)
    flag = A("sbmg_flag")
    y = np.zeros((nc, 4), dtype=np.float32)
    y[:, :3] = rng.integers(-512, 513, (nc, 3))
    y[ident] = 0
    e4 = np.full(4 * nS, np.nan, dtype=np.float32)
    ks.call("shim_sbmg_prolong", nS, nc, hs["par"], hs["pw"], flag, y.ravel(), e4, None, None, 0)
    e = e4.reshape(-1, 4)[:, :3].astype(np.float64)
    Ps = ks.prolongation(hs["par"], hs["pw"], nc)
    np.testing.assert_array_equal(e, np.where((flag == 0)[:, None], Ps @ y[:, :3].astype(np.float64), 0.0))
    sb_ptr, sb_col = A("sb_ptr"), A("sb_col")[:lv.info["sb_nblocks"]]
    B = A("sb_vals")[:9 * len(sb_col)].reshape(-1, 3, 3).astype(np.float64)
    Ab = sp.bsr_matrix((B, sb_col, sb_ptr), shape=(3 * nS, 3 * nS)).tocsr()
    r = (Ab @ e.ravel()).reshape(-1, 3)
    r4 = np.zeros((nS, 4), dtype=np.float32)
    r4[:, :3] = r
    cflag = ident.astype(np.uint8)
    rc4 = np.full(4 * nc, np.nan, dtype=np.float32)
    ks.call("shim_sbmg_restrict", nc, nS, N2, hs["chptr"], hs["child"], hs["chw"], lv.snode.astype(np.int32), lv.rs, flag, cflag,
            r4.ravel(), rc4, None, None, 0)
    _, bnd = ks.sbmg_restrict(nc, hs["chptr"], hs["child"], hs["chw"], lv.snode, lv.rs, flag, cflag, r4.ravel())
    Cb = sp.bsr_matrix((cvals.reshape(-1, 3, 3).astype(np.float64), hs["ccol"], hs["cptr"]), shape=(3 * nc, 3 * nc)).tocsr()
    yy = y[:, :3].astype(np.float64).ravel()
    # cvals against the exact blocks: (L + 10) u sum |terms| per entry (the contract's bound), applied to |y|
    Sb = sp.bsr_matrix((((Lc[:, None] + 10) * U32 * S).reshape(-1, 3, 3), hs["ccol"], hs["cptr"]), shape=(3 * nc, 3 * nc)).tocsr()
    check(rc4.reshape(-1, 4)[:, :3], (Cb @ yy).reshape(-1, 3), 2 * bnd + (Sb @ np.abs(yy)).reshape(-1, 3),
          "solid level: restrict(scaled residual of P y) against cvals y")


def test_live_diagonal_scalings_invert_the_jacobian(live):
    which, case, hb = live
    lv = Live(hb, case)
    A, N2, nS = lv.A, lv.N2, lv.info["nS"]
    all_ranks = np.arange(N2)
    nd = lv.rank2node
    drows = (3 * nd[:, None] + np.arange(3)).ravel()
    rs3 = lv.rs[:6 * N2].reshape(-1, 6)
    Add = (lv.M[drows][:, drows].diagonal() * rs3[:, :3].ravel())           # row-equilibrated, as the block holds it
    At, _ = lv.Avv_t(all_ranks)
    Avv_d = At.diagonal() * rs3[:, 3:].ravel()
    ref = np.zeros((N2, 4))
    ref[:, :3] = (1.0 / Add).reshape(-1, 3)
    check(A("dd_dinv32"), ref.ravel(), (U32 + 8 * EPS) * np.abs(ref.ravel()), "dd_dinv32 = 1 / diag A_dd")
    fluid = np.repeat(A("node_solid") == 0, 3)
    ref[:, :3] = np.where(fluid, 1.0 / Avv_d, 0.0).reshape(-1, 3)
    check(A("vvf_dinv32"), ref.ravel(), (U32 + 8 * EPS) * np.abs(ref.ravel()), "vvf_dinv32 = mask_f / diag Avv~")
    snode = lv.snode
    sref = np.zeros((nS, 4))
    sref[:, :3] = (1.0 / Avv_d).reshape(-1, 3)[snode]
    check(A("sb_dinv"), sref.ravel(), (U32 + 8 * EPS) * np.abs(sref.ravel()), "sb_dinv = 1 / diag Avv~ on the solid nodes")
    # the 3x3 diagonal blocks of the solid nodes
    Ats, _ = lv.Avv_t(snode)
    blk = np.stack([np.asarray(Ats[3 * np.arange(nS) + c, 3 * np.arange(nS) + j]).ravel() for c in range(3) for j in range(3)],
                   axis=1).reshape(-1, 3, 3) * rs3[snode, 3:][:, :, None]
    inv, _ = ks.inv3(blk)
    b9 = A("sb_binv9").reshape(-1, 3, 3)
    check(b9, np.asarray(inv, dtype=np.float64), ks.inverse_bound(blk, inv, EPS), "sb_binv9 = inverse of the diagonal blocks")
    np.testing.assert_array_equal(A("sb_binv12").reshape(-1, 3, 4)[:, :, :3], b9.astype(np.float32))
    # the Schur complement's Jacobi scaling: k_diag_inverse on its own values
    s_vals, s_diagpos = A("s_vals"), A("s_diagpos")
    np.testing.assert_array_equal(A("s_dinv"), 1.0 / s_vals[s_diagpos])


MG = ("mg_par", "mg_pw", "mg_chptr", "mg_child", "mg_chw", "mg_cptr", "mg_ccol", "mg_cfine", "mg_Ac", "mg_cc", "mg_d0",
      "mg_dcinv4", "mg_cflag")
SBMG = ("sbmg_par", "sbmg_pw", "sbmg_chptr", "sbmg_child", "sbmg_chw", "sbmg_cptr", "sbmg_ccol", "sbmg_cfine", "sbmg_cvals",
        "sbmg_cbinv12", "sbmg_flag", "sbmg_cflag")


def test_live_reproducible_and_kept_operator_fits(live, capsys):
    """a second context at the same state holds the same bits; after a Jacobian at another state, the displacement level (kept
    or rebuilt, dd_cache_hits says which) is the restatement of the NEW matrix"""
    which, case, hb = live
    hb2 = make_ctx(case, 3)
    try:
        for name in MG + SBMG:
            np.testing.assert_array_equal(ks.ctx_array(hb2.ctx, name), ks.ctx_array(hb.ctx, name), err_msg=name)
        hits0 = hb2.timers()["dd_cache_hits"]
        refresh(hb2, case, 11)
        kept = hb2.timers()["dd_cache_hits"] > hits0
        lv = Live(hb2, case)
        assert lv.info["mg_ready"] and lv.info["sbmg_ready"], lv.info
        h, hs = check_hierarchy(lv)
        check_displacement_level(lv, h)
        check_solid_level(lv, hs)
        with capsys.disabled():
            print(f"\n[{which}] displacement coarse operator after a new Jacobian: {'kept' if kept else 'rebuilt'}")
    finally:
        hb2.close()
