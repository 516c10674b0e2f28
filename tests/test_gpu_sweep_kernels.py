"""The preconditioner's sweep kernels (vasp_amd/csrc/fsi_block.hip), one launch at a time through the test shim, against the
contract written above k_sweep_tiled_f32, restated in FP64 numpy on the operator values the kernel actually holds:

    t = A d_in;  x += d_in;  r -= t;  d_out = c1 d_in + c2 dinv r        (product-only variants: y = A x)

FP32 copies are used as the float32 values themselves, FP16 records as the test's own np.float16 rounding (after checking that
the library packs the same bits).  With exact inputs the bound is the accumulation rounding alone: (row length + 8) u sum |a_ij d_j|
per row, u = 2^-24 for FP32 accumulation, eps64 for FP64 - a dropped, doubled or misplaced entry misses it by orders of magnitude.

a) synthetic operators (graphs, values and tiles built in numpy as fsi_setup.hip builds them), b) live contexts on two meshes: their
records and tiles, their FP64 operators against a scipy restatement from the assembled Jacobian (displacement pairs, solid
blocks, the Schur complement on its full pattern), and one sweep of each record kernel on the context's own structure."""
import numpy as np
import pytest

import kernel_shim as ks

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
EPS = np.finfo(np.float64).eps
C1, C2 = 0.61, 1.37


check = ks.check


# ---- synthetic node graphs -------------------------------------------------------------------------------------------------
def node_graph(N2, seed, limit_tile=False):
    """rows of 1 (diagonal only) to ~90 pairs (more than the 64 the tiled kernels prefetch); with limit_tile the first 256 nodes see
    exactly TILE_LIMIT distinct neighbours"""
    rng = np.random.default_rng(seed)
    diag_only = [0, N2 // 3, N2 - 1] if N2 > 3 else [0]
    rowptr, cols = ks.local_graph(N2, rng, reach=48, max_deg=90, diag_only=diag_only)
    if limit_tile:
        assert N2 >= ks.TILE_LIMIT + 100
        pool = rng.permutation(np.arange(256, N2))[:ks.TILE_LIMIT - 256]
        rows = [np.unique(np.concatenate([[i], pool[i::256]])) for i in range(256)]
        rest = [cols[rowptr[i]:rowptr[i + 1]] for i in range(256, N2)]
        lens = [len(r) for r in rows + rest]
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        cols = np.concatenate(rows + rest).astype(np.int32)
    return rowptr, cols


def vec4(rng, n, scale=1.0):
    v = np.zeros((n, 4), dtype=np.float32)
    v[:, :3] = (scale * rng.standard_normal((n, 3))).astype(np.float32)
    return v


def node_product(rowptr, cols, vals, d):
    """FP64 t = A d for per-pair values vals[pairs][nv] (nv = 1: one ratio for the three components) and its magnitude sum"""
    N2 = len(rowptr) - 1
    a = np.asarray(vals, dtype=np.float64).reshape(len(cols), -1)
    if a.shape[1] == 1:
        a = np.repeat(a, 3, axis=1)
    p = a * np.asarray(d, dtype=np.float64)[cols, :3]
    starts = rowptr[:-1]
    t, S = np.add.reduceat(p, starts, axis=0), np.add.reduceat(np.abs(p), starts, axis=0)
    L = np.diff(rowptr)[:, None].astype(np.float64)
    assert len(t) == N2
    return t, S, L


def node_sweep_ref(rowptr, cols, vals, rowflag, dinv, din, x, r, c1, c2):
    t, S, L = node_product(rowptr, cols, vals, din)
    d = din[:, :3].astype(np.float64)
    if rowflag is not None:
        f = rowflag.reshape(-1, 3).astype(bool)
        t[f], S[f] = d[f], np.abs(d[f])
    bt = 2 * (L + 8) * U32 * S
    di = np.ones_like(d) if dinv is None else dinv[:, :3].astype(np.float64)
    r1 = r[:, :3] - t
    br = bt + 2 * U32 * (np.abs(r[:, :3]) + np.abs(t))
    dout = c1 * d + c2 * r1 * di
    bd = np.abs(c2 * di) * br + 4 * U32 * (np.abs(c1 * d) + np.abs(c2 * r1 * di))
    x1 = x[:, :3] + d
    return (x1, 2 * U32 * np.abs(x1)), (r1, br), (dout, bd)


def check_node_sweep(name, res, din0, din, dout, x, r, pads_zero=True):
    (x1, bx), (r1, br), (d1, bd) = res
    check(x[:, :3], x1, bx, f"{name}: x += d_in")
    check(r[:, :3], r1, br, f"{name}: r -= A d_in")
    check(dout[:, :3], d1, bd, f"{name}: d_out")
    np.testing.assert_array_equal(din, din0, err_msg=f"{name} wrote d_in")
    if pads_zero:
        assert not dout[:, 3].any() and not x[:, 3].any() and not r[:, 3].any(), f"{name}: padding lane"


def node_inputs(N2, seed, nv, flag_frac=0.1):
    rng = np.random.default_rng(seed)
    din, x, r, dinv = vec4(rng, N2), vec4(rng, N2), vec4(rng, N2, 3.0), vec4(rng, N2, 0.5)
    rowflag = (rng.random(3 * N2) < flag_frac).astype(np.uint8)
    return rng, din, x, r, dinv, rowflag


NODE_SIZES = [37, 1100, 1000]     # one partial tile; 5 / 9 tiles (not multiples of 8) with partial last tiles; 4 / 8 tiles


@pytest.mark.parametrize("N2", NODE_SIZES)
def test_displacement_family(N2):
    rowptr, cols = node_graph(N2, N2)
    rng, din, x, r, dinv, rowflag = node_inputs(N2, N2 + 1, 1)
    chat = rng.uniform(-1, 1, len(cols)).astype(np.float32)
    chat[rowptr[:-1][:5]] = 1.0e3                       # a few planted large ratios
    rec_bits = ks.pack_h1(chat, np.zeros(len(chat)))
    chat_h = ks.half_value(rec_bits).astype(np.float32)  # the FP16-rounded operator the record sweeps hold
    # products: y = A x with the Dirichlet rows' identity
    t, S, L = node_product(rowptr, cols, chat, din)
    f = rowflag.reshape(-1, 3).astype(bool)
    t[f], S[f] = din[:, :3][f], 0.0
    y = np.full((N2, 4), 7.0, dtype=np.float32)
    ks.call("shim_spmv_sc_f32", N2, rowptr, cols, chat, rowflag, din, y)
    check(y[:, :3], t, 2 * (L + 8) * U32 * S, "spmv_sc_f32")
    assert not y[:, 3].any()
    for tn in (128, 256):
        uptr, ulist, ploc, max_nu = ks.build_tiles(rowptr, cols, tn, ks.TILE_LIMIT)
        for flag in (rowflag, None):
            y = np.full((N2, 4), 7.0, dtype=np.float32)
            ks.call("shim_spmv_tiled_f32", 1, tn, N2, max_nu, rowptr, chat, ploc, uptr, ulist, flag, din, y)
            tt, SS, _ = node_product(rowptr, cols, chat, din)
            if flag is not None:
                tt[f], SS[f] = din[:, :3][f], 0.0
            check(y[:, :3], tt, 2 * (L + 8) * U32 * SS, f"spmv_tiled_f32<1, {tn}> rowflag={flag is not None}")
        # fused sweeps (FP32 ratios and FP16 records), with and without dinv
        for dv in (dinv, None):
            for kind in ("f32", "h"):
                xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.full((N2, 4), 9.0, dtype=np.float32)
                if kind == "f32":
                    ks.call("shim_sweep_tiled_f32", 1, tn, N2, max_nu, rowptr, chat, ploc, uptr, ulist, rowflag, dv,
                            C1, C2, ds, do, xs, rs)
                    vals = chat
                else:
                    rec = ks.pack_h1(chat, ploc)
                    ks.call("shim_sweep_tiled_h", 1, tn, N2, max_nu, rowptr, rec, uptr, ulist, rowflag, dv, C1, C2, ds, do, xs, rs)
                    vals = chat_h
                res = node_sweep_ref(rowptr, cols, vals, rowflag, dv, din, x, r, C1, C2)
                check_node_sweep(f"sweep_tiled_{kind}<1, {tn}> dinv={dv is not None}", res, din, ds, do, xs, rs)
    # the untiled fused sweep (Jacobi-scaled: no dinv)
    xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.full((N2, 4), 9.0, dtype=np.float32)
    ks.call("shim_sweep_sc_f32", N2, rowptr, cols, chat, rowflag, C1, C2, ds, do, xs, rs)
    check_node_sweep("sweep_sc_f32", node_sweep_ref(rowptr, cols, chat, rowflag, None, din, x, r, C1, C2), din, ds, do, xs, rs)
    # the unfused path: product, then the Chebyshev update (and its start)
    n = 4 * N2
    tv = vec4(rng, N2).ravel()
    xs, rs, ds = x.ravel().copy(), r.ravel().copy(), din.ravel().copy()
    dvf = dinv.ravel()
    ks.call("shim_cheb_step_f32", n, tv, dvf, C1, C2, xs, rs, ds)
    r1 = r.ravel().astype(np.float64) - tv
    check(xs, x.ravel().astype(np.float64) + din.ravel(), 2 * U32 * np.abs(x.ravel() + din.ravel()), "cheb_step_f32: x")
    check(rs, r1, 2 * U32 * (np.abs(r.ravel()) + np.abs(tv)), "cheb_step_f32: r")
    check(ds, C1 * din.ravel().astype(np.float64) + C2 * rs.astype(np.float64) * dvf,
          4 * U32 * (np.abs(C1 * din.ravel()) + np.abs(C2 * rs * dvf)), "cheb_step_f32: d")
    rhs = vec4(rng, N2).ravel()
    xs, rs, ds = np.full(n, 5.0, np.float32), np.full(n, 5.0, np.float32), np.full(n, 5.0, np.float32)
    ks.call("shim_cheb_init_f32", n, rhs, dvf, np.float32(0.7), xs, rs, ds)
    assert not xs.any()
    np.testing.assert_array_equal(rs, rhs)
    check(ds, rhs.astype(np.float64) * 0.7 * dvf, 3 * U32 * np.abs(rhs * 0.7 * dvf), "cheb_init_f32: d")


@pytest.mark.parametrize("N2", [37, 1100])
def test_velocity_block_family(N2):
    rowptr, cols = node_graph(N2, 3 * N2)
    rng, din, x, r, dinv, rowflag = node_inputs(N2, N2 + 5, 3)
    vals = rng.uniform(-1, 1, 3 * len(cols)).astype(np.float32)
    vals_h = ks.half_value(ks.half_bits(vals)).astype(np.float32)
    t, S, L = node_product(rowptr, cols, vals, din)
    y = np.full((N2, 4), 7.0, dtype=np.float32)
    ks.call("shim_spmv_db_f32", N2, rowptr, cols, vals, din, y)
    check(y[:, :3], t, 2 * (L + 8) * U32 * S, "spmv_db_f32")
    assert not y[:, 3].any()
    for tn in (128, 256):
        uptr, ulist, ploc, max_nu = ks.build_tiles(rowptr, cols, tn, ks.TILE_LIMIT)
        y = np.full((N2, 4), 7.0, dtype=np.float32)
        ks.call("shim_spmv_tiled_f32", 3, tn, N2, max_nu, rowptr, vals, ploc, uptr, ulist, None, din, y)
        check(y[:, :3], t, 2 * (L + 8) * U32 * S, f"spmv_tiled_f32<3, {tn}>")
        for kind in ("f32", "h"):
            xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.full((N2, 4), 9.0, dtype=np.float32)
            if kind == "f32":
                ks.call("shim_sweep_tiled_f32", 3, tn, N2, max_nu, rowptr, vals, ploc, uptr, ulist, rowflag, dinv,
                        C1, C2, ds, do, xs, rs)
                v = vals
            else:
                rec = ks.pack_h3(vals, ploc)
                ks.call("shim_sweep_tiled_h", 3, tn, N2, max_nu, rowptr, rec, uptr, ulist, rowflag, dinv, C1, C2, ds, do, xs, rs)
                v = vals_h
            res = node_sweep_ref(rowptr, cols, v, rowflag, dinv, din, x, r, C1, C2)
            check_node_sweep(f"sweep_tiled_{kind}<3, {tn}>", res, din, ds, do, xs, rs)


def test_tile_at_the_lds_limit():
    assert ks.load().shim_tile_limit() == ks.TILE_LIMIT, "the library's tile_limit() moved: the limit cases below no longer reach it"
    N2 = ks.TILE_LIMIT + 700
    rowptr, cols = node_graph(N2, 11, limit_tile=True)
    rng, din, x, r, dinv, rowflag = node_inputs(N2, 12, 1)
    chat = rng.uniform(-1, 1, len(cols)).astype(np.float32)
    uptr, ulist, ploc, max_nu = ks.build_tiles(rowptr, cols, 256, ks.TILE_LIMIT)
    assert max_nu == ks.TILE_LIMIT
    for kind in ("f32", "h"):
        xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.zeros((N2, 4), dtype=np.float32)
        if kind == "f32":
            ks.call("shim_sweep_tiled_f32", 1, 256, N2, max_nu, rowptr, chat, ploc, uptr, ulist, rowflag, dinv, C1, C2, ds, do, xs, rs)
            v = chat
        else:
            ks.call("shim_sweep_tiled_h", 1, 256, N2, max_nu, rowptr, ks.pack_h1(chat, ploc), uptr, ulist, rowflag, dinv,
                    C1, C2, ds, do, xs, rs)
            v = ks.half_value(ks.half_bits(chat)).astype(np.float32)
        check_node_sweep(f"sweep_tiled_{kind}<1, 256> at {max_nu} distinct neighbours",
                         node_sweep_ref(rowptr, cols, v, rowflag, dinv, din, x, r, C1, C2), din, ds, do, xs, rs)


# ---- solid block (3x3 block CSR) -------------------------------------------------------------------------------------------
def solid_inputs(nS, seed):
    rng = np.random.default_rng(seed)
    sb_ptr, sb_col = ks.local_graph(nS, rng, reach=40, max_deg=80, diag_only=[0, nS - 1] if nS > 2 else [0])
    vals = rng.uniform(-1, 1, 9 * len(sb_col)).astype(np.float32)
    binv = np.zeros((nS, 3, 4), dtype=np.float32)
    binv[:, :, :3] = rng.uniform(-1, 1, (nS, 3, 3)).astype(np.float32)
    return rng, sb_ptr, sb_col, vals, binv.ravel()


def block_product(sb_ptr, sb_col, vals, d):
    A = np.asarray(vals, dtype=np.float64).reshape(-1, 3, 3)
    dv = np.asarray(d, dtype=np.float64).reshape(-1, 4)[sb_col, :3]
    p = A * dv[:, None, :]
    t = np.add.reduceat(p.sum(axis=2), sb_ptr[:-1], axis=0)
    S = np.add.reduceat(np.abs(p).sum(axis=2), sb_ptr[:-1], axis=0)
    L = 3 * np.diff(sb_ptr)[:, None].astype(np.float64)
    return t, S, L


def bmul(binv12, v):
    B = np.asarray(binv12, dtype=np.float64).reshape(-1, 3, 4)[:, :, :3]
    v = np.asarray(v, dtype=np.float64)
    return np.einsum("nij,nj->ni", B, v), np.einsum("nij,nj->ni", np.abs(B), np.abs(v))


def solid_sweep_ref(t, S, L, binv, din, x, r):
    d = din.reshape(-1, 4)[:, :3].astype(np.float64)
    r0 = r.reshape(-1, 4)[:, :3].astype(np.float64)
    r1 = r0 - t
    br = 2 * (L + 8) * U32 * S + 2 * U32 * (np.abs(r0) + np.abs(t))
    z, zm = bmul(binv, r1)
    _, bz = bmul(binv, br)
    dout = C1 * d + C2 * z
    bd = np.abs(C2) * (bz + 4 * U32 * zm) + 4 * U32 * (np.abs(C1 * d) + np.abs(C2 * z))
    x1 = x.reshape(-1, 4)[:, :3] + d
    return (x1, 2 * U32 * np.abs(x1)), (r1, br), (dout, bd)


def check_solid(name, res, x0, r0, d0, din, dout, x, r, dout0):
    (x1, bx), (r1, br), (dd, bd) = res
    x4, r4, o4 = x.reshape(-1, 4), r.reshape(-1, 4), dout.reshape(-1, 4)
    check(x4[:, :3], x1, bx, f"{name}: x")
    check(r4[:, :3], r1, br, f"{name}: r")
    check(o4[:, :3], dd, bd, f"{name}: d_out")
    np.testing.assert_array_equal(din, d0, err_msg=f"{name} wrote d_in")
    # the padding lane is not touched by the block sweeps
    np.testing.assert_array_equal(x4[:, 3], x0.reshape(-1, 4)[:, 3])
    np.testing.assert_array_equal(r4[:, 3], r0.reshape(-1, 4)[:, 3])
    np.testing.assert_array_equal(o4[:, 3], dout0.reshape(-1, 4)[:, 3])


@pytest.mark.parametrize("nS", [1, 17, 1000])
def test_solid_block_family(nS):
    rng, sb_ptr, sb_col, vals, binv = solid_inputs(nS, nS)
    din, x, r = vec4(rng, nS).ravel(), vec4(rng, nS).ravel(), vec4(rng, nS, 3.0).ravel()
    x[3::4], r[3::4] = 2.5, -1.5                            # padding lanes the sweeps must leave alone
    t, S, L = block_product(sb_ptr, sb_col, vals, din)
    y = np.full(4 * nS, 7.0, dtype=np.float32)
    ks.call("shim_spmv_sb", nS, sb_ptr, sb_col, vals, din, y)
    check(y.reshape(-1, 4)[:, :3], t, 2 * (L + 8) * U32 * S, "spmv_sb")
    assert not y[3::4].any()
    vals_h = ks.half_value(ks.half_bits(vals)).astype(np.float32)
    th, Sh, _ = block_product(sb_ptr, sb_col, vals_h, din)
    for name in ("sweep_sb_b3<0>", "sweep_sb_b3<1>", "sweep_sb_h"):
        xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.full(4 * nS, 9.0, dtype=np.float32)
        do0 = do.copy()
        if name == "sweep_sb_h":
            ks.call("shim_sweep_sb_h", nS, sb_ptr, ks.pack_sb(vals, sb_col), binv, C1, C2, ds, do, xs, rs)
            res = solid_sweep_ref(th, Sh, L, binv, din, x, r)
        else:
            ks.call("shim_sweep_sb_b3", nS, sb_ptr, sb_col, vals, binv, C1, C2, ds, do, xs, rs, int(name[-2]))
            res = solid_sweep_ref(t, S, L, binv, din, x, r)
        check_solid(name, res, x, r, din, ds, do, xs, rs, do0)
    # the unfused path: t given, then the block-Jacobi Chebyshev update; and its start
    tv = vec4(rng, nS).ravel()
    xs, rs, ds = x.copy(), r.copy(), din.copy()
    ks.call("shim_cheb_step_b3", nS, tv, binv, C1, C2, xs, rs, ds)
    tt = tv.reshape(-1, 4)[:, :3].astype(np.float64)
    d0, x0, r0 = (v.reshape(-1, 4)[:, :3].astype(np.float64) for v in (din, x, r))
    r1 = r0 - tt
    br = 2 * U32 * (np.abs(r0) + np.abs(tt))
    z, zm = bmul(binv, r1)
    check(xs.reshape(-1, 4)[:, :3], x0 + d0, 2 * U32 * np.abs(x0 + d0), "cheb_step_b3: x")
    check(rs.reshape(-1, 4)[:, :3], r1, br, "cheb_step_b3: r")
    check(ds.reshape(-1, 4)[:, :3], C1 * d0 + C2 * z,
          np.abs(C2) * (bmul(binv, br)[1] + 4 * U32 * zm) + 4 * U32 * (np.abs(C1 * d0) + np.abs(C2 * z)), "cheb_step_b3: d")
    np.testing.assert_array_equal(xs[3::4], x[3::4])
    assert not ds[3::4].any()
    np.testing.assert_array_equal(rs[3::4], r[3::4])
    rhs = vec4(rng, nS).ravel()
    xs, rs, ds = np.full(4 * nS, 5.0, np.float32), np.full(4 * nS, 5.0, np.float32), np.full(4 * nS, 5.0, np.float32)
    ks.call("shim_cheb_init_b3", nS, rhs, binv, np.float32(0.7), xs, rs, ds)
    assert not xs.any()
    np.testing.assert_array_equal(rs, rhs)
    z, zm = bmul(binv, rhs.reshape(-1, 4)[:, :3])
    check(ds.reshape(-1, 4)[:, :3], 0.7 * z, 6 * U32 * 0.7 * zm, "cheb_init_b3: d")
    assert not ds[3::4].any()


# ---- Schur sweeps (FP64 vectors) ---------------------------------------------------------------------------------------------
def schur_graph(n, seed, limit_tile=False):
    rng = np.random.default_rng(seed)
    rowptr, cols = ks.local_graph(n, rng, reach=90, max_deg=130, diag_only=[1, n - 2] if n > 3 else [0])
    if limit_tile:                                          # rows 0 .. 255 see exactly SCHUR_TILE_LIMIT distinct columns
        assert n >= ks.SCHUR_TILE_LIMIT + 100
        pool = rng.permutation(np.arange(256, n))[:ks.SCHUR_TILE_LIMIT - 256]
        rows = [np.unique(np.concatenate([[i], pool[i::256]])) for i in range(256)]
        rest = [cols[rowptr[i]:rowptr[i + 1]] for i in range(256, n)]
        rowptr = np.concatenate([[0], np.cumsum([len(q) for q in rows + rest])]).astype(np.int64)
        cols = np.concatenate(rows + rest).astype(np.int32)
    diagpos = np.array([rowptr[i] + int(np.flatnonzero(cols[rowptr[i]:rowptr[i + 1]] == i)[0]) for i in range(n)], dtype=np.int64)
    vals = rng.uniform(-1, 1, len(cols))
    vals[diagpos] = rng.uniform(2, 4, n)
    return rng, rowptr, cols, diagpos, vals


def schur_ref(rowptr, cols, a, dinv, din, x, r):
    p = np.asarray(a, dtype=np.float64) * din[cols]
    t, S = np.add.reduceat(p, rowptr[:-1]), np.add.reduceat(np.abs(p), rowptr[:-1])
    L = np.diff(rowptr).astype(np.float64)
    r1 = r - t
    br = 2 * (L + 8) * EPS * S + 2 * EPS * (np.abs(r) + np.abs(t))
    dout = C1 * din + C2 * r1 * dinv
    bd = np.abs(C2 * dinv) * br + 4 * EPS * (np.abs(C1 * din) + np.abs(C2 * r1 * dinv))
    return (x + din, 2 * EPS * np.abs(x + din)), (r1, br), (dout, bd)


def check_schur(name, res, din0, din, dout, x, r):
    (x1, bx), (r1, br), (d1, bd) = res
    check(x, x1, bx, f"{name}: x")
    check(r, r1, br, f"{name}: r")
    check(dout, d1, bd, f"{name}: d_out")
    np.testing.assert_array_equal(din, din0, err_msg=f"{name} wrote d_in")


def schur_vectors(rng, n):
    return rng.standard_normal(n), rng.standard_normal(n), 3 * rng.standard_normal(n)


@pytest.mark.parametrize("n", [1, 300, 1000, ks.SCHUR_TILE_LIMIT + 300])
def test_schur_family(n):
    limit = n > ks.SCHUR_TILE_LIMIT
    rng, rowptr, cols, diagpos, vals = schur_graph(n, n, limit_tile=limit)
    din, x, r = schur_vectors(rng, n)
    dinv_diag = 1.0 / vals[diagpos]
    xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.full(n, 9.0)
    ks.call("shim_sweep_csr_f64", n, rowptr, cols, vals, diagpos, C1, C2, ds, do, xs, rs)
    check_schur("sweep_csr_f64", schur_ref(rowptr, cols, vals, dinv_diag, din, x, r), din, ds, do, xs, rs)
    v32 = vals.astype(np.float32)
    xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.full(n, 9.0)
    ks.call("shim_sweep_csr_mixed", n, rowptr, cols, v32, diagpos, vals, C1, C2, ds, do, xs, rs)
    check_schur("sweep_csr_mixed", schur_ref(rowptr, cols, v32, dinv_diag, din, x, r), din, ds, do, xs, rs)
    vh = ks.half_value(ks.half_bits(v32))
    dinv = rng.uniform(0.2, 0.5, n)
    for tr in (32, 64, 128, 256):
        uptr, ulist, ploc, max_nu = ks.build_tiles(rowptr, cols, tr, ks.SCHUR_TILE_LIMIT)
        if limit and tr == 256:
            assert max_nu == ks.SCHUR_TILE_LIMIT
        rec = ks.pack_h1(v32, ploc)
        xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.full(n, 9.0)
        ks.call("shim_sweep_schur_tiled", tr, n, max_nu, rowptr, rec, uptr, ulist, dinv, C1, C2, ds, do, xs, rs)
        check_schur(f"sweep_schur_tiled<{tr}>", schur_ref(rowptr, cols, vh, dinv, din, x, r), din, ds, do, xs, rs)


# ---- the library's FP16 packing against the test's own rounding ------------------------------------------------------------
def edge_floats(rng, n):
    special = np.array([0.0, -0.0, 1.0, -1.0, 1 + 2**-11, 1 + 3 * 2**-11, 1 - 2**-12, 65504.0, 65519.0, 65520.0, 1e6, -1e6,
                        2**-14, 2**-24, 2**-25, 3 * 2**-26, 6e-8, -5.9e-8, 1e-30, 0.1, 1 / 3], dtype=np.float32)
    v = rng.standard_normal(n).astype(np.float32) * np.float32(10.0) ** rng.integers(-9, 5, n).astype(np.float32)
    v[:len(special)] = special
    return v


def test_fp16_packing_matches_the_reference_rounding():
    rng = np.random.default_rng(5)
    n = 4099
    v = edge_floats(rng, 9 * n)
    loc = rng.integers(0, 65536, n).astype(np.uint16)
    rec = np.zeros(n, dtype=np.uint32)
    ks.call("shim_pack_h1", n, v[:n], loc, rec)
    np.testing.assert_array_equal(rec, ks.pack_h1(v[:n], loc))
    rec3 = np.zeros(2 * n, dtype=np.uint32)
    ks.call("shim_pack_h3", n, v[:3 * n], loc, rec3)
    np.testing.assert_array_equal(rec3, ks.pack_h3(v[:3 * n], loc))
    col = rng.integers(0, 2**31 - 1, n).astype(np.int32)
    recs = np.zeros(6 * n, dtype=np.uint32)
    ks.call("shim_pack_sb", n, v, col, recs)
    np.testing.assert_array_equal(recs, ks.pack_sb(v, col))


# ---- b) live contexts: the records and tiles the sweeps read, and one sweep on the context's own tile structure --------------
@pytest.fixture(scope="module", params=["fixture", "generated"])
def live_ctx(request, stenosis_case, tmp_path_factory):
    from conftest import prepare_case
    from vasp_amd.capi import HipBackend
    from test_gpu_parity import boundary_data, random_state
    if request.param == "fixture":
        case = stenosis_case
    else:
        from vasp_amd.meshgen import write_mesh
        tmp = tmp_path_factory.mktemp("sweepgen")
        write_mesh(tmp / "s.h5", 12000)
        case = prepare_case("offset_stenosis", tmp / "s.h5", tmp / "run", dt="0.001", T="0.002")
    ns, desc = case[0], case[1]
    # every structure the sweeps read is pinned here, not taken from the environment
    hb = HipBackend(desc, tuning=dict(tiles=1, tile_nodes=256, fused_sweeps=1, scalar_dd=1, sweeps_fp32=1, sweeps_fp16=1,
                                      solid_fp32=1, solid_fused=1, schur_fp32=1, schur_tile_rows=64))
    g, P = boundary_data(case, 1e-3)
    U, U1 = random_state(ns["mesh"], hb.ndof, seed=3)
    hb.set_state("n", U)
    hb.set_state("n-1", U1)
    hb.set_dirichlet_values(g)
    hb.set_interface_pressure(P)
    hb.assemble_residual()
    hb.assemble_jacobian()
    hb.apply_preconditioner(np.random.default_rng(0).standard_normal(hb.ndof))      # forces the preconditioner's refresh
    yield request.param, hb
    hb.close()


def test_live_context_records_and_tiles(live_ctx):
    which, hb = live_ctx
    info = ks.ctx_info(hb.ctx)
    A = lambda name: ks.ctx_array(hb.ctx, name)      # noqa: E731
    N2, V = info["N2"], info["V"]
    if which == "generated":
        assert N2 % 256 != 0, "the generated mesh was meant to leave a partial last tile"
    assert info["tiled"] and info["schur_tiled"] and info["sweeps_fp16"], info
    # node tiles: the numpy builder on the context's own graph gives the tiles and local indices the library uploaded
    nadj_ptr, nadj = A("nadj_ptr"), A("nadj")
    uptr, ulist, ploc, max_nu = ks.build_tiles(nadj_ptr, nadj, info["tile_nodes"], ks.TILE_LIMIT)
    np.testing.assert_array_equal(A("tile_uptr"), uptr)
    np.testing.assert_array_equal(A("tile_ulist"), ulist)
    np.testing.assert_array_equal(A("tile_ploc"), ploc)
    assert info["tile_max_nu"] == max_nu
    chat = A("dd_chat")
    assert np.isfinite(chat).all()
    np.testing.assert_array_equal(A("dd_rec"), ks.pack_h1(chat, ploc))
    vv = A("vv_db32")
    assert np.isfinite(vv).all()
    np.testing.assert_array_equal(A("vv_rec"), ks.pack_h3(vv, ploc))
    # solid blocks
    sb_vals, sb_col = A("sb_vals"), A("sb_col")
    assert np.isfinite(sb_vals).all()
    np.testing.assert_array_equal(A("sb_rec")[:6 * info["sb_nblocks"]], ks.pack_sb(sb_vals[:9 * info["sb_nblocks"]], sb_col[:info["sb_nblocks"]]))
    # Schur: FP32 copy = rounding of the FP64 values; records = FP16 rounding + tile-local column of the context's own tiles
    s_rowptr, s_cols, s_vals, s_vals32 = A("s_rowptr"), A("s_cols"), A("s_vals"), A("s_vals32")
    assert np.isfinite(s_vals).all()
    np.testing.assert_array_equal(s_vals32, s_vals.astype(np.float32))
    suptr, sulist, sploc, smax = ks.build_tiles(s_rowptr, s_cols, info["schur_tile"], ks.SCHUR_TILE_LIMIT)
    np.testing.assert_array_equal(A("s_tile_uptr"), suptr)
    np.testing.assert_array_equal(A("s_tile_ulist"), sulist)
    np.testing.assert_array_equal(A("s_ploc"), sploc)
    assert info["s_tile_max_nu"] == smax
    s_rec = A("s_rec")
    np.testing.assert_array_equal(s_rec, ks.pack_h1(s_vals32, sploc))
    # every record's local index names its own column through its tile's list
    row = np.repeat(np.arange(V), np.diff(s_rowptr))
    np.testing.assert_array_equal(sulist[suptr[row // info["schur_tile"]] + (s_rec >> 16)], s_cols)

    # one sweep of the Schur and displacement record kernels on the context's own structure
    rng = np.random.default_rng(1)
    din, x, r = schur_vectors(rng, V)
    dinv = A("s_dinv")
    assert np.isfinite(dinv).all()
    xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.zeros(V)
    ks.call("shim_sweep_schur_tiled", info["schur_tile"], V, smax, s_rowptr, s_rec, suptr, sulist, dinv, C1, C2, ds, do, xs, rs)
    check_schur("live sweep_schur_tiled", schur_ref(s_rowptr, s_cols, ks.half_value(s_rec), dinv, din, x, r), din, ds, do, xs, rs)
    rowflag = A("dd_rowflag")
    din4, x4, r4 = vec4(rng, N2), vec4(rng, N2), vec4(rng, N2)
    xs, rs, ds, do = x4.copy(), r4.copy(), din4.copy(), np.zeros((N2, 4), dtype=np.float32)
    ks.call("shim_sweep_tiled_h", 1, info["tile_nodes"], N2, max_nu, nadj_ptr, A("dd_rec"), uptr, ulist, rowflag, None, C1, C2,
            ds, do, xs, rs)
    vh = ks.half_value(ks.half_bits(chat)).astype(np.float32)
    check_node_sweep("live sweep_tiled_h<1>", node_sweep_ref(nadj_ptr, nadj, vh, rowflag, None, din4, x4, r4, C1, C2),
                     din4, ds, do, xs, rs)
    # the velocity block's records (NV = 3) and the solid block's records on the context's own structure
    xs, rs, ds, do = x4.copy(), r4.copy(), din4.copy(), np.zeros((N2, 4), dtype=np.float32)
    ks.call("shim_sweep_tiled_h", 3, info["tile_nodes"], N2, max_nu, nadj_ptr, A("vv_rec"), uptr, ulist, None, None, C1, C2,
            ds, do, xs, rs)
    v3, _ = ks.unpack_h3(A("vv_rec"))
    np.testing.assert_array_equal(v3.astype(np.float32), ks.half_value(ks.half_bits(vv)).astype(np.float32).reshape(-1, 3))
    check_node_sweep("live sweep_tiled_h<3>", node_sweep_ref(nadj_ptr, nadj, v3, None, None, din4, x4, r4, C1, C2),
                     din4, ds, do, xs, rs)
    nS, nb = info["nS"], info["sb_nblocks"]
    assert nS > 0 and nb > 0
    sb_ptr, binv = A("sb_ptr"), A("sb_binv12")
    d4, y4, q4 = vec4(rng, nS).ravel(), vec4(rng, nS).ravel(), vec4(rng, nS).ravel()
    sbv_h = ks.half_value(ks.half_bits(sb_vals[:9 * nb])).astype(np.float32)
    t, S, L = block_product(sb_ptr, sb_col[:nb], sbv_h, d4)
    xs, rs, ds, do = y4.copy(), q4.copy(), d4.copy(), np.zeros(4 * nS, dtype=np.float32)
    ks.call("shim_sweep_sb_h", nS, sb_ptr, A("sb_rec"), binv, C1, C2, ds, do, xs, rs)
    check_solid("live sweep_sb_h", solid_sweep_ref(t, S, L, binv, d4, y4, q4), y4, q4, d4, ds, do, xs, rs, np.zeros(4 * nS))
    # which variants the context runs: tiled sweeps fused with the update (bit 0) on FP16 records (bit 1)
    flags = hb.timers()["sweep_flags"]
    assert flags & 1 and flags & 2, f"sweep_flags {flags:#x}: the pinned tuning should run the fused FP16-record sweeps"


@pytest.mark.parametrize("tiles, tile_nodes, schur_tile", [(1, 128, 32), (1, 256, 256), (0, 256, 64)])
def test_live_context_tiles_at_every_tile_size(stenosis_case, tiles, tile_nodes, schur_tile):
    """The node tiles and the Schur tiles of a fresh context (fsi_setup.hip builds both with one function) are ks.build_tiles on
    the context's own graphs, entry for entry, at the other sizes FsiTuning offers; with tiles = 0 there are no node tiles."""
    from vasp_amd.capi import HipBackend
    hb = HipBackend(stenosis_case[1], tuning=dict(tiles=tiles, tile_nodes=tile_nodes, schur_tile_rows=schur_tile))
    try:
        info = ks.ctx_info(hb.ctx)
        A = lambda name: ks.ctx_array(hb.ctx, name)      # noqa: E731
        assert info["tile_nodes"] == tile_nodes and info["schur_tile"] == schur_tile, info
        if tiles:
            uptr, ulist, ploc, max_nu = ks.build_tiles(A("nadj_ptr"), A("nadj"), tile_nodes, ks.TILE_LIMIT)
            assert info["tiled"] == 1
            np.testing.assert_array_equal(A("tile_uptr"), uptr)
            np.testing.assert_array_equal(A("tile_ulist"), ulist)
            np.testing.assert_array_equal(A("tile_ploc"), ploc)
            assert info["tile_max_nu"] == max_nu
        else:
            assert info["tiled"] == 0 and info["tile_max_nu"] == 0
            assert len(A("tile_uptr")) == 0 and len(A("tile_ulist")) == 0 and len(A("tile_ploc")) == 0
        suptr, sulist, sploc, smax = ks.build_tiles(A("s_rowptr"), A("s_cols"), schur_tile, ks.SCHUR_TILE_LIMIT)
        assert info["schur_tiled"] == 1
        np.testing.assert_array_equal(A("s_tile_uptr"), suptr)
        np.testing.assert_array_equal(A("s_tile_ulist"), sulist)
        np.testing.assert_array_equal(A("s_ploc"), sploc)
        assert info["s_tile_max_nu"] == smax
    finally:
        hb.close()


def test_live_context_operators_are_the_jacobian_blocks(live_ctx):
    """The FP64 sources of the sweeps' copies against a scipy restatement from the assembled Jacobian (fsi_get_matrix, user
    layout, mapped through solver2user and row-equilibrated by rowscale).  Solver layout: node rank r holds d rows 6r + i and
    v rows 6r + 3 + i, pressure position q row 6 N2 + q.  Avv~ = Avv + ktheta Avd and Apv~ = Apv + ktheta Apd on the
    displacement columns of solid nodes (k_extract_blocks)."""
    import scipy.sparse as sp
    _, hb = live_ctx
    info = ks.ctx_info(hb.ctx)
    A = lambda name: ks.ctx_array(hb.ctx, name)      # noqa: E731
    N2, V = info["N2"], info["V"]
    lb = ks.live_blocks(hb)                          # the scipy restatement, shared with tests/test_gpu_block_kernels.py
    M, Vd, Pd, node = lb["M"], lb["Vd"], lb["Pd"], np.arange(N2)
    Add, Avv_t, Avv_mag, Apv_t, Apv_mag, App, Avp = (lb[k] for k in ("Add", "Avv_t", "Avv_mag", "Apv_t", "Apv_mag", "App", "Avp"))

    # displacement pair values: dd_db[3e + i] = Add[3r + i, 3b + i], i.e. a0_ab = dd_db / rowscale_a is the assembled entry
    nadj_ptr, nadj = A("nadj_ptr"), A("nadj").astype(np.int64)
    r_e = np.repeat(node, np.diff(nadj_ptr))
    ref = np.stack([np.asarray(Add[3 * r_e + i, 3 * nadj + i]).ravel() for i in range(3)], axis=1)
    db = A("dd_db").reshape(-1, 3)
    check(db, ref, 2 * EPS * np.abs(ref), "dd_db against the Jacobian's displacement block")
    # chat: the ratio to the diagonal in the first component whose row has off-diagonal entries (1 / 0 on identity rows)
    is_diag = nadj == r_e
    assert np.array_equal(np.bincount(r_e[is_diag], minlength=N2), np.ones(N2, dtype=np.int64))
    diag_e = np.flatnonzero(is_diag)
    offnz = (ref != 0) & ~is_diag[:, None]
    ident = np.add.reduceat(offnz.astype(np.int64), nadj_ptr[:-1], axis=0) == 0
    np.testing.assert_array_equal(A("dd_rowflag").reshape(-1, 3), ident.astype(np.uint8))
    refc = np.argmax(~ident, axis=1)
    ratio = ref[np.arange(len(r_e)), refc[r_e]] / ref[diag_e[r_e], refc[r_e]]
    chat_ref = np.where(ident.all(axis=1)[r_e], is_diag.astype(np.float64), ratio)
    check(A("dd_chat"), chat_ref, (2.0 ** -24 + 8 * EPS) * np.abs(chat_ref), "dd_chat against Add / diag(Add)")

    # solid blocks: sb_vals = FP32 rounding of the 3x3 blocks of Avv~ between solid nodes
    nb, snode = info["sb_nblocks"], A("snode").astype(np.int64)
    sb_ptr, sb_col = A("sb_ptr"), A("sb_col")[:nb].astype(np.int64)
    rr, cc = snode[np.repeat(np.arange(info["nS"]), np.diff(sb_ptr))], snode[sb_col]
    blk_ref = np.stack([np.asarray(Avv_t[3 * rr + c, 3 * cc + j]).ravel() for c in range(3) for j in range(3)], axis=1)
    blk_mag = np.stack([np.asarray(Avv_mag[3 * rr + c, 3 * cc + j]).ravel() for c in range(3) for j in range(3)], axis=1)
    check(A("sb_vals")[:9 * nb].reshape(-1, 9), blk_ref, 2.0 ** -24 * np.abs(blk_ref) + 8 * EPS * blk_mag,
          "sb_vals against the solid rows of the velocity block")

    # Schur complement S = A_pp - Apv~ diag(Avv~)^-1 A_vp on its full two-ring pattern
    dinv = 1.0 / Avv_t.diagonal()
    S_ref = (App - Apv_t @ sp.diags(dinv) @ Avp).tocsr()
    S_mag = (abs(App) + Apv_mag @ sp.diags(np.abs(dinv)) @ abs(Avp)).tocsr()
    one = lambda X: sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)      # noqa: E731
    pattern = (one(App) + one(M[Pd][:, Vd]) @ one(Avp)).tocsr()
    pattern.sort_indices()
    s_rowptr, s_cols = A("s_rowptr"), A("s_cols")
    np.testing.assert_array_equal(s_rowptr, pattern.indptr, err_msg="Schur pattern: row lengths")
    np.testing.assert_array_equal(s_cols, pattern.indices, err_msg="Schur pattern: a fill entry missing or extra")
    S_ctx = sp.csr_matrix((A("s_vals"), s_cols, s_rowptr), shape=(V, V))
    excess = (abs(S_ctx - S_ref) - 256 * EPS * S_mag).tocsr()
    worst = excess.data.max() if excess.nnz else 0.0
    assert worst <= 0.0, f"s_vals differs from the restated Schur complement by {worst:.3e} beyond the bound"
