"""The sweep kernels of the all-FP64-storage mode added beside the ones they replace (vasp_amd/csrc/fsi_block.hip), against
those, BITWISE: the same values in the same precision, the products added in the same order, so d_out, x and r must be the same bits.

    k_sweep_schur_tiled_f64<tile>                  vs  k_sweep_csr_mixed<8, 8, double>   (launch_sweep_csr_f64)
    k_sweep_tiled_r<3, tn, records>  (r3)          vs  k_sweep_tiled_f32<3, tn>
    k_sweep_tiled_r<1, tn, two arrays>  (a1)       vs  k_sweep_tiled_f32<1, tn>
    k_sweep_sb_r                                   vs  k_sweep_sb_b3<0>

Covered: rows longer than 64 entries, empty rows, Dirichlet rowflag rows, a tile at the LDS limit, every Schur tile size.  And a
live context in the FP64-storage configuration: its records are exactly the packing of the arrays they came from."""
import numpy as np
import pytest

import fp32_records as fr
import kernel_shim as ks
from test_gpu_sweep_kernels import node_graph, node_inputs, schur_graph, schur_vectors, solid_inputs, vec4

pytestmark = pytest.mark.gpu

C1, C2 = 0.61, 1.37


@pytest.fixture(scope="module", autouse=True)
def shim():
    return fr.load()


def same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    ui = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    g, r = got.view(ui).ravel(), ref.view(ui).ravel()
    bad = np.flatnonzero(g != r)
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(g)} entries differ; first at {bad[0]}: {got.ravel()[bad[0]]!r} against "
                           f"{ref.ravel()[bad[0]]!r}")


def empty_rows(rowptr, cols, rows, *per_entry):
    """the graph with the entries of `rows` removed (those rows become empty); per_entry arrays (len(cols) x k) follow"""
    n = len(rowptr) - 1
    keep = np.ones(len(cols), dtype=bool)
    for i in rows:
        keep[rowptr[i]:rowptr[i + 1]] = False
    lens = np.diff(rowptr).copy()
    lens[list(rows)] = 0
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert len(rp) == n + 1
    out = [np.ascontiguousarray(a.reshape(len(cols), -1)[keep].reshape(-1)) for a in per_entry]
    return (rp, np.ascontiguousarray(cols[keep]), *out)


def long_rows(rowptr, cols, rows, length):
    """the graph with each row of `rows` replaced by `length` consecutive columns around it (its diagonal included)"""
    n = len(rowptr) - 1
    out = [cols[rowptr[i]:rowptr[i + 1]] for i in range(n)]
    for i in rows:
        lo = max(0, min(i - length // 2, n - length))
        out[i] = np.arange(lo, lo + length, dtype=np.int32)
    rp = np.concatenate([[0], np.cumsum([len(q) for q in out])]).astype(np.int64)
    return rp, np.concatenate(out).astype(np.int32)


# ---- Schur ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,empty", [(1, False), (300, False), (1000, False), (1000, True), (ks.SCHUR_TILE_LIMIT + 300, False)])
def test_schur_tiled_f64_is_the_csr_sweep(n, empty):
    limit = n > ks.SCHUR_TILE_LIMIT
    rng, rowptr, cols, diagpos, vals = schur_graph(n, n + 17, limit_tile=limit)
    if empty:
        # rows without entries (their update still divides by a diagonal: point them at some entry, as both kernels read it)
        gone = [3, 64, 65, 511, n - 1]
        rowptr, cols, vals = empty_rows(rowptr, cols, gone, vals)
        diagpos = np.array([rowptr[i] + int(np.flatnonzero(cols[rowptr[i]:rowptr[i + 1]] == i)[0]) if rowptr[i + 1] > rowptr[i] else 0
                            for i in range(n)], dtype=np.int64)
    if n >= 300:
        assert np.diff(rowptr).max() > 64, "rows longer than one 64-entry round"
    din, x, r = schur_vectors(rng, n)
    ref = [x.copy(), r.copy(), din.copy(), np.full(n, 9.0)]
    ks.call("shim_sweep_csr_f64", n, rowptr, cols, vals, diagpos, C1, C2, ref[2], ref[3], ref[0], ref[1])
    for tr in (32, 64, 128, 256):
        uptr, ulist, ploc, max_nu = ks.build_tiles(rowptr, cols, tr, ks.SCHUR_TILE_LIMIT)
        if limit and tr == 256:
            assert max_nu == ks.SCHUR_TILE_LIMIT
        xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.full(n, 9.0)
        ks.call("shim_sweep_schur_tiled_f64", tr, n, max_nu, rowptr, vals, ploc, uptr, ulist, diagpos, C1, C2, ds, do, xs, rs)
        name = f"sweep_schur_tiled_f64<{tr}> n={n}"
        same_bits(do, ref[3], f"{name}: d_out")
        same_bits(xs, ref[0], f"{name}: x")
        same_bits(rs, ref[1], f"{name}: r")
        same_bits(ds, din, f"{name}: d_in untouched")


# ---- fluid velocity block (NV = 3) and displacement block (NV = 1) -----------------------------------------------------------
def node_case(N2, seed, limit_tile=False, empty=False):
    rowptr, cols = node_graph(N2, seed, limit_tile=limit_tile)
    if N2 >= 1000:      # rows past the four prefetched 16-pair strips: 65 (one pair into the tail loop), 80 and 130 pairs
        rowptr, cols = long_rows(rowptr, cols, [N2 - 300], 65)
        rowptr, cols = long_rows(rowptr, cols, [N2 - 200], 80)
        rowptr, cols = long_rows(rowptr, cols, [N2 - 100], 130)
    if empty:
        rowptr, cols = empty_rows(rowptr, cols, [1, 2, N2 // 2, N2 - 2])
    return rowptr, cols


def run_new(nv, tn, N2, max_nu, rowptr, vals, ploc, rec, uptr, ulist, flag, dv, ds, do, xs, rs):
    if nv == 1:
        ks.call("shim_sweep_tiled_a1", tn, N2, max_nu, rowptr, vals, ploc, uptr, ulist, flag, dv, C1, C2, ds, do, xs, rs)
    else:
        ks.call("shim_sweep_tiled_r3", tn, N2, max_nu, rowptr, rec, uptr, ulist, flag, dv, C1, C2, ds, do, xs, rs)


@pytest.mark.parametrize("N2,empty", [(37, False), (1100, False), (1000, False), (1100, True)])
@pytest.mark.parametrize("nv", [1, 3])
def test_tiled_records_are_the_f32_sweep(N2, empty, nv):
    rowptr, cols = node_case(N2, 5 * N2 + nv, empty=empty)
    if N2 >= 1000:
        assert np.diff(rowptr).max() > 64, "rows longer than the four prefetched 16-pair strips"
    rng, din, x, r, dinv, rowflag = node_inputs(N2, N2 + 3 * nv, nv, flag_frac=0.15)
    vals = rng.uniform(-1, 1, nv * len(cols)).astype(np.float32)
    vals[rng.integers(0, len(vals), 7)] = -0.0
    for tn in (128, 256):
        uptr, ulist, ploc, max_nu = ks.build_tiles(rowptr, cols, tn, ks.TILE_LIMIT)
        rec = fr.pack_f3(vals, ploc) if nv == 3 else None
        for flag, dv in ((rowflag, dinv), (None, None), (rowflag, None)):
            ref = [x.copy(), r.copy(), din.copy(), np.full((N2, 4), 9.0, dtype=np.float32)]
            ks.call("shim_sweep_tiled_f32", nv, tn, N2, max_nu, rowptr, vals, ploc, uptr, ulist, flag, dv, C1, C2,
                    ref[2], ref[3], ref[0], ref[1])
            xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.full((N2, 4), 9.0, dtype=np.float32)
            run_new(nv, tn, N2, max_nu, rowptr, vals, ploc, rec, uptr, ulist, flag, dv, ds, do, xs, rs)
            name = f"sweep_tiled_{'a1' if nv == 1 else 'r3'}<{tn}> N2={N2} rowflag={flag is not None} dinv={dv is not None}"
            same_bits(do, ref[3], f"{name}: d_out")
            same_bits(xs, ref[0], f"{name}: x")
            same_bits(rs, ref[1], f"{name}: r")
            same_bits(ds, din, f"{name}: d_in untouched")


@pytest.mark.parametrize("nv", [1, 3])
def test_tiled_records_at_the_lds_limit(nv):
    N2 = ks.TILE_LIMIT + 700
    rowptr, cols = node_case(N2, 11 + nv, limit_tile=True)
    rng, din, x, r, dinv, rowflag = node_inputs(N2, 12 + nv, nv)
    vals = rng.uniform(-1, 1, nv * len(cols)).astype(np.float32)
    uptr, ulist, ploc, max_nu = ks.build_tiles(rowptr, cols, 256, ks.TILE_LIMIT)
    assert max_nu == ks.TILE_LIMIT
    rec = fr.pack_f3(vals, ploc) if nv == 3 else None
    ref = [x.copy(), r.copy(), din.copy(), np.zeros((N2, 4), dtype=np.float32)]
    ks.call("shim_sweep_tiled_f32", nv, 256, N2, max_nu, rowptr, vals, ploc, uptr, ulist, rowflag, dinv, C1, C2, ref[2], ref[3],
            ref[0], ref[1])
    xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.zeros((N2, 4), dtype=np.float32)
    run_new(nv, 256, N2, max_nu, rowptr, vals, ploc, rec, uptr, ulist, rowflag, dinv, ds, do, xs, rs)
    for got, want, what in ((do, ref[3], "d_out"), (xs, ref[0], "x"), (rs, ref[1], "r")):
        same_bits(got, want, f"sweep_tiled nv={nv}<256> at {max_nu} distinct neighbours: {what}")


# ---- solid block, fine level ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nS,empty", [(1, False), (17, False), (1000, False), (1000, True)])
def test_solid_records_are_the_b3_sweep(nS, empty):
    rng, sb_ptr, sb_col, vals, binv = solid_inputs(nS, 3 * nS + 1)
    if empty:
        sb_ptr, sb_col, vals = empty_rows(sb_ptr, sb_col, [2, 500, nS - 3], vals)
    if nS > 17:
        assert np.diff(sb_ptr).max() > 32, "rows longer than one round of two 16-block strips"
    din, x, r = vec4(rng, nS).ravel(), vec4(rng, nS).ravel(), vec4(rng, nS, 3.0).ravel()
    x[3::4], r[3::4] = 2.5, -1.5
    rec = fr.pack_sb_f32(vals, sb_col)
    ref = [x.copy(), r.copy(), din.copy(), np.full(4 * nS, 9.0, dtype=np.float32)]
    ks.call("shim_sweep_sb_b3", nS, sb_ptr, sb_col, vals, binv, C1, C2, ref[2], ref[3], ref[0], ref[1], 0)
    xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.full(4 * nS, 9.0, dtype=np.float32)
    ks.call("shim_sweep_sb_r", nS, sb_ptr, rec, binv, C1, C2, ds, do, xs, rs)
    for got, want, what in ((do, ref[3], "d_out"), (xs, ref[0], "x"), (rs, ref[1], "r"), (ds, din, "d_in untouched")):
        same_bits(got, want, f"sweep_sb_r nS={nS}: {what}")


# ---- the library's packing against the restatement ------------------------------------------------------------------------------
def test_fp32_packing_matches_the_restatement():
    rng = np.random.default_rng(9)
    n = 4099
    v = rng.standard_normal(9 * n).astype(np.float32)
    v[:4] = (0.0, -0.0, np.inf, 1e-45)
    loc = rng.integers(0, 65536, n).astype(np.uint16)
    rec3 = np.zeros(4 * n, dtype=np.uint32)
    ks.call("shim_pack_f3", n, v[:3 * n], loc, rec3)
    np.testing.assert_array_equal(rec3, fr.pack_f3(v[:3 * n], loc))
    col = rng.integers(0, 2**31 - 1, n).astype(np.int32)
    recs = np.zeros(10 * n, dtype=np.uint32)
    ks.call("shim_pack_sb_f32", n, v, col, recs)
    np.testing.assert_array_equal(recs, fr.pack_sb_f32(v, col))


# ---- a live context in the FP64-storage configuration ------------------------------------------------------------------------------
FP64_STORAGE_ENV = {"FSI_KRYLOV_FP32": "0", "FSI_OPERATOR_FP32": "0", "FSI_SCHUR_FP32": "0", "FSI_SWEEPS_FP16": "0"}


@pytest.fixture(scope="module")
def fp64_ctx(stenosis_case):
    from vasp_amd.capi import HipBackend
    from test_gpu_parity import boundary_data, random_state
    case = stenosis_case
    ns, desc = case[0], case[1]
    with pytest.MonkeyPatch.context() as mp:
        for k, v in FP64_STORAGE_ENV.items():
            mp.setenv(k, v)
        hb = HipBackend(desc, tuning=dict(tiles=1, tile_nodes=256, fused_sweeps=1, scalar_dd=1, sweeps_fp32=1, sweeps_fp16=0,
                                          solid_fp32=1, solid_fused=1, schur_fp32=0, schur_tile_rows=64))
        g, P = boundary_data(case, 1e-3)
        U, U1 = random_state(ns["mesh"], hb.ndof, seed=3)
        hb.set_state("n", U)
        hb.set_state("n-1", U1)
        hb.set_dirichlet_values(g)
        hb.set_interface_pressure(P)
        hb.assemble_residual()
        hb.assemble_jacobian()
        hb.apply_preconditioner(np.random.default_rng(0).standard_normal(hb.ndof))      # forces the preconditioner's refresh
    yield hb
    hb.close()


def test_live_fp64_context_records(fp64_ctx):
    hb = fp64_ctx
    info = ks.ctx_info(hb.ctx)
    A = lambda name: ks.ctx_array(hb.ctx, name)      # noqa: E731
    N2, V = info["N2"], info["V"]
    assert info["tiled"] and info["schur_tiled"] and not info["sweeps_fp16"], info
    nadj_ptr, nadj, ploc = A("nadj_ptr"), A("nadj"), A("tile_ploc")
    np_ = int(nadj_ptr[N2])
    chat, vv = A("dd_chat"), A("vv_db32")
    assert np.isfinite(chat).all() and np.isfinite(vv).all()
    assert len(chat) == np_ and len(vv) == 3 * np_ and len(ploc) == np_
    np.testing.assert_array_equal(A("vv_rec32").view(np.uint32), fr.pack_f3(vv, ploc))
    nb = info["sb_nblocks"]
    assert info["nS"] > 0 and nb > 0
    sb_vals, sb_col = A("sb_vals"), A("sb_col")
    np.testing.assert_array_equal(A("sb_rec32").view(np.uint32)[:10 * nb], fr.pack_sb_f32(sb_vals[:9 * nb], sb_col[:nb]))
    assert len(A("vv_rec")) == 0 and len(A("dd_rec")) == 0, "FP16 records in the FP64-storage mode"

    # one sweep of each new kernel on the context's own structure, against the kernel it replaces
    rng = np.random.default_rng(4)
    s_rowptr, s_cols, s_vals, s_diag = A("s_rowptr"), A("s_cols"), A("s_vals"), A("s_diagpos")
    suptr, sulist, sploc = A("s_tile_uptr"), A("s_tile_ulist"), A("s_ploc")
    din, x, r = schur_vectors(rng, V)
    ref = [x.copy(), r.copy(), din.copy(), np.zeros(V)]
    ks.call("shim_sweep_csr_f64", V, s_rowptr, s_cols, s_vals, s_diag, C1, C2, ref[2], ref[3], ref[0], ref[1])
    xs, rs, ds, do = x.copy(), r.copy(), din.copy(), np.zeros(V)
    ks.call("shim_sweep_schur_tiled_f64", info["schur_tile"], V, info["s_tile_max_nu"], s_rowptr, s_vals, sploc, suptr, sulist,
            s_diag, C1, C2, ds, do, xs, rs)
    for got, want, what in ((do, ref[3], "d_out"), (xs, ref[0], "x"), (rs, ref[1], "r")):
        same_bits(got, want, f"live sweep_schur_tiled_f64: {what}")
    uptr, ulist = A("tile_uptr"), A("tile_ulist")
    rowflag = A("dd_rowflag")
    for nv, vals, rec, flag in ((1, chat, None, rowflag), (3, vv, A("vv_rec32").view(np.uint32), None)):
        d4, x4, r4 = vec4(rng, N2), vec4(rng, N2), vec4(rng, N2)
        ref = [x4.copy(), r4.copy(), d4.copy(), np.zeros((N2, 4), dtype=np.float32)]
        ks.call("shim_sweep_tiled_f32", nv, info["tile_nodes"], N2, info["tile_max_nu"], nadj_ptr, vals, ploc, uptr, ulist, flag,
                None, C1, C2, ref[2], ref[3], ref[0], ref[1])
        xs, rs, ds, do = x4.copy(), r4.copy(), d4.copy(), np.zeros((N2, 4), dtype=np.float32)
        run_new(nv, info["tile_nodes"], N2, info["tile_max_nu"], nadj_ptr, vals, ploc, rec, uptr, ulist, flag, None, ds, do, xs, rs)
        for got, want, what in ((do, ref[3], "d_out"), (xs, ref[0], "x"), (rs, ref[1], "r")):
            same_bits(got, want, f"live sweep_tiled nv={nv}: {what}")
    nS = info["nS"]
    sb_ptr, binv = A("sb_ptr"), A("sb_binv12")
    d4, y4, q4 = vec4(rng, nS).ravel(), vec4(rng, nS).ravel(), vec4(rng, nS).ravel()
    ref = [y4.copy(), q4.copy(), d4.copy(), np.zeros(4 * nS, dtype=np.float32)]
    ks.call("shim_sweep_sb_b3", nS, sb_ptr, sb_col, sb_vals, binv, C1, C2, ref[2], ref[3], ref[0], ref[1], 0)
    xs, rs, ds, do = y4.copy(), q4.copy(), d4.copy(), np.zeros(4 * nS, dtype=np.float32)
    ks.call("shim_sweep_sb_r", nS, sb_ptr, A("sb_rec32").view(np.uint32), binv, C1, C2, ds, do, xs, rs)
    for got, want, what in ((do, ref[3], "d_out"), (xs, ref[0], "x"), (rs, ref[1], "r")):
        same_bits(got, want, f"live sweep_sb_r: {what}")
