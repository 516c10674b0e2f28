"""ctypes loader of ``vasp_amd/libfsi_kernel_shim.so`` (vasp_amd/csrc/fsi_kernel_shim.hip) and the host-side reference builders
of the kernel tests (tests/test_gpu_gcr_kernels.py, tests/test_gpu_sweep_kernels.py, tests/test_gpu_product_kernels.py,
tests/test_gpu_coarse_kernels.py, tests/test_gpu_bcr_kernels.py, tests/test_gpu_block_kernels.py, tests/test_gpu_ilu_kernels.py,
tests/test_gpu_vector_kernels.py, tests/test_gpu_element_kernels.py, tests/test_gpu_element_jacobian.py,
tests/test_gpu_post_cell_kernels.py).  Helper modules beside
this one: tests/fp32_records.py, tests/chain_consumers.py, tests/block_apply.py - one whole application of the block
preconditioner restated stage by stage (tests/test_block_apply_reference.py on the CPU, tests/test_gpu_block_application.py) - and
tests/post_cells.py: the wall shear stress, hemodynamic sums and indices, solid stress / strain and principal values of
fsi_post.hip, fsi_hemo.hip and fsi_stress.hip restated per cell in np.longdouble, with their bounds (shim_wss, shim_hemo_sample,
shim_hemo_finish, shim_spec_wss_sample, shim_stress_strain, shim_stress_sample, shim_stress_average, shim_tensor_sample,
shim_tensor_principal; tests/test_post_cell_references.py on the CPU, tests/test_gpu_post_cell_kernels.py), and
tests/gcr_solve.py: the properties of a recycled GCR solve and of its kept store, and a host twin of the solve (ctx_krylov_info,
ctx_krylov_columns, ctx_solve_gcr, ctx_precondition here; tests/test_gcr_solve_reference.py on the CPU,
tests/test_gpu_gcr_solve.py).

The shim runs ONE ``fsi::launch_*`` call of libvaspfsi.so on host arrays; the builders restate, in numpy, what the library's
host code hands those kernels: the LDS tiles of a graph (fsi_setup.hip build_tiles, node tiles and Schur tiles), the FP16 records of
k_pack_h1 / k_pack_h3 / k_pack_sb, the monolithic matrix's column layout, padded FP32 copy and d-row pair form, and the P2 -> P1
hierarchy of the two coarse levels with the contracts of their kernels, and the exact coarse solve by block cyclic reduction
(fsi_bcr.hip: the reduction restated on a block-tridiagonal matrix, its blocked Gauss-Jordan inverse, synthetic tube graphs whose
breadth-first levels are known), and for the multicolour ILU(0) path matrices that obey the contract of its level kernels, the
definition of ILU(0) as a check of a given factor and the triangular solves' own equations, each with its rounding bound, and for
the element kernels of fsi_assembly.hip the tables fsi_setup.hip hands them (element_structure), cell lists with materials and
states (ElementCase), the project's oracle in extended precision as the reference of element vectors and matrices with the
bound per block of a cell (K_RESIDUAL, K_JACOBIAN: four times what the oracle's own FP64 evaluation orders reach), and
restatements of the geometry, the L2 integrand, the cell statistics and the probe interpolation in np.longdouble, and the host
side of the recycled GCR (fsi_gcr_host.hpp: the store's slots, the coefficient algebra of a cycle, the policies).  The
builders are tested on the CPU (tests/test_kernel_references.py), so that a failure
of a GPU test is one of the kernel, not of its reference."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from vasp_amd import capi

LIB_PATH = Path(capi.__file__).resolve().parent / "libfsi_kernel_shim.so"

# argument codes: p pointer (numpy array or None), i int32, l int64, f float, d double, s C string
_SIGS = {
    "shim_gcr_dots": "ipllipppl", "shim_gcr_axpy": "ipllippppl", "shim_gcr_update": "iplpliilppddpppl",
    "shim_gcr_flush_width": "i", "shim_gcr_flush": "plilipppip", "shim_dot": "pplp", "shim_hashed_sum": "pllllp",
    "shim_spmv_sc_f32": "lpppppp", "shim_sweep_sc_f32": "lppppffpppp", "shim_spmv_db_f32": "lppppp",
    "shim_spmv_tiled_f32": "iilipppppppp", "shim_sweep_tiled_f32": "iilipppppppffpppp",
    "shim_sweep_tiled_h": "iilippppppffpppp",
    "shim_pack_h1": "lppp", "shim_pack_h3": "lppp", "shim_pack_sb": "lppp",
    "shim_cheb_init_f32": "lppfppp", "shim_cheb_step_f32": "lppffppp",
    "shim_spmv_sb": "lppppp", "shim_sweep_sb_b3": "lppppffppppi", "shim_sweep_sb_h": "lpppffpppp",
    "shim_cheb_init_b3": "lppfppp", "shim_cheb_step_b3": "lppffppp",
    "shim_sweep_csr_f64": "lppppddpppp", "shim_sweep_csr_mixed": "lpppppddpppp", "shim_sweep_schur_tiled": "ilipppppddpppp",
    "shim_ctx_info": "ppi", "shim_ctx_apply_info": "ppipi", "shim_ctx_array": "psppp", "shim_tile_limit": "", "shim_cheb_coefficients": "ddiippp",
    "shim_expand_cols": "llpppppppp", "shim_spmv": "lpppplpi", "shim_spmv_node6": "llpppppplppp", "shim_drows_extract": "lpppppp",
    "shim_pad_cols32": "lpppp", "shim_pad_vals32": "llppplllpli", "shim_spmv_node6p": "llppplpplppplppp",
    "shim_matrix_finish": "lppppplpp", "shim_ctx_spmv": "pippp",
    "shim_ctx_krylov_info": "ppipippp", "shim_ctx_krylov_columns": "ppppp", "shim_ctx_solve_gcr": "pppdippp",
    "shim_ctx_precondition": "ppp",
    "shim_mg_d0": "lppppppp", "shim_mg_rap": "llpppppppppppppp", "shim_mg_coarse_finish": "llppppppppp",
    "shim_mg_restrict": "llpppppppfppp", "shim_mg_prolong": "llppppp", "shim_sbmg_flags": "lpppp",
    "shim_sbmg_rap": "lllppppppppppppppp", "shim_sbmg_coarse_finish": "llpppppppp", "shim_sbmg_restrict": "lllpppppppppppl",
    "shim_sbmg_prolong": "llpppppppl", "shim_sb_binv": "llppplpp", "shim_sb_dinv": "llppplp", "shim_dinv_f32": "lppplp",
    "shim_diag_inverse": "lpplp", "shim_block_scale_d": "lpp", "shim_solid_cycle_init": "llpppfpppp", "shim_gather3_f32": "llppp",
    "shim_scatter3_f32": "llppp",
    "shim_bcr_invert": "lpplplp", "shim_bcr_gemm": "lppplplp", "shim_bcr_apply": "ilpplppl", "shim_bcr_fill": "lpppdpl",
    "shim_bcr_gather": "lpppl", "shim_bcr_scatter": "lpplp", "shim_bcr_run": "lppipdipppppppplpl",
    "shim_tail": "", "shim_block_structure": "llpppppppppppp", "shim_extract_blocks": "lldppppppppppppppppp",
    "shim_extract_db": "lpppppi", "shim_extract_chat": "lpppppp", "shim_db_rowmask": "lppp", "shim_mask_outside": "lppp",
    "shim_to_f32": "lpp", "shim_gather_vals": "lpplp", "shim_sb_gather": "llpppplp", "shim_schur_full": "llppppppppppppppppp",
    "shim_pres_rhs32": "llpppppppp", "shim_vel_correct32": "llppppppp", "shim_vel_correct": "lpppplpplppp",
    "shim_pres_rows": "lppppdppppldpdp", "shim_cheb_init": "lppppldppp",
    "shim_cheb_step": "lpppplddppp", "shim_db_rows_sub": "llppppppp", "shim_spmv_db": "lpppppp",
    "shim_residual_csr": "lpppplpp", "shim_residual_rows": "lppppplplppl", "shim_split": "llpppp", "shim_merge": "llpppp",
    "shim_merge_f32d": "llpppp", "shim_pad_init_f32": "lpppfppp", "shim_pad_to_f32": "lppp", "shim_unpad_from_f32": "lpp",
    "shim_mask_ripple": "lpp", "shim_mask_scale": "lppplp",
    "shim_ilu0": "lipppppppp", "shim_sptrsv": "lipppppppppp", "shim_ctx_levels": "ppi",
    "shim_fill": "ldp", "shim_copy": "lpp", "shim_axpy": "ldpp", "shim_axpby": "ldpdpp", "shim_scale": "ldp", "shim_mul": "lppp",
    "shim_div": "lppp", "shim_negate": "lpp", "shim_gather": "lplpp", "shim_scatter": "lpppl", "shim_gather3": "llppp",
    "shim_scatter3": "llppp", "shim_round_to_f32": "lpp", "shim_add_indexed": "lppdpl", "shim_add_at": "lppdpl",
    "shim_bc_rhs": "lppppl", "shim_bc_set": "lpppl", "shim_robin_residual": "lppppddpppl", "shim_f32_ripple4": "lp",
    "shim_f32_sumsq": "lpp",
    "shim_geometry": "llppp", "shim_elem_residual": "lll" + "p" * 10 + "ll" + "p" * 6,
    "shim_elem_jacobian": "iiilll" + "p" * 14 + "ippp", "shim_l2norm": "llpppp", "shim_stat_parts": "",
    "shim_cell_stats": "lllppppp", "shim_probe": "lllppppp",
    "shim_gcr_store_op": "ilppppp", "shim_gcr_sizes": "lip", "shim_gcr_cycle_algebra": "lipppppppip",
    "shim_gcr_cycle_end": "iidddi", "shim_gcr_orth_lost": "piddd", "shim_gcr_verdict_due": "dddiiiiiii",
    "shim_gcr_verdict_skippable": "dddiiiiiiidd", "shim_gcr_tolerances": "pp", "shim_room_refusal": "ssdsldpl",
    "shim_wss": "lllpppppdp", "shim_hemo_sample": "lllpppppp" + "ldd" + "p" * 7, "shim_hemo_finish": "ldpppp",
    "shim_spec_wss_sample": "lll" + "p" * 7 + "ldp", "shim_stress_strain": "lll" + "p" * 12, "shim_stress_sample": "lll" + "p" * 13,
    "shim_stress_average": "ldpp", "shim_tensor_sample": "llli" + "p" * 12, "shim_tensor_principal": "lpp",
}
LAUNCH_REFUSED = 2           # fsi_kernels.hpp: a launch function refused its arguments and launched nothing
_CT = {"p": C.c_void_p, "i": C.c_int32, "l": C.c_int64, "f": C.c_float, "d": C.c_double, "s": C.c_char_p}
_lib = None


def load():
    """libvaspfsi.so first (the shim resolves it next to itself), then the shim.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        capi.load_library()
        if not LIB_PATH.exists():
            raise RuntimeError(f"{LIB_PATH} not found: make -C vasp_amd/csrc builds it")
        lib = C.CDLL(str(LIB_PATH))
        for name, sig in _SIGS.items():
            fn = getattr(lib, name)
            fn.argtypes = [_CT[c] for c in sig]
            fn.restype = C.c_int
        lib.shim_last_error.restype = C.c_char_p
        lib.shim_ctx_ktheta.argtypes = [C.c_void_p]
        lib.shim_ctx_ktheta.restype = C.c_double
        lib.shim_ctx_coarse.argtypes = [C.c_void_p, C.c_int32]
        lib.shim_ctx_coarse.restype = C.c_double
        _lib = lib
    return _lib


def _arg(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags.c_contiguous, "shim arguments must be contiguous"
        return a.ctypes.data_as(C.c_void_p)
    return a


def status(name, *args):
    """Run one shim entry point and return its status (0 ok, else see fsi_kernel_shim.hip); arrays as in call()."""
    return getattr(load(), name)(*[_arg(a) for a in args])


def call(name, *args):
    """Run one shim entry point; numpy arrays are passed by pointer (outputs are written in place)."""
    rc = status(name, *args)
    if rc != 0:
        raise RuntimeError(f"{name}: {load().shim_last_error().decode()}")
    return rc


def check(got, ref, bound, what):
    """|got - ref| <= bound entry by entry (NaN fails), with the first offender in the message"""
    got, ref, bound = (np.asarray(a, dtype=np.float64).ravel() for a in (got, ref, bound))
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {bad.sum()} of {len(got)} outside the bound; first at {i}: got {got[i]!r}, "
                             f"reference {ref[i]!r}, error {err[i]:.3e} > bound {bound[i]:.3e}")


CTX_INFO = ("N2", "V", "nS", "sb_nblocks", "tiled", "tile_nodes", "tile_max_nu", "schur_tiled", "schur_tile", "s_tile_max_nu",
            "sweeps_fp16", "a32_ptail", "a32_tail_src", "a32_tail_nnz", "op32_ok", "kry_fp32", "drows_ok",
            "mg_nc", "mg_cnnz", "mg_ready", "sbmg_nc", "sbmg_nblk", "sbmg_ready", "bcr_ready", "product_form64", "product_form32")
_ELEM = {("f", 4): np.float32, ("f", 8): np.float64, ("i", 1): np.uint8, ("i", 2): np.uint16, ("i", 4): np.int32,
         ("i", 8): np.int64}
_UNSIGNED = {"dd_rec", "vv_rec", "sb_rec", "s_rec"}
_FLOAT = {"dd_chat", "vv_db32", "sb_vals", "sb_binv12", "s_vals", "s_vals32", "s_dinv", "dd_db", "rowscale", "A", "A32", "Ad64", "Ad32", "drows_dd", "drows_dv",
          "mg_pw", "mg_chw", "mg_Ac", "mg_cc", "mg_d0", "mg_dcinv4", "sbmg_pw", "sbmg_chw", "sbmg_cvals", "sbmg_cbinv12",
          "sb_binv9", "sb_dinv", "dd_dinv32", "vvf_dinv32", "Mdd.vals", "Mvv.vals", "Adv", "Avp", "Apv", "App", "Avp32", "Apv32",
          "vv_db", "adv_db", "dd_db32", "vv_dinv", "mask_f", "mask_s", "ss_vals", "LU", "blk", "sbmg_work", "mg_work", "ones32", "mg_cones", "bs"}


def ctx_info(ctx) -> dict:
    lib = load()
    out = np.zeros(len(CTX_INFO), dtype=np.int64)
    lib.shim_ctx_info(ctx, _arg(out), len(CTX_INFO))
    return dict(zip(CTX_INFO, (int(v) for v in out)))


def ctx_spmv(ctx, working, x, y):
    """fsi::host::spmv on the context's solver-ordered vectors (y written in place); returns (status, op32_products added,
    drows_products added)"""
    cnt = np.zeros(2, dtype=np.int64)
    rc = status("shim_ctx_spmv", ctx, int(working), x, y, cnt)
    return rc, int(cnt[0]), int(cnt[1])


KRYLOV_INFO = ("cap", "hw", "made", "nfree", "kry_fp32", "kry_fp32_policy", "ldq", "ldz", "hot_next", "window_cols", "gcr_restarts",
               "kry_fp32_failures_total", "gcr_reorth_forced", "gcr_arnoldi_steps", "verdicts_skipped", "gcr_stagnated", "gcr_stalled",
               "f64_suspect", "ndof")
KRYLOV_INFO_D = ("f32_last_drift", "gcr_escape")


def ctx_krylov_info(ctx) -> dict:
    """the store and the counters of a live context's recycled GCR (shim_ctx_krylov_info): the KRYLOV_INFO fields as ints, the
    KRYLOV_INFO_D fields as floats, born [cap], free (the free list, in its order) and hot_slots [GCR_WINDOW] as int lists"""
    lib = load()
    iout, dout = np.zeros(len(KRYLOV_INFO), dtype=np.int64), np.zeros(len(KRYLOV_INFO_D))
    lib.shim_ctx_krylov_info(ctx, _arg(iout), len(iout), _arg(dout), len(dout), None, None, None)
    cap = int(iout[0])
    born, free, hot = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int32), np.zeros(32, dtype=np.int32)
    k = lib.shim_ctx_krylov_info(ctx, _arg(iout), len(iout), _arg(dout), len(dout), _arg(born), _arg(free), _arg(hot))
    assert k == len(KRYLOV_INFO), (k, len(KRYLOV_INFO))
    info = dict(zip(KRYLOV_INFO, (int(v) for v in iout)))
    info.update(zip(KRYLOV_INFO_D, (float(v) for v in dout)))
    info.update(born=[int(v) for v in born], free=[int(v) for v in free[:info["nfree"]]], hot_slots=[int(v) for v in hot])
    return info


def ctx_krylov_columns(ctx, info=None):
    """(Q [hw][ldq] float32 or float64 as the store holds it, Z [hw][ldz], Qh [GCR_WINDOW][ldq]) of a live context, padding rows
    included.  Qh is NaN throughout where the context has no window."""
    info = ctx_krylov_info(ctx) if info is None else info
    hw, ldq, ldz = info["hw"], info["ldq"], info["ldz"]
    sz = C.c_int32(0)
    call("shim_ctx_krylov_columns", ctx, None, None, None, C.byref(sz))
    assert sz.value == (4 if info["kry_fp32"] else 8), (sz.value, info["kry_fp32"])
    Q = np.zeros((hw, ldq), dtype=np.float32 if sz.value == 4 else np.float64)
    Z = np.zeros((hw, ldz))
    Qh = np.full((32, ldq), np.nan)
    call("shim_ctx_krylov_columns", ctx, Q, Z, Qh, C.byref(sz))
    return Q, Z, Qh


def ctx_solve_gcr(ctx, rhs, rtol, max_it=4000, fill=-7.25):
    """fsi::host::solve_gcr on the equilibrated system in solver ordering: (status, message, x [ndof + TAIL] whose tail started as
    `fill`, iterations, relres, monolithic products launched)"""
    n = len(rhs)
    x = np.full(n + TAIL, fill)
    it, rr, cnt = C.c_int32(0), C.c_double(0.0), np.zeros(1, dtype=np.int64)
    rc = status("shim_ctx_solve_gcr", ctx, np.ascontiguousarray(rhs, dtype=np.float64), x, float(rtol), int(max_it), C.byref(it),
                C.byref(rr), cnt)
    return rc, (load().shim_last_error().decode() if rc else ""), x, it.value, rr.value, int(cnt[0])


def ctx_precondition(ctx, r, fill=-7.25):
    """z = M^-1 r of the context's active preconditioner in solver ordering (fsi::host::precondition)"""
    z = np.full(len(r) + TAIL, fill)
    call("shim_ctx_precondition", ctx, np.ascontiguousarray(r, dtype=np.float64), z)
    assert np.all(z[len(r):] == fill), "precondition wrote behind z"
    return z[:len(r)].copy()


def ctx_ktheta(ctx) -> float:
    return float(load().shim_ctx_ktheta(ctx))


COARSE = ("mg_gersh", "sbmg_gersh", "mg_clmax", "sbmg_clmax", "lmax_s", "lmax_f", "lmax_p", "lmax_d", "cheb_kappa_s", "cheb_kappa_f",
          "cheb_kappa_p", "cheb_kappa_d", "dd_is_db", "adv_is_db", "dd_is_scalar", "adv_solid_only", "pv32_ok")


def ctx_coarse(ctx) -> dict:
    """the coarse levels' row-sum bounds (of the last rebuild) and the largest eigenvalues their Chebyshev intervals use"""
    lib = load()
    return {name: float(lib.shim_ctx_coarse(ctx, k)) for k, name in enumerate(COARSE)}


def ctx_array(ctx, name: str) -> np.ndarray:
    """Copy of a device array a live FsiCtx owns (the names of shim_ctx_array)."""
    lib = load()
    n, sz = C.c_int64(0), C.c_int32(0)
    if lib.shim_ctx_array(ctx, name.encode(), None, C.byref(n), C.byref(sz)) != 0:
        raise RuntimeError(lib.shim_last_error().decode())
    dt = _ELEM[("f" if name in _FLOAT else "i", sz.value)]
    if name in _UNSIGNED:
        dt = np.uint32
    out = np.zeros(n.value, dtype=dt)
    if lib.shim_ctx_array(ctx, name.encode(), _arg(out), C.byref(n), C.byref(sz)) != 0:
        raise RuntimeError(lib.shim_last_error().decode())
    return out


# ---- reference builders ------------------------------------------------------------------------------------------------------
TILE_LIMIT = 3584            # fsi_block.hip TILE_LIMIT: distinct neighbour nodes of a node tile (tile_limit(); checked on the GPU)
SCHUR_TILE_LIMIT = 7000      # fsi_setup.hip: distinct columns of a Schur tile (56 KB of LDS as doubles)


def build_tiles(rowptr, cols, rows_per_tile, limit):
    """Tiles of consecutive rows as fsi_setup.hip builds them: per tile the sorted distinct columns of its rows (ulist, tile t at
    uptr[t] .. uptr[t + 1]) and per entry the column's index in its tile's list (ploc).  Returns (uptr, ulist, ploc, max_nu), or
    None when a tile has more than `limit` distinct columns (the library then does not use the tiled kernels)."""
    n = len(rowptr) - 1
    nt = (n + rows_per_tile - 1) // rows_per_tile
    uptr = np.zeros(nt + 1, dtype=np.int64)
    ploc = np.zeros(len(cols), dtype=np.uint16)
    lists = []
    for t in range(nt):
        e0, e1 = rowptr[t * rows_per_tile], rowptr[min(n, (t + 1) * rows_per_tile)]
        u = np.unique(cols[e0:e1])
        if len(u) > limit:
            return None
        ploc[e0:e1] = np.searchsorted(u, cols[e0:e1])
        lists.append(u)
        uptr[t + 1] = uptr[t] + len(u)
    ulist = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, dtype=np.int32)
    max_nu = int(np.diff(uptr).max()) if nt else 0
    return uptr, ulist, ploc, max_nu


def xcd_unit(L, n):
    """fsi_kernels.hpp xcd_unit: the unit logical workgroup L takes (-1: none)."""
    chunk = (n + 7) >> 3
    s, t = L >> 3, (L & 7) * chunk + (L >> 3)
    return t if (s < chunk and t < n) else -1


def half_bits(v):
    """FP16 bits of float32 values, round to nearest even (numpy's and the device's float -> _Float16 conversion)."""
    with np.errstate(over="ignore"):          # beyond 65504 the conversion gives inf, as on the device
        return np.asarray(v, dtype=np.float32).astype(np.float16).view(np.uint16).astype(np.uint32)


def half_value(bits):
    return (np.asarray(bits, dtype=np.uint32) & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float64)


def pack_h1(v, loc):
    """k_pack_h1: rec[e] = half(v[e]) | loc[e] << 16"""
    return (half_bits(v) | (np.asarray(loc, dtype=np.uint32) << 16)).astype(np.uint32)


def pack_h3(v, loc):
    """k_pack_h3: two words per pair, (half v0 | half v1 << 16), (half v2 | loc << 16)"""
    h = half_bits(np.asarray(v, dtype=np.float32).reshape(-1, 3))
    rec = np.empty((len(h), 2), dtype=np.uint32)
    rec[:, 0] = h[:, 0] | (h[:, 1] << 16)
    rec[:, 1] = h[:, 2] | (np.asarray(loc, dtype=np.uint32) << 16)
    return rec.reshape(-1)


def pack_sb(v, col):
    """k_pack_sb: six words per 3x3 block, (a0 a1) (a2 a3) (a4 a5) (a6 a7) (a8 0) (column)"""
    h = half_bits(np.asarray(v, dtype=np.float32).reshape(-1, 9))
    rec = np.zeros((len(h), 6), dtype=np.uint32)
    for k in range(4):
        rec[:, k] = h[:, 2 * k] | (h[:, 2 * k + 1] << 16)
    rec[:, 4] = h[:, 8]
    rec[:, 5] = np.asarray(col, dtype=np.int64).astype(np.uint32)
    return rec.reshape(-1)


def unpack_h1(rec):
    """(values in FP64, local indices) of k_pack_h1 records"""
    rec = np.asarray(rec, dtype=np.uint32)
    return half_value(rec), (rec >> 16).astype(np.int64)


def unpack_h3(rec):
    rec = np.asarray(rec, dtype=np.uint32).reshape(-1, 2)
    v = np.stack([half_value(rec[:, 0]), half_value(rec[:, 0] >> 16), half_value(rec[:, 1])], axis=1)
    return v, (rec[:, 1] >> 16).astype(np.int64)


def unpack_sb(rec):
    rec = np.asarray(rec, dtype=np.uint32).reshape(-1, 6)
    v = np.empty((len(rec), 9))
    for k in range(4):
        v[:, 2 * k] = half_value(rec[:, k])
        v[:, 2 * k + 1] = half_value(rec[:, k] >> 16)
    v[:, 8] = half_value(rec[:, 4])
    return v, rec[:, 5].astype(np.int64)


def local_graph(n, rng, reach=24, max_deg=40, diag_only=()):
    """A symmetric-pattern node graph with a diagonal entry in every row and neighbours within `reach` (tiles then see a few hundred
    distinct columns, as on a Morton-ordered mesh); rows in `diag_only` hold the diagonal alone.  Columns ascending per row."""
    rows = []
    diag_only = set(int(i) for i in diag_only)
    for i in range(n):
        if i in diag_only:
            rows.append(np.array([i]))
            continue
        k = int(rng.integers(0, max_deg))
        nb = rng.integers(max(0, i - reach), min(n, i + reach + 1), size=k)
        nb = [j for j in nb if j not in diag_only]
        rows.append(np.unique(np.concatenate([[i], np.asarray(nb, dtype=np.int64)])))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    cols = np.concatenate(rows).astype(np.int32) if n else np.zeros(0, dtype=np.int32)
    return rowptr, cols


# ---- the monolithic matrix: structure, padded FP32 copy, d rows in pair form (fsi_solver.hip, fsi_product.hip) ---------------
def mono_graph(N2, V, rng, reach=24, max_deg=12, heavy=(), heavy_deg=(), diag_only=(), no_padj=()):
    """A node graph as the monolithic layout reads it.  nadj_ptr / nadj: every node's neighbour ranks, ascending, itself included
    (up to max_deg random ones within `reach`; node heavy[k] gets heavy_deg[k] neighbours from anywhere; diag_only nodes itself
    alone).  vrank: V distinct vertex nodes, the node of pressure position q.  padj_ptr / padj: per node the pressure positions
    of its vertex neighbours, ascending (a vertex node meets itself, so its pressure row has a diagonal), except the nodes in
    no_padj, which get none (their rows have no pressure column, the pressure row of a vertex among them no diagonal)."""
    assert 0 <= V <= N2
    k = rng.integers(0, max_deg + 1, N2)
    src = np.repeat(np.arange(N2, dtype=np.int64), k)
    dst = np.clip(src + rng.integers(-reach, reach + 1, len(src)), 0, N2 - 1)
    src, dst = np.concatenate([src, np.arange(N2)]), np.concatenate([dst, np.arange(N2)])
    drop = np.isin(src, np.asarray(list(diag_only) + list(heavy), dtype=np.int64)) & (src != dst)
    src, dst = src[~drop], dst[~drop]
    for r, d in zip(heavy, heavy_deg):
        nb = rng.choice(N2, size=min(d, N2), replace=False)
        src, dst = np.concatenate([src, np.full(len(nb), r)]), np.concatenate([dst, nb])
    code = np.unique(src * N2 + dst)
    src, dst = code // N2, code % N2
    nadj_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N2))]).astype(np.int64)
    nadj = dst.astype(np.int32)
    vrank = rng.choice(N2, size=V, replace=False).astype(np.int32)
    pos = np.full(N2, -1, dtype=np.int64)
    pos[vrank] = np.arange(V)
    keep = pos[dst] >= 0
    keep &= ~np.isin(src, np.asarray(list(no_padj), dtype=np.int64))
    ps, pq = src[keep], pos[dst[keep]]
    o = np.lexsort((pq, ps))
    padj_ptr = np.concatenate([[0], np.cumsum(np.bincount(ps, minlength=N2))]).astype(np.int64)
    padj = pq[o].astype(np.int32)
    return nadj_ptr, nadj, padj_ptr, padj, vrank


def expand_cols(N2, nadj_ptr, nadj, padj_ptr, padj, vrank):
    """The k_expand_cols contract.  Rows: dof t of node r is row 6 r + t, pressure position q row 6 N2 + q.  Every row of node r
    (and the pressure row of a vertex at r) holds, for each neighbour s of r in ascending order, the columns 6 s .. 6 s + 5, then
    the columns 6 N2 + u of r's pressure neighbours u.  diagpos: the entry of column = row, -1 where the row has none.
    Returns (rowptr, cols, diagpos)."""
    V = len(vrank)
    deg, pdeg = np.diff(nadj_ptr), np.diff(padj_ptr)
    Lnode = 6 * deg + pdeg
    rank = np.concatenate([np.repeat(np.arange(N2), 6), np.asarray(vrank, dtype=np.int64)])
    L = Lnode[rank]
    rowptr = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    n = 6 * N2 + V
    # the column pattern of each node, once
    nrow = np.concatenate([np.repeat(6 * np.asarray(nadj, dtype=np.int64), 6) + np.tile(np.arange(6), len(nadj)),
                           6 * N2 + np.asarray(padj, dtype=np.int64)])
    owner = np.concatenate([np.repeat(np.repeat(np.arange(N2), deg), 6), np.repeat(np.arange(N2), pdeg)])
    o = np.argsort(owner, kind="stable")
    pattern, pptr = nrow[o], np.concatenate([[0], np.cumsum(Lnode)])
    row = np.repeat(np.arange(n), L)
    t = np.arange(rowptr[-1]) - rowptr[row]
    cols = pattern[pptr[rank[row]] + t].astype(np.int32)
    diagpos = np.full(n, -1, dtype=np.int64)
    hit = np.flatnonzero(cols == row)
    diagpos[row[hit]] = hit
    return rowptr, cols, diagpos


def pad_layout(N2, rowptr):
    """The FP32 copy's layout (fsi_setup.hip): node r's six value rows padded to Lp = L rounded up to a multiple of 4, block at
    p32[r] (entries), index row at p32[r] / 6; the pressure rows unpadded behind, at ptail.  Returns (p32, ptail, tail_src,
    nnz_tail)."""
    L = rowptr[6 * np.arange(N2) + 1] - rowptr[6 * np.arange(N2)]
    p32 = np.concatenate([[0], np.cumsum(6 * ((L + 3) & ~3))]).astype(np.int64)
    tail_src = int(rowptr[6 * N2])
    return p32, int(p32[-1]), tail_src, int(rowptr[-1]) - tail_src


def pad_copy(N2, rowptr, cols, A, v_rows_only=False):
    """What k_pad_cols32 / k_pad_vals32 (+ k_round_to_f32 on the pressure rows) write: (cols32, A32, written), the padding entries
    with column 0 and value 0, written[i] whether entry i of A32 is written (value rows 0 .. 2 are not with v_rows_only)."""
    p32, ptail, tail_src, nnz_tail = pad_layout(N2, rowptr)
    L = rowptr[6 * np.arange(N2) + 1] - rowptr[6 * np.arange(N2)]
    Lp = (L + 3) & ~3
    cols32 = np.zeros(ptail // 6, dtype=np.int32)
    A32 = np.zeros(ptail + nnz_tail, dtype=np.float32)
    written = np.ones(len(A32), dtype=bool)
    r = np.repeat(np.arange(N2), 6 * L)
    t = np.arange(tail_src) - rowptr[6 * r]
    first = t < L[r]                                                  # entries of the first row of each node
    cols32[p32[r[first]] // 6 + t[first]] = cols[:tail_src][first]
    k = t // L[r]                                                     # value row 0 .. 5 of the node's block
    tt = t - k * L[r]
    A32[p32[r] + k * Lp[r] + tt] = np.asarray(A[:tail_src], dtype=np.float32)
    A32[ptail:] = np.asarray(A[tail_src:], dtype=np.float32)
    if v_rows_only:
        blk = np.repeat(np.arange(N2), 6 * Lp)
        kk = (np.arange(ptail) - p32[blk]) // Lp[blk]
        written[:ptail] = kk >= 3
    return cols32, A32, written


def drows_entries(N2, rowptr, nadj_ptr):
    """The entries of the d rows (value rows 0 .. 2 of every node) and where the pair form keeps them: (entry, slot) with slot
    the index into the [pairs x 6] pair array or -1 where the forms leave a structural zero"""
    rows = (6 * np.arange(N2)[:, None] + np.arange(3)).ravel()
    L = rowptr[rows + 1] - rowptr[rows]
    row = np.repeat(rows, L)
    entry = np.repeat(rowptr[rows], L) + (np.arange(L.sum()) - np.repeat(np.concatenate([[0], np.cumsum(L)[:-1]]), L))
    r, i = row // 6, row % 6
    t = entry - rowptr[row]
    c = t % 6
    deg6 = 6 * (nadj_ptr[r + 1] - nadj_ptr[r])
    kept = (t < deg6) & ((c == i) | (c == i + 3))
    slot = np.where(kept, 6 * (nadj_ptr[r] + t // 6) + np.where(c == i, i, 3 + i), -1)
    return entry, slot


def drows_extract(N2, rowptr, A, nadj_ptr):
    """k_drows_extract: the d rows in pair form [dd_0 dd_1 dd_2 dv_0 dv_1 dv_2] per node pair (row (r, i) keeps, for neighbour k,
    the entries of columns d_i and v_i), and the verdict: True if any other entry of a d row is not exactly zero"""
    entry, slot = drows_entries(N2, rowptr, nadj_ptr)
    ad = np.zeros(6 * int(nadj_ptr[N2]), dtype=np.float64)
    kept = slot >= 0
    ad[slot[kept]] = A[entry[kept]]
    return ad, bool(np.any(A[entry[~kept]] != 0.0))


def drows_expand(N2, rowptr, ad, nadj_ptr, nnz):
    """The inverse of drows_extract: a length-nnz array holding the d rows the pair form stands for (zero elsewhere)"""
    entry, slot = drows_entries(N2, rowptr, nadj_ptr)
    out = np.zeros(nnz, dtype=np.float64)
    kept = slot >= 0
    out[entry[kept]] = np.asarray(ad, dtype=np.float64)[slot[kept]]
    return out


def csr_product(rowptr, cols, vals, x):
    """(y, S, L) of y = A x in extended precision: y, sum_j |a_ij x_j| and the row lengths (float64)"""
    n = len(rowptr) - 1
    p = np.asarray(vals, dtype=np.longdouble) * np.asarray(x, dtype=np.longdouble)[cols]
    y, S = np.zeros(n, dtype=np.longdouble), np.zeros(n, dtype=np.longdouble)
    L = np.diff(rowptr)
    nz = L > 0
    if p.size:
        y[nz] = np.add.reduceat(p, rowptr[:-1][nz])
        S[nz] = np.add.reduceat(np.abs(p), rowptr[:-1][nz])
    return y.astype(np.float64), S.astype(np.float64), L.astype(np.float64)


# ---- the two-level coarse levels (fsi_setup.hip build_hierarchy; fsi_block.hip k_mg_* / k_sbmg_*) and the diagonal scalings --
U32 = 2.0 ** -24
UFC_EDGES = ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1))      # local edge e of a P2 tet joins these local vertices


def edge_ends(tet_nodes, N2, V):
    """[N2][2] end vertices of every edge-midpoint node (-1 for vertices), as the library takes them: from the LAST cell in the
    order given that holds the edge, in that cell's local vertex order (so an edge's two ends may come either way round)"""
    tn = np.asarray(tet_nodes, dtype=np.int64).reshape(-1, 10)
    nd = tn[:, 4:].ravel()
    a = tn[:, [e[0] for e in UFC_EDGES]].ravel()
    b = tn[:, [e[1] for e in UFC_EDGES]].ravel()
    u, first_rev = np.unique(nd[::-1], return_index=True)
    last = len(nd) - 1 - first_rev
    ends = np.full((N2, 2), -1, dtype=np.int64)
    ends[u, 0], ends[u, 1] = a[last], b[last]
    return ends


def children(par, pw, nc):
    """(chptr, child, chw): the transpose of the parent lists, per coarse node its fine nodes in ascending order with the weights"""
    par, pw = np.asarray(par).reshape(-1, 2), np.asarray(pw, dtype=np.float32).reshape(-1, 2)
    fine = np.repeat(np.arange(len(par)), 2)
    keep = pw.ravel() != 0
    p, f, w = par.ravel()[keep].astype(np.int64), fine[keep], pw.ravel()[keep]
    o = np.argsort(p, kind="stable")                                # fine nodes stay ascending within a coarse node
    chptr = np.concatenate([[0], np.cumsum(np.bincount(p, minlength=nc))]).astype(np.int64)
    return chptr, f[o].astype(np.int32), w[o].astype(np.float32)


def _vertex_pairs(tet_nodes):
    """(i, j) of every two vertices that share a cell (itself included), unique"""
    tv = np.asarray(tet_nodes, dtype=np.int64).reshape(-1, 10)[:, :4]
    i, j = np.repeat(tv, 4, axis=1).ravel(), np.tile(tv, (1, 4)).ravel()
    code = np.unique(i * (tv.max() + 1) + j)
    return code // (tv.max() + 1), code % (tv.max() + 1)


def p1_hierarchy(tet_nodes, V, rank2node, snode=None):
    """The P2 -> P1 hierarchy fsi_setup.hip builds, restated.  tet_nodes: [cells][10] in the library's cell order, rank2node: node
    of every solver rank (node = solver2user[6 r] // 3).  Displacement level (snode None): coarse node i = the i-th vertex in rank
    order (cfine[i] its rank); par / pw [N2][2]: a vertex its own coarse node with weights (1, 0), a midpoint its edge's two ends
    (edge_ends) with (1/2, 1/2); chptr / child / chw their transpose in fine-rank order; cptr / ccol: the vertices that share a
    cell with coarse node i, ascending.  Compact solid level (snode: the ranks of the solid nodes, ascending; fine node = index
    into snode): the same on the solid nodes, cfine holding compact indices; None where an edge's end vertex is not a solid node
    (the library then switches the level off)."""
    rank2node = np.asarray(rank2node, dtype=np.int64)
    N2 = len(rank2node)
    rk = np.empty(N2, dtype=np.int64)
    rk[rank2node] = np.arange(N2)
    ends = edge_ends(tet_nodes, N2, V)
    pi, pj = _vertex_pairs(tet_nodes)
    if snode is None:
        fine_rank = np.arange(N2)
    else:
        fine_rank = np.asarray(snode, dtype=np.int64)
    nf = len(fine_rank)
    fidx = np.full(N2, -1, dtype=np.int64)                           # rank -> fine index
    fidx[fine_rank] = np.arange(nf)
    is_v = rank2node[fine_rank] < V
    cfine = np.flatnonzero(is_v)
    cidx = np.full(nf, -1, dtype=np.int64)
    cidx[cfine] = np.arange(len(cfine))
    nc = len(cfine)
    par = np.zeros((nf, 2), dtype=np.int64)
    pw = np.zeros((nf, 2), dtype=np.float32)
    par[cfine, 0] = par[cfine, 1] = cidx[cfine]
    pw[cfine, 0] = 1.0
    mid = np.flatnonzero(~is_v)
    e = ends[rank2node[fine_rank[mid]]]
    assert (e >= 0).all() and (e < V).all(), "a midpoint without its edge"
    fe = fidx[rk[e]]
    if (fe < 0).any():
        return None
    par[mid] = cidx[fe]
    pw[mid] = 0.5
    chptr, child, chw = children(par, pw, nc)
    # coarse pattern: vertex pairs sharing a cell, both coarse nodes of this level; ascending in rank = ascending in coarse index
    ci = np.where(fidx[rk[pi]] >= 0, cidx[np.maximum(fidx[rk[pi]], 0)], -1)
    cj = np.where(fidx[rk[pj]] >= 0, cidx[np.maximum(fidx[rk[pj]], 0)], -1)
    keep = (ci >= 0) & (cj >= 0)
    code = np.unique(ci[keep] * nc + cj[keep])
    cptr = np.concatenate([[0], np.cumsum(np.bincount(code // nc, minlength=nc))]).astype(np.int64)
    return dict(nc=nc, par=par.ravel().astype(np.int32), pw=pw.ravel(), chptr=chptr, child=child, chw=chw, cptr=cptr,
                ccol=(code % nc).astype(np.int32), cfine=cfine.astype(np.int32))


def prolongation(par, pw, nc):
    """P as scipy CSR [fine x coarse]: P[a, par[a][k]] = pw[a][k]"""
    import scipy.sparse as sp
    par, pw = np.asarray(par, dtype=np.int64).reshape(-1, 2), np.asarray(pw, dtype=np.float64).reshape(-1, 2)
    n = len(par)
    return sp.csr_matrix((pw.ravel(), (np.repeat(np.arange(n), 2), par.ravel())), shape=(n, nc))


def galerkin(P, A0, free):
    """P^T A0_free P, A0_free = A0 with the rows and columns of the non-free (Dirichlet / identity) fine nodes removed"""
    import scipy.sparse as sp
    Df = sp.diags(np.asarray(free, dtype=np.float64))
    return (P.T @ (Df @ A0 @ Df) @ P).tocsr()


def _coarse_lookup(cptr, ccol, nc, i, j):
    """entry of column j in coarse row i (the last such entry), -1 where the row has none"""
    row = np.repeat(np.arange(nc), np.diff(cptr))
    key = row * np.int64(nc) + np.asarray(ccol, dtype=np.int64)
    o = np.argsort(key, kind="stable")
    ks_ = key[o]
    q = np.asarray(i, dtype=np.int64) * nc + np.asarray(j, dtype=np.int64)
    pos = np.searchsorted(ks_, q, side="right") - 1
    ok = (pos >= 0) & (ks_[np.maximum(pos, 0)] == q)
    return np.where(ok, o[np.maximum(pos, 0)], -1)


def _rap_terms(nc, chptr, child, chw, fptr, fcol, free, par, pw):
    """every contribution of a RAP kernel in its walk order: coarse row i, child slot k, fine entry ee, parent j, the FP32 weight
    product float(w_i w_j).  Children and neighbours that are not free are skipped, parent slots of weight 0 as well."""
    nch = np.diff(chptr)
    i = np.repeat(np.arange(nc), nch)
    k = np.arange(len(child))
    a = np.asarray(child, dtype=np.int64)
    m = free[a]
    i, k, a = i[m], k[m], a[m]
    deg = fptr[a + 1] - fptr[a]
    rep = np.repeat(np.arange(len(a)), deg)
    ee = fptr[a][rep] + (np.arange(deg.sum()) - np.repeat(np.cumsum(deg) - deg, deg))
    i, k, a = i[rep], k[rep], a[rep]
    b = np.asarray(fcol, dtype=np.int64)[ee]
    m = free[b]
    i, k, a, ee, b = i[m], k[m], a[m], ee[m], b[m]
    par, pw = np.asarray(par).reshape(-1, 2), np.asarray(pw, dtype=np.float32).reshape(-1, 2)
    out = []
    for pj in range(2):
        wj = pw[b, pj]
        m = wj != 0
        ww = (np.asarray(chw, dtype=np.float32)[k[m]] * wj[m]).astype(np.float32)
        out.append((i[m], k[m], a[m], ee[m], par[b[m], pj].astype(np.int64), ww))
    return tuple(np.concatenate([o[t] for o in out]) for t in range(6))


def _rap_gather(nc, cptr, ccol, i, j, terms, absterms):
    """(sum, magnitude sum, count) per coarse entry of the contributions (i, j, term); missed: rows of <= 64 entries (the only
    ones the kernels check, see k_mg_rap) that receive a contribution with no entry of its column"""
    e = _coarse_lookup(cptr, ccol, nc, i, j)
    n = int(cptr[-1])
    L = np.zeros(n)
    np.add.at(L, e[e >= 0], 1.0)
    shape = (n,) + terms.shape[1:]
    val, mag = np.zeros(shape), np.zeros(shape)
    np.add.at(val, e[e >= 0], terms[e >= 0])
    np.add.at(mag, e[e >= 0], absterms[e >= 0])
    short = np.diff(cptr) <= 64
    missed = bool(np.any((e < 0) & short[i]))
    # every lane whose column occurs twice in a row takes the full sum
    row = np.repeat(np.arange(nc), np.diff(cptr))
    last = _coarse_lookup(cptr, ccol, nc, row, ccol)
    return val[last], mag[last], L[last], missed


def mg_d0(N2, nadj_ptr, nadj, db, rowscale, rowflag):
    """k_mg_d0: d0[r] = float(db[3 e] / rowscale[6 r]) at the row's (last) diagonal pair e, 0 on a Dirichlet row (rowflag[3 r]) or a
    row without a diagonal; mixed: a node whose three rowflags differ (flags[1] bit 32)"""
    row = np.repeat(np.arange(N2), np.diff(nadj_ptr))
    e = np.arange(len(row))
    last = np.full(N2, -1, dtype=np.int64)
    dg = np.asarray(nadj) == row
    np.maximum.at(last, row[dg], e[dg])
    f = np.asarray(rowflag).reshape(-1, 3)
    d = np.where(last >= 0, np.asarray(db)[3 * np.maximum(last, 0)] / np.asarray(rowscale)[6 * np.arange(N2)], 0.0)
    d = np.where(f[:, 0] != 0, 0.0, d)
    mixed = bool(np.any((f[:, 0] != f[:, 1]) | (f[:, 0] != f[:, 2])))
    return d.astype(np.float32), mixed


def mg_rap(nc, chptr, child, chw, nadj_ptr, nadj, db, rowscale, rowflag, par, pw, cptr, ccol):
    """k_mg_rap: Ac[e] = sum over the contributions to (i, ccol[e]) of (double)float(w_i w_j) * (db[3 ee] * (1 / rowscale[6 a])),
    children a and neighbours b with rowflag[3 .] set skipped.  Returns (Ac, sum |terms|, count, missed) in FP64."""
    free = np.asarray(rowflag).reshape(-1, 3)[:, 0] == 0
    i, k, a, ee, j, ww = _rap_terms(nc, chptr, child, chw, np.asarray(nadj_ptr), nadj, free, par, pw)
    t = ww.astype(np.float64) * (np.asarray(db)[3 * ee] * (1.0 / np.asarray(rowscale)[6 * a]))
    return _rap_gather(nc, cptr, ccol, i, j, t, np.abs(t))


def _row_sequential_sum(cptr, v):
    """FP32 sum of v over each row in entry order, one rounding per addition (as a single thread adds)"""
    n = len(cptr) - 1
    L = np.diff(cptr)
    s = np.zeros(n, dtype=np.float32)
    v = np.asarray(v, dtype=np.float32)
    for t in range(int(L.max()) if n else 0):
        m = L > t
        s[m] = (s[m] + v[cptr[:-1][m] + t]).astype(np.float32)
    return s


def mg_coarse_finish(nc, cptr, ccol, Ac, cfine, rowflag):
    """k_mg_coarse_finish: d = Ac at the row's (last) diagonal entry, 0 without one; an identity row where the vertex's fine row is
    a Dirichlet row or !(d > 0) (cc 1 on the diagonal entry, 0 elsewhere, cflag 1, dcinv 0), else cc = float(Ac / d),
    dcinv = float(1 / d); dcinv4 pads 0; rowmax = the largest FP32 sum of |cc| over a row, added in entry order.
    Returns (cc, cflag [3 nc], dcinv4 [4 nc], rowmax)."""
    row = np.repeat(np.arange(nc), np.diff(cptr))
    e = np.arange(len(row))
    dg = np.full(nc, -1, dtype=np.int64)
    m = np.asarray(ccol) == row
    np.maximum.at(dg, row[m], e[m])
    Ac = np.asarray(Ac, dtype=np.float64)
    d = np.where(dg >= 0, Ac[np.maximum(dg, 0)], 0.0)
    ident = (np.asarray(rowflag).reshape(-1, 3)[np.asarray(cfine, dtype=np.int64), 0] != 0) | ~(d > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        cc = np.where(ident[row], (e == dg[row]).astype(np.float64), Ac / d[row]).astype(np.float32)
        di = np.where(ident, 0.0, 1.0 / d).astype(np.float32)
    cflag = np.repeat(ident.astype(np.uint8), 3)
    dcinv4 = np.zeros((nc, 4), dtype=np.float32)
    dcinv4[:, :3] = di[:, None]
    rs = np.abs(cc)
    rowmax = _row_sequential_sum(cptr, rs).max() if nc else np.float32(0)
    return cc, cflag, dcinv4.ravel(), np.float32(rowmax)


def mg_restrict(nc, chptr, child, chw, d0, r4, dcinv4):
    """k_mg_restrict: rc = dcinv * sum_k float(chw_k d0[a_k]) r[a_k] per component.  Returns (value, bound) [nc][3] in FP64, the
    bound (L + 10) 2^-24 |dcinv| sum |terms| with L the children of the coarse node"""
    a = np.asarray(child, dtype=np.int64)
    w = (np.asarray(chw, dtype=np.float32) * np.asarray(d0, dtype=np.float32)[a]).astype(np.float64)
    r = np.asarray(r4, dtype=np.float32).reshape(-1, 4)[a, :3].astype(np.float64)
    t = w[:, None] * r
    i = np.repeat(np.arange(nc), np.diff(chptr))
    s, S = np.zeros((nc, 3)), np.zeros((nc, 3))
    np.add.at(s, i, t)
    np.add.at(S, i, np.abs(t))
    di = np.asarray(dcinv4, dtype=np.float32).reshape(-1, 4)[:, :1].astype(np.float64)
    L = np.diff(chptr)[:, None].astype(np.float64)
    return di * s, (L + 10) * U32 * np.abs(di) * S


def mg_prolong(par, pw, live, xc4):
    """k_mg_prolong / k_sbmg_prolong: e[a] = pw0 x[par0] + pw1 x[par1] where live[a] (d0 != 0, resp. !flag), else 0.  Returns
    (value, bound) [N][3]: bound 2 * 2^-24 (|pw0 x0| + |pw1 x1|), 0 on the rows that must be exactly zero"""
    par, pw = np.asarray(par, dtype=np.int64).reshape(-1, 2), np.asarray(pw, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    x = np.asarray(xc4, dtype=np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    u, v = pw[:, :1] * x[par[:, 0]], pw[:, 1:] * x[par[:, 1]]
    live = np.asarray(live, dtype=bool)[:, None]
    return np.where(live, u + v, 0.0), np.where(live, 2 * U32 * (np.abs(u) + np.abs(v)), 0.0)


def sbmg_flags(nS, sb_ptr, sb_col, vals):
    """k_sbmg_flags: 0 where each of the node's three rows has a non-zero outside the diagonal entry of its diagonal block, else 1"""
    v = np.asarray(vals, dtype=np.float32).reshape(-1, 3, 3)[:sb_ptr[nS]]
    row = np.repeat(np.arange(nS), np.diff(sb_ptr))
    dg = np.asarray(sb_col)[:len(row)] == row
    off = v != 0
    off[dg] &= ~np.eye(3, dtype=bool)
    per = np.zeros((nS, 3), dtype=np.int64)
    np.add.at(per, row, off.any(axis=2).astype(np.int64))
    return (~(per > 0).all(axis=1)).astype(np.uint8)


def sbmg_rap(nc, chptr, child, chw, sb_ptr, sb_col, vals, snode, rowscale, flag, par, pw, cptr, ccol):
    """k_sbmg_rap: cvals[e][c][t] = sum over the contributions of float(w_i w_j) * vals[ee][c][t] * float(1 / rowscale[6 r + 3 + c])
    (r = snode[a]), flagged children / neighbours skipped.  Returns (cvals [n][9], sum |terms|, count, missed) in FP64."""
    free = np.asarray(flag) == 0
    i, k, a, ee, j, ww = _rap_terms(nc, chptr, child, chw, np.asarray(sb_ptr), sb_col, free, par, pw)
    r = np.asarray(snode, dtype=np.int64)[a]
    isc = (1.0 / np.asarray(rowscale)[6 * r[:, None] + 3 + np.arange(3)]).astype(np.float32).astype(np.float64)
    v = np.asarray(vals, dtype=np.float32).reshape(-1, 3, 3)[ee].astype(np.float64)
    t = (ww.astype(np.float64)[:, None, None] * v * isc[:, :, None]).reshape(-1, 9)
    return _rap_gather(nc, cptr, ccol, i, j, t, np.abs(t))


def inv3(a):
    """inverse of [n][3][3] blocks by the adjugate in extended precision (np.longdouble); returns (inverse, det) in that type"""
    a = np.asarray(a, dtype=np.longdouble).reshape(-1, 3, 3)
    c = np.empty_like(a)
    for r in range(3):
        for s in range(3):
            m = np.delete(np.delete(a, r, axis=1), s, axis=2)
            c[:, s, r] = (-1) ** (r + s) * (m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 1, 0])
    det = a[:, 0, 0] * c[:, 0, 0] + a[:, 0, 1] * c[:, 1, 0] + a[:, 0, 2] * c[:, 2, 0]
    with np.errstate(divide="ignore", invalid="ignore"):      # singular blocks: inf / nan, replaced by the callers' rules
        return c / det[:, None, None], det


def inverse_bound(a, inv, u, c=16.0):
    """elementwise c u |A^-1| |A| |A^-1| of [n][3][3] blocks"""
    ai, aa = np.abs(np.asarray(inv, dtype=np.float64)), np.abs(np.asarray(a, dtype=np.float64).reshape(-1, 3, 3))
    return c * u * (ai @ aa @ ai)


def sbmg_coarse_finish(nc, cptr, ccol, cvals, cfine, flag):
    """k_sbmg_coarse_finish, the decisions and the exact parts: the (last) diagonal block a (identity without one); an identity row
    where the fine vertex is flagged, the row has no diagonal block, !(det a > 0) or !(a00 > 0) - there every block of the row is
    replaced by 0 and the diagonal one by I, cbinv = I, cflag 1.  Returns (ident [nc], cvals after, inverse reference [nc][3][3]
    (extended precision, identity on identity rows), the diagonal blocks [nc][3][3])."""
    row = np.repeat(np.arange(nc), np.diff(cptr))
    e = np.arange(len(row))
    dg = np.full(nc, -1, dtype=np.int64)
    m = np.asarray(ccol) == row
    np.maximum.at(dg, row[m], e[m])
    cv = np.asarray(cvals, dtype=np.float32).reshape(-1, 3, 3)
    a = np.tile(np.eye(3, dtype=np.float32), (nc, 1, 1))
    a[dg >= 0] = cv[dg[dg >= 0]]
    inv, det = inv3(a)
    ident = (np.asarray(flag)[np.asarray(cfine, dtype=np.int64)] != 0) | (dg < 0) | ~(det > 0) | ~(a[:, 0, 0] > 0)
    after = cv.copy()
    irow = ident[row]
    after[irow] = 0
    after[irow & (e == dg[row])] = np.eye(3, dtype=np.float32)
    inv[ident] = np.eye(3)
    return ident, after.reshape(-1), inv, a


def sbmg_rowmax(nc, cptr, cvals, cbinv12, ident):
    """the largest row sum max_c sum_e sum_j |(B^-1 C_e)_cj| with the kernel's own B^-1 (cbinv12) on the blocks it kept; 1 on
    identity rows.  Returns (value, bound) in FP64"""
    b = np.asarray(cbinv12, dtype=np.float32).reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    cv = np.asarray(cvals, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)
    row = np.repeat(np.arange(nc), np.diff(cptr))
    p = np.einsum("eck,ekj->ecj", b[row], cv)
    pm = np.einsum("eck,ekj->ecj", np.abs(b[row]), np.abs(cv))
    s, S = np.zeros((nc, 3)), np.zeros((nc, 3))
    np.add.at(s, row, np.abs(p).sum(axis=2))
    np.add.at(S, row, pm.sum(axis=2))
    L = 3 * np.diff(cptr)[:, None] + 8.0
    s = np.where(ident[:, None], 1.0, s)
    bnd = np.where(ident[:, None], 0.0, L * U32 * S)
    return float(s.max()) if nc else 0.0, float(bnd.max()) if nc else 0.0


def sbmg_restrict(nc, chptr, child, chw, snode, rowscale, flag, cflag, r4):
    """k_sbmg_restrict: rc = sum over the free children of chw r[a] / float(rowscale[6 snode[a] + 3 + c]), 0 on identity coarse
    rows (cflag).  Returns (value, bound) [nc][3] in FP64, bound (L + 10) 2^-24 sum |terms|"""
    a = np.asarray(child, dtype=np.int64)
    i = np.repeat(np.arange(nc), np.diff(chptr))
    m = (np.asarray(flag)[a] == 0) & (np.asarray(cflag)[i] == 0)
    a, i = a[m], i[m]
    w = np.asarray(chw, dtype=np.float32)[m].astype(np.float64)
    rs = np.asarray(rowscale)[6 * np.asarray(snode, dtype=np.int64)[a][:, None] + 3 + np.arange(3)].astype(np.float32).astype(np.float64)
    t = w[:, None] * np.asarray(r4, dtype=np.float32).reshape(-1, 4)[a, :3].astype(np.float64) / rs
    s, S = np.zeros((nc, 3)), np.zeros((nc, 3))
    np.add.at(s, i, t)
    np.add.at(S, i, np.abs(t))
    L = np.diff(chptr)[:, None].astype(np.float64)
    return s, (L + 10) * U32 * S


# ---- the exact coarse solve by block cyclic reduction (fsi_bcr.hip) ----------------------------------------------------------
BCR_PANEL = 32
BCR_RUN_STATS = ("usable", "blocks", "max_block", "levels", "bytes32", "bytes64", "setup_flops", "launches", "planned", "tasks",
                 "n32", "n64")


def bcr_reference(A, off, operators=False):
    """Block cyclic reduction of a block-tridiagonal matrix (blocks off[k]:off[k+1]) exactly as fsi_bcr.hip schedules it:
    operators in FP32, vectors FP64.  Returns solve(rhs); with operators=True also the FP64 operators in the planner's task
    order: per reduction level its forward tasks [G_jl | G_jr], then its backward tasks [D_e^-1 | H_ea | H_ec], last the top
    D_t^-1, each as (level, kind 0 forward / 1 backward / 2 top, block, W, input segments [("b" | "x", block)])."""
    K = len(off) - 1
    blk = lambda i, j: A[off[i]:off[i + 1], off[j]:off[j + 1]].copy()
    D = {k: blk(k, k) for k in range(K)}
    L = {k: (blk(k, k - 1) if k > 0 else None) for k in range(K)}
    U = {k: (blk(k, k + 1) if k + 1 < K else None) for k in range(K)}
    active, levels, ops = list(range(K)), [], []
    while len(active) > 1:
        na = len(active)
        Dinv = {active[i]: np.linalg.inv(D[active[i]]) for i in range(1, na, 2)}
        fwd, bwd, newL, newU = [], [], {}, {}
        for i in range(1, na, 2):
            e, a, c = active[i], active[i - 1], (active[i + 1] if i + 1 < na else None)
            W, segs = [Dinv[e], -Dinv[e] @ L[e]], [("b", e), ("x", a)]
            if c is not None:
                W.append(-Dinv[e] @ U[e]); segs.append(("x", c))
            bwd.append((e, np.hstack(W), segs))
        for i in range(0, na, 2):
            j, l, r = active[i], (active[i - 1] if i > 0 else None), (active[i + 1] if i + 1 < na else None)
            W, segs = [], []
            newL[j] = newU[j] = None
            if l is not None:
                Gl = -L[j] @ Dinv[l]; W.append(Gl); segs.append(("b", l)); D[j] = D[j] + Gl @ U[l]
                if i >= 2:
                    newL[j] = Gl @ L[l]
            if r is not None:
                Gr = -U[j] @ Dinv[r]; W.append(Gr); segs.append(("b", r)); D[j] = D[j] + Gr @ L[r]
                if i + 2 < na:
                    newU[j] = Gr @ U[r]
            if W:
                fwd.append((j, np.hstack(W), segs))
        for i in range(0, na, 2):
            L[active[i]], U[active[i]] = newL[active[i]], newU[active[i]]
        lv = len(levels)
        ops += [(lv, 0, j, W, sg) for j, W, sg in fwd] + [(lv, 1, e, W, sg) for e, W, sg in bwd]
        levels.append(([(j, W.astype(np.float32), sg) for j, W, sg in fwd], [(e, W.astype(np.float32), sg) for e, W, sg in bwd]))
        active = active[0::2]
    Dt = np.linalg.inv(D[active[0]])
    ops.append((len(levels), 2, active[0], Dt, [("b", active[0])]))
    top = (active[0], Dt.astype(np.float32))

    def solve(rhs):
        b, x = rhs.astype(np.float64).copy(), np.zeros(len(rhs))
        seg = lambda v, k: v[off[k]:off[k + 1]]
        for fwd, _ in levels:
            upd = {j: seg(b, j) + W.astype(np.float64) @ np.concatenate([seg(b, k) for _, k in segs]) for j, W, segs in fwd}
            for j, v in upd.items():
                b[off[j]:off[j + 1]] = v
        x[off[top[0]]:off[top[0] + 1]] = top[1].astype(np.float64) @ seg(b, top[0])
        for _, bwd in reversed(levels):
            for e, W, segs in bwd:
                x[off[e]:off[e + 1]] = W.astype(np.float64) @ np.concatenate([seg(b if s == "b" else x, k) for s, k in segs])
        return x
    return (solve, ops) if operators else solve


def bcr_tasks_of(ops, off):
    """the task table of shim_bcr_run ([n][16]) and an FP32 arena for operators in bcr_reference's order (rows padded to a
    multiple of 4 columns, as bcr_plan lays them out)"""
    tasks, chunks, a32 = [], [], 0
    for lv, kind, blk, W, segs in ops:
        rows, cols = W.shape
        ldw = (cols + 3) & ~3
        t = [a32, rows, ldw, off[blk], len(segs)] + [0] * 9 + [lv, kind]
        for k, (src, b) in enumerate(segs):
            t[5 + 3 * k:8 + 3 * k] = [off[b], off[b + 1] - off[b], 1 if src == "x" else 0]
        Wp = np.zeros((rows, ldw), dtype=np.float32)
        Wp[:, :cols] = W
        chunks.append(Wp.ravel())
        a32 += rows * ldw
        tasks.append(t)
    return np.asarray(tasks, dtype=np.int64), np.concatenate(chunks)


def bcr_task_operator(task, arena32):
    """the FP32 operator W [rows][columns of its segments] of a task row of shim_bcr_run (padding columns dropped)"""
    w, rows, ldw, nseg = int(task[0]), int(task[1]), int(task[2]), int(task[4])
    cols = sum(int(task[6 + 3 * k]) for k in range(nseg))
    return np.asarray(arena32[w:w + rows * ldw], dtype=np.float32).reshape(rows, ldw)[:, :cols]


def bcr_task_apply(tasks, arena32, rhs, absolute=False):
    """The solve of fsi_bcr.hip (forward levels, top, backward levels in reverse) with the given FP32 operators and FP64
    vectors, in the solve's own order.  absolute: with |W| and |rhs| - every term's magnitude carried through, the scale of the
    round-off bound of the kernels' sums."""
    tasks = np.asarray(tasks).reshape(-1, 16)
    b, x = np.array(rhs, dtype=np.float64), np.zeros(len(rhs))
    if absolute:
        b = np.abs(b)
    nlev = int(tasks[:, 14].max())

    def run(t):
        W = bcr_task_operator(t, arena32).astype(np.float64)
        W = np.abs(W) if absolute else W
        v = np.concatenate([(x if t[7 + 3 * k] else b)[t[5 + 3 * k]:t[5 + 3 * k] + t[6 + 3 * k]] for k in range(int(t[4]))])
        return W @ v
    for lv in range(nlev):
        for t in tasks[(tasks[:, 14] == lv) & (tasks[:, 15] == 0)]:
            b[t[3]:t[3] + t[1]] += run(t)
    for t in tasks[tasks[:, 15] == 2]:
        x[t[3]:t[3] + t[1]] = run(t)
    for lv in reversed(range(nlev)):
        for t in tasks[(tasks[:, 14] == lv) & (tasks[:, 15] == 1)]:
            x[t[3]:t[3] + t[1]] = run(t)
    return x


def gj_inverse(A):
    """The blocked Gauss-Jordan of k_bcr_panel / k_bcr_gemm without pivoting, in FP64: per panel of 32 columns the pivot block's
    inverse P, R = P A[panel rows, :] (P itself on the panel's columns), the column panel C (its own rows zeroed), then
    A[panel rows] = R, A[:, panel] = 0 outside the panel rows, A -= C R.  Returns (inverse, bad): bad when a pivot of the
    in-panel Gauss-Jordan is not finite or |pivot| <= 1e-290 (where the kernel raises its flag and divides by 1)."""
    A = np.array(A, dtype=np.float64)
    m = len(A)
    bad = False
    for k0 in range(0, m, BCR_PANEL):
        nb = min(BCR_PANEL, m - k0)
        Ps, Q = A[k0:k0 + nb, k0:k0 + nb].copy(), np.eye(nb)
        for p in range(nb):
            piv = Ps[p, p]
            b = not (abs(piv) > 1e-290) or not np.isfinite(piv)
            bad |= b
            ip = 1.0 if b else 1.0 / piv
            Ps[p, p + 1:] *= ip
            Q[p] *= ip
            for r in range(nb):
                if r != p:
                    f = Ps[r, p]
                    Ps[r, p + 1:] -= f * Ps[p, p + 1:]
                    Q[r] -= f * Q[p]
        R = Q @ A[k0:k0 + nb]
        R[:, k0:k0 + nb] = Q
        C = A[:, k0:k0 + nb].copy()
        C[k0:k0 + nb] = 0.0
        A[:, k0:k0 + nb] = 0.0
        A[k0:k0 + nb] = R
        A -= C @ R
    return A, bad


def bcr_inverse_layout(ms, ld32s=None):
    """Arenas of a batch of in-place inverses as bcr_plan lays them out: per block m x m values, then its panel scratch cb [m][32]
    and rb [32][m]; FP32 copies at o32 with row length ld32 (>= m; a multiple of 4 by default, -1: no copy).  Returns (desc
    [n][6] int64 for shim_bcr_invert, n64, n32, offsets of the blocks)."""
    desc, a64, a32, offs = [], 0, 0, []
    for k, m in enumerate(ms):
        ld32 = ((m + 3) & ~3) if ld32s is None else ld32s[k]
        a = a64; a64 += m * m
        cb = a64; a64 += m * BCR_PANEL
        rb = a64; a64 += m * BCR_PANEL
        o32 = -1
        if ld32 >= 0:
            o32 = a32; a32 += m * ld32; a32 = (a32 + 3) & ~3
        desc.append([a, o32, cb, rb, m, ld32])
        offs.append(a)
    return np.asarray(desc, dtype=np.int64).reshape(-1, 6), a64, a32, offs


def gemm_tiles(M, N):
    """bcr_gemm_tiles: the (ti, tj) of the 64 x 64 tiles of an M x N product, row-tile major"""
    return [(ti, tj) for ti in range((M + 63) // 64) for tj in range((N + 63) // 64)]


def task_tiles(rows):
    """bcr_task_tiles: first row of every 16-row tile of a solve task, and the rows k_bcr_apply's four waves write from it"""
    return [(r0, [r0 + 4 * w + k for w in range(4) for k in range(4) if r0 + 4 * w + k < rows]) for r0 in range(0, rows, 16)]


def tube_graph(tubes, rng, shuffle=True):
    """Synthetic walls: every tube a list of ring sizes (nodes), each node linked to itself and to every node of its own ring and
    of the rings beside it.  Ids are shuffled, then in each tube the smallest id is moved into ring 0, so that the planner's
    breadth-first search starts at that end: from a root in ring 0 of R rings the farthest set is ring R - 1 alone when R >= 3,
    or R == 2 with a single-node ring 0, or R == 1 with a single node (asserted), and the levels are the rings counted from the
    far end: level = R - 1 - ring, shared by the tubes.  Returns dict(nc, cptr, ccol, level, pos, tube, ring, m) with pos the
    planner's numbering (by level, ascending id inside one) and m the unknowns per level."""
    ids, ring_of, tube_of, lev = [], [], [], []
    nid = 0
    for t, rings in enumerate(tubes):
        R = len(rings)
        assert R >= 3 or rings[0] == 1, "ring 0 must be a single node below three rings"
        for k, n in enumerate(rings):
            ids.append(np.arange(nid, nid + n)); nid += n
            ring_of += [k] * n; tube_of += [t] * n; lev += [R - 1 - k] * n
    nc = nid
    ring_of, tube_of, lev = np.asarray(ring_of), np.asarray(tube_of), np.asarray(lev)
    perm = rng.permutation(nc) if shuffle else np.arange(nc)          # node id of generator slot s
    for t in range(len(tubes)):
        slots = np.flatnonzero(tube_of == t)
        smin = slots[np.argmin(perm[slots])]
        s0 = slots[ring_of[slots] == 0][0]
        perm[smin], perm[s0] = perm[s0], perm[smin]
    rows, cols = [], []
    start = 0
    for t, rings in enumerate(tubes):
        offs = np.concatenate([[0], np.cumsum(rings)]) + start
        for k in range(len(rings)):
            mine = np.arange(offs[k], offs[k + 1])
            nb = np.arange(offs[max(k - 1, 0)], offs[min(k + 2, len(rings))])
            rows.append(np.repeat(mine, len(nb))); cols.append(np.tile(nb, len(mine)))
        start = offs[-1]
    r, c = perm[np.concatenate(rows)], perm[np.concatenate(cols)]
    o = np.lexsort((c, r))
    r, c = r[o], c[o]
    cptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=nc))]).astype(np.int64)
    level = np.empty(nc, dtype=np.int32)
    level[perm] = lev
    ring = np.empty(nc, dtype=np.int64); ring[perm] = ring_of
    tube = np.empty(nc, dtype=np.int64); tube[perm] = tube_of
    order = np.lexsort((np.arange(nc), level))
    pos = np.empty(nc, dtype=np.int32)
    pos[order] = np.arange(nc)
    return dict(nc=nc, cptr=cptr, ccol=c.astype(np.int32), level=level, pos=pos, tube=tube, ring=ring,
                m=3 * np.bincount(level).astype(np.int64))


def tube_values(g, kappa, rng, skew=0.3):
    """FP32 3x3 blocks [nnz][9] of a non-symmetric operator on a tube graph whose condition number is about kappa: a block
    graph Laplacian with random definite edge blocks (symmetric part), a skew-symmetric part of relative size `skew` on the
    edges, and sigma I on the diagonal with sigma = lambda_max / kappa.  The symmetric part stays definite, so elimination without
    pivoting does not break down."""
    nc, cptr, ccol = g["nc"], g["cptr"], g["ccol"]
    row = np.repeat(np.arange(nc), np.diff(cptr))
    nnz = len(ccol)
    lo, hi = np.minimum(row, ccol).astype(np.int64), np.maximum(row, ccol).astype(np.int64)
    key = lo * nc + hi
    uk, inv = np.unique(key, return_inverse=True)
    B = rng.standard_normal((len(uk), 3, 3))
    Me = np.einsum("eij,ekj->eik", B, B) / 3 + 0.3 * np.eye(3)           # definite edge blocks, one per unordered pair
    Ke = skew * rng.standard_normal((len(uk), 3, 3))
    off = row != ccol
    vals = np.zeros((nnz, 3, 3))
    up = off & (row < ccol)
    vals[off] = -Me[inv[off]]
    vals[up] += Ke[inv[up]]
    vals[off & ~up] -= np.transpose(Ke[inv[off & ~up]], (0, 2, 1))
    diag = np.flatnonzero(~off)
    dsum = np.zeros((nc, 3, 3))
    np.add.at(dsum, row[off], Me[inv[off]])
    lmax = 2.0 * np.abs(dsum).sum(axis=2).max() if nc > 1 else 1.0
    vals[diag] = dsum[row[diag]] + (lmax / kappa) * np.eye(3)
    return vals.reshape(nnz, 9).astype(np.float32)


def tube_dense(g, cvals, shift=0.0):
    """the dense FP64 operator of FP32 block values in the solve's own (planner's) order, A + shift blockdiag(A) formed as k_bcr_fill
    forms it: (1 + shift) * double(v) on a node's own block"""
    nc, cptr, ccol, pos = g["nc"], g["cptr"], g["ccol"], g["pos"].astype(np.int64)
    row = np.repeat(np.arange(nc), np.diff(cptr))
    v = np.asarray(cvals, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)
    f = np.where(row == ccol, 1.0 + shift, 1.0)
    A = np.zeros((3 * nc, 3 * nc))
    for a in range(3):
        for b in range(3):
            A[3 * pos[row] + a, 3 * pos[ccol] + b] = f * v[:, a, b]
    return A


def bcr_run(g, value_sets, shift, rhs=None, rc4=None, arena=False):
    """shim_bcr_run on a tube graph: returns dict(stats, ready, pos, x [sets][nrhs][3 nc], xc4 [sets][nrhs][4 nc], arena32,
    tasks [ntasks][16]); x / xc4 start as NaN sentinels (left where a refresh was not ready)"""
    nc, cptr, ccol = g["nc"], g["cptr"], g["ccol"]
    sets = np.ascontiguousarray(np.asarray(value_sets, dtype=np.float32).reshape(len(value_sets), -1))
    nrhs = len(rhs) if rhs is not None else (0 if rc4 is None else len(rc4))
    rhs = None if rhs is None else np.ascontiguousarray(np.asarray(rhs, dtype=np.float64))
    rc4 = None if rc4 is None else np.ascontiguousarray(np.asarray(rc4, dtype=np.float32))
    stats = np.zeros(len(BCR_RUN_STATS), dtype=np.int64)
    ready = np.full(len(sets), -1, dtype=np.int32)
    pos = np.full(nc, -1, dtype=np.int32)
    x = np.full((len(sets), nrhs, 3 * nc), np.nan)
    xc4 = np.full((len(sets), nrhs, 4 * nc), np.nan, dtype=np.float32)
    cap32 = cap_t = 0
    a32 = tk = None
    if arena:                                   # a plan-only call first for the sizes
        call("shim_bcr_run", nc, cptr, ccol, 0, sets, shift, 0, None, None, stats, None, None, None, None, None, 0, None, 0)
        cap32, cap_t = int(stats[10]), int(stats[9])
        a32 = np.full(max(cap32, 1), np.nan, dtype=np.float32)
        tk = np.full((max(cap_t, 1), 16), -7, dtype=np.int64)
    call("shim_bcr_run", nc, cptr, ccol, len(sets), sets, shift, nrhs, rhs, rc4, stats, ready, pos, x if rhs is not None else None,
         xc4 if rc4 is not None else None, a32, cap32, tk, cap_t)
    return dict(stats=dict(zip(BCR_RUN_STATS, (int(v) for v in stats))), ready=ready, pos=pos, x=x, xc4=xc4, arena32=a32,
                tasks=None if tk is None else tk[:cap_t])


# ---- the field split, the Schur complement and the pressure step (fsi_block.hip; tests/test_gpu_block_kernels.py) ------------
# The restatements below go through scipy: the monolithic matrix is a CSR matrix of entry NUMBERS, its field blocks are taken by
# row / column sets, and only the result is laid out in the kernels' arrays.  None of them repeats a kernel's index arithmetic.
TAIL = 8                     # fsi_kernel_shim.hip SHIM_TAIL: sentinel entries behind every output of the block entry points
EPS64 = float(np.finfo(np.float64).eps)
SCHUR_ROW_LIMIT = 1024       # fsi_block.hip MAXS2: entries of a Schur row the LDS accumulator holds


def out(n, dtype, fill):
    """an output array of n entries plus the TAIL sentinels, all set to `fill`"""
    return np.full(int(n) + TAIL, fill, dtype=dtype)


def tail_untouched(a, n, fill):
    t = a[int(n):]
    return len(t) == TAIL and (np.all(np.isnan(t)) if isinstance(fill, float) and np.isnan(fill) else np.all(t == fill))


def shaped_graph(N2, V, rng, shapes=(), reach=24, max_deg=12, vertices_first=False):
    """mono_graph with chosen nodes of an exact shape: shapes is a list of (deg, pdeg, is_vertex), each given to one node (distinct,
    drawn at random among the vertices / the other nodes): the node has exactly deg neighbours (itself included) of which exactly
    pdeg are vertices.  Returns (graph, nodes) with nodes[k] the node of shapes[k]."""
    import scipy.sparse as sp
    vrank = (np.arange(V) if vertices_first else rng.choice(N2, size=V, replace=False)).astype(np.int32)
    isv = np.zeros(N2, dtype=bool)
    isv[vrank] = True
    k = rng.integers(0, max_deg + 1, N2)
    src = np.repeat(np.arange(N2, dtype=np.int64), k)
    dst = np.clip(src + rng.integers(-reach, reach + 1, len(src)), 0, N2 - 1)
    vs, os_ = np.flatnonzero(isv), np.flatnonzero(~isv)
    want_v = np.array([bool(sh[2]) for sh in shapes], dtype=bool)
    nodes = np.zeros(len(shapes), dtype=np.int64)
    nodes[want_v] = rng.choice(vs, size=int(want_v.sum()), replace=False) if want_v.any() else []
    nodes[~want_v] = rng.choice(os_, size=int((~want_v).sum()), replace=False) if (~want_v).any() else []
    keep = ~np.isin(src, nodes)
    src, dst = [src[keep], np.arange(N2)], [dst[keep], np.arange(N2)]
    for r, (deg, pdeg, _) in zip(nodes, shapes):
        pv = pdeg - int(isv[r])
        po = deg - pdeg - int(not isv[r])
        assert pv >= 0 and po >= 0, "the node itself counts: a vertex has pdeg >= 1, any other node deg - pdeg >= 1"
        nb = np.concatenate([rng.choice(vs[vs != r], size=pv, replace=False), rng.choice(os_[os_ != r], size=po, replace=False)])
        src.append(np.full(len(nb), r))
        dst.append(nb)
    G = sp.csr_matrix((np.ones(sum(map(len, src))), (np.concatenate(src), np.concatenate(dst))), shape=(N2, N2))
    G.sum_duplicates()
    G.sort_indices()
    pos = np.full(N2, -1, dtype=np.int64)
    pos[vrank] = np.arange(V)
    Pm = sp.csr_matrix((np.ones(V), (vrank.astype(np.int64), np.arange(V))), shape=(N2, V))
    PA = (G @ Pm).tocsr()
    PA.sort_indices()
    g = (G.indptr.astype(np.int64), G.indices.astype(np.int32), PA.indptr.astype(np.int64), PA.indices.astype(np.int32), vrank)
    return g, nodes


def entry_matrix(N2, V, graph):
    """The monolithic pattern (expand_cols) as a scipy CSR matrix whose values are the entry numbers + 1, and the row / column
    sets of the three fields (d, v, p)"""
    import scipy.sparse as sp
    rowptr, cols, _ = expand_cols(N2, *graph)
    n = 6 * N2 + V
    E = sp.csr_matrix((np.arange(1, rowptr[-1] + 1, dtype=np.float64), cols, rowptr), shape=(n, n))
    assert E.has_sorted_indices
    Dd = np.arange(6 * N2).reshape(N2, 6)[:, :3].ravel()
    return E, Dd, Dd + 3, 6 * N2 + np.arange(V)


def _blk(E, rows, cols):
    B = E[rows][:, cols].tocsr()
    B.sort_indices()
    return B


def block_structure(N2, V, graph):
    """The structure arrays of launch_block_structure (and rowptr_pv / rowptr_pp / cols_pp, which the host builds): each block is
    the CSR pattern of the monolithic matrix restricted to its row and column sets."""
    E, Dd, Vd, Pd = entry_matrix(N2, V, graph)
    vv, vp, pv, pp = _blk(E, Vd, Vd), _blk(E, Vd, Pd), _blk(E, Pd, Vd), _blk(E, Pd, Pd)
    i64, i32 = (lambda a: np.ascontiguousarray(a, dtype=np.int64)), (lambda a: np.ascontiguousarray(a, dtype=np.int32))
    row = np.repeat(np.arange(3 * N2), np.diff(vv.indptr))
    diagpos3 = np.full(3 * N2, -1, dtype=np.int64)
    hit = np.flatnonzero(vv.indices == row)
    diagpos3[row[hit]] = hit
    return dict(rowptr3=i64(vv.indptr), cols3=i32(vv.indices), diagpos3=diagpos3, rowptr_vp=i64(vp.indptr), cols_vp=i32(vp.indices),
                rowptr_pv=i64(pv.indptr), cols_pv=i32(pv.indices), rowptr_pp=i64(pp.indptr), cols_pp=i32(pp.indices))


def extract_blocks(N2, V, graph, A, node_solid, ktheta):
    """The six value arrays of launch_extract_blocks in the block_structure layout.  Avv = A_vv + A_vd K, Apv = A_pv + A_pd K with
    K = ktheta on the displacement columns of solid nodes (the d and v columns of a node share their pattern, so A_vd lies on A_vv's).
    Also: Avv_mag / Apv_mag = |e_v| + |ktheta e_d| (|e_v| off the solid columns), Avv_solid / Apv_solid the entries in solid
    columns, and the parts e_v, e_d themselves (Avv_v, Avv_d, Apv_v, Apv_d)."""
    E, Dd, Vd, Pd = entry_matrix(N2, V, graph)
    A = np.asarray(A, dtype=np.float64)
    val = lambda B: A[B.data.astype(np.int64) - 1]      # noqa: E731
    res = dict(Add=val(_blk(E, Dd, Dd)), Adv=val(_blk(E, Dd, Vd)), Avp=val(_blk(E, Vd, Pd)), App=val(_blk(E, Pd, Pd)))
    for name, rows in (("Avv", Vd), ("Apv", Pd)):
        Bv, Bd = _blk(E, rows, Vd), _blk(E, rows, Dd)
        assert np.array_equal(Bv.indptr, Bd.indptr) and np.array_equal(Bv.indices, Bd.indices)
        sol = np.asarray(node_solid)[Bv.indices // 3] != 0
        ev, ed = val(Bv), val(Bd)
        res[name] = np.where(sol, ev + ktheta * ed, ev)
        res[name + "_mag"] = np.abs(ev) + np.where(sol, np.abs(ktheta * ed), 0.0)
        res[name + "_solid"], res[name + "_v"], res[name + "_d"] = sol, ev, ed
    return res


def assemble_blocks(N2, V, graph, st, b, node_solid, ktheta):
    """the inverse of extract_blocks (K undone): the monolithic value array"""
    E, Dd, Vd, Pd = entry_matrix(N2, V, graph)
    A = np.full(E.nnz, np.nan)
    put = lambda rows, cols, v: A.__setitem__(_blk(E, rows, cols).data.astype(np.int64) - 1, v)      # noqa: E731
    put(Dd, Dd, b["Add"]); put(Dd, Vd, b["Adv"]); put(Vd, Pd, b["Avp"]); put(Pd, Pd, b["App"])
    put(Vd, Dd, b["Avv_d"]); put(Pd, Dd, b["Apv_d"])
    put(Vd, Vd, np.where(b["Avv_solid"], b["Avv"] - ktheta * b["Avv_d"], b["Avv"]))
    put(Pd, Vd, np.where(b["Apv_solid"], b["Apv"] - ktheta * b["Apv_d"], b["Apv"]))
    return A


def _group_sum(key, v, n):
    """sum of the longdouble values v by integer key into n bins"""
    res = np.zeros(n, dtype=np.longdouble)
    if len(key):
        o = np.argsort(key, kind="stable")
        ks_, vs = key[o], np.asarray(v, dtype=np.longdouble)[o]
        first = np.flatnonzero(np.concatenate([[True], ks_[1:] != ks_[:-1]]))
        res[ks_[first]] = np.add.reduceat(vs, first)
    return res


def schur_pattern(V, st):
    """s_rowptr, s_cols: the columns of A_pp and of (pattern of A_pv) x (pattern of A_vp), ascending per row"""
    import scipy.sparse as sp
    n3 = len(st["rowptr3"]) - 1
    one = lambda ptr, col, shape: sp.csr_matrix((np.ones(len(col)), col, ptr), shape=shape)      # noqa: E731
    Pt = (one(st["rowptr_pp"], st["cols_pp"], (V, V)) + one(st["rowptr_pv"], st["cols_pv"], (V, n3)) @
          one(st["rowptr_vp"], st["cols_vp"], (n3, V))).tocsr()
    Pt.sort_indices()
    return Pt.indptr.astype(np.int64), Pt.indices.astype(np.int32)


def schur_full(V, st, s_rowptr, s_cols, Apv, App, Avp, Avv):
    """S = A_pp - Apv diag(Avv)^-1 A_vp entry by entry on the given pattern: (S, sum |terms|, number of terms, rows over the
    limit), the sums in extended precision.  A term is an A_pp entry or one product (Apv_qR / Avv_RR) Avp_Rc; exact zeros of Apv,
    Avp, App are no terms (the kernel skips them).  Rows longer than SCHUR_ROW_LIMIT are listed and left out (S = NaN there)."""
    ld = np.longdouble
    nS = int(s_rowptr[V])
    skey = np.repeat(np.arange(V, dtype=np.int64), np.diff(s_rowptr)) * max(V, 1) + s_cols
    rows_pp = np.repeat(np.arange(V, dtype=np.int64), np.diff(st["rowptr_pp"]))
    # products: every Apv entry (q, R) with every Avp entry (R, c)
    rows_pv = np.repeat(np.arange(V, dtype=np.int64), np.diff(st["rowptr_pv"]))
    R = st["cols_pv"].astype(np.int64)
    cnt = np.diff(st["rowptr_vp"])[R]
    e = np.repeat(np.arange(len(R)), cnt)
    t = st["rowptr_vp"][R[e]] + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    coef = np.asarray(Apv, dtype=ld)[e] / np.asarray(Avv, dtype=ld)[st["diagpos3"][R[e]]]
    term = -coef * np.asarray(Avp, dtype=ld)[t]
    live = (np.asarray(Apv)[e] != 0.0) & (np.asarray(Avp)[t] != 0.0)
    key = np.concatenate([rows_pp * max(V, 1) + st["cols_pp"], (rows_pv[e] * max(V, 1) + st["cols_vp"][t])[live]])
    val = np.concatenate([np.asarray(App, dtype=ld), term[live]])
    nz = np.concatenate([np.asarray(App) != 0.0, np.ones(int(live.sum()), dtype=bool)])
    key, val = key[nz], val[nz]
    where = np.searchsorted(skey, key)
    assert np.all(where < nS) and np.array_equal(skey[where], key), "a term outside the Schur pattern"
    S, mag = _group_sum(where, val, nS), _group_sum(where, np.abs(val), nS)
    L = np.bincount(where, minlength=nS).astype(np.float64)
    over = np.flatnonzero(np.diff(s_rowptr) > SCHUR_ROW_LIMIT)
    S = S.astype(np.float64)
    for q in over:
        S[s_rowptr[q]:s_rowptr[q + 1]] = np.nan
    return S, mag.astype(np.float64), L, over


def db_extract(N2, graph, st, vals):
    """k_extract_db: db[e][i] = the (i, i) entry of node pair e's 3x3 block, and whether any other entry is not zero"""
    import scipy.sparse as sp
    n3 = 3 * N2
    M = sp.csr_matrix((np.arange(1, len(vals) + 1, dtype=np.float64), st["cols3"], st["rowptr3"]), shape=(n3, n3))
    nadj_ptr, nadj = graph[0], graph[1].astype(np.int64)
    r = np.repeat(np.arange(N2), np.diff(nadj_ptr))
    vals = np.asarray(vals)
    db = np.stack([vals[np.asarray(M[3 * r + i, 3 * nadj + i]).ravel().astype(np.int64) - 1] for i in range(3)], axis=1)
    used = np.zeros(len(vals), dtype=bool)
    for i in range(3):
        used[np.asarray(M[3 * r + i, 3 * nadj + i]).ravel().astype(np.int64) - 1] = True
    return db.ravel(), bool(np.any(vals[~used] != 0.0))


def db_terms(N2, graph, db, x):
    """per row 3r + i of y = db x: (y, sum |terms|, L) in extended precision"""
    nadj_ptr, nadj = graph[0], graph[1].astype(np.int64)
    p = np.asarray(db, dtype=np.longdouble).reshape(-1, 3) * np.asarray(x, dtype=np.longdouble).reshape(-1, 3)[nadj]
    y, S = np.zeros((N2, 3), dtype=np.longdouble), np.zeros((N2, 3), dtype=np.longdouble)
    deg = np.diff(nadj_ptr)
    nz = deg > 0
    if len(p):
        y[nz] = np.add.reduceat(p, nadj_ptr[:-1][nz], axis=0)
        S[nz] = np.add.reduceat(np.abs(p), nadj_ptr[:-1][nz], axis=0)
    return y.ravel(), S.ravel(), np.repeat(deg, 3).astype(np.float64)


def rowmask(N2, graph, db):
    """k_db_rowmask: 1 where the node has a non-zero db entry"""
    r = np.repeat(np.arange(N2), np.diff(graph[0]))
    return (np.bincount(r, weights=(np.asarray(db).reshape(-1, 3) != 0.0).any(axis=1), minlength=N2) > 0).astype(np.uint8)


def chat_extract(N2, graph, db):
    """k_extract_chat: (chat, rowflag [3 N2], spread) - a row is an identity row when no off-diagonal pair entry of its component
    is non-zero; chat = the ratio to the diagonal in the first free component (1 on the diagonal / 0 elsewhere when all three
    rows of the node are identity rows); spread[e] = the largest |ratio_i - ratio_ref| over the other free components (what the
    kernel's flag bit 4 tests against 1e-9 |c| + 1e-12)."""
    nadj_ptr, nadj = graph[0], graph[1].astype(np.int64)
    db = np.asarray(db, dtype=np.float64).reshape(-1, 3)
    r = np.repeat(np.arange(N2), np.diff(nadj_ptr))
    isd = nadj == r
    assert np.array_equal(np.bincount(r[isd], minlength=N2), np.ones(N2)), "every node needs its diagonal pair"
    de = np.flatnonzero(isd)
    ident = np.stack([np.bincount(r, weights=((db[:, i] != 0.0) & ~isd), minlength=N2) == 0 for i in range(3)], axis=1)
    ref = np.argmax(~ident, axis=1)
    with np.errstate(all="ignore"):
        ratio = db / db[de[r]]
        c = ratio[np.arange(len(r)), ref[r]]
        chat = np.where(ident.all(axis=1)[r], isd.astype(np.float64), c)
        spread = np.where(~ident[r] & ~ident.all(axis=1)[r][:, None], np.abs(ratio - c[:, None]), 0.0).max(axis=1, initial=0.0)
    return chat, ident.astype(np.uint8).ravel(), spread


def ripple(n, mask=None):
    """k_mask_ripple: h = i * 0x9E3779B97F4A7C15; h ^= h >> 29; h *= 0xBF58476D1CE4E5B9; h ^= h >> 32 (mod 2^64);
    x = mask * ((h & 0xFFFF) / 65535 - 0.5)"""
    with np.errstate(over="ignore"):
        h = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    x = (h & np.uint64(0xFFFF)).astype(np.float64) / 65535.0 - 0.5
    return x if mask is None else np.asarray(mask, dtype=np.float64) * x


def power_lmax(apply, scale, n, mask=None, steps=40, dtype=np.float64):
    """power_lmax_op of fsi_precond.hip: x = ripple; 40 times y = scale(apply(x)), lam = |y| / |x|, x = y / |y|; returns lam (the
    library stores 1.2 lam).  apply / scale work in `dtype`."""
    x = ripple(n, mask).astype(dtype)
    lam = dtype(1.0)
    for _ in range(steps):
        y = scale(apply(x))
        xx, yy = np.dot(x, x), np.dot(y, y)
        if not (xx > 0 and yy > 0 and np.isfinite(yy)):
            break
        lam = np.sqrt(yy / xx)
        x = y * (dtype(1.0) / np.sqrt(yy))
    return float(lam)


def live_blocks(hb):
    """The field blocks of a live context restated with scipy from the assembled Jacobian (fsi_get_matrix, user layout, mapped
    through solver2user and row-equilibrated by rowscale).  Solver layout: node rank r holds d rows 6r + i and v rows 6r + 3 + i,
    pressure position q row 6 N2 + q.  Avv~ = Avv + ktheta Avd and Apv~ = Apv + ktheta Apd on the displacement columns of solid
    nodes (k_extract_blocks); the _mag matrices hold |e_v| + |ktheta e_d|."""
    import scipy.sparse as sp
    info = ctx_info(hb.ctx)
    N2, V = info["N2"], info["V"]
    s2u, rs = ctx_array(hb.ctx, "solver2user").astype(np.int64), ctx_array(hb.ctx, "rowscale")
    assert hb.ndof == 6 * N2 + V == len(s2u)
    M = hb.matrix()[s2u][:, s2u].tocsr()             # every stored entry kept: the pattern below is the matrix graph
    M.data *= np.repeat(rs, np.diff(M.indptr))
    node = np.arange(N2)
    Dd = (6 * node[:, None] + np.arange(3)).ravel()
    Vd, Pd = Dd + 3, 6 * N2 + np.arange(V)
    K = sp.diags(ctx_ktheta(hb.ctx) * np.repeat(ctx_array(hb.ctx, "node_solid") != 0, 3).astype(np.float64))
    return dict(N2=N2, V=V, M=M, Dd=Dd, Vd=Vd, Pd=Pd, K=K, Add=M[Dd][:, Dd].tocsr(), Adv=M[Dd][:, Vd].tocsr(),
                Avv_t=(M[Vd][:, Vd] + M[Vd][:, Dd] @ K).tocsr(), Avv_mag=(abs(M[Vd][:, Vd]) + abs(M[Vd][:, Dd]) @ K).tocsr(),
                Apv_t=(M[Pd][:, Vd] + M[Pd][:, Dd] @ K).tocsr(), Apv_mag=(abs(M[Pd][:, Vd]) + abs(M[Pd][:, Dd]) @ K).tocsr(),
                App=M[Pd][:, Pd].tocsr(), Avp=M[Vd][:, Pd].tocsr())


# ---- multicolour ILU(0) and its triangular solves (fsi_solver.hip k_ilu0_level / k_sptrsv_level; tests/test_gpu_ilu_kernels.py) --
# Nothing below repeats the kernels' arithmetic: the factor is held to the DEFINITION of ILU(0), (L U)_ij = a_ij on the pattern,
# and the solves to their own equations row by row, each with the rounding bound of the operation count involved.
ILU_MAXROW = 1024            # fsi_solver.hip MAXROW: entries of a row the factorisation's LDS tile holds


def level_layout(levels):
    """levels: [(ngroups, group_rows)], numbered in order.  Returns (n, first, ngroups, group_rows, level_of, group_of) with
    group_of a number that is distinct for every group of the matrix."""
    ng = np.array([l[0] for l in levels], dtype=np.int64)
    gr = np.array([l[1] for l in levels], dtype=np.int32)
    rows = ng * gr
    first = np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int64) if len(levels) else np.zeros(0, dtype=np.int64)
    n = int(rows.sum())
    level_of = np.repeat(np.arange(len(levels)), rows)
    gfirst = np.concatenate([[0], np.cumsum(ng)[:-1]]) if len(levels) else np.zeros(0, dtype=np.int64)
    within = np.arange(n) - first[level_of]
    group_of = gfirst[level_of] + within // np.maximum(gr[level_of], 1)
    return n, first, ng, gr, level_of, group_of


def level_violations(levels, rowptr, cols):
    """The contract of the level kernels: entries (i, j) with i and j in the same level but in different groups (there must be none)"""
    n, _, _, _, level_of, group_of = level_layout(levels)
    assert n == len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    return int(np.count_nonzero((level_of[row] == level_of[cols]) & (group_of[row] != group_of[cols])))


def level_matrix(levels, rng, symmetric=True, row_len=30, couple_group=True, own_group_only=False, heavy=(), heavy_len=(),
                 diag_first=(), diag_last=(), isolated=(), zero_lower=0.0, dominance=1.25):
    """A CSR matrix that obeys the contract of k_ilu0_level / k_sptrsv_level on `levels` = [(ngroups, group_rows)]: a row may
    reference any row of another level and any row of its own group (below and above itself), never another group of its own
    level.  Columns ascending, a diagonal entry in every row.
      row_len        about this many entries per row: the own group (with couple_group) and rows of other levels drawn at random
      couple_group   every row holds all rows of its own group (a node's d / v rows)
      own_group_only nothing but the own group: the matrix is block diagonal and ILU(0) is the exact LU of every block
      symmetric      the pattern is made symmetric (the contract is symmetric, so it survives)
      heavy, heavy_len   rows with exactly that many entries (1 = the diagonal alone); a row in diag_first / diag_last has the
                     diagonal as its first / last entry.  These rows are set after the symmetrisation.
      isolated       rows no other row references (their column is removed everywhere else)
      zero_lower     this fraction of the strictly lower entries is exactly 0.0
      dominance      |a_ii| = dominance * sum_j |a_ij|: strictly diagonally dominant by rows, so every pivot stays away from zero
    Returns a dict: n, the level arrays first / ngroups / group_rows, rowptr, cols, diagpos, vals."""
    n, first, ng, gr, level_of, group_of = level_layout(levels)
    heavy = [int(r) for r in heavy]
    special = set(heavy)
    # the entries outside the own group are drawn among the rows of the OTHER levels (none if there is no other level)
    own = (ng * gr)[level_of] if n else np.zeros(0, dtype=np.int64)
    k = np.maximum(row_len - 1 - (gr[level_of] - 1 if couple_group else 0), 0) if n else np.zeros(0, dtype=np.int64)
    k = np.where(own_group_only | (own == n), 0, (k + 1) // 2 if symmetric else k)
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    u = rng.integers(0, np.maximum(n - own[i], 1))
    j = np.where(u < first[level_of[i]], u, u + own[i])
    if not symmetric:          # a one-sided band besides the random entries, so that the two triangles differ in size too
        extra = np.arange(n, dtype=np.int64)
        i, j = np.concatenate([i, extra, extra]), np.concatenate([j, (extra * 7 + 3) % max(n, 1), (extra * 13 + 5) % max(n, 1)])
    if couple_group or own_group_only:
        gstart = first[level_of] + ((np.arange(n) - first[level_of]) // gr[level_of]) * gr[level_of]
        for t in range(int(gr.max()) if len(gr) else 0):
            ok = t < gr[level_of]
            i, j = np.concatenate([i, np.arange(n)[ok]]), np.concatenate([j, (gstart + t)[ok]])
    if symmetric:
        i, j = np.concatenate([i, j]), np.concatenate([j, i])
    i, j = np.concatenate([i, np.arange(n)]), np.concatenate([j, np.arange(n)])
    keep = (level_of[i] != level_of[j]) | (group_of[i] == group_of[j])
    keep &= ~np.isin(i, np.asarray(heavy, dtype=np.int64))
    keep &= ~(np.isin(j, np.asarray(list(isolated), dtype=np.int64)) & (i != j))
    i, j = i[keep], j[keep]
    for r, L in zip(heavy, heavy_len):
        allowed = np.flatnonzero(((level_of != level_of[r]) | (group_of == group_of[r])) & (np.arange(n) != r)
                                 & ~np.isin(np.arange(n), np.asarray(list(isolated), dtype=np.int64)))
        if r in diag_first:
            allowed = allowed[allowed > r]
        if r in diag_last:
            allowed = allowed[allowed < r]
        assert len(allowed) >= L - 1, f"row {r}: only {len(allowed)} columns allowed, {L - 1} wanted"
        pick = rng.choice(allowed, size=L - 1, replace=False)
        i, j = np.concatenate([i, np.full(L, r)]), np.concatenate([j, pick, [r]])
    code = np.unique(i * n + j)
    i, j = code // max(n, 1), code % max(n, 1)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))]).astype(np.int64)
    cols = j.astype(np.int32)
    diagpos = np.flatnonzero(i == j).astype(np.int64)
    assert len(diagpos) == n
    vals = rng.uniform(-1.0, 1.0, len(cols))
    lower = np.flatnonzero(j < i)
    if zero_lower > 0 and len(lower):
        vals[lower[rng.random(len(lower)) < zero_lower]] = 0.0
    vals[diagpos] = 0.0
    off = np.zeros(n)
    np.add.at(off, i, np.abs(vals))
    vals[diagpos] = np.where(rng.random(n) < 0.5, -1.0, 1.0) * (dominance * off + 1.0)
    for r in special | set(int(r) for r in diag_first) | set(int(r) for r in diag_last):
        if r in diag_first:
            assert diagpos[r] == rowptr[r]
        if r in diag_last:
            assert diagpos[r] == rowptr[r + 1] - 1
    return dict(n=n, first=first, ngroups=ng, group_rows=gr, rowptr=rowptr, cols=cols, diagpos=diagpos, vals=vals,
                level_of=level_of, group_of=group_of)


def ilu0_ikj(rowptr, cols, diagpos, vals, group_of=None, fault=None):
    """ILU(0) restated in plain FP64, row by row in the IKJ order: for every lower entry (i, k) in column order l = a_ik / u_kk,
    then a_ij -= l u_kj at every j > k that row i holds.  fault (negative controls of the identity check, each applied once, at the
    first place it can be): "drop_update" skips one update, "neighbour_column" applies one update to the entry next to the matching
    one, "stale_pivot" divides by the UNFACTORED diagonal of a row of the same group (what a wave would read if it did not wait
    for its own stores; group_of is needed for it).  Returns (LU, whether the fault was applied)."""
    n = len(rowptr) - 1
    LU = np.array(vals, dtype=np.float64)
    done = fault is None
    for i in range(n):
        s, e, d = int(rowptr[i]), int(rowptr[i + 1]), int(diagpos[i])
        where = {int(c): s + t for t, c in enumerate(cols[s:e])}
        for t in range(s, d):
            k = int(cols[t])
            piv = LU[diagpos[k]]
            if fault == "stale_pivot" and not done and group_of[k] == group_of[i] and vals[diagpos[k]] != piv:
                piv, done = vals[diagpos[k]], True
            l = LU[t] / piv
            LU[t] = l
            for q in range(int(diagpos[k]) + 1, int(rowptr[k + 1])):
                p = where.get(int(cols[q]))
                if p is None:
                    continue
                if not done and fault == "drop_update" and LU[q] != 0.0 and l != 0.0:
                    done = True
                    continue
                if not done and fault == "neighbour_column" and p + 1 < e and LU[q] != 0.0 and l != 0.0:
                    p, done = p + 1, True
                LU[p] -= l * LU[q]
    return LU, done


def ilu0_identity(rowptr, cols, diagpos, A, LU):
    """The definition of ILU(0) as a check of a given factor, in extended precision, row by row.  For every pattern entry (i, j):
    s_ij = sum over k < min(i, j) with (i, k) and (k, j) in the pattern of l_ik u_kj, plus u_ij (j >= i) or l_ij u_jj (j < i);
    S_ij the same sum over absolute values plus |a_ij|; n_ij the number of terms.  Returns (err, bound) per entry with
    err = |a_ij - s_ij| and bound = (n_ij + 2) eps S_ij: the componentwise backward error of Doolittle elimination
    (Higham, Accuracy and Stability of Numerical Algorithms, theorem 9.3: |A - LU| <= gamma_n |L||U|) restricted to the pattern;
    it holds for any order of the updates and with or without contraction into FMAs."""
    ld = np.longdouble
    n = len(rowptr) - 1
    lu, a = np.asarray(LU, dtype=ld), np.asarray(A, dtype=ld)
    err, bound = np.zeros(len(cols), dtype=ld), np.zeros(len(cols), dtype=ld)
    for i in range(n):
        s, e, d = int(rowptr[i]), int(rowptr[i + 1]), int(diagpos[i])
        ci = cols[s:e]
        acc, mag, cnt = np.zeros(e - s, dtype=ld), np.zeros(e - s, dtype=ld), np.ones(e - s, dtype=np.int64)
        for t in range(s, d):
            k = int(cols[t])
            us, ue = int(diagpos[k]) + 1, int(rowptr[k + 1])
            pos = np.searchsorted(ci, cols[us:ue])
            hit = pos < len(ci)
            hit[hit] = ci[pos[hit]] == cols[us:ue][hit]
            p = lu[t] * lu[us:ue][hit]
            acc[pos[hit]] += p                     # the columns of a row are distinct: no index repeats
            mag[pos[hit]] += np.abs(p)
            cnt[pos[hit]] += 1
        last = np.concatenate([lu[s:d] * lu[diagpos[cols[s:d]]], lu[d:e]])
        acc += last
        mag += np.abs(last)
        err[s:e] = np.abs(a[s:e] - acc)
        bound[s:e] = (cnt + 2) * ld(EPS64) * (mag + np.abs(a[s:e]))
    return err, bound


def _triangles(rowptr, cols, diagpos, LU):
    import scipy.sparse as sp
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    low = cols < row
    # (the unit diagonal goes in with the entries: a sum of two sparse matrices would drop the factor's explicit zeros)
    d = np.arange(n)
    L = sp.csr_matrix((np.concatenate([np.asarray(LU, dtype=np.float64)[low], np.ones(n)]),
                       (np.concatenate([row[low], d]), np.concatenate([cols[low], d]))), shape=(n, n))
    U = sp.csr_matrix((np.asarray(LU, dtype=np.float64)[~low], (row[~low], cols[~low])), shape=(n, n))
    return row, L, U


def _sample(M, row, cols):
    """the entries of the sparse matrix M at the positions (row, cols), zero where M holds none"""
    M = M.tocsr()
    M.sort_indices()
    n = M.shape[1]
    mrow = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    key = mrow.astype(np.int64) * n + M.indices
    want = row.astype(np.int64) * n + cols
    p = np.searchsorted(key, want)
    ok = p < len(key)
    ok[ok] = key[p[ok]] == want[ok]
    out = np.zeros(len(want), dtype=M.dtype)
    out[ok] = M.data[p[ok]]
    return out


def ilu0_identity_f64(rowptr, cols, diagpos, A, LU):
    """ilu0_identity through scipy's FP64 sparse products, for matrices too large for the row loops: (L U), (|L| |U|) and the term
    counts sampled on the pattern.  The sums are formed in FP64 here, so the check's own rounding is of the size of the bound:
    callers hold err to TWICE the bound returned."""
    row, L, U = _triangles(rowptr, cols, diagpos, LU)
    s = _sample(L @ U, row, cols)
    S = _sample(abs(L) @ abs(U), row, cols) + np.abs(A)
    Lp, Up = L.copy(), U.copy()
    Lp.data[:] = 1.0
    Up.data[:] = 1.0
    cnt = _sample(Lp @ Up, row, cols)               # explicit zeros of the factor count as terms, as in ilu0_identity
    return np.abs(np.asarray(A) - s), (cnt + 2) * EPS64 * S


def _row_sums(rowptr, p):
    """the sums of p over the rows of a CSR structure (zero for an empty row)"""
    out = np.zeros(len(rowptr) - 1, dtype=p.dtype)
    nz = np.diff(rowptr) > 0
    if len(p):
        out[nz] = np.add.reduceat(p, rowptr[:-1][nz])
    return out


def sptrsv_residuals(rowptr, cols, diagpos, LU, rhs, y, x):
    """The two triangular solves held to their own equations, row by row in extended precision; the bounds hold for any order of
    a row's sum.  Forward (unit lower): |rhs_i - y_i - sum_{j<i} l_ij y_j| <= (L_i + 2) eps (|rhs_i| + |y_i| + sum |l_ij y_j|);
    backward: |y_i - sum_{j>=i} u_ij x_j| <= (U_i + 3) eps (|y_i| + sum |u_ij x_j|), L_i / U_i the entries of the two parts of
    row i.  Returns (err_forward, bound_forward, err_backward, bound_backward)."""
    ld = np.longdouble
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    low = cols < row
    lu, yl, xl, rl = (np.asarray(v, dtype=ld) for v in (LU, y, x, rhs))
    pl = np.where(low, lu * yl[cols], ld(0))
    pu = np.where(~low, lu * xl[cols], ld(0))
    nl = _row_sums(rowptr, low.astype(np.int64))
    nu = np.diff(rowptr) - nl
    ef = np.abs(rl - yl - _row_sums(rowptr, pl))
    bf = (nl + 2) * ld(EPS64) * (np.abs(rl) + np.abs(yl) + _row_sums(rowptr, np.abs(pl)))
    eb = np.abs(yl - _row_sums(rowptr, pu))
    bb = (nu + 3) * ld(EPS64) * (np.abs(yl) + _row_sums(rowptr, np.abs(pu)))
    return ef, bf, eb, bb


def worst_ratio(err, bound):
    """max err / bound (an error where the bound is zero counts as inf, NaN as inf)"""
    err, bound = np.asarray(err, dtype=np.longdouble).ravel(), np.asarray(bound, dtype=np.longdouble).ravel()
    if len(err) == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def ctx_levels(ctx):
    """[(first_row, ngroups, group_rows)] of a live context's multicolour ordering"""
    lib = load()
    k = lib.shim_ctx_levels(ctx, None, 0)
    out = np.zeros(3 * max(k, 1), dtype=np.int64)
    lib.shim_ctx_levels(ctx, _arg(out), k)
    return [tuple(int(v) for v in out[3 * i:3 * i + 3]) for i in range(k)]


def f32_ripple4(nnodes):
    """k_f32_ripple4 restated with numpy integers: node i gets h = low 32 bits of (i * 2654435761) xor low 32 bits of (i >> 7),
    and the float4 (h & 1023, (h >> 10) & 1023, (h >> 20) & 1023) / 512 - 1 with a zero fourth lane (all exact in FP32)"""
    i = np.arange(nnodes, dtype=np.uint64)
    h = ((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ ((i >> np.uint64(7)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    out = np.zeros((nnodes, 4), dtype=np.float32)
    for c, sh in enumerate((0, 10, 20)):
        out[:, c] = ((h >> np.uint32(sh)) & np.uint32(1023)).astype(np.float32) / np.float32(512.0) - np.float32(1.0)
    return out.reshape(-1)


# ---- the element kernels (fsi_assembly.hip; tests/test_gpu_element_kernels.py, tests/test_gpu_element_jacobian.py) -----------
U64 = 2.0 ** -53
LD = np.longdouble
DELTA_S, ALPHA_L = 1.0e7, 1.0        # oracle.fsi_oracle.DELTA and the "constant" Laplace lifting: the Scheme the library is given
PART_LINEAR, PART_NONLINEAR = 1, 2   # fsi_element.hpp
FIELD_SLICES = (slice(0, 30), slice(30, 60), slice(60, 64))
# oracle order [d_x(10) d_y d_z v_x v_y v_z p(4)] -> Re order [node][d_x d_y d_z v_x v_y v_z], p(4): RE_OF_ORACLE[l] is where the
# oracle's local entry l sits in a row of Re
RE_OF_ORACLE = np.array([6 * (l % 10) + 3 * (l // 30) + (l % 30) // 10 if l < 60 else l for l in range(64)])


def re_from_oracle(x):
    """[..., 64] element vectors in the oracle's local order -> in the order of k_residual's Re"""
    y = np.empty_like(x)
    y[..., RE_OF_ORACLE] = x
    return y


def oracle_from_re(y):
    """the inverse of re_from_oracle"""
    return np.asarray(y)[..., RE_OF_ORACLE]


def element_structure(tet_nodes, V, rank_of_node):
    """What fsi_setup.hip builds for the element kernels from a P2 cell list (vertices are the nodes below V, local vertices first)
    and the rank of every node: cell_rank [C][10], cell_prow [C][4], cell_dofs [C][64] (local order of the oracle, solver
    numbering: dof t of the node at rank r is 6 r + t, the pressure of the q-th vertex in rank order 6 N2 + q), the node graph in
    ranks nadj_ptr / nadj (nodes that share a cell, itself included, ascending) and its vertex part padj_ptr / padj (pressure
    positions, ascending), vrank [V], the monolithic rowptr / cols / diagpos through expand_cols, enbr [C][10][10] (where node b
    stands among the neighbours of node a), epnbr [C][10][4] (where vertex b stands among its vertex neighbours), and the residual
    gather's incidences inc_ptr / inc by rank and pinc_ptr / pinc by pressure position, each entry 16 * cell + local node,
    ascending.  Nodes in no cell have empty rows and no incidences."""
    from types import SimpleNamespace
    tn = np.asarray(tet_nodes, dtype=np.int64).reshape(-1, 10)
    rk = np.asarray(rank_of_node, dtype=np.int64)
    C, N2 = len(tn), len(rk)
    assert sorted(rk.tolist()) == list(range(N2)) and tn[:, :4].max() < V <= N2 and tn[:, 4:].min() >= V
    cr = rk[tn]
    order = np.argsort(rk[:V])                                     # vertices in rank order
    prank = np.empty(V, dtype=np.int64)
    prank[order] = np.arange(V)
    vrank = rk[:V][order]
    prow = 6 * N2 + prank[tn[:, :4]]
    dofs = np.empty((C, 64), dtype=np.int64)
    for cmp in range(3):
        dofs[:, 10 * cmp:10 * cmp + 10] = 6 * cr + cmp
        dofs[:, 30 + 10 * cmp:40 + 10 * cmp] = 6 * cr + 3 + cmp
    dofs[:, 60:] = prow
    # the node graph: pairs of ranks that share a cell
    ra, rb = np.repeat(cr[:, :, None], 10, axis=2), np.repeat(cr[:, None, :], 10, axis=1)
    code = np.unique(ra * N2 + rb)
    src, dst = code // N2, code % N2
    nadj_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N2))]).astype(np.int64)
    enbr = np.searchsorted(code, ra * N2 + rb) - nadj_ptr[ra]
    pos_of_rank = np.full(N2, -1, dtype=np.int64)
    pos_of_rank[vrank] = np.arange(V)
    isv = pos_of_rank[dst] >= 0
    pcode = src[isv] * V + pos_of_rank[dst[isv]]                   # ascending: the positions rise with the ranks
    assert np.all(np.diff(pcode) > 0)
    padj_ptr = np.concatenate([[0], np.cumsum(np.bincount(src[isv], minlength=N2))]).astype(np.int64)
    pa, pb = np.repeat(cr[:, :, None], 4, axis=2), np.repeat(prank[tn[:, None, :4]], 10, axis=1)
    epnbr = np.searchsorted(pcode, pa * V + pb) - padj_ptr[pa]
    rowptr, cols, diagpos = expand_cols(N2, nadj_ptr, dst.astype(np.int32), padj_ptr, (pcode % V).astype(np.int32), vrank)
    cell = np.arange(C, dtype=np.int64)

    def incidences(owner, nown, nloc):
        e = (16 * cell[:, None] + np.arange(nloc)).ravel()
        o = np.argsort(owner.ravel(), kind="stable")               # cells ascending inside an owner
        return np.concatenate([[0], np.cumsum(np.bincount(owner.ravel(), minlength=nown))]).astype(np.int64), e[o].astype(np.int32)
    inc_ptr, inc = incidences(cr, N2, 10)
    pinc_ptr, pinc = incidences(prow - 6 * N2, V, 4)
    assert enbr.max() < 65536 and (epnbr.max() if V else 0) < 65536
    return SimpleNamespace(C=C, N2=N2, V=V, ndof=6 * N2 + V, cell_rank=np.ascontiguousarray(cr, dtype=np.int32),
                           cell_prow=np.ascontiguousarray(prow, dtype=np.int32), cell_dofs=np.ascontiguousarray(dofs, dtype=np.int32),
                           nadj_ptr=nadj_ptr, nadj=dst.astype(np.int32), padj_ptr=padj_ptr, padj=(pcode % V).astype(np.int32),
                           vrank=vrank.astype(np.int32), rowptr=rowptr, cols=cols, diagpos=diagpos,
                           enbr=np.ascontiguousarray(enbr, dtype=np.uint16), epnbr=np.ascontiguousarray(epnbr, dtype=np.uint16),
                           inc_ptr=inc_ptr, inc=inc, pinc_ptr=pinc_ptr, pinc=pinc)


def element_positions(es):
    """[C][64][64] position in the monolithic matrix of entry (i, j) of every element matrix (oracle's local order), as k_jacobian
    computes it: rowptr[row] + 6 enbr[a][b] + 3 field + component for the d and v columns, rowptr[row] + 6 deg(a) + epnbr[a][b]
    for the pressure columns, a the local node of row i"""
    i = np.arange(64)
    a = np.where(i < 60, i % 10, i - 60)                           # local node of a row / column
    fc = np.where(i < 60, 3 * (i // 30) + (i % 30) // 10, 0)
    r0 = es.rowptr[es.cell_dofs.astype(np.int64)]                  # [C][64]
    deg6 = 6 * np.diff(es.nadj_ptr)[es.cell_rank.astype(np.int64)]  # [C][10]
    nb = es.enbr.reshape(-1, 10, 10).astype(np.int64)
    pb = es.epnbr.reshape(-1, 10, 4).astype(np.int64)
    pos = np.empty((es.C, 64, 64), dtype=np.int64)
    pos[:, :, :60] = r0[:, :, None] + 6 * nb[:, a][:, :, a[:60]] + fc[None, None, :60]
    pos[:, :, 60:] = r0[:, :, None] + deg6[:, a][:, :, None] + pb[:, a]
    return pos


def geometry_reference(coords, tets):
    """k_geometry's contract in extended precision from the FP64 coordinates: (Jinv [C][3][3] with Jinv[k][j] = d xi_k / d x_j,
    det [C] signed, the edge matrix J [C][3][3] = d x_i / d xi_k), all np.longdouble"""
    x = np.asarray(coords, dtype=LD)[np.asarray(tets, dtype=np.int64)]
    J = np.stack([x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]], axis=2)
    inv, det = inv3(J)
    return inv, det, J


def geometry_fp64(coords, tets):
    """[C][10] the geometry array the element kernels read, rounded from geometry_reference"""
    inv, det, _ = geometry_reference(coords, tets)
    return np.ascontiguousarray(np.concatenate([inv.reshape(-1, 9), np.abs(det)[:, None]], axis=1), dtype=np.float64)


def geometry_bound(coords, tets):
    """(bound on the nine inverse entries [C][3][3], bound on |det| [C]) for the adjugate inverse in FP64 of the FP64 edge matrix:
    inverse_bound's c u |A^-1| |A| |A^-1| with c = 16 for the inverse itself and 1 more for the rounding of the edge differences
    (each entry of A carries at most u |A_ij|, which the inverse passes on as u |A^-1| |A| |A^-1| to first order; the differences
    of the cells moved away from the origin are the case it is there for); the determinant's three products of a rounded
    difference with a rounded cofactor are (2 + 1 + 2 + 1 + 2) u of the sum of the absolute products each, 10 u in all with the
    two additions"""
    inv, det, J = geometry_reference(coords, tets)
    J64 = J.astype(np.float64)
    a = np.abs(J64)
    perm = (a[:, 0, 0] * (a[:, 1, 1] * a[:, 2, 2] + a[:, 1, 2] * a[:, 2, 1]) + a[:, 0, 1] * (a[:, 1, 0] * a[:, 2, 2] + a[:, 1, 2] * a[:, 2, 0])
            + a[:, 0, 2] * (a[:, 1, 0] * a[:, 2, 1] + a[:, 1, 1] * a[:, 2, 0]))
    return inverse_bound(J64, inv, U64, c=17.0), 10.0 * U64 * perm


def elem_params(desc):
    """(sc [5], fluid [8][2], solid [8][7]) of a description as the shim's ElemParams arrays"""
    sc = np.array([desc["dt"], desc["theta"], 1.0 - desc["theta"], DELTA_S, ALPHA_L])
    fluid, solid = np.zeros((8, 2)), np.zeros((8, 7))
    for r, p in enumerate(desc["fluid_props"]):
        fluid[r] = p
    models = desc.get("solid_models", [0] * len(desc["solid_props"]))
    for r, p in enumerate(desc["solid_props"]):
        p = tuple(p) + (0.0,) * (6 - len(p))
        solid[r] = p[:3] + (float(models[r]),) + p[3:6]
    return sc, fluid, solid


# Two fluid and three solid regions, so that region > 0 and model == 1 are read
ELEMENT_FLUIDS = [(1000.0, 3.5e-3), (1060.0, 4.2e-3)]
ELEMENT_SOLIDS = [(1000.0, 344827.6, 3103448.3, 0.0, 0.0, 0.0), (1200.0, 5.0e5, 2.0e6, 0.0, 0.0, 0.0),
                  (1100.0, 3.0e5, 2.0e6, 1.0e5, 5.0e4, 1.0e4)]
ELEMENT_MODELS = [0, 0, 1]


class ElementCase:
    """A cell list with everything one launch of an element kernel takes and everything its reference needs: the P2 mesh (coords,
    node_coords, tets, tet_nodes), kinds and regions, a random node -> rank permutation with its element_structure (es), the FP64
    geometry array the kernel and the reference both start from, the materials above, and a state scaled as random_state of
    tests/test_gpu_parity.py, in the oracle's layout (U, U1) and in the solver's (Us, U1s)."""

    def __init__(self, coords, tets, kind, region, seed, theta=0.51, dt=1.0e-3, node_coords=None, tet_nodes=None):
        from vasp_amd.mesh import FsiMesh
        rng = np.random.default_rng(seed)
        if tet_nodes is None:
            m = FsiMesh.from_arrays(coords, tets, np.asarray(kind) + 1)
            assert np.array_equal(m.tets, tets), "cells must be vertex-sorted"
            node_coords, tet_nodes = m.node_coords, m.tet_nodes
        self.coords, self.tets = np.ascontiguousarray(coords, dtype=np.float64), np.ascontiguousarray(tets, dtype=np.int64)
        self.node_coords, self.tet_nodes = node_coords, np.ascontiguousarray(tet_nodes, dtype=np.int64)
        self.kind, self.region = np.ascontiguousarray(kind, dtype=np.int32), np.ascontiguousarray(region, dtype=np.int32)
        self.C, self.V, self.N2 = len(self.tets), len(self.coords), len(node_coords)
        self.rank = rng.permutation(self.N2)
        self.es = element_structure(self.tet_nodes, self.V, self.rank)
        self.geom = geometry_fp64(self.coords, self.tets)
        self.desc = dict(coords=self.coords, tets=self.tets, tet_nodes=self.tet_nodes, num_nodes=self.N2, cell_kind=self.kind,
                         cell_region=self.region, fluid_props=ELEMENT_FLUIDS, solid_props=ELEMENT_SOLIDS,
                         solid_models=ELEMENT_MODELS, dt=dt, theta=theta)
        self.params = elem_params(self.desc)
        # h: the smallest altitude of any cell (1 / |grad lambda_k|), so that displacements of 0.02 h keep det(I + grad d) > 0 in
        # flat cells too (the Mooney-Rivlin energy has a logarithm of it)
        gl = self.geom[:, :9].reshape(-1, 3, 3)
        gl = np.concatenate([-gl.sum(axis=1, keepdims=True), gl], axis=1)
        h = float(1.0 / np.sqrt((gl ** 2).sum(axis=2)).max())
        N2, ndof = self.N2, 6 * self.N2 + self.V
        U, U1 = np.zeros(ndof), np.zeros(ndof)
        U[:3 * N2] = 0.02 * h * rng.standard_normal(3 * N2)
        U1[:3 * N2] = U[:3 * N2] + 0.002 * h * rng.standard_normal(3 * N2)
        U[3 * N2:6 * N2] = 0.1 * rng.standard_normal(3 * N2)
        U1[3 * N2:6 * N2] = U[3 * N2:6 * N2] + 0.01 * rng.standard_normal(3 * N2)
        U[6 * N2:] = 10 * rng.standard_normal(self.V)
        U1[6 * N2:] = U[6 * N2:] + rng.standard_normal(self.V)
        self.U, self.U1 = U, U1
        self.user_dofs = self.user_cell_dofs(self.tet_nodes, self.tets, N2)
        self.Us, self.U1s = self.to_solver(U), self.to_solver(U1)

    @staticmethod
    def user_cell_dofs(tn, tets, N2):
        cols = [off + 3 * tn + c for off in (0, 3 * N2) for c in range(3)]
        return np.concatenate(cols + [6 * N2 + tets], axis=1)

    def to_solver(self, X):
        """a vector in the oracle's layout in the solver's; dofs of nodes in no cell are dropped (they stay 0)"""
        Y = np.zeros(self.es.ndof, dtype=X.dtype)
        Y[self.es.cell_dofs.ravel()] = X[self.user_dofs.ravel()]
        return Y

    def prefix(self, C):
        """the first C cells on the same nodes, ranks and state (the other nodes then lie in no cell)"""
        return self.subset(np.arange(C))

    def subset(self, cells):
        """the listed cells as a case of their own (same nodes, ranks and state)"""
        import copy
        cells = np.asarray(cells, dtype=np.int64)
        s = copy.copy(self)
        s.C, s.tets, s.tet_nodes, s.kind, s.region, s.geom = (len(cells), self.tets[cells], self.tet_nodes[cells], self.kind[cells],
                                                              self.region[cells], self.geom[cells])
        s.es = element_structure(s.tet_nodes, self.V, self.rank)
        s.user_dofs = self.user_dofs[cells]
        s.desc = dict(self.desc, tets=s.tets, tet_nodes=s.tet_nodes, cell_kind=s.kind, cell_region=s.region)
        s.Us, s.U1s = s.to_solver(self.U), s.to_solver(self.U1)
        return s

    def with_theta(self, theta):
        import copy
        s = copy.copy(self)
        s.desc = dict(self.desc, theta=theta)
        s.params = elem_params(s.desc)
        return s

    def oracle(self, dtype=np.float64, impl="numpy", given_geometry=True):
        """the project's oracle on this case: numpy in `dtype` from the case's FP64 geometry array, or (impl "c") the C restatement,
        which derives its geometry from the coordinates"""
        from oracle.fsi_oracle import FsiOracle
        if impl == "c":
            o = FsiOracle(self.desc)
            assert o.c is not None, "the C oracle is not available"
            return o
        return FsiOracle(self.desc, impl="numpy", dtype=dtype, geom=self.geom if given_geometry else None)

    def residual_reference(self, o=None):
        """[C][64] R_linear + R_nonlinear of the oracle `o` (default: extended precision from the FP64 geometry array), oracle order"""
        o = o or self.oracle(LD)
        Rl, Rn = o.element_residuals(self.U.astype(o.dtype), self.U1.astype(o.dtype))
        return Rl + Rn

    def jacobian_reference(self, o=None):
        """([C][64][64] J_linear, J_nonlinear) of the oracle `o` (default: complex step in extended precision)"""
        o = o or self.oracle(LD)
        return o.element_jacobians(self.U.astype(o.dtype), self.U1.astype(o.dtype))


def tube_case(target, seed, theta=0.51):
    """ElementCase on vasp_amd.meshgen.generate(target): a conforming tube of fluid cells in a solid wall; regions by cell index"""
    from vasp_amd import meshgen
    m = meshgen.generate(target)
    C = len(m["tets"])
    kind = (m["cell_markers"] == 2).astype(np.int32)
    region = np.where(kind == 0, np.arange(C) % 2, np.arange(C) % 3)
    return ElementCase(m["coords"], m["tets"], kind, region, seed, theta=theta)


def hand_case(C, seed, theta=0.51, size=1.0e-3):
    """1, 2 or 3 hand-built cells: a strip of tetrahedra on six points, a fluid cell, a solid Mooney-Rivlin cell and a solid
    St. Venant-Kirchhoff cell in region 1; the cells' orientations alternate"""
    pts = size * np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.3, 0.2, 1.1], [1.2, 1.0, 0.9], [0.1, 1.1, 1.3]])
    tets = np.array([[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5]])[:C]
    kind, region = np.array([0, 1, 1])[:C], np.array([1, 2, 1])[:C]
    return ElementCase(pts[:C + 3], tets, kind, region, seed, theta=theta)


def node_disjoint(tet_nodes, cells=None, limit=None):
    """Greedy colouring of the cells (in the order given) into lists that share no node: [lists of cell ids].  With `limit`, stop
    once that many cells are placed."""
    tn = np.asarray(tet_nodes, dtype=np.int64)
    cells = np.arange(len(tn)) if cells is None else np.asarray(cells)
    used, lists, placed = [], [], 0
    for c in cells:
        nodes = set(tn[c].tolist())
        for k, u in enumerate(used):
            if not (u & nodes):
                u |= nodes
                lists[k].append(int(c))
                break
        else:
            used.append(set(nodes))
            lists.append([int(c)])
        placed += 1
        if limit and placed >= limit:
            break
    return lists


# The block bound.  For a cell and a block B (the d, v or p rows of its element vector; a (row field, column field) pair of its
# element matrix) a kernel must satisfy |got - ref| <= K_B 2^-53 max_B |ref| against the oracle in extended precision, both from the
# same FP64 geometry array, tables and state.  K_B = 4 x the larger of the two ratios the oracle's own FP64 evaluation orders reach
# on the tests' inputs (numpy from the given geometry; C from the coordinates, against the extended-precision evaluation from the
# coordinates), rounded up; the factor 4 covers a third summation order, FMA contraction and the pull-back of the gradient slots
# to reference coordinates.  Measured on the CPU with measure_block_ratios() on block_ratio_cases(); the figures are in the
# comments, tests/test_kernel_references.py asserts that both FP64 oracles stay within K_B / 4.  Index: [kind][block], kind 0 fluid,
# 1 solid; residual blocks 0 d, 1 v, 2 p rows; Jacobian blocks [part][kind][row field][column field].  A block that is zero in the
# reference has K = 0: the kernel must leave an exact zero (or, in the matrix, the prefill) there.
def block_ratios(got, ref, kind):
    """largest |got - ref| / (2^-53 max_B |ref|) per kind and block over the cells: vectors [C][64] -> [2][3]; matrices [C][64][64]
    -> [2][3][3]; blocks the reference has zero count as 0 when got is zero too, else inf"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    mat = ref.ndim == 3
    out = np.zeros((2, 3, 3) if mat else (2, 3))
    for k in (0, 1):
        sel = np.flatnonzero(np.asarray(kind) == k)
        if not len(sel):
            continue
        for bi, rs in enumerate(FIELD_SLICES):
            for bj, cs in enumerate(FIELD_SLICES if mat else (None,)):
                g, r = (got[sel][:, rs, cs], ref[sel][:, rs, cs]) if mat else (got[sel][:, rs], ref[sel][:, rs])
                ax = tuple(range(1, r.ndim))
                err, mx = np.abs(g - r).max(axis=ax), np.abs(r).max(axis=ax)
                with np.errstate(divide="ignore", invalid="ignore"):
                    q = np.where(err == 0, 0, err / (U64 * mx))
                q = float(np.where(np.isnan(q), np.inf, q).max())
                if mat:
                    out[k, bi, bj] = q
                else:
                    out[k, bi] = q
    return out


def block_bound(ref, kind, K):
    """K_B 2^-53 max_B |ref| spread over the entries: [C][64] for K [2][3], [C][64][64] for K [2][3][3]"""
    ref = np.abs(np.asarray(ref, dtype=LD))
    K = np.asarray(K, dtype=np.float64)
    kind = np.asarray(kind, dtype=np.int64)
    b = np.zeros(ref.shape, dtype=LD)
    for bi, rs in enumerate(FIELD_SLICES):
        if ref.ndim == 2:
            b[:, rs] = (K[kind, bi] * U64 * ref[:, rs].max(axis=1))[:, None]
        else:
            for bj, cs in enumerate(FIELD_SLICES):
                b[:, rs, cs] = (K[kind, bi, bj] * U64 * ref[:, rs, cs].max(axis=(1, 2)))[:, None, None]
    return b


_cases = {}


def element_cases(name):
    """The inputs of the element-kernel tests, built once per process.  "tube": the 6000-cell tube, theta 0.51; "tube_theta1": every
    15th of its cells with theta = 1 (th1 == 0); "hand3" / "hand3_theta1": the three hand-built cells; "big": the 48000-cell tube;
    "jac": up to 192 cells of the tube that share no node, fluid and solid cells alternating, every region among them"""
    if name not in _cases:
        if name == "tube":
            _cases[name] = tube_case(6000, seed=11)
        elif name == "tube_theta1":
            t = element_cases("tube")
            _cases[name] = t.with_theta(1.0).subset(np.arange(0, t.C, 15))
        elif name == "hand3":
            _cases[name] = hand_case(3, seed=5)
        elif name == "hand3_theta1":
            _cases[name] = hand_case(3, seed=6, theta=1.0)
        elif name == "big":
            _cases[name] = tube_case(48000, seed=12)
        elif name == "jac":
            t = element_cases("tube")
            fl, so = np.flatnonzero(t.kind == 0), np.flatnonzero(t.kind == 1)
            mixed = np.stack([fl[:len(so)], so], axis=1).ravel()          # fluid and solid cells in turn
            _cases[name] = t.subset(np.array(node_disjoint(t.tet_nodes, mixed)[0][:192]))
            assert _cases[name].C >= 150
        else:
            raise KeyError(name)
    return _cases[name]


RESIDUAL_RATIO_CASES = ("tube", "tube_theta1", "hand3", "hand3_theta1")


def measure_residual_ratios(names=RESIDUAL_RATIO_CASES):
    """{oracle: [2][3]} the largest block ratio of the oracle's two FP64 evaluation orders against extended precision over the cases"""
    out = {"numpy": np.zeros((2, 3)), "c": np.zeros((2, 3))}
    for n in names:
        case = element_cases(n)
        ref = case.residual_reference()
        out["numpy"] = np.maximum(out["numpy"], block_ratios(case.residual_reference(case.oracle(np.float64)), ref, case.kind))
        out["c"] = np.maximum(out["c"], block_ratios(case.residual_reference(case.oracle(impl="c")), ref, case.kind))
    return out


def measure_jacobian_ratios():
    """{oracle: [2 parts][2][3][3]} the same for the element matrices of the "jac" case"""
    case = element_cases("jac")
    ref = case.jacobian_reference()
    out = {}
    for name, o in (("numpy", case.oracle(np.float64)), ("c", case.oracle(impl="c"))):
        J = case.jacobian_reference(o)
        out[name] = np.stack([block_ratios(J[p], ref[p], case.kind) for p in (0, 1)])
    return out


# CPU-measured ratios (measure_residual_ratios(), numpy / C, per kind the d, v, p rows) and K = 4 x the larger, rounded up to a
# multiple of 4 that leaves the measurement a tenth of room under K / 4 (another compiler or numpy may move its last digit):
#   fluid  4.5 / 7.6 -> 36     8.5 / 9.8 -> 44     6.8 / 20.7 -> 92
#   solid  5.4 / 10.8 -> 48    84.7 / 92.2 -> 408 (the strain E = (F^T F - I) / 2 of a 2 % deformation cancels two digits before the
#          stiffness multiplies it)                 p rows: zero
K_RESIDUAL = np.array([[36.0, 44.0, 92.0], [48.0, 408.0, 0.0]])
# measure_jacobian_ratios(), [part linear / nonlinear][kind][row field][column field]; the blocks not named are zero in the reference:
#   linear     fluid (d,d) 3.8 / 6.0 -> 28   (v,v) 5.0 / 5.9 -> 28
#              solid (d,d) 5.1 / 12.6 -> 56  (d,v) 6.4 / 12.8 -> 56  (v,v) 5.5 / 13.8 -> 64
#   nonlinear  fluid (v,d) 5.1 / 6.4 -> 28   (v,v) 3.9 / 4.5 -> 20   (v,p) 3.6 / 5.1 -> 24   (p,d) 4.8 / 6.0 -> 28   (p,v) 4.1 / 5.3 -> 24
#              solid (v,d) 4.9 / 12.3 -> 56
# On an MI355X every block of every kernel stayed below half of its bound against the extended-precision reference (the figures are
# in the headers of the two test files), so no constant had to be explained or touched.
K_JACOBIAN = np.zeros((2, 2, 3, 3))
K_JACOBIAN[0, 0, 0, 0], K_JACOBIAN[0, 0, 1, 1] = 28.0, 28.0
K_JACOBIAN[0, 1, 0, 0], K_JACOBIAN[0, 1, 0, 1], K_JACOBIAN[0, 1, 1, 1] = 56.0, 56.0, 64.0
K_JACOBIAN[1, 0, 1] = (28.0, 20.0, 24.0)
K_JACOBIAN[1, 0, 2, :2] = (28.0, 24.0)
K_JACOBIAN[1, 1, 1, 0] = 56.0


def sequential_gather(Re, ptr, lst, mul, off):
    """k_residual_gather's sum in FP64, by a loop over the incidences in the order of the list: out[r][t] = the entries
    Re[cell][mul * local + off + t] of owner r's incidences added one after the other to 0.0 (t < mul)"""
    Re = np.asarray(Re, dtype=np.float64).reshape(-1, 64)
    n = len(ptr) - 1
    deg = np.diff(ptr)
    s = np.zeros((n, mul))
    for k in range(int(deg.max()) if n else 0):
        live = np.flatnonzero(deg > k)
        e = np.asarray(lst, dtype=np.int64)[ptr[live] + k]
        s[live] = s[live] + Re[e >> 4][np.arange(len(live))[:, None], (mul * (e & 15) + off)[:, None] + np.arange(mul)]
    return s


def assembled(es, elem_vals, absolute=False):
    """sum of the element vectors [C][64] (oracle order) into the solver-layout vector, in extended precision"""
    out = np.zeros(es.ndof, dtype=LD)
    v = np.asarray(elem_vals, dtype=LD)
    np.add.at(out, es.cell_dofs.astype(np.int64).ravel(), (np.abs(v) if absolute else v).ravel())
    return out


def l2_reference(case, X):
    """(value, bound) of launch_l2norm: the Keast-24 integral of |d|^2 + |v|^2 + p^2 over the cells from the FP64 tables, geometry
    weights and state, in extended precision.  Bound (terms + c) u sum |terms| with the squares of the absolute interpolations as
    the terms: 2 x (10 products and additions + 1) for a squared P2 value, 7 additions of squares, 3 factors of the weight, and the
    additions of the reduction (cells per wave, 6 shuffle steps, 2 per workgroup, blocks / 256 + 8 in k_sum_parts); c = 8"""
    from oracle.fsi_oracle import keast24, tabulate_p2
    qp, qw = keast24()
    N, _, L, _ = tabulate_p2(qp)
    N, L, qw = N.astype(LD), L.astype(LD), qw.astype(LD)
    loc = np.asarray(X, dtype=LD)[case.es.cell_dofs.astype(np.int64)]             # [C][64]
    w = case.geom[:, 9].astype(LD)[:, None] * qw[None, :]
    f = loc[:, :60].reshape(-1, 6, 10)
    val, vabs = np.einsum("qa,cfa->cqf", N, f), np.einsum("qa,cfa->cqf", np.abs(N), np.abs(f))
    p, pabs = np.einsum("qa,ca->cq", L, loc[:, 60:]), np.einsum("qa,ca->cq", np.abs(L), np.abs(loc[:, 60:]))
    value = (w * ((val ** 2).sum(axis=2) + p ** 2)).sum()
    T = (w * ((vabs ** 2).sum(axis=2) + pabs ** 2)).sum()
    blocks = min((case.C + 3) // 4, 4096)
    terms = 2 * 11 + 7 + 3 + -(-case.C // (4 * blocks)) + 6 + 2 + -(-blocks // 256) + 8
    return value, (terms + 8) * U64 * T


def cell_stats_reference(case, X):
    """launch_cell_stats per cell, in extended precision: (mean |v| [C], its bound, mean det(I + grad d) [C], its bound).  Bounds
    (terms + c) u sum |terms| over the absolute interpolations: |v| from three 10-term sums, 3 squares, a root and the weight
    (10 + 3 + 3 + 2), the determinant from gradients of 30 terms of 3-term physical gradients and the 6 products of the cofactor
    expansion (33 + 3 + 9), then the 24 weighted points through 6 shuffle steps (+ 8); c = 8"""
    from oracle.fsi_oracle import keast24, tabulate_p2
    qp, qw = keast24()
    N, dN, _, _ = tabulate_p2(qp)
    N, dN, wq = N.astype(LD), dN.astype(LD), 6.0 * qw.astype(LD)
    es = case.es
    loc = np.asarray(X, dtype=LD)[es.cell_dofs.astype(np.int64)]
    d = loc[:, :30].reshape(-1, 3, 10)
    v = loc[:, 30:60].reshape(-1, 3, 10)
    Jinv = case.geom[:, :9].astype(LD).reshape(-1, 3, 3)
    G, Gabs = np.einsum("qak,ckj->cqaj", dN, Jinv), np.einsum("qak,ckj->cqaj", np.abs(dN), np.abs(Jinv))
    vq, vqa = np.einsum("qa,cia->cqi", N, v), np.einsum("qa,cia->cqi", np.abs(N), np.abs(v))
    sv = (wq * np.sqrt((vq ** 2).sum(axis=2))).sum(axis=1)
    bv = (18 + 8 + 8) * U64 * (wq * np.sqrt((vqa ** 2).sum(axis=2))).sum(axis=1)
    F = np.eye(3, dtype=LD) + np.einsum("cia,cqaj->cqij", d, G)
    Fa = np.eye(3, dtype=LD) + np.einsum("cia,cqaj->cqij", np.abs(d), Gabs)
    det = (F[..., 0, 0] * (F[..., 1, 1] * F[..., 2, 2] - F[..., 1, 2] * F[..., 2, 1])
           - F[..., 0, 1] * (F[..., 1, 0] * F[..., 2, 2] - F[..., 1, 2] * F[..., 2, 0])
           + F[..., 0, 2] * (F[..., 1, 0] * F[..., 2, 1] - F[..., 1, 1] * F[..., 2, 0]))
    perm = (Fa[..., 0, 0] * (Fa[..., 1, 1] * Fa[..., 2, 2] + Fa[..., 1, 2] * Fa[..., 2, 1])
            + Fa[..., 0, 1] * (Fa[..., 1, 0] * Fa[..., 2, 2] + Fa[..., 1, 2] * Fa[..., 2, 0])
            + Fa[..., 0, 2] * (Fa[..., 1, 0] * Fa[..., 2, 1] + Fa[..., 1, 1] * Fa[..., 2, 0]))
    sj = (wq * det).sum(axis=1)
    bj = (45 + 8 + 8) * U64 * (wq * perm).sum(axis=1)
    return sv, bv, sj, bj


def probe_reference(case, cells, bary, X):
    """launch_probe: (values [n][7] = d, v, p at the barycentric coordinates, bound) in extended precision; the basis from the FP64
    coordinates (2 roundings each), 10 products and additions: (10 + 4) u sum |N| |X| (pressure: 4 + 2)"""
    l = np.asarray(bary, dtype=LD).reshape(-1, 4)
    Nb = np.concatenate([l * (2 * l - 1), 4 * l[:, [e[0] for e in UFC_EDGES]] * l[:, [e[1] for e in UFC_EDGES]]], axis=1)
    loc = np.asarray(X, dtype=LD)[case.es.cell_dofs.astype(np.int64)[np.asarray(cells, dtype=np.int64)]]
    f = loc[:, :60].reshape(-1, 6, 10)
    val = np.concatenate([np.einsum("na,nfa->nf", Nb, f), np.einsum("na,na->n", l, loc[:, 60:])[:, None]], axis=1)
    ab = np.concatenate([14 * U64 * np.einsum("na,nfa->nf", np.abs(Nb), np.abs(f)),
                         6 * U64 * np.einsum("na,na->n", np.abs(l), np.abs(loc[:, 60:]))[:, None]], axis=1)
    return val, ab


# ---- the host side of the recycled GCR (fsi_gcr_host.hpp), restated ----------------------------------------------------------------
GCR_WINDOW = 32              # columns of the FP64 window
GCR_FLUSH_BATCH = 32         # directions made before a flush


def gcr_ring(cap):
    return min(64, cap // 2)


def gcr_retire_batch(cap):
    return max(1, min(32, cap // 4))


class GcrStoreRef:
    """GcrStore: slots of the kept directions.  born[slot] is the creation index of the direction in the slot (-1: free); a new
    direction takes the free list's back, else the high-water mark hw; a full store retires the `batch` oldest directions born
    at or after cap - ring; the window (a ring of GCR_WINDOW columns) mirrors the latest directions and loses retired ones."""

    def __init__(self, cap):
        self.cap = cap
        self.reset()

    def reset(self):
        self.born = [-1] * self.cap
        self.free = []
        self.hw = self.made = 0
        self.clear_window()

    def clear_window(self):
        self.hot = [-1] * GCR_WINDOW
        self.hot_next = 0

    def full(self):
        return not self.free and self.hw == self.cap

    def take(self):
        """(slot, whether its column has never been written and must be cleared)"""
        if self.free:
            return self.free.pop(), False
        self.hw += 1
        return self.hw - 1, True

    def set_born(self, slot):
        self.born[slot] = self.made
        self.made += 1

    def retire(self, batch):
        protect = self.cap - gcr_ring(self.cap)
        cand = sorted((b, s) for s, b in enumerate(self.born[:self.hw]) if b >= protect)
        out = [s for _, s in cand[:batch]]
        for s in out:
            self.born[s] = -1
            self.free.append(s)
        return out

    def window_cols(self):
        return max([k + 1 for k in range(GCR_WINDOW) if self.hot[k] >= 0], default=0)

    def window_put(self, slot):
        col = self.hot_next
        self.hot[col] = slot
        self.hot_next = (col + 1) % GCR_WINDOW
        return col

    def window_drop_retired(self):
        out = [k for k in range(GCR_WINDOW) if self.hot[k] >= 0 and self.born[self.hot[k]] < 0]
        for k in out:
            self.hot[k] = -1
        return out

    def state(self):
        return list(self.born), list(self.free), list(self.hot), (self.hw, self.made, self.hot_next)


GCR_STORE_OPS = {"init": 0, "full": 1, "take": 2, "retire": 3, "window_put": 4, "window_drop_retired": 5, "set_born": 6,
                 "window_cols": 7, "reset": 8, "clear_window": 9}


def gcr_store_op(cap, op, arg=0):
    """one operation on the shim's GcrStore: (its result as a list of ints, the store's state as GcrStoreRef.state() gives it)"""
    res = np.full(cap + 2, -7, dtype=np.int32)
    born, free, hot = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int32), np.zeros(GCR_WINDOW, dtype=np.int32)
    scal = np.zeros(4, dtype=np.int64)
    call("shim_gcr_store_op", GCR_STORE_OPS[op], arg, res, born, free, hot, scal)
    if op in ("retire", "window_drop_retired"):
        out = [int(v) for v in res[1:1 + res[0]]]
    elif op == "take":
        out = [int(res[0]), int(res[1])]
    else:
        out = [int(res[0])]
    return out, ([int(v) for v in born], [int(v) for v in free[:scal[3]]], [int(v) for v in hot], tuple(int(v) for v in scal[:3]))


def gcr_cycle_reference(cap, Z, slots, ms, htot, wn, alpha):
    """GcrCycle's algebra in extended precision.  Z [cap][n]: what the slots hold - an explicit direction in an older slot, the
    raw preconditioned vector in a slot of this cycle.  Direction k, stored in slots[k] after coefficients htot[k][:ms[k]], is
        p_k = (Z[slots[k]] - sum_j htot[k][j] P_j) / wn[k],   P_j = p_k' if slots[k'] = j for an earlier k', else Z_j
    (j = slots[k] and zero coefficients are left out), and x moves by sum_k alpha[k] p_k.  Returns (P [knew][n], X [n], and a
    function bound(cn) -> (EP [knew][n], EX [n]) from the coefficient columns the library computed).

    Bound: the library builds c_k[j] = (delta - sum_k' h_k' c_k'[j] - h_j) / wn in FP64: one rounding per addition into the
    entry, one for the product, one for the division, so its own error is at most (additions + 2) 2^-52 times the sum of the
    absolute values of the terms (2^-52: twice the unit round-off), and it inherits sum_k' |h_k'| E_k'[j] / wn from the
    earlier directions of the cycle.  y[j] += alpha_k c_k[j]: knew additions and a product, on top of |alpha_k| E_k[j]."""
    Z = np.asarray(Z, dtype=LD)
    knew = len(slots)
    P = np.zeros((knew, Z.shape[1]), dtype=LD)
    newest = {}
    terms = []                   # per direction: [(coefficient h, earlier direction k' or None, column j)]
    for k in range(knew):
        acc = Z[slots[k]].copy()
        tk = []
        for j in range(ms[k]):
            h = htot[k][j]
            if h == 0.0 or j == slots[k]:
                continue
            acc -= LD(h) * (P[newest[j]] if j in newest else Z[j])
            tk.append((float(h), newest.get(j), j))
        P[k] = acc / LD(wn[k])
        newest[slots[k]] = k
        terms.append(tk)
    X = sum((LD(alpha[k]) * P[k] for k in range(knew)), np.zeros(Z.shape[1], dtype=LD))

    def bound(cn):
        cn = np.abs(np.asarray(cn, dtype=np.float64))
        EC = np.zeros((knew, cap))
        for k in range(knew):
            adds, mag, inherit = np.zeros(cap), np.zeros(cap), np.zeros(cap)
            mag[slots[k]] = 1.0
            for h, kp, j in terms[k]:
                if kp is None:
                    adds[j] += 1
                    mag[j] += abs(h)
                else:
                    adds += 1
                    mag += abs(h) * cn[kp]
                    inherit += abs(h) * EC[kp]
            EC[k] = ((adds + 2) * 2.0 ** -52 * mag + inherit) / abs(wn[k])
        a = np.abs(np.asarray(alpha, dtype=np.float64))
        EY = (knew + 2) * 2.0 ** -52 * (a[:, None] * cn).sum(axis=0) + (a[:, None] * EC).sum(axis=0)
        absZ = np.abs(Z).astype(np.float64)
        return EC @ absZ, EY @ absZ
    return P, X, bound


def gcr_cycle_end_ref(since_gain, f32, rnorm, target, r_entry, store_full):
    """0 go, 1 stagnated, 2 stalled (gcr_cycle_end)"""
    if since_gain >= 40 and (f32 or rnorm <= 100.0 * target):
        return 1
    if f32 and since_gain >= 6 and rnorm <= 1e-4 * r_entry:
        return 1
    if since_gain >= 128 and store_full:
        return 2
    return 0


def gcr_orth_lost_ref(h, w2, wn2, floor):
    if not (wn2 > 0.0 and w2 > 0.0):
        return False
    hsq = 0.0
    for v in h:
        hsq += v * v
    return abs(wn2 - (w2 - hsq)) / wn2 / np.sqrt(w2 / wn2) > floor


def gcr_verdict_due_ref(rtol, rnorm, bnorm, cyc, cycle_its, stagnated, stalled, store_full, fell_back, suspect):
    return bool(rtol < 1e-8 or fell_back or store_full or cycle_its > 64 or stalled or stagnated or suspect or cyc > 0
                or rnorm > rtol * bnorm)


def gcr_verdict_skippable_ref(rtol, rnorm, bnorm, cyc, cycle_its, stagnated, stalled, store_full, in_newton, final_cycle, skip_rtol,
                              last_drift):
    return bool(in_newton and final_cycle and rtol >= skip_rtol and rnorm <= rtol * bnorm and cycle_its <= GCR_WINDOW
                and not stagnated and 0.0 <= last_drift <= 0.01 * rtol)
