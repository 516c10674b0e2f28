"""ctypes binding of ``libvaspfsi.so`` (``include/vaspfsi.h``) and the backend the time-step driver uses.

There is no CPU fallback: if the HIP library has not been built, or no GPU is visible, constructing a
``HipBackend`` raises.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import List, Optional

import numpy as np

LIB_PATH = Path(__file__).resolve().parent / "libvaspfsi.so"

FSI_OK = 0
ERROR_NAMES = {1: "FSI_ERR_INVALID", 2: "FSI_ERR_DEVICE", 3: "FSI_ERR_DIVERGED", 4: "FSI_ERR_LINEAR", 5: "FSI_ERR_PIVOT"}

EXPORTED_SYMBOLS = (
    "fsi_create", "fsi_destroy", "fsi_last_error", "fsi_set_dirichlet", "fsi_set_dirichlet_values",
    "fsi_set_pressure_facets", "fsi_set_interface_pressure", "fsi_set_robin_facets", "fsi_solver_setup",
    "fsi_assemble_residual", "fsi_assemble_jacobian", "fsi_solve", "fsi_newton_solve", "fsi_shift",
    "fsi_get_state", "fsi_set_state", "fsi_set_frame", "fsi_num_dofs", "fsi_matrix_nnz", "fsi_device_memory", "fsi_apply_preconditioner", "fsi_get_matrix", "fsi_spmv",
    "fsi_get_timers", "fsi_get_solver_events", "fsi_xcd_order", "fsi_bcr_plan_graph", "fsi_solid_coarse_info", "fsi_solid_coarse_matrix", "fsi_solid_coarse_solve", "fsi_get_values", "fsi_stress_strain", "fsi_wall_shear_stress", "fsi_hemo_begin", "fsi_hemo_sample", "fsi_hemo_indices", "fsi_hemo_export", "fsi_hemo_import", "fsi_hemo_end", "fsi_stress_begin", "fsi_stress_sample", "fsi_stress_averages", "fsi_stress_export", "fsi_stress_import", "fsi_stress_end", "fsi_band_begin", "fsi_band_begin_cells", "fsi_band_sample", "fsi_band_filter", "fsi_band_select", "fsi_band_filter_next", "fsi_band_trace", "fsi_band_amplitude", "fsi_band_phase", "fsi_band_phase_fetch", "fsi_band_spi", "fsi_band_spi_fetch", "fsi_band_pod_gram", "fsi_band_pod_modes", "fsi_band_pod_fetch", "fsi_band_cells", "fsi_band_cell_rate", "fsi_band_cell_rate_current", "fsi_band_cell_weights", "fsi_band_cell_vortex", "fsi_band_cell_vortex_current", "fsi_band_fetch", "fsi_band_export", "fsi_band_import", "fsi_band_end", "fsi_band_room", "fsi_board_begin", "fsi_board_end", "fsi_band_board_attach", "fsi_board_table", "fsi_order_statistics", "fsi_spec_begin", "fsi_spec_begin_rows", "fsi_spec_begin_wss", "fsi_spec_room", "fsi_spec_sample", "fsi_spec_filter", "fsi_spec_fetch", "fsi_spec_spectrogram", "fsi_spec_periodogram", "fsi_spec_spectrogram_sum", "fsi_spec_periodogram_sum", "fsi_spec_export", "fsi_spec_import", "fsi_spec_end", "fsi_calibration_streams", "fsi_set_newton_forcing", "fsi_set_linear_solver", "fsi_set_chebyshev", "fsi_probe", "fsi_flow_stats", "fsi_set_partition",
    "fsi_rccl_unique_id", "fsi_set_rccl", "fsi_create_tuned", "fsi_get_tuning", "fsi_tuning_defaults", "fsi_tuning_from_env", "fsi_tuning_copy_out",
)


class FsiMeshDesc(C.Structure):
    _fields_ = [("num_vertices", C.c_int64), ("num_nodes", C.c_int64), ("num_cells", C.c_int64),
                ("coords", C.c_void_p), ("tet_nodes", C.c_void_p), ("cell_kind", C.c_void_p),
                ("cell_region", C.c_void_p)]


class FsiParams(C.Structure):
    _fields_ = [("dt", C.c_double), ("theta", C.c_double), ("num_fluid_regions", C.c_int32),
                ("fluid_props", C.c_void_p), ("num_solid_regions", C.c_int32), ("solid_props", C.c_void_p),
                ("solid_models", C.c_void_p), ("delta", C.c_double), ("laplace_alpha", C.c_double)]


class FsiTuning(C.Structure):
    """include/vaspfsi.h: every product option of a context (storage precisions, sizes, Newton / Krylov policy, the
    preconditioner's structure and sweep counts).  ``HipBackend(desc, tuning={"krylov_fp32": 0, ...})`` starts from the
    library's defaults with the environment's FSI_<NAME> overrides and sets the named fields."""
    _fields_ = [("struct_size", C.c_int32), ("krylov_fp32", C.c_int32), ("operator_fp32", C.c_int32), ("schur_fp32", C.c_int32),
                ("sweeps_fp32", C.c_int32), ("sweeps_fp16", C.c_int32), ("solid_fp32", C.c_int32), ("pv_fp32", C.c_int32),
                ("krylov_capacity", C.c_int32), ("krylov_fp32_floor", C.c_double),
                ("assembly_atomic", C.c_int32), ("node_order", C.c_int32), ("tiles", C.c_int32), ("tile_nodes", C.c_int32), ("schur_tile_rows", C.c_int32), ("jacobian_waves", C.c_int32),
                ("jacobian_mfma", C.c_int32),
                ("newton_forcing", C.c_double), ("newton_forcing_late", C.c_double), ("newton_late_factor", C.c_double),
                ("f32_cycle_floor", C.c_double), ("f32_verdict_skip_rtol", C.c_double), ("orth_floor32", C.c_double),
                ("orth_floor64", C.c_double), ("gcr_escape", C.c_double), ("gcr_reorth", C.c_double),
                ("prec_streams", C.c_int32), ("experiment", C.c_int32), ("cheb4", C.c_int32), ("coarse_power", C.c_int32), ("solid_mg", C.c_int32),
                ("dd_mg", C.c_int32), ("mg_keep", C.c_int32), ("solid_block_jacobi", C.c_int32), ("solid_fused", C.c_int32),
                ("fused_sweeps", C.c_int32), ("scalar_dd", C.c_int32),
                ("its_solid", C.c_int32), ("its_fluid", C.c_int32), ("its_schur", C.c_int32), ("its_disp", C.c_int32),
                ("kappa_solid", C.c_double), ("kappa_fluid", C.c_double), ("kappa_schur", C.c_double), ("kappa_disp", C.c_double),
                ("sbmg_pre", C.c_int32), ("sbmg_post", C.c_int32), ("sbmg_cits", C.c_int32), ("sbmg_alpha", C.c_double),
                ("sbmg_ckappa", C.c_double),
                ("mg_pre", C.c_int32), ("mg_post", C.c_int32), ("mg_cits", C.c_int32), ("mg_alpha", C.c_double), ("mg_ckappa", C.c_double),
                ("solid_coarse_exact", C.c_int32), ("compact_drows", C.c_int32), ("bcr_shift", C.c_double), ("newton_adaptive", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class FsiNewtonOpts(C.Structure):
    _fields_ = [("atol", C.c_double), ("rtol", C.c_double), ("max_it", C.c_int32), ("lmbda", C.c_double),
                ("recompute", C.c_int32), ("recompute_tstep", C.c_int32), ("counter", C.c_int32),
                ("first_step_num", C.c_int32), ("lin_rtol", C.c_double), ("lin_max_it", C.c_int32),
                ("lin_solver", C.c_int32)]


class FsiNewtonIter(C.Structure):
    _fields_ = [("residual", C.c_double), ("rel_res", C.c_double), ("recomputed", C.c_int32),
                ("lin_iters", C.c_int32), ("lin_relres", C.c_double)]


class FsiTimers(C.Structure):
    _fields_ = [("residual_ms", C.c_double), ("residual_calls", C.c_int64), ("jacobian_ms", C.c_double),
                ("jacobian_calls", C.c_int64), ("factor_ms", C.c_double), ("factor_calls", C.c_int64),
                ("spmv_ms", C.c_double), ("spmv_calls", C.c_int64), ("precond_ms", C.c_double),
                ("precond_calls", C.c_int64), ("ortho_ms", C.c_double), ("ortho_calls", C.c_int64),
                ("krylov_ms", C.c_double), ("krylov_solves", C.c_int64), ("krylov_iters", C.c_int64),
                ("inner_vv_iters", C.c_int64), ("inner_schur_iters", C.c_int64), ("inner_dd_iters", C.c_int64),
                ("precond_applies", C.c_int64), ("solid_spmv_ms", C.c_double), ("solid_spmv_calls", C.c_int64),
                ("solid_nnz", C.c_int64), ("solid_rows", C.c_int64), ("db_spmv_ms", C.c_double),
                ("db_spmv_calls", C.c_int64), ("db_pairs", C.c_int64), ("db_nodes", C.c_int64),
                ("sc_spmv_ms", C.c_double), ("sc_spmv_calls", C.c_int64), ("disp_scalar", C.c_int64), ("tile_entries", C.c_int64),
                ("ortho_q_cols", C.c_int64), ("ortho_q_launches", C.c_int64), ("ortho_z_cols", C.c_int64),
                ("ortho_z_launches", C.c_int64), ("q_elem_bytes", C.c_int64), ("ldq", C.c_int64), ("ldz", C.c_int64),
                ("krylov_dirs", C.c_int64), ("krylov_cap", C.c_int64), ("schur_nnz", C.c_int64), ("schur_rows", C.c_int64),
                ("flush_ms", C.c_double), ("flush_calls", C.c_int64), ("schur_ms", C.c_double), ("schur_calls", C.c_int64),
                ("schur_elem_bytes", C.c_int64), ("node_pairs", C.c_int64),
                ("node_vertex_pairs", C.c_int64), ("spmv_fp32_calls", C.c_int64), ("sweep_flags", C.c_int64), ("part_allreduces", C.c_int64),
                ("assembly_colours", C.c_int64), ("gcr_arnoldi_steps", C.c_int64), ("gcr_restarts", C.c_int64),
                ("newton_retries", C.c_int64), ("fp32_fallbacks", C.c_int64), ("verdicts_skipped", C.c_int64),
                ("reorth_forced", C.c_int64), ("dd_cache_hits", C.c_int64), ("newton_late_solves", C.c_int64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class FsiError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{ERROR_NAMES.get(code, code)}: {message}")
        self.code = code


_lib = None


def load_library(path: Optional[Path] = None):
    """Load libvaspfsi.so and declare the prototypes. Raises if the library has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise RuntimeError(f"{p} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()' "
                           f"or make -C vasp_amd/csrc). There is no CPU fallback.")
    lib = C.CDLL(str(p))
    vp, i64, i32, dbl = C.c_void_p, C.c_int64, C.c_int32, C.c_double
    lib.fsi_create.argtypes = [C.POINTER(FsiMeshDesc), C.POINTER(FsiParams), C.c_int, C.POINTER(vp)]
    lib.fsi_create_tuned.argtypes = [C.POINTER(FsiMeshDesc), C.POINTER(FsiParams), C.c_int, C.POINTER(FsiTuning), C.POINTER(vp)]
    lib.fsi_get_tuning.argtypes = [vp, C.POINTER(FsiTuning)]
    lib.fsi_tuning_defaults.argtypes = [C.POINTER(FsiTuning)]
    lib.fsi_tuning_from_env.argtypes = [C.POINTER(FsiTuning)]
    lib.fsi_tuning_copy_out.argtypes = [C.POINTER(FsiTuning), C.POINTER(FsiTuning)]
    lib.fsi_destroy.argtypes = [vp]
    lib.fsi_last_error.argtypes = [vp]
    lib.fsi_last_error.restype = C.c_char_p
    lib.fsi_set_dirichlet.argtypes = [vp, i64, vp]
    lib.fsi_set_dirichlet_values.argtypes = [vp, i64, vp]
    lib.fsi_set_pressure_facets.argtypes = [vp, i64, vp, vp]
    lib.fsi_set_interface_pressure.argtypes = [vp, dbl]
    lib.fsi_set_robin_facets.argtypes = [vp, i64, vp, vp, vp]
    lib.fsi_solver_setup.argtypes = [vp]
    lib.fsi_assemble_residual.argtypes = [vp, C.POINTER(dbl)]
    lib.fsi_assemble_jacobian.argtypes = [vp]
    lib.fsi_solve.argtypes = [vp, dbl, i32, i32, C.POINTER(i32), C.POINTER(dbl)]
    lib.fsi_newton_solve.argtypes = [vp, C.POINTER(FsiNewtonOpts), C.POINTER(FsiNewtonIter), C.POINTER(i32)]
    lib.fsi_shift.argtypes = [vp]
    lib.fsi_get_state.argtypes = [vp, C.c_int, vp]
    lib.fsi_set_state.argtypes = [vp, C.c_int, vp]
    lib.fsi_set_frame.argtypes = [vp, C.c_int, i64, vp, vp, vp]
    lib.fsi_get_values.argtypes = [vp, C.c_int, i64, vp, vp]
    lib.fsi_calibration_streams.argtypes = [vp, i64]
    lib.fsi_set_newton_forcing.argtypes = [vp, dbl]
    lib.fsi_stress_strain.argtypes = [vp, i64, vp, vp]
    lib.fsi_wall_shear_stress.argtypes = [vp, i64, vp, vp, dbl, vp]
    lib.fsi_hemo_begin.argtypes = [vp, i64, vp, vp, dbl, dbl]
    lib.fsi_hemo_sample.argtypes = [vp, vp]
    lib.fsi_hemo_indices.argtypes = [vp, vp, C.POINTER(i64)]
    lib.fsi_hemo_export.argtypes = [vp, vp, C.POINTER(i64)]
    lib.fsi_hemo_import.argtypes = [vp, vp, i64]
    lib.fsi_hemo_end.argtypes = [vp]
    lib.fsi_stress_begin.argtypes = [vp, i64, vp]
    lib.fsi_stress_sample.argtypes = [vp, vp]
    lib.fsi_stress_averages.argtypes = [vp, vp, C.POINTER(i64)]
    lib.fsi_stress_export.argtypes = [vp, vp, C.POINTER(i64)]
    lib.fsi_stress_import.argtypes = [vp, vp, i64]
    lib.fsi_stress_end.argtypes = [vp]
    lib.fsi_band_begin.argtypes = [vp, i32, i64, vp, vp, i64]
    lib.fsi_band_begin_cells.argtypes = [vp, i32, i64, vp, i64]
    lib.fsi_band_sample.argtypes = [vp, i32]
    lib.fsi_band_filter.argtypes = [vp, i32, i32, vp, vp, vp, i32]
    lib.fsi_band_amplitude.argtypes = [vp, i32, i32]
    lib.fsi_band_phase.argtypes = [vp, i32, i64]
    lib.fsi_band_phase_fetch.argtypes = [vp, i32, i32, i64, vp]
    lib.fsi_band_spi.argtypes = [vp, i32, vp, i64, i64, vp, vp]
    lib.fsi_band_spi_fetch.argtypes = [vp, i32, i32, vp]
    lib.fsi_band_pod_gram.argtypes = [vp, i32, i32, vp]
    lib.fsi_band_pod_modes.argtypes = [vp, i32, i32, vp]
    lib.fsi_band_pod_fetch.argtypes = [vp, i32, i32, i64, vp]
    lib.fsi_band_cells.argtypes = [vp, i32, i64, vp, vp]
    lib.fsi_band_cell_rate.argtypes = [vp, i32, i32, i64, i64, i64, vp]
    lib.fsi_band_cell_rate_current.argtypes = [vp, i32, i32, i64, i64, i64, vp, vp, vp]
    lib.fsi_band_cell_weights.argtypes = [vp, i32, vp]
    lib.fsi_band_cell_vortex.argtypes = [vp, i32, i32, i64, i64, i64, vp, vp]
    lib.fsi_band_cell_vortex_current.argtypes = [vp, i32, i32, i64, i64, i64, vp, vp]
    lib.fsi_band_fetch.argtypes = [vp, i32, i32, i64, vp, C.POINTER(dbl), C.POINTER(i64)]
    lib.fsi_band_select.argtypes = [vp, i32, i64, i64, i64]
    lib.fsi_band_filter_next.argtypes = [vp, i32, i32, vp, vp, vp, i32]
    lib.fsi_band_trace.argtypes = [vp, i32, i32, i64, vp, vp]
    lib.fsi_band_export.argtypes = [vp, i32, i64, i64, vp]
    lib.fsi_band_import.argtypes = [vp, i32, i64, vp]
    lib.fsi_band_end.argtypes = [vp, i32]
    lib.fsi_band_room.argtypes = [vp, i64, i64, C.POINTER(dbl), C.POINTER(dbl)]
    lib.fsi_board_begin.argtypes = [vp, i64, i64]
    lib.fsi_board_end.argtypes = [vp]
    lib.fsi_band_board_attach.argtypes = [vp, i32, i64]
    lib.fsi_board_table.argtypes = [vp, i64, i64, i32, vp, vp, vp, vp, vp]
    lib.fsi_order_statistics.argtypes = [vp, i64, vp, i32, vp, vp, C.POINTER(i64)]
    lib.fsi_spec_begin.argtypes = [vp, i32, i64, vp, vp, i32, i64]
    lib.fsi_spec_begin_rows.argtypes = [vp, i32, i64, vp, vp, vp, i64]
    lib.fsi_spec_begin_wss.argtypes = [vp, i64, vp, vp, dbl, i64, vp, vp, i64]
    lib.fsi_spec_room.argtypes = [vp, i64, i32, i64, C.POINTER(dbl), C.POINTER(dbl)]
    lib.fsi_spec_sample.argtypes = [vp, i32]
    lib.fsi_spec_filter.argtypes = [vp, i32, i32, vp, vp, vp, i32]
    lib.fsi_spec_fetch.argtypes = [vp, i32, i32, i64, vp]
    lib.fsi_spec_spectrogram.argtypes = [vp, i32, i64, i64, i64, vp, i32, dbl, vp]
    lib.fsi_spec_periodogram.argtypes = [vp, i32, vp, i32, dbl, vp]
    lib.fsi_spec_spectrogram_sum.argtypes = [vp, i32, i64, i64, i64, vp, i32, dbl, i64, i64, vp]
    lib.fsi_spec_periodogram_sum.argtypes = [vp, i32, vp, i32, dbl, i64, i64, vp]
    lib.fsi_spec_export.argtypes = [vp, i32, i64, i64, vp]
    lib.fsi_spec_import.argtypes = [vp, i32, i64, vp]
    lib.fsi_spec_end.argtypes = [vp, i32]
    lib.fsi_num_dofs.argtypes = [vp]
    lib.fsi_num_dofs.restype = i64
    lib.fsi_matrix_nnz.argtypes = [vp]
    lib.fsi_matrix_nnz.restype = i64
    lib.fsi_device_memory.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    lib.fsi_get_matrix.argtypes = [vp, vp, vp, vp]
    lib.fsi_spmv.argtypes = [vp, vp, vp]
    lib.fsi_apply_preconditioner.argtypes = [vp, vp, vp]
    lib.fsi_get_timers.argtypes = [vp, C.POINTER(FsiTimers), C.c_int]
    lib.fsi_get_solver_events.argtypes = [vp, vp]
    lib.fsi_bcr_plan_graph.argtypes = [i64, vp, vp, vp, vp, vp]
    lib.fsi_xcd_order.argtypes = [i64, vp]
    lib.fsi_xcd_order.restype = i64
    lib.fsi_solid_coarse_info.argtypes = [vp, vp]
    lib.fsi_solid_coarse_matrix.argtypes = [vp, vp, vp, vp]
    lib.fsi_solid_coarse_solve.argtypes = [vp, vp, vp]
    lib.fsi_set_linear_solver.argtypes = [vp, i32]
    lib.fsi_probe.argtypes = [vp, i64, vp, vp, vp]
    lib.fsi_flow_stats.argtypes = [vp, vp]
    lib.fsi_set_chebyshev.argtypes = [vp, i32, dbl, i32, dbl, i32, dbl, i32, dbl]
    lib.fsi_set_partition.argtypes = [vp, i64, i64, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.fsi_rccl_unique_id.argtypes = [vp]
    lib.fsi_set_rccl.argtypes = [vp, C.c_char_p, i32, i32, vp, vp]
    for name in EXPORTED_SYMBOLS:
        fn = getattr(lib, name)
        if name in ("fsi_tuning_defaults", "fsi_tuning_from_env", "fsi_tuning_copy_out"):
            fn.restype = None
        elif name not in ("fsi_last_error", "fsi_num_dofs", "fsi_matrix_nnz"):
            fn.restype = C.c_int
    if path is None:
        _lib = lib
    return lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


STATE = {"n": 0, "n-1": 1, "b": 2, "du": 3}


def _spread3(x: np.ndarray) -> np.ndarray:
    """Bits of a 21-bit integer spread to every third position (for a 63-bit Morton key)."""
    x = x.astype(np.uint64) & np.uint64(0x1FFFFF)
    x = (x | (x << np.uint64(32))) & np.uint64(0x1F00000000FFFF)
    x = (x | (x << np.uint64(16))) & np.uint64(0x1F0000FF0000FF)
    x = (x | (x << np.uint64(8))) & np.uint64(0x100F00F00F00F00F)
    x = (x | (x << np.uint64(4))) & np.uint64(0x10C30C30C30C30C3)
    x = (x | (x << np.uint64(2))) & np.uint64(0x1249249249249249)
    return x


def cell_locality_order(coords: np.ndarray, tets: np.ndarray, num_owned: Optional[int] = None) -> np.ndarray:
    """Permutation that puts the cells along a Morton (Z-order) curve through their centroids - the curve the library
    numbers the nodes along - so that the ~24 cells around a node are assembled close in time and the node's state, its
    residual entries and its matrix rows are still on die when the next of them needs them.  A mesh file's own order need
    not have that property: the generator of the bench mesh emits twelve sweeps over the whole domain (one tetrahedron per
    hexahedron and sweep), which made every element kernel fetch each node twelve times (k_residual: 3.4 GB of HBM traffic
    for 1.9 GB of algorithmic bytes).  With ``num_owned`` (element partition: owned cells first, then ghost cells) the two
    groups are ordered separately."""
    c = np.asarray(coords, dtype=np.float64)[np.asarray(tets)[:, :4]].mean(axis=1)
    lo, ext = c.min(axis=0), np.maximum(np.ptp(c, axis=0), 1e-300)
    q = np.minimum(((c - lo) / ext.max() * (2 ** 21 - 1)).astype(np.int64), 2 ** 21 - 1)
    key = _spread3(q[:, 0]) | (_spread3(q[:, 1]) << np.uint64(1)) | (_spread3(q[:, 2]) << np.uint64(2))
    if num_owned is None:
        return np.argsort(key, kind="stable")
    no = int(num_owned)
    return np.concatenate([np.argsort(key[:no], kind="stable"), no + np.argsort(key[no:], kind="stable")])


class HipBackend:
    """One problem instance resident on one GPU; the methods are what ``monolithic.run`` calls per time step."""

    def __init__(self, desc: dict, device: int = 0, lin_rtol: float = 1e-10, lin_max_it: int = 4000,
                 lin_solver: int = 0, precond: int = 0,
                 newton_forcing: Optional[float] = None, num_owned_cells: Optional[int] = None,
                 tuning: Optional[dict] = None):
        import os
        self.lib = load_library()
        self.ctx = C.c_void_p()
        # the sizes of the open sessions, for the arrays handed to the library: a begin replaces a record whole, an end removes it
        self._hemo_nf = self._stress_n = 0      # facets / cells of the hemodynamics and the stress / strain session; 0: none
        self._band = {}              # hi_pass_begin(_cells): quantity -> its NO_BAND with the session's numbers
        self._spec_shape = {}        # spec_begin: quantity -> [rows, recorded frames]
        self.lin_rtol, self.lin_max_it, self.lin_solver = lin_rtol, lin_max_it, lin_solver
        coords = np.ascontiguousarray(desc["coords"], dtype=np.float64)
        # cells are handed to the library in a locality order (VASPFSI_CELL_ORDER=mesh: as the caller numbers them); cell
        # indices at this boundary (probes, stress cells, facet cells) stay the caller's and are mapped here
        tn_user = np.asarray(desc["tet_nodes"])
        if os.environ.get("VASPFSI_CELL_ORDER", "morton") == "mesh":
            order = np.arange(len(tn_user))
        else:
            order = cell_locality_order(coords, tn_user, num_owned_cells)
        self.cell_order = order
        self.cell_u2i = np.empty(len(order), dtype=np.int32)
        self.cell_u2i[order] = np.arange(len(order), dtype=np.int32)
        tet_nodes = np.ascontiguousarray(tn_user[order], dtype=np.int32)
        kind = np.ascontiguousarray(np.asarray(desc["cell_kind"])[order], dtype=np.int32)
        region = np.ascontiguousarray(np.asarray(desc["cell_region"])[order], dtype=np.int32)
        fprops = np.ascontiguousarray(np.asarray(desc["fluid_props"], dtype=np.float64).reshape(-1, 2))
        sp_rows = [tuple(r) + (0.0,) * (6 - len(r)) for r in desc["solid_props"]]     # rho, mu, lambda[, C10, C01, C11]
        sprops = np.ascontiguousarray(np.asarray(sp_rows, dtype=np.float64).reshape(-1, 6))
        smodels = np.ascontiguousarray(desc.get("solid_models", [0] * len(sprops)), dtype=np.int32)
        md = FsiMeshDesc(len(coords), int(desc["num_nodes"]), len(tet_nodes), _ptr(coords), _ptr(tet_nodes),
                         _ptr(kind), _ptr(region))
        pr = FsiParams(float(desc["dt"]), float(desc["theta"]), len(fprops), _ptr(fprops), len(sprops), _ptr(sprops),
                       _ptr(smodels), float(desc.get("delta", 1.0e7)), float(desc.get("laplace_alpha", 1.0)))
        if tuning:          # named FsiTuning fields over the defaults + environment overrides; fsi_create_tuned takes the struct as given
            t = FsiTuning()
            self.lib.fsi_tuning_from_env(C.byref(t))
            for k, v in tuning.items():
                if k not in dict(FsiTuning._fields_):
                    raise KeyError(f"FsiTuning has no field {k!r}")
                setattr(t, k, v)
            rc = self.lib.fsi_create_tuned(C.byref(md), C.byref(pr), device, C.byref(t), C.byref(self.ctx))
        else:
            rc = self.lib.fsi_create(C.byref(md), C.byref(pr), device, C.byref(self.ctx))
        if rc != FSI_OK:
            msg = self.lib.fsi_last_error(self.ctx).decode() if self.ctx else "fsi_create failed"
            if self.ctx:
                self.lib.fsi_destroy(self.ctx)
                self.ctx = C.c_void_p()
            raise FsiError(rc, msg)
        self.ndof = int(self.lib.fsi_num_dofs(self.ctx))
        self._check(self.lib.fsi_set_linear_solver(self.ctx, int(precond)))
        if newton_forcing is not None:          # 0: every Newton system solved to lin_rtol, as the reference's direct LU
            self._check(self.lib.fsi_set_newton_forcing(self.ctx, float(newton_forcing)))
        bc = np.ascontiguousarray(desc.get("bc_dofs", np.zeros(0)), dtype=np.int64)
        self._check(self.lib.fsi_set_dirichlet(self.ctx, len(bc), _ptr(bc)))
        self.nbc = len(bc)
        pf = desc.get("pressure_facets")
        if pf is not None and len(pf):
            pf = np.ascontiguousarray(pf, dtype=np.int32)
            pc = np.ascontiguousarray(self.cell_u2i[np.asarray(desc["pressure_facet_cell"], dtype=np.int64)], dtype=np.int32)
            self._check(self.lib.fsi_set_pressure_facets(self.ctx, len(pf), _ptr(pf), _ptr(pc)))
        rf = desc.get("robin_facets")
        if rf is not None and len(rf):
            rf = np.ascontiguousarray(rf, dtype=np.int32)
            rk = np.ascontiguousarray(desc["robin_k"], dtype=np.float64)
            rcoef = np.ascontiguousarray(desc["robin_c"], dtype=np.float64)
            self._check(self.lib.fsi_set_robin_facets(self.ctx, len(rf), _ptr(rf), _ptr(rk), _ptr(rcoef)))
        self._check(self.lib.fsi_solver_setup(self.ctx))
        self.history: List[list] = []
        self._flow_stats = None

    # ---- plumbing ---------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != FSI_OK:
            raise FsiError(rc, self.lib.fsi_last_error(self.ctx).decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.fsi_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- backend protocol of monolithic.run -----------------------------------------------------------
    def set_dirichlet_values(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        self._check(self.lib.fsi_set_dirichlet_values(self.ctx, len(v), _ptr(v)))

    def set_interface_pressure(self, P: float):
        self._check(self.lib.fsi_set_interface_pressure(self.ctx, float(P)))

    def newton_solve(self, *, counter, first_step_num, atol, rtol, max_it, lmbda, recompute, recompute_tstep, log=None):
        opts = FsiNewtonOpts(atol, rtol, int(max_it), lmbda, int(recompute), int(recompute_tstep), int(counter),
                             int(first_step_num), self.lin_rtol, self.lin_max_it, self.lin_solver)
        iters = (FsiNewtonIter * int(max_it))()
        n = C.c_int32(0)
        self._flow_stats = None
        rc = self.lib.fsi_newton_solve(self.ctx, C.byref(opts), iters, C.byref(n))
        hist = []
        for i in range(n.value):
            it = iters[i]
            if log:
                if it.recomputed:
                    log("Compute Jacobian matrix")
                log("Newton iteration %d: r (atol) = %.3e (tol = %.3e), r (rel) = %.3e (tol = %.3e) "
                    % (i, it.residual, atol, it.rel_res, rtol))
            hist.append((it.residual, it.rel_res, bool(it.recomputed), it.lin_iters, it.lin_relres))
        self.history.append(hist)
        if rc == 3:
            raise RuntimeError("Error: The simulation has diverged during the Newton solve.")
        self._check(rc)
        return hist

    def shift(self):
        self._check(self.lib.fsi_shift(self.ctx))

    def get_state(self, which, out=None):
        out = np.empty(self.ndof) if out is None else out
        self._check(self.lib.fsi_get_state(self.ctx, STATE[which], _ptr(out)))
        return out

    def get_values(self, which, dofs):
        """state[dofs] (user layout) without copying the whole vector off the device."""
        dofs = np.ascontiguousarray(dofs, dtype=np.int64)
        out = np.empty(len(dofs))
        self._check(self.lib.fsi_get_values(self.ctx, STATE[which], len(dofs), _ptr(dofs), _ptr(out)))
        return out

    def set_state(self, which, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (self.ndof,)
        self._flow_stats = None
        self._check(self.lib.fsi_set_state(self.ctx, STATE[which], _ptr(x)))

    def set_frame(self, which, d=None, v=None, p=None) -> None:
        """One saved Visualization frame into the state (fsi_set_frame): d, v (n, 3) and p (n,) or (n, 1) on the files' n nodes,
        n the mesh's vertices (save_deg 1: mid-edge nodes take their edge's mean) or its P2 nodes (save_deg 2).  A field that
        is None keeps what the state holds.  C-contiguous FP64 arrays - the views of a mapped file - are passed as they are."""
        given = {k: a for k, a in (("d", d), ("v", v), ("p", p)) if a is not None}
        if not given:
            return
        arrs, n = {}, None
        for k, a in given.items():
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous):
                a = np.ascontiguousarray(a, dtype=np.float64)
            rows = a.shape[0] if a.ndim else 0
            if a.size != rows * (1 if k == "p" else 3):
                raise ValueError(f"set_frame: {k} of shape {a.shape}, expected (n, {1 if k == 'p' else 3})")
            if n is not None and rows != n:
                raise ValueError(f"set_frame: {k} has {rows} nodes, another field {n}")
            arrs[k], n = a, rows
        self._flow_stats = None
        ptr = lambda k: _ptr(arrs[k]) if k in arrs else None
        self._check(self.lib.fsi_set_frame(self.ctx, STATE[which], n, ptr("d"), ptr("v"), ptr("p")))

    # ---- pieces of the hot path (tests, benchmarks) ----------------------------------------------------
    def assemble_residual(self) -> float:
        nrm = C.c_double(0.0)
        self._check(self.lib.fsi_assemble_residual(self.ctx, C.byref(nrm)))
        return nrm.value

    def assemble_jacobian(self):
        self._check(self.lib.fsi_assemble_jacobian(self.ctx))

    def solve(self, lin_rtol=None, lin_max_it=None, lin_solver=None):
        it, rr = C.c_int32(0), C.c_double(0.0)
        self._check(self.lib.fsi_solve(self.ctx, self.lin_rtol if lin_rtol is None else lin_rtol,
                                       self.lin_max_it if lin_max_it is None else lin_max_it,
                                       self.lin_solver if lin_solver is None else lin_solver, C.byref(it), C.byref(rr)))
        return it.value, rr.value

    def device_memory(self):
        """(free, total) bytes of the context's device, from the library's own HIP runtime."""
        f, t = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.fsi_device_memory(self.ctx, C.byref(f), C.byref(t)))
        return f.value, t.value

    def matrix(self):
        """The assembled Jacobian (after ident_zeros and bc.apply) as scipy CSR in the user dof layout."""
        import scipy.sparse as sp
        nnz = int(self.lib.fsi_matrix_nnz(self.ctx))
        rp = np.empty(self.ndof + 1, dtype=np.int64)
        ci = np.empty(nnz, dtype=np.int64)
        va = np.empty(nnz, dtype=np.float64)
        self._check(self.lib.fsi_get_matrix(self.ctx, _ptr(rp), _ptr(ci), _ptr(va)))
        return sp.csr_matrix((va, ci, rp), shape=(self.ndof, self.ndof))

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty(self.ndof)
        self._check(self.lib.fsi_spmv(self.ctx, _ptr(x), _ptr(y)))
        return y

    def apply_preconditioner(self, r):
        """z = M^-1 r: one application of the active preconditioner (user layout), as the Krylov method applies it."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.empty(self.ndof)
        self._check(self.lib.fsi_apply_preconditioner(self.ctx, _ptr(r), _ptr(z)))
        return z

    def set_linear_solver(self, precond: int = 0):
        self._check(self.lib.fsi_set_linear_solver(self.ctx, int(precond)))

    def set_chebyshev(self, its_solid=0, kappa_solid=0.0, its_fluid=0, kappa_fluid=0.0, its_schur=0, kappa_schur=0.0,
                      its_disp=0, kappa_disp=0.0):
        self._check(self.lib.fsi_set_chebyshev(self.ctx, int(its_solid), float(kappa_solid), int(its_fluid),
                                               float(kappa_fluid), int(its_schur), float(kappa_schur), int(its_disp),
                                               float(kappa_disp)))

    def probe(self, cells, bary):
        """(n,7) array d(3) v(3) p of dvp_["n"] at located points (cells (n,), barycentric (n,4))."""
        cells = np.ascontiguousarray(self.cell_u2i[np.asarray(cells, dtype=np.int64)], dtype=np.int32)
        bary = np.ascontiguousarray(bary, dtype=np.float64)
        out = np.empty((len(cells), 7))
        self._check(self.lib.fsi_probe(self.ctx, len(cells), _ptr(cells), _ptr(bary), _ptr(out)))
        return out

    def flow_stats(self):
        """(mean, min, max of the cell-mean |v|, min of the cell-mean det(I + grad d)) of dvp_["n"].  post_solve asks twice
        per step (flow properties, minimum Jacobian [REF src/vasp/simulations/simulation_common.py:253-348]): the second call of
        a step returns the first one's numbers (the state changes only through newton_solve / set_state)."""
        if self._flow_stats is None:
            out = np.empty(4)
            self._check(self.lib.fsi_flow_stats(self.ctx, _ptr(out)))
            self._flow_stats = tuple(out)
        return self._flow_stats

    def stress_strain(self, cells):
        """DG1 Cauchy stress / Green-Lagrange strain / largest principal values on solid ``cells`` of dvp_["n"]."""
        cells = np.ascontiguousarray(self.cell_u2i[np.asarray(cells, dtype=np.int64)], dtype=np.int32)
        out = np.empty((len(cells), 80))
        self._check(self.lib.fsi_stress_strain(self.ctx, len(cells), _ptr(cells), _ptr(out)))
        return self._stress_frame(out)

    def wall_shear_stress(self, facet_cells, facet_local, mu: float):
        """(nf, 3, 3) projected tangential traction at the vertices of exterior facets (cell, opposite local vertex)."""
        fc = np.ascontiguousarray(self.cell_u2i[np.asarray(facet_cells, dtype=np.int64)], dtype=np.int32)
        fl = np.ascontiguousarray(facet_local, dtype=np.int32)
        out = np.empty((len(fc), 3, 3))
        self._check(self.lib.fsi_wall_shear_stress(self.ctx, len(fc), _ptr(fc), _ptr(fl), float(mu), _ptr(out)))
        return out

    HEMO_INDICES = ("TAWSS", "OSI", "RRT", "ECAP", "TWSSG")

    def hemodynamics_begin(self, facet_cells, facet_local, mu: float, dt_sample: float) -> None:
        """Open the device-side hemodynamics session (fsi_hemo_begin) on exterior facets (cell, opposite local vertex) with
        dynamic viscosity ``mu`` and ``dt_sample`` between two samples; replaces an open session."""
        fc = np.ascontiguousarray(self.cell_u2i[np.asarray(facet_cells, dtype=np.int64)], dtype=np.int32)
        fl = np.ascontiguousarray(facet_local, dtype=np.int32)
        self._check(self.lib.fsi_hemo_begin(self.ctx, len(fc), _ptr(fc), _ptr(fl), float(mu), float(dt_sample)))
        self._hemo_nf = len(fc)

    def hemodynamics_sample(self, wss: bool = False):
        """Add the WSS of dvp_["n"] to the session's sums (fsi_hemo_sample); with ``wss`` return it, (nf, 3, 3) as
        ``wall_shear_stress``, else None."""
        out = np.empty((self._hemo_nf, 3, 3)) if wss else None
        self._check(self.lib.fsi_hemo_sample(self.ctx, _ptr(out) if wss else None))
        return out

    def hemodynamics_indices(self) -> dict:
        """TAWSS, OSI, RRT, ECAP, TWSSG as (nf, 3) arrays (DG1 dofs of the boundary mesh) and ``samples``."""
        out = np.empty((5, self._hemo_nf, 3))
        n = C.c_int64(0)
        self._check(self.lib.fsi_hemo_indices(self.ctx, _ptr(out), C.byref(n)))
        res = {k: out[i].copy() for i, k in enumerate(self.HEMO_INDICES)}
        res["samples"] = int(n.value)
        return res

    def _sums(self, what: str, sums, n: int) -> np.ndarray:
        """The sums handed to an import as the library takes them; another size than the open session's is refused here,
        where the size is known (the C call takes a pointer)."""
        a = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1)
        if a.size != n:
            raise FsiError(1, f"{what}: sums of {a.size} values, the open session has {n}")
        return a

    def hemodynamics_export(self):
        """(acc, samples): the session's accumulator, (24 nf,) in the layout of fsi_hemo_export, and its sample count."""
        out = np.empty(24 * self._hemo_nf)
        n = C.c_int64(0)
        self._check(self.lib.fsi_hemo_export(self.ctx, _ptr(out), C.byref(n)))
        return out, int(n.value)

    def hemodynamics_import(self, acc, samples: int) -> None:
        """Replace the open session's accumulator and sample count by exported ones (fsi_hemo_import); an accumulator of
        another number of facets is refused."""
        a = self._sums("hemodynamics_import", acc, 24 * self._hemo_nf)
        self._check(self.lib.fsi_hemo_import(self.ctx, _ptr(a), int(samples)))

    def hemodynamics_end(self) -> None:
        self._check(self.lib.fsi_hemo_end(self.ctx))
        self._hemo_nf = 0

    @staticmethod
    def _stress_frame(out: np.ndarray) -> dict:
        return dict(TrueStress=out[:, :36].reshape(-1, 4, 3, 3), GreenLagrangeStrain=out[:, 36:72].reshape(-1, 4, 3, 3),
                    MaxPrincipalStress=out[:, 72:76].copy(), MaxPrincipalStrain=out[:, 76:80].copy())

    def stress_strain_begin(self, cells) -> None:
        """Open the device-side stress / strain session (fsi_stress_begin) on solid ``cells`` (user order, as
        ``stress_strain``); replaces an open session."""
        ci = np.ascontiguousarray(self.cell_u2i[np.asarray(cells, dtype=np.int64)], dtype=np.int32)
        self._check(self.lib.fsi_stress_begin(self.ctx, len(ci), _ptr(ci)))
        self._stress_n = len(ci)

    def stress_strain_sample(self, frame: bool = False):
        """Sample dvp_["n"] (fsi_stress_sample): the principal values go to the session's sums; with ``frame`` return the
        frame, keyed as ``stress_strain`` (bitwise equal to it), else None."""
        out = np.empty((self._stress_n, 80)) if frame else None
        self._check(self.lib.fsi_stress_sample(self.ctx, _ptr(out) if frame else None))
        return self._stress_frame(out) if frame else None

    def stress_strain_averages(self) -> dict:
        """MaxPrincipalStress_avg and MaxPrincipalStrain_avg as (n, 4) arrays (DG1 coefficients per cell) and ``samples``."""
        out = np.empty((2, self._stress_n, 4))
        k = C.c_int64(0)
        self._check(self.lib.fsi_stress_averages(self.ctx, _ptr(out), C.byref(k)))
        return dict(MaxPrincipalStress_avg=out[0].copy(), MaxPrincipalStrain_avg=out[1].copy(), samples=int(k.value))

    def stress_strain_export(self):
        """(sums, samples): the session's sums, (n, 8) as fsi_stress_export, and its sample count."""
        out = np.empty((self._stress_n, 8))
        k = C.c_int64(0)
        self._check(self.lib.fsi_stress_export(self.ctx, _ptr(out), C.byref(k)))
        return out, int(k.value)

    def stress_strain_import(self, sums, samples: int) -> None:
        """Replace the open session's sums and sample count by exported ones (fsi_stress_import); sums of another number of
        cells are refused."""
        a = self._sums("stress_strain_import", sums, 8 * self._stress_n)
        self._check(self.lib.fsi_stress_import(self.ctx, _ptr(a), int(samples)))

    def stress_strain_end(self) -> None:
        self._check(self.lib.fsi_stress_end(self.ctx))
        self._stress_n = 0

    BAND_QUANTITY = {"d": 0, "v": 1, "p": 2, "strain": 3, "stress": 4}
    BAND_WHAT = {"raw": 0, "filtered": 1, "amplitude": 2, "magnitude": 3}
    # The record of a band-pass session: a frame is shape = (nodes, ncomp), the history has `recorded` frames of which `selected`
    # are selected (the size of a trace), `cells` cells are attached and the phase mean has `period` frames.  As it stands here:
    # no session - the arrays sized from it are empty and the library, which looks for the session first, refuses the call.
    NO_BAND = dict(shape=(0, 0), recorded=0, selected=0, cells=0, period=0)

    def hi_pass_begin(self, quantity: str, nodes, nodes_b=None, capacity: int = 1) -> None:
        """Open the band-pass session of ``quantity`` ('d', 'v' or 'p'; fsi_band_begin) on ``nodes`` (P2 node ids, vertex
        ids for 'p'; with ``nodes_b`` >= 0 a row is the mean of the two nodes) for up to ``capacity`` frames; replaces an open
        session of the quantity.  Raises FsiError when the history would not fit the device."""
        q = self.BAND_QUANTITY[quantity]
        a = np.ascontiguousarray(nodes, dtype=np.int32)
        b = None if nodes_b is None else np.ascontiguousarray(nodes_b, dtype=np.int32)
        if b is not None and b.shape != a.shape:
            raise ValueError("nodes_b must have the shape of nodes")
        self._check(self.lib.fsi_band_begin(self.ctx, q, len(a), _ptr(a), None if b is None else _ptr(b), int(capacity)))
        self._band[quantity] = dict(self.NO_BAND, shape=(len(a), 1 if quantity == "p" else 3))

    def hi_pass_begin_cells(self, quantity: str, cells, capacity: int = 1) -> None:
        """Open the band-pass session of the tensor ``quantity`` ('strain': Green-Lagrange strain, 'stress': Cauchy stress;
        fsi_band_begin_cells) on solid ``cells`` (user order, as ``stress_strain_begin``) for up to ``capacity`` frames;
        replaces an open session of the quantity.  Its frames are (4 cells, 6): per DG1 dof 4 i + a the components 11, 12, 22,
        23, 33, 31; the other ``hi_pass_*`` methods serve it, 'magnitude' being the largest principal value per dof."""
        q = self.BAND_QUANTITY[quantity]
        ci = np.ascontiguousarray(self.cell_u2i[np.asarray(cells, dtype=np.int64).reshape(-1)], dtype=np.int32)
        self._check(self.lib.fsi_band_begin_cells(self.ctx, q, len(ci), _ptr(ci), int(capacity)))
        self._band[quantity] = dict(self.NO_BAND, shape=(4 * len(ci), 6))

    def hi_pass_sample(self, quantity: str) -> None:
        """Record the session's rows of dvp_["n"] as the next frame of its history (fsi_band_sample)."""
        self._check(self.lib.fsi_band_sample(self.ctx, self.BAND_QUANTITY[quantity]))
        rec = self._band[quantity]
        rec["recorded"] += 1
        rec["selected"] = rec["recorded"]             # a new frame resets the selection to every recorded frame

    def hi_pass_filter(self, quantity: str, b, a, zi, padlen: int) -> None:
        """scipy.signal.filtfilt(b, a, .) of every row over the recorded frames (fsi_band_filter); zi = lfilter_zi(b, a)."""
        b, a, zi = (np.ascontiguousarray(x, dtype=np.float64) for x in (b, a, zi))
        if len(a) != len(b) or len(zi) != len(b) - 1:
            raise ValueError("b and a must have one length, zi one less")
        self._check(self.lib.fsi_band_filter(self.ctx, self.BAND_QUANTITY[quantity], len(b), _ptr(b), _ptr(a), _ptr(zi), int(padlen)))

    def hi_pass_select(self, quantity: str, first: int = 0, count: int = -1, stride: int = 1) -> int:
        """Form the filtered series, the amplitude and the traces on the recorded frames ``first, first + stride, ...``,
        ``count`` of them (-1: as many as fit) (fsi_band_select); a raw fetch keeps absolute frame indices.  Returns the
        number of selected frames."""
        first, count, stride = int(first), int(count), int(stride)
        self._check(self.lib.fsi_band_select(self.ctx, self.BAND_QUANTITY[quantity], first, count, stride))
        rec = self._band[quantity]
        rec["selected"] = (rec["recorded"] - 1 - first) // stride + 1 if count == -1 else count
        return rec["selected"]

    def hi_pass_filter_next(self, quantity: str, b, a, zi, padlen: int) -> None:
        """One more stage on the filtered series, y <- filtfilt(b, a, y), in place on the device (fsi_band_filter_next)."""
        b, a, zi = (np.ascontiguousarray(x, dtype=np.float64) for x in (b, a, zi))
        if len(a) != len(b) or len(zi) != len(b) - 1:
            raise ValueError("b and a must have one length, zi one less")
        self._check(self.lib.fsi_band_filter_next(self.ctx, self.BAND_QUANTITY[quantity], len(b), _ptr(b), _ptr(a), _ptr(zi), int(padlen)))

    def hi_pass_trace(self, quantity: str, what: str, points) -> np.ndarray:
        """The series of the listed nodes (indices into the session's node list) over the selected frames, 'raw' or
        'filtered', as (points, frames, 1 + ncomp) with the magnitude first (fsi_band_trace): one copy from the device."""
        pts = np.ascontiguousarray(points, dtype=np.int32).reshape(-1)
        rec = self._band.get(quantity, self.NO_BAND)
        out = np.empty((len(pts), rec["selected"], 1 + rec["shape"][1]))
        self._check(self.lib.fsi_band_trace(self.ctx, self.BAND_QUANTITY[quantity], self.BAND_WHAT[what], len(pts), _ptr(pts), _ptr(out)))
        return out

    def hi_pass_amplitude(self, quantity: str, window: int) -> None:
        """Select the amplitude of the filtered series (fsi_band_amplitude): flat-window RMS over ``window`` frames, or the
        series itself with ``window`` 0."""
        self._check(self.lib.fsi_band_amplitude(self.ctx, self.BAND_QUANTITY[quantity], int(window)))

    PHASE_WHAT = {"mean": 0, "energy": 1, "energy_cycle_mean": 2, "energy_time_mean": 3}

    def hi_pass_phase(self, quantity: str, period: int) -> None:
        """The phase-averaged decomposition of the selected frames, whole cycles of ``period`` frames (fsi_band_phase): the
        fluctuation about the mean over the cycles becomes the filtered series - 'filtered' and 'amplitude' fetches and a
        'filtered' trace serve it -, the means and the fluctuation's energy come from ``hi_pass_phase_fetch``."""
        self._check(self.lib.fsi_band_phase(self.ctx, self.BAND_QUANTITY[quantity], int(period)))
        self._band[quantity]["period"] = int(period)

    def hi_pass_phase_fetch(self, quantity: str, what: str, frame: int = 0) -> np.ndarray:
        """After ``hi_pass_phase``: 'mean' of phase ``frame`` as (n, ncomp); 'energy' 0.5 |u'|^2 of fluctuation frame
        ``frame``, 'energy_cycle_mean' its mean over the cycles at phase ``frame``, 'energy_time_mean' its mean over all
        selected frames (``frame`` 0), each as (n,) (fsi_band_phase_fetch)."""
        n, ncomp = self._band.get(quantity, self.NO_BAND)["shape"]
        out = np.empty((n, ncomp)) if what == "mean" else np.empty(n)
        self._check(self.lib.fsi_band_phase_fetch(self.ctx, self.BAND_QUANTITY[quantity], self.PHASE_WHAT[what], int(frame), _ptr(out)))
        return out

    SPI_WHAT = {"rows": 0, "nodes": 1, "sums": 2}

    def hi_pass_spi(self, quantity: str, window, bin0: int, nb: int, Ct=None, St=None) -> None:
        """One slab of the spectral power index of the selected raw frames (fsi_band_spi): the ``nb`` lowest bins from
        ``bin0`` of the DFT over the n selected frames, ``window`` (n,) or None for the boxcar.  ``Ct`` / ``St`` (n, nb): the
        slab's cos / sin columns, frame-major; None: ``spectrogram.spec_tables`` of the selected count.  A slab with
        ``bin0`` > 0 adds onto the slabs before it; the index comes from ``hi_pass_spi_fetch``."""
        bin0, nb = int(bin0), int(nb)
        n = self._band.get(quantity, self.NO_BAND)["selected"]
        if Ct is None and nb >= 1 and bin0 >= 0 and n >= 1:
            from .spectrogram import spec_tables
            C, S = spec_tables(n, n, bin0, nb)
            Ct, St = C.T, S.T
        w = None if window is None else np.ascontiguousarray(window, dtype=np.float64).reshape(-1)
        if w is not None and len(w) != n:
            raise ValueError(f"the window has {len(w)} values, {n} frames are selected")
        Ct, St = (None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (Ct, St))
        if Ct is not None and (Ct.shape != (n, nb) or St.shape != (n, nb)):
            raise ValueError(f"Ct and St must be (frames, nb) = ({n}, {nb}), got {Ct.shape} and {St.shape}")
        self._check(self.lib.fsi_band_spi(self.ctx, self.BAND_QUANTITY[quantity], None if w is None else _ptr(w), bin0, nb,
                                          None if Ct is None else _ptr(Ct), None if St is None else _ptr(St)))

    def hi_pass_spi_fetch(self, quantity: str, what: str = "nodes") -> np.ndarray:
        """After ``hi_pass_spi``: 'rows' the index of every row as (n, ncomp), 'nodes' the power-summed index of every node as
        (n,), 'sums' the three sums L2, X0^2, Q of every row as (3, n, ncomp) (fsi_band_spi_fetch)."""
        n, ncomp = self._band.get(quantity, self.NO_BAND)["shape"]
        out = np.empty(n) if what == "nodes" else np.empty((n, ncomp)) if what == "rows" else np.empty((3, n, ncomp))
        self._check(self.lib.fsi_band_spi_fetch(self.ctx, self.BAND_QUANTITY[quantity], self.SPI_WHAT[what], _ptr(out)))
        return out

    POD_WHAT = {"gram": 0, "mean": 1, "mode": 2}

    def hi_pass_pod_gram(self, quantity: str, series: str = "raw", weights=None) -> None:
        """The Gram matrix of the proper orthogonal decomposition of the selected frames (fsi_band_pod_gram): ``series`` 'raw'
        the selected raw frames, 'series' the filtered series or the fluctuation; ``weights`` one value >= 0 per node of the
        session, or None for 1.  Replaces a decomposition that stood, its modes included; the matrix and the mean come from
        ``hi_pass_pod_fetch``, the eigen step is ``hi_pass.pod_eig``."""
        if series not in ("raw", "series"):
            raise FsiError(1, "hi_pass_pod_gram: series must be 'raw' or 'series'")
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        n = self._band.get(quantity, self.NO_BAND)["shape"][0]
        if w is not None and n and len(w) != n:
            raise ValueError(f"{len(w)} weights, the session has {n} nodes")
        self._check(self.lib.fsi_band_pod_gram(self.ctx, self.BAND_QUANTITY[quantity], self.RATE_SERIES[series], None if w is None else _ptr(w)))

    def hi_pass_pod_modes(self, quantity: str, table) -> None:
        """The modes ``Phi_m = sum_j table[j, m] y_j`` of the decomposition whose Gram matrix stands (fsi_band_pod_modes):
        ``table`` (frames, nmodes), 1 <= nmodes <= 64, ``hi_pass.pod_table`` of the eigen step."""
        T = np.ascontiguousarray(table, dtype=np.float64)
        frames = self._band.get(quantity, self.NO_BAND)["selected"]      # a decomposition stands on the selection that stands
        if T.ndim != 2 or (frames and T.shape[0] != frames):
            raise ValueError(f"the table must be (frames, nmodes) = ({frames}, nmodes), got {T.shape}")
        self._check(self.lib.fsi_band_pod_modes(self.ctx, self.BAND_QUANTITY[quantity], T.shape[1], _ptr(T) if T.size else None))

    def hi_pass_pod_fetch(self, quantity: str, what: str, index: int = 0) -> np.ndarray:
        """After ``hi_pass_pod_gram``: 'gram' the matrix (frames, frames), 'mean' the mean the frames were taken about
        (n, ncomp); after ``hi_pass_pod_modes``: 'mode' ``index`` as (n, ncomp) (fsi_band_pod_fetch)."""
        rec = self._band.get(quantity, self.NO_BAND)
        frames = rec["selected"]
        out = np.empty((frames, frames)) if what == "gram" else np.empty(rec["shape"])
        self._check(self.lib.fsi_band_pod_fetch(self.ctx, self.BAND_QUANTITY[quantity], self.POD_WHAT[what], int(index), _ptr(out) if out.size else None))
        return out

    RATE_SERIES = {"raw": 0, "series": 1, "phase_mean": 2}

    def hi_pass_cells(self, quantity: str, cells) -> np.ndarray:
        """Attach mesh ``cells`` (user order) to the session of 'd' or 'v' (fsi_band_cells): every P2 node of every cell must be
        a node of the session.  Returns the gradients of the cells' barycentric coordinates the kernel will use, (n, 4, 3); a
        second call replaces the list."""
        ci = np.ascontiguousarray(self.cell_u2i[np.asarray(cells, dtype=np.int64).reshape(-1)], dtype=np.int32)
        grad = np.empty((len(ci), 4, 3))
        self._check(self.lib.fsi_band_cells(self.ctx, self.BAND_QUANTITY[quantity], len(ci), _ptr(ci), _ptr(grad)))
        self._band[quantity]["cells"] = len(ci)
        return grad

    def _cell_frames(self, quantity: str, series: str, first: int, step: int, count: int) -> tuple:
        """``(first, step, count)`` as integers, ``count`` -1 made as many frames as the series has, and the number of attached
        cells; refusing is the entry point's."""
        first, step, count, rec = int(first), int(step), int(count), self._band.get(quantity, self.NO_BAND)
        if count == -1 and step >= 1:
            count = ((rec["period"] if series == "phase_mean" else rec["selected"]) - 1 - first) // step + 1
        return first, step, count, rec["cells"]

    def hi_pass_cell_rate(self, quantity: str, series: str, first: int = 0, step: int = 1, count: int = -1) -> np.ndarray:
        """Per attached cell the mean over frames ``first, first + step, ...`` (``count`` of them, -1: as many as the series
        has) of the cell mean of 2 S:S, S = sym(grad w), summed in frame order from +0.0 and divided by the count
        (fsi_band_cell_rate).  ``series``: 'raw' the selected frames, 'series' the filtered series or the fluctuation,
        'phase_mean' the frames of the phase mean.  (n,)."""
        first, step, count, n = self._cell_frames(quantity, series, first, step, count)
        out = np.empty(n)
        self._check(self.lib.fsi_band_cell_rate(self.ctx, self.BAND_QUANTITY[quantity], self.RATE_SERIES[series], first, step, count,
                                                _ptr(out) if len(out) else None))
        return out

    def hi_pass_cell_rate_current(self, quantity: str, series: str, first: int = 0, step: int = 1, count: int = -1):
        """``hi_pass_cell_rate`` in the current configuration x = X + d(X) (fsi_band_cell_rate_current): the geometry is the
        history of the 'd' session on the same nodes and frames.  Returns ``(rate, volume_ratio, min_jacobian)``, (n,) each:
        the mean over the frames of the mean of 2 S:S over the deformed cell, S = sym(grad w F^-1); the mean over the frames
        of the deformed cell's volume over the undeformed; the smallest det F met at the rule's four points."""
        first, step, count, n = self._cell_frames(quantity, series, first, step, count)
        rate, volume_ratio, min_jacobian = np.empty(n), np.empty(n), np.empty(n)
        self._check(self.lib.fsi_band_cell_rate_current(self.ctx, self.BAND_QUANTITY[quantity], self.RATE_SERIES[series], first, step, count,
                                                        *(_ptr(a) if n else None for a in (rate, volume_ratio, min_jacobian))))
        return rate, volume_ratio, min_jacobian

    VORTEX_FIELDS = ("Q", "enstrophy", "helicity", "abs_helicity", "speed2")      # FSI_VORTEX_*, hi_pass.VORTEX_FIELDS

    def hi_pass_cell_weights(self, quantity: str, weights) -> None:
        """One weight per attached cell, in the list's order (the cell volumes, for a bulk integral), for the sums of
        ``hi_pass_cell_vortex`` (fsi_band_cell_weights); None drops them, as a new cell list does."""
        if weights is None:
            self._check(self.lib.fsi_band_cell_weights(self.ctx, self.BAND_QUANTITY[quantity], None))
            return
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        n = self._band.get(quantity, self.NO_BAND)["cells"]
        if n and len(w) != n:
            raise ValueError(f"{len(w)} weights, the session has {n} cells")
        self._check(self.lib.fsi_band_cell_weights(self.ctx, self.BAND_QUANTITY[quantity], _ptr(w) if len(w) else None))

    def hi_pass_cell_vortex(self, quantity: str, series: str, first: int = 0, step: int = 1, count: int = -1, cells: bool = True,
                            sums: bool = False):
        """``(cells, sums)`` of the frames ``hi_pass_cell_rate`` would take (fsi_band_cell_vortex).  ``cells`` (5, n) or None: per
        attached cell the ordered mean over the frames of the exact cell means ``VORTEX_FIELDS`` - the Q-criterion
        0.5 (|Omega|^2 - |S|^2), the enstrophy |omega|^2, the helicity w . omega, its absolute value (of the cell mean of each
        frame, not the cell mean of |w . omega|) and |w|^2.  ``sums`` (5,) or None: the ordered sum over the cells of weight
        times each row (``hi_pass_cell_weights`` first; the bracket is that of ``hi_pass.cell_wsum``)."""
        return self._cell_vortex(self.lib.fsi_band_cell_vortex, len(self.VORTEX_FIELDS), quantity, series, first, step, count, cells, sums)

    def _cell_vortex(self, entry, fields: int, quantity: str, series: str, first: int, step: int, count: int, cells: bool, sums: bool):
        """``hi_pass_cell_vortex`` and ``hi_pass_cell_vortex_current``: ``entry`` with outputs of ``fields`` rows."""
        first, step, count, n = self._cell_frames(quantity, series, first, step, count)
        out = np.empty((fields, n)) if cells else None
        total = np.empty(fields) if sums else None
        self._check(entry(self.ctx, self.BAND_QUANTITY[quantity], self.RATE_SERIES[series], first, step, count,
                          _ptr(out) if cells and n else None, _ptr(total) if sums else None))
        return out, total

    VORTEX_CURRENT_FIELDS = VORTEX_FIELDS + ("volume_ratio",)      # FSI_VORTEX_VOLUME_RATIO, hi_pass.VORTEX_CURRENT_FIELDS

    def hi_pass_cell_vortex_current(self, quantity: str, series: str, first: int = 0, step: int = 1, count: int = -1, cells: bool = True,
                                    sums: bool = False):
        """``hi_pass_cell_vortex`` in the current configuration x = X + d(X) (fsi_band_cell_vortex_current): the geometry is the
        history of the 'd' session on the same nodes and frames, paired as ``hi_pass_cell_rate_current`` pairs it.  ``cells``
        (6, n) or None: per attached cell the ordered mean over the frames of the means over the **deformed** cell
        ``VORTEX_CURRENT_FIELDS`` - the five of ``hi_pass_cell_vortex`` with ``grad w F^-1`` for the gradient, and the deformed
        cell's volume over the undeformed.  ``sums`` (6,) or None: the ordered sum over the cells of weight times the same mean
        of each integral per undeformed volume; with the undeformed volumes as weights and one frame, the integrals over the
        current fluid domain and its volume."""
        return self._cell_vortex(self.lib.fsi_band_cell_vortex_current, len(self.VORTEX_CURRENT_FIELDS), quantity, series, first, step, count,
                                 cells, sums)

    def hi_pass_fetch(self, quantity: str, what: str, frame: int, with_max: bool = False):
        """One frame 'raw', 'filtered' or 'amplitude' as (n, ncomp), or 'magnitude' as (n,) (fsi_band_fetch); with
        ``with_max`` (amplitude, magnitude) also the frame's largest magnitude and the first node that has it."""
        n, ncomp = self._band.get(quantity, self.NO_BAND)["shape"]
        out = np.empty(n) if what == "magnitude" else np.empty((n, ncomp))
        mx, am = C.c_double(0.0), C.c_int64(0)
        self._check(self.lib.fsi_band_fetch(self.ctx, self.BAND_QUANTITY[quantity], self.BAND_WHAT[what], int(frame), _ptr(out),
                                            C.byref(mx) if with_max else None, C.byref(am) if with_max else None))
        return (out, mx.value, int(am.value)) if with_max else out

    def hi_pass_export(self, quantity: str, first: int, count: int) -> np.ndarray:
        """Raw frames ``first .. first + count - 1`` of the history as (count, n, ncomp), in one copy (fsi_band_export)."""
        n, ncomp = self._band.get(quantity, self.NO_BAND)["shape"]
        out = np.empty((max(int(count), 0), n, ncomp))
        self._check(self.lib.fsi_band_export(self.ctx, self.BAND_QUANTITY[quantity], int(first), int(count), _ptr(out)))
        return out

    def hi_pass_import(self, quantity: str, frames) -> None:
        """Append exported frames, (count, n, ncomp), to the history as that many samples would have (fsi_band_import)."""
        n, ncomp = self._band.get(quantity, self.NO_BAND)["shape"]
        x = np.ascontiguousarray(frames, dtype=np.float64)
        if x.ndim < 1 or (n and x.size != len(x) * n * ncomp):
            raise FsiError(1, f"hi_pass_import: frames of shape {x.shape}, the open session has frames of {(n, ncomp)}")
        self._check(self.lib.fsi_band_import(self.ctx, self.BAND_QUANTITY[quantity], len(x), _ptr(x)))
        rec = self._band[quantity]
        rec["recorded"] += len(x)
        rec["selected"] = rec["recorded"]

    def hi_pass_end(self, quantity: str) -> None:
        self._check(self.lib.fsi_band_end(self.ctx, self.BAND_QUANTITY[quantity]))
        self._band.pop(quantity, None)

    def hi_pass_room(self, rows: int, capacity: int):
        """(need, available) in bytes: what a band-pass session of ``rows`` rows and ``capacity`` frames takes and what the
        device has for it - the two numbers ``hi_pass_begin`` / ``hi_pass_begin_cells`` compare (fsi_band_room)."""
        need, avail = C.c_double(0.0), C.c_double(0.0)
        self._check(self.lib.fsi_band_room(self.ctx, int(rows), int(capacity), C.byref(need), C.byref(avail)))
        return int(need.value), int(avail.value)

    def hi_pass_board_begin(self, nodes: int, frames: int) -> None:
        """Open the magnitude board, (frames, nodes) FP64 on the device (fsi_board_begin); replaces an open one."""
        self._check(self.lib.fsi_board_begin(self.ctx, int(nodes), int(frames)))

    def hi_pass_board_end(self) -> None:
        self._check(self.lib.fsi_board_end(self.ctx))

    def hi_pass_board_attach(self, quantity: str, node0: int) -> None:
        """From now on an 'amplitude' or 'magnitude' fetch of frame k of the session also stores its magnitudes into
        ``board[k, node0:node0 + n]`` (fsi_band_board_attach); ``node0`` -1 detaches."""
        self._check(self.lib.fsi_band_board_attach(self.ctx, self.BAND_QUANTITY[quantity], int(node0)))

    def hi_pass_board_table(self, first: int, count: int, ranks):
        """(values (count, len(ranks)), NaN counts, maxima, first nodes of the maxima) of ``count`` board frames from
        ``first``: the order statistics at the zero-based ``ranks`` (fsi_board_table)."""
        r = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
        count = int(count)
        values, nans = np.empty((max(count, 0), len(r))), np.zeros(max(count, 0), dtype=np.int64)
        mx, am = np.empty(max(count, 0)), np.zeros(max(count, 0), dtype=np.int64)
        self._check(self.lib.fsi_board_table(self.ctx, int(first), count, len(r), _ptr(r), _ptr(values), _ptr(nans), _ptr(mx), _ptr(am)))
        return values, nans, mx, am

    def order_statistics(self, values, ranks):
        """(np.sort(values)[ranks], number of NaNs) of a host array, selected on the device (fsi_order_statistics)."""
        x = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        r = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
        out, nans = np.empty(len(r)), C.c_int64(0)
        self._check(self.lib.fsi_order_statistics(self.ctx, len(x), _ptr(x), len(r), _ptr(r), _ptr(out), C.byref(nans)))
        return out, int(nans.value)

    SPEC_MODE = {"x": 0, "y": 1, "z": 2, "all": 3, "mag": 4}
    SPEC_SCALING = {"spectrum": 0, "density": 1}
    SPEC_QUANTITY = {"d": 0, "v": 1, "p": 2, "wss": 3}

    def spec_begin(self, quantity: str, nodes, nodes_b=None, component: str = "all", capacity: int = 1) -> None:
        """Open the spectrogram session of ``quantity`` (fsi_spec_begin) on ``nodes`` (as ``hi_pass_begin``; a node may be
        listed twice) for up to ``capacity`` frames.  ``component``: 'x', 'y', 'z', 'all' (the three stacked, component-major)
        or 'mag' (taken when a frame is recorded); the pressure has one.  Raises FsiError when the history does not fit."""
        a = np.ascontiguousarray(nodes, dtype=np.int32)
        b = None if nodes_b is None else np.ascontiguousarray(nodes_b, dtype=np.int32)
        if b is not None and b.shape != a.shape:
            raise ValueError("nodes_b must have the shape of nodes")
        self._check(self.lib.fsi_spec_begin(self.ctx, self.SPEC_QUANTITY[quantity], len(a), _ptr(a), None if b is None else _ptr(b),
                                            self.SPEC_MODE[component], int(capacity)))
        self._spec_shape[quantity] = [len(a) * (3 if component == "all" and quantity != "p" else 1), 0]

    def spec_begin_rows(self, quantity: str, nodes, nodes_b=None, comps=None, capacity: int = 1) -> None:
        """Open the spectrogram session of ``quantity`` on listed rows (fsi_spec_begin_rows): row r is component ``comps[r]``
        (0 .. 2) of ``nodes[r]``, or its mean with ``nodes_b[r]`` where that is >= 0; the pressure takes no ``comps``.  Any
        range of the component-major rows of ``spec_begin(..., "all")`` can be opened so - a strip of a history that does
        not fit the device.  Raises FsiError when the history does not fit."""
        a = np.ascontiguousarray(nodes, dtype=np.int32)
        b = None if nodes_b is None else np.ascontiguousarray(nodes_b, dtype=np.int32)
        c = None if comps is None else np.ascontiguousarray(comps, dtype=np.int32)
        if any(x is not None and x.shape != a.shape for x in (b, c)):
            raise ValueError("nodes_b and comps must have the shape of nodes")
        self._check(self.lib.fsi_spec_begin_rows(self.ctx, self.SPEC_QUANTITY[quantity], len(a), _ptr(a), None if b is None else _ptr(b),
                                                 None if c is None else _ptr(c), int(capacity)))
        self._spec_shape[quantity] = [len(a), 0]

    def spec_begin_wss(self, facet_cells, facet_local, mu: float, dofs, comps, capacity: int = 1) -> None:
        """Open the spectrogram session of the wall shear stress (quantity ``"wss"``, fsi_spec_begin_wss).  ``facet_cells`` /
        ``facet_local``: ALL exterior facets of the fluid, as for ``hemodynamics_begin`` (a cell's projection couples its
        exterior facets).  Row r is component ``comps[r]`` (0 .. 2, or 3: the magnitude) of DG1 dof ``dofs[r]`` of the
        boundary mesh, dof 3 f + k being vertex k of facet f; a dof may be listed twice.  A strip of a longer row list is a
        sub-list.  Raises FsiError when the history does not fit."""
        fc = np.ascontiguousarray(self.cell_u2i[np.asarray(facet_cells, dtype=np.int64)], dtype=np.int32)
        fl = np.ascontiguousarray(facet_local, dtype=np.int32)
        d = np.ascontiguousarray(dofs, dtype=np.int32)
        c = np.ascontiguousarray(comps, dtype=np.int32)
        if fl.shape != fc.shape or c.shape != d.shape or d.ndim != 1:
            raise ValueError("facet_local must have the shape of facet_cells, comps that of dofs")
        self._check(self.lib.fsi_spec_begin_wss(self.ctx, len(fc), _ptr(fc), _ptr(fl), float(mu), len(d), _ptr(d), _ptr(c), int(capacity)))
        self._spec_shape["wss"] = [len(d), 0]

    def spec_room(self, rows: int, capacity: int, magnitude: bool = False):
        """(need, available) in bytes: what a spectrogram session of ``rows`` rows (``magnitude``: of component 'mag') and
        ``capacity`` frames takes and what the device has for it - the two numbers ``spec_begin`` / ``spec_begin_rows``
        compare (fsi_spec_room)."""
        need, avail = C.c_double(0.0), C.c_double(0.0)
        self._check(self.lib.fsi_spec_room(self.ctx, int(rows), int(bool(magnitude)), int(capacity), C.byref(need), C.byref(avail)))
        return int(need.value), int(avail.value)

    def spec_sample(self, quantity: str) -> None:
        """Record the session's rows of dvp_["n"] as the next frame of its history (fsi_spec_sample)."""
        self._check(self.lib.fsi_spec_sample(self.ctx, self.SPEC_QUANTITY[quantity]))
        self._spec_shape[quantity][1] += 1

    def spec_filter(self, quantity: str, b=None, a=None, zi=None, padlen: int = 0) -> None:
        """scipy.signal.filtfilt(b, a, .) of every row, the source of the transforms that follow (fsi_spec_filter); without
        coefficients: the raw series."""
        if b is None:
            self._check(self.lib.fsi_spec_filter(self.ctx, self.SPEC_QUANTITY[quantity], 0, None, None, None, 0))
            return
        b, a, zi = (np.ascontiguousarray(x, dtype=np.float64) for x in (b, a, zi))
        if len(a) != len(b) or len(zi) != len(b) - 1:
            raise ValueError("b and a must have one length, zi one less")
        self._check(self.lib.fsi_spec_filter(self.ctx, self.SPEC_QUANTITY[quantity], len(b), _ptr(b), _ptr(a), _ptr(zi), int(padlen)))

    def _spec_open(self, quantity: str):
        """[rows, recorded frames] of the open session; without one, the library's own refusal."""
        if quantity not in self._spec_shape:
            self._check(self.lib.fsi_spec_sample(self.ctx, self.SPEC_QUANTITY[quantity]))     # "fsi_spec_begin first"
        return self._spec_shape[quantity]

    def spec_fetch(self, quantity: str, frame: int, filtered: bool = False) -> np.ndarray:
        """One frame of the raw or the filtered history: (rows,) (fsi_spec_fetch)."""
        out = np.empty(self._spec_open(quantity)[0])
        self._check(self.lib.fsi_spec_fetch(self.ctx, self.SPEC_QUANTITY[quantity], int(bool(filtered)), int(frame), _ptr(out)))
        return out

    def spec_spectrogram(self, quantity: str, nperseg: int, noverlap: int, nfft: int, window, scaling: str, fs: float) -> np.ndarray:
        """The mean over the rows of scipy.signal.spectrogram's power: (nfft // 2 + 1, segments) (fsi_spec_spectrogram)."""
        w = np.ascontiguousarray(window, dtype=np.float64)
        if w.shape != (int(nperseg),):
            raise ValueError("the window must have nperseg entries")
        frames = self._spec_open(quantity)[1]
        if not 0 <= noverlap < nperseg <= max(frames, 1):
            raise ValueError("needs 0 <= noverlap < nperseg <= recorded frames")
        nseg = (frames - int(noverlap)) // (int(nperseg) - int(noverlap))
        out = np.empty((int(nfft) // 2 + 1, max(nseg, 0)))
        self._check(self.lib.fsi_spec_spectrogram(self.ctx, self.SPEC_QUANTITY[quantity], int(nperseg), int(noverlap), int(nfft), _ptr(w),
                                                  self.SPEC_SCALING[scaling], float(fs), _ptr(out)))
        return out

    def spec_periodogram(self, quantity: str, window, scaling: str, fs: float) -> np.ndarray:
        """The mean over the rows of scipy.signal.periodogram's power: (frames // 2 + 1,) (fsi_spec_periodogram)."""
        w = np.ascontiguousarray(window, dtype=np.float64)
        frames = self._spec_open(quantity)[1]
        if w.shape != (frames,):
            raise ValueError("the window must have one entry per recorded frame")
        out = np.empty(frames // 2 + 1)
        self._check(self.lib.fsi_spec_periodogram(self.ctx, self.SPEC_QUANTITY[quantity], _ptr(w), self.SPEC_SCALING[scaling], float(fs), _ptr(out)))
        return out

    @staticmethod
    def _spec_carry(carry, shape, first_row: int):
        """The carry of a ``_sum`` call as the library takes it: a new one for the first strip, else the caller's own array
        (it is updated in place); none with ``first_row`` > 0 goes to the library as NULL, for its refusal."""
        if carry is None:
            return np.zeros(shape) if int(first_row) == 0 else None
        if not (isinstance(carry, np.ndarray) and carry.dtype == np.float64 and carry.flags.c_contiguous and carry.shape == shape):
            raise ValueError(f"the carry must be a C-contiguous float64 array of shape {shape}")
        return carry

    def spec_spectrogram_sum(self, quantity: str, nperseg: int, noverlap: int, nfft: int, window, scaling: str, fs: float,
                             first_row: int, total_rows: int = 0, carry=None) -> np.ndarray:
        """``spec_spectrogram`` of a session that holds rows ``first_row ...`` of a longer list (fsi_spec_spectrogram_sum):
        ``carry``, (nfft // 2 + 1, segments), the sum over the row blocks before ``first_row`` (None with ``first_row`` 0), is
        updated in place and returned; with ``total_rows`` > 0 - the last strip - it returns the mean over that many rows,
        the bits of ``spec_spectrogram`` on all rows."""
        w = np.ascontiguousarray(window, dtype=np.float64)
        if w.shape != (int(nperseg),):
            raise ValueError("the window must have nperseg entries")
        frames = self._spec_open(quantity)[1]
        if not 0 <= noverlap < nperseg <= max(frames, 1):
            raise ValueError("needs 0 <= noverlap < nperseg <= recorded frames")
        nseg = (frames - int(noverlap)) // (int(nperseg) - int(noverlap))
        carry = self._spec_carry(carry, (int(nfft) // 2 + 1, max(nseg, 0)), first_row)
        self._check(self.lib.fsi_spec_spectrogram_sum(self.ctx, self.SPEC_QUANTITY[quantity], int(nperseg), int(noverlap), int(nfft), _ptr(w),
                                                      self.SPEC_SCALING[scaling], float(fs), int(first_row), int(total_rows),
                                                      None if carry is None else _ptr(carry)))
        return carry

    def spec_periodogram_sum(self, quantity: str, window, scaling: str, fs: float, first_row: int, total_rows: int = 0,
                             carry=None) -> np.ndarray:
        """``spec_periodogram`` with the carry of ``spec_spectrogram_sum``, (frames // 2 + 1,) (fsi_spec_periodogram_sum)."""
        w = np.ascontiguousarray(window, dtype=np.float64)
        frames = self._spec_open(quantity)[1]
        if w.shape != (frames,):
            raise ValueError("the window must have one entry per recorded frame")
        carry = self._spec_carry(carry, (frames // 2 + 1,), first_row)
        self._check(self.lib.fsi_spec_periodogram_sum(self.ctx, self.SPEC_QUANTITY[quantity], _ptr(w), self.SPEC_SCALING[scaling], float(fs),
                                                      int(first_row), int(total_rows), None if carry is None else _ptr(carry)))
        return carry

    def spec_export(self, quantity: str, first: int, count: int) -> np.ndarray:
        """Raw frames ``first .. first + count - 1`` of the history as (count, rows), in one copy (fsi_spec_export)."""
        out = np.empty((max(int(count), 0), self._spec_open(quantity)[0]))
        self._check(self.lib.fsi_spec_export(self.ctx, self.SPEC_QUANTITY[quantity], int(first), int(count), _ptr(out)))
        return out

    def spec_import(self, quantity: str, frames) -> None:
        """Append exported frames, (count, rows), to the history as that many samples would have (fsi_spec_import)."""
        shape = self._spec_open(quantity)
        x = np.ascontiguousarray(frames, dtype=np.float64)
        if x.ndim < 1 or x.size != len(x) * shape[0]:
            raise FsiError(1, f"spec_import: frames of shape {x.shape}, the open session has {shape[0]} rows")
        self._check(self.lib.fsi_spec_import(self.ctx, self.SPEC_QUANTITY[quantity], len(x), _ptr(x)))
        shape[1] += len(x)

    def spec_end(self, quantity: str) -> None:
        self._check(self.lib.fsi_spec_end(self.ctx, self.SPEC_QUANTITY[quantity]))
        self._spec_shape.pop(quantity, None)

    def tuning(self) -> dict:
        """The FsiTuning the context was created with."""
        t = FsiTuning()
        self._check(self.lib.fsi_get_tuning(self.ctx, C.byref(t)))
        return t.as_dict()

    # ---- the solid cycle's coarse level (test hooks of the exact solve, csrc/fsi_bcr.hip) ---------------------------------
    def solid_coarse_info(self) -> dict:
        out = np.zeros(12, dtype=np.int64)
        self._check(self.lib.fsi_solid_coarse_info(self.ctx, _ptr(out)))
        keys = ("nodes", "blocks3x3", "planned", "ready", "bfs_blocks", "levels", "operator_bytes", "launches_per_solve", "max_block",
                "solves", "setup_flops", "cycle_ready")
        return {k: int(v) for k, v in zip(keys, out)}

    def solid_coarse_matrix(self):
        """The coarse operator as scipy CSR (3 unknowns per coarse node)."""
        import scipy.sparse as sp
        info = self.solid_coarse_info()
        nc, nb = info["nodes"], info["blocks3x3"]
        cptr, ccol, cvals = np.empty(nc + 1, dtype=np.int64), np.empty(nb, dtype=np.int32), np.empty(9 * nb, dtype=np.float32)
        self._check(self.lib.fsi_solid_coarse_matrix(self.ctx, _ptr(cptr), _ptr(ccol), _ptr(cvals)))
        return sp.bsr_matrix((cvals.reshape(nb, 3, 3).astype(np.float64), ccol, cptr), shape=(3 * nc, 3 * nc)).tocsr(), cptr, ccol

    def solid_coarse_solve(self, rhs):
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        x = np.empty_like(rhs)
        self._check(self.lib.fsi_solid_coarse_solve(self.ctx, _ptr(rhs), _ptr(x)))
        return x

    def solver_events(self) -> dict:
        """Run totals (since the context was created; timer resets do not touch them) of what the linear solver had to do beyond
        iterating - a cheap read: no device synchronisation, unlike ``timers()``."""
        out = np.zeros(8, dtype=np.int64)
        self._check(self.lib.fsi_get_solver_events(self.ctx, _ptr(out)))
        return {"newton_retries": int(out[0]), "fp32_fallbacks": int(out[1]), "gcr_restarts": int(out[2]),
                "adaptive_solves": int(out[3]), "adaptive_tightened": int(out[4]), "exact_coarse_solves": int(out[5])}

    def timers(self, reset=False) -> dict:
        t = FsiTimers()
        self._check(self.lib.fsi_get_timers(self.ctx, C.byref(t), int(reset)))
        return t.as_dict()
