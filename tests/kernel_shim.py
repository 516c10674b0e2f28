"""ctypes loader of ``vasp_amd/libfsi_kernel_shim.so`` (vasp_amd/csrc/fsi_kernel_shim.hip) and the host-side reference builders
of the kernel tests (tests/test_gpu_gcr_kernels.py, tests/test_gpu_sweep_kernels.py).

The shim runs ONE ``fsi::launch_*`` call of libvaspfsi.so on host arrays; the builders restate, in numpy, what the library's
host code hands those kernels: the LDS tiles of a graph (fsi_capi.hip, node tiles and Schur tiles) and the FP16 records of
k_pack_h1 / k_pack_h3 / k_pack_sb.  The builders are tested on the CPU (tests/test_kernel_references.py), so that a failure
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
    "shim_ctx_info": "ppi", "shim_ctx_array": "psppp", "shim_tile_limit": "",
}
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
        _lib = lib
    return _lib


def _arg(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags.c_contiguous, "shim arguments must be contiguous"
        return a.ctypes.data_as(C.c_void_p)
    return a


def call(name, *args):
    """Run one shim entry point; numpy arrays are passed by pointer (outputs are written in place)."""
    lib = load()
    rc = getattr(lib, name)(*[_arg(a) for a in args])
    if rc != 0:
        raise RuntimeError(f"{name}: {lib.shim_last_error().decode()}")
    return rc


CTX_INFO = ("N2", "V", "nS", "sb_nblocks", "tiled", "tile_nodes", "tile_max_nu", "schur_tiled", "schur_tile", "s_tile_max_nu",
            "sweeps_fp16")
_ELEM = {("f", 4): np.float32, ("f", 8): np.float64, ("i", 1): np.uint8, ("i", 2): np.uint16, ("i", 4): np.int32,
         ("i", 8): np.int64}
_UNSIGNED = {"dd_rec", "vv_rec", "sb_rec", "s_rec"}
_FLOAT = {"dd_chat", "vv_db32", "sb_vals", "sb_binv12", "s_vals", "s_vals32", "s_dinv", "dd_db", "rowscale"}


def ctx_info(ctx) -> dict:
    lib = load()
    out = np.zeros(len(CTX_INFO), dtype=np.int64)
    lib.shim_ctx_info(ctx, _arg(out), len(CTX_INFO))
    return dict(zip(CTX_INFO, (int(v) for v in out)))


def ctx_ktheta(ctx) -> float:
    return float(load().shim_ctx_ktheta(ctx))


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
SCHUR_TILE_LIMIT = 7000      # fsi_capi.hip: distinct columns of a Schur tile (56 KB of LDS as doubles)


def build_tiles(rowptr, cols, rows_per_tile, limit):
    """Tiles of consecutive rows as fsi_capi.hip builds them: per tile the sorted distinct columns of its rows (ulist, tile t at
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
