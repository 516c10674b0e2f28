"""ctypes loader of ``vasp_amd/libfsi_kernel_shim.so`` (vasp_amd/csrc/fsi_kernel_shim.hip) and the host-side reference builders
of the kernel tests (tests/test_gpu_gcr_kernels.py, tests/test_gpu_sweep_kernels.py, tests/test_gpu_product_kernels.py).

The shim runs ONE ``fsi::launch_*`` call of libvaspfsi.so on host arrays; the builders restate, in numpy, what the library's
host code hands those kernels: the LDS tiles of a graph (fsi_capi.hip, node tiles and Schur tiles), the FP16 records of
k_pack_h1 / k_pack_h3 / k_pack_sb, and the monolithic matrix's column layout, padded FP32 copy and d-row pair form.  The builders are tested on the CPU (tests/test_kernel_references.py), so that a failure
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
    "shim_expand_cols": "llpppppppp", "shim_spmv": "lpppplpi", "shim_spmv_node6": "llpppppplppp", "shim_drows_extract": "lpppppp",
    "shim_pad_cols32": "lpppp", "shim_pad_vals32": "llppplllpli", "shim_spmv_node6p": "llppplpplppplppp",
    "shim_matrix_finish": "lppppplpp", "shim_ctx_spmv": "pippp",
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
            "sweeps_fp16", "a32_ptail", "a32_tail_src", "a32_tail_nnz", "op32_ok", "kry_fp32", "drows_ok")
_ELEM = {("f", 4): np.float32, ("f", 8): np.float64, ("i", 1): np.uint8, ("i", 2): np.uint16, ("i", 4): np.int32,
         ("i", 8): np.int64}
_UNSIGNED = {"dd_rec", "vv_rec", "sb_rec", "s_rec"}
_FLOAT = {"dd_chat", "vv_db32", "sb_vals", "sb_binv12", "s_vals", "s_vals32", "s_dinv", "dd_db", "rowscale", "A", "A32", "Ad64", "Ad32"}


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


# ---- the monolithic matrix: structure, padded FP32 copy, d rows in pair form (fsi_solver.hip, fsi_capi.hip) ------------------
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
    """The FP32 copy's layout (fsi_capi.hip): node r's six value rows padded to Lp = L rounded up to a multiple of 4, block at
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
