"""CPU self-tests of the host-side references the kernel tests build on (tests/kernel_shim.py), so that a failure of
tests/test_gpu_gcr_kernels.py, tests/test_gpu_sweep_kernels.py, tests/test_gpu_product_kernels.py,
tests/test_gpu_coarse_kernels.py, tests/test_gpu_bcr_kernels.py or tests/test_gpu_ilu_kernels.py is one of a kernel, not of its
reference."""
import numpy as np
import pytest

import kernel_shim as ks
from vasp_amd import capi


@pytest.mark.parametrize("n,rows_per_tile", [(1, 256), (37, 256), (1000, 128), (1100, 256), (1100, 128), (300, 32), (300, 64)])
def test_tile_builder_covers_every_entry_once(n, rows_per_tile):
    rowptr, cols = ks.local_graph(n, np.random.default_rng(n), reach=48, max_deg=90, diag_only=[0, n - 1])
    uptr, ulist, ploc, max_nu = ks.build_tiles(rowptr, cols, rows_per_tile, ks.TILE_LIMIT)
    nt = (n + rows_per_tile - 1) // rows_per_tile
    assert len(uptr) == nt + 1 and uptr[0] == 0 and uptr[-1] == len(ulist)
    assert max_nu == np.diff(uptr).max()
    row = np.repeat(np.arange(n), np.diff(rowptr))
    tile = row // rows_per_tile
    np.testing.assert_array_equal(ulist[uptr[tile] + ploc], cols)          # every local index names its own column
    for t in range(nt):
        u = ulist[uptr[t]:uptr[t + 1]]
        assert np.all(np.diff(u) > 0)                                    # sorted, distinct
        e0, e1 = rowptr[t * rows_per_tile], rowptr[min(n, (t + 1) * rows_per_tile)]
        np.testing.assert_array_equal(u, np.unique(cols[e0:e1]))         # exactly the tile's columns
    # the launch the tiled kernels get: xcd_span(nt) logical workgroups, each tile taken by exactly one (as fsi_xcd_order says)
    lib = capi.load_library()
    span = lib.fsi_xcd_order(nt, None)
    out = np.full(max(span, 1), -7, dtype=np.int64)
    assert lib.fsi_xcd_order(nt, capi._ptr(out)) == span
    mine = [ks.xcd_unit(L, nt) for L in range(span)]
    np.testing.assert_array_equal(out[:span], mine)
    taken = sorted(t for t in mine if t >= 0)
    assert taken == list(range(nt))


def test_tile_builder_refuses_a_tile_over_the_limit():
    rowptr = np.array([0, 5], dtype=np.int64)
    cols = np.arange(5, dtype=np.int32)
    assert ks.build_tiles(rowptr, cols, 256, 5) is not None
    assert ks.build_tiles(rowptr, cols, 256, 4) is None


def test_fp16_record_emulation_round_trips():
    """the bit layout the shim documents: h1 = half | loc << 16, h3 = (h0 | h1 << 16, h2 | loc << 16), sb = 5 words of halves +
    the column; every finite half bit pattern survives pack / unpack, and the float32 -> half rounding is to nearest even"""
    bits = np.arange(65536, dtype=np.uint32)
    finite = np.isfinite(bits.astype(np.uint16).view(np.float16))
    halves = bits[finite].astype(np.uint16).view(np.float16).astype(np.float32)
    n = len(halves)
    loc = (np.arange(n) * 7919 % 65536).astype(np.uint16)
    rec = ks.pack_h1(halves, loc)
    v, l2 = ks.unpack_h1(rec)
    np.testing.assert_array_equal(rec & 0xFFFF, bits[finite])
    np.testing.assert_array_equal(v.astype(np.float32).view(np.uint32), halves.view(np.uint32))
    np.testing.assert_array_equal(l2, loc)
    m = n // 3
    v3, l3 = ks.unpack_h3(ks.pack_h3(halves[:3 * m], loc[:m]))
    np.testing.assert_array_equal(v3.ravel().astype(np.float32).view(np.uint32), halves[:3 * m].view(np.uint32))
    np.testing.assert_array_equal(l3, loc[:m])
    k = n // 9
    col = (np.arange(k) * 104729).astype(np.int32)
    vs, cs = ks.unpack_sb(ks.pack_sb(halves[:9 * k], col))
    np.testing.assert_array_equal(vs.ravel().astype(np.float32).view(np.uint32), halves[:9 * k].view(np.uint32))
    np.testing.assert_array_equal(cs, col)
    # round to nearest, ties to even: 1 + 2^-11 is halfway between 1 and 1 + 2^-10 and goes to 1; 1 + 3 * 2^-11 goes up
    t = np.array([1 + 2**-11, 1 + 3 * 2**-11, 65519.0, 65520.0, 2**-25, 3 * 2**-26], dtype=np.float32)
    np.testing.assert_array_equal(ks.half_value(ks.half_bits(t)), [1.0, 1 + 2**-9, 65504.0, np.inf, 0.0, 2**-24])


def test_tile_limit_is_the_librarys():
    """the synthetic limit cases build a tile of exactly TILE_LIMIT distinct neighbours: it must be the library's tile_limit()"""
    assert ks.load().shim_tile_limit() == ks.TILE_LIMIT


@pytest.mark.parametrize("fourth", [0, 1])
@pytest.mark.parametrize("lmax,kappa", [(1.7, 30.0), (2.3841, 4.0), (0.93, 1000.0)])
def test_chebyshev_schedule_keeps_the_coefficients(lmax, kappa, fourth):
    """fsi_cheb.hpp against the formulas of the preconditioner before it had one schedule, restated in float64: the
    float32 coefficients the sweep kernels take, and init(), bit for bit; after restart() the schedule starts again"""
    n = 40
    c1, c2, init = np.zeros(2 * n), np.zeros(2 * n), np.zeros(1)
    ks.call("shim_cheb_coefficients", lmax, kappa, fourth, n, c1, c2, init)
    lmax, kappa = np.float64(lmax), np.float64(kappa)
    w1, w2 = np.zeros(n), np.zeros(n)
    if fourth:
        winit = np.float64(4.0) / (np.float64(3.0) * lmax)
        for k in range(n):
            i = np.float64(k + 1)
            w1[k] = (2.0 * i - 1.0) / (2.0 * i + 3.0)
            w2[k] = (8.0 * i + 4.0) / ((2.0 * i + 3.0) * lmax)
    else:
        lmin = lmax / kappa
        th, de = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
        sig = th / de
        rho = 1.0 / sig
        winit = 1.0 / th
        for k in range(n):
            rn = 1.0 / (2.0 * sig - rho)
            w1[k], w2[k] = rn * rho, 2.0 * rn / de
            rho = rn
    assert init[0].tobytes() == np.float64(winit).tobytes()
    for got, want, what in ((c1, w1, "c1"), (c2, w2, "c2")):
        assert np.array_equal(got[:n].view(np.uint64), want.view(np.uint64)), what
        assert np.array_equal(got[:n].astype(np.float32).view(np.uint32), want.astype(np.float32).view(np.uint32)), what
        assert np.array_equal(got[n:].view(np.uint64), got[:n].view(np.uint64)), f"{what} after restart()"
    assert np.all(np.isfinite(c1)) and np.all(c2 > 0) and c1[0] != c1[1]      # (a schedule that moves: the restart is seen)


# ---- the monolithic matrix's references (tests/test_gpu_product_kernels.py) ---------------------------------------------------
def small_mono(N2, V, seed, **kw):
    rng = np.random.default_rng(seed)
    g = ks.mono_graph(N2, V, rng, **kw)
    return rng, g, ks.expand_cols(N2, *g)


MONO_CASES = [(1, 0, {}), (1, 1, {}), (5, 3, dict(diag_only=[2])), (37, 20, dict(heavy=[4], heavy_deg=[30], no_padj=[])),
              (300, 120, dict(heavy=[0, 7], heavy_deg=[100, 60], diag_only=[299], max_deg=20))]


@pytest.mark.parametrize("N2,V,kw", MONO_CASES)
def test_monolithic_layout_is_the_node_graph_expanded(N2, V, kw):
    """expand_cols against a loop over rows: the six columns of every neighbour, ascending, then the pressure columns"""
    rng, (nadj_ptr, nadj, padj_ptr, padj, vrank), (rowptr, cols, diagpos) = small_mono(N2, V, N2 + V, **kw)
    same_node = np.diff(np.repeat(np.arange(N2), np.diff(nadj_ptr))) == 0
    assert np.all(np.diff(nadj)[same_node] > 0)                              # neighbours ascending
    for row in range(6 * N2 + V):
        r = row // 6 if row < 6 * N2 else int(vrank[row - 6 * N2])
        want = [6 * int(s) + e for s in nadj[nadj_ptr[r]:nadj_ptr[r + 1]] for e in range(6)]
        want += [6 * N2 + int(u) for u in padj[padj_ptr[r]:padj_ptr[r + 1]]]
        got = cols[rowptr[row]:rowptr[row + 1]]
        np.testing.assert_array_equal(got, want)
        hit = np.flatnonzero(got == row)
        assert diagpos[row] == (rowptr[row] + hit[0] if len(hit) else -1)
    # every node row has its diagonal; a vertex node meets itself in its pressure neighbours
    assert np.all(diagpos[:6 * N2] >= 0)
    assert np.all(diagpos[6 * N2:] >= 0)


def test_monolithic_graph_reaches_the_edges():
    """the generator's knobs do what the GPU tests rely on: more than 64 neighbours, rows over 256 / 512 entries, a diagonal-only
    node, node rows without pressure columns and pressure rows without a pressure column"""
    N2, V = 400, 150
    nadj_ptr, nadj, padj_ptr, padj, vrank = ks.mono_graph(N2, V, np.random.default_rng(3), heavy=[10, 11], heavy_deg=[95, 50],
                                                         diag_only=[3], no_padj=range(40))
    deg, pdeg = np.diff(nadj_ptr), np.diff(padj_ptr)
    assert deg[10] >= 95 and deg[11] >= 50 and deg[3] == 1 and nadj[nadj_ptr[3]] == 3
    L = 6 * deg + pdeg
    assert L[10] > 512 and 256 < L[11] <= 512
    assert not pdeg[:40].any() and pdeg[40:].any()
    rowptr, cols, diagpos = ks.expand_cols(N2, nadj_ptr, nadj, padj_ptr, padj, vrank)
    nodiag = vrank < 40
    assert nodiag.any() and (~nodiag).any()
    assert np.all(diagpos[6 * N2:][nodiag] == -1) and np.all(diagpos[6 * N2:][~nodiag] >= 0)


@pytest.mark.parametrize("N2,V,kw", MONO_CASES)
def test_padded_layout_covers_every_entry_once(N2, V, kw):
    """pad_copy against a loop over nodes as fsi_setup.hip / k_pad_*32 state it; every entry of A lands once, padding is value 0
    and column 0, the pressure rows follow unpadded; all four L mod 4 are met over the cases"""
    rng, g, (rowptr, cols, diagpos) = small_mono(N2, V, N2 + V + 1, **kw)
    nnz = int(rowptr[-1])
    A = np.arange(1, nnz + 1, dtype=np.float64)                     # exact in FP32 here, and distinct
    for v_rows_only in (False, True):
        cols32, A32, written = ks.pad_copy(N2, rowptr, cols, A, v_rows_only)
        p32, ptail, tail_src, nnz_tail = ks.pad_layout(N2, rowptr)
        assert ptail + nnz_tail == len(A32) and tail_src == rowptr[6 * N2] and nnz_tail == nnz - tail_src
        for r in range(N2):
            s0, L = rowptr[6 * r], rowptr[6 * r + 1] - rowptr[6 * r]
            Lp = (L + 3) // 4 * 4
            assert p32[r + 1] - p32[r] == 6 * Lp and p32[r] % 24 == 0          # 16-byte aligned value and index rows
            assert all(rowptr[6 * r + k] == s0 + k * L for k in range(6))
            np.testing.assert_array_equal(cols32[p32[r] // 6:p32[r] // 6 + Lp], list(cols[s0:s0 + L]) + [0] * (Lp - L))
            for k in range(6):
                blk = A32[p32[r] + k * Lp:p32[r] + (k + 1) * Lp]
                np.testing.assert_array_equal(blk, list(A[s0 + k * L:s0 + (k + 1) * L]) + [0] * (Lp - L))
                assert written[p32[r] + k * Lp:p32[r] + (k + 1) * Lp].all() == (k >= 3 or not v_rows_only)
        np.testing.assert_array_equal(A32[ptail:], A[tail_src:])
        assert written[ptail:].all()
        got = A32[written & (A32 != 0)]
        want = A[:tail_src] if not v_rows_only else A[np.concatenate([np.arange(rowptr[6 * r + 3], rowptr[6 * r + 6]) for r in range(N2)])]
        np.testing.assert_array_equal(np.sort(got), np.sort(np.concatenate([want, A[tail_src:]])))


def test_padded_layout_meets_every_row_length_mod_4():
    seen = set()
    for N2, V, kw in MONO_CASES:
        _, _, (rowptr, _, _) = small_mono(N2, V, N2 + V + 1, **kw)
        seen |= set(((rowptr[6 * np.arange(N2) + 1] - rowptr[6 * np.arange(N2)]) % 4).tolist())
    assert seen == {0, 1, 2, 3}


def pair_matrix(N2, rowptr, rng, nadj_ptr):
    """random values, the d rows reduced to the pair pattern"""
    A = rng.uniform(-1, 1, int(rowptr[-1]))
    entry, slot = ks.drows_entries(N2, rowptr, nadj_ptr)
    A[entry[slot < 0]] = 0.0
    return A


@pytest.mark.parametrize("N2,V,kw", MONO_CASES)
def test_pair_extraction_round_trips(N2, V, kw):
    """extraction then expansion gives the d rows back; the pair values are the entries of columns d_i / v_i of each neighbour,
    found through the column indices (not through positions)"""
    rng, (nadj_ptr, nadj, padj_ptr, padj, vrank), (rowptr, cols, diagpos) = small_mono(N2, V, N2 + V + 2, **kw)
    A = pair_matrix(N2, rowptr, rng, nadj_ptr)
    ad, bad = ks.drows_extract(N2, rowptr, A, nadj_ptr)
    assert not bad and len(ad) == 6 * len(nadj)
    back = ks.drows_expand(N2, rowptr, ad, nadj_ptr, len(A))
    drow = np.zeros(len(A), dtype=bool)
    for r in range(N2):
        drow[rowptr[6 * r]:rowptr[6 * r + 3]] = True
    np.testing.assert_array_equal(back[drow], A[drow])
    assert not back[~drow].any()
    for r in range(N2):
        for i in range(3):
            row = 6 * r + i
            c = dict(zip(cols[rowptr[row]:rowptr[row + 1]].tolist(), A[rowptr[row]:rowptr[row + 1]]))
            for k in range(nadj_ptr[r], nadj_ptr[r + 1]):
                s = int(nadj[k])
                assert ad[6 * k + i] == c[6 * s + i] and ad[6 * k + 3 + i] == c[6 * s + 3 + i]


@pytest.mark.parametrize("where", ["d column", "v column", "pressure column"])
def test_pair_verdict_fires_on_one_off_pattern_entry(where):
    N2, V = 37, 20
    rng, (nadj_ptr, nadj, padj_ptr, padj, vrank), (rowptr, cols, diagpos) = small_mono(N2, V, 9, heavy=[4], heavy_deg=[30])
    A = pair_matrix(N2, rowptr, rng, nadj_ptr)
    assert not ks.drows_extract(N2, rowptr, A, nadj_ptr)[1]
    r = int(np.argmax(np.diff(padj_ptr)))                     # a node with pressure columns
    row = 6 * r + 1                                           # the d_y row of node r
    rc = cols[rowptr[row]:rowptr[row + 1]]
    want = {"d column": lambda c: c < 6 * N2 and c % 6 == 2, "v column": lambda c: c < 6 * N2 and c % 6 == 5,
            "pressure column": lambda c: c >= 6 * N2}[where]
    t = next(t for t, c in enumerate(rc.tolist()) if want(c))
    B = A.copy()
    B[rowptr[row] + t] = 2.0 ** -40
    assert ks.drows_extract(N2, rowptr, B, nadj_ptr)[1]
    # the same entry in a v row is none of the pair form's business
    C = A.copy()
    vrow = 6 * r + 4
    C[rowptr[vrow] + t] = 0.5
    assert not ks.drows_extract(N2, rowptr, C, nadj_ptr)[1]


def test_shim_signatures_match_the_library_source():
    """the ctypes argument codes of kernel_shim against the parameter lists of fsi_kernel_shim.hip (a wrong code would pass a
    pointer where the library reads an int64, and a GPU test would fail for the wrong reason)"""
    import re
    src = (ks.LIB_PATH.parent / "csrc" / "fsi_kernel_shim.hip").read_text()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"^(?:int|double) (shim_\w+)\(([^)]*)\)", src, re.M)}

    def code(param):
        param = " ".join(param.split())
        if "*" in param:
            return "s" if param.startswith("const char*") else "p"
        ty = param.rsplit(" ", 1)[0]
        return {"int64_t": "l", "int": "i", "float": "f", "double": "d"}[ty]
    for name, sig in ks._SIGS.items():
        params = [p for p in decl[name].split(",") if p.strip()]
        assert "".join(code(p) for p in params) == sig, name


# ---- the two-level hierarchy and the coarse-level contracts (kernel_shim.p1_hierarchy, mg_* / sbmg_*) ------------------------
def _mesh(which):
    from vasp_amd.mesh import FsiMesh
    from vasp_amd.meshgen import generate
    from pathlib import Path
    if which == "fixture":
        return FsiMesh.read(Path(__file__).parent / "golden" / "offset_stenosis" / "offset_stenosis.h5")
    g = generate(3000)
    return FsiMesh.from_arrays(g["coords"], g["tets"], g["cell_markers"], g["facets"], g["facet_markers"])


def _cell_graph(tet_nodes, rk, N2):
    """pattern of a matrix on the P2 cell graph (nodes that share a cell), in rank order, as scipy CSR of ones"""
    import scipy.sparse as sp
    t = rk[np.asarray(tet_nodes, dtype=np.int64)]
    i, j = np.repeat(t, 10, axis=1).ravel(), np.tile(t, (1, 10)).ravel()
    G = sp.csr_matrix((np.ones(len(i)), (i, j)), shape=(N2, N2))
    G.data[:] = 1.0
    return G


@pytest.mark.parametrize("which", ["fixture", "generated"])
@pytest.mark.parametrize("order", ["identity", "random"])
def test_p1_hierarchy_is_the_edge_structure(which, order):
    mesh = _mesh(which)
    V, N2 = mesh.num_vertices, mesh.num_nodes
    rng = np.random.default_rng(5)
    rank2node = np.arange(N2) if order == "identity" else rng.permutation(N2)
    rk = np.empty(N2, dtype=np.int64)
    rk[rank2node] = np.arange(N2)
    cells = rng.permutation(len(mesh.tet_nodes))       # the library's cell order is its own: the orientation rule must not care
    h = ks.p1_hierarchy(mesh.tet_nodes[cells], V, rank2node)
    nc, par, pw = h["nc"], h["par"].reshape(-1, 2), h["pw"].reshape(-1, 2)
    assert nc == V
    cfine = h["cfine"].astype(np.int64)
    np.testing.assert_array_equal(cfine, np.flatnonzero(rank2node < V))    # vertices in rank order
    cnode = rank2node[cfine]
    is_v = rank2node < V
    np.testing.assert_array_equal(par[is_v, 0], np.searchsorted(cfine, np.flatnonzero(is_v)))
    np.testing.assert_array_equal(par[is_v, 1], par[is_v, 0])
    np.testing.assert_array_equal(pw[is_v], np.tile([1.0, 0.0], (V, 1)).astype(np.float32))
    # every midpoint's parents are its edge's two ends, weights 1/2
    mid = np.flatnonzero(~is_v)
    ends = np.sort(cnode[par[mid]], axis=1)
    np.testing.assert_array_equal(ends, mesh.edges[rank2node[mid] - V])
    assert (pw[mid] == np.float32(0.5)).all()
    # child / chw: exactly the transpose of par / pw, fine ranks ascending
    P = ks.prolongation(par, pw, nc)
    PT = P.T.tocsr()
    PT.eliminate_zeros()
    PT.sort_indices()
    np.testing.assert_array_equal(h["chptr"], PT.indptr)
    np.testing.assert_array_equal(h["child"], PT.indices)
    np.testing.assert_array_equal(h["chw"], PT.data.astype(np.float32))
    # ccol: exactly the pattern of P^T A P for a matrix A on the P2 cell graph
    G = _cell_graph(mesh.tet_nodes, rk, N2)
    Pat = (abs(P).T @ G @ abs(P)).tocsr()
    Pat.sort_indices()
    np.testing.assert_array_equal(h["cptr"], Pat.indptr)
    np.testing.assert_array_equal(h["ccol"], Pat.indices)
    # the compact solid variant on the nodes of the solid cells
    solid = np.zeros(N2, dtype=bool)
    solid[rk[mesh.tet_nodes[mesh.cell_markers == 2].ravel()]] = True
    snode = np.flatnonzero(solid)
    hs = ks.p1_hierarchy(mesh.tet_nodes[cells], V, rank2node, snode)
    assert hs is not None and hs["nc"] == int((rank2node[snode] < V).sum())
    Ps = ks.prolongation(hs["par"], hs["pw"], hs["nc"])
    # the compact level is the full one restricted to the solid nodes
    cmap = np.full(nc, -1, dtype=np.int64)
    cmap[np.searchsorted(cfine, snode[hs["cfine"]])] = np.arange(hs["nc"])
    Psub = P[snode].tocsc()[:, np.flatnonzero(cmap >= 0)]
    assert abs(Psub - Ps).max() == 0 and Psub.nnz == Ps.nnz
    Gs = G[snode][:, snode]
    Pats = (abs(Ps).T @ Gs @ abs(Ps)).tocsr()
    Pats.sort_indices()
    np.testing.assert_array_equal(hs["cptr"], Pats.indptr)
    np.testing.assert_array_equal(hs["ccol"], Pats.indices)
    # refused: a midpoint in the set without one of its end vertices
    r_mid = snode[~(rank2node[snode] < V)][0]
    end0 = rk[mesh.edges[rank2node[r_mid] - V][0]]
    assert ks.p1_hierarchy(mesh.tet_nodes[cells], V, rank2node, snode[snode != end0]) is None


def test_edge_ends_follow_the_last_cell():
    # two cells share the edge (0, 1), in opposite local order: the later cell decides
    tn = np.array([[0, 1, 2, 3, 4, 5, 6, 7, 8, 9], [1, 0, 2, 10, 11, 12, 6, 13, 14, 9]], dtype=np.int64)
    e = ks.edge_ends(tn, 15, 4)
    assert tuple(e[9]) == (1, 0)            # local edge 5 = (0, 1) of the second cell: vertices 1, 0
    assert tuple(ks.edge_ends(tn[::-1], 15, 4)[9]) == (0, 1)


def test_galerkin_is_the_dense_product():
    import scipy.sparse as sp
    rng = np.random.default_rng(2)
    nf, nc = 23, 7
    par = rng.integers(0, nc, (nf, 2)).astype(np.int32)
    pw = rng.random((nf, 2)).astype(np.float32)
    pw[3] = (1.0, 0.0)
    A = sp.random(nf, nf, density=0.3, random_state=3, format="csr") + sp.eye(nf)
    free = np.ones(nf, dtype=bool)
    free[[2, 11]] = False
    Pd = np.zeros((nf, nc))
    for a in range(nf):
        for k in range(2):
            Pd[a, par[a, k]] += pw[a, k]
    Ad = A.toarray()
    Ad[~free] = 0
    Ad[:, ~free] = 0
    np.testing.assert_allclose(ks.galerkin(ks.prolongation(par, pw, nc), A, free).toarray(), Pd.T @ Ad @ Pd, rtol=1e-14, atol=1e-14)


def _small_level(rng, nc=30, nmid=50, deg=5):
    """a random hierarchy (vertices + midpoints with two distinct parents), its fine graph and the full coarse pattern"""
    import scipy.sparse as sp
    N2 = nc + nmid
    par = np.zeros((N2, 2), dtype=np.int32)
    pw = np.zeros((N2, 2), dtype=np.float32)
    par[:nc, 0] = par[:nc, 1] = np.arange(nc)
    pw[:nc, 0] = 1.0
    a = rng.integers(0, nc, nmid)
    par[nc:, 0], par[nc:, 1] = a, (a + 1 + rng.integers(0, nc - 1, nmid)) % nc
    pw[nc:] = 0.5
    nadj_ptr, nadj = ks.local_graph(N2, rng, reach=N2, max_deg=deg)
    chptr, child, chw = ks.children(par, pw, nc)
    G = sp.csr_matrix((np.ones(len(nadj)), nadj, nadj_ptr), shape=(N2, N2))
    P = ks.prolongation(par, pw, nc)
    Pat = (abs(P).T @ G @ abs(P) + sp.eye(nc)).tocsr()
    Pat.sort_indices()
    return N2, par, pw, nadj_ptr, nadj, chptr, child, chw, Pat.indptr.astype(np.int64), Pat.indices.astype(np.int32), P


def test_mg_rap_reference_is_the_galerkin_product():
    """with dyadic weights every term is exact: the reference's sums equal P^T A0_free P, a0_ab = db_ab / rowscale_a"""
    import scipy.sparse as sp
    rng = np.random.default_rng(4)
    N2, par, pw, nadj_ptr, nadj, chptr, child, chw, cptr, ccol, P = _small_level(rng)
    nc = len(cptr) - 1
    db = rng.standard_normal(3 * len(nadj))
    rowscale = rng.uniform(0.5, 2.0, 6 * N2)
    rowflag = np.zeros(3 * N2, dtype=np.uint8)
    rowflag[3 * np.array([1, 40, 41])] = 1
    Ac, S, L, missed = ks.mg_rap(nc, chptr, child, chw, nadj_ptr, nadj, db, rowscale, rowflag, par, pw, cptr, ccol)
    assert not missed
    row = np.repeat(np.arange(N2), np.diff(nadj_ptr))
    A0 = sp.csr_matrix((db[0::3] / rowscale[6 * row], nadj, nadj_ptr), shape=(N2, N2))
    G = ks.galerkin(P, A0, rowflag[0::3] == 0).toarray()
    crow = np.repeat(np.arange(nc), np.diff(cptr))
    np.testing.assert_allclose(Ac, G[crow, ccol], rtol=0, atol=1e-12 * np.abs(G).max())
    assert (S >= np.abs(Ac)).all() and (L >= (S > 0)).all()
    # a coarse pattern without one of the product's entries: reported in a row of <= 64 entries only
    e = int(np.flatnonzero((ccol != crow) & (S > 0))[0])
    cptr2 = cptr.copy()
    cptr2[crow[e] + 1:] -= 1
    assert ks.mg_rap(nc, chptr, child, chw, nadj_ptr, nadj, db, rowscale, rowflag, par, pw, cptr2, np.delete(ccol, e))[3]


def test_mg_d0_and_finish_identity_rules():
    N2 = 4
    nadj_ptr = np.array([0, 2, 4, 5, 6], dtype=np.int64)
    nadj = np.array([0, 1, 1, 0, 0, 3], dtype=np.int32)        # node 2 has no diagonal
    db = np.arange(1.0, 19.0)
    rowscale = np.full(6 * N2, 2.0)
    rowflag = np.zeros(3 * N2, dtype=np.uint8)
    rowflag[3:6] = 1                                            # node 1: Dirichlet
    d0, mixed = ks.mg_d0(N2, nadj_ptr, nadj, db, rowscale, rowflag)
    np.testing.assert_array_equal(d0, np.float32([1.0 / 2, 0, 0, 16.0 / 2]))
    assert not mixed
    rowflag[7] = 1
    assert ks.mg_d0(N2, nadj_ptr, nadj, db, rowscale, rowflag)[1]
    # finish: row 0 regular, row 1 Dirichlet vertex, row 2 diagonal <= 0, row 3 no diagonal
    cptr = np.array([0, 2, 4, 6, 7], dtype=np.int64)
    ccol = np.array([0, 1, 0, 1, 2, 3, 2], dtype=np.int32)
    Ac = np.array([4.0, -1.0, 2.0, 3.0, -5.0, 1.0, 7.0])
    cfine = np.array([0, 1, 2, 3], dtype=np.int32)
    rowflag = np.zeros(12, dtype=np.uint8)
    rowflag[3] = 1
    cc, cflag, dcinv4, rowmax = ks.mg_coarse_finish(4, cptr, ccol, Ac, cfine, rowflag)
    np.testing.assert_array_equal(cc, np.float32([1.0, -0.25, 0, 1, 1, 0, 0]))
    np.testing.assert_array_equal(cflag, np.repeat(np.uint8([0, 1, 1, 1]), 3))
    np.testing.assert_array_equal(dcinv4.reshape(-1, 4), np.float32([[0.25] * 3 + [0], [0] * 4, [0] * 4, [0] * 4]))
    assert rowmax == np.float32(1.25)


def test_sbmg_finish_identity_rules_and_block_inverse():
    rng = np.random.default_rng(6)
    blocks = [np.diag([3.0, 2.0, 4.0]) + 0.3 * rng.standard_normal((3, 3)),       # regular, non-symmetric
              np.array([[1.0, 2, 0], [0, 0, 0], [0.5, 0, 1]]),                      # det = 0
              np.diag([1.0, 1.0, -1.0]) + np.array([[0, 0.2, 0], [0, 0, 0], [0.1, 0, 0]]),   # det < 0
              np.array([[-1.0, 0, 0.1], [0, -1, 0], [0, 0.3, 1]]),                  # a00 <= 0 with det > 0
              np.diag([2.0, 2.0, 2.0])]                                              # fine vertex flagged
    nc = len(blocks) + 1                                                             # + a row without a diagonal block
    cptr = np.array([0, 2, 3, 4, 5, 6, 7], dtype=np.int64)
    ccol = np.array([0, 5, 1, 2, 3, 4, 0], dtype=np.int32)
    cv = np.zeros((7, 3, 3), dtype=np.float32)
    for i, b in enumerate(blocks):
        cv[cptr[i]] = b
    cv[1] = rng.standard_normal((3, 3))
    cv[6] = rng.standard_normal((3, 3))
    flag = np.array([0, 0, 0, 0, 1, 0], dtype=np.uint8)
    ident, after, inv, a = ks.sbmg_coarse_finish(nc, cptr, ccol, cv.ravel(), np.arange(nc, dtype=np.int32), flag)
    np.testing.assert_array_equal(ident, [False, True, True, True, True, True])
    after = after.reshape(-1, 3, 3)
    np.testing.assert_array_equal(after[:2], cv[:2])                                  # a kept row is untouched
    for e in (2, 3, 4, 5):
        np.testing.assert_array_equal(after[e], np.eye(3))
    np.testing.assert_array_equal(after[6], 0)                                        # no diagonal block: the row is zeroed
    np.testing.assert_allclose(np.asarray(inv[0], dtype=np.float64), np.linalg.inv(cv[0].astype(np.float64)), rtol=1e-13)
    # the extended-precision inverse of non-symmetric blocks is the inverse, not its transpose
    A = rng.standard_normal((50, 3, 3)) + 4 * np.eye(3)
    inv50, _ = ks.inv3(A)
    err = np.abs(np.asarray(inv50, dtype=np.float64) @ A - np.eye(3)).max()
    assert err < 1e-14
    assert np.abs(np.asarray(inv50, dtype=np.float64).transpose(0, 2, 1) @ A - np.eye(3)).max() > 1e-3


def test_sbmg_rap_reference_is_the_block_galerkin_product():
    import scipy.sparse as sp
    rng = np.random.default_rng(8)
    nS, par, pw, sb_ptr, sb_col, chptr, child, chw, cptr, ccol, P = _small_level(rng)
    nc = len(cptr) - 1
    vals = rng.standard_normal(9 * len(sb_col)).astype(np.float32)
    N2 = nS + 5
    snode = np.sort(rng.choice(N2, nS, replace=False)).astype(np.int32)
    rowscale = 2.0 ** rng.integers(-2, 3, 6 * N2).astype(np.float64)     # powers of two: every product below is exact
    flag = np.zeros(nS, dtype=np.uint8)
    flag[[3, 33]] = 1
    cv, S, L, missed = ks.sbmg_rap(nc, chptr, child, chw, sb_ptr, sb_col, vals, snode, rowscale, flag, par, pw, cptr, ccol)
    assert not missed
    row = np.repeat(np.arange(nS), np.diff(sb_ptr))
    isc = 1.0 / rowscale.reshape(-1, 6)[snode, 3:]
    B = vals.reshape(-1, 3, 3).astype(np.float64) * isc[row][:, :, None]
    A = sp.bsr_matrix((B, sb_col, sb_ptr), shape=(3 * nS, 3 * nS)).tocsr()
    G = ks.galerkin(sp.kron(P, sp.eye(3)).tocsr(), A, np.repeat(flag == 0, 3)).toarray()
    crow = np.repeat(np.arange(nc), np.diff(cptr))
    ref = np.stack([G[3 * crow + c, 3 * ccol + t] for c in range(3) for t in range(3)], axis=1)
    np.testing.assert_allclose(cv, ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    # k_sbmg_flags: a node whose second row holds its diagonal alone is flagged
    v2 = vals.reshape(-1, 3, 3).copy()
    i = 7
    v2[sb_ptr[i]:sb_ptr[i + 1], 1, :] = 0
    dg = sb_ptr[i] + int(np.flatnonzero(sb_col[sb_ptr[i]:sb_ptr[i + 1]] == i)[0])
    v2[dg, 1, 1] = 5.0
    f = ks.sbmg_flags(nS, sb_ptr, sb_col, v2.ravel())
    assert f[i] == 1 and f.sum() == 1


# ---- the exact coarse solve by block cyclic reduction (kernel_shim.gj_inverse, tube_graph, bcr_reference) -------------------
def _dominant(m, rng):
    """a non-symmetric, diagonally dominant m x m block"""
    A = rng.standard_normal((m, m))
    return A + np.diag(np.abs(A).sum(axis=1) + 1.0)


@pytest.mark.parametrize("m", [1, 2, 3, 31, 32, 33, 63, 64, 65, 97])
def test_blocked_gauss_jordan_restatement_is_the_inverse(m):
    rng = np.random.default_rng(m)
    A = _dominant(m, rng)
    X, bad = ks.gj_inverse(A)
    ref = np.linalg.inv(A)
    assert not bad
    ai, aa = np.abs(ref), np.abs(A)
    ks.check(X, ref, 8 * (m + 4) * np.finfo(float).eps * (ai @ aa @ ai), f"gj_inverse m={m}")


@pytest.mark.parametrize("k", [0, 31, 32, 33])
def test_blocked_gauss_jordan_restatement_flags_a_zero_pivot(k):
    A = _dominant(40, np.random.default_rng(k))
    A[k, k] = 0.0
    A[k, :] = 0.0
    assert ks.gj_inverse(A)[1]
    B = np.eye(3)
    B[1, 1] = 1.0
    B[0, 1], B[1, 0] = 1.0, 1.0               # the second pivot vanishes only after the first elimination: 1 - 1 * 1
    assert ks.gj_inverse(B)[1]


def test_bcr_tile_builders_cover_every_output_once():
    for M in (1, 15, 16, 17, 63, 64, 65, 130):
        for N in (1, 16, 17, 64, 65, 130):
            hit = np.zeros((M, N), dtype=np.int64)
            for ti, tj in ks.gemm_tiles(M, N):                      # a workgroup: four waves, 32 x 32 each
                for w in range(4):
                    i0, j0 = 64 * ti + 32 * (w >> 1), 64 * tj + 32 * (w & 1)
                    hit[i0:min(i0 + 32, M), j0:min(j0 + 32, N)] += 1
            assert (hit == 1).all(), (M, N)
    for rows in (1, 2, 3, 4, 5, 15, 16, 17, 65, 433):
        got = sorted(r for _, rs in ks.task_tiles(rows) for r in rs)
        assert got == list(range(rows)), rows
    desc, n64, n32, _ = ks.bcr_inverse_layout([1, 33, 2, 65], ld32s=[4, 36, -1, 72])
    used64, used32 = np.zeros(n64, dtype=np.int64), np.zeros(n32, dtype=np.int64)
    for a, o32, cb, rb, m, ld32 in desc:
        for first, count in ((a, m * m), (cb, 32 * m), (rb, 32 * m)):
            used64[first:first + count] += 1
        if o32 >= 0:
            used32[o32:o32 + m * ld32] += 1
    assert (used64 == 1).all() and used32.max() == 1


@pytest.mark.parametrize("tubes", [[[1]], [[1, 10]], [[11, 1, 10]], [[10, 11, 22, 72, 144, 72, 22, 11, 1]],
                                   [[1, 10, 11], [22, 11, 10, 1, 10, 33]], [[1] * 17], [[30, 10, 1, 22, 11, 72, 144, 1]]])
def test_tube_graph_levels_are_the_planners(tubes):
    """the breadth-first levels and the numbering fsi_bcr_plan_graph derives are the rings the generator claims"""
    g = ks.tube_graph(tubes, np.random.default_rng(len(tubes[0])))
    lib = capi.load_library()
    stats = np.zeros(8, dtype=np.int64)
    pos, level = np.empty(g["nc"], dtype=np.int32), np.empty(g["nc"], dtype=np.int32)
    assert lib.fsi_bcr_plan_graph(g["nc"], capi._ptr(g["cptr"]), capi._ptr(g["ccol"]), capi._ptr(stats), capi._ptr(pos),
                                  capi._ptr(level)) == 0
    np.testing.assert_array_equal(level, g["level"])
    np.testing.assert_array_equal(pos, g["pos"])
    assert stats[0] == 1 and stats[1] == len(g["m"]) and stats[2] == g["m"].max()
    assert not np.array_equal(g["pos"], np.arange(g["nc"])) or g["nc"] <= 2
    want = np.zeros(max(len(t) for t in tubes), dtype=np.int64)
    for t in tubes:
        want[:len(t)] += 3 * np.asarray(t[::-1])
    np.testing.assert_array_equal(g["m"], want)


def test_planner_takes_rings_of_666_nodes_and_declines_667():
    lib = capi.load_library()
    for n, usable in ((666, 1), (667, 0)):
        g = ks.tube_graph([[n, 1, n]], np.random.default_rng(n))
        stats = np.zeros(8, dtype=np.int64)
        lib.fsi_bcr_plan_graph(g["nc"], capi._ptr(g["cptr"]), capi._ptr(g["ccol"]), capi._ptr(stats), None, None)
        assert stats[0] == usable and stats[2] == 3 * n


def test_task_table_restatement_is_the_reference_solve():
    """bcr_task_apply on the reference's own FP32 operators, laid out as a task table, is bcr_reference's solve"""
    rng = np.random.default_rng(3)
    g = ks.tube_graph([[1, 10, 11], [22, 11, 10, 1, 10]], rng)
    A = ks.tube_dense(g, ks.tube_values(g, 1e2, rng), 2e-4)
    off = np.concatenate([[0], np.cumsum(g["m"])])
    solve, ops = ks.bcr_reference(A, off, operators=True)
    tasks, a32 = ks.bcr_tasks_of([(lv, k, b, W.astype(np.float32), sg) for lv, k, b, W, sg in ops], off)
    rhs = rng.standard_normal(len(A))
    x = ks.bcr_task_apply(tasks, a32, rhs)
    np.testing.assert_allclose(x, solve(rhs), rtol=0, atol=1e-12 * np.abs(x).max())
    assert np.linalg.norm(A @ x - rhs) <= 1e-5 * np.linalg.norm(rhs)
    assert (ks.bcr_task_apply(tasks, a32, rhs, absolute=True) >= np.abs(x)).all()


# ---- the field split, the Schur complement and the pressure step (kernel_shim.block_structure ... power_lmax) ----------------------
def _product_cases():
    import test_gpu_product_kernels as tp
    return tp.CASES


@pytest.mark.parametrize("name", ["N1_V1", "N5_V3", "N8_V0", "N37_V20", "N1100_V400", "N70001_V9001"])
def test_field_blocks_reassemble_to_the_monolithic_matrix(name):
    """extract_blocks followed by assemble_blocks (K undone) gives back every entry except the pressure columns of the d rows,
    which no block holds"""
    N2, V, kw = _product_cases()[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    g = ks.mono_graph(N2, V, rng, **kw)
    rowptr, cols, _ = ks.expand_cols(N2, *g)
    A = rng.uniform(-1, 1, int(rowptr[-1]))
    solid = (rng.random(N2) < 0.3).astype(np.int32)
    st = ks.block_structure(N2, V, g)
    b = ks.extract_blocks(N2, V, g, A, solid, 0.37)
    back = ks.assemble_blocks(N2, V, g, st, b, solid, 0.37)
    row = np.repeat(np.arange(6 * N2 + V), np.diff(rowptr))
    held = ~((row < 6 * N2) & (row % 6 < 3) & (cols >= 6 * N2))
    assert np.array_equal(np.isnan(back), ~held)
    # exact off the solid columns; on them (e_v + k e_d) - k e_d rounds twice
    err = np.abs(back[held] - A[held])
    assert err.max(initial=0.0) <= 4 * np.finfo(np.float64).eps * (1 + 0.37)
    scol = np.zeros(6 * N2 + V, dtype=bool)
    scol[:6 * N2] = np.repeat(solid != 0, 6) & (np.arange(6 * N2) % 6 >= 3)
    exact = held & ~(scol[cols] & ((row >= 6 * N2) | (row % 6 >= 3)))
    assert np.array_equal(back[exact], A[exact])
    # the structure is a partition: the blocks' sizes add up to the entries held
    sizes = 2 * len(st["cols3"]) * 2 + len(st["cols_vp"]) + 2 * len(st["cols_pv"]) + len(st["cols_pp"])
    assert sizes == held.sum()


def test_schur_restatement_is_the_dense_complement():
    import scipy.sparse as sp
    rng = np.random.default_rng(2)
    N2, V = 60, 25
    g, _ = ks.shaped_graph(N2, V, rng, [(17, 9, True), (16, 0, False)])
    rowptr, _, _ = ks.expand_cols(N2, *g)
    A = rng.uniform(-1, 1, int(rowptr[-1]))
    A[::11] = 0.0
    dpos = ks.expand_cols(N2, *g)[2]
    A[dpos[dpos >= 0]] = rng.uniform(0.5, 2.0, (dpos >= 0).sum())
    solid = (rng.random(N2) < 0.3).astype(np.int32)
    st = ks.block_structure(N2, V, g)
    b = ks.extract_blocks(N2, V, g, A, solid, 0.37)
    sr, sc = ks.schur_pattern(V, st)
    assert all(np.all(np.diff(sc[sr[q]:sr[q + 1]]) > 0) for q in range(V))
    S, mag, L, over = ks.schur_full(V, st, sr, sc, b["Apv"], b["App"], b["Avp"], b["Avv"])
    m = lambda ptr, col, v, sh: sp.csr_matrix((v, col, ptr), shape=sh).toarray()      # noqa: E731
    Apv, Avp = m(st["rowptr_pv"], st["cols_pv"], b["Apv"], (V, 3 * N2)), m(st["rowptr_vp"], st["cols_vp"], b["Avp"], (3 * N2, V))
    dense = m(st["rowptr_pp"], st["cols_pp"], b["App"], (V, V)) - Apv @ np.diag(1.0 / b["Avv"][st["diagpos3"]]) @ Avp
    assert not len(over) and not np.allclose(dense, dense.T)
    got = m(sr, sc, S, (V, V))
    assert np.abs(got - dense).max() <= 64 * np.finfo(np.float64).eps * mag.max()
    assert np.all(dense[m(sr, sc, np.ones(len(sc)), (V, V)) == 0] == 0.0), "the pattern misses an entry of the complement"
    assert L.max() > 8 and np.all(mag >= np.abs(S))


def test_ripple_is_the_hash_of_the_kernel_comment():
    """h = i * 0x9E3779B97F4A7C15, h ^= h >> 29, h *= 0xBF58476D1CE4E5B9, h ^= h >> 32 in 64-bit arithmetic, here with Python's
    unbounded integers reduced by hand"""
    M = (1 << 64) - 1
    ref = []
    for i in range(6):
        h = (i * 0x9E3779B97F4A7C15) & M
        h ^= h >> 29
        h = (h * 0xBF58476D1CE4E5B9) & M
        h ^= h >> 32
        ref.append((h & 0xFFFF) / 65535.0 - 0.5)
    x = ks.ripple(100000)
    assert x[0] == -0.5 and np.array_equal(x[:6], np.array(ref))
    assert x.min() >= -0.5 and x.max() <= 0.5 and abs(x.mean()) < 0.01
    mask = (np.arange(100000) % 3 == 0).astype(np.float64)
    assert np.array_equal(ks.ripple(100000, mask), mask * x)


def test_component_diagonal_restatements():
    rng = np.random.default_rng(4)
    N2, V = 40, 12
    g, _ = ks.shaped_graph(N2, V, rng, [(17, 9, True)])
    st = ks.block_structure(N2, V, g)
    npairs = int(g[0][-1])
    vals = rng.uniform(-1, 1, 9 * npairs)
    db, off = ks.db_extract(N2, g, st, vals)
    assert off
    # the dense 3 N2 x 3 N2 matrix of db is the component-diagonal part of the dense matrix of vals
    import scipy.sparse as sp
    D = sp.csr_matrix((vals, st["cols3"], st["rowptr3"]), shape=(3 * N2, 3 * N2)).toarray()
    keep = (np.arange(3 * N2)[:, None] % 3) == (np.arange(3 * N2)[None, :] % 3)
    x = rng.standard_normal(3 * N2)
    y, S, L = ks.db_terms(N2, g, db, x)
    assert np.allclose(y, (D * keep) @ x, rtol=0, atol=1e-13) and np.all(S >= np.abs(y) - 1e-15)
    assert ks.db_extract(N2, g, st, np.where(keep[np.repeat(np.arange(3 * N2), np.diff(st["rowptr3"])), st["cols3"]], vals, 0.0))[1] is False
    db0 = db.reshape(-1, 3).copy()
    db0[g[0][5]:g[0][6]] = 0.0
    m = ks.rowmask(N2, g, db0.ravel())
    assert m[5] == 0 and m.sum() == N2 - 1
    # chat: identity rows, the reference component, the spread
    r = np.repeat(np.arange(N2), np.diff(g[0]))
    isd = g[1] == r
    c = np.where(isd, 1.0, rng.uniform(0.5, 2, npairs))
    dbc = c[:, None] * np.array([1.0, 2.0, 4.0])
    dbc[(r == 3) & ~isd, 0] = 0.0                      # node 3: component 0 is an identity row, the reference is component 1
    dbc[(r == 4) & ~isd] = 0.0                         # node 4: all identity
    chat, flag, spread = ks.chat_extract(N2, g, dbc.ravel())
    assert np.array_equal(chat, np.where((r == 4), isd.astype(float), c)) and spread.max() == 0.0
    assert flag.reshape(-1, 3)[3].tolist() == [1, 0, 0] and flag.reshape(-1, 3)[4].tolist() == [1, 1, 1]
    e = np.flatnonzero((r == 7) & ~isd)[0]
    dbc[e, 2] *= 1 + 1e-6
    assert 1e-7 < ks.chat_extract(N2, g, dbc.ravel())[2].max() < 1e-5


def test_power_iteration_restatement_finds_the_largest_eigenvalue():
    rng = np.random.default_rng(5)
    n = 50
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.linspace(0.1, 1.0, n)
    lam[-1] = 3.0
    A = Q @ np.diag(lam) @ Q.T
    d = np.full(n, 2.0)
    got = ks.power_lmax(lambda x: A @ x, lambda y: y / d, n)
    assert abs(got - 1.5) < 1e-6
    mask = (np.arange(n) < 30).astype(np.float64)
    got = ks.power_lmax(lambda x: A @ x, lambda y: mask * y / d, n, mask)
    assert abs(got - np.abs(np.linalg.eigvals((A / d[:, None])[:30, :30])).max()) < 1e-3
    assert abs(ks.power_lmax(lambda x: A.astype(np.longdouble) @ x, lambda y: y / d, n, dtype=np.longdouble) - 1.5) < 1e-6


def test_the_block_cases_reach_the_edges():
    import test_gpu_block_kernels as tb
    c = tb.graph_case("N700_V300")
    deg, pdeg = np.diff(c["g"][0]), np.diff(c["g"][2])
    assert {1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 100} <= set(deg.tolist())
    assert {0, 1, 7, 8, 9, 17, 24} <= set(pdeg.tolist())
    vdeg = deg[c["g"][4]]                                  # k_pres_rhs32: the strips a pressure row takes
    for lo, hi in ((1, 16), (17, 48), (49, 64), (65, 1000)):
        assert ((vdeg >= lo) & (vdeg <= hi)).any()
    assert [tb.CASES[k][0] for k in ("N1_V1", "N31_V9", "N32_V32", "N33_V17")] == [1, 31, 32, 33]
    for name, (covered, size) in tb.CAPS.items():
        assert size > covered, name
    # the over-limit Schur row exists in the case meant to have one and in no other
    for name in tb.CASES:
        cc = tb.graph_case(name)
        assert np.diff(ks.schur_pattern(cc["V"], cc["st"])[0]).max(initial=0) <= ks.SCHUR_ROW_LIMIT
    for longest, n_over in ((1024, 0), (1025, 1)):
        N2, g = tb.limit_graph(longest)
        lens = np.diff(ks.schur_pattern(N2, ks.block_structure(N2, N2, g))[0])
        assert lens[0] == 1024 and lens[1] == longest and (lens > ks.SCHUR_ROW_LIMIT).sum() == n_over
    # the solid sets: none, all, about a tenth, the heavy nodes
    for kind, lo, hi in (("none", 0, 0), ("all", 700, 700), ("tenth", 40, 110), ("heavy", 8, 40)):
        s = tb.blocks_case("N700_V300", kind)["solid"]
        assert lo <= s.sum() <= hi, kind
    assert np.all(deg[tb.blocks_case("N700_V300", "heavy")["solid"] != 0] >= 47)
    b = tb.blocks_case("N700_V300")["b"]
    assert (b["Apv"] == 0).any() and np.signbit(b["Avp"][b["Avp"] == 0]).any()


# ---- multicolour ILU(0) and its triangular solves (tests/test_gpu_ilu_kernels.py) ---------------------------------------------
ILU_MIXED = [(40, 6), (33, 6), (1, 6), (0, 6), (25, 1), (17, 1)]


@pytest.mark.parametrize("symmetric", [True, False])
def test_level_matrix_obeys_the_level_contract(symmetric):
    m = ks.level_matrix(ILU_MIXED, np.random.default_rng(3), symmetric=symmetric, zero_lower=0.1)
    n, rowptr, cols, diagpos, vals = m["n"], m["rowptr"], m["cols"], m["diagpos"], m["vals"]
    assert n == 6 * 74 + 42 and len(rowptr) == n + 1
    assert ks.level_violations(ILU_MIXED, rowptr, cols) == 0
    row = np.repeat(np.arange(n), np.diff(rowptr))
    assert np.all((np.diff(cols) > 0) | (np.diff(row) > 0))                  # ascending, distinct columns in every row
    np.testing.assert_array_equal(cols[diagpos], np.arange(n))              # a diagonal entry in every row
    assert 20 <= np.diff(rowptr).mean() <= 70
    off = np.zeros(n)
    np.add.at(off, row, np.abs(vals))
    off -= np.abs(vals[diagpos])
    assert np.all(np.abs(vals[diagpos]) > off)                              # strictly dominant by rows
    assert np.count_nonzero(vals[cols < row] == 0.0) > 10                    # exactly zero lower entries
    # rows reference their own group below AND above themselves, and other levels
    g = m["group_of"]
    same = g[row] == g[cols]
    assert np.any(same & (cols > row)) and np.any(same & (cols < row)) and np.any(~same)
    import scipy.sparse as sp
    P = sp.csr_matrix((np.ones(len(cols)), cols, rowptr), shape=(n, n))
    assert ((P != P.T).nnz == 0) == symmetric
    # a violation is seen
    bad = cols.copy()
    r = int(m["first"][0]) + 2                                               # row 2 of group 0 of level 0 -> a column of group 1
    bad[rowptr[r]] = 6
    assert ks.level_violations(ILU_MIXED, rowptr, bad) == 1


def test_level_matrix_row_lengths_and_diagonal_positions():
    levels = [(40, 6), (200, 6), (30, 1), (20, 1)]
    n = 40 * 6 + 200 * 6 + 50
    heavy = [3, n - 5, 250, 251, 252, 253, 1447, 1460]
    m = ks.level_matrix(levels, np.random.default_rng(5), heavy=heavy, heavy_len=[1024, 1024, 1, 63, 64, 65, 129, 1025],
                        diag_first=[3], diag_last=[n - 5], isolated=[1460])
    L = np.diff(m["rowptr"])
    assert [int(L[r]) for r in heavy] == [1024, 1024, 1, 63, 64, 65, 129, 1025]
    assert m["diagpos"][3] == m["rowptr"][3] and m["diagpos"][n - 5] == m["rowptr"][n - 4] - 1
    assert ks.level_violations(levels, m["rowptr"], m["cols"]) == 0
    row = np.repeat(np.arange(n), L)
    assert np.count_nonzero((m["cols"] == 1460) & (row != 1460)) == 0        # no other row depends on the isolated one
    assert L[np.setdiff1d(np.arange(n), heavy)].max() <= ks.ILU_MAXROW


def test_own_group_only_matrix_is_block_diagonal_and_well_conditioned():
    m = ks.level_matrix([(7, 6), (3, 1), (5, 6)], np.random.default_rng(8), own_group_only=True)
    import scipy.sparse as sp
    A = sp.csr_matrix((m["vals"], m["cols"], m["rowptr"]), shape=(m["n"],) * 2).toarray()
    g = m["group_of"]
    assert np.all(A[g[:, None] != g[None, :]] == 0.0)
    for k in np.unique(g):
        B = A[np.ix_(g == k, g == k)]
        assert np.all(B != 0.0) and np.linalg.cond(B) < 100


def test_ilu0_identity_accepts_the_plain_factor_and_sees_each_fault():
    """What makes the GPU test of k_ilu0_level meaningful: a plain FP64 IKJ factor passes the identity check, and each of the three
    ways the kernel could be subtly wrong - a missed update, the unfactored pivot of a row of the same group, an update applied
    to the neighbouring column - fails it."""
    for symmetric in (True, False):
        m = ks.level_matrix(ILU_MIXED, np.random.default_rng(11), symmetric=symmetric, zero_lower=0.1)
        rp, co, dp, A = m["rowptr"], m["cols"], m["diagpos"], m["vals"]
        LU, _ = ks.ilu0_ikj(rp, co, dp, A)
        err, bound = ks.ilu0_identity(rp, co, dp, A, LU)
        r = ks.worst_ratio(err, bound)
        print(f"plain IKJ factor (symmetric {symmetric}): worst error / bound {r:.3f}")
        assert r <= 1.0
        e64, b64 = ks.ilu0_identity_f64(rp, co, dp, A, LU)                   # the scipy form of the same check
        assert ks.worst_ratio(e64, 2 * b64) <= 1.0
        np.testing.assert_allclose(np.asarray(b64, dtype=np.float64), np.asarray(bound, dtype=np.float64), rtol=1e-12)
        for fault in ("drop_update", "stale_pivot", "neighbour_column"):
            bad, applied = ks.ilu0_ikj(rp, co, dp, A, group_of=m["group_of"], fault=fault)
            assert applied, fault
            err, bound = ks.ilu0_identity(rp, co, dp, A, bad)
            assert ks.worst_ratio(err, bound) > 1e3, fault
            e64, b64 = ks.ilu0_identity_f64(rp, co, dp, A, bad)
            assert ks.worst_ratio(e64, 2 * b64) > 1e3, fault


def test_ilu0_identity_is_exact_lu_on_block_diagonal_matrices():
    m = ks.level_matrix([(5, 6), (4, 1)], np.random.default_rng(12), own_group_only=True)
    LU, _ = ks.ilu0_ikj(m["rowptr"], m["cols"], m["diagpos"], m["vals"])
    import scipy.sparse as sp
    lu = sp.csr_matrix((LU, m["cols"], m["rowptr"]), shape=(m["n"],) * 2).toarray()
    A = sp.csr_matrix((m["vals"], m["cols"], m["rowptr"]), shape=(m["n"],) * 2).toarray()
    Lf, Uf = np.tril(lu, -1) + np.eye(m["n"]), np.triu(lu)
    assert np.abs(Lf @ Uf - A).max() <= 50 * ks.EPS64 * np.abs(A).max()


def test_sptrsv_residuals_accept_a_plain_solve_and_see_a_wrong_one():
    m = ks.level_matrix(ILU_MIXED, np.random.default_rng(13), symmetric=False)
    rp, co, dp = m["rowptr"], m["cols"], m["diagpos"]
    LU, _ = ks.ilu0_ikj(rp, co, dp, m["vals"])
    n = m["n"]
    rhs = np.random.default_rng(14).standard_normal(n)
    y, x = np.zeros(n), np.zeros(n)
    for i in range(n):
        s, d = rp[i], dp[i]
        y[i] = rhs[i] - np.dot(LU[s:d], y[co[s:d]])
    for i in range(n - 1, -1, -1):
        d, e = dp[i], rp[i + 1]
        x[i] = (y[i] - np.dot(LU[d + 1:e], x[co[d + 1:e]])) / LU[d]
    ef, bf, eb, bb = ks.sptrsv_residuals(rp, co, dp, LU, rhs, y, x)
    assert ks.worst_ratio(ef, bf) <= 1.0 and ks.worst_ratio(eb, bb) <= 1.0
    import scipy.sparse as sp
    lu = sp.csr_matrix((LU, co, rp), shape=(n, n)).toarray()
    ref = np.linalg.solve(np.triu(lu), np.linalg.solve(np.tril(lu, -1) + np.eye(n), rhs))
    assert np.abs(x - ref).max() <= 1e-12 * np.abs(ref).max()
    y2 = y.copy()
    y2[n // 2] *= 1 + 1e-12                                                  # a stale value in one row
    ef, bf, eb, bb = ks.sptrsv_residuals(rp, co, dp, LU, rhs, y2, x)
    assert ks.worst_ratio(ef, bf) > 10 and ks.worst_ratio(eb, bb) > 10
    x2 = x.copy()
    x2[5] = x[6]
    assert ks.worst_ratio(*ks.sptrsv_residuals(rp, co, dp, LU, rhs, y, x2)[2:]) > 1e3


def test_f32_ripple4_reference():
    x = ks.f32_ripple4(1000).reshape(-1, 4)
    assert np.all(x[:, 3] == 0) and np.all(np.abs(x[:, :3]) <= 1) and np.all(x[:, :3] * 512 == np.round(x[:, :3] * 512))
    # node 300: h = (300 * 2654435761 mod 2^32) xor 2, by hand in Python integers
    h = ((300 * 2654435761) & 0xFFFFFFFF) ^ (300 >> 7)
    np.testing.assert_array_equal(x[300, :3], [(h & 1023) / 512 - 1, ((h >> 10) & 1023) / 512 - 1, ((h >> 20) & 1023) / 512 - 1])
    assert len(np.unique(x[:, 0])) > 300                                      # not a constant
    big = ks.f32_ripple4(4096 * 256 + 257).reshape(-1, 4)                     # node numbers beyond 2^20: the product needs 64 bits
    i = 4096 * 256 + 200
    h = ((i * 2654435761) & 0xFFFFFFFF) ^ (i >> 7)
    assert big[i, 2] == ((h >> 20) & 1023) / 512 - 1


# ---- the element kernels' references (kernel_shim.element_structure ... probe_reference; tests/test_gpu_element_*.py) ------------
def test_element_structure_names_the_right_columns_and_incidences():
    """for every cell and local pair, cols[rowptr[row] + 6 enbr + 3 f + c] and the epnbr position are the column's dof; the dofs are
    what k_residual computes from the ranks; the incidence lists hold every (cell, local node) once, under its owner, ascending"""
    for case in (ks.element_cases("tube").prefix(700), ks.element_cases("hand3"), ks.element_cases("jac")):
        es = case.es
        dofs = es.cell_dofs.astype(np.int64)
        pos = ks.element_positions(es)
        np.testing.assert_array_equal(es.cols[pos], np.broadcast_to(dofs[:, None, :], pos.shape))
        assert pos.min() >= 0 and np.all(pos < es.rowptr[dofs + 1][:, :, None]) and np.all(pos >= es.rowptr[dofs][:, :, None])
        lane = np.arange(60)
        np.testing.assert_array_equal(dofs[:, :60], 6 * es.cell_rank[:, lane % 10].astype(np.int64) + 3 * (lane // 30) + (lane % 30) // 10)
        np.testing.assert_array_equal(dofs[:, 60:], es.cell_prow)
        np.testing.assert_array_equal(es.vrank[es.cell_prow - 6 * es.N2], es.cell_rank[:, :4])       # a pressure row sits at its vertex
        for ptr, lst, owner, nloc in ((es.inc_ptr, es.inc, es.cell_rank, 10), (es.pinc_ptr, es.pinc, es.cell_prow - 6 * es.N2, 4)):
            assert len(lst) == nloc * es.C == ptr[-1] and len(np.unique(lst)) == len(lst)
            own = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
            np.testing.assert_array_equal(owner[lst >> 4, lst & 15], own)
            inside = np.ones(len(lst), dtype=bool)
            inside[ptr[:-1][np.diff(ptr) > 0]] = False                       # first entry of every owner
            assert np.all(np.diff(lst.astype(np.int64))[inside[1:]] > 0)
    # a shifted epnbr index names another column (or leaves the row): the check above would catch it
    es = ks.element_cases("hand3").es
    bad = es.epnbr.copy()
    bad[1, 2, 3] += 1
    import copy
    es2 = copy.copy(es)
    es2.epnbr = bad
    pos = ks.element_positions(es2)
    hit = np.minimum(pos, len(es.cols) - 1)
    assert not np.array_equal(es.cols[hit], np.broadcast_to(es.cell_dofs.astype(np.int64)[:, None, :], pos.shape))


def test_element_local_reordering():
    l = np.arange(64)
    re = ks.re_from_oracle(l)
    for f in range(2):
        for c in range(3):
            for a in range(10):
                assert re[6 * a + 3 * f + c] == 30 * f + 10 * c + a
    np.testing.assert_array_equal(re[60:], [60, 61, 62, 63])
    x = np.random.default_rng(0).standard_normal((5, 64))
    np.testing.assert_array_equal(ks.oracle_from_re(ks.re_from_oracle(x)), x)
    np.testing.assert_array_equal(ks.re_from_oracle(ks.oracle_from_re(x)), x)


def test_geometry_reference_inverts_the_edge_matrix():
    case = ks.element_cases("tube")
    inv, det, J = ks.geometry_reference(case.coords, case.tets)
    assert (det > 0).any() and (det < 0).any()                              # vertex-sorted cells come in both orientations
    assert np.abs(inv @ J - np.eye(3)).max() < 1e-15
    bi, bd = ks.geometry_bound(case.coords, case.tets)
    J64 = J.astype(np.float64)
    from oracle.fsi_oracle import _inv3
    inv64, det64 = _inv3(J64)                                               # the adjugate in FP64, as k_geometry
    assert np.all(np.abs(inv64 - inv) <= bi)
    assert np.all(np.abs(det64 - det) <= bd)
    np.testing.assert_array_equal(case.geom[:, 9], np.abs(det).astype(np.float64))


def test_fp64_oracles_stay_within_a_quarter_of_the_residual_block_bounds():
    """K_RESIDUAL is 4 x what the oracle's own FP64 evaluation orders reach against extended precision on the tests' inputs: the
    constants cannot be loosened without this failing to be tight, and the inputs are benign (no block of any cell is lost to
    cancellation).  A reference with one pressure weight off by 1e-6, or without the last cell, is far outside the bound."""
    r = ks.measure_residual_ratios()
    for name in ("numpy", "c"):
        assert np.all(r[name] <= ks.K_RESIDUAL / 4), (name, r[name])
    assert np.all(np.maximum(r["numpy"], r["c"]) >= ks.K_RESIDUAL / 8 - 1e-9)       # and K is not more than 8 x the measurement
    case = ks.element_cases("tube").prefix(17)
    ref = case.residual_reference()
    o = case.oracle(ks.LD)
    o.L = o.L.copy()
    o.L[5, 2] *= 1 + 1e-6                                                    # a deliberately wrong table entry
    wrong = case.residual_reference(o)
    q = ks.block_ratios(wrong, ref, case.kind)
    assert q[0, 2] > 1e3 * ks.K_RESIDUAL[0, 2]
    err = np.abs(wrong - ref) > ks.block_bound(ref, case.kind, ks.K_RESIDUAL)
    assert err[case.kind == 0][:, 60:].any() and not err[case.kind == 1][:, 60:].any()
    short = ref.copy()
    short[-1] = 0
    assert (np.abs(short - ref) > ks.block_bound(ref, case.kind, ks.K_RESIDUAL))[-1].any()


def test_fp64_oracles_stay_within_a_quarter_of_the_jacobian_block_bounds():
    r = ks.measure_jacobian_ratios()
    for name in ("numpy", "c"):
        assert np.all(r[name] <= ks.K_JACOBIAN / 4), (name, r[name])
    assert np.all(np.maximum(r["numpy"], r["c"]) >= ks.K_JACOBIAN / 8 - 1e-9)
    case = ks.element_cases("jac")
    for k in (0, 1):
        assert (case.kind == k).sum() >= 60 and len(np.unique(case.region[case.kind == k])) == (2, 3)[k]
    assert len(np.unique(case.tet_nodes)) == 10 * case.C                     # no two cells share a node


def test_sequential_gather_is_the_ordered_sum():
    es = ks.element_cases("tube").prefix(300).es
    Re = np.random.default_rng(3).integers(-1000, 1000, (es.C, 64)).astype(np.float64)     # integers: every order gives the same sum
    F = np.concatenate([ks.sequential_gather(Re, es.inc_ptr, es.inc, 6, 0).ravel(), ks.sequential_gather(Re, es.pinc_ptr, es.pinc, 1, 60).ravel()])
    ref = ks.assembled(es, ks.oracle_from_re(Re)).astype(np.float64)
    np.testing.assert_array_equal(F, ref)
    # order: 1e16, 1, -1e16 gives 0 in list order and would give 1 in any order that meets the large terms first
    ptr, lst = np.array([0, 3]), np.array([0, 16, 32], dtype=np.int32)
    R3 = np.zeros((3, 64))
    R3[:, 0] = (1e16, 1.0, -1e16)
    assert ks.sequential_gather(R3, ptr, lst, 6, 0)[0, 0] == 0.0


def test_l2_statistics_and_probe_references():
    case = ks.element_cases("tube").prefix(5)
    o = case.oracle(np.float64)
    val, bound = ks.l2_reference(case, case.Us)
    assert abs(o.function_norm(case.U) ** 2 - float(val)) <= float(bound)
    drop = ks.l2_reference(case.prefix(4), case.Us)[0]                       # the last cell of an odd C dropped: far outside the bound
    assert abs(float(drop - val)) > 1e6 * float(bound)
    sv, bv, sj, bj = ks.cell_stats_reference(case, np.zeros(case.es.ndof))
    assert np.all(sv == 0) and np.all(np.abs(sj - 1) < 1e-14)        # the tabulated weights sum to 1/6 to 2e-15
    # an affine displacement d = A x has det(I + A) everywhere, and v = const its own length
    A = np.array([[0.1, 0.02, 0.0], [0.0, -0.05, 0.03], [0.01, 0.0, 0.2]])
    X = np.zeros(6 * case.N2 + case.V)
    X[:3 * case.N2] = (case.node_coords @ A.T).ravel()
    X[3 * case.N2:6 * case.N2] = np.tile([3.0, 4.0, 12.0], case.N2)
    sv, bv, sj, bj = ks.cell_stats_reference(case, case.to_solver(X))
    assert np.all(np.abs(sv - 13) <= bv + 1e-16) and np.all(np.abs(sj - np.linalg.det(np.eye(3) + A)) <= bj + 1e-12)
    cells = np.array([0, 3, 4], dtype=np.int32)
    bary = np.array([[0, 1.0, 0, 0], [0.5, 0, 0.5, 0], [0.1, 0.2, 0.3, 0.4]])
    got, b = ks.probe_reference(case, cells, bary, case.to_solver(X))
    x = np.einsum("na,nai->ni", bary, case.coords[case.tets[cells]])
    assert np.abs(got[:, :3] - x @ A.T).max() < 1e-15 and np.abs(got[:, 3:6] - [3.0, 4.0, 12.0]).max() < 1e-14


# ---- the host side of the recycled GCR (fsi_gcr_host.hpp through the shim, against kernel_shim's restatements) ----------------
@pytest.mark.parametrize("cap,ring,batch", [(8, 4, 2), (200, 64, 32)])
def test_gcr_store_replays_a_scripted_run(cap, ring, batch):
    """3 cap directions, retiring whenever the store is full: slots, born, free list and window after every operation"""
    sizes = np.zeros(10, dtype=np.int64)
    ks.call("shim_gcr_sizes", cap, 5, sizes)
    assert list(sizes[:4]) == [ks.GCR_WINDOW, ks.GCR_FLUSH_BATCH, ring, batch] == [32, 32, ks.gcr_ring(cap), ks.gcr_retire_batch(cap)]
    # the staging buffer: coefficients, their two sums, what rides along, the window's area behind the largest pass, all inside
    coef, sums, lagged, updated, window, size = (int(v) for v in sizes[4:])
    assert (sums, lagged, updated) == (5, 7, 7) and coef >= cap + 4 and window >= cap + 4 and size >= window + ks.GCR_WINDOW + 2
    ref = ks.GcrStoreRef(cap)

    def both(op, *arg):
        got, state = ks.gcr_store_op(cap, op, *arg)
        want = getattr(ref, op)(*arg) if op != "init" else None
        assert state == ref.state(), (op, arg)
        return got, want
    both("init", cap)
    cleared, retired_ever = [], set()
    for k in range(3 * cap):
        (full,), want = both("full")
        assert bool(full) == want == (k >= cap and not ref.free)
        if full:
            age = list(ref.born)
            gone, want = both("retire", batch)
            assert gone == want and len(gone) == batch
            assert all(age[s] >= cap - ring for s in gone) and all(ref.born[s] < 0 for s in gone)
            assert sorted(age[s] for s in gone) == sorted(b for b in age if b >= cap - ring)[:batch]          # the oldest of the ring
            cols, want = both("window_drop_retired")
            assert cols == want
            assert not set(gone) & {s for s in ref.hot if s >= 0}                  # a retired slot leaves the window
            retired_ever |= set(gone)
        else:
            gone = []
        hw_before = ref.hw
        (slot, clear), want = both("take")
        assert (slot, bool(clear)) == want
        assert bool(clear) == (slot >= hw_before)          # beyond the old high-water mark: reported for clearing ...
        if clear:
            cleared.append(slot)
        (col,), want = both("window_put", slot)
        assert col == want == k % ks.GCR_WINDOW
        both("set_born", slot)
        assert ref.born[slot] == k
        (nh,), want = both("window_cols")
        assert nh == want
        # no direction born before cap - ring is ever retired: the first cap - ring directions are all still there
        assert sorted(b for b in ref.born if 0 <= b < cap - ring) == list(range(min(k + 1, cap - ring)))
    assert cleared == list(range(cap))                     # ... exactly once
    assert retired_ever and all(s >= cap - ring for s in retired_ever)          # (slot = birth index while the store grew)
    both("clear_window")
    both("reset")
    assert ref.state() == ([-1] * cap, [], [-1] * ks.GCR_WINDOW, (0, 0, 0))


@pytest.mark.parametrize("cap,nold,knew", [(8, 3, 1), (8, 3, 5), (40, 8, 32)])
def test_gcr_cycle_algebra_expands_the_directions(cap, nold, knew):
    """sum_j cn[k][j] Z_j against the recursively defined p_k, and sum_j y[j] Z_j against sum_k alpha_k p_k, in np.longdouble,
    n = 40; coefficients on older slots and on directions of the same cycle, some exactly zero, one on the direction's own
    slot (ignored).  Every direction of a cycle sits in a slot of its own, so 32 of them need a store of more than 8: that
    case runs at cap = 40 with 8 older directions.  The flush arrays: y, then gcr_flush_width(knew) columns."""
    n = 40
    rng = np.random.default_rng(100 * cap + knew)
    Z = rng.standard_normal((cap, n))
    slots = np.arange(nold, nold + knew, dtype=np.int32)
    ms = (slots + 1).astype(np.int32)                      # the store grows: every pass scans the slots so far, its own included
    htot = rng.standard_normal((knew, cap))
    htot[rng.random((knew, cap)) < 0.2] = 0.0
    for k in range(knew):
        htot[k, ms[k]:] = np.nan                           # never read
    wn, alpha = rng.uniform(0.5, 2.0, knew), rng.standard_normal(knew)
    y, cn = np.full(cap, 7.0), np.full((knew, cap), 7.0)
    m = int(ms[-1])
    kw = ks.load().shim_gcr_flush_width(knew)
    pack = np.full((kw + 1) * m, 7.0)
    ks.call("shim_gcr_cycle_algebra", cap, knew, slots, ms, htot, wn, alpha, y, cn, m, pack)
    P, X, bound = ks.gcr_cycle_reference(cap, Z, slots, ms, htot, wn, alpha)
    EP, EX = bound(cn)
    LD = np.longdouble
    ks.check((cn.astype(LD) @ Z.astype(LD)).astype(np.float64), P.astype(np.float64), EP + 1e-18 * np.abs(P).astype(np.float64), "p_k")
    ks.check((y.astype(LD) @ Z.astype(LD)).astype(np.float64), X.astype(np.float64), EX + 1e-18 * np.abs(X).astype(np.float64), "x")
    assert np.all(EP <= 1e-9 * (np.abs(cn) @ np.abs(Z))) and np.all(cn[:, m:] == 0) and np.all(y[m:] == 0)
    want = np.zeros((kw + 1, m))
    want[0], want[1:knew + 1] = y[:m], cn[:, :m]
    np.testing.assert_array_equal(pack, want.ravel())


def test_gcr_cycle_end_rule_at_its_thresholds():
    R = 1.0          # |r| the cycle was entered with
    rows = [  # since_gain, f32, rnorm, target, store_full -> 0 go, 1 stagnated, 2 stalled
        (39, 0, 99e-9, 1e-9, 0, 0), (40, 0, 99e-9, 1e-9, 0, 1), (40, 0, 101e-9, 1e-9, 0, 0), (39, 0, 101e-9, 1e-9, 0, 0),
        (39, 1, 1e-2, 1e-9, 0, 0), (40, 1, 1e-2, 1e-9, 0, 1), (40, 1, 101e-9, 1e-9, 0, 1), (39, 1, 99e-9 + 1e-3, 1e-9, 0, 0),
        (5, 1, 1e-4 * R, 1e-9, 0, 0), (6, 1, 1e-4 * R, 1e-9, 0, 1), (6, 1, 1.01e-4 * R, 1e-9, 0, 0), (6, 0, 1e-4 * R, 1e-9, 0, 0),
        (127, 0, 1e-2, 1e-9, 1, 0), (128, 0, 1e-2, 1e-9, 1, 2), (128, 0, 1e-2, 1e-9, 0, 0), (127, 0, 1e-2, 1e-9, 0, 0),
        (128, 1, 1e-2, 1e-9, 1, 1)]
    for since, f32, rnorm, target, full, want in rows:
        got = ks.status("shim_gcr_cycle_end", since, f32, rnorm, target, R, full)
        assert got == want == ks.gcr_cycle_end_ref(since, f32, rnorm, target, R, full), (since, f32, rnorm, target, full)


def test_gcr_orthogonality_test_at_the_floors():
    """disc / canc = | |w'|^2 - (|w|^2 - |h|^2) | / |w'|^2 / sqrt(|w|^2 / |w'|^2) against orth_floor32 = 3e-7 and orth_floor64 = 1e-9"""
    h = np.array([3.0, 4.0, 0.0, 12.0])                    # |h|^2 = 169, |w|^2 = 170: |w|^2 - |h|^2 = 1 exactly
    for floor in (3e-7, 1e-9):
        for factor, want in ((0.9, 0), (1.1, 1)):
            d = factor * floor * np.sqrt(170.0)            # wn2 = 1 + d: disc = d / wn2, canc = sqrt(170 / wn2)
            wn2 = 1.0 + d
            got = ks.status("shim_gcr_orth_lost", h, 4, 170.0, wn2, floor)
            assert got == want == int(ks.gcr_orth_lost_ref(h, 170.0, wn2, floor)), (floor, factor)
    assert ks.status("shim_gcr_orth_lost", h, 4, 170.0, 0.0, 1e-9) == 0 and ks.status("shim_gcr_orth_lost", h, 4, 0.0, 1.0, 1e-9) == 0


def test_gcr_verdict_policies_term_by_term():
    # FP64 basis, verdict due: a quiet first cycle is not judged; every term alone makes it due
    quiet = dict(rtol=1e-5, rnorm=0.9e-5, bnorm=1.0, cyc=0, cycle_its=64, stagnated=0, stalled=0, store_full=0, fell_back=0, suspect=0)
    cases = [({}, 0), (dict(rtol=0.99e-8, rnorm=1e-9), 1), (dict(rtol=1e-8, rnorm=0.9e-8), 0), (dict(fell_back=1), 1), (dict(store_full=1), 1),
             (dict(cycle_its=65), 1), (dict(stalled=1), 1), (dict(stagnated=1), 1), (dict(suspect=1), 1), (dict(cyc=1), 1),
             (dict(rnorm=1.01e-5), 1), (dict(rnorm=1e-5), 0)]
    for change, want in cases:
        a = list({**quiet, **change}.values())
        assert ks.status("shim_gcr_verdict_due", *a) == want == int(ks.gcr_verdict_due_ref(*a)), change
    # FP32 basis, verdict may be skipped: everything in favour skips; every term alone forbids it
    fine = dict(rtol=1e-3, rnorm=0.9e-3, bnorm=1.0, cyc=0, cycle_its=32, stagnated=0, stalled=0, store_full=0, in_newton=1, final_cycle=1,
                skip_rtol=3e-4, last_drift=0.9e-5)
    cases = [({}, 1), (dict(in_newton=0), 0), (dict(final_cycle=0), 0), (dict(rtol=2.9e-4, rnorm=1e-4, last_drift=1e-6), 0),
             (dict(rtol=3e-4, rnorm=1e-4, last_drift=1e-6), 1), (dict(rnorm=1.01e-3), 0), (dict(rnorm=1e-3), 1), (dict(cycle_its=33), 0),
             (dict(stagnated=1), 0), (dict(last_drift=-1.0), 0), (dict(last_drift=0.0), 1), (dict(last_drift=1.01e-5), 0),
             (dict(stalled=1, store_full=1, cyc=3), 1)]
    for change, want in cases:
        a = list({**fine, **change}.values())
        assert ks.status("shim_gcr_verdict_skippable", *a) == want == int(ks.gcr_verdict_skippable_ref(*a)), change


def test_gcr_tolerance_policies():
    """the second-pass threshold, where an adaptive solve starts and how it tightens, the storage of a lifetime's basis"""
    def run(f32=0, part=0, rtol_floor=1e-5, forced=0.0, rtol=1e-3, utol=0.0, ratio=0.0, floor=1e-6, bu=1.0, ru=1.0, hint=0.0, f32floor=1e-7):
        out = np.zeros(4)
        ks.call("shim_gcr_tolerances", np.array([f32, part, rtol_floor, forced, rtol, utol, ratio, floor, bu, ru, hint, f32floor], dtype=np.float64), out)
        return out
    assert run(f32=1)[0] == 0.01 and run(f32=1, part=1)[0] == 0.01 and run(f32=1, forced=0.3)[0] == 0.3
    assert run(rtol_floor=1e-5)[0] == 0.01 and run(rtol_floor=1e-12)[0] == 0.5 and run(rtol_floor=1e-10)[0] == 1.0 / (1e-10 * 9e10)
    assert run(rtol_floor=1e-5, part=1)[0] == 0.1 and run(rtol_floor=1e-12, part=1)[0] == 0.5 and run(part=1, forced=0.02)[0] == 0.02
    assert run(rtol=1e-3)[1] == 1e-3 and run(rtol=1e-3, utol=1e-4, ratio=0.0)[1] == 1e-3          # not adaptive / nothing known yet
    assert run(rtol=1e-3, utol=1e-4, ratio=2.0)[1] == 0.7 * 1e-4 / 2.0 and run(rtol=1e-3, utol=1e-4, ratio=1e-3)[1] == 1e-3
    assert run(rtol=1e-3, utol=1e-4, ratio=1e6)[1] == 1e-6 and run(rtol=1e-6, utol=1e-4, ratio=1e6, floor=1e-6)[1] == 1e-6
    assert run(rtol=1e-3, utol=1e-4, ru=1e-4)[2] == 0.5e-3 and run(rtol=1e-3, utol=1e-4, ru=1e-3)[2] == 1e-3 * 0.05
    assert run(rtol=1e-3, utol=1e-4, ru=1.0)[2] == 1e-3 * 0.02 and run(rtol=1e-5, utol=1e-4, ru=1.0, floor=1e-6)[2] == 1e-6
    assert run(rtol=1e-6)[3] == 1 and run(rtol=1e-7)[3] == 0 and run(rtol=1e-3, hint=1e-8)[3] == 0 and run(rtol=1e-8, hint=1e-3)[3] == 0
    assert run(rtol=1e-3, hint=1.1e-7)[3] == 1
