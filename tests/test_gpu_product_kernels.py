"""The monolithic matrix's structure kernels (vasp_amd/csrc/fsi_solver.hip) and outer products (fsi_product.hip), one launch at a
time through the test shim, against FP64 restatements of their contracts (tests/kernel_shim.py) on the exact values the kernels hold:

    k_expand_cols, k_pad_cols32, k_pad_vals32 (+ k_round_to_f32), k_drows_extract, k_matrix_finish     bitwise
    k_spmv, k_spmv_node6 (+ k_spmv_prow), k_spmv_node6c, k_spmv_node6p, k_spmv_node6pc                |y - A x| <= (L + 8) eps S

with S = sum_j |a_ij x_j| per row, a_ij the FP64 values or the FP32 copy's own float values, and the reference summed in extended
precision.  The FP32 forms are also held against the FP64 matrix, with 2^-24 S added.  A dropped, doubled or misplaced entry misses
these bounds by orders of magnitude; every y entry starts as NaN, so an unwritten one fails too.

a) synthetic node graphs (nodes with more than 64 neighbours, rows over 256 and 512 entries, a diagonal-only node, pressure rows
with and without pressure columns, N2 from 1 to past every capped grid, V = 0), b) live contexts with the FP32 operator pinned:
their structure, FP32 copy and pair form against the same restatements, and the product the Krylov iterations run."""
import functools

import numpy as np
import pytest

import kernel_shim as ks

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
U32 = 2.0 ** -24
check = ks.check

# name: (N2, V, mono_graph knobs).  70001 nodes: not a multiple of 8, more than the 8192-block grids of k_pad_* / k_spmv and the
# 16384 blocks of k_drows_extract cover in one pass (four nodes or rows per block)
CASES = {
    "N1_V1": (1, 1, {}),
    "N5_V3": (5, 3, dict(diag_only=[2])),
    "N8_V0": (8, 0, dict(heavy=[3], heavy_deg=[8])),
    "N37_V20": (37, 20, dict(heavy=[4], heavy_deg=[30], no_padj=[0, 1, 2])),
    "N1100_V400": (1100, 400, dict(max_deg=14, heavy=[0, 500, 1099], heavy_deg=[100, 70, 50], diag_only=[7], no_padj=range(20, 40))),
    "N70001_V9001": (70001, 9001, dict(max_deg=6, heavy=[3, 40000, 70000], heavy_deg=[100, 60, 45], diag_only=[11],
                                       no_padj=range(100, 130))),
}
SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -(1 + 2.0 ** -24), 0.1, 1 / 3, 2.0 ** -126,
                    3.0e-39, -1.0e-40, 1.0e-46, 0.999999999])


@functools.lru_cache(maxsize=1)
def case(name):
    """graph, layout, a matrix with random entries everywhere (A) and one with its d rows in the pair pattern (Ap), and x"""
    N2, V, kw = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    g = ks.mono_graph(N2, V, rng, **kw)
    rowptr, cols, diagpos = ks.expand_cols(N2, *g)
    nnz = int(rowptr[-1])
    A = rng.uniform(-1, 1, nnz)
    A[:min(nnz, len(SPECIAL))] = SPECIAL[:nnz]
    Ap = A.copy()
    entry, slot = ks.drows_entries(N2, rowptr, g[0])
    Ap[entry[slot < 0]] = 0.0
    x = rng.standard_normal(6 * N2 + V)
    return dict(N2=N2, V=V, g=g, rowptr=rowptr, cols=cols, diagpos=diagpos, A=A, Ap=Ap, x=x)


def test_the_cases_reach_the_edges():
    big = case("N70001_V9001")
    L = np.diff(big["rowptr"])
    deg = np.diff(big["g"][0])
    assert deg.max() > 64 and L.max() > 512 and ((L > 256) & (L <= 512)).any()
    assert big["N2"] % 8 and big["N2"] > 4 * 16384
    assert (big["diagpos"][6 * big["N2"]:] < 0).any() and (big["diagpos"][6 * big["N2"]:] >= 0).any()
    assert set((L[:6 * big["N2"]] % 4).tolist()) == {0, 1, 2, 3}


# ---- structure ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_expand_cols(name):
    c = case(name)
    N2, V = c["N2"], c["V"]
    n = 6 * N2 + V
    cols = np.full(len(c["cols"]), -7, dtype=np.int32)
    diagpos = np.full(n, -9, dtype=np.int64)
    ks.call("shim_expand_cols", N2, V, *c["g"], c["rowptr"], cols, diagpos)
    np.testing.assert_array_equal(cols, c["cols"])
    has = c["diagpos"] >= 0
    np.testing.assert_array_equal(diagpos[has], c["diagpos"][has])
    assert np.all(diagpos[~has] == -9), "k_expand_cols wrote a diagonal position for a row without a diagonal"


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", CASES)
def test_padded_fp32_copy(name):
    c = case(name)
    N2, V, rowptr = c["N2"], c["V"], c["rowptr"]
    p32, ptail, tail_src, nnz_tail = ks.pad_layout(N2, rowptr)
    cols32 = np.full(ptail // 6, -5, dtype=np.int32)
    ks.call("shim_pad_cols32", N2, rowptr, c["cols"], p32, cols32)
    for v_rows_only in (0, 1):
        ref_cols, ref, written = ks.pad_copy(N2, rowptr, c["cols"], c["A"], bool(v_rows_only))
        np.testing.assert_array_equal(cols32, ref_cols)
        extra = 5                                              # entries past the copy: nobody writes them
        A32 = np.full(ptail + nnz_tail + extra, np.float32(-3.25))
        ks.call("shim_pad_vals32", N2, V, rowptr, c["A"], p32, ptail, nnz_tail, tail_src, A32, len(A32), v_rows_only)
        w = np.concatenate([written, np.zeros(extra, dtype=bool)])
        bad = np.flatnonzero(bits32(A32[w]) != bits32(ref[written]))
        assert not len(bad), (f"v_rows_only={v_rows_only}: {len(bad)} entries differ from float32(A) / padding 0; first at "
                              f"{np.flatnonzero(w)[bad[0]]}: {A32[w][bad[0]]!r} against {ref[written][bad[0]]!r}")
        assert np.all(A32[~w] == np.float32(-3.25)), f"v_rows_only={v_rows_only}: an entry outside the written rows changed"


@pytest.mark.parametrize("name", CASES)
def test_drows_extract(name):
    c = case(name)
    N2, rowptr, nadj_ptr = c["N2"], c["rowptr"], c["g"][0]
    npairs = int(nadj_ptr[-1])
    ref, bad = ks.drows_extract(N2, rowptr, c["Ap"], nadj_ptr)
    assert not bad
    nodes = rowptr[6 * N2]
    for A, want_flag, with32 in ((c["Ap"], 0, True), (c["Ap"], 0, False), (c["A"], 1, True)):
        ad64 = np.full(6 * npairs, np.nan)
        ad32 = np.full(6 * npairs, np.float32(np.nan)) if with32 else None
        flag = np.zeros(1, dtype=np.int32)
        ks.call("shim_drows_extract", N2, rowptr, np.ascontiguousarray(A[:nodes]), nadj_ptr, ad64, ad32, flag)
        r64 = ks.drows_extract(N2, rowptr, A, nadj_ptr)[0]
        np.testing.assert_array_equal(ad64.view(np.uint64), r64.view(np.uint64))
        if with32:
            np.testing.assert_array_equal(bits32(ad32), bits32(r64.astype(np.float32)))
        assert flag[0] == want_flag
    # one off-pattern entry in the last node's d rows (the last round of the grid-stride loop): a pressure column if it has one,
    # else a d column of another component
    r = N2 - 1
    row = 6 * r + 2
    rc = c["cols"][rowptr[row]:rowptr[row + 1]]
    t = len(rc) - 1 if rc[-1] >= 6 * N2 else 0
    assert rc[t] >= 6 * N2 or rc[t] % 6 != 2
    B = c["Ap"][:nodes].copy()
    B[rowptr[row] + t] = 2.0 ** -60
    flag = np.zeros(1, dtype=np.int32)
    ks.call("shim_drows_extract", N2, rowptr, B, nadj_ptr, np.zeros(6 * npairs), None, flag)
    assert flag[0] == 1


@pytest.mark.parametrize("n", [1, 37, 20011])
def test_matrix_finish(n):
    """A + Apre, then identity on rows whose maximum is below 3e-16 (ident_zeros) and on Dirichlet rows, else row scaling by
    1.0 / max; rows just above and below the threshold, empty rows, rows longer than 64, a grid-stride loop (20011 rows)"""
    rng = np.random.default_rng(n)
    L = rng.integers(1, 40, n)
    L[rng.random(n) < 0.1] = 0
    long_ = rng.random(n) < 0.05
    L[long_] = rng.integers(65, 700, long_.sum())
    if n >= 37:
        L[:8] = [0, 1, 63, 64, 65, 128, 129, 600]
    rowptr = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    nnz = int(rowptr[-1])
    diagpos = rowptr[:-1] + (rng.random(n) * np.maximum(L, 1)).astype(np.int64)
    A = rng.uniform(-1, 1, nnz) * 10.0 ** rng.uniform(-3, 3, nnz)
    Apre = np.where(rng.random(nnz) < 0.3, rng.uniform(-1, 1, nnz), 0.0)
    row = np.repeat(np.arange(n), L)
    kind = rng.integers(0, 6, n)                     # 0: below 3e-16, 1: just above, 2: exactly 3e-16, 3: cancels to ~1e-17
    for q in np.flatnonzero((kind <= 3) & (L > 0)):
        s, e = rowptr[q], rowptr[q + 1]
        v = rng.uniform(-1, 1, e - s)
        v /= np.abs(v).max()
        top = {0: np.nextafter(3.0e-16, 0.0), 1: np.nextafter(3.0e-16, 1.0), 2: 3.0e-16, 3: 1.0e-17}[int(kind[q])]
        A[s:e] = v * top
        Apre[s:e] = 0.0
        if kind[q] == 3:
            A[s:e] += 0.75
            Apre[s:e] = -0.75
    bc = rng.choice(n, size=max(1, n // 20), replace=True).astype(np.int32)
    # reference
    v = A + Apre
    mx = np.zeros(n)
    nz = L > 0
    mx[nz] = np.maximum.reduceat(np.abs(v), rowptr[:-1][nz]) if nnz else 0.0
    isbc = np.zeros(n, dtype=bool)
    isbc[bc] = True
    ident = (mx < 3.0e-16) | isbc
    assert (ident & ~isbc & (mx > 0)).any() or n == 1
    sc = np.where(ident, 1.0, 1.0 / np.where(ident, 1.0, mx))
    ref = np.where(ident[row], (np.arange(nnz) == diagpos[row]).astype(np.float64), v * sc[row])
    Ag, rs, mask = A.copy(), np.full(n, np.nan), np.full(n, 5, dtype=np.int32)
    ks.call("shim_matrix_finish", n, rowptr, diagpos, Ag, Apre, bc, len(bc), rs, mask)
    np.testing.assert_array_equal(mask, isbc.astype(np.int32))
    np.testing.assert_array_equal(rs.view(np.uint64), sc.view(np.uint64))
    bad = np.flatnonzero(Ag.view(np.uint64) != ref.view(np.uint64))
    assert not len(bad), f"{len(bad)} entries differ; first {bad[0]} (row {row[bad[0]]}): {Ag[bad[0]]!r} against {ref[bad[0]]!r}"


# ---- products ----------------------------------------------------------------------------------------------------------------
def run_product(kind, c, A, x, graph=True, n32=None):
    """one product through the shim; y starts as NaN"""
    N2, V, rowptr, cols = c["N2"], c["V"], c["rowptr"], c["cols"]
    nadj_ptr, nadj, _, _, vrank = c["g"]
    n = 6 * N2 + V
    y = np.full(n, np.nan)
    gv = (vrank, nadj_ptr, nadj) if graph else (None, None, None)
    npairs = len(nadj)
    if kind.startswith("generic"):
        ks.call("shim_spmv", n, rowptr, cols, A, x, n, y, int(kind[-1]))
    elif kind in ("node6", "node6c"):
        ad = ks.drows_extract(N2, rowptr, A, nadj_ptr)[0] if kind == "node6c" else None
        ks.call("shim_spmv_node6", N2, V, rowptr, cols, A, *gv, npairs, x, y, ad)
    else:
        p32, ptail, tail_src, nnz_tail = ks.pad_layout(N2, rowptr)
        cols32, A32, written = ks.pad_copy(N2, rowptr, cols, A, kind == "node6pc")
        A32[~written] = np.nan                                 # value rows 0 .. 2 of a pair-form copy: never read
        ad = ks.drows_extract(N2, rowptr, A, nadj_ptr)[0].astype(np.float32) if kind == "node6pc" else None
        ks.call("shim_spmv_node6p", N2, V, p32, cols32, A32, len(A32), rowptr, cols, ptail - tail_src, *gv, npairs, x, y, ad)
    unwritten = int(np.isnan(y).sum())
    assert not unwritten, f"{kind} graph={graph}: {unwritten} of {n} y entries not written"
    return y


@pytest.mark.parametrize("name", CASES)
def test_fp64_products(name):
    c = case(name)
    rowptr, cols, x = c["rowptr"], c["cols"], c["x"]
    ref, S, L = ks.csr_product(rowptr, cols, c["A"], x)
    bound = (L + 8) * EPS * S
    for kind, graph in (("generic0", True), ("generic1", True), ("generic2", True), ("node6", True), ("node6", False)):
        check(run_product(kind, c, c["A"], x, graph), ref, bound, f"{kind} graph={graph}")
    # the d rows in pair form, against the same matrix's six-row product and its reference
    refp, Sp, _ = ks.csr_product(rowptr, cols, c["Ap"], x)
    yc = run_product("node6c", c, c["Ap"], x)
    check(yc, refp, (L + 8) * EPS * Sp, "node6c")
    check(yc, run_product("node6", c, c["Ap"], x), 2 * (L + 8) * EPS * Sp, "node6c against node6 on the same matrix")


@pytest.mark.parametrize("name", CASES)
def test_fp32_copy_products(name):
    c = case(name)
    rowptr, cols, x = c["rowptr"], c["cols"], c["x"]
    for A, kinds in ((c["A"], (("node6p", True), ("node6p", False))), (c["Ap"], (("node6p", True), ("node6pc", True)))):
        ref32, S32, L = ks.csr_product(rowptr, cols, A.astype(np.float32), x)
        ref64, S64, _ = ks.csr_product(rowptr, cols, A, x)
        ys = {}
        for kind, graph in kinds:
            y = run_product(kind, c, A, x, graph)
            check(y, ref32, (L + 8) * EPS * S32, f"{kind} graph={graph} against its float values")
            check(y, ref64, (L + 8) * EPS * S32 + U32 * S64, f"{kind} graph={graph} against the FP64 matrix")
            ys[kind, graph] = y
        if ("node6pc", True) in ys:
            check(ys["node6pc", True], ys["node6p", True], 2 * (L + 8) * EPS * S32, "node6pc against node6p on the same matrix")


def test_pair_form_without_the_node_graph_is_refused():
    """ad32 / ad64 without nadj_ptr or nadj: the launchers launch nothing and say so (the six-row kernels would read value rows
    0 .. 2, which a copy made with v_rows_only does not hold)"""
    c = case("N37_V20")
    N2, V, rowptr, cols, x = c["N2"], c["V"], c["rowptr"], c["cols"], c["x"]
    nadj_ptr, nadj, _, _, vrank = c["g"]
    n = 6 * N2 + V
    p32, ptail, tail_src, nnz_tail = ks.pad_layout(N2, rowptr)
    cols32 = np.zeros(ptail // 6, dtype=np.int32)
    ks.call("shim_pad_cols32", N2, rowptr, cols, p32, cols32)
    A32 = np.full(ptail + nnz_tail, np.float32(np.nan))
    ks.call("shim_pad_vals32", N2, V, rowptr, c["Ap"], p32, ptail, nnz_tail, tail_src, A32, len(A32), 1)
    ad64 = ks.drows_extract(N2, rowptr, c["Ap"], nadj_ptr)[0]
    ad32 = ad64.astype(np.float32)
    for ptr, nb in ((nadj_ptr, None), (None, nadj), (None, None)):
        y = np.full(n, 17.0)
        rc = ks.status("shim_spmv_node6p", N2, V, p32, cols32, A32, len(A32), rowptr, cols, ptail - tail_src, vrank, ptr, nb,
                       len(nadj), x, y, ad32)
        assert rc == ks.LAUNCH_REFUSED, rc
        assert np.all(y == 17.0), "launch_spmv_node6p wrote y after refusing"
        y = np.full(n, 17.0)
        rc = ks.status("shim_spmv_node6", N2, V, rowptr, cols, c["Ap"], vrank, ptr, nb, len(nadj), x, y, ad64)
        assert rc == ks.LAUNCH_REFUSED, rc
        assert np.all(y == 17.0), "launch_spmv_node6 wrote y after refusing"


# ---- b) live contexts: the structure, the FP32 copy and the pair form of an assembled Jacobian, and the product the Krylov
# iterations run -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generated_case(tmp_path_factory):
    from conftest import prepare_case
    from vasp_amd.meshgen import write_mesh
    tmp = tmp_path_factory.mktemp("productgen")
    write_mesh(tmp / "s.h5", 12000)
    return prepare_case("offset_stenosis", tmp / "s.h5", tmp / "run", dt="0.001", T="0.002")


@pytest.fixture(scope="module", params=[("fixture", 0), ("fixture", 1), ("generated", 0), ("generated", 1)],
                ids=lambda p: f"{p[0]}-compact{p[1]}")
def live_op(request, stenosis_case, generated_case):
    from vasp_amd.capi import HipBackend
    from test_gpu_parity import boundary_data, random_state
    which, compact = request.param
    case_ = stenosis_case if which == "fixture" else generated_case
    ns, desc = case_[0], case_[1]
    hb = HipBackend(desc, tuning=dict(krylov_fp32=1, operator_fp32=1, compact_drows=compact))
    assert hb.tuning()["compact_drows"] == compact
    g, P = boundary_data(case_, 1e-3)
    U, U1 = random_state(ns["mesh"], hb.ndof, seed=4)
    hb.set_state("n", U)
    hb.set_state("n-1", U1)
    hb.set_dirichlet_values(g)
    hb.set_interface_pressure(P)
    hb.assemble_residual()
    hb.assemble_jacobian()
    yield compact, hb
    hb.close()


def test_live_context_structure_copy_and_products(live_op):
    compact, hb = live_op
    info = ks.ctx_info(hb.ctx)
    get = lambda name: ks.ctx_array(hb.ctx, name)      # noqa: E731
    N2, V = info["N2"], info["V"]
    n = 6 * N2 + V
    assert hb.ndof == n
    assert info["op32_ok"] and info["kry_fp32"], info
    assert bool(info["drows_ok"]) == bool(compact), info
    # the column layout the products rely on (k_spmv_prow and drows_pairs skip the column indices of the six-column groups)
    nadj_ptr, nadj = get("nadj_ptr"), get("nadj")
    rowptr_ref, cols_ref, diag_ref = ks.expand_cols(N2, nadj_ptr, nadj, get("padj_ptr"), get("padj"), get("vrank"))
    rowptr, cols, diagpos = get("rowptr"), get("cols"), get("diagpos")
    np.testing.assert_array_equal(rowptr, rowptr_ref)
    np.testing.assert_array_equal(cols, cols_ref)
    np.testing.assert_array_equal(diagpos, diag_ref)
    np.testing.assert_array_equal(cols[diagpos], np.arange(n))
    # the FP32 copy
    A = get("A")
    assert len(A) == rowptr[-1] and np.isfinite(A).all() and np.abs(A).max() <= 1.0
    p32, ptail, tail_src, nnz_tail = ks.pad_layout(N2, rowptr)
    np.testing.assert_array_equal(get("a32_ptr"), p32)
    assert (info["a32_ptail"], info["a32_tail_src"], info["a32_tail_nnz"]) == (ptail, tail_src, nnz_tail)
    cols32, ref32, written = ks.pad_copy(N2, rowptr, cols, A, bool(compact))
    np.testing.assert_array_equal(get("a32_cols"), cols32)
    A32 = get("A32")
    assert len(A32) == ptail + nnz_tail
    np.testing.assert_array_equal(bits32(A32[written]), bits32(ref32[written]))
    # the pair form
    if compact:
        ad, bad = ks.drows_extract(N2, rowptr, A, nadj_ptr)
        assert not bad
        np.testing.assert_array_equal(get("Ad64").view(np.uint64), ad.view(np.uint64))
        np.testing.assert_array_equal(bits32(get("Ad32")), bits32(ad.astype(np.float32)))
    # the products: working = 1 runs on the FP32 copy (and the pair form), working = 0 on the FP64 matrix
    x = np.random.default_rng(6).standard_normal(n)
    ref64, S64, L = ks.csr_product(rowptr, cols, A, x)
    ref32, S32, _ = ks.csr_product(rowptr, cols, A.astype(np.float32), x)
    y = np.full(n, np.nan)
    rc, op32, dr = ks.ctx_spmv(hb.ctx, 1, x, y)
    assert rc == 0 and op32 == 1 and dr == compact, (rc, op32, dr)
    check(y, ref32, (L + 8) * EPS * S32, "working product against the FP32 copy's values")
    check(y, ref64, (L + 8) * EPS * S32 + U32 * S64, "working product against the FP64 matrix")
    y = np.full(n, np.nan)
    rc, op32, dr = ks.ctx_spmv(hb.ctx, 0, x, y)
    assert rc == 0 and op32 == 0 and dr == compact, (rc, op32, dr)
    check(y, ref64, (L + 8) * EPS * S64, "FP64 product")
