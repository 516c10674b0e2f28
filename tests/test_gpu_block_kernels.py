"""The field-split, Schur-complement and pressure-step kernels of vasp_amd/csrc/fsi_block.hip, one launch at a time through the
test shim, against FP64 / extended-precision restatements (tests/kernel_shim.py, themselves tested on the CPU in
tests/test_kernel_references.py).

Kernels that only move or convert numbers are compared value for value and bit for bit; kernels that accumulate are held to bounds
counted from their roundings, with L the number of terms of an entry, the reference sums in extended precision and eps = 2^-52:

    Avv~, Apv~ on solid columns                      2 eps (|e_v| + |k theta e_d|)
    k_schur_full                                     (L + 4) eps sum |terms|
    k_spmv_db, k_db_rows_sub, k_residual_csr / _rows, k_pres_rows
                                                     (L + 3) eps (sum |terms| + |b|)
    k_pres_rhs32                                     (L + 3) eps (sum |terms| + |c|), the FP32 coefficients as given
    k_vel_correct, k_vel_correct32                   (L + 4) eps (sum |terms| |dinv| + |vs|)
    k_cheb_init / k_cheb_step                        4 eps of the sum of magnitudes, x bitwise
    k_pad_init_f32                                   x, r bitwise; d within 2 x 2^-24 |d|
    k_extract_chat                                   (2^-24 + 4 eps) |chat|

Every output starts as NaN (or a sentinel) and carries ks.TAIL sentinel entries behind its end.  Synthetic graphs hold nodes of
exactly 1, 15, 16, 17, 47, 48, 49, 63, 64, 65 and 100 neighbours with 0, 1, 7, 8, 9, 17 and 24 vertex neighbours, N2 of 1, 31, 32,
33, V = 0, and one case per capped grid that exceeds the cap (CAPS, read from the launchers)."""
import functools

import numpy as np
import pytest

import kernel_shim as ks

pytestmark = pytest.mark.gpu

EPS = ks.EPS64
U32 = 2.0 ** -24
check = ks.check
NAN = float("nan")
KTHETA = 0.37

# (deg, pdeg, is_vertex): exact neighbour / vertex-neighbour counts of single nodes (ks.shaped_graph)
SHAPES = [(1, 1, True), (15, 7, True), (16, 8, True), (17, 9, True), (47, 17, True), (48, 1, True), (49, 8, True), (63, 7, True),
          (64, 9, True), (65, 17, True), (100, 24, True), (1, 0, False), (16, 0, False), (17, 1, False), (64, 7, False),
          (65, 8, False), (100, 9, False), (30, 17, False)]
# name: (N2, V, shapes, shaped_graph knobs)
CASES = {
    "N1_V1": (1, 1, [], {}),
    "N31_V9": (31, 9, [(17, 9, True), (16, 0, False)], {}),
    "N32_V32": (32, 32, [(17, 17, True), (1, 1, True)], {}),
    "N33_V17": (33, 17, [(16, 8, True), (15, 7, False), (1, 0, False)], {}),
    "N700_V300": (700, 300, SHAPES, dict(max_deg=14)),
}
# what one launch of each capped grid covers (blocks x rows per block, from the launchers of fsi_block.hip), and the size of the
# case that passes it
CAPS = {
    "extract_blocks": (16384 * 4, 6 * 11000 + 100),     # monolithic rows
    "schur_full": (32768, 33000),                       # pressure rows, one block each
    "pres_rhs32": (32768 * 16, 524300),                 # pressure rows
    "pres_rows": (8192 * 4, 33000),
    "residual_csr": (8192 * 4, 33000),
    "vel_correct32": (65536 * 32, 2097200),             # nodes
    "vel_correct": (65536 * 32, 3 * 699100),            # rows
    "db_rows_sub": (16384 * 16, 262200),                # listed nodes
    "db_rowmask": (16384 * 16, 262200),
    "residual_rows": (16384 * 16, 262200),
    "gridn": (4096 * 256, 1048700),                     # entries of a grid-stride launch
}
SOLID = ("none", "all", "tenth", "heavy")


def values(rng, n):
    """distinct random values with a sprinkling of exact zeros of both signs"""
    v = rng.uniform(-1.0, 1.0, n)
    u = rng.random(n)
    v[u < 0.02] = 0.0
    v[u > 0.98] = -0.0
    return v


def mono_values(N2, V, g, rng):
    """(rowptr, A): values() on the monolithic pattern with every diagonal entry in 0.5 <= |a| <= 2, so that the diagonal of
    Avv~ = e_v + k theta e_d (|k theta e_d| <= 0.37) that the Schur complement divides by is never zero"""
    rowptr, _, diagpos = ks.expand_cols(N2, *g)
    A = values(rng, int(rowptr[-1]))
    d = diagpos[diagpos >= 0]
    A[d] = rng.uniform(0.5, 2.0, len(d)) * rng.choice([-1.0, 1.0], len(d))
    return rowptr, A


def solid_set(kind, N2, deg, rng):
    if kind == "none":
        return np.zeros(N2, dtype=np.int32)
    if kind == "all":
        return np.ones(N2, dtype=np.int32)
    if kind == "tenth":
        return (rng.random(N2) < 0.1).astype(np.int32)
    return (deg >= min(47, deg.max())).astype(np.int32)       # the heavy nodes


@functools.lru_cache(maxsize=None)
def graph_case(name):
    N2, V, shapes, kw = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    g, nodes = ks.shaped_graph(N2, V, rng, shapes, **kw)
    st = ks.block_structure(N2, V, g)
    rowptr, A = mono_values(N2, V, g, rng)
    return dict(N2=N2, V=V, g=g, nodes=nodes, st=st, rowptr=rowptr, A=A)


@functools.lru_cache(maxsize=None)
def blocks_case(name, solid="tenth"):
    c = graph_case(name)
    rng = np.random.default_rng(len(solid) + sum(map(ord, name)))
    sol = solid_set(solid, c["N2"], np.diff(c["g"][0]), rng)
    return dict(c, solid=sol, b=ks.extract_blocks(c["N2"], c["V"], c["g"], c["A"], sol, KTHETA))


@functools.lru_cache(maxsize=None)
def light_graph(N2, V, seed=0):
    """a cheap graph for the grid-cap cases: up to two random neighbours per node"""
    return ks.mono_graph(N2, V, np.random.default_rng(seed), reach=6, max_deg=2)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref, dtype=got.dtype)
    bad = np.flatnonzero(bits(got) != bits(ref))
    assert not len(bad), f"{what}: {len(bad)} of {len(got)} entries differ in their bits; first at {bad[0]}: {got[bad[0]]!r} against {ref[bad[0]]!r}"


def same_values(got, ref, what):
    """equal as numbers (a NaN never is): for entries where the kernel may form -0.0 + 0.0"""
    bad = np.flatnonzero(~(np.asarray(got) == np.asarray(ref)))
    assert not len(bad), f"{what}: {len(bad)} entries differ; first at {bad[0]}: {got[bad[0]]!r} against {ref[bad[0]]!r}"


def tails(fill, **arrays):
    for name, (a, n) in arrays.items():
        assert ks.tail_untouched(a, n, fill), f"{name}: the kernel wrote past its end"


FLAGS0 = np.array([0x100, 0x200, 0x400, 0x800], dtype=np.int32)      # bits no kernel here owns: they must survive


def flags_are(flags, word, bit, what):
    ref = FLAGS0.copy()
    ref[word] |= bit
    assert np.array_equal(flags, ref), f"{what}: flags {flags.tolist()} instead of {ref.tolist()}"


# ---- structure -----------------------------------------------------------------------------------------------------------------
def run_structure(N2, V, g, st):
    I64, I32 = np.int64, np.int32
    o = dict(rowptr3=ks.out(3 * N2 + 1, I64, -7), cols3=ks.out(len(st["cols3"]), I32, -7), diagpos3=ks.out(3 * N2, I64, -7),
             rowptr_vp=ks.out(3 * N2 + 1, I64, -7), cols_vp=ks.out(len(st["cols_vp"]), I32, -7),
             cols_pv=ks.out(len(st["cols_pv"]), I32, -7))
    ks.call("shim_block_structure", N2, V, *g, o["rowptr3"], o["cols3"], o["diagpos3"], o["rowptr_vp"], o["cols_vp"], st["rowptr_pv"],
            o["cols_pv"])
    for k, a in o.items():
        np.testing.assert_array_equal(a[:-ks.TAIL], st[k], err_msg=k)
        assert np.all(a[-ks.TAIL:] == -7), f"{k}: written past its end"


@pytest.mark.parametrize("name", CASES)
def test_block_structure(name):
    c = graph_case(name)
    run_structure(c["N2"], c["V"], c["g"], c["st"])


def test_block_structure_without_pressure_rows():
    g = ks.mono_graph(8, 0, np.random.default_rng(8), heavy=[3], heavy_deg=[8])
    run_structure(8, 0, g, ks.block_structure(8, 0, g))


# ---- values of the blocks --------------------------------------------------------------------------------------------------------
def run_extract(N2, V, g, st, rowptr, A, solid, b):
    names = ("Add", "Adv", "Avv", "Avp", "Apv", "App")
    o = {k: ks.out(len(b[k]), np.float64, NAN) for k in names}
    ks.call("shim_extract_blocks", N2, V, KTHETA, rowptr, A, g[0], g[1], g[2], g[4], solid, st["rowptr3"], st["rowptr_vp"],
            st["rowptr_pv"], st["rowptr_pp"], *[o[k] for k in names])
    for k in names:
        assert ks.tail_untouched(o[k], len(b[k]), NAN), f"{k}: written past its end"
    for k in ("Add", "Adv", "Avp", "App"):
        same_bits(o[k][:-ks.TAIL], b[k], k)
    for k in ("Avv", "Apv"):
        got, sol = o[k][:-ks.TAIL], b[k + "_solid"]
        # off the solid columns the kernel forms e_v + 0.0 * e_d: the value of e_v, its bits unless e_v is a zero
        same_values(got[~sol], b[k][~sol], f"{k} off the solid columns")
        nz = ~sol & (b[k] != 0.0)
        same_bits(got[nz], b[k][nz], f"{k} off the solid columns")
        check(got[sol], b[k][sol], 2 * EPS * b[k + "_mag"][sol], f"{k} on the solid columns (e_v + k theta e_d)")


# every case with a tenth of its nodes solid; the case with heavy nodes with every solid set
@pytest.mark.parametrize("name,solid", [(n, "tenth") for n in CASES] + [("N700_V300", s) for s in SOLID if s != "tenth"])
def test_extract_blocks(name, solid):
    c = blocks_case(name, solid)
    run_extract(c["N2"], c["V"], c["g"], c["st"], c["rowptr"], c["A"], c["solid"], c["b"])


def test_extract_blocks_past_the_grid_cap():
    N2, V = 11000, 100
    assert 6 * N2 + V == CAPS["extract_blocks"][1] > CAPS["extract_blocks"][0]
    g = light_graph(N2, V)
    rng = np.random.default_rng(5)
    st = ks.block_structure(N2, V, g)
    rowptr, A = mono_values(N2, V, g, rng)
    solid = (rng.random(N2) < 0.3).astype(np.int32)
    run_extract(N2, V, g, st, rowptr, A, solid, ks.extract_blocks(N2, V, g, A, solid, KTHETA))


@pytest.mark.parametrize("name", CASES)
def test_extract_db_and_its_flag(name):
    c = blocks_case(name)
    N2, g, st = c["N2"], c["g"], c["st"]
    npairs = int(g[0][-1])
    full = c["b"]["Avv"]
    ref, off = ks.db_extract(N2, g, st, full)
    diag_only = np.zeros_like(full)
    # a block matrix that IS component-diagonal (zeros of both signs elsewhere)
    keep = np.zeros(len(full), dtype=bool)
    import scipy.sparse as sp
    M = sp.csr_matrix((np.arange(len(full), dtype=np.float64), st["cols3"], st["rowptr3"]), shape=(3 * N2, 3 * N2))
    rows = np.repeat(np.arange(3 * N2), np.diff(st["rowptr3"]))
    keep[rows % 3 == st["cols3"] % 3] = True
    assert M.nnz == len(full)
    diag_only[keep] = full[keep]
    diag_only[~keep] = np.where(np.arange((~keep).sum()) % 2, -0.0, 0.0)
    for vals, chk, want in ((full, 1, off), (full, 0, False), (diag_only, 1, False)):
        db = ks.out(3 * npairs, np.float64, NAN)
        flags = FLAGS0.copy()
        ks.call("shim_extract_db", N2, g[0], st["rowptr3"], vals, db, flags, chk)
        r, _ = ks.db_extract(N2, g, st, vals)
        same_bits(db[:-ks.TAIL], r, "db")
        assert ks.tail_untouched(db, 3 * npairs, NAN)
        flags_are(flags, 1, 8 if want else 0, f"extract_db check={chk}")
    assert off or npairs == 1 or not np.any(full[~keep] != 0.0)


def chat_inputs(name, gap):
    """a component-diagonal block whose three components carry the same ratios to the diagonal, except one entry of one node whose
    second component's ratio is off by the relative amount `gap`; some rows are identity rows"""
    c = graph_case(name)
    N2, g = c["N2"], c["g"]
    rng = np.random.default_rng(17)
    nadj_ptr, nadj = g[0], g[1].astype(np.int64)
    r = np.repeat(np.arange(N2), np.diff(nadj_ptr))
    ratio = rng.uniform(0.5, 2.0, len(r)) * rng.choice([-1.0, 1.0], len(r))
    ratio[nadj == r] = 1.0
    scale = np.exp2(rng.integers(-3, 4, (N2, 3)).astype(np.float64))      # powers of two: the ratios stay exactly equal
    db = ratio[:, None] * scale[r]
    ident = rng.random((N2, 3)) < 0.15
    db[ident[r] & (nadj != r)[:, None]] = 0.0
    free = np.flatnonzero((~ident[r]).all(axis=1) & (nadj != r))
    if gap and len(free):
        db[free[0], 1] *= 1.0 + gap
    return c, np.ascontiguousarray(db.ravel()), len(free)


@pytest.mark.parametrize("name", CASES)
def test_extract_chat(name):
    for gap, fires in ((0.0, False), (1e-12, False), (1e-6, True)):
        c, db, nfree = chat_inputs(name, gap)
        N2, g = c["N2"], c["g"]
        npairs = int(g[0][-1])
        ref, rowflag_ref, spread = ks.chat_extract(N2, g, db)
        chat, rowflag, flags = ks.out(npairs, np.float32, NAN), ks.out(3 * N2, np.uint8, 77), FLAGS0.copy()
        ks.call("shim_extract_chat", N2, g[0], g[1], db, chat, rowflag, flags)
        np.testing.assert_array_equal(rowflag[:-ks.TAIL], rowflag_ref)
        assert np.all(rowflag[-ks.TAIL:] == 77) and ks.tail_untouched(chat, npairs, NAN)
        check(chat[:-ks.TAIL], ref, (U32 + 4 * EPS) * np.abs(ref), f"chat (gap {gap})")
        if nfree:
            assert (spread.max() > 1e-7) == fires, "the reference's own spread does not match the case"
        flags_are(flags, 1, 16 if (fires and nfree) else 0, f"extract_chat with ratios {gap} apart")


# ---- the component-diagonal products ------------------------------------------------------------------------------------------------
def db_inputs(N2, g, rng, zero_rows=0.5):
    npairs = int(g[0][-1])
    db = values(rng, 3 * npairs).reshape(-1, 3)
    r = np.repeat(np.arange(N2), np.diff(g[0]))
    db[(rng.random(N2) < zero_rows)[r]] = 0.0
    db[::7] = np.where(np.arange(len(db[::7]))[:, None] % 2, -0.0, db[::7])
    return np.ascontiguousarray(db.ravel()), rng.standard_normal(3 * N2)


def run_db_family(N2, g, rng):
    db, x = db_inputs(N2, g, rng)
    mask_ref = ks.rowmask(N2, g, db)
    mask = ks.out(N2, np.uint8, 9)
    ks.call("shim_db_rowmask", N2, g[0], db, mask)
    np.testing.assert_array_equal(mask[:-ks.TAIL], mask_ref, err_msg="rowmask")
    assert np.all(mask[-ks.TAIL:] == 9)
    mask_ref = np.ascontiguousarray(mask_ref)
    # mask_outside: flag bit 0 of word 0 iff a masked row lies outside the set
    inside = np.ascontiguousarray(mask_ref.astype(np.int32))
    for node_set, want in ((inside, 0), (np.ones(N2, dtype=np.int32), 0)) + (((np.zeros(N2, dtype=np.int32)), 1),) * bool(mask_ref.any()):
        flags = FLAGS0.copy()
        ks.call("shim_mask_outside", N2, mask_ref, np.ascontiguousarray(node_set), flags)
        flags_are(flags, 0, want, "mask_outside")
    if mask_ref.any():
        one_out = inside.copy()
        one_out[np.flatnonzero(mask_ref)[-1]] = 0
        flags = FLAGS0.copy()
        ks.call("shim_mask_outside", N2, mask_ref, one_out, flags)
        flags_are(flags, 0, 1, "mask_outside with one masked node outside the set")
    y_ref, S, L = ks.db_terms(N2, g, db, x)
    bound = (L + 3) * EPS * S
    # spmv_db without and with the row mask (masked rows: zeros written, nothing read)
    for m in (None, mask_ref):
        y = ks.out(3 * N2, np.float64, NAN)
        ks.call("shim_spmv_db", N2, g[0], g[1], db, x, y, m)
        check(y[:-ks.TAIL], y_ref, bound, f"spmv_db (mask {m is not None})")
        assert ks.tail_untouched(y, 3 * N2, NAN)
        if m is not None:
            same_bits(y[:-ks.TAIL].reshape(-1, 3)[m == 0], np.zeros((int((m == 0).sum()), 3)), "spmv_db: masked rows")
    # db_rows_sub: y -= db x on listed rows with a set mask; every other entry keeps its bits
    y0 = rng.standard_normal(3 * N2)
    lists = [np.arange(N2, dtype=np.int32), np.ascontiguousarray(np.flatnonzero(rng.random(N2) < 0.3).astype(np.int32))]
    for lst in lists:
        for m in (None, mask_ref):
            y = np.concatenate([y0, np.full(ks.TAIL, NAN)])
            ks.call("shim_db_rows_sub", len(lst), N2, lst, g[0], g[1], db, m, x, y)
            touched = np.zeros(N2, dtype=bool)
            touched[lst] = True
            if m is not None:
                touched &= m != 0
            t3 = np.repeat(touched, 3)
            check(y[:-ks.TAIL][t3], (y0 - y_ref)[t3], ((L + 3) * EPS * (S + np.abs(y0)))[t3], "db_rows_sub: listed rows")
            same_bits(y[:-ks.TAIL][~t3], y0[~t3], "db_rows_sub: rows outside the list or with a clear mask")
            assert ks.tail_untouched(y, 3 * N2, NAN)


@pytest.mark.parametrize("name", CASES)
def test_db_products_and_row_mask(name):
    c = graph_case(name)
    run_db_family(c["N2"], c["g"], np.random.default_rng(3))


def test_db_products_past_the_grid_caps():
    N2 = CAPS["db_rows_sub"][1]
    assert N2 > CAPS["db_rows_sub"][0] and N2 > CAPS["db_rowmask"][0]
    run_db_family(N2, light_graph(N2, 50), np.random.default_rng(4))


# ---- elementwise kernels on grid-stride launches -----------------------------------------------------------------------------------------
SIZES = [1, 31, 32, 33, 700, CAPS["gridn"][1]]


@pytest.mark.parametrize("n", SIZES)
def test_conversions_and_gathers(n):
    rng = np.random.default_rng(n)
    a = values(rng, n) * np.exp2(rng.integers(-140, 20, n).astype(np.float64))      # down into the FP32 subnormals
    a[:4] = [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -(1 + 2.0 ** -24), 3.0e-39][:min(4, n)]
    b = ks.out(n, np.float32, NAN)
    ks.call("shim_to_f32", n, a, b)
    same_bits(b[:-ks.TAIL], a.astype(np.float32), "to_f32")
    assert ks.tail_untouched(b, n, NAN)
    pos = rng.integers(0, n, n).astype(np.int64)
    dst = ks.out(n, np.float64, NAN)
    ks.call("shim_gather_vals", n, pos, a, n, dst)
    same_bits(dst[:-ks.TAIL], a[pos], "gather_vals")
    assert ks.tail_untouched(dst, n, NAN)
    # mask_ripple
    for mask in (None, (rng.random(n) < 0.5).astype(np.float64)):
        x = ks.out(n, np.float64, NAN)
        ks.call("shim_mask_ripple", n, mask, x)
        same_values(x[:-ks.TAIL], ks.ripple(n, mask), "mask_ripple")
        assert ks.tail_untouched(x, n, NAN)
    # mask_scale, cheb_init, cheb_step on a scattered diagonal
    nA = 2 * n + 3
    A = rng.uniform(0.5, 2.0, nA) * rng.choice([-1.0, 1.0], nA)
    diagpos = rng.integers(0, nA, n).astype(np.int64)
    D = A[diagpos]
    ld = np.longdouble
    for mask in (None, (rng.random(n) < 0.5).astype(np.float64)):
        m = np.ones(n) if mask is None else mask
        y0 = rng.standard_normal(n)
        y = np.concatenate([y0, np.full(ks.TAIL, NAN)])
        ks.call("shim_mask_scale", n, mask, diagpos, A, nA, y)
        ref = (m.astype(ld) * y0 / D).astype(np.float64)
        check(y[:-ks.TAIL], ref, 2 * EPS * np.abs(ref), "mask_scale")
        assert ks.tail_untouched(y, n, NAN)
        rhs, inv_theta = rng.standard_normal(n), 0.731
        x, r, d = (ks.out(n, np.float64, NAN) for _ in range(3))
        ks.call("shim_cheb_init", n, mask, rhs, diagpos, A, nA, inv_theta, x, r, d)
        same_bits(x[:-ks.TAIL], np.zeros(n), "cheb_init x")
        same_values(r[:-ks.TAIL], m * rhs, "cheb_init r")
        dref = ((m * rhs).astype(ld) * inv_theta / D).astype(np.float64)
        check(d[:-ks.TAIL], dref, 4 * EPS * np.abs(dref), "cheb_init d")
        tails(NAN, x=(x, n), r=(r, n), d=(d, n))
        t, c1, c2 = rng.standard_normal(n), 0.412, 1.377
        x0, r0, d0 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
        x, r, d = (np.concatenate([v, np.full(ks.TAIL, NAN)]) for v in (x0, r0, d0))
        ks.call("shim_cheb_step", n, mask, t, diagpos, A, nA, c1, c2, x, r, d)
        same_bits(x[:-ks.TAIL], x0 + d0, "cheb_step x")
        rref = r0.astype(ld) - m * t
        check(r[:-ks.TAIL], rref.astype(np.float64), 4 * EPS * (np.abs(r0) + np.abs(m * t)), "cheb_step r")
        dref = c1 * d0.astype(ld) + c2 * rref / D
        dmag = np.abs(c1 * d0) + np.abs(c2 / D) * (np.abs(r0) + np.abs(m * t))
        check(d[:-ks.TAIL], dref.astype(np.float64), 4 * EPS * dmag, "cheb_step d")
        tails(NAN, x=(x, n), r=(r, n), d=(d, n))


@pytest.mark.parametrize("nn", [1, 31, 32, 33, 700, CAPS["gridn"][1] // 3 + 1])
def test_field_vector_layouts(nn):
    """split / merge / merge_f32d (nn nodes and V = nn // 2 + 1 pressure rows) and the float4 pads"""
    rng = np.random.default_rng(nn)
    N2, V = nn, nn // 2 + 1
    if nn > 10000:
        assert 3 * nn > CAPS["gridn"][0]
    r = rng.standard_normal(6 * N2 + V)
    rd, rv, rp = ks.out(3 * N2, np.float64, NAN), ks.out(3 * N2, np.float64, NAN), ks.out(V, np.float64, NAN)
    ks.call("shim_split", N2, V, r, rd, rv, rp)
    nodes = r[:6 * N2].reshape(N2, 6)
    same_bits(rd[:-ks.TAIL], nodes[:, :3].ravel(), "split d")
    same_bits(rv[:-ks.TAIL], nodes[:, 3:].ravel(), "split v")
    same_bits(rp[:-ks.TAIL], r[6 * N2:], "split p")
    tails(NAN, rd=(rd, 3 * N2), rv=(rv, 3 * N2), rp=(rp, V))
    zd, zv, zp = rng.standard_normal(3 * N2), rng.standard_normal(3 * N2), rng.standard_normal(V)
    zref = np.concatenate([np.concatenate([zd.reshape(N2, 3), zv.reshape(N2, 3)], axis=1).ravel(), zp])
    z = ks.out(6 * N2 + V, np.float64, NAN)
    ks.call("shim_merge", N2, V, zd, zv, zp, z)
    same_bits(z[:-ks.TAIL], zref, "merge")
    assert ks.tail_untouched(z, 6 * N2 + V, NAN)
    xd4 = rng.standard_normal((N2, 4)).astype(np.float32)
    xd4[:, 3] = 123.0                                                  # the pad lane is not read
    zref = np.concatenate([np.concatenate([xd4[:, :3].astype(np.float64), zv.reshape(N2, 3)], axis=1).ravel(), zp])
    z = ks.out(6 * N2 + V, np.float64, NAN)
    ks.call("shim_merge_f32d", N2, V, xd4, zv, zp, z)
    same_bits(z[:-ks.TAIL], zref, "merge_f32d")
    assert ks.tail_untouched(z, 6 * N2 + V, NAN)
    # pads
    a = values(rng, 3 * nn) * np.exp2(rng.integers(-30, 30, 3 * nn).astype(np.float64))
    scale4 = rng.uniform(0.5, 2.0, (nn, 4)).astype(np.float32)
    dinv4 = rng.uniform(0.5, 2.0, (nn, 4)).astype(np.float32)
    fnan = np.float32(NAN)
    for sc in (None, scale4):
        ref = np.zeros((nn, 4), dtype=np.float32)
        ref[:, :3] = a.reshape(nn, 3).astype(np.float32) * (np.float32(1) if sc is None else sc[:, :3])
        b = ks.out(4 * nn, np.float32, fnan)
        ks.call("shim_pad_to_f32", nn, a, sc, b)
        same_bits(b[:-ks.TAIL], ref.ravel(), "pad_to_f32 (pad lane +0)")
        assert np.isnan(b[-ks.TAIL:]).all()
        x, r4, d = (ks.out(4 * nn, np.float32, fnan) for _ in range(3))
        inv_theta = np.float32(0.731)
        ks.call("shim_pad_init_f32", nn, a, sc, dinv4, inv_theta, x, r4, d)
        same_bits(x[:-ks.TAIL], np.zeros(4 * nn, dtype=np.float32), "pad_init x")
        same_bits(r4[:-ks.TAIL], ref.ravel(), "pad_init r")
        dref = ref.astype(np.float64) * np.float64(inv_theta) * dinv4
        check(d[:-ks.TAIL], dref.ravel(), 2 * U32 * np.abs(dref.ravel()), "pad_init d")
        assert np.all(d[:-ks.TAIL].reshape(nn, 4)[:, 3] == 0.0)
        for v in (x, r4, d):
            assert np.isnan(v[-ks.TAIL:]).all()
    f4 = rng.standard_normal((nn, 4)).astype(np.float32)
    b = ks.out(3 * nn, np.float64, NAN)
    ks.call("shim_unpad_from_f32", nn, f4, b)
    same_bits(b[:-ks.TAIL], f4[:, :3].astype(np.float64).ravel(), "unpad_from_f32")
    assert ks.tail_untouched(b, 3 * nn, NAN)


@pytest.mark.parametrize("nS", [1, 33, 700])
def test_solid_block_gather(nS):
    """k_sb_gather: vals[9 b + 3 c + j] = float(Avv[src_b + c stride_row(b) + j])"""
    rng = np.random.default_rng(nS)
    stride = rng.integers(3, 40, nS).astype(np.int32)
    nb = 3 * nS
    sb_row = np.sort(rng.integers(0, nS, nb)).astype(np.int32)
    nA = 5000
    Avv = values(rng, nA)
    sb_src = np.array([rng.integers(0, nA - 2 * stride[r] - 3) for r in sb_row], dtype=np.int64)
    vals = ks.out(9 * nb, np.float32, NAN)
    ks.call("shim_sb_gather", nb, nS, sb_row, sb_src, stride, Avv, nA, vals)
    ref = np.stack([Avv[sb_src + c * stride[sb_row] + j] for c in range(3) for j in range(3)], axis=1).astype(np.float32)
    same_bits(vals[:-ks.TAIL], ref.ravel(), "sb_gather")
    assert ks.tail_untouched(vals, 9 * nb, NAN)


# ---- the Schur complement ----------------------------------------------------------------------------------------------------------
def run_schur(N2, V, g, st, b, expect_over=()):
    s_rowptr, s_cols = ks.schur_pattern(V, st)
    S_ref, mag, L, over = ks.schur_full(V, st, s_rowptr, s_cols, b["Apv"], b["App"], b["Avp"], b["Avv"])
    assert list(over) == list(expect_over)
    nS = int(s_rowptr[V])
    S, flags = ks.out(nS, np.float64, NAN), FLAGS0.copy()
    ks.call("shim_schur_full", V, N2, s_rowptr, s_cols, g[4], g[0], g[1], g[2], g[3], st["rowptr_pv"], b["Apv"], st["rowptr_pp"],
            b["App"], st["rowptr_vp"], b["Avp"], st["diagpos3"], b["Avv"], S, flags)
    flags_are(flags, 1, 4 if len(over) else 0, "schur_full")
    assert ks.tail_untouched(S, nS, NAN)
    skipped = np.isnan(S_ref)
    assert np.isnan(S[:-ks.TAIL][skipped]).all(), "a row over the LDS limit was written"
    check(S[:-ks.TAIL][~skipped], S_ref[~skipped], ((L + 4) * EPS * mag)[~skipped], "schur_full")
    return np.diff(s_rowptr)


@pytest.mark.parametrize("name", CASES)
def test_schur_full(name):
    c = blocks_case(name)
    run_schur(c["N2"], c["V"], c["g"], c["st"], c["b"])


@functools.lru_cache(maxsize=None)
def limit_graph(longest):
    """every node a vertex; node 0 sees nodes 2 .. 1024 (a Schur row of exactly 1024 entries with itself), node 1 sees
    2 .. longest - 1 (a row of `longest`); all others themselves alone"""
    import scipy.sparse as sp
    N2 = longest + 4
    rows = np.concatenate([np.arange(N2), np.zeros(1023, dtype=np.int64), np.ones(longest - 1, dtype=np.int64)])
    cols = np.concatenate([np.arange(N2), np.arange(2, 1025), np.arange(2, longest + 1)])
    G = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(N2, N2))
    G.sort_indices()
    ptr, ind = G.indptr.astype(np.int64), G.indices.astype(np.int32)
    return N2, (ptr, ind, ptr.copy(), ind.copy(), np.arange(N2, dtype=np.int32))


@pytest.mark.parametrize("longest", [1024, 1025])
def test_schur_rows_at_the_lds_limit(longest):
    N2, g = limit_graph(longest)
    rng = np.random.default_rng(longest)
    st = ks.block_structure(N2, N2, g)
    rowptr, A = mono_values(N2, N2, g, rng)
    solid = np.zeros(N2, dtype=np.int32)
    lens = run_schur(N2, N2, g, st, ks.extract_blocks(N2, N2, g, A, solid, KTHETA), expect_over=[1] if longest > 1024 else [])
    assert lens[0] == 1024 and lens[1] == longest


def test_schur_full_past_the_grid_cap():
    V = CAPS["schur_full"][1]
    assert V > CAPS["schur_full"][0]
    N2 = V + 50
    g = light_graph(N2, V, 2)
    rng = np.random.default_rng(6)
    st = ks.block_structure(N2, V, g)
    rowptr, A = mono_values(N2, V, g, rng)
    solid = (rng.random(N2) < 0.2).astype(np.int32)
    run_schur(N2, V, g, st, ks.extract_blocks(N2, V, g, A, solid, KTHETA))


# ---- the pressure step ---------------------------------------------------------------------------------------------------------------
def run_pressure_rows(N2, V, g, st, Apv, App, rng, fp64=True):
    n3 = 3 * N2
    w, cvec, x = rng.standard_normal(n3), rng.standard_normal(V), rng.standard_normal(V)
    apv32 = np.ascontiguousarray(Apv.astype(np.float32))
    s, S, L = ks.csr_product(st["rowptr_pv"], st["cols_pv"], apv32.astype(np.float64), w)
    y = ks.out(V, np.float64, NAN)
    ks.call("shim_pres_rhs32", V, N2, g[4], g[0], g[1], st["rowptr_pv"], apv32, w, cvec, y)
    check(y[:-ks.TAIL], cvec - s, (L + 3) * EPS * (S + np.abs(cvec)), "pres_rhs32")
    assert ks.tail_untouched(y, V, NAN)
    if not fp64:
        return
    s2, S2, L2 = ks.csr_product(st["rowptr_pv"], st["cols_pv"], Apv, w)
    s1, S1, L1 = ks.csr_product(st["rowptr_pp"], st["cols_pp"], App, x)
    for alpha, beta, gamma in ((0.0, -1.0, 1.0), (1.0, 0.0, 0.0), (0.7, -1.3, 0.45), (1.0, -1.0, 0.0)):
        y = ks.out(V, np.float64, NAN)
        ks.call("shim_pres_rows", V, st["rowptr_pp"], st["cols_pp"], App, x, alpha, st["rowptr_pv"], st["cols_pv"], Apv, w, n3, beta,
                cvec, gamma, y)
        ref = alpha * s1 + beta * s2 + gamma * cvec
        Ln = (L1 if alpha else 0.0) + (L2 if beta else 0.0)
        check(y[:-ks.TAIL], ref, (Ln + 3) * EPS * (abs(alpha) * S1 + abs(beta) * S2 + np.abs(gamma * cvec)), f"pres_rows {alpha, beta, gamma}")
        assert ks.tail_untouched(y, V, NAN)
    # residual_csr on the pressure-velocity block: y = c - Apv w
    y = ks.out(V, np.float64, NAN)
    ks.call("shim_residual_csr", V, st["rowptr_pv"], st["cols_pv"], Apv, w, n3, cvec, y)
    check(y[:-ks.TAIL], cvec - s2, (L2 + 3) * EPS * (S2 + np.abs(cvec)), "residual_csr")
    assert ks.tail_untouched(y, V, NAN)


@pytest.mark.parametrize("name", CASES)
def test_pressure_right_hand_side(name):
    c = blocks_case(name)
    run_pressure_rows(c["N2"], c["V"], c["g"], c["st"], c["b"]["Apv"], c["b"]["App"], np.random.default_rng(11))


def pv_only(N2, V, g):
    """rowptr_pv / cols_pv / rowptr_pp / cols_pp straight from the graph for the big cases (the full restatement is tested on the
    small ones): a pressure row holds the three velocity columns of each neighbour of its node, then nothing else"""
    deg, pdeg = np.diff(g[0]), np.diff(g[2])
    vr = g[4].astype(np.int64)
    rowptr_pv = np.concatenate([[0], np.cumsum(3 * deg[vr])]).astype(np.int64)
    seg = np.repeat(g[0][vr], deg[vr]) + (np.arange(deg[vr].sum()) - np.repeat(np.cumsum(deg[vr]) - deg[vr], deg[vr]))
    cols_pv = (3 * g[1][seg].astype(np.int64)[:, None] + np.arange(3)).ravel().astype(np.int32)
    rowptr_pp = np.concatenate([[0], np.cumsum(pdeg[vr])]).astype(np.int64)
    segp = np.repeat(g[2][vr], pdeg[vr]) + (np.arange(pdeg[vr].sum()) - np.repeat(np.cumsum(pdeg[vr]) - pdeg[vr], pdeg[vr]))
    return dict(rowptr_pv=rowptr_pv, cols_pv=cols_pv, rowptr_pp=rowptr_pp, cols_pp=g[3][segp].astype(np.int32))


def test_pressure_rows_past_the_grid_caps():
    rng = np.random.default_rng(12)
    V = CAPS["pres_rows"][1]
    assert V > CAPS["pres_rows"][0] and V > CAPS["residual_csr"][0]
    N2 = V + 50
    g = light_graph(N2, V, 2)
    st = ks.block_structure(N2, V, g)
    assert all(np.array_equal(st[k], v) for k, v in pv_only(N2, V, g).items()), "the big cases' short cut is not the restatement"
    run_pressure_rows(N2, V, g, st, values(rng, len(st["cols_pv"])), values(rng, len(st["cols_pp"])), rng)
    V = CAPS["pres_rhs32"][1]
    assert V > CAPS["pres_rhs32"][0]
    g = light_graph(V, V, 3)
    st = pv_only(V, V, g)
    run_pressure_rows(V, V, g, st, values(rng, len(st["cols_pv"])), None, rng, fp64=False)


def run_vel_correct(N2, V, g, rng, fp64=True):
    """dv = vs - D^-1 A_vp dp: the FP32 node form on (padj_ptr, padj) and the FP64 CSR form on the rows' own structure"""
    padj_ptr, padj = g[2], g[3]
    pdeg = np.diff(padj_ptr)
    n3 = 3 * N2
    rowptr_vp = np.concatenate([[0], np.cumsum(np.repeat(pdeg, 3))]).astype(np.int64)
    node = np.repeat(np.arange(N2), 3 * pdeg)
    k = (np.arange(rowptr_vp[-1]) - np.repeat(rowptr_vp[:-1][::3], 3 * pdeg)) % np.maximum(np.repeat(pdeg, 3 * pdeg), 1)
    cols_vp = np.ascontiguousarray(padj[padj_ptr[node] + k].astype(np.int32))
    avp = values(rng, int(rowptr_vp[-1]))
    avp32 = np.ascontiguousarray(avp.astype(np.float32))
    dp, vs = rng.standard_normal(V), rng.standard_normal(n3)
    D = rng.uniform(0.5, 2.0, n3) * rng.choice([-1.0, 1.0], n3)
    dinv = 1.0 / D
    ld = np.longdouble
    for vsi in (vs, None):
        v0 = np.zeros(n3) if vsi is None else vsi
        s, S, L = ks.csr_product(rowptr_vp, cols_vp, avp32.astype(np.float64), dp)
        dv = ks.out(n3, np.float64, NAN)
        ks.call("shim_vel_correct32", N2, V, padj_ptr, padj, avp32, dp, dinv, vsi, dv)
        ref = (v0.astype(ld) - s.astype(ld) * dinv).astype(np.float64)
        check(dv[:-ks.TAIL], ref, (L + 4) * EPS * (S * np.abs(dinv) + np.abs(v0)), f"vel_correct32 (vs {vsi is not None})")
        assert ks.tail_untouched(dv, n3, NAN)
        if not fp64:
            continue
        s, S, L = ks.csr_product(rowptr_vp, cols_vp, avp, dp)
        diagpos = rng.permutation(n3).astype(np.int64)
        Avv = np.zeros(n3)
        Avv[diagpos] = D
        for di in (dinv, None):
            dv = ks.out(n3, np.float64, NAN)
            ks.call("shim_vel_correct", n3, rowptr_vp, cols_vp, avp, dp, V, diagpos, Avv, n3, vsi, dv, di)
            ref = (v0.astype(ld) - (s.astype(ld) * dinv if di is not None else s.astype(ld) / D)).astype(np.float64)
            check(dv[:-ks.TAIL], ref, (L + 4) * EPS * (S * np.abs(dinv) + np.abs(v0)), f"vel_correct (vs {vsi is not None}, dinv {di is not None})")
            assert ks.tail_untouched(dv, n3, NAN)


@pytest.mark.parametrize("name", CASES)
def test_velocity_correction(name):
    c = graph_case(name)
    run_vel_correct(c["N2"], c["V"], c["g"], np.random.default_rng(13))


def test_velocity_correction_past_the_grid_caps():
    """N2 past 65 536 blocks x 32 nodes for the node form; the CSR form's 3 x 699 100 rows pass the same cap"""
    rng = np.random.default_rng(14)
    for which, fp64 in (("vel_correct", True), ("vel_correct32", False)):
        N2 = CAPS[which][1] // (3 if fp64 else 1)
        assert CAPS[which][1] > CAPS[which][0]
        V = 64
        pdeg = rng.integers(0, 3, N2)
        pdeg[-5:] = [9, 0, 1, 8, 2]
        padj_ptr = np.concatenate([[0], np.cumsum(pdeg)]).astype(np.int64)
        padj = rng.integers(0, V, int(padj_ptr[-1])).astype(np.int32)
        run_vel_correct(N2, V, (None, None, padj_ptr, padj, None), rng, fp64=fp64)


def run_residual_rows(nrows, ny, rng):
    nx, nvals = 500, 3000
    rows = np.ascontiguousarray(rng.choice(ny, size=nrows, replace=False).astype(np.int32))
    L = rng.integers(0, 40, nrows)
    L[:3] = [0, 16, 17][:nrows]
    ptr = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    col = rng.integers(0, nx, int(ptr[-1])).astype(np.int32)
    src = rng.integers(0, nvals, int(ptr[-1])).astype(np.int64)
    vals, x, b = values(rng, nvals), rng.standard_normal(nx), rng.standard_normal(ny)
    y0 = rng.standard_normal(ny)
    y = np.concatenate([y0, np.full(ks.TAIL, NAN)])
    ks.call("shim_residual_rows", nrows, rows, ptr, col, src, vals, nvals, x, nx, b, y, ny)
    s, S, Lf = ks.csr_product(ptr, col, vals[src], x)
    check(y[:-ks.TAIL][rows], b[rows] - s, (Lf + 3) * EPS * (S + np.abs(b[rows])), "residual_rows")
    rest = np.ones(ny, dtype=bool)
    rest[rows] = False
    same_bits(y[:-ks.TAIL][rest], y0[rest], "residual_rows: rows outside the list")
    assert ks.tail_untouched(y, ny, NAN)


@pytest.mark.parametrize("nrows,ny", [(1, 1), (33, 100), (700, 2000), (CAPS["residual_rows"][1], CAPS["residual_rows"][1] + 10)])
def test_residual_rows(nrows, ny):
    if nrows > 10000:
        assert nrows > CAPS["residual_rows"][0]
    run_residual_rows(nrows, ny, np.random.default_rng(nrows))


# ---- nothing to do -------------------------------------------------------------------------------------------------------------------
def test_empty_launches_return_without_launching():
    """V = 0 (N8_V0 of the product tests) and empty row lists: status 0, outputs untouched"""
    N2, V = 8, 0
    g = ks.mono_graph(N2, V, np.random.default_rng(8), heavy=[3], heavy_deg=[8])
    st = ks.block_structure(N2, V, g)
    rng = np.random.default_rng(0)
    npairs = int(g[0][-1])
    w = rng.standard_normal(3 * N2)
    e64, e32 = np.zeros(0), np.zeros(0, dtype=np.float32)
    y = ks.out(V, np.float64, NAN)
    assert ks.status("shim_pres_rhs32", V, N2, g[4], g[0], g[1], st["rowptr_pv"], e32, w, e64, y) == 0 and np.isnan(y).all()
    assert ks.status("shim_pres_rows", V, st["rowptr_pp"], st["cols_pp"], e64, e64, 1.0, st["rowptr_pv"], st["cols_pv"], e64, w, 3 * N2,
                     -1.0, e64, 1.0, y) == 0 and np.isnan(y).all()
    S, flags = ks.out(0, np.float64, NAN), FLAGS0.copy()
    z64 = np.zeros(1, dtype=np.int64)
    assert ks.status("shim_schur_full", V, N2, z64, np.zeros(0, dtype=np.int32), g[4], g[0], g[1], g[2], g[3], st["rowptr_pv"], e64,
                     st["rowptr_pp"], e64, st["rowptr_vp"], e64, st["diagpos3"], rng.standard_normal(9 * npairs), S, flags) == 0
    assert np.isnan(S).all() and np.array_equal(flags, FLAGS0)
    db, x = rng.standard_normal(3 * npairs), rng.standard_normal(3 * N2)
    y = ks.out(3 * N2, np.float64, NAN)
    assert ks.status("shim_db_rows_sub", 0, N2, np.zeros(0, dtype=np.int32), g[0], g[1], db, None, x, y) == 0 and np.isnan(y).all()
    y = ks.out(5, np.float64, NAN)
    assert ks.status("shim_residual_rows", 0, np.zeros(0, dtype=np.int32), z64, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64),
                     e64, 0, x, len(x), rng.standard_normal(5), y, 5) == 0 and np.isnan(y).all()


# ---- live contexts -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["fixture", "generated"])
def live(request, stenosis_case, tmp_path_factory):
    """a context on the stenosis fixture / a generated mesh with its preconditioner refreshed once (tuning pinned), and the scipy
    restatement of its blocks"""
    from conftest import prepare_case
    from vasp_amd.capi import HipBackend
    from test_gpu_parity import boundary_data, random_state
    if request.param == "fixture":
        case = stenosis_case
    else:
        from vasp_amd.meshgen import write_mesh
        tmp = tmp_path_factory.mktemp("blockgen")
        write_mesh(tmp / "s.h5", 12000)
        case = prepare_case("offset_stenosis", tmp / "s.h5", tmp / "run", dt="0.001", T="0.002")
    ns, desc = case[0], case[1]
    hb = HipBackend(desc, tuning=dict(tiles=1, tile_nodes=256, fused_sweeps=1, scalar_dd=1, sweeps_fp32=1, sweeps_fp16=1,
                                      solid_fp32=1, solid_fused=1, schur_fp32=1, schur_tile_rows=64, pv_fp32=1))
    g, P = boundary_data(case, 1e-3)
    U, U1 = random_state(ns["mesh"], hb.ndof, seed=3)
    hb.set_state("n", U)
    hb.set_state("n-1", U1)
    hb.set_dirichlet_values(g)
    hb.set_interface_pressure(P)
    hb.assemble_residual()
    hb.assemble_jacobian()
    hb.apply_preconditioner(np.random.default_rng(0).standard_normal(hb.ndof))      # forces the preconditioner's refresh
    yield request.param, hb, ks.live_blocks(hb)
    hb.close()


def ctx_csr(hb, vals, cols, rowptr, shape):
    import scipy.sparse as sp
    A = lambda name: ks.ctx_array(hb.ctx, name)      # noqa: E731
    v = A(vals) if isinstance(vals, str) else vals
    return sp.csr_matrix((v, A(cols), A(rowptr)), shape=shape)


def within(X, ref, mag, factor, what):
    """|X - ref| <= factor |mag| entry by entry, entries stored on one side only included"""
    excess = (abs(X - ref) - factor * abs(mag)).tocsr()
    worst = excess.data.max() if excess.nnz else 0.0
    assert worst <= 0.0, f"{what}: off by {worst:.3e} beyond the bound"


def test_live_block_arrays_are_the_jacobian_blocks(live):
    _, hb, lb = live
    A = lambda name: ks.ctx_array(hb.ctx, name)      # noqa: E731
    N2, V = lb["N2"], lb["V"]
    n3 = 3 * N2
    b3 = ("cols3", "rowptr3", (n3, n3))
    Avv = ctx_csr(hb, "Mvv.vals", *b3)
    within(ctx_csr(hb, "Mdd.vals", *b3), lb["Add"], lb["Add"], 2 * EPS, "Add")
    within(ctx_csr(hb, "Adv", *b3), lb["Adv"], lb["Adv"], 2 * EPS, "Adv")
    within(Avv, lb["Avv_t"], lb["Avv_mag"], 2 * EPS, "Avv~")
    within(ctx_csr(hb, "Apv", "cols_pv", "rowptr_pv", (V, n3)), lb["Apv_t"], lb["Apv_mag"], 2 * EPS, "Apv~")
    within(ctx_csr(hb, "Avp", "cols_vp", "rowptr_vp", (n3, V)), lb["Avp"], lb["Avp"], 2 * EPS, "Avp")
    within(ctx_csr(hb, "App", "cols_pp", "rowptr_pp", (V, V)), lb["App"], lb["App"], 2 * EPS, "App")
    # the structure is the one the restatement of the synthetic cases gives on the context's own graph
    g = tuple(A(k) for k in ("nadj_ptr", "nadj", "padj_ptr", "padj", "vrank"))
    st = ks.block_structure(N2, V, g)
    for k in ("rowptr3", "cols3", "diagpos3", "rowptr_vp", "cols_vp", "rowptr_pv", "cols_pv", "rowptr_pp", "cols_pp"):
        np.testing.assert_array_equal(A(k), st[k], err_msg=k)
    # component diagonals, FP32 copies, inverse diagonal: moves and single roundings of the context's own arrays
    same_bits(A("vv_db"), ks.db_extract(N2, g, st, A("Mvv.vals"))[0], "vv_db")
    adv_db, adv_off = ks.db_extract(N2, g, st, A("Adv"))
    same_bits(A("adv_db"), adv_db, "adv_db")
    dd_db, dd_off = ks.db_extract(N2, g, st, A("Mdd.vals"))
    same_bits(A("dd_db"), dd_db, "dd_db")
    same_bits(A("Avp32"), A("Avp").astype(np.float32), "Avp32")
    same_bits(A("Apv32"), A("Apv").astype(np.float32), "Apv32")
    same_bits(A("dd_db32"), A("dd_db").astype(np.float32), "dd_db32")
    same_bits(A("vv_dinv"), 1.0 / A("Mvv.vals")[A("diagpos3")], "vv_dinv")
    mask = ks.rowmask(N2, g, adv_db)
    np.testing.assert_array_equal(A("adv_rowmask"), mask)
    has = np.add.reduceat((lb["Adv"] != 0).sum(axis=1).A1, np.arange(0, n3, 3)) > 0
    np.testing.assert_array_equal(mask != 0, has, err_msg="adv_rowmask against the rows of the restated Adv")
    solid = A("node_solid") != 0
    assert mask.any() and np.all(solid[mask != 0])
    # the flags, as the restatement decides them
    coo = lambda X: X.tocoo()      # noqa: E731
    off_comp = lambda X: bool(np.any((coo(X).row % 3 != coo(X).col % 3) & (coo(X).data != 0.0)))      # noqa: E731
    flags = ks.ctx_coarse(hb.ctx)
    assert dd_off == off_comp(lb["Add"]) and adv_off == off_comp(lb["Adv"])
    assert flags["dd_is_db"] == (not off_comp(lb["Add"])) and flags["adv_is_db"] == (not off_comp(lb["Adv"]))
    assert flags["adv_solid_only"] == float(np.all(solid[has])) and flags["pv32_ok"] == 1.0
    _, _, spread = ks.chat_extract(N2, g, dd_db)
    chat = ks.chat_extract(N2, g, dd_db)[0]
    scalar = bool(np.all(spread <= 1e-9 * (np.abs(chat) + 1e-30) + 1e-12))
    assert spread.max() < 1e-10 or spread.max() > 1e-8, "the displacement block sits on the ratio test's threshold"
    assert flags["dd_is_scalar"] == float(flags["dd_is_db"] and scalar)


def test_live_pressure_step_by_hand(live):
    """One pressure step on the context's own arrays against the scipy blocks: rp - Apv~ vs, vs - D^-1 Avp dp, rd - Adv v.  FP32
    forms: the FP64 bound plus 2^-24 sum |terms| for the rounded coefficients; FP64 fall-backs: the FP64 bound alone, plus the
    2 eps |entry| the block arrays themselves may be off (test_live_block_arrays_are_the_jacobian_blocks)."""
    _, hb, lb = live
    A = lambda name: ks.ctx_array(hb.ctx, name)      # noqa: E731
    N2, V = lb["N2"], lb["V"]
    n3 = 3 * N2
    rng = np.random.default_rng(21)
    vs, rp, dp, rd = rng.standard_normal(n3), rng.standard_normal(V), rng.standard_normal(V), rng.standard_normal(n3)
    g = tuple(A(k) for k in ("nadj_ptr", "nadj", "padj_ptr", "padj", "vrank"))

    def product(X, mag, x):
        X, mag = X.tocsr(), mag.tocsr()
        X.sort_indices()
        s, S, L = ks.csr_product(X.indptr, X.indices, X.data, x)
        return s, abs(mag) @ np.abs(x), L
    # pressure right-hand side
    s, S, L = product(lb["Apv_t"], lb["Apv_mag"], vs)
    y = ks.out(V, np.float64, NAN)
    ks.call("shim_pres_rhs32", V, N2, g[4], g[0], g[1], A("rowptr_pv"), A("Apv32"), vs, rp, y)
    check(y[:-ks.TAIL], rp - s, (L + 5) * EPS * (S + np.abs(rp)) + U32 * S, "pres_rhs32 against rp - Apv~ vs")
    y = ks.out(V, np.float64, NAN)
    ks.call("shim_pres_rows", V, A("rowptr_pp"), A("cols_pp"), A("App"), None, 0.0, A("rowptr_pv"), A("cols_pv"), A("Apv"), vs, n3, -1.0,
            rp, 1.0, y)
    check(y[:-ks.TAIL], rp - s, (L + 5) * EPS * (S + np.abs(rp)), "pres_rows against rp - Apv~ vs")
    y = ks.out(V, np.float64, NAN)
    ks.call("shim_residual_csr", V, A("rowptr_pv"), A("cols_pv"), A("Apv"), vs, n3, rp, y)
    check(y[:-ks.TAIL], rp - s, (L + 5) * EPS * (S + np.abs(rp)), "residual_csr against rp - Apv~ vs")
    # velocity correction
    D = lb["Avv_t"].diagonal()
    s, S, L = product(lb["Avp"], lb["Avp"], dp)
    ref = (vs.astype(np.longdouble) - s.astype(np.longdouble) / D).astype(np.float64)
    mag = S / np.abs(D)
    dv = ks.out(n3, np.float64, NAN)
    ks.call("shim_vel_correct32", N2, V, g[2], g[3], A("Avp32"), dp, A("vv_dinv"), vs, dv)
    check(dv[:-ks.TAIL], ref, (L + 8) * EPS * (mag + np.abs(vs)) + U32 * mag, "vel_correct32 against vs - D^-1 Avp dp")
    for dinv in (A("vv_dinv"), None):
        dv = ks.out(n3, np.float64, NAN)
        Avv = A("Mvv.vals")
        ks.call("shim_vel_correct", n3, A("rowptr_vp"), A("cols_vp"), A("Avp"), dp, V, A("diagpos3"), Avv, len(Avv), vs, dv, dinv)
        check(dv[:-ks.TAIL], ref, (L + 8) * EPS * (mag + np.abs(vs)), "vel_correct against vs - D^-1 Avp dp")
    # displacement right-hand side
    v = rng.standard_normal(n3)
    s, S, L = product(lb["Adv"], lb["Adv"], v)
    bound = (L + 5) * EPS * (S + np.abs(rd))
    solid_list = np.ascontiguousarray(np.flatnonzero(A("node_solid") != 0).astype(np.int32))
    y = np.concatenate([rd, np.full(ks.TAIL, NAN)])
    ks.call("shim_db_rows_sub", len(solid_list), N2, solid_list, g[0], g[1], A("adv_db"), A("adv_rowmask"), v, y)
    check(y[:-ks.TAIL], rd - s, bound, "db_rows_sub against rd - Adv v")
    t = ks.out(n3, np.float64, NAN)
    ks.call("shim_spmv_db", N2, g[0], g[1], A("adv_db"), v, t, A("adv_rowmask"))
    check(rd - t[:-ks.TAIL], rd - s, bound, "spmv_db + axpby against rd - Adv v")
    # the fluid rows next to the wall: y[rows] = b[rows] - (Avv~ x)[rows] restricted to their solid columns
    fs_rows, fs_ptr, fs_col, fs_src = A("fs_rows"), A("fs_ptr"), A("fs_col"), A("fs_src")
    if len(fs_rows):
        Avv = A("Mvv.vals")
        x, b = rng.standard_normal(n3), rng.standard_normal(n3)
        y = np.concatenate([b, np.full(ks.TAIL, NAN)])
        ks.call("shim_residual_rows", len(fs_rows), fs_rows, fs_ptr, fs_col, fs_src, Avv, len(Avv), x, n3, b, y, n3)
        row = np.repeat(fs_rows.astype(np.int64), np.diff(fs_ptr))
        entries = np.asarray(lb["Avv_t"][row, fs_col.astype(np.int64)]).ravel()
        ments = np.asarray(lb["Avv_mag"][row, fs_col.astype(np.int64)]).ravel()
        s, _, L = ks.csr_product(fs_ptr, fs_col, entries, x)
        S = np.add.reduceat(np.concatenate([ments * np.abs(x[fs_col]), [0.0]]), np.minimum(fs_ptr[:-1], len(ments)))
        S[np.diff(fs_ptr) == 0] = 0.0
        check(y[:-ks.TAIL][fs_rows], b[fs_rows] - s, (L + 5) * EPS * (S + np.abs(b[fs_rows])), "residual_rows on fs_*")
        solid3 = np.repeat(A("node_solid") != 0, 3)
        assert np.all(solid3[fs_col]) and not np.any(solid3[fs_rows]), "fs_*: fluid rows, solid columns"


def _reversed_order(X):
    """(X', perm) with X' x[perm] = X x summed in the reversed column order"""
    n = X.shape[1]
    Y = X[:, ::-1].tocsr()
    Y.sort_indices()
    return Y


def test_live_chebyshev_intervals(live, capsys):
    """lmax_s, lmax_f, lmax_p, lmax_d against 1.2 x the restated 40-step power iteration on the scipy blocks.  The tolerance is 16 x
    the restatement's own sensitivity (its FP64 run against a run with every row summed in the reversed order) plus 1e-12 relative.
    The refresh's self-test may widen all four intervals together by 1.6^k (k < 8): k is read from lmax_d and must be the same
    whole number for all four.  Measured on an MI355X (random state, both meshes): k = 5, every ratio context / (1.2 x restatement)
    equal to 1.6^5 = 10.48576 to 3e-15 relative; the restatement's own sensitivity between 1.2e-13 and 1.6e-12 absolute (lmax_p and
    lmax_s largest), so tolerances of 2.3e-12 .. 3.1e-11.  Against scipy's eigs on the fixture mesh the 40-step estimate 1.2 lam
    lies ABOVE the spectral radius for three blocks (lmax_d 1.18, lmax_s 1.20, lmax_p 2.97 times rho) and BELOW it for the
    component-diagonal fluid block (0.46 rho: the one exemption; the context's widened lmax_f is 4.85 rho)."""
    import scipy.sparse as sp
    which, hb, lb = live
    A = lambda name: ks.ctx_array(hb.ctx, name)      # noqa: E731
    N2, V = lb["N2"], lb["V"]
    n3 = 3 * N2
    got = ks.ctx_coarse(hb.ctx)
    cd = lb["Avv_t"].tocoo()
    keep = cd.row % 3 == cd.col % 3
    Avv_cd = sp.csr_matrix((cd.data[keep], (cd.row[keep], cd.col[keep])), shape=(n3, n3))
    dinv_v = 1.0 / lb["Avv_t"].diagonal()
    mask_f = A("mask_f")
    dinv = 1.0 / lb["Avv_t"].diagonal()
    S = (lb["App"] - lb["Apv_t"] @ sp.diags(dinv) @ lb["Avp"]).tocsr()
    snode = A("snode").astype(np.int64)
    srow = (3 * snode[:, None] + np.arange(3)).ravel()
    Ass = lb["Avv_t"][srow][:, srow].tocsr()
    nS = len(snode)
    Binv = np.linalg.inv(np.stack([Ass[3 * k:3 * k + 3, 3 * k:3 * k + 3].toarray() for k in range(nS)])) if nS else np.zeros((0, 3, 3))
    bj = lambda y: np.einsum("kij,kj->ki", Binv, y.reshape(nS, 3)).ravel()      # noqa: E731
    blocks = {
        "lmax_f": (Avv_cd, lambda y: mask_f * y * dinv_v, n3, mask_f),
        "lmax_d": (lb["Add"], lambda y: y / lb["Add"].diagonal(), n3, None),
        "lmax_p": (S, lambda y: y / S.diagonal(), V, None),
        "lmax_s": (Ass, bj, 3 * nS, None),
    }
    ref, tol = {}, {}
    for name, (X, scale, n, mask) in blocks.items():
        X = X.tocsr()
        Xr = _reversed_order(X)
        a = ks.power_lmax(lambda x: X @ x, scale, n, mask)
        b = ks.power_lmax(lambda x: Xr @ x[::-1], scale, n, mask)
        ref[name], tol[name] = 1.2 * a, 16 * 1.2 * abs(a - b) + 1e-12 * 1.2 * a
    k = int(round(np.log(got["lmax_d"] / ref["lmax_d"]) / np.log(1.6)))
    with capsys.disabled():
        for name in blocks:
            print(f"\n[intervals {which}] {name}: context {got[name]!r}, 1.2 x restatement {ref[name]!r}, ratio "
                  f"{got[name] / ref[name]:.15f}, widened 1.6^{k}, tolerance {tol[name]:.3e} "
                  f"(own sensitivity {tol[name] / 16 / 1.2:.3e})", end="")
        print()
    assert 0 <= k < 8
    for name in blocks:
        want = ref[name] * 1.6 ** k
        assert abs(got[name] - want) <= tol[name] * 1.6 ** k + 4 * EPS * want, f"{name}: {got[name]!r} against {want!r}"
    if which == "fixture":
        from scipy.sparse.linalg import LinearOperator, eigs, ArpackNoConvergence
        below = []
        for name, (X, scale, n, mask) in blocks.items():
            X = X.tocsr()
            m = np.ones(n) if mask is None else mask
            op = LinearOperator((n, n), matvec=lambda x, X=X, scale=scale, m=m: scale(X @ (m * x)), dtype=np.float64)
            try:
                rho = float(np.abs(eigs(op, k=1, which="LM", tol=1e-8, maxiter=4000, return_eigenvectors=False)).max())
            except ArpackNoConvergence:
                with capsys.disabled():
                    print(f"[intervals fixture] {name}: the eigenvalue solver did not converge, no ratio")
                continue
            with capsys.disabled():
                print(f"[intervals fixture] {name}: lmax / rho = {got[name] / rho:.6f} (restatement {ref[name] / rho:.6f})")
            if ref[name] >= rho:
                assert got[name] >= rho, f"{name} = {got[name]} lies below the spectral radius {rho}"
            else:
                below.append(name)
        assert len(below) <= 1, f"the restated estimate lies below the spectral radius for {below}"
