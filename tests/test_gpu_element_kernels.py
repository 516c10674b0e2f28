"""The element kernels of fsi_assembly.hip, one launch function at a time on an MI355X through libfsi_kernel_shim.so:
launch_geometry (k_geometry), launch_residual (k_residual, k_residual_gather; gathered and atomic form), launch_l2norm (k_l2norm,
k_sum_parts), launch_cell_stats (k_cell_stats, k_stats_reduce) and launch_probe (k_probe).  The Jacobian kernels are in
tests/test_gpu_element_jacobian.py.

References: the project's oracle in extended precision from the same FP64 geometry array, tables and state (kernel_shim.ElementCase),
and numpy restatements in np.longdouble.  An element vector is compared per cell and per block (d, v, p rows) under
kernel_shim.K_RESIDUAL: |got - ref| <= K_B 2^-53 max_B |ref|; a block the reference has zero must be exactly zero.  No cell and no
block is left out.  Bitwise: the gathered F against the sequential FP64 sum of the kernel's own Re in incidence order, the
48000-cell launch (three rounds of the persistent grid) against launches over its chunks of 16384 cells, min / max of the statistics
against the kernel's own cell values.  Every output starts as NaN (or a sentinel) and carries the shim's tail.

Largest error / bound observed on an MI355X (the tests print every figure; -s shows them).  No block came near its bound:

    geometry (all sizes, both offsets)          inverse 0.22    |det| 0.28
    residual, gathered, 1 .. 17 cells           fluid d 0.08  v 0.10  p 0.03     solid d 0.06  v 0.03
    residual, gathered, theta = 1 (400 cells)   fluid d 0.11  v 0.11  p 0.05     solid d 0.10  v 0.11
    residual, gathered, 6000 cells              fluid d 0.12  v 0.18  p 0.07     solid d 0.13  v 0.20
    residual, gathered, 48000 cells (FP64 C oracle, K + K / 4: the oracle's own error is in the figure)
                                                fluid d 0.22  v 0.25  p 0.65     solid d 0.15  v 0.18
    residual, atomic (summed bounds)            0.11
    L2 norm 0.009     cell statistics: mean |v| 0.052, mean det 0.048, their sum 0.032     probe 0.24
"""
import numpy as np
import pytest

import kernel_shim as ks

pytestmark = pytest.mark.gpu

LD = ks.LD
NAN = float("nan")
BLOCKS = ("d", "v", "p")


def same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    bad = np.flatnonzero(got.view(np.uint64).ravel() != ref.view(np.uint64).ravel())
    if len(bad):
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ in their bits, first at {bad[0]}: "
                             f"{got.ravel()[bad[0]]!r} for {ref.ravel()[bad[0]]!r}")


def within(got, ref, bound, what):
    """|got - ref| <= bound entry by entry in extended precision (NaN fails); prints and returns the largest ratio"""
    got, ref, bound = (np.asarray(a, dtype=LD).ravel() for a in (got, ref, bound))
    err = np.abs(got - ref)
    r = ks.worst_ratio(err, bound)
    print(f"RATIO {what}: {r:.3f}")
    if not r <= 1.0:
        i = int(np.flatnonzero(~(err <= bound))[0])
        raise AssertionError(f"{what}: {int((~(err <= bound)).sum())} of {len(got)} outside the bound, first at {i}: got {float(got[i])!r}, "
                             f"reference {float(ref[i])!r}, error {float(err[i]):.3e} > bound {float(bound[i]):.3e}")
    return r


def blocks_within(got, ref, kind, K, what, share=1.0):
    """every block of every cell under its bound; the ratios per kind and block are printed"""
    q = ks.block_ratios(got, ref, kind) / share
    for k, name in enumerate(("fluid", "solid")):
        print(f"RATIO {what} {name}: " + "  ".join(f"{b} {q[k, i] / K[k, i]:.3f}" if K[k, i] else f"{b} zero" for i, b in enumerate(BLOCKS)))
    bound = ks.block_bound(ref, kind, K) * share
    within(got, ref, bound, what)
    assert np.all(np.asarray(got)[bound == 0] == 0.0), f"{what}: a block the reference has zero is not zero"


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def soup(C, seed, offset=0.0):
    """C cells of the tube as cells of their own (4 C vertices), each scaled about its centroid to a size between 1e-4 and 1e-2,
    its vertices in random order (both orientations), the whole moved by `offset`"""
    rng = np.random.default_rng(seed)
    t = ks.element_cases("tube")
    x = t.coords[t.tets[rng.choice(t.C, C, replace=False)]]                        # [C][4][3]
    cen = x.mean(axis=1, keepdims=True)
    size = np.sqrt(((x - cen) ** 2).sum(axis=2)).max(axis=1)
    target = 10.0 ** rng.uniform(-4, -2, C)
    x = cen + (x - cen) * (target / size)[:, None, None]
    for c in range(C):
        x[c] = x[c][rng.permutation(4)]
    return np.ascontiguousarray(x.reshape(-1, 3) + offset), np.arange(4 * C, dtype=np.int32).reshape(C, 4)


@pytest.mark.parametrize("offset", [0.0, 1.0])
@pytest.mark.parametrize("C", [1, 255, 256, 257])
def test_geometry(C, offset):
    coords, tets = soup(C, 100 + C, offset)
    variants = [tets] if C > 1 else [tets, tets[:, [1, 0, 2, 3]].copy()]           # one cell: both orientations in turn
    signs = []
    for tt in variants:
        tt = np.ascontiguousarray(tt)
        inv, det, _ = ks.geometry_reference(coords, tt)
        bi, bd = ks.geometry_bound(coords, tt)
        g = ks.out(10 * C, np.float64, NAN)
        ks.call("shim_geometry", C, len(coords), coords, tt, g)
        got = g[:10 * C].reshape(C, 10)
        within(got[:, :9], inv.reshape(C, 9), bi.reshape(C, 9), f"geometry C={C} offset={offset} inverse")
        within(got[:, 9], np.abs(det), bd, f"geometry C={C} offset={offset} |det|")
        assert np.all(got[:, 9] > 0)
        # the inverse keeps its sign: det(Jinv) has the sign of det(J)
        assert np.array_equal(np.sign(np.linalg.det(got[:, :9].reshape(C, 3, 3))), np.sign(det.astype(np.float64)))
        assert ks.tail_untouched(g, 10 * C, NAN)
        signs += list(np.sign(det.astype(np.float64)))
    assert -1 in signs and 1 in signs


# ---- residual ------------------------------------------------------------------------------------------------------------------------
def run_residual(case, lists=None, atomic_F=None):
    """one launch_residual on the case: (Re [C][64] in Re order, F) in the gathered form (lists: (N2, V, inc_ptr, inc, pinc_ptr, pinc),
    default the case's own), F in the atomic form (atomic_F: the prefill)"""
    es, (sc, fl, so) = case.es, case.params
    head = (case.C, es.ndof, es.N2, case.geom, es.cell_rank, es.cell_prow, case.kind, case.region, sc, fl, so, case.Us, case.U1s)
    if atomic_F is not None:
        F = np.concatenate([atomic_F, np.full(ks.TAIL, NAN)])
        ks.call("shim_elem_residual", *head, 0, 0, None, None, None, None, None, F)
        assert ks.tail_untouched(F, es.ndof, NAN)
        return F[:es.ndof]
    N2, V, inc_ptr, inc, pinc_ptr, pinc = lists or (es.N2, es.V, es.inc_ptr, es.inc, es.pinc_ptr, es.pinc)
    Re, F = ks.out(64 * case.C, np.float64, NAN), ks.out(6 * N2 + V, np.float64, NAN)
    ks.call("shim_elem_residual", *head, N2, V, inc_ptr, inc, pinc_ptr, pinc, Re, F)
    assert ks.tail_untouched(Re, 64 * case.C, NAN) and ks.tail_untouched(F, 6 * N2 + V, NAN)
    return Re[:64 * case.C].reshape(-1, 64), F[:6 * N2 + V]


def gathered_by_hand(Re, N2, V, inc_ptr, inc, pinc_ptr, pinc):
    return np.concatenate([ks.sequential_gather(Re, inc_ptr, inc, 6, 0).ravel(), ks.sequential_gather(Re, pinc_ptr, pinc, 1, 60).ravel()])


NO_LISTS = (1, 0, np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))


def small_case(name):
    """the cases kernel_shim.K_RESIDUAL was measured on, and their first cells"""
    kind, n = name.split(":")
    base = {"hand": "hand3", "hand_theta1": "hand3_theta1", "theta1": "tube_theta1", "prefix": "tube"}[kind]
    case = ks.element_cases(base)
    return case if int(n) == case.C else case.prefix(int(n))


@pytest.mark.parametrize("name", ["hand:1", "hand:2", "hand:3", "prefix:15", "prefix:16", "prefix:17", "hand_theta1:3", "theta1:400", "prefix:6000"])
def test_residual_gathered(name):
    case = small_case(name)
    es = case.es
    Re, F = run_residual(case)
    blocks_within(ks.oracle_from_re(Re), case.residual_reference(), case.kind, ks.K_RESIDUAL, f"residual {name}")
    same_bits(F, gathered_by_hand(Re, es.N2, es.V, es.inc_ptr, es.inc, es.pinc_ptr, es.pinc), f"gathered F {name}")
    assert not np.isnan(F).any()                                                 # every entry is written, nodes in no cell with 0.0


def test_residual_gathered_48000_and_its_rounds():
    """48000 cells are 24000 pairs on a grid of 8192 workgroups: three trips of the grid-stride loop with sS, sU and sJ reused.  Re must be
    bit for bit what launches over chunks of at most 16384 cells (one trip each) give on the same arrays; and every block is within
    the bound of the FP64 C oracle, which has a quarter of it for itself (test_kernel_references.py): K + K / 4."""
    case = ks.element_cases("big")
    es = case.es
    assert case.C > 2 * 16384
    Re, F = run_residual(case)
    same_bits(F, gathered_by_hand(Re, es.N2, es.V, es.inc_ptr, es.inc, es.pinc_ptr, es.pinc), "gathered F 48000")
    import copy
    for c0 in range(0, case.C, 16384):
        c1 = min(case.C, c0 + 16384)
        part = copy.copy(case)
        part.C, part.geom, part.kind, part.region = c1 - c0, case.geom[c0:c1], case.kind[c0:c1], case.region[c0:c1]
        part.es = copy.copy(es)
        part.es.cell_rank, part.es.cell_prow = es.cell_rank[c0:c1], es.cell_prow[c0:c1]
        Rc, _ = run_residual(part, lists=NO_LISTS)
        same_bits(Rc, Re[c0:c1], f"Re of cells {c0}..{c1} alone")
    ref = case.residual_reference(case.oracle(impl="c"))
    blocks_within(ks.oracle_from_re(Re), ref, case.kind, ks.K_RESIDUAL, "residual 48000 (C oracle)", share=1.25)


# 6 N2 + V = 252, 258, 255, 256, 257, 768 and 1877: below, above and on multiples of the gather's 256 threads
@pytest.mark.parametrize("N2,V", [(42, 0), (43, 0), (42, 3), (42, 4), (42, 5), (128, 0), (300, 77)])
def test_residual_gather_alone(N2, V):
    """k_residual_gather on incidence lists that are not the mesh's: nodes with 0, 1, 7, 8, 9, 16, 17 and 30 incidences (the loop takes
    eight per trip), V = 0, and 6 N2 + V on both sides of a multiple of 256, over the element vectors of 40 cells (launch_residual
    always runs k_residual first, so Re is what that kernel leaves for a random state)"""
    case = ks.element_cases("tube").prefix(40)
    rng = np.random.default_rng(1000 * N2 + V)
    shapes = [0, 1, 7, 8, 9, 16, 17, 30]

    def lists(n, nloc):
        deg = np.array([shapes[i % 8] for i in range(n)], dtype=np.int64)[rng.permutation(n)] if n else np.zeros(0, dtype=np.int64)
        ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        cells = [np.sort(rng.integers(0, case.C, int(d))) for d in deg]              # ascending; a cell may come twice
        ent = np.concatenate(cells + [np.zeros(0, dtype=np.int64)])
        return ptr, (16 * ent + rng.integers(0, nloc, len(ent))).astype(np.int32)
    inc_ptr, inc = lists(N2, 10)
    pinc_ptr, pinc = lists(V, 4)
    Re, F = run_residual(case, lists=(N2, V, inc_ptr, inc, pinc_ptr, pinc))
    assert not np.isnan(Re).any()
    same_bits(F, gathered_by_hand(Re, N2, V, inc_ptr, inc, pinc_ptr, pinc), f"synthetic gather N2={N2} V={V}")


@pytest.mark.parametrize("name", ["hand:3", "prefix:17", "theta1:400", "prefix:6000"])
def test_residual_atomic(name):
    """F += the element vectors with atomics: F - prefill against the sum of the reference's element vectors under the summed block
    bounds.  The prefill is random and of the size of the entry's own sum, so that its rounding does not hide the small rows:
    n additions to it cost (n + 1) u (|prefill| + sum |terms|).  Dofs of nodes in no cell keep their prefill bit for bit."""
    case = small_case(name)
    es = case.es
    ref = case.residual_reference()
    total, size = ks.assembled(es, ref), ks.assembled(es, ref, absolute=True)
    n = np.bincount(es.cell_dofs.ravel(), minlength=es.ndof)
    rng = np.random.default_rng(7)
    pre = rng.uniform(0.5, 1.0, es.ndof) * rng.choice([-1.0, 1.0], es.ndof) * np.where(size > 0, size, 1.0).astype(np.float64)
    F = run_residual(case, atomic_F=pre.copy())
    same_bits(F[n == 0], pre[n == 0], f"atomic {name}: dofs in no cell")
    bound = ks.assembled(es, ks.block_bound(ref, case.kind, ks.K_RESIDUAL)) + (n + 1) * ks.U64 * (np.abs(pre) + size)
    t = n > 0
    within(F.astype(LD)[t] - pre.astype(LD)[t], total[t], bound[t], f"residual atomic {name}")
    same_bits(F[t & (size == 0)], pre[t & (size == 0)], f"atomic {name}: rows the reference has zero")


# ---- L2 norm, cell statistics, probe ----------------------------------------------------------------------------------------------------
def sized(C):
    return ks.element_cases("big") if C == 48000 else small_case(f"prefix:{C}")


@pytest.mark.parametrize("C", [1, 3, 4, 5, 6000, 48000])
def test_l2norm(C):
    case = sized(C)
    out = ks.out(1, np.float64, NAN)
    ks.call("shim_l2norm", case.C, case.es.ndof, case.geom, case.es.cell_dofs, case.Us, out)
    val, bound = ks.l2_reference(case, case.Us)
    within(out[:1], [val], [bound], f"l2norm C={C}")
    assert ks.tail_untouched(out, 1, NAN)


def inverted_state(case, cell):
    """the case's state with the displacement of one cell's ten nodes set to x -> diag(-2.5, 0, 0) x: det(I + grad d) = -1.5 there"""
    X = case.U.copy()
    nodes = case.tet_nodes[cell]
    d = np.zeros((len(nodes), 3))
    d[:, 0] = -2.5 * (case.node_coords[nodes, 0] - case.node_coords[nodes[0], 0])
    X[:3 * case.N2].reshape(-1, 3)[nodes] = d
    return case.to_solver(X)


def check_stats(C, geom, cell_rank, cell_prow, es, X, ref, what, expect_negative=False):
    parts = ks.load().shim_stat_parts()
    n = 2 * C + 8 + 4 * parts
    cv = ks.out(n, np.float64, NAN)
    ks.call("shim_cell_stats", C, es.ndof, es.N2, geom, cell_rank, cell_prow, X, cv)
    sv, bv, sj, bj = ref
    within(cv[:C], sv, bv, f"{what} mean |v|")
    within(cv[C:2 * C], sj, bj, f"{what} mean det")
    got = cv[2 * C:2 * C + 4]
    nparts = min(parts, max(1, (C + 1023) // 1024))
    terms = -(-C // (1024 * nparts)) + 10 + -(-nparts // 1024) + 10
    within(got[:1], [cv[:C].astype(LD).sum()], [(terms + 8) * ks.U64 * np.abs(cv[:C]).astype(LD).sum()], f"{what} sum")
    same_bits(got[1:], [cv[:C].min(), cv[:C].max(), cv[C:2 * C].min()], f"{what} min / max of the kernel's own cell values")
    assert ks.tail_untouched(cv, n, NAN)
    assert (got[3] < 0) == expect_negative


@pytest.mark.parametrize("C", [1, 3, 4, 5, 6000, 48000])
def test_cell_stats(C):
    case = sized(C)
    inverted = C == 6000
    X = inverted_state(case, 1234) if inverted else case.Us
    check_stats(case.C, case.geom, case.es.cell_rank, case.es.cell_prow, case.es, X, ks.cell_stats_reference(case, X), f"cell stats C={C}",
                expect_negative=inverted)


def test_cell_stats_past_the_first_stage_of_the_reduction():
    """the 48000 cells six times over, 288000: k_cell_stats strides (above 32768 cells) and stage 1 of k_stats_reduce does (above 262144)"""
    case = ks.element_cases("big")
    rep = 6
    assert rep * case.C > 262144
    ref = tuple(np.tile(a, rep) for a in ks.cell_stats_reference(case, case.Us))
    check_stats(rep * case.C, np.tile(case.geom, (rep, 1)), np.tile(case.es.cell_rank, (rep, 1)), np.tile(case.es.cell_prow, (rep, 1)),
                case.es, case.Us, ref, "cell stats 288000")


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_probe(n):
    """points at a vertex, on an edge, inside and slightly outside their cell, in turn"""
    case = ks.element_cases("tube")
    rng = np.random.default_rng(n)
    cells = rng.integers(0, case.C, n).astype(np.int32)
    bary = np.zeros((n, 4))
    for i in range(n):
        k = (i + n) % 4
        if k == 0:
            bary[i, rng.integers(0, 4)] = 1.0
        elif k == 1:
            a, b = rng.choice(4, 2, replace=False)
            bary[i, a] = rng.uniform(0.1, 0.9)
            bary[i, b] = 1.0 - bary[i, a]
        else:
            l = rng.uniform(0.05, 1.0, 4)
            bary[i] = l / l.sum()
            if k == 3:
                a, b = rng.choice(4, 2, replace=False)
                bary[i, b] += bary[i, a] + 1e-3
                bary[i, a] = -1e-3
    out = ks.out(7 * n, np.float64, NAN)
    ks.call("shim_probe", n, case.C, case.es.ndof, case.es.cell_dofs, cells, bary, case.Us, out)
    val, bound = ks.probe_reference(case, cells, bary, case.Us)
    within(out[:7 * n], val, bound, f"probe n={n}")
    assert ks.tail_untouched(out, 7 * n, NAN)
