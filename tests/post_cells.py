"""Per-cell references of the post-processing kernels (fsi_post.hip k_wss / k_stress_strain, fsi_hemo.hip k_hemo_sample /
k_hemo_finish / k_spec_wss_sample, fsi_stress.hip k_stress_sample / k_stress_average / k_tensor_sample / k_tensor_principal), their
inputs and their bounds, for tests/test_gpu_post_cell_kernels.py (one launch through libfsi_kernel_shim.so, tests/kernel_shim.py) and
tests/test_post_cell_references.py (the builders on the CPU).

Everything is restated in np.longdouble from the FP64 geometry array, tables and state the kernel is given, and none of it repeats a
kernel's algebra: the traction is integrated with the 12-point triangle rule on the P2 gradient (as oracle.post_oracle), not read
from vertex values; the 4 x 4 and 3 x 3 systems are solved with pivoting, not with the closed inverses the kernels use.

Bounds.  Tractions and tensors: per cell and block (the 12 traction coefficients; the 36 stress, the 36 strain coefficients)
|got - ref| <= K 2^-53 max_block |ref|, K = 4 x the ratio oracle.post_oracle reaches in FP64 numpy from the same geometry array
against the extended-precision builder on exactly the tests' inputs, rounded up to a multiple of 4 that leaves the measurement a
tenth of room (the rule of kernel_shim.K_RESIDUAL: the factor 4 covers another summation order and FMA contraction).  The measured
figures stand beside the constants; tests/test_post_cell_references.py asserts that the FP64 oracle stays within K / 4.  The plain
arithmetic (sums, quotients, indices) is bounded by its operation count, derived beside each builder.  Principal values: the closed
form in np.longdouble is the reference, a first-order a-priori bound of its FP64 error the bound (principal_bound)."""
from __future__ import annotations

import numpy as np

import kernel_shim as ks
from oracle import post_oracle
from oracle.fsi_oracle import keast24, tabulate_p2, triangle12

LD = np.longdouble
U64 = ks.U64
FVERTS = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])    # local vertices of the facet opposite local vertex f, ascending
MU_WSS = 3.5e-3


# ---- tables, as fsi_assembly.hip and fsi_sessions.hip form them -----------------------------------------------------------------
def post_tables():
    """(qw [24], dN [24][10][3], L [24][4]) of the Keast-24 rule, FP64, contiguous: what upload_post_tables takes"""
    qp, qw = keast24()
    _, dN, L, _ = tabulate_p2(qp)
    return np.ascontiguousarray(qw), np.ascontiguousarray(dN), np.ascontiguousarray(L)


def triangle_tables():
    """(tw [12], tl [12][3]) of the 12-point triangle rule with tl = (1 - x - y, x, y): what hemo_upload_tables takes"""
    tp, tw = triangle12()
    return np.ascontiguousarray(tw), np.ascontiguousarray(np.stack([1.0 - tp[:, 0] - tp[:, 1], tp[:, 0], tp[:, 1]], axis=1))


def solve_pivoted(M, B):
    """X of M X = B for [n][k][k] systems and [n][k][m] right-hand sides: Gaussian elimination with partial pivoting in
    np.longdouble (np.linalg does not take that type)"""
    M, B = np.array(M, dtype=LD), np.array(B, dtype=LD)
    n, k = M.shape[0], M.shape[1]
    ar = np.arange(n)
    for j in range(k):
        p = j + np.argmax(np.abs(M[:, j:, j]), axis=1)
        for A in (M, B):
            top, piv = A[ar, j].copy(), A[ar, p].copy()
            A[ar, j], A[ar, p] = piv, top
        for r in range(j + 1, k):
            l = M[:, r, j] / M[:, j, j]
            M[:, r] -= l[:, None] * M[:, j]
            B[:, r] -= l[:, None] * B[:, j]
    X = np.empty_like(B)
    for j in reversed(range(k)):
        X[:, j] = (B[:, j] - np.einsum("nc,ncm->nm", M[:, j, j + 1:], X[:, j + 1:])) / M[:, j, j][:, None]
    return X


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def shape_quality(x):
    """6 sqrt(2) V / l_rms^3 of tetrahedra [n][4][3]: 1 for the regular tetrahedron, -> 0 for a degenerate one"""
    x = np.asarray(x, dtype=np.float64)
    e = np.stack([x[:, b] - x[:, a] for a in range(4) for b in range(a + 1, 4)], axis=1)
    vol = np.abs(np.linalg.det(np.stack([x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]], axis=1))) / 6.0
    return 6.0 * np.sqrt(2.0) * vol / np.sqrt((e ** 2).sum(axis=2).mean(axis=1)) ** 3


SHAPE_NAMES = ("regular", "regular-", "sliver", "sliver-", "needle", "needle-")


def shape_points(size=1.0e-3):
    """[6][4][3]: a regular tetrahedron, a flat sliver (four points near the corners of a square, quality about 1e-3) and a needle
    (a small triangle and a far apex, quality about 1e-3), each in both orientations (two vertices exchanged), moved off the origin"""
    e, r = 4.0e-4, 1.0e-2
    s3 = np.sqrt(3.0) / 2.0
    base = [np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]),
            np.array([[1.0, 0.0, e], [-1.0, 0.0, e], [0.0, 1.0, -e], [0.0, -1.0, -e]]),
            np.array([[r, 0.0, 0.0], [-0.5 * r, s3 * r, 0.0], [-0.5 * r, -s3 * r, 0.0], [0.0, 0.0, 1.0]])]
    out = []
    for k, b in enumerate(base):
        for flip in (False, True):
            x = b[[1, 0, 2, 3]] if flip else b
            out.append(size * (x + np.array([3.0 * len(out), 0.5, -0.25])))
    return np.array(out)


_cases = {}


def cases(name):
    """ElementCases built once per process: "hand3" (kernel_shim.hand_case(3)), "tube" (kernel_shim.element_cases("tube")), "shapes":
    the six cells of shape_points as cells of their own, solid, regions 0 1 2 2 0 1 (so a regular cell, a sliver and a needle
    each meet the Mooney-Rivlin model of region 2 or a St. Venant-Kirchhoff one)"""
    if name not in _cases:
        if name == "hand3":
            _cases[name] = ks.hand_case(3, seed=21)
        elif name == "tube":
            _cases[name] = ks.element_cases("tube")
        elif name == "shapes":
            x = shape_points()
            tets = np.arange(24).reshape(6, 4)
            _cases[name] = ks.ElementCase(x.reshape(-1, 3), tets, np.ones(6, dtype=np.int32), np.array([0, 1, 2, 2, 0, 1]), seed=22)
        else:
            raise KeyError(name)
    return _cases[name]


def cell_h(geom):
    """[C] the smallest altitude of every cell, 1 / max_k |grad lambda_k|"""
    gl = np.asarray(geom)[:, :9].reshape(-1, 3, 3)
    gl = np.concatenate([-gl.sum(axis=1, keepdims=True), gl], axis=1)
    return 1.0 / np.sqrt((gl ** 2).sum(axis=2)).max(axis=1)


def state_with(case, seed, disp=None, vel=None):
    """(U in the oracle's layout, Us in the solver's) of the case's own state with the displacement replaced by `disp` x the node's
    h (the smallest altitude among its cells) x a standard normal vector (disp 0: exact zeros), and / or the velocity by the nodal
    values vel(node_coords) [N2][3]"""
    rng = np.random.default_rng(seed)
    U = case.U.copy()
    N2 = case.N2
    if disp is not None:
        h = np.full(N2, np.inf)
        np.minimum.at(h, case.tet_nodes.ravel(), np.repeat(cell_h(case.geom), 10))
        h[~np.isfinite(h)] = 0.0
        U[:3 * N2] = (disp * h[:, None] * rng.standard_normal((N2, 3))).ravel() if disp else 0.0
    if vel is not None:
        U[3 * N2:6 * N2] = np.asarray(vel(case.node_coords), dtype=np.float64).ravel()
    return U, case.to_solver(U)


def local_fields(case, U, cells):
    """(d [n][10][3], v [n][10][3]) of the listed cells from a state in the oracle's layout"""
    loc = np.asarray(U)[case.user_dofs[np.asarray(cells, dtype=np.int64)]]
    d, v, _ = _unpack(loc)
    return d, v


def _unpack(loc):
    d = np.stack([loc[:, 0:10], loc[:, 10:20], loc[:, 20:30]], axis=2)
    v = np.stack([loc[:, 30:40], loc[:, 40:50], loc[:, 50:60]], axis=2)
    return d, v, loc[:, 60:64]


# ---- wall shear stress (k_wss; wss_dg1_cell of fsi_wss.hpp) -----------------------------------------------------------------------
def rule_defect():
    """(M3, dM3): the 12-point rule's mass matrix of the unit-area triangle and its defect against (1 + delta_ab) / 12, np.longdouble.
    The rule's points and weights are 15-digit numbers: dM3 is about 5 x 2^-53, 6.7e-15 of 1 / 12.  oracle.post_oracle integrates
    with this rule; wss_reference does not (see there)."""
    tw, tl = (a.astype(LD) for a in triangle_tables())
    M3 = np.einsum("q,qa,qb->ab", 2 * tw, tl, tl)
    return M3, M3 - (1 + np.eye(3, dtype=LD)) / 12


def midpoint_rule():
    """(w [3], lam [3][3]) the edge-midpoint rule of the reference triangle in np.longdouble: weights 1 / 6 at (1/2, 1/2, 0), (0, 1/2,
    1/2), (1/2, 0, 1/2), exact for every quadratic - and its numbers are exact in any binary format but for the rounding of 1 / 6"""
    h = LD(1) / 2
    return np.full(3, LD(1) / 6), np.array([[h, h, 0], [0, h, h], [h, 0, h]], dtype=LD)


def wss_reference(geom, v, masks, mu):
    """[n][4][3] DG1 coefficients of the projected tangential traction of n (cell, mask) pairs in np.longdouble: geom [n][10] the
    cells' rows of the FP64 geometry array, v [n][10][3] the velocity at their local nodes.  Per facet set in the mask: outward normal
    -grad lambda_f / |grad lambda_f|, area |det| |grad lambda_f| / 2, Ft = F - (F.n) n with F = -mu (grad v + grad v^T) n from the P2
    gradient at the points of a quadrature rule on the facet; mass matrix and right-hand side by the same rule; rows of the 4 x 4
    matrix that stay zero become identity rows; pivoted solve.  Mask 0 and vertices on no set facet give exact zeros.

    The rule is the edge-midpoint rule (midpoint_rule()).  The gradient of a P2 field is linear, so both integrands, lambda_a lambda_b
    and lambda_a Ft, are quadratic and the rule integrates them exactly, to the rounding of np.longdouble.  The 12-point rule of
    oracle.post_oracle would not do: its 15-digit numbers miss the facet mass matrix by 6.7e-15 (rule_defect()), which over several
    facets - where the rule weighs the facets against each other - moves the solution by up to 40 x 2^-53 of the cell's largest
    coefficient, as much as the whole bound of a kernel that integrates exactly."""
    geom, v, masks = np.asarray(geom, dtype=LD), np.asarray(v, dtype=LD), np.asarray(masks, dtype=np.int64)
    n = len(masks)
    tw, tl = midpoint_rule()
    Jinv = geom[:, :9].reshape(n, 3, 3)
    gl = np.concatenate([-Jinv.sum(axis=1, keepdims=True), Jinv], axis=1)
    M, b = np.zeros((n, 4, 4), dtype=LD), np.zeros((n, 4, 3), dtype=LD)
    for f in range(4):
        sel = np.flatnonzero(masks >> f & 1)
        if not len(sel):
            continue
        lam = np.zeros((len(tw), 4), dtype=LD)
        lam[:, FVERTS[f]] = tl
        _, dNref, _, _ = tabulate_p2(lam[:, 1:4])
        G = np.einsum("qak,ckj->cqaj", dNref.astype(LD), Jinv[sel])
        gv = np.einsum("cai,cqaj->cqij", v[sel], G)
        gn = np.sqrt((gl[sel, f] ** 2).sum(axis=1))
        nrm = -gl[sel, f] / gn[:, None]
        area = geom[sel, 9] * gn / 2
        Fv = -np.einsum("cqij,cj->cqi", LD(mu) * (gv + np.swapaxes(gv, -1, -2)), nrm)
        Ft = Fv - np.einsum("cqi,ci->cq", Fv, nrm)[:, :, None] * nrm[:, None, :]
        wq = 2 * area[:, None] * tw[None, :]
        M[sel] += np.einsum("cq,qa,qb->cab", wq, lam, lam)
        b[sel] += np.einsum("cq,qa,cqi->cai", wq, lam, Ft)
    zero = np.abs(M).sum(axis=2) == 0
    for a in range(4):
        M[zero[:, a], a, a] = 1
    return solve_pivoted(M, b)


def wss_oracle64(case, cells, masks, U, mu, rule="midpoint"):
    """the same from oracle.post_oracle.wall_shear_stress in FP64 numpy on the case's geometry array: [n][4][3], zero on the vertices
    on no set facet (every list entry is given to the oracle as a cell of its own, so a cell may be listed under several masks)"""
    cells, masks = np.asarray(cells, dtype=np.int64), np.asarray(masks, dtype=np.int64)
    n = len(cells)
    fc = np.array([i for i in range(n) for f in range(4) if masks[i] >> f & 1], dtype=np.int64)
    fl = np.array([f for i in range(n) for f in range(4) if masks[i] >> f & 1], dtype=np.int64)
    out = np.zeros((n, 4, 3))
    if len(fc):
        v_nodal = np.asarray(U)[3 * case.N2:6 * case.N2].reshape(-1, 3)
        w = post_oracle.wall_shear_stress(case.coords, case.tets[cells], case.tet_nodes[cells], v_nodal, fc, fl, mu, geom=case.geom[cells], rule=rule)
        for k in range(len(fc)):
            out[fc[k], FVERTS[fl[k]]] = w[k]
    return out


def cell_ratios(got, ref):
    """[n] |got - ref| / (2^-53 max |ref|) per leading index (0 where both are zero, inf where only the reference is)"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    n = len(ref)
    err, mx = np.abs(got - ref).reshape(n, -1).max(axis=1), np.abs(ref).reshape(n, -1).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0, err / (U64 * mx))
    return np.where(np.isnan(q), np.inf, q).astype(np.float64)


def cell_bound(ref, K):
    """K 2^-53 max |ref| over each leading index, spread over its entries"""
    ref = np.abs(np.asarray(ref, dtype=LD))
    n = len(ref)
    mx = ref.reshape(n, -1).max(axis=1)
    return np.broadcast_to((K * U64 * mx).reshape((n,) + (1,) * (ref.ndim - 1)), ref.shape)


def wss_lists(name):
    """(cells, masks) of the wall-shear tests on a case: every mask 0 .. 15 on every cell of "hand3" and "shapes"; on "tube" the first
    130 fluid cells with the masks 0 .. 15 in turn"""
    case = cases(name)
    if name == "tube":
        cells = np.flatnonzero(case.kind == 0)[:130]
        return cells.astype(np.int32), (np.arange(130) % 16).astype(np.int32)
    return np.repeat(np.arange(case.C), 16).astype(np.int32), np.tile(np.arange(16), case.C).astype(np.int32)


_wss = {}


def wss_inputs(name, field="random"):
    """dict(case, cells, masks, U, Us, ref [n][4][3] longdouble) for a case and a velocity field, built once: "random" the case's own
    state; "translation", "rotation", "shear" the closed-form fields of rigid_fields()"""
    key = (name, field)
    if key not in _wss:
        case = cases(name)
        cells, masks = wss_lists(name)
        U, Us = (case.U, case.Us) if field == "random" else state_with(case, 0, vel=rigid_fields()[field])
        _, v = local_fields(case, U, cells)
        _wss[key] = dict(case=case, cells=cells, masks=masks, U=U, Us=Us, v=v, ref=wss_reference(case.geom[cells], v, masks, MU_WSS))
    return _wss[key]


SHEAR_RATE = 40.0
OMEGA = np.array([30.0, -20.0, 50.0])
V0 = np.array([0.3, -0.2, 0.5])


def rigid_fields():
    """velocity fields whose traction is known in closed form: a translation and a rotation (sym grad v = 0: no traction) and the
    shear v = (SHEAR_RATE y, 0, 0), whose traction on a facet of normal n is the tangential part of -mu SHEAR_RATE (n_y, n_x, 0)"""
    return {"translation": lambda x: np.broadcast_to(V0, x.shape), "rotation": lambda x: np.cross(OMEGA, x),
            "shear": lambda x: np.stack([SHEAR_RATE * x[:, 1], 0 * x[:, 0], 0 * x[:, 0]], axis=1)}


def shear_traction(geom, f, mu):
    """[n][3] the constant tangential traction of the shear field on facet f of the cells, np.longdouble"""
    geom = np.asarray(geom, dtype=LD)
    Jinv = geom[:, :9].reshape(-1, 3, 3)
    gl = np.concatenate([-Jinv.sum(axis=1, keepdims=True), Jinv], axis=1)[:, f]
    nrm = -gl / np.sqrt((gl ** 2).sum(axis=1))[:, None]
    F = -LD(mu) * LD(SHEAR_RATE) * np.stack([nrm[:, 1], nrm[:, 0], 0 * nrm[:, 0]], axis=1)
    return F - (F * nrm).sum(axis=1)[:, None] * nrm


def gradient_scale(geom, v, mu):
    """[n] mu max_ij sum_a |v_a,i| max_vertices |dN_a / dx_j|: the size of the terms the velocity gradient is summed from (the scale a
    cancelled traction is judged on: a rigid motion has no traction, but the sum that says so has terms of this size)"""
    geom, v = np.asarray(geom, dtype=LD), np.abs(np.asarray(v, dtype=LD))
    Jinv = geom[:, :9].reshape(-1, 3, 3)
    lam = np.eye(4)
    _, dNref, _, _ = tabulate_p2(lam[:, 1:4])
    G = np.abs(np.einsum("qak,ckj->cqaj", dNref.astype(LD), Jinv)).max(axis=1)         # [n][10][3]
    return LD(mu) * np.einsum("cai,caj->cij", v, G).reshape(len(geom), -1).max(axis=1)


# CPU-measured ratios of oracle.post_oracle.wall_shear_stress (FP64 numpy, given geometry, rule="midpoint") against wss_reference on
# the tests' inputs (measure_wss_ratios(); the largest over the list, every mask among it), and K = 4 x that, rounded up to a multiple
# of 4 that leaves the measurement a tenth of room under K / 4 (the rule of kernel_shim.K_RESIDUAL).  Random states, per-cell block ratio:
#   hand3 7.59 -> 36     shapes 16.42 -> 76     tube 7.64 -> 36
# The oracle is measured with the exact rule because that is what K stands for, the rounding of an FP64 evaluation.  With its own
# 12-point rule the oracle sits at 38.4 / 39.6 / 47.9 on the same inputs: five sixths of that is the rule's defect (rule_defect()),
# which neither the reference nor a kernel that integrates exactly has, and which would hide a kernel error of 150 x 2^-53.
K_WSS = {"hand3": 36.0, "shapes": 76.0, "tube": 36.0}
# The closed-form fields, |oracle - reference| against 2^-53 gradient_scale (the traction of a rigid motion is zero and that of the
# shear may be - a facet whose normal is along z - so the block's own maximum is no scale; the terms of the gradient's sum are):
#   translation  hand3 0.23  shapes 0.21  tube 0.39 -> 4     rotation  0.33  0.38  0.52 -> 4     shear  0.44  0.49  0.72 -> 4
K_WSS_FIELD = {"translation": 4.0, "rotation": 4.0, "shear": 4.0}


def measure_wss_ratios():
    """{(case, field): largest ratio} of the FP64 oracle against the extended-precision builder: per-cell block ratios for "random"
    and "shear", |oracle| / (2^-53 gradient_scale) for the rigid fields"""
    out = {}
    for name in ("hand3", "shapes", "tube"):
        for field in ("random", "shear", "translation", "rotation"):
            w = wss_inputs(name, field)
            case = w["case"]
            o = wss_oracle64(case, w["cells"], w["masks"], w["U"], MU_WSS)
            if field == "random":
                out[name, field] = float(cell_ratios(o, w["ref"]).max())
            else:
                s = gradient_scale(case.geom[w["cells"]], w["v"], MU_WSS)
                out[name, field] = float((np.abs(o - w["ref"]).reshape(len(s), -1).max(axis=1) / (U64 * s)).max())
    return out


# ---- hemodynamic sums and indices (k_hemo_sample, k_hemo_finish) ------------------------------------------------------------------
def twssg_projection(D):
    """[n][3] P1 projection on a facet of |D|, D [n][3 vertices][3 components] the linear field's vertex values: the norm at the 12
    points of the triangle rule, the right-hand side int lambda_a |D| with the physical weights 2 A w_q and a pivoted 3 x 3 solve of
    the mass matrix 2 A sum_q w_q lambda_a lambda_b (the area cancels; A = 1 here)"""
    D = np.asarray(D, dtype=LD)
    tw, tl = (a.astype(LD) for a in triangle_tables())
    nq = np.sqrt((np.einsum("qk,nki->nqi", tl, D) ** 2).sum(axis=2))
    rhs = np.einsum("q,qa,nq->na", 2 * tw, tl, nq)
    M = np.broadcast_to(np.einsum("q,qa,qb->ab", 2 * tw, tl, tl), (len(D), 3, 3))
    return solve_pivoted(M, rhs[:, :, None])[:, :, 0]


def hemo_reference(acc, b, b_err, masks, fidx, dt):
    """One k_hemo_sample on the accumulators acc = dict(sum_tau [ndof][3], tau_prev [ndof][3], sum_mag [ndof], sum_twssg [ndof]) in
    np.longdouble with their bounds in acc["err"] (same keys): b [n][4][3] the tractions of the list entries (reference), b_err [n]
    the bound of their entries on the device.  Returns the new dict; dofs of no listed facet keep value and bound.

    Bounds, with u = 2^-53, e the traction's bound and everything first order:
      tau_prev   e                                    (the kernel stores its own traction)
      sum_tau    old + e + u |new sum|                (one addition)
      sum_mag    old + sqrt(3) e + 4 u |tau| + u |new sum|     (| |a| - |b| | <= |a - b|; three products, two additions and a root)
      sum_twssg  old + 5 (sqrt(3) (e + old tau_prev bound) / dt + 32 u max_vertices |D|) + u |new sum|, D = (tau - tau_prev) / dt:
                 the projection is proj_a = 6 sum_b (4 delta_ab - 1) sum_q w_q lambda_qb |D_q|, sum_q w_q lambda_qb = 1 / 6 and
                 sum_b |4 delta_ab - 1| = 5, so an error eps of |D_q| reaches proj_a as at most 5 eps; |D_q| moves by at most the
                 norm of the vertex error, sqrt(3) x the componentwise one; and of rounding it carries the subtraction and division
                 of D (2 u), 15 operations and a root to |D_q| (8 u), the weight (u), the 12-term sums (12 u) and the closing
                 4 r - rs and 6 x (4 u): 27 u of max |D|, taken as 32 u."""
    new = {k: np.array(acc[k], dtype=LD) for k in ("sum_tau", "tau_prev", "sum_mag", "sum_twssg")}
    err = {k: np.array(acc["err"][k], dtype=LD) for k in new}
    masks = np.asarray(masks, dtype=np.int64)
    r3 = np.sqrt(LD(3))
    for f in range(4):
        sel = np.flatnonzero(masks >> f & 1)
        if not len(sel):
            continue
        dofs = 3 * np.asarray(fidx, dtype=np.int64).reshape(-1, 4)[sel, f][:, None] + np.arange(3)        # [m][3]
        t = np.asarray(b, dtype=LD)[sel][:, FVERTS[f]]                                                   # [m][3][3]
        e = np.asarray(b_err, dtype=LD)[sel][:, None]
        D = (t - new["tau_prev"][dofs]) / LD(dt)
        eD = (e + err["tau_prev"][dofs].max(axis=2)) / LD(dt)
        Dmax = np.sqrt((D ** 2).sum(axis=2)).max(axis=1)[:, None]
        new["sum_twssg"][dofs] += twssg_projection(D)
        err["sum_twssg"][dofs] += 5 * (r3 * eD.max(axis=1)[:, None] + 32 * U64 * Dmax) + U64 * np.abs(new["sum_twssg"][dofs])
        new["sum_tau"][dofs] += t
        err["sum_tau"][dofs] += e[:, :, None] + U64 * np.abs(new["sum_tau"][dofs])
        mag = np.sqrt((t ** 2).sum(axis=2))
        new["sum_mag"][dofs] += mag
        err["sum_mag"][dofs] += r3 * e + 4 * U64 * mag + U64 * np.abs(new["sum_mag"][dofs])
        new["tau_prev"][dofs] = t
        err["tau_prev"][dofs] = np.broadcast_to(e[:, :, None], t.shape)
    new["err"] = err
    return new


def hemo_start(nf, prefill):
    """accumulators over 3 nf dofs: prefill (a dict of arrays, exact) or zeros, with zero bounds"""
    shapes = dict(sum_tau=(3 * nf, 3), tau_prev=(3 * nf, 3), sum_mag=(3 * nf,), sum_twssg=(3 * nf,))
    acc = {k: np.array(prefill[k], dtype=LD).reshape(s) if prefill else np.zeros(s, dtype=LD) for k, s in shapes.items()}
    acc["err"] = {k: np.zeros(s, dtype=LD) for k, s in shapes.items()}
    return acc


def hemo_finish_reference(n, sum_tau, sum_mag, sum_twssg):
    """(out [5][ndof], bound [5][ndof]) of k_hemo_finish in np.longdouble: TAWSS = sum_mag / n, m = |sum_tau / n|, OSI =
    (1 - m / TAWSS) / 2, RRT = 1 / m, ECAP = OSI / TAWSS, TWSSG = sum_twssg / n, in plain IEEE arithmetic: a vanishing denominator
    gives inf or NaN there too, and the bound of such an entry is 0 (the check is then on the value's class).

    Bounds (u = 2^-53, each figure doubled for FMA contraction and another order): TAWSS and TWSSG one division, 2 u; m three
    divisions, three products, two additions and a root, at most 5 u, hence RRT 6 u, taken as 12 u; m / TAWSS (5 + 1 + 1) u, so
    OSI = (1 - x) / 2 moves by 7 u x / 2 + u |OSI|, taken as 8 u x + 2 u |OSI| - the cancellation of a unidirectional history (x -> 1)
    sits in the first term; ECAP that over TAWSS plus 2 u, taken as (8 u x + 6 u |OSI|) / TAWSS."""
    n = LD(n)
    st, sm, sg = (np.asarray(a, dtype=LD) for a in (sum_tau, sum_mag, sum_twssg))
    with np.errstate(divide="ignore", invalid="ignore"):
        tawss = sm / n
        m = np.sqrt(((st.reshape(-1, 3) / n) ** 2).sum(axis=1))
        x = m / tawss
        osi = (1 - x) / 2
        out = np.stack([tawss, osi, 1 / m, osi / tawss, sg / n])
        bound = U64 * np.stack([2 * np.abs(tawss), 8 * x + 2 * np.abs(osi), 12 / m, (8 * x + 6 * np.abs(osi)) / tawss, 2 * np.abs(sg / n)])
    bound = np.where(np.isfinite(out) & np.isfinite(bound), bound, 0)
    return out, bound


# ---- principal values (max_eig_sym3 of fsi_stress.hpp; k_tensor_principal) ---------------------------------------------------------
def _det3(T):
    return (T[..., 0, 0] * (T[..., 1, 1] * T[..., 2, 2] - T[..., 1, 2] * T[..., 2, 1])
            - T[..., 0, 1] * (T[..., 1, 0] * T[..., 2, 2] - T[..., 1, 2] * T[..., 2, 0])
            + T[..., 0, 2] * (T[..., 1, 0] * T[..., 2, 1] - T[..., 1, 1] * T[..., 2, 0]))


def closed_form(T, dtype=LD, branches=False):
    """get_eig's largest root of the characteristic polynomial with its three perturbations (p < 1e-16, |q| < 1e-24, the
    discriminant < 1e-40), evaluated in `dtype` on tensors [..., 3, 3]; with branches also the three masks of the perturbations taken"""
    T = np.asarray(T, dtype=dtype)
    c = dtype
    I1 = T[..., 0, 0] + T[..., 1, 1] + T[..., 2, 2]
    TT = (T * T).sum(axis=(-1, -2))
    I2 = c(0.5) * (I1 * I1 - TT)
    I3 = _det3(T)
    p = I1 * I1 - 3 * I2
    bp = p < c(1e-16)
    p = np.where(bp, np.abs(p) + c(2e-16), p)
    q = c(13.5) * I3 + I1 * I1 * I1 - c(4.5) * I1 * I2
    bq = np.abs(q) < c(1e-24)
    q = np.where(bq, q + np.sign(q) * c(2e-24), q)
    nom2 = 27 * (c(0.25) * I2 * I2 * (p - I2) + I3 * (c(6.75) * I3 - q))
    bn = nom2 < c(1e-40)
    nom2 = np.where(bn, np.abs(nom2) + c(2e-40), nom2)
    phi = np.arctan2(np.sqrt(nom2), q) / 3
    lam = (np.sqrt(p) * 2 * np.cos(phi) + I1) / 3
    return (lam, bp, bq, bn) if branches else lam


def principal_reference(amp):
    """k_tensor_principal in np.longdouble on amp [n][6] = 11, 12, 22, 23, 33, 31: exactly 0 where every |a_k| < 1e-8, else the
    closed form"""
    a = np.asarray(amp, dtype=np.float64).reshape(-1, 6)
    T = tensor_of(a)
    zero = (np.abs(a) < 1e-8).all(axis=1)
    return np.where(zero, LD(0), closed_form(T))


def tensor_of(amp):
    a = np.asarray(amp).reshape(-1, 6)
    return np.stack([np.stack([a[:, 0], a[:, 1], a[:, 5]], axis=1), np.stack([a[:, 1], a[:, 2], a[:, 3]], axis=1),
                     np.stack([a[:, 5], a[:, 3], a[:, 4]], axis=1)], axis=1)


def amplitudes_of(T):
    T = np.asarray(T)
    return np.ascontiguousarray(np.stack([T[..., 0, 0], T[..., 0, 1], T[..., 1, 1], T[..., 1, 2], T[..., 2, 2], T[..., 2, 0]], axis=-1),
                                dtype=np.float64)


def true_max_eigenvalue(T):
    """the largest eigenvalue of symmetric tensors [n][3][3] in np.longdouble: LAPACK's FP64 value polished by Newton steps on the
    characteristic polynomial in extended precision (for the cases that say how far the closed form is from it)"""
    T = np.asarray(T, dtype=LD)
    lam = np.linalg.eigvalsh(T.astype(np.float64))[:, -1].astype(LD)
    I1 = T[:, 0, 0] + T[:, 1, 1] + T[:, 2, 2]
    I2 = (I1 * I1 - (T * T).sum(axis=(1, 2))) / 2
    I3 = _det3(T)
    for _ in range(3):
        f = ((lam - I1) * lam + I2) * lam - I3
        df = (3 * lam - 2 * I1) * lam + I2
        with np.errstate(divide="ignore", invalid="ignore"):
            step = np.where(df != 0, f / df, 0)
        lam = lam - np.where(np.isfinite(step), step, 0)
    return lam


def _exact_inputs(T):
    """True where every entry is a small integer multiple of one power of two (|k| <= 64): the invariants I1, |T|^2, I2, I3, p and q
    are then integers below 2^53 in that unit and exact in FP64 in any order of evaluation, FMA or not"""
    T = np.asarray(T, dtype=np.float64)
    a = np.abs(T).reshape(T.shape[:-2] + (9,))
    big = a.max(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        unit = 2.0 ** (np.floor(np.log2(np.where(big > 0, big, 1.0))) - 6)
    k = a / unit[..., None]
    return (k == np.round(k)).all(axis=-1) & (k <= 128).all(axis=-1)


def principal_bound(T, dT=0.0, u=U64):
    """First-order a-priori bound of the closed form's error in arithmetic of unit roundoff u (FP64 by default) on tensors [..., 3, 3],
    without its constant (K_PRINCIPAL multiplies it), in np.longdouble.  dT: a bound of an error the entries themselves carry
    (absolute, per entry), propagated the same way.  principal_check_bound() is what a kernel is held to.

    u = 2^-53; |x| below is the same expression on the absolute values (what the terms of a cancelling sum add up to).
      I1      3 entries: 2 u |I1| + 3 dT
      |T|^2   9 products, 8 additions: 9 u |T|^2 + 2 dT sum |T_ij|
      I2      = (I1^2 - |T|^2) / 2: |I1| dI1 + dTT / 2 + u (I1^2 + |T|^2)
      I3      six triple products: 6 u |I3| + dT (sum of the absolute 2 x 2 minors)
      p       = I1^2 - 3 I2: 2 |I1| dI1 + 3 dI2 + 2 u (I1^2 + 3 |I2|): the cancellation at the scale of |I1| and |T|_F
      q       = 13.5 I3 + I1^3 - 4.5 I1 I2: 13.5 dI3 + 3 I1^2 dI1 + 4.5 (|I2| dI1 + |I1| dI2) + 3 u (13.5 |I3| + |I1|^3 + 4.5 |I1 I2|)
      D       = 27 (I2^2 (p - I2) / 4 + I3 (6.75 I3 - q)), the cancelled discriminant: the product rule on the above + 4 u of its terms
      sqrt D  | sqrt(D + d) - sqrt(D) | <= min(d / (2 sqrt D), sqrt d): a discriminant cancelled to nothing still has a bounded root
      phi     = atan2(sqrt D, q) / 3: the point (q, sqrt D) moves by e = hypot(dq, d sqrt D) at the radius r = hypot(q, sqrt D), its
              angle by (|q| d sqrt D + sqrt D dq) / r^2 to first order while 8 e < r, by at most e / (r - e) while 2 e < r, and by
              anything (pi) beyond: there q and the discriminant are rounding noise; then / 3, + 2 u |phi|
      lambda  = (2 sqrt p cos phi + I1) / 3: (2 |cos phi| d sqrt p + 2 sqrt p min((|sin phi| + dphi) dphi, 2) + dI1) / 3
              + 2 u (2 sqrt p + |I1|): a cosine moves by at most 2 whatever became of its angle, so where p, q and the discriminant
              have all cancelled (a hydrostatic tensor of 1e6 with a deviator of 1) the bound says what is still true: the value
              lies within 4 / 3 sqrt p of I1 / 3
    with d sqrt p = min(dp / (2 sqrt p), sqrt dp) + u sqrt p.  Where the entries are small integers in one power of two
    (_exact_inputs) and dT = 0, the invariants, p and q are exact in FP64 - so are their perturbed values when the perturbation
    replaces an exact zero - and their terms drop out: what is left is the discriminant (where it holds a perturbed, inexact p or
    q), the root, atan2, cos and the closing sum.  That is what pins the branch cases: for I the bound is a few 2^-53 around
    1 + 8.16e-9."""
    T = np.asarray(T, dtype=LD)
    a = np.abs(T)
    u = LD(u)
    dT = np.asarray(dT, dtype=LD)
    ex = _exact_inputs(T) & np.all(dT == 0)
    cu = np.where(ex, LD(0), u)
    I1, I1a = T[..., 0, 0] + T[..., 1, 1] + T[..., 2, 2], a[..., 0, 0] + a[..., 1, 1] + a[..., 2, 2]
    TT = (T * T).sum(axis=(-1, -2))
    I2, I2a = (I1 * I1 - TT) / 2, (I1a * I1a + TT) / 2
    I3 = _det3(T)
    minors = 0
    for i in range(3):
        for j in range(3):
            r, s = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            minors = minors + a[..., r[0], s[0]] * a[..., r[1], s[1]] + a[..., r[0], s[1]] * a[..., r[1], s[0]]
    I3a = (a[..., 0, 0] * (a[..., 1, 1] * a[..., 2, 2] + a[..., 1, 2] * a[..., 2, 1]) + a[..., 0, 1] * (a[..., 1, 0] * a[..., 2, 2] + a[..., 1, 2] * a[..., 2, 0])
           + a[..., 0, 2] * (a[..., 1, 0] * a[..., 2, 1] + a[..., 1, 1] * a[..., 2, 0]))
    dI1 = 2 * cu * I1a + 3 * dT
    dTT = 9 * cu * TT + 2 * dT * a.sum(axis=(-1, -2))
    dI2 = np.abs(I1) * dI1 + dTT / 2 + cu * (I1 * I1 + TT)
    dI3 = 6 * cu * I3a + dT * minors
    p0 = I1 * I1 - 3 * I2
    dp = 2 * np.abs(I1) * dI1 + 3 * dI2 + 2 * cu * (I1 * I1 + 3 * np.abs(I2))
    bp = p0 < LD(1e-16)
    p = np.where(bp, np.abs(p0) + LD(2e-16), p0)
    p_inexact = ~ex | (bp & (p0 != 0))
    q0 = LD(13.5) * I3 + I1 ** 3 - LD(4.5) * I1 * I2
    dq = 13.5 * dI3 + 3 * I1 * I1 * dI1 + 4.5 * (np.abs(I2) * dI1 + np.abs(I1) * dI2) + 3 * cu * (13.5 * np.abs(I3) + np.abs(I1) ** 3 + 4.5 * np.abs(I1 * I2))
    bq = np.abs(q0) < LD(1e-24)
    q = np.where(bq, q0 + np.sign(q0) * LD(2e-24), q0)
    q_inexact = ~ex | (bq & (q0 != 0))
    # a perturbed p = 2e-16 (from an exact 0) is the same FP64 number everywhere, but its products in D round
    cn = np.where(ex & ~bp & ~bq, LD(0), u)
    dp = dp + np.where(p_inexact & bp, u * p, 0)
    A, B = I2 * I2 * (p - I2) / 4, I3 * (LD(6.75) * I3 - q)
    dA = (2 * np.abs(I2) * dI2 * np.abs(p - I2) + I2 * I2 * (dp + dI2)) / 4 + 4 * cn * I2 * I2 * (np.abs(p) + np.abs(I2)) / 4
    dB = dI3 * np.abs(LD(6.75) * I3 - q) + np.abs(I3) * (6.75 * dI3 + dq) + 4 * cn * np.abs(I3) * (6.75 * np.abs(I3) + np.abs(q))
    D0 = 27 * (A + B)
    dD = 27 * (dA + dB)
    D = np.where(D0 < LD(1e-40), np.abs(D0) + LD(2e-40), D0)
    rD = np.sqrt(D)
    drD = np.minimum(dD / (2 * rD), np.sqrt(dD)) + u * rD
    phi = np.arctan2(rD, q) / 3
    rad, e = np.hypot(rD, q), np.hypot(drD, dq)
    with np.errstate(divide="ignore", invalid="ignore"):
        dtheta = np.where(8 * e < rad, (np.abs(q) * drD + rD * dq) / (D + q * q), np.where(2 * e < rad, e / (rad - e), LD(np.pi)))
    dtheta = np.where((q == 0) & (dq == 0), 0, dtheta)            # an exact q = 0: the angle is pi / 2 whatever the root is
    dphi = dtheta / 3 + 2 * u * np.abs(phi)
    sp = np.sqrt(p)
    dsp = np.minimum(dp / (2 * sp), np.sqrt(dp)) + u * sp
    return (2 * np.abs(np.cos(phi)) * dsp + 2 * sp * np.minimum((np.abs(np.sin(phi)) + dphi) * dphi, 2) + dI1) / 3 + 2 * u * (2 * sp + np.abs(I1))


U80 = 2.0 ** -64


def principal_check_bound(T, dT=0.0):
    """what |kernel - closed_form(T) in np.longdouble| is held to: K_PRINCIPAL x the FP64 bound, plus the same bound for the
    reference's own arithmetic (2^-64: on the cancelled families the extended-precision value is uncertain too), plus the part of an
    error dT the kernel's own tensor may carry in every entry.  Away from the perturbations the closed form IS the largest eigenvalue,
    which moves by at most the norm of what moves the tensor, 3 dT (Weyl); carried through the invariants one by one, as
    principal_bound does with rounding errors, the same dT would count as if it hit p, q and the discriminant independently, a
    million times more where the mean stress dominates.  Where a perturbation fires the closed form is not an eigenvalue, and the
    propagated figure stands."""
    b0 = principal_bound(T)
    out = K_PRINCIPAL * b0 + principal_bound(T, u=U80)
    if np.any(np.asarray(dT) != 0):
        _, bp, bq, bn = closed_form(T, LD, True)
        out = out + np.where(bp | bq | bn, principal_bound(T, dT) - b0, 3 * np.asarray(dT, dtype=LD))
    return out


def _sym(rng, n, lam, jitter=0.0):
    """n symmetric tensors with the eigenvalues lam [n][3] in a random frame"""
    Q = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    T = np.einsum("nik,nk,njk->nij", Q, np.asarray(lam, dtype=np.float64), Q)
    return 0.5 * (T + np.swapaxes(T, 1, 2))


def principal_families():
    """{family: tensors [n][3][3] FP64, symmetric bit for bit} of the principal-value tests"""
    rng = np.random.default_rng(31)
    n = 64
    scale = 10.0 ** rng.uniform(-3, 5, n)
    fam = {}
    fam["separated"] = _sym(rng, n, scale[:, None] * (np.array([-1.0, 0.2, 1.3]) + 0.2 * rng.uniform(-1, 1, (n, 3))))
    fam["near_double"] = _sym(rng, n, scale[:, None] * (np.array([1.0, 1.0 + 1e-6, -0.5]) * rng.choice([-1.0, 1.0], n)[:, None]))
    fam["hydrostatic"] = 1.0e6 * np.eye(3) + _sym(rng, n, np.array([-1.0, 0.3, 0.9]) + 0.2 * rng.uniform(-1, 1, (n, 3)))
    d = np.diag
    fam["exact"] = np.array([np.eye(3), 4 * np.eye(3), -2 * np.eye(3), d([2.0, 2, 1]), d([2.0, 1, 1]), d([3.0, 2, 1]), d([-1.0, -2, -3]),
                             np.ones((3, 3)), np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, 0]]), 2.0 ** -27 * np.eye(3)])
    lo = np.nextafter(1e-8, 0.0)
    zr = [lo * np.ones((3, 3)), -lo * np.ones((3, 3)), lo * np.array([[1.0, -1, 1], [-1, 1, -1], [1, -1, 1]]), np.zeros((3, 3))]
    one = np.zeros((6, 3, 3))
    for k, (i, j) in enumerate(((0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 0))):
        one[k, i, j] = one[k, j, i] = 1e-8
    fam["zero_rule"] = np.concatenate([np.array(zr), one])
    return fam


EXACT_NAMES = ("I", "4I", "-2I", "diag(2,2,1)", "diag(2,1,1)", "diag(3,2,1)", "diag(-1,-2,-3)", "ones", "shear", "2^-27 I")
# CPU-measured |FP64 numpy kopp_max_eigenvalue - closed_form in longdouble| / principal_bound per family (measure_principal_ratios()):
#   separated 0.101   near_double 0.059   hydrostatic 0.113   exact 0.325 (I: the value's own last place)   zero_rule 0.095
#   the stress kernels' principal values (measure_stress_ratios(), against pbound): at most 0.022
# K = 4 x the largest, plus a tenth of room, rounded up to the next 0.05
K_PRINCIPAL = 1.45


def measure_principal_ratios():
    out = {}
    for name, T in principal_families().items():
        ref = closed_form(T)
        got = post_oracle.kopp_max_eigenvalue(T)
        out[name] = ks.worst_ratio(np.abs(got - ref), principal_bound(T) + principal_bound(T, u=U80))
    return out


# ---- solid stress and strain (stress_strain_cell of fsi_stress.hpp) ----------------------------------------------------------------
def stress_reference(case, cells, U, K_tensors=(0.0, 0.0)):
    """dict(stress [n][4][3][3], strain [n][4][3][3], pstress [n][4], pstrain [n][4], pbound [2][n][4]) of the listed cells in
    np.longdouble from the case's FP64 geometry array, the FP64 Keast tables and the state U (oracle layout): grad d at the 24 points,
    S from oracle.post_oracle.second_piola in np.longdouble (the exponent -2/3 too), sigma = F S F^T / J, E = (F^T F - I) / 2, both
    projected onto DG1 by a pivoted solve of the quadrature mass matrix; then the closed form on the symmetrised projected tensors at
    the points, projected the same way.  pbound: principal_bound of every point's tensor (with the tensors' own block bound, K_tensors
    = (K of the stress, K of the strain), as dT), carried through the absolute projection weights: K_PRINCIPAL x the rounding part
    plus the input part."""
    cells = np.asarray(cells, dtype=np.int64)
    n = len(cells)
    qw, dN, L = (a.astype(LD) for a in post_tables())
    geom = case.geom[cells].astype(LD)
    Jinv, det = geom[:, :9].reshape(n, 3, 3), geom[:, 9]
    d, _ = local_fields(case, U, cells)
    G = np.einsum("qak,ckj->cqaj", dN, Jinv)
    g = np.einsum("cai,cqaj->cqij", d.astype(LD), G)
    F = np.eye(3, dtype=LD) + g
    J = _det3(F)
    S = np.zeros_like(g)
    _, _, solid = case.params
    for r in np.unique(case.region[cells]):
        sel = case.region[cells] == r
        _, mu, lam, model, C10, C01, C11 = (LD(x) for x in solid[r])
        S[sel] = post_oracle.second_piola(g[sel], mu, lam, int(model), C10, C01, C11)
    sigma = (F @ S @ np.swapaxes(F, -1, -2)) / J[..., None, None]
    E = (np.swapaxes(F, -1, -2) @ F - np.eye(3, dtype=LD)) / 2
    w = det[:, None] * qw[None, :]
    M = np.einsum("cq,qa,qb->cab", w, L, L)

    def project(f):
        rhs = np.einsum("cq,qa,cq...->ca...", w, L, f)
        return solve_pivoted(M, rhs.reshape(n, 4, -1)).reshape(rhs.shape)
    W = np.abs(solve_pivoted(M, np.einsum("cq,qa->caq", w, L)))                 # [n][4][24] |weights| of the projection
    out = dict(stress=project(sigma), strain=project(E))
    pb = []
    inv_vol = (20 / (det / 6))[:, None]
    for key, K in zip(("stress", "strain"), K_tensors):
        Tq = np.einsum("qa,caij->cqij", L, out[key])
        Tq = (Tq + np.swapaxes(Tq, -1, -2)) / 2
        out["p" + key] = project(closed_form(Tq))   
        dT = cell_bound(out[key], K).reshape(n, -1)[:, :1]                       # the kernel's tensor may be this far off, per entry
        lam_q = closed_form(Tq)
        # the projection's own arithmetic in the kernel: r_b = sum_q L_qb w_q lambda_q (24 products and additions, the rounded tables: at
        # most 27 x 2^-53 of the sum of the absolute terms), then 20 / vol (r_a - 0.2 sum_b r_b), where a constant cancels to a ninth of
        # its terms (1 / 4 + 1 / 5 against 1 / 20)
        rabs = np.einsum("cq,qa,cq->ca", w, L, np.abs(lam_q))
        proj = 27 * LD(U64) * inv_vol * (rabs + rabs.sum(axis=1, keepdims=True) / 5)
        pb.append(np.einsum("caq,cq->ca", W, principal_check_bound(Tq, np.broadcast_to(dT, Tq.shape[:2]))) + proj)
    out["pbound"] = np.stack(pb)
    return out


def stress_oracle64(case, cells, U):
    """the same four fields from oracle.post_oracle.stress_strain_dg1 (FP64 numpy, eig="kopp") on the case's geometry array"""
    cells = np.asarray(cells, dtype=np.int64)
    d_nodal = np.asarray(U)[:3 * case.N2].reshape(-1, 3)
    out = dict(stress=np.zeros((len(cells), 4, 3, 3)), strain=np.zeros((len(cells), 4, 3, 3)), pstress=np.zeros((len(cells), 4)),
               pstrain=np.zeros((len(cells), 4)))
    for r in np.unique(case.region[cells]):
        sel = np.flatnonzero(case.region[cells] == r)
        o = post_oracle.stress_strain_dg1(case.coords, case.tets, case.tet_nodes, d_nodal, cells[sel], ks.ELEMENT_SOLIDS[r],
                                          model=ks.ELEMENT_MODELS[r], eig="kopp", geom=case.geom)
        for k, name in (("stress", "TrueStress"), ("strain", "GreenLagrangeStrain"), ("pstress", "MaxPrincipalStress"),
                        ("pstrain", "MaxPrincipalStrain")):
            out[k][sel] = o[name]
    return out


DISPLACEMENTS = {"zero": 0.0, "large": 0.02, "small": 1.0e-6}


def stress_lists(name):
    """the solid cells a case contributes to the stress tests: all of "hand3" and "shapes"; of "tube" 65 solid cells, every 7th,
    whose regions cycle through both models"""
    case = cases(name)
    so = np.flatnonzero(case.kind == 1)
    return (so[::7][:65] if name == "tube" else so).astype(np.int32)


_stress = {}


def stress_inputs(name, disp):
    """dict(case, cells, U, Us, ref) of a case and a displacement family of DISPLACEMENTS, built once"""
    key = (name, disp)
    if key not in _stress:
        case = cases(name)
        cells = stress_lists(name)
        U, Us = state_with(case, 40 + len(disp), disp=DISPLACEMENTS[disp])
        _stress[key] = dict(case=case, cells=cells, U=U, Us=Us,
                            ref=stress_reference(case, cells, U, (K_STRESS_BY.get(key, 0.0), K_STRAIN_BY.get(key, 0.0))))
    return _stress[key]


# CPU-measured block ratios of oracle.post_oracle.stress_strain_dg1 (FP64 numpy, given geometry) against stress_reference
# (measure_stress_ratios(); stress / strain) and K = 4 x that, rounded up as above (to two digits where it is large):
#   0.02 h   hand3 9.73 -> 44 / 6.91 -> 32      shapes 15.74 -> 72 / 8.53 -> 40      tube 41.47 -> 184 / 26.39 -> 120
#   1e-6 h   hand3 2.195e5 -> 9.7e5 / 1.078e5 -> 4.8e5    shapes 1.531e5 -> 6.8e5 / 1.514e5 -> 6.7e5    tube 1.078e6 -> 4.8e6 / 4.62e5 -> 2.1e6
#            (C = F^T F is formed next to 1 before the 1 is taken off: at |grad d| of 1e-6 six digits cancel, in the oracle and in
#            the kernel alike, and the ratio is of the order of 1 / |grad d|; per cell that is still an error of 1e-10 of the cell's
#            own strain, where a tolerance on the field's maximum sees nothing of a cell that is lightly loaded)
# The zero family has no constant: both tensors are exact zeros.
K_STRESS_BY = {("hand3", "large"): 44.0, ("shapes", "large"): 72.0, ("tube", "large"): 184.0,
               ("hand3", "small"): 9.7e5, ("shapes", "small"): 6.8e5, ("tube", "small"): 4.8e6}
K_STRAIN_BY = {("hand3", "large"): 32.0, ("shapes", "large"): 40.0, ("tube", "large"): 120.0,
               ("hand3", "small"): 4.8e5, ("shapes", "small"): 6.7e5, ("tube", "small"): 2.1e6}


def measure_stress_ratios():
    """{(case, displacement): (stress, strain, principal)}: the FP64 oracle's largest block ratios and the largest ratio of its
    principal values' error to pbound"""
    out = {}
    for name in ("hand3", "shapes", "tube"):
        for disp in ("large", "small"):
            s = stress_inputs(name, disp)
            o = stress_oracle64(s["case"], s["cells"], s["U"])
            pe = np.stack([np.abs(o["pstress"] - s["ref"]["pstress"]), np.abs(o["pstrain"] - s["ref"]["pstrain"])])
            out[name, disp] = (float(cell_ratios(o["stress"], s["ref"]["stress"]).max()),
                               float(cell_ratios(o["strain"], s["ref"]["strain"]).max()), ks.worst_ratio(pe, s["ref"]["pbound"]))
    return out
