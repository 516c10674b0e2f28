"""Vortex metrics in the current configuration ``x = X + d(X)``, host side: the 14-point rule of degree 5, the NumPy twin of
k_cell_vortex_current (``hi_pass.cell_vortex_current``, ``HostBandSession.cell_vortex_current``) against an independent
restatement in extended precision and against known answers (d = 0, a rigid rotation, a dilation, a quadratic displacement),
special values, the ordered sums over frames and the pairing with the displacement's frames, the twin's refusals, the option
``--hi-pass-vortex-configuration`` and the driver's files with a stub backend.

The per-cell bound of a numerator ``n_f`` is ``K_n 2^-53 B_c`` and that of a mean ``r_f = n_f / Jbar`` is ``K_r 2^-53 B_c / |Jbar|``,
``B_c`` being the twin's formula with the absolute value of every product in the numerators and the true ``|J_p|`` wherever a
determinant divides or weights (``bounds_current``).  The roundings on the longest path, to first order:

* a vertex gradient entry: 13 (tests/test_hi_pass_vortex.py);
* an entry of ``G_p`` or ``D_p``: a barycentric coordinate (``1 - 3 a``: 2), the product, three additions: 19; ``1 + D_p``: 20;
* an adjugate entry: a product of two entries of F and a difference: 42; ``J_p``: F times adj and two additions: 65, relative to
  ``B_J``, the determinant with the absolute value of every product.  Where ``J_p`` divides, its error counts relative to
  ``|J_p|``: with ``kappa_c = max(max_p B_J / |J_p|, sum_p om_p B_J / |Jbar|)``, the conditioning of the cell's determinants,
  ``1 / J_p`` has ``65 kappa + 1``;
* ``L_p``: ``G_p`` times adj (19 + 42 + 1) and two additions, 64, times ``1 / J_p``: ``66 + 65 kappa``;
* ``f_0``: a product of two entries and nine additions (the factor -0.5 is exact): ``142 + 130 kappa``; ``f_1``: omega is a
  difference, its square, three additions: ``138 + 130 kappa``; ``v_p``: a basis value (5), the product, ten additions: 16;
  ``f_2``: ``87 + 65 kappa``; ``f_4``: 36;
* ``om_p J_p``: ``1 + 65 kappa``; its product with ``f`` and the fourteen additions: ``K_n = 158 + 195 kappa`` for ``n_0``, the
  largest; ``Jbar``: 80, relative to ``sum_p om_p B_J``;
* the last division: ``K_r = K_n + 80 kappa + 1``.

``K_n = 160 + 195 kappa_c`` and ``K_r = 160 + 275 kappa_c`` leave the second-order terms their room.  The volume ratio is held to
``80 * 2^-53 sum_p om_p B_J``.

Largest share of the bound used against the restatement (random w, random d with ``|grad d| <= 0.3``, kappa_c up to 3.4):
0.00065 (Q), 0.00090 (enstrophy), 0.00059 (helicity), 0.0042 (speed2) of the means, 0.00064, 0.00070, 0.00062 and 0.0043 of the
numerators; 0.034 of the volume ratio."""
import argparse
import contextlib
import io
import math
import re

import numpy as np
import pytest

from conftest import ROOT
from test_hi_pass_cell_rate import EPS, LD, PHASE, _history, _parameters, _session, _vectors, _velocity
from test_hi_pass_cell_rate_current import _abs_vertex_gradients, _displacement, _displacements, _quadratic_displacement
from test_hi_pass_vortex import C as C_REFERENCE, MEAN_FILES, PHASE_FILES, TABLES, _files, _tree_of, bounds as bounds_reference
from test_session_restart import CYL, SPLIT, _restart, _run, one_modification_time  # noqa: F401  (the fixture holds h5lite's clock)
from vasp_amd import flow_metrics as fm
from vasp_amd import hi_pass as hp
from vasp_amd import vortex as vx
from vasp_amd.mesh import TET_EDGES, FsiMesh
from vasp_amd.quadrature import tabulate_tet, tet_rule_deg6

CURRENT = ["--hi-pass-vortex", "--hi-pass-vortex-configuration", "current"]


def K_n(kappa):
    return 160.0 + 195.0 * kappa


def K_r(kappa):
    return 160.0 + 275.0 * kappa


@pytest.fixture(scope="module")
def mesh():
    return FsiMesh.read(CYL)


@pytest.fixture(scope="module")
def cells(mesh):
    """Every cell of the cylinder fixture: its P2 nodes, the gradients of its barycentric coordinates, its node coordinates."""
    c = np.arange(mesh.num_cells)
    return mesh.tet_nodes[c], fm.barycentric_gradients(mesh, c), mesh.node_coords[mesh.tet_nodes[c]]


def rule_ld():
    """(lam (14, 4), om (14,)) in ``np.longdouble`` from the six named constants."""
    a1, a2, b = LD(hp.VORTEX_RULE_A1), LD(hp.VORTEX_RULE_A2), LD(hp.VORTEX_RULE_B)
    lam = []
    for a in (a1, a2):
        lam += [[LD(1) - LD(3) * a if t == q else a for t in range(4)] for q in range(4)]
    lam += [[LD(0.5) - b if t in (int(p), int(r)) else b for t in range(4)] for p, r in TET_EDGES]
    om = [LD(hp.VORTEX_RULE_W1)] * 4 + [LD(hp.VORTEX_RULE_W2)] * 4 + [LD(hp.VORTEX_RULE_W3)] * 6
    return np.array(lam, dtype=LD), np.array(om, dtype=LD)


# ---- the rule ----------------------------------------------------------------------------------------------------------------

def test_the_rule_is_exact_to_degree_5_and_not_to_degree_6():
    """The mean of ``x^a y^b z^c`` over the reference tetrahedron is ``6 a! b! c! / (a + b + c + 3)!``.  The six constants are
    decimals rounded to FP64, each off by at most 2^-53 relative: a barycentric coordinate moves by at most ``3 a 2^-53 < 2^-53``,
    a monomial of degree n <= 5 with coordinates in [0, 1] by at most ``n 2^-53``, a weight by ``2^-53`` of itself - the mean
    by at most ``6 * 2^-53``; 8 leaves the extended-precision sum its own roundings.  Largest error observed: 0.125 * 2^-53 (the sum of the weights), 0.042 * 2^-53 above degree 0."""
    lam, om = rule_ld()
    assert lam.shape == (14, 4) and abs(float(om.sum() - 1)) <= 2 * EPS and (om > 0).all() and (lam > 0).all()
    assert (np.abs(lam.sum(axis=1) - 1) <= 2 * EPS).all()
    assert (np.abs(lam - hp.VORTEX_RULE_LAM.astype(LD)) <= 2 * EPS).all() and np.array_equal(om.astype(np.float64), hp.VORTEX_RULE_OM)
    x, y, z = lam[:, 1], lam[:, 2], lam[:, 3]
    worst = {}
    for n in range(7):
        for a in range(n + 1):
            for b in range(n + 1 - a):
                c = n - a - b
                exact = LD(6 * math.factorial(a) * math.factorial(b) * math.factorial(c)) / LD(math.factorial(n + 3))
                err = abs(float((om * x ** a * y ** b * z ** c).sum() - exact))
                worst[n] = max(worst.get(n, 0.0), err)
    print("largest error of a monomial's mean, by degree, in units of 2^-53:", {n: e / EPS for n, e in worst.items()})
    assert all(worst[n] <= 8 * EPS for n in range(6))
    assert worst[6] > 1e-6
    # the table of basis values is the P2 basis of the quadrature module at the points, and a partition of unity
    N = tabulate_tet(lam[:, 1:])[0]
    assert (np.abs(N - hp.VORTEX_RULE_BASIS.astype(LD)) <= 6 * EPS).all() and (np.abs(hp.VORTEX_RULE_BASIS.sum(axis=1) - 1) <= 8 * EPS).all()


# ---- the twin against the restatement ------------------------------------------------------------------------------------------

def restated(w, d, g, lam=None, om=None):
    """(means (6, n), numerators (6, n), J (points, n)) in ``np.longdouble`` by another route: the P2 basis and its reference
    gradients at the points themselves (``tabulate_tet``), mapped by the gradients of the barycentric coordinates 1 .. 3 - no
    vertex value of a gradient is formed -, the inverse of F by cross products of its rows, tensor contractions for the sums."""
    if lam is None:
        lam, om = rule_ld()
    N, dN = tabulate_tet(np.asarray(lam)[:, 1:])[:2]
    w, d, g, om = (np.asarray(a).astype(LD) for a in (w, d, g, om))
    phys = np.einsum("qak,ckj->cqaj", dN.astype(LD), g[:, 1:4])
    G, F = np.einsum("cai,cqaj->cqij", w, phys), np.einsum("cai,cqaj->cqij", d, phys) + np.eye(3, dtype=LD)
    r0, r1, r2 = F[:, :, 0], F[:, :, 1], F[:, :, 2]
    c0, c1, c2 = np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)            # the columns of adj F
    J = np.einsum("cqi,cqi->cq", r0, c0)
    L = np.einsum("cqik,cqkj->cqij", G, np.stack([c0, c1, c2], axis=3) / J[:, :, None, None])
    v = np.einsum("qa,cai->cqi", N.astype(LD), w)
    omega = np.stack([L[..., 2, 1] - L[..., 1, 2], L[..., 0, 2] - L[..., 2, 0], L[..., 1, 0] - L[..., 0, 1]], axis=-1)
    f = [-np.einsum("cqij,cqji->cq", L, L) / LD(2), np.einsum("cqi,cqi->cq", omega, omega), np.einsum("cqi,cqi->cq", v, omega),
         None, np.einsum("cqi,cqi->cq", v, v)]
    wj = J * om
    jbar = wj.sum(axis=1)
    num = [None if a is None else (wj * a).sum(axis=1) for a in f]
    num[3] = np.abs(num[2])
    mean = [a / jbar for a in num]
    mean[3] = np.abs(mean[2])
    return np.stack(mean + [jbar]), np.stack(num + [jbar]), J.T


def bounds_current(w, d, g):
    """(B (6, n), kappa (n,), B of the volume ratio (n,)) of the module docstring: the twin's arithmetic on the absolute vertex
    gradients and nodal values with a sum in the place of every difference, and the true ``|J_p|`` where J divides or weights."""
    w, d, g = (np.asarray(a, dtype=np.float64) for a in (w, d, g))
    lam, om, basis = hp.VORTEX_RULE_LAM, hp.VORTEX_RULE_OM, hp.VORTEX_RULE_BASIS
    J_true = np.abs(restated(w, d, g)[2].astype(np.float64))
    G, D = np.array(_abs_vertex_gradients(w, g)), np.array(_abs_vertex_gradients(d, g))      # (4, 3, 3, n)
    aw = np.abs(w)
    B, BJ = np.zeros((6, len(w))), np.zeros(len(w))
    kappa = np.ones(len(w))
    with np.errstate(all="ignore"):
        for p in range(14):
            gp = np.einsum("t,tijc->ijc", lam[p], G)
            F = np.einsum("t,tijc->ijc", lam[p], D) + np.eye(3)[:, :, None]
            m = lambda a, b, c, e: F[a] * F[b] + F[c] * F[e]
            A = [[m((1, 1), (2, 2), (1, 2), (2, 1)), m((0, 2), (2, 1), (0, 1), (2, 2)), m((0, 1), (1, 2), (0, 2), (1, 1))],
                 [m((1, 2), (2, 0), (1, 0), (2, 2)), m((0, 0), (2, 2), (0, 2), (2, 0)), m((0, 2), (1, 0), (0, 0), (1, 2))],
                 [m((1, 0), (2, 1), (1, 1), (2, 0)), m((0, 1), (2, 0), (0, 0), (2, 1)), m((0, 0), (1, 1), (0, 1), (1, 0))]]
            bj = (F[0, 0] * A[0][0] + F[0, 1] * A[1][0]) + F[0, 2] * A[2][0]
            kappa = np.maximum(kappa, bj / J_true[p])
            L = [[((gp[i, 0] * A[0][j] + gp[i, 1] * A[1][j]) + gp[i, 2] * A[2][j]) / J_true[p] for j in range(3)] for i in range(3)]
            omega = [L[2][1] + L[1][2], L[0][2] + L[2][0], L[1][0] + L[0][1]]
            v = np.einsum("a,cai->ic", np.abs(basis[p]), aw)
            wj = om[p] * J_true[p]
            B[0] += wj * (0.5 * sum(L[i][j] * L[j][i] for i in range(3) for j in range(3)))
            B[1] += wj * sum(o * o for o in omega)
            B[2] += wj * sum(v[i] * omega[i] for i in range(3))
            B[4] += wj * sum(v[i] * v[i] for i in range(3))
            BJ += om[p] * bj
        B[3], B[5] = B[2], BJ
        jbar = np.abs(restated(w, d, g)[0][5].astype(np.float64))
        return B, np.maximum(kappa, BJ / jbar), BJ


def _scaled_displacement(shape, g, seed, size=0.3):
    """Random nodal d, scaled per cell so that the largest entry of its vertex gradients, taken with the absolute value of every
    product, is ``size``: ``|grad d| <= size`` whatever cancels."""
    d = np.random.default_rng(seed).uniform(-1.0, 1.0, shape)
    return d * (size / np.max(_abs_vertex_gradients(d, g), axis=(0, 1, 2)))[:, None, None]


def _shares(err, limit):
    with np.errstate(all="ignore"):
        return {name: float(np.nanmax(err[f] / limit[f])) for f, name in enumerate(hp.VORTEX_CURRENT_FIELDS)}


def test_twin_against_the_longdouble_restatement(mesh, cells):
    """Largest share of the bound used: see the module docstring."""
    conn, g, X = cells
    rng = np.random.default_rng(0)
    w = rng.standard_normal((len(conn), 10, 3)) * rng.uniform(0.1, 10.0, (len(conn), 1, 1)) + rng.standard_normal((len(conn), 1, 3))
    d = _scaled_displacement(w.shape, g, 1)
    means, nums = hp.cell_vortex_current(w, d, g)
    ref_means, ref_nums, J = restated(w, d, g)
    B, kappa, BJ = bounds_current(w, d, g)
    jbar = np.abs(ref_means[5].astype(np.float64))
    assert means.shape == nums.shape == (6, len(conn)) and means.dtype == nums.dtype == np.float64
    assert (J.astype(np.float64) > 0.4).all() and kappa.max() < 4.0                    # det F stays well conditioned
    err_n, err_r = np.abs(nums.astype(LD) - ref_nums).astype(np.float64), np.abs(means.astype(LD) - ref_means).astype(np.float64)
    limit_n, limit_r = K_n(kappa) * EPS * B, K_r(kappa) * EPS * B / jbar
    limit_n[5] = limit_r[5] = 80 * EPS * BJ
    print("numerators, share of the bound used:", _shares(err_n, limit_n))
    print("means, share of the bound used:", _shares(err_r, limit_r), "largest kappa_c:", kappa.max())
    assert (err_n <= limit_n).all() and (err_r <= limit_r).all()
    assert np.array_equal(means[3], np.abs(means[2])) and np.array_equal(nums[3], np.abs(nums[2])) and np.array_equal(means[5], nums[5])
    assert (means[1] > 0).all() and (means[4] > 0).all() and (means[0] < 0).any() and (means[0] > 0).any()
    with pytest.raises(RuntimeError, match="expected"):
        hp.cell_vortex_current(w, d[:, :4], g)


# ---- known answers -------------------------------------------------------------------------------------------------------------

def _fields(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 10, 3)) * rng.uniform(0.1, 10.0, (n, 1, 1)) + rng.standard_normal((n, 1, 3))


def test_zero_displacement_is_the_undeformed_cell_vortex(mesh, cells):
    """With d = 0 every integrand is of degree <= 4 on the cell and the rule exact: fields 0 to 4 are ``hi_pass.cell_vortex``
    within the two derived bounds - that of tests/test_hi_pass_vortex.py for the closed forms, ``K_r(1)`` here -, and the volume
    ratio is 1 within the fourteen additions of the weights.  Largest share of the summed bounds used: 0.0054."""
    conn, g, X = cells
    w = _fields(len(conn), 2)
    for d in (np.zeros_like(w), -np.zeros_like(w)):
        means, nums = hp.cell_vortex_current(w, d, g)
        B, kappa, BJ = bounds_current(w, d, g)
        assert np.array_equal(kappa, np.ones(len(conn))) and np.allclose(BJ, 1.0, rtol=0, atol=16 * EPS)
        limit = K_r(1.0) * EPS * B[:5] + C_REFERENCE * EPS * bounds_reference(w, g)
        err = np.abs(means[:5] - hp.cell_vortex(w, g))
        print("d = 0: share of the two bounds used:", (err / limit).max(axis=1))
        assert (err <= limit).all()
        assert (np.abs(means[5] - 1.0) <= 16 * EPS).all() and (np.abs(nums[:5] - means[:5]) <= 16 * EPS * np.abs(means[:5])).all()


def _rotation():
    axis = np.array([0.3, -1.1, 0.7]).astype(LD)
    axis = axis / np.sqrt((axis * axis).sum())
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=LD)
    a = LD(0.8)
    return np.eye(3, dtype=LD) + np.sin(a) * Kx + (LD(1) - np.cos(a)) * (Kx @ Kx)


def test_a_rigid_rotation_reproduces_the_undeformed_values(mesh, cells):
    """``d = (R - I) X`` and ``w = R u(X)``: the rotated cell carries the rotated field, whose Q, enstrophy, helicity and |w|^2
    are those of u on the undeformed cell, and the volume ratio is 1.  d and w are formed in extended precision and rounded
    once; those roundings and the ones of the closed forms of ``cell_vortex`` are taken as in the d = 0 test, with 64 more for
    the inputs: ``(K_r + 64) 2^-53 B_c + C 2^-53 B_reference``."""
    conn, g, X = cells
    R = _rotation()
    assert (np.abs(R @ R.T - np.eye(3)) < 1e-18).all()
    u = _fields(len(conn), 3)
    d = (X.astype(LD) @ (R - np.eye(3, dtype=LD)).T).astype(np.float64)
    w = (u.astype(LD) @ R.T).astype(np.float64)
    means, nums = hp.cell_vortex_current(w, d, g)
    B, kappa, BJ = bounds_current(w, d, g)
    limit = (K_r(kappa) + 64) * EPS * B[:5] + C_REFERENCE * EPS * bounds_reference(u, g)
    err = np.abs(means[:5] - hp.cell_vortex(u, g))
    print("rigid rotation: share of the bound used:", (err / limit).max(axis=1), "largest kappa_c:", kappa.max())
    assert (err <= limit).all()
    assert (np.abs(means[5] - 1.0) <= (80 + 64) * EPS * BJ).all()
    # the undeformed formula on the rotated field is another number: R u has another gradient with respect to X
    assert (np.abs(hp.cell_vortex(w, g)[2] - hp.cell_vortex(u, g)[2]) > 1e3 * limit[2]).mean() > 0.9


@pytest.mark.parametrize("s", (1.25, 0.8))
def test_a_uniform_dilation_scales_every_field_by_its_power(mesh, cells, s):
    """``d = (s - 1) X``: lengths grow by s.  Q and the enstrophy scale by ``s^-2``, the helicity by ``s^-1``, ``|v|^2`` is
    unchanged and the volume ratio is ``s^3``."""
    conn, g, X = cells
    w = _fields(len(conn), 4)
    d = (s - 1.0) * X
    means, nums = hp.cell_vortex_current(w, d, g)
    want = hp.cell_vortex(w, g).astype(LD) * np.array([s ** -2, s ** -2, 1.0 / s, 1.0 / s, 1.0], dtype=LD)[:, None]
    B, kappa, BJ = bounds_current(w, d, g)
    limit = (K_r(kappa) + 64) * EPS * B[:5] / np.abs(means[5]) + C_REFERENCE * EPS * bounds_reference(w, g) * np.array([s ** -2, s ** -2, 1 / s, 1 / s, 1.0])[:, None]
    err = np.abs(means[:5].astype(LD) - want).astype(np.float64)
    print(f"dilation by {s}: share of the bound used:", (err / limit).max(axis=1))
    assert (err <= limit).all()
    assert (np.abs(means[5] - s ** 3) <= (80 + 64) * EPS * BJ).all()
    assert (np.abs(nums[4] - means[5] * means[4]) <= 2 * EPS * np.abs(nums[4])).all()    # the numerator is the integral: Jbar times the mean


def test_a_quadratic_displacement_has_its_exact_volume(mesh, cells):
    """A P2-representable d: det F is a cubic polynomial on the cell, so ``Jbar`` is the deformed cell's volume ratio - here
    against the degree-6 rule on 24 points in extended precision - and ``cell_wsum`` of it with the undeformed volumes is the
    deformed volume of the listed cells.  The sum's bound: the 80 of Jbar, the product with the weight and the additions of
    the bracket (6 + 2 + the groups), times 2^-53 and the sum of the absolute terms."""
    conn, g, X = cells
    d = _quadratic_displacement(X)
    w = _fields(len(conn), 5)
    means, nums = hp.cell_vortex_current(w, d, g)
    qp, qw = tet_rule_deg6()
    lam6 = np.column_stack([1.0 - qp.sum(axis=1), qp]).astype(LD)
    six = restated(w, d, g, lam6, (qw / qw.sum()).astype(LD))[0][5]
    B, kappa, BJ = bounds_current(w, d, g)
    err = np.abs(means[5].astype(LD) - six).astype(np.float64)
    print("quadratic d: Jbar against degree 6, largest err / (80 2^-53 B_J):", (err / (80 * EPS * BJ)).max(), "Jbar in", means[5].min(), means[5].max())
    assert (err <= (80 + 24) * EPS * BJ).all() and means[5].min() > 1.05 and means[5].max() > means[5].min() + 0.05
    vol = fm.cell_volumes(mesh, np.arange(mesh.num_cells))
    got = hp.cell_wsum(means[5], vol)
    exact = (vol.astype(LD) * six).sum()
    groups = (len(vol) + 255) // 256
    assert abs(float(LD(got) - exact)) <= (80 + 24 + 1 + 8 + groups) * EPS * float((vol * BJ).sum())
    assert abs(got / float(np.sum(vol)) - 1.0) > 0.05                                  # and it is not the undeformed volume
    # the four-point rule of the flow metrics is of degree 2: on a cubic det F it is off, this one is not
    four = hp.cell_rate_current(w, d, g)[1]
    assert np.abs(four.astype(LD) - six).max() > 1e3 * np.abs(means[5].astype(LD) - six).max()


# ---- special values ------------------------------------------------------------------------------------------------------------

def _pair(mesh, cells, frames=12, period=4, ncell=7):
    conn, g, _ = cells
    x, d = _history(mesh, frames, period), _displacements(mesh, frames)
    s, geo = _session(x), _session(d)
    s.cells(conn[:ncell], g[:ncell])
    r = [hp.cell_vortex_current(x[k][conn[:ncell]], d[k][conn[:ncell]], g[:ncell]) for k in range(frames)]
    return x, d, s, geo, np.stack([a[0] for a in r]), np.stack([a[1] for a in r])


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_a_nan_reaches_only_its_cells_and_an_inverted_cell_is_carried_through(mesh, cells):
    conn, g, X = cells
    x, d, s, geo, r, num = _pair(mesh, cells, ncell=40)
    conn, g = conn[:40], g[:40]
    wt = np.random.default_rng(9).uniform(0.5, 2.0, 40)
    for which, node in (("d", int(conn[5, 7])), ("v", int(conn[9, 2]))):
        xx, dd = x.copy(), d.copy()
        (dd if which == "d" else xx)[3, node, 1] = np.nan
        s2, geo2 = _session(xx), _session(dd)
        s2.cells(conn, g)
        s2.cell_weights(wt)
        hit = (conn == node).any(axis=1)
        assert 1 <= hit.sum() < 40
        got, sums = s2.cell_vortex_current("raw", geo2, cells=True, sums=True)
        assert np.isnan(got[:5, hit]).all() and _same(got[:, ~hit], hp.ordered_mean(r)[:, ~hit]) and np.isnan(sums[:5]).all()
        if which == "d":
            assert np.isnan(got[5, hit]).all() and np.isnan(sums[5])
        else:                                                                            # the volume is formed from d alone
            assert _same(got[5], hp.ordered_mean(r)[5]) and np.isfinite(sums[5])
        one = s2.cell_vortex_current("raw", geo2, 2, 1, 1)[0]
        assert _same(one, r[2])                                                          # the other frames are untouched
    # vertex 0 of cell 4 pushed through the opposite face with its three edges (local nodes 7, 8, 9 are their mid-points), in
    # frame 6 only: the cell is the mirror image of itself 1.5 times as high - a volume ratio of -1.5 at every point, no
    # exception, nothing clamped, and the means are finite
    moved = [0, 7, 8, 9]
    assert all(0 in (int(p), int(q)) for p, q in TET_EDGES[3:])
    c = X[4]
    push = (c[1] + c[2] + c[3]) / 3.0 - c[0]
    away = ~np.isin(conn, conn[4, moved]).any(axis=1)
    dd = d.copy()
    dd[6, conn[4, moved]] = 2.5 * push * np.array([1.0, 0.5, 0.5, 0.5])[:, None]
    got, num6 = hp.cell_vortex_current(x[6][conn], dd[6][conn], g)
    assert _same(s.cell_vortex_current("raw", _session(dd), 6, 1, 1)[0], got)
    assert away.sum() >= 20 and _same(got[:, away], r[6][:, away])
    assert -1.7 < got[5, 4] < -1.3                                                       # -1.5 but for the breathing of the other nodes
    assert np.isfinite(got[:, 4]).all() and got[1, 4] > 0 and got[4, 4] > 0 and got[3, 4] >= 0 and num6[1, 4] < 0 and num6[3, 4] >= 0
    # the same cell made flat on an otherwise undeformed mesh: J_p = 0 to rounding at every point, nothing is caught
    flat = np.zeros_like(d[6])
    flat[conn[4, moved]] = push * np.array([1.0, 0.5, 0.5, 0.5])[:, None]
    got = hp.cell_vortex_current(x[6][conn], flat[conn], g)[0]
    assert abs(got[5, 4]) < 1e-12 and (not np.isfinite(got[1, 4]) or got[1, 4] > 1e20) and np.isfinite(got[:, away]).all()


# ---- the twin sessions -----------------------------------------------------------------------------------------------------------

def test_session_twin_orders_frames_pairs_them_and_refuses_what_the_device_refuses(mesh, cells):
    conn, g, _ = cells
    conn, g = conn[:7], g[:7]
    x, d, s, geo, r, num = _pair(mesh, cells)
    what = "hi-pass cell_vortex_current: "
    for k in (0, 5, 11):
        got, sums = s.cell_vortex_current("raw", geo, k, 1, 1)
        assert _same(got, r[k]) and sums is None                                         # one frame: its own bits
    assert _same(s.cell_vortex_current("raw", geo)[0], hp.ordered_mean(r))
    assert _same(s.cell_vortex_current("raw", geo, 1, 4, 3)[0], (((0.0 + r[1]) + r[5]) + r[9]) / 3.0)
    assert _same(s.cell_vortex_current("raw", geo)[0][3], hp.ordered_mean(np.abs(r[:, 2])))      # the mean of |cell mean|, frame by frame
    with pytest.raises(RuntimeError, match=re.escape(what + "sums without weights (cell_weights first)")):
        s.cell_vortex_current("raw", geo, sums=True)
    with pytest.raises(RuntimeError, match=re.escape(what + "neither cells nor sums asked for")):
        s.cell_vortex_current("raw", geo, cells=False)
    wt = np.random.default_rng(7).uniform(0.5, 2.0, 7)
    s.cell_weights(wt)
    none, sums = s.cell_vortex_current("raw", geo, 2, 1, 1, False, True)
    assert none is None and _same(sums, hp.cell_wsum(num[2], wt))                       # the sums are those of the numerators
    assert not _same(sums[:5], hp.cell_wsum(r[2], wt)[:5]) and sums[5] == hp.cell_wsum(r[2][5], wt)
    both = s.cell_vortex_current("raw", geo, 1, 4, 3, True, True)
    assert _same(both[1], hp.cell_wsum((((0.0 + num[1]) + num[5]) + num[9]) / 3.0, wt))
    # the field's selection maps onto recorded d frames, whatever d's own selection is
    assert s.select(2, 4, 2) == 4
    geo.select(1, 3, 3)
    assert _same(s.cell_vortex_current("raw", geo)[0], hp.ordered_mean(r[2:10:2])) and _same(s.cell_vortex_current("raw", geo, 3, 1, 1)[0], r[8])
    # the fluctuation is paired with the raw d frame of the same index, the phase mean with d's phase mean
    s.phase(2)
    f = np.stack([s.fetch("filtered", k) for k in range(4)])
    want = [hp.cell_vortex_current(f[k][conn], d[2 + 2 * k][conn], g)[0] for k in range(4)]
    assert _same(s.cell_vortex_current("series", geo, 1, 2, 2)[0], ((0.0 + want[1]) + want[3]) / 2.0)
    with pytest.raises(RuntimeError, match=re.escape(what + "the session of d has no phase average (phase of d first)")):
        s.cell_vortex_current("phase_mean", geo)
    geo.select(2, 4, 2)
    geo.phase(2)
    pm = [hp.cell_vortex_current(s.phase_fetch("mean", j)[conn], geo.phase_fetch("mean", j)[conn], g)[0] for j in range(2)]
    assert _same(s.cell_vortex_current("phase_mean", geo, 1, 1, 1)[0], pm[1]) and _same(s.cell_vortex_current("phase_mean", geo)[0], hp.ordered_mean(np.stack(pm)))
    # every refusal, in the words of the two functions it joins
    before = s.cell_vortex("raw")[0]
    for series, why in (("filtered", "series must be one of raw, series, phase_mean"),):
        with pytest.raises(RuntimeError, match=re.escape(what + why)):
            s.cell_vortex_current(series, geo)
    with pytest.raises(RuntimeError, match="needs step >= 1 and count >= 1, got step = 0, count = 1"):
        s.cell_vortex_current("raw", geo, 0, 0, 1)
    with pytest.raises(RuntimeError, match=r"frames 3, 3 \+ 1, ... \(2 of them\) fall outside the series of 4 frames"):
        s.cell_vortex_current("raw", geo, 3, 1, 2)
    for none in (None, hp.HostBandSession(3, 12), _session(d[:, :, :1], 1)):
        with pytest.raises(RuntimeError, match=re.escape(what + "no session of d: the current configuration is x = X + d")):
            s.cell_vortex_current("raw", none)
    with pytest.raises(RuntimeError, match=f"the session of d is on {mesh.num_nodes - 1} nodes, the session of the quantity on {mesh.num_nodes}"):
        s.cell_vortex_current("raw", _session(d[:, :-1]))
    with pytest.raises(RuntimeError, match="the session of d has recorded 11 frames, the session of the quantity 12"):
        s.cell_vortex_current("raw", _session(d[:11]))
    geo.phase(1)
    with pytest.raises(RuntimeError, match="the phase average of d has a period of 1 frames, that of the quantity 2"):
        s.cell_vortex_current("phase_mean", geo)
    geo.select(0, 4, 2)
    geo.phase(2)
    with pytest.raises(RuntimeError, match="the phase average of d is over another selection of frames"):
        s.cell_vortex_current("phase_mean", geo)
    assert _same(s.cell_vortex("raw")[0], before)                                       # the refused calls changed nothing
    fresh = _session(x)
    with pytest.raises(RuntimeError, match=re.escape(what + "no cell list (cells first)")):
        fresh.cell_vortex_current("raw", geo)
    fresh.cells(conn, g)
    for series, why in (("series", "no filtered series (filter or phase first)"), ("phase_mean", "no phase average (phase first)")):
        with pytest.raises(RuntimeError, match=re.escape(what + why)):
            fresh.cell_vortex_current(series, geo)
    # the device's forwarder hands the geometry to the context
    calls = []
    backend = type("B", (), {"hi_pass_cell_vortex_current": lambda self, *a, **k: calls.append((a, k))})()
    hp.DeviceSession(backend, "hi_pass", "v").cell_vortex_current("raw", geo, 1, 1, 1, False, sums=True)
    assert calls == [(("v", "raw", 1, 1, 1, False), {"sums": True})]


# ---- the option ------------------------------------------------------------------------------------------------------------------

def test_both_parsers_take_the_option_and_every_refusal_comes_in_its_words(mesh, tmp_path):
    from vasp_amd import postprocess
    from vasp_amd.monolithic import add_session_arguments
    ap = argparse.ArgumentParser()
    add_session_arguments(ap)
    key = "hi_pass_vortex_configuration"
    assert vars(ap.parse_args([]))[key] is None and vx.configuration({}) == "reference" and vx.configuration({key: None}) == "reference"
    assert vars(ap.parse_args(["--hi-pass-vortex-configuration", "current"]))[key] == "current"
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        ap.parse_args(["--hi-pass-vortex-configuration", "deformed"])
    with pytest.raises(SystemExit, match="--hi-pass-vortex-configuration takes reference or current, got 'deformed'"):
        vx.configuration({key: "deformed"})
    assert postprocess.parse(["--folder", "x", "--hi-pass", "d", "v", *CURRENT])[key] == "current"
    assert vx.CONFIGURATIONS == fm.CONFIGURATIONS
    deg2 = ["--save-deg", "2"]
    for q in (["d", "v"], ["v", "d"], ["d", "v", "p"]):
        assert hp.hi_pass_refusal(_parameters(["--hi-pass", *q, *deg2, *CURRENT, *PHASE]), 1, None) == ""
    # beside the flow metrics, in either configuration
    for word in ("reference", "current"):
        both = [*CURRENT, "--hi-pass-flow-metrics", "--hi-pass-flow-metrics-configuration", word]
        assert hp.hi_pass_refusal(_parameters(["--hi-pass", "d", "v", *deg2, *both, *PHASE]), 1, None) == ""
    reference = ["--hi-pass-vortex", "--hi-pass-vortex-configuration", "reference"]
    assert hp.hi_pass_refusal(_parameters(["--hi-pass", "v", *deg2, *reference, *PHASE]), 1, None) == ""
    why = hp.hi_pass_refusal(_parameters(["--hi-pass", "v", "p", *deg2, *CURRENT, *PHASE]), 1, None)
    assert why == vx.NEEDS_D == ("--hi-pass-vortex-configuration current needs d among the --hi-pass quantities: the current configuration is "
                                 "x = X + d, formed from the displacement history")
    assert hp.hi_pass_refusal(_parameters(["--hi-pass", "d", "p", *deg2, *CURRENT, *PHASE]), 1, None) == vx.NEEDS_V      # as before
    assert hp.hi_pass_refusal(_parameters(["--hi-pass", "d", "v", *CURRENT, *PHASE]), 1, None) == vx.NEEDS_DEG2
    for word in ("current", "reference"):                                             # the option without --hi-pass-vortex
        why = hp.hi_pass_refusal(_parameters(["--hi-pass", "d", "v", *deg2, "--hi-pass-vortex-configuration", word, *PHASE]), 1, None)
        assert why == vx.NEEDS_VORTEX_CONFIGURATION == "--hi-pass-vortex-configuration chooses the configuration of --hi-pass-vortex: it needs that option"
    assert all("\n" not in text for text in (vx.NEEDS_D, vx.NEEDS_VORTEX_CONFIGURATION))
    # the driver refuses before it opens a session; strips of rows stay refused
    ns = dict(_parameters(["--hi-pass", "v", *deg2, *CURRENT]), save_deg=2, results_folder=tmp_path)
    with pytest.raises(SystemExit) as e:
        hp.HiPassRun(object(), mesh, ns)
    assert str(e.value) == vx.NEEDS_D
    ns = dict(_parameters(["--hi-pass", "d", "v", *deg2, "--hi-pass-vortex-configuration", "current"]), save_deg=2, results_folder=tmp_path)
    with pytest.raises(SystemExit) as e:
        hp.HiPassRun(object(), mesh, ns)
    assert str(e.value) == vx.NEEDS_VORTEX_CONFIGURATION
    ns = dict(_parameters(["--hi-pass", "d", "v", *deg2, *CURRENT]), save_deg=2, results_folder=tmp_path, hi_pass_strip=(0, 8))
    with pytest.raises(SystemExit) as e:
        hp.HiPassRun(object(), mesh, ns)
    assert str(e.value) == vx.VORTEX_STRIPS and not (tmp_path / "VortexMetrics").exists()


# ---- the driver with a stub backend ----------------------------------------------------------------------------------------------

SERIES = [*CURRENT, "--hi-pass-vortex-series"]


def _twin_files(mesh, ns_like, x, d, folder, period=None, series=True, grad=None):
    """``<folder>/VortexMetrics`` as ``vortex.VortexMetrics`` writes it from the twin sessions of the frames x and d."""
    ns = dict(ns_like, results_folder=folder, hi_pass_vortex=True, hi_pass_vortex_series=series, hi_pass_vortex_configuration="current")
    metrics = vx.VortexMetrics(mesh, ns)
    s, geo = _session(x), _session(d)
    n = len(x)
    for a in (geo, s):
        a.select(0, n, 1)
    metrics.attach(s, False, grad)
    metrics.collect(s, n, 0.001, 0.0, geo)
    if period:
        m = n // period * period
        for a in (geo, s):
            a.select(0, m, 1)
            a.phase(period)
        metrics.collect_phase(s, period, geo)
    lines = []
    metrics.write(lines.append, 0.001, 0.0)
    return metrics, lines


def test_driver_writes_the_current_configuration_files(tmp_path, mesh):
    """14 saved frames, ``--hi-pass v d``, three whole cycles of 4: every file is what the closing formulas give on the twin's
    six means and numerator sums of the velocity and displacement frames the run wrote; the volume column varies in time."""
    ns, lines = _run(tmp_path / "cur" / "case", T="0.0135", options=["--hi-pass", "v", "d", *SERIES, *PHASE])
    results = tmp_path / "cur" / "case" / "1"
    out = results / "VortexMetrics"
    x, d = _velocity(results), _displacement(results)
    assert x.shape == d.shape == (14, mesh.num_nodes, 3)
    assert {p.name for p in out.iterdir()} == _files(MEAN_FILES + ("volume_ratio",) + PHASE_FILES + vx.SERIES_FILES) | TABLES
    cells = fm.fluid_cells(mesh, ns["dx_f_id"])
    conn, g, vol = mesh.tet_nodes[cells], fm.barycentric_gradients(mesh, cells), fm.cell_volumes(mesh, cells)
    both = [hp.cell_vortex_current(x[k][conn], d[k][conn], g) for k in range(14)]
    r, num = np.stack([a[0] for a in both]), np.stack([a[1] for a in both])
    mean = hp.ordered_mean(r)
    with np.errstate(all="ignore"):
        want = dict(q_criterion_avg=mean[0], vorticity_rms=np.sqrt(mean[1]), helicity_avg=mean[2], helicity_intensity=mean[3],
                    helicity_balance=vx.ratio_or_zero(mean[2], mean[3]), kinetic_energy_avg=0.5 * mean[4], volume_ratio=mean[5])
        series = dict(q_criterion=r[:, 0], vorticity=np.sqrt(r[:, 1]), helicity=r[:, 2], lnh=vx.ratio_or_zero(r[:, 2], np.sqrt(r[:, 4] * r[:, 1])))
        for name, values in want.items():
            got = _vectors(out / f"{name}.h5")
            assert got.shape == (1, len(cells), 1) and got.dtype == np.float32 and _same(got[0, :, 0], values.astype(np.float32)), name
        for name, values in series.items():
            assert _same(_vectors(out / f"{name}.h5")[:, :, 0], values.astype(np.float32)), name
    # vortex.csv: the volume of each frame and the integrals over it, from the numerator sums
    text = (out / "vortex.csv").read_text().splitlines()
    assert text[0] == "# " + vx.CURVES_HEADER and len(text) == 15
    table = np.array([[float(a) for a in line.split(", ")] for line in text[1:]])
    sums = np.stack([hp.cell_wsum(num[k], vol) for k in range(14)])
    assert _same(table[:, 1], sums[:, 5]) and len(set(table[:, 1])) == 14 and not (table[:, 1] == np.sum(vol)).any()
    assert _same(table[:, 2:], np.stack([0.5 * sums[:, 4], sums[:, 1], sums[:, 2], sums[:, 3], sums[:, 0]], axis=1))
    h = [float(a) for a in (out / "helicity_indices.csv").read_text().splitlines()[1].split(", ")]
    with np.errstate(all="ignore"):
        assert _same(h[0], float(hp.ordered_mean(sums[:, 2] / sums[:, 5]))) and _same(h[1], float(hp.ordered_mean(sums[:, 3] / sums[:, 5])))
    # the summary's weights are volume * volume_ratio
    rows = {row.split(", ")[0]: row.split(", ")[1:] for row in (out / "vortex_summary.csv").read_text().splitlines()[1:]}
    assert list(rows) == [*MEAN_FILES, "volume_ratio", "vorticity_rms_fluctuation"]
    with np.errstate(all="ignore"):
        row = fm.summary_row(want["vorticity_rms"], vol * mean[5], cells)
    assert [float(a) for a in rows["vorticity_rms"][:3]] == pytest.approx(list(row[:3]), rel=0, abs=0, nan_ok=True)
    # the phase files, and all of it once more as the twin's own files, byte for byte
    metrics, said = _twin_files(mesh, ns, x, d, tmp_path / "twin", period=4)
    got, twin = _tree_of(out), _tree_of(tmp_path / "twin" / "VortexMetrics")
    assert sorted(got) == sorted(twin) and len(got) == 2 * 13 + 3
    for name in twin:
        assert got[name] == twin[name], name
    line = [text for text in lines if text.startswith("Vortex metrics of")]
    assert len(line) == 1 and f"{len(cells)} fluid cells over 14 frames in the current configuration" in line[0] and "volume_ratio" in line[0]
    # d before v, whatever the order given
    assert [l.split()[1].rstrip(":") for l in lines if "phase average over cycles" in l] == ["displacement", "velocity"]
    # with the flow metrics beside it, in either configuration, the vortex files keep their bytes and the cells are attached once
    for word in ("reference", "current"):
        _run(tmp_path / word / "case", T="0.0135", options=["--hi-pass", "v", "d", *SERIES, *PHASE, "--hi-pass-flow-metrics",
                                                             "--hi-pass-flow-metrics-configuration", word])
        assert _tree_of(tmp_path / word / "case" / "1" / "VortexMetrics") == got, word


def test_reference_is_a_run_without_the_word(tmp_path):
    base = ["--hi-pass", "v", "d", "--hi-pass-vortex", "--hi-pass-vortex-series", *PHASE]
    _, old = _run(tmp_path / "old" / "case", T="0.0135", options=base)
    _, new = _run(tmp_path / "new" / "case", T="0.0135", options=[*base, "--hi-pass-vortex-configuration", "reference"])
    for sub in ("VortexMetrics", "Visualization_hi_pass"):
        a, b = _tree_of(tmp_path / "old" / "case" / "1" / sub), _tree_of(tmp_path / "new" / "case" / "1" / sub)
        assert a == b and len(a) > 4, sub
    assert not (tmp_path / "new" / "case" / "1" / "VortexMetrics" / "volume_ratio.h5").exists()
    strip = lambda lines: [l.replace(str(tmp_path / "old"), "").replace(str(tmp_path / "new"), "") for l in lines]
    assert strip(old) == strip(new) and any("in the reference configuration" in l for l in new if l.startswith("Vortex metrics of"))


class _HostOnly:
    """A backend without device sessions: ``postprocess`` then records on the host twin."""

    def __init__(self, desc):
        pass


def test_a_split_run_and_postprocess_write_the_bytes_of_an_unsplit_run(tmp_path):
    """The option keeps no state of its own: a run stopped after 17 of 40 steps and continued with --restart-folder, and
    ``postprocess`` on the finished folder of the unsplit run, write the files of the unsplit run."""
    from vasp_amd import postprocess
    options = ["--hi-pass", "d", "v", *SERIES, *PHASE]
    _run(tmp_path / "whole" / "case", options=options)
    half = tmp_path / "half" / "case" / "1"
    half.mkdir(parents=True)
    ns, lines = _run(half.parent, options=options, kill_at=SPLIT, kill_path=half / "killturtle")
    assert ns["backend"].steps == SPLIT
    ns, lines = _restart(half, options=options)
    assert any("Vortex metrics of" in line and "over 40 frames in the current configuration" in line for line in lines)
    whole, split = _tree_of(tmp_path / "whole" / "case" / "1" / "VortexMetrics"), _tree_of(half / "VortexMetrics")
    assert sorted(whole) == sorted(split) and len(whole) == 2 * 13 + 3
    for name in whole:
        assert whole[name] == split[name], name
    said = []
    with contextlib.redirect_stdout(io.StringIO()):
        postprocess.run(["--folder", str(tmp_path / "whole" / "case" / "1"), "--output-folder", str(tmp_path / "post"), *options],
                        backend_factory=_HostOnly, out=said.append)
    post = _tree_of(tmp_path / "post" / "VortexMetrics")
    assert sorted(post) == sorted(whole) and any("in the current configuration" in line for line in said)
    for name in whole:
        assert post[name] == whole[name], name


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------

def test_header_binding_and_tables_agree():
    from vasp_amd import capi
    header = (ROOT / "include" / "vaspfsi.h").read_text()
    lib = capi.load_library()
    name = "fsi_band_cell_vortex_current"
    m = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S)
    assert m and name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")) == 8
    comment = header[:m.start()].rsplit("/*", 1)[1]
    assert "Replaces: nothing in the reference." in comment
    assert capi.HipBackend.VORTEX_CURRENT_FIELDS == hp.VORTEX_CURRENT_FIELDS == hp.VORTEX_FIELDS + ("volume_ratio",)
    assert re.search(r"#define FSI_VORTEX_VOLUME_RATIO 5\b", header) and re.search(r"#define FSI_VORTEX_CURRENT_FIELDS 6\b", header)
    assert re.search(r"#define FSI_VORTEX_FIELDS 5\b", header) and hasattr(capi.HipBackend, "hi_pass_cell_vortex_current")
    assert (vx.Q, vx.ENSTROPHY, vx.HELICITY, vx.ABS_HELICITY, vx.SPEED2, vx.VOLUME_RATIO) == tuple(range(6))
    assert re.search(r"^int %s\(FsiCtx\* ctx" % name, (ROOT / "vasp_amd" / "csrc" / "fsi_sessions.hip").read_text(), flags=re.M)
    src = (ROOT / "vasp_amd" / "csrc" / "fsi_vortex.hip").read_text()
    assert "__launch_bounds__(256) void k_cell_vortex_current" in src
    assert src.index("#pragma clang fp contract(off)") < src.index("k_cell_vortex_current(int64_t n")
    # the six constants stand with all their digits in the kernel, the header's comment and the twin
    for text in ("0.31088591926330060980", "0.11268792571801585080", "0.092735250310891226402", "0.073493043116361949544",
                 "0.045503704125649649492", "0.042546020777081466438"):
        assert text in src and text in comment and text in (ROOT / "vasp_amd" / "hi_pass.py").read_text(), text
    hpp = (ROOT / "vasp_amd" / "csrc" / "fsi_vortex.hpp").read_text()
    assert "launch_cell_vortex_current" in hpp and re.search(r"k_cell_vortex_current: \d+ VGPRs, \d+ AGPRs, \d+ SGPRs, no scratch", hpp)
    lam, om, basis = hp.vortex_rule()
    assert np.array_equal(lam, hp.VORTEX_RULE_LAM) and np.array_equal(om, hp.VORTEX_RULE_OM) and np.array_equal(basis, hp.VORTEX_RULE_BASIS)
