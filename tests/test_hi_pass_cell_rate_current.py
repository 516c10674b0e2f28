"""The strain rate of a recorded history in the current configuration ``x = X + d(X)``, host side: the NumPy twin of
k_cell_rate_current (``hi_pass.cell_rate_current``, ``HostBandSession.cell_rate_current``) against an independent restatement
in extended precision, against known answers on curved cells and against the degree-6 rule; the ordered sums over frames, the
pairing of the field's frames with the displacement's, special values, the twin's refusals, the option
``--hi-pass-flow-metrics-configuration`` and the driver's files with a stub backend.

The per-cell bound ``K_c * 2^-53 * B_c``.  ``B_c`` is the twin's formula with the absolute value of every product in the
numerators and the true ``|J_q|`` in the denominators.  ``K_c`` counts the roundings on the longest path from an input to the
result, to first order:

* a vertex gradient entry: a coefficient times a gradient value, a sum inside an edge term, the product with the nodal value
  and ten additions - 13;
* the sum over the four vertices +4, ``b * sum`` and ``(a - b) * G_q`` and their sum +2, and ``a - b`` itself and the
  restatement's ``1 - 3 b`` in the place of a, +2: 21 for an entry of ``G_q`` or ``D_q``; ``1 + D_q`` +1: 22 for F;
* an adjugate entry: two entries of F, a product, a difference - 46; ``J_q``: F times adj, +1, two additions - 71, relative to
  ``B_J``, the determinant with the absolute value of every product;
* the numerator of ``L_q``: ``G_q`` times adj, +1, two additions - 70; the division +1.  The error of ``J_q`` enters a quotient
  relative to ``|J_q|``, not to ``B_J``: with ``kappa = max_q B_J / |J_q|`` of the cell, the conditioning of its determinants,
  it counts ``71 kappa``.  ``L_q``: ``71 + 71 kappa``;
* ``S_q`` +1, its square twice that +1, nine of them summed +9: ``154 + 142 kappa``; ``J_q e_q``: ``+ 71 kappa + 1``, four
  summed +4: ``159 + 213 kappa``; the denominator ``sum_q J_q``: ``71 kappa + 4``; the last division +1.

``K_c = 164 + 284 kappa_c`` (448 where d = 0).  The volume ratio is held to ``76 * 2^-53`` times the mean of the four ``B_J``.

Largest ``err / (2^-53 B_c)`` observed against the restatement: 0.72, where the bound allows 448 and more (random v, random d
with ``|grad d| <= 0.3``, kappa_c up to 2.9, J between 0.67 and 1.5)."""
import argparse

import numpy as np
import pytest

from conftest import ROOT
from test_hi_pass_cell_rate import EPS, LD, PHASE, _history, _parameters, _session, _vectors, _velocity
from test_session_restart import CYL, _run, one_modification_time  # noqa: F401  (the fixture holds h5lite's clock)
from vasp_amd import flow_metrics as fm
from vasp_amd import hi_pass as hp
from vasp_amd.mesh import TET_EDGES, FsiMesh
from vasp_amd.quadrature import tabulate_tet, tet_rule_deg6

A_, B_ = hp.RULE_A, hp.RULE_B
RULE_POINTS = np.array([[B_, B_, B_], [A_, B_, B_], [B_, A_, B_], [B_, B_, A_]])      # barycentric coordinates 1 .. 3 of point q
RULE_WEIGHTS = np.full(4, 1.0 / 24.0)
CURRENT = ["--hi-pass-flow-metrics", "--hi-pass-flow-metrics-configuration", "current"]


def K(kappa):
    return 164.0 + 284.0 * kappa


@pytest.fixture(scope="module")
def mesh():
    return FsiMesh.read(CYL)


@pytest.fixture(scope="module")
def cells(mesh):
    """Every cell of the cylinder fixture: its P2 nodes, the gradients of its barycentric coordinates, its node coordinates."""
    c = np.arange(mesh.num_cells)
    return mesh.tet_nodes[c], fm.barycentric_gradients(mesh, c), mesh.node_coords[mesh.tet_nodes[c]]


def _abs_vertex_gradients(w, g):
    """``hi_pass.vertex_gradients`` with the absolute value of every product."""
    w, g = np.abs(w), np.abs(g)
    G = [[[None] * 3 for _ in range(3)] for _ in range(4)]
    for t in range(4):
        for i in range(3):
            for j in range(3):
                s = np.zeros(len(w))
                for a in range(4):
                    s = s + w[:, a, i] * ((3.0 if a == t else 1.0) * g[:, a, j])
                for e in range(6):
                    p, r = TET_EDGES[e]
                    s = s + (w[:, 4 + e, i] * 4.0) * ((1.0 if p == t else 0.0) * g[:, r, j] + (1.0 if r == t else 0.0) * g[:, p, j])
                G[t][i][j] = s
    return G


def _chain(G, D, J_true=None):
    """The arithmetic of ``hi_pass.cell_rate_current`` after the vertex gradients.  With ``J_true`` (4, cells): the same with a
    sum in the place of every difference - G and D are absolute sums then - and ``|J_true|`` where J divides or weights.
    Returns (rate, J (4, cells))."""
    n = len(G[0][0][0])
    sign = 1.0 if J_true is None else -1.0
    TG = [[((G[0][i][j] + G[1][i][j]) + G[2][i][j]) + G[3][i][j] for j in range(3)] for i in range(3)]
    TD = [[((D[0][i][j] + D[1][i][j]) + D[2][i][j]) + D[3][i][j] for j in range(3)] for i in range(3)]
    num, den, Js = np.zeros(n), np.zeros(n), []
    for q in range(4):
        g = [[B_ * TG[i][j] + (A_ - B_) * G[q][i][j] for j in range(3)] for i in range(3)]
        F = [[(1.0 if i == j else 0.0) + (B_ * TD[i][j] + (A_ - B_) * D[q][i][j]) for j in range(3)] for i in range(3)]
        m = lambda a, b, c, d: F[a[0]][a[1]] * F[b[0]][b[1]] - sign * (F[c[0]][c[1]] * F[d[0]][d[1]])
        A = [[m((1, 1), (2, 2), (1, 2), (2, 1)), m((0, 2), (2, 1), (0, 1), (2, 2)), m((0, 1), (1, 2), (0, 2), (1, 1))],
             [m((1, 2), (2, 0), (1, 0), (2, 2)), m((0, 0), (2, 2), (0, 2), (2, 0)), m((0, 2), (1, 0), (0, 0), (1, 2))],
             [m((1, 0), (2, 1), (1, 1), (2, 0)), m((0, 1), (2, 0), (0, 0), (2, 1)), m((0, 0), (1, 1), (0, 1), (1, 0))]]
        J = (F[0][0] * A[0][0] + F[0][1] * A[1][0]) + F[0][2] * A[2][0]
        Js.append(J)
        Jd = J if J_true is None else np.abs(J_true[q])
        L = [[((g[i][0] * A[0][j] + g[i][1] * A[1][j]) + g[i][2] * A[2][j]) / Jd for j in range(3)] for i in range(3)]
        e = sum(0.5 * (L[i][j] + L[j][i]) * (0.5 * (L[i][j] + L[j][i])) for i in range(3) for j in range(3))
        num, den = num + Jd * (2.0 * e), den + Jd
    return num / den, np.stack(Js)


def bound_current(v, d, g):
    """(B_c, kappa_c, B of the volume ratio) of the module docstring."""
    v, d, g = (np.asarray(a, dtype=np.float64) for a in (v, d, g))
    with np.errstate(all="ignore"):
        _, J = _chain(hp.vertex_gradients(v, g), hp.vertex_gradients(d, g))
        B, BJ = _chain(_abs_vertex_gradients(v, g), _abs_vertex_gradients(d, g), J)
        return B, (BJ / np.abs(J)).max(axis=0), 0.25 * BJ.sum(axis=0)


def by_quadrature(v, d, g, points=RULE_POINTS, weights=RULE_WEIGHTS):
    """(rate, volume ratio, smallest J) by a rule on the reference tetrahedron in ``np.longdouble``: the P2 basis gradients at
    the points (``tabulate_tet``) mapped by the gradients of the barycentric coordinates 1 .. 3, F = I + grad d, its inverse by
    cross products of its rows, the J-weighted mean.  No vertex value of a gradient is formed."""
    dN = tabulate_tet(np.asarray(points, dtype=np.float64))[1].astype(LD)      # (Q, 10, 3)
    v, d, g, qw = (np.asarray(a).astype(LD) for a in (v, d, g, weights))
    phys = np.einsum("qak,ckj->cqaj", dN, g[:, 1:4])
    G, F = np.einsum("cai,cqaj->cqij", v, phys), np.einsum("cai,cqaj->cqij", d, phys) + np.eye(3, dtype=LD)
    r0, r1, r2 = F[:, :, 0], F[:, :, 1], F[:, :, 2]
    c0, c1, c2 = np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)            # the columns of adj F
    J = np.einsum("cqi,cqi->cq", r0, c0)
    inv = np.stack([c0, c1, c2], axis=3) / J[:, :, None, None]
    L = np.einsum("cqik,cqkj->cqij", G, inv)
    S = (L + L.transpose(0, 1, 3, 2)) / LD(2)
    e = LD(2) * np.einsum("cqij,cqij->cq", S, S)
    return (e * J) @ qw / (J @ qw), (J @ qw) / qw.sum(), J.min(axis=1)


def test_twin_against_the_longdouble_restatement(mesh, cells):
    """Random v and random nodal d, scaled per cell so that the largest entry of the vertex gradients of d, taken with the
    absolute value of every product, is 0.3: ``|grad d| <= 0.3`` whatever cancels, and det F stays well conditioned.  Largest
    err / (2^-53 B_c): see the module docstring."""
    conn, g, X = cells
    rng = np.random.default_rng(0)
    v = rng.standard_normal((len(conn), 10, 3)) * rng.uniform(0.1, 10.0, (len(conn), 1, 1))
    d = rng.uniform(-1.0, 1.0, v.shape)
    d = d * (0.3 / np.max(_abs_vertex_gradients(d, g), axis=(0, 1, 2)))[:, None, None]
    rate, vol, mj = hp.cell_rate_current(v, d, g)
    ref_rate, ref_vol, ref_mj = by_quadrature(v, d, g)
    B, kappa, Bvol = bound_current(v, d, g)
    assert (mj > 0.5).all() and kappa.max() < 4.0                                     # det F stays well conditioned
    err = np.abs(rate.astype(LD) - ref_rate).astype(np.float64)
    print("largest err / (2^-53 B_c):", (err / (EPS * B)).max(), "largest kappa_c:", kappa.max(), "J from", mj.min(), "volume ratio to", vol.max())
    assert (err <= K(kappa) * EPS * B).all()
    assert (np.abs(vol.astype(LD) - ref_vol).astype(np.float64) <= 76 * EPS * Bvol).all()
    assert (np.abs(mj.astype(LD) - ref_mj).astype(np.float64) <= 71 * EPS * 4.0 * Bvol).all()
    assert all(a.dtype == np.float64 and a.shape == (len(conn),) for a in (rate, vol, mj)) and (rate > 0).all()
    with pytest.raises(RuntimeError, match="expected"):
        hp.cell_rate_current(v, d[:, :4], g)


def _quadratic_displacement(X):
    """d = affine + quadratic in X, a P2 field: the cells of x = X + d are curved.  det F between about 1.1 and 1.5."""
    L = np.abs(X).max()
    Xs = X / L
    Bm = np.array([[0.10, 0.03, -0.02], [0.00, 0.08, 0.04], [-0.03, 0.02, 0.06]])
    quad = np.stack([0.04 * Xs[..., 0] * Xs[..., 1], 0.05 * Xs[..., 1] * Xs[..., 1] - 0.03 * Xs[..., 2] * Xs[..., 0], 0.04 * Xs[..., 2] * Xs[..., 2]], axis=-1)
    return (Xs @ Bm.T + quad) * L


def test_known_answers_on_curved_cells(mesh, cells):
    """``v = A x(X)`` on ``x = X + d`` with a quadratic d has ``L = A`` at every point: ``rate = 2 sym(A):sym(A)``; a rigid
    rotation ``v = omega x x(X)`` has 0.  v is formed in extended precision and rounded once.  The inputs carry roundings of
    their own - the mid-edge coordinates, the inverse of the cell's Jacobian behind the gradients, v itself - which the bound
    takes as 64 more: ``(K_c + 64) 2^-53 B_c``.  The undeformed ``cell_rate`` misses the answer by more than 10 % (measured: 40 %)."""
    conn, g, X = cells
    d = _quadratic_displacement(X)
    x = X.astype(LD) + d.astype(LD)
    rng = np.random.default_rng(1)
    A = rng.standard_normal((3, 3))
    sym = 0.5 * (A + A.T)
    exact = 2.0 * np.sum(sym * sym)
    v = (x @ A.T.astype(LD)).astype(np.float64)
    rate, vol, mj = hp.cell_rate_current(v, d, g)
    B, kappa, _ = bound_current(v, d, g)
    assert (mj > 0).all() and (by_quadrature(v, d, g, *tet_rule_deg6())[2] > 0).all()      # every J_q > 0, at the 24 points too
    print("v = A x: largest err / (2^-53 B_c):", (np.abs(rate - exact) / (EPS * B)).max(), "J in", mj.min(), vol.max())
    assert (np.abs(rate - exact) <= (K(kappa) + 64) * EPS * B).all()
    off = np.abs(hp.cell_rate(v, g) - exact) / exact
    print("the undeformed cell_rate is off by up to", off.max())
    assert off.max() > 0.10
    omega = np.array([0.3, -1.1, 0.7]).astype(LD)
    v = np.cross(omega, x).astype(np.float64)
    rate = hp.cell_rate_current(v, d, g)[0]
    B, kappa, _ = bound_current(v, d, g)
    assert (np.abs(rate) <= (K(kappa) + 64) * EPS * B).all() and (B > 0).all()


def test_zero_displacement_is_the_undeformed_rate(mesh, cells):
    from test_hi_pass_cell_rate import bound
    conn, g, X = cells
    rng = np.random.default_rng(2)
    v = rng.standard_normal((len(conn), 10, 3)) * rng.uniform(0.1, 10.0, (len(conn), 1, 1))
    d = np.zeros_like(v)
    rate, vol, mj = hp.cell_rate_current(v, d, g)
    B, kappa, _ = bound_current(v, d, g)
    assert np.array_equal(kappa, np.ones(len(conn)))
    err = np.abs(rate - hp.cell_rate(v, g))
    print("d = 0: largest relative difference to cell_rate:", (err / rate).max())
    assert (err <= K(1.0) * EPS * B + 80 * EPS * bound(v, g)).all()
    assert np.array_equal(vol, np.ones(len(conn))) and np.array_equal(mj, np.ones(len(conn)))
    rate, vol, mj = hp.cell_rate_current(v, -d, g)                                    # d = -0.0 as well
    assert np.array_equal(vol, np.ones(len(conn))) and np.array_equal(mj, np.ones(len(conn)))


def test_rule_against_the_degree_6_rule(mesh, cells):
    """Radial breathing of 5 % modulated along the axis (y) and a quadratic velocity: the four-point rule against the
    J-weighted degree-6 rule, both in longdouble.  Measured: maximum 3.8e-5, median 2.1e-6 relative; the undeformed formula is off by up to 15 %."""
    conn, g, X = cells
    half = np.abs(X[..., 1]).max()
    amp = 0.05 * (1.0 + 0.5 * np.cos(np.pi * X[..., 1] / half))
    d = np.stack([amp * X[..., 0], np.zeros_like(amp), amp * X[..., 2]], axis=-1)
    Xs = X / np.abs(X).max()
    v = np.stack([Xs[..., 1] * Xs[..., 1] - 0.5 * Xs[..., 0] * Xs[..., 2], 0.3 * Xs[..., 0] * Xs[..., 1] + Xs[..., 2],
                  1.0 - Xs[..., 0] * Xs[..., 0] - Xs[..., 2] * Xs[..., 2] + 0.2 * Xs[..., 1]], axis=-1)
    four = by_quadrature(v, d, g)[0]
    six = by_quadrature(v, d, g, *tet_rule_deg6())[0]
    rel = (np.abs(four - six) / six).astype(np.float64)
    print("four points against degree 6: maximum", rel.max(), "median", np.median(rel))
    assert rel.max() <= 1e-3
    twin = hp.cell_rate_current(v, d, g)[0]
    assert (np.abs(twin - six.astype(np.float64)) / twin).max() <= 1e-3
    undeformed = np.abs(hp.cell_rate(v, g) - six.astype(np.float64)) / six.astype(np.float64)
    print("the undeformed cell_rate against degree 6: maximum", undeformed.max())
    assert undeformed.max() > 0.05


# ---- frames ----------------------------------------------------------------------------------------------------------------

def _displacements(mesh, frames, seed=3):
    """(frames, N2, 3): a breathing of a few percent that changes from frame to frame, plus noise."""
    rng = np.random.default_rng(seed)
    X = mesh.node_coords
    amp = 0.03 * np.sin(0.9 * np.arange(frames) + 0.4)[:, None]
    d = np.stack([amp * X[:, 0], 0.5 * amp * X[:, 1], amp * X[:, 2]], axis=-1)
    return d + 2e-6 * rng.standard_normal(d.shape)


def _pair(mesh, cells, frames=12, period=4, ncell=7):
    conn, g, _ = cells
    x, d = _history(mesh, frames, period), _displacements(mesh, frames)
    s, geo = _session(x), _session(d)
    s.cells(conn[:ncell], g[:ncell])
    r = [hp.cell_rate_current(x[k][conn[:ncell]], d[k][conn[:ncell]], g[:ncell]) for k in range(frames)]
    return x, d, s, geo, [np.stack([f[i] for f in r]) for i in range(3)]


def _min(J):
    m = np.full(J.shape[1:], np.inf)
    for row in J:
        m = np.where(row < m, row, m)
    return m


def _same(got, rate, vol, mj):
    return np.array_equal(got[0], rate, equal_nan=True) and np.array_equal(got[1], vol, equal_nan=True) and np.array_equal(got[2], mj, equal_nan=True)


def test_ordered_sums_strides_windows_and_the_phase_pairing(mesh, cells):
    conn, g, _ = cells
    conn, g = conn[:7], g[:7]
    x, d, s, geo, (r, vol, mj) = _pair(mesh, cells)
    for k in (0, 5, 11):
        assert _same(s.cell_rate_current("raw", geo, k, 1, 1), r[k], vol[k], mj[k])          # one frame: its own bits
    assert _same(s.cell_rate_current("raw", geo), hp.ordered_mean(r), hp.ordered_mean(vol), _min(mj))
    assert _same(s.cell_rate_current("raw", geo, 1, 4, 3), (((0.0 + r[1]) + r[5]) + r[9]) / 3.0, (((0.0 + vol[1]) + vol[5]) + vol[9]) / 3.0, _min(mj[1::4]))
    assert _same(s.cell_rate_current("raw", geo, 2, 3), hp.ordered_mean(r[2::3]), hp.ordered_mean(vol[2::3]), _min(mj[2::3]))
    assert (mj.min(axis=0) < mj.max(axis=0)).all() and np.array_equal(s.cell_rate_current("raw", geo)[2], mj.min(axis=0))
    # the field's selection maps onto recorded d frames, whatever d's own selection is
    assert s.select(2, 4, 2) == 4
    geo.select(1, 3, 3)
    assert _same(s.cell_rate_current("raw", geo), hp.ordered_mean(r[2:10:2]), hp.ordered_mean(vol[2:10:2]), _min(mj[2:10:2]))
    assert _same(s.cell_rate_current("raw", geo, 3, 1, 1), r[8], vol[8], mj[8])
    # the fluctuation is paired with the raw d frame of the same index, the phase mean with d's phase mean
    s.phase(2)
    f = np.stack([s.fetch("filtered", k) for k in range(4)])
    want = [hp.cell_rate_current(f[k][conn], d[2 + 2 * k][conn], g) for k in range(4)]
    assert _same(s.cell_rate_current("series", geo, 1, 2, 2), ((0.0 + want[1][0]) + want[3][0]) / 2.0, ((0.0 + want[1][1]) + want[3][1]) / 2.0,
                 _min(np.stack([want[1][2], want[3][2]])))
    with pytest.raises(RuntimeError, match="the session of d has no phase average"):
        s.cell_rate_current("phase_mean", geo)
    geo.select(2, 4, 2)
    geo.phase(2)
    pm = [hp.cell_rate_current(s.phase_fetch("mean", j)[conn], geo.phase_fetch("mean", j)[conn], g) for j in range(2)]
    assert _same(s.cell_rate_current("phase_mean", geo, 1, 1, 1), *pm[1])
    assert _same(s.cell_rate_current("phase_mean", geo), hp.ordered_mean(np.stack([p[0] for p in pm])), hp.ordered_mean(np.stack([p[1] for p in pm])),
                 _min(np.stack([p[2] for p in pm])))
    # period 4 x 3 cycles: the cycle means at each phase
    s.select(0, 12, 1)
    s.phase(4)
    f = np.stack([s.fetch("filtered", k) for k in range(12)])
    for j in range(4):
        want = [hp.cell_rate_current(f[k][conn], d[k][conn], g) for k in range(j, 12, 4)]
        assert _same(s.cell_rate_current("series", geo, j, 4, 3), *(hp.ordered_mean(np.stack([w[i] for w in want])) for i in range(2)),
                     _min(np.stack([w[2] for w in want])))


def test_a_nan_reaches_only_its_cells_and_an_inverted_cell_is_carried_through(mesh, cells):
    conn, g, X = cells
    x, d, s, geo, (r, vol, mj) = _pair(mesh, cells, ncell=40)
    conn, g = conn[:40], g[:40]
    for which, node in (("d", int(conn[5, 7])), ("v", int(conn[9, 2]))):
        xx, dd = x.copy(), d.copy()
        (dd if which == "d" else xx)[3, node, 1] = np.nan
        s2, geo2 = _session(xx), _session(dd)
        s2.cells(conn, g)
        hit = (conn == node).any(axis=1)
        assert 1 <= hit.sum() < 40
        got = s2.cell_rate_current("raw", geo2)
        assert np.isnan(got[0][hit]).all() and np.array_equal(got[0][~hit], hp.ordered_mean(r)[~hit])
        assert np.array_equal(got[1][~hit], hp.ordered_mean(vol)[~hit]) and np.array_equal(got[2][~hit], _min(mj)[~hit])
        if which == "d":      # the NaN J never replaces the minimum: it is that of the other frames
            assert np.isnan(got[1][hit]).all() and np.isfinite(got[2][hit]).all()
            assert np.array_equal(got[2][hit], _min(np.delete(mj, 3, axis=0))[hit])
        else:
            assert np.array_equal(got[1], hp.ordered_mean(vol)) and np.array_equal(got[2], _min(mj))
    # vertex 0 of cell 4 pushed through the opposite face, in frame 6 only
    dd = d.copy()
    c = X[4]
    centre = (c[1] + c[2] + c[3]) / 3.0
    dd[6, conn[4, 0]] = 2.5 * (centre - c[0])
    geo2 = _session(dd)
    got = s.cell_rate_current("raw", geo2)                                          # no exception
    assert got[2][4] < 0 and np.array_equal(got[2][4], s.cell_rate_current("raw", geo2, 6, 1, 1)[2][4])
    away = ~(conn == conn[4, 0]).any(axis=1)
    assert away.sum() >= 20 and _same([a[away] for a in got], hp.ordered_mean(r)[away], hp.ordered_mean(vol)[away], _min(mj)[away])


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_every_refusal_of_the_twin(mesh, cells):
    conn, g, _ = cells
    conn, g = conn[:5], g[:5]
    x, d = _history(mesh, 8, 4), _displacements(mesh, 8)
    s, geo = _session(x), _session(d)
    with pytest.raises(RuntimeError, match=r"cell_rate_current: no cell list \(cells first\)"):
        s.cell_rate_current("raw", geo)
    s.cells(conn, g)
    before = s.cell_rate("raw")
    with pytest.raises(RuntimeError, match="series must be one of raw, series, phase_mean"):
        s.cell_rate_current("filtered", geo)
    with pytest.raises(RuntimeError, match=r"no filtered series \(filter or phase first\)"):
        s.cell_rate_current("series", geo)
    with pytest.raises(RuntimeError, match=r"no phase average \(phase first\)"):
        s.cell_rate_current("phase_mean", geo)
    for first, step, count in ((0, 0, 1), (0, 1, 0), (0, -1, 2), (0, 1, -2)):
        with pytest.raises(RuntimeError, match="needs step >= 1 and count >= 1"):
            s.cell_rate_current("raw", geo, first, step, count)
    for first, step, count in ((8, 1, 1), (-1, 1, 1), (0, 1, 9), (1, 4, 3), (7, 1, 2)):
        with pytest.raises(RuntimeError, match="fall outside the series of 8 frames"):
            s.cell_rate_current("raw", geo, first, step, count)
    # the session of d: none, other nodes, other frames
    for none in (None, hp.HostBandSession(3, 8), _session(d[:, :, :1], 1)):
        with pytest.raises(RuntimeError, match="no session of d"):
            s.cell_rate_current("raw", none)
    with pytest.raises(RuntimeError, match=f"the session of d is on {mesh.num_nodes - 1} nodes, the session of the quantity on {mesh.num_nodes}"):
        s.cell_rate_current("raw", _session(d[:, :-1]))
    with pytest.raises(RuntimeError, match="the session of d has recorded 7 frames, the session of the quantity 8"):
        s.cell_rate_current("raw", _session(d[:7]))
    # the phase mean: none, another period, another selection
    s.phase(4)
    with pytest.raises(RuntimeError, match=r"the session of d has no phase average \(phase of d first\)"):
        s.cell_rate_current("phase_mean", geo)
    geo.phase(2)
    with pytest.raises(RuntimeError, match="the phase average of d has a period of 2 frames, that of the quantity 4"):
        s.cell_rate_current("phase_mean", geo)
    geo.select(4, 4, 1)
    geo.phase(4)
    with pytest.raises(RuntimeError, match="the phase average of d is over another selection of frames"):
        s.cell_rate_current("phase_mean", geo)
    assert all(a.shape == (5,) for a in s.cell_rate_current("series", geo))           # raw d frames: d's selection does not matter
    geo.select(0, 8, 1)
    geo.phase(4)
    assert all(a.shape == (5,) for a in s.cell_rate_current("phase_mean", geo, 3))
    assert np.array_equal(s.cell_rate("raw"), before)                                 # the refused calls changed nothing
    s.end()
    with pytest.raises(RuntimeError, match="no cell list"):
        s.cell_rate_current("raw", geo)


def test_the_option_and_its_refusals(mesh, tmp_path):
    from vasp_amd import postprocess
    from vasp_amd.monolithic import add_session_arguments
    ap = argparse.ArgumentParser()
    add_session_arguments(ap)
    key = "hi_pass_flow_metrics_configuration"
    assert vars(ap.parse_args([]))[key] is None and fm.configuration({}) == "reference" and fm.configuration({key: None}) == "reference"
    assert vars(ap.parse_args(["--hi-pass-flow-metrics-configuration", "current"]))[key] == "current"
    with pytest.raises(SystemExit):
        ap.parse_args(["--hi-pass-flow-metrics-configuration", "deformed"])
    assert postprocess.parse(["--folder", "x", "--hi-pass", "d", "v", *CURRENT])[key] == "current"
    deg2 = ["--save-deg", "2"]
    for q in (["d", "v"], ["v", "d"], ["d", "v", "p"]):
        assert hp.hi_pass_refusal(_parameters(["--hi-pass", *q, *deg2, *CURRENT, *PHASE]), 1, None) == ""
    reference = ["--hi-pass-flow-metrics", "--hi-pass-flow-metrics-configuration", "reference"]
    assert hp.hi_pass_refusal(_parameters(["--hi-pass", "v", *deg2, *reference, *PHASE]), 1, None) == ""
    why = hp.hi_pass_refusal(_parameters(["--hi-pass", "v", "p", *deg2, *CURRENT, *PHASE]), 1, None)
    assert why == fm.NEEDS_D and "needs d among the --hi-pass quantities" in why and "\n" not in why
    assert hp.hi_pass_refusal(_parameters(["--hi-pass", "d", "p", *deg2, *CURRENT, *PHASE]), 1, None) == fm.NEEDS_V      # as before
    assert hp.hi_pass_refusal(_parameters(["--hi-pass", "d", "v", *CURRENT, *PHASE]), 1, None) == fm.NEEDS_DEG2
    for word in ("current", "reference"):                                             # the option without --hi-pass-flow-metrics
        why = hp.hi_pass_refusal(_parameters(["--hi-pass", "d", "v", *deg2, "--hi-pass-flow-metrics-configuration", word, *PHASE]), 1, None)
        assert why == fm.NEEDS_METRICS and "it needs that option" in why and "\n" not in why
    # strips of rows stay refused
    ns = dict(_parameters(["--hi-pass", "d", "v", *deg2, *CURRENT]), save_deg=2, results_folder=tmp_path, hi_pass_strip=(0, 8))
    with pytest.raises(SystemExit) as e:
        hp.HiPassRun(object(), mesh, ns)
    assert str(e.value) == hp.METRICS_STRIPS and not (tmp_path / "FlowMetrics").exists()


# ---- the driver with a stub backend ------------------------------------------------------------------------------------------

def expected_current(mesh, ns_like, x, d, period, grad=None):
    """The metrics of velocity frames x and displacement frames d in the current configuration, by the closing formulas on
    the twin's rates; ``grad``: the gradients to use (default: the host's own).  Returns (cells, metrics, volume weights)."""
    cells = fm.fluid_cells(mesh, ns_like["dx_f_id"])
    grad = fm.barycentric_gradients(mesh, cells) if grad is None else grad
    nu, h = fm.kinematic_viscosity(mesh, cells, ns_like), fm.cell_diameters(mesh, cells)
    s, geo = _session(x), _session(d)
    s.cells(mesh.tet_nodes[cells], grad)
    raw, volume_ratio, min_jacobian = s.cell_rate_current("raw", geo)
    out = fm.strain_metrics(raw, nu, h, float(ns_like["dt"]))
    out.update(volume_ratio=volume_ratio, min_jacobian=min_jacobian)
    if period:
        n = len(x) // period * period
        for a in (s, geo):
            a.select(0, n, 1)
            a.phase(period)
        out.update(fm.turbulence_metrics(s.cell_rate_current("series", geo)[0], s.cell_rate_current("phase_mean", geo)[0], nu, h, float(ns_like["dt"])))
        out["turbulent_dissipation_phase_mean"] = nu[None] * np.stack([s.cell_rate_current("series", geo, j, period, n // period)[0] for j in range(period)])
    with np.errstate(all="ignore"):
        return cells, out, fm.cell_volumes(mesh, cells) * volume_ratio


def _displacement(results):
    return _vectors(results / "Visualization" / "displacement.h5")


def _tree(folder):
    return {str(p.relative_to(folder)): p.read_bytes() for p in sorted(folder.rglob("*")) if p.is_file()}


def test_driver_writes_the_current_configuration_metrics(tmp_path, mesh):
    """14 saved frames, ``--hi-pass v d``: d is processed before v, the files are the closing formulas on the twin's
    current-configuration rates, the table has the two new rows and volume weights ``volume * volume_ratio``."""
    from test_hi_pass_cell_rate import PHASE_NAMES
    ns, lines = _run(tmp_path / "cur" / "case", T="0.0135", options=["--hi-pass", "v", "d", *CURRENT, *PHASE])
    results = tmp_path / "cur" / "case" / "1"
    out = results / "FlowMetrics"
    x, d = _velocity(results), _displacement(results)
    assert x.shape == d.shape == (14, mesh.num_nodes, 3)
    cells, want, weights = expected_current(mesh, ns, x, d, 4)
    names = ("strain_rate", "dissipation", "l_plus", "t_plus", "volume_ratio", "min_jacobian", *PHASE_NAMES)
    assert {p.name for p in out.iterdir()} == {f"{n}.{e}" for n in names for e in ("h5", "xdmf")} | {"flow_metrics.csv"}
    for name in names:
        got = _vectors(out / f"{name}.h5")
        assert got.shape == (4 if name.endswith("phase_mean") else 1, len(cells), 1) and got.dtype == np.float32, name
        with np.errstate(all="ignore"):
            assert np.array_equal(got[:, :, 0], np.atleast_2d(want[name]).astype(np.float32), equal_nan=True), name
    table = (out / "flow_metrics.csv").read_text().splitlines()
    assert table[0] == fm.CSV_HEADER and len(table) == 1 + 13 + 4
    rows = {r.split(", ")[0]: r.split(", ")[1:] for r in table[1:]}
    assert list(rows)[:6] == ["strain_rate", "dissipation", "l_plus", "t_plus", "volume_ratio", "min_jacobian"]
    for name in ("volume_ratio", "min_jacobian", "l_plus"):
        mean, lo, hi, cell = fm.summary_row(want[name], weights, cells)
        assert [float(a) for a in rows[name][:3]] == pytest.approx([mean, lo, hi], rel=0, abs=0, nan_ok=True) and int(rows[name][3]) == cell
    line = [l for l in lines if l.startswith("Flow metrics of")]
    assert len(line) == 1 and "in the current configuration" in line[0] and "volume_ratio, min_jacobian" in line[0]
    # d before v, whatever the order given; every quantity's own lines and files as in a run without the metrics
    said = [l for l in lines if "phase average over cycles" in l]
    assert [l.split()[1].rstrip(":") for l in said] == ["displacement", "velocity"]
    _run(tmp_path / "plain" / "case", T="0.0135", options=["--hi-pass", "v", "d", *PHASE])
    assert _tree(results / "Visualization_hi_pass") == _tree(tmp_path / "plain" / "case" / "1" / "Visualization_hi_pass")


def test_reference_is_a_run_without_the_new_option(tmp_path):
    base = ["--hi-pass", "v", "d", "--hi-pass-flow-metrics", *PHASE]
    _, old = _run(tmp_path / "old" / "case", T="0.0135", options=base)
    _, new = _run(tmp_path / "new" / "case", T="0.0135", options=[*base, "--hi-pass-flow-metrics-configuration", "reference"])
    for sub in ("FlowMetrics", "Visualization_hi_pass"):
        a, b = _tree(tmp_path / "old" / "case" / "1" / sub), _tree(tmp_path / "new" / "case" / "1" / sub)
        assert a == b and len(a) > 4, sub
    assert not any(n.startswith(("volume_ratio", "min_jacobian")) for n in _tree(tmp_path / "new" / "case" / "1" / "FlowMetrics"))
    strip = lambda lines: [l.replace(str(tmp_path / "old"), "").replace(str(tmp_path / "new"), "") for l in lines]
    assert strip(old) == strip(new) and any("in the reference configuration" in l for l in new)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------

def test_header_binding_and_kernel_source_agree():
    import re
    from vasp_amd import capi
    header = (ROOT / "include" / "vaspfsi.h").read_text()
    lib = capi.load_library()
    name = "fsi_band_cell_rate_current"
    m = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S)
    assert m and name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")) == 9
    assert "Replaces: nothing in the reference; VaMPy's metrics on an FSI run" in header[:m.start()].rsplit("/*", 1)[1]
    assert hasattr(capi.HipBackend, "hi_pass_cell_rate_current")
    assert re.search(r"^int %s\(FsiCtx\* ctx" % name, (ROOT / "vasp_amd" / "csrc" / "fsi_sessions.hip").read_text(), flags=re.M)
    src = (ROOT / "vasp_amd" / "csrc" / "fsi_rate.hip").read_text()
    assert "#pragma clang fp contract(off)" in src and "__launch_bounds__(256) void k_cell_rate_current" in src
    assert src.index("#pragma clang fp contract(off)") < src.index("k_cell_rate_current(int64_t n")
    assert "__shared__" not in src and "0.5854101966249685" in src and "0.1381966011250105" in src
    hpp = (ROOT / "vasp_amd" / "csrc" / "fsi_rate.hpp").read_text()
    assert "launch_cell_rate_current" in hpp and re.search(r"k_cell_rate_current: \d+ VGPRs, \d+ AGPRs, \d+ SGPRs, no scratch", hpp)
