"""Q-criterion, enstrophy, helicity and kinetic energy of a recorded history on mesh cells and ``--hi-pass-vortex``, host side:
the NumPy twin of csrc/fsi_vortex.hip (``hi_pass.cell_vortex``, ``hi_pass.cell_wsum``, ``HostBandSession.cell_weights`` /
``cell_vortex``) against an independent restatement in extended precision, against the degree-6 quadrature rule and against
known answers; the bracket of the ordered sum; the closing formulas of vasp_amd/vortex.py, the option with its refusals and the
driver's files with a stub backend.

The per-cell bound of a field: ``C * 2^-53 * B_c`` with ``C = 70`` and ``B_c`` the twin's formula with the absolute value of every
term (``bounds``).  The roundings on the longest path of any term, to first order:

* a gradient entry is a sum of ten terms, each a product of up to three rounded factors, added in ten additions: 13;
* Q: a product of two entries (2 * 13 + 1 = 27) goes through the 36 additions of the vertex sum, the closing addition and the
  two multiplications by 0.05 (itself rounded) and -0.5: 27 + 36 + 3 = 66.  The other half, (sum_t G)(sum_t G), has
  2 * (13 + 4) + 1 + 9 + 3 = 47;
* enstrophy: omega is a difference of two entries (14), its square 29, twelve additions and the closing three: 44;
* helicity: u = sum_a M w has 1 (M = k / 60 is rounded) + 1 + 10 = 12, omega 14, their product 27, twelve additions: 39.  The
  absolute value adds none, and | |a| - |b| | <= |a - b|;
* speed2: u = sum_b MM w has 12, w u 13, thirty additions: 43.

66 is the largest; 70 leaves the second-order terms their room.  Q and the helicity cancel, so their B_c is far above their
value, and the share of the bound that is used is printed."""
import argparse
import contextlib
import io
import itertools
import math

import numpy as np
import pytest

from test_hi_pass_cell_rate import bound as rate_bound
from test_session_restart import CYL, SPLIT, _restart, _run, one_modification_time  # noqa: F401  (the fixture holds h5lite's clock)
from vasp_amd import flow_metrics as fm
from vasp_amd import hi_pass as hp
from vasp_amd import vortex as vx
from vasp_amd.mesh import TET_EDGES, FsiMesh
from vasp_amd.quadrature import tabulate_tet, tet_rule_deg6

EPS = 2.0 ** -53
LD = np.longdouble
C = 70
PHASE = ["--hi-pass-phase-average", "--hi-pass-cycle", "0.004"]
VORTEX = ["--hi-pass-vortex"]
SERIES = ["--hi-pass-vortex", "--hi-pass-vortex-series"]
MEAN_FILES = ("q_criterion_avg", "vorticity_rms", "helicity_avg", "helicity_intensity", "helicity_balance", "kinetic_energy_avg")
PHASE_FILES = ("q_criterion_phase_mean", "vorticity_rms_fluctuation")
TABLES = {"vortex.csv", "vortex_summary.csv", "helicity_indices.csv"}


@pytest.fixture(scope="module")
def mesh():
    return FsiMesh.read(CYL)


def _random_tets(n, seed):
    """(nodes (n, 10, 3), grad (n, 4, 3)) of random tetrahedra of very different sizes and shapes."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 4, 3)) * rng.uniform(1e-3, 10.0, (n, 1, 1))
    J = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=1)
    keep = np.abs(np.linalg.det(J)) > 1e-3 * np.linalg.norm(J, axis=(1, 2)) ** 3
    X, J = X[keep], J[keep]
    g = np.empty((len(X), 4, 3))
    g[:, 1:] = np.linalg.inv(J).transpose(0, 2, 1)
    g[:, 0] = -((g[:, 1] + g[:, 2]) + g[:, 3])
    nodes = np.concatenate([X, np.stack([0.5 * (X[:, p] + X[:, r]) for p, r in TET_EDGES], axis=1)], axis=1)
    return nodes, g


@pytest.fixture(scope="module")
def cells(mesh):
    """(nodes (n, 10, 3), grad (n, 4, 3)): 300 random cells of the cylinder fixture, then random tetrahedra."""
    c = np.sort(np.random.default_rng(0).permutation(mesh.num_cells)[:300])
    nodes, g = _random_tets(300, 1)
    assert len(nodes) > 200
    return np.concatenate([mesh.node_coords[mesh.tet_nodes[c]], nodes]), np.concatenate([fm.barycentric_gradients(mesh, c), g])


def _fields(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 10, 3)) * rng.uniform(0.1, 10.0, (n, 1, 1)) + rng.standard_normal((n, 1, 3))


def bounds(w, g):
    """(5, n): B_c of every field - ``hi_pass.cell_vortex`` with the absolute value of every term."""
    w, g = np.abs(np.asarray(w, dtype=np.float64)), np.abs(np.asarray(g, dtype=np.float64))
    n = len(w)
    M, MM = np.abs(hp.VORTEX_M), np.abs(hp.VORTEX_MM)
    qd, ed, h = np.zeros(n), np.zeros(n), np.zeros(n)
    T = [[np.zeros(n) for _ in range(3)] for _ in range(3)]
    for t in range(4):
        G = [[None] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(3):
                s = np.zeros(n)
                for a in range(4):
                    s = s + w[:, a, i] * ((3.0 if a == t else 1.0) * g[:, a, j])
                for e in range(6):
                    p, r = TET_EDGES[e]
                    s = s + (w[:, 4 + e, i] * 4.0) * ((1.0 if p == t else 0.0) * g[:, r, j] + (1.0 if r == t else 0.0) * g[:, p, j])
                G[i][j] = s
        for i in range(3):
            for j in range(3):
                qd = qd + G[i][j] * G[j][i]
                T[i][j] = T[i][j] + G[i][j]
        om = [G[2][1] + G[1][2], G[0][2] + G[2][0], G[1][0] + G[0][1]]
        for i in range(3):
            ed = ed + om[i] * om[i]
            h = h + sum(M[a][t] * w[:, a, i] for a in range(10)) * om[i]
    qp = sum(T[i][j] * T[j][i] for i in range(3) for j in range(3))
    W = [T[2][1] + T[1][2], T[0][2] + T[2][0], T[1][0] + T[0][1]]
    ep = sum(W[i] * W[i] for i in range(3))
    s2 = sum(w[:, a, i] * sum(MM[a][b] * w[:, b, i] for b in range(10)) for i in range(3) for a in range(10))
    return np.stack([0.5 * (0.05 * (qd + qp)), 0.05 * (ed + ep), h, h, s2])


def _rational_tables():
    M, MM = hp.vortex_tables()
    return M.astype(LD) / LD(60), MM.astype(LD) / LD(420)


def restated(w, g):
    """(5, n) in ``np.longdouble``, by another route: the P2 basis gradients at the four vertices of the reference cell
    (``tabulate_tet``) mapped by the gradients of the barycentric coordinates 1 .. 3, tensor contractions for the means, and the
    tables as quotients of integers in extended precision."""
    w, g = np.asarray(w).astype(LD), np.asarray(g).astype(LD)
    dN = tabulate_tet(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))[1].astype(LD)      # (4, 10, 3)
    G = np.einsum("cai,takcj->ctij", w, np.einsum("tak,ckj->takcj", dN, g[:, 1:4]))
    mean = lambda f, h: (np.einsum("ct...,ct...->c...", f, h) + f.sum(axis=1) * h.sum(axis=1)) / LD(20)
    om = np.stack([G[..., 2, 1] - G[..., 1, 2], G[..., 0, 2] - G[..., 2, 0], G[..., 1, 0] - G[..., 0, 1]], axis=-1)
    M, MM = _rational_tables()
    hel = np.einsum("at,cai,cti->c", M, w, om)
    return np.stack([-mean(G, G.transpose(0, 1, 3, 2)).sum(axis=(1, 2)) / LD(2), mean(om, om).sum(axis=1), hel, np.abs(hel),
                     np.einsum("ab,cai,cbi->c", MM, w, w)])


def by_quadrature(w, g, absolute=False):
    """(5, n) in ``np.longdouble`` by the degree-6 rule on 24 points: the integrands are the velocity and its gradient at the
    points (``tabulate_tet``), no vertex value and no table is used.  ``absolute``: the same 24-point sums with the absolute
    value of every term - what the rule's own rounding is measured against."""
    qp, qw = tet_rule_deg6()
    N, dN = (a.astype(LD) for a in tabulate_tet(qp)[:2])
    w, g, qw = np.asarray(w).astype(LD), np.asarray(g).astype(LD), (qw / qw.sum()).astype(LD)
    if absolute:
        N, dN, w, g = np.abs(N), np.abs(dN), np.abs(w), np.abs(g)
    v = np.einsum("qa,cai->cqi", N, w)
    G = np.einsum("cai,cqaj->cqij", w, np.einsum("qak,ckj->cqaj", dN, g[:, 1:4]))
    sign = LD(1) if absolute else LD(-1)
    om = np.stack([G[..., 2, 1] + sign * G[..., 1, 2], G[..., 0, 2] + sign * G[..., 2, 0], G[..., 1, 0] + sign * G[..., 0, 1]], axis=-1)
    hel = np.einsum("q,cqi,cqi->c", qw, v, om)
    return np.stack([np.einsum("q,cqij,cqji->c", qw, G, G) / LD(2) * sign, np.einsum("q,cqi,cqi->c", qw, om, om), hel, np.abs(hel),
                     np.einsum("q,cqi,cqi->c", qw, v, v)])


def _share(err, limit):
    return {name: float((err[f] / limit[f]).max()) for f, name in enumerate(hp.VORTEX_FIELDS)}


def test_twin_against_the_extended_precision_restatement(cells):
    """Largest err / (C 2^-53 B_c) observed: 0.009 (Q), 0.009 (enstrophy), 0.006 (helicity), 0.036 (speed2)."""
    nodes, g = cells
    w = _fields(len(nodes), 2)
    got, B = hp.cell_vortex(w, g), bounds(w, g)
    assert got.shape == (5, len(nodes)) and got.dtype == np.float64
    err = np.abs(got.astype(LD) - restated(w, g)).astype(np.float64)
    print("twin against the restatement, share of the bound used:", _share(err, C * EPS * B))
    assert (err <= C * EPS * B).all()
    assert (got[1] > 0).all() and (got[4] > 0).all() and np.array_equal(got[3], np.abs(got[2])) and (got[0] < 0).any() and (got[0] > 0).any()
    assert np.median(np.abs(got[0]) / B[0]) < 0.5                                          # Q cancels: the bound is on the terms


def test_the_closed_forms_are_exact_against_the_quadrature_rule(cells):
    """The bound is that of the twin plus the same count and the 24 additions for the rule's own sum, on the rule's absolute
    terms: ``C 2^-53 B_c + (C + 24) 2^-53 Bq_c``.  Largest share of it observed: 0.009, 0.009, 0.007 and 0.023."""
    nodes, g = cells
    w = _fields(len(nodes), 3)
    got = hp.cell_vortex(w, g)
    limit = C * EPS * bounds(w, g) + (C + 24) * EPS * by_quadrature(w, g, absolute=True).astype(np.float64)
    err = np.abs(got.astype(LD) - by_quadrature(w, g)).astype(np.float64)
    print("twin against the quadrature, share of the bound used:", _share(err, limit))
    assert (err <= limit).all()
    # the P1 interpolant of the same vertices is another field: the edge nodes matter, far beyond the bound
    flat = w.copy()
    flat[:, 4:] = np.stack([0.5 * (w[:, p] + w[:, r]) for p, r in TET_EDGES], axis=1)
    assert (np.abs(hp.cell_vortex(flat, g) - got)[[0, 1, 2, 4]] > 1e6 * limit[[0, 1, 2, 4]]).mean() > 0.9


def _within(got, want, B, what):
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    print(what, "share of the bound used:", float((err / (C * EPS * B)).max()))
    assert (err <= C * EPS * B).all(), what


def test_known_answers(cells):
    nodes, g = cells
    n = len(nodes)
    x = nodes.astype(LD)
    om = np.array([0.3, -1.1, 0.7])
    o2 = (om.astype(LD) ** 2).sum()
    # rigid rotation v = Omega x X: Q = |Omega|^2, enstrophy 4 |Omega|^2, helicity 0
    w = np.cross(om, nodes)
    got, B = hp.cell_vortex(w, g), bounds(w, g)
    _within(got[0], o2, B[0], "rotation, Q")
    _within(got[1], 4 * o2, B[1], "rotation, enstrophy")
    _within(got[2], LD(0), B[2], "rotation, helicity")
    # screw motion v = Omega x X + c Omega: helicity 2 c |Omega|^2
    c = 0.37
    w = np.cross(om, nodes) + c * om
    got, B = hp.cell_vortex(w, g), bounds(w, g)
    _within(got[2], 2 * LD(c) * o2, B[2], "screw, helicity")
    _within(got[3], 2 * LD(c) * o2, B[3], "screw, |helicity|")
    _within(got[0], o2, B[0], "screw, Q")
    # symmetric traceless v = A x: Q = -0.5 A:A, no vorticity; simple shear v = (k y, 0, 0): Q = 0, enstrophy k^2
    A = np.array([[1.0, 0.4, -0.3], [0.4, -2.5, 0.8], [-0.3, 0.8, 1.5]])
    w = nodes @ A.T
    got, B = hp.cell_vortex(w, g), bounds(w, g)
    _within(got[0], -(A.astype(LD) ** 2).sum() / 2, B[0], "strain, Q")
    _within(got[1], LD(0), B[1], "strain, enstrophy")
    _within(got[2], LD(0), B[2], "strain, helicity")
    w = np.zeros((n, 10, 3))
    w[:, :, 0] = 1.7 * nodes[:, :, 1]
    got, B = hp.cell_vortex(w, g), bounds(w, g)
    _within(got[0], LD(0), B[0], "shear, Q")
    _within(got[1], LD(1.7) ** 2, B[1], "shear, enstrophy")
    # a quadratic field v = (0, c, x^2 / 2): omega = (0, -x, 0), so Q = 0, enstrophy mean(x^2), helicity -c mean(x) and
    # |v|^2 = c^2 + mean(x^4) / 4.  The mean over a tetrahedron of the k-th power of a linear function with vertex values x_t is
    # 6 k! / (k + 3)! times the complete homogeneous symmetric polynomial h_k(x_0 .. x_3)
    w = np.zeros((n, 10, 3))
    w[:, :, 1] = c
    w[:, :, 2] = 0.5 * nodes[:, :, 0] ** 2
    xv = x[:, :4, 0]
    hk = lambda k: sum(np.prod(xv[:, list(idx)], axis=1) for idx in itertools.combinations_with_replacement(range(4), k))
    got, B = hp.cell_vortex(w, g), bounds(w, g)
    _within(got[0], LD(0), B[0], "quadratic, Q")
    _within(got[1], hk(2) / 10, B[1], "quadratic, enstrophy")
    _within(got[2], -LD(c) * xv.sum(axis=1) / 4, B[2], "quadratic, helicity")
    _within(got[4], LD(c) ** 2 + hk(4) / 35 / 4, B[4], "quadratic, speed2")
    assert (got[1] > 0).all() and (np.abs(got[2]) > 0).all()
    # nothing is clamped; shapes are checked
    w[3, 7, 1] = np.nan
    got = hp.cell_vortex(w, g)
    assert np.isnan(got[:, 3]).all() and np.isfinite(np.delete(got, 3, axis=1)).all()
    zero = hp.cell_vortex(np.zeros((n, 10, 3)), g)
    assert not zero[1:].any() and not np.signbit(zero[1:]).any() and not zero[0].any()
    with pytest.raises(RuntimeError, match="expected"):
        hp.cell_vortex(w[:, :4], g)


def test_q_is_a_quarter_of_the_enstrophy_less_a_quarter_of_the_strain_rate(cells):
    """``Q = 0.25 * enstrophy - 0.25 * cell_rate`` (``cell_rate`` is the mean of 2 S:S), within the sum of the three bounds: C for
    Q and the enstrophy, the 80 of tests/test_hi_pass_cell_rate.py for the rate."""
    nodes, g = cells
    w = _fields(len(nodes), 4)
    got, B = hp.cell_vortex(w, g), bounds(w, g)
    rate = hp.cell_rate(w, g)
    limit = EPS * (C * B[0] + 0.25 * C * B[1] + 0.25 * 80 * rate_bound(w, g)) + 2 * EPS * (0.25 * got[1] + 0.25 * rate)
    err = np.abs(got[0].astype(LD) - (LD(0.25) * got[1].astype(LD) - LD(0.25) * rate.astype(LD))).astype(np.float64)
    print("Q identity, share of the bound used:", float((err / limit).max()))
    assert (err <= limit).all()


def test_the_localised_normalised_helicity_stays_in_its_range(cells):
    """|lnh| <= 1 by Cauchy-Schwarz.  On random fields a few ulp over 1 would show; on a screw motion that is almost a
    translation along Omega lnh is 1 to rounding: there the three means carry 39, 43 and 44 roundings with factors of |M|, |MM|
    over their sums of at most 21 / 15 and 212 / 28, the root halves the last two and three more operations close: 128 covers
    it."""
    nodes, g = cells
    lnh = vx.frame_fields(hp.cell_vortex(_fields(len(nodes), 5), g))["lnh"]
    assert (np.abs(lnh) <= 1.0 + 4 * EPS).all() and np.abs(lnh).max() > 0.05
    om = np.array([0.3, -1.1, 0.7])
    for c in (1e6, 1e9):
        lnh = vx.frame_fields(hp.cell_vortex(np.cross(om, nodes) + c * om, g))["lnh"]
        print("screw motion, c =", c, ": largest lnh - 1 in units of 2^-53:", float((lnh - 1.0).max() / EPS))
        assert (lnh <= 1.0 + 128 * EPS).all() and (lnh > 0.999).all()
    assert np.array_equal(vx.frame_fields(np.zeros((5, 3)))["lnh"], np.zeros(3))             # 0 where the product is 0
    assert np.isnan(vx.frame_fields(np.full((5, 2), np.nan))["lnh"]).all()


# ---- the ordered sum -------------------------------------------------------------------------------------------------------

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
BIG = 2.0 ** 60                                     # BIG + 1 == BIG: a 1 added to it is lost, a 1 added after it cancelled stays


def _tree(p):
    """The bracket written out on Python floats: per 256 a balanced tree in each 64, the four in order, the groups in order."""
    p = list(p) + [0.0] * (-len(p) % 256)
    def pairs(x):
        return x[0] if len(x) == 1 else pairs([x[i] + x[i + 1] for i in range(0, len(x), 2)])
    total = 0.0
    for b in range(0, len(p), 256):
        s = [pairs(p[b + 64 * k:b + 64 * k + 64]) for k in range(4)]
        total = total + (((s[0] + s[1]) + s[2]) + s[3])
    return total


@pytest.mark.parametrize("n", SIZES)
def test_the_ordered_sum_is_accurate_and_is_the_written_out_bracket(n):
    rng = np.random.default_rng(n)
    values, weights = rng.standard_normal((3, n)) * 10.0 ** rng.uniform(-3, 3, (3, n)), rng.uniform(0.1, 2.0, n)
    got = hp.cell_wsum(values, weights)
    assert got.shape == (3,) and got.dtype == np.float64
    groups = (n + 255) // 256
    for row, s in zip(values, got):
        p = weights * row
        assert abs(s - math.fsum(p)) <= (9 + groups) * EPS * math.fsum(np.abs(p))        # six levels, three wave additions, the groups
        assert s == _tree(p) and s == hp.cell_wsum(row, weights)
    with pytest.raises(RuntimeError, match="expected"):
        hp.cell_wsum(values, weights[:-1] if n > 1 else np.ones(2))


def _placed(n, at):
    x = np.zeros(n)
    for k, v in at.items():
        x[k] = v
    return x


@pytest.mark.parametrize("n", SIZES)
def test_the_bracket_of_the_ordered_sum_by_hand(n):
    """Cases in which a serial sum, a flat pairwise sum and the bracket of k_cell_wsum give different doubles, worked by hand."""
    one = np.ones(n)
    assert hp.cell_wsum(_placed(n, {0: 3.0}), 0.5 * one) == 1.5
    minus = hp.cell_wsum(np.full(n, -0.0), one)
    assert minus == 0.0 and not np.signbit(minus)                                          # the groups are added from +0.0
    if n >= 63:
        # across pair boundaries inside a wave: (BIG + 1) + (-BIG + 1) = 0, where the serial sum keeps the last 1
        x = _placed(n, {0: BIG, 1: 1.0, 2: -BIG, 3: 1.0})
        assert hp.cell_wsum(x, one) == 0.0 and float(np.cumsum(x)[-1]) == 1.0
        # shifted by one the pairs are (., BIG), (1, -BIG), (1, .): BIG + -BIG, then + 1
        assert hp.cell_wsum(_placed(n, {1: BIG, 2: 1.0, 3: -BIG, 4: 1.0}), one) == 1.0
        # a level up: (1 + 1) + (BIG + -BIG) = 2; serial: ((1 + 1) + BIG) + -BIG = 0
        x = _placed(n, {0: 1.0, 1: 1.0, 2: BIG, 3: -BIG})
        assert hp.cell_wsum(x, one) == 2.0 and float(np.cumsum(x)[-1]) == 0.0
    if n >= 255:
        # across the wave boundaries: the four wave sums 1, BIG, -BIG, 1 in wave order give ((1 + BIG) - BIG) + 1 = 1; a balanced
        # tree over the waves, (1 + BIG) + (-BIG + 1), would give 0
        assert hp.cell_wsum(_placed(n, {5: 1.0, 70: BIG, 130: -BIG, 200: 1.0}), one) == 1.0
        # 63 | 64: the pair (62, 63) closes wave 0 with 1 + BIG = BIG, wave 1 opens with (-BIG + 1) = -BIG: 0; serial: 1
        x = _placed(n, {62: 1.0, 63: BIG, 64: -BIG, 65: 1.0})
        assert hp.cell_wsum(x, one) == 0.0 and float(np.cumsum(x)[-1]) == 1.0
        # a flat pairwise sum over n values halves n, not 256: its first split of 255 is at 127, and 1 | BIG there differs
        assert hp.cell_wsum(_placed(n, {126: 1.0, 127: BIG, 128: -BIG, 129: 1.0}), one) == 0.0      # (126, 127) and (128, 129) are pairs
    if n >= 257:
        # across the workgroup boundary: (254, 255) is the last pair of group 0, so group 0 = 1 + BIG = BIG and the 1 is lost;
        # group 1 = -BIG; the groups from +0.0 in ascending order: (0 + BIG) + -BIG = 0
        x = _placed(n, {254: 1.0, 255: BIG, 256: -BIG})
        assert hp.cell_wsum(x, one) == 0.0
        # group 0 = BIG, group 1 = 1: (0 + BIG) + 1 = BIG
        x = _placed(n, {255: BIG, 256: 1.0})
        assert hp.cell_wsum(x, one) == BIG
    if n >= 513:
        # three groups 1, BIG, -BIG: ascending ((0 + 1) + BIG) + -BIG = 0; descending would keep the 1
        assert hp.cell_wsum(_placed(n, {3: 1.0, 300: BIG, 512: -BIG}), one) == 0.0
        assert hp.cell_wsum(_placed(n, {3: BIG, 300: -BIG, 512: 1.0}), one) == 1.0
    # a weight is applied before anything is added, in one rounding
    w = np.full(n, 1.0 / 3.0)
    assert hp.cell_wsum(_placed(n, {0: 3.0, n - 1: 0.1 if n > 1 else 3.0}), w) == _tree(w * _placed(n, {0: 3.0, n - 1: 0.1 if n > 1 else 3.0}))


# ---- the twin sessions -------------------------------------------------------------------------------------------------------

def _history(mesh, frames, seed=6):
    return np.random.default_rng(seed).standard_normal((frames, mesh.num_nodes, 3))


def test_session_twin_orders_frames_and_refuses_what_the_device_refuses(mesh):
    c = np.arange(40)
    conn, g = mesh.tet_nodes[c], fm.barycentric_gradients(mesh, c)
    x = _history(mesh, 8)
    s = hp.HostBandSession(3, 8)
    s.import_(x)
    with pytest.raises(RuntimeError, match=r"hi-pass cell_vortex: no cell list \(cells first\)"):
        s.cell_vortex("raw")
    with pytest.raises(RuntimeError, match=r"hi-pass cell_weights: no cell list \(cells first\)"):
        s.cell_weights(np.ones(40))
    s.cells(conn, g)
    r = np.stack([hp.cell_vortex(x[k][conn], g) for k in range(8)])
    got, sums = s.cell_vortex("raw", 3, 1, 1)
    assert np.array_equal(got, r[3]) and sums is None                                       # one frame: its own bits
    assert np.array_equal(s.cell_vortex("raw")[0], hp.ordered_mean(r))
    assert np.array_equal(s.cell_vortex("raw", 1, 3, 3)[0], (((0.0 + r[1]) + r[4]) + r[7]) / 3.0)
    assert np.array_equal(s.cell_vortex("raw")[0][3], hp.ordered_mean(np.abs(r[:, 2])))     # the mean of |cell mean|, frame by frame
    with pytest.raises(RuntimeError, match=r"hi-pass cell_vortex: sums without weights \(cell_weights first\)"):
        s.cell_vortex("raw", sums=True)
    with pytest.raises(RuntimeError, match="neither cells nor sums"):
        s.cell_vortex("raw", cells=False)
    with pytest.raises(ValueError, match="39 weights, the session has 40 cells"):
        s.cell_weights(np.ones(39))
    wt = np.random.default_rng(7).uniform(0.5, 2.0, 40)
    s.cell_weights(wt)
    none, sums = s.cell_vortex("raw", 2, 1, 1, False, True)
    assert none is None and np.array_equal(sums, hp.cell_wsum(r[2], wt))
    both = s.cell_vortex("raw", cells=True, sums=True)
    assert np.array_equal(both[1], hp.cell_wsum(both[0], wt))
    for series, why in (("filtered", "series must be one of raw, series, phase_mean"), ("series", r"no filtered series \(filter or phase first\)"),
                        ("phase_mean", r"no phase average \(phase first\)")):
        with pytest.raises(RuntimeError, match="hi-pass cell_vortex: " + why):
            s.cell_vortex(series)
    with pytest.raises(RuntimeError, match="needs step >= 1 and count >= 1, got step = 0, count = 1"):
        s.cell_vortex("raw", 0, 0, 1)
    with pytest.raises(RuntimeError, match=r"frames 7, 7 \+ 1, ... \(2 of them\) fall outside the series of 8 frames"):
        s.cell_vortex("raw", 7, 1, 2)
    s.phase(4)
    assert np.array_equal(s.cell_vortex("phase_mean", 1, 1, 1)[0], hp.cell_vortex(s.phase_fetch("mean", 1)[conn], g))
    assert s.cell_vortex("series")[0].shape == (5, 40)
    s.cells(conn[:7], g[:7])                                                                # a new list drops the weights
    with pytest.raises(RuntimeError, match="sums without weights"):
        s.cell_vortex("raw", sums=True)
    s.cell_weights(np.ones(7))
    s.cell_weights(None)
    with pytest.raises(RuntimeError, match="sums without weights"):
        s.cell_vortex("raw", sums=True)


# ---- the option ------------------------------------------------------------------------------------------------------------

def _parameters(extra):
    from vasp_amd.monolithic import parameters
    with contextlib.redirect_stdout(io.StringIO()):
        return parameters(["-p", "cylinder", "--verbose", "False", "-dt", "0.001", "--save-step", "1", "-T", "0.0115", *extra])[2]


def test_both_parsers_take_the_two_options():
    from vasp_amd import postprocess
    from vasp_amd.monolithic import add_session_arguments
    ap = argparse.ArgumentParser()
    add_session_arguments(ap)
    none = vars(ap.parse_args([]))
    assert none["hi_pass_vortex"] is None and none["hi_pass_vortex_series"] is None
    both = vars(ap.parse_args(SERIES))
    assert both["hi_pass_vortex"] is True and both["hi_pass_vortex_series"] is True
    assert vars(ap.parse_args(VORTEX))["hi_pass_vortex_series"] is None
    post = postprocess.parse(["--folder", "x", "--hi-pass", "v", *SERIES])
    assert post["hi_pass_vortex"] is True and post["hi_pass_vortex_series"] is True


def test_every_refusal_of_the_option_in_its_words(mesh, tmp_path):
    from vasp_amd import hi_pass_strips, monolithic, postprocess
    deg2 = ["--save-deg", "2"]
    assert hp.hi_pass_refusal(_parameters(["--hi-pass", "v", *deg2, *SERIES, *PHASE]), 1, None) == ""
    assert hp.hi_pass_refusal(_parameters(["--hi-pass", "d", "v", "p", *deg2, *VORTEX, "--hi-pass-flow-metrics", *PHASE]), 1, None) == ""
    why = hp.hi_pass_refusal(_parameters(["--hi-pass", "d", "p", *deg2, *VORTEX, *PHASE]), 1, None)
    assert why == vx.NEEDS_V == "--hi-pass-vortex needs v among the --hi-pass quantities: the vorticity is formed from the velocity history"
    for deg in (["--save-deg", "1"], []):
        why = hp.hi_pass_refusal(_parameters(["--hi-pass", "v", *deg, *VORTEX, *PHASE]), 1, None)
        assert why == vx.NEEDS_DEG2 and why.startswith("--hi-pass-vortex needs --save-deg 2: at save_deg 1 the session holds the vertices only")
    why = hp.hi_pass_refusal(_parameters(["--hi-pass", "v", *deg2, "--hi-pass-vortex-series", *PHASE]), 1, None)
    assert why == vx.NEEDS_VORTEX == "--hi-pass-vortex-series writes the per-frame fields of --hi-pass-vortex: it needs that option"
    assert all("\n" not in text for text in (vx.NEEDS_V, vx.NEEDS_DEG2, vx.NEEDS_VORTEX, vx.VORTEX_STRIPS))
    # without --hi-pass at all: both drivers refuse before anything else is done
    _run(tmp_path / "case", T="0.0015", options=[])
    for main, lead in ((monolithic.run, ["-p", "cylinder"]), (postprocess.run, ["--folder", str(tmp_path / "case" / "1")])):
        for options, text in ((VORTEX, vx.NEEDS_V), (["--hi-pass-vortex-series"], vx.NEEDS_VORTEX)):
            with pytest.raises(SystemExit) as e, contextlib.redirect_stdout(io.StringIO()):
                main([*lead, *options])
            assert str(e.value) == text
    # strips of rows refuse the option with words of their own
    ns = dict(_parameters(["--hi-pass", "v", *deg2, *VORTEX]), save_deg=2, results_folder=tmp_path, hi_pass_strip=(0, 8))
    with pytest.raises(SystemExit) as e:
        hp.HiPassRun(object(), mesh, ns)
    assert str(e.value) == vx.VORTEX_STRIPS and str(e.value).startswith("--hi-pass-vortex: the history goes through the session in strips of rows")
    job = hi_pass_strips.Job("field", "v", 8, 3, 1, 12)
    with pytest.raises(SystemExit) as e:
        hi_pass_strips.run_quantity(job, object(), mesh, ns, 1 << 20, lambda rows, capacity: 0, lambda *a: None)
    assert str(e.value) == vx.VORTEX_STRIPS
    assert not (tmp_path / "VortexMetrics").exists() and not (tmp_path / "Visualization_hi_pass").exists()
    assert not (tmp_path / "case" / "1" / "VortexMetrics").exists()


def test_strips_in_postprocess_refuse_the_option(tmp_path):
    """A finished folder whose history does not fit --history-memory: refused in the option's words, before and in the run."""
    from vasp_amd import postprocess
    _run(tmp_path / "case", options=[])                                                 # 40 frames: the default band needs 34
    for extra, text in ((VORTEX, vx.VORTEX_STRIPS), (["--hi-pass-flow-metrics", *VORTEX], hp.METRICS_STRIPS)):
        with pytest.raises(SystemExit) as e, contextlib.redirect_stdout(io.StringIO()):
            postprocess.run(["--folder", str(tmp_path / "case" / "1"), "--hi-pass", "v", *extra, "--history-memory", "400000"],
                            backend_factory=lambda desc: object(), out=lambda line: None)
        assert str(e.value) == text


# ---- the driver with a stub backend ------------------------------------------------------------------------------------------

def _vectors(path):
    from vasp_amd.h5lite import read_h5
    g = read_h5(path)["VisualisationVector"]
    return np.stack([np.asarray(g[str(k)].data) for k in range(len(g.keys()))])


def _files(names):
    return {f"{n}.{e}" for n in names for e in ("h5", "xdmf")}


def _tree_of(folder):
    return {str(p.relative_to(folder)): p.read_bytes() for p in sorted(folder.rglob("*")) if p.is_file()}


def test_driver_writes_the_files_of_the_saved_frames(tmp_path, mesh):
    """14 saved frames, three whole cycles of 4: the files with and without the series and the phase average, their values from
    the twin on the velocity frames the run wrote, the tables and the log line."""
    ns, lines = _run(tmp_path / "all" / "case", T="0.0135", options=["--hi-pass", "v", *SERIES, *PHASE])
    out = tmp_path / "all" / "case" / "1" / "VortexMetrics"
    assert {p.name for p in out.iterdir()} == _files(MEAN_FILES + PHASE_FILES + vx.SERIES_FILES) | TABLES
    _run(tmp_path / "mean" / "case", options=["--hi-pass", "v", *VORTEX])               # 40 frames: the default band needs 34
    assert {p.name for p in (tmp_path / "mean" / "case" / "1" / "VortexMetrics").iterdir()} == _files(MEAN_FILES) | TABLES
    _run(tmp_path / "series" / "case", options=["--hi-pass", "v", *SERIES])
    assert {p.name for p in (tmp_path / "series" / "case" / "1" / "VortexMetrics").iterdir()} == _files(MEAN_FILES + vx.SERIES_FILES) | TABLES
    _run(tmp_path / "phase" / "case", T="0.0135", options=["--hi-pass", "v", *VORTEX, *PHASE])
    assert {p.name for p in (tmp_path / "phase" / "case" / "1" / "VortexMetrics").iterdir()} == _files(MEAN_FILES + PHASE_FILES) | TABLES
    # the values: the twin on the frames the run wrote
    x = _vectors(tmp_path / "all" / "case" / "1" / "Visualization" / "velocity.h5")
    assert x.shape == (14, mesh.num_nodes, 3)
    cells = fm.fluid_cells(mesh, ns["dx_f_id"])
    conn, g, vol = mesh.tet_nodes[cells], fm.barycentric_gradients(mesh, cells), fm.cell_volumes(mesh, cells)
    r = np.stack([hp.cell_vortex(x[k][conn], g) for k in range(14)])
    mean = hp.ordered_mean(r)
    want = dict(q_criterion_avg=mean[0], vorticity_rms=np.sqrt(mean[1]), helicity_avg=mean[2], helicity_intensity=mean[3],
                helicity_balance=mean[2] / mean[3], kinetic_energy_avg=0.5 * mean[4])
    for name, values in want.items():
        got = _vectors(out / f"{name}.h5")
        assert got.shape == (1, len(cells), 1) and got.dtype == np.float32 and np.array_equal(got[0, :, 0], values.astype(np.float32)), name
    series = dict(q_criterion=r[:, 0], vorticity=np.sqrt(r[:, 1]), helicity=r[:, 2], lnh=r[:, 2] / np.sqrt(r[:, 4] * r[:, 1]))
    for name, values in series.items():
        got = _vectors(out / f"{name}.h5")
        assert got.shape == (14, len(cells), 1) and np.array_equal(got[:, :, 0], values.astype(np.float32)), name
        assert (out / f"{name}.xdmf").read_text().count('Center="Cell"') == 14
    assert (np.abs(series["lnh"]) <= 1.0 + 4 * EPS).all()
    s = hp.HostBandSession(3, 14)
    s.import_(x)
    s.select(0, 12, 1)
    s.phase(4)
    s.cells(conn, g)
    assert np.array_equal(_vectors(out / "q_criterion_phase_mean.h5")[:, :, 0],
                          np.stack([hp.cell_vortex(s.phase_fetch("mean", j)[conn], g)[0] for j in range(4)]).astype(np.float32))
    assert np.array_equal(_vectors(out / "vorticity_rms_fluctuation.h5")[0, :, 0], np.sqrt(s.cell_vortex("series")[0][1]).astype(np.float32))
    # vortex.csv: the ordered sums with the cell volumes; its volume column is the sum of the cell volumes
    text = (out / "vortex.csv").read_text().splitlines()
    assert text[0] == "# " + vx.CURVES_HEADER and len(text) == 15
    table = np.array([[float(a) for a in line.split(", ")] for line in text[1:]])
    assert (table[:, 1] == np.sum(vol)).all() and np.array_equal(table[:, 0], np.arange(14) * 1e-3)
    sums = np.stack([hp.cell_wsum(r[k], vol) for k in range(14)])
    assert np.array_equal(table[:, 2:], np.stack([0.5 * sums[:, 4], sums[:, 1], sums[:, 2], sums[:, 3], sums[:, 0]], axis=1))
    assert np.allclose(table[:, 3], [math.fsum(vol * r[k, 1]) for k in range(14)], rtol=1e-13, atol=0)
    # the helicity indices and their relations
    h = [float(a) for a in (out / "helicity_indices.csv").read_text().splitlines()[1].split(", ")]
    assert (out / "helicity_indices.csv").read_text().splitlines()[0] == "# h1, h2, h3, h4"
    assert h[0] == hp.ordered_mean(sums[:, 2] / np.sum(vol)) and h[1] == hp.ordered_mean(sums[:, 3] / np.sum(vol))
    assert h[2] == h[0] / h[1] and h[3] == abs(h[2]) and abs(h[0]) <= h[1] and 0 < h[3] <= 1 and h[1] > 0
    assert vx.helicity_indices(np.zeros((3, 7)) + [0, 1, 0, 0, 0, 0, 0]) == [0.0, 0.0, 0.0, 0.0]
    # the summary table and the log line
    rows = (out / "vortex_summary.csv").read_text().splitlines()
    assert rows[0] == fm.CSV_HEADER and [row.split(", ")[0] for row in rows[1:]] == [*MEAN_FILES, "vorticity_rms_fluctuation"]
    got = {row.split(", ")[0]: row.split(", ")[1:] for row in rows[1:]}
    v = want["vorticity_rms"]
    assert [float(a) for a in got["vorticity_rms"][:3]] == [float(np.sum(v * vol) / np.sum(vol)), v.min(), v.max()]
    assert int(got["vorticity_rms"][3]) == cells[np.argmax(v)]
    line = [text for text in lines if text.startswith("Vortex metrics of")]
    assert len(line) == 1 and f"{len(cells)} fluid cells over 14 frames" in line[0] and f"h1 = {h[0]:.4g}" in line[0]
    assert lines.index(line[0]) > max(i for i, text in enumerate(lines) if "phase average over cycles" in text)


def test_a_run_without_the_option_is_unchanged_and_flow_metrics_stay_their_bytes(tmp_path, monkeypatch):
    base = ["--hi-pass", "v", "p", "--hi-pass-flow-metrics", "--hi-pass-bands", "0", "200", *PHASE]
    _run(tmp_path / "without" / "case", T="0.0135", options=base)
    attached, cells_of = [], hp.HostBandSession.cells
    monkeypatch.setattr(hp.HostBandSession, "cells", lambda self, *a: (attached.append(len(a[0])), cells_of(self, *a))[1])
    _run(tmp_path / "with" / "case", T="0.0135", options=[*base, *SERIES])
    assert len(attached) == 1                       # both options use one list of fluid cells: it is attached once
    _run(tmp_path / "alone" / "case", T="0.0135", options=[o for o in base if o != "--hi-pass-flow-metrics"] + [*SERIES])
    assert attached == attached[:1] * 2
    old, new = tmp_path / "without" / "case" / "1", tmp_path / "with" / "case" / "1"
    assert not (old / "VortexMetrics").exists() and (new / "VortexMetrics" / "lnh.h5").exists()
    for sub in ("FlowMetrics", "Visualization_hi_pass", "Visualization"):
        a, b = _tree_of(old / sub), _tree_of(new / sub)
        assert a == b and len(a) > 1, sub
    a, b = _tree_of(tmp_path / "alone" / "case" / "1" / "VortexMetrics"), _tree_of(new / "VortexMetrics")
    assert a == b and len(a) > 1                    # and the vortex files are those of a run with the option alone


def test_a_split_run_writes_the_bytes_of_an_unsplit_run(tmp_path):
    """Everything is formed at the end from the recorded history, which the checkpoint carries: a run stopped after 17 of 40 steps
    and continued with --restart-folder writes the files of the unsplit run."""
    options = ["--hi-pass", "v", *SERIES, *PHASE]
    _run(tmp_path / "whole" / "case", options=options)
    half = tmp_path / "half" / "case" / "1"
    half.mkdir(parents=True)
    ns, lines = _run(half.parent, options=options, kill_at=SPLIT, kill_path=half / "killturtle")
    assert ns["backend"].steps == SPLIT
    ns, lines = _restart(half, options=options)
    assert any("Vortex metrics of" in line and "over 40 frames" in line for line in lines)
    whole, split = _tree_of(tmp_path / "whole" / "case" / "1" / "VortexMetrics"), _tree_of(half / "VortexMetrics")
    assert sorted(whole) == sorted(split) and len(whole) == 2 * 12 + 3
    for name in whole:
        assert whole[name] == split[name], name


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------

def test_header_binding_and_tables_agree():
    import re
    from conftest import ROOT
    from vasp_amd import capi
    header = (ROOT / "include" / "vaspfsi.h").read_text()
    lib = capi.load_library()
    for name in ("fsi_band_cell_weights", "fsi_band_cell_vortex"):
        m = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S)
        assert m and name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
        assert "Replaces: nothing in the reference." in header[:m.start()].rsplit("/*", 1)[1], name
    assert capi.HipBackend.VORTEX_FIELDS == hp.VORTEX_FIELDS and re.search(r"#define FSI_VORTEX_FIELDS %d\b" % len(hp.VORTEX_FIELDS), header)
    for k, field in enumerate(hp.VORTEX_FIELDS):
        assert re.search(r"#define FSI_VORTEX_%s %d\b" % (field.upper(), k), header), field
    M, MM = hp.vortex_tables()
    assert np.array_equal(hp.VORTEX_M, M / 60.0) and np.array_equal(hp.VORTEX_MM, MM / 420.0) and np.array_equal(MM, MM.T)
    assert M.sum(axis=0).tolist() == [15] * 4 and MM.sum() == 420                      # partition of unity: sum_a M[a][t] = 1 / 4, sum MM = 1
