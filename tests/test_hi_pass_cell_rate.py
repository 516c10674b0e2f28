"""The strain rate of a recorded history on mesh cells and the flow metrics of ``--hi-pass-flow-metrics``, host side: the NumPy
twin of csrc/fsi_rate.hip (``hi_pass.cell_rate``, ``HostBandSession.cells`` / ``cell_rate``) against an independent restatement
in extended precision and against known answers, the ordered sum over frames and the twin's refusals, the closing formulas of
vasp_amd/flow_metrics.py, the option with its refusals and the driver's files with a stub backend.

The per-cell bound: ``80 * 2^-53 * B_c``, ``B_c`` being the twin's formula with the absolute value of every product - a forward
bound of everything that is rounded: a gradient entry is a sum of 22 products (4 vertex terms of two products, 6 edge terms of
three products and a sum), it enters a square, and the closing sums add 36 + 9 + 2 terms; eighty roundings cover the chain."""
import argparse
import contextlib
import io
import re

import numpy as np
import pytest

from conftest import ROOT
from test_session_restart import CYL, _run, one_modification_time  # noqa: F401  (the fixture holds h5lite's clock)
from vasp_amd import flow_metrics as fm
from vasp_amd import hi_pass as hp
from vasp_amd.mesh import TET_EDGES, FsiMesh
from vasp_amd.quadrature import tabulate_tet, tet_rule_deg6

EPS = 2.0 ** -53
LD = np.longdouble


@pytest.fixture(scope="module")
def mesh():
    return FsiMesh.read(CYL)


@pytest.fixture(scope="module")
def cells(mesh):
    """Every cell of the cylinder fixture, its P2 nodes and the gradients of its barycentric coordinates."""
    c = np.arange(mesh.num_cells)
    return c, mesh.tet_nodes[c], fm.barycentric_gradients(mesh, c)


def bound(w, g):
    """B_c: ``hi_pass.cell_rate`` with the absolute value of every product."""
    w, g = np.abs(np.asarray(w, dtype=np.float64)), np.abs(np.asarray(g, dtype=np.float64))
    n = len(w)
    q, T = np.zeros(n), [[np.zeros(n) for _ in range(3)] for _ in range(3)]
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
                S = 0.5 * (G[i][j] + G[j][i])
                q = q + S * S
                T[i][j] = T[i][j] + S
    p = np.zeros(n)
    for i in range(3):
        for j in range(3):
            p = p + T[i][j] * T[i][j]
    return 0.1 * (q + p)


def by_quadrature(w, g):
    """The cell mean of ``2 sym(grad w):sym(grad w)`` by the degree-6 rule on 24 points, in ``np.longdouble``: the P2 basis
    gradients at the points (``tabulate_tet``) mapped by the gradients of the barycentric coordinates 1 .. 3, which are those
    of the reference coordinates.  No vertex value of the gradient is formed."""
    qp, qw = tet_rule_deg6()
    dN = tabulate_tet(qp)[1].astype(LD)                         # (Q, 10, 3) reference gradients
    w, g, qw = np.asarray(w).astype(LD), np.asarray(g).astype(LD), qw.astype(LD)
    phys = np.einsum("qak,ckj->cqaj", dN, g[:, 1:4])            # d N_a / d x_j at every point of every cell
    G = np.einsum("cai,cqaj->cqij", w, phys)
    S = (G + G.transpose(0, 1, 3, 2)) / LD(2)
    return (np.einsum("q,cqij,cqij->c", qw, S, S) * LD(2)) / qw.sum()


def test_twin_against_the_quadrature_restatement(mesh, cells):
    """Random P2 fields on every cell of the cylinder fixture.  The largest err / (2^-53 B_c) observed: 1.8 (the bound allows
    80).  The restatement takes the reference-coordinate route (``quadrature.tabulate_tet``), not the vertex formula; the
    centroid shortcut - the gradient at the centroid alone - misses the bound by many orders of magnitude."""
    c, conn, g = cells
    rng = np.random.default_rng(0)
    w = rng.standard_normal((len(c), 10, 3)) * rng.uniform(0.1, 10.0, (len(c), 1, 1))
    got, B = hp.cell_rate(w, g), bound(w, g)
    ref = by_quadrature(w, g)
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    print("largest err / (2^-53 B_c):", (err / (EPS * B)).max())
    assert (err <= 80 * EPS * B).all()
    assert got.dtype == np.float64 and got.shape == (len(c),) and (got > 0).all()
    # the centroid shortcut: 2 S:S of the mean of the four vertex gradients
    centre = by_quadrature(w, g) * 0
    qp = np.full((1, 3), 0.25)
    dN = tabulate_tet(qp)[1].astype(LD)
    G = np.einsum("cai,caj->cij", w.astype(LD), np.einsum("ak,ckj->caj", dN[0], g[:, 1:4].astype(LD)))
    S = (G + G.transpose(0, 2, 1)) / LD(2)
    centre = 2 * np.einsum("cij,cij->c", S, S)
    assert (np.abs(centre - ref).astype(np.float64) > 80 * EPS * B).mean() > 0.99


def test_known_answers(mesh, cells):
    """``w = A x + b`` has ``2 sym(A):sym(A)`` on every cell, a rigid rotation ``w = omega x x`` has 0."""
    c, conn, g = cells
    x = mesh.node_coords[conn]                                  # (cells, 10, 3)
    rng = np.random.default_rng(1)
    A, b = rng.standard_normal((3, 3)), rng.standard_normal(3)
    w = x @ A.T + b
    sym = 0.5 * (A + A.T)
    got, B = hp.cell_rate(w, g), bound(w, g)
    assert (np.abs(got - 2.0 * np.sum(sym * sym)) <= 80 * EPS * B).all()
    omega = np.array([0.3, -1.1, 0.7])
    w = np.cross(omega, x)
    got, B = hp.cell_rate(w, g), bound(w, g)
    assert (np.abs(got) <= 80 * EPS * B).all() and (B > 0).all()
    assert not hp.cell_rate(np.zeros((len(c), 10, 3)), g).any() and not np.signbit(hp.cell_rate(np.zeros((len(c), 10, 3)), g)).any()
    w[3, 2, 1] = np.nan
    got = hp.cell_rate(w, g)
    assert np.isnan(got[3]) and np.isfinite(np.delete(got, 3)).all()
    with pytest.raises(RuntimeError, match="expected"):
        hp.cell_rate(w[:, :4], g)


def _history(mesh, frames, period, seed=2):
    """(frames, N2, 3): a part that repeats with ``period`` and a fluctuation of a tenth of it."""
    rng = np.random.default_rng(seed)
    cycle = rng.standard_normal((period, mesh.num_nodes, 3))
    return np.tile(cycle, (frames // period, 1, 1)) + 0.1 * rng.standard_normal((frames, mesh.num_nodes, 3))


def _session(x, ncomp=3):
    s = hp.HostBandSession(ncomp, len(x))
    s.import_(x)
    return s


def test_decomposition_identity(mesh, cells):
    """Over whole cycles ``R(raw) = mean_phi R(mean_phi) + R(u')``: the cross term vanishes under the phase average.  The bound
    is ``80 * 2^-53`` times the mean over the frames of B_c of the raw frames, and the identity is held to three times it: three
    rates are compared, the decomposition itself rounds u' and the mean, and a sum over frames rounds once per frame.  Largest
    observed error: 0.008 of the bound."""
    c, conn, g = cells
    for period, cycles in ((4, 3), (3, 4)):
        x = _history(mesh, period * cycles, period)
        s = _session(x)
        s.phase(period)
        s.cells(conn, g)
        raw, fluct, mean = s.cell_rate("raw"), s.cell_rate("series"), s.cell_rate("phase_mean")
        B = np.mean([bound(x[k][conn], g) for k in range(len(x))], axis=0)
        err = np.abs(raw - (mean + fluct))
        print("decomposition: largest err / (80 * 2^-53 * B):", (err / (80 * EPS * B)).max())
        assert (err <= 3 * 80 * EPS * B).all() and (fluct > 0).all() and (mean > fluct).all()


def test_ordered_sum_over_first_step_count(mesh, cells):
    c, conn, g = cells
    conn, g = conn[:7], g[:7]
    x = _history(mesh, 12, 4)
    s = _session(x)
    s.cells(conn, g)
    r = np.stack([hp.cell_rate(x[k][conn], g) for k in range(12)])
    for k in (0, 5, 11):
        assert np.array_equal(s.cell_rate("raw", k, 1, 1), r[k])                     # one frame: its own bits
    assert np.array_equal(s.cell_rate("raw"), hp.ordered_mean(r)) and np.array_equal(s.cell_rate("raw", 0, 1, 12), hp.ordered_mean(r))
    assert np.array_equal(s.cell_rate("raw", 1, 4, 3), (((0.0 + r[1]) + r[5]) + r[9]) / 3.0)
    assert np.array_equal(s.cell_rate("raw", 2, 3), hp.ordered_mean(r[2::3])) and np.array_equal(s.cell_rate("raw", 11), r[11])
    # through a selection's stride, and on the series and the phase means
    assert s.select(2, 4, 2) == 4
    assert np.array_equal(s.cell_rate("raw"), hp.ordered_mean(r[2:10:2])) and np.array_equal(s.cell_rate("raw", 3, 1, 1), r[8])
    s.phase(2)
    f = np.stack([s.fetch("filtered", k) for k in range(4)])
    rf = np.stack([hp.cell_rate(f[k][conn], g) for k in range(4)])
    assert np.array_equal(s.cell_rate("series", 1, 2, 2), ((0.0 + rf[1]) + rf[3]) / 2.0)
    assert np.array_equal(s.cell_rate("phase_mean", 1, 1, 1), hp.cell_rate(s.phase_fetch("mean", 1)[conn], g))
    assert np.array_equal(s.cell_rate("phase_mean"), hp.ordered_mean(np.stack([hp.cell_rate(s.phase_fetch("mean", j)[conn], g) for j in range(2)])))
    # the list survives select, filter and phase; a NaN or an inf goes through
    x[3, conn[2, 4], 1] = np.inf
    s = _session(x)
    s.cells(conn, g)
    s.select(0, 12, 1)
    with np.errstate(invalid="ignore"):
        s.filter(np.array([1.0, 0.0]), np.array([1.0, 0.0]), np.zeros(1), 0)
    got = s.cell_rate("raw")
    hit = (conn == conn[2, 4]).any(axis=1)
    assert hit[2] and not np.isfinite(got[hit]).any() and np.isfinite(got[~hit]).all()
    assert np.array_equal(s.cell_rate("series"), got, equal_nan=True)                    # the identity filter


def test_every_refusal_of_the_twin(mesh, cells):
    c, conn, g = cells
    conn, g = conn[:5], g[:5]
    x = _history(mesh, 8, 4)
    s = _session(x)
    with pytest.raises(RuntimeError, match=r"no cell list \(cells first\)"):
        s.cell_rate("raw")
    for bad_conn, bad_g in ((conn[:0], g[:0]), (conn[:, :9], g), (conn, g[:4]), (conn, g[:, :3])):
        with pytest.raises(RuntimeError, match="needs n > 0 cells, conn"):
            s.cells(bad_conn, bad_g)
    with pytest.raises(RuntimeError, match=f"cell 1 has node {mesh.num_nodes}, which is no node of the session"):
        s.cells(np.where(np.arange(50).reshape(5, 10) == 13, mesh.num_nodes, conn), g)
    with pytest.raises(RuntimeError, match="cell 0 has node -1"):
        s.cells(np.where(np.arange(50).reshape(5, 10) == 0, -1, conn), g)
    with pytest.raises(RuntimeError, match="a session of d or v"):
        _session(x[:, :, :1], 1).cells(conn, g)
    with pytest.raises(RuntimeError, match="no cell list"):                            # the refused calls attached nothing
        s.cell_rate("raw")
    assert s.cells(conn, g).shape == (5, 4, 3)
    with pytest.raises(RuntimeError, match="needs n > 0 cells"):                         # a refused call leaves the list in place
        s.cells(conn[:0], g[:0])
    assert s.cell_rate("raw").shape == (5,)
    with pytest.raises(RuntimeError, match="series must be one of raw, series, phase_mean"):
        s.cell_rate("filtered")
    with pytest.raises(RuntimeError, match=r"no filtered series \(filter or phase first\)"):
        s.cell_rate("series")
    with pytest.raises(RuntimeError, match=r"no phase average \(phase first\)"):
        s.cell_rate("phase_mean")
    for first, step, count in ((0, 0, 1), (0, 1, 0), (0, -1, 2), (0, 1, -2)):
        with pytest.raises(RuntimeError, match="needs step >= 1 and count >= 1"):
            s.cell_rate("raw", first, step, count)
    for first, step, count in ((8, 1, 1), (-1, 1, 1), (0, 1, 9), (1, 4, 3), (7, 1, 2)):
        with pytest.raises(RuntimeError, match="fall outside the series of 8 frames"):
            s.cell_rate("raw", first, step, count)
    s.phase(4)
    with pytest.raises(RuntimeError, match="fall outside the series of 4 frames"):
        s.cell_rate("phase_mean", 4, 1, 1)
    assert s.cell_rate("raw", 3, 4, 2).shape == (5,) and s.cell_rate("phase_mean", 3).shape == (5,)
    s.cells(conn[:2], g[:2])                                                          # a second call replaces the list
    assert s.cell_rate("series").shape == (2,)
    s.end()
    with pytest.raises(RuntimeError, match="no cell list"):
        s.cell_rate("raw")


def same_bits(a, b) -> bool:
    """Equal values with NaN equal to NaN, and equal signs of the zeros: the rule of the GPU tests."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[a == 0]), np.signbit(b[b == 0]))


def test_twin_bits_are_those_recorded():
    """The GPU tests hold the device to the twins bit for bit; this holds the twins to their own recorded bits, so that a
    change to the pieces they share (``hi_pass.vertex_gradients``) cannot move both.  golden/hi_pass/cell_twin_bits.npz
    (golden/make_cell_twin_bits.py): 7 cells - one with a NaN, one with an inf, one of zeros of both signs, one folded by its
    displacement so that one ``J_q < 0`` - and what ``cell_rate``, ``cell_rate_current``, ``cell_vortex`` and ``cell_wsum`` of
    the vortex rows gave for them when the fixture was recorded.  The sums over all seven cells are NaN in every row, so the
    sums over the cells with finite rows are held as well."""
    z = np.load(ROOT / "tests" / "golden" / "hi_pass" / "cell_twin_bits.npz")
    w, d, grad, weights = z["w"], z["d"], z["grad"], z["weights"]
    assert w.shape == d.shape == (7, 10, 3) and np.isnan(w).any() and np.isinf(w).any() and np.signbit(w[w == 0]).any()
    assert same_bits(hp.cell_rate(w, grad), z["rate"])
    for got, name in zip(hp.cell_rate_current(w, d, grad), ("rate_current", "volume_ratio", "min_jacobian")):
        assert same_bits(got, z[name]), name
    assert (z["min_jacobian"] < 0).sum() == 1 and np.isnan(z["rate"]).any() and (z["rate"] == 0).any()
    vortex = hp.cell_vortex(w, grad)
    assert same_bits(vortex, z["vortex"])
    finite = np.isfinite(vortex).all(axis=0)
    assert same_bits(hp.cell_wsum(vortex, weights), z["wsum"]) and same_bits(hp.cell_wsum(vortex[:, finite], weights[finite]), z["wsum_finite"])
    assert finite.sum() == 5 and np.isfinite(z["wsum_finite"]).all()


# ---- the closing formulas -------------------------------------------------------------------------------------------------

def test_closing_formulas_on_hand_made_arrays():
    nu, h, dt = np.array([2.0, 0.5, 1.0]), np.array([1.0, 2.0, 4.0]), 0.25
    m = fm.strain_metrics(np.array([16.0, 4.0, 0.0]), nu, h, dt)
    assert np.array_equal(m["strain_rate"], [4.0, 2.0, 0.0]) and np.array_equal(m["dissipation"], [32.0, 2.0, 0.0])
    assert np.array_equal(m["l_plus"], [np.sqrt(2.0), 4.0, 0.0]) and np.array_equal(m["t_plus"], [1.0, 0.5, 0.0])
    t = fm.turbulence_metrics(np.array([4.0, 32.0, 0.0]), np.array([1.0, 2.0, 3.0]), nu, h, dt)
    assert np.array_equal(t["turbulent_dissipation"], [8.0, 16.0, 0.0]) and np.array_equal(t["mean_flow_dissipation"], [2.0, 1.0, 3.0])
    assert np.array_equal(t["kolmogorov_length"], [1.0, np.sqrt(np.sqrt(0.125 / 16.0)), np.inf])       # (nu^3 / eps)^(1/4)
    assert np.array_equal(t["kolmogorov_time"], [0.5, np.sqrt(0.5 / 16.0), np.inf])
    assert np.array_equal(t["kolmogorov_velocity"], [2.0, np.sqrt(np.sqrt(8.0)), 0.0])
    assert np.array_equal(t["length_ratio"], [1.0, 2.0 / np.sqrt(np.sqrt(0.125 / 16.0)), 0.0])            # eps' = 0: eta = inf, h / eta = 0
    assert np.array_equal(t["time_ratio"], [0.5, 0.25 / np.sqrt(0.5 / 16.0), 0.0])
    nan = fm.turbulence_metrics(np.array([np.nan]), np.array([1.0]), nu[:1], h[:1], dt)
    assert np.isnan(nan["kolmogorov_length"][0]) and np.isnan(nan["length_ratio"][0])                    # nothing is clamped
    assert fm.summary_row(np.array([1.0, 5.0, 3.0]), np.array([1.0, 1.0, 2.0]), np.array([10, 20, 30])) == (3.0, 1.0, 5.0, 20)


def test_fluid_cells_and_their_constants(mesh):
    v = dict(dx_f_id=1, mu_f=3.5e-3, rho_f=1.025e3)
    cells = fm.fluid_cells(mesh, 1)
    assert 0 < len(cells) < mesh.num_cells and (mesh.cell_markers[cells] == 1).all() and (np.diff(cells) > 0).all()
    assert np.array_equal(fm.kinematic_viscosity(mesh, cells, v), np.full(len(cells), 3.5e-3 / 1.025e3))
    two = fm.kinematic_viscosity(mesh, np.arange(mesh.num_cells), dict(dx_f_id=[1, 2], mu_f=[1.0, 3.0], rho_f=2.0))
    assert np.array_equal(two, np.where(mesh.cell_markers == 1, 0.5, 1.5))
    assert fm.cell_diameters(mesh, np.arange(mesh.num_cells)).min() == mesh.hmin()
    x = mesh.coords
    lo, hi = x.min(axis=0), x.max(axis=0)
    vol = fm.cell_volumes(mesh, np.arange(mesh.num_cells))
    assert (vol > 0).all() and 0.5 * np.prod(hi - lo) < vol.sum() < np.prod(hi - lo)
    g = fm.barycentric_gradients(mesh, cells)
    xc = mesh.coords[mesh.tets[cells]]
    lam = np.einsum("caj,cbj->cab", g, xc - xc[:, :1])                                  # L_a(x_b) - L_a(x_0)
    assert np.allclose(lam + np.eye(4)[:, :1], np.broadcast_to(np.eye(4), lam.shape), atol=1e-9)
    geometry, topology = fm.submesh(mesh, cells)
    assert topology.shape == (len(cells), 4) and np.array_equal(geometry[topology], xc)


# ---- the option ------------------------------------------------------------------------------------------------------------

def _parameters(extra):
    from vasp_amd.monolithic import parameters
    with contextlib.redirect_stdout(io.StringIO()):
        return parameters(["-p", "cylinder", "--verbose", "False", "-dt", "0.001", "--save-step", "1", "-T", "0.0115", *extra])[2]


PHASE = ["--hi-pass-phase-average", "--hi-pass-cycle", "0.004"]


def test_option_parsing_and_the_three_refusals(mesh, tmp_path):
    from vasp_amd import hi_pass_strips, postprocess
    from vasp_amd.monolithic import add_session_arguments
    ap = argparse.ArgumentParser()
    add_session_arguments(ap)
    assert vars(ap.parse_args([]))["hi_pass_flow_metrics"] is None
    assert vars(ap.parse_args(["--hi-pass-flow-metrics"]))["hi_pass_flow_metrics"] is True
    assert postprocess.parse(["--folder", "x", "--hi-pass", "v", "--hi-pass-flow-metrics"])["hi_pass_flow_metrics"] is True
    on = ["--hi-pass-flow-metrics", *PHASE]
    assert hp.hi_pass_refusal(_parameters(["--hi-pass", "v", "--save-deg", "2", *on]), 1, None) == ""
    assert hp.hi_pass_refusal(_parameters(["--hi-pass", "d", "v", "p", "--save-deg", "2", *on]), 1, None) == ""
    why = hp.hi_pass_refusal(_parameters(["--hi-pass", "d", "p", "--save-deg", "2", *on]), 1, None)
    assert why == fm.NEEDS_V and "needs v among the --hi-pass quantities" in why and "\n" not in why
    for deg in (["--save-deg", "1"], []):
        why = hp.hi_pass_refusal(_parameters(["--hi-pass", "v", *deg, *on]), 1, None)
        assert why == fm.NEEDS_DEG2 and "needs --save-deg 2" in why and "vertices only" in why and "\n" not in why
    assert "padlen" in hp.hi_pass_refusal(_parameters(["--hi-pass", "v", "--save-deg", "1"]), 1, None)       # without the option: as before
    # strips of rows refuse the option, in one line
    ns = dict(_parameters(["--hi-pass", "v", "--save-deg", "2", "--hi-pass-flow-metrics"]), save_deg=2, results_folder=tmp_path, hi_pass_strip=(0, 8))
    with pytest.raises(SystemExit) as e:
        hp.HiPassRun(object(), mesh, ns)
    assert str(e.value) == hp.METRICS_STRIPS and "strips of rows" in str(e.value) and "\n" not in str(e.value)
    job = hi_pass_strips.Job("field", "v", 8, 3, 1, 12)
    with pytest.raises(SystemExit) as e:
        hi_pass_strips.run_quantity(job, object(), mesh, ns, 1 << 20, lambda rows, capacity: 0, lambda *a: None)
    assert str(e.value) == hp.METRICS_STRIPS
    assert not (tmp_path / "FlowMetrics").exists() and not (tmp_path / "Visualization_hi_pass").exists()


# ---- the driver with a stub backend ------------------------------------------------------------------------------------------

def _vectors(path):
    from vasp_amd.h5lite import read_h5
    g = read_h5(path)["VisualisationVector"]
    return np.stack([np.asarray(g[str(k)].data) for k in range(len(g.keys()))])


def _velocity(results):
    return _vectors(results / "Visualization" / "velocity.h5")


def expected_metrics(mesh, ns_like, x, period, grad=None, bands=()):
    """The metrics of velocity frames x (frames, N2, 3) by the closing formulas on the twin's rates; ``grad``: the gradients to
    use (default: the host's own)."""
    cells = fm.fluid_cells(mesh, ns_like["dx_f_id"])
    conn = mesh.tet_nodes[cells]
    grad = fm.barycentric_gradients(mesh, cells) if grad is None else grad
    nu, h = fm.kinematic_viscosity(mesh, cells, ns_like), fm.cell_diameters(mesh, cells)
    s = _session(x)
    s.cells(conn, grad)
    out = fm.strain_metrics(s.cell_rate("raw"), nu, h, float(ns_like["dt"]))
    if period:
        n = len(x) // period * period
        s.select(0, n, 1)
        s.phase(period)
        out.update(fm.turbulence_metrics(s.cell_rate("series"), s.cell_rate("phase_mean"), nu, h, float(ns_like["dt"])))
        out["turbulent_dissipation_phase_mean"] = nu[None] * np.stack([s.cell_rate("series", j, period, n // period) for j in range(period)])
    return cells, out


PHASE_NAMES = ("turbulent_dissipation", "mean_flow_dissipation", "kolmogorov_length", "kolmogorov_time", "kolmogorov_velocity", "length_ratio",
               "time_ratio", "turbulent_dissipation_phase_mean")


def test_driver_writes_the_metrics_of_the_saved_frames(tmp_path, mesh):
    """14 saved frames: strain metrics over all of them, the turbulence metrics over three whole cycles of 4."""
    ns, lines = _run(tmp_path / "case", T="0.0135", options=["--hi-pass", "v", "p", "--hi-pass-flow-metrics", *PHASE])
    results = tmp_path / "case" / "1"
    out = results / "FlowMetrics"
    x = _velocity(results)
    assert x.shape == (14, mesh.num_nodes, 3)
    cells, want = expected_metrics(mesh, ns, x, 4)
    names = ("strain_rate", "dissipation", "l_plus", "t_plus", *PHASE_NAMES)
    assert {p.name for p in out.iterdir()} == {f"{n}.{e}" for n in names for e in ("h5", "xdmf")} | {"flow_metrics.csv"}
    for name in names:
        got = _vectors(out / f"{name}.h5")
        frames = 4 if name.endswith("phase_mean") else 1
        assert got.shape == (frames, len(cells), 1) and got.dtype == np.float32, name
        assert np.array_equal(got[:, :, 0], np.atleast_2d(want[name]).astype(np.float32)), name
        text = (out / f"{name}.xdmf").read_text()
        assert text.count('Center="Cell"') == frames and 'Center="Node"' not in text and f'Dimensions="{len(cells)} 1"' in text
        assert [float(t) for t in re.findall(r'<Time Value="([^"]+)"', text)] == [k * 1e-3 for k in range(frames)]
    from vasp_amd.h5lite import read_h5
    g = read_h5(out / "l_plus.h5")["Mesh"]["0"]["mesh"]
    geometry, topology = fm.submesh(mesh, cells)
    assert np.array_equal(g["geometry"].data, geometry.astype(np.float32)) and np.array_equal(g["topology"].data, topology)
    assert (want["strain_rate"] > 0).all() and (want["turbulent_dissipation"] > 0).all() and np.isfinite(want["length_ratio"]).all()
    # the table: volume-weighted mean, minimum, maximum and the cell of the maximum; the log line carries three maxima
    table = (out / "flow_metrics.csv").read_text().splitlines()
    assert table[0] == fm.CSV_HEADER and len(table) == 1 + 11 + 4
    rows = {r.split(", ")[0]: r.split(", ")[1:] for r in table[1:]}
    vol = fm.cell_volumes(mesh, cells)
    for name in ("l_plus", "turbulent_dissipation", "turbulent_dissipation_phase_mean[3]"):
        v = want["turbulent_dissipation_phase_mean"][3] if name.endswith("]") else want[name]
        assert [float(a) for a in rows[name][:3]] == [float(np.sum(v * vol) / np.sum(vol)), v.min(), v.max()] and int(rows[name][3]) == cells[np.argmax(v)]
    line = [l for l in lines if l.startswith("Flow metrics of")]
    assert len(line) == 1 and all(f"max {k} = {want[k].max():.4g}" in line[0] for k in ("l_plus", "t_plus", "length_ratio"))
    assert lines.index(line[0]) > max(i for i, l in enumerate(lines) if "Hi-pass velocity: phase average over cycles" in l)


def test_without_the_phase_average_and_with_a_band(tmp_path, mesh):
    """40 frames and the low-pass band 0 - 200 Hz: the four strain metrics and the band's dissipation; nothing else the options
    write changes."""
    base = ["--hi-pass", "v", "--hi-pass-bands", "0", "200"]
    ns, lines = _run(tmp_path / "with" / "case", options=[*base, "--hi-pass-flow-metrics"])
    _run(tmp_path / "without" / "case", options=base)
    results = tmp_path / "with" / "case" / "1"
    out = results / "FlowMetrics"
    assert {p.stem for p in out.iterdir()} == {"strain_rate", "dissipation", "l_plus", "t_plus", "dissipation_0_to_200", "flow_metrics"}
    x = _velocity(results)
    cells, want = expected_metrics(mesh, ns, x, 0)
    for name in ("strain_rate", "dissipation", "l_plus", "t_plus"):
        assert np.array_equal(_vectors(out / f"{name}.h5")[0, :, 0], want[name].astype(np.float32)), name
    prm = hp.design(1e-3, 0.0, 200.0)
    s = _session(x)
    s.cells(mesh.tet_nodes[cells], fm.barycentric_gradients(mesh, cells))
    s.filter(prm["b"], prm["a"], prm["zi"], prm["padlen"])
    nu = fm.kinematic_viscosity(mesh, cells, ns)
    assert np.array_equal(_vectors(out / "dissipation_0_to_200.h5")[0, :, 0], (nu * s.cell_rate("series")).astype(np.float32))
    old = {p.name: p.read_bytes() for p in (tmp_path / "without" / "case" / "1" / "Visualization_hi_pass").iterdir()}
    new = {p.name: p.read_bytes() for p in (results / "Visualization_hi_pass").iterdir()}
    assert old == new and not (tmp_path / "without" / "case" / "1" / "FlowMetrics").exists()


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------

def test_header_binding_and_kernel_source_agree():
    from vasp_amd import capi
    header = (ROOT / "include" / "vaspfsi.h").read_text()
    lib = capi.load_library()
    for name in ("fsi_band_cells", "fsi_band_cell_rate"):
        m = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S)
        assert m and name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
        comment = header[:m.start()].rsplit("/*", 1)[1]
        assert "Replaces: nothing in the reference; VaMPy's metrics on an FSI run" in comment, name
    for k, series in enumerate(hp.RATE_SERIES):
        assert re.search(r"#define FSI_RATE_%s %d\b" % (series.upper(), k), header) and capi.HipBackend.RATE_SERIES[series] == k
    src = (ROOT / "vasp_amd" / "csrc" / "fsi_rate.hip").read_text()
    assert "#pragma clang fp contract(off)" in src and "__launch_bounds__(256) void k_cell_rate" in src
    assert "__shared__" not in src and "atomic" not in src.lower().replace("no atomics", "")
    assert "fsi_rate.hip" in (ROOT / "vasp_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"\d+ VGPRs", (ROOT / "vasp_amd" / "csrc" / "fsi_rate.hpp").read_text())
