"""The strain rate of a recorded history on mesh cells on the device (csrc/fsi_rate.hip; fsi_band_cells, fsi_band_cell_rate;
HipBackend.hi_pass_cells / hi_pass_cell_rate; ``--hi-pass-flow-metrics``) against the NumPy twin (vasp_amd/hi_pass.py:
cell_rate, HostBandSession.cells / cell_rate), which tests/test_hi_pass_cell_rate.py holds to an extended-precision restatement.
The twin is handed the gradients the device formed (``grad_out``), and everything is compared bit for bit: the kernel is FP64
additions, multiplications and one true division in the twin's order, compiled without contraction.  The histories are filled
with hi_pass_import: no time step is taken but in the end-to-end run.

Not tested here: the refusal of a cell list that does not fit the device, which would need a nearly full device, and a
partitioned context, which needs several ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_hi_pass_cell_rate import EPS, bound
from vasp_amd import flow_metrics as fm
from vasp_amd import hi_pass as hp

pytestmark = pytest.mark.gpu

STENOSIS = GOLDEN / "offset_stenosis" / "offset_stenosis.h5"
SIZES = (1, 63, 65, 257)                         # one lane, either side of a wavefront, past a block of 256
CASES = ((4, 3), (3, 4))                         # (period, cycles): 12 frames


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[a == 0]), np.signbit(b[b == 0]))


@pytest.fixture(scope="module")
def hb(cylinder_case):
    from vasp_amd.capi import HipBackend
    backend = HipBackend(cylinder_case[1])
    yield backend
    backend.close()


@pytest.fixture(scope="module")
def mesh(cylinder_case):
    return cylinder_case[0]["mesh"]


def _frames(n, nodes, seed):
    """(n, nodes, 3): a pulsatile part and a fluctuation, with one -0.0."""
    rng = np.random.default_rng(seed)
    x = 0.3 * np.sin(0.7 * np.arange(n))[:, None, None] * rng.uniform(0.5, 1.5, (1, nodes, 3)) + 3e-3 * rng.standard_normal((n, nodes, 3))
    x[0, 0, 0] = -0.0
    return x


def _cells(mesh, n, seed=0):
    return np.sort(np.random.default_rng(seed).permutation(mesh.num_cells)[:n])


def _open(hb, mesh, x, cells, q="v"):
    """The session of q on every P2 node with the history x and the listed cells attached, and its host twin on the
    device's gradients."""
    hb.hi_pass_begin(q, np.arange(mesh.num_nodes, dtype=np.int32), None, len(x))
    hb.hi_pass_import(q, x)
    grad = hb.hi_pass_cells(q, cells)
    assert grad.shape == (len(cells), 4, 3) and np.isfinite(grad).all()
    twin = hp.HostBandSession(3, len(x))
    twin.import_(x)
    twin.cells(mesh.tet_nodes[cells], grad)
    return twin


def _compare(hb, twin, series, frames, period=None, q="v"):
    """Every single frame, the time mean and, with a period, every cycle mean of one series."""
    for k in range(frames):
        assert same_bits(hb.hi_pass_cell_rate(q, series, k, 1, 1), twin.cell_rate(series, k, 1, 1)), (series, k)
    assert same_bits(hb.hi_pass_cell_rate(q, series), twin.cell_rate(series)), series
    assert same_bits(hb.hi_pass_cell_rate(q, series, 0, 1, frames), twin.cell_rate(series, 0, 1, frames)), series
    if period:
        for j in range(period):
            assert same_bits(hb.hi_pass_cell_rate(q, series, j, period, frames // period), twin.cell_rate(series, j, period, frames // period)), (series, j)


@pytest.mark.parametrize("period,cycles", CASES, ids=[f"P{p}C{c}" for p, c in CASES])
@pytest.mark.parametrize("ncell", SIZES)
def test_device_equals_the_twin_bit_for_bit(hb, mesh, ncell, period, cycles):
    n = period * cycles
    x = _frames(n, mesh.num_nodes, 10 * ncell + period)
    cells = _cells(mesh, ncell, ncell)
    twin = _open(hb, mesh, x, cells)
    try:
        _compare(hb, twin, "raw", n, period)
        hb.hi_pass_phase("v", period)
        twin.phase(period)
        _compare(hb, twin, "raw", n, period)
        _compare(hb, twin, "series", n, period)
        _compare(hb, twin, "phase_mean", period)
        got = hb.hi_pass_cell_rate("v", "raw")
        assert got.shape == (ncell,) and (got > 0).all()
        assert same_bits(hb.hi_pass_export("v", 0, n), x)                               # the raw history is unchanged
    finally:
        hb.hi_pass_end("v")


@pytest.mark.parametrize("period,cycles", CASES, ids=[f"P{p}C{c}" for p, c in CASES])
@pytest.mark.parametrize("ncell", (65, 257))
def test_a_strided_view(hb, mesh, ncell, period, cycles):
    """select(first=2, stride=2): selected frame k is recorded frame 2 + 2 k; the raw series goes through the stride."""
    n = period * cycles
    x = _frames(2 + 2 * n + 1, mesh.num_nodes, 7 * ncell + cycles)
    cells = _cells(mesh, ncell, 3)
    twin = _open(hb, mesh, x, cells)
    try:
        assert hb.hi_pass_select("v", 2, n, 2) == n == twin.select(2, n, 2)             # the list survives the selection
        _compare(hb, twin, "raw", n, period)
        assert same_bits(hb.hi_pass_cell_rate("v", "raw", 1, 1, 1), hp.cell_rate(x[4][mesh.tet_nodes[cells]], twin.cell_grad))
        hb.hi_pass_phase("v", period)
        twin.phase(period)
        _compare(hb, twin, "series", n, period)
        _compare(hb, twin, "phase_mean", period)
        assert same_bits(hb.hi_pass_export("v", 0, len(x)), x)
    finally:
        hb.hi_pass_end("v")


@pytest.mark.parametrize("ncell", SIZES)
def test_a_history_of_one_frame(hb, mesh, ncell):
    x = _frames(1, mesh.num_nodes, ncell)
    cells = _cells(mesh, ncell, 5)
    twin = _open(hb, mesh, x, cells, "d")
    try:
        _compare(hb, twin, "raw", 1, q="d")
        assert same_bits(hb.hi_pass_cell_rate("d", "raw"), hp.cell_rate(x[0][mesh.tet_nodes[cells]], twin.cell_grad))      # the frame's own bits
        hb.hi_pass_phase("d", 1)
        twin.phase(1)
        _compare(hb, twin, "series", 1, 1, q="d")
        _compare(hb, twin, "phase_mean", 1, q="d")
        assert same_bits(hb.hi_pass_cell_rate("d", "series"), np.zeros(ncell))          # one cycle is its own mean: u' = +0
    finally:
        hb.hi_pass_end("d")


def test_a_shuffled_node_list_gives_the_same_bits(hb, mesh):
    x = _frames(4, mesh.num_nodes, 41)
    cells = _cells(mesh, 257, 7)
    twin = _open(hb, mesh, x, cells)
    try:
        want = [hb.hi_pass_cell_rate("v", "raw", k, 1, 1) for k in range(4)] + [hb.hi_pass_cell_rate("v", "raw")]
        grad = twin.cell_grad
    finally:
        hb.hi_pass_end("v")
    perm = np.random.default_rng(8).permutation(mesh.num_nodes).astype(np.int32)
    hb.hi_pass_begin("v", perm, None, 4)
    try:
        hb.hi_pass_import("v", x[:, perm])
        assert same_bits(hb.hi_pass_cells("v", cells), grad)
        got = [hb.hi_pass_cell_rate("v", "raw", k, 1, 1) for k in range(4)] + [hb.hi_pass_cell_rate("v", "raw")]
        assert all(same_bits(a, b) for a, b in zip(got, want))
        assert same_bits(want[4], twin.cell_rate("raw"))
    finally:
        hb.hi_pass_end("v")


def test_an_exactly_periodic_history_has_a_fluctuation_rate_of_plus_zero(hb, mesh):
    """Values of eleven bits: the sums over three and over four cycles and their divisions are exact, u' = x - x = +0.0."""
    for period, cycles in CASES:
        rng = np.random.default_rng(period)
        cycle = rng.integers(-1000, 1000, (period, mesh.num_nodes, 3)) / 1024.0
        x = np.tile(cycle, (cycles, 1, 1))
        twin = _open(hb, mesh, x, _cells(mesh, 257, 9))
        try:
            hb.hi_pass_phase("v", period)
            twin.phase(period)
            for args in ((), (5, 1, 1), (1, period, cycles)):
                got = hb.hi_pass_cell_rate("v", "series", *args)
                assert same_bits(got, np.zeros(257)) and not np.signbit(got).any()
            assert np.allclose(hb.hi_pass_cell_rate("v", "phase_mean"), hb.hi_pass_cell_rate("v", "raw"), rtol=1e-13, atol=0)      # the mean is the cycle itself
            assert (hb.hi_pass_cell_rate("v", "raw") > 0).all()
        finally:
            hb.hi_pass_end("v")


def test_a_nan_reaches_exactly_the_cells_of_its_node(hb, mesh):
    n = 6
    x = _frames(n, mesh.num_nodes, 51)
    cells = _cells(mesh, 257, 11)
    conn = mesh.tet_nodes[cells]
    node = int(conn[130, 7])                                                            # a mid-edge node of a listed cell
    hit = (conn == node).any(axis=1)
    assert 1 <= hit.sum() < 257
    twin = _open(hb, mesh, x, cells)
    try:
        clean = [hb.hi_pass_cell_rate("v", "raw", k, 1, 1) for k in range(n)] + [hb.hi_pass_cell_rate("v", "raw")]
    finally:
        hb.hi_pass_end("v")
    x[3, node, 1] = np.nan
    twin = _open(hb, mesh, x, cells)
    try:
        for k in range(n):
            got = hb.hi_pass_cell_rate("v", "raw", k, 1, 1)
            assert same_bits(got, twin.cell_rate("raw", k, 1, 1))
            if k != 3:
                assert same_bits(got, clean[k])
            else:
                assert np.isnan(got[hit]).all() and same_bits(got[~hit], clean[3][~hit])
        mean = hb.hi_pass_cell_rate("v", "raw")
        assert np.isnan(mean[hit]).all() and same_bits(mean[~hit], clean[n][~hit]) and same_bits(mean, twin.cell_rate("raw"))
        x[2, node, 0] = np.inf                                                          # an inf too: nothing is clamped
        hb.hi_pass_end("v")
        twin = _open(hb, mesh, x, cells)
        got = hb.hi_pass_cell_rate("v", "raw", 2, 1, 1)
        assert same_bits(got, twin.cell_rate("raw", 2, 1, 1)) and not np.isfinite(got[hit]).any() and np.isfinite(got[~hit]).all()
        assert same_bits(hb.hi_pass_export("v", 0, n), x)
    finally:
        hb.hi_pass_end("v")


def test_the_affine_known_answer_on_the_device(hb, mesh):
    """``w = A x + b`` at the P2 nodes has ``2 sym(A):sym(A)`` on every cell, within ``80 * 2^-53 * B_c`` (the bound of
    tests/test_hi_pass_cell_rate.py, formed with the device's gradients)."""
    rng = np.random.default_rng(61)
    A, b = rng.standard_normal((3, 3)), rng.standard_normal(3)
    x = (mesh.node_coords @ A.T + b)[None]
    cells = np.arange(mesh.num_cells)
    twin = _open(hb, mesh, x, cells)
    try:
        got = hb.hi_pass_cell_rate("v", "raw", 0, 1, 1)
        sym = 0.5 * (A + A.T)
        B = bound(x[0][mesh.tet_nodes[cells]], twin.cell_grad)
        err = np.abs(got - 2.0 * np.sum(sym * sym))
        print("affine field on the device: largest err / (2^-53 B_c):", (err / (EPS * B)).max())
        assert (err <= 80 * EPS * B).all()
        # the gradients the device uses are those of the mesh, to rounding
        assert np.allclose(twin.cell_grad, fm.barycentric_gradients(mesh, cells), rtol=1e-9, atol=1e-9 * np.abs(twin.cell_grad).max())
    finally:
        hb.hi_pass_end("v")


def _raw_cells(hb, q, cells, grad=True):
    """fsi_band_cells with library cell indices as they are: (return code, message)."""
    ci = np.ascontiguousarray(cells, dtype=np.int32)
    g = np.empty((max(len(ci), 1), 4, 3))
    rc = hb.lib.fsi_band_cells(hb.ctx, q, len(ci), ci.ctypes.data, g.ctypes.data if grad else None)
    return rc, hb.lib.fsi_last_error(hb.ctx).decode() if rc else ""


def test_every_refusal_has_its_message_and_leaves_the_list_in_place(hb, mesh, cylinder_case):
    from vasp_amd.capi import FsiError
    N2, V = mesh.num_nodes, mesh.num_vertices
    x = _frames(20, N2, 71)
    cells = _cells(mesh, 65, 13)
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_cells("v", cells)
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_cell_rate("v", "raw", 0, 1, 1)
    hb.hi_pass_begin("v", np.arange(N2, dtype=np.int32), None, 20)
    hb.hi_pass_begin("p", np.arange(V, dtype=np.int32), None, 2)
    solid = np.nonzero(np.asarray(cylinder_case[1]["cell_kind"]) == 1)[0][:3]
    hb.hi_pass_begin_cells("strain", solid, 2)
    try:
        hb.hi_pass_import("v", x)
        with pytest.raises(FsiError, match=r"no cell list \(fsi_band_cells first\)"):
            hb.hi_pass_cell_rate("v", "raw", 0, 1, 1)
        for q in ("p", "strain"):                                                       # p and the tensor quantities
            with pytest.raises(FsiError, match=r"fsi_band_cells: quantity must be 0 \(d\) or 1 \(v\)"):
                hb.hi_pass_cells(q, cells)
            assert hb.lib.fsi_band_cell_rate(hb.ctx, hb.BAND_QUANTITY[q], 0, 0, 1, 1, x.ctypes.data) == 1
            assert "quantity must be 0 (d) or 1 (v)" in hb.lib.fsi_last_error(hb.ctx).decode()
        rc, why = _raw_cells(hb, 1, [])
        assert rc == 1 and "needs n > 0 cells" in why
        for bad in (-1, mesh.num_cells):
            rc, why = _raw_cells(hb, 1, [0, bad, 1])
            assert rc == 1 and "cell out of range" in why
        with pytest.raises(FsiError, match=r"no cell list \(fsi_band_cells first\)"):    # the refused calls attached nothing
            hb.hi_pass_cell_rate("v", "raw", 0, 1, 1)
        twin = hp.HostBandSession(3, 20)
        twin.import_(x)
        twin.cells(mesh.tet_nodes[cells], hb.hi_pass_cells("v", cells))
        assert _raw_cells(hb, 1, hb.cell_u2i[cells], grad=False)[0] == 0                 # grad_out is nullable
        before = hb.hi_pass_cell_rate("v", "raw")
        assert same_bits(before, twin.cell_rate("raw"))
        # the calls on the series
        with pytest.raises(FsiError, match=r"no filtered series \(fsi_band_filter or fsi_band_phase first\)"):
            hb.hi_pass_cell_rate("v", "series", 0, 1, 1)
        with pytest.raises(FsiError, match=r"no phase average \(fsi_band_phase first\)"):
            hb.hi_pass_cell_rate("v", "phase_mean", 0, 1, 1)
        for first, step, count in ((0, 0, 1), (0, -1, 1), (0, 1, 0), (0, 1, -3)):
            with pytest.raises(FsiError, match="needs step >= 1 and count >= 1"):
                hb.hi_pass_cell_rate("v", "raw", first, step, count)
        for first, step, count in ((20, 1, 1), (-1, 1, 1), (0, 1, 21), (1, 10, 3), (19, 1, 2)):
            with pytest.raises(FsiError, match="fall outside the series of 20 frames") as e:
                hb.hi_pass_cell_rate("v", "raw", first, step, count)
            assert e.value.code == 1
        assert hb.lib.fsi_band_cell_rate(hb.ctx, 1, 0, 0, 1, 1, None) == 1 and "out is NULL" in hb.lib.fsi_last_error(hb.ctx).decode()
        assert hb.lib.fsi_band_cell_rate(hb.ctx, 1, 3, 0, 1, 1, x.ctypes.data) == 1 and "series must be" in hb.lib.fsi_last_error(hb.ctx).decode()
        # a cell list that is refused leaves the one that stands
        for bad in ([0, mesh.num_cells], []):
            assert _raw_cells(hb, 1, bad)[0] == 1
        assert same_bits(hb.hi_pass_cell_rate("v", "raw"), before)
        # the list survives a filter, a selection and a phase average; the filtered series is the twin's
        low = hp.design(1e-3, 0.0, 200.0)
        hb.hi_pass_filter("v", low["b"], low["a"], low["zi"], low["padlen"])
        twin.filter(low["b"], low["a"], low["zi"], low["padlen"])
        _compare(hb, twin, "series", 20)
        assert hb.hi_pass_select("v", 0, 12, 1) == 12 == twin.select(0, 12, 1)
        with pytest.raises(FsiError, match="no filtered series"):
            hb.hi_pass_cell_rate("v", "series")
        hb.hi_pass_phase("v", 4)
        twin.phase(4)
        with pytest.raises(FsiError, match="fall outside the series of 4 frames"):
            hb.hi_pass_cell_rate("v", "phase_mean", 4, 1, 1)
        with pytest.raises(FsiError, match="fall outside the series of 12 frames"):
            hb.hi_pass_cell_rate("v", "series", 0, 1, 13)
        _compare(hb, twin, "series", 12, 4)
        _compare(hb, twin, "phase_mean", 4)
        # a second call replaces the list
        other = _cells(mesh, 7, 17)
        twin.cells(mesh.tet_nodes[other], hb.hi_pass_cells("v", other))
        assert hb.hi_pass_cell_rate("v", "raw").shape == (7,) and same_bits(hb.hi_pass_cell_rate("v", "raw"), twin.cell_rate("raw"))
    finally:
        hb.hi_pass_end("p")
        hb.hi_pass_end("strain")
    # fsi_band_begin frees the list, fsi_band_end too
    hb.hi_pass_begin("v", np.arange(N2, dtype=np.int32), None, 2)
    try:
        hb.hi_pass_import("v", x[:2])
        with pytest.raises(FsiError, match=r"no cell list \(fsi_band_cells first\)"):
            hb.hi_pass_cell_rate("v", "raw", 0, 1, 1)
    finally:
        hb.hi_pass_end("v")
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_cell_rate("v", "raw", 0, 1, 1)


def test_a_session_must_hold_every_node_of_a_cell_as_its_own_row(hb, mesh):
    """A session on the vertices only, and one whose row of a node is the mean of two: refused with the first such cell and
    node.  A node listed twice: its first occurrence is used."""
    from vasp_amd.capi import FsiError
    N2, V = mesh.num_nodes, mesh.num_vertices
    cells = _cells(mesh, 63, 19)
    first_cell = int(hb.cell_u2i[cells[0]])
    hb.hi_pass_begin("v", np.arange(V, dtype=np.int32), None, 1)                         # what save_deg 1 records
    try:
        with pytest.raises(FsiError) as e:
            hb.hi_pass_cells("v", cells)
        assert f"cell {first_cell} (entry 0 of the list) has P2 node {mesh.tet_nodes[cells[0], 4]}, which is no node of the session" in str(e.value)
    finally:
        hb.hi_pass_end("v")
    node = int(mesh.tet_nodes[cells[2], 1])
    nodes_b = np.full(N2, -1, dtype=np.int32)
    nodes_b[node] = 0
    hb.hi_pass_begin("v", np.arange(N2, dtype=np.int32), nodes_b, 1)
    try:
        with pytest.raises(FsiError, match=f"has P2 node {node}, which is no node of the session"):
            hb.hi_pass_cells("v", cells)
    finally:
        hb.hi_pass_end("v")
    # N2 + 1 session nodes: node `node` once more at the end, with other values
    x = _frames(2, N2 + 1, 81)
    hb.hi_pass_begin("v", np.append(np.arange(N2), node).astype(np.int32), None, 2)
    try:
        hb.hi_pass_import("v", x)
        twin = hp.HostBandSession(3, 2)
        twin.import_(x)
        twin.cells(mesh.tet_nodes[cells], hb.hi_pass_cells("v", cells))                  # indices < N2: the first occurrence
        assert same_bits(hb.hi_pass_cell_rate("v", "raw"), twin.cell_rate("raw"))
    finally:
        hb.hi_pass_end("v")


# ---- end to end -------------------------------------------------------------------------------------------------------

def test_end_to_end_run_writes_the_metrics_of_the_frames_it_wrote(tmp_path, stenosis_case):
    """12 steps on the small stenosis mesh, every one saved, a cycle of 4 ms: three cycles of 4 frames, on the device in a fresh
    process.  The files hold one value per fluid cell: the closing formulas on the twin's rates of the velocity frames the run
    wrote, the twin being handed the gradients the device forms of the same mesh."""
    from test_hi_pass_cell_rate import PHASE_NAMES, _velocity, _vectors, expected_metrics
    from vasp_amd.capi import HipBackend
    options = ["--hi-pass", "v", "--hi-pass-phase-average", "--hi-pass-cycle", "0.004", "--hi-pass-flow-metrics"]
    results = tmp_path / "case" / "1"
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "vasp_amd.monolithic", "-p", "offset_stenosis", "-dt", "0.001", "-T", "0.0115",
           "--verbose", "False", "--folder", str(results.parent), "--sub-folder", "1", "--save-step", "1", "--save-deg", "2",
           "--checkpoint-step", "1000", *options, "--new-arguments", f"mesh_path={STENOSIS}"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "phase average over cycles 1 to 3 of 4 frames written" in r.stdout and "Flow metrics of" in r.stdout
    ns, desc = stenosis_case[0], stenosis_case[1]
    mesh = ns["mesh"]
    cells = fm.fluid_cells(mesh, ns["dx_f_id"])
    backend = HipBackend(desc)
    try:
        backend.hi_pass_begin("v", np.arange(mesh.num_nodes, dtype=np.int32), None, 1)
        grad = backend.hi_pass_cells("v", cells)
        backend.hi_pass_end("v")
    finally:
        backend.close()
    x = _velocity(results)
    assert x.shape == (12, mesh.num_nodes, 3) and x.dtype == np.float64
    got_cells, want = expected_metrics(mesh, dict(ns, dt=0.001), x, 4, grad)
    assert np.array_equal(got_cells, cells) and 0 < len(cells) < mesh.num_cells
    out = results / "FlowMetrics"
    names = ("strain_rate", "dissipation", "l_plus", "t_plus", *PHASE_NAMES)
    assert {p.name for p in out.iterdir()} == {f"{n}.{e}" for n in names for e in ("h5", "xdmf")} | {"flow_metrics.csv"}
    for name in names:
        got = _vectors(out / f"{name}.h5")
        assert got.shape == (4 if name.endswith("phase_mean") else 1, len(cells), 1), name
        assert np.array_equal(got[:, :, 0], np.atleast_2d(want[name]).astype(np.float32), equal_nan=True), name
    assert np.isfinite(want["strain_rate"]).all() and want["strain_rate"].max() > 0 and want["turbulent_dissipation"].max() > 0
    assert len((out / "flow_metrics.csv").read_text().splitlines()) == 1 + 11 + 4
