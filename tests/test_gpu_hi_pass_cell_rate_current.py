"""The strain rate of a recorded history in the current configuration on the device (k_cell_rate_current, csrc/fsi_rate.hip;
fsi_band_cell_rate_current; HipBackend.hi_pass_cell_rate_current; ``--hi-pass-flow-metrics-configuration current``) against
the NumPy twin (hi_pass.cell_rate_current, HostBandSession.cell_rate_current), which tests/test_hi_pass_cell_rate_current.py
holds to an extended-precision restatement.  The twin is handed the gradients the device formed, and the three results - rate,
volume ratio, smallest det F - are compared bit for bit.  The histories are filled with hi_pass_import: no time step is taken
but in the end-to-end runs.

Not tested here: the refusal of result buffers that do not fit the device, which would need a nearly full device, and a
partitioned context, which needs several ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_gpu_hi_pass_cell_rate import CASES, SIZES, _cells, _frames, same_bits
from vasp_amd import flow_metrics as fm
from vasp_amd import hi_pass as hp

pytestmark = pytest.mark.gpu

CYL = GOLDEN / "cylinder" / "cylinder.h5"
FILTER = (np.array([0.6, 0.4]), np.array([1.0, -0.2]), np.array([0.1]), 3)       # one band on 12 frames: two taps, padlen 3


@pytest.fixture(scope="module")
def hb(cylinder_case):
    from vasp_amd.capi import HipBackend
    backend = HipBackend(cylinder_case[1])
    yield backend
    backend.close()


@pytest.fixture(scope="module")
def mesh(cylinder_case):
    return cylinder_case[0]["mesh"]


def _displacements(mesh, n, seed):
    """(n, N2, 3): a smooth breathing of a few percent that changes from frame to frame, plus noise of 0.2 % of a cell."""
    rng = np.random.default_rng(seed)
    X = mesh.node_coords
    amp = 0.04 * np.sin(0.8 * np.arange(n) + 0.3)[:, None]
    d = np.stack([amp * X[:, 0], 0.3 * amp * X[:, 1], amp * X[:, 2]], axis=-1)
    return d + 2e-7 * rng.standard_normal(d.shape)


def _open(hb, mesh, x, d, cells, q="v"):
    """The sessions of d and of q on every P2 node with their histories, the listed cells attached to q, and the host twins
    (field, geometry) on the device's gradients."""
    nodes = np.arange(mesh.num_nodes, dtype=np.int32)
    hb.hi_pass_begin("d", nodes, None, len(d))
    hb.hi_pass_import("d", d)
    if q != "d":
        hb.hi_pass_begin(q, nodes, None, len(x))
        hb.hi_pass_import(q, x)
    grad = hb.hi_pass_cells(q, cells)
    geo = hp.HostBandSession(3, len(d))
    geo.import_(d)
    twin = geo
    if q != "d":
        twin = hp.HostBandSession(3, len(x))
        twin.import_(x)
    twin.cells(mesh.tet_nodes[cells], grad)
    return twin, geo


def _close(hb, *quantities):
    for q in quantities:
        hb.hi_pass_end(q)


def _same(got, want) -> bool:
    return len(got) == len(want) == 3 and all(same_bits(a, b) for a, b in zip(got, want))


def _compare(hb, twin, geo, series, frames, period=None, q="v"):
    """Every single frame, the time mean, a strided selection and, with a period, every cycle mean of one series."""
    for k in range(frames):
        assert _same(hb.hi_pass_cell_rate_current(q, series, k, 1, 1), twin.cell_rate_current(series, geo, k, 1, 1)), (series, k)
    assert _same(hb.hi_pass_cell_rate_current(q, series), twin.cell_rate_current(series, geo)), series
    if frames > 2:
        assert _same(hb.hi_pass_cell_rate_current(q, series, 1, 2), twin.cell_rate_current(series, geo, 1, 2)), series
    if period:
        for j in range(period):
            assert _same(hb.hi_pass_cell_rate_current(q, series, j, period, frames // period),
                         twin.cell_rate_current(series, geo, j, period, frames // period)), (series, j)


@pytest.mark.parametrize("period,cycles", CASES, ids=[f"P{p}C{c}" for p, c in CASES])
@pytest.mark.parametrize("ncell", SIZES)
def test_device_equals_the_twin_bit_for_bit(hb, mesh, ncell, period, cycles):
    n = period * cycles
    x, d = _frames(n, mesh.num_nodes, 10 * ncell + period), _displacements(mesh, n, ncell + period)
    cells = _cells(mesh, ncell, ncell)
    twin, geo = _open(hb, mesh, x, d, cells)
    try:
        _compare(hb, twin, geo, "raw", n, period)
        rate, volume_ratio, min_jacobian = hb.hi_pass_cell_rate_current("v", "raw")
        assert rate.shape == (ncell,) and (rate > 0).all() and (np.abs(volume_ratio - 1.0) < 0.2).all() and (volume_ratio != 1.0).all()
        assert (min_jacobian > 0.7).all() and (min_jacobian < volume_ratio).all()
        assert not same_bits(rate, hb.hi_pass_cell_rate("v", "raw"))                    # the undeformed rate is another number
        # the filtered series after one band: paired with the raw d frames
        hb.hi_pass_filter("v", *FILTER)
        twin.filter(*FILTER)
        _compare(hb, twin, geo, "series", n, period)
        # a strided selection of both, and the phase average
        for s in ("v", "d"):
            assert hb.hi_pass_select(s, 1, n // 2, 2) == n // 2
        twin.select(1, n // 2, 2)
        geo.select(1, n // 2, 2)
        _compare(hb, twin, geo, "raw", n // 2)
        for s in ("v", "d"):
            assert hb.hi_pass_select(s, 0, n, 1) == n
            hb.hi_pass_phase(s, period)
        for a in (twin, geo):
            a.select(0, n, 1)
            a.phase(period)
        _compare(hb, twin, geo, "raw", n, period)
        _compare(hb, twin, geo, "series", n, period)
        _compare(hb, twin, geo, "phase_mean", period)
        assert same_bits(hb.hi_pass_export("v", 0, n), x) and same_bits(hb.hi_pass_export("d", 0, n), d)      # the histories are unchanged
    finally:
        _close(hb, "v", "d")


def test_the_displacement_itself_as_the_field(hb, mesh):
    """quantity 0: the field and the geometry are the same session."""
    d = _displacements(mesh, 6, 23)
    cells = _cells(mesh, 65, 5)
    twin, geo = _open(hb, mesh, None, d, cells, "d")
    try:
        assert twin is geo
        _compare(hb, twin, geo, "raw", 6, q="d")
        hb.hi_pass_phase("d", 3)
        twin.phase(3)
        _compare(hb, twin, geo, "series", 6, 3, q="d")
        _compare(hb, twin, geo, "phase_mean", 3, q="d")
    finally:
        _close(hb, "d")


def test_the_pairing_does_not_follow_the_selection_of_d(hb, mesh):
    """After the cells are attached the d session's selection moves on: RAW and SERIES results keep their bits - they take
    the recorded d frames at the field's absolute indices -, PHASE_MEAN is refused."""
    from vasp_amd.capi import FsiError
    n = 12
    x, d = _frames(n, mesh.num_nodes, 91), _displacements(mesh, n, 92)
    cells = _cells(mesh, 65, 21)
    twin, geo = _open(hb, mesh, x, d, cells)
    try:
        assert hb.hi_pass_select("v", 2, 4, 2) == 4 == twin.select(2, 4, 2)
        hb.hi_pass_phase("v", 2)
        twin.phase(2)
        raw, series = hb.hi_pass_cell_rate_current("v", "raw"), hb.hi_pass_cell_rate_current("v", "series", 1, 2, 2)
        assert _same(raw, twin.cell_rate_current("raw", geo)) and _same(series, twin.cell_rate_current("series", geo, 1, 2, 2))
        one = hp.cell_rate_current(x[8][mesh.tet_nodes[cells]], d[8][mesh.tet_nodes[cells]], twin.cell_grad)
        assert _same(hb.hi_pass_cell_rate_current("v", "raw", 3, 1, 1), one)          # selected frame 3 is recorded frame 8, of d too
        assert hb.hi_pass_select("d", 1, 3, 3) == 3
        hb.hi_pass_filter("d", *FILTER[:3], 0)
        assert _same(hb.hi_pass_cell_rate_current("v", "raw"), raw) and _same(hb.hi_pass_cell_rate_current("v", "series", 1, 2, 2), series)
        with pytest.raises(FsiError, match=r"fsi_band_cell_rate_current: the session of d has no phase average \(fsi_band_phase of d first\)"):
            hb.hi_pass_cell_rate_current("v", "phase_mean")
        hb.hi_pass_phase("d", 3)
        with pytest.raises(FsiError, match="the phase average of d has a period of 3 frames, that of the quantity 2"):
            hb.hi_pass_cell_rate_current("v", "phase_mean")
        assert hb.hi_pass_select("d", 0, 4, 2) == 4
        hb.hi_pass_phase("d", 2)
        with pytest.raises(FsiError, match="the phase average of d is over another selection of frames"):
            hb.hi_pass_cell_rate_current("v", "phase_mean")
        assert _same(hb.hi_pass_cell_rate_current("v", "raw"), raw)
        assert hb.hi_pass_select("d", 2, 4, 2) == 4 == geo.select(2, 4, 2)
        hb.hi_pass_phase("d", 2)
        geo.phase(2)
        assert _same(hb.hi_pass_cell_rate_current("v", "phase_mean"), twin.cell_rate_current("phase_mean", geo))
    finally:
        _close(hb, "v", "d")


def test_special_values_go_through_as_in_the_twin(hb, mesh):
    """A NaN in one d node and in one v node reach the cells of those nodes only; a cell with a vertex pushed through its
    opposite face has a negative smallest det F.  Plain arithmetic on finite or NaN inputs."""
    n = 6
    x, d = _frames(n, mesh.num_nodes, 51), _displacements(mesh, n, 52)
    cells = _cells(mesh, 257, 11)
    conn = mesh.tet_nodes[cells]
    twin, geo = _open(hb, mesh, x, d, cells)
    try:
        clean = hb.hi_pass_cell_rate_current("v", "raw")
        assert _same(clean, twin.cell_rate_current("raw", geo)) and all(np.isfinite(a).all() for a in clean)
    finally:
        _close(hb, "v", "d")
    node_d, node_v = int(conn[130, 7]), int(conn[20, 1])
    flipped = int(conn[200, 0])
    hit_d, hit_v, hit_f = ((conn == k).any(axis=1) for k in (node_d, node_v, flipped))
    x[3, node_v, 1] = np.nan
    d[2, node_d, 0] = np.nan
    X = mesh.node_coords
    d[4, flipped] = 2.5 * (X[conn[200, 1:4]].mean(axis=0) - X[flipped])
    twin, geo = _open(hb, mesh, x, d, cells)
    try:
        got = hb.hi_pass_cell_rate_current("v", "raw")
        assert _same(got, twin.cell_rate_current("raw", geo))
        for k in range(n):
            assert _same(hb.hi_pass_cell_rate_current("v", "raw", k, 1, 1), twin.cell_rate_current("raw", geo, k, 1, 1)), k
        untouched = ~(hit_d | hit_v | hit_f)
        assert untouched.sum() > 150 and all(same_bits(a[untouched], b[untouched]) for a, b in zip(got, clean))
        assert np.isnan(got[0][hit_d | hit_v]).all() and np.isnan(got[1][hit_d]).all()
        assert np.isfinite(got[2]).all()                                                # a NaN never replaces the minimum
        assert got[2][200] < 0 and (got[2][~hit_f] > 0).all()
        assert same_bits(hb.hi_pass_export("v", 0, n), x) and same_bits(hb.hi_pass_export("d", 0, n), d)
    finally:
        _close(hb, "v", "d")


def _raw_call(hb, q, series, first, step, count, n, outputs=(True, True, True)):
    """fsi_band_cell_rate_current as it is: (return code, message, the three arrays or None)."""
    arrays = [np.full(n, -7.0) if on else None for on in outputs]
    rc = hb.lib.fsi_band_cell_rate_current(hb.ctx, q, series, first, step, count, *(a.ctypes.data if a is not None else None for a in arrays))
    return rc, hb.lib.fsi_last_error(hb.ctx).decode() if rc else "", arrays


def test_every_refusal_has_its_message_and_changes_nothing(hb, mesh):
    from vasp_amd.capi import FsiError
    N2, V = mesh.num_nodes, mesh.num_vertices
    n = 8
    x, d = _frames(n, N2, 71), _displacements(mesh, n, 72)
    cells = _cells(mesh, 65, 13)
    nodes = np.arange(N2, dtype=np.int32)
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_cell_rate_current("v", "raw", 0, 1, 1)
    hb.hi_pass_begin("v", nodes, None, n)
    hb.hi_pass_begin("p", np.arange(V, dtype=np.int32), None, 2)
    try:
        hb.hi_pass_import("v", x)
        with pytest.raises(FsiError, match=r"fsi_band_cell_rate_current: no cell list \(fsi_band_cells first\)"):
            hb.hi_pass_cell_rate_current("v", "raw", 0, 1, 1)
        rc, why, _ = _raw_call(hb, hb.BAND_QUANTITY["p"], 0, 0, 1, 1, 65)
        assert rc == 1 and "fsi_band_cell_rate_current: quantity must be 0 (d) or 1 (v)" in why
        grad = hb.hi_pass_cells("v", cells)
        before = hb.hi_pass_cell_rate("v", "raw")
        # the refusals fsi_band_cell_rate has, in its words
        assert _raw_call(hb, 1, 3, 0, 1, 1, 65)[1].endswith("series must be FSI_RATE_RAW, FSI_RATE_SERIES or FSI_RATE_PHASE_MEAN")
        with pytest.raises(FsiError, match=r"no filtered series \(fsi_band_filter or fsi_band_phase first\)"):
            hb.hi_pass_cell_rate_current("v", "series", 0, 1, 1)
        with pytest.raises(FsiError, match=r"no phase average \(fsi_band_phase first\)"):
            hb.hi_pass_cell_rate_current("v", "phase_mean", 0, 1, 1)
        rc, why, _ = _raw_call(hb, 1, 0, 0, 1, 1, 65, (False, True, True))
        assert rc == 1 and why == "fsi_band_cell_rate_current: rate_out is NULL"
        for first, step, count in ((0, 0, 1), (0, -1, 1), (0, 1, 0), (0, 1, -3)):
            with pytest.raises(FsiError, match="needs step >= 1 and count >= 1"):
                hb.hi_pass_cell_rate_current("v", "raw", first, step, count)
        for first, step, count in ((8, 1, 1), (-1, 1, 1), (0, 1, 9), (1, 4, 3), (7, 1, 2)):
            with pytest.raises(FsiError, match="fall outside the series of 8 frames") as e:
                hb.hi_pass_cell_rate_current("v", "raw", first, step, count)
            assert e.value.code == 1
        # the session of d: none, other nodes, other frames
        with pytest.raises(FsiError, match=r"fsi_band_cell_rate_current: no session of quantity 0 \(d\)"):
            hb.hi_pass_cell_rate_current("v", "raw")
        perm = np.random.default_rng(3).permutation(N2).astype(np.int32)
        hb.hi_pass_begin("d", perm, None, n)
        hb.hi_pass_import("d", d[:, perm])
        with pytest.raises(FsiError, match="the session of d lists other nodes than the session of the quantity"):
            hb.hi_pass_cell_rate_current("v", "raw")
        hb.hi_pass_begin("d", nodes, None, n)
        hb.hi_pass_import("d", d[:7])
        with pytest.raises(FsiError, match="the session of d has recorded 7 frames, the session of the quantity 8"):
            hb.hi_pass_cell_rate_current("v", "raw")
        assert same_bits(hb.hi_pass_cell_rate("v", "raw"), before)                      # the refused calls changed nothing
        hb.hi_pass_import("d", d[7:])
        twin, geo = hp.HostBandSession(3, n), hp.HostBandSession(3, n)
        twin.import_(x)
        geo.import_(d)
        twin.cells(mesh.tet_nodes[cells], grad)
        want = twin.cell_rate_current("raw", geo)
        assert _same(hb.hi_pass_cell_rate_current("v", "raw"), want)
        # the two last outputs may be NULL
        for outputs in ((True, False, False), (True, True, False), (True, False, True)):
            rc, why, arrays = _raw_call(hb, 1, 0, 0, 1, n, 65, outputs)
            assert rc == 0, why
            assert all(a is None or same_bits(a, w) for a, w in zip(arrays, want))
        # the phase mean: refused, and fsi_band_cell_rate still returns its bits
        hb.hi_pass_phase("v", 4)
        with pytest.raises(FsiError, match="the session of d has no phase average"):
            hb.hi_pass_cell_rate_current("v", "phase_mean")
        assert same_bits(hb.hi_pass_cell_rate("v", "raw"), before)
        twin.phase(4)
        assert same_bits(hb.hi_pass_cell_rate("v", "phase_mean"), twin.cell_rate("phase_mean"))
        # a second cell list: the further results follow its size
        other = _cells(mesh, 7, 17)
        twin.cells(mesh.tet_nodes[other], hb.hi_pass_cells("v", other))
        assert _same(hb.hi_pass_cell_rate_current("v", "raw"), twin.cell_rate_current("raw", geo))
    finally:
        _close(hb, "p", "v", "d")
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_cell_rate_current("v", "raw", 0, 1, 1)


# ---- end to end -------------------------------------------------------------------------------------------------------

EPOCH = "1700000000"                             # h5lite stamps its headers with SOURCE_DATE_EPOCH where it is set


def _tree(folder):
    return {str(p.relative_to(folder)): p.read_bytes() for p in sorted(folder.rglob("*")) if p.is_file()}


def _device_run(tmp_path, name, options):
    """8 steps of the cylinder problem on the device in a fresh process, every one saved: (results folder, stdout)."""
    results = tmp_path / name / "case" / "1"
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""), SOURCE_DATE_EPOCH=EPOCH)
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "vasp_amd.monolithic", "-p", "cylinder", "-dt", "0.001", "-T", "0.0075",
           "--verbose", "False", "--folder", str(results.parent), "--sub-folder", "1", "--save-step", "1", "--save-deg", "2",
           "--checkpoint-step", "1000", "--hi-pass", "d", "v", "--hi-pass-phase-average", "--hi-pass-cycle", "0.004", *options,
           "--new-arguments", f"mesh_path={CYL}"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return results, r.stdout


def test_end_to_end_run_writes_what_the_twin_writes_from_the_same_frames(tmp_path, hb, mesh, cylinder_case, monkeypatch):
    """Two cycles of 4 frames.  Every file under FlowMetrics/ is byte for byte what ``FlowMetrics`` writes on the host from the
    twin's current-configuration rates of the displacement and velocity frames the run wrote, the twin being handed the
    gradients the device forms of the same mesh."""
    from test_hi_pass_cell_rate import _vectors
    results, stdout = _device_run(tmp_path, "current", ["--hi-pass-flow-metrics", "--hi-pass-flow-metrics-configuration", "current"])
    assert "phase average over cycles 1 to 2 of 4 frames written" in stdout and "in the current configuration" in stdout
    x, d = _vectors(results / "Visualization" / "velocity.h5"), _vectors(results / "Visualization" / "displacement.h5")
    assert x.shape == d.shape == (8, mesh.num_nodes, 3) and x.dtype == d.dtype == np.float64
    ns = dict(cylinder_case[0], dt=0.001, results_folder=tmp_path / "twin", hi_pass_flow_metrics_configuration="current")
    monkeypatch.setenv("SOURCE_DATE_EPOCH", EPOCH)
    metrics = fm.FlowMetrics(mesh, ns)
    hb.hi_pass_begin("v", np.arange(mesh.num_nodes, dtype=np.int32), None, 1)
    try:
        grad = hb.hi_pass_cells("v", metrics.cells)
    finally:
        hb.hi_pass_end("v")
    s, geo = hp.HostBandSession(3, 8), hp.HostBandSession(3, 8)
    s.import_(x)
    geo.import_(d)
    s.cells(mesh.tet_nodes[metrics.cells], grad)
    metrics.raw = metrics.rate(s, geo, "raw")
    for a in (geo, s):
        a.select(0, 8, 1)
        a.phase(4)
    metrics.phase = dict(fluctuation=metrics.rate(s, geo, "series"), mean=metrics.rate(s, geo, "phase_mean"),
                         cycle_mean=np.stack([metrics.rate(s, geo, "series", j, 4, 2) for j in range(4)]))
    metrics.write(lambda line: None, 0.001, 0.0)
    got, want = _tree(results / "FlowMetrics"), _tree(tmp_path / "twin" / "FlowMetrics")
    assert sorted(got) == sorted(want) and len(got) == 2 * 14 + 1
    for name in want:
        assert got[name] == want[name], name
    assert 0 < len(metrics.cells) < mesh.num_cells and np.isfinite(metrics.raw).all() and metrics.raw.max() > 0
    assert np.isfinite(metrics.volume_ratio).all() and (metrics.min_jacobian > 0).all()


def test_end_to_end_reference_is_a_run_without_the_option(tmp_path):
    with_word, _ = _device_run(tmp_path, "reference", ["--hi-pass-flow-metrics", "--hi-pass-flow-metrics-configuration", "reference"])
    without, _ = _device_run(tmp_path, "plain", ["--hi-pass-flow-metrics"])
    for sub in ("FlowMetrics", "Visualization_hi_pass"):
        a, b = _tree(with_word / sub), _tree(without / sub)
        assert a == b and len(a) > 4, sub
    assert not (with_word / "FlowMetrics" / "volume_ratio.h5").exists()
