"""Q-criterion, enstrophy, helicity and kinetic energy of a recorded history on mesh cells on the device (csrc/fsi_vortex.hip;
fsi_band_cell_weights, fsi_band_cell_vortex; HipBackend.hi_pass_cell_weights / hi_pass_cell_vortex; ``--hi-pass-vortex``) against
the NumPy twin (vasp_amd/hi_pass.py: cell_vortex, cell_wsum, HostBandSession.cell_weights / cell_vortex), which
tests/test_hi_pass_vortex.py holds to an extended-precision restatement, the quadrature rule and known answers.  The twin is
handed the gradients the device formed, and everything is compared bit for bit, the sign of a zero included: the kernels are
FP64 additions, multiplications and one true division in the twin's order, compiled without contraction.  The histories are
filled with hi_pass_import: no time step is taken but in the end-to-end run.

Not tested here: the refusal of buffers that do not fit the device, which would need a nearly full device, and a partitioned
context, which needs several ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from vasp_amd import hi_pass as hp
from vasp_amd import vortex as vx

pytestmark = pytest.mark.gpu

CYL = GOLDEN / "cylinder" / "cylinder.h5"
SIZES = (1, 63, 65, 257)                         # one lane, either side of a wavefront, past a workgroup of 256
SUM_SIZES = (1, 63, 64, 65, 255, 256, 257, 513)  # every boundary of the sum's bracket: pair, wave, workgroup, two workgroups
CASES = ((4, 3), (3, 4))                         # (period, cycles): 12 frames
EPOCH = "1700000000"                             # h5lite stamps its headers with SOURCE_DATE_EPOCH where it is set


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
    assert mesh.num_cells >= n
    return np.sort(np.random.default_rng(seed).permutation(mesh.num_cells)[:n])


def _open(hb, mesh, x, cells, q="v"):
    """The session of q on every P2 node with the history x and the listed cells attached, and its host twin on the
    device's gradients."""
    hb.hi_pass_begin(q, np.arange(mesh.num_nodes, dtype=np.int32), None, len(x))
    hb.hi_pass_import(q, x)
    grad = hb.hi_pass_cells(q, cells)
    twin = hp.HostBandSession(3, len(x))
    twin.import_(x)
    twin.cells(mesh.tet_nodes[cells], grad)
    return twin


def _compare(hb, twin, series, frames, period=None):
    """Every single frame, the time mean, a strided selection of frames and, with a period, every cycle mean of one series: all
    five rows."""
    for k in range(frames):
        assert same_bits(hb.hi_pass_cell_vortex("v", series, k, 1, 1)[0], twin.cell_vortex(series, k, 1, 1)[0]), (series, k)
    assert same_bits(hb.hi_pass_cell_vortex("v", series)[0], twin.cell_vortex(series)[0]), series
    if frames > 2:
        args = (1, 2, (frames - 2) // 2 + 1)
        assert same_bits(hb.hi_pass_cell_vortex("v", series, *args)[0], twin.cell_vortex(series, *args)[0]), (series, args)
    if period:
        for j in range(period):
            args = (j, period, frames // period)
            assert same_bits(hb.hi_pass_cell_vortex("v", series, *args)[0], twin.cell_vortex(series, *args)[0]), (series, j)


@pytest.mark.parametrize("period,cycles", CASES, ids=[f"P{p}C{c}" for p, c in CASES])
@pytest.mark.parametrize("ncell", SIZES)
def test_device_equals_the_twin_bit_for_bit(hb, mesh, ncell, period, cycles):
    """24 recorded frames: the low-pass filtered series of all of them, then the raw frames, the fluctuation and the phase mean of
    the first 12, then a selection with a stride."""
    n = period * cycles
    x = _frames(24, mesh.num_nodes, 10 * ncell + period)
    cells = _cells(mesh, ncell, ncell)
    twin = _open(hb, mesh, x, cells)
    try:
        low = hp.design(1e-3, 0.0, 200.0)
        hb.hi_pass_filter("v", low["b"], low["a"], low["zi"], low["padlen"])
        twin.filter(low["b"], low["a"], low["zi"], low["padlen"])
        _compare(hb, twin, "series", 24)
        assert hb.hi_pass_select("v", 0, n, 1) == n == twin.select(0, n, 1)
        _compare(hb, twin, "raw", n, period)
        hb.hi_pass_phase("v", period)
        twin.phase(period)
        _compare(hb, twin, "raw", n, period)
        _compare(hb, twin, "series", n, period)
        _compare(hb, twin, "phase_mean", period)
        got = hb.hi_pass_cell_vortex("v", "raw")[0]
        assert got.shape == (5, ncell) and (got[1] > 0).all() and (got[4] > 0).all() and (got[3] >= np.abs(got[2])).all()
        assert hb.hi_pass_select("v", 2, 11, 2) == 11 == twin.select(2, 11, 2)            # selected frame k is recorded frame 2 + 2 k
        _compare(hb, twin, "raw", 11)
        assert same_bits(hb.hi_pass_cell_vortex("v", "raw", 1, 1, 1)[0], hp.cell_vortex(x[4][mesh.tet_nodes[cells]], twin.cell_grad))
        assert same_bits(hb.hi_pass_export("v", 0, 24), x)                                 # the raw history is unchanged
    finally:
        hb.hi_pass_end("v")


@pytest.mark.parametrize("ncell", SUM_SIZES)
def test_sums_equal_the_ordered_sum_bit_for_bit(hb, mesh, ncell):
    from vasp_amd.capi import FsiError
    x = _frames(3, mesh.num_nodes, ncell)
    cells = _cells(mesh, ncell, ncell + 1)
    assert len(cells) == ncell
    rng = np.random.default_rng(ncell)
    weights = rng.uniform(0.1, 3.0, ncell)
    if ncell >= 3:
        weights[ncell // 2], weights[ncell - 1] = 0.0, -0.0
    twin = _open(hb, mesh, x, cells)
    try:
        with pytest.raises(FsiError, match=r"fsi_band_cell_vortex: sums_out without weights \(fsi_band_cell_weights first\)"):
            hb.hi_pass_cell_vortex("v", "raw", sums=True)
        hb.hi_pass_cell_weights("v", weights)
        twin.cell_weights(weights)
        for args in ((0, 1, 1), (2, 1, 1), (0, 1, 3), (0, 2, 2)):
            none, alone = hb.hi_pass_cell_vortex("v", "raw", *args, cells=False, sums=True)
            got, sums = hb.hi_pass_cell_vortex("v", "raw", *args, cells=True, sums=True)
            want, want_sums = twin.cell_vortex("raw", *args, cells=True, sums=True)
            assert none is None and alone.shape == (5,) and same_bits(alone, sums)
            assert same_bits(got, want) and same_bits(sums, hp.cell_wsum(got, weights)) and same_bits(sums, want_sums), args
        if ncell == 1:                                                                     # a weight of -0.0: the sum is +0.0
            hb.hi_pass_cell_weights("v", np.array([-0.0]))
            sums = hb.hi_pass_cell_vortex("v", "raw", cells=False, sums=True)[1]
            assert same_bits(sums, np.zeros(5)) and same_bits(sums, hp.cell_wsum(twin.cell_vortex("raw")[0], np.array([-0.0])))
        # a second cell list drops the weights
        other = _cells(mesh, max(ncell - 1, 1), 3)
        twin.cells(mesh.tet_nodes[other], hb.hi_pass_cells("v", other))
        with pytest.raises(FsiError, match=r"sums_out without weights \(fsi_band_cell_weights first\)"):
            hb.hi_pass_cell_vortex("v", "raw", cells=False, sums=True)
        assert same_bits(hb.hi_pass_cell_vortex("v", "raw")[0], twin.cell_vortex("raw")[0])
        hb.hi_pass_cell_weights("v", np.ones(len(other)))
        assert same_bits(hb.hi_pass_cell_vortex("v", "raw", sums=True)[1], hp.cell_wsum(twin.cell_vortex("raw")[0], np.ones(len(other))))
        hb.hi_pass_cell_weights("v", None)                                                 # NULL drops them too
        with pytest.raises(FsiError, match="sums_out without weights"):
            hb.hi_pass_cell_vortex("v", "raw", sums=True)
    finally:
        hb.hi_pass_end("v")


def test_a_nan_reaches_exactly_the_cells_of_its_node_and_their_sums(hb, mesh):
    n = 4
    x = _frames(n, mesh.num_nodes, 51)
    cells = _cells(mesh, 257, 11)
    conn = mesh.tet_nodes[cells]
    node = int(conn[130, 7])                                                            # a mid-edge node of a listed cell
    hit = (conn == node).any(axis=1)
    assert 1 <= hit.sum() < 257
    weights = np.random.default_rng(5).uniform(0.5, 2.0, 257)
    twin = _open(hb, mesh, x, cells)
    try:
        hb.hi_pass_cell_weights("v", weights)
        clean = [hb.hi_pass_cell_vortex("v", "raw", k, 1, 1, True, True) for k in range(n)]
        assert all(np.isfinite(c).all() and np.isfinite(s).all() for c, s in clean)
    finally:
        hb.hi_pass_end("v")
    x[2, node, 1] = np.nan
    twin = _open(hb, mesh, x, cells)
    try:
        hb.hi_pass_cell_weights("v", weights)
        twin.cell_weights(weights)
        for k in range(n):
            got, sums = hb.hi_pass_cell_vortex("v", "raw", k, 1, 1, True, True)
            want, want_sums = twin.cell_vortex("raw", k, 1, 1, True, True)
            assert same_bits(got, want) and same_bits(sums, want_sums)
            if k != 2:
                assert same_bits(got, clean[k][0]) and same_bits(sums, clean[k][1])
            else:
                assert np.isnan(got[:, hit]).all() and same_bits(got[:, ~hit], clean[2][0][:, ~hit]) and np.isnan(sums).all()
        mean, sums = hb.hi_pass_cell_vortex("v", "raw", cells=True, sums=True)
        assert np.isnan(mean[:, hit]).all() and np.isfinite(mean[:, ~hit]).all() and np.isnan(sums).all()
        assert same_bits(mean, twin.cell_vortex("raw")[0])
        hb.hi_pass_end("v")
        x[2, node, 1] = np.inf                                                          # an inf: nothing is clamped
        twin = _open(hb, mesh, x, cells)
        hb.hi_pass_cell_weights("v", weights)
        twin.cell_weights(weights)
        got, sums = hb.hi_pass_cell_vortex("v", "raw", 2, 1, 1, True, True)
        want, want_sums = twin.cell_vortex("raw", 2, 1, 1, True, True)
        assert same_bits(got, want) and same_bits(sums, want_sums)
        assert not np.isfinite(got[:, hit]).any() and np.isfinite(got[:, ~hit]).all() and not np.isfinite(sums).any()
        assert same_bits(hb.hi_pass_export("v", 0, n), x)
    finally:
        hb.hi_pass_end("v")


def test_every_refusal_has_its_message_and_changes_nothing(hb, mesh, cylinder_case):
    from vasp_amd.capi import FsiError
    N2, V = mesh.num_nodes, mesh.num_vertices
    x = _frames(12, N2, 71)
    cells = _cells(mesh, 65, 13)
    out, sums = np.empty((5, 65)), np.empty(5)
    raw = lambda q, series, first, step, count, c=True, s=False: (
        hb.lib.fsi_band_cell_vortex(hb.ctx, q, series, first, step, count, out.ctypes.data if c else None, sums.ctypes.data if s else None),
        hb.lib.fsi_last_error(hb.ctx).decode())
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_cell_vortex("v", "raw", 0, 1, 1)
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_cell_weights("v", None)
    hb.hi_pass_begin("v", np.arange(N2, dtype=np.int32), None, 12)
    hb.hi_pass_begin("p", np.arange(V, dtype=np.int32), None, 2)
    try:
        hb.hi_pass_import("v", x)
        with pytest.raises(FsiError, match=r"fsi_band_cell_vortex: no cell list \(fsi_band_cells first\)"):
            hb.hi_pass_cell_vortex("v", "raw", 0, 1, 1)
        with pytest.raises(FsiError, match=r"fsi_band_cell_weights: no cell list \(fsi_band_cells first\)"):
            hb.hi_pass_cell_weights("v", np.ones(65))
        rc, why = raw(hb.BAND_QUANTITY["p"], 0, 0, 1, 1)
        assert rc == 1 and why == "fsi_band_cell_vortex: quantity must be 0 (d) or 1 (v)"
        assert hb.lib.fsi_band_cell_weights(hb.ctx, hb.BAND_QUANTITY["p"], sums.ctypes.data) == 1
        assert hb.lib.fsi_last_error(hb.ctx).decode() == "fsi_band_cell_weights: quantity must be 0 (d) or 1 (v)"
        twin = hp.HostBandSession(3, 12)
        twin.import_(x)
        twin.cells(mesh.tet_nodes[cells], hb.hi_pass_cells("v", cells))
        weights = np.random.default_rng(3).uniform(0.5, 2.0, 65)
        hb.hi_pass_cell_weights("v", weights)
        twin.cell_weights(weights)
        rate = hb.hi_pass_cell_rate("v", "raw")
        before = hb.hi_pass_cell_vortex("v", "raw", cells=True, sums=True)
        assert same_bits(before[0], twin.cell_vortex("raw")[0]) and same_bits(before[1], twin.cell_vortex("raw", sums=True)[1])
        for args, text in (((1, 3, 0, 1, 1), "series must be FSI_RATE_RAW, FSI_RATE_SERIES or FSI_RATE_PHASE_MEAN"),
                           ((1, 1, 0, 1, 1), "no filtered series (fsi_band_filter or fsi_band_phase first)"),
                           ((1, 2, 0, 1, 1), "no phase average (fsi_band_phase first)"),
                           ((1, 0, 0, 1, 1, False, False), "cells_out and sums_out are both NULL"),
                           ((1, 0, 0, 0, 1), "needs step >= 1 and count >= 1, got step = 0, count = 1"),
                           ((1, 0, 0, 1, 0), "needs step >= 1 and count >= 1, got step = 1, count = 0"),
                           ((1, 0, 12, 1, 1), "frames 12, 12 + 1, ... (1 of them) fall outside the series of 12 frames"),
                           ((1, 0, -1, 1, 1), "frames -1, -1 + 1, ... (1 of them) fall outside the series of 12 frames"),
                           ((1, 0, 1, 6, 3), "frames 1, 1 + 6, ... (3 of them) fall outside the series of 12 frames")):
            rc, why = raw(*args)
            assert rc == 1 and why == "fsi_band_cell_vortex: " + text, args
        with pytest.raises(ValueError, match="64 weights, the session has 65 cells"):
            hb.hi_pass_cell_weights("v", np.ones(64))
        # the refused calls changed nothing: the strain rate and the five fields are their earlier bits, the weights stand
        assert same_bits(hb.hi_pass_cell_rate("v", "raw"), rate)
        again = hb.hi_pass_cell_vortex("v", "raw", cells=True, sums=True)
        assert same_bits(again[0], before[0]) and same_bits(again[1], before[1])
        # the same words for the phase mean's own length
        hb.hi_pass_phase("v", 4)
        rc, why = raw(1, 2, 4, 1, 1)
        assert rc == 1 and why == "fsi_band_cell_vortex: frames 4, 4 + 1, ... (1 of them) fall outside the series of 4 frames"
    finally:
        hb.hi_pass_end("p")
        hb.hi_pass_end("v")
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_cell_vortex("v", "raw", 0, 1, 1)


# ---- end to end -------------------------------------------------------------------------------------------------------

OPTIONS = ["--hi-pass", "v", "--hi-pass-phase-average", "--hi-pass-cycle", "0.004", "--hi-pass-vortex", "--hi-pass-vortex-series"]


def _tree(folder):
    return {str(p.relative_to(folder)): p.read_bytes() for p in sorted(folder.rglob("*")) if p.is_file()}


def _child(tmp_path, module, arguments):
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""), SOURCE_DATE_EPOCH=EPOCH)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", module, *arguments], cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_end_to_end_run_and_postprocess_write_what_the_twin_writes(tmp_path, hb, mesh, cylinder_case, monkeypatch):
    """8 saved steps of the cylinder problem on the device in a fresh process, two cycles of 4 frames.  Every file under
    VortexMetrics/ is byte for byte what ``vortex.VortexMetrics`` writes on the host from the twin on the velocity frames the
    run wrote, the twin being handed the gradients the device forms of the same mesh; ``vasp_amd.postprocess`` on the finished
    folder, in a second process, writes the same bytes."""
    from test_hi_pass_cell_rate import _vectors
    results = tmp_path / "run" / "case" / "1"
    stdout = _child(tmp_path, "vasp_amd.monolithic",
                    ["-p", "cylinder", "-dt", "0.001", "-T", "0.0075", "--verbose", "False", "--folder", str(results.parent), "--sub-folder", "1",
                     "--save-step", "1", "--save-deg", "2", "--checkpoint-step", "1000", *OPTIONS, "--new-arguments", f"mesh_path={CYL}"])
    assert "phase average over cycles 1 to 2 of 4 frames written" in stdout and "Vortex metrics of" in stdout
    x = _vectors(results / "Visualization" / "velocity.h5")
    assert x.shape == (8, mesh.num_nodes, 3) and x.dtype == np.float64
    ns = dict(cylinder_case[0], results_folder=tmp_path / "twin", hi_pass_vortex=True, hi_pass_vortex_series=True)
    monkeypatch.setenv("SOURCE_DATE_EPOCH", EPOCH)
    metrics = vx.VortexMetrics(mesh, ns)
    hb.hi_pass_begin("v", np.arange(mesh.num_nodes, dtype=np.int32), None, 1)
    try:
        grad = hb.hi_pass_cells("v", metrics.cells)
    finally:
        hb.hi_pass_end("v")
    s = hp.HostBandSession(3, 8)
    s.import_(x)
    s.select(0, 8, 1)
    metrics.attach(s, False, grad)
    metrics.collect(s, 8, 0.001, 0.0)
    s.phase(4)
    metrics.collect_phase(s, 4)
    metrics.write(lambda line: None, 0.001, 0.0)
    got, want = _tree(results / "VortexMetrics"), _tree(tmp_path / "twin" / "VortexMetrics")
    assert sorted(got) == sorted(want) and len(got) == 2 * 12 + 3
    for name in want:
        assert got[name] == want[name], name
    assert 0 < len(metrics.cells) < mesh.num_cells and np.isfinite(metrics.mean).all() and metrics.mean[1].max() > 0
    # the finished folder through vasp_amd.postprocess, into a folder of its own
    stdout = _child(tmp_path, "vasp_amd.postprocess", ["--folder", str(results), "--output-folder", str(tmp_path / "post"), *OPTIONS])
    assert "Vortex metrics of" in stdout
    post = _tree(tmp_path / "post" / "VortexMetrics")
    assert sorted(post) == sorted(want)
    for name in want:
        assert post[name] == want[name], name
