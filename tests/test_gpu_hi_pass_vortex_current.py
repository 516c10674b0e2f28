"""Vortex metrics in the current configuration on the device (k_cell_vortex_current in csrc/fsi_vortex.hip;
fsi_band_cell_vortex_current; HipBackend.hi_pass_cell_vortex_current; ``--hi-pass-vortex-configuration current``) against the
NumPy twin (vasp_amd/hi_pass.py: cell_vortex_current, cell_wsum, HostBandSession.cell_vortex_current), which
tests/test_hi_pass_vortex_current.py holds to an extended-precision restatement, the rule's exactness and known answers.  The
twin is handed the gradients the device formed, and everything is compared bit for bit, the sign of a zero included: the kernel
is FP64 additions, multiplications and true divisions in the twin's order, compiled without contraction.  The histories are
filled with hi_pass_import: no time step is taken but in the end-to-end run.

Not tested here: the refusal of buffers that do not fit the device, which would need a nearly full device, and a partitioned
context, which needs several ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_gpu_hi_pass_cell_rate import CASES, SIZES, _cells, _frames, same_bits
from test_gpu_hi_pass_cell_rate_current import FILTER, _close, _displacements, _open
from vasp_amd import hi_pass as hp
from vasp_amd import vortex as vx

pytestmark = pytest.mark.gpu

CYL = GOLDEN / "cylinder" / "cylinder.h5"
EPOCH = "1700000000"                             # h5lite stamps its headers with SOURCE_DATE_EPOCH where it is set


@pytest.fixture(scope="module")
def hb(cylinder_case):
    from vasp_amd.capi import HipBackend
    backend = HipBackend(cylinder_case[1])
    yield backend
    backend.close()


@pytest.fixture(scope="module")
def mesh(cylinder_case):
    return cylinder_case[0]["mesh"]


def _weights(n, seed):
    w = np.random.default_rng(seed).uniform(0.1, 3.0, n)
    if n >= 3:
        w[n // 2], w[n - 1] = 0.0, -0.0
    return w


def _same(got, want) -> bool:
    """(cells, sums) of the device and of the twin: both present or both None, and the same bits."""
    return len(got) == len(want) == 2 and all((a is None and b is None) or (a is not None and b is not None and same_bits(a, b))
                                             for a, b in zip(got, want))


def _compare(hb, twin, geo, series, frames, period=None, q="v"):
    """Every single frame with its sums, the time mean with its sums, a strided selection and, with a period, every cycle mean
    of one series: the six means and the six sums of the numerators."""
    for k in range(frames):
        assert _same(hb.hi_pass_cell_vortex_current(q, series, k, 1, 1, True, True), twin.cell_vortex_current(series, geo, k, 1, 1, True, True)), (series, k)
    assert _same(hb.hi_pass_cell_vortex_current(q, series, cells=True, sums=True), twin.cell_vortex_current(series, geo, cells=True, sums=True)), series
    if frames > 2:
        assert _same(hb.hi_pass_cell_vortex_current(q, series, 1, 2), twin.cell_vortex_current(series, geo, 1, 2)), series
    if period:
        for j in range(period):
            args = (j, period, frames // period, False, True)
            assert _same(hb.hi_pass_cell_vortex_current(q, series, *args), twin.cell_vortex_current(series, geo, *args)), (series, j)


@pytest.mark.parametrize("period,cycles", CASES, ids=[f"P{p}C{c}" for p, c in CASES])
@pytest.mark.parametrize("ncell", SIZES)
def test_device_equals_the_twin_bit_for_bit(hb, mesh, ncell, period, cycles):
    """12 recorded frames of v and d: the raw frames, the filtered series after one band (paired with the raw d frames), a strided
    selection of both, then the fluctuation and the phase mean (paired with d's phase mean) - means and sums."""
    n = period * cycles
    x, d = _frames(n, mesh.num_nodes, 10 * ncell + period), _displacements(mesh, n, ncell + period)
    cells = _cells(mesh, ncell, ncell)
    weights = _weights(ncell, ncell)
    twin, geo = _open(hb, mesh, x, d, cells)
    try:
        hb.hi_pass_cell_weights("v", weights)
        twin.cell_weights(weights)
        _compare(hb, twin, geo, "raw", n, period)
        got, sums = hb.hi_pass_cell_vortex_current("v", "raw", cells=True, sums=True)
        assert got.shape == (6, ncell) and sums.shape == (6,) and (got[1] > 0).all() and (got[4] > 0).all() and (got[3] >= np.abs(got[2])).all()
        assert (np.abs(got[5] - 1.0) < 0.2).all() and (got[5] != 1.0).all()
        assert not same_bits(got[:5], hb.hi_pass_cell_vortex("v", "raw")[0])               # the undeformed fields are other numbers
        one = hp.cell_vortex_current(x[3][mesh.tet_nodes[cells]], d[3][mesh.tet_nodes[cells]], twin.cell_grad)
        alone = hb.hi_pass_cell_vortex_current("v", "raw", 3, 1, 1, True, True)
        assert same_bits(alone[0], one[0]) and same_bits(alone[1], hp.cell_wsum(one[1], weights))      # one frame: its own bits
        hb.hi_pass_filter("v", *FILTER)
        twin.filter(*FILTER)
        _compare(hb, twin, geo, "series", n, period)
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
        hb.hi_pass_cell_weights("d", np.ones(65))
        twin.cell_weights(np.ones(65))
        _compare(hb, twin, geo, "raw", 6, q="d")
        hb.hi_pass_phase("d", 3)
        twin.phase(3)
        _compare(hb, twin, geo, "series", 6, 3, q="d")
        _compare(hb, twin, geo, "phase_mean", 3, q="d")
    finally:
        _close(hb, "d")


def test_the_pairing_does_not_follow_the_selection_of_d(hb, mesh):
    """After the cells are attached the d session's selection moves on: RAW and SERIES results keep their bits - they take the
    recorded d frames at the field's absolute indices -, PHASE_MEAN is refused in the words of fsi_band_cell_rate_current."""
    from vasp_amd.capi import FsiError
    n = 12
    x, d = _frames(n, mesh.num_nodes, 91), _displacements(mesh, n, 92)
    cells = _cells(mesh, 65, 21)
    twin, geo = _open(hb, mesh, x, d, cells)
    call = lambda *a: hb.hi_pass_cell_vortex_current("v", *a, cells=True, sums=True)
    try:
        weights = _weights(65, 4)
        hb.hi_pass_cell_weights("v", weights)
        twin.cell_weights(weights)
        assert hb.hi_pass_select("v", 2, 4, 2) == 4 == twin.select(2, 4, 2)
        hb.hi_pass_phase("v", 2)
        twin.phase(2)
        raw, series = call("raw"), call("series", 1, 2, 2)
        assert _same(raw, twin.cell_vortex_current("raw", geo, cells=True, sums=True))
        assert _same(series, twin.cell_vortex_current("series", geo, 1, 2, 2, True, True))
        one = hp.cell_vortex_current(x[8][mesh.tet_nodes[cells]], d[8][mesh.tet_nodes[cells]], twin.cell_grad)
        assert same_bits(call("raw", 3, 1, 1)[0], one[0])                               # selected frame 3 is recorded frame 8, of d too
        assert hb.hi_pass_select("d", 1, 3, 3) == 3
        hb.hi_pass_filter("d", *FILTER[:3], 0)
        assert _same(call("raw"), raw) and _same(call("series", 1, 2, 2), series)
        with pytest.raises(FsiError, match=r"fsi_band_cell_vortex_current: the session of d has no phase average \(fsi_band_phase of d first\)"):
            call("phase_mean")
        hb.hi_pass_phase("d", 3)
        with pytest.raises(FsiError, match="fsi_band_cell_vortex_current: the phase average of d has a period of 3 frames, that of the quantity 2"):
            call("phase_mean")
        assert hb.hi_pass_select("d", 0, 4, 2) == 4
        hb.hi_pass_phase("d", 2)
        with pytest.raises(FsiError, match=r"fsi_band_cell_vortex_current: the phase average of d is over another selection of frames than that of the "
                                           r"quantity \(fsi_band_select and fsi_band_phase of d as of the quantity\)"):
            call("phase_mean")
        assert _same(call("raw"), raw)
        assert hb.hi_pass_select("d", 2, 4, 2) == 4 == geo.select(2, 4, 2)
        hb.hi_pass_phase("d", 2)
        geo.phase(2)
        assert _same(call("phase_mean"), twin.cell_vortex_current("phase_mean", geo, cells=True, sums=True))
    finally:
        _close(hb, "v", "d")


def test_special_values_go_through_as_in_the_twin(hb, mesh):
    """A NaN in one d node and in one v node reach the cells of those nodes only, and the sums; a cell turned inside out with
    its three edges has a negative volume ratio and finite fields.  Plain arithmetic on finite or NaN inputs."""
    n = 6
    x, d = _frames(n, mesh.num_nodes, 51), _displacements(mesh, n, 52)
    cells = _cells(mesh, 257, 11)
    conn = mesh.tet_nodes[cells]
    weights = np.random.default_rng(5).uniform(0.5, 2.0, 257)
    twin, geo = _open(hb, mesh, x, d, cells)
    try:
        hb.hi_pass_cell_weights("v", weights)
        twin.cell_weights(weights)
        clean = hb.hi_pass_cell_vortex_current("v", "raw", cells=True, sums=True)
        assert _same(clean, twin.cell_vortex_current("raw", geo, cells=True, sums=True)) and all(np.isfinite(a).all() for a in clean)
    finally:
        _close(hb, "v", "d")
    node_d, node_v = int(conn[130, 7]), int(conn[20, 1])
    moved = conn[200, [0, 7, 8, 9]]                                                      # vertex 0 and the mid-points of its three edges
    hit_d, hit_v, hit_f = (conn == node_d).any(axis=1), (conn == node_v).any(axis=1), np.isin(conn, moved).any(axis=1)
    x[3, node_v, 1] = np.nan
    d[2, node_d, 0] = np.nan
    X = mesh.node_coords
    d[4, moved] = 2.5 * (X[conn[200, 1:4]].mean(axis=0) - X[moved[0]]) * np.array([1.0, 0.5, 0.5, 0.5])[:, None]
    twin, geo = _open(hb, mesh, x, d, cells)
    try:
        hb.hi_pass_cell_weights("v", weights)
        twin.cell_weights(weights)
        got = hb.hi_pass_cell_vortex_current("v", "raw", cells=True, sums=True)
        assert _same(got, twin.cell_vortex_current("raw", geo, cells=True, sums=True))
        for k in range(n):
            assert _same(hb.hi_pass_cell_vortex_current("v", "raw", k, 1, 1, True, True), twin.cell_vortex_current("raw", geo, k, 1, 1, True, True)), k
        untouched = ~(hit_d | hit_v | hit_f)
        assert untouched.sum() > 150 and same_bits(got[0][:, untouched], clean[0][:, untouched])
        assert np.isnan(got[0][:5][:, hit_d | hit_v]).all() and np.isnan(got[0][5][hit_d]).all() and np.isnan(got[1]).all()
        only_v = hit_v & ~hit_d & ~hit_f
        assert same_bits(got[0][5][only_v], clean[0][5][only_v])                          # the volume is formed from d alone
        inverted = hb.hi_pass_cell_vortex_current("v", "raw", 4, 1, 1)[0]
        assert -1.7 < inverted[5, 200] < -1.3 and np.isfinite(inverted[:, 200]).all() and inverted[1, 200] > 0 and inverted[4, 200] > 0
        assert (inverted[5][~hit_f] > 0).all()
        assert same_bits(hb.hi_pass_export("v", 0, n), x) and same_bits(hb.hi_pass_export("d", 0, n), d)
    finally:
        _close(hb, "v", "d")


def _raw_call(hb, q, series, first, step, count, n, outputs=(True, True)):
    """fsi_band_cell_vortex_current as it is: (return code, message, the two arrays or None)."""
    arrays = [np.full((6, n), -7.0) if outputs[0] else None, np.full(6, -7.0) if outputs[1] else None]
    rc = hb.lib.fsi_band_cell_vortex_current(hb.ctx, q, series, first, step, count, *(a.ctypes.data if a is not None else None for a in arrays))
    return rc, hb.lib.fsi_last_error(hb.ctx).decode() if rc else "", arrays


def test_every_refusal_has_its_message_and_changes_nothing(hb, mesh):
    """Every refusal of fsi_band_cell_vortex and of fsi_band_cell_rate_current, under the new function's name; after them those
    two functions return their earlier bits, and the outputs of a refused call are untouched."""
    from vasp_amd.capi import FsiError
    N2, V = mesh.num_nodes, mesh.num_vertices
    n = 8
    fn = "fsi_band_cell_vortex_current: "
    x, d = _frames(n, N2, 71), _displacements(mesh, n, 72)
    cells = _cells(mesh, 65, 13)
    nodes = np.arange(N2, dtype=np.int32)
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_cell_vortex_current("v", "raw", 0, 1, 1)
    hb.hi_pass_begin("v", nodes, None, n)
    hb.hi_pass_begin("p", np.arange(V, dtype=np.int32), None, 2)
    try:
        hb.hi_pass_import("v", x)
        with pytest.raises(FsiError, match=r"fsi_band_cell_vortex_current: no cell list \(fsi_band_cells first\)"):
            hb.hi_pass_cell_vortex_current("v", "raw", 0, 1, 1)
        rc, why, _ = _raw_call(hb, hb.BAND_QUANTITY["p"], 0, 0, 1, 1, 65)
        assert rc == 1 and why == fn + "quantity must be 0 (d) or 1 (v)"
        grad = hb.hi_pass_cells("v", cells)
        weights = _weights(65, 3)
        rc, why, _ = _raw_call(hb, 1, 0, 0, 1, 1, 65)
        assert rc == 1 and why == fn + "sums_out without weights (fsi_band_cell_weights first)"
        hb.hi_pass_cell_weights("v", weights)
        rate = hb.hi_pass_cell_rate("v", "raw")
        vortex = hb.hi_pass_cell_vortex("v", "raw", cells=True, sums=True)
        # the refusals fsi_band_cell_vortex has, in its words
        for args, text in (((1, 3, 0, 1, 1), "series must be FSI_RATE_RAW, FSI_RATE_SERIES or FSI_RATE_PHASE_MEAN"),
                           ((1, 1, 0, 1, 1), "no filtered series (fsi_band_filter or fsi_band_phase first)"),
                           ((1, 2, 0, 1, 1), "no phase average (fsi_band_phase first)"),
                           ((1, 0, 0, 1, 1, 65, (False, False)), "cells_out and sums_out are both NULL"),
                           ((1, 0, 0, 0, 1), "needs step >= 1 and count >= 1, got step = 0, count = 1"),
                           ((1, 0, 0, 1, 0), "needs step >= 1 and count >= 1, got step = 1, count = 0"),
                           ((1, 0, 8, 1, 1), "frames 8, 8 + 1, ... (1 of them) fall outside the series of 8 frames"),
                           ((1, 0, -1, 1, 1), "frames -1, -1 + 1, ... (1 of them) fall outside the series of 8 frames"),
                           ((1, 0, 1, 4, 3), "frames 1, 1 + 4, ... (3 of them) fall outside the series of 8 frames")):
            rc, why, arrays = _raw_call(hb, *(args if len(args) > 5 else (*args, 65)))
            assert rc == 1 and why == fn + text, args
            assert all(a is None or (a == -7.0).all() for a in arrays)
        # the session of d: none, other nodes, other frames - the words of fsi_band_cell_rate_current
        rc, why, arrays = _raw_call(hb, 1, 0, 0, 1, 1, 65)
        assert rc == 1 and why == fn + "no session of quantity 0 (d): the current configuration is x = X + d (fsi_band_begin of d first)"
        assert all((a == -7.0).all() for a in arrays)
        perm = np.random.default_rng(3).permutation(N2).astype(np.int32)
        hb.hi_pass_begin("d", perm, None, n)
        hb.hi_pass_import("d", d[:, perm])
        rc, why, _ = _raw_call(hb, 1, 0, 0, 1, 1, 65)
        assert rc == 1 and why == fn + "the session of d lists other nodes than the session of the quantity: both must be opened on the same node list"
        hb.hi_pass_begin("d", nodes, None, n)
        hb.hi_pass_import("d", d[:7])
        rc, why, _ = _raw_call(hb, 1, 0, 0, 1, 1, 65)
        assert rc == 1 and why == fn + "the session of d has recorded 7 frames, the session of the quantity 8: both must hold the same frames"
        hb.hi_pass_import("d", d[7:])
        twin, geo = hp.HostBandSession(3, n), hp.HostBandSession(3, n)
        twin.import_(x)
        geo.import_(d)
        twin.cells(mesh.tet_nodes[cells], grad)
        twin.cell_weights(weights)
        want = twin.cell_vortex_current("raw", geo, cells=True, sums=True)
        assert _same(hb.hi_pass_cell_vortex_current("v", "raw", cells=True, sums=True), want)
        current = hb.hi_pass_cell_rate_current("v", "raw")
        # either output may be NULL
        for outputs in ((True, False), (False, True)):
            rc, why, arrays = _raw_call(hb, 1, 0, 0, 1, n, 65, outputs)
            assert rc == 0, why
            assert all(a is None or same_bits(a, w) for a, w in zip(arrays, want))
        # the phase mean: the d session has none, another period
        hb.hi_pass_phase("v", 4)
        with pytest.raises(FsiError, match=r"fsi_band_cell_vortex_current: the session of d has no phase average \(fsi_band_phase of d first\)"):
            hb.hi_pass_cell_vortex_current("v", "phase_mean")
        hb.hi_pass_phase("d", 2)
        with pytest.raises(FsiError, match="fsi_band_cell_vortex_current: the phase average of d has a period of 2 frames, that of the quantity 4"):
            hb.hi_pass_cell_vortex_current("v", "phase_mean")
        rc, why, _ = _raw_call(hb, 1, 2, 4, 1, 1, 65)
        assert rc == 1 and why == fn + "frames 4, 4 + 1, ... (1 of them) fall outside the series of 4 frames"
        # the refused calls changed nothing: the three earlier functions return their earlier bits, the weights stand
        assert same_bits(hb.hi_pass_cell_rate("v", "raw"), rate)
        again = hb.hi_pass_cell_vortex("v", "raw", cells=True, sums=True)
        assert same_bits(again[0], vortex[0]) and same_bits(again[1], vortex[1])
        assert all(same_bits(a, b) for a, b in zip(hb.hi_pass_cell_rate_current("v", "raw"), current))
        assert _same(hb.hi_pass_cell_vortex_current("v", "raw", cells=True, sums=True), want)
        # a second cell list: the buffers follow its size, the weights are dropped
        other = _cells(mesh, 7, 17)
        twin.cells(mesh.tet_nodes[other], hb.hi_pass_cells("v", other))
        with pytest.raises(FsiError, match=r"fsi_band_cell_vortex_current: sums_out without weights \(fsi_band_cell_weights first\)"):
            hb.hi_pass_cell_vortex_current("v", "raw", sums=True)
        assert same_bits(hb.hi_pass_cell_vortex_current("v", "raw")[0], twin.cell_vortex_current("raw", geo)[0])
    finally:
        _close(hb, "p", "v", "d")
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_cell_vortex_current("v", "raw", 0, 1, 1)


@pytest.mark.parametrize("ncell", (1, 65, 257, 513))
def test_the_five_field_sums_keep_their_bits(hb, mesh, ncell):
    """k_cell_wsum and k_cell_wsum_close take a field count now: with 5 fields the sums of fsi_band_cell_vortex are the ordered
    sums of ``hi_pass.cell_wsum`` as before, also after a call that ran them with 6."""
    x, d = _frames(3, mesh.num_nodes, ncell), _displacements(mesh, 3, ncell)
    cells = _cells(mesh, ncell, ncell + 1)
    weights = _weights(ncell, ncell)
    twin, geo = _open(hb, mesh, x, d, cells)
    try:
        hb.hi_pass_cell_weights("v", weights)
        twin.cell_weights(weights)
        for args in ((0, 1, 1), (0, 1, 3)):
            got, sums = hb.hi_pass_cell_vortex("v", "raw", *args, cells=True, sums=True)
            assert sums.shape == (5,) and same_bits(sums, hp.cell_wsum(got, weights)) and same_bits(sums, twin.cell_vortex("raw", *args, sums=True)[1])
            six = hb.hi_pass_cell_vortex_current("v", "raw", *args, cells=False, sums=True)[1]
            assert six.shape == (6,) and same_bits(six, twin.cell_vortex_current("raw", geo, *args, cells=False, sums=True)[1])
            assert same_bits(hb.hi_pass_cell_vortex("v", "raw", *args, cells=False, sums=True)[1], sums)
    finally:
        _close(hb, "v", "d")


# ---- end to end -------------------------------------------------------------------------------------------------------

def _tree(folder):
    return {str(p.relative_to(folder)): p.read_bytes() for p in sorted(folder.rglob("*")) if p.is_file()}


def test_end_to_end_run_writes_what_the_twin_writes_from_the_same_frames(tmp_path, hb, mesh, cylinder_case, monkeypatch):
    """8 saved steps of the cylinder problem on the device in a fresh process, two cycles of 4 frames, ``--hi-pass d v``.  Every
    file under VortexMetrics/ is byte for byte what ``vortex.VortexMetrics`` writes on the host from the twin on the displacement
    and velocity frames the run wrote, the twin being handed the gradients the device forms of the same mesh."""
    from test_hi_pass_cell_rate import _vectors
    results = tmp_path / "run" / "case" / "1"
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""), SOURCE_DATE_EPOCH=EPOCH)
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "vasp_amd.monolithic", "-p", "cylinder", "-dt", "0.001", "-T", "0.0075",
           "--verbose", "False", "--folder", str(results.parent), "--sub-folder", "1", "--save-step", "1", "--save-deg", "2",
           "--checkpoint-step", "1000", "--hi-pass", "d", "v", "--hi-pass-phase-average", "--hi-pass-cycle", "0.004", "--hi-pass-vortex",
           "--hi-pass-vortex-series", "--hi-pass-vortex-configuration", "current", "--new-arguments", f"mesh_path={CYL}"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "phase average over cycles 1 to 2 of 4 frames written" in r.stdout and "over 8 frames in the current configuration" in r.stdout
    x, d = _vectors(results / "Visualization" / "velocity.h5"), _vectors(results / "Visualization" / "displacement.h5")
    assert x.shape == d.shape == (8, mesh.num_nodes, 3) and x.dtype == d.dtype == np.float64
    ns = dict(cylinder_case[0], results_folder=tmp_path / "twin", hi_pass_vortex=True, hi_pass_vortex_series=True,
              hi_pass_vortex_configuration="current")
    monkeypatch.setenv("SOURCE_DATE_EPOCH", EPOCH)
    metrics = vx.VortexMetrics(mesh, ns)
    hb.hi_pass_begin("v", np.arange(mesh.num_nodes, dtype=np.int32), None, 1)
    try:
        grad = hb.hi_pass_cells("v", metrics.cells)
    finally:
        hb.hi_pass_end("v")
    s, geo = hp.HostBandSession(3, 8), hp.HostBandSession(3, 8)
    s.import_(x)
    geo.import_(d)
    for a in (geo, s):
        a.select(0, 8, 1)
    metrics.attach(s, False, grad)
    metrics.collect(s, 8, 0.001, 0.0, geo)
    for a in (geo, s):
        a.phase(4)
    metrics.collect_phase(s, 4, geo)
    metrics.write(lambda line: None, 0.001, 0.0)
    got, want = _tree(results / "VortexMetrics"), _tree(tmp_path / "twin" / "VortexMetrics")
    assert sorted(got) == sorted(want) and len(got) == 2 * 13 + 3
    for name in want:
        assert got[name] == want[name], name
    assert 0 < len(metrics.cells) < mesh.num_cells and np.isfinite(metrics.mean).all() and metrics.mean[1].max() > 0
    assert (metrics.mean[5] > 0).all() and len(set(metrics.curves[:, 1])) > 1            # the volume column varies in time
