"""The spectral power index on the device (csrc/fsi_spi.hip; fsi_band_spi, fsi_band_spi_fetch; HipBackend.hi_pass_spi /
hi_pass_spi_fetch; ``--hi-pass-spi``) against the NumPy twin (vasp_amd/hi_pass.py: HostBandSession.spi / spi_fetch), which
tests/test_hi_pass_spi.py holds to numpy's rfft and to an extended-precision DFT.

Bounds: those derived in the docstring of tests/test_hi_pass_spi.py (``spi_bound``).  Device and twin form the same mean - the
same ordered sum - and from it the same y_j bits; they differ in the order inside a dot product (the matrix pipe's against
BLAS's) and inside the sums over bins and frames.  So the three sums L2, X0^2 and Q are held to the accumulation-only part of
the bound, and the index to the bound itself.  A node's index 1 - 2 sum_c L2_c / sum_c AC_c moves by at most
(2 sum_c dL2_c + (1 - SPI) sum_c dAC_c) / (sum_c AC_c - sum_c dAC_c) (``node_bound``), the row's bound with the sums over the
components in place of the row's terms.  The tests print the largest share of each bound the device uses.

The histories are filled with hi_pass_import: no time step is taken but in the end-to-end run."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_hi_pass_spi import WINDOWS, pulsatile_rows, spi_bound, spi_reference, window_of
from vasp_amd import hi_pass as hp

pytestmark = pytest.mark.gpu

STENOSIS = GOLDEN / "offset_stenosis" / "offset_stenosis.h5"
# rows: 129 - a second block of one row; 195; one row; 128 - exactly one block
SHAPES = (("v", 43), ("v", 65), ("p", 1), ("p", 128))
# (frames, kc): 7 frames are less than one chunk of 16, 50 no multiple of it; kc 1: no low bin; 17: a second wave's tile;
# 66: a second pass of 64 bins
CASES = ((7, 1), (7, 2), (50, 2), (50, 17), (160, 17), (160, 66))


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[a == 0]), np.signbit(b[b == 0]))


@pytest.fixture(scope="module")
def hb(cylinder_case):
    from vasp_amd.capi import HipBackend
    backend = HipBackend(cylinder_case[1])
    yield backend
    backend.close()


def _open(hb, q, nodes, x, capacity=None):
    """The session of q on the first ``nodes`` nodes with the history x, and its host twin."""
    hb.hi_pass_begin(q, np.arange(nodes, dtype=np.int32), None, capacity or len(x))
    hb.hi_pass_import(q, x)
    twin = hp.HostBandSession(x.shape[2], capacity or len(x))
    twin.import_(x)
    return twin


def node_bound(ref, b):
    """The module docstring's bound on the index of a node, from the rows' reference values and bounds, (nodes, ncomp)."""
    AC, dAC, dL2 = ref["AC"].sum(axis=1), b["dAC"].sum(axis=1), b["dL2"].sum(axis=1)
    spi = 1 - 2 * ref["L2"].sum(axis=1) / AC
    return (2 * dL2 + (1 - spi) * dAC) / (AC - dAC), AC - dAC


def _share(diff, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(diff == 0, 0.0, diff / bound)))


def _all(session_fetch):
    return {what: session_fetch(what) for what in hp.SPI_WHAT}


@pytest.mark.parametrize("n,kc", CASES, ids=[f"n{n}kc{k}" for n, k in CASES])
@pytest.mark.parametrize("q,nodes", SHAPES, ids=[f"{q}{n}" for q, n in SHAPES])
def test_device_against_the_twin_within_the_derived_bound(hb, q, nodes, n, kc):
    ncomp = 1 if q == "p" else 3
    x = pulsatile_rows(n, (nodes, ncomp), seed=1000 * n + kc + nodes)
    twin = _open(hb, q, nodes, x)
    try:
        for window in WINDOWS:
            w = window_of(window, n)
            hb.hi_pass_spi(q, w, 0, kc)
            twin.spi(w, 0, kc)
            ref = spi_reference(x, w, kc)
            acc, full = spi_bound(x, w, kc, ref, accumulation_only=True), spi_bound(x, w, kc, ref)
            assert (acc["margin"] > 0).all() and (full["margin"] > 0).all()          # the bounds say something on every row
            dev, host = _all(lambda what: hb.hi_pass_spi_fetch(q, what)), _all(twin.spi_fetch)
            assert dev["sums"].shape == (3, nodes, ncomp) and dev["rows"].shape == (nodes, ncomp) and dev["nodes"].shape == (nodes,)
            shares = {}
            for k, (name, key) in enumerate((("L2", "dL2"), ("X0^2", "dX0sq"), ("Q", "dQ"))):
                diff = np.abs(dev["sums"][k] - host["sums"][k])
                shares[name] = _share(diff, acc[key])
                assert (diff <= acc[key]).all(), (name, window)
            diff = np.abs(dev["rows"] - host["rows"])
            shares["SPI"] = _share(diff, full["dSPI"])
            assert (diff <= full["dSPI"]).all(), window
            assert (np.abs(dev["rows"] - ref["spi"]) <= full["dSPI"]).all(), window      # and against the extended-precision DFT
            nb, margin = node_bound(ref, full)
            assert (margin > 0).all()
            diff = np.abs(dev["nodes"] - host["nodes"])
            shares["node"] = _share(diff, nb)
            assert (diff <= nb).all(), window
            print(f"{q}{nodes} n = {n} kc = {kc} {window}: SPI {dev['rows'].min():.3g} .. {dev['rows'].max():.3g}; largest shares of the "
                  "bounds " + ", ".join(f"{k} {v:.3g}" for k, v in shares.items()))
            if kc == 1:                            # no low bin: all the power is high, exactly
                assert (dev["rows"] == 1.0).all() and (dev["nodes"] == 1.0).all() and not dev["sums"][0].any()
            else:
                assert ((dev["rows"] > 0) & (dev["rows"] < 1)).all()
            if ncomp == 1:
                assert same_bits(dev["nodes"], dev["rows"][:, 0])
            # the same call again gives the same bits
            hb.hi_pass_spi(q, w, 0, kc)
            again = _all(lambda what: hb.hi_pass_spi_fetch(q, what))
            assert all(same_bits(again[what], dev[what]) for what in hp.SPI_WHAT), window
        assert same_bits(hb.hi_pass_export(q, 0, n), x)                               # the raw frames are untouched
    finally:
        hb.hi_pass_end(q)


@pytest.mark.parametrize("q,nodes", (("v", 43), ("p", 1)), ids=["v43", "p1"])
def test_a_strided_view_equals_a_session_of_those_frames(hb, q, nodes):
    """select(first=3, stride=2): selected frame k is recorded frame 3 + 2 k.  The history is addressed through the stride:
    the sums and the index are those of a session that imported only those frames, bit for bit."""
    n, kc, ncomp = 50, 17, 1 if q == "p" else 3
    x = pulsatile_rows(3 + 2 * n + 1, (nodes, ncomp), seed=77 + nodes)
    got = {}
    for window in WINDOWS:
        w = window_of(window, n)
        twin = _open(hb, q, nodes, x)
        try:
            assert hb.hi_pass_select(q, 3, n, 2) == n == twin.select(3, n, 2)
            hb.hi_pass_spi(q, w, 0, kc)
            got[window] = _all(lambda what: hb.hi_pass_spi_fetch(q, what))
            assert same_bits(hb.hi_pass_export(q, 0, len(x)), x)
            twin.spi(w, 0, kc)
            view = x[3:3 + 2 * n:2]
            ref = spi_reference(view, w, kc)
            assert (np.abs(got[window]["rows"] - twin.spi_fetch("rows")) <= spi_bound(view, w, kc, ref)["dSPI"]).all()
        finally:
            hb.hi_pass_end(q)
        _open(hb, q, nodes, np.ascontiguousarray(x[3:3 + 2 * n:2]))
        try:
            hb.hi_pass_spi(q, w, 0, kc)
            for what in hp.SPI_WHAT:
                assert same_bits(hb.hi_pass_spi_fetch(q, what), got[window][what]), (window, what)
        finally:
            hb.hi_pass_end(q)
    assert not same_bits(got["boxcar"]["rows"], got["hann"]["rows"])


def test_two_slabs_against_one(hb):
    """Bins 0 .. 39 and 40 .. 65 of 160 frames against one slab of 66: the second slab adds onto the first one's row sums."""
    n, kc, nodes = 160, 66, 43
    x = pulsatile_rows(n, (nodes, 3), seed=5)
    _open(hb, "v", nodes, x)
    try:
        for window in WINDOWS:
            w = window_of(window, n)
            acc = spi_bound(x, w, kc, spi_reference(x, w, kc), accumulation_only=True)
            hb.hi_pass_spi("v", w, 0, kc)
            one = _all(lambda what: hb.hi_pass_spi_fetch("v", what))
            runs = []
            for _ in range(2):
                hb.hi_pass_spi("v", w, 0, 40)
                first = hb.hi_pass_spi_fetch("v", "sums")
                hb.hi_pass_spi("v", w, 40, 26)
                runs.append(_all(lambda what: hb.hi_pass_spi_fetch("v", what)))
                assert same_bits(runs[-1]["sums"][1:], first[1:]) and (runs[-1]["sums"][0] > first[0]).all()      # X0^2 and Q stand
            assert all(same_bits(runs[0][what], runs[1][what]) for what in hp.SPI_WHAT)
            two = runs[0]
            assert same_bits(two["sums"][1:], one["sums"][1:])
            diff = np.abs(two["sums"][0] - one["sums"][0])
            assert (diff <= acc["dL2"]).all() and (np.abs(two["rows"] - one["rows"]) <= acc["dSPI"]).all()
            print(f"two slabs, {window}: largest share of the accumulation bound, L2 {_share(diff, acc['dL2']):.3g}, SPI "
                  f"{_share(np.abs(two['rows'] - one['rows']), acc['dSPI']):.3g}")
    finally:
        hb.hi_pass_end("v")


def test_special_values_stay_in_their_rows_and_the_history_is_left_alone(hb):
    n, kc, nodes = 50, 5, 65
    x = pulsatile_rows(n, (nodes, 3), seed=9)
    x[:, 2, :] = 0.0                              # a node at rest
    x[:, 3, 1] = 0.0                              # one silent component
    x[0, 3, 1] = -0.0
    x[7, 40, 2] = np.nan
    x[n - 1, 64, 0] = np.inf
    clean = x.copy()
    clean[:, 40, 2] = clean[:, 64, 0] = 1.0       # the two rows that hold a special value
    low = hp.design(1e-3, 0.0, 200.0)
    keys = ("b", "a", "zi", "padlen")
    twin = _open(hb, "v", nodes, x)
    try:
        hb.hi_pass_filter("v", *(low[k] for k in keys))
        before = np.stack([hb.hi_pass_fetch("v", "filtered", k) for k in range(n)])
        hb.hi_pass_spi("v", None, 0, kc)
        twin.spi(None, 0, kc)
        rows, nodes_spi, sums = (hb.hi_pass_spi_fetch("v", what) for what in hp.SPI_WHAT)
        bad = np.zeros((nodes, 3), dtype=bool)
        bad[40, 2] = bad[64, 0] = True
        assert np.isnan(rows[bad]).all() and np.isfinite(rows[~bad]).all()
        assert np.isnan(nodes_spi[[40, 64]]).all() and np.isfinite(np.delete(nodes_spi, [40, 64])).all()
        assert not np.isfinite(sums[:, bad]).any() and np.isfinite(sums[:, ~bad]).all()
        assert not rows[2].any() and not np.signbit(rows[2]).any() and nodes_spi[2] == 0.0 and not sums[:, 2].any()
        assert rows[3, 1] == 0.0 and not sums[:, 3, 1].any() and 0 < nodes_spi[3] < 1
        assert same_bits(np.isnan(rows), np.isnan(twin.spi_fetch("rows"))) and same_bits(np.isnan(nodes_spi), np.isnan(twin.spi_fetch("nodes")))
        # every other row is what it is without the two special values, bit for bit: a row depends on that row alone
        assert same_bits(hb.hi_pass_export("v", 0, n), x)
        assert same_bits(np.stack([hb.hi_pass_fetch("v", "filtered", k) for k in range(n)]), before)      # the series still stands
        hb.hi_pass_filter("v", *(low[k] for k in keys))
        assert same_bits(np.stack([hb.hi_pass_fetch("v", "filtered", k) for k in range(n)]), before)
        assert same_bits(hb.hi_pass_spi_fetch("v", "rows"), rows)                                          # a filter leaves the index alone
    finally:
        hb.hi_pass_end("v")
    _open(hb, "v", nodes, clean)
    try:
        hb.hi_pass_spi("v", None, 0, kc)
        assert same_bits(hb.hi_pass_spi_fetch("v", "rows")[~bad], rows[~bad])
        assert same_bits(np.delete(hb.hi_pass_spi_fetch("v", "nodes"), [40, 64]), np.delete(nodes_spi, [40, 64]))
    finally:
        hb.hi_pass_end("v")


def test_refusals_leave_the_context_stepping(hb, cylinder_case):
    from vasp_amd.capi import FsiError
    x = pulsatile_rows(12, (65, 3), seed=4)
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_spi("v", None, 0, 2)
    solid = np.nonzero(np.asarray(cylinder_case[1]["cell_kind"]) == 1)[0][:3]
    hb.hi_pass_begin_cells("strain", solid, 8)
    try:
        hb.hi_pass_import("strain", np.zeros((8, 12, 6)))
        with pytest.raises(FsiError, match="a strain / stress session has no spectral power index") as e:
            hb.hi_pass_spi("strain", None, 0, 2)
        assert e.value.code == 1
    finally:
        hb.hi_pass_end("strain")
    twin = _open(hb, "v", 65, x, capacity=14)
    try:
        with pytest.raises(FsiError, match=r"no spectral power index \(fsi_band_spi first\)"):
            hb.hi_pass_spi_fetch("v", "rows")
        with pytest.raises(FsiError, match="needs bin0 >= 0, nb >= 1 bins and their cos / sin columns"):
            hb.hi_pass_spi("v", None, 0, 0)
        with pytest.raises(FsiError, match=r"a slab out of order: bin0 = 2, no slab stands before it \(bin0 = 0 first\)"):
            hb.hi_pass_spi("v", None, 2, 1)
        with pytest.raises(FsiError, match="bins 0 .. 6 of 12 selected frames: a low bin lies below the Nyquist frequency, at most bin 5"):
            hb.hi_pass_spi("v", None, 0, 7)
        hb.hi_pass_spi("v", None, 0, 2)
        with pytest.raises(FsiError, match="a slab out of order: bin0 = 3, the next slab starts at bin 2"):
            hb.hi_pass_spi("v", None, 3, 1)
        assert hb.lib.fsi_band_spi_fetch(hb.ctx, 1, 3, None) == 1 and hb.lib.fsi_band_spi_fetch(hb.ctx, 1, 0, None) == 1
        assert hb.lib.fsi_band_spi(hb.ctx, 1, None, 0, 2, None, None) == 1
        hb.hi_pass_spi("v", None, 2, 2)            # the refused calls left the sums standing
        twin.spi(None, 0, 4)
        ref = spi_reference(x, None, 4)
        assert (np.abs(hb.hi_pass_spi_fetch("v", "rows") - twin.spi_fetch("rows")) <= spi_bound(x, None, 4, ref)["dSPI"]).all()
        # a selection, an import and a sample drop the index
        for undo in (lambda: hb.hi_pass_select("v", 0, 10, 1), lambda: hb.hi_pass_import("v", x[:1]), lambda: hb.hi_pass_sample("v")):
            hb.hi_pass_spi("v", None, 0, 2)
            assert hb.hi_pass_spi_fetch("v", "nodes").shape == (65,)
            undo()
            with pytest.raises(FsiError, match=r"no spectral power index \(fsi_band_spi first\)"):
                hb.hi_pass_spi_fetch("v", "nodes")
        hb.hi_pass_select("v", 0, 1, 1)
        with pytest.raises(FsiError, match="1 selected frames, the index needs at least 2"):
            hb.hi_pass_spi("v", None, 0, 1)
    finally:
        hb.hi_pass_end("v")
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_spi_fetch("v", "rows")
    # the context still steps
    ns, _, bc_values, pressure, hook = cylinder_case
    run = dict(ns)
    run["t"] = float(ns["dt"])
    with contextlib.redirect_stdout(io.StringIO()):
        hook("pre_solve")(**run)
    hb.set_dirichlet_values(bc_values())
    hb.set_interface_pressure(float(pressure.P) if pressure is not None else 0.0)
    hist = hb.newton_solve(counter=0, first_step_num=0, **{k: ns[k] for k in ("atol", "rtol", "max_it", "lmbda", "recompute", "recompute_tstep")})
    assert len(hist) >= 1 and np.isfinite(hb.get_state("n")).all()


# ---- end to end -------------------------------------------------------------------------------------------------------

def test_end_to_end_run_and_the_finished_folder_write_the_same_index(tmp_path):
    """12 steps on the small stenosis mesh, every one saved: bins of 83 Hz, a cut-off of 200 Hz leaves bins 1 and 2 below.  The
    run in a fresh process; the finished folder through vasp_amd.postprocess gives the same datasets and the same spi.csv; the
    written field is hi_pass_spi_fetch of the saved frames."""
    from test_gpu_hi_pass import _files
    from vasp_amd import postprocess
    from vasp_amd.h5lite import read_h5
    options = ["--hi-pass", "v", "p", "--hi-pass-spi", "--hi-pass-spi-cutoff", "200"]
    results = tmp_path / "case" / "1"
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "vasp_amd.monolithic", "-p", "offset_stenosis", "-dt", "0.001", "-T", "0.0115",
           "--verbose", "False", "--folder", str(results.parent), "--sub-folder", "1", "--save-step", "1", "--save-deg", "2",
           "--checkpoint-step", "1000", *options, "--new-arguments", f"mesh_path={STENOSIS}"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Hi-pass velocity_spi_200: spectral power index over 12 frames, 2 bins of 83.3333 Hz below the cut-off (boxcar), written" in r.stdout
    lines = []
    ns = postprocess.run(["--folder", str(results), "--output-folder", str(tmp_path / "again"), *options], out=lines.append)
    backend = ns["backend"]
    try:
        assert any("Read 12 of 12 frames" in line for line in lines)
        run, again = _files(results / "Visualization_hi_pass"), _files(tmp_path / "again" / "Visualization_hi_pass")
        stems = ["velocity_spi_200", "pressure_spi_200"]
        assert {k.split(":")[0] for k in run} == {f"{s}.{e}" for s in stems for e in ("h5", "xdmf")} | {"spi.csv"}
        assert sorted(run) == sorted(again)
        for name in run:
            assert run[name] == again[name], name
        header, *rows = (results / "Visualization_hi_pass" / "spi.csv").read_text().splitlines()
        assert header == "# " + hp.SPI_HEADER and [r.split(",")[0] for r in rows] == ["velocity", "pressure"]
        for (name, q), row in zip((("velocity", "v"), ("pressure", "p")), rows):
            g = read_h5(results / "Visualization" / f"{name}.h5")["VisualisationVector"]
            x = np.stack([np.asarray(g[str(k)].data) for k in range(12)])
            assert x.dtype == np.float64
            nodes = len(x[0])
            backend.hi_pass_begin(q, *hp.output_nodes(ns["mesh"], 2, q), 12)
            try:
                backend.hi_pass_import(q, x)
                backend.hi_pass_spi(q, None, 0, 3)
                field = backend.hi_pass_spi_fetch(q, "nodes")
            finally:
                backend.hi_pass_end(q)
            written = np.frombuffer(run[f"{name}_spi_200.h5:/VisualisationVector/0"][2], dtype=np.float32)
            assert written.shape == (nodes,) and np.array_equal(written, field.astype(np.float32), equal_nan=True)
            cols = [c.strip() for c in row.split(",")]
            assert len(cols) == 11 and cols[1:4] == ["200.0", "boxcar", "12"] and cols[6] == "3"
            good = field[np.isfinite(field)]
            assert [float(c) for c in cols[7:10]] == [good.min(), good.mean(), good.max()]
            assert int(cols[10]) == int(np.flatnonzero(np.isfinite(field))[np.argmax(good)])
            assert 0 <= good.min() and good.max() <= 1 and good.max() > 0
    finally:
        backend.close()
