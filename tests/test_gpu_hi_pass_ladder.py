"""What each call of a band-pass session does to each piece of its derived state, on the device (csrc/fsi_sessions.hip: the
fsi_band_* entry points and the ladder of FsiCtx::Band) - the table of tests/test_hi_pass_ladder.py, row by row: "gone" is
the FsiError of the getter with its text, "stays" the bits of the fetch before the call, "new" the bits of the NumPy twin
taken through the same calls (of the spectral power index, which the device forms within a bound of the twin's and not in its
bits, that the second slab added onto the low bins' power and left the other two sums alone).  Quantity v with 12 imported frames: on the first 66 nodes for the columns of the frames, and
on every P2 node with two weighted cells attached for the columns of the cell list as well."""
import numpy as np
import pytest

from test_hi_pass_ladder import A, A2, B, B2, COLUMNS, FRAMES, PERIOD, SELECTION, TABLE, WEIGHTS, WINDOW, ZI, ZI2, same_bits, snapshot
from vasp_amd import hi_pass as hp

pytestmark = pytest.mark.gpu

Q = "v"
NO_SERIES = "fsi_band_fetch: no filtered series (fsi_band_filter first)"
GONE = {"series": "fsi_band_trace: no filtered series (fsi_band_filter first)",
        "amplitude": "fsi_band_fetch: no amplitude (fsi_band_amplitude first)",      # NO_SERIES where the series is gone too
        "phase": "fsi_band_phase_fetch: no phase average (fsi_band_phase first)",
        "spi": "fsi_band_spi_fetch: no spectral power index (fsi_band_spi first)",
        "weights": "fsi_band_cell_vortex: sums_out without weights (fsi_band_cell_weights first)"}


@pytest.fixture(scope="module")
def hb(cylinder_case):
    from vasp_amd.capi import HipBackend
    backend = HipBackend(cylinder_case[1])
    yield backend
    backend.close()


def device_snapshot(hb, nodes: int, frames: int, period: int, cells: bool, at: int) -> dict:
    """Every column as the device's getter returns it - the bits, in the twin's layout, or the text of the refusal;
    ``frames``: the selected count, ``period``: that of the phase average if one stands."""
    from vasp_amd.capi import FsiError

    def get(f):
        try:
            return f()
        except FsiError as e:
            return str(e).split(": ", 1)[1]
    every = np.arange(nodes)
    got = dict(selection=hb.hi_pass_trace(Q, "raw", every)[:, :, 1:].transpose(1, 0, 2),
               series=get(lambda: hb.hi_pass_trace(Q, "filtered", every)[:, :, 1:]),
               amplitude=get(lambda: np.stack([hb.hi_pass_fetch(Q, "amplitude", k) for k in range(frames)])),
               phase=get(lambda: np.stack([hb.hi_pass_phase_fetch(Q, "mean", j) for j in range(max(period, 1))])),
               spi=get(lambda: hb.hi_pass_spi_fetch(Q, "sums")))
    if cells:
        got.update(cells=get(lambda: hb.hi_pass_cell_rate(Q, "raw", at, 1, 1)),
                   weights=get(lambda: hb.hi_pass_cell_vortex(Q, "raw", at, 1, 1, cells=False, sums=True)[1]))
    return got


def _calls(hb, twin, mesh, extra, cells2):
    """The row's call on the device and on the twin -> (selected frames, period of the phase average) after it, None: as before."""
    def both(name, *args):
        getattr(hb, f"hi_pass_{name.rstrip('_')}")(Q, *args)
        getattr(twin, name)(*args)

    def sample():
        hb.hi_pass_sample(Q)                          # the rows of dvp_["n"]: the twin is handed what the device recorded
        twin.sample(hb.hi_pass_fetch(Q, "raw", FRAMES))

    def cells():
        twin.cells(mesh.tet_nodes[cells2], hb.hi_pass_cells(Q, cells2))
    return {"sample": (sample, FRAMES + 1, 0),
            "import": (lambda: both("import_", extra[None]), FRAMES + 1, 0),
            "select": (lambda: both("select", 1, 5, 2), 5, 0),
            "filter": (lambda: both("filter", B2, A2, ZI2, 0), None, 0),
            "filter_next": (lambda: both("filter_next", B2, A2, ZI2, 0), None, 0),
            "phase": (lambda: both("phase", 2), None, 2),
            "amplitude": (lambda: both("amplitude", 2), None, None),
            "spi": (lambda: both("spi", None, 1, 1), None, None),
            "cells": (cells, None, None)}


ROWS = [(call, series, whole) for call in TABLE for series in (("phase", "filter") if call.startswith("filter") else ("phase",))
        for whole in (False, True) if whole or call != "cells"]


@pytest.mark.parametrize("call,series,whole", ROWS, ids=[f"{c}-after-{s}-{'cells' if w else '66'}" for c, s, w in ROWS])
def test_a_call_drops_what_depends_on_its_link_and_nothing_else(hb, cylinder_case, call, series, whole):
    mesh = cylinder_case[0]["mesh"]
    nodes = mesh.num_nodes if whole else 66
    rng = np.random.default_rng(21)
    x, extra = rng.standard_normal((FRAMES, nodes, 3)), rng.standard_normal((nodes, 3))
    hb.hi_pass_begin(Q, np.arange(nodes, dtype=np.int32), None, FRAMES + 1)      # one free frame, for the sample and import rows
    try:
        hb.hi_pass_import(Q, x)
        twin = hp.HostBandSession(3, FRAMES + 1)
        twin.import_(x)
        if whole:
            twin.cells(mesh.tet_nodes[[3, 11]], hb.hi_pass_cells(Q, [3, 11]))
            hb.hi_pass_cell_weights(Q, WEIGHTS)
            twin.cell_weights(WEIGHTS)
        frames, period = SELECTION[1], PERIOD if series == "phase" else 0
        assert hb.hi_pass_select(Q, *SELECTION) == frames == twin.select(*SELECTION)
        hb.hi_pass_spi(Q, None, 0, 1)
        twin.spi(None, 0, 1)
        if series == "phase":
            hb.hi_pass_phase(Q, PERIOD)
            twin.phase(PERIOD)
        else:
            hb.hi_pass_filter(Q, B, A, ZI, 0)
            twin.filter(B, A, ZI, 0)
        hb.hi_pass_amplitude(Q, WINDOW)
        twin.amplitude(WINDOW)
        before = device_snapshot(hb, nodes, frames, period, whole, 1)
        for col, value in before.items():             # everything stands, but the phase average under a filtered series
            assert isinstance(value, np.ndarray) or (col == "phase" and series == "filter"), (col, value)
        run, new_frames, new_period = _calls(hb, twin, mesh, extra, [5, 8])[call]
        run()
        frames, period = new_frames or frames, period if new_period is None else new_period
        at = 3 if TABLE[call][0] == "all" else 1
        after, want = device_snapshot(hb, nodes, frames, period, whole, at), snapshot(twin, at, nodes)
        fates = dict(zip(COLUMNS, TABLE[call]))
        for col in after:
            fate = fates[col]
            if fate == "gone":
                text = NO_SERIES if col == "amplitude" and fates["series"] == "gone" else GONE[col]
                assert isinstance(after[col], str) and after[col] == text, (col, after[col])
            elif fate == "stays":
                assert same_bits(after[col], before[col]), col
            elif col == "spi":                        # extended: the second slab added onto L2, X0^2 and Q stand (the device's DFT
                assert same_bits(after[col][1:], before[col][1:]) and (after[col][0] > before[col][0]).all()      # is the twin's within the
                assert not before[col][0].any()                                                                   # bound of test_gpu_hi_pass_spi.py)
            else:                                     # "all" too: the twin's selection is every recorded frame
                assert same_bits(after[col], want[col]), col
                assert not same_bits(after[col], before[col]), col
        if fates["selection"] == "all":
            assert after["selection"].shape[0] == FRAMES + 1 and same_bits(after["selection"], hb.hi_pass_export(Q, 0, FRAMES + 1))
    finally:
        hb.hi_pass_end(Q)
