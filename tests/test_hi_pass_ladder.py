"""What each call of a band-pass session does to each piece of its derived state, on the NumPy twin
(vasp_amd/hi_pass.py: HostBandSession) - the table of DESIGN.md ("The ladder of a band-pass session"), one row per call:

    recorded frames -> selection -> series (filtered / fluctuation) -> amplitude
                                 \\-> spectral power index (of the selected raw frames: survives a new series)
    cell list -> weights                (independent of the frames)

A session is brought to the state in which everything stands, the row's call is applied and every column is looked at:
"gone" is the getter's own refusal, "stays" the same bits as before the call, "new" the bits of a session that took the
direct route to the same state.  tests/test_gpu_hi_pass_ladder.py holds the device to the same table."""
import numpy as np
import pytest

from vasp_amd import hi_pass as hp

NODES, FRAMES, PERIOD, WINDOW = 8, 12, 4, 3
SELECTION = (2, 8, 1)                                # first, count, stride: two whole cycles of PERIOD
B, A, ZI = np.array([0.25, 0.25]), np.array([1.0, -0.5]), np.array([0.75])      # stable two-tap low-passes of gain 1 with their
B2, A2, ZI2 = np.array([0.1, 0.1]), np.array([1.0, -0.8]), np.array([0.9])       # zi = lfilter_zi(b, a): (1 + a1) zi = b1 - a1 b0
COLUMNS = ("selection", "series", "amplitude", "phase", "spi", "cells", "weights")
# the call -> what it leaves of every column; "all": the selection is every recorded frame again
TABLE = {
    "sample":      ("all",   "gone",  "gone",  "gone",  "gone",  "stays", "stays"),
    "import":      ("all",   "gone",  "gone",  "gone",  "gone",  "stays", "stays"),
    "select":      ("new",   "gone",  "gone",  "gone",  "gone",  "stays", "stays"),
    "filter":      ("stays", "new",   "gone",  "gone",  "stays", "stays", "stays"),
    "filter_next": ("stays", "new",   "gone",  "gone",  "stays", "stays", "stays"),
    "phase":       ("stays", "new",   "gone",  "new",   "stays", "stays", "stays"),
    "amplitude":   ("stays", "stays", "new",   "stays", "stays", "stays", "stays"),
    "spi":         ("stays", "stays", "stays", "stays", "new",   "stays", "stays"),
    "cells":       ("stays", "stays", "stays", "stays", "stays", "new",   "gone"),
}
GONE = {"series": "hi-pass trace: no filtered series (filter first)",
        "amplitude": None,                           # the one getter without a refusal of its own: the attribute is looked at
        "phase": "hi-pass phase_fetch: no phase average (phase first)",
        "spi": "hi-pass spi_fetch: no spectral power index (spi first)",
        "weights": "hi-pass cell_vortex: sums without weights (cell_weights first)"}

RNG = np.random.default_rng(20)
X = RNG.standard_normal((FRAMES, NODES, 3))
EXTRA = RNG.standard_normal((NODES, 3))              # the frame a sample or an import appends
CONN = RNG.integers(0, NODES, (2, 2, 10))            # two lists of two cells
GRAD = RNG.standard_normal((2, 2, 4, 3))
WEIGHTS = np.array([0.75, 1.5])


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[a == 0]), np.signbit(b[b == 0]))


def standing(series: str):
    """A session in which everything stands: 12 frames, two weighted cells, a selection, a one-slab spectral power index, the
    series (``series``: 'phase' the fluctuation about the phase average, 'filter' a filtered series) and its amplitude."""
    s = hp.HostBandSession(3, FRAMES + 1)            # one free frame, for the sample and the import rows
    s.import_(X)
    s.cells(CONN[0], GRAD[0])
    s.cell_weights(WEIGHTS)
    s.select(*SELECTION)
    s.spi(None, 0, 1)
    if series == "phase":
        s.phase(PERIOD)
    else:
        s.filter(B, A, ZI, 0)
    s.amplitude(WINDOW)
    return s


def snapshot(s, at: int = 1, nodes: int = NODES) -> dict:
    """Every column as its getter returns it: the bits, or the text of the refusal.  The cell columns are looked at through
    recorded frame 3, selected frame ``at``."""
    def get(f):
        try:
            return f()
        except RuntimeError as e:
            return str(e)
    return dict(selection=s.selected(),
                series=get(lambda: s.trace("filtered", range(nodes))[:, :, 1:]),
                amplitude=None if s.amp is None else np.stack([s.fetch("amplitude", k) for k in range(len(s.amp))]),
                phase=get(lambda: np.stack([s.phase_fetch("mean", j) for j in range(max(s.phase_period, 1))])),
                spi=get(lambda: s.spi_fetch("sums")),
                cells=get(lambda: s.cell_rate("raw", at, 1, 1)),
                weights=get(lambda: s.cell_vortex("raw", at, 1, 1, cells=False, sums=True)[1]))


CALLS = {"sample": lambda s: s.sample(EXTRA),
         "import": lambda s: s.import_(EXTRA[None]),
         "select": lambda s: s.select(1, 5, 2),      # recorded frames 1, 3, .. 9
         "filter": lambda s: s.filter(B2, A2, ZI2, 0),
         "filter_next": lambda s: s.filter_next(B2, A2, ZI2, 0),
         "phase": lambda s: s.phase(2),
         "amplitude": lambda s: s.amplitude(2),
         "spi": lambda s: s.spi(None, 1, 1),         # a second slab: the index is extended
         "cells": lambda s: s.cells(CONN[1], GRAD[1])}


def fresh(call: str, series: str, before: dict) -> dict:
    """The columns the call makes new, from their definitions."""
    sel = X[slice(1, 10, 2)] if call == "select" else before["selection"]
    if call == "select":
        return dict(selection=sel)
    if call == "filter":
        return dict(series=hp.filtfilt_rows(B2, A2, sel, ZI2, 0).transpose(1, 0, 2))
    if call == "filter_next":
        return dict(series=hp.filtfilt_rows(B2, A2, before["series"].transpose(1, 0, 2), ZI2, 0).transpose(1, 0, 2))
    if call == "phase":
        mean, fluct = hp.phase_average(sel, 2)
        return dict(series=fluct.transpose(1, 0, 2), phase=mean)
    if call == "amplitude":
        return dict(amplitude=hp.windowed_rms_running(before["series"].transpose(1, 0, 2), 2))
    if call == "spi":
        L2a, X0, Q, mean = hp.spi_sums(sel, None, 0, 1)
        L2b = hp.spi_sums(sel, None, 1, 1, mean)[0]
        return dict(spi=np.stack([L2a + L2b, X0, Q]))
    if call == "cells":
        return dict(cells=hp.cell_rate(X[3][CONN[1]], GRAD[1]))
    return {}


ROWS = [(call, series) for call in TABLE for series in (("phase", "filter") if call.startswith("filter") else ("phase",))]


@pytest.mark.parametrize("call,series", ROWS, ids=[f"{c}-after-{s}" for c, s in ROWS])
def test_a_call_drops_what_depends_on_its_link_and_nothing_else(call, series):
    s = standing(series)
    before = snapshot(s)
    for col in COLUMNS:                              # everything stands, but the phase average under a filtered series
        assert isinstance(before[col], np.ndarray) or (col == "phase" and series == "filter"), col
    CALLS[call](s)
    after, new = snapshot(s, 3 if TABLE[call][0] == "all" else 1), fresh(call, series, before)
    for col, fate in zip(COLUMNS, TABLE[call]):
        if fate == "gone":
            assert (after[col] is None) if GONE[col] is None else (after[col] == GONE[col]), (col, after[col])
        elif fate == "stays":
            assert same_bits(after[col], before[col]), col
        elif fate == "all":
            assert s.view == slice(None) and same_bits(after[col], np.concatenate([X, EXTRA[None]])), col
        else:
            assert same_bits(after[col], new[col]), col
            assert not same_bits(after[col], before[col]), col


def test_the_table_names_every_call_and_every_column():
    assert set(TABLE) == set(CALLS) and all(len(row) == len(COLUMNS) for row in TABLE.values())
    assert set(GONE) == {c for row in TABLE.values() for c, fate in zip(COLUMNS, row) if fate == "gone"}


# ---- the room rule's refusal texts (csrc/fsi_room.hpp through the kernel shim, host only) -------------------------------------

TAIL = ", the device has 1000000 bytes free of which 62500 stay with the context"      # "%.0f" of 62500.5 rounds to even
# entry point, subject, layout -> the text, written out from the format of each of the nine sites with need 123456789012,
# free 1000000, reserve 62500.5 and 195 rows, 12 frames, 7 cells, 66 nodes, a period of 4, 3 of 5 bins, 8-frame segments, 2 of them
ROOM_TEXTS = (
    ("fsi_band_cell_vortex", "the five results need", "7 cells x 40",
     "fsi_band_cell_vortex: the five results need 123456789012 bytes (7 cells x 40)" + TAIL),
    ("fsi_band_begin", "the session needs", "195 rows x 12 frames, raw and filtered",
     "fsi_band_begin: the session needs 123456789012 bytes (195 rows x 12 frames, raw and filtered)" + TAIL),
    ("fsi_spec_begin", "the session needs", "195 rows x 12 frames, raw and filtered, and the transforms' tables",
     "fsi_spec_begin: the session needs 123456789012 bytes (195 rows x 12 frames, raw and filtered, and the transforms' tables)" + TAIL),
    ("fsi_spec_spectrogram", "the transform needs",
     "tables of 8 frames x 3 of 5 bins, cos and sin, 2 segments x 195 rows of means and partial sums, and the result",
     "fsi_spec_spectrogram: the transform needs 123456789012 bytes (tables of 8 frames x 3 of 5 bins, cos and sin, 2 segments x 195 rows of "
     "means and partial sums, and the result)" + TAIL),
    ("fsi_band_phase", "the phase means need", "195 rows x 4 frames",
     "fsi_band_phase: the phase means need 123456789012 bytes (195 rows x 4 frames)" + TAIL),
    ("fsi_band_spi", "the sums and tables need", "195 rows, 12 frames x 3 bins of cos and sin",
     "fsi_band_spi: the sums and tables need 123456789012 bytes (195 rows, 12 frames x 3 bins of cos and sin)" + TAIL),
    ("fsi_band_cells", "the cell list needs", "7 cells x 144: ten nodes, twelve gradients, one result",
     "fsi_band_cells: the cell list needs 123456789012 bytes (7 cells x 144: ten nodes, twelve gradients, one result)" + TAIL),
    ("fsi_band_cell_rate_current", "the two further results need", "7 cells x 16",
     "fsi_band_cell_rate_current: the two further results need 123456789012 bytes (7 cells x 16)" + TAIL),
    ("fsi_board_begin", "the board needs", "66 nodes x 12 frames",
     "fsi_board_begin: the board needs 123456789012 bytes (66 nodes x 12 frames)" + TAIL),
)


def room_text(fn: str, subject: str, need: float, layout: str, free: int, reserve: float) -> str:
    import kernel_shim as ks
    out = np.zeros(512, dtype=np.uint8)
    ks.call("shim_room_refusal", fn.encode(), subject.encode(), float(need), layout.encode(), int(free), float(reserve), out, len(out))
    return out.tobytes().split(b"\0", 1)[0].decode()


@pytest.mark.parametrize("fn,subject,layout,text", ROOM_TEXTS, ids=[f"{r[0]}-{r[1].split()[1]}" for r in ROOM_TEXTS])
def test_a_room_refusal_reads_as_it_always_did(fn, subject, layout, text):
    from conftest import ROOT
    assert room_text(fn, subject, 123456789012.0, layout, 1000000, 62500.5) == text
    assert f'"{subject}"' in (ROOT / "vasp_amd" / "csrc" / "fsi_sessions.hip").read_text()      # the site says it in these words


def test_the_byte_counts_of_a_room_refusal_are_printf_s():
    """"%.0f" of the two doubles - ties to even, no exponent however large - and "%zu" of the free bytes."""
    text = room_text("f", "s", 8.0 * 2.0 ** 51, "l", 2 ** 63 + 1, 62501.5)
    assert text == "f: s 18014398509481984 bytes (l), the device has 9223372036854775809 bytes free of which 62502 stay with the context"
    assert room_text("f", "s", 1e30, "", 0, 0.5).startswith("f: s 1000000000000000019884624838656 bytes (), the device has 0 bytes free of which 0 stay")
