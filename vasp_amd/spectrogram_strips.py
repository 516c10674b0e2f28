"""Spectrograms of a history larger than the device: ``python -m vasp_amd.postprocess --spectrogram ...`` in strips of rows.

What the pipeline takes from a session are three means over the rows of a per-row power - the spectrogram of the high-passed
rows, the spectrogram of the raw rows and their periodogram [REF src/vasp/postprocessing/postprocessing_h5py/spectrograms.py:
409-417,448-463] - and the filter and the transform work on each row by itself.  The session adds the rows without atomics,
block by block of ``granule`` rows in index order (csrc/fsi_spec.hip, k_spec_power and k_spec_reduce; ``spectrogram.sum_power``
on the host), so a strip ``[r0, r1)`` of the quantity's rows whose first row is a multiple of the granule forms exactly the
blocks one session on all rows forms, and the running sum carried from strip to strip (``spectrogram_sum`` /
``periodogram_sum``) ends in the same bits.  The four CSV files are those of the unsplit path byte for byte.

The rows of ``--spectrogram-component all`` are component-major (row = c * n + i): a strip of them can cross a component
boundary and is opened on listed rows (``HipBackend.spec_begin_rows``).  A strip of magnitudes is a sub-list of the nodes.
The wall shear stress is opened on listed rows from the start (``HipBackend.spec_begin_wss``): a strip is a sub-list of them.

The sound file of ``--spectrogram-sampling PointList`` is not written here: a list of points never needs strips.

One quantity at a time; per quantity the fewest strips of equal size whose session fits (``plan_row_strips``); the frames
are read once per strip, only the field the quantity reads.  The log names the counts and the seconds.
"""
from __future__ import annotations

import time as _time
from typing import Callable, List, Tuple

import numpy as np

from . import spectrogram as sg


def plan_row_strips(rows: int, granule: int, capacity: int, limit: int, need: Callable[[int, int], int]) -> List[Tuple[int, int]]:
    """The fewest strips ``[r0, r1)`` of equal size - the size rounded up to a multiple of ``granule``, the last strip
    possibly shorter - over ``rows`` rows such that a session of one strip, ``need(rows, capacity)`` bytes, fits into
    ``limit`` bytes.  None is empty.  SystemExit with the byte counts when not even one granule of rows fits."""
    rows, granule = int(rows), int(granule)
    if rows < 1 or granule < 1:
        raise SystemExit(f"--spectrogram in strips: needs rows >= 1 and a granule >= 1, got {rows} and {granule}")
    size_of = lambda k: min(rows, -(-(-(-rows // k)) // granule) * granule)      # ceil(rows / k), rounded up to the granule
    if need(min(granule, rows), capacity) > limit:
        raise SystemExit(f"--history-memory: {min(granule, rows)} rows, the fewest a strip of a spectrogram history holds, need "
                         f"{need(min(granule, rows), capacity)} bytes over {capacity} frames, the histories may take {limit}")
    lo, hi = 1, -(-rows // granule)             # hi strips of one granule fit, checked above; need grows with the rows
    while lo < hi:
        mid = (lo + hi) // 2
        if need(size_of(mid), capacity) <= limit:
            hi = mid
        else:
            lo = mid + 1
    size = size_of(lo)
    return [(r, min(r + size, rows)) for r in range(0, rows, size)]


def granule_of(backend) -> int:
    """Rows a strip boundary must be a multiple of, for a backend or a backend class: the device's row block, or the column
    chunk of the host sessions."""
    return sg.DeviceSpecSession.granule if hasattr(backend, "spec_begin_rows") else sg.host_chunk(backend)


def need_of(backend, magnitude: bool) -> Callable[[int, int], int]:
    """``need(rows, capacity)`` in the bytes the begin calls compare: ``fsi_spec_room``'s, or its host twin's."""
    room = backend.spec_room if hasattr(backend, "spec_room") else sg.host_room
    return lambda rows, capacity: room(rows, capacity, magnitude)[0]


def total_need(run: "sg.SpectrogramRun", capacity: int) -> int:
    """The sessions of all asked quantities, open together as the unsplit path opens them."""
    return sum(need_of(run.backend, is_magnitude(run, q))(run.rows(q), capacity) for q in run.quantities)


def is_magnitude(run: "sg.SpectrogramRun", q: str) -> bool:
    return q != "p" and run.opts["component"] == "mag"


def row_lists(run: "sg.SpectrogramRun", q: str):
    """(nodes, nodes_b or None, comps or None) of every row of the quantity, in the session's row order."""
    sel, comp = run.sel[q], run.opts["component"]
    nodes, nodes_b = sel["nodes"], sel["nodes_b"]
    if q == "p":
        return nodes, nodes_b, None
    reps = 3 if comp == "all" else 1
    comps = np.repeat(np.arange(3, dtype=np.int32), len(nodes)) if comp == "all" else np.full(len(nodes), "xyz".index(comp), dtype=np.int32)
    return np.tile(nodes, reps), None if nodes_b is None else np.tile(nodes_b, reps), comps


class _Strip:
    """Rows ``[r0, r1)`` of one quantity in a session of their own; ``sample`` is what the frame loop calls."""

    def __init__(self, run: "sg.SpectrogramRun", q: str, r0: int, r1: int, capacity: int):
        self.run, self.q, self.r0, self.r1 = run, q, r0, r1
        backend = run.backend
        self.device = hasattr(backend, "spec_begin_rows")
        self.frames = 0
        if not self.device:
            self.session = sg.HostSpecSession(r1 - r0, capacity, sg.host_chunk(backend))
            return
        self.session = sg.DeviceSpecSession(backend, q)
        if q == "wss":
            backend.spec_begin_wss(*run.begin_args(q, r0, r1), capacity)
        elif is_magnitude(run, q):
            sel = run.sel[q]
            self.session.begin(sel["nodes"][r0:r1], None if sel["nodes_b"] is None else sel["nodes_b"][r0:r1], "mag", capacity)
        else:
            nodes, nodes_b, comps = row_lists(run, q)
            self.session.begin_rows(nodes[r0:r1], None if nodes_b is None else nodes_b[r0:r1], None if comps is None else comps[r0:r1],
                                    capacity)

    def sample(self, t: float, state) -> None:
        if self.device:
            self.session.sample()
        else:
            self.session.sample(self.run._host_frame(self.q, state())[self.r0:self.r1])
        self.frames += 1


def run_quantity(q: str, run: "sg.SpectrogramRun", limit: int, sample_frames: Callable, out=print) -> dict:
    """All strips of one quantity of ``run`` (a ``SpectrogramRun`` without sessions) and its four files.
    ``sample_frames(fields, sessions)``: the frame loop of ``postprocess.run`` over the selected frames, reading ``fields`` and
    handing each frame to ``sessions``.  Returns the counts and seconds it logs."""
    tick = _time.perf_counter
    backend = run.backend
    rows, n = run.rows(q), run.expected
    capacity = n + 1
    strips = plan_row_strips(rows, granule_of(backend), capacity, limit, need_of(backend, is_magnitude(run, q)))
    tp = sg.transform_plan(rows, n, n * run.dt_files, run.opts)
    seconds = dict(read=0.0, transform=0.0)
    carries = None
    for r0, r1 in strips:
        strip = _Strip(run, q, r0, r1, capacity)
        try:
            t = tick()
            sample_frames([sg.FIELD_OF[q]], [strip])
            seconds["read"] += tick() - t
            if strip.frames != n:
                raise SystemExit(f"--spectrogram {q} in strips: {strip.frames} frames were read, {n} were planned")
            t = tick()
            carries = sg.session_powers(strip.session, tp, (r0, r1 == rows), carries)
            seconds["transform"] += tick() - t
        finally:
            strip.session.end()
    res = sg.results(carries, tp, run.start_t, run.min_color(q))
    sg.write_files(run.folder, run.sel[q]["name"], run.case + run.sel[q]["case_suffix"], res, run.min_color(q))
    out(f"Spectrograms of {q} in strips: {len(strips)} strips of at most {strips[0][1] - strips[0][0]} rows ({rows} in all), the {n} frames "
        f"read {len(strips)} times; {seconds['read']:.2f} s reading, {seconds['transform']:.2f} s transforming; written to {run.folder}")
    return dict(strips=len(strips), passes=len(strips), seconds=seconds)
