"""Band-pass a history larger than the device: ``python -m vasp_amd.postprocess --hi-pass ... --hi-pass-tensor ...`` in strips
of rows.

The filter, the windowed RMS and the tensor's principal value work on each row by itself, so the rows of a quantity can go
through the session a strip at a time - a strip being a contiguous range ``[i0, i1)`` of the quantity's nodes (d, v, p) or
listed solid cells (strain, stress), whose part of every written dataset is one contiguous block.  Two things couple the rows:

* the frame-major layout of the files: every frame of a series is reserved first (``h5lite.H5Series.reserve``), in frame
  order, and each strip fills its block of every frame - the file is, byte for byte, the one the unsplit path appends;
* the amplitude table, with its eleven percentiles, the maximum and its node per frame over all nodes
  [REF src/vasp/postprocessing/postprocessing_h5py/create_hi_pass_viz.py:377-390]: the amplitude magnitudes of all strips
  are kept on a board ``[frame][node]`` on the device (``HipBackend.hi_pass_board_*``; ``hi_pass.HostBoard`` for a backend
  without it) and the table is formed there by an exact selection (csrc/fsi_band.hip, k_band_select) and
  ``hi_pass.percentiles_from_ranks``, numpy's interpolation.

One quantity at a time; per quantity the fewest strips of equal size whose session fits beside the board (``plan_strips``).
Without ``--hi-pass-amplitude`` the frames are read once per strip and every series (the bands, the multiband chain) is
filtered from the strip's history.  With it there is one board per quantity, which holds one series at a time: the strips
are passed once per series, so the frames are read ``series x strips`` times.  The log names the counts and the seconds.
"""
from __future__ import annotations

import time as _time
from typing import Callable, List, Tuple

import numpy as np

from . import hi_pass as hp
from . import hi_pass_tensor as hpt


def plan_strips(units: int, rows_per_unit: int, capacity: int, board_bytes: int, limit: int,
                need: Callable[[int, int], int], what: str = "node") -> List[Tuple[int, int]]:
    """The fewest strips ``[i0, i1)`` of equal size (the last may be shorter) over ``units`` nodes or cells of
    ``rows_per_unit`` rows each, such that a session of one strip - ``need(rows, capacity)`` bytes - fits into ``limit``
    bytes beside a board of ``board_bytes``.  A strip never cuts a unit, none is empty.  SystemExit with the byte counts when
    the board alone does not fit, or not even one unit's rows beside it."""
    if board_bytes > limit:
        raise SystemExit(f"--hi-pass-amplitude: the board of amplitude magnitudes alone needs {board_bytes} bytes, the band-pass "
                         f"histories may take {limit} (--history-memory); dropping --hi-pass-amplitude needs none")
    room = limit - board_bytes
    if need(rows_per_unit, capacity) > room:
        raise SystemExit(f"--history-memory: the {rows_per_unit} rows of one {what} need {need(rows_per_unit, capacity)} bytes over "
                         f"{capacity} frames" + (f" beside the board's {board_bytes}" if board_bytes else "") +
                         f", the band-pass histories may take {limit}")
    fits = lambda k: need(-(-units // k) * rows_per_unit, capacity) <= room
    lo, hi = 1, units                           # fits(units): one unit per strip, checked above; need grows with the rows
    while lo < hi:
        mid = (lo + hi) // 2
        if fits(mid):
            hi = mid
        else:
            lo = mid + 1
    size = -(-units // lo)
    return [(i, min(i + size, units)) for i in range(0, units, size)]


class Job:
    """One band-pass quantity: ``units`` nodes (``kind`` "field") or solid cells ("tensor") of ``rows_per_unit`` rows, of
    which the board has ``nodes_per_unit`` columns each; ``frames``: the frames its series are written on."""

    def __init__(self, kind: str, q: str, units: int, rows_per_unit: int, nodes_per_unit: int, frames: int):
        self.kind, self.q, self.units, self.rows_per_unit, self.nodes_per_unit, self.frames = kind, q, units, rows_per_unit, nodes_per_unit, frames

    def board_bytes(self, amplitude: bool) -> int:
        return 8 * self.units * self.nodes_per_unit * self.frames if amplitude else 0


def jobs(mesh, ns: dict) -> List[Job]:
    """The band-pass quantities ``ns`` asks for, in the order d, v, p, strain, stress."""
    out = []
    if ns.get("hi_pass"):
        stride, t0, t1 = hp.frame_window(ns)
        n = hp.select_frames(hp.saved_times(ns), float(ns["dt"]), stride, hp.frame_start(ns, t0), t1)[1]
        for q in hp.quantities(ns):
            out.append(Job("field", q, len(hp.output_nodes(mesh, int(ns["save_deg"]), q)[0]), 1 if q == "p" else 3, 1, n))
    if ns.get("hi_pass_tensor"):
        from .stress_strain import solid_cells
        cells = len(solid_cells(mesh, ns["dx_s_id"]))
        for q in hpt.quantities(ns):
            out.append(Job("tensor", q, cells, 24, 4, len(hp.saved_times(ns))))
    return out


def everything_fits(job_list: List[Job], capacity: int, amplitude: bool, limit: int, need) -> bool:
    """The histories of all quantities, open together as the unsplit path opens them, with a board each where the amplitude
    is asked for, against ``limit`` bytes."""
    total = sum(need(j.units * j.rows_per_unit, capacity) + j.board_bytes(amplitude) for j in job_list if j.units)
    return total <= limit


class _FieldSeries:
    """``<viz>.h5`` of ``HiPassWriter`` with every frame reserved: ``fill`` writes the rows of nodes ``i0 ...`` of frame k."""

    def __init__(self, writer: hp.HiPassWriter, viz: str, n: int, ncomp: int):
        self.writer, self.viz, self.n, self.ncomp = writer, viz, n, ncomp
        self.h5 = writer.open(viz)
        self.addr = [self.h5.reserve(str(k), (len(writer.geometry), ncomp), np.float32) for k in range(n)]

    def fill(self, k: int, i0: int, frame) -> None:
        self.h5.fill(self.addr[k], 4 * self.ncomp * i0, np.asarray(frame).reshape(-1, self.ncomp).astype(np.float32))

    def close(self, dt_files: float, t0: float) -> None:
        self.h5.close()
        self.writer.write_xdmf(self.viz, self.n, self.ncomp, dt_files, t0)


class _TensorSeries:
    """The same of ``hi_pass_tensor.TensorSeries``: ``fill`` writes the dofs of cells ``i0 ...`` of frame k."""

    def __init__(self, writer: hpt.TensorWriter, viz: str, n: int, ncomp: int):
        self.series = writer.open(viz, ncomp)
        self.addr = [self.series.reserve() for _ in range(n)]

    def fill(self, k: int, i0: int, frame) -> None:
        self.series.fill(self.addr[k], i0, frame)

    def close(self, dt_files: float, t0: float) -> None:
        self.series.close(dt_files, t0)


def run_quantity(job: Job, backend, mesh, ns: dict, limit: int, need, sample_frames: Callable, out=print) -> dict:
    """All passes of one quantity.  ``sample_frames(fields, sessions)``: the frame loop of ``postprocess.run`` over the
    selected frames, reading ``fields`` and handing each frame to ``sessions``.  Returns the counts and seconds it logs."""
    tick = _time.perf_counter
    field = job.kind == "field"
    amplitude = bool(ns.get("hi_pass_amplitude"))
    capacity = len(hp.saved_times(ns)) + 1
    run_cls, key, strip_key = (hp.HiPassRun, "hi_pass", "hi_pass_strip") if field else (hpt.HiPassTensorRun, "hi_pass_tensor", "hi_pass_tensor_strip")
    if field and ns.get("hi_pass_flow_metrics"):
        raise SystemExit(hp.METRICS_STRIPS)
    if field and ns.get("hi_pass_vortex"):
        from .vortex import VORTEX_STRIPS
        raise SystemExit(VORTEX_STRIPS)
    if job.units == 0:
        run_cls(backend, mesh, {**ns, key: [job.q]})      # its own refusal: nothing to record
    strips = plan_strips(job.units, job.rows_per_unit, capacity, job.board_bytes(amplitude), limit, need, "node" if field else "cell")
    n, ncomp = job.frames, (job.rows_per_unit if field else 9)
    board_nodes = job.units * job.nodes_per_unit
    seconds = dict(read=0.0, filter=0.0, table=0.0)
    board = None
    if amplitude and n:
        board = hp.DeviceBoard(backend, board_nodes, n) if hasattr(backend, "hi_pass_board_begin") else hp.HostBoard(board_nodes, n)
    series, groups, passes, said = None, [[]], 0, []
    try:
        gi = 0
        while gi < len(groups):
            files = {}
            for si, (i0, i1) in enumerate(strips):
                run = run_cls(backend, mesh, {**ns, key: [job.q], strip_key: (i0, i1)})
                try:
                    t = tick()
                    sample_frames(list(run.reads) if run.reads is not None else [job.q], [run])
                    seconds["read"] += tick() - t
                    passes += 1
                    session = run.sessions[job.q]
                    if n == 0:
                        if si == 0:
                            said.append(f"Hi-pass {job.q}: none of the {run.frames} recorded frames lies in the window and stride asked for: nothing written")
                        continue
                    if field:
                        first = hp.select_frames(run.times, run.dt, run.stride, run.t0, run.t1)[0]
                        session.select(first, n, run.stride)
                        ids = [i for i in run.point_ids if i0 <= i < i1]
                        if gi == 0 and ids:
                            run._write_traces(session, job.q, n, ids, [i - i0 for i in ids])
                    if series is None:
                        series = run.series_list(job.q, n, said.append)
                        groups = [[j] for j in range(len(series))] if amplitude and series else [list(range(len(series)))]
                    window = run.window
                    for j in groups[gi]:
                        viz, stages, rms = series[j]
                        t = tick()
                        run.apply(session, stages)
                        seconds["filter"] += tick() - t
                        _fill_series(files, run.writer, field, viz, n, ncomp, i0, session, board if amplitude else None,
                                     job.nodes_per_unit, rms, window, said if si == 0 else None)
                finally:
                    for s in run.sessions.values():
                        s.end()
            for f in files.values():
                f.close(run.dt_files, run.t0)
            if board is not None and series:
                viz, _, rms = series[groups[gi][0]]
                if not (rms and n < window):
                    t = tick()
                    run.writer.write_table(viz, hp.board_table(board, n, board_nodes, run.dt_files, run.t0))
                    seconds["table"] += tick() - t
            gi += 1
    finally:
        if board is not None:
            board.end()
    for line in said:
        out(line)
    label = hp.VIZ_TYPE[job.q] if field else hpt.VIZ_TYPE[job.q]
    out(f"Hi-pass {label} in strips: {len(strips)} strips of at most {strips[0][1] - strips[0][0]} {'nodes' if field else 'cells'} "
        f"({job.units} in all), the {len(hp.saved_times(ns))} frames read {passes} times; {seconds['read']:.2f} s reading, "
        f"{seconds['filter']:.2f} s filtering, {seconds['table']:.2f} s on tables")
    return dict(strips=len(strips), passes=passes, seconds=seconds)


def _fill_series(files: dict, writer, field: bool, viz: str, n: int, ncomp: int, i0: int, session, board, nodes_per_unit: int,
                 rms: bool, window: int, said) -> None:
    """The strip's block of every frame of ``<viz>.h5`` and, with a board, of ``<viz>_amplitude.h5`` (for a tensor also of
    ``<viz>_max_principal_amplitude.h5``); the amplitude fetches feed the board at the strip's first node."""
    make = _FieldSeries if field else _TensorSeries
    shape = (lambda a: a) if field else hpt.expand

    def series(name: str, nc: int):
        if name not in files:
            files[name] = make(writer, name, n, nc)
        return files[name]

    f = series(viz, ncomp)
    for k in range(n):
        f.fill(k, i0, shape(session.fetch("filtered", k)))
    if board is None:
        return
    if rms and n < window:
        if said is not None:
            said.append(f"Hi-pass {viz}: {n} frames recorded, fewer than the window of {window}: no amplitude written")
        return
    session.amplitude(window if rms else 0)
    board.attach(session, i0 * nodes_per_unit)
    try:
        a = series(f"{viz}_amplitude", ncomp)
        p = None if field else series(f"{viz}_max_principal_amplitude", 1)
        for k in range(n):
            if p is not None:
                p.fill(k, i0, session.fetch("magnitude", k))
            a.fill(k, i0, shape(session.fetch("amplitude", k)))
    finally:
        board.attach(session, -1)
