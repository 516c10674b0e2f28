"""Vortex identification of a run on its fluid cells: `<results>/VortexMetrics/`, libhdf5-free.

``--hi-pass-vortex``: the structures of the flow - the Q-criterion, the vorticity, the helicity and its localised normalised
form (LNH) - and their bulk descriptors, the kinetic-energy, enstrophy and helicity curves over time and the helicity indices
h1 to h4 of Gallo et al. (J. Biomech. 2012).  Nothing in the reference forms these.  They are closed, in NumPy, from five
device quantities per cell and frame, all exact cell means of the P2 velocity (``HipBackend.hi_pass_cell_vortex``,
csrc/fsi_vortex.hip; the NumPy twin is ``hi_pass.cell_vortex`` / ``HostBandSession.cell_vortex``): field 0 ``Q``
= 0.5 (|Omega|^2 - |S|^2), 1 the enstrophy ``|omega|^2``, 2 the helicity ``v . omega``, 3 its absolute value - of the cell mean
of each frame, not the cell mean of ``|v . omega|`` -, 4 ``|v|^2``; on the velocity history a ``--hi-pass v`` session holds.
The bulk integrals are the device's ordered sums over the fluid cells with the cell volumes as weights
(``hi_pass_cell_weights``, ``hi_pass.cell_wsum``).

One frame per cell file, over the selected frames:

    q_criterion_avg      time mean of field 0                      helicity_avg         time mean of field 2
    vorticity_rms        sqrt(time mean of field 1)                helicity_intensity   time mean of field 3
    kinetic_energy_avg   0.5 * time mean of field 4                helicity_balance     helicity_avg / helicity_intensity, 0 where that is 0

With ``--hi-pass-vortex-series`` per selected frame, from one call per frame that is written before the next is made:

    q_criterion  field 0        vorticity  sqrt(field 1)        helicity  field 2
    lnh          field 2 / sqrt(field 4 * field 1), 0 where the product is 0; |lnh| <= 1 by Cauchy-Schwarz, all three being means
                 over the same cell

With ``--hi-pass-phase-average``: ``q_criterion_phase_mean``, ``period`` frames, field 0 of each frame of the phase mean, and
``vorticity_rms_fluctuation``, sqrt of the time mean of field 1 of the fluctuation u'.

``vortex.csv``: per selected frame the time, the fluid volume and the integrals over it of 0.5 |v|^2, |omega|^2, the helicity,
its absolute value and Q.  ``vortex_summary.csv``: the table of ``flow_metrics.csv`` for the one-frame cell files.
``helicity_indices.csv``: h1, the mean over the frames of the integral of the helicity over the volume; h2, the same of its
absolute value; h3 = h1 / h2 (0 if h2 is 0); h4 = |h3|.

``--hi-pass-vortex-configuration current`` takes all of it in the current configuration ``x = X + d(X)`` of the ALE mesh, as
``--hi-pass-flow-metrics-configuration current`` takes the dissipation (default: ``reference``, the undeformed mesh; the two
options are independent).  It needs ``d`` among the ``--hi-pass`` quantities.  The velocity gradient is ``grad_X v F^-1``,
``F = I + grad_X d``, and the five fields are means over the **deformed** cell, on the 14-point rule of degree 5
(``HipBackend.hi_pass_cell_vortex_current``, k_cell_vortex_current; the twin is ``hi_pass.cell_vortex_current`` /
``HostBandSession.cell_vortex_current``).  A sixth field is the deformed cell's volume over the undeformed.  The files and the
closing formulas are the same, and:

    volume_ratio         time mean of field 5
    vortex.csv           the volume is that of the current fluid domain at the frame, the integrals are over it: the device's sums
                         of the integrals per undeformed volume, with the undeformed volumes as weights
    helicity indices     each frame's integral over its own current volume
    vortex_summary.csv   the weights are volume * volume_ratio

Frame k of the velocity is paired with the recorded displacement of the same saved frame, also where the velocity is the
fluctuation; the phase mean of the velocity with the phase mean of the displacement.

Out of scope: partitioned contexts and a history that goes through the session in strips of rows.  Nothing is clamped: a NaN
stays a NaN.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional

import numpy as np

from .flow_metrics import FlowMetricsWriter, barycentric_gradients, cell_volumes, fluid_cells, submesh, summary_row
from .hi_pass import ordered_mean
from .mesh import FsiMesh

NEEDS_V = "--hi-pass-vortex needs v among the --hi-pass quantities: the vorticity is formed from the velocity history"
NEEDS_DEG2 = ("--hi-pass-vortex needs --save-deg 2: at save_deg 1 the session holds the vertices only, a cell's gradient needs its ten "
              "P2 nodes")
NEEDS_VORTEX = "--hi-pass-vortex-series writes the per-frame fields of --hi-pass-vortex: it needs that option"
VORTEX_STRIPS = ("--hi-pass-vortex: the history goes through the session in strips of rows, which do not keep a cell's 30 rows together "
                 "(give it room with --history-memory, or fewer frames with --stride)")
CURVES_HEADER = ("time (s), volume, integral of 0.5 |v|^2, integral of |omega|^2, integral of helicity, integral of |helicity|, "
                 "integral of Q")
INDICES_HEADER = "h1, h2, h3, h4"
NEEDS_D = ("--hi-pass-vortex-configuration current needs d among the --hi-pass quantities: the current configuration is "
           "x = X + d, formed from the displacement history")
NEEDS_VORTEX_CONFIGURATION = "--hi-pass-vortex-configuration chooses the configuration of --hi-pass-vortex: it needs that option"
CONFIGURATIONS = ("reference", "current")
SERIES_FILES = ("q_criterion", "vorticity", "helicity", "lnh")
Q, ENSTROPHY, HELICITY, ABS_HELICITY, SPEED2, VOLUME_RATIO = range(6)      # hi_pass.VORTEX_CURRENT_FIELDS


def configuration(v: dict) -> str:
    """'reference' (the default) or 'current': ``--hi-pass-vortex-configuration``."""
    word = v.get("hi_pass_vortex_configuration") or "reference"
    if word not in CONFIGURATIONS:
        raise SystemExit(f"--hi-pass-vortex-configuration takes {' or '.join(CONFIGURATIONS)}, got {word!r}")
    return word


def refusal(v: dict, quantities: List[str]) -> str:
    """Why ``--hi-pass-vortex`` cannot run with the resolved parameters ('' if it can, or without the option)."""
    if not v.get("hi_pass_vortex"):
        return NEEDS_VORTEX if v.get("hi_pass_vortex_series") else NEEDS_VORTEX_CONFIGURATION if v.get("hi_pass_vortex_configuration") else ""
    if "v" not in quantities:
        return NEEDS_V
    if int(v.get("save_deg") or 1) != 2:
        return NEEDS_DEG2
    if configuration(v) == "current" and "d" not in quantities:
        return NEEDS_D
    return ""


# ------------------------------------------------------------------------------------------------
# the closing formulas
# ------------------------------------------------------------------------------------------------

def ratio_or_zero(num, den) -> np.ndarray:
    """``num / den``, 0 where ``den`` is 0; a NaN stays a NaN."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(den == 0.0, 0.0, num / np.where(den == 0.0, 1.0, den))


def mean_fields(mean: np.ndarray) -> Dict[str, np.ndarray]:
    """The one-frame cell files from the time means of the five fields, (5, cells) or the first five rows of (6, cells)."""
    with np.errstate(all="ignore"):
        return dict(q_criterion_avg=mean[Q], vorticity_rms=np.sqrt(mean[ENSTROPHY]), helicity_avg=mean[HELICITY],
                    helicity_intensity=mean[ABS_HELICITY], helicity_balance=ratio_or_zero(mean[HELICITY], mean[ABS_HELICITY]),
                    kinetic_energy_avg=0.5 * mean[SPEED2])


def frame_fields(frame: np.ndarray) -> Dict[str, np.ndarray]:
    """The per-frame files ``SERIES_FILES`` from the five fields of one frame, (5, cells) or the first five rows of (6, cells)."""
    with np.errstate(all="ignore"):
        return dict(q_criterion=frame[Q], vorticity=np.sqrt(frame[ENSTROPHY]), helicity=frame[HELICITY],
                    lnh=ratio_or_zero(frame[HELICITY], np.sqrt(frame[SPEED2] * frame[ENSTROPHY])))


def curve_row(time: float, volume: float, sums: np.ndarray) -> List[float]:
    """A line of ``vortex.csv`` from the five weighted sums of one frame."""
    return [float(time), float(volume), 0.5 * float(sums[SPEED2]), float(sums[ENSTROPHY]), float(sums[HELICITY]), float(sums[ABS_HELICITY]),
            float(sums[Q])]


def helicity_indices(curves: np.ndarray) -> List[float]:
    """h1 .. h4 from the lines of ``vortex.csv``: the ordered means over the frames of the helicity and of its absolute value,
    each integrated over the volume and divided by it; their ratio (0 if h2 is 0) and its absolute value."""
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 7)
    with np.errstate(all="ignore"):
        h1, h2 = float(ordered_mean(curves[:, 4] / curves[:, 1])), float(ordered_mean(curves[:, 5] / curves[:, 1]))
        h3 = 0.0 if h2 == 0.0 else h1 / h2
    return [h1, h2, h3, abs(h3)]


# ------------------------------------------------------------------------------------------------
# the driver's side
# ------------------------------------------------------------------------------------------------

class VortexMetrics:
    """What ``HiPassRun`` holds for the option: the fluid cells and their volumes; ``collect`` and ``collect_phase`` take the
    fields from the velocity session and stream the per-frame files, ``write`` closes the rest into the files, the tables and
    one log line."""

    def __init__(self, mesh: FsiMesh, ns: dict):
        self.mesh = mesh
        self.cells = fluid_cells(mesh, ns["dx_f_id"])
        if len(self.cells) == 0:
            raise SystemExit(f"--hi-pass-vortex: no cell carries a fluid marker (dx_f_id = {ns['dx_f_id']})")
        self.volume = cell_volumes(mesh, self.cells)
        self.series = bool(ns.get("hi_pass_vortex_series"))
        self.configuration = configuration(ns)
        self.writer = FlowMetricsWriter(Path(ns["results_folder"]) / "VortexMetrics", *submesh(mesh, self.cells))
        self.mean: Optional[np.ndarray] = None
        self.curves: Optional[np.ndarray] = None
        self.phase: Optional[dict] = None

    def attach(self, session, device: bool, grad=None, attached: bool = False) -> None:
        """The fluid cells and their volumes to the velocity session - the list ``FlowMetrics.attach`` attaches: the device
        forms the gradients itself, the host twin is handed ``grad`` (default: those of the undeformed mesh).  ``attached``: the
        flow metrics have attached that list already; only the weights are added."""
        if not attached and device:
            session.cells(self.cells)
        elif not attached:
            session.cells(self.mesh.tet_nodes[self.cells], barycentric_gradients(self.mesh, self.cells) if grad is None else grad)
        session.cell_weights(self.volume)

    def fields(self, session, geometry, series: str, *frames):
        """``(cells, sums)`` of a series of the velocity session in the configuration asked for; ``geometry``: the session of d.
        (5, n) and (5,) in the reference configuration; (6, n) and (6,) in the current one, the last sum being the current
        volume of the fluid cells."""
        if self.configuration == "reference":
            return session.cell_vortex(series, *frames)
        return session.cell_vortex_current(series, geometry, *frames)

    def collect(self, session, n: int, time_between_files: float, start_t: float, geometry=None) -> None:
        """The time means of the ``n`` selected raw frames, and frame by frame the bulk integrals and - with
        ``--hi-pass-vortex-series`` - the per-frame files: one call per frame, written before the next is made.  The volume of
        a line of ``vortex.csv`` is that of the undeformed fluid cells or, in the current configuration, the frame's own."""
        self.mean = np.asarray(self.fields(session, geometry, "raw")[0])
        volume = float(np.sum(self.volume))
        self.curves = np.empty((n, 7))
        files = {name: self.writer.open_series(name) for name in SERIES_FILES} if self.series else {}
        try:
            for k in range(n):
                frame, sums = self.fields(session, geometry, "raw", k, 1, 1, self.series, True)
                if self.configuration == "current":
                    volume = float(sums[VOLUME_RATIO])
                self.curves[k] = curve_row(start_t + k * time_between_files, volume, sums)
                if self.series:
                    for name, values in frame_fields(np.asarray(frame)).items():
                        files[name].append(str(k), values.reshape(-1, 1).astype(np.float32))
        except BaseException:
            for series in files.values():
                series.close()
            raise
        for name, series in files.items():
            self.writer.close_series(name, series, n, time_between_files, start_t)

    def collect_phase(self, session, period: int, geometry=None) -> None:
        """With the session's phase average in place: Q of every frame of the phase mean, the enstrophy of the fluctuation.  In
        the current configuration the phase mean goes with the phase mean of d, the fluctuation with the recorded frames of d."""
        self.phase = dict(q_mean=np.stack([np.asarray(self.fields(session, geometry, "phase_mean", j, 1, 1)[0])[Q] for j in range(period)]),
                          enstrophy=np.asarray(self.fields(session, geometry, "series")[0])[ENSTROPHY])

    def write(self, out, time_between_files: float, start_t: float) -> None:
        metrics = mean_fields(self.mean)
        volume = self.volume
        if self.configuration == "current":
            metrics["volume_ratio"] = self.mean[VOLUME_RATIO]
            with np.errstate(all="ignore"):
                volume = self.volume * self.mean[VOLUME_RATIO]
        if self.phase is not None:
            metrics["q_criterion_phase_mean"] = self.phase["q_mean"]
            with np.errstate(all="ignore"):
                metrics["vorticity_rms_fluctuation"] = np.sqrt(self.phase["enstrophy"])
        rows = []
        for name, values in metrics.items():
            self.writer.write(name, values, time_between_files, start_t)
            if values.ndim == 1:
                rows.append((name, *summary_row(values, volume, self.cells)))
        self.writer.write_table(rows, "vortex_summary.csv")
        with open(self.writer.folder / "vortex.csv", "w") as f:
            f.write("# " + CURVES_HEADER + "\n")
            for row in self.curves:
                f.write(", ".join(repr(float(x)) for x in row) + "\n")
        h = helicity_indices(self.curves)
        (self.writer.folder / "helicity_indices.csv").write_text("# " + INDICES_HEADER + "\n" + ", ".join(repr(x) for x in h) + "\n")
        written = list(metrics) + (list(SERIES_FILES) if self.series else [])
        top = {r[0]: r[3] for r in rows}
        out(f"Vortex metrics of {len(self.cells)} fluid cells over {len(self.curves)} frames in the {self.configuration} configuration "
            f"({', '.join(written)}) written to "
            f"{self.writer.folder}: max q_criterion_avg = {top['q_criterion_avg']:.4g}, max vorticity_rms = {top['vorticity_rms']:.4g}, "
            f"h1 = {h[0]:.4g}, h2 = {h[1]:.4g}, h3 = {h[2]:.4g}")
