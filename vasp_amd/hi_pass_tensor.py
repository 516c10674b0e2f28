"""Band-pass filtered Green-Lagrange strain and Cauchy stress of the wall, their windowed RMS amplitude and the largest
principal value of that amplitude: the tensor files of `<results>/Visualization_hi_pass/`, libhdf5-free.

Counterpart of ``vasp-create-hi-pass-viz -q strain|stress``
[REF src/vasp/postprocessing/postprocessing_h5py/create_hi_pass_viz.py:92-95,110-120,218-230,246-325,658-663], which reads the
files of ``vasp-compute-stress`` back.  Here the six components the reference keeps of a tensor - 11, 12, 22, 23, 33, 31 - are
recorded per DG1 dof of every solid cell while the run steps (``HipBackend.hi_pass_begin_cells``, csrc/fsi_stress.hip), go
through the filter and the RMS of ``--hi-pass`` unchanged (csrc/fsi_band.hip), and the principal value of the amplitude is
taken on the device.  There is no host twin of the cell arithmetic: a backend without the device call is an error.

Per quantity and band, ``viz = GreenLagrangeStrain_<lo>_to_<hi>`` or ``TrueStress_<lo>_to_<hi>``:

* ``<viz>.h5``: ``<viz>/<viz>_k/vector``, float32 (cells * 4 * 9, 1) - the nine entries per dof expanded from the six rows as the
  reference does (11, 12, 31, 12, 22, 23, 31, 23, 33) - and under frame 0 ``cell_dofs``, ``x_cell_dofs``, ``cells``,
  ``mesh/{geometry,topology}`` as ``stress_strain.StressStrainWriter`` writes them for the same solid sub-mesh;
  ``<viz>.xdmf`` as ``create_checkpoint_xdmf_file`` writes it [REF postprocessing_h5py_common.py:594-682];
* with ``--hi-pass-amplitude``: ``<viz>_amplitude.{h5,xdmf}`` (the same layout, of the RMS amplitudes),
  ``<viz>_max_principal_amplitude.{h5,xdmf}`` (scalar DG1, (cells * 4, 1), the dof map of ``MaxPrincipalStrain`` for both
  quantities, as create_transformed_matrix takes it, :250-259) and ``<viz>.csv``, the percentile table of the principal
  amplitude over the dofs.  No PNG.

Every recorded frame is filtered and written (the reference's matrix drops the last saved frame, ``num_cols = num_ts - 1``).
The window is ``--hi-pass-tensor-window`` (default 50, the reference's fixed value for these quantities, :224); bands and
``--hi-pass-amplitude`` are those of ``--hi-pass``.  The reference loops over the bands only (:658-663): ``--hi-pass-multiband``,
the frame window / stride options and point ids act on d, v, p alone.
"""
from __future__ import annotations

from pathlib import Path
from typing import List

import numpy as np

from .h5lite import Dataset, Group, H5Series
from .hemodynamics import XDMF_FOOTER, _dg1_group, _xdmf_grid, _xdmf_head
from .hi_pass import (CSV_HEADER, SessionRun, amplitude_row, bands, design, frame_spacing, frame_start, frame_times, padlen_of,
                      restart_refusal, sha256_of)
from .mesh import FsiMesh
from .stress_strain import solid_cells, solid_submesh

VIZ_TYPE = {"strain": "GreenLagrangeStrain", "stress": "TrueStress"}        # [REF create_hi_pass_viz.py:92-95]
WINDOW = 50                                                                  # [REF create_hi_pass_viz.py:224]
SHORTCUT = 1e-8                                                              # [REF create_hi_pass_viz.py:307]
EXPAND = (0, 1, 5, 1, 2, 3, 5, 3, 4)            # rows 11, 12, 22, 23, 33, 31 -> the nine entries, row-major [REF :254-263]
D_V_P_ONLY = ("hi_pass_multiband", "hi_pass_pass_stop", "hi_pass_stride", "hi_pass_start_time", "hi_pass_end_time",
              "hi_pass_point_ids")


def quantities(v: dict) -> List[str]:
    q = v.get("hi_pass_tensor") or []
    q = [q] if isinstance(q, str) else list(q)
    bad = [x for x in q if x not in VIZ_TYPE]
    if bad:
        raise SystemExit(f"--hi-pass-tensor takes strain and / or stress, got {bad}")
    return [x for x in VIZ_TYPE if x in q]


def window(v: dict) -> int:
    w = v.get("hi_pass_tensor_window")
    return WINDOW if w is None else int(w)


def expand(frame: np.ndarray) -> np.ndarray:
    """(dofs, 6) rows of one frame -> (dofs, 9), the symmetric tensor row-major [REF create_hi_pass_viz.py:254-263]."""
    return np.asarray(frame).reshape(-1, 6)[:, EXPAND]


def principal_amplitude(amp: np.ndarray, max_eig) -> np.ndarray:
    """The rule of the device's principal-amplitude kernel on the host [REF create_hi_pass_viz.py:295-314]: per dof the
    tensor of ``expand``; exactly 0 where every entry is below 1e-8 in magnitude, else ``max_eig`` of it (a restatement of
    turtleFSI's ``get_eig`` on (..., 3, 3) arrays)."""
    T = expand(amp).reshape(-1, 3, 3).astype(np.float64)
    small = (np.abs(T) < SHORTCUT).all(axis=(1, 2))
    out = np.zeros(len(T))
    if (~small).any():
        out[~small] = max_eig(T[~small])
    return out


def hi_pass_tensor_refusal(v: dict, world: int, backend_cls) -> str:
    """Why ``--hi-pass-tensor`` cannot run with the resolved parameters ``v`` ('' if it can)."""
    quantities(v)
    if not v.get("save_step"):
        return "--hi-pass-tensor records the saved frames: it needs --save-step"
    if v.get("restart_folder"):
        why = restart_refusal(v, HiPassTensorRun.key, HiPassTensorRun.words)
        if why:
            return why
    if world > 1:
        return "--hi-pass-tensor runs on one rank only (WORLD_SIZE > 1)"
    if backend_cls is not None and not hasattr(backend_cls, "hi_pass_begin_cells"):
        return f"--hi-pass-tensor needs a backend with hi_pass_begin_cells ({getattr(backend_cls, '__name__', backend_cls)} has none)"
    if not v.get("hi_pass"):
        given = ["--" + k.replace("_", "-") for k in D_V_P_ONLY if v.get(k) is not None]
        if given:
            return (f"{', '.join(given)}: these options of --hi-pass act on d, v and p; --hi-pass-tensor writes every band of "
                    "--hi-pass-bands on every saved frame and nothing else")
    times, past = frame_times(v, HiPassTensorRun.key, HiPassTensorRun.words)
    frames = len(times)
    saves = f"saves {frames} frames"
    if v.get("restart_folder"):
        saves += f" ({past} saved before the restart and {len(times) - past} to come)"
    for lo, hi in bands(v):
        if frames < padlen_of(lo) + 1:
            return (f"--hi-pass-tensor: the run {saves}, the filter of band {lo:g} - {hi:g} Hz needs at least "
                    f"padlen + 1 = {padlen_of(lo) + 1}")
    if window(v) < 1:
        return "--hi-pass-tensor-window must be at least 1"
    if v.get("hi_pass_amplitude") and frames < window(v):
        return f"--hi-pass-amplitude: the run {saves}, fewer than the window of {window(v)} (--hi-pass-tensor-window)"
    return ""


class TensorWriter:
    """DG1 series in DOLFIN's ``write_checkpoint`` layout on the solid sub-mesh, as the reference's hi-pass tool writes them
    for strain and stress: ``<viz>/<viz>_k/vector`` float32 (h5py's default, create_hi_pass_viz.py:265,323), the dof map and
    the mesh under frame 0 in the types ``StressStrainWriter`` gives them (``hemodynamics._dg1_group``)."""

    def __init__(self, folder, geometry: np.ndarray, topology: np.ndarray):
        self.folder = Path(folder)
        self.folder.mkdir(parents=True, exist_ok=True)
        self.geometry, self.topology = geometry, topology

    def open(self, viz: str, ncomp: int) -> "TensorSeries":
        return TensorSeries(self, viz, ncomp)

    def write_series(self, viz: str, frames, num_ts: int, ncomp: int, time_between_files: float, start_t: float) -> None:
        """frames: an iterable of num_ts arrays of cells * 4 * ncomp values, dof-major; one frame in memory at a time."""
        series = self.open(viz, ncomp)
        try:
            for frame in frames:
                series.append(frame)
            if series.frames != num_ts:
                raise ValueError(f"{viz}: {series.frames} frames, expected {num_ts}")
        finally:
            series.close(time_between_files, start_t)

    def write_table(self, viz: str, table: np.ndarray) -> None:
        np.savetxt(self.folder / f"{viz}.csv", table, delimiter=",", header=CSV_HEADER)


class TensorSeries:
    """One series of ``TensorWriter``: ``append`` a frame at a time, ``close`` writes the XDMF of the frames appended."""

    def __init__(self, writer: TensorWriter, viz: str, ncomp: int):
        self.w, self.viz, self.ncomp, self.frames = writer, viz, ncomp, 0
        self._h5 = H5Series(writer.folder / f"{viz}.h5", Group(), viz)

    def append(self, frame) -> None:
        n = len(self.w.topology)
        values = np.asarray(frame, dtype=np.float64).reshape((n, 4, 3, 3) if self.ncomp == 9 else (n, 4))
        g = _dg1_group(values, self.w.geometry, self.w.topology, dofmap=self.frames == 0, celltype="tetrahedron")
        g["vector"] = Dataset(np.asarray(g["vector"].data).astype(np.float32))
        self._h5.append_group(f"{self.viz}_{self.frames}", g)
        self.frames += 1

    def reserve(self) -> int:
        """``append`` of a frame whose values come later, a block of cells at a time (``fill``); returns what ``fill`` takes."""
        n = len(self.w.topology)
        g = _dg1_group(np.zeros((1, 4, 3, 3) if self.ncomp == 9 else (1, 4)), self.w.geometry, self.w.topology, dofmap=self.frames == 0,
                       celltype="tetrahedron")
        g["vector"] = Dataset(np.zeros((n * 4 * self.ncomp, 1), dtype=np.float32))
        addr = self._h5.reserve_group(f"{self.viz}_{self.frames}", g, "vector")
        self.frames += 1
        return addr

    def fill(self, addr: int, cell0: int, values) -> None:
        """The values of cells ``cell0 ...`` (cells x 4 x ncomp, as ``append`` takes them) into a reserved frame."""
        block = np.asarray(values, dtype=np.float64).reshape(-1, 1).astype(np.float32)
        self._h5.fill(addr, 4 * (4 * self.ncomp * int(cell0)), block)

    def close(self, time_between_files: float, start_t: float) -> None:
        self._h5.close()
        n, nv = len(self.w.topology), len(self.w.geometry)
        grids = "".join(_xdmf_grid(self.viz, k, k * time_between_files + start_t, n, nv, self.ncomp, "tetrahedron")
                        for k in range(self.frames))
        (self.w.folder / f"{self.viz}.xdmf").write_text(_xdmf_head(self.viz) + grids + XDMF_FOOTER)


class HiPassTensorRun(SessionRun):
    """The driver's side of ``--hi-pass-tensor``: one session per quantity on the solid cells (``dx_s_id``, every region, as
    ``--stress-strain``), one recorded frame per saved frame, and at the end per band the filtered tensor, with
    ``--hi-pass-amplitude`` its amplitude, the largest principal value of the amplitude and its table.  Times in the files are
    ``k * dt * save_step``, as ``HiPassRun`` sets them without a frame window."""
    prefix, begin = "hi_pass", "begin_cells"
    file_stem = key = "hi_pass_tensor"
    option, words = "--hi-pass-tensor", "--hi-pass-tensor cannot be used with --restart-folder"
    reads = ("d",)

    def __init__(self, backend, mesh: FsiMesh, ns: dict):
        self.backend = backend
        self.quantities = quantities(ns)
        self.bands = bands(ns)
        self.amplitude = bool(ns.get("hi_pass_amplitude"))
        self.window = window(ns)
        self.dt_files = self.dt_sample = frame_spacing(ns)
        self.t0 = frame_start(ns)
        self.cells = solid_cells(mesh, ns["dx_s_id"])
        if len(self.cells) == 0:
            raise SystemExit(f"--hi-pass-tensor: no cell carries a solid marker (dx_s_id = {ns['dx_s_id']})")
        self.writer = TensorWriter(Path(ns["results_folder"]) / "Visualization_hi_pass", *solid_submesh(mesh, self.cells))
        # a strip (vasp_amd.hi_pass_strips): the session is opened on solid cells i0 .. i1 - 1; the writer keeps the whole sub-mesh
        self.strip = ns.get("hi_pass_tensor_strip")
        if self.strip is not None:
            self.cells = self.cells[self.strip[0]:self.strip[1]]
        self.open_sessions(backend, ns, lambda q: (self.cells,), self._no_host_session)

    @staticmethod
    def _no_host_session(q: str, capacity: int):
        raise SystemExit("--hi-pass-tensor needs a backend with hi_pass_begin_cells: the cell arithmetic has no host twin")

    def rows(self, q: str) -> int:
        return 24 * len(self.cells)

    def fingerprint(self, q: str) -> dict:
        return dict(dt_sample=self.dt_sample, rows=self.rows(q), cells=sha256_of(self.cells))

    def _write_band(self, out, session, viz: str, n: int, rms: bool) -> None:
        self.writer.write_series(viz, (expand(session.fetch("filtered", k)) for k in range(n)), n, 9, self.dt_files, self.t0)
        if not self.amplitude:
            return
        if rms and n < self.window:
            out(f"Hi-pass {viz}: {n} frames recorded, fewer than the window of {self.window}: no amplitude written")
            return
        session.amplitude(self.window if rms else 0)       # low-pass: the amplitude is the filtered tensor itself (:229-230)
        table = np.empty((n, 13))
        principal = self.writer.open(f"{viz}_max_principal_amplitude", 1)

        def amp_frames():
            for k in range(n):
                mag, mx, am = session.fetch("magnitude", k, True)
                table[k] = amplitude_row(k * self.dt_files + self.t0, mag, mx, am)
                principal.append(mag)
                yield expand(session.fetch("amplitude", k))

        try:
            self.writer.write_series(f"{viz}_amplitude", amp_frames(), n, 9, self.dt_files, self.t0)
        finally:
            principal.close(self.dt_files, self.t0)
        self.writer.write_table(viz, table)

    def series_list(self, q: str, n: int, out):
        """(viz, stages, rms) per band, as ``HiPassRun.series_list``: one series per band, no multiband chain."""
        series = []
        for lo, hi in self.bands:
            prm = design(self.dt_files, lo, hi)
            viz = f"{VIZ_TYPE[q]}_{prm['name']}"
            if n <= prm["padlen"]:
                out(f"Hi-pass {viz}: {n} frames recorded, the filter needs more than {prm['padlen']}: nothing written")
                continue
            series.append((viz, [prm], prm["btype"] != "lowpass"))
        return series

    @staticmethod
    def apply(session, stages) -> None:
        for prm in stages:
            session.filter(prm["b"], prm["a"], prm["zi"], prm["padlen"])

    def write(self, out) -> None:
        n = self.frames
        if n == 0:
            out("Hi-pass tensors: no frame was recorded, nothing written")
            return
        for q, session in self.sessions.items():
            for viz, stages, rms in self.series_list(q, n, out):
                self.apply(session, stages)
                self._write_band(out, session, viz, n, rms)
        out(f"Hi-pass tensors of {n} frames ({', '.join(self.quantities)}) written to {self.writer.folder}")
