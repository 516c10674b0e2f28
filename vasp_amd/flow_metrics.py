"""Flow and simulation metrics of a run on its fluid cells: `<results>/FlowMetrics/`, libhdf5-free.

``--hi-pass-flow-metrics``: is the mesh and the time step fine enough for what the flow does, and where does the fluctuating
motion dissipate.  Nothing in the reference forms these; the sister tool VaMPy does for a rigid-wall run ("flow and simulation
metrics").  Here they are closed, in NumPy, from one device quantity per cell: ``R(x)``, the mean over the frames of a series x
of the exact cell mean of ``2 S:S``, ``S = sym(grad x)`` (``HipBackend.hi_pass_cell_rate``, csrc/fsi_rate.hip; its NumPy twin
is ``hi_pass.cell_rate`` / ``HostBandSession.cell_rate``), on the velocity history a ``--hi-pass v`` session holds - the raw
frames, a band-passed series, and with ``--hi-pass-phase-average`` the phase mean and the fluctuation u'.  By default the
gradient is that of the undeformed geometry, as in the hemodynamics of the reference.

``--hi-pass-flow-metrics-configuration current`` takes every rate in the current configuration ``x = X + d(X)`` of the ALE mesh
instead: of a series w ``S = sym(grad_X w F^-1)``, ``F = I + grad_X d``, averaged over the deformed cell
(``HipBackend.hi_pass_cell_rate_current``, k_cell_rate_current; the twin is ``hi_pass.cell_rate_current`` /
``HostBandSession.cell_rate_current``), with the displacement history of ``--hi-pass d`` on the same nodes and frames - each
velocity frame with the displacement of the same frame, the phase mean with the displacement's phase mean.  Every metric keeps
its name and its closing formula.  Two more cell files come from the raw call: ``volume_ratio``, the mean over the frames of
the deformed cell's volume over the undeformed - how much the ALE extension compresses the fluid mesh - and ``min_jacobian``,
the smallest ``det F`` met in the cell - how close it comes to inverting one; the table's volume weights become
``volume * volume_ratio``.  h stays the diameter of the **undeformed** cell in both configurations.

This module holds the fluid cells of ``dx_f_id`` and their sub-mesh, per cell the kinematic viscosity ``nu = mu_f / rho_f`` of
its region, the cell diameter h (twice the circumradius, what ``FsiMesh.hmin`` takes the minimum of) and the volume, the
closing formulas, and the cell-centred writer.  With dt the solver's time step:

    strain_rate            sqrt(R(raw))                         l_plus    h sqrt(strain_rate / nu)
    dissipation            nu R(raw)                            t_plus    dt strain_rate
    turbulent_dissipation  eps' = nu R(u')                      mean_flow_dissipation   nu * mean over the phases of R(mean)
    kolmogorov_length      eta = (nu^3 / eps')^(1/4)            kolmogorov_time         tau = (nu / eps')^(1/2)
    kolmogorov_velocity    (nu eps')^(1/4)                      length_ratio h / eta,   time_ratio dt / tau
    turbulent_dissipation_phase_mean   ``period`` frames: nu times the mean over the cycles of R(u') at each phase
    dissipation_{lo}_to_{hi}           nu R(band-passed velocity), per band of ``--hi-pass-bands``

Nothing is clamped: where eps' = 0 the Kolmogorov scales are IEEE inf and the ratios 0, a NaN stays a NaN.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

from .h5lite import Dataset, Group, H5Series
from .mesh import FsiMesh

CSV_HEADER = "metric, volume-weighted mean, minimum, maximum, cell with the maximum"


def as_list(x) -> list:
    return list(x) if isinstance(x, (list, tuple, np.ndarray)) else [x]


def fluid_cells(mesh: FsiMesh, fluid_ids) -> np.ndarray:
    """The cells whose marker is in ``fluid_ids`` (an int or a list, as ``dx_f_id``), ascending."""
    return np.nonzero(np.isin(mesh.cell_markers, np.asarray(as_list(fluid_ids))))[0]


def submesh(mesh: FsiMesh, cells) -> Tuple[np.ndarray, np.ndarray]:
    """(geometry (nv, 3), topology (n, 4)) of the listed cells: the vertices they use, compacted in ascending order."""
    used, topo = np.unique(mesh.tets[np.asarray(cells)], return_inverse=True)
    return np.ascontiguousarray(mesh.coords[used], dtype=np.float64), topo.reshape(-1, 4).astype(np.int64)


def kinematic_viscosity(mesh: FsiMesh, cells, v: dict) -> np.ndarray:
    """``mu_f / rho_f`` of the region of every listed cell: region i is the cells marked ``dx_f_id[i]``, with entry i of
    ``mu_f`` and ``rho_f`` where they are lists of more than one (``monolithic.build_properties``)."""
    ids, mu, rho = as_list(v["dx_f_id"]), as_list(v["mu_f"]), as_list(v["rho_f"])
    nu = np.full(len(cells), np.nan)
    markers = mesh.cell_markers[np.asarray(cells)]
    for i, marker in enumerate(ids):
        nu[markers == marker] = float(mu[i if len(mu) > 1 else 0]) / float(rho[i if len(rho) > 1 else 0])
    return nu


def cell_diameters(mesh: FsiMesh, cells) -> np.ndarray:
    """Twice the circumradius of every listed cell: the cell diameter whose minimum over the mesh is ``FsiMesh.hmin``."""
    x = mesh.coords[mesh.tets[np.asarray(cells)]]
    a, b, c = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    num = (np.einsum("ij,ij->i", a, a)[:, None] * np.cross(b, c) + np.einsum("ij,ij->i", b, b)[:, None] * np.cross(c, a)
           + np.einsum("ij,ij->i", c, c)[:, None] * np.cross(a, b))
    den = 2.0 * np.einsum("ij,ij->i", a, np.cross(b, c))
    return 2.0 * np.linalg.norm(num, axis=1) / np.abs(den)


def cell_volumes(mesh: FsiMesh, cells) -> np.ndarray:
    x = mesh.coords[mesh.tets[np.asarray(cells)]]
    return np.abs(np.einsum("ij,ij->i", x[:, 1] - x[:, 0], np.cross(x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]))) / 6.0


def barycentric_gradients(mesh: FsiMesh, cells) -> np.ndarray:
    """(n, 4, 3): the gradients of the barycentric coordinates of the listed cells in the undeformed geometry - what the host
    twin is handed where there is no device to form them (``HipBackend.hi_pass_cells`` returns the device's own)."""
    x = mesh.coords[mesh.tets[np.asarray(cells)]]
    J = np.stack([x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]], axis=1)      # rows x_k - x_0
    inv = np.linalg.inv(J)                                                             # grad L_k = column k - 1
    g = np.empty((len(x), 4, 3))
    g[:, 1:] = inv.transpose(0, 2, 1)
    g[:, 0] = -((g[:, 1] + g[:, 2]) + g[:, 3])
    return g


# ------------------------------------------------------------------------------------------------
# the closing formulas
# ------------------------------------------------------------------------------------------------

def strain_metrics(rate_raw, nu, h, dt: float) -> Dict[str, np.ndarray]:
    """strain_rate, dissipation, l_plus, t_plus from ``R(raw)``."""
    with np.errstate(all="ignore"):
        strain = np.sqrt(np.asarray(rate_raw, dtype=np.float64))
        return dict(strain_rate=strain, dissipation=nu * rate_raw, l_plus=h * np.sqrt(strain / nu), t_plus=dt * strain)


def turbulence_metrics(rate_fluctuation, rate_phase_mean, nu, h, dt: float) -> Dict[str, np.ndarray]:
    """The metrics of the phase-averaged decomposition from ``R(u')`` and the mean over the phases of ``R(mean)``."""
    with np.errstate(all="ignore"):
        eps = nu * np.asarray(rate_fluctuation, dtype=np.float64)
        eta = np.sqrt(np.sqrt(nu * nu * nu / eps))
        tau = np.sqrt(nu / eps)
        return dict(turbulent_dissipation=eps, mean_flow_dissipation=nu * rate_phase_mean, kolmogorov_length=eta, kolmogorov_time=tau,
                    kolmogorov_velocity=np.sqrt(np.sqrt(nu * eps)), length_ratio=h / eta, time_ratio=dt / tau)


def summary_row(values, volumes, cells) -> Tuple[float, float, float, int]:
    """(volume-weighted mean, minimum, maximum, mesh cell that holds the maximum) of one value per cell."""
    with np.errstate(all="ignore"):
        values = np.asarray(values, dtype=np.float64)
        k = int(np.argmax(values))
        return float(np.sum(values * volumes) / np.sum(volumes)), float(values.min()), float(values.max()), int(cells[k])


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------

def xdmf_text(name: str, num_ts: int, time_between_files: float, start_t: float, n_cells: int, n_nodes: int) -> str:
    """The series layout of ``hi_pass.xdmf_text`` with one scalar per cell: ``Center="Cell"``."""
    text = f'''<?xml version="1.0"?>
<!DOCTYPE Xdmf SYSTEM "Xdmf.dtd" []>
<Xdmf Version="3.0" xmlns:xi="http://www.w3.org/2001/XInclude">
  <Domain>
    <Grid Name="TimeSeries_{name}" GridType="Collection" CollectionType="Temporal">
      <Grid Name="mesh" GridType="Uniform">
        <Topology NumberOfElements="{n_cells}" TopologyType="Tetrahedron" NodesPerElement="4">
          <DataItem Dimensions="{n_cells} 4" NumberType="UInt" Format="HDF">{name}.h5:/Mesh/0/mesh/topology</DataItem>
        </Topology>
        <Geometry GeometryType="XYZ">
          <DataItem Dimensions="{n_nodes} 3" Format="HDF">{name}.h5:/Mesh/0/mesh/geometry</DataItem>
        </Geometry>
'''
    for idx in range(num_ts):
        text += f'''        <Time Value="{idx * time_between_files + start_t}" />
        <Attribute Name="{name}" AttributeType="Scalar" Center="Cell">
          <DataItem Dimensions="{n_cells} 1" Format="HDF">{name}.h5:/VisualisationVector/{idx}</DataItem>
        </Attribute>
      </Grid>
'''
        if idx < num_ts - 1:
            text += f'''      <Grid>
        <xi:include xpointer="xpointer(//Grid[@Name=&quot;TimeSeries_{name}&quot;]/Grid[1]/*[self::Topology or self::Geometry])" />
'''
    return text + "    </Grid>\n  </Domain>\n</Xdmf>\n"


class FlowMetricsWriter:
    """``<results>/FlowMetrics/``: per metric ``<name>.h5`` with ``Mesh/0/mesh/{geometry f32, topology i32}`` of the fluid
    sub-mesh and ``VisualisationVector/<k>`` f32 (cells, 1), the conventions of ``hi_pass.HiPassWriter``, and ``<name>.xdmf``
    with ``Attribute Center="Cell"``; and the table ``flow_metrics.csv``.  (``vortex.VortexMetrics`` writes
    ``<results>/VortexMetrics/`` with it.)"""

    def __init__(self, folder, geometry: np.ndarray, topology: np.ndarray):
        self.folder = Path(folder)
        self.folder.mkdir(parents=True, exist_ok=True)
        self.geometry = np.ascontiguousarray(geometry, dtype=np.float32)
        self.topology = np.ascontiguousarray(topology, dtype=np.int32)

    def open_series(self, name: str) -> H5Series:
        """``<name>.h5`` with the sub-mesh, open for ``append(str(k), (cells, 1) f32)``; ``close_series`` ends it."""
        meshg, zero, inner, root = Group(), Group(), Group(), Group()
        inner["geometry"] = Dataset(self.geometry)
        inner["topology"] = Dataset(self.topology)
        zero["mesh"] = inner
        meshg["0"] = zero
        root["Mesh"] = meshg
        return H5Series(self.folder / f"{name}.h5", root, "VisualisationVector")

    def close_series(self, name: str, series: H5Series, count: int, time_between_files: float = 0.0, start_t: float = 0.0) -> None:
        series.close()
        (self.folder / f"{name}.xdmf").write_text(xdmf_text(name, count, time_between_files, start_t, len(self.topology), len(self.geometry)))

    def write(self, name: str, frames, time_between_files: float = 0.0, start_t: float = 0.0) -> None:
        """frames: (cells,) for one value per cell at ``start_t``, or (k, cells) for a series."""
        frames = np.atleast_2d(np.asarray(frames, dtype=np.float64))
        if frames.shape[1] != len(self.topology):
            raise ValueError(f"{name}: {frames.shape[1]} values, the fluid has {len(self.topology)} cells")
        series = self.open_series(name)
        try:
            for k, frame in enumerate(frames):
                series.append(str(k), frame.reshape(-1, 1).astype(np.float32))
        except BaseException:
            series.close()
            raise
        self.close_series(name, series, len(frames), time_between_files, start_t)

    def write_table(self, rows: List[Tuple[str, float, float, float, int]], file_name: str = "flow_metrics.csv") -> None:
        with open(self.folder / file_name, "w") as f:
            f.write(CSV_HEADER + "\n")
            for name, mean, lo, hi, cell in rows:
                f.write(f"{name}, {mean!r}, {lo!r}, {hi!r}, {cell}\n")


# ------------------------------------------------------------------------------------------------
# the driver's side
# ------------------------------------------------------------------------------------------------

NEEDS_V = "--hi-pass-flow-metrics needs v among the --hi-pass quantities: the metrics are formed from the velocity history"
NEEDS_DEG2 = ("--hi-pass-flow-metrics needs --save-deg 2: at save_deg 1 the session holds the vertices only, a cell's gradient needs "
              "its ten P2 nodes")


NEEDS_D = ("--hi-pass-flow-metrics-configuration current needs d among the --hi-pass quantities: the current configuration is "
           "x = X + d, formed from the displacement history")
NEEDS_METRICS = "--hi-pass-flow-metrics-configuration chooses the configuration of --hi-pass-flow-metrics: it needs that option"
CONFIGURATIONS = ("reference", "current")


def configuration(v: dict) -> str:
    """'reference' (the default) or 'current': ``--hi-pass-flow-metrics-configuration``."""
    word = v.get("hi_pass_flow_metrics_configuration") or "reference"
    if word not in CONFIGURATIONS:
        raise SystemExit(f"--hi-pass-flow-metrics-configuration takes {' or '.join(CONFIGURATIONS)}, got {word!r}")
    return word


def refusal(v: dict, quantities: List[str]) -> str:
    """Why ``--hi-pass-flow-metrics`` cannot run with the resolved parameters ('' if it can, or without the option)."""
    if not v.get("hi_pass_flow_metrics"):
        return NEEDS_METRICS if v.get("hi_pass_flow_metrics_configuration") else ""
    if "v" not in quantities:
        return NEEDS_V
    if int(v.get("save_deg") or 1) != 2:
        return NEEDS_DEG2
    if configuration(v) == "current" and "d" not in quantities:
        return NEEDS_D
    return ""


class FlowMetrics:
    """What ``HiPassRun`` holds for the option: the fluid cells, their constants and the rates it collects at ``finish``;
    ``write`` closes them into the files, the table and one log line."""

    def __init__(self, mesh: FsiMesh, ns: dict):
        self.mesh = mesh
        self.cells = fluid_cells(mesh, ns["dx_f_id"])
        if len(self.cells) == 0:
            raise SystemExit(f"--hi-pass-flow-metrics: no cell carries a fluid marker (dx_f_id = {ns['dx_f_id']})")
        self.nu = kinematic_viscosity(mesh, self.cells, ns)
        self.h, self.volume = cell_diameters(mesh, self.cells), cell_volumes(mesh, self.cells)
        self.dt = float(ns["dt"])
        self.configuration = configuration(ns)
        self.volume_ratio: Optional[np.ndarray] = None       # with 'current', from the raw call
        self.min_jacobian: Optional[np.ndarray] = None
        self.writer = FlowMetricsWriter(Path(ns["results_folder"]) / "FlowMetrics", *submesh(mesh, self.cells))
        self.raw: Optional[np.ndarray] = None
        self.bands: Dict[str, np.ndarray] = {}
        self.phase: Optional[dict] = None

    def attach(self, session, device: bool) -> None:
        """The fluid cells to the velocity session: the device forms the gradients itself, the host twin is handed them."""
        if device:
            session.cells(self.cells)
        else:
            session.cells(self.mesh.tet_nodes[self.cells], barycentric_gradients(self.mesh, self.cells))

    def rate(self, session, geometry, series: str, *frames) -> np.ndarray:
        """``R`` of a series of the velocity session in the configuration asked for; ``geometry``: the session of d.  In the
        current configuration the raw series over all its frames also leaves the volume ratio and the smallest det F."""
        if self.configuration == "reference":
            return session.cell_rate(series, *frames)
        rate, volume_ratio, min_jacobian = session.cell_rate_current(series, geometry, *frames)
        if series == "raw" and not frames:
            self.volume_ratio, self.min_jacobian = volume_ratio, min_jacobian
        return rate

    def write(self, out, time_between_files: float, start_t: float) -> None:
        metrics: Dict[str, np.ndarray] = {}
        if self.raw is not None:
            metrics.update(strain_metrics(self.raw, self.nu, self.h, self.dt))
        volume = self.volume
        if self.volume_ratio is not None:
            metrics.update(volume_ratio=self.volume_ratio, min_jacobian=self.min_jacobian)
            with np.errstate(all="ignore"):
                volume = self.volume * self.volume_ratio
        if self.phase is not None:
            metrics.update(turbulence_metrics(self.phase["fluctuation"], self.phase["mean"], self.nu, self.h, self.dt))
            metrics["turbulent_dissipation_phase_mean"] = self.nu[None, :] * self.phase["cycle_mean"]
        for name, rate in self.bands.items():
            metrics[f"dissipation_{name}"] = self.nu * rate
        rows = []
        for name, values in metrics.items():
            self.writer.write(name, values, time_between_files, start_t)
            if values.ndim == 1:
                rows.append((name, *summary_row(values, volume, self.cells)))
            else:
                rows.extend((f"{name}[{j}]", *summary_row(frame, volume, self.cells)) for j, frame in enumerate(values))
        self.writer.write_table(rows)
        top = {r[0]: r[3] for r in rows}
        said = ", ".join(f"max {k} = {top[k]:.4g}" for k in ("l_plus", "t_plus", "length_ratio") if k in top)
        out(f"Flow metrics of {len(self.cells)} fluid cells in the {self.configuration} configuration ({', '.join(metrics)}) written to "
            f"{self.writer.folder}: {said}")
