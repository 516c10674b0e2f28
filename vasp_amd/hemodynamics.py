"""Hemodynamic indices of a run: the boundary facets of the fluid, their triangle mesh and the files of
`<results>/Hemodynamic_indices/`, libhdf5-free.

Counterpart of ``vasp-compute-hemo`` [REF src/vasp/postprocessing/postprocessing_fenics/compute_hemodynamics.py:160-372],
whose arithmetic runs on the device during the run (``HipBackend.hemodynamics_*``, csrc/fsi_hemo.hip).  What is written:

* ``WSS.{h5,xdmf}``: the time series of the sampled frames, ``/WSS/WSS_k/vector`` (k = 0, 1, ...), in DOLFIN's
  ``XDMFFile.write_checkpoint`` layout for a vector DG1 function on triangles; ``cell_dofs``, ``x_cell_dofs``, ``cells`` and
  ``mesh/{geometry,topology}`` sit under ``WSS_0``, where the reference's consumer reads them
  [REF src/vasp/postprocessing/postprocessing_h5py/postprocessing_h5py_common.py:198-251] and its XDMF template points
  [REF :639-670].  Frames are appended in place (``h5lite.H5Series.append_group``): one frame in memory at a time.
* ``TAWSS``, ``OSI``, ``RRT``, ``ECAP``, ``TWSSG``: one scalar DG1 function each, ``/<name>/<name>_0``, at time 0.

Dofs follow ``output.checkpoint``: DG1 node 3 f + k is vertex k of facet f, global dof = ncomp * node + component
(interleaved ``vector``), ``cell_dofs`` component-major per cell.  The vertices of facet f are the local vertices of its
cell without the opposite one, ascending - the order of ``HipBackend.wall_shear_stress``.  Geometry is the undeformed mesh.
"""
from __future__ import annotations

import os
import re
from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np

from .h5lite import Dataset, Group, H5Series, write_h5
from .hi_pass import check_fingerprint, frame_spacing, load_array, restart_entry, restart_refusal, save_array, sessions_folder, sha256_of
from .mesh import FsiMesh

INDEX_NAMES = ("TAWSS", "OSI", "RRT", "ECAP", "TWSSG")
FACET_VERTS = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])       # local vertices of the facet opposite vertex i


def fluid_boundary_facets(mesh: FsiMesh, fluid_ids) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Exterior facets of the fluid sub-mesh (cells whose marker is in ``fluid_ids``): wall, inlet and outlet caps - what
    DOLFIN's ``BoundaryMesh(fluid_mesh, "exterior")`` holds.  Returns (facet id, cell, local index of the opposite vertex),
    in facet-id order."""
    fc = mesh.facet_cells
    is_f = np.isin(mesh.cell_markers, np.atleast_1d(np.asarray(fluid_ids)))
    c0, c1 = fc[:, 0], fc[:, 1]
    f0 = is_f[c0]
    f1 = np.where(c1 >= 0, is_f[np.maximum(c1, 0)], False)
    sel = np.nonzero(f0 ^ f1)[0]                       # exactly one fluid cell: boundary of the fluid sub-mesh
    cell = np.where(f0[sel], c0[sel], c1[sel])
    tv = mesh.tets[cell]                                # (n, 4)
    on_facet = (tv[:, :, None] == mesh.facets[sel][:, None, :]).any(axis=2)
    local = np.argmin(on_facet, axis=1)                 # the one vertex of the cell not on the facet
    return sel, cell, local


def boundary_triangles(mesh: FsiMesh, cells, local) -> Tuple[np.ndarray, np.ndarray]:
    """Triangle mesh of the listed facets: (geometry (nv, 3): the original coordinates of the vertices it uses, compacted;
    topology (nf, 3): per facet its vertices in DG1 dof order)."""
    tri = mesh.tets[np.asarray(cells)[:, None], FACET_VERTS[np.asarray(local)]]
    used, topo = np.unique(tri, return_inverse=True)
    return np.ascontiguousarray(mesh.coords[used], dtype=np.float64), topo.reshape(-1, 3).astype(np.int64)


CELLS = {"triangle": ("Triangle", 3), "tetrahedron": ("Tetrahedron", 4)}      # XDMF topology type, vertices per cell
ATTRIBUTE_TYPES = {1: "Scalar", 3: "Vector", 9: "Tensor"}                       # by the number of components


def _dg1_group(values: np.ndarray, geometry: np.ndarray, topology: np.ndarray, dofmap: bool,
               celltype: str = "triangle") -> Group:
    """``<name>_k`` of ``write_checkpoint``: ``vector`` of a DG1 function (values (ncell, vertices per cell[, component
    shape]), interleaved per node, components row-major), with the dof map and the mesh when ``dofmap``."""
    nf, nvc = len(topology), CELLS[celltype][1]
    ncomp = int(np.prod(values.shape[2:], dtype=np.int64))
    g = Group()
    g["vector"] = Dataset(np.ascontiguousarray(values, dtype=np.float64).reshape(-1, 1))
    if dofmap:
        nodes = np.arange(nvc * nf, dtype=np.int64).reshape(nf, nvc)
        cell_dofs = (ncomp * nodes[:, :, None] + np.arange(ncomp)[None, None, :]).transpose(0, 2, 1).reshape(-1)
        g["cell_dofs"] = Dataset(cell_dofs.astype(np.int64))
        g["x_cell_dofs"] = Dataset((np.arange(nf + 1) * nvc * ncomp).astype(np.int64))
        g["cells"] = Dataset(np.arange(nf, dtype=np.int64))
        mg = Group()
        mg["geometry"] = Dataset(np.ascontiguousarray(geometry, dtype=np.float64))
        mg["topology"] = Dataset(np.ascontiguousarray(topology, dtype=np.int64), {"celltype": celltype})
        g["mesh"] = mg
    return g


def _xdmf_grid(name: str, k: int, t: float, nf: int, nv: int, ncomp: int, celltype: str = "triangle", h5: str = "",
               first: int = 0) -> str:
    """The grid of frame k; ``h5``: the file that holds it (default ``<name>.h5``), ``first``: the frame of that file that
    carries the dof map and the mesh."""
    h5, first = h5 or f"{name}.h5", f"{name}/{name}_{first}"
    topo_type, nvc = CELLS[celltype]
    ndofs = nvc * nf * ncomp
    att = ATTRIBUTE_TYPES[ncomp]
    return f'''      <Grid Name="{name}_{k}" GridType="Uniform">
        <Topology NumberOfElements="{nf}" TopologyType="{topo_type}" NodesPerElement="{nvc}">
          <DataItem Dimensions="{nf} {nvc}" NumberType="UInt" Format="HDF">{h5}:{first}/mesh/topology</DataItem>
        </Topology>
        <Geometry GeometryType="XYZ">
          <DataItem Dimensions="{nv} 3" Format="HDF">{h5}:{first}/mesh/geometry</DataItem>
        </Geometry>
         <Time Value="{float(t)!r}" />
        <Attribute ItemType="FiniteElementFunction" ElementFamily="DG" ElementDegree="1" ElementCell="{celltype}" Name="{name}" Center="Other" AttributeType="{att}">
          <DataItem Dimensions="{ndofs} 1" NumberType="UInt" Format="HDF">{h5}:{first}/cell_dofs</DataItem>
          <DataItem Dimensions="{ndofs} 1" NumberType="Float" Format="HDF">{h5}:{name}/{name}_{k}/vector</DataItem>
          <DataItem Dimensions="{nf + 1} 1" NumberType="UInt" Format="HDF">{h5}:{first}/x_cell_dofs</DataItem>
          <DataItem Dimensions="{nf} 1" NumberType="UInt" Format="HDF">{h5}:{first}/cells</DataItem>
        </Attribute>
      </Grid>
'''


def _xdmf_head(name: str) -> str:
    return f'''<?xml version="1.0"?>
<Xdmf Version="3.0">
  <Domain>
    <Grid GridType="Collection" CollectionType="Temporal" Name="{name}">
'''


XDMF_FOOTER = "    </Grid>\n  </Domain>\n</Xdmf>\n"


class Dg1Series:
    """One DG1 time series: ``<name>.h5`` and its XDMF, both grown in place one frame at a time.

    ``adopt`` > 0 continues the series after ``--restart-folder`` the way ``output.VisualizationWriter`` continues its own:
    the first ``adopt`` grids of the XDMF stay (later ones, written after the checkpoint by a run that was killed, are cut),
    new frames go to ``<name>_run_<N>.h5`` with continued frame numbers, and the first group of the new file carries the dof
    map and the mesh, as frame 0 does in the first."""

    def __init__(self, folder: Path, name: str, ncomp: int, celltype: str, geometry: np.ndarray, topology: np.ndarray, adopt: int = 0):
        self.folder, self.name, self.ncomp, self.celltype = Path(folder), name, ncomp, celltype
        self.geometry, self.topology = geometry, topology
        self.frames = self._first = 0           # frames of the series, and the first of them in this run's file
        self.file = f"{name}.h5"
        self._h5 = None
        if adopt:
            self._adopt(int(adopt))

    def _adopt(self, frames: int) -> None:
        path = self.folder / f"{self.name}.xdmf"
        text = path.read_text() if path.exists() else ""
        starts = [m.start() for m in re.finditer(r'^      <Grid Name="%s_\d+"' % re.escape(self.name), text, flags=re.M)]
        if len(starts) < frames or not text.endswith(XDMF_FOOTER):
            raise SystemExit(f"{path} lists {len(starts)} frames, the saved session state continues a series of {frames}")
        ends = starts[1:] + [len(text) - len(XDMF_FOOTER)]
        path.write_text(text[:ends[frames - 1]] + XDMF_FOOTER)
        runs = [int(p.stem.rsplit("_", 1)[1]) for p in self.folder.glob(f"{self.name}_run_*.h5") if p.stem.rsplit("_", 1)[1].isdigit()]
        self.file = f"{self.name}_run_{1 + max(runs, default=0)}.h5"
        self.frames = self._first = frames

    def append(self, values: np.ndarray, t: float) -> None:
        k = self.frames
        if self._h5 is None:
            self._h5 = H5Series(self.folder / self.file, Group(), self.name)
        self._h5.append_group(f"{self.name}_{k}", _dg1_group(values, self.geometry, self.topology, dofmap=k == self._first,
                                                            celltype=self.celltype))
        path = self.folder / f"{self.name}.xdmf"
        grid = _xdmf_grid(self.name, k, t, len(self.topology), len(self.geometry), self.ncomp, self.celltype, self.file, self._first)
        if k == 0:
            path.write_text(_xdmf_head(self.name) + grid + XDMF_FOOTER)
        else:                                   # the new grid overwrites the closing tags, which follow it again
            with open(path, "r+b") as f:
                f.seek(-len(XDMF_FOOTER.encode()), os.SEEK_END)
                f.write((grid + XDMF_FOOTER).encode())
        self.frames += 1

    def close(self) -> None:
        if self._h5 is not None:
            self._h5.close()
            self._h5 = None


def xdmf_frames(path) -> List[Tuple[float, str, int]]:
    """(time, h5 file, frame number) of every grid of a DG1 series' XDMF, in its order."""
    text = Path(path).read_text()
    times = [float(x) for x in re.findall(r'<Time Value="(.+?)"', text)]
    vectors = re.findall(r'"HDF">([^:<]+):[^<]*?_(\d+)/vector</DataItem>', text)
    return [(t, f, int(k)) for t, (f, k) in zip(times, vectors)]


class HemodynamicsWriter:
    """``<results>/Hemodynamic_indices/``: ``write_wss`` appends one WSS frame (h5 and XDMF grow in place),
    ``write_indices`` writes the five index files once.  ``adopt``: the frames of the WSS series a restarted run continues."""

    def __init__(self, folder, geometry: np.ndarray, topology: np.ndarray, adopt: int = 0):
        self.folder = Path(folder)
        self.folder.mkdir(parents=True, exist_ok=True)
        self.geometry, self.topology = geometry, topology
        self._wss = Dg1Series(self.folder, "WSS", 3, "triangle", geometry, topology, adopt)

    @property
    def frames(self) -> int:
        return self._wss.frames

    def write_wss(self, tau: np.ndarray, t: float) -> None:
        """tau (nf, 3, 3): the frame's WSS at the facet vertices."""
        nf = len(self.topology)
        if tau.shape != (nf, 3, 3):
            raise ValueError(f"WSS frame of shape {tau.shape}, expected {(nf, 3, 3)}")
        self._wss.append(tau, t)

    def write_indices(self, indices: Dict[str, np.ndarray]) -> None:
        """indices: TAWSS, OSI, RRT, ECAP, TWSSG as (nf, 3) arrays; each to ``<name>.{h5,xdmf}`` at time 0."""
        nf, nv = len(self.topology), len(self.geometry)
        for name in INDEX_NAMES:
            vals = np.asarray(indices[name], dtype=np.float64)
            if vals.shape != (nf, 3):
                raise ValueError(f"{name} of shape {vals.shape}, expected {(nf, 3)}")
            outer, root = Group(), Group()
            outer[f"{name}_0"] = _dg1_group(vals, self.geometry, self.topology, dofmap=True)
            root[name] = outer
            write_h5(self.folder / f"{name}.h5", root)
            (self.folder / f"{name}.xdmf").write_text(_xdmf_head(name) + _xdmf_grid(name, 0, 0.0, nf, nv, 1) + XDMF_FOOTER)

    def close(self) -> None:
        self._wss.close()


def osi_range_message(osi: np.ndarray, tol: float = 1e-12) -> str:
    """The reference's closing check [REF compute_hemodynamics.py:366-372] as a log line."""
    nan = int(np.isnan(osi).sum())                     # 0 / 0 where a dof never saw any shear
    lo, hi = (float(np.nanmin(osi)), float(np.nanmax(osi))) if nan < osi.size else (np.nan, np.nan)
    ok = nan == 0 and -tol <= lo < 0.5 and -tol < hi <= 0.5 + tol
    return (f"OSI range [{lo:.6g}, {hi:.6g}]" + (f" ({nan} dofs NaN)" if nan else "") + ": "
            + ("within 0 to 0.5" if ok else "NOT within 0 to 0.5"))


def hemodynamics_refusal(v: dict, world: int, backend_cls) -> str:
    """Why ``--hemodynamics`` cannot run with the resolved parameters ``v`` ('' if it can)."""
    if not v.get("save_step"):
        return "--hemodynamics samples the saved frames: it needs --save-step"
    if v.get("restart_folder"):
        why = restart_refusal(v, HemodynamicsRun.key, HemodynamicsRun.words)
        if why:
            return why
    if world > 1:
        return "--hemodynamics runs on one rank only (WORLD_SIZE > 1)"
    if backend_cls is not None and not hasattr(backend_cls, "hemodynamics_begin"):
        return f"--hemodynamics needs a backend with hemodynamics_begin ({getattr(backend_cls, '__name__', backend_cls)} has none)"
    return ""


class HemodynamicsRun:
    """The driver's side of ``--hemodynamics``: the session on the exterior facets of the fluid (``dx_f_id``), one WSS
    frame per saved Visualization frame, the indices at the end.  ``dt_sample`` = dt * save_step; mu = ``mu_f`` (its first
    entry when it is a list, as the reference's ``vasp-compute-hemo`` takes one viscosity)."""

    key, option = "hemodynamics", "--hemodynamics"
    words = "--hemodynamics cannot continue under --restart-folder"
    reads = ("v",)                                  # the fields of dvp_["n"] the session reads

    def __init__(self, backend, mesh: FsiMesh, ns: dict):
        mu = ns["mu_f"][0] if isinstance(ns["mu_f"], (list, tuple)) else ns["mu_f"]
        dt_sample = frame_spacing(ns)
        _, cells, local = fluid_boundary_facets(mesh, ns["dx_f_id"])
        geometry, topology = boundary_triangles(mesh, cells, local)
        self.backend = backend
        self.fingerprint = dict(dt_sample=dt_sample, mu=float(mu), rows=len(cells), facets=sha256_of(cells, local))
        self.times: List[float] = []
        entry = restart_entry(ns, self.key, self.words)
        if entry is not None:
            check_fingerprint(self.option, "the wall shear stress", entry["fingerprint"], self.fingerprint)
        backend.hemodynamics_begin(cells, local, float(mu), dt_sample)
        if entry is not None:                   # the sums, tau_prev and the count of the run that wrote the checkpoint
            acc = load_array(sessions_folder(ns["restart_folder"]) / "hemodynamics.npy", entry["sha256"], self.option)
            backend.hemodynamics_import(acc, int(entry["samples"]))
            self.times = [float(x) for x in entry["times"]]
        self.writer = HemodynamicsWriter(Path(ns["results_folder"]) / "Hemodynamic_indices", geometry, topology,
                                         adopt=int(entry["series_frames"]) if entry is not None else 0)

    def sample(self, t: float, state=None) -> None:
        self.writer.write_wss(self.backend.hemodynamics_sample(wss=True), t)
        self.times.append(float(t))

    def save(self, folder, t: float, counter: int) -> dict:
        """The accumulator to ``hemodynamics.npy``; returns the manifest's entry - None for a backend that cannot hand its
        accumulator out: without an entry a restart with the option is refused."""
        if not hasattr(self.backend, "hemodynamics_export"):
            return None
        acc, samples = self.backend.hemodynamics_export()
        return dict(samples=samples, times=list(self.times), fingerprint=self.fingerprint, series_frames=self.writer.frames,
                    sha256=save_array(Path(folder) / "hemodynamics.npy", acc))

    def finish(self, out=print) -> None:
        """The five index files (over the frames sampled so far) and the reference's OSI range check as a log line."""
        try:
            if self.writer.frames == 0:
                out("Hemodynamic indices: no frame was sampled, nothing written")
                return
            ind = self.backend.hemodynamics_indices()
            self.writer.write_indices(ind)
            out(f"Hemodynamic indices of {ind['samples']} frames written to {self.writer.folder}")
            out(osi_range_message(ind["OSI"]))
        finally:
            self.writer.close()
