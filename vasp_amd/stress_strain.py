"""Solid stress and strain of a run: the solid sub-mesh and the files of `<results>/StressStrain/`, libhdf5-free.

Counterpart of ``vasp-compute-stress`` [REF src/vasp/postprocessing/postprocessing_fenics/compute_stress_strain.py:160-290],
whose arithmetic runs on the device during the run (``HipBackend.stress_strain_*``, csrc/fsi_stress.hip).  What is written:

* ``TrueStress``, ``GreenLagrangeStrain`` (tensor DG1), ``MaxPrincipalStress``, ``MaxPrincipalStrain`` (scalar DG1): one
  time series each, ``/<name>/<name>_k/vector`` (k = 0, 1, ...), in DOLFIN's ``XDMFFile.write_checkpoint`` layout on
  tetrahedra; ``cell_dofs``, ``x_cell_dofs``, ``cells`` and ``mesh/{geometry,topology}`` sit under ``<name>_0``, where the
  reference's consumer reads them [REF src/vasp/postprocessing/postprocessing_h5py/postprocessing_h5py_common.py:198-260].
  Frames are appended in place (``h5lite.H5Series.append_group``): one frame in memory at a time.
* ``MaxPrincipalStress_avg``, ``MaxPrincipalStrain_avg``: the mean of the sampled principal values, ``/<name>/<name>_0``, at
  time 0.

Dofs follow ``hemodynamics``: DG1 node 4 c + a is local vertex a of solid cell c, global dof = ncomp * node + component
(interleaved ``vector``; a tensor's 9 components row-major, as the consumer reshapes it to (-1, 9)), ``cell_dofs``
component-major per cell.  The solid cells are those whose marker is in ``dx_s_id``, ascending; geometry is the undeformed
coordinates of the vertices they use, compacted in ascending vertex order.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Dict, Tuple

import numpy as np

from .h5lite import Group, H5Series, write_h5
from .hemodynamics import XDMF_FOOTER, _dg1_group, _xdmf_grid, _xdmf_head
from .mesh import FsiMesh

FRAME_NAMES = ("TrueStress", "GreenLagrangeStrain", "MaxPrincipalStress", "MaxPrincipalStrain")
AVERAGE_NAMES = ("MaxPrincipalStress_avg", "MaxPrincipalStrain_avg")
COMPONENTS = {"TrueStress": 9, "GreenLagrangeStrain": 9, "MaxPrincipalStress": 1, "MaxPrincipalStrain": 1}


def solid_cells(mesh: FsiMesh, solid_ids) -> np.ndarray:
    """The cells whose marker is in ``solid_ids`` (an int or a list, as ``dx_s_id``), ascending."""
    return np.nonzero(np.isin(mesh.cell_markers, np.atleast_1d(np.asarray(solid_ids))))[0]


def solid_submesh(mesh: FsiMesh, cells) -> Tuple[np.ndarray, np.ndarray]:
    """Tetrahedral mesh of the listed cells: (geometry (nv, 3): the original coordinates of the vertices it uses, compacted
    in ascending vertex order; topology (n, 4): per cell its vertices in local order, so DG1 coefficient a is vertex a)."""
    used, topo = np.unique(mesh.tets[np.asarray(cells)], return_inverse=True)
    return np.ascontiguousarray(mesh.coords[used], dtype=np.float64), topo.reshape(-1, 4).astype(np.int64)


class StressStrainWriter:
    """``<results>/StressStrain/``: ``write_frame`` appends one frame to the four series (h5 and XDMF grow in place),
    ``write_averages`` writes the two average files once."""

    def __init__(self, folder, geometry: np.ndarray, topology: np.ndarray):
        self.folder = Path(folder)
        self.folder.mkdir(parents=True, exist_ok=True)
        self.geometry, self.topology = geometry, topology
        self.frames = 0
        self._series: Dict[str, H5Series] = {}

    def _shape(self, name: str) -> tuple:
        return (len(self.topology), 4, 3, 3) if COMPONENTS[name] == 9 else (len(self.topology), 4)

    def write_frame(self, frame: Dict[str, np.ndarray], t: float) -> None:
        """frame: the four fields keyed as ``HipBackend.stress_strain`` ((n, 4, 3, 3) tensors, (n, 4) principal values)."""
        n, nv = len(self.topology), len(self.geometry)
        for name in FRAME_NAMES:
            if np.shape(frame[name]) != self._shape(name):
                raise ValueError(f"{name} of shape {np.shape(frame[name])}, expected {self._shape(name)}")
        k = self.frames
        for name in FRAME_NAMES:
            if name not in self._series:
                self._series[name] = H5Series(self.folder / f"{name}.h5", Group(), name)
            self._series[name].append_group(f"{name}_{k}", _dg1_group(np.asarray(frame[name]), self.geometry, self.topology,
                                                                      dofmap=k == 0, celltype="tetrahedron"))
            path = self.folder / f"{name}.xdmf"
            grid = _xdmf_grid(name, k, t, n, nv, COMPONENTS[name], celltype="tetrahedron")
            if k == 0:
                path.write_text(_xdmf_head(name) + grid + XDMF_FOOTER)
            else:                               # the new grid overwrites the closing tags, which follow it again
                with open(path, "r+b") as f:
                    f.seek(-len(XDMF_FOOTER.encode()), os.SEEK_END)
                    f.write((grid + XDMF_FOOTER).encode())
        self.frames += 1

    def write_averages(self, averages: Dict[str, np.ndarray]) -> None:
        """averages: MaxPrincipalStress_avg, MaxPrincipalStrain_avg as (n, 4) arrays; each to ``<name>.{h5,xdmf}`` at time 0."""
        n, nv = len(self.topology), len(self.geometry)
        for name in AVERAGE_NAMES:
            vals = np.asarray(averages[name], dtype=np.float64)
            if vals.shape != (n, 4):
                raise ValueError(f"{name} of shape {vals.shape}, expected {(n, 4)}")
            outer, root = Group(), Group()
            outer[f"{name}_0"] = _dg1_group(vals, self.geometry, self.topology, dofmap=True, celltype="tetrahedron")
            root[name] = outer
            write_h5(self.folder / f"{name}.h5", root)
            (self.folder / f"{name}.xdmf").write_text(_xdmf_head(name) + _xdmf_grid(name, 0, 0.0, n, nv, 1, celltype="tetrahedron")
                                                      + XDMF_FOOTER)

    def close(self) -> None:
        for s in self._series.values():
            s.close()
        self._series = {}


def stress_strain_refusal(v: dict, world: int, backend_cls) -> str:
    """Why ``--stress-strain`` cannot run with the resolved parameters ``v`` ('' if it can)."""
    if not v.get("save_step"):
        return "--stress-strain samples the saved frames: it needs --save-step"
    if v.get("restart_folder"):
        return "--stress-strain does not carry its sums through a checkpoint: it cannot be used with --restart-folder"
    if world > 1:
        return "--stress-strain runs on one rank only (WORLD_SIZE > 1)"
    if backend_cls is not None and not hasattr(backend_cls, "stress_strain_begin"):
        return f"--stress-strain needs a backend with stress_strain_begin ({getattr(backend_cls, '__name__', backend_cls)} has none)"
    return ""


class StressStrainRun:
    """The driver's side of ``--stress-strain``: the session on the solid cells (``dx_s_id``, every region), one frame per
    saved Visualization frame, the averages at the end."""

    def __init__(self, backend, mesh: FsiMesh, ns: dict):
        cells = solid_cells(mesh, ns["dx_s_id"])
        if len(cells) == 0:
            raise SystemExit(f"--stress-strain: no cell carries a solid marker (dx_s_id = {ns['dx_s_id']})")
        geometry, topology = solid_submesh(mesh, cells)
        self.backend = backend
        backend.stress_strain_begin(cells)
        self.writer = StressStrainWriter(Path(ns["results_folder"]) / "StressStrain", geometry, topology)

    def sample(self, t: float, state=None) -> None:
        self.writer.write_frame(self.backend.stress_strain_sample(frame=True), t)

    def finish(self, out=print) -> None:
        """The two average files (over the frames sampled so far) and one log line."""
        try:
            if self.writer.frames == 0:
                out("Stress and strain: no frame was sampled, nothing written")
                return
            avg = self.backend.stress_strain_averages()
            self.writer.write_averages(avg)
            out(f"Stress and strain of {avg['samples']} frames written to {self.writer.folder}")
        finally:
            self.writer.close()
