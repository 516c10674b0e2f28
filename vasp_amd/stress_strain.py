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

from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np

from .h5lite import Group, write_h5
from .hemodynamics import XDMF_FOOTER, Dg1Series, _dg1_group, _xdmf_grid, _xdmf_head
from .hi_pass import check_fingerprint, frame_spacing, load_array, restart_entry, restart_refusal, save_array, sessions_folder, sha256_of
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
    ``write_averages`` writes the two average files once.  ``adopt``: the frames of the four series a restarted run
    continues (``hemodynamics.Dg1Series``)."""

    def __init__(self, folder, geometry: np.ndarray, topology: np.ndarray, adopt: int = 0):
        self.folder = Path(folder)
        self.folder.mkdir(parents=True, exist_ok=True)
        self.geometry, self.topology = geometry, topology
        self.frames = int(adopt)
        self._series = {name: Dg1Series(self.folder, name, COMPONENTS[name], "tetrahedron", geometry, topology, adopt)
                        for name in FRAME_NAMES}

    def _shape(self, name: str) -> tuple:
        return (len(self.topology), 4, 3, 3) if COMPONENTS[name] == 9 else (len(self.topology), 4)

    def write_frame(self, frame: Dict[str, np.ndarray], t: float) -> None:
        """frame: the four fields keyed as ``HipBackend.stress_strain`` ((n, 4, 3, 3) tensors, (n, 4) principal values)."""
        for name in FRAME_NAMES:
            if np.shape(frame[name]) != self._shape(name):
                raise ValueError(f"{name} of shape {np.shape(frame[name])}, expected {self._shape(name)}")
        for name in FRAME_NAMES:
            self._series[name].append(np.asarray(frame[name]), t)
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


def stress_strain_refusal(v: dict, world: int, backend_cls) -> str:
    """Why ``--stress-strain`` cannot run with the resolved parameters ``v`` ('' if it can)."""
    if not v.get("save_step"):
        return "--stress-strain samples the saved frames: it needs --save-step"
    if v.get("restart_folder"):
        why = restart_refusal(v, StressStrainRun.key, StressStrainRun.words)
        if why:
            return why
    if world > 1:
        return "--stress-strain runs on one rank only (WORLD_SIZE > 1)"
    if backend_cls is not None and not hasattr(backend_cls, "stress_strain_begin"):
        return f"--stress-strain needs a backend with stress_strain_begin ({getattr(backend_cls, '__name__', backend_cls)} has none)"
    return ""


class StressStrainRun:
    """The driver's side of ``--stress-strain``: the session on the solid cells (``dx_s_id``, every region), one frame per
    saved Visualization frame, the averages at the end."""

    key, option = "stress_strain", "--stress-strain"
    words = "--stress-strain cannot continue under --restart-folder"
    reads = ("d",)                                  # the fields of dvp_["n"] the session reads

    def __init__(self, backend, mesh: FsiMesh, ns: dict):
        cells = solid_cells(mesh, ns["dx_s_id"])
        if len(cells) == 0:
            raise SystemExit(f"--stress-strain: no cell carries a solid marker (dx_s_id = {ns['dx_s_id']})")
        geometry, topology = solid_submesh(mesh, cells)
        self.backend = backend
        self.fingerprint = dict(dt_sample=frame_spacing(ns), rows=len(cells), cells=sha256_of(cells))
        self.times: List[float] = []
        entry = restart_entry(ns, self.key, self.words)
        if entry is not None:
            check_fingerprint(self.option, "the solid cells", entry["fingerprint"], self.fingerprint)
        backend.stress_strain_begin(cells)
        if entry is not None:                   # the sums and the count of the run that wrote the checkpoint
            sums = load_array(sessions_folder(ns["restart_folder"]) / "stress_strain.npy", entry["sha256"], self.option)
            backend.stress_strain_import(sums, int(entry["samples"]))
            self.times = [float(x) for x in entry["times"]]
        self.writer = StressStrainWriter(Path(ns["results_folder"]) / "StressStrain", geometry, topology,
                                         adopt=int(entry["series_frames"]) if entry is not None else 0)

    def sample(self, t: float, state=None) -> None:
        self.writer.write_frame(self.backend.stress_strain_sample(frame=True), t)
        self.times.append(float(t))

    def save(self, folder, t: float, counter: int) -> dict:
        """The sums to ``stress_strain.npy``; returns the manifest's entry - None for a backend that cannot hand its sums
        out: without an entry a restart with the option is refused."""
        if not hasattr(self.backend, "stress_strain_export"):
            return None
        sums, samples = self.backend.stress_strain_export()
        return dict(samples=samples, times=list(self.times), fingerprint=self.fingerprint, series_frames=self.writer.frames,
                    sha256=save_array(Path(folder) / "stress_strain.npy", sums))

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
