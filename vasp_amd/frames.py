"""The saved frames of a finished results folder: `<results>/Visualization/{displacement,velocity,pressure}.{xdmf,h5}` read
back one frame at a time, libhdf5-free.

Counterpart of ``output_file_lists`` and the frame loops behind it
[REF src/vasp/postprocessing/postprocessing_common.py:63-121;
src/vasp/postprocessing/postprocessing_fenics/create_hdf5.py:89-98,139-160]: the XDMF of a field names, per time step, the
HDF5 file and the dataset that hold it - ``<name>.h5`` and, behind a restart, ``<name>_run_<N>.h5``.  The files are mapped,
not read (``h5lite.open_h5``): a frame is a view of its block in the mapping, so a series of any length costs the memory of
the pages in use.  What ``output.VisualizationWriter`` wrote is FP64 copies of the state: at ``save_deg 2`` d and v on every P2
node and p on the vertices (with the edge means behind them), which is the whole state; at ``save_deg 1`` the vertex values,
from which ``state_from_frame`` makes the P1 field the reference's tools see in such a folder.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from .h5lite import H5Error, open_h5
from .mesh import FsiMesh
from .output import FIELDS, xdmf_entries

FIELD_OF = {"d": "displacement", "v": "velocity", "p": "pressure"}      # as hi_pass.VIZ_TYPE


def selected_indices(times: Sequence[float], dt: float, stride: int = 1, t0: float = 0.0, t1: Optional[float] = None) -> List[int]:
    """The frames k of a series with ``k % stride == 0`` and ``t0 <= t_k <= t1`` (t1 None: no upper limit; the comparisons
    allow dt / 10): the rule of ``hi_pass.select_frames``, as a list."""
    return [k for k in range(0, len(times), int(stride)) if times[k] >= t0 - dt / 10 and (t1 is None or times[k] <= t1 + dt / 10)]


def state_from_frame(mesh: FsiMesh, save_deg: int, d=None, v=None, p=None) -> np.ndarray:
    """The user-layout vector ``[d | v | p]`` of one saved frame - the host twin of ``HipBackend.set_frame``.  ``save_deg 2``:
    d and v as they are, ``p[:V]``.  ``save_deg 1``: the vertex values, and ``0.5 * (a + b)`` of an edge's two vertices on its
    mid-edge node.  A field that is None stays zero."""
    V, N2 = mesh.num_vertices, mesh.num_nodes
    n = N2 if int(save_deg) >= 2 else V
    x = np.zeros(mesh.num_dofs)
    xd, xv, xp = mesh.split(x)
    e = mesh.edges
    for dst, src in ((xd, d), (xv, v)):
        if src is None:
            continue
        src = np.asarray(src, dtype=np.float64).reshape(n, 3)
        dst[:n] = src
        if n < N2:
            dst[V:] = 0.5 * (src[e[:, 0]] + src[e[:, 1]])
    if p is not None:
        xp[:] = np.asarray(p, dtype=np.float64).reshape(n)[:V]
    return x


class FrameSource:
    """The frames of ``<results>/Visualization``: ``times``, ``entries[field]`` = (time, file, index) per frame as the three
    XDMF files list them, and ``frames(indices, fields)``, which yields ``(t, {field: view})`` of the listed frames and maps
    only the files of the listed fields; ``state(mesh, views)`` is the host twin's vector of such a frame at the series'
    ``save_deg`` (given, or set by whoever has compared the frames' node count with a mesh).  Whatever is missing or
    inconsistent is refused at construction or by ``check_files`` with a SystemExit that names what was looked for."""

    def __init__(self, results, save_deg: Optional[int] = None):
        self.results = Path(str(results))
        self.folder = self.results / "Visualization"
        self.save_deg = None if save_deg is None else int(save_deg)
        if not self.results.is_dir():
            raise SystemExit(f"results folder {self.results} not found")
        self.entries: Dict[str, List[Tuple[float, str, int]]] = {}
        for name, _, _ in FIELDS:
            path = self.folder / f"{name}.xdmf"
            if not path.exists():
                raise SystemExit(f"{path} not found: the folder holds no saved {name} frames (was the run started with --save-step?)")
            self.entries[name] = xdmf_entries(path)
        first = FIELDS[0][0]
        self.times = [e[0] for e in self.entries[first]]
        for name, _, _ in FIELDS[1:]:
            other = [e[0] for e in self.entries[name]]
            if other != self.times:
                k = next((i for i, (a, b) in enumerate(zip(self.times, other)) if a != b), min(len(self.times), len(other)))
                raise SystemExit(f"{self.folder / (name + '.xdmf')} lists {len(other)} frames, {first}.xdmf lists {len(self.times)}: the "
                                 f"frame times of the two differ from frame {k} on")
        self._open: Dict[str, Tuple[str, object]] = {}       # per field: the mapped file of the frame read last

    def __len__(self) -> int:
        return len(self.times)

    def check_files(self, fields: Sequence[str]) -> None:
        """Every HDF5 file the XDMF entries of the listed fields (d, v, p) name exists."""
        for q in fields:
            for h5 in sorted({e[1] for e in self.entries[FIELD_OF[q]]}):
                if not (self.folder / h5).exists():
                    raise SystemExit(f"{self.folder / h5} not found: {FIELD_OF[q]}.xdmf names it")

    def _dataset(self, q: str, k: int):
        name = FIELD_OF[q]
        _, h5, idx = self.entries[name][k]
        held = self._open.get(q)
        if held is None or held[0] != h5:
            if held is not None:
                held[1].close()
            path = self.folder / h5
            if not path.exists():
                raise SystemExit(f"{path} not found: {name}.xdmf names it")
            self._open[q] = held = (h5, open_h5(path))
        series = held[1]["VisualisationVector"]
        if str(idx) not in series:
            raise H5Error(f"{self.folder / h5} holds no /VisualisationVector/{idx}, which {name}.xdmf names")
        return series[str(idx)]

    def node_count(self, fields: Sequence[str]) -> int:
        """Rows of a frame of the listed fields (those of the first frame; every field must agree)."""
        counts = {q: int(self._dataset(q, 0).shape[0]) for q in fields}
        if len(set(counts.values())) > 1:
            raise SystemExit(f"{self.folder}: the fields' frames have different node counts: {counts}")
        return next(iter(counts.values()))

    def frames(self, indices: Sequence[int], fields: Sequence[str]) -> Iterator[Tuple[float, Dict[str, np.ndarray]]]:
        """``(t, views)`` per listed frame: ``views[q]`` is the (n, 3) block of d or v or the (n,) block of p in the mapped
        file - zero-copy, read-only, valid until the source moves to another file of the field or is closed."""
        for k in indices:
            views = {}
            for q in fields:
                a = self._dataset(q, k).data
                views[q] = a.reshape(-1) if q == "p" else a
            yield self.times[k], views

    def state(self, mesh: FsiMesh, views: Dict[str, np.ndarray]) -> np.ndarray:
        """``state_from_frame`` of the views of one frame; fields that were not read stay zero."""
        if self.save_deg is None:
            raise ValueError("FrameSource.state: the series' save_deg is not known")
        return state_from_frame(mesh, self.save_deg, **views)

    def close(self) -> None:
        for _, f in self._open.values():
            f.close()
        self._open = {}
