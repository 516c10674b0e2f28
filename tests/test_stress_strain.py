"""Solid stress and strain (vasp_amd/stress_strain.py, ``--stress-strain``) on the host: the solid sub-mesh, the file layout
of ``StressStrain/`` under the independent HDF5 walker and the consumer's recipe, the driver's refusals, and a driver run
with a host stand-in for the device session."""
import json

import numpy as np
import pytest

from conftest import GOLDEN, make_avf_case
from test_hemodynamics import output_file_lists

FRAME_NAMES = ("TrueStress", "GreenLagrangeStrain", "MaxPrincipalStress", "MaxPrincipalStrain")
AVERAGE_NAMES = ("MaxPrincipalStress_avg", "MaxPrincipalStrain_avg")


def oracle_frame(mesh, desc, d_nodal, cells, eig="kopp"):
    """oracle.post_oracle.stress_strain_dg1 on ``cells`` (ascending solid cells), called once per solid region with that
    region's properties and material model, put back in the order of ``cells``."""
    from oracle.post_oracle import stress_strain_dg1
    cells = np.asarray(cells)
    region = np.asarray(desc["cell_region"])[cells]
    out = {k: np.zeros((len(cells), 4, 3, 3) if k in FRAME_NAMES[:2] else (len(cells), 4)) for k in FRAME_NAMES}
    for r, props in enumerate(desc["solid_props"]):
        sel = np.nonzero(region == r)[0]
        if len(sel) == 0:
            continue
        ref = stress_strain_dg1(mesh.coords, mesh.tets, mesh.tet_nodes, d_nodal, cells[sel], props,
                                model=desc["solid_models"][r], eig=eig)
        for k in FRAME_NAMES:
            out[k][sel] = ref[k]
    return out


# ---- the solid sub-mesh --------------------------------------------------------------------------------------------------

def _mesh_and_ids(which, tmp_path):
    from vasp_amd.mesh import FsiMesh
    if which == "avf":
        ns, desc = make_avf_case(tmp_path)[:2]
        return ns["mesh"], ns["dx_s_id"], desc
    return FsiMesh.read(GOLDEN / which / f"{which}.h5"), 2, None


@pytest.mark.parametrize("which", ["cylinder", "offset_stenosis", "avf"])
def test_solid_submesh(which, tmp_path):
    from vasp_amd.stress_strain import solid_cells, solid_submesh
    mesh, ids, desc = _mesh_and_ids(which, tmp_path)
    cells = solid_cells(mesh, ids)
    ids = np.atleast_1d(ids)
    assert len(cells) > 0 and (np.diff(cells) > 0).all()                             # ascending, no repeats
    np.testing.assert_array_equal(cells, [c for c in range(mesh.num_cells) if mesh.cell_markers[c] in ids])
    for i in ids:                                                                      # every region, all of its cells
        assert (mesh.cell_markers[cells] == i).sum() == (mesh.cell_markers == i).sum() > 0
    if desc is not None:                                                               # the driver's own solid cells
        assert len(ids) == 2
        np.testing.assert_array_equal(cells, np.nonzero(np.asarray(desc["cell_kind"]) == 1)[0])
        np.testing.assert_array_equal(np.bincount(np.asarray(desc["cell_region"])[cells]),
                                      [(mesh.cell_markers == i).sum() for i in ids])
    geom, topo = solid_submesh(mesh, cells)
    used = np.unique(mesh.tets[cells])
    assert topo.shape == (len(cells), 4) and topo.dtype == np.int64
    assert geom.shape == (len(used), 3) and geom.dtype == np.float64
    np.testing.assert_array_equal(geom, mesh.coords[used])                            # compacted, ascending vertex order
    np.testing.assert_array_equal(used[topo], mesh.tets[cells])                       # local vertex order kept
    np.testing.assert_array_equal(geom[topo], mesh.coords[mesh.tets[cells]])


def test_solid_cells_accepts_an_int_or_a_list():
    from vasp_amd.mesh import FsiMesh
    from vasp_amd.stress_strain import solid_cells
    mesh = FsiMesh.read(GOLDEN / "cylinder" / "cylinder.h5")
    np.testing.assert_array_equal(solid_cells(mesh, 2), solid_cells(mesh, [2]))
    np.testing.assert_array_equal(solid_cells(mesh, [1, 2]), np.arange(mesh.num_cells))


# ---- files ---------------------------------------------------------------------------------------------------------------

def _frames(n, count, seed=1):
    rng = np.random.default_rng(seed)
    return [dict(TrueStress=rng.standard_normal((n, 4, 3, 3)), GreenLagrangeStrain=rng.standard_normal((n, 4, 3, 3)),
                 MaxPrincipalStress=rng.standard_normal((n, 4)), MaxPrincipalStrain=rng.standard_normal((n, 4)))
            for _ in range(count)]


def _writer_case(tmp_path, frames=3):
    from vasp_amd.mesh import FsiMesh
    from vasp_amd.stress_strain import StressStrainWriter, solid_cells, solid_submesh
    mesh = FsiMesh.read(GOLDEN / "cylinder" / "cylinder.h5")
    geom, topo = solid_submesh(mesh, solid_cells(mesh, 2))
    n = len(topo)
    w = StressStrainWriter(tmp_path / "StressStrain", geom, topo)
    fr = _frames(n, frames)
    for k, f in enumerate(fr):
        w.write_frame(f, 0.001 * (k + 1))
    rng = np.random.default_rng(2)
    avg = {name: rng.standard_normal((n, 4)) for name in AVERAGE_NAMES}
    w.write_averages(avg)
    w.close()
    return w.folder, geom, topo, fr, avg


def test_writer_layout_under_the_independent_walker(tmp_path):
    from test_h5_structure_independent import Walker
    folder, geom, topo, frames, avg = _writer_case(tmp_path)
    n, nv = len(topo), len(geom)
    for name in FRAME_NAMES:
        ncomp = 9 if name in ("TrueStress", "GreenLagrangeStrain") else 1
        tree = Walker(folder / f"{name}.h5").tree()
        first = f"/{name}/{name}_0"
        for k, f in enumerate(frames):
            d = tree[f"/{name}/{name}_{k}/vector"]
            assert d["kind"] == "dataset"
            assert np.frombuffer(d["raw"], dtype="<f8").tobytes() == f[name].astype("<f8").tobytes()
        assert f"/{name}/{name}_1/cell_dofs" not in tree                  # the dof map lives under <name>_0, where it is read
        cell_dofs = np.frombuffer(tree[f"{first}/cell_dofs"]["raw"], dtype="<i8")
        assert len(cell_dofs) == 4 * ncomp * n and (np.sort(cell_dofs) == np.arange(4 * ncomp * n)).all()
        np.testing.assert_array_equal(np.frombuffer(tree[f"{first}/x_cell_dofs"]["raw"], dtype="<i8"), 4 * ncomp * np.arange(n + 1))
        # component-major per cell, interleaved global numbering: cell c, component i, vertex a -> ncomp (4 c + a) + i
        c, i, a = 7, ncomp - 1, 2
        assert cell_dofs[4 * ncomp * c + 4 * i + a] == ncomp * (4 * c + a) + i
        np.testing.assert_array_equal(np.frombuffer(tree[f"{first}/cells"]["raw"], dtype="<i8"), np.arange(n))
        assert np.frombuffer(tree[f"{first}/mesh/geometry"]["raw"], dtype="<f8").tobytes() == geom.tobytes()
        np.testing.assert_array_equal(np.frombuffer(tree[f"{first}/mesh/topology"]["raw"], dtype="<i8").reshape(-1, 4), topo)
        h5s, times, idx = output_file_lists(folder / f"{name}.xdmf")
        assert h5s == [f"{name}.h5"] * len(frames) and idx == list(range(len(frames)))
        assert times == [0.001 * (k + 1) for k in range(len(frames))]
        text = (folder / f"{name}.xdmf").read_text()
        assert 'CollectionType="Temporal"' in text and text.rstrip().endswith("</Xdmf>")
        assert text.count(f'<DataItem Dimensions="{4 * ncomp * n} 1" NumberType="Float" Format="HDF">{name}.h5:{name}/{name}_') == len(frames)
        assert f'<DataItem Dimensions="{nv} 3" Format="HDF">{name}.h5:{name}/{name}_0/mesh/geometry' in text
        assert f'TopologyType="Tetrahedron" NodesPerElement="4"' in text and f'Dimensions="{n} 4" NumberType="UInt"' in text
        assert 'ItemType="FiniteElementFunction" ElementFamily="DG" ElementDegree="1" ElementCell="tetrahedron"' in text
        assert f'AttributeType="{"Tensor" if ncomp == 9 else "Scalar"}"' in text
    for name in AVERAGE_NAMES:
        tr = Walker(folder / f"{name}.h5").tree()
        base = f"/{name}/{name}_0"
        np.testing.assert_array_equal(np.frombuffer(tr[f"{base}/vector"]["raw"], dtype="<f8"), avg[name].reshape(-1))
        np.testing.assert_array_equal(np.frombuffer(tr[f"{base}/cell_dofs"]["raw"], dtype="<i8"), np.arange(4 * n))
        np.testing.assert_array_equal(np.frombuffer(tr[f"{base}/x_cell_dofs"]["raw"], dtype="<i8"), 4 * np.arange(n + 1))
        h5s, times, idx = output_file_lists(folder / f"{name}.xdmf")
        assert h5s == [f"{name}.h5"] and times == [0.0] and idx == [0]
        xt = (folder / f"{name}.xdmf").read_text()
        assert 'AttributeType="Scalar"' in xt and 'ElementCell="tetrahedron"' in xt and f'Dimensions="{4 * n} 1" NumberType="Float"' in xt


def test_writer_files_read_back_through_h5lite(tmp_path):
    from vasp_amd.h5lite import read_h5
    folder, geom, topo, frames, avg = _writer_case(tmp_path, frames=2)
    for name in FRAME_NAMES:
        g = read_h5(folder / f"{name}.h5")
        for k, f in enumerate(frames):
            np.testing.assert_array_equal(np.asarray(g[name][f"{name}_{k}"]["vector"].data).reshape(f[name].shape), f[name])
        assert g[name][f"{name}_0"]["mesh"]["topology"].attrs["celltype"] in ("tetrahedron", b"tetrahedron")
    for name in AVERAGE_NAMES:
        np.testing.assert_array_equal(np.asarray(read_h5(folder / f"{name}.h5")[name][f"{name}_0"]["vector"].data).reshape(-1, 4),
                                      avg[name])


def test_consumer_recipe_gives_back_the_written_tensors(tmp_path):
    """What the reference's hi-pass tools do [REF src/vasp/postprocessing/postprocessing_h5py/postprocessing_h5py_common.py:
    198-260]: the h5 files and indices from output_file_lists, the dof info from <name>_0, and each frame's
    ``TrueStress/TrueStress_{k}/vector`` reshaped to (-1, 9); the node of cell c, vertex a is cell_dofs[x_cell_dofs[c] + a] / 9."""
    from vasp_amd.h5lite import read_h5
    folder, geom, topo, frames, _ = _writer_case(tmp_path, frames=4)
    for name, key in (("TrueStress", "TrueStress/TrueStress_{}/vector"), ("GreenLagrangeStrain",
                                                                         "GreenLagrangeStrain/GreenLagrangeStrain_{}/vector")):
        h5s, times, idx = output_file_lists(folder / f"{name}.xdmf")
        assert len(idx) >= 3 and times[2] - times[1] == pytest.approx(0.001)       # the consumer's time_between_files
        data = read_h5(folder / h5s[0])
        first = data[list(data.keys())[0]][f"{name}_0"]
        info = {k: np.asarray(first[k].data) if "/" not in k else np.asarray(first["mesh"][k.split("/")[1]].data)
                for k in ("cell_dofs", "cells", "mesh/geometry", "mesh/topology", "x_cell_dofs")}
        x, cd = info["x_cell_dofs"].reshape(-1), info["cell_dofs"].reshape(-1)
        nodes = np.stack([cd[x[:-1] + a] // 9 for a in range(4)], axis=1)           # (n, 4): component 0 of each vertex
        for h5, k in zip(h5s, idx):
            vec = np.asarray(read_h5(folder / h5)[name][f"{name}_{k}"]["vector"].data).reshape(-1, 9)
            assert key.format(k).startswith(f"{name}/{name}_{k}")
            np.testing.assert_array_equal(vec[nodes].reshape(-1, 4, 3, 3), frames[k][name])
        np.testing.assert_array_equal(info["mesh/geometry"][info["mesh/topology"]], geom[topo])


def test_writer_refuses_a_frame_of_the_wrong_shape(tmp_path):
    from vasp_amd.stress_strain import StressStrainWriter
    w = StressStrainWriter(tmp_path / "s", np.zeros((4, 3)), np.array([[0, 1, 2, 3]]))
    bad = _frames(1, 1)[0]
    bad["TrueStress"] = bad["TrueStress"][:, :3]
    with pytest.raises(ValueError, match="TrueStress"):
        w.write_frame(bad, 0.0)
    w.close()


def test_hemodynamics_files_are_unchanged_by_the_generalised_helpers():
    """The DG1 group and XDMF helpers now take the cell type; on triangles they give what they gave before."""
    from vasp_amd.hemodynamics import _dg1_group, _xdmf_grid
    topo = np.array([[0, 1, 2], [1, 2, 3]])
    g = _dg1_group(np.arange(18.0).reshape(2, 3, 3), np.zeros((4, 3)), topo, dofmap=True)
    np.testing.assert_array_equal(g["x_cell_dofs"].data, [0, 9, 18])
    assert g["mesh"]["topology"].attrs["celltype"] == "triangle"
    grid = _xdmf_grid("WSS", 1, 0.5, 2, 4, 3)
    assert 'TopologyType="Triangle" NodesPerElement="3"' in grid and 'Dimensions="2 3" NumberType="UInt"' in grid
    assert 'ElementCell="triangle"' in grid and 'AttributeType="Vector"' in grid and 'Dimensions="18 1"' in grid


# ---- the driver's refusals and the option ---------------------------------------------------------------------------------

class _NeverBuilt:
    """A backend factory that must not be reached."""
    def __init__(self, desc):
        raise AssertionError("the backend was created")


def _refused(tmp_path, extra, factory=_NeverBuilt):
    from vasp_amd import monolithic
    with pytest.raises(SystemExit) as e:
        monolithic.run(["-p", "cylinder", "-dt", "0.001", "-T", "0.002", "--folder", str(tmp_path), "--sub-folder", "1",
                        "--verbose", "False", "--new-arguments", f"mesh_path={GOLDEN / 'cylinder' / 'cylinder.h5'}", *extra],
                       backend_factory=factory)
    return str(e.value)


def test_refused_without_save_step(tmp_path):
    msg = _refused(tmp_path, ["--save-step", "0", "--stress-strain"])
    assert "--stress-strain" in msg and "--save-step" in msg


def test_refused_with_restart_folder(tmp_path):
    assert "--restart-folder" in _refused(tmp_path, ["--restart-folder", str(tmp_path / "old"), "--stress-strain"])


def test_refused_on_more_than_one_rank(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert "WORLD_SIZE" in _refused(tmp_path, ["--stress-strain"])


def test_refused_for_a_backend_without_the_session(tmp_path):
    from oracle.backend import OracleBackend

    class Oracle(OracleBackend):
        def __init__(self, desc):
            raise AssertionError("the backend was created")

    assert "stress_strain_begin" in _refused(tmp_path, ["--stress-strain"], factory=Oracle)


def test_option_from_a_config_file_and_new_arguments(tmp_path):
    from vasp_amd.monolithic import parse
    cfg = tmp_path / "run.cfg"
    cfg.write_text("stress-strain = True\n")
    assert parse(["-c", str(cfg)])["stress_strain"] is True
    cfg.write_text("stress_strain = True\n")
    assert parse(["-c", str(cfg)])["stress_strain"] is True
    assert parse(["--new-arguments", "stress_strain=True"])["stress_strain"] is True
    assert parse(["--stress-strain"])["stress_strain"] is True
    assert "stress_strain" not in parse([])


def test_no_option_leaves_the_parameter_set_as_it_was():
    """Without --stress-strain the resolved parameters (what default_variables.json holds) carry no new key."""
    from vasp_amd.monolithic import parameters
    _, _, plain = parameters(["-p", "cylinder"])
    assert "stress_strain" not in plain
    _, _, v = parameters(["-p", "cylinder", "--stress-strain"])
    assert v["stress_strain"] is True and set(v) - set(plain) == {"stress_strain"}
    json.dumps(v)


# ---- the driver's side of --stress-strain with a host stand-in for the device session ------------------------------------

class _StressStub:
    """Host stand-in for HipBackend in the time loop: the state's displacement is step * D (D fixed, small, random); the
    session computes its frames with oracle_frame and keeps their principal values for the averages."""
    mesh = None

    def __init__(self, desc):
        self.desc = desc
        self.N2 = int(desc["num_nodes"])
        self.n = 6 * self.N2 + len(desc["coords"])
        self.U = np.zeros(self.n)
        m = type(self).mesh
        self.D = 0.002 * m.hmin() * np.random.default_rng(3).standard_normal(3 * self.N2)
        self.steps = 0
        self.frames = None

    def set_dirichlet_values(self, v): pass
    def set_interface_pressure(self, P): pass
    def shift(self): pass
    def set_state(self, which, x): self.U[:] = x

    def newton_solve(self, **kw):
        self.steps += 1
        self.U[:3 * self.N2] = self.steps * self.D
        return [(1e-8, 1e-9, False, 2, 1e-9)]

    def get_state(self, which, out=None):
        out[:] = self.U
        return out

    def stress_strain_begin(self, cells):
        self.cells, self.frames = np.asarray(cells), []

    def stress_strain_sample(self, frame=False):
        f = oracle_frame(type(self).mesh, self.desc, self.U[:3 * self.N2].reshape(-1, 3), self.cells)
        self.frames.append(f)
        return f if frame else None

    def stress_strain_averages(self):
        s = {k: np.zeros((len(self.cells), 4)) for k in ("MaxPrincipalStress", "MaxPrincipalStrain")}
        for f in self.frames:
            for k in s:
                s[k] += f[k]
        return dict(MaxPrincipalStress_avg=s["MaxPrincipalStress"] / len(self.frames),
                    MaxPrincipalStrain_avg=s["MaxPrincipalStrain"] / len(self.frames), samples=len(self.frames))


def _stub_run(tmp_path, extra, T):
    import contextlib
    import io
    from vasp_amd import monolithic
    from vasp_amd.mesh import FsiMesh
    _StressStub.mesh = FsiMesh.read(GOLDEN / "cylinder" / "cylinder.h5")
    lines = []
    with contextlib.redirect_stdout(io.StringIO()):
        ns = monolithic.run(["-p", "cylinder", "-dt", "0.001", "-T", T, "--theta", "0.51", "--folder", str(tmp_path), "--sub-folder",
                             "1", "--save-deg", "1", "--verbose", "False", "--stress-strain",
                             "--new-arguments", f"mesh_path={GOLDEN / 'cylinder' / 'cylinder.h5'}", *extra],
                            backend_factory=_StressStub, out=lines.append)
    return ns, lines


def test_driver_samples_the_saved_frames_and_writes_the_averages(tmp_path):
    from vasp_amd.h5lite import read_h5
    from vasp_amd.stress_strain import solid_cells
    ns, lines = _stub_run(tmp_path, ["--save-step", "2"], T="0.005")
    sb = ns["backend"]
    res = tmp_path / "1" / "StressStrain"
    np.testing.assert_array_equal(sb.cells, solid_cells(_StressStub.mesh, 2))
    _, vtimes, _ = output_file_lists(tmp_path / "1" / "Visualization" / "velocity.xdmf")
    assert len(sb.frames) == 3                                           # counters 0, 2, 4 of five steps
    for name in FRAME_NAMES:
        _, times, idx = output_file_lists(res / f"{name}.xdmf")
        assert times == vtimes and idx == [0, 1, 2]
        g = read_h5(res / f"{name}.h5")[name]
        for k, f in enumerate(sb.frames):
            np.testing.assert_array_equal(np.asarray(g[f"{name}_{k}"]["vector"].data).reshape(f[name].shape), f[name])
    ref = sb.stress_strain_averages()
    for name in AVERAGE_NAMES:
        got = np.asarray(read_h5(res / f"{name}.h5")[name][f"{name}_0"]["vector"].data).reshape(-1, 4)
        np.testing.assert_array_equal(got, ref[name])
    assert any(line.startswith("Stress and strain of 3 frames written to") for line in lines)
    assert not (tmp_path / "1" / "Hemodynamic_indices").exists()


def test_killturtle_stop_still_writes_the_averages_of_the_frames_so_far(tmp_path):
    (tmp_path / "1").mkdir(parents=True)
    (tmp_path / "1" / "killturtle").write_text("")
    ns, lines = _stub_run(tmp_path, ["--save-step", "1"], T="0.02")
    assert ns["backend"].steps == 1 and len(ns["backend"].frames) == 1
    for name in FRAME_NAMES + AVERAGE_NAMES:
        assert (tmp_path / "1" / "StressStrain" / f"{name}.h5").exists(), name
        assert (tmp_path / "1" / "StressStrain" / f"{name}.xdmf").exists(), name
    assert any("Stress and strain of 1 frames" in line for line in lines)
