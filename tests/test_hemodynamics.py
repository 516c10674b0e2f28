"""Hemodynamic indices (vasp_amd/hemodynamics.py, ``--hemodynamics``) on the host: the boundary facets, the file layout of
``Hemodynamic_indices/``, the driver's refusals, and the numpy restatement of the reference's accumulation that the GPU
tests (test_gpu_hemodynamics.py) hold the device against."""
import json
import re

import numpy as np
import pytest

from conftest import GOLDEN, make_avf_case

INDEX_NAMES = ("TAWSS", "OSI", "RRT", "ECAP", "TWSSG")


# ---- the restatement of compute_hemodyanamics [REF src/vasp/postprocessing/postprocessing_fenics/compute_hemodynamics.py:
# ---- 257-350], written from the reference's formulas, independent of the kernel's closed forms ---------------------------

def twssg_projection(D, areas):
    """P1 L2 projection on each triangle of |D| for a linear vector field D (nf, 3 vertices, 3): the mass matrix and the
    right-hand side both by the 12-point degree-6 rule, solved per facet (project_dg onto DG1 of the boundary mesh)."""
    from oracle.fsi_oracle import triangle12
    tp, tw = triangle12()
    lam = np.stack([1 - tp[:, 0] - tp[:, 1], tp[:, 0], tp[:, 1]], axis=1)          # (12, 3)
    g = np.linalg.norm(np.einsum("qk,fki->fqi", lam, D), axis=2)                    # |D| at the quadrature points
    w = 2.0 * np.asarray(areas)[:, None] * tw[None, :]
    M = np.einsum("fq,qa,qb->fab", w, lam, lam)
    rhs = np.einsum("fq,qa,fq->fa", w, lam, g)
    return np.linalg.solve(M, rhs[..., None])[..., 0]


def hemo_reference(taus, dt, areas):
    """Indices (nf, 3) from the WSS frames ``taus`` (each (nf, 3, 3)), time ``dt`` between frames, facet areas."""
    nf = len(areas)
    prev = np.zeros((nf, 3, 3))                    # tau_prev = 0 before the first frame [REF :244]
    s_tau, s_mag, s_tw = np.zeros((nf, 3, 3)), np.zeros((nf, 3)), np.zeros((nf, 3))
    for tau in taus:
        s_mag += np.linalg.norm(tau, axis=2)
        s_tau += tau
        s_tw += twssg_projection((tau - prev) / dt, areas)
        prev = tau
    n = len(taus)
    tawss = s_mag / n
    m = np.linalg.norm(s_tau / n, axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        osi = 0.5 * (1 - m / tawss)
        return dict(TAWSS=tawss, OSI=osi, RRT=1 / m, ECAP=osi / tawss, TWSSG=s_tw / n)


def facet_areas(geometry, topology):
    x = geometry[topology]
    return 0.5 * np.linalg.norm(np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]), axis=1)


def output_file_lists(xdmf_file):
    """Restatement of the reference's parser [REF src/vasp/postprocessing/postprocessing_common.py:63-121]."""
    lines = open(xdmf_file).readlines()
    h5s, times, idx = [], [], []
    checkpoint_data = any("FiniteElementFunction" in line for line in lines)
    for line in lines:
        if "<Time Value" in line:
            times.append(float(re.findall('<Time Value="(.+?)"', line)[0]))
        if checkpoint_data and "vector" in line:
            h5s.append(re.findall(r'"HDF">(.*?):', line)[0])
            idx.append(int(re.findall(r"_([0-9]+)\/vector", line)[0]))
        elif not checkpoint_data and "VisualisationVector" in line:
            h5s.append(re.findall('"HDF">(.+?):/', line)[0])
            idx.append(int(re.findall("VisualisationVector/(.+?)</DataItem", line)[0]))
    return h5s, times, idx


def test_restatement_on_hand_made_sequences():
    """Known answers: tau_k = c_k tau0 with tau0 the same vector at the three vertices of a facet."""
    rng = np.random.default_rng(0)
    nf = 4
    areas = rng.uniform(0.5, 2.0, nf)
    t0 = rng.standard_normal((nf, 1, 3)) * np.ones((1, 3, 1))
    c = np.array([1.0, -0.5, 2.0, 0.25, -1.5])
    dt = 0.01
    got = hemo_reference([ck * t0 for ck in c], dt, areas)
    mag = np.linalg.norm(t0, axis=2)
    np.testing.assert_allclose(got["TAWSS"], np.abs(c).mean() * mag, rtol=1e-13)
    np.testing.assert_allclose(got["OSI"], 0.5 * (1 - abs(c.sum()) / np.abs(c).sum()), rtol=0, atol=1e-14)
    np.testing.assert_allclose(got["RRT"], 1 / (abs(c.mean()) * mag), rtol=1e-13)
    np.testing.assert_allclose(got["ECAP"], got["OSI"] / got["TAWSS"], rtol=1e-13)
    jumps = np.abs(np.diff(np.concatenate([[0.0], c])))              # |c_k - c_{k-1}|, c_0 = 0: the first term is |tau_1| / dt
    np.testing.assert_allclose(got["TWSSG"], jumps.mean() / dt * mag, rtol=1e-12)
    # a reversing flow: tau, -tau -> OSI = 1/2, RRT = inf, ECAP = 1 / (2 TAWSS)
    rev = hemo_reference([t0, -t0], dt, areas)
    np.testing.assert_allclose(rev["OSI"], 0.5, atol=1e-15)
    assert np.isinf(rev["RRT"]).all()
    # no shear at all: 0 / 0 -> NaN, as numpy gives it (no clamping)
    zero = hemo_reference([0 * t0], dt, areas)
    assert np.isnan(zero["OSI"]).all() and np.isinf(zero["RRT"]).all() and (zero["TWSSG"] == 0).all()


def test_twssg_projection_of_a_linear_magnitude():
    """|D| linear on the facet (D = s(x) e with s >= 0 linear) is P1 already: the projection returns its vertex values."""
    areas = np.array([0.3, 1.7])
    s = np.array([[1.0, 2.0, 3.5], [0.1, 0.0, 4.0]])
    e = np.array([0.6, 0.0, 0.8])
    np.testing.assert_allclose(twssg_projection(s[:, :, None] * e, areas), s, rtol=1e-12, atol=1e-14)


# ---- boundary facets --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["cylinder", "offset_stenosis", "avf"])
def test_fluid_boundary_facets_match_the_test_helper(which, tmp_path):
    from test_post_oracle import fluid_boundary_facets as helper
    from vasp_amd.hemodynamics import fluid_boundary_facets
    from vasp_amd.mesh import FsiMesh
    if which == "avf":
        ns = make_avf_case(tmp_path)[0]
        mesh, ids = ns["mesh"], ns["dx_f_id"]
    else:
        mesh = FsiMesh.read(GOLDEN / which / f"{which}.h5")
        ids = (1,)
    ref = helper(mesh, np.atleast_1d(ids))
    got = fluid_boundary_facets(mesh, ids)
    assert len(ref[0]) > 0
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)


def test_boundary_triangles_keep_the_dof_order_and_coordinates():
    from vasp_amd.hemodynamics import FACET_VERTS, boundary_triangles, fluid_boundary_facets
    from vasp_amd.mesh import FsiMesh
    mesh = FsiMesh.read(GOLDEN / "cylinder" / "cylinder.h5")
    fids, cell, local = fluid_boundary_facets(mesh, 1)
    geom, topo = boundary_triangles(mesh, cell, local)
    assert topo.shape == (len(fids), 3) and len(geom) == len(np.unique(mesh.facets[fids]))
    np.testing.assert_array_equal(geom[topo], mesh.coords[mesh.tets[cell[:, None], FACET_VERTS[local]]])
    assert (np.sort(mesh.tets[cell[:, None], FACET_VERTS[local]], axis=1) == np.sort(mesh.facets[fids], axis=1)).all()


# ---- files ---------------------------------------------------------------------------------------------------------------

def _writer_case(tmp_path, frames=3):
    from vasp_amd.hemodynamics import HemodynamicsWriter, boundary_triangles, fluid_boundary_facets
    from vasp_amd.mesh import FsiMesh
    mesh = FsiMesh.read(GOLDEN / "cylinder" / "cylinder.h5")
    _, cell, local = fluid_boundary_facets(mesh, 1)
    geom, topo = boundary_triangles(mesh, cell, local)
    nf = len(topo)
    rng = np.random.default_rng(1)
    w = HemodynamicsWriter(tmp_path / "Hemodynamic_indices", geom, topo)
    taus = [rng.standard_normal((nf, 3, 3)) for _ in range(frames)]
    for k, tau in enumerate(taus):
        w.write_wss(tau, 0.001 * (k + 1))
    ind = {name: rng.standard_normal((nf, 3)) for name in INDEX_NAMES}
    w.write_indices(ind)
    w.close()
    return w.folder, geom, topo, taus, ind


def test_writer_layout_under_the_independent_walker(tmp_path):
    from test_h5_structure_independent import Walker
    folder, geom, topo, taus, ind = _writer_case(tmp_path)
    nf, nv = len(topo), len(geom)
    tree = Walker(folder / "WSS.h5").tree()
    first = "/WSS/WSS_0"
    for k, tau in enumerate(taus):
        d = tree[f"/WSS/WSS_{k}/vector"]
        assert d["kind"] == "dataset" and np.frombuffer(d["raw"], dtype="<f8").tobytes() == tau.astype("<f8").tobytes()
    assert f"/WSS/WSS_1/cell_dofs" not in tree                         # the dof map lives under WSS_0, where it is read
    cell_dofs = np.frombuffer(tree[f"{first}/cell_dofs"]["raw"], dtype="<i8")
    x_cell_dofs = np.frombuffer(tree[f"{first}/x_cell_dofs"]["raw"], dtype="<i8")
    assert len(cell_dofs) == 9 * nf and (np.sort(cell_dofs) == np.arange(9 * nf)).all()
    np.testing.assert_array_equal(x_cell_dofs, 9 * np.arange(nf + 1))
    # component-major per cell, interleaved global numbering: cell f, component i, vertex k -> 3 (3 f + k) + i
    f, i, k = 5, 2, 1
    assert cell_dofs[9 * f + 3 * i + k] == 3 * (3 * f + k) + i
    np.testing.assert_array_equal(np.frombuffer(tree[f"{first}/cells"]["raw"], dtype="<i8"), np.arange(nf))
    assert np.frombuffer(tree[f"{first}/mesh/geometry"]["raw"], dtype="<f8").tobytes() == geom.tobytes()
    np.testing.assert_array_equal(np.frombuffer(tree[f"{first}/mesh/topology"]["raw"], dtype="<i8").reshape(-1, 3), topo)
    # XDMF: the consumer's parser finds the frames, the dimensions are the dof counts
    h5s, times, idx = output_file_lists(folder / "WSS.xdmf")
    assert h5s == ["WSS.h5"] * len(taus) and idx == list(range(len(taus)))
    assert times == [0.001 * (k + 1) for k in range(len(taus))]
    text = (folder / "WSS.xdmf").read_text()
    assert text.count(f'<DataItem Dimensions="{9 * nf} 1" NumberType="Float" Format="HDF">WSS.h5:WSS/WSS_') == len(taus)
    assert f'<DataItem Dimensions="{nv} 3" Format="HDF">WSS.h5:WSS/WSS_0/mesh/geometry' in text
    assert 'ItemType="FiniteElementFunction" ElementFamily="DG" ElementDegree="1" ElementCell="triangle"' in text
    assert text.rstrip().endswith("</Xdmf>")
    for name in INDEX_NAMES:
        tr = Walker(folder / f"{name}.h5").tree()
        base = f"/{name}/{name}_0"
        vals = np.frombuffer(tr[f"{base}/vector"]["raw"], dtype="<f8")
        np.testing.assert_array_equal(vals, ind[name].reshape(-1))
        np.testing.assert_array_equal(np.frombuffer(tr[f"{base}/cell_dofs"]["raw"], dtype="<i8"), np.arange(3 * nf))
        np.testing.assert_array_equal(np.frombuffer(tr[f"{base}/x_cell_dofs"]["raw"], dtype="<i8"), 3 * np.arange(nf + 1))
        h5s, times, idx = output_file_lists(folder / f"{name}.xdmf")
        assert h5s == [f"{name}.h5"] and times == [0.0] and idx == [0]
        xt = (folder / f"{name}.xdmf").read_text()
        assert f'AttributeType="Scalar"' in xt and f'Dimensions="{3 * nf} 1" NumberType="Float"' in xt


def test_writer_files_read_back_through_h5lite(tmp_path):
    from vasp_amd.h5lite import read_h5
    folder, geom, topo, taus, ind = _writer_case(tmp_path, frames=2)
    g = read_h5(folder / "WSS.h5")
    for k, tau in enumerate(taus):
        np.testing.assert_array_equal(np.asarray(g["WSS"][f"WSS_{k}"]["vector"].data).reshape(-1, 3, 3), tau)
    assert g["WSS"]["WSS_0"]["mesh"]["topology"].attrs["celltype"] in ("triangle", b"triangle")
    for name in INDEX_NAMES:
        np.testing.assert_array_equal(np.asarray(read_h5(folder / f"{name}.h5")[name][f"{name}_0"]["vector"].data).reshape(-1, 3),
                                      ind[name])


# ---- the driver's refusals -----------------------------------------------------------------------------------------------

class _NeverBuilt:
    """A backend factory that must not be reached."""
    def __init__(self, desc):
        raise AssertionError("the backend was created")


def _refused(tmp_path, extra, factory=_NeverBuilt, env=None, monkeypatch=None):
    from vasp_amd import monolithic
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    with pytest.raises(SystemExit) as e:
        monolithic.run(["-p", "cylinder", "-dt", "0.001", "-T", "0.002", "--folder", str(tmp_path), "--sub-folder", "1",
                        "--verbose", "False", "--new-arguments", f"mesh_path={GOLDEN / 'cylinder' / 'cylinder.h5'}", *extra],
                       backend_factory=factory)
    return str(e.value)


def test_refused_without_save_step(tmp_path):
    assert "--save-step" in _refused(tmp_path, ["--save-step", "0", "--hemodynamics"])


def test_refused_with_restart_folder(tmp_path):
    assert "--restart-folder" in _refused(tmp_path, ["--restart-folder", str(tmp_path / "old"), "--hemodynamics"])


def test_refused_on_more_than_one_rank(tmp_path, monkeypatch):
    msg = _refused(tmp_path, ["--hemodynamics"], env={"WORLD_SIZE": "2", "RANK": "1"}, monkeypatch=monkeypatch)
    assert "WORLD_SIZE" in msg


def test_refused_for_a_backend_without_the_session(tmp_path):
    from oracle.backend import OracleBackend

    class Oracle(OracleBackend):
        def __init__(self, desc):
            raise AssertionError("the backend was created")

    assert "hemodynamics_begin" in _refused(tmp_path, ["--hemodynamics"], factory=Oracle)


def test_osi_range_line():
    from vasp_amd.hemodynamics import osi_range_message
    assert osi_range_message(np.array([0.0, 0.2, 0.5])).endswith(": within 0 to 0.5")
    assert osi_range_message(np.array([-1e-6, 0.2])).endswith("NOT within 0 to 0.5")
    assert "1 dofs NaN" in osi_range_message(np.array([np.nan, 0.2]))


def test_option_from_a_config_file_and_new_arguments(tmp_path):
    from vasp_amd.monolithic import parse
    cfg = tmp_path / "run.cfg"
    cfg.write_text("hemodynamics = True\n")
    assert parse(["-c", str(cfg)])["hemodynamics"] is True
    assert parse(["--new-arguments", "hemodynamics=True"])["hemodynamics"] is True
    assert parse(["--hemodynamics"])["hemodynamics"] is True
    assert "hemodynamics" not in parse([])


def test_no_option_leaves_the_parameter_set_as_it_was(tmp_path):
    """Without --hemodynamics the resolved parameters (what default_variables.json holds) carry no new key."""
    from vasp_amd.monolithic import parameters
    _, _, v = parameters(["-p", "cylinder"])
    assert "hemodynamics" not in v
    _, _, v = parameters(["-p", "cylinder", "--hemodynamics"])
    assert v["hemodynamics"] is True
    json.dumps(v)


# ---- the driver's side of --hemodynamics with a host stand-in for the device session -----------------------------------

class _HemoStub:
    """Host stand-in for HipBackend in the time loop: the state's velocity is step * V (V fixed, random), the session keeps
    the WSS frames it was asked for (oracle.post_oracle.wall_shear_stress) and forms the indices with hemo_reference."""
    mesh = None

    def __init__(self, desc):
        self.N2 = int(desc["num_nodes"])
        self.n = 6 * self.N2 + len(desc["coords"])
        self.U = np.zeros(self.n)
        self.V = np.random.default_rng(3).standard_normal(3 * self.N2)
        self.steps = 0
        self.taus = None

    def set_dirichlet_values(self, v): pass
    def set_interface_pressure(self, P): pass
    def shift(self): pass
    def set_state(self, which, x): self.U[:] = x

    def newton_solve(self, **kw):
        self.steps += 1
        self.U[3 * self.N2:6 * self.N2] = self.steps * self.V
        return [(1e-8, 1e-9, False, 2, 1e-9)]

    def get_state(self, which, out=None):
        out[:] = self.U
        return out

    def hemodynamics_begin(self, cells, local, mu, dt_sample):
        self.args, self.taus = (np.asarray(cells), np.asarray(local), mu, dt_sample), []

    def hemodynamics_sample(self, wss=False):
        from oracle.post_oracle import wall_shear_stress
        m = type(self).mesh
        cells, local, mu, _ = self.args
        self.taus.append(wall_shear_stress(m.coords, m.tets, m.tet_nodes, self.U[3 * self.N2:6 * self.N2].reshape(-1, 3), cells,
                                           local, mu))
        return self.taus[-1] if wss else None

    def hemodynamics_indices(self):
        from vasp_amd.hemodynamics import boundary_triangles
        geom, topo = boundary_triangles(type(self).mesh, self.args[0], self.args[1])
        out = hemo_reference(self.taus, self.args[3], facet_areas(geom, topo))
        out["samples"] = len(self.taus)
        return out


def _stub_run(tmp_path, extra, T):
    import contextlib
    import io
    from vasp_amd import monolithic
    from vasp_amd.mesh import FsiMesh
    _HemoStub.mesh = FsiMesh.read(GOLDEN / "cylinder" / "cylinder.h5")
    lines = []
    with contextlib.redirect_stdout(io.StringIO()):
        ns = monolithic.run(["-p", "cylinder", "-dt", "0.001", "-T", T, "--theta", "0.51", "--folder", str(tmp_path), "--sub-folder",
                             "1", "--save-deg", "1", "--verbose", "False", "--hemodynamics",
                             "--new-arguments", f"mesh_path={GOLDEN / 'cylinder' / 'cylinder.h5'}", *extra],
                            backend_factory=_HemoStub, out=lines.append)
    return ns, lines


def test_driver_samples_the_saved_frames_and_writes_the_indices(tmp_path):
    from vasp_amd.h5lite import read_h5
    ns, lines = _stub_run(tmp_path, ["--save-step", "2"], T="0.005")
    hb = ns["backend"]
    res = tmp_path / "1"
    _, vtimes, _ = output_file_lists(res / "Visualization" / "velocity.xdmf")
    _, times, idx = output_file_lists(res / "Hemodynamic_indices" / "WSS.xdmf")
    assert len(hb.taus) == 3 and times == vtimes and idx == [0, 1, 2]          # counters 0, 2, 4 of five steps
    cells, local, mu, dt_sample = hb.args
    assert mu == 3.5e-3 and dt_sample == 0.002
    ref = hb.hemodynamics_indices()
    for name in INDEX_NAMES:
        got = np.asarray(read_h5(res / "Hemodynamic_indices" / f"{name}.h5")[name][f"{name}_0"]["vector"].data).reshape(-1, 3)
        np.testing.assert_array_equal(got, ref[name])
    assert any("OSI range" in line for line in lines)


def test_killturtle_stop_still_writes_the_indices_of_the_frames_so_far(tmp_path):
    (tmp_path / "1").mkdir(parents=True)
    (tmp_path / "1" / "killturtle").write_text("")
    ns, lines = _stub_run(tmp_path, ["--save-step", "1"], T="0.02")
    assert ns["backend"].steps == 1 and len(ns["backend"].taus) == 1
    for name in ("WSS",) + INDEX_NAMES:
        assert (tmp_path / "1" / "Hemodynamic_indices" / f"{name}.h5").exists(), name
