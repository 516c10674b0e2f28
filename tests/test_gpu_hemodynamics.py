"""Hemodynamic indices accumulated on the device (csrc/fsi_hemo.hip, HipBackend.hemodynamics_*, ``--hemodynamics``)
against the WSS kernel, the host restatement of the reference's accumulation (test_hemodynamics.py), closed forms and the
reference's own Poiseuille test."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, prepare_case
from test_hemodynamics import INDEX_NAMES, facet_areas, hemo_reference, output_file_lists, twssg_projection

pytestmark = pytest.mark.gpu

MU = 3.5e-3


@pytest.fixture(scope="module")
def cyl(cylinder_case):
    from vasp_amd.capi import HipBackend
    hb = HipBackend(cylinder_case[1])
    yield hb
    hb.close()


@pytest.fixture(scope="module")
def facets(cylinder_case):
    from vasp_amd.hemodynamics import boundary_triangles, fluid_boundary_facets
    mesh = cylinder_case[0]["mesh"]
    _, cell, local = fluid_boundary_facets(mesh, 1)
    geom, topo = boundary_triangles(mesh, cell, local)
    return cell, local, facet_areas(geom, topo)


def _velocity_state(ndof, mesh, v):
    U = np.zeros(ndof)
    N2 = mesh.num_nodes
    U[3 * N2:6 * N2] = np.asarray(v).reshape(-1)
    return U


def _close(got, ref, rtol):
    scale = np.abs(ref[np.isfinite(ref)]).max()
    assert np.abs(got - ref).max() <= rtol * scale, (np.abs(got - ref).max(), scale)


def test_sampled_wss_equals_the_wall_shear_stress_kernel(cyl, cylinder_case, facets):
    mesh = cylinder_case[0]["mesh"]
    cell, local, _ = facets
    rng = np.random.default_rng(11)
    cyl.set_state("n", _velocity_state(cyl.ndof, mesh, rng.standard_normal((mesh.num_nodes, 3))))
    ref = cyl.wall_shear_stress(cell, local, MU)
    cyl.hemodynamics_begin(cell, local, MU, 1e-3)
    got = cyl.hemodynamics_sample(wss=True)
    assert cyl.hemodynamics_sample() is None
    assert np.abs(got - ref).max() <= 1e-14 * np.abs(ref).max()
    assert np.array_equal(got, ref)                       # same device function on the same state: the same bits
    cyl.hemodynamics_end()
    cyl.set_state("n", np.zeros(cyl.ndof))


def test_indices_match_the_host_restatement(cyl, cylinder_case, facets):
    """Six independent random velocity states; the host side accumulates oracle.post_oracle.wall_shear_stress."""
    from oracle.post_oracle import wall_shear_stress
    mesh = cylinder_case[0]["mesh"]
    cell, local, areas = facets
    dt = 2.5e-3
    rng = np.random.default_rng(12)
    cyl.hemodynamics_begin(cell, local, MU, dt)
    taus = []
    for _ in range(6):
        v = rng.standard_normal((mesh.num_nodes, 3))
        cyl.set_state("n", _velocity_state(cyl.ndof, mesh, v))
        cyl.hemodynamics_sample()
        taus.append(wall_shear_stress(mesh.coords, mesh.tets, mesh.tet_nodes, v, cell, local, MU))
    got = cyl.hemodynamics_indices()
    ref = hemo_reference(taus, dt, areas)
    assert got["samples"] == 6
    for name in INDEX_NAMES:
        assert got[name].shape == (len(cell), 3)
        if name == "OSI":
            assert np.abs(got[name] - ref[name]).max() <= 1e-12, name
        else:
            _close(got[name], ref[name], 1e-10)
    again = cyl.hemodynamics_indices()                    # the session stays open; reading twice changes nothing
    for name in INDEX_NAMES:
        assert np.array_equal(again[name], got[name])
    cyl.hemodynamics_end()
    cyl.set_state("n", np.zeros(cyl.ndof))


def test_indices_of_scaled_states_follow_from_one_sample(cyl, cylinder_case, facets):
    """States c_k V: tau_k = c_k tau0, so every index is a closed form of tau0 and the c_k."""
    mesh = cylinder_case[0]["mesh"]
    cell, local, areas = facets
    V = np.random.default_rng(13).standard_normal((mesh.num_nodes, 3))
    c = np.array([0.7, -1.3, 2.1, 0.4, -0.9, 1.6])
    dt = 1e-3
    cyl.hemodynamics_begin(cell, local, MU, 1.0)
    cyl.set_state("n", _velocity_state(cyl.ndof, mesh, V))
    tau0 = cyl.hemodynamics_sample(wss=True)
    cyl.hemodynamics_begin(cell, local, MU, dt)           # replaces the session: the sums start again at zero
    for ck in c:
        cyl.set_state("n", _velocity_state(cyl.ndof, mesh, ck * V))
        cyl.hemodynamics_sample()
    got = cyl.hemodynamics_indices()
    assert got["samples"] == len(c)
    mag = np.linalg.norm(tau0, axis=2)
    jumps = np.abs(np.diff(np.concatenate([[0.0], c])))
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    assert np.abs(got["OSI"] - 0.5 * (1 - abs(c.sum()) / np.abs(c).sum())).max() <= 1e-12
    assert rel(got["TAWSS"], np.abs(c).mean() * mag) <= 1e-12
    assert rel(got["RRT"], 1 / (abs(c.mean()) * mag)) <= 1e-12
    assert rel(got["TWSSG"], jumps.mean() / dt * twssg_projection(tau0, areas)) <= 1e-12
    cyl.hemodynamics_end()
    cyl.set_state("n", np.zeros(cyl.ndof))


def test_poiseuille_flow_known_answer(tmp_path):
    """The reference's own test restated [REF tests/test_compute_hemodynamics.py:9-88]: u = G/(4 mu)(R^2 - r^2) e_x in a
    tube; TAWSS on the straight wall = G R / 2 within 2.5 % (the polygonal wall lowers it by cos(pi / 4 nc)), OSI in
    [0, 1/2] and zero for a steady field.  Sharper: on cells with one boundary facet tau = (2 mu U / R^2) h e_x at every
    vertex, h = distance of the facet's plane from the axis (P2 reproduces the quadratic, the traction is constant)."""
    from vasp_amd.capi import HipBackend
    from vasp_amd.hemodynamics import boundary_triangles, fluid_boundary_facets
    from vasp_amd.meshgen import R_LUMEN, X_MAX, sizes_for, write_mesh
    assert sizes_for(50_000)[0] >= 4
    write_mesh(tmp_path / "tube.h5", 50_000)
    ns, desc = prepare_case("offset_stenosis", tmp_path / "tube.h5", tmp_path / "run")[:2]
    mesh = ns["mesh"]
    mu, G, R = 3.5e-3, 40.0, R_LUMEN
    U = G * R ** 2 / (4 * mu)
    x = mesh.node_coords
    v = np.zeros((mesh.num_nodes, 3))
    v[:, 0] = G / (4 * mu) * (R ** 2 - x[:, 1] ** 2 - x[:, 2] ** 2)
    _, cell, local = fluid_boundary_facets(mesh, ns["dx_f_id"])
    geom, topo = boundary_triangles(mesh, cell, local)
    hb = HipBackend(desc)
    try:
        hb.set_state("n", _velocity_state(hb.ndof, mesh, v))
        hb.hemodynamics_begin(cell, local, mu, 1e-3)
        for _ in range(3):
            tau = hb.hemodynamics_sample(wss=True)
        ind = hb.hemodynamics_indices()
    finally:
        hb.close()
    xf = geom[topo]                                                     # (nf, 3, 3) facet vertex coordinates
    D = 2 * R
    rad = np.linalg.norm(xf[:, :, 1:], axis=2)
    straight = ((xf[:, :, 0] >= D).all(axis=1) & (xf[:, :, 0] <= X_MAX - 0.3 * D).all(axis=1)
                & np.isclose(rad, R, rtol=1e-9).all(axis=1))            # lumen wall facets downstream of the stenosis
    assert straight.sum() > 100
    areas = facet_areas(geom, topo)
    mean_tawss = (areas[straight] * ind["TAWSS"][straight].mean(axis=1)).sum() / areas[straight].sum()
    assert abs(mean_tawss / (G * R / 2) - 1) <= 0.025, mean_tawss / (G * R / 2)
    assert ind["OSI"].min() >= -1e-12 and ind["OSI"].max() <= 0.5
    assert np.abs(ind["OSI"][straight]).max() <= 1e-12
    single = straight & (np.bincount(cell)[cell] == 1)
    assert single.sum() > 50
    nrm = np.cross(xf[:, 1] - xf[:, 0], xf[:, 2] - xf[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    h = np.abs(np.einsum("fi,fi->f", xf[:, 0], nrm))                    # the axis is x: distance of the plane from it
    exact = np.zeros((len(cell), 3, 3))
    exact[:, :, 0] = (2 * mu * U / R ** 2 * h)[:, None]
    assert np.abs(tau[single] - exact[single]).max() <= 1e-10 * np.abs(exact[single]).max()


def _run_cylinder(folder, extra):
    cmd = [sys.executable, "-m", "vasp_amd.monolithic", "-p", "cylinder", "-dt", "0.001", "-T", "0.004", "--theta", "0.51",
           "--verbose", "False", "--folder", str(folder), "--sub-folder", "1", "--save-step", "1", "--save-deg", "2",
           "--checkpoint-step", "2", "--new-arguments", f"mesh_path={GOLDEN / 'cylinder' / 'cylinder.h5'}", *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return folder / "1", r.stdout


def test_end_to_end_run_matches_its_own_visualization_files(tmp_path):
    """--hemodynamics in a fresh process; the indices it wrote vs a host recomputation from its Visualization/velocity.h5
    (save_deg 2: the P2 nodal values - what vasp-compute-hemo would read)."""
    import json
    from oracle.post_oracle import wall_shear_stress
    from vasp_amd.h5lite import read_h5
    from vasp_amd.hemodynamics import boundary_triangles, fluid_boundary_facets
    from vasp_amd.mesh import FsiMesh
    res, log = _run_cylinder(tmp_path / "with", ["--hemodynamics"])
    hemo = res / "Hemodynamic_indices"
    for name in ("WSS",) + INDEX_NAMES:
        assert (hemo / f"{name}.h5").exists() and (hemo / f"{name}.xdmf").exists(), name
    assert "OSI range" in log
    mesh = FsiMesh.read(GOLDEN / "cylinder" / "cylinder.h5")
    _, cell, local = fluid_boundary_facets(mesh, 1)
    geom, topo = boundary_triangles(mesh, cell, local)
    _, vtimes, vidx = output_file_lists(res / "Visualization" / "velocity.xdmf")
    h5s, times, idx = output_file_lists(hemo / "WSS.xdmf")
    k = len(vtimes)                                                      # every step writes a frame (save_step 1)
    assert k >= 4 and times == vtimes and idx == list(range(k)) and h5s == ["WSS.h5"] * k
    vel = read_h5(res / "Visualization" / "velocity.h5")["VisualisationVector"]
    wss = read_h5(hemo / "WSS.h5")["WSS"]
    taus = []
    for k in vidx:
        v = np.asarray(vel[str(k)].data)[:mesh.num_nodes]
        taus.append(wall_shear_stress(mesh.coords, mesh.tets, mesh.tet_nodes, v, cell, local, 3.5e-3))
        _close(np.asarray(wss[f"WSS_{k}"]["vector"].data).reshape(-1, 3, 3), taus[-1], 1e-10)
    ref = hemo_reference(taus, 1e-3, facet_areas(geom, topo))
    for name in INDEX_NAMES:
        got = np.asarray(read_h5(hemo / f"{name}.h5")[name][f"{name}_0"]["vector"].data).reshape(-1, 3)
        if name == "OSI":
            assert np.abs(got - ref[name]).max() <= 1e-12
        else:
            _close(got, ref[name], 1e-10)
    # the same run without the option: no Hemodynamic_indices/, today's key set in the checkpoint's JSON
    plain, _ = _run_cylinder(tmp_path / "without", [])
    assert not (plain / "Hemodynamic_indices").exists()
    keys_plain = set(json.loads((plain / "Checkpoint" / "default_variables.json").read_text()))
    keys_hemo = set(json.loads((res / "Checkpoint" / "default_variables.json").read_text()))
    assert "hemodynamics" not in keys_plain and keys_hemo - keys_plain == {"hemodynamics"}


def test_session_errors(cylinder_case, facets):
    from vasp_amd.capi import FsiError, HipBackend, _ptr
    cell, local, _ = facets
    hb = HipBackend(cylinder_case[1])
    try:
        with pytest.raises(FsiError, match="fsi_hemo_begin first"):
            hb.hemodynamics_sample()
        with pytest.raises(FsiError):
            hb.hemodynamics_indices()
        bad, zero = np.array([len(hb.cell_u2i) + 5], dtype=np.int32), np.zeros(1, dtype=np.int32)
        with pytest.raises(FsiError, match="out of range"):
            hb._check(hb.lib.fsi_hemo_begin(hb.ctx, 1, _ptr(bad), _ptr(zero), MU, 1e-3))
        with pytest.raises(FsiError, match="mu > 0"):
            hb.hemodynamics_begin(cell, local, 0.0, 1e-3)
        with pytest.raises(FsiError, match="dt_sample > 0"):
            hb.hemodynamics_begin(cell, local, MU, 0.0)
        with pytest.raises(FsiError, match="twice"):
            hb.hemodynamics_begin(np.concatenate([cell, cell[:1]]), np.concatenate([local, local[:1]]), MU, 1e-3)
        hb.hemodynamics_begin(cell, local, MU, 1e-3)
        with pytest.raises(FsiError, match="no sample"):
            hb.hemodynamics_indices()
        hb.hemodynamics_sample()
        assert hb.hemodynamics_indices()["samples"] == 1
        hb.hemodynamics_end()
        with pytest.raises(FsiError):
            hb.hemodynamics_sample()
    finally:
        hb.close()
