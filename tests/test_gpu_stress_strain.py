"""Solid stress and strain sampled on the device (csrc/fsi_stress.hip, HipBackend.stress_strain_*, ``--stress-strain``)
against the one-shot kernel (fsi_stress_strain), the host's running sums, oracle/post_oracle.py and the run's own
Visualization files."""
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, make_avf_case, prepare_case
from test_hemodynamics import output_file_lists
from test_stress_strain import AVERAGE_NAMES, FRAME_NAMES, oracle_frame

pytestmark = pytest.mark.gpu

TENSORS = ("TrueStress", "GreenLagrangeStrain")


@pytest.fixture(scope="module")
def cyl(cylinder_case):
    from vasp_amd.capi import HipBackend
    hb = HipBackend(cylinder_case[1])
    yield hb
    hb.close()


def _solid(desc):
    return np.nonzero(np.asarray(desc["cell_kind"]) == 1)[0]


def _strained(ndof, mesh, scale, rng):
    U = np.zeros(ndof)
    U[:3 * mesh.num_nodes] = scale * mesh.hmin() * rng.standard_normal(3 * mesh.num_nodes)
    return U


def _check_against_oracle(got, ref, lapack=None):
    """The tolerances of test_gpu_parity.py::test_stress_strain_kernel_matches_oracle.  With ``lapack`` (the oracle with
    eig="eigvalsh"), a principal value that the closed form itself cannot give to 1e-7 - a stress dominated by its
    hydrostatic part, where get_eig's discriminant cancels - is held instead to LAPACK, within ten times the oracle's own
    closed-form error there."""
    for key in FRAME_NAMES:
        scale = np.abs(ref[key]).max()
        tol = 1e-10 if key in TENSORS else 1e-7
        err = np.abs(got[key] - ref[key]).max()
        if err <= tol * scale or lapack is None or key in TENSORS:
            assert err <= tol * scale, key
        else:
            own = np.abs(ref[key] - lapack[key]).max()
            assert own > tol * scale, key                                # only where the closed form is that ill-conditioned
            assert np.abs(got[key] - lapack[key]).max() <= 10 * own + tol * scale, key


def test_sampled_frame_equals_the_one_shot_kernel(cyl, cylinder_case):
    mesh, desc = cylinder_case[0]["mesh"], cylinder_case[1]
    solid = _solid(desc)
    rng = np.random.default_rng(21)
    cyl.stress_strain_begin(solid)
    for scale in (0.005, 0.03, 0.08):
        cyl.set_state("n", _strained(cyl.ndof, mesh, scale, rng))
        ref = cyl.stress_strain(solid)
        got = cyl.stress_strain_sample(frame=True)
        assert set(got) == set(FRAME_NAMES)
        for key in FRAME_NAMES:
            assert got[key].shape == ref[key].shape
            assert np.array_equal(got[key], ref[key]), key            # same device function on the same state: the same bits
        assert cyl.stress_strain_sample() is None
    # a subset of the cells, in the caller's order, samples the same bits per cell
    sub = solid[::-7]
    cyl.stress_strain_begin(sub)
    got = cyl.stress_strain_sample(frame=True)
    ref = cyl.stress_strain(sub)
    for key in FRAME_NAMES:
        assert np.array_equal(got[key], ref[key]), key
    cyl.stress_strain_end()
    cyl.set_state("n", np.zeros(cyl.ndof))


def test_averages_are_the_sequential_sums_over_the_samples(cyl, cylinder_case):
    mesh, desc = cylinder_case[0]["mesh"], cylinder_case[1]
    solid = _solid(desc)
    rng = np.random.default_rng(22)
    cyl.stress_strain_begin(solid)
    s = {k: np.zeros((len(solid), 4)) for k in ("MaxPrincipalStress", "MaxPrincipalStrain")}
    k = 5
    for i in range(k):
        cyl.set_state("n", _strained(cyl.ndof, mesh, 0.01 * (i + 1), rng))
        f = cyl.stress_strain_sample(frame=(i % 2 == 0)) or cyl.stress_strain(solid)
        for key in s:
            s[key] = s[key] + f[key]                                     # axpy(1.0, ...) in sample order
    got = cyl.stress_strain_averages()
    assert got["samples"] == k
    for key in s:
        ref = s[key] / k
        avg = got[f"{key}_avg"]
        assert avg.shape == (len(solid), 4)
        assert np.abs(avg - ref).max() <= 1e-15 * np.abs(ref).max(), key
    again = cyl.stress_strain_averages()                              # the session stays open; reading twice changes nothing
    for name in AVERAGE_NAMES:
        assert np.array_equal(again[name], got[name])
    cyl.stress_strain_begin(solid)                                     # replaces the session: the sums start again at zero
    cyl.set_state("n", _strained(cyl.ndof, mesh, 0.02, rng))
    one = cyl.stress_strain_sample(frame=True)
    got = cyl.stress_strain_averages()
    assert got["samples"] == 1
    assert np.array_equal(got["MaxPrincipalStress_avg"], one["MaxPrincipalStress"])
    assert np.array_equal(got["MaxPrincipalStrain_avg"], one["MaxPrincipalStrain"])
    cyl.stress_strain_end()
    cyl.set_state("n", np.zeros(cyl.ndof))


def test_session_matches_the_oracle_stvk(cyl, cylinder_case):
    mesh, desc = cylinder_case[0]["mesh"], cylinder_case[1]
    assert desc["solid_models"] == [0]
    solid = _solid(desc)
    U = _strained(cyl.ndof, mesh, 0.03, np.random.default_rng(5))
    cyl.set_state("n", U)
    cyl.stress_strain_begin(solid)
    got = cyl.stress_strain_sample(frame=True)
    cyl.stress_strain_end()
    cyl.set_state("n", np.zeros(cyl.ndof))
    _check_against_oracle(got, oracle_frame(mesh, desc, U[:3 * mesh.num_nodes].reshape(-1, 3), solid))


@pytest.mark.parametrize("case_name", ["predeform", "avf"])
def test_session_matches_the_oracle_mooney_rivlin(case_name, tmp_path):
    """MooneyRivlin: the predeform problem on the cylinder, and the avf problem with its two solid regions (the oracle called
    once per region with that region's properties).  Tensors and the principal strain to 1e-10 / 1e-7 of the closed-form
    oracle; the principal stress, where MooneyRivlin's hydrostatic part makes get_eig's closed form lose digits (the
    oracle's own kopp and LAPACK values differ by up to ~2e-4 of the maximum on the avf vein), against LAPACK."""
    from vasp_amd.capi import HipBackend
    from vasp_amd.stress_strain import solid_cells
    if case_name == "predeform":
        case = prepare_case("predeform", GOLDEN / "cylinder" / "cylinder.h5", tmp_path, dt="0.01", T="0.02", theta="1.0")
        scale = 0.01
    else:
        case = make_avf_case(tmp_path)
        scale = 0.002                                            # the generated mesh has slivers: keep det F > 0 everywhere
    ns, desc = case[0], case[1]
    mesh = ns["mesh"]
    assert set(desc["solid_models"]) == {1} and len(desc["solid_models"]) == (2 if case_name == "avf" else 1)
    cells = solid_cells(mesh, ns["dx_s_id"])
    np.testing.assert_array_equal(cells, _solid(desc))
    hb = HipBackend(desc)
    try:
        U = _strained(hb.ndof, mesh, scale, np.random.default_rng(7))
        hb.set_state("n", U)
        hb.stress_strain_begin(cells)
        got = hb.stress_strain_sample(frame=True)
        hb.stress_strain_end()
    finally:
        hb.close()
    d = U[:3 * mesh.num_nodes].reshape(-1, 3)
    _check_against_oracle(got, oracle_frame(mesh, desc, d, cells), oracle_frame(mesh, desc, d, cells, eig="eigvalsh"))


def _run_cylinder(folder, extra):
    cmd = [sys.executable, "-m", "vasp_amd.monolithic", "-p", "cylinder", "-dt", "0.001", "-T", "0.004", "--theta", "0.51",
           "--verbose", "False", "--folder", str(folder), "--sub-folder", "1", "--save-step", "1", "--save-deg", "2",
           "--checkpoint-step", "2", "--new-arguments", f"mesh_path={GOLDEN / 'cylinder' / 'cylinder.h5'}", *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return folder / "1", r.stdout


def _datasets(folder):
    """Every dataset of every .h5 file under ``folder``: {(file, path): array}."""
    from vasp_amd.h5lite import Dataset, read_h5
    out = {}

    def walk(g, prefix, fname):
        for k in g.keys():
            v = g[k]
            if isinstance(v, Dataset):
                out[(fname, prefix + k)] = np.asarray(v.data)
            else:
                walk(v, prefix + k + "/", fname)

    for p in sorted(folder.glob("*.h5")):
        walk(read_h5(p), "/", p.name)
    return out


def test_end_to_end_run_matches_its_own_visualization_files(tmp_path, cylinder_case):
    """--stress-strain in a fresh process; its frames vs the oracle recomputed from its Visualization/displacement.h5
    (save_deg 2: the first num_nodes rows are the P2 nodal values - what vasp-compute-stress rebuilds), the averages vs the
    mean of the written frames."""
    from vasp_amd.h5lite import read_h5
    from vasp_amd.mesh import FsiMesh
    from vasp_amd.stress_strain import solid_cells, solid_submesh
    res, log = _run_cylinder(tmp_path / "with", ["--stress-strain"])
    out = res / "StressStrain"
    for name in FRAME_NAMES + AVERAGE_NAMES:
        assert (out / f"{name}.h5").exists() and (out / f"{name}.xdmf").exists(), name
    assert "Stress and strain of" in log
    mesh = FsiMesh.read(GOLDEN / "cylinder" / "cylinder.h5")
    desc = cylinder_case[1]
    cells = solid_cells(mesh, 2)
    geom, topo = solid_submesh(mesh, cells)
    _, vtimes, vidx = output_file_lists(res / "Visualization" / "displacement.xdmf")
    k = len(vtimes)
    assert k >= 4
    series = {}
    for name in FRAME_NAMES:
        h5s, times, idx = output_file_lists(out / f"{name}.xdmf")
        assert times == vtimes and idx == list(range(k)) and h5s == [f"{name}.h5"] * k, name
        series[name] = read_h5(out / f"{name}.h5")[name]
        first = series[name][f"{name}_0"]
        np.testing.assert_array_equal(np.asarray(first["mesh"]["geometry"].data), geom)
        np.testing.assert_array_equal(np.asarray(first["mesh"]["topology"].data).reshape(-1, 4), topo)
    disp = read_h5(res / "Visualization" / "displacement.h5")["VisualisationVector"]
    sums = {key: np.zeros((len(cells), 4)) for key in ("MaxPrincipalStress", "MaxPrincipalStrain")}
    for j, vk in enumerate(vidx):
        d = np.asarray(disp[str(vk)].data)[:mesh.num_nodes]
        ref = oracle_frame(mesh, desc, d, cells)
        got = {}
        for name in FRAME_NAMES:
            shape = (len(cells), 4, 3, 3) if name in TENSORS else (len(cells), 4)
            got[name] = np.asarray(series[name][f"{name}_{j}"]["vector"].data).reshape(shape)
        _check_against_oracle(got, ref)
        for key in sums:
            sums[key] = sums[key] + got[key]
    for key in sums:
        avg = np.asarray(read_h5(out / f"{key}_avg.h5")[f"{key}_avg"][f"{key}_avg_0"]["vector"].data).reshape(-1, 4)
        ref = sums[key] / k
        assert np.abs(avg - ref).max() <= 1e-15 * np.abs(ref).max(), key
    # the same run without the option: no StressStrain/, today's key set in the checkpoint's JSON
    plain, _ = _run_cylinder(tmp_path / "without", [])
    assert not (plain / "StressStrain").exists()
    keys_plain = set(json.loads((plain / "Checkpoint" / "default_variables.json").read_text()))
    keys_with = set(json.loads((res / "Checkpoint" / "default_variables.json").read_text()))
    assert "stress_strain" not in keys_plain and keys_with - keys_plain == {"stress_strain"}


def test_with_hemodynamics_the_other_outputs_are_unchanged(tmp_path):
    """--hemodynamics --stress-strain together: the two sessions are independent, so Hemodynamic_indices/ and
    Visualization/ are, array for array, those of a --hemodynamics-only run."""
    both, log = _run_cylinder(tmp_path / "both", ["--hemodynamics", "--stress-strain"])
    hemo, _ = _run_cylinder(tmp_path / "hemo", ["--hemodynamics"])
    assert (both / "StressStrain" / "TrueStress.h5").exists() and not (hemo / "StressStrain").exists()
    assert "OSI range" in log and "Stress and strain of" in log
    for sub in ("Hemodynamic_indices", "Visualization"):
        a, b = _datasets(both / sub), _datasets(hemo / sub)
        assert len(a) > 0 and set(a) == set(b), sub
        for key in a:
            assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (sub, key)


def test_session_errors(cylinder_case):
    from vasp_amd.capi import FsiError, HipBackend, _ptr
    desc = cylinder_case[1]
    solid = _solid(desc)
    fluid = np.nonzero(np.asarray(desc["cell_kind"]) == 0)[0]
    hb = HipBackend(desc)
    try:
        with pytest.raises(FsiError, match="fsi_stress_begin first"):
            hb.stress_strain_sample()
        with pytest.raises(FsiError, match="fsi_stress_begin first"):
            hb.stress_strain_averages()
        with pytest.raises(FsiError, match="not a solid cell"):
            hb.stress_strain_begin(np.concatenate([solid[:3], fluid[:1]]))
        bad = np.array([len(hb.cell_u2i) + 5], dtype=np.int32)
        with pytest.raises(FsiError, match="out of range"):
            hb._check(hb.lib.fsi_stress_begin(hb.ctx, 1, _ptr(bad)))
        bad[0] = -1
        with pytest.raises(FsiError, match="out of range"):
            hb._check(hb.lib.fsi_stress_begin(hb.ctx, 1, _ptr(bad)))
        with pytest.raises(FsiError, match="n > 0"):
            hb.stress_strain_begin(np.zeros(0, dtype=np.int64))
        hb.stress_strain_begin(solid)
        with pytest.raises(FsiError, match="no sample"):
            hb.stress_strain_averages()
        hb.stress_strain_sample()
        assert hb.stress_strain_averages()["samples"] == 1
        hb.stress_strain_end()
        with pytest.raises(FsiError, match="fsi_stress_begin first"):
            hb.stress_strain_sample()
        with pytest.raises(FsiError, match="fsi_stress_begin first"):
            hb.stress_strain_averages()
    finally:
        hb.close()
