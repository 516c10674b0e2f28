"""``fsi_set_frame`` and ``python -m vasp_amd.postprocess`` on the device: a saved frame put into the state is the state that
was saved, and the five options evaluated on a finished folder write the files the run itself wrote.  Every comparison is
bitwise.  A child process that ends with a time limit, an abort or a fault ends its test: nothing more is started."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

CYL = GOLDEN / "cylinder" / "cylinder.h5"
BAND = ["--hi-pass-bands", "0", "100", "--hi-pass-amplitude", "--hi-pass-window", "8"]
REGION = ["--spectrogram-fsi-region", "0", "0", "0", "100"]
FIVE = ["--hemodynamics", "--stress-strain", "--hi-pass", "d", "v", "p", *BAND, "--hi-pass-point-ids", "0", "5", "--hi-pass-tensor", "strain",
        "--hi-pass-tensor-window", "8", "--spectrogram", "v", *REGION]
TREES = ("Hemodynamic_indices", "StressStrain", "Visualization_hi_pass", "Visualization_separate_domain", "Spectrograms")
RUN = ["-dt", "0.001", "-T", "0.0235", "--theta", "0.51", "--verbose", "False", "--save-step", "1", "--save-deg", "2", "--checkpoint-step", "5"]


# ---- 1. fsi_set_frame against fsi_set_state ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cyl(cylinder_case):
    from vasp_amd.capi import HipBackend
    hb = HipBackend(cylinder_case[1])
    yield hb, cylinder_case[0]["mesh"]
    hb.close()


def _frame(mesh, x, save_deg):
    """d, v, p of the state x as a Visualization file of ``save_deg`` holds them."""
    d, v, p = mesh.split(x)
    if save_deg < 2:
        V = mesh.num_vertices
        return np.ascontiguousarray(d[:V]), np.ascontiguousarray(v[:V]), p.copy()
    e = mesh.edges
    return d.copy(), v.copy(), np.concatenate([p, 0.5 * (p[e[:, 0]] + p[e[:, 1]])])[:, None]


def test_a_save_deg_2_frame_is_the_state_bit_for_bit(cyl):
    hb, mesh = cyl
    rng = np.random.default_rng(21)
    x, y = rng.standard_normal(hb.ndof), rng.standard_normal(hb.ndof)
    hb.set_state("n", y)
    hb.set_state("n-1", y)
    d, v, p = _frame(mesh, x, 2)
    hb.set_frame("n", d, v, p)
    assert np.array_equal(hb.get_state("n"), x) and np.array_equal(hb.get_state("n-1"), y)
    # a field that is not given keeps what the state holds
    hb.set_state("n", y)
    hb.set_frame("n", d=d, p=p)
    got = mesh.split(hb.get_state("n"))
    assert np.array_equal(got[0], mesh.split(x)[0]) and np.array_equal(got[1], mesh.split(y)[1]) and np.array_equal(got[2], mesh.split(x)[2])
    hb.set_frame("n", v=v)
    assert np.array_equal(hb.get_state("n"), x)
    hb.set_frame("n-1", p=p)
    got = mesh.split(hb.get_state("n-1"))
    assert np.array_equal(got[2], mesh.split(x)[2]) and np.array_equal(got[0], mesh.split(y)[0])
    # read-only views of a mapped file go in as they are
    d.flags.writeable = False
    hb.set_state("n", y)
    hb.set_frame("n", d, v, p)
    assert np.array_equal(hb.get_state("n"), x)


def test_a_save_deg_1_frame_is_the_host_twins_state(cyl):
    from vasp_amd.frames import state_from_frame
    hb, mesh = cyl
    rng = np.random.default_rng(22)
    V, e = mesh.num_vertices, mesh.edges
    for call in range(2):                       # the edge table is built in the first call and used in the second
        x = rng.standard_normal(hb.ndof)
        d, v, p = _frame(mesh, x, 1)
        hb.set_state("n", rng.standard_normal(hb.ndof))
        hb.set_frame("n", d, v, p)
        got, ref = hb.get_state("n"), state_from_frame(mesh, 1, d, v, p)
        assert np.array_equal(got, ref), call
        gd = mesh.split(got)[0]
        assert np.array_equal(gd[:V], d) and np.array_equal(gd[V:], 0.5 * (d[e[:, 0]] + d[e[:, 1]])) and np.abs(gd[V:]).min() > 0
        assert np.array_equal(mesh.split(got)[2], p)


def test_a_frame_of_another_size_and_a_null_context_are_invalid(cyl):
    from vasp_amd.capi import FsiError, _ptr
    hb, mesh = cyl
    V, N2 = mesh.num_vertices, mesh.num_nodes
    x = np.random.default_rng(23).standard_normal(hb.ndof)
    hb.set_state("n", x)
    bad = np.zeros((V + 1, 3))
    with pytest.raises(FsiError, match=rf"{V + 1} nodes.*{V} vertices.*{N2} P2 nodes") as err:
        hb.set_frame("n", d=bad)
    assert err.value.code == 1
    assert hb.lib.fsi_set_frame(None, 0, V, _ptr(bad), None, None) == 1
    assert hb.lib.fsi_set_frame(hb.ctx, 2, V, _ptr(bad), None, None) == 1              # the last rhs is no frame's place
    assert np.array_equal(hb.get_state("n"), x)                                         # nothing was written
    d, v, p = _frame(mesh, x + 1.0, 2)
    hb.set_frame("n", d, v, p)
    assert np.array_equal(hb.get_state("n"), x + 1.0)


# ---- 2. a finished run, all five options -------------------------------------------------------------------------------

def _child(module, argv, cwd, limit):
    """One child under its own time limit; anything but exit status 0 fails the caller, which then starts nothing more."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", module, *argv], cwd=cwd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        pytest.fail(f"python -m {module} ended with status {r.returncode}:\n" + r.stdout[-3000:] + r.stderr[-3000:], pytrace=False)
    return r.stdout


@pytest.fixture(scope="module")
def finished(tmp_path_factory):
    """(results of a 24-step run with the five options, the folder ``postprocess`` wrote the same options into)."""
    tmp = tmp_path_factory.mktemp("finished")
    results, again = tmp / "case" / "1", tmp / "again"
    log = _child("vasp_amd.monolithic", ["-p", "cylinder", *RUN, *FIVE, "--folder", str(results.parent), "--sub-folder", "1",
                                         "--new-arguments", f"mesh_path={CYL}"], tmp, 300)
    assert "Solved for timestep 24," in log and "Hemodynamic indices of 24 frames" in log
    log = _child("vasp_amd.postprocess", ["--folder", str(results), "--output-folder", str(again), *FIVE], tmp, 120)
    assert "Read 24 of 24 frames" in log
    return results, again


def _datasets(path):
    from vasp_amd.h5lite import Dataset, read_h5
    out = {}

    def walk(g, prefix):
        for k in g.keys():
            if isinstance(g[k], Dataset):
                a = np.asarray(g[k].data)
                out[prefix + k] = (str(a.dtype), a.shape, a.tobytes())
            else:
                walk(g[k], prefix + k + "/")

    walk(read_h5(path), "/")
    return out


def _same_tree(a, b):
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir()) and names, a.name
    for name in names:
        if name.endswith(".h5"):
            got = _datasets(a / name)
            assert got == _datasets(b / name) and got, name
        else:
            assert (a / name).read_bytes() == (b / name).read_bytes(), name
    return names


def _series(folder, name):
    """The frames of a DG1 series in the XDMF's order, each from the file the XDMF names: (times, vectors)."""
    from vasp_amd.h5lite import read_h5
    from vasp_amd.hemodynamics import xdmf_frames
    listed = xdmf_frames(folder / f"{name}.xdmf")
    files = {f: read_h5(folder / f)[name] for f in sorted({f for _, f, _ in listed})}
    return [t for t, _, _ in listed], [np.asarray(files[f][f"{name}_{k}"]["vector"].data) for _, f, k in listed]


def test_the_five_options_on_a_finished_folder_write_what_the_run_wrote(finished):
    from vasp_amd.stress_strain import FRAME_NAMES
    results, again = finished
    names = {tree: _same_tree(results / tree, again / tree) for tree in TREES}
    assert len(names["Hemodynamic_indices"]) == 12 and len(names["StressStrain"]) == 12 and len(names["Spectrograms"]) == 4
    assert sorted(names["Visualization_separate_domain"]) == sorted(f"{f}_point_id_{i}.csv" for f in ("displacement", "velocity", "pressure") for i in (0, 5))
    assert any(n.startswith("GreenLagrangeStrain_0_to_100_max_principal_amplitude") for n in names["Visualization_hi_pass"])
    for folder, series in (("Hemodynamic_indices", ("WSS",)), ("StressStrain", FRAME_NAMES)):
        for name in series:                       # frame by frame behind the XDMF, with the run's times
            (t_run, x_run), (t_new, x_new) = _series(results / folder, name), _series(again / folder, name)
            assert t_run == t_new and len(t_run) == 24 and all(np.array_equal(a, b) for a, b in zip(x_run, x_new)), name
    assert not (again / "Checkpoint").exists() and not (again / "Visualization").exists()


# ---- 3. a window -------------------------------------------------------------------------------------------------------

def _drive(argv, out_folder, keys, by_state=False, half_spacing=False):
    """The options ``keys`` over the frames ``postprocess.prepare`` selects for ``argv``, in a context of this process:
    FrameSource, set_frame (or, ``by_state``, the host twin's vector through set_state), sample, finish."""
    from vasp_amd import postprocess
    from vasp_amd.fem import FormTerms
    from vasp_amd.frames import state_from_frame
    from vasp_amd.monolithic import SESSIONS, _session_part, build_description
    with contextlib.redirect_stdout(io.StringIO()):
        ns, mesh, source, indices, fields = postprocess.prepare(argv)
    ns = dict(ns, results_folder=out_folder)
    desc, _, _ = build_description(mesh, ns["default_variables"], [], FormTerms())
    hb = postprocess.default_backend(desc)
    try:
        runs = [_session_part(module, cls)(hb, mesh, ns) for key, module, _, cls, _ in SESSIONS if key in keys]
        for t, views in source.frames(indices, fields):
            if by_state:
                keep = hb.get_state("n")
                x = state_from_frame(mesh, int(ns["save_deg"]), **views)
                for q, part, old in zip("dvp", mesh.split(x), mesh.split(keep)):
                    if q not in views:
                        part[...] = old
                hb.set_state("n", x)
            else:
                hb.set_frame("n", **views)
            for r in runs:
                r.sample(t, None)
        lines = []
        for r in runs:
            r.finish(lines.append)
        twssg = None
        if half_spacing:                          # the same frames with half the sample spacing: every term of TWSSG doubles
            fp = runs[0].fingerprint
            hb.hemodynamics_begin(*_facets(mesh, ns), fp["mu"], fp["dt_sample"] / 2)
            for t, views in source.frames(indices, fields):
                hb.set_frame("n", **views)
                hb.hemodynamics_sample()
            twssg = hb.hemodynamics_indices()["TWSSG"]
    finally:
        source.close()
        hb.close()
    return ns, [source.times[k] for k in indices], runs, twssg


def _facets(mesh, ns):
    from vasp_amd.hemodynamics import fluid_boundary_facets
    _, cells, local = fluid_boundary_facets(mesh, ns["dx_f_id"])
    return cells, local


def test_a_window_of_a_finished_folder(finished, tmp_path):
    from vasp_amd.h5lite import read_h5
    from vasp_amd.stress_strain import FRAME_NAMES
    results, _ = finished
    argv = ["--folder", str(results), "--hemodynamics", "--stress-strain", "--stride", "2", "--start-time", "0.004"]
    log = _child("vasp_amd.postprocess", [*argv, "--output-folder", str(tmp_path / "tool")], tmp_path, 120)
    assert "Read 10 of 24 frames" in log and "Hemodynamic indices of 10 frames" in log and "Stress and strain of 10 frames" in log
    ns, times, runs, twssg_half = _drive(argv, tmp_path / "own", ("hemodynamics", "stress_strain"), half_spacing=True)
    t_run, x_run = _series(results / "Hemodynamic_indices", "WSS")
    assert times == t_run[4:24:2] and abs(times[0] - 0.005) < 1e-12 and ns["frame_stride"] == 2
    assert runs[0].fingerprint["dt_sample"] == 0.001 * 1 * 2 == runs[1].fingerprint["dt_sample"]
    for tree in ("Hemodynamic_indices", "StressStrain"):
        _same_tree(tmp_path / "tool" / tree, tmp_path / "own" / tree)
    for folder, series in (("Hemodynamic_indices", ("WSS",)), ("StressStrain", FRAME_NAMES)):
        for name in series:
            t_tool, x_tool = _series(tmp_path / "tool" / folder, name)
            assert t_tool == times and len(x_tool) == 10, name
    # the WSS frames are those the run wrote at these times; the indices are not the run's (other frames, other spacing)
    _, x_tool = _series(tmp_path / "tool" / "Hemodynamic_indices", "WSS")
    assert all(np.array_equal(x_tool[j], x_run[t_run.index(t)]) for j, t in enumerate(times))
    index = lambda folder, name: np.asarray(read_h5(folder / "Hemodynamic_indices" / f"{name}.h5")[name][f"{name}_0"]["vector"].data)
    assert not np.array_equal(index(tmp_path / "tool", "TAWSS"), index(results, "TAWSS"))
    twssg = index(tmp_path / "tool", "TWSSG").reshape(twssg_half.shape)
    assert np.isfinite(twssg).any() and np.array_equal(2.0 * twssg, twssg_half, equal_nan=True)       # formed with dt * save_step * 2
    assert sorted(p.name for p in (tmp_path / "tool").iterdir()) == ["Hemodynamic_indices", "StressStrain"]


# ---- 4. a restarted folder ---------------------------------------------------------------------------------------------

HOOK_PROBLEM = '''
"""cylinder with a hook that drops killturtle in the step that ends at t = 0.011."""
from pathlib import Path as _Path
from vasp_amd.problems.cylinder import *  # noqa: F401,F403
from vasp_amd.problems import cylinder as _base


def post_solve(**ns):
    upd = _base.post_solve(**ns)
    if abs(ns["t"] - 0.011) < 1e-9:
        (_Path(ns["results_folder"]) / "killturtle").write_text("")
    return upd
'''


def test_a_restarted_folder_is_read_through_both_files_of_a_field(tmp_path):
    """A run without sessions stopped in its 11th step and continued to 24: ``<name>.h5`` holds 11 frames, ``<name>_run_1.h5``
    13.  ``postprocess`` over that folder writes what the sessions of this process form from the same frames, put into the
    state as whole vectors of the host twin."""
    (tmp_path / "split_case.py").write_text(HOOK_PROBLEM)
    results = tmp_path / "case" / "1"
    run = ["-p", "split_case", *RUN]
    log = _child("vasp_amd.monolithic", [*run, "--folder", str(results.parent), "--sub-folder", "1", "--new-arguments", f"mesh_path={CYL}"], tmp_path, 300)
    assert "killturtle found" in log and "Solved for timestep 11," in log and "Solved for timestep 12," not in log
    log = _child("vasp_amd.monolithic", [*run, "--restart-folder", str(results), "--new-arguments", f"mesh_path={CYL}"], tmp_path, 300)
    assert "t = 0.0240" in log and "t = 0.0250" not in log
    from vasp_amd.frames import FrameSource
    src = FrameSource(results, 2)
    assert [e[1:] for e in src.entries["velocity"]] == [("velocity.h5", k) for k in range(11)] + [("velocity_run_1.h5", k) for k in range(13)]
    src.close()
    options = ["--hemodynamics", "--hi-pass", "v", "p", *BAND, "--spectrogram", "v", *REGION]
    log = _child("vasp_amd.postprocess", ["--folder", str(results), "--output-folder", str(tmp_path / "tool"), *options], tmp_path, 120)
    assert "Read 24 of 24 frames" in log
    _drive(["--folder", str(results), *options], tmp_path / "own", ("hemodynamics", "hi_pass", "spectrogram"), by_state=True)
    for tree in ("Hemodynamic_indices", "Visualization_hi_pass", "Spectrograms"):
        _same_tree(tmp_path / "tool" / tree, tmp_path / "own" / tree)
