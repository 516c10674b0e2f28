"""Band-pass sessions on the device (csrc/fsi_band.hip, HipBackend.hi_pass_*, ``--hi-pass``) against the host restatement
of scipy's filtfilt and of the reference's windowed RMS (vasp_amd/hi_pass.py)."""
import contextlib
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from vasp_amd import hi_pass as hp

pytestmark = pytest.mark.gpu

FRAMES = 72
DT = 1e-3
WINDOW = 8
STENOSIS = GOLDEN / "offset_stenosis" / "offset_stenosis.h5"


def _signal(ndof, frames=FRAMES, seed=11):
    """(frames, ndof): per dof a slow carrier, a tone three decades below it with its own frequency and phase, and noise."""
    rng = np.random.default_rng(seed)
    f, ph = rng.uniform(40.0, 450.0, ndof), rng.uniform(0.0, 2 * np.pi, ndof)
    t = (1 + np.arange(frames))[:, None] * DT
    return 1e-3 * np.sin(2 * np.pi * 1.5 * t + ph) + 1e-6 * np.sin(2 * np.pi * f * t + 2 * ph) + 1e-9 * rng.standard_normal((frames, ndof))


def _rows(mesh, states, q):
    """The rows of quantity q as the save_deg 2 Visualization writer forms them: (frames, nodes, ncomp)."""
    N2 = mesh.num_nodes
    if q == "p":
        p, e = states[:, 6 * N2:], mesh.edges
        return np.concatenate([p, 0.5 * (p[:, e[:, 0]] + p[:, e[:, 1]])], axis=1)[:, :, None]
    off = 0 if q == "d" else 3 * N2
    return states[:, off:off + 3 * N2].reshape(len(states), N2, 3)


@pytest.fixture(scope="module")
def recorded(stenosis_case):
    """A context on the small stenosis mesh driven through fsi_set_state with a prescribed signal, every frame sampled by
    the three sessions."""
    from vasp_amd.capi import HipBackend
    mesh, desc = stenosis_case[0]["mesh"], stenosis_case[1]
    hb = HipBackend(desc)
    states = _signal(hb.ndof)
    for q in "dvp":
        hb.hi_pass_begin(q, *hp.output_nodes(mesh, 2, q), capacity=FRAMES)
    for k in range(FRAMES):
        hb.set_state("n", states[k])
        for q in "dvp":
            hb.hi_pass_sample(q)
    yield hb, mesh, states
    hb.close()


def test_raw_frames_are_the_states_that_were_set(recorded):
    hb, mesh, states = recorded
    for q in "dvp":
        x = _rows(mesh, states, q)
        for k in (0, 1, FRAMES // 2, FRAMES - 1):
            assert np.array_equal(hb.hi_pass_fetch(q, "raw", k), x[k]), (q, k)


@pytest.mark.parametrize("band", [(25.0, 1000.0), (0.0, 200.0)], ids=["bandpass", "lowpass"])
def test_filtered_frames_equal_the_host_restatement_bit_for_bit(recorded, band):
    """Every filtered frame of every row of d, v and p equals vasp_amd.hi_pass.filtfilt_rows - which equals
    scipy.signal.filtfilt (tests/test_hi_pass.py) - exactly: FP64 multiply, add and subtract are correctly rounded on the
    device and the kernel is compiled without contraction."""
    hb, mesh, states = recorded
    prm = hp.design(DT, *band)
    for q in "dvp":
        y = hp.filtfilt_rows(prm["b"], prm["a"], _rows(mesh, states, q), prm["zi"], prm["padlen"])
        hb.hi_pass_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
        got = np.stack([hb.hi_pass_fetch(q, "filtered", k) for k in range(FRAMES)])
        diff = np.abs(got - y).max()
        print(f"{q} {prm['btype']}: max |device - host| = {diff:.3e}, max |y| = {np.abs(y).max():.3e}, "
              f"{int((got != y).sum())} of {y.size} values differ")
        assert np.array_equal(got, y), q
        # the raw history is kept: it is still what was set
        assert np.array_equal(hb.hi_pass_fetch(q, "raw", 3), _rows(mesh, states, q)[3])


def test_amplitudes_against_the_host_restatement(recorded):
    """Bound: the device sums a window's squares as vasp_amd.hi_pass.windowed_rms_running does (running, refreshed every 64
    windows), the reference's formula sums them directly (numpy.convolve).  The spread between the two ON THE HOST, on these
    rows, is what the summation order is worth; the device may differ from the reference's formula by 4 x that spread (the
    square root and the division add last-bit differences).  Measured on an MI355X: spread 7.6e-21 (d), 6.4e-21 (v), 1.2e-20
    (p) at amplitudes up to 2.9e-6, the device at exactly that distance from the direct sum and at distance 0 from the running
    restatement; the test prints the figures of the run."""
    hb, mesh, states = recorded
    prm = hp.design(DT, 25.0, 1000.0)
    for q in "dvp":
        y = hp.filtfilt_rows(prm["b"], prm["a"], _rows(mesh, states, q), prm["zi"], prm["padlen"])
        direct, running = hp.windowed_rms_rows(y, WINDOW), hp.windowed_rms_running(y, WINDOW)
        spread = np.abs(direct - running).max()
        hb.hi_pass_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
        hb.hi_pass_amplitude(q, WINDOW)
        amp, mag, mx, am = [], [], [], []
        for k in range(FRAMES):
            a, m1, i1 = hb.hi_pass_fetch(q, "amplitude", k, with_max=True)
            m, m2, i2 = hb.hi_pass_fetch(q, "magnitude", k, with_max=True)
            assert (m1, i1) == (m2, i2)
            amp.append(a), mag.append(m), mx.append(m1), am.append(i1)
        amp, mag = np.stack(amp), np.stack(mag)
        err = np.abs(amp - direct).max()
        print(f"{q}: host direct vs running spread {spread:.3e}, device vs direct {err:.3e}, device vs running "
              f"{np.abs(amp - running).max():.3e}, max amplitude {direct.max():.3e}")
        assert spread > 0
        assert err <= 4 * spread, q
        assert not np.isnan(amp).any() and (amp >= 0).all() and not np.isnan(mag).any()
        pad = (WINDOW - 1) // 2
        assert not amp[:pad].any() and not amp[pad + FRAMES - WINDOW + 1:].any() and amp[pad:pad + FRAMES - WINDOW + 1].all()
        # magnitude, maximum and argmax: numpy's on the fetched frames
        assert np.abs(mag - np.stack([hp.amplitude_magnitude(a) for a in amp])).max() <= 4 * np.finfo(float).eps * mag.max()
        assert np.array_equal(np.array(mx), mag.max(axis=1)) and np.array_equal(np.array(am), mag.argmax(axis=1)), q
        # a frame's value does not depend on the order of the fetches
        for k in (FRAMES - 5, 40, 3, 40, 41):
            assert np.array_equal(hb.hi_pass_fetch(q, "amplitude", k), amp[k]), (q, k)
    # low-pass: the amplitude is the filtered series itself
    low = hp.design(DT, 0.0, 200.0)
    hb.hi_pass_filter("v", low["b"], low["a"], low["zi"], low["padlen"])
    hb.hi_pass_amplitude("v", 0)
    a, m1, i1 = hb.hi_pass_fetch("v", "amplitude", 9, with_max=True)
    assert np.array_equal(a, hb.hi_pass_fetch("v", "filtered", 9))
    m = np.linalg.norm(a, axis=1)
    assert i1 == np.argmax(hb.hi_pass_fetch("v", "magnitude", 9)) and abs(m1 - m.max()) <= 4 * np.finfo(float).eps * m.max()


def test_session_errors(recorded, cylinder_case):
    from vasp_amd.capi import FsiError, HipBackend
    hb0, mesh, _ = recorded
    prm = hp.design(DT, 25.0, 1000.0)
    with pytest.raises(FsiError, match="history is full"):
        hb0.hi_pass_sample("d")
    with pytest.raises(FsiError, match="window of 73 frames, the series has 72"):
        hb0.hi_pass_filter("d", prm["b"], prm["a"], prm["zi"], prm["padlen"])
        hb0.hi_pass_amplitude("d", FRAMES + 1)
    with pytest.raises(FsiError, match="frame out of range"):
        hb0.hi_pass_fetch("d", "filtered", FRAMES)
    hb = HipBackend(cylinder_case[1])
    try:
        cmesh = cylinder_case[0]["mesh"]
        with pytest.raises(FsiError, match="fsi_band_begin first"):
            hb.hi_pass_sample("v")
        with pytest.raises(FsiError, match="node out of range"):
            hb.hi_pass_begin("p", [cmesh.num_vertices], None, 4)
        with pytest.raises(FsiError, match="node out of range"):
            hb.hi_pass_begin("d", [-1], None, 4)
        hb.hi_pass_begin("v", np.arange(cmesh.num_vertices), None, 40)
        for _ in range(33):
            hb.hi_pass_sample("v")
        with pytest.raises(FsiError, match="33 recorded frames, the filter needs more than padlen = 33"):
            hb.hi_pass_filter("v", prm["b"], prm["a"], prm["zi"], prm["padlen"])
        with pytest.raises(FsiError, match="fsi_band_filter first"):
            hb.hi_pass_fetch("v", "filtered", 0)
        hb.hi_pass_sample("v")
        hb.hi_pass_filter("v", prm["b"], prm["a"], prm["zi"], prm["padlen"])
        with pytest.raises(FsiError, match="fsi_band_amplitude first"):
            hb.hi_pass_fetch("v", "amplitude", 0)
        assert not hb.hi_pass_fetch("v", "filtered", 5).any()            # a zero state: zero in, zero out
        hb.hi_pass_end("v")
        with pytest.raises(FsiError, match="fsi_band_begin first"):
            hb.hi_pass_sample("v")
    finally:
        hb.close()


def test_a_history_beyond_device_memory_is_refused_and_the_context_still_steps(stenosis_case):
    from vasp_amd.capi import FsiError, HipBackend
    ns, desc, bc_values, pressure, hook = stenosis_case
    mesh = ns["mesh"]
    hb = HipBackend(desc)
    try:
        free_b, total_b = hb.device_memory()
        capacity = int(total_b // (8 * 3 * mesh.num_nodes)) + 1          # the raw history alone exceeds the whole device
        with pytest.raises(FsiError) as e:
            hb.hi_pass_begin("v", *hp.output_nodes(mesh, 2, "v"), capacity=capacity)
        msg = str(e.value)
        assert e.value.code == 1 and "FSI_ERR_INVALID" in msg
        need, free_said = (int(x) for x in re.search(r"needs (\d+) bytes .* has (\d+) bytes free", msg).groups())
        assert need > total_b and need >= 2 * 8 * 3 * mesh.num_nodes * capacity
        assert 0 < free_said <= total_b and abs(free_said - free_b) <= 1 << 30
        assert hb.device_memory()[0] >= free_b - (1 << 26)               # nothing was allocated
        with pytest.raises(FsiError, match="fsi_band_begin first"):
            hb.hi_pass_sample("v")
        # the context still steps
        run = dict(ns)
        run["t"] = float(ns["dt"])
        with contextlib.redirect_stdout(io.StringIO()):
            hook("pre_solve")(**run)
        hb.set_dirichlet_values(bc_values())
        hb.set_interface_pressure(float(pressure.P) if pressure is not None else 0.0)
        hist = hb.newton_solve(counter=0, first_step_num=0, **{k: ns[k] for k in ("atol", "rtol", "max_it", "lmbda", "recompute", "recompute_tstep")})
        assert len(hist) >= 1 and np.isfinite(hb.get_state("n")).all()
        hb.hi_pass_begin("v", *hp.output_nodes(mesh, 2, "v"), capacity=40)        # and a session that fits opens
        hb.hi_pass_sample("v")
        assert np.array_equal(hb.hi_pass_fetch("v", "raw", 0).ravel(), hb.get_state("n")[3 * mesh.num_nodes:6 * mesh.num_nodes])
    finally:
        hb.close()


def test_a_refused_begin_leaves_the_open_session_of_the_quantity_as_it_was(cylinder_case):
    """As fsi_spec_begin: a begin refused for a node out of range or for a history beyond the device keeps the history the
    caller had - its frames can be fetched and the next sample goes behind them."""
    from vasp_amd.capi import FsiError, HipBackend
    mesh, desc = cylinder_case[0]["mesh"], cylinder_case[1]
    V, N2 = mesh.num_vertices, mesh.num_nodes
    hb = HipBackend(desc)
    try:
        states = 1e-4 * np.random.default_rng(9).standard_normal((4, hb.ndof))
        hb.hi_pass_begin("v", np.arange(V), None, 8)
        for k in range(3):
            hb.set_state("n", states[k])
            hb.hi_pass_sample("v")
        third = states[2, 3 * N2:3 * N2 + 3 * V].reshape(V, 3)
        assert np.array_equal(hb.hi_pass_fetch("v", "raw", 2), third)
        with pytest.raises(FsiError, match="node out of range"):
            hb.hi_pass_begin("v", [N2], None, 8)
        total_b = hb.device_memory()[1]
        with pytest.raises(FsiError, match=r"needs \d+ bytes .* has \d+ bytes free"):
            hb.hi_pass_begin("v", np.arange(V), None, int(total_b // (8 * 3 * V)) + 1)      # the raw history alone exceeds the device
        assert np.array_equal(hb.hi_pass_fetch("v", "raw", 2), third)
        hb.set_state("n", states[3])
        hb.hi_pass_sample("v")
        assert np.array_equal(hb.hi_pass_fetch("v", "raw", 3), states[3, 3 * N2:3 * N2 + 3 * V].reshape(V, 3))
        assert np.array_equal(hb.hi_pass_fetch("v", "raw", 2), third)
    finally:
        hb.close()


def test_all_sessions_side_by_side_and_destroy_without_end(cylinder_case):
    from vasp_amd.capi import HipBackend
    from vasp_amd.hemodynamics import fluid_boundary_facets
    mesh, desc = cylinder_case[0]["mesh"], cylinder_case[1]
    hb = HipBackend(desc)
    free0 = hb.device_memory()[0]
    U = 1e-4 * np.random.default_rng(4).standard_normal(hb.ndof)
    hb.set_state("n", U)
    _, cells, local = fluid_boundary_facets(mesh, 1)
    hb.hemodynamics_begin(cells, local, 3.5e-3, 1e-3)
    solid = np.nonzero(np.asarray(desc["cell_kind"]) == 1)[0]
    hb.stress_strain_begin(solid)
    for q in "dvp":
        hb.hi_pass_begin(q, *hp.output_nodes(mesh, 2, q), capacity=50)
    alone = HipBackend(desc)
    try:
        alone.set_state("n", U)
        alone.stress_strain_begin(solid)
        ref_frame = alone.stress_strain_sample(frame=True)
    finally:
        alone.close()
    wss = hb.hemodynamics_sample(wss=True)
    frame = hb.stress_strain_sample(frame=True)
    for q in "dvp":
        hb.hi_pass_sample(q)
    assert np.isfinite(wss).all()
    for key in frame:
        assert np.array_equal(frame[key], ref_frame[key]), key                # the other sessions are untouched by the three
    N2 = mesh.num_nodes
    assert np.array_equal(hb.hi_pass_fetch("d", "raw", 0).ravel(), U[:3 * N2])
    assert np.array_equal(hb.hi_pass_fetch("v", "raw", 0).ravel(), U[3 * N2:6 * N2])
    e, p = mesh.edges, U[6 * N2:]
    assert np.array_equal(hb.hi_pass_fetch("p", "raw", 0).ravel(), np.concatenate([p, 0.5 * (p[e[:, 0]] + p[e[:, 1]])]))
    hb.close()                              # no *_end: fsi_destroy frees the five sessions
    again = HipBackend(desc)
    try:
        assert again.device_memory()[0] >= free0 - (1 << 26)
    finally:
        again.close()


# ---- end to end -------------------------------------------------------------------------------------------------------

HOOK_PROBLEM = '''
"""offset_stenosis with a hook that keeps the state of every saved frame."""
import numpy as _np
from vasp_amd.problems.offset_stenosis import *  # noqa: F401,F403
from vasp_amd.problems import offset_stenosis as _base

_states = []


def post_solve(**ns):
    upd = _base.post_solve(**ns)
    if ns["counter"] % int(ns["save_step"]) == 0:
        _states.append(_np.array(ns["dvp_"]["n"].vector(), dtype=_np.float64))
    return upd


def finished(results_folder, **ns):
    _np.save(str(results_folder) + "/hook_states.npy", _np.stack(_states))
'''


def _run(cwd, name, extra):
    (cwd / "hp_case.py").write_text(HOOK_PROBLEM)
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "vasp_amd.monolithic", "-p", "hp_case", "-dt", "0.001", "-T", "0.04", "--verbose", "False",
           "--folder", str(cwd / name), "--sub-folder", "1", "--save-step", "1", "--save-deg", "2", "--checkpoint-step", "1000",
           "--new-arguments", f"mesh_path={STENOSIS}", *extra]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=1500, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return cwd / name / "1", r.stdout.replace(str(cwd / name), "<folder>")


def _files(folder):
    """What a folder of results holds: the text files byte for byte, of an .h5 file every dataset (path, dtype, shape and
    bytes) - its object headers carry the time of writing, so two runs never give the same file bytes."""
    from vasp_amd.h5lite import Dataset, read_h5
    out = {}

    def walk(g, prefix):
        for k in g.keys():
            if isinstance(g[k], Dataset):
                a = np.asarray(g[k].data)
                out[prefix + k] = (str(a.dtype), a.shape, a.tobytes())
            else:
                walk(g[k], prefix + k + "/")

    for p in sorted(folder.iterdir()):
        if p.suffix == ".h5":
            walk(read_h5(p), p.name + ":/")
        else:
            out[p.name] = p.read_bytes()
    return out


def _vectors(path):
    from vasp_amd.h5lite import read_h5
    g = read_h5(path)["VisualisationVector"]
    return np.stack([np.asarray(g[str(k)].data) for k in range(len(g.keys()))])


def test_end_to_end_run_writes_the_restatement_of_its_own_states(tmp_path):
    """--hi-pass d v p --hi-pass-amplitude --hi-pass-window 8 on the small stenosis mesh, 41 saved frames, in fresh processes.
    The filtered files hold the host restatement of the hooked states cast to float32, exactly; the amplitude files hold
    the device's running-sum amplitudes, held to the reference's formula as in test_amplitudes_against_the_host_restatement
    (4 x the host's direct-versus-running spread, plus half a float32 ulp for the cast)."""
    from vasp_amd.mesh import FsiMesh
    flags = ["--hi-pass", "d", "v", "p", "--hi-pass-amplitude", "--hi-pass-window", "8"]
    res, log = _run(tmp_path, "with", flags)
    plain, log_plain = _run(tmp_path, "without", [])
    twice, _ = _run(tmp_path, "twice", flags)
    mesh = FsiMesh.read(STENOSIS)
    states = np.load(res / "hook_states.npy")
    n = len(states)
    assert n >= 40 and states.shape[1] == mesh.num_dofs
    out = res / "Visualization_hi_pass"
    assert "Hi-pass fields of %d frames (d, v, p)" % n in log
    prm = hp.design(1e-3, 25.0, 1000.0)
    for q, name in hp.VIZ_TYPE.items():
        x = _rows(mesh, states, q)
        assert np.array_equal(_vectors(res / "Visualization" / f"{name}.h5"), x)          # the hook saw what the writer wrote
        y = hp.filtfilt_rows(prm["b"], prm["a"], x, prm["zi"], prm["padlen"])
        got = _vectors(out / f"{name}_25_to_1000.h5")
        assert got.dtype == np.float32 and np.array_equal(got, y.astype(np.float32)), q
        direct, running = hp.windowed_rms_rows(y, 8), hp.windowed_rms_running(y, 8)
        spread = np.abs(direct - running).max()
        amp = _vectors(out / f"{name}_25_to_1000_amplitude.h5")
        err = np.abs(amp.astype(np.float64) - direct)
        print(f"{q}: amplitude files vs the reference formula {err.max():.3e}, host spread {spread:.3e}, max {direct.max():.3e}")
        assert amp.dtype == np.float32 and not np.isnan(amp).any() and (amp >= 0).all()
        assert (err <= 4 * spread + 0.5 * np.finfo(np.float32).eps * np.abs(direct)).all(), q
        table = np.loadtxt(out / f"{name}_25_to_1000.csv", delimiter=",")
        assert table.shape == (n, 13) and np.array_equal(table[:, 12], table[:, 12].astype(int))
        assert (out / f"{name}_25_to_1000.xdmf").read_text() == hp.xdmf_text(
            n, 1e-3, 0.0, 8 * mesh.num_cells, mesh.num_nodes, "Scalar" if q == "p" else "Vector", f"{name}_25_to_1000")
    # the run's own output is untouched by the flag: Visualization/ (text byte for byte, every dataset bit for bit) and every
    # line the problem printed
    assert not (plain / "Visualization_hi_pass").exists()
    viz = _files(res / "Visualization")
    assert len(viz) == 3 * (1 + 2 + n) and viz == _files(plain / "Visualization")
    assert np.array_equal(np.load(plain / "hook_states.npy"), states)

    def printed(text):
        keep = [re.sub(r" in [0-9.]+ s$", "", line) for line in text.splitlines() if not line.startswith("Hi-pass")]
        return [line for line in keep if "<folder>" not in line]

    assert any("Probe" in line or "probe" in line for line in printed(log))
    assert printed(log) == printed(log_plain)
    # a second identical run writes identical files
    again = _files(out)
    assert len(again) == 3 * (2 * (1 + 2 + n) + 1) and _files(twice / "Visualization_hi_pass") == again
