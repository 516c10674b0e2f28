"""The post-processing sessions through a checkpoint and --restart-folder, host side: the host twins' export / import, the
state under Checkpoint/sessions/, the driver with a stub backend (a run split by a stop and a restart writes the bytes of an
unsplit run), the manifest's rules, the refusals and the continued WSS / stress series.  Every comparison is bitwise."""
import contextlib
import io
import json
import shutil
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN
from vasp_amd import hi_pass as hp
from vasp_amd import spectrogram as sp

CYL = GOLDEN / "cylinder" / "cylinder.h5"
DT = 1e-3
FRAMES, SPLIT = 40, 17
REGION = ["--spectrogram-fsi-region", "0", "0", "0", "100"]
OPTIONS = ["--hi-pass", "v", "p", "--hi-pass-amplitude", "--hi-pass-window", "8", "--hi-pass-point-ids", "0", "5",
           "--spectrogram", "v", *REGION]
OUTPUTS = ("Visualization_hi_pass", "Visualization_separate_domain", "Spectrograms")


def _signal(ndof, frames=FRAMES, seed=11):
    """(frames, ndof): per dof a slow carrier, a tone three decades below it with its own frequency and phase, and noise
    (the input of tests/test_gpu_hi_pass.py)."""
    rng = np.random.default_rng(seed)
    f, ph = rng.uniform(40.0, 450.0, ndof), rng.uniform(0.0, 2 * np.pi, ndof)
    t = (1 + np.arange(frames))[:, None] * DT
    return 1e-3 * np.sin(2 * np.pi * 1.5 * t + ph) + 1e-6 * np.sin(2 * np.pi * f * t + 2 * ph) + 1e-9 * rng.standard_normal((frames, ndof))


# ---- the host twins ---------------------------------------------------------------------------------------------------

def _twins():
    return hp.HostBandSession(3, FRAMES), sp.HostSpecSession(21, FRAMES)


def _continued(make, x):
    """(whole, split): a session that recorded all of x, and one that imported the first SPLIT frames of another in two
    pieces and recorded the rest."""
    whole, first, split = make(), make(), make()
    for f in x:
        whole.sample(f)
    for f in x[:SPLIT]:
        first.sample(f)
    split.import_(first.export(0, 10))
    split.import_(first.export(10, SPLIT - 10))
    assert len(split.raw) == SPLIT
    for f in x[SPLIT:]:
        split.sample(f)
    return whole, split


def test_host_band_session_continues_from_exported_frames():
    x = _signal(21)
    whole, split = _continued(lambda: _twins()[0], x)
    prm = hp.design(DT, 25.0, 1000.0)
    assert prm["padlen"] == 33
    out = []
    for s in (whole, split):
        s.filter(prm["b"], prm["a"], prm["zi"], prm["padlen"])
        s.amplitude(8)
        out.append((np.stack([s.fetch("raw", k) for k in range(FRAMES)]), np.stack([s.fetch("filtered", k) for k in range(FRAMES)]),
                    np.stack([s.fetch("amplitude", k) for k in range(FRAMES)]), s.trace("raw", [0, 5]), s.trace("filtered", [6])))
    for a, b in zip(*out):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert np.array_equal(out[1][0].reshape(FRAMES, -1), x) and out[1][2].any()


def test_host_spec_session_continues_from_exported_frames():
    x = _signal(21)
    whole, split = _continued(lambda: _twins()[1], x)
    w = sp.window_values("blackmanharris", 16)
    for s in (whole, split):
        assert s.export(0, FRAMES).shape == (FRAMES, 21)
    assert np.array_equal(whole.export(0, FRAMES), split.export(0, FRAMES))
    assert np.array_equal(whole.spectrogram(16, 12, 32, w, "spectrum", 1 / DT), split.spectrogram(16, 12, 32, w, "spectrum", 1 / DT))
    wp = sp.window_values("blackmanharris", FRAMES)
    assert np.array_equal(whole.periodogram(wp, "spectrum", 1 / DT), split.periodogram(wp, "spectrum", 1 / DT))


def test_an_import_past_the_capacity_is_refused_and_appends_nothing():
    x = _signal(21)
    for s, name in zip(_twins(), ("hi-pass", "spectrogram")):
        for f in x[:30]:
            s.sample(f)
        with pytest.raises(RuntimeError, match=name + " import: 30 recorded frames \\+ 11 exceed the capacity of 40"):
            s.import_(x[:11].reshape((11,) + np.shape(s.raw[0])))
        assert len(s.raw) == 30
        s.import_(x[:10].reshape((10,) + np.shape(s.raw[0])))
        assert len(s.raw) == 40
        with pytest.raises(RuntimeError, match="export"):
            s.export(35, 6)


# ---- the driver with a stub backend -----------------------------------------------------------------------------------

class _Stub:
    """Host stand-in for HipBackend without device sessions.  The state of step k (the k-th step of the whole run: ``start``
    steps were taken before a restart) is a function of k alone; at step ``kill_at`` it drops ``killturtle``."""
    start, kill_at, kill_path = 0, -1, None

    def __init__(self, desc):
        self.n = 6 * int(desc["num_nodes"]) + len(desc["coords"])
        rng = np.random.default_rng(5)
        self.f, self.ph, self.mean = rng.uniform(40.0, 400.0, self.n), rng.uniform(0, 6.28, self.n), rng.uniform(-1, 1, self.n)
        self.U = np.zeros(self.n)
        self.steps = 0

    def set_dirichlet_values(self, v): pass
    def set_interface_pressure(self, P): pass
    def shift(self): pass
    def set_state(self, which, x): self.U[:] = x

    def newton_solve(self, **kw):
        self.steps += 1
        k = self.start + self.steps
        t = DT * k
        self.U = 1e-3 * self.mean + 1e-3 * np.sin(2 * np.pi * 1.5 * t + self.ph) + 1e-6 * np.sin(2 * np.pi * self.f * t + self.ph)
        if k == self.kill_at:
            Path(self.kill_path).write_text("")
        return [(1e-8, 1e-9, False, 2, 1e-9)]

    def get_state(self, which, out=None):
        out[:] = self.U
        return out


def _run(folder, extra=(), T="0.039", save_deg="2", options=OPTIONS, **stub):
    """One run in <folder>/1, or with ``--restart-folder`` in ``extra`` its continuation; the results folder's parent names
    the spectrogram files, so every case here lives in a folder called ``case``."""
    from vasp_amd import monolithic
    lines = []
    with contextlib.redirect_stdout(io.StringIO()):
        ns = monolithic.run(["-p", "cylinder", "-dt", "0.001", "-T", T, "--theta", "0.51", "--folder", str(folder), "--sub-folder", "1",
                             "--save-step", "1", "--save-deg", save_deg, "--checkpoint-step", "5", "--verbose", "False", *options, *extra,
                             "--new-arguments", f"mesh_path={CYL}"], backend_factory=type("_Stub", (_Stub,), stub), out=lines.append)
    return ns, lines


def _restart(results, extra=(), **kw):
    return _run(results.parent, ["--restart-folder", str(results), *extra], start=SPLIT, **kw)


def _outputs(results):
    return {str(p.relative_to(results)): p.read_bytes() for sub in OUTPUTS if (results / sub).exists()
            for p in sorted((results / sub).rglob("*")) if p.is_file()}


@pytest.fixture(scope="module", autouse=True)
def one_modification_time():
    """h5lite stamps every dataset header with the time it is written (as libhdf5 does); with the clock held, files written
    from the same data are the same bytes whenever they are written."""
    import types
    from vasp_amd import h5lite
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(h5lite, "time", types.SimpleNamespace(time=lambda: 1.7e9))
        yield


@pytest.fixture(scope="module")
def runs(tmp_path_factory, one_modification_time):
    """(whole, half): the outputs of an unsplit run of 40 frames, and the results folder of the same run stopped by
    killturtle after 17 steps."""
    base = tmp_path_factory.mktemp("restart")
    _run(base / "whole" / "case")
    half = base / "half" / "case" / "1"
    half.mkdir(parents=True)
    ns, lines = _run(half.parent, kill_at=SPLIT, kill_path=half / "killturtle")
    assert ns["backend"].steps == SPLIT and any("killturtle found" in line for line in lines)
    return _outputs(base / "whole" / "case" / "1"), half


def _copy(half, tmp_path):
    results = tmp_path / "case" / "1"
    shutil.copytree(half, results)
    return results


def test_a_stopped_run_leaves_its_session_state_beside_the_checkpoint(runs):
    _, half = runs
    folder = half / "Checkpoint" / "sessions"
    manifest = json.loads((folder / "sessions.json").read_text())
    meta = json.loads((half / "Checkpoint" / "default_variables.json").read_text())
    assert manifest["counter"] == meta["counter"] == SPLIT - 1 and manifest["t"] == meta["t"]
    assert sorted(manifest["sessions"]) == ["hi_pass", "spectrogram"]
    band = manifest["sessions"]["hi_pass"]
    assert band["frames"] == SPLIT and len(band["times"]) == SPLIT and sorted(band["quantities"]) == ["p", "v"]
    assert band["times"][0] == 1e-3 and (np.diff(band["times"]) > 0).all() and band["times"][-1] == meta["t"]
    assert band["times"] == manifest["sessions"]["spectrogram"]["times"]
    for q, fp in band["quantities"].items():
        assert fp["save_deg"] == 2 and fp["dt_sample"] == 1e-3 and len(fp["nodes"]) == 64
        assert (folder / f"hi_pass_{q}.f64").stat().st_size == 8 * fp["rows"] * SPLIT
    spec = manifest["sessions"]["spectrogram"]
    assert spec["quantities"]["v"]["component"] == "all" and spec["quantities"]["v"]["rows"] == 3000
    assert (folder / "spectrogram_v.f64").stat().st_size == 8 * 3000 * SPLIT
    assert not list(folder.glob("tmp_*"))
    # checkpoints at counters 0, 5, 10, 15 and at the stop: every save appended the frames since the last one - the file is the
    # history in order
    x = np.fromfile(folder / "hi_pass_p.f64", dtype="<f8").reshape(SPLIT, -1)
    from vasp_amd.h5lite import read_h5
    g = read_h5(half / "Visualization" / "pressure.h5")["VisualisationVector"]
    assert np.array_equal(x, np.stack([np.asarray(g[str(k)].data).reshape(-1) for k in range(SPLIT)]))


def test_a_split_run_writes_the_bytes_of_an_unsplit_run(runs, tmp_path):
    whole, half = runs
    results = _copy(half, tmp_path)
    stopped = _outputs(results)
    assert set(stopped) < set(whole)                  # 17 frames: the traces only, no filter has enough of them
    ns, lines = _restart(results)
    assert ns["backend"].steps == FRAMES - SPLIT
    assert any("Hi-pass fields of 40 frames (v, p)" in line for line in lines) and any("Spectrograms of 40 frames" in line for line in lines)
    split = _outputs(results)
    assert sorted(split) == sorted(whole) and len(whole) == 2 * 5 + 4 + 4
    for name in whole:
        assert split[name] == whole[name], name
    manifest = json.loads((results / "Checkpoint" / "sessions" / "sessions.json").read_text())
    # the last checkpoint step: counter 35 was the 20th step of the restarted run
    assert manifest["sessions"]["hi_pass"]["frames"] == SPLIT + 20 and manifest["counter"] == 35
    assert (results / "Visualization" / "velocity_run_1.h5").exists()


def test_a_manifest_of_another_checkpoint_is_refused(runs, tmp_path):
    results = _copy(runs[1], tmp_path)
    path = results / "Checkpoint" / "sessions" / "sessions.json"
    manifest = json.loads(path.read_text())
    manifest["counter"] = 10
    path.write_text(json.dumps(manifest))
    with pytest.raises(SystemExit, match=r"belongs to counter = 10,.* the checkpoint beside it to counter = 16"):
        _restart(results)
    assert not (results / "Visualization" / "velocity_run_1.h5").exists()      # before the first step


@pytest.mark.parametrize("extra,save_deg,field", [(["--spectrogram-seed", "3"], "2", "nodes"), ([], "1", "save_deg")])
def test_a_state_recorded_otherwise_is_refused_with_the_field(runs, tmp_path, extra, save_deg, field):
    results = _copy(runs[1], tmp_path)
    with pytest.raises(SystemExit, match=r"recorded otherwise than this run would record, it differs in .*%s \(saved " % field):
        _restart(results, extra, save_deg=save_deg)


def test_a_history_shorter_than_the_manifest_says_is_refused(runs, tmp_path):
    results = _copy(runs[1], tmp_path)
    path = results / "Checkpoint" / "sessions" / "hi_pass_v.f64"
    size = path.stat().st_size
    with open(path, "r+b") as f:
        f.truncate(size - 8)
    with pytest.raises(SystemExit, match=rf"hi_pass_v.f64 holds {size - 8} bytes, the 17 frames of 7500 rows .* need {size}"):
        _restart(results)


def test_a_stale_tail_behind_the_manifests_frames_is_ignored(runs, tmp_path):
    whole, half = runs
    results = _copy(half, tmp_path)
    for name in ("hi_pass_v.f64", "hi_pass_p.f64", "spectrogram_v.f64"):
        with open(results / "Checkpoint" / "sessions" / name, "ab") as f:
            f.write(np.full(12345, 7.0).tobytes())
    _restart(results)
    split = _outputs(results)
    assert sorted(split) == sorted(whole) and all(split[name] == whole[name] for name in whole)
    fp = json.loads((results / "Checkpoint" / "sessions" / "sessions.json").read_text())["sessions"]["hi_pass"]
    assert (results / "Checkpoint" / "sessions" / "hi_pass_v.f64").stat().st_size == 8 * 7500 * fp["frames"]     # the tail is gone


def test_a_quantity_added_at_the_restart_is_refused(runs, tmp_path):
    results = _copy(runs[1], tmp_path)
    with pytest.raises(SystemExit, match="--hi-pass d: .* recorded v p; a quantity added at a restart has no past"):
        _restart(results, options=["--hi-pass", "d", "v", "p", "--hi-pass-point-ids", "0", "5"])
    # a saved session that is not asked for is left alone, and one asked for alone continues
    before = (results / "Checkpoint" / "sessions" / "spectrogram_v.f64").read_bytes()
    ns, lines = _restart(results, options=["--hi-pass", "p", "--hi-pass-bands", "0", "200"])
    assert any("Hi-pass fields of 40 frames (p)" in line for line in lines)
    assert (results / "Checkpoint" / "sessions" / "spectrogram_v.f64").read_bytes() == before
    assert not (results / "Spectrograms").exists()


# ---- refusals ---------------------------------------------------------------------------------------------------------

def _parameters(extra):
    from vasp_amd.monolithic import parameters
    with contextlib.redirect_stdout(io.StringIO()):
        return parameters(["-p", "cylinder", "--verbose", "False", "-dt", "0.001", "-T", "0.039", "--save-step", "1", *REGION, *extra])[2]


def _refusals():
    from vasp_amd.hemodynamics import hemodynamics_refusal
    from vasp_amd.stress_strain import stress_strain_refusal
    return (("hemodynamics", ["--hemodynamics"], hemodynamics_refusal, "--restart-folder"),
            ("stress_strain", ["--stress-strain"], stress_strain_refusal, "--restart-folder"),
            ("hi_pass", ["--hi-pass", "v"], hp.hi_pass_refusal, "cannot be used with --restart-folder"),
            ("spectrogram", ["--spectrogram", "v"], sp.spectrogram_refusal, "cannot be used with --restart-folder"))


def test_without_saved_state_every_option_is_refused_with_the_path_it_looked_for(tmp_path):
    for key, option, refusal, words in _refusals():
        msg = refusal(_parameters(option + ["--restart-folder", str(tmp_path)]), 1, None)
        assert words in msg and "saved no state for the option" in msg, key
        assert str(tmp_path / "Checkpoint" / "sessions" / "sessions.json") in msg, key
    # a manifest without the option's entry: the same refusal
    folder = tmp_path / "Checkpoint" / "sessions"
    folder.mkdir(parents=True)
    (folder / "sessions.json").write_text(json.dumps(dict(t=0.017, counter=16, sessions={})))
    for key, option, refusal, words in _refusals():
        msg = refusal(_parameters(option + ["--restart-folder", str(tmp_path)]), 1, None)
        assert words in msg and f"an entry {key!r}" in msg, key


def test_with_saved_state_no_option_is_refused(tmp_path):
    folder = tmp_path / "Checkpoint" / "sessions"
    folder.mkdir(parents=True)
    times = [1e-3 * (k + 1) for k in range(SPLIT)]
    entry = dict(frames=SPLIT, samples=SPLIT, times=times, quantities={}, fingerprint={})
    (folder / "sessions.json").write_text(json.dumps(dict(t=times[-1], counter=16, sessions={key: entry for key, *_ in _refusals()})))
    (tmp_path / "Checkpoint" / "default_variables.json").write_text(json.dumps(dict(t=times[-1], counter=16)))
    for key, option, refusal, _ in _refusals():
        assert refusal(_parameters(option + ["--restart-folder", str(tmp_path)]), 1, None) == "", key
    # the other refusals stay: more than one rank, no --save-step
    for key, option, refusal, _ in _refusals():
        assert "one rank only" in refusal(_parameters(option + ["--restart-folder", str(tmp_path)]), 2, None), key
    with pytest.raises(SystemExit, match="d, v and / or p"):
        hp.quantities({"hi_pass": ["strain"]})
    # the frame counts are those of the saved frames and the frames to come: 17 + 13 with -T 0.0295
    v = _parameters(["--hi-pass", "v", "--restart-folder", str(tmp_path), "-T", "0.0295"])
    assert hp.frame_times(v, "hi_pass", "")[1] == SPLIT and len(hp.frame_times(v, "hi_pass", "")[0]) == 30
    msg = hp.hi_pass_refusal(v, 1, None)
    assert "saves 30 frames (17 saved before the restart and 13 to come)" in msg and "padlen + 1 = 34" in msg
    assert hp.hi_pass_refusal(dict(v, hi_pass_bands=[0, 200]), 1, None) == ""            # low-pass: 19
    msg = hp.hi_pass_refusal(dict(v, T=0.039, hi_pass_amplitude=True), 1, None)
    assert "saves 40 frames (17 saved before the restart and 23 to come), fewer than the window of 250" in msg
    v = _parameters(["--spectrogram", "v", "--restart-folder", str(tmp_path), "-T", "0.0205"])
    msg = sp.spectrogram_refusal(v, 1, None)
    assert "saves 21 frames (17 saved before the restart and 4 to come)" in msg and "padlen + 1 = 22" in msg
    assert sp.spectrogram_refusal(dict(v, T=0.039), 1, None) == ""
    # 30 frames in 3 windows: segments of 16 frames, without overlap one whole segment... and a second: 30 // 16 = 1
    assert "at least two" in sp.spectrogram_refusal(dict(v, T=0.0295, spectrogram_overlap_frac=0.0), 1, None)


def test_a_restart_with_too_few_frames_in_all_is_refused_before_the_first_step(runs, tmp_path):
    results = _copy(runs[1], tmp_path)
    with pytest.raises(SystemExit, match=r"saves 30 frames \(17 saved before the restart and 13 to come\).*padlen \+ 1 = 34"):
        _restart(results, T="0.0295")
    assert not (results / "Visualization" / "velocity_run_1.h5").exists()


# ---- the series that are appended during the run ----------------------------------------------------------------------

def _series_files(folder, name):
    from vasp_amd.h5lite import read_h5
    return {p.name: read_h5(p)[name] for p in sorted(folder.glob(f"{name}*.h5"))}


def _check_series(folder, name, frames, times):
    """7 frames behind one XDMF: 0 .. 2 in <name>.h5, 3 .. 6 in <name>_run_1.h5, each file's first group with the dof map.
    <name>.h5 keeps the group a run wrote after its last checkpoint; the XDMF no longer lists it."""
    from vasp_amd.hemodynamics import xdmf_frames
    files = _series_files(folder, name)
    assert sorted(files) == [f"{name}.h5", f"{name}_run_1.h5"]
    listed = xdmf_frames(folder / f"{name}.xdmf")
    assert [t for t, _, _ in listed] == times and [k for _, _, k in listed] == list(range(7))
    assert [f for _, f, _ in listed] == [f"{name}.h5"] * 3 + [f"{name}_run_1.h5"] * 4
    for (t, f, k), frame in zip(listed, frames):
        assert np.array_equal(np.asarray(files[f][f"{name}_{k}"]["vector"].data).reshape(-1), np.asarray(frame).reshape(-1)), (name, k)
    for f, first in ((f"{name}.h5", 0), (f"{name}_run_1.h5", 3)):
        assert sorted(files[f].keys()) == sorted(f"{name}_{k}" for k in (range(4) if first == 0 else range(3, 7)))
        g = files[f][f"{name}_{first}"]
        assert {"cell_dofs", "x_cell_dofs", "cells", "mesh"} <= set(g.keys())
        assert "cell_dofs" not in files[f][f"{name}_{first + 1}"].keys()
    text = (folder / f"{name}.xdmf").read_text()
    assert text.count("<Grid Name=") == 7 and text.count(f"{name}_run_1.h5:{name}/{name}_3/mesh/topology") == 4
    assert text.count(f"{name}.h5:{name}/{name}_0/cell_dofs") == 3


def test_wss_and_stress_series_continue_in_a_new_file_behind_the_same_xdmf(tmp_path):
    from vasp_amd.hemodynamics import HemodynamicsWriter
    from vasp_amd.stress_strain import COMPONENTS, FRAME_NAMES, StressStrainWriter
    rng = np.random.default_rng(2)
    times = [1e-3 * (k + 1) for k in range(7)]
    geometry = rng.standard_normal((5, 3))
    tri, tet = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4]]), np.array([[0, 1, 2, 3], [1, 2, 3, 4]])
    tau = rng.standard_normal((8, 3, 3, 3))
    frames = [dict(TrueStress=rng.standard_normal((2, 4, 3, 3)), GreenLagrangeStrain=rng.standard_normal((2, 4, 3, 3)),
                   MaxPrincipalStress=rng.standard_normal((2, 4)), MaxPrincipalStrain=rng.standard_normal((2, 4))) for _ in range(8)]
    # the first run writes one frame more than its last checkpoint saw: the restart cuts it
    hw, sw = HemodynamicsWriter(tmp_path / "h", geometry, tri), StressStrainWriter(tmp_path / "s", geometry, tet)
    for k in (0, 1, 2, 7):
        hw.write_wss(tau[k], 9.0 if k == 7 else times[k])
        sw.write_frame(frames[k], 9.0 if k == 7 else times[k])
    hw.close(), sw.close()
    hw, sw = HemodynamicsWriter(tmp_path / "h", geometry, tri, adopt=3), StressStrainWriter(tmp_path / "s", geometry, tet, adopt=3)
    assert hw.frames == sw.frames == 3
    for k in range(3, 7):
        hw.write_wss(tau[k], times[k])
        sw.write_frame(frames[k], times[k])
    hw.close(), sw.close()
    assert hw.frames == sw.frames == 7
    _check_series(tmp_path / "h", "WSS", tau[:7], times)
    for name in FRAME_NAMES:
        _check_series(tmp_path / "s", name, [f[name] for f in frames[:7]], times)
        assert f'AttributeType="{"Tensor" if COMPONENTS[name] == 9 else "Scalar"}"' in (tmp_path / "s" / f"{name}.xdmf").read_text()
    with pytest.raises(SystemExit, match="lists 7 frames, the saved session state continues a series of 9"):
        HemodynamicsWriter(tmp_path / "h", geometry, tri, adopt=9)
