"""The post-processing sessions through a checkpoint and a restart, on the device (fsi_*_export / fsi_*_import,
HipBackend.*_export / *_import, ``--restart-folder`` with the four options): a session that imports what another exported and
samples the rest holds the bits of one that sampled everything.  Every comparison is bitwise."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, prepare_case
from vasp_amd import hi_pass as hp
from vasp_amd import spectrogram as sp

pytestmark = pytest.mark.gpu

FRAMES, SPLIT = 40, 17
DT = 1e-3
WINDOW = 8
CYL = GOLDEN / "cylinder" / "cylinder.h5"


def _signal(ndof, frames=FRAMES, seed=11):
    """(frames, ndof): per dof a slow carrier, a tone three decades below it with its own frequency and phase, and noise
    (the input of tests/test_gpu_hi_pass.py)."""
    rng = np.random.default_rng(seed)
    f, ph = rng.uniform(40.0, 450.0, ndof), rng.uniform(0.0, 2 * np.pi, ndof)
    t = (1 + np.arange(frames))[:, None] * DT
    return 1e-3 * np.sin(2 * np.pi * 1.5 * t + ph) + 1e-6 * np.sin(2 * np.pi * f * t + 2 * ph) + 1e-9 * rng.standard_normal((frames, ndof))


@contextlib.contextmanager
def _context(desc):
    from vasp_amd.capi import HipBackend
    hb = HipBackend(desc)
    try:
        yield hb
    finally:
        hb.close()


# ---- hemodynamics, stress and strain ----------------------------------------------------------------------------------

def test_hemodynamic_sums_and_tau_prev_are_carried(cylinder_case):
    """Six states: context A samples them all; B samples three, exports and is closed; C imports and samples the other three.
    The indices of A and C are the same bits, NaN pattern included.  TWSSG's first term in C is |(tau_4 - tau_3) / dt| only
    with the tau_prev that was carried: with tau_prev zeroed in the imported accumulator it differs."""
    from vasp_amd.capi import FsiError
    from vasp_amd.hemodynamics import INDEX_NAMES, fluid_boundary_facets
    mesh, desc = cylinder_case[0]["mesh"], cylinder_case[1]
    _, cell, local = fluid_boundary_facets(mesh, 1)
    nf, N2 = len(cell), mesh.num_nodes
    rng = np.random.default_rng(3)
    states = np.zeros((6, mesh.num_dofs))
    states[:, 3 * N2:6 * N2] = 0.3 * rng.standard_normal((6, 3 * N2)) + rng.standard_normal(3 * N2)
    with _context(desc) as a:
        a.hemodynamics_begin(cell, local, 3.5e-3, DT)
        for x in states:
            a.set_state("n", x)
            a.hemodynamics_sample()
        whole = a.hemodynamics_indices()
    with _context(desc) as b:
        b.hemodynamics_begin(cell, local, 3.5e-3, DT)
        acc0, n0 = b.hemodynamics_export()
        assert n0 == 0 and acc0.shape == (24 * nf,) and not acc0.any()
        for x in states[:3]:
            b.set_state("n", x)
            tau = b.hemodynamics_sample(wss=True)
        acc, samples = b.hemodynamics_export()
        assert samples == 3
        # the layout the header documents: sum_tau[nd][3], tau_prev[nd][3], sum_mag[nd], sum_twssg[nd] with nd = 3 nf
        nd = 3 * nf
        assert np.array_equal(acc[3 * nd:6 * nd].reshape(nf, 3, 3), tau) and (acc[6 * nd:7 * nd] >= 0).all() and acc[7 * nd:].any()
        assert np.array_equal(b.hemodynamics_export()[0], acc)               # an export changes nothing
        b.hemodynamics_end()
    with _context(desc) as c:
        c.hemodynamics_begin(cell, local, 3.5e-3, DT)
        c.hemodynamics_import(acc, samples)
        for x in states[3:]:
            c.set_state("n", x)
            c.hemodynamics_sample()
        split = c.hemodynamics_indices()
        assert split["samples"] == whole["samples"] == 6
        for name in INDEX_NAMES:
            assert np.array_equal(split[name], whole[name], equal_nan=True), name
            assert np.array_equal(np.isnan(split[name]), np.isnan(whole[name])), name
        assert np.isfinite(whole["TWSSG"]).any()
        # without the carried tau_prev TWSSG is another number
        lost = acc.copy()
        lost[3 * nd:6 * nd] = 0.0
        c.hemodynamics_begin(cell, local, 3.5e-3, DT)
        c.hemodynamics_import(lost, samples)
        for x in states[3:]:
            c.set_state("n", x)
            c.hemodynamics_sample()
        other = c.hemodynamics_indices()
        assert np.array_equal(other["TAWSS"], whole["TAWSS"]) and not np.array_equal(other["TWSSG"], whole["TWSSG"], equal_nan=True)
        # refusals leave the session as it was: an accumulator of another number of facets, a negative count, no session
        c.hemodynamics_begin(cell[:-1], local[:-1], 3.5e-3, DT)
        with pytest.raises(FsiError, match="the open session has %d" % (24 * (nf - 1))):
            c.hemodynamics_import(acc, samples)
        with pytest.raises(FsiError, match="samples >= 0"):
            c.hemodynamics_import(acc[:24 * (nf - 1)], -1)
        assert c.hemodynamics_export()[1] == 0 and not c.hemodynamics_export()[0].any()
        c.hemodynamics_end()
        with pytest.raises(FsiError, match="fsi_hemo_begin first"):
            c.hemodynamics_export()
        with pytest.raises(FsiError, match="fsi_hemo_begin first"):
            c._check(c.lib.fsi_hemo_import(c.ctx, acc.ctypes.data, 1))


def test_stress_sums_are_carried(cylinder_case):
    from vasp_amd.capi import FsiError
    from vasp_amd.stress_strain import solid_cells
    mesh, desc = cylinder_case[0]["mesh"], cylinder_case[1]
    cells = solid_cells(mesh, 2)
    N2 = mesh.num_nodes
    rng = np.random.default_rng(4)
    states = np.zeros((6, mesh.num_dofs))
    states[:, :3 * N2] = 0.02 * mesh.hmin() * rng.standard_normal((6, 3 * N2))
    with _context(desc) as a:
        a.stress_strain_begin(cells)
        for x in states:
            a.set_state("n", x)
            a.stress_strain_sample()
        whole = a.stress_strain_averages()
    with _context(desc) as b:
        b.stress_strain_begin(cells)
        for x in states[:3]:
            b.set_state("n", x)
            frame = b.stress_strain_sample(frame=True)
        sums, samples = b.stress_strain_export()
        assert samples == 3 and sums.shape == (len(cells), 8) and sums.any()
        b.stress_strain_end()
    with _context(desc) as c:
        c.stress_strain_begin(cells)
        c.stress_strain_import(sums, samples)
        for x in states[3:]:
            c.set_state("n", x)
            c.stress_strain_sample()
        split = c.stress_strain_averages()
        assert split["samples"] == whole["samples"] == 6
        for name in ("MaxPrincipalStress_avg", "MaxPrincipalStrain_avg"):
            assert np.array_equal(split[name], whole[name]) and whole[name].any(), name
        c.stress_strain_begin(cells[:-2])
        with pytest.raises(FsiError, match="the open session has %d" % (8 * (len(cells) - 2))):
            c.stress_strain_import(sums, samples)
        assert c.stress_strain_export()[1] == 0
        c.stress_strain_end()
        with pytest.raises(FsiError, match="fsi_stress_begin first"):
            c.stress_strain_export()
    assert frame["MaxPrincipalStress"].shape == (len(cells), 4)


# ---- band-pass and spectrogram histories ------------------------------------------------------------------------------

def _band_results(hb, q):
    """Everything a band-pass session answers with on its 40 frames: raw, band-pass and low-pass filtered frames, the
    amplitudes with their maximum and argmax, a raw and a filtered trace."""
    out = {"raw": np.stack([hb.hi_pass_fetch(q, "raw", k) for k in range(FRAMES)])}
    for name, band in (("bandpass", (25.0, 1000.0)), ("lowpass", (0.0, 200.0))):
        prm = hp.design(DT, *band)
        hb.hi_pass_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
        out[name] = np.stack([hb.hi_pass_fetch(q, "filtered", k) for k in range(FRAMES)])
        hb.hi_pass_amplitude(q, WINDOW if name == "bandpass" else 0)
        amp = [hb.hi_pass_fetch(q, "amplitude", k, with_max=True) for k in range(FRAMES)]
        out[name + " amplitude"] = np.stack([a for a, _, _ in amp])
        out[name + " max"] = np.array([m for _, m, _ in amp])
        out[name + " argmax"] = np.array([i for _, _, i in amp])
        out[name + " trace"] = hb.hi_pass_trace(q, "filtered", [0, 5, 11])
    out["trace"] = hb.hi_pass_trace(q, "raw", [0, 5, 11])
    return out


def test_band_pass_history_continues_from_exported_frames(stenosis_case):
    """d, v and p on the save_deg 2 rows of the small stenosis mesh (the p rows of the edge nodes are two-node means), 40
    frames, split at 17 with the export in two pieces."""
    from vasp_amd.capi import FsiError
    mesh, desc = stenosis_case[0]["mesh"], stenosis_case[1]
    with _context(desc) as a, _context(desc) as b:
        states = _signal(a.ndof)
        for hb in (a, b):
            for q in "dvp":
                hb.hi_pass_begin(q, *hp.output_nodes(mesh, 2, q), capacity=FRAMES)
        for k in range(FRAMES):
            a.set_state("n", states[k])
            for q in "dvp":
                a.hi_pass_sample(q)
        pieces = {}
        with _context(desc) as first:
            for q in "dvp":
                first.hi_pass_begin(q, *hp.output_nodes(mesh, 2, q), capacity=SPLIT)
            for k in range(SPLIT):
                first.set_state("n", states[k])
                for q in "dvp":
                    first.hi_pass_sample(q)
            for q in "dvp":
                first.hi_pass_select(q, 3, 4, 2)                            # an export takes absolute indices whatever is selected
                pieces[q] = (first.hi_pass_export(q, 0, 10), first.hi_pass_export(q, 10, SPLIT - 10))
                with pytest.raises(FsiError, match="first \\+ count <= the 17 recorded frames"):
                    first.hi_pass_export(q, 10, SPLIT - 9)
                with pytest.raises(FsiError, match="count >= 1"):
                    first.hi_pass_export(q, 0, 0)
        for q in "dvp":
            n, ncomp = len(hp.output_nodes(mesh, 2, q)[0]), 1 if q == "p" else 3
            assert pieces[q][0].shape == (10, n, ncomp) and pieces[q][1].shape == (SPLIT - 10, n, ncomp)
            for piece in pieces[q]:
                b.hi_pass_import(q, piece)
        for k in range(SPLIT, FRAMES):
            b.set_state("n", states[k])
            for q in "dvp":
                b.hi_pass_sample(q)
        for q in "dvp":
            whole, split = _band_results(a, q), _band_results(b, q)
            assert whole["bandpass amplitude"].any() and whole["raw"][SPLIT - 1].any()
            for key in whole:
                assert whole[key].shape == split[key].shape and np.array_equal(whole[key], split[key]), (q, key)
        # the history is full: an import is refused and the session answers as before; so is one of another row count
        before = _band_results(b, "p")
        with pytest.raises(FsiError, match="40 recorded frames \\+ 1 exceed the capacity of 40"):
            b.hi_pass_import("p", pieces["p"][0][:1])
        with pytest.raises(FsiError, match="the open session has frames of"):
            b.hi_pass_import("p", pieces["v"][0][:1])
        after = _band_results(b, "p")
        assert all(np.array_equal(before[key], after[key]) for key in before)
        b.hi_pass_end("d")
        with pytest.raises(FsiError, match="fsi_band_begin first"):
            b._check(b.lib.fsi_band_import(b.ctx, 0, 1, pieces["d"][0].ctypes.data))


@pytest.mark.parametrize("component", ["all", "mag"])
def test_spectrogram_history_continues_from_exported_frames(stenosis_case, component):
    from vasp_amd.capi import FsiError
    mesh, desc = stenosis_case[0]["mesh"], stenosis_case[1]
    nodes = np.random.default_rng(1).choice(mesh.num_nodes, 300)              # drawn with replacement, as the driver draws
    K, NOV, NFFT = 16, 12, 32
    w, wp = sp.window_values("blackmanharris", K), sp.window_values("blackmanharris", FRAMES)
    hpf = sp.highpass_design(1 / DT, 25.0)
    with _context(desc) as a, _context(desc) as b:
        states = _signal(a.ndof)
        a.spec_begin("v", nodes, None, component, capacity=FRAMES)
        b.spec_begin("v", nodes, None, component, capacity=FRAMES)
        for k in range(FRAMES):
            a.set_state("n", states[k])
            a.spec_sample("v")
        with _context(desc) as first:
            first.spec_begin("v", nodes, None, component, capacity=SPLIT)
            for k in range(SPLIT):
                first.set_state("n", states[k])
                first.spec_sample("v")
            pieces = first.spec_export("v", 0, 10), first.spec_export("v", 10, SPLIT - 10)
        rows = len(nodes) * (3 if component == "all" else 1)
        assert pieces[0].shape == (10, rows) and pieces[1].shape == (SPLIT - 10, rows)
        if component == "mag":                                                  # the rows are what was recorded: the magnitudes
            v = states[:10, 3 * mesh.num_nodes:6 * mesh.num_nodes].reshape(10, -1, 3)[:, nodes]
            assert np.array_equal(pieces[0], np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]))
        for piece in pieces:
            b.spec_import("v", piece)
        for k in range(SPLIT, FRAMES):
            b.set_state("n", states[k])
            b.spec_sample("v")
        for hb in (a, b):
            assert np.array_equal(hb.spec_export("v", 0, FRAMES), np.stack([hb.spec_fetch("v", k) for k in range(FRAMES)]))
        assert np.array_equal(a.spec_export("v", 0, FRAMES), b.spec_export("v", 0, FRAMES))
        for filtered in (False, True):
            for hb in (a, b):
                hb.spec_filter("v", hpf["b"], hpf["a"], hpf["zi"], hpf["padlen"]) if filtered else hb.spec_filter("v")
            P = [hb.spec_spectrogram("v", K, NOV, NFFT, w, "spectrum", 1 / DT) for hb in (a, b)]
            psd = [hb.spec_periodogram("v", wp, "spectrum", 1 / DT) for hb in (a, b)]
            assert P[0].shape == (NFFT // 2 + 1, 7) and P[0].any() and np.array_equal(P[0], P[1]), filtered
            assert psd[0].any() and np.array_equal(psd[0], psd[1]), filtered
        # importing selects the raw series, as recording a frame does; past the capacity it is refused
        with pytest.raises(FsiError, match="exceed the capacity of 40"):
            b.spec_import("v", pieces[0][:1])
        assert np.array_equal(b.spec_periodogram("v", wp, "spectrum", 1 / DT), psd[1])       # still the filtered series
        b.spec_begin("v", nodes, None, component, capacity=FRAMES)
        b.spec_import("v", pieces[0])
        b.spec_filter("v", hpf["b"], hpf["a"], hpf["zi"], 3)                      # the filtered series is selected ...
        b.spec_import("v", pieces[1][:2])                                       # ... until frames arrive
        after_import = b.spec_periodogram("v", np.ones(12), "spectrum", 1 / DT)
        b.spec_filter("v")
        assert np.array_equal(after_import, b.spec_periodogram("v", np.ones(12), "spectrum", 1 / DT))
        b.spec_filter("v", hpf["b"], hpf["a"], hpf["zi"], 3)
        assert not np.array_equal(after_import, b.spec_periodogram("v", np.ones(12), "spectrum", 1 / DT))


# ---- end to end -------------------------------------------------------------------------------------------------------

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

E2E = dict(hemodynamics=True, stress_strain=True, hi_pass=["d", "v", "p"], hi_pass_bands=[0, 200], hi_pass_amplitude=True,
           hi_pass_window=8, hi_pass_point_ids=[0, 5], spectrogram=["v"], spectrogram_fsi_region=[0, 0, 0, 100])
E2E_ARGV = ["--hemodynamics", "--stress-strain", "--hi-pass", "d", "v", "p", "--hi-pass-bands", "0", "200", "--hi-pass-amplitude",
            "--hi-pass-window", "8", "--hi-pass-point-ids", "0", "5", "--spectrogram", "v", "--spectrogram-fsi-region", "0", "0", "0", "100"]


def _child(cwd, extra, limit=300):
    """One run of the driver in a fresh child process under its own time limit."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "vasp_amd.monolithic", "-p", "restart_case", "-dt", "0.001", "-T", "0.0235",
           "--theta", "0.51", "--verbose", "False", "--save-step", "1", "--save-deg", "2", "--checkpoint-step", "5", *E2E_ARGV, *extra,
           "--new-arguments", f"mesh_path={CYL}"]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _datasets(path):
    """Every dataset of an .h5 file as path -> (dtype, shape, bytes): its object headers carry the time of writing."""
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


def _series(folder, name):
    """The frames of a DG1 series in the XDMF's order, each from the file the XDMF names: (times, vectors)."""
    from vasp_amd.h5lite import read_h5
    from vasp_amd.hemodynamics import xdmf_frames
    listed = xdmf_frames(folder / f"{name}.xdmf")
    files = {f: read_h5(folder / f)[name] for f in sorted({f for _, f, _ in listed})}
    assert [k for _, _, k in listed] == list(range(len(listed)))
    return [t for t, _, _ in listed], [np.asarray(files[f][f"{name}_{k}"]["vector"].data) for _, f, k in listed], sorted(files)


def test_a_stopped_and_restarted_run_writes_what_one_set_of_sessions_forms_from_its_states(tmp_path, cylinder_case):
    """All four options on the cylinder, save_deg 2, a checkpoint every 5 steps: the first child is stopped by killturtle in
    its 11th step (a stop by -T after 11 steps cannot be asked for: the options refuse a run of fewer than padlen + 1 = 19
    and 22 frames before it starts), the second continues it under --restart-folder to 24 steps.  The yardstick is a replay
    and not a second solve (a restarted trajectory differs from an unsplit one at the Newton tolerance): the states rebuilt
    from the split run's own Visualization frames, in both files of each field, pushed through fsi_set_state and one
    uninterrupted set of sessions in a fresh context."""
    from vasp_amd.h5lite import read_h5
    from vasp_amd.hemodynamics import HemodynamicsRun, INDEX_NAMES
    from vasp_amd.spectrogram import SpectrogramRun
    from vasp_amd.stress_strain import AVERAGE_NAMES, FRAME_NAMES, StressStrainRun
    from test_hemodynamics import output_file_lists
    (tmp_path / "restart_case.py").write_text(HOOK_PROBLEM)
    res = tmp_path / "split" / "case" / "1"
    log1 = _child(tmp_path, ["--folder", str(res.parent), "--sub-folder", "1"])
    assert "killturtle found" in log1 and "Solved for timestep 11," in log1 and "Solved for timestep 12," not in log1
    manifest = json.loads((res / "Checkpoint" / "sessions" / "sessions.json").read_text())
    assert manifest["counter"] == 10 and sorted(manifest["sessions"]) == ["hemodynamics", "hi_pass", "spectrogram", "stress_strain"]
    assert manifest["sessions"]["hemodynamics"]["samples"] == manifest["sessions"]["hi_pass"]["frames"] == 11
    log2 = _child(tmp_path, ["--restart-folder", str(res)])
    for line in ("Hemodynamic indices of 24 frames", "Stress and strain of 24 frames", "Hi-pass fields of 24 frames (d, v, p)",
                 "Spectrograms of 24 frames"):
        assert line in log2, line
    # the states of the split run, from its Visualization files: d and v on every P2 node, p on the vertices
    mesh = cylinder_case[0]["mesh"]
    N2, V = mesh.num_nodes, mesh.num_vertices
    fields = {}
    for name in ("displacement", "velocity", "pressure"):
        h5s, times, idx = output_file_lists(res / "Visualization" / f"{name}.xdmf")
        assert h5s == [f"{name}.h5"] * 11 + [f"{name}_run_1.h5"] * 13 and idx == list(range(11)) + list(range(13))
        files = {f: read_h5(res / "Visualization" / f)["VisualisationVector"] for f in set(h5s)}
        fields[name] = np.stack([np.asarray(files[f][str(k)].data) for f, k in zip(h5s, idx)])
    assert len(times) == 24 and (np.diff(times) > 0.9e-3).all() and (np.diff(times) < 1.1e-3).all()      # no gap, no repeat
    states = np.concatenate([fields["displacement"].reshape(24, -1), fields["velocity"].reshape(24, -1), fields["pressure"][:, :V, 0]], axis=1)
    assert states.shape == (24, 6 * N2 + V)
    # one uninterrupted set of sessions on those states, through the drivers' own classes, in a folder named like the run's
    with contextlib.redirect_stdout(io.StringIO()):
        ns, desc, *_ = prepare_case("cylinder", CYL, tmp_path / "replay" / "case", T="0.0235",
                                    extra=["save_step=1", "save_deg=2"] + [f"{k}={v!r}" for k, v in E2E.items()])
    rep = tmp_path / "replay" / "case" / "1"
    with _context(desc) as hb:
        sessions = [cls(hb, ns["mesh"], ns) for cls in (HemodynamicsRun, StressStrainRun, hp.HiPassRun, SpectrogramRun)]
        for t, x in zip(times, states):
            hb.set_state("n", x)
            for s in sessions:
                s.sample(t, lambda: x)
        lines = []
        for s in sessions:
            s.finish(lines.append)
    assert any("Hi-pass fields of 24 frames" in line for line in lines)
    # the series that were appended during the run: 24 frames behind one XDMF, 11 + 13 in two files, the replay's in one
    for folder, names in (("Hemodynamic_indices", ("WSS",)), ("StressStrain", FRAME_NAMES)):
        for name in names:
            t_split, x_split, f_split = _series(res / folder, name)
            t_rep, x_rep, _ = _series(rep / folder, name)
            assert f_split == [f"{name}.h5", f"{name}_run_1.h5"] and t_split == t_rep == times
            assert len(x_split) == 24 and all(np.array_equal(a, b) for a, b in zip(x_split, x_rep)), name
    # what is written at the end over all frames: indices and averages, hi-pass files (float32), traces, spectrogram CSVs
    for folder, names in (("Hemodynamic_indices", INDEX_NAMES), ("StressStrain", AVERAGE_NAMES)):
        for name in names:
            got, ref = _datasets(res / folder / f"{name}.h5"), _datasets(rep / folder / f"{name}.h5")
            assert got == ref and len(got) >= 6, name
            vec = np.frombuffer(got[f"/{name}/{name}_0/vector"][2])
            assert np.isfinite(vec).any()
    compared = 0
    for folder in ("Visualization_hi_pass", "Visualization_separate_domain", "Spectrograms"):
        mine, theirs = sorted(p.name for p in (res / folder).iterdir()), sorted(p.name for p in (rep / folder).iterdir())
        assert mine == theirs and mine, folder
        for name in mine:
            if name.endswith(".h5"):
                got = _datasets(res / folder / name)
                assert got == _datasets(rep / folder / name), name
                assert got["/VisualisationVector/23"][0] == "float32" and len(got) == 2 + 24
            else:
                assert (res / folder / name).read_bytes() == (rep / folder / name).read_bytes(), name
            compared += 1
    assert compared == 3 * 5 + 3 * 2 + 4
