"""Host side of ``python -m vasp_amd.postprocess``: the lazy HDF5 reader, the frame source, the state builder, the frame
selection, the command end to end with a backend that has no device sessions, its refusals and the shared option parser.
Every comparison is exact: the Visualization files are FP64 copies of the state and the host sessions are deterministic."""
import contextlib
import io
import shutil

import numpy as np
import pytest

from conftest import GOLDEN
from vasp_amd import hi_pass as hp
from vasp_amd.frames import FrameSource, selected_indices, state_from_frame
from vasp_amd.h5lite import Dataset, H5Error, open_h5, read_h5
from vasp_amd.output import FIELDS, VisualizationWriter

CYL = GOLDEN / "cylinder" / "cylinder.h5"
DT = 1e-3
REGION = ["--spectrogram-fsi-region", "0", "0", "0", "100"]
OPTIONS = ["--hi-pass", "d", "v", "p", "--hi-pass-bands", "0", "100", "--hi-pass-amplitude", "--hi-pass-window", "8",
           "--spectrogram", "v", *REGION]


@pytest.fixture(scope="module")
def mesh(cylinder_case):
    return cylinder_case[0]["mesh"]


@pytest.fixture(scope="module")
def written(mesh, tmp_path_factory):
    """Per save_deg a folder with a series of 5 frames and its continuation of 3 (``run_index=1``): (results, states, times)."""
    out = {}
    rng = np.random.default_rng(3)
    for deg in (1, 2):
        results = tmp_path_factory.mktemp(f"series{deg}")
        states = rng.standard_normal((8, mesh.num_dofs))
        times = [DT * (k + 1) for k in range(8)]
        w = VisualizationWriter(results / "Visualization", mesh, deg)
        for k in range(5):
            w.write(states[k], times[k])
        w.close()
        w = VisualizationWriter(results / "Visualization", mesh, deg, run_index=1)
        for k in range(5, 8):
            w.write(states[k], times[k])
        w.close()
        out[deg] = (results, states, times)
    return out


# ---- 1. the lazy reader and the frame source ---------------------------------------------------------------------------

def _walk(g, prefix=""):
    for k in sorted(g.keys()):
        if isinstance(g[k], Dataset):
            yield prefix + "/" + k, g[k]
        else:
            yield from _walk(g[k], prefix + "/" + k)


@pytest.mark.parametrize("deg", [1, 2])
def test_lazy_reader_gives_read_h5s_datasets_as_views(written, mesh, deg):
    results, states, times = written[deg]
    n = mesh.num_nodes if deg == 2 else mesh.num_vertices
    for name, _, _ in FIELDS:
        for file, frames in ((f"{name}.h5", 5), (f"{name}_run_1.h5", 3)):
            path = results / "Visualization" / file
            eager = dict(_walk(read_h5(path)))
            with open_h5(path) as lazy:
                mine = dict(_walk(lazy.root))
                assert sorted(mine) == sorted(eager) and len([k for k in mine if "VisualisationVector" in k]) == frames
                for key, ds in eager.items():
                    assert mine[key].shape == ds.shape and mine[key].attrs.keys() == ds.attrs.keys(), key
                    a = mine[key].data
                    assert a.dtype == ds.data.dtype and np.array_equal(a, ds.data), key
                frame = lazy["VisualisationVector"]["0"].data
                assert frame.base is not None and not frame.flags.owndata and not frame.flags.writeable
                assert frame.shape == (n, 1 if name == "pressure" else 3) and frame.flags.c_contiguous


def test_lazy_reader_resolves_the_repointed_tables_of_a_long_series(tmp_path):
    """40 appends with a small metadata reserve: the series group's tables moved and doubled several times."""
    from vasp_amd.h5lite import Group, H5Series
    s = H5Series(tmp_path / "long.h5", Group(), "VisualisationVector", reserve=256)
    for k in range(40):
        s.append(str(k), np.full((7, 3), float(k)))
    s.close()
    with open_h5(tmp_path / "long.h5") as lazy:
        series = lazy["VisualisationVector"]
        assert sorted(series, key=int) == [str(k) for k in range(40)]
        assert all(np.array_equal(series[str(k)].data, np.full((7, 3), float(k))) for k in range(40))


def test_lazy_reader_names_a_dataset_it_cannot_map(tmp_path):
    """A chunked layout (class 2) in the layout message of a dataset: H5Error with the dataset's path."""
    from vasp_amd.h5lite import Group, write_h5
    root, g = Group(), Group()
    g["x"] = Dataset(np.arange(6.0))
    root["grp"] = g
    write_h5(tmp_path / "c.h5", root)
    raw = bytearray((tmp_path / "c.h5").read_bytes())
    import struct
    hits = [i for i in range(0, len(raw) - 8, 8) if struct.unpack_from("<HH", raw, i) == (0x0008, 24) and raw[i + 8] == 3 and raw[i + 9] == 1]
    assert len(hits) == 1
    raw[hits[0] + 9] = 2
    (tmp_path / "c.h5").write_bytes(bytes(raw))
    with pytest.raises(H5Error, match="/grp/x"):
        open_h5(tmp_path / "c.h5")


@pytest.mark.parametrize("deg", [1, 2])
def test_frame_source_lists_the_writers_frames(written, deg):
    results, states, times = written[deg]
    src = FrameSource(results, deg)
    assert len(src) == 8 and src.times == times
    for name, _, _ in FIELDS:
        assert src.entries[name] == [(times[k], f"{name}.h5", k) for k in range(5)] + [(times[5 + k], f"{name}_run_1.h5", k) for k in range(3)]
    src.close()


# ---- 2. the state builder ----------------------------------------------------------------------------------------------

def test_state_from_frame_returns_a_save_deg_2_state_bit_for_bit(written, mesh):
    results, states, times = written[2]
    src = FrameSource(results, 2)
    src.check_files("dvp")
    assert src.node_count("dvp") == mesh.num_nodes
    seen = 0
    for k, (t, views) in enumerate(src.frames(range(8), "dvp")):
        assert t == times[k] and all(a.base is not None for a in views.values())
        assert np.array_equal(state_from_frame(mesh, 2, **views), states[k]) and np.array_equal(src.state(mesh, views), states[k])
        seen += 1
    assert seen == 8
    src.close()


def test_state_from_frame_interpolates_a_save_deg_1_state(written, mesh):
    results, states, times = written[1]
    V, N2, e = mesh.num_vertices, mesh.num_nodes, mesh.edges
    src = FrameSource(results, 1)
    assert src.node_count("dvp") == V
    for k, (t, views) in zip((0, 6), src.frames((0, 6), "dvp")):
        x = state_from_frame(mesh, 1, **views)
        d0, v0, p0 = mesh.split(states[k])
        for got, ref in zip(mesh.split(x)[:2], (d0, v0)):
            assert np.array_equal(got[:V], ref[:V])
            assert np.array_equal(got[V:], 0.5 * (ref[e[:, 0]] + ref[e[:, 1]])) and len(got) == N2
        assert np.array_equal(mesh.split(x)[2], p0)
    src.close()


def test_a_pressure_selection_touches_neither_displacement_nor_velocity_files(written, mesh, tmp_path):
    results, states, times = written[2]
    copy = tmp_path / "only_p"
    shutil.copytree(results, copy)
    for name in ("displacement", "velocity"):
        for f in (f"{name}.h5", f"{name}_run_1.h5"):
            (copy / "Visualization" / f).unlink()
    src = FrameSource(copy, 2)
    src.check_files("p")
    for k, (t, views) in enumerate(src.frames(range(8), "p")):
        assert sorted(views) == ["p"]
        assert np.array_equal(mesh.split(state_from_frame(mesh, 2, **views))[2], mesh.split(states[k])[2])
    src.close()
    with pytest.raises(SystemExit, match="displacement.h5"):
        FrameSource(copy, 2).check_files("dp")


# ---- 3. frame selection ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride,t0,t1", [(2, 0.004, 0.02), (1, 0.0, None), (3, 0.0105, 0.0195), (5, 0.02, 0.021), (2, 0.03, None)])
def test_selection_is_hi_pass_select_frames(stride, t0, t1):
    times = [DT * (k + 1) for k in range(24)]
    first, count = hp.select_frames(times, DT, stride, t0, t1)
    assert selected_indices(times, DT, stride, t0, t1) == list(range(first, first + count * stride, stride))
    if (stride, t0, t1) == (2, 0.004, 0.02):
        assert selected_indices(times, DT, stride, t0, t1) == [4, 6, 8, 10, 12, 14, 16, 18]       # t = 0.005, 0.007, ..., 0.019


# ---- 4. the host path end to end ---------------------------------------------------------------------------------------

def _never(desc):
    raise AssertionError("a backend was built")


def _post(argv, factory):
    from vasp_amd import postprocess
    lines = []
    with contextlib.redirect_stdout(io.StringIO()):
        ns = postprocess.run(argv, backend_factory=factory, out=lines.append)
    return ns, lines


def _host_run(folder, options):
    """24 steps of the cylinder in <folder>/1 with a backend without device sessions: (results folder, the stub class)."""
    from test_session_restart import _Stub
    from vasp_amd import monolithic
    with contextlib.redirect_stdout(io.StringIO()):
        monolithic.run(["-p", "cylinder", "-dt", "0.001", "-T", "0.0235", "--theta", "0.51", "--folder", str(folder), "--sub-folder", "1",
                        "--save-step", "1", "--save-deg", "2", "--checkpoint-step", "5", "--verbose", "False", *options,
                        "--new-arguments", f"mesh_path={CYL}"], backend_factory=_Stub, out=lambda *a: None)
    return folder / "1", _Stub


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    return _host_run(tmp_path_factory.mktemp("hostrun") / "case", OPTIONS)


def _datasets(path):
    return {k: (str(ds.data.dtype), ds.data.shape, ds.data.tobytes()) for k, ds in _walk(read_h5(path))}


def _same_tree(a, b):
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir()) and names
    for name in names:
        if name.endswith(".h5"):
            assert _datasets(a / name) == _datasets(b / name), name
        else:
            assert (a / name).read_bytes() == (b / name).read_bytes(), name
    return names


def test_postprocess_writes_what_the_run_wrote(host_run, tmp_path):
    results, stub = host_run
    out = tmp_path / "again"
    ns, lines = _post(["--folder", str(results), "--output-folder", str(out), *OPTIONS], stub)
    assert ns["frames_read"] == 24 and any("Hi-pass fields of 24 frames (d, v, p)" in line for line in lines)
    assert any("Spectrograms of 24 frames" in line for line in lines)
    hi = _same_tree(results / "Visualization_hi_pass", out / "Visualization_hi_pass")
    assert len([n for n in hi if n.endswith(".h5")]) == 6 and len([n for n in hi if n.endswith(".csv")]) == 3
    assert len(_same_tree(results / "Spectrograms", out / "Spectrograms")) == 4
    assert not (out / "Checkpoint").exists()


def test_the_runs_own_window_options_given_alone_act_as_in_the_run(tmp_path):
    """--hi-pass-start-time / --hi-pass-end-time without --stride / --start-time / --end-time: every frame is read, and the
    option selects among them and labels the files as it does in the run (22 of 24 frames, from t = 0.003)."""
    options = ["--hi-pass", "v", "p", "--hi-pass-bands", "0", "100", "--hi-pass-amplitude", "--hi-pass-window", "8", "--hi-pass-point-ids", "3",
               "--hi-pass-start-time", "0.003", "--hi-pass-end-time", "0.0245"]
    results, stub = _host_run(tmp_path / "case", options)
    ns, lines = _post(["--folder", str(results), "--output-folder", str(tmp_path / "again"), *options], stub)
    assert ns["frames_read"] == 24 and ns["frame_start"] is None and any("Hi-pass fields of 22 frames (v, p)" in line for line in lines)
    _same_tree(results / "Visualization_hi_pass", tmp_path / "again" / "Visualization_hi_pass")
    assert _same_tree(results / "Visualization_separate_domain", tmp_path / "again" / "Visualization_separate_domain") == [
        "pressure_point_id_3.csv", "velocity_point_id_3.csv"]
    trace = np.loadtxt(tmp_path / "again" / "Visualization_separate_domain" / "pressure_point_id_3.csv", delimiter=",")
    assert trace.shape == (22, 2) and abs(trace[0, 0] - 0.003) < 1e-12 and abs(trace[-1, 0] - 0.024) < 1e-12


def test_a_window_sets_the_frames_the_spacing_and_the_start_time_the_sessions_see(host_run, tmp_path, mesh):
    results, stub = host_run
    from vasp_amd import postprocess
    from vasp_amd.spectrogram import SpectrogramRun
    band = ["--folder", str(results), "--hi-pass", "p", "--hi-pass-bands", "0", "100", "--hi-pass-point-ids", "3"]
    backend = stub({"num_nodes": mesh.num_nodes, "coords": mesh.coords})
    for argv, indices, stride, start, fields in (
            ([*band, "--spectrogram", "v", *REGION, "--start-time", "0.003"], list(range(2, 24)), 1, 0.003, ["v", "p"]),
            ([*band, "--stride", "1", "--end-time", "0.02"], list(range(0, 20)), 1, None, ["p"])):      # no --start-time: the options keep their own
        with contextlib.redirect_stdout(io.StringIO()):
            ns, _, source, got, read = postprocess.prepare(argv, stub)
        assert got == indices and ns["frame_times"] == [source.times[k] for k in indices] and read == fields
        assert (ns["frame_stride"], ns["frame_start"]) == (stride, start)
        source.close()
        ns = dict(ns, results_folder=tmp_path / "w")
        hi = hp.HiPassRun(backend, mesh, ns)
        assert (hi.t0, hi.dt_files, hi.stride) == (start or 0.0, 0.001 * 1, 1)
        if "v" in fields:
            spec = SpectrogramRun(backend, mesh, ns)
            assert (spec.start_t, spec.dt_files) == (start, 0.001 * 1) and spec.case == "case"      # the folder that was read names the files
    # a stride changes the spacing every session is told: the hemodynamic sample spacing, the filters' sampling rate
    from vasp_amd.hi_pass import frame_spacing, saved_times
    v = dict(dt=0.001, save_step=2, T=0.01)
    assert frame_spacing(v) == 0.001 * 2 and frame_spacing(dict(v, frame_stride=3)) == 0.001 * 2 * 3
    assert saved_times(dict(v, frame_times=[0.5, 0.7])) == [0.5, 0.7] and len(saved_times(v)) == 6


# ---- 5. refusals -------------------------------------------------------------------------------------------------------

def _refused(argv, match):
    from vasp_amd import postprocess
    with pytest.raises(SystemExit, match=match), contextlib.redirect_stdout(io.StringIO()):
        postprocess.run(argv, backend_factory=_never, out=lambda *a: None)


def test_refusals_come_before_any_backend(host_run, tmp_path, monkeypatch):
    results, _ = host_run
    base = ["--hi-pass", "d", "v", "p", "--hi-pass-bands", "0", "100"]
    _refused(["--folder", str(tmp_path / "nowhere"), *base], "nowhere")
    copy = tmp_path / "copy"
    shutil.copytree(results, copy, ignore=shutil.ignore_patterns("Visualization_hi_pass", "Spectrograms"))
    (copy / "Visualization" / "pressure.xdmf").rename(copy / "Visualization" / "pressure.kept")
    _refused(["--folder", str(copy), *base], "pressure.xdmf")
    (copy / "Visualization" / "pressure.kept").rename(copy / "Visualization" / "pressure.xdmf")
    # a velocity series one frame shorter than the displacement series: its last <Grid> cut from the XDMF
    path = copy / "Visualization" / "velocity.xdmf"
    text = path.read_text()
    cut = text.rindex("      <Grid>\n")
    path.write_text(text[:cut] + VisualizationWriter.FOOTER)
    _refused(["--folder", str(copy), *base], r"velocity.xdmf lists 23 frames, displacement.xdmf lists 24")
    path.write_text(text)
    (copy / "Visualization" / "velocity.h5").unlink()
    _refused(["--folder", str(copy), *base], "velocity.h5 not found")
    _refused(["--folder", str(results), *base, "--stride", "2", "--hi-pass-stride", "2"],
             r"--stride together with --hi-pass-stride.*on a finished folder use --stride")
    _refused(["--folder", str(results), *base, "--start-time", "0.0", "--end-time", "0.0105"], r"saves 10 frames.*padlen \+ 1 = 19")
    _refused(["--folder", str(results), "--spectrogram", "v", *REGION, "--stride", "2"], r"--spectrogram: the run saves 12 frames")
    _refused(["--folder", str(results), "--hemodynamics", "--stress-strain", "--start-time", "1.0"],
             r"no saved frame of .*Visualization lies in the window.*its 24 frames run from t = 0.001 to 0.024")
    (copy / "Checkpoint" / "default_variables.json").unlink()
    _refused(["--folder", str(copy), *base], r"Checkpoint/default_variables.json not found")
    monkeypatch.setenv("WORLD_SIZE", "2")
    _refused(["--folder", str(results), *base], "WORLD_SIZE = 2")


def test_a_frame_of_another_mesh_is_refused(host_run, stenosis_case, tmp_path):
    """The results folder of the cylinder run with the Visualization files of the stenosis mesh."""
    results, _ = host_run
    copy = tmp_path / "othermesh"
    shutil.copytree(results, copy, ignore=shutil.ignore_patterns("Visualization*", "Spectrograms"))
    other = stenosis_case[0]["mesh"]
    w = VisualizationWriter(copy / "Visualization", other, 1)
    w.write(np.zeros(other.num_dofs), 0.001)
    w.close()
    _refused(["--folder", str(copy), "--hi-pass", "v"], rf"a frame has {other.num_vertices} nodes, the mesh .* has 352 vertices .* and 2500 P2 nodes")


# ---- 6. the shared parser ----------------------------------------------------------------------------------------------

def test_monolithic_parse_returns_what_it_returned(tmp_path):
    from vasp_amd import postprocess
    from vasp_amd.monolithic import parse
    argv = ["--spectrogram", "v", "p", "--spectrogram-sampling", "All", "--spectrogram-fsi-region", "0.008", "0", "0", "0.004",
            "--spectrogram-min-color", "-12", "--spectrogram-interface-only", "--spectrogram-seed", "3"]
    a = dict(spectrogram=["v", "p"], spectrogram_sampling="All", spectrogram_fsi_region=[0.008, 0, 0, 0.004], spectrogram_min_color=-12,
             spectrogram_interface_only=True, spectrogram_seed=3)
    assert parse(argv) == dict(a, problem="offset_stenosis")
    assert parse([]) == {"problem": "offset_stenosis"}
    cfg = tmp_path / "run.cfg"
    cfg.write_text('spectrogram = ["d"]\nspectrogram_fsi_region = [0, 0, 0, 1]\nspectrogram-n-samples = 20\nspectrogram_window = hann\n')
    c = dict(spectrogram=["d"], spectrogram_fsi_region=[0, 0, 0, 1], spectrogram_n_samples=20, spectrogram_window="hann")
    assert parse(["-c", str(cfg)]) == dict(c, problem="offset_stenosis")
    n = dict(spectrogram=["p"], spectrogram_component="mag", spectrogram_point_ids=[4, 5])
    assert parse(["--new-arguments", "spectrogram=['p']", "spectrogram_component=mag", "spectrogram_point_ids=[4, 5]"]) == dict(n, problem="offset_stenosis")
    assert list(parse(argv)) == ["spectrogram", "spectrogram_fsi_region", "spectrogram_interface_only", "spectrogram_sampling",
                                 "spectrogram_seed", "spectrogram_min_color", "problem"]      # the order the options are declared in
    # the tool's parser takes the same options with the same defaults
    assert postprocess.parse(["--folder", "x", *argv]) == dict(results="x", **a)
    assert postprocess.parse(["--folder", "x", "-c", str(cfg), "--stride", "2"]) == dict(c, results="x", stride=2)
    assert postprocess.parse(["--folder", "x"]) == dict(results="x")
