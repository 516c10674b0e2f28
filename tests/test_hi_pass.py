"""Host side of --hi-pass (vasp_amd/hi_pass.py): the NumPy restatement of scipy's filtfilt and of the reference's windowed
RMS, the reference's band rules, the files of Visualization_hi_pass/, the refusals, and the C-ABI's new entry points."""
import contextlib
import importlib.util
import io
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from vasp_amd import hi_pass as hp

_spec = importlib.util.spec_from_file_location("make_hi_pass", GOLDEN / "make_hi_pass.py")
make_hi_pass = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_hi_pass)
CASES = make_hi_pass.CASES
CYL = GOLDEN / "cylinder" / "cylinder.h5"


# ---- the filter -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(CASES)))
def test_restatement_equals_scipy_filtfilt_exactly(i):
    from scipy.signal import filtfilt
    dt, lo, hi, n = CASES[i]
    prm = hp.design(dt, lo, hi)
    x = make_hi_pass.rows(dt, n, 100 + i)
    got = hp.filtfilt_rows(prm["b"], prm["a"], x, prm["zi"], prm["padlen"])
    for r in range(x.shape[1]):
        assert np.array_equal(got[:, r], filtfilt(prm["b"], prm["a"], x[:, r])), r
    # the signal of interest sits three decades below the carrier: the band-pass result is small against the input
    if prm["btype"] == "bandpass":
        assert np.abs(got).max() < 1e-2 * np.abs(x).max()
    assert np.array_equal(hp.filtfilt_rows(prm["b"], prm["a"], x), got)             # zi and padlen default to scipy's


@pytest.mark.parametrize("i", range(len(CASES)))
def test_restatement_equals_the_stored_results(i):
    """The same with the stored coefficients and results: independent of the installed scipy's design and filter."""
    g = np.load(GOLDEN / "hi_pass" / "filtfilt.npz")
    dt, lo, hi, n = CASES[i]
    assert np.array_equal(g[f"x{i}"], make_hi_pass.rows(dt, n, 100 + i))
    got = hp.filtfilt_rows(g[f"b{i}"], g[f"a{i}"], g[f"x{i}"], g[f"zi{i}"], 3 * len(g[f"b{i}"]))
    assert np.array_equal(got, g[f"y{i}"])
    prm = hp.design(dt, lo, hi)                # scipy's design moves by ulps between versions, not more
    for key in ("b", "a", "zi"):
        np.testing.assert_allclose(prm[key], g[f"{key}{i}"], rtol=1e-9, atol=0)


def test_filtfilt_refuses_a_series_no_longer_than_padlen():
    prm = hp.design(1e-3, 25.0, 1000.0)
    with pytest.raises(ValueError, match="greater than padlen, which is 33"):
        hp.filtfilt_rows(prm["b"], prm["a"], np.zeros((33, 2)))
    assert hp.filtfilt_rows(prm["b"], prm["a"], np.zeros((34, 2))).shape == (34, 2)
    assert hp.padlen_of(25.0) == 33 and hp.padlen_of(0.0) == 18 == hp.design(1e-3, 0.0, 200.0)["padlen"]


# ---- the amplitude ----------------------------------------------------------------------------------------------------

def _reference_rms(signal_array, window_size):
    """calculate_windowed_rms(., ., "flat") written out."""
    signal_squared = np.power(signal_array, 2)
    window = np.ones(window_size) / float(window_size)
    RMS = np.sqrt(np.convolve(signal_squared, window, mode="valid"))
    len_RMS, len_sq = len(RMS), len(signal_squared)
    pad_length = int((len_sq - len_RMS) / 2)
    padded = np.zeros(len_sq)
    for i in range(len_sq):
        if pad_length <= i < len_RMS + pad_length:
            padded[i] = RMS[i - pad_length]
    return padded


@pytest.mark.parametrize("n,w", [(50, 8), (50, 9), (51, 8), (40, 40), (40, 1), (300, 250)])
def test_rms_restatement_equals_the_reference_formula(n, w):
    y = np.random.default_rng(n + w).standard_normal((n, 3)) * 1e-6
    got = hp.windowed_rms_rows(y, w)
    for r in range(3):
        ref = _reference_rms(y[:, r], w)
        assert np.array_equal(got[:, r], ref)
        assert np.array_equal(np.nonzero(ref)[0], np.arange((w - 1) // 2, (w - 1) // 2 + n - w + 1))      # odd and even n - w
    run = hp.windowed_rms_running(y, w)
    assert np.array_equal(run == 0, got == 0) and not np.isnan(run).any() and (run >= 0).all()
    assert np.abs(run - got).max() <= 1e-6 * np.abs(got).max()


def test_running_sum_never_gives_nan():
    """A burst followed by exact zeros: add-and-subtract leaves a sum of rounding size, possibly negative; the clamp holds."""
    y = np.zeros((400, 2))
    y[:70] = np.random.default_rng(0).standard_normal((70, 2)) * 1e3
    run = hp.windowed_rms_running(y, 8, refresh=10 ** 9)           # never refreshed: the worst case
    assert not np.isnan(run).any() and (run >= 0).all()
    assert np.array_equal(hp.windowed_rms_running(y, 8)[140:], np.zeros((260, 2)))      # refreshed: exactly zero again


def test_amplitude_magnitude_is_numpys_norm():
    a = np.random.default_rng(1).standard_normal((100, 3))
    assert np.array_equal(hp.amplitude_magnitude(a), np.linalg.norm(a, axis=1))
    assert np.array_equal(hp.amplitude_magnitude(a[:, :1]), a[:, 0])


def _host_sessions(capacity):
    from vasp_amd.spectrogram import HostSpecSession
    return hp.HostBandSession(3, capacity), HostSpecSession(6, capacity)


def test_the_two_host_sessions_record_and_filter_the_same_history():
    """One recording half (HostHistory): the same frames in, the same bytes out of both sessions, raw and filtered."""
    frames = np.random.default_rng(5).standard_normal((40, 6))
    prm = hp.design(1e-3, 25.0, 1000.0)
    band, spec = _host_sessions(40)
    for s in (band, spec):
        for f in frames:
            s.sample(f)
        s.filter(prm["b"], prm["a"], prm["zi"], prm["padlen"])
    for k in range(40):
        assert band.fetch("raw", k).tobytes() == spec.fetch(k).tobytes() == frames[k].tobytes(), k
        assert band.fetch("filtered", k).tobytes() == spec.fetch(k, filtered=True).tobytes(), k
    assert band.fetch("raw", 0).shape == (2, 3) and spec.fetch(0).shape == (6,)
    assert np.array_equal(np.stack(spec.filtered), hp.filtfilt_rows(prm["b"], prm["a"], frames, prm["zi"], prm["padlen"]))


def test_both_host_sessions_refuse_a_frame_beyond_their_capacity():
    for s, name in zip(_host_sessions(3), ("hi-pass", "spectrogram")):
        for _ in range(3):
            s.sample(np.zeros(6))
        with pytest.raises(RuntimeError, match=name + r" history is full \(capacity declared at begin\)"):
            s.sample(np.zeros(6))
        assert len(s.raw) == 3


# ---- the band rules ---------------------------------------------------------------------------------------------------

def test_band_rules_give_the_reference_numbers():
    p = hp.band_parameters(3.3964e-4, 25.0, 1000.0)             # int(1 / 3.3964e-4) = 2944
    assert (p["fs"], p["critical"], p["highcut"], p["btype"], p["name"]) == (2943, 1471.0, 1000.0, "bandpass", "25_to_1000")
    p = hp.band_parameters(3.3964e-4, 25.0, 100000.0)
    assert (p["highcut"], p["name"]) == (1471.0, "25_to_100000")                # clipped; the name keeps the band asked for
    p = hp.band_parameters(1e-3, 25.0, 1000.0)
    assert (p["fs"], p["critical"], p["highcut"], p["btype"]) == (999, 499.0, 499.0, "bandpass")
    assert hp.band_parameters(1e-3, 0.05, 200.0)["btype"] == "lowpass" and hp.band_parameters(1e-3, 0.1, 200.0)["btype"] == "bandpass"
    d = hp.design(1e-3, 25.0, 1000.0)
    assert len(d["b"]) == len(d["a"]) == 11 and len(d["zi"]) == 10 and d["padlen"] == 33 and d["a"][0] == 1.0
    d = hp.design(1e-3, 0.0, 200.0)
    assert len(d["b"]) == len(d["a"]) == 6 and len(d["zi"]) == 5


# ---- files ------------------------------------------------------------------------------------------------------------

XDMF_2 = '''<?xml version="1.0"?>
<!DOCTYPE Xdmf SYSTEM "Xdmf.dtd" []>
<Xdmf Version="3.0" xmlns:xi="http://www.w3.org/2001/XInclude">
  <Domain>
    <Grid Name="TimeSeries_pressure_25_to_1000" GridType="Collection" CollectionType="Temporal">
      <Grid Name="mesh" GridType="Uniform">
        <Topology NumberOfElements="2" TopologyType="Tetrahedron" NodesPerElement="4">
          <DataItem Dimensions="2 4" NumberType="UInt" Format="HDF">pressure_25_to_1000.h5:/Mesh/0/mesh/topology</DataItem>
        </Topology>
        <Geometry GeometryType="XYZ">
          <DataItem Dimensions="5 3" Format="HDF">pressure_25_to_1000.h5:/Mesh/0/mesh/geometry</DataItem>
        </Geometry>
        <Time Value="0.0" />
        <Attribute Name="pressure_25_to_1000" AttributeType="Scalar" Center="Node">
          <DataItem Dimensions="5 1" Format="HDF">pressure_25_to_1000.h5:/VisualisationVector/0</DataItem>
        </Attribute>
      </Grid>
      <Grid>
        <xi:include xpointer="xpointer(//Grid[@Name=&quot;TimeSeries_pressure_25_to_1000&quot;]/Grid[1]/*[self::Topology or self::Geometry])" />
        <Time Value="0.002" />
        <Attribute Name="pressure_25_to_1000" AttributeType="Scalar" Center="Node">
          <DataItem Dimensions="5 1" Format="HDF">pressure_25_to_1000.h5:/VisualisationVector/1</DataItem>
        </Attribute>
      </Grid>
    </Grid>
  </Domain>
</Xdmf>
'''


def test_writer_files_follow_the_reference_templates(tmp_path):
    from vasp_amd.h5lite import read_h5
    geom = np.random.default_rng(0).standard_normal((5, 3))
    topo = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], dtype=np.int64)
    w = hp.HiPassWriter(tmp_path / "Visualization_hi_pass", geom, topo)
    frames = [np.random.default_rng(k).standard_normal((5, 1)) * 1e-7 for k in range(2)]
    w.write_series("pressure_25_to_1000", iter(frames), 2, 1, 0.002, 0.0)
    assert (tmp_path / "Visualization_hi_pass" / "pressure_25_to_1000.xdmf").read_text() == XDMF_2
    g = read_h5(tmp_path / "Visualization_hi_pass" / "pressure_25_to_1000.h5")
    assert sorted(g.keys()) == ["Mesh", "VisualisationVector"] and sorted(g["VisualisationVector"].keys()) == ["0", "1"]
    ge, to = np.asarray(g["Mesh"]["0"]["mesh"]["geometry"].data), np.asarray(g["Mesh"]["0"]["mesh"]["topology"].data)
    assert ge.dtype == np.float32 and ge.shape == (5, 3) and np.array_equal(ge, geom.astype(np.float32))
    assert to.dtype == np.int32 and to.shape == (2, 4) and np.array_equal(to, topo)
    for k in range(2):
        d = np.asarray(g["VisualisationVector"][str(k)].data)
        assert d.dtype == np.float32 and d.shape == (5, 1) and np.array_equal(d, frames[k].astype(np.float32))
    vec = [np.random.default_rng(9).standard_normal((5, 3))]
    w.write_series("velocity_25_to_1000_amplitude", iter(vec), 1, 3, 0.002, 0.0)
    text = (tmp_path / "Visualization_hi_pass" / "velocity_25_to_1000_amplitude.xdmf").read_text()
    assert 'AttributeType="Vector"' in text and '<DataItem Dimensions="5 3" Format="HDF">velocity_25_to_1000_amplitude.h5:/VisualisationVector/0<' in text
    assert "xi:include" not in text
    with pytest.raises(ValueError, match="expected 3"):
        w.write_series("x", iter(vec), 3, 3, 0.002, 0.0)
    # the table: 13 columns under the reference's header, as numpy.savetxt writes it
    mag = np.abs(np.random.default_rng(2).standard_normal(50))
    row = hp.amplitude_row(0.004, mag, mag.max(), int(np.argmax(mag)))
    assert row.shape == (13,) and row[0] == 0.004 and row[3] == np.percentile(mag, 100) and row[4] == mag.min() and row[12] == np.argmax(mag)
    assert row[1] == np.percentile(mag, 95) and row[8] == np.percentile(mag, 97.5) and row[11] == np.percentile(mag, 1)
    w.write_table("velocity_25_to_1000", np.stack([row, row]))
    lines = (tmp_path / "Visualization_hi_pass" / "velocity_25_to_1000.csv").read_text().splitlines()
    assert lines[0] == "# " + hp.CSV_HEADER and len(hp.CSV_HEADER.split(", ")) == 13 and len(lines) == 3
    assert lines[0].startswith("# time (s), 95th percentile amplitude, 5th percentile amplitude, maximum amplitude, minimum amplitude, average")
    assert lines[0].endswith("1st percentile amplitude, ID of node with max amplitude")
    np.testing.assert_array_equal(np.loadtxt(tmp_path / "Visualization_hi_pass" / "velocity_25_to_1000.csv", delimiter=","), np.stack([row, row]))


# ---- the command line, the refusals, the driver -------------------------------------------------------------------------

def test_options_from_the_command_line_a_config_file_and_new_arguments(tmp_path):
    from vasp_amd.monolithic import parse
    a = parse(["--hi-pass", "d", "v", "p", "--hi-pass-bands", "25", "1000", "0", "200", "--hi-pass-window", "8", "--hi-pass-amplitude"])
    assert a["hi_pass"] == ["d", "v", "p"] and a["hi_pass_bands"] == [25, 1000, 0, 200] and a["hi_pass_window"] == 8
    assert a["hi_pass_amplitude"] is True
    assert hp.bands(a) == [(25.0, 1000.0), (0.0, 200.0)] and hp.quantities({"hi_pass": ["p", "d"]}) == ["d", "p"]
    assert hp.bands({}) == [(25.0, 1000.0)]
    plain = parse([])
    assert not any(k.startswith("hi_pass") for k in plain)
    cfg = tmp_path / "run.cfg"
    cfg.write_text('hi_pass = ["v"]\nhi_pass_bands = [30, 400]\nhi-pass-window = 16\n')
    c = parse(["-c", str(cfg)])
    assert c["hi_pass"] == ["v"] and c["hi_pass_bands"] == [30, 400] and c["hi_pass_window"] == 16
    n = parse(["--new-arguments", "hi_pass=['p']", "hi_pass_amplitude=True"])
    assert n["hi_pass"] == ["p"] and n["hi_pass_amplitude"] is True
    with pytest.raises(SystemExit, match="pairs"):
        hp.bands({"hi_pass_bands": [25, 1000, 30]})
    with pytest.raises(SystemExit, match="d, v and / or p"):
        hp.quantities({"hi_pass": ["strain"]})


def test_expected_frames_counts_what_the_loop_saves():
    assert hp.expected_frames(dict(dt=0.001, T=0.04, save_step=1)) == 41              # t = 0 .. 0.04 at the loop's test
    assert hp.expected_frames(dict(dt=0.001, T=0.005, save_step=2)) == 3                 # counters 0, 2, 4
    assert hp.expected_frames(dict(dt=0.001, T=0.0105, save_step=10, counter=1)) == 1


def _refusal(extra, world=1, cls=None):
    from vasp_amd.monolithic import parameters
    with contextlib.redirect_stdout(io.StringIO()):
        _, _, v = parameters(["-p", "cylinder", "--hi-pass", "v", "--verbose", "False", *extra])
    return hp.hi_pass_refusal(v, world, cls)


def test_each_refusal_has_its_message(tmp_path, monkeypatch):
    ok = ["-dt", "0.001", "-T", "0.039", "--save-step", "1"]           # 40 frames: the loop steps while t <= T
    assert _refusal(ok) == ""
    assert "cannot be used with --restart-folder" in _refusal(ok + ["--restart-folder", str(tmp_path)])
    assert "one rank only (WORLD_SIZE > 1)" in _refusal(ok, world=2)
    assert "needs --save-step" in _refusal(["-dt", "0.001", "-T", "0.04", "--save-step", "0"])
    msg = _refusal(["-dt", "0.001", "-T", "0.032", "--save-step", "1"])
    assert "saves 33 frames" in msg and "padlen + 1 = 34" in msg
    assert _refusal(["-dt", "0.001", "-T", "0.032", "--save-step", "1", "--hi-pass-bands", "0", "200"]) == ""       # low-pass: 19
    msg = _refusal(ok + ["--hi-pass-amplitude"])
    assert "saves 40 frames, fewer than the window of 250" in msg
    assert _refusal(ok + ["--hi-pass-amplitude", "--hi-pass-window", "40"]) == ""
    # through the driver: refused before anything is built (no results folder appears), on every rank
    from vasp_amd import monolithic
    argv = ["-p", "cylinder", "-dt", "0.001", "-T", "0.01", "--save-step", "1", "--verbose", "False", "--folder", str(tmp_path / "r"),
            "--hi-pass", "d", "--new-arguments", f"mesh_path={CYL}"]
    with pytest.raises(SystemExit, match="padlen"):
        monolithic.run(argv, backend_factory=_Stub)
    assert not (tmp_path / "r").exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    with pytest.raises(SystemExit, match="one rank only"):
        monolithic.run(argv[:5] + ["0.04"] + argv[6:], backend_factory=_Stub)


class _Stub:
    """Host stand-in for HipBackend in the time loop, without a device session: every dof follows its own tone on a slow
    carrier, so HiPassRun records on the host."""

    def __init__(self, desc):
        self.n = 6 * int(desc["num_nodes"]) + len(desc["coords"])
        rng = np.random.default_rng(5)
        self.f, self.ph = rng.uniform(40.0, 400.0, self.n), rng.uniform(0, 6.28, self.n)
        self.U = np.zeros(self.n)
        self.steps = 0
        self.states = []

    def set_dirichlet_values(self, v): pass
    def set_interface_pressure(self, P): pass
    def shift(self): pass
    def set_state(self, which, x): self.U[:] = x

    def newton_solve(self, **kw):
        self.steps += 1
        t = 1e-3 * self.steps
        self.U = 1e-3 * np.sin(2 * np.pi * 1.5 * t + self.ph) + 1e-6 * np.sin(2 * np.pi * self.f * t + self.ph)
        self.states.append(self.U.copy())
        return [(1e-8, 1e-9, False, 2, 1e-9)]

    def get_state(self, which, out=None):
        out[:] = self.U
        return out


def _stub_run(folder, extra, T="0.039", save_deg="2"):
    from vasp_amd import monolithic
    lines = []
    with contextlib.redirect_stdout(io.StringIO()):
        ns = monolithic.run(["-p", "cylinder", "-dt", "0.001", "-T", T, "--theta", "0.51", "--folder", str(folder), "--sub-folder", "1",
                             "--save-step", "1", "--save-deg", save_deg, "--verbose", "False", "--new-arguments", f"mesh_path={CYL}",
                             *extra], backend_factory=_Stub, out=lines.append)
    return ns, lines


def _vectors(path):
    from vasp_amd.h5lite import read_h5
    g = read_h5(path)["VisualisationVector"]
    return np.stack([np.asarray(g[str(k)].data) for k in range(len(g.keys()))])


@pytest.mark.parametrize("save_deg", ["1", "2"])
def test_driver_writes_the_restatement_of_the_saved_frames(tmp_path, save_deg):
    from vasp_amd.h5lite import read_h5
    ns, lines = _stub_run(tmp_path, ["--hi-pass", "d", "v", "p", "--hi-pass-amplitude", "--hi-pass-window", "8",
                                     "--hi-pass-bands", "25", "1000", "0", "200"], save_deg=save_deg)
    mesh, states = ns["mesh"], np.stack(ns["backend"].states)
    assert len(states) == 40
    out = tmp_path / "1" / "Visualization_hi_pass"
    viz = read_h5(tmp_path / "1" / "Visualization" / "velocity.h5")
    assert any("Hi-pass fields of 40 frames (d, v, p)" in line for line in lines)
    N2, V = mesh.num_nodes, mesh.num_vertices
    nn = N2 if save_deg == "2" else V
    e = mesh.edges
    for q, name in hp.VIZ_TYPE.items():
        if q == "p":
            x = states[:, 6 * N2:]
            if save_deg == "2":
                x = np.concatenate([x, 0.5 * (x[:, e[:, 0]] + x[:, e[:, 1]])], axis=1)
            x = x[:, :, None]
        else:
            off = 0 if q == "d" else 3 * N2
            x = states[:, off:off + 3 * N2].reshape(40, N2, 3)[:, :nn]
        for lo, hi in ((25.0, 1000.0), (0.0, 200.0)):
            prm = hp.design(1e-3, lo, hi)
            y = hp.filtfilt_rows(prm["b"], prm["a"], x)
            got = _vectors(out / f"{name}_{prm['name']}.h5")
            assert got.dtype == np.float32 and got.shape == x.shape and np.array_equal(got, y.astype(np.float32)), (q, lo)
            amp = y if lo < 0.1 else hp.windowed_rms_running(y, 8)
            assert np.array_equal(_vectors(out / f"{name}_{prm['name']}_amplitude.h5"), amp.astype(np.float32)), (q, lo)
            table = np.loadtxt(out / f"{name}_{prm['name']}.csv", delimiter=",")
            mag = np.stack([hp.amplitude_magnitude(a) for a in amp])
            assert table.shape == (40, 13)
            np.testing.assert_allclose(table[:, 0], np.arange(40) * 1e-3, rtol=1e-15, atol=0)
            assert np.array_equal(table[:, 3], mag.max(axis=1)) and np.array_equal(table[:, 12], mag.argmax(axis=1))
            assert np.array_equal(table[:, 5], np.percentile(mag, 50, axis=1))
            text = (out / f"{name}_{prm['name']}.xdmf").read_text()
            assert text == hp.xdmf_text(40, 1e-3, 0.0, len(np.asarray(viz["Mesh"]["0"]["mesh"]["topology"].data)), nn,
                                        "Scalar" if q == "p" else "Vector", f"{name}_{prm['name']}")
        g = read_h5(out / f"{name}_25_to_1000.h5")["Mesh"]["0"]["mesh"]
        assert np.array_equal(np.asarray(g["geometry"].data), np.asarray(viz["Mesh"]["0"]["mesh"]["geometry"].data).astype(np.float32))
        assert np.array_equal(np.asarray(g["topology"].data), np.asarray(viz["Mesh"]["0"]["mesh"]["topology"].data))


def test_without_amplitude_only_the_filtered_fields_are_written(tmp_path):
    _stub_run(tmp_path, ["--hi-pass", "v"])
    names = sorted(p.name for p in (tmp_path / "1" / "Visualization_hi_pass").iterdir())
    assert names == ["velocity_25_to_1000.h5", "velocity_25_to_1000.xdmf"]
    ns, _ = _stub_run(tmp_path / "plain", [])
    assert not (tmp_path / "plain" / "1" / "Visualization_hi_pass").exists()


def test_killturtle_stop_writes_what_the_recorded_frames_allow(tmp_path):
    """Stopped after one step: one frame is fewer than padlen + 1 - a log line, no file, no exception."""
    (tmp_path / "1").mkdir(parents=True)
    (tmp_path / "1" / "killturtle").write_text("")
    ns, lines = _stub_run(tmp_path, ["--hi-pass", "v"])
    assert ns["backend"].steps == 1
    assert any("1 frames recorded, the filter needs more than 33: nothing written" in line for line in lines)
    assert list((tmp_path / "1" / "Visualization_hi_pass").glob("*.h5")) == []


# ---- the C-ABI --------------------------------------------------------------------------------------------------------

BAND_CALLS = ("fsi_band_begin", "fsi_band_sample", "fsi_band_filter", "fsi_band_amplitude", "fsi_band_fetch", "fsi_band_end")


def test_header_and_binding_agree_on_the_band_entry_points():
    from vasp_amd import capi
    header = (ROOT / "include" / "vaspfsi.h").read_text()
    lib = capi.load_library()
    for name in BAND_CALLS:
        m = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S)
        assert m, name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
        # every call names the reference lines it replaces
        doc = header[:m.start()].rsplit("/*", 1)[1]
        assert "REF" in doc or name == "fsi_band_end", name
    for k, what in enumerate(("RAW", "FILTERED", "AMPLITUDE", "MAGNITUDE")):
        assert re.search(r"#define FSI_BAND_%s %d\b" % (what, k), header)
        assert capi.HipBackend.BAND_WHAT[what.lower()] == k
    for meth in ("hi_pass_begin", "hi_pass_sample", "hi_pass_filter", "hi_pass_amplitude", "hi_pass_fetch", "hi_pass_end"):
        assert hasattr(capi.HipBackend, meth)
    src = (ROOT / "vasp_amd" / "csrc" / "fsi_band.hip").read_text()
    assert "#pragma clang fp contract(off)" in src
    assert int(re.search(r"BAND_RMS_REFRESH = (\d+)", (ROOT / "vasp_amd" / "csrc" / "fsi_band.hpp").read_text()).group(1)) == hp.RMS_REFRESH
