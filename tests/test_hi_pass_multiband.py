"""Host side of the multiband cascades, the frame window and stride and the point traces of --hi-pass (vasp_amd/hi_pass.py):
the staged restatement against scipy, the band-stop design, the pass / stop rule and its file name, the host session's
select / filter_next / trace, the refusals, the driver without a device session, and the C-ABI's new entry points."""
import re

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_hi_pass import _signal
from test_hi_pass import _refusal, _stub_run, _vectors
from vasp_amd import hi_pass as hp

DT = 1e-3
CASCADE = ((25.0, 450.0, "bandpass"), (100.0, 150.0, "bandstop"), (200.0, 230.0, "bandstop"))


def _staged(x, dt, stages):
    for lo, hi, btype in stages:
        prm = hp.design(dt, lo, hi, btype)
        x = hp.filtfilt_rows(prm["b"], prm["a"], x, prm["zi"], prm["padlen"])
    return x


# ---- the filter -------------------------------------------------------------------------------------------------------

def test_staged_restatement_equals_staged_scipy_filtfilt_exactly():
    """fs = 999: pass 25 - 450, stop 100 - 150, stop 200 - 230 on 72 frames x 300 rows; after every stage each row equals
    scipy.signal.filtfilt of the previous stage's row bit for bit."""
    from scipy.signal import filtfilt
    x = _signal(300)
    assert x.shape == (72, 300)
    ref = x
    for lo, hi, btype in CASCADE:
        prm = hp.design(DT, lo, hi, btype)
        assert len(prm["b"]) == len(prm["a"]) == 11 and prm["padlen"] == 33 and prm["a"][0] == 1.0
        x = hp.filtfilt_rows(prm["b"], prm["a"], x, prm["zi"], prm["padlen"])
        ref = np.stack([filtfilt(prm["b"], prm["a"], ref[:, r]) for r in range(ref.shape[1])], axis=1)
        assert np.array_equal(x, ref), (lo, hi)
    assert np.array_equal(x, _staged(_signal(300), DT, CASCADE))


def test_band_stop_design_is_scipys():
    from scipy.signal import butter, lfilter_zi
    prm = hp.design(DT, 100.0, 150.0, btype="bandstop")
    b, a = butter(hp.ORDER, [100.0 / 499.5, 150.0 / 499.5], btype="bandstop")
    assert np.array_equal(prm["b"], b) and np.array_equal(prm["a"], a) and np.array_equal(prm["zi"], lfilter_zi(b, a))
    assert (prm["btype"], prm["padlen"], prm["name"], prm["fs"]) == ("bandstop", 33, "100_to_150", 999)
    # a stage that passes: the band as it is, a band-pass even below 0.1 Hz, where the single band turns low-pass
    prm = hp.design(DT, 0.05, 450.0, btype="bandpass")
    b, a = butter(hp.ORDER, [0.05 / 499.5, 450.0 / 499.5], btype="bandpass")
    assert np.array_equal(prm["b"], b) and np.array_equal(prm["a"], a) and prm["btype"] == "bandpass"
    assert hp.design(DT, 0.05, 450.0)["btype"] == "lowpass"
    # without btype nothing changed: the clipped band-pass
    b, a = butter(hp.ORDER, [25.0 / 499.5, 499.0 / 499.5], btype="bandpass")
    assert np.array_equal(hp.design(DT, 25.0, 1000.0)["b"], b) and np.array_equal(hp.design(DT, 25.0, 1000.0, None)["a"], a)
    # a stage is not clipped: scipy would raise for Wn >= 1, the band and fs / 2 are named instead
    for lo, hi in ((25.0, 1000.0), (25.0, 499.5), (0.0, 200.0), (200.0, 100.0)):
        with pytest.raises(ValueError, match=r"band %g - %g Hz cannot be a stage.* fs / 2 = 499.5 Hz" % (lo, hi)):
            hp.design(DT, lo, hi, btype="bandstop")
    with pytest.raises(ValueError, match="btype must be"):
        hp.design(DT, 25.0, 100.0, btype="highpass")


def test_pass_stop_rule_override_and_chained_name():
    bands = [(25.0, 10000.0), (100.0, 150.0), (1000.0, 2000.0), (0.0, 1000.4)]
    assert hp.pass_stop_list(bands) == ["pass", "stop", "stop", "pass"]                 # wider than 1000 Hz passes
    assert hp.pass_stop_list(bands[:2], ["stop", "pass"]) == ["stop", "pass"]
    assert hp.multiband_name("velocity", [(25.0, 10000.0), (99.6, 150.4)], ["pass", "stop"]) == "velocity_pass_25_to_10000_stop_100_to_150"
    with pytest.raises(SystemExit, match="one word per band: 1 words for 2 bands"):
        hp.pass_stop_list(bands[:2], ["pass"])
    with pytest.raises(SystemExit, match=r"the words pass and stop, got \['band'\]"):
        hp.pass_stop_list(bands[:2], ["pass", "band"])
    v = {"hi_pass_bands": [25, 450, 100, 150], "hi_pass_multiband": True}
    assert hp.multiband(v) == ["stop", "stop"] and hp.multiband(dict(v, hi_pass_pass_stop=["pass", "stop"])) == ["pass", "stop"]
    assert hp.multiband({"hi_pass_bands": [25, 450, 100, 150]}) == []
    with pytest.raises(SystemExit, match="at least two bands in --hi-pass-bands, got 1"):
        hp.multiband({"hi_pass_bands": [25, 450], "hi_pass_multiband": True})
    with pytest.raises(SystemExit, match="belongs to --hi-pass-multiband"):
        hp.multiband({"hi_pass_bands": [25, 450, 100, 150], "hi_pass_pass_stop": ["pass", "stop"]})


def test_options_from_the_command_line():
    from vasp_amd.monolithic import parse
    a = parse(["--hi-pass", "v", "--hi-pass-bands", "25", "450", "100", "150", "--hi-pass-multiband", "--hi-pass-pass-stop", "pass", "stop",
               "--hi-pass-stride", "2", "--hi-pass-start-time", "0.02", "--hi-pass-end-time", "0.15", "--hi-pass-point-ids", "0", "5"])
    assert a["hi_pass_multiband"] is True and a["hi_pass_pass_stop"] == ["pass", "stop"] and a["hi_pass_point_ids"] == [0, 5]
    assert hp.frame_window(a) == (2, 0.02, 0.15) and hp.point_ids(a) == [0, 5] and hp.multiband(a) == ["pass", "stop"]
    assert hp.frame_window({}) == (1, 0.0, None) and hp.point_ids({}) == [] and hp.multiband({}) == []
    assert not any(k.startswith("hi_pass") for k in parse([]))


def test_frame_selection():
    times = [1e-3 * (k + 1) for k in range(41)]
    assert hp.select_frames(times, 1e-3, 1, 0.0, None) == (0, 41)                        # the defaults keep every frame
    assert hp.select_frames(times, 1e-3, 2, 0.0, None) == (0, 21)
    assert hp.select_frames(times, 1e-3, 3, 0.0105, 0.03) == (12, 6)                     # k = 12, 15, .., 27: t = 0.013 .. 0.028
    assert hp.select_frames(times, 1e-3, 1, 0.005, 0.005) == (4, 1)                      # t_4 = 0.005 up to rounding
    assert hp.select_frames(times, 1e-3, 1, 0.05, None) == (0, 0)
    assert hp.saved_times(dict(dt=0.001, T=0.005, save_step=2)) == pytest.approx([0.001, 0.003, 0.005])
    assert hp.expected_frames(dict(dt=0.001, T=0.04, save_step=1)) == 41


# ---- the host session ---------------------------------------------------------------------------------------------------

def test_host_session_select_filter_next_and_trace_against_numpy_slicing():
    x = _signal(30, frames=90, seed=3).reshape(90, 10, 3)
    s = hp.HostBandSession(3, 90)
    for f in x:
        s.sample(f)
    stages = [hp.design(DT, *st) for st in CASCADE[:2]]
    with pytest.raises(RuntimeError, match="no filtered series"):
        s.filter_next(*(stages[1][k] for k in ("b", "a", "zi", "padlen")))
    for first, count, stride in ((0, -1, 1), (1, -1, 2), (5, 40, 2), (0, 90, 1), (3, 1, 50)):
        n = s.select(first, count, stride)
        sel = x[first::stride][:count] if count != -1 else x[first::stride]
        assert n == len(sel)
        with pytest.raises(RuntimeError, match="no filtered series"):
            s.trace("filtered", [0])
        raw = s.trace("raw", [0, 9, 0])
        assert raw.shape == (3, n, 4) and np.array_equal(raw[0], raw[2])
        assert np.array_equal(raw[1, :, 1:], sel[:, 9]) and np.array_equal(raw[1, :, 0], np.linalg.norm(sel[:, 9], axis=1))
        assert np.array_equal(s.fetch("raw", first), x[first])                           # a raw fetch stays absolute
        if n <= 33:
            with pytest.raises(ValueError, match="greater than padlen"):
                s.filter(*(stages[0][k] for k in ("b", "a", "zi", "padlen")))
            continue
        s.filter(*(stages[0][k] for k in ("b", "a", "zi", "padlen")))
        s.filter_next(*(stages[1][k] for k in ("b", "a", "zi", "padlen")))
        y = _staged(sel, DT, CASCADE[:2])
        assert np.array_equal(np.stack([s.fetch("filtered", k) for k in range(n)]), y)
        assert np.array_equal(s.trace("filtered", [4])[0, :, 1:], y[:, 4])
        s.amplitude(8)
        assert np.array_equal(s.fetch("amplitude", n // 2), hp.windowed_rms_running(y, 8)[n // 2])
    for bad in ((0, -1, 0), (90, -1, 1), (0, 46, 2), (-1, -1, 1), (0, 0, 1)):
        with pytest.raises(RuntimeError, match="first \\+ \\(count - 1\\) \\* stride < the 90 recorded frames"):
            s.select(*bad)
    for bad in ([10], [-1]):
        with pytest.raises(RuntimeError, match="node out of range"):
            s.trace("raw", bad)
    p =hp.HostBandSession(1, 4)                                                         # a scalar: the magnitude is the value
    for k in range(4):
        p.sample(np.arange(5.0) - k)
    assert p.select(1, -1, 2) == 2
    t = p.trace("raw", [0, 4])
    assert t.shape == (2, 2, 2) and np.array_equal(t[1, :, 0], [3.0, 1.0]) and np.array_equal(t[..., 0], t[..., 1])
    p2 = hp.HostBandSession(1, 4)
    p2.sample(np.zeros(5))
    p2.select(0, 1, 1)
    p2.sample(np.zeros(5))                                                               # a new frame resets the selection
    assert p2.trace("raw", [0]).shape == (1, 2, 2)


# ---- the refusals -------------------------------------------------------------------------------------------------------

def test_each_new_refusal_has_its_message():
    ok = ["-dt", "0.001", "-T", "0.099", "--save-step", "1", "--hi-pass-bands", "25", "450", "100", "150"]           # 100 frames
    multi = ok + ["--hi-pass-multiband", "--hi-pass-pass-stop", "pass", "stop"]
    assert _refusal(ok) == "" and _refusal(multi) == "" and _refusal(ok + ["--hi-pass-multiband"]) == ""
    assert _refusal(multi + ["--hi-pass-stride", "1", "--hi-pass-start-time", "0.01", "--hi-pass-point-ids", "0", "7"]) == ""
    # the selected frames count, not the saved ones
    msg = _refusal(ok + ["--hi-pass-stride", "3"])                                       # k = 0, 3, .., 99: 34 frames
    assert msg == ""
    msg = _refusal(ok + ["--hi-pass-stride", "4"])
    assert "saves 25 frames in the window and stride asked for" in msg and "padlen + 1 = 34" in msg
    msg = _refusal(ok + ["--hi-pass-start-time", "0.05", "--hi-pass-end-time", "0.08"])
    assert "saves 31 frames in the window and stride asked for" in msg and "padlen + 1 = 34" in msg
    msg = _refusal(ok + ["--hi-pass-stride", "2", "--hi-pass-amplitude", "--hi-pass-window", "60"])
    assert "saves 50 frames in the window and stride asked for, fewer than the window of 60" in msg
    assert _refusal(ok + ["--hi-pass-stride", "2", "--hi-pass-amplitude", "--hi-pass-window", "50"]) == ""
    # a multiband stage is not clipped: fs / 2 of the strided frames
    msg = _refusal(multi[:6] + ["--hi-pass-bands", "25", "450", "100", "600", "--hi-pass-multiband"])
    assert "band 100 - 600 Hz cannot be a stage" in msg and "fs / 2 = 499.5 Hz" in msg
    msg = _refusal(multi + ["--hi-pass-stride", "2"])
    assert "band 25 - 450 Hz cannot be a stage" in msg and "fs / 2 = 249.5 Hz" in msg
    # a stage has 11 coefficients whatever the band: two low-pass bands (padlen 18 each) fit 30 frames, a cascade does not
    low = ["-dt", "0.001", "-T", "0.029", "--save-step", "1", "--hi-pass-bands", "0.05", "200", "0.05", "300"]
    assert _refusal(low) == ""
    assert "saves 30 frames, a stage needs at least padlen + 1 = 34" in _refusal(low + ["--hi-pass-multiband"])
    for extra, text in ((["--hi-pass-multiband"], "at least two bands in --hi-pass-bands, got 1"),):
        with pytest.raises(SystemExit, match=text):
            _refusal(ok[:6] + extra)
    for extra, text in ((["--hi-pass-multiband", "--hi-pass-pass-stop", "pass"], "one word per band: 1 words for 2 bands"),
                        (["--hi-pass-pass-stop", "pass", "stop"], "belongs to --hi-pass-multiband"),
                        (["--hi-pass-stride", "0"], "--hi-pass-stride must be an integer >= 1"),
                        (["--hi-pass-start-time", "0.05", "--hi-pass-end-time", "0.01"], "need 0 <= start <= end"),
                        (["--hi-pass-point-ids", "-1"], "indices >= 0")):
        with pytest.raises(SystemExit, match=text):
            _refusal(ok + extra)


def test_a_point_id_out_of_range_is_refused_before_the_time_loop(tmp_path):
    with pytest.raises(SystemExit, match=r"--hi-pass-point-ids: \[100000\] out of range, velocity is written on \d+ nodes"):
        _stub_run(tmp_path, ["--hi-pass", "v", "--hi-pass-point-ids", "3", "100000"])
    assert not (tmp_path / "1" / "Visualization_hi_pass").exists() and not (tmp_path / "1" / "Visualization_separate_domain").exists()


# ---- the driver, without a device session -------------------------------------------------------------------------------

def _rows_of(mesh, states, q):
    N2, e = mesh.num_nodes, mesh.edges
    if q == "p":
        x = states[:, 6 * N2:]
        return np.concatenate([x, 0.5 * (x[:, e[:, 0]] + x[:, e[:, 1]])], axis=1)[:, :, None]
    off = 0 if q == "d" else 3 * N2
    return states[:, off:off + 3 * N2].reshape(len(states), N2, 3)


def test_driver_with_all_new_options_writes_the_staged_restatement(tmp_path):
    """160 saved frames, every second one between t = 0.021 and 0.15: k = 20, 22, .., 148, 65 frames 2 ms apart (fs = 499)."""
    from vasp_amd.h5lite import read_h5
    flags = ["--hi-pass", "d", "v", "p", "--hi-pass-bands", "25", "200", "60", "90", "--hi-pass-multiband", "--hi-pass-pass-stop", "pass", "stop",
             "--hi-pass-stride", "2", "--hi-pass-start-time", "0.021", "--hi-pass-end-time", "0.15", "--hi-pass-point-ids", "0", "7",
             "--hi-pass-amplitude", "--hi-pass-window", "8"]
    ns, lines = _stub_run(tmp_path, flags, T="0.159")
    mesh, states = ns["mesh"], np.stack(ns["backend"].states)
    assert len(states) == 160
    n, dtf = 65, 2e-3
    assert any(f"Hi-pass fields of {n} frames (d, v, p)" in line for line in lines)
    out, traces = tmp_path / "1" / "Visualization_hi_pass", tmp_path / "1" / "Visualization_separate_domain"
    ncell = len(np.asarray(read_h5(tmp_path / "1" / "Visualization" / "velocity.h5")["Mesh"]["0"]["mesh"]["topology"].data))
    times = 0.021 + np.arange(n) * dtf
    for q, name in hp.VIZ_TYPE.items():
        x = _rows_of(mesh, states, q)[20:149:2]
        assert len(x) == n
        series = {f"{name}_25_to_200": _staged(x, dtf, [(25.0, 200.0, None)]), f"{name}_60_to_90": _staged(x, dtf, [(60.0, 90.0, None)]),
                  f"{name}_pass_25_to_200_stop_60_to_90": _staged(x, dtf, [(25.0, 200.0, "bandpass"), (60.0, 90.0, "bandstop")])}
        for viz, y in series.items():
            got = _vectors(out / f"{viz}.h5")
            assert got.dtype == np.float32 and np.array_equal(got, y.astype(np.float32)), viz
            amp = hp.windowed_rms_running(y, 8)                        # a cascade's amplitude is the windowed RMS, as a band-pass's
            assert np.array_equal(_vectors(out / f"{viz}_amplitude.h5"), amp.astype(np.float32)), viz
            table = np.loadtxt(out / f"{viz}.csv", delimiter=",")
            assert table.shape == (n, 13)
            np.testing.assert_allclose(table[:, 0], times, rtol=1e-15, atol=0)
            mag = np.stack([hp.amplitude_magnitude(a) for a in amp])
            assert np.array_equal(table[:, 3], mag.max(axis=1)) and np.array_equal(table[:, 12], mag.argmax(axis=1))
            for v in (viz, f"{viz}_amplitude"):
                assert (out / f"{v}.xdmf").read_text() == hp.xdmf_text(n, dtf, 0.021, ncell, mesh.num_nodes, "Scalar" if q == "p" else "Vector", v)
        text = (out / f"{name}_pass_25_to_200_stop_60_to_90.xdmf").read_text()
        assert re.findall(r'<Time Value="(.*?)" />', text)[:3] == ["0.021", "0.023", "0.025"]
        # the traces: the recorded rows, not filtered; one time per frame
        for i in (0, 7):
            lines_csv = (traces / f"{name}_point_id_{i}.csv").read_text().splitlines()
            data = np.loadtxt(traces / f"{name}_point_id_{i}.csv", delimiter=",")
            if q == "p":
                assert lines_csv[0] == "# time (s), Magnitude" and data.shape == (n, 2)
                assert np.array_equal(data[:, 1], x[:, i, 0])
            else:
                assert lines_csv[0] == "# time (s), Magnitude, X Component, Y Component, Z Component" and data.shape == (n, 5)
                assert np.array_equal(data[:, 2:], x[:, i]) and np.array_equal(data[:, 1], hp.amplitude_magnitude(x[:, i]))
            np.testing.assert_allclose(data[:, 0], times, rtol=1e-15, atol=0)
        assert not list(traces.glob("*.png"))
    assert len(list(out.glob("*.h5"))) == 3 * 3 * 2 and len(list(traces.iterdir())) == 6


def test_a_run_with_only_the_old_options_writes_what_it_wrote_before(tmp_path):
    """The datasets and texts of tests/test_hi_pass.py's run, and the same again when the new options are given their defaults."""
    from test_gpu_hi_pass import _files
    old = ["--hi-pass", "v", "p", "--hi-pass-amplitude", "--hi-pass-window", "8", "--hi-pass-bands", "25", "1000", "0", "200"]
    ns, _ = _stub_run(tmp_path / "old", old)
    mesh, states = ns["mesh"], np.stack(ns["backend"].states)
    out = tmp_path / "old" / "1" / "Visualization_hi_pass"
    for q in "vp":
        x, name = _rows_of(mesh, states, q), hp.VIZ_TYPE[q]
        for lo, hi in ((25.0, 1000.0), (0.0, 200.0)):
            prm = hp.design(DT, lo, hi)
            y = hp.filtfilt_rows(prm["b"], prm["a"], x)
            assert np.array_equal(_vectors(out / f"{name}_{prm['name']}.h5"), y.astype(np.float32))
            amp = y if lo < 0.1 else hp.windowed_rms_running(y, 8)
            assert np.array_equal(_vectors(out / f"{name}_{prm['name']}_amplitude.h5"), amp.astype(np.float32))
            np.testing.assert_allclose(np.loadtxt(out / f"{name}_{prm['name']}.csv", delimiter=",")[:, 0], np.arange(40) * 1e-3, rtol=1e-15, atol=0)
    assert not (tmp_path / "old" / "1" / "Visualization_separate_domain").exists()
    assert sorted(p.name for p in out.iterdir()) == sorted(f"{name}_{band}{kind}" for name in ("velocity", "pressure") for band in ("25_to_1000", "0_to_200")
                                                           for kind in (".h5", ".xdmf", ".csv", "_amplitude.h5", "_amplitude.xdmf"))
    _stub_run(tmp_path / "same", old + ["--hi-pass-stride", "1", "--hi-pass-start-time", "0"])
    assert _files(tmp_path / "same" / "1" / "Visualization_hi_pass") == _files(out)


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------

def test_header_and_binding_agree_on_the_new_entry_points():
    from vasp_amd import capi
    header = (ROOT / "include" / "vaspfsi.h").read_text()
    lib = capi.load_library()
    for name in ("fsi_band_select", "fsi_band_filter_next", "fsi_band_trace"):
        m = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S)
        assert m, name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
        assert "REF" in header[:m.start()].rsplit("/*", 1)[1], name                      # the reference lines it replaces
    for meth in ("hi_pass_select", "hi_pass_filter_next", "hi_pass_trace"):
        assert hasattr(capi.HipBackend, meth)
    for meth in ("select", "filter_next", "trace"):
        assert hasattr(hp.HostBandSession, meth)
    src = (ROOT / "vasp_amd" / "csrc" / "fsi_band.hip").read_text()
    assert "k_band_filter_next" in src and "k_band_trace" in src and src.count("#pragma clang fp contract(off)") == 1
    assert src.index("#pragma clang fp contract(off)") < src.index("k_band_filter_next(")
