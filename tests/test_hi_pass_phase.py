"""Phase-averaged fields and the turbulent kinetic energy under ``--hi-pass-phase-average``, host side: the NumPy twin of
csrc/fsi_phase.hip (``HostBandSession.phase`` / ``phase_fetch``) against what the reference's own ``compute_tke`` and
``compute_average_over_cycles`` returned (tests/golden/tke/compute_tke.npz, written by tests/golden/make_tke.py), the period
arithmetic with its refusals, and the driver's files with a stub backend - whole, cut by a checkpoint and continued."""
import contextlib
import io
import re
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_session_restart import CYL, SPLIT, _restart, _run, one_modification_time  # noqa: F401  (the fixture holds h5lite's clock)
from vasp_amd import hi_pass as hp

GOLD = np.load(GOLDEN / "tke" / "compute_tke.npz")
CASES = ((4, 3), (1, 5), (5, 1), (3, 11))        # tests/golden/make_tke.py
RANGE = (4, 6, 2, 4)


def same_bits(a, b) -> bool:
    """Equal values with NaN equal to NaN, and equal signs of the zeros."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[a == 0]), np.signbit(b[b == 0]))


def _session(u, ncomp=3):
    s = hp.HostBandSession(ncomp, len(u))
    for frame in u:
        s.sample(frame)
    return s


def _all(s, period, n):
    return dict(mean=np.stack([s.phase_fetch("mean", j) for j in range(period)]),
                fluct=np.stack([s.fetch("filtered", k) for k in range(n)]),
                tke=np.stack([s.phase_fetch("energy", k) for k in range(n)]),
                tke_cycle_mean=np.stack([s.phase_fetch("energy_cycle_mean", j) for j in range(period)]),
                tke_time_mean=s.phase_fetch("energy_time_mean", 0))


# ---- the twin against the reference's functions -------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(CASES)))
def test_twin_equals_compute_tke_bit_for_bit(i):
    period, cycles = CASES[i]
    u = GOLD[f"u{i}"]
    assert u.shape == (period * cycles, 5, 3) and np.signbit(u[0, 0, 0]) and np.isnan(u).any() and np.isinf(u).any()
    s = _session(u)
    s.phase(period)
    for key, got in _all(s, period, len(u)).items():
        assert same_bits(got, GOLD[f"{key}{i}"]), key
    assert np.array_equal(s.fetch("raw", len(u) - 1), u[-1], equal_nan=True)
    if cycles == 1:        # one cycle is its own mean: the fluctuation is exactly +0 where it is finite (-0 - +0 = -0 for the one -0.0)
        f = np.stack([s.fetch("filtered", k) for k in range(len(u))])
        finite = np.isfinite(f)
        assert not f[finite].any() and np.signbit(f[finite]).sum() == 1 and np.signbit(f[0, 0, 0])


def test_a_cycle_range_inside_a_longer_record():
    period, cycles, c0, c1 = RANGE
    u = GOLD["u_range"]
    s = _session(u)
    n = (c1 - c0 + 1) * period
    assert s.select((c0 - 1) * period, n, 1) == n
    s.phase(period)
    got = _all(s, period, n)
    lo, hi = (c0 - 1) * period, c1 * period      # the reference leaves zeros outside the range: only the cycles in range compare
    assert same_bits(got["mean"], GOLD["mean_range"])
    assert same_bits(got["fluct"], GOLD["fluct_range"][lo:hi]) and same_bits(got["tke"], GOLD["tke_range"][lo:hi])
    assert same_bits(got["tke_cycle_mean"], GOLD["tke_cycle_mean_range"]) and same_bits(got["tke_time_mean"], GOLD["tke_time_mean_range"])


def test_a_strided_view_a_scalar_and_the_amplitude_of_the_fluctuation():
    rng = np.random.default_rng(3)
    u = rng.standard_normal((26, 7, 1))
    s = _session(u, 1)
    assert s.select(2, 12, 2) == 12
    s.phase(4)
    x = u[2:26:2]
    mean = ((0.0 + x[0:4]) + x[4:8] + x[8:12]) / 3.0
    assert np.array_equal(np.stack([s.phase_fetch("mean", j) for j in range(4)]), mean)
    f = x - np.tile(mean, (3, 1, 1))
    assert np.array_equal(np.stack([s.fetch("filtered", k) for k in range(12)]), f)
    assert np.array_equal(s.phase_fetch("energy", 5), 0.5 * (f[5, :, 0] * f[5, :, 0]))
    s.amplitude(4)
    assert np.array_equal(np.stack([s.fetch("amplitude", k) for k in range(12)]), hp.windowed_rms_running(f, 4))
    assert np.array_equal(s.trace("filtered", [6, 0])[:, :, 1], f[:, [6, 0], 0].T)


def test_twin_refusals_and_invalidation():
    u = np.random.default_rng(4).standard_normal((12, 3, 3))
    s = _session(u)
    with pytest.raises(RuntimeError, match=r"no phase average \(phase first\)"):
        s.phase_fetch("mean", 0)
    for bad in (0, -1, 5, 24):
        with pytest.raises(RuntimeError, match=rf"period = {bad} frames, 12 selected frames"):
            s.phase(bad)
    assert s.filtered is None                     # a refused call left the session as it was
    s.phase(4)
    for what, frame in (("mean", 4), ("energy", 12), ("energy_cycle_mean", 4), ("energy_time_mean", 1), ("mean", -1)):
        with pytest.raises(RuntimeError, match="out of range"):
            s.phase_fetch(what, frame)
    with pytest.raises(RuntimeError, match="what must be one of"):
        s.phase_fetch("filtered", 0)
    for undo in (lambda: s.select(0, 12, 1), lambda: s.sample(u[0]), lambda: s.import_(u[:1]),
                 lambda: s.filter(np.array([1.0, 0.0]), np.array([1.0, 0.0]), np.zeros(1), 0),
                 lambda: s.filter_next(np.array([1.0, 0.0]), np.array([1.0, 0.0]), np.zeros(1), 0)):
        s = _session(u)
        s.capacity = 13
        s.phase(4)
        undo()
        with pytest.raises(RuntimeError, match="no phase average"):
            s.phase_fetch("mean", 0)
    tensor = _session(np.zeros((4, 2, 6)), 6)
    tensor.phase(2)
    assert tensor.phase_fetch("mean", 1).shape == (2, 6)
    with pytest.raises(RuntimeError, match="strain / stress session has no energy"):
        tensor.phase_fetch("energy", 0)


# ---- the period arithmetic and the refusals before a run ------------------------------------------------------------------

def _parameters(extra):
    from vasp_amd.monolithic import parameters
    with contextlib.redirect_stdout(io.StringIO()):
        return parameters(["-p", "cylinder", "--hi-pass", "v", "--verbose", "False", "-dt", "0.001", "--save-step", "1", *extra])[2]


def _refusal(extra):
    return hp.hi_pass_refusal(_parameters(extra), 1, None)


def test_period_arithmetic():
    assert hp.phase_period(0.951, 1e-3) == 951 and hp.phase_period(0.004, 1e-3) == 4 and hp.phase_period(1e-3, 1e-3) == 1
    assert hp.phase_period(0.951 * (1 + 5e-7), 1e-3) == 951                      # within 1e-6 relative of a whole number
    for cycle, dt in ((0.0045, 1e-3), (0.951 * (1 + 3e-6), 1e-3), (4e-4, 1e-3)):
        with pytest.raises(SystemExit) as e:
            hp.phase_period(cycle, dt)
        assert repr(cycle) in str(e.value) and repr(cycle / dt) in str(e.value) and "not a whole number" in str(e.value)
    assert hp.phase_cycles({}, 4, 12) == (1, 3) and hp.phase_cycles({}, 4, 15) == (1, 3) and hp.phase_cycles({}, 5, 5) == (1, 1)
    assert hp.phase_cycles(dict(hi_pass_start_cycle=2, hi_pass_end_cycle=2), 4, 12) == (2, 2)
    assert hp.phase_cycles(dict(hi_pass_start_cycle=2), 4, 14) == (2, 3)
    assert hp.phase_cycle({}) is None
    assert hp.phase_cycle(dict(hi_pass_phase_average=True, T_Cycle=0.951)) == 0.951
    assert hp.phase_cycle(dict(hi_pass_phase_average=True, T_Cycle=0.951, hi_pass_cycle=0.5)) == 0.5


def test_each_refusal_has_its_message():
    on = ["--hi-pass-phase-average"]
    assert _refusal(["-T", "0.0115", *on, "--hi-pass-cycle", "0.004"]) == ""      # 12 frames: no band has enough, the phase average has
    assert "padlen + 1 = 34" in _refusal(["-T", "0.0115"])                         # without the option nothing has changed
    assert _refusal(["-T", "0.0235", *on, "--hi-pass-cycle", "0.008", "--hi-pass-stride", "2"]) == ""        # 4 selected frames a cycle
    msg = _refusal(["-T", "0.0115", *on, "--hi-pass-cycle", "0.0045"])
    assert "a cycle of 0.0045 s is 4.5 frames of 0.001 s" in msg and "not a whole number" in msg
    msg = _refusal(["-T", "0.0235", *on, "--hi-pass-cycle", "0.005", "--hi-pass-stride", "2"])
    assert "is 2.5 frames of 0.002 s" in msg
    msg = _refusal(["-T", "0.0025", *on, "--hi-pass-cycle", "0.004"])
    assert "hold 3 frames, fewer than one whole cycle of 4" in msg
    for extra in (["--hi-pass-start-cycle", "0"], ["--hi-pass-end-cycle", "4"], ["--hi-pass-start-cycle", "3", "--hi-pass-end-cycle", "2"]):
        msg = _refusal(["-T", "0.0115", *on, "--hi-pass-cycle", "0.004", *extra])
        assert "need 1 <= start <= end <= 3, the whole cycles of 4 frames among the 12 frames" in msg, extra
    assert _refusal(["-T", "0.0115", *on, "--hi-pass-cycle", "0.004", "--hi-pass-start-cycle", "2", "--hi-pass-end-cycle", "3"]) == ""
    v = _parameters(["-T", "0.0115", *on])
    if v.get("T_Cycle") is None:                  # the problem gives no cycle length: refused before the run
        with pytest.raises(SystemExit, match="needs the length of a cycle: give --hi-pass-cycle"):
            hp.hi_pass_refusal(v, 1, None)
    with pytest.raises(SystemExit, match="needs the length of a cycle"):
        hp.hi_pass_refusal({**v, "T_Cycle": None}, 1, None)
    assert hp.hi_pass_refusal({**v, "T_Cycle": 0.004}, 1, None) == ""              # the resolved parameters' T_Cycle is the default
    with pytest.raises(SystemExit, match="--hi-pass-cycle belongs to --hi-pass-phase-average"):
        _refusal(["-T", "0.039", "--hi-pass-cycle", "0.004"])
    with pytest.raises(SystemExit, match="must be a number of seconds > 0"):
        _refusal(["-T", "0.0115", *on, "--hi-pass-cycle", "-1"])


def test_a_history_in_strips_refuses_the_option(tmp_path):
    from vasp_amd.mesh import FsiMesh
    mesh = FsiMesh.read(CYL)
    ns = dict(_parameters(["-T", "0.0115", "--hi-pass-phase-average", "--hi-pass-cycle", "0.004"]), save_deg=2, results_folder=tmp_path,
              hi_pass_strip=(0, 8))
    with pytest.raises(SystemExit) as e:
        hp.HiPassRun(object(), mesh, ns)
    assert str(e.value) == hp.PHASE_STRIPS and "strips of rows" in str(e.value)
    assert not (tmp_path / "Visualization_hi_pass").exists()


# ---- the driver with a stub backend -------------------------------------------------------------------------------------

PHASE = ["--hi-pass-phase-average", "--hi-pass-cycle", "0.004"]


def _vectors(path):
    from vasp_amd.h5lite import read_h5
    g = read_h5(path)["VisualisationVector"]
    return np.stack([np.asarray(g[str(k)].data) for k in range(len(g.keys()))])


def _times(path):
    return [float(t) for t in re.findall(r'<Time Value="([^"]+)"', path.read_text())]


def _frames(results, name):
    from vasp_amd.h5lite import read_h5
    g = read_h5(results / "Visualization" / f"{name}.h5")["VisualisationVector"]
    return np.stack([np.asarray(g[str(k)].data) for k in range(len(g.keys()))])


def test_driver_writes_the_phase_average_of_the_saved_frames(tmp_path):
    """14 saved frames, every one selected: three whole cycles of 4 and two frames over.  Cycles 2 to 3 with a second run."""
    options = ["--hi-pass", "v", "p", "--hi-pass-amplitude", "--hi-pass-window", "4", "--hi-pass-point-ids", "0", "5", *PHASE]
    ns, lines = _run(tmp_path / "case", T="0.0135", options=options)
    results = tmp_path / "case" / "1"
    out, sep = results / "Visualization_hi_pass", results / "Visualization_separate_domain"
    assert any("Hi-pass velocity: phase average over cycles 1 to 3 of 4 frames written" in line for line in lines)
    assert any("14 frames recorded, the filter needs more than 33: nothing written" in line for line in lines)      # the default band
    names = {p.name for p in out.iterdir()}
    stems = {"velocity_phase_mean": 4, "velocity_fluctuation": 12, "velocity_fluctuation_amplitude": 12, "velocity_tke": 12,
             "velocity_tke_phase_mean": 4, "velocity_tke_avg": 1, "pressure_phase_mean": 4, "pressure_fluctuation": 12,
             "pressure_fluctuation_amplitude": 12}
    assert names == {f"{s}.{ext}" for s in stems for ext in ("h5", "xdmf")} | {"velocity_fluctuation.csv", "pressure_fluctuation.csv"}
    for stem, count in stems.items():
        assert len(_vectors(out / f"{stem}.h5")) == count, stem
        np.testing.assert_allclose(_times(out / f"{stem}.xdmf"), np.arange(count) * 1e-3, rtol=0, atol=1e-15, err_msg=stem)
    for name, ncomp in (("velocity", 3), ("pressure", 1)):
        x = _frames(results, name)[:12]
        assert x.shape[2] == ncomp and x.dtype == np.float64
        mean, f = hp.phase_average(x, 4)
        assert np.array_equal(_vectors(out / f"{name}_phase_mean.h5"), mean.astype(np.float32))
        assert np.array_equal(_vectors(out / f"{name}_fluctuation.h5"), f.astype(np.float32))
        assert np.array_equal(_vectors(out / f"{name}_fluctuation_amplitude.h5"), hp.windowed_rms_running(f, 4).astype(np.float32))
        table = np.loadtxt(out / f"{name}_fluctuation.csv", delimiter=",")
        assert table.shape == (12, 13)
        for i in (0, 5):
            data = np.loadtxt(sep / f"{name}_fluctuation_point_id_{i}.csv", delimiter=",")
            assert data.shape == (12, 1 + 1 + (ncomp if ncomp == 3 else 0))
            np.testing.assert_allclose(data[:, 0], np.arange(12) * 1e-3, rtol=0, atol=1e-15)
            assert np.array_equal(data[:, -ncomp:], f[:, i])
            assert np.array_equal(data[:, 1], hp.amplitude_magnitude(f[:, i]) if ncomp == 3 else f[:, i, 0])
            assert (sep / f"{name}_point_id_{i}.csv").exists()                      # the recorded series, as without the option
        if name == "velocity":
            e = hp.fluctuation_energy(f)
            assert np.array_equal(_vectors(out / "velocity_tke.h5")[:, :, 0], e.astype(np.float32))
            assert np.array_equal(_vectors(out / "velocity_tke_phase_mean.h5")[:, :, 0], hp.ordered_mean(e.reshape(3, 4, -1)).astype(np.float32))
            assert np.array_equal(_vectors(out / "velocity_tke_avg.h5")[0, :, 0], hp.ordered_mean(e).astype(np.float32))
            assert e.max() > 0
    # cycles 2 to 3: the files of the range start at the range's first frame
    ns, lines = _run(tmp_path / "range", T="0.0135", options=["--hi-pass", "v", *PHASE, "--hi-pass-start-cycle", "2"])
    out2 = tmp_path / "range" / "1" / "Visualization_hi_pass"
    x = _frames(tmp_path / "range" / "1", "velocity")[4:12]
    mean, f = hp.phase_average(x, 4)
    assert np.array_equal(_vectors(out2 / "velocity_phase_mean.h5"), mean.astype(np.float32))
    assert np.array_equal(_vectors(out2 / "velocity_fluctuation.h5"), f.astype(np.float32))
    np.testing.assert_allclose(_times(out2 / "velocity_fluctuation.xdmf"), (4 + np.arange(8)) * 1e-3, rtol=0, atol=1e-15)
    np.testing.assert_allclose(_times(out2 / "velocity_tke.xdmf"), (4 + np.arange(8)) * 1e-3, rtol=0, atol=1e-15)
    assert _times(out2 / "velocity_tke_avg.xdmf") == [0.0] and len(_times(out2 / "velocity_phase_mean.xdmf")) == 4
    assert not (out2 / "velocity_fluctuation_amplitude.h5").exists()


def _outputs(results):
    return {str(p.relative_to(results)): p.read_bytes() for sub in ("Visualization_hi_pass", "Visualization_separate_domain")
            if (results / sub).exists() for p in sorted((results / sub).rglob("*")) if p.is_file()}


def test_a_run_cut_by_a_checkpoint_and_continued_writes_the_same_bytes(tmp_path):
    """40 frames, stride 2 and a cycle of 8 ms: 20 selected frames, five cycles of 4, beside the low-pass band; cut after 17
    steps."""
    options = ["--hi-pass", "v", "--hi-pass-bands", "0", "200", "--hi-pass-amplitude", "--hi-pass-window", "4", "--hi-pass-stride", "2",
               "--hi-pass-point-ids", "3", "--hi-pass-phase-average", "--hi-pass-cycle", "0.008", "--hi-pass-end-cycle", "4"]
    _run(tmp_path / "whole" / "case", options=options)
    whole = _outputs(tmp_path / "whole" / "case" / "1")
    half = tmp_path / "half" / "case" / "1"
    half.mkdir(parents=True)
    ns, _ = _run(half.parent, options=options, kill_at=SPLIT, kill_path=half / "killturtle")
    assert ns["backend"].steps == SPLIT
    ns, lines = _restart(half, options=options)
    assert any("phase average over cycles 1 to 4 of 4 frames" in line for line in lines)
    split = _outputs(half)
    assert sorted(split) == sorted(whole) and "Visualization_hi_pass/velocity_tke_avg.h5" in whole
    assert len(_vectors(half / "Visualization_hi_pass" / "velocity_fluctuation.h5")) == 16
    for name in whole:
        assert split[name] == whole[name], name


def test_without_the_option_the_files_are_those_of_before(tmp_path):
    base = ["--hi-pass", "v", "--hi-pass-amplitude", "--hi-pass-window", "8", "--hi-pass-point-ids", "0"]
    _run(tmp_path / "without" / "case", options=base)
    _run(tmp_path / "with" / "case", options=base + ["--hi-pass-phase-average", "--hi-pass-cycle", "0.01"])
    old, new = _outputs(tmp_path / "without" / "case" / "1"), _outputs(tmp_path / "with" / "case" / "1")
    assert sorted(old) == ["Visualization_hi_pass/velocity_25_to_1000.csv", "Visualization_hi_pass/velocity_25_to_1000.h5",
                           "Visualization_hi_pass/velocity_25_to_1000.xdmf", "Visualization_hi_pass/velocity_25_to_1000_amplitude.h5",
                           "Visualization_hi_pass/velocity_25_to_1000_amplitude.xdmf", "Visualization_separate_domain/velocity_point_id_0.csv"]
    assert set(old) < set(new) and all(new[k] == v for k, v in old.items())           # what the options of before write: not a byte changed
    assert all("_phase_mean" in k or "_fluctuation" in k or "_tke" in k for k in set(new) - set(old))


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------

def test_header_binding_and_kernel_source_agree():
    from vasp_amd import capi
    from vasp_amd.monolithic import add_session_arguments
    import argparse
    header = (ROOT / "include" / "vaspfsi.h").read_text()
    lib = capi.load_library()
    for name in ("fsi_band_phase", "fsi_band_phase_fetch"):
        m = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S)
        assert m and name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
        assert "REF" in header[:m.start()].rsplit("/*", 1)[1], name                  # every call names what it replaces
    for k, what in enumerate(hp.PHASE_WHAT):
        assert re.search(r"#define FSI_PHASE_%s %d\b" % (what.upper(), k), header) and capi.HipBackend.PHASE_WHAT[what] == k
    src = (ROOT / "vasp_amd" / "csrc" / "fsi_phase.hip").read_text()
    assert "#pragma clang fp contract(off)" in src
    assert "fsi_phase.hip" in (ROOT / "vasp_amd" / "csrc" / "Makefile").read_text()
    ap = argparse.ArgumentParser()
    add_session_arguments(ap)
    ns = vars(ap.parse_args([]))
    assert all(ns[k] is None for k in ("hi_pass_phase_average", "hi_pass_cycle", "hi_pass_start_cycle", "hi_pass_end_cycle"))
