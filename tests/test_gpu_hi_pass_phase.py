"""Phase-averaged fields and the energy of the fluctuation on the device (csrc/fsi_phase.hip; fsi_band_phase,
fsi_band_phase_fetch; HipBackend.hi_pass_phase / hi_pass_phase_fetch; ``--hi-pass-phase-average``) against the NumPy twin
(vasp_amd/hi_pass.py: HostBandSession.phase / phase_fetch), which tests/test_hi_pass_phase.py holds to the reference's own
compute_tke.  Everything is compared bit for bit: the kernels are FP64 additions, subtractions, multiplications and true
divisions in the twin's order, compiled without contraction.  The histories are filled with hi_pass_import: no time step is
taken but in the end-to-end run."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from vasp_amd import hi_pass as hp

pytestmark = pytest.mark.gpu

STENOSIS = GOLDEN / "offset_stenosis" / "offset_stenosis.h5"
CASES = ((4, 3), (1, 5), (5, 1), (3, 11))        # (period, cycles); 11 cycles exceed the 8 a lane keeps in registers
SHAPES = (("v", 65), ("v", 66), ("p", 1))        # 195 rows: odd, the 8-byte path, three wavefronts and three lanes; 198: even, the
WHATS = ("mean", "energy", "energy_cycle_mean", "energy_time_mean")                    # 16-byte path, no multiple of 64; one row


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[a == 0]), np.signbit(b[b == 0]))


@pytest.fixture(scope="module")
def hb(cylinder_case):
    from vasp_amd.capi import HipBackend
    backend = HipBackend(cylinder_case[1])
    src = (ROOT / "vasp_amd" / "csrc" / "fsi_phase.hpp").read_text()
    assert "PHASE_REG_CYCLES = 8;" in src          # what CASES and the comment above rely on
    yield backend
    backend.close()


def _frames(n, nodes, ncomp, seed, special=True):
    """(n, nodes, ncomp): a pulsatile part and a fluctuation; with ``special`` one -0.0, one row with a NaN and one with an inf."""
    rng = np.random.default_rng(seed)
    x = 0.3 * np.sin(0.7 * np.arange(n))[:, None, None] * rng.uniform(0.5, 1.5, (1, nodes, ncomp)) + 3e-3 * rng.standard_normal((n, nodes, ncomp))
    if special:
        x[0, 0, 0] = -0.0
        x[n // 2, nodes // 2, ncomp - 1] = np.nan
        x[n - 1, nodes - 1, 0] = np.inf
    return x


def _open(hb, q, nodes, x):
    """The session of q on the first ``nodes`` nodes with the history x, and its host twin."""
    hb.hi_pass_begin(q, np.arange(nodes, dtype=np.int32), None, len(x))
    hb.hi_pass_import(q, x)
    twin = hp.HostBandSession(x.shape[2], len(x))
    twin.import_(x)
    return twin


def _compare(hb, q, twin, period, n):
    for j in range(period):
        assert same_bits(hb.hi_pass_phase_fetch(q, "mean", j), twin.phase_fetch("mean", j)), ("mean", j)
        assert same_bits(hb.hi_pass_phase_fetch(q, "energy_cycle_mean", j), twin.phase_fetch("energy_cycle_mean", j)), ("cycle mean", j)
    for k in range(n):
        assert same_bits(hb.hi_pass_fetch(q, "filtered", k), twin.fetch("filtered", k)), ("fluctuation", k)
        assert same_bits(hb.hi_pass_phase_fetch(q, "energy", k), twin.phase_fetch("energy", k)), ("energy", k)
    assert same_bits(hb.hi_pass_phase_fetch(q, "energy_time_mean"), twin.phase_fetch("energy_time_mean"))


@pytest.mark.parametrize("period,cycles", CASES, ids=[f"P{p}C{c}" for p, c in CASES])
@pytest.mark.parametrize("q,nodes", SHAPES, ids=[f"{q}{n}" for q, n in SHAPES])
def test_device_equals_the_twin_bit_for_bit(hb, q, nodes, period, cycles):
    n, ncomp = period * cycles, 1 if q == "p" else 3
    x = _frames(n, nodes, ncomp, 100 * period + cycles)
    twin = _open(hb, q, nodes, x)
    try:
        hb.hi_pass_phase(q, period)
        twin.phase(period)
        _compare(hb, q, twin, period, n)
        if cycles == 1:                           # one cycle is its own mean: exactly zero wherever the input is finite
            f = np.stack([hb.hi_pass_fetch(q, "filtered", k) for k in range(n)])
            assert not f[np.isfinite(f)].any() and np.signbit(f[np.isfinite(f)]).sum() == 1
        assert same_bits(hb.hi_pass_export(q, 0, n), x)                                 # the raw frames are untouched
    finally:
        hb.hi_pass_end(q)


@pytest.mark.parametrize("q,nodes", SHAPES, ids=[f"{q}{n}" for q, n in SHAPES])
@pytest.mark.parametrize("period,cycles", [(4, 3), (3, 11)], ids=["registers", "second_read"])
def test_a_strided_view(hb, q, nodes, period, cycles):
    """select(first=2, stride=2): selected frame k is recorded frame 2 + 2 k; the frames between and behind stay unread."""
    n, ncomp = period * cycles, 1 if q == "p" else 3
    x = _frames(2 + 2 * n + 1, nodes, ncomp, 7 * period + cycles)
    twin = _open(hb, q, nodes, x)
    try:
        assert hb.hi_pass_select(q, 2, n, 2) == n == twin.select(2, n, 2)
        hb.hi_pass_phase(q, period)
        twin.phase(period)
        _compare(hb, q, twin, period, n)
        assert same_bits(twin.fetch("filtered", 1), x[4] - twin.phase_fetch("mean", 1))
        assert same_bits(hb.hi_pass_export(q, 0, len(x)), x)
    finally:
        hb.hi_pass_end(q)


def test_amplitude_and_trace_of_the_fluctuation(hb):
    """The windowed RMS of u' - the turbulence intensity - through the unchanged amplitude calls: k_band_rms sums as
    windowed_rms_running does, and division and square root are correctly rounded, so the frames are the twin's bits."""
    period, cycles, nodes = 4, 3, 66
    n = period * cycles
    x = _frames(n, nodes, 3, 5, special=False)
    twin = _open(hb, "v", nodes, x)
    try:
        hb.hi_pass_phase("v", period)
        twin.phase(period)
        f = np.stack([twin.fetch("filtered", k) for k in range(n)])
        hb.hi_pass_amplitude("v", 4)
        twin.amplitude(4)
        running = hp.windowed_rms_running(f, 4)
        for k in range(n):
            amp, mx, am = hb.hi_pass_fetch("v", "amplitude", k, with_max=True)
            assert np.array_equal(amp, running[k]) and np.array_equal(amp, twin.fetch("amplitude", k)), k
            mag = hp.amplitude_magnitude(amp)
            assert mx == mag.max() and am == int(np.argmax(mag)), k
        assert running[1:10].all() and not running[0].any() and not running[10:].any()
        points = [0, 64, 65, 0]
        tr = hb.hi_pass_trace("v", "filtered", points)
        assert tr.shape == (4, n, 4) and np.array_equal(tr, twin.trace("filtered", points))
        assert np.array_equal(tr[:, :, 1:], f[:, points].transpose(1, 0, 2))
        _compare(hb, "v", twin, period, n)          # the amplitude calls left the phase average alone
    finally:
        hb.hi_pass_end("v")


def test_a_tensor_session_by_rows(hb, cylinder_case):
    """Three solid cells: 12 dofs x 6 components = 72 rows.  The mean and the fluctuation are formed row by row; the three
    energies are refused."""
    from vasp_amd.capi import FsiError
    solid = np.nonzero(np.asarray(cylinder_case[1]["cell_kind"]) == 1)[0][:3]
    x = _frames(8, 12, 6, 17)
    hb.hi_pass_begin_cells("strain", solid, 8)
    try:
        hb.hi_pass_import("strain", x)
        twin = hp.HostBandSession(6, 8)
        twin.import_(x)
        hb.hi_pass_phase("strain", 4)
        twin.phase(4)
        for j in range(4):
            assert same_bits(hb.hi_pass_phase_fetch("strain", "mean", j), twin.phase_fetch("mean", j))
        for k in range(8):
            assert same_bits(hb.hi_pass_fetch("strain", "filtered", k), twin.fetch("filtered", k))
        for what in WHATS[1:]:
            with pytest.raises(FsiError, match="strain / stress session has no energy"):
                hb.hi_pass_phase_fetch("strain", what, 0)
        assert same_bits(hb.hi_pass_phase_fetch("strain", "mean", 3), twin.phase_fetch("mean", 3))
    finally:
        hb.hi_pass_end("strain")


def test_refusals_leave_the_session_usable_and_a_filter_gives_the_band_again(hb):
    from vasp_amd.capi import FsiError
    period, cycles, nodes = 3, 11, 65
    n = period * cycles
    x = _frames(n + 1, nodes, 3, 23, special=False)
    twin = _open(hb, "v", nodes, x)
    low = hp.design(1e-3, 0.0, 200.0)
    keys = ("b", "a", "zi", "padlen")
    try:
        with pytest.raises(FsiError, match=r"no phase average \(fsi_band_phase first\)"):
            hb.hi_pass_phase_fetch("v", "mean", 0)
        with pytest.raises(FsiError, match="fsi_band_begin first"):
            hb.hi_pass_phase("d", 3)
        with pytest.raises(FsiError, match="period = 3 frames, 34 selected frames"):     # every recorded frame: no multiple
            hb.hi_pass_phase("v", 3)
        assert hb.hi_pass_select("v", 0, n, 1) == n == twin.select(0, n, 1)
        for bad in (0, -2, 5, 2 * n):
            with pytest.raises(FsiError, match=rf"period = {bad} frames, {n} selected frames") as e:
                hb.hi_pass_phase("v", bad)
            assert e.value.code == 1
        with pytest.raises(FsiError, match=r"no filtered series \(fsi_band_filter first\)"):      # the refused calls left no series
            hb.hi_pass_fetch("v", "filtered", 0)
        hb.hi_pass_phase("v", period)
        twin.phase(period)
        for what, frame in (("mean", period), ("energy", n), ("energy_cycle_mean", period), ("energy_time_mean", 1), ("energy", -1)):
            with pytest.raises(FsiError, match="out of range"):
                hb.hi_pass_phase_fetch("v", what, frame)
        assert hb.lib.fsi_band_phase_fetch(hb.ctx, 1, 4, 0, None) == 1 and hb.lib.fsi_band_phase_fetch(hb.ctx, 1, 0, 0, None) == 1
        with pytest.raises(FsiError, match="period = 5 frames"):                           # a refused call keeps the result that stands
            hb.hi_pass_phase("v", 5)
        _compare(hb, "v", twin, period, n)
        # a second call with another period replaces the first
        hb.hi_pass_phase("v", 11)
        twin.phase(11)
        _compare(hb, "v", twin, 11, n)
        # the plain band again, and with it the phase average is gone
        hb.hi_pass_filter("v", *(low[k] for k in keys))
        y = hp.filtfilt_rows(low["b"], low["a"], x[:n], low["zi"], low["padlen"])
        assert np.array_equal(np.stack([hb.hi_pass_fetch("v", "filtered", k) for k in range(n)]), y)
        with pytest.raises(FsiError, match=r"no phase average \(fsi_band_phase first\)"):
            hb.hi_pass_phase_fetch("v", "mean", 0)
        # each of the other calls that change the series or the frames invalidates it too
        for undo in (lambda: hb.hi_pass_select("v", 0, n, 1), lambda: hb.hi_pass_filter_next("v", *(low[k] for k in keys[:3]), 0)):
            hb.hi_pass_phase("v", period)
            assert hb.hi_pass_phase_fetch("v", "mean", 0).shape == (nodes, 3)
            undo()
            with pytest.raises(FsiError, match=r"no phase average \(fsi_band_phase first\)"):
                hb.hi_pass_phase_fetch("v", "energy", 0)
        assert np.array_equal(hb.hi_pass_export("v", 0, n + 1), x)
    finally:
        hb.hi_pass_end("v")
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_phase_fetch("v", "mean", 0)


def test_an_import_and_a_sample_invalidate_the_phase_average(hb):
    from vasp_amd.capi import FsiError
    x = _frames(8, 66, 3, 31, special=False)
    hb.hi_pass_begin("v", np.arange(66, dtype=np.int32), None, 10)
    try:
        hb.hi_pass_import("v", x)
        for more in (lambda: hb.hi_pass_import("v", x[:1]), lambda: hb.hi_pass_sample("v")):
            hb.hi_pass_select("v", 0, 8, 1)
            hb.hi_pass_phase("v", 4)
            assert hb.hi_pass_phase_fetch("v", "energy_time_mean").shape == (66,)
            more()
            with pytest.raises(FsiError, match=r"no phase average \(fsi_band_phase first\)"):
                hb.hi_pass_phase_fetch("v", "mean", 0)
    finally:
        hb.hi_pass_end("v")


# ---- end to end -------------------------------------------------------------------------------------------------------

class _HostOnly:
    """A backend without device sessions: ``postprocess`` then records on the host twin."""

    def __init__(self, desc):
        pass


def test_end_to_end_run_writes_the_files_of_the_host_twin(tmp_path):
    """12 steps on the small stenosis mesh, every one saved, a cycle of 4 ms: three cycles of 4 frames, on the device in a
    fresh process.  The same options over the finished folder on the host twin write the same files, byte for byte (every
    dataset of an .h5 file: its headers carry the time of writing)."""
    from test_gpu_hi_pass import _files
    from vasp_amd import postprocess
    options = ["--hi-pass", "v", "p", "--hi-pass-phase-average", "--hi-pass-cycle", "0.004", "--hi-pass-amplitude", "--hi-pass-window", "4",
               "--hi-pass-point-ids", "0", "5"]
    results = tmp_path / "case" / "1"
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "vasp_amd.monolithic", "-p", "offset_stenosis", "-dt", "0.001", "-T", "0.0115",
           "--verbose", "False", "--folder", str(results.parent), "--sub-folder", "1", "--save-step", "1", "--save-deg", "2",
           "--checkpoint-step", "1000", *options, "--new-arguments", f"mesh_path={STENOSIS}"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "phase average over cycles 1 to 3 of 4 frames written" in r.stdout
    lines = []
    postprocess.run(["--folder", str(results), "--output-folder", str(tmp_path / "twin"), *options], backend_factory=_HostOnly, out=lines.append)
    assert any("Read 12 of 12 frames" in line for line in lines)
    device, twin = _files(results / "Visualization_hi_pass"), _files(tmp_path / "twin" / "Visualization_hi_pass")
    stems = ["velocity_phase_mean", "velocity_fluctuation", "velocity_fluctuation_amplitude", "velocity_tke", "velocity_tke_phase_mean",
             "velocity_tke_avg", "pressure_phase_mean", "pressure_fluctuation", "pressure_fluctuation_amplitude"]
    assert {k.split(":")[0] for k in device} == {f"{s}.{e}" for s in stems for e in ("h5", "xdmf")} | {"velocity_fluctuation.csv", "pressure_fluctuation.csv"}
    assert sorted(device) == sorted(twin)
    for name in device:
        assert device[name] == twin[name], name
    assert len([k for k in device if k.startswith("velocity_tke.h5:/VisualisationVector/")]) == 12
    tke = np.frombuffer(device["velocity_tke_avg.h5:/VisualisationVector/0"][2], dtype=np.float32)
    assert np.isfinite(tke).all() and tke.max() > 0
    traces, twin_traces = _files(results / "Visualization_separate_domain"), _files(tmp_path / "twin" / "Visualization_separate_domain")
    assert sorted(traces) == sorted(f"{name}{kind}_point_id_{i}.csv" for name in ("velocity", "pressure") for kind in ("", "_fluctuation") for i in (0, 5))
    assert traces == twin_traces
