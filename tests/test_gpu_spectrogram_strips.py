"""The spectrogram in strips of rows on the device: the carried reduce (csrc/fsi_spec.hip, k_spec_reduce<true>) through
``fsi_spec_spectrogram_sum`` / ``fsi_spec_periodogram_sum`` against the unsplit calls on one session of all rows - which
tests/test_gpu_spectrogram.py holds against scipy -, ``fsi_spec_begin_rows`` against ``fsi_spec_begin``, ``fsi_spec_room``
against the begin call, the refusals, and ``python -m vasp_amd.postprocess --spectrogram`` unsplit and in strips on one finished
run.  Every comparison is bitwise; files are compared byte for byte.  A child process that ends with a time limit, an abort
or a fault ends its test: nothing more is started."""
import contextlib
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from vasp_amd import spectrogram as sg

pytestmark = pytest.mark.gpu

CYL = GOLDEN / "cylinder" / "cylinder.h5"
FRAMES = 48                         # more than padlen 21, no multiple of 16
FS = 1000.0
K, NOV, NFFT = 16, 12, 32           # 17 bins, 9 segments
SCALINGS = ("spectrum", "density")


@pytest.fixture(scope="module")
def cyl(cylinder_case):
    """A context on the cylinder and 48 prescribed states: per dof a mean of order 1e4, a tone of its own and noise."""
    from vasp_amd.capi import HipBackend
    hb = HipBackend(cylinder_case[1])
    rng = np.random.default_rng(23)
    f, ph = rng.uniform(40.0, 450.0, hb.ndof), rng.uniform(0.0, 2 * np.pi, hb.ndof)
    t = (1 + np.arange(FRAMES))[:, None] / FS
    states = 1e4 * rng.uniform(-1, 1, hb.ndof) + np.sin(2 * np.pi * f * t + ph) + rng.uniform(0.01, 1, hb.ndof) * rng.standard_normal((FRAMES, hb.ndof))
    yield hb, cylinder_case[0]["mesh"], states
    hb.close()


def _record(hb, q, states):
    for s in states:
        hb.set_state("n", s)
        hb.spec_sample(q)


def _transforms(hb, q, call):
    """The filtered spectrogram, the raw spectrogram and the raw periodogram in both scalings: ``call(kind, key, *args)``."""
    prm = sg.highpass_design(FS, 25.0)
    w, wp = sg.window_values("blackmanharris", K), sg.window_values("blackmanharris", FRAMES)
    out = {}
    hb.spec_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
    for scaling in SCALINGS:
        out["filtered", scaling] = call("spectrogram", ("filtered", scaling), K, NOV, NFFT, w, scaling, FS)
    hb.spec_filter(q)
    for scaling in SCALINGS:
        out["raw", scaling] = call("spectrogram", ("raw", scaling), K, NOV, NFFT, w, scaling, FS)
        out["psd", scaling] = call("periodogram", ("psd", scaling), wp, scaling, FS)
    return out


def _whole(hb, q, states, begin):
    """One session on all rows: its six mean powers and its recorded frames."""
    begin()
    try:
        _record(hb, q, states)
        ref = _transforms(hb, q, lambda kind, key, *args: getattr(hb, f"spec_{kind}")(q, *args))
        return ref, hb.spec_export(q, 0, FRAMES)
    finally:
        hb.spec_end(q)


def _in_strips(hb, q, states, cuts, begin_strip, frames_ref):
    """The six carried powers over the strips ``cuts`` of the rows; every strip records what the whole session recorded."""
    total_rows = cuts[-1][1]
    carries = {}
    for r0, r1 in cuts:
        begin_strip(r0, r1)
        try:
            _record(hb, q, states)
            assert np.array_equal(hb.spec_export(q, 0, FRAMES), frames_ref[:, r0:r1]), (q, r0, r1)
            total = total_rows if r1 == total_rows else 0
            got = _transforms(hb, q, lambda kind, key, *args: getattr(hb, f"spec_{kind}_sum")(q, *args, r0, total, carries.get(key)))
            if carries:                         # the caller's array is updated in place
                assert all(got[key] is carries[key] for key in got)
            carries = got
        finally:
            hb.spec_end(q)
    return carries


def _assert_same(got, ref, what):
    assert sorted(got) == sorted(ref) and len(ref) == 6
    for key in ref:
        assert got[key].shape == ref[key].shape and np.isfinite(ref[key]).all() and (ref[key] > 0).all(), (what, key)
        assert got[key].tobytes() == ref[key].tobytes(), (what, key, np.abs(got[key] - ref[key]).max())


# ---- 1. the carried sums against one session on all rows ---------------------------------------------------------------

@pytest.mark.parametrize("cuts", [((0, 128), (128, 384), (384, 423)), ((0, 423),)], ids=["three strips", "one strip"])
def test_component_all_in_strips_gives_the_unsplit_bits(cyl, cuts):
    """141 nodes of v, 423 component-major rows with component boundaries at 141 and 282: the middle strip crosses one and
    holds two row blocks, the last is ragged."""
    hb, mesh, states = cyl
    nodes = np.random.default_rng(3).choice(mesh.num_nodes, 141, replace=False).astype(np.int32)
    ref, frames = _whole(hb, "v", states, lambda: hb.spec_begin("v", nodes, None, "all", capacity=FRAMES))
    assert frames.shape == (FRAMES, 423)
    row_nodes, comps = np.tile(nodes, 3), np.repeat(np.arange(3, dtype=np.int32), 141)
    got = _in_strips(hb, "v", states, cuts, lambda r0, r1: hb.spec_begin_rows("v", row_nodes[r0:r1], None, comps[r0:r1], capacity=FRAMES), frames)
    _assert_same(got, ref, cuts)


def test_component_mag_in_strips_gives_the_unsplit_bits(cyl):
    hb, mesh, states = cyl
    nodes = np.random.default_rng(4).choice(mesh.num_nodes, 300, replace=False).astype(np.int32)
    ref, frames = _whole(hb, "d", states, lambda: hb.spec_begin("d", nodes, None, "mag", capacity=FRAMES))
    got = _in_strips(hb, "d", states, ((0, 256), (256, 300)), lambda r0, r1: hb.spec_begin("d", nodes[r0:r1], None, "mag", capacity=FRAMES), frames)
    _assert_same(got, ref, "mag")


def test_pressure_in_strips_gives_the_unsplit_bits(cyl):
    """200 rows of p: nodes drawn with replacement (some twice), every third row the mean of two nodes."""
    hb, mesh, states = cyl
    rng = np.random.default_rng(5)
    nodes = rng.integers(0, mesh.num_vertices, 200).astype(np.int32)
    nodes[7] = nodes[150] = nodes[0]                                                 # listed twice, across the strip boundary too
    nodes_b = np.where(np.arange(200) % 3 == 0, rng.integers(0, mesh.num_vertices, 200), -1).astype(np.int32)
    assert len(np.unique(nodes)) < 200 and (nodes_b >= 0).any() and (nodes_b < 0).any()
    ref, frames = _whole(hb, "p", states, lambda: hb.spec_begin("p", nodes, nodes_b, "x", capacity=FRAMES))
    got = _in_strips(hb, "p", states, ((0, 128), (128, 200)), lambda r0, r1: hb.spec_begin_rows("p", nodes[r0:r1], nodes_b[r0:r1], None, capacity=FRAMES),
                     frames)
    _assert_same(got, ref, "p")


# ---- 2. fsi_spec_begin_rows against fsi_spec_begin ---------------------------------------------------------------------

@pytest.mark.parametrize("component", ["y", "all"])
def test_begin_rows_records_what_begin_records(cyl, component):
    hb, mesh, states = cyl
    nodes = np.random.default_rng(6).choice(mesh.num_nodes, 77, replace=False).astype(np.int32)
    hb.spec_begin("v", nodes, None, component, capacity=5)
    _record(hb, "v", states[:5])
    ref = [hb.spec_fetch("v", k) for k in range(5)]
    hb.spec_end("v")
    reps = 3 if component == "all" else 1
    comps = np.repeat(np.arange(3, dtype=np.int32), 77) if component == "all" else np.full(77, 1, dtype=np.int32)
    hb.spec_begin_rows("v", np.tile(nodes, reps), None, comps, capacity=5)
    try:
        _record(hb, "v", states[:5])
        N2 = mesh.num_nodes
        for k in range(5):
            got = hb.spec_fetch("v", k)
            assert got.shape == (77 * reps,) and np.array_equal(got, ref[k]), (component, k)
            vel = states[k][3 * N2:6 * N2].reshape(N2, 3)[nodes]
            assert np.array_equal(got, sg.component_rows(vel, component))
    finally:
        hb.spec_end("v")


# ---- 3. fsi_spec_room and the begin calls ------------------------------------------------------------------------------

def test_spec_room_agrees_with_the_begin_call(cyl):
    from vasp_amd.capi import FsiError
    hb, mesh, _ = cyl
    N2 = mesh.num_nodes
    rows = 3 * N2
    row_nodes, comps = np.tile(np.arange(N2, dtype=np.int32), 3), np.repeat(np.arange(3, dtype=np.int32), N2)
    need1, available = hb.spec_room(rows, 1)
    assert need1 == sg.host_room(rows, 1)[0]                                         # the host twin states the same bytes
    assert hb.spec_room(300, 41, magnitude=True)[0] == sg.host_room(300, 41, True)[0] == sg.host_room(300, 41)[0] + 16 * 600
    lo, hi = 1, int(available // (16 * rows)) + 1                                    # need(hi) > available: the histories alone
    assert hb.spec_room(rows, hi)[0] > available
    while hi - lo > 1:                                                               # the largest capacity with need <= available
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if hb.spec_room(rows, mid)[0] <= available else (lo, mid)
    fits = lo
    need, avail = hb.spec_room(rows, fits)
    over, _ = hb.spec_room(rows, fits + 1)
    print(f"room: {rows} rows, available {avail} bytes, capacity {fits} needs {need}, capacity {fits + 1} needs {over}")
    assert need <= avail < over and need == sg.host_room(rows, fits)[0] and over == sg.host_room(rows, fits + 1)[0]
    free_before = hb.device_memory()[0]
    for begin in (lambda: hb.spec_begin_rows("v", row_nodes, None, comps, capacity=fits + 1),
                  lambda: hb.spec_begin("v", np.arange(N2, dtype=np.int32), None, "all", capacity=fits + 1)):
        with pytest.raises(FsiError) as e:
            begin()
        said = re.search(r"needs (\d+) bytes .* has (\d+) bytes free of which (\d+) stay", str(e.value))
        assert int(said.group(1)) == over and abs(int(said.group(2)) - int(said.group(3)) - avail) <= 1
    assert "fsi_spec_begin_rows" not in str(e.value) and hb.device_memory()[0] >= free_before - (1 << 26)      # nothing allocated
    with pytest.raises(FsiError, match="fsi_spec_begin first"):
        hb.spec_sample("v")
    hb.spec_begin_rows("v", row_nodes[:300], None, comps[:300], capacity=8)          # a later small begin succeeds
    hb.spec_sample("v")
    hb.spec_end("v")


# ---- 4. the refusals ---------------------------------------------------------------------------------------------------

def test_refused_sum_calls_leave_the_carry_and_the_context_as_they_were(cyl, cylinder_case):
    from vasp_amd.capi import FsiError, _ptr
    hb, mesh, states = cyl
    ns, _, bc_values, pressure, hook = cylinder_case
    lib, ctx = hb.lib, hb.ctx
    rng = np.random.default_rng(8)
    nodes = rng.choice(mesh.num_nodes, 256, replace=False).astype(np.int32)
    comps = rng.integers(0, 3, 256).astype(np.int32)
    with pytest.raises(FsiError, match="fsi_spec_begin_rows: needs the component of every row"):
        hb.spec_begin_rows("v", nodes, None, None, capacity=FRAMES)
    with pytest.raises(FsiError, match="fsi_spec_begin_rows: component out of range"):
        hb.spec_begin_rows("v", nodes, None, np.where(np.arange(256) == 9, 3, comps), capacity=FRAMES)
    with pytest.raises(FsiError, match="fsi_spec_begin_rows: node out of range"):
        hb.spec_begin_rows("p", [mesh.num_vertices], None, None, capacity=FRAMES)
    with pytest.raises(FsiError, match="fsi_spec_begin_rows: needs n > 0 nodes and a capacity > 0"):
        hb.spec_begin_rows("v", nodes, None, comps, capacity=0)
    hb.spec_begin_rows("v", nodes, None, comps, capacity=FRAMES)                      # 256 rows: two whole row blocks
    hb.spec_begin("d", nodes[:100], None, "x", capacity=FRAMES)                       # 100 rows: a ragged block
    try:
        for s in states[:24]:
            hb.set_state("n", s)
            hb.spec_sample("v")
            hb.spec_sample("d")
        w, wp = sg.window_values("hann", K), sg.window_values("blackmanharris", 24)
        cs, cp = np.full((NFFT // 2 + 1, 3), -1.0), np.full(13, -1.0)
        free_before = hb.device_memory()[0]

        def spectrogram(q=1, nperseg=K, noverlap=NOV, nfft=NFFT, window=w, scaling=0, fs=FS, first_row=0, total_rows=0, carry=cs):
            return lib.fsi_spec_spectrogram_sum(ctx, q, nperseg, noverlap, nfft, None if window is None else _ptr(window), scaling, fs, first_row,
                                                total_rows, None if carry is None else _ptr(carry))

        def periodogram(q=1, window=wp, scaling=0, fs=FS, first_row=0, total_rows=0, carry=cp):
            return lib.fsi_spec_periodogram_sum(ctx, q, None if window is None else _ptr(window), scaling, fs, first_row, total_rows,
                                                None if carry is None else _ptr(carry))

        def refused(rc, text):
            said = lib.fsi_last_error(ctx).decode()
            assert rc == 1 and text in said and "\n" not in said, said
            assert (cs == -1.0).all() and (cp == -1.0).all()

        for call, name in ((spectrogram, "fsi_spec_spectrogram_sum"), (periodogram, "fsi_spec_periodogram_sum")):
            refused(call(first_row=-128), f"{name}: first_row = -128, a strip starts at a multiple of 128 rows")
            refused(call(first_row=100), f"{name}: first_row = 100, a strip starts at a multiple of 128 rows")
            refused(call(q=0, first_row=128), f"{name}: the session has 100 rows and is not the last strip")
            refused(call(first_row=128, total_rows=383), f"{name}: total_rows = 383, the last strip ends at first_row + rows = 128 + 256")
            refused(call(total_rows=-256), f"{name}: total_rows = -256")
            refused(call(carry=None), f"{name}: needs a window, a carry")
            # every refusal of the unsplit calls
            refused(call(window=None), f"{name}: needs a window")
            refused(call(scaling=2), f"{name}: needs a window")
            refused(call(fs=0.0), f"{name}: needs a window")
            refused(call(q=2), f"{name}: no spectrogram session for this quantity")
            refused(call(q=5), f"{name}: quantity must be")
        refused(spectrogram(nperseg=32, window=sg.window_values("hann", 32), nfft=64), "one segment needs nperseg = 32")
        refused(spectrogram(nfft=8), "nfft >= nperseg")
        refused(spectrogram(noverlap=K), "0 <= noverlap < nperseg")
        refused(spectrogram(nfft=1 << 38), "fsi_spec_spectrogram_sum: the transform needs")          # spec_power's room check
        refused(spectrogram(nfft=1 << 27), "tables are limited to")
        assert lib.fsi_spec_spectrogram_sum(None, 1, K, NOV, NFFT, _ptr(w), 0, FS, 0, 0, _ptr(cs)) == 1
        assert hb.device_memory()[0] >= free_before - (1 << 26)                                     # nothing allocated
        with pytest.raises(FsiError, match="first_row = 64"):
            hb.spec_spectrogram_sum("v", K, NOV, NFFT, w, "spectrum", FS, 64, 0, np.zeros((17, 3)))
        with pytest.raises(ValueError, match="the carry must be a C-contiguous float64 array of shape"):
            hb.spec_periodogram_sum("v", wp, "spectrum", FS, 128, 0, np.zeros(12))
        # the session still transforms: one strip that holds every row is the mean, a first strip of more the plain sum
        assert hb.spec_spectrogram_sum("v", K, NOV, NFFT, w, "spectrum", FS, 0, 256).tobytes() == hb.spec_spectrogram("v", K, NOV, NFFT, w, "spectrum", FS).tobytes()
        assert hb.spec_periodogram_sum("v", wp, "density", FS, 0, 256).tobytes() == hb.spec_periodogram("v", wp, "density", FS).tobytes()
        assert spectrogram(carry=cs) == 0 and periodogram(carry=cp) == 0                            # first_row 0: the -1 are ignored
        assert (cs / 256.0).tobytes() == hb.spec_spectrogram("v", K, NOV, NFFT, w, "spectrum", FS).tobytes()
        assert (cp / 256.0).tobytes() == hb.spec_periodogram("v", wp, "spectrum", FS).tobytes()
        # and the context still takes a Newton step
        run = dict(ns)
        run["t"] = float(ns["dt"])
        with contextlib.redirect_stdout(io.StringIO()):
            hook("pre_solve")(**run)
        zero = np.zeros(hb.ndof)
        hb.set_state("n", zero)
        hb.set_state("n-1", zero)
        hb.set_dirichlet_values(bc_values())
        hb.set_interface_pressure(float(pressure.P) if pressure is not None else 0.0)
        hist = hb.newton_solve(counter=0, first_step_num=0, **{k: ns[k] for k in ("atol", "rtol", "max_it", "lmbda", "recompute", "recompute_tstep")})
        assert len(hist) >= 1 and np.isfinite(hb.get_state("n")).all()
        hb.spec_sample("v")
        N2 = mesh.num_nodes
        assert np.array_equal(hb.spec_fetch("v", 24), hb.get_state("n")[3 * N2:6 * N2].reshape(N2, 3)[nodes, comps])
    finally:
        for q in ("v", "d"):
            with contextlib.suppress(Exception):
                hb.spec_end(q)


# ---- 5. the whole tool -------------------------------------------------------------------------------------------------

RUN = ["-dt", "0.001", "-T", "0.0395", "--theta", "0.51", "--verbose", "False", "--save-step", "1", "--save-deg", "2", "--checkpoint-step", "50"]
OPTIONS = ["--spectrogram", "d", "v", "p", "--spectrogram-sampling", "All", "--spectrogram-region", "box",
           "--spectrogram-fsi-region", "-100", "100", "-100", "100", "-100", "100"]


def _child(module, argv, cwd, limit):
    """One child under its own time limit; anything but exit status 0 fails the caller, which then starts nothing more."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", module, *argv], cwd=cwd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        pytest.fail(f"python -m {module} ended with status {r.returncode}:\n" + r.stdout[-3000:] + r.stderr[-3000:], pytrace=False)
    return r.stdout


def _same_bytes(a, b):
    names = sorted(p.name for p in (a / "Spectrograms").iterdir())
    assert names == sorted(p.name for p in (b / "Spectrograms").iterdir()) and names
    for name in names:
        assert (a / "Spectrograms" / name).read_bytes() == (b / "Spectrograms" / name).read_bytes(), name
    return names


def test_the_tool_in_strips_writes_the_unsplit_files_byte_for_byte(tmp_path):
    """One 40-step cylinder run at save_deg 2, then every node of the mesh: --history-memory in fsi_spec_room's bytes (the host
    twin's, which test 3 compares with the device's) such that the largest quantity takes exactly three strips."""
    from vasp_amd import postprocess
    from vasp_amd import spectrogram_strips as strips
    results = tmp_path / "case" / "1"
    log = _child("vasp_amd.monolithic", ["-p", "cylinder", *RUN, "--folder", str(results.parent), "--sub-folder", "1",
                                         "--new-arguments", f"mesh_path={CYL}"], tmp_path, 300)
    assert "Solved for timestep 40," in log
    with contextlib.redirect_stdout(io.StringIO()):
        ns, mesh, source, indices, _ = postprocess.prepare(["--folder", str(results), *OPTIONS])
    source.close()
    plan = sg.SpectrogramRun(None, mesh, ns, open_sessions=False)
    rows = {q: plan.rows(q) for q in plan.quantities}
    need = lambda r, capacity: sg.host_room(r, capacity)[0]
    big = max(rows.values())
    size = -(-(-(-big // 3)) // 128) * 128
    limit = need(size, len(indices) + 1)
    count = {q: len(strips.plan_row_strips(rows[q], 128, len(indices) + 1, limit, need)) for q in rows}
    assert len(indices) == 40 and max(count.values()) == 3 and big > 3 * 128, (rows, count)
    base = ["--folder", str(results), *OPTIONS]
    log = _child("vasp_amd.postprocess", [*base, "--output-folder", str(tmp_path / "whole")], tmp_path, 120)
    assert "Read 40 of 40 frames" in log and "in strips" not in log and "Spectrograms of 40 frames (d, v, p; All" in log
    log = _child("vasp_amd.postprocess", [*base, "--output-folder", str(tmp_path / "split"), "--history-memory", str(limit)], tmp_path, 180)
    said = re.findall(r"Spectrograms of (\w) in strips: (\d+) strips of at most (\d+) rows \((\d+) in all\), the 40 frames read (\d+) times; "
                      r"([\d.]+) s reading, ([\d.]+) s transforming", log)
    print("\n".join(line for line in log.splitlines() if "in strips" in line))
    assert [(s[0], int(s[1]), int(s[3]), int(s[4])) for s in said] == [(q, count[q], rows[q], count[q]) for q in ("d", "v", "p")], log[-2000:]
    assert all(int(s[2]) % 128 == 0 or int(s[1]) == 1 for s in said)
    names = _same_bytes(tmp_path / "whole", tmp_path / "split")
    assert len(names) == 12                                                          # four CSV files per quantity
    _child("vasp_amd.postprocess", [*base, "--output-folder", str(tmp_path / "again"), "--history-memory", str(limit)], tmp_path, 180)
    _same_bytes(tmp_path / "split", tmp_path / "again")
