"""Spectrogram sessions on the device (csrc/fsi_spec.hip, HipBackend.spec_*, ``--spectrogram``) against scipy and against the
host twin of the session (vasp_amd/spectrogram.py: HostSpecSession).  Fixtures and scipy only.

Bounds: against scipy the device is held to the bound derived in tests/test_spectrogram.py (``power_bound``).  Against the
host twin - the same table, the same mean, the same y_j = w_j (x_j - m), the same order of the sum over the rows - only the
order inside a dot product differs (BLAS there, v_mfma_f64_16x16x4_f64 here), so it is held to the accumulation part of that
bound alone: K roundings on either side plus 8 for a table entry that the two libraries round differently,
(2 K + 8) 2^-53 sum_j |w_j (x_j - m)| per row and bin (``accumulation_only``); no term for the mean, no factor for an FFT."""
import contextlib
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_spectrogram import (assert_log_close, host_session, power_bound, read_csv, reference_pipeline, scipy_periodogram_rows,
                              scipy_spectrogram_rows)
from vasp_amd import hi_pass as hp
from vasp_amd import spectrogram as sp

pytestmark = pytest.mark.gpu

FRAMES = 333                       # odd; no multiple of 4, 16 or 64
FS = 1000.0
K, NOV, NFFT = 90, 67, 180         # 91 bins, 11 segments: no multiple of the MFMA tile in any dimension
STENOSIS = GOLDEN / "offset_stenosis" / "offset_stenosis.h5"


def _signal(ndof, frames=FRAMES, seed=11):
    """(frames, ndof): per dof a mean of order 1e4, a slow carrier, a tone with its own frequency and noise of its own level."""
    rng = np.random.default_rng(seed)
    f, ph = rng.uniform(40.0, 450.0, ndof), rng.uniform(0.0, 2 * np.pi, ndof)
    t = (1 + np.arange(frames))[:, None] / FS
    return 1e4 * rng.uniform(-1, 1, ndof) + 50 * np.sin(2 * np.pi * 7 * t + ph) + np.sin(2 * np.pi * f * t + 2 * ph) \
        + rng.uniform(0.01, 1, ndof) * rng.standard_normal((frames, ndof))


def _rows(mesh, states, q, nodes, component):
    N2 = mesh.num_nodes
    if q == "p":
        return states[:, 6 * N2:][:, nodes]
    off = 0 if q == "d" else 3 * N2
    vec = states[:, off:off + 3 * N2].reshape(len(states), N2, 3)[:, nodes]
    return np.stack([sp.component_rows(v, component) for v in vec])


@pytest.fixture(scope="module")
def recorded(stenosis_case):
    """A context on the small stenosis mesh driven through fsi_set_state with a prescribed signal.  Sessions: v, the three
    components of every second P2 node stacked (a few thousand rows); p on 63 vertices; d, the magnitude at one node; and
    beside them the band-pass session of v on a different node list."""
    from vasp_amd.capi import HipBackend
    mesh, desc = stenosis_case[0]["mesh"], stenosis_case[1]
    hb = HipBackend(desc)
    states = _signal(hb.ndof)
    lists = {"v": (np.arange(0, mesh.num_nodes, 2), "all"), "p": (np.arange(5, 5 + 63), "x"), "d": (np.array([mesh.num_nodes - 3]), "mag")}
    for q, (nodes, comp) in lists.items():
        hb.spec_begin(q, nodes, None, comp, capacity=FRAMES)
    band_nodes = np.arange(1, mesh.num_nodes, 3).astype(np.int32)
    hb.hi_pass_begin("v", band_nodes, None, capacity=FRAMES)
    for k in range(FRAMES):
        hb.set_state("n", states[k])
        for q in lists:
            hb.spec_sample(q)
        hb.hi_pass_sample("v")
    yield hb, mesh, states, lists, band_nodes
    hb.close()


def test_recorded_frames_are_the_states_that_were_set(recorded):
    hb, mesh, states, lists, _ = recorded
    for q, (nodes, comp) in lists.items():
        x = _rows(mesh, states, q, nodes, comp)
        assert x.shape[1] == {"v": 3 * len(nodes), "p": 63, "d": 1}[q]
        for k in (0, 1, FRAMES // 2, FRAMES - 1):
            assert np.array_equal(hb.spec_fetch(q, k), x[k]), (q, k)


@pytest.mark.parametrize("filtered", [False, True], ids=["raw", "highpassed"])
def test_spectrogram_and_periodogram_against_scipy_and_the_host_session(recorded, filtered):
    hb, mesh, states, lists, _ = recorded
    w = sp.window_values("blackmanharris", K)
    wp = sp.window_values("blackmanharris", FRAMES)
    prm = sp.highpass_design(FS, 25.0)
    for q, (nodes, comp) in lists.items():
        x = _rows(mesh, states, q, nodes, comp)
        host = host_session(x)
        if filtered:
            hb.spec_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
            host.filter(prm["b"], prm["a"], prm["zi"], prm["padlen"])
            src = host.filtered
            for k in (0, 17, FRAMES - 1):                                  # launch_band_filter: scipy's filtfilt bit for bit
                assert np.array_equal(hb.spec_fetch(q, k, filtered=True), src[k]), (q, k)
        else:
            hb.spec_filter(q)
            src = x
        for scaling in ("spectrum", "density"):
            got = hb.spec_spectrogram(q, K, NOV, NFFT, w, scaling, FS)
            ref_rows = scipy_spectrogram_rows(src, FS, K, NOV, NFFT, "blackmanharris", scaling)
            bound = power_bound(src, ref_rows, w, K, K - NOV, NFFT, scaling, FS)
            twin = host.spectrogram(K, NOV, NFFT, w, scaling, FS)
            part = power_bound(src, ref_rows, w, K, K - NOV, NFFT, scaling, FS, accumulation_only=True)
            e_ref, e_twin = np.abs(got - ref_rows.mean(axis=0)), np.abs(got - twin)
            print(f"{q} rows {src.shape[1]} {'filtered' if filtered else 'raw'} {scaling} spectrogram: share of the bound against scipy "
                  f"{(e_ref / bound).max():.3e}, of its accumulation part against the host twin {(e_twin / part).max():.3e}, "
                  f"max relative error {(e_ref / ref_rows.mean(axis=0)).max():.3e}")
            assert got.shape == (NFFT // 2 + 1, (FRAMES - NOV) // (K - NOV))
            assert (e_ref <= bound).all() and (e_twin <= part).all(), (q, scaling)
            got = hb.spec_periodogram(q, wp, scaling, FS)
            ref_rows = scipy_periodogram_rows(src, FS, scaling)
            bound = power_bound(src, ref_rows, wp, FRAMES, FRAMES, FRAMES, scaling, FS)[:, 0]
            part = power_bound(src, ref_rows, wp, FRAMES, FRAMES, FRAMES, scaling, FS, accumulation_only=True)[:, 0]
            e_ref, e_twin = np.abs(got - ref_rows.mean(axis=0)[:, 0]), np.abs(got - host.periodogram(wp, scaling, FS))
            print(f"{q} rows {src.shape[1]} {'filtered' if filtered else 'raw'} {scaling} periodogram: share against scipy "
                  f"{(e_ref / bound).max():.3e}, against the host twin {(e_twin / part).max():.3e}")
            assert got.shape == (FRAMES // 2 + 1,)
            assert (e_ref <= bound).all() and (e_twin <= part).all(), (q, scaling)


def test_the_same_call_twice_gives_the_same_bits(recorded):
    hb = recorded[0]
    w = sp.window_values("hann", K)
    prm = sp.highpass_design(FS, 25.0)
    for q in ("v", "p", "d"):
        hb.spec_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
        a = hb.spec_spectrogram(q, K, NOV, NFFT, w, "spectrum", FS)
        pa = hb.spec_periodogram(q, sp.window_values("blackmanharris", FRAMES), "spectrum", FS)
        hb.spec_filter(q)
        raw = hb.spec_spectrogram(q, K, NOV, NFFT, w, "spectrum", FS)
        hb.spec_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
        b = hb.spec_spectrogram(q, K, NOV, NFFT, w, "spectrum", FS)
        pb = hb.spec_periodogram(q, sp.window_values("blackmanharris", FRAMES), "spectrum", FS)
        assert a.tobytes() == b.tobytes() and pa.tobytes() == pb.tobytes() and not np.array_equal(a, raw), q
        assert np.isfinite(a).all() and (a >= 0).all()


def test_runs_beside_the_band_pass_session_of_the_same_quantity(recorded):
    hb, mesh, states, lists, band_nodes = recorded
    prm = hp.design(1 / FS, 25.0, 1000.0)
    hb.hi_pass_filter("v", prm["b"], prm["a"], prm["zi"], prm["padlen"])
    before = np.stack([hb.hi_pass_fetch("v", "filtered", k) for k in range(FRAMES)])
    N2 = mesh.num_nodes
    x = states[:, 3 * N2:6 * N2].reshape(FRAMES, N2, 3)[:, band_nodes]
    assert np.array_equal(before, hp.filtfilt_rows(prm["b"], prm["a"], x, prm["zi"], prm["padlen"]))
    hpf = sp.highpass_design(FS, 25.0)
    hb.spec_filter("v", hpf["b"], hpf["a"], hpf["zi"], hpf["padlen"])
    P = hb.spec_spectrogram("v", K, NOV, NFFT, sp.window_values("blackmanharris", K), "spectrum", FS)
    hb.spec_periodogram("v", sp.window_values("blackmanharris", FRAMES), "spectrum", FS)
    after = np.stack([hb.hi_pass_fetch("v", "filtered", k) for k in range(FRAMES)])
    assert after.tobytes() == before.tobytes() and np.isfinite(P).all()
    assert np.array_equal(hb.hi_pass_fetch("v", "raw", 7), x[7])
    nodes, comp = lists["v"]
    assert np.array_equal(hb.spec_fetch("v", 7), _rows(mesh, states[7:8], "v", nodes, comp)[0])


def test_session_errors(recorded, cylinder_case):
    from vasp_amd.capi import FsiError, HipBackend
    hb0 = recorded[0]
    with pytest.raises(FsiError, match="history is full"):
        hb0.spec_sample("p")
    with pytest.raises(FsiError, match="frame out of range"):
        hb0.spec_fetch("p", FRAMES)
    hb = HipBackend(cylinder_case[1])
    try:
        cmesh = cylinder_case[0]["mesh"]
        with pytest.raises(FsiError, match="fsi_spec_begin first"):
            hb.spec_sample("v")
        with pytest.raises(FsiError, match="fsi_spec_begin first"):          # the binding holds no shape: the library's refusal
            hb.spec_fetch("v", 0)
        with pytest.raises(FsiError, match="fsi_spec_begin first"):
            hb.spec_periodogram("v", np.ones(4), "spectrum", FS)
        with pytest.raises(FsiError, match="node out of range"):
            hb.spec_begin("p", [cmesh.num_vertices], None, "x", 4)
        hb.spec_begin("v", np.arange(40), None, "z", 64)
        for _ in range(21):
            hb.spec_sample("v")
        prm = sp.highpass_design(FS, 25.0)
        with pytest.raises(FsiError, match="21 recorded frames, the filter needs more than padlen = 21"):
            hb.spec_filter("v", prm["b"], prm["a"], prm["zi"], prm["padlen"])
        with pytest.raises(FsiError, match="fsi_spec_filter first"):
            hb.spec_fetch("v", 0, filtered=True)
        with pytest.raises(FsiError, match="one segment needs nperseg = 32"):
            hb._check(hb.lib.fsi_spec_spectrogram(hb.ctx, 1, 32, 0, 64, sp.window_values("hann", 32).ctypes.data, 0, FS,
                                                  np.empty(33).ctypes.data))
        assert not hb.spec_spectrogram("v", 16, 12, 32, sp.window_values("hann", 16), "spectrum", FS).any()     # zero in, zero out
        hb.spec_end("v")
        with pytest.raises(FsiError, match="fsi_spec_begin first"):
            hb.spec_sample("v")
    finally:
        hb.close()


def test_a_transform_beyond_device_memory_is_refused_and_the_context_still_steps(stenosis_case):
    """A transform length whose result and tables exceed the whole device (nfft = 2^38: 2^37 + 1 bins, 1.1 TB of result) is refused with the
    bytes it needs and the bytes the device has free; nothing is allocated, the output is not touched, the session and the
    context go on."""
    from vasp_amd.capi import FsiError, HipBackend
    ns, desc, bc_values, pressure, hook = stenosis_case
    mesh = ns["mesh"]
    hb = HipBackend(desc)
    try:
        hb.spec_begin("v", np.arange(100), None, "all", capacity=40)
        for _ in range(24):
            hb.spec_sample("v")
        free_b, total_b = hb.device_memory()
        out = np.full(8, -1.0)
        w = sp.window_values("hann", 24)
        with pytest.raises(FsiError) as e:
            hb._check(hb.lib.fsi_spec_spectrogram(hb.ctx, 1, 24, 0, 1 << 38, w.ctypes.data, 0, FS, out.ctypes.data))
        msg = str(e.value)
        assert e.value.code == 1 and "FSI_ERR_INVALID" in msg
        need, free_said = (int(x) for x in re.search(r"needs (\d+) bytes .* has (\d+) bytes free", msg).groups())
        assert need > total_b and need >= 8 * ((1 << 37) + 1)
        assert 0 < free_said <= total_b and abs(free_said - free_b) <= 1 << 30
        assert (out == -1.0).all() and hb.device_memory()[0] >= free_b - (1 << 26)          # nothing written, nothing allocated
        assert hb.spec_spectrogram("v", 24, 0, 48, w, "spectrum", FS).shape == (25, 1)      # the session goes on
        with pytest.raises(FsiError, match=r"tables are limited to"):                       # a table the host is not asked for
            hb._check(hb.lib.fsi_spec_spectrogram(hb.ctx, 1, 24, 0, 1 << 27, w.ctypes.data, 0, FS, out.ctypes.data))
        # a history beyond the device is refused as by fsi_band_begin, and the open session of the quantity stays as it was
        with pytest.raises(FsiError, match=r"needs \d+ bytes .* has \d+ bytes free"):
            hb.spec_begin("v", np.arange(mesh.num_nodes), None, "x", capacity=int(total_b // (8 * mesh.num_nodes)) + 1)
        assert (out == -1.0).all() and np.array_equal(hb.spec_fetch("v", 23), hb.spec_fetch("v", 0))
        run = dict(ns)
        run["t"] = float(ns["dt"])
        with contextlib.redirect_stdout(io.StringIO()):
            hook("pre_solve")(**run)
        hb.set_dirichlet_values(bc_values())
        hb.set_interface_pressure(float(pressure.P) if pressure is not None else 0.0)
        hist = hb.newton_solve(counter=0, first_step_num=0, **{k: ns[k] for k in ("atol", "rtol", "max_it", "lmbda", "recompute", "recompute_tstep")})
        assert len(hist) >= 1 and np.isfinite(hb.get_state("n")).all()
        hb.spec_sample("v")
        assert np.array_equal(hb.spec_fetch("v", 24).reshape(3, 100).T.ravel(), hb.get_state("n")[3 * mesh.num_nodes:3 * mesh.num_nodes + 300])
    finally:
        hb.close()


def test_destroy_without_end_leaks_nothing(cylinder_case):
    from vasp_amd.capi import HipBackend
    mesh, desc = cylinder_case[0]["mesh"], cylinder_case[1]
    hb = HipBackend(desc)
    free0 = hb.device_memory()[0]
    hb.set_state("n", 1e-4 * np.random.default_rng(4).standard_normal(hb.ndof))
    for q, comp in (("d", "mag"), ("v", "all"), ("p", "x")):
        hb.spec_begin(q, *hp.output_nodes(mesh, 1, q), comp, capacity=20000)
        hb.spec_sample(q)
    assert hb.device_memory()[0] < free0 - (1 << 28)            # the sessions hold memory ...
    hb.close()                                                  # ... no fsi_spec_end: fsi_destroy frees them
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


def test_end_to_end_run_writes_the_pipeline_of_its_own_states(tmp_path):
    """--spectrogram v p --spectrogram-sampling All on the small stenosis mesh, 100 saved frames, in a fresh process: four
    CSV files per quantity whose numbers are the host pipeline (scipy's, row by row) on the states the run's own post_solve
    hook recorded, within the derived bounds carried through the logarithm and the clamp."""
    from vasp_amd.mesh import FsiMesh
    (tmp_path / "sp_case.py").write_text(HOOK_PROBLEM)
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "vasp_amd.monolithic", "-p", "sp_case", "-dt", "0.001", "-T", "0.099", "--verbose", "False",
           "--folder", str(tmp_path / "run"), "--sub-folder", "1", "--save-step", "1", "--save-deg", "2", "--checkpoint-step", "1000",
           "--spectrogram", "v", "p", "--spectrogram-sampling", "All", "--new-arguments", f"mesh_path={STENOSIS}"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=1500, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = tmp_path / "run" / "1"
    states = np.load(res / "hook_states.npy")
    n = len(states)
    assert n == 100 and "Spectrograms of 100 frames (v, p; All" in r.stdout
    from vasp_amd.monolithic import parameters
    with contextlib.redirect_stdout(io.StringIO()):
        _, _, v = parameters(["-p", "offset_stenosis", "--spectrogram-sampling", "All", "--verbose", "False"])
    o = sp.options(v)
    with contextlib.redirect_stdout(io.StringIO()):
        from conftest import prepare_case
        mesh = prepare_case("offset_stenosis", STENOSIS, tmp_path / "prep")[0]["mesh"]
    T = n * 1e-3
    out = res / "Spectrograms"
    assert len(list(out.iterdir())) == 8
    for q, min_color in (("v", -20), ("p", -5)):
        sel = sp.select_nodes(mesh, 2, q, v, o)
        x = _rows(mesh, states, q, sel["nodes"], "all")
        ref = reference_pipeline(x, T, o, min_color)
        names = sp.file_names(sel["name"], "run", ref["num_windows"], min_color)
        head, tab = read_csv(out / names["spectrogram"])
        nseg = (n - ref["nov"]) // (ref["K"] - ref["nov"])
        assert tab.shape == (ref["K"] + 1, 1 + nseg) and len(head.split(",")) == nseg
        assert_log_close(tab[:, 1:], ref["Pf"], ref["bf"], min_color)
        _, tab_p = read_csv(out / names["psd"])
        assert tab_p.shape == (n // 2 + 1, 2)
        assert_log_close(tab_p[:, 1], ref["Pp"], ref["bp"])
        # chromagram and SBI: those of the raw rows' power, which the device gives within its bound; through the filter
        # bank (non-negative weights, columns normalised to sum 1) a relative change of the power by at most e moves a
        # chroma entry by at most 2 e of itself, and c log c by (|log c| + 1) times that
        _, tab_c = read_csv(out / names["chromagram"])
        Pr = np.exp(np.maximum(np.log(ref["Pr"]), min_color))
        chroma = sp.chromagram(Pr, ref["fs"], 2 * ref["K"])
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(ref["Pr"] > 2 * ref["br"], ref["br"] / (ref["Pr"] - ref["br"]), 0.0).max() + 16 * np.finfo(float).eps
        print(f"{q}: rows {x.shape[1]}, largest relative bound on the raw power {e:.3e}, chroma off by "
              f"{(np.abs(tab_c[:, 1:] - chroma) / chroma).max():.3e} of itself")
        assert tab_c.shape == (24, 1 + nseg) and (np.abs(tab_c[:, 1:] - chroma) <= 2 * e * chroma).all()
        _, tab_s = read_csv(out / names["sbi"])
        dsbi = (2 * e * chroma * (np.abs(np.log(chroma)) + 1)).sum(axis=0) / np.log(24)
        assert tab_s.shape == (nseg, 2) and (np.abs(tab_s[:, 1] - sp.sbi(chroma)) <= dsbi + 16 * np.finfo(float).eps).all()
