"""Band-pass sessions on the strain and stress tensors of the solid cells (fsi_band_begin_cells, csrc/fsi_stress.hip:
k_tensor_sample, k_tensor_principal; HipBackend.hi_pass_begin_cells; ``--hi-pass-tensor``) against the stress / strain
session's own frames, the host restatement of scipy's filtfilt and of the windowed RMS (vasp_amd/hi_pass.py) and the closed
form of the principal value (oracle.post_oracle.kopp_max_eigenvalue)."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from vasp_amd import hi_pass as hp
from vasp_amd import hi_pass_tensor as hpt

pytestmark = pytest.mark.gpu

FRAMES = 48                  # more than the band-pass padlen of 33
DT = 1e-3
WINDOW = 8
KEEP = (0, 20, FRAMES - 1)   # the frames at which the stress / strain session's own frame is kept
ENTRIES = [0, 1, 4, 5, 8, 6]             # 11, 12, 22, 23, 33, 31 of the nine [REF postprocessing_h5py_common.py:349-354]
NAMES = {"strain": "GreenLagrangeStrain", "stress": "TrueStress"}
CYL = GOLDEN / "cylinder" / "cylinder.h5"


@contextlib.contextmanager
def _context(desc):
    from vasp_amd.capi import HipBackend
    hb = HipBackend(desc)
    try:
        yield hb
    finally:
        hb.close()


def _solid(desc):
    return np.nonzero(np.asarray(desc["cell_kind"]) == 1)[0]


def _states(mesh, desc, ndof, frames=FRAMES, seed=31):
    """(frames, ndof) and the cell lists: a displacement of 1e-3 hmin - per dof a constant part and a tone of its own
    frequency and phase - scaled by 1e-7 on the nodes of every 9th solid cell (strains near 1e-9 there) and zero on the nodes
    of every 31st; velocity and pressure are noise."""
    rng = np.random.default_rng(seed)
    N2, h = mesh.num_nodes, mesh.hmin()
    solid = _solid(desc)
    tiny, zero = solid[4::9], solid[7::31]
    f, ph = rng.uniform(40.0, 450.0, 3 * N2), rng.uniform(0.0, 2 * np.pi, 3 * N2)
    t = (1 + np.arange(frames))[:, None] * DT
    d = 1e-3 * h * (rng.standard_normal(3 * N2) + 0.5 * np.sin(2 * np.pi * f * t + ph)).reshape(frames, 3, N2)      # component-major
    nodes = np.asarray(mesh.tet_nodes)
    d[:, :, np.unique(nodes[tiny])] *= 1e-7
    d[:, :, np.unique(nodes[zero])] = 0.0
    states = 1e-4 * rng.standard_normal((frames, ndof))
    states[:, :3 * N2] = _as_state_order(mesh, d)
    return states, solid, tiny, zero


def _as_state_order(mesh, d):
    """(frames, 3, N2) -> the displacement block of a state, node-major as tests/test_gpu_hi_pass.py::_rows reads it."""
    return d.transpose(0, 2, 1).reshape(len(d), -1)


def _six(frame, name):
    """The six kept entries of a stress / strain session's frame: (cells * 4, 6)."""
    return frame[name].reshape(-1, 9)[:, ENTRIES]


@pytest.fixture(scope="module")
def recorded(cylinder_case):
    """One context on the cylinder driven through fsi_set_state; both tensor sessions record every frame, the stress /
    strain session beside them samples the same states and its frame is kept at three of them."""
    mesh, desc = cylinder_case[0]["mesh"], cylinder_case[1]
    with _context(desc) as hb:
        states, solid, tiny, zero = _states(mesh, desc, hb.ndof)
        hb.stress_strain_begin(solid)
        for q in NAMES:
            hb.hi_pass_begin_cells(q, solid, FRAMES)
        kept = {}
        for k in range(FRAMES):
            hb.set_state("n", states[k])
            for q in NAMES:
                hb.hi_pass_sample(q)
            if k in KEEP:
                kept[k] = hb.stress_strain_sample(frame=True)
        raw = {q: hb.hi_pass_export(q, 0, FRAMES) for q in NAMES}
        yield dict(hb=hb, mesh=mesh, desc=desc, states=states, solid=solid, tiny=tiny, zero=zero, kept=kept, raw=raw)


def _dofs(cells_listed, cells):
    """The DG1 dofs 4 i + a of ``cells`` within the session on ``cells_listed``."""
    pos = np.nonzero(np.isin(cells_listed, cells))[0]
    return (4 * pos[:, None] + np.arange(4)[None, :]).reshape(-1)


def test_raw_frames_are_the_stress_sessions_bits(recorded):
    r = recorded
    hb, solid = r["hb"], r["solid"]
    n = len(solid)
    assert n > 64 and len(r["tiny"]) > 8 and len(r["zero"]) > 2
    for q, name in NAMES.items():
        assert r["raw"][q].shape == (FRAMES, 4 * n, 6)
        for k in KEEP:
            want = _six(r["kept"][k], name)
            got = hb.hi_pass_fetch(q, "raw", k)
            assert got.shape == (4 * n, 6) and np.array_equal(got, want), (q, k)
            assert np.array_equal(r["raw"][q][k], want)
        # where a tensor is not bitwise symmetric, "31" is entry 6 and "12" entry 1, not their transposes: ENTRIES says so
        full = r["kept"][KEEP[1]][name].reshape(-1, 9)
        print(f"{name}: {int((full[:, 6] != full[:, 2]).sum() + (full[:, 1] != full[:, 3]).sum())} of {2 * len(full)} "
              f"off-diagonal pairs (31 / 13, 12 / 21) differ in their bits")
        if q == "stress":               # F S F^T / J summed in index order: without such pairs the choice of entry would go unchecked
            assert (full[:, 6] != full[:, 2]).any() and (full[:, 1] != full[:, 3]).any()
        assert not r["raw"][q][:, _dofs(solid, r["zero"])].any()
    assert np.abs(r["raw"]["strain"][:, _dofs(solid, r["tiny"])]).max() < 1e-8 < np.abs(r["raw"]["strain"]).max()
    # a partial list in the caller's order, both quantities open at once, in a context of its own
    sub = solid[::-7]
    with _context(r["desc"]) as part:
        part.stress_strain_begin(sub)
        for q in NAMES:
            part.hi_pass_begin_cells(q, sub, 3)
        for j, k in enumerate(KEEP):
            part.set_state("n", r["states"][k])
            frame = part.stress_strain_sample(frame=True)
            for q, name in NAMES.items():
                part.hi_pass_sample(q)
                got = part.hi_pass_fetch(q, "raw", j)
                assert got.shape == (4 * len(sub), 6) and np.array_equal(got, _six(frame, name)), (q, k)
                assert np.array_equal(got, r["raw"][q][k].reshape(n, 4, 6)[::-7].reshape(-1, 6))      # per cell the bits of the full list


@pytest.mark.parametrize("band", [(25.0, 1000.0), (0.0, 200.0)], ids=["bandpass", "lowpass"])
def test_filtered_frames_equal_the_host_restatement_bit_for_bit(recorded, band):
    hb = recorded["hb"]
    prm = hp.design(DT, *band)
    for q in NAMES:
        y = hp.filtfilt_rows(prm["b"], prm["a"], recorded["raw"][q], prm["zi"], prm["padlen"])
        hb.hi_pass_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
        got = np.stack([hb.hi_pass_fetch(q, "filtered", k) for k in range(FRAMES)])
        print(f"{q} {prm['btype']}: max |device - host| = {np.abs(got - y).max():.3e}, max |y| = {np.abs(y).max():.3e}, "
              f"{int((got != y).sum())} of {y.size} values differ")
        assert np.array_equal(got, y), q
        assert np.array_equal(hb.hi_pass_fetch(q, "raw", 3), recorded["raw"][q][3])              # the raw history is kept


def test_amplitudes_against_the_host_restatement(recorded):
    """The rule of tests/test_gpu_hi_pass.py::test_amplitudes_against_the_host_restatement, unchanged: distance 0 from the
    running-sum restatement (the device's summation), at most 4 x the host's own direct-versus-running spread from the
    reference's direct sum; the padding frames are zero.  Measured on an MI355X: spread 6.9e-18 (strain, amplitudes up to 7.5e-3)
    and 5.9e-11 (stress, up to 4.0e4), the device at exactly that distance from the direct sum; the test prints the figures."""
    hb = recorded["hb"]
    prm = hp.design(DT, 25.0, 1000.0)
    for q in NAMES:
        y = hp.filtfilt_rows(prm["b"], prm["a"], recorded["raw"][q], prm["zi"], prm["padlen"])
        direct, running = hp.windowed_rms_rows(y, WINDOW), hp.windowed_rms_running(y, WINDOW)
        spread = np.abs(direct - running).max()
        hb.hi_pass_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
        hb.hi_pass_amplitude(q, WINDOW)
        amp = np.stack([hb.hi_pass_fetch(q, "amplitude", k) for k in range(FRAMES)])
        err = np.abs(amp - direct).max()
        print(f"{q}: host direct vs running spread {spread:.3e}, device vs direct {err:.3e}, device vs running "
              f"{np.abs(amp - running).max():.3e}, max amplitude {direct.max():.3e}")
        assert spread > 0
        assert np.array_equal(amp, running), q
        assert err <= 4 * spread, q
        assert not np.isnan(amp).any() and (amp >= 0).all()
        pad = (WINDOW - 1) // 2
        assert not amp[:pad].any() and not amp[pad + FRAMES - WINDOW + 1:].any() and amp[pad:pad + FRAMES - WINDOW + 1].any(axis=(1, 2)).all()
        for k in (FRAMES - 6, 30, 3, 30, 31):                  # a frame's value does not depend on the order of the fetches
            assert np.array_equal(hb.hi_pass_fetch(q, "amplitude", k), amp[k]), (q, k)


def _check_principal(got, six, label, cast=0.0):
    """The host applies the < 1e-8 test to the device's own frame ``six`` (dofs, 6): exactly 0.0 on the shortcut dofs; elsewhere
    the rule of tests/test_gpu_stress_strain.py::_check_against_oracle for a principal value - within 1e-7 * scale of the
    closed form restated on the host, or, where the closed form itself misses LAPACK by more than that, within ten times
    the closed form's own miss plus 1e-7 * scale of LAPACK.  ``cast``: the relative distance a cast of ``got`` on its way here may
    have added (half a float32 ulp for a value read back from a file).  Returns the shortcut mask."""
    from oracle.post_oracle import kopp_max_eigenvalue
    T = hpt.expand(six).reshape(-1, 3, 3)
    small = (np.abs(T) < 1e-8).all(axis=(1, 2))
    assert got.shape == (len(T),)
    assert np.array_equal(got[small], np.zeros(small.sum())) and not np.signbit(got[small]).any()
    if (~small).any():
        closed, lapack = kopp_max_eigenvalue(T[~small]), np.linalg.eigvalsh(T[~small])[:, -1]
        scale, tol = np.abs(closed).max(), 1e-7
        slack = cast * np.abs(closed).max()
        err = np.abs(got[~small] - closed).max()
        print(f"{label}: {small.sum()} of {len(T)} dofs take the shortcut; device vs closed form {err:.3e} = {err / (tol * scale):.3e} of the bound "
              f"(scale {scale:.3e}), closed form vs LAPACK {np.abs(closed - lapack).max():.3e}")
        if err > tol * scale + slack:
            own = np.abs(closed - lapack).max()
            assert own > tol * scale, label                     # only where the closed form is that ill-conditioned
            assert np.abs(got[~small] - lapack).max() <= 10 * own + tol * scale + slack, label
    return small


def test_principal_amplitude(recorded):
    hb, solid = recorded["hb"], recorded["solid"]
    zero, tiny = _dofs(solid, recorded["zero"]), _dofs(solid, recorded["tiny"])
    prm = hp.design(DT, 25.0, 1000.0)
    for q in NAMES:
        hb.hi_pass_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
        hb.hi_pass_amplitude(q, WINDOW)
        for k in (1, 5, 24, FRAMES - 5, FRAMES - 2):          # two of them padding frames: every amplitude is zero there
            amp = hb.hi_pass_fetch(q, "amplitude", k)
            mag, mx, am = hb.hi_pass_fetch(q, "magnitude", k, with_max=True)
            amp2, mx2, am2 = hb.hi_pass_fetch(q, "amplitude", k, with_max=True)
            assert np.array_equal(amp, amp2) and (mx, am) == (mx2, am2)
            small = _check_principal(mag, amp, f"{q} frame {k}")
            assert mx == mag.max() and am == int(np.argmax(mag)), (q, k)
            if 3 <= k <= FRAMES - 5:
                assert small[zero].all() and not small.all()
                # both kinds occur: cells without displacement, and cells whose strain amplitudes lie near 1e-9
                assert (small[tiny].all() and amp[tiny].any() and 1e-11 < amp[tiny].max() < 1e-8) if q == "strain" else not small[tiny].all()
            else:
                assert small.all() and mx == 0.0 and am == 0
    # window 0, the reference's low-pass case: the rule applied to the filtered tensor itself
    low = hp.design(DT, 0.0, 200.0)
    for q in NAMES:
        hb.hi_pass_filter(q, low["b"], low["a"], low["zi"], low["padlen"])
        hb.hi_pass_amplitude(q, 0)
        y = hb.hi_pass_fetch(q, "filtered", 9)
        assert np.array_equal(hb.hi_pass_fetch(q, "amplitude", 9), y) and (y < 0).any()
        mag, mx, am = hb.hi_pass_fetch(q, "magnitude", 9, with_max=True)
        small = _check_principal(mag, y, f"{q} low-pass frame 9")
        assert small[zero].all() and not small.all() and mx == mag.max() and am == int(np.argmax(mag))


def test_session_errors(recorded, cylinder_case):
    from vasp_amd.capi import FsiError, _ptr
    hb0, desc, solid = recorded["hb"], recorded["desc"], recorded["solid"]
    fluid = np.nonzero(np.asarray(desc["cell_kind"]) == 0)[0]
    prm = hp.design(DT, 25.0, 1000.0)
    with pytest.raises(FsiError, match="history is full"):
        hb0.hi_pass_sample("strain")
    with pytest.raises(FsiError, match="no point traces"):
        hb0.hi_pass_trace("stress", "raw", [0, 1])
    with _context(desc) as hb:
        with pytest.raises(FsiError, match="fsi_band_begin_cells first"):
            hb.hi_pass_sample("strain")
        with pytest.raises(FsiError, match="not a solid cell"):
            hb.hi_pass_begin_cells("strain", np.concatenate([solid[:3], fluid[:1]]), 4)
        bad = np.array([len(hb.cell_u2i) + 5], dtype=np.int32)
        for value in (bad[0], -1):
            bad[0] = value
            with pytest.raises(FsiError, match="cell out of range"):
                hb._check(hb.lib.fsi_band_begin_cells(hb.ctx, 3, 1, _ptr(bad), 4))
        with pytest.raises(FsiError, match=r"quantity must be 0 \(d\), 1 \(v\) or 2 \(p\)"):
            hb.hi_pass_begin("strain", [0], None, 4)
        with pytest.raises(FsiError, match=r"quantity must be 3 \(strain\) or 4 \(stress\)"):
            hb._check(hb.lib.fsi_band_begin_cells(hb.ctx, 0, 1, _ptr(np.array(hb.cell_u2i[solid[:1]], dtype=np.int32)), 4))
        with pytest.raises(FsiError, match="fsi_band_begin_cells first"):
            hb.hi_pass_sample("stress")
        # a refused begin leaves the open session's frames as they were, and the next sample goes behind them
        hb.hi_pass_begin_cells("stress", solid[:40], 34)
        for k in range(2):
            hb.set_state("n", recorded["states"][k])
            hb.hi_pass_sample("stress")
        second = recorded["raw"]["stress"][1].reshape(len(solid), 24)[:40].reshape(-1, 6)
        assert np.array_equal(hb.hi_pass_fetch("stress", "raw", 1), second)
        with pytest.raises(FsiError, match="not a solid cell"):
            hb.hi_pass_begin_cells("stress", fluid[:2], 8)
        total_b = hb.device_memory()[1]
        with pytest.raises(FsiError, match=r"needs \d+ bytes \(960 rows x \d+ frames, raw and filtered\), the device has \d+ bytes free"):
            hb.hi_pass_begin_cells("stress", solid[:40], int(total_b // (8 * 960)) + 1)      # the raw history alone exceeds the device
        assert np.array_equal(hb.hi_pass_fetch("stress", "raw", 1), second)
        for k in range(2, 33):
            hb.set_state("n", recorded["states"][k])
            hb.hi_pass_sample("stress")
        assert np.array_equal(hb.hi_pass_fetch("stress", "raw", 1), second)
        assert np.array_equal(hb.hi_pass_fetch("stress", "raw", 32), recorded["raw"]["stress"][32].reshape(len(solid), 24)[:40].reshape(-1, 6))
        with pytest.raises(FsiError, match="33 recorded frames, the filter needs more than padlen = 33"):
            hb.hi_pass_filter("stress", prm["b"], prm["a"], prm["zi"], prm["padlen"])
        with pytest.raises(FsiError, match="fsi_band_filter first"):
            hb.hi_pass_fetch("stress", "filtered", 0)
        hb.hi_pass_sample("stress")
        with pytest.raises(FsiError, match="history is full"):
            hb.hi_pass_sample("stress")
        hb.hi_pass_filter("stress", prm["b"], prm["a"], prm["zi"], prm["padlen"])
        with pytest.raises(FsiError, match="fsi_band_amplitude first"):
            hb.hi_pass_fetch("stress", "magnitude", 0)
        with pytest.raises(FsiError, match="no point traces"):
            hb.hi_pass_trace("stress", "filtered", [0])
        hb.hi_pass_end("stress")
        with pytest.raises(FsiError, match="fsi_band_begin_cells first"):
            hb.hi_pass_sample("stress")
        # nothing left a fault behind: the context still computes
        hb.stress_strain_begin(solid)
        assert np.array_equal(_six(hb.stress_strain_sample(frame=True), "TrueStress"), recorded["raw"]["stress"][32])      # the state set last


def test_side_by_side_with_every_other_session(recorded):
    """d, v, p band sessions, the stress / strain session and the hemodynamics session beside the two tensor sessions: each
    output is bitwise that of a context that runs its sessions alone."""
    from vasp_amd.hemodynamics import fluid_boundary_facets
    mesh, desc, solid, states = recorded["mesh"], recorded["desc"], recorded["solid"], recorded["states"]
    low = hp.design(DT, 0.0, 200.0)
    frames = low["padlen"] + 2
    _, cells, local = fluid_boundary_facets(mesh, 1)

    def run(tensors, others):
        out = {}
        with _context(desc) as hb:
            if others:
                hb.hemodynamics_begin(cells, local, 3.5e-3, DT)
                hb.stress_strain_begin(solid)
                for q in "dvp":
                    hb.hi_pass_begin(q, *hp.output_nodes(mesh, 2, q), capacity=frames)
            if tensors:
                for q in NAMES:
                    hb.hi_pass_begin_cells(q, solid, frames)
            for k in range(frames):
                hb.set_state("n", states[k])
                if others:
                    hb.hemodynamics_sample()
                    out["frame"] = hb.stress_strain_sample(frame=True)
                for q in (list("dvp") if others else []) + (list(NAMES) if tensors else []):
                    hb.hi_pass_sample(q)
            if others:
                out["hemo"] = hb.hemodynamics_indices()
                out["avg"] = hb.stress_strain_averages()
            for q in (list("dvp") if others else []) + (list(NAMES) if tensors else []):
                hb.hi_pass_filter(q, low["b"], low["a"], low["zi"], low["padlen"])
                hb.hi_pass_amplitude(q, WINDOW)
                out[q] = [hb.hi_pass_fetch(q, "raw", frames - 1), hb.hi_pass_fetch(q, "filtered", 7), hb.hi_pass_fetch(q, "amplitude", 9),
                          *hb.hi_pass_fetch(q, "magnitude", 9, with_max=True)]
        return out

    def same(a, b):
        if isinstance(a, dict):
            return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)

    together, tensors, others = run(True, True), run(True, False), run(False, True)
    assert set(together) == set(tensors) | set(others) and set(tensors) == set(NAMES)
    for key in together:
        assert same(together[key], (tensors if key in NAMES else others)[key]), key
    for q in NAMES:
        assert np.array_equal(together[q][0], recorded["raw"][q][frames - 1]) and together[q][2].any()


def test_history_continues_from_exported_frames(recorded):
    hb, desc, solid, states = recorded["hb"], recorded["desc"], recorded["solid"], recorded["states"]
    from vasp_amd.capi import FsiError
    prm = hp.design(DT, 25.0, 1000.0)
    split = 20
    want = {}
    for q in NAMES:
        hb.hi_pass_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
        hb.hi_pass_amplitude(q, WINDOW)
        want[q] = ([hb.hi_pass_fetch(q, "filtered", k) for k in range(FRAMES)],
                   [hb.hi_pass_fetch(q, "magnitude", k, with_max=True) for k in range(FRAMES)],
                   [hb.hi_pass_fetch(q, "amplitude", k) for k in range(FRAMES)])
    exported = {q: hb.hi_pass_export(q, 0, split) for q in NAMES}
    assert all(np.array_equal(exported[q], recorded["raw"][q][:split]) for q in NAMES)
    with _context(desc) as b:
        for q in NAMES:
            b.hi_pass_begin_cells(q, solid[:-1], FRAMES)
            with pytest.raises(FsiError, match="hi_pass_import: frames of shape"):
                b.hi_pass_import(q, exported[q])                   # a session on a shorter cell list
            with pytest.raises(FsiError, match="needs count >= 1"):   # the C side refuses what it can see
                b.hi_pass_import(q, exported[q][:0, :4 * (len(solid) - 1)])
            b.hi_pass_begin_cells(q, solid, FRAMES)
            b.hi_pass_import(q, exported[q])
        for k in range(split, FRAMES):
            b.set_state("n", states[k])
            for q in NAMES:
                b.hi_pass_sample(q)
        for q in NAMES:
            assert np.array_equal(b.hi_pass_export(q, 0, FRAMES), recorded["raw"][q])
            b.hi_pass_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
            b.hi_pass_amplitude(q, WINDOW)
            for k in range(FRAMES):
                assert np.array_equal(b.hi_pass_fetch(q, "filtered", k), want[q][0][k]), (q, k)
                mag, mx, am = b.hi_pass_fetch(q, "magnitude", k, with_max=True)
                assert np.array_equal(mag, want[q][1][k][0]) and (mx, am) == want[q][1][k][1:], (q, k)
                assert np.array_equal(b.hi_pass_fetch(q, "amplitude", k), want[q][2][k]), (q, k)


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

E2E_ARGV = ["--stress-strain", "--hi-pass-tensor", "strain", "stress", "--hi-pass-bands", "0", "200", "--hi-pass-amplitude",
            "--hi-pass-tensor-window", "8"]


def _child(cwd, extra, limit=300):
    """One run of the driver in a fresh child process under its own time limit (sized as the end-to-end run of
    tests/test_gpu_session_restart.py: 24 saved frames, more than the low-pass padlen of 18)."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "vasp_amd.monolithic", "-p", "tensor_case", "-dt", "0.001", "-T", "0.0235",
           "--theta", "0.51", "--verbose", "False", "--save-step", "1", "--save-deg", "1", "--checkpoint-step", "5", *E2E_ARGV, *extra,
           "--new-arguments", f"mesh_path={CYL}"]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _datasets(path):
    from vasp_amd.h5lite import Dataset, read_h5
    out = {}

    def walk(g, prefix):
        for k in g.keys():
            if isinstance(g[k], Dataset):
                out[prefix + k] = np.asarray(g[k].data)
            else:
                walk(g[k], prefix + k + "/")

    walk(read_h5(path), "")
    return out


def _stress_strain_series(folder, name):
    """The frames of a series of StressStrain/ in the XDMF's order, each from the file the XDMF names."""
    from vasp_amd.h5lite import read_h5
    from vasp_amd.hemodynamics import xdmf_frames
    listed = xdmf_frames(folder / f"{name}.xdmf")
    files = {f: read_h5(folder / f)[name] for f in sorted({f for _, f, _ in listed})}
    return [t for t, _, _ in listed], np.stack([np.asarray(files[f][f"{name}_{k}"]["vector"].data) for _, f, k in listed]), sorted(files)


def test_end_to_end_split_by_a_checkpoint_and_a_restart(tmp_path, cylinder_case):
    """--stress-strain --hi-pass-tensor strain stress --hi-pass-bands 0 200 --hi-pass-amplitude --hi-pass-tensor-window 8 on
    the cylinder: the first child is stopped by killturtle in its 11th step, the second continues it under --restart-folder
    to 24 frames.  The run's own recorded frames are those of StressStrain/ (bitwise, test_raw_frames_...), in both files of
    each series.  The filtered and the amplitude files (low-pass: the amplitude is the filtered tensor) hold float32 of the
    host restatement of those frames, exactly; and every file of Visualization_hi_pass/ holds the bytes that ONE unsplit
    session forms from the same frames (imported in one go into a fresh context, written by the driver's own class)."""
    (tmp_path / "tensor_case.py").write_text(HOOK_PROBLEM)
    res = tmp_path / "split" / "case" / "1"
    log1 = _child(tmp_path, ["--folder", str(res.parent), "--sub-folder", "1"])
    assert "killturtle found" in log1 and "Solved for timestep 11," in log1 and "Solved for timestep 12," not in log1
    manifest = json.loads((res / "Checkpoint" / "sessions" / "sessions.json").read_text())
    assert manifest["counter"] == 10 and sorted(manifest["sessions"]) == ["hi_pass_tensor", "stress_strain"]
    entry = manifest["sessions"]["hi_pass_tensor"]
    assert entry["frames"] == 11 and sorted(entry["quantities"]) == ["strain", "stress"]
    mesh, desc = cylinder_case[0]["mesh"], cylinder_case[1]
    solid = _solid(desc)
    n = len(solid)
    assert entry["quantities"]["strain"]["rows"] == 24 * n and entry["quantities"]["strain"]["cells"] == hp.sha256_of(solid)
    for q in NAMES:
        assert (res / "Checkpoint" / "sessions" / f"hi_pass_tensor_{q}.f64").stat().st_size == 8 * 24 * n * 11
    log2 = _child(tmp_path, ["--restart-folder", str(res)])
    out = res / "Visualization_hi_pass"
    assert "Hi-pass tensors of 24 frames (strain, stress) written to" in log2 and "Stress and strain of 24 frames" in log2
    low = hp.design(1e-3, 0.0, 200.0)
    info = ("cell_dofs", "cells", "mesh/geometry", "mesh/topology", "x_cell_dofs")
    expect = set()
    rows = {}
    for q, name in NAMES.items():
        times, x, files = _stress_strain_series(res / "StressStrain", name)
        assert files == [f"{name}.h5", f"{name}_run_1.h5"] and x.shape == (24, 36 * n, 1)
        rows[q] = x.reshape(24, 4 * n, 9)[:, :, ENTRIES]
        y = hp.filtfilt_rows(low["b"], low["a"], rows[q], low["zi"], low["padlen"])
        viz = f"{name}_0_to_200"
        want9 = np.stack([hpt.expand(f) for f in y]).reshape(24, -1).astype(np.float32)
        ss = _datasets(res / "StressStrain" / f"{name}.h5")
        mp = _datasets(res / "StressStrain" / "MaxPrincipalStrain.h5")
        for suffix, ncomp in (("", 9), ("_amplitude", 9), ("_max_principal_amplitude", 1)):
            v = viz + suffix
            expect |= {v + ".h5", v + ".xdmf"}
            d = _datasets(out / f"{v}.h5")
            assert sorted(d) == sorted([f"{v}/{v}_{k}/vector" for k in range(24)] + [f"{v}/{v}_0/{i}" for i in info]), v
            src, sname = (ss, name) if ncomp == 9 else (mp, "MaxPrincipalStrain")
            for i in info:
                a, b = d[f"{v}/{v}_0/{i}"], src[f"{sname}/{sname}_0/{i}"]
                assert a.dtype == b.dtype and np.array_equal(a, b), (v, i)
            got = np.stack([d[f"{v}/{v}_{k}/vector"] for k in range(24)])
            assert got.dtype == np.float32 and got.shape == (24, 4 * n * ncomp, 1)
            if ncomp == 9:
                assert np.array_equal(got[:, :, 0], want9), v
            else:
                for k in (0, 9, 23):
                    _check_principal(got[k, :, 0].astype(np.float64), y[k], f"{v} frame {k}", cast=0.5 * np.finfo(np.float32).eps)
            text = (out / f"{v}.xdmf").read_text()
            assert text.count("<Grid Name=") == 24 and f'<Topology NumberOfElements="{n}" TopologyType="Tetrahedron"' in text
            assert [float(t) for t in __import__("re").findall(r'<Time Value="(.+?)" />', text)] == [k * 1e-3 for k in range(24)]
        expect.add(viz + ".csv")
        table = np.loadtxt(out / f"{viz}.csv", delimiter=",")
        assert table.shape == (24, 13) and (out / f"{viz}.csv").read_text().splitlines()[0] == "# " + hp.CSV_HEADER
    assert sorted(p.name for p in out.iterdir()) == sorted(expect)
    # one unsplit session on the same frames, written by the driver's class into a folder of its own
    from conftest import prepare_case
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        ns, rdesc, *_ = prepare_case("cylinder", CYL, tmp_path / "replay" / "case", T="0.0235",
                                     extra=["save_step=1", "hi_pass_tensor=['strain','stress']", "hi_pass_bands=[0,200]", "hi_pass_amplitude=True",
                                            "hi_pass_tensor_window=8"])
    rep = tmp_path / "replay" / "case" / "1" / "Visualization_hi_pass"
    with _context(rdesc) as hb:
        run = hpt.HiPassTensorRun(hb, ns["mesh"], ns)
        for q in NAMES:
            hb.hi_pass_import(q, rows[q])
        run.frames = 24
        lines = []
        run.finish(lines.append)
    assert any("Hi-pass tensors of 24 frames" in line for line in lines)
    assert sorted(p.name for p in rep.iterdir()) == sorted(expect)
    for name in sorted(expect):
        if name.endswith(".h5"):
            a, b = _datasets(out / name), _datasets(rep / name)
            assert sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a), name
        else:
            assert (out / name).read_bytes() == (rep / name).read_bytes(), name
