"""The spectrogram session of the wall shear stress on the device (k_spec_wss_sample in csrc/fsi_hemo.hip,
fsi_spec_begin_wss, ``--spectrogram wss``) against the project's WSS kernel (bit for bit), ``oracle.post_oracle``, scipy and
the host twin of the session; strips, export / import, refusals and the run end to end.

Bounds: the recorded rows ARE the WSS kernel's values (one device function, ``wss_dg1_cell``): ``np.array_equal``.  Against the
oracle the x / y / z rows are held to ``1e-10 * max|ref|``, the bound test_wall_shear_stress_kernel_matches_oracle uses for
this arithmetic.  The transforms are held to ``power_bound`` (tests/test_spectrogram.py) against scipy and to its
accumulation part against ``HostSpecSession``, both formed on the rows fetched from the device: the kernel under test is the
sampler, not the transform."""
import contextlib
import ctypes as C
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_spectrogram import host_session, power_bound, scipy_periodogram_rows, scipy_spectrogram_rows
from vasp_amd import hi_pass as hp
from vasp_amd import spectrogram as sp

pytestmark = pytest.mark.gpu

MU = 3.5e-3
CYL = GOLDEN / "cylinder" / "cylinder.h5"
FRAMES = 333                       # odd; no multiple of 4, 16 or 64
FS = 1000.0
K, NOV, NFFT = 90, 67, 180         # 91 bins, 11 segments: no multiple of the MFMA tile in any dimension
SPLIT = 17


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _velocity_state(ndof, mesh, v):
    U = np.zeros(ndof)
    U[3 * mesh.num_nodes:6 * mesh.num_nodes] = np.asarray(v).reshape(-1)
    return U


@pytest.fixture(scope="module")
def cyl(cylinder_case):
    from vasp_amd.capi import HipBackend
    from vasp_amd.hemodynamics import fluid_boundary_facets
    mesh = cylinder_case[0]["mesh"]
    hb = HipBackend(cylinder_case[1])
    _, cell, local = fluid_boundary_facets(mesh, 1)
    yield hb, mesh, cell, local
    hb.close()


def _row_list(nd, rng):
    """Every dof's x, y and z (component-major), every dof's magnitude, a shuffled block of dofs drawn with replacement with
    any of the four codes, and a tail that makes the count = 37 (mod 128)."""
    every = np.arange(nd)
    pick = rng.choice(nd, 200)
    assert len(np.unique(pick)) < len(pick)
    dofs = np.concatenate([np.tile(every, 3), every, pick])
    comps = np.concatenate([np.repeat([0, 1, 2], nd), np.full(nd, 3), rng.integers(0, 4, 200)])
    tail = (37 - len(dofs)) % 128
    dofs = np.concatenate([dofs, rng.choice(nd, tail)])
    comps = np.concatenate([comps, rng.integers(0, 4, tail)])
    assert len(dofs) % 128 == 37
    return dofs.astype(np.int32), comps.astype(np.int32)


@pytest.fixture(scope="module")
def recorded(cyl):
    """Three random velocity states; one session on the long row list; per state the frame it recorded and the WSS kernel's
    values of the same state."""
    hb, mesh, cell, local = cyl
    rng = np.random.default_rng(31)
    nd = 3 * len(cell)
    dofs, comps = _row_list(nd, rng)
    vs = [rng.standard_normal((mesh.num_nodes, 3)) for _ in range(3)]
    hb.spec_begin_wss(cell, local, MU, dofs, comps, capacity=3)
    taus = []
    for v in vs:
        hb.set_state("n", _velocity_state(hb.ndof, mesh, v))
        hb.spec_sample("wss")
        taus.append(hb.wall_shear_stress(cell, local, MU))
    frames = [hb.spec_fetch("wss", k) for k in range(3)]
    assert np.array_equal(hb.spec_export("wss", 0, 3), np.stack(frames))
    hb.spec_end("wss")
    hb.set_state("n", np.zeros(hb.ndof))
    return dofs, comps, vs, taus, frames


# ---- 1. recorded bits -------------------------------------------------------------------------------------------------

def test_recorded_rows_are_the_bits_of_the_wall_shear_stress_kernel(cyl, recorded):
    hb, mesh, cell, local = cyl
    dofs, comps, vs, taus, frames = recorded
    nd = 3 * len(cell)
    per_cell = np.unique(cell, return_counts=True)[1]
    assert (per_cell == 1).any() and (per_cell > 1).any()                      # the inlet rim: cells with several exterior facets
    from oracle.post_oracle import wall_shear_stress
    for v, tau, got in zip(vs, taus, frames):
        values = tau.reshape(nd, 3)                                            # dof 3 f + k: vertex k of facet f
        table = np.column_stack([values, sp.component_rows(values, "mag")])
        assert got.shape == (len(dofs),) and np.abs(got).max() > 0
        assert np.array_equal(got[:3 * nd], sp.component_rows(values, "all"))
        assert np.array_equal(got[3 * nd:4 * nd], sp.component_rows(values, "mag"))
        assert np.array_equal(got, table[dofs, comps])
        ref = wall_shear_stress(mesh.coords, mesh.tets, mesh.tet_nodes, v, cell, local, MU).reshape(nd, 3)
        err = np.abs(got[:3 * nd] - sp.component_rows(ref, "all")).max()
        print(f"x / y / z rows against the oracle: {err / np.abs(ref).max():.3e} of max|ref|")
        assert err <= 1e-10 * np.abs(ref).max()


# ---- 2. a sub-list records what the full list records -----------------------------------------------------------------

def test_five_scattered_dofs_record_the_entries_of_the_full_session(cyl, recorded):
    """Most boundary cells are untouched, and one touched cell has several exterior facets of which one dof is sampled: its
    mask must still be the cell's full one."""
    hb, mesh, cell, local = cyl
    _, _, vs, taus, _ = recorded
    cells, counts = np.unique(cell, return_counts=True)
    rim = int(np.nonzero(cell == cells[counts > 1][0])[0][0])                  # a facet of a cell with several exterior facets
    single = np.nonzero(np.isin(cell, cells[counts == 1]))[0]
    facets = [rim, *single[[0, len(single) // 3, len(single) // 2, len(single) - 1]]]
    dofs = np.array([3 * f + k for f, k in zip(facets, (1, 0, 2, 1, 0))], dtype=np.int32)
    comps = np.array([0, 1, 2, 3, 1], dtype=np.int32)
    assert len(np.unique(cell[facets])) == 5 < len(cells)
    hb.spec_begin_wss(cell, local, MU, dofs, comps, capacity=3)
    try:
        for v, tau in zip(vs, taus):
            hb.set_state("n", _velocity_state(hb.ndof, mesh, v))
            hb.spec_sample("wss")
        for k, tau in enumerate(taus):
            values = tau.reshape(-1, 3)
            table = np.column_stack([values, sp.component_rows(values, "mag")])
            assert np.array_equal(hb.spec_fetch("wss", k), table[dofs, comps]), k
    finally:
        hb.spec_end("wss")
        hb.set_state("n", np.zeros(hb.ndof))


# ---- 3. - 5. a driven history: transforms, strips, export / import ----------------------------------------------------

def _signal(n, frames=FRAMES, seed=11):
    """(frames, n): per entry a mean of order 1e4, a slow carrier, a tone with its own frequency and noise of its own level."""
    rng = np.random.default_rng(seed)
    f, ph = rng.uniform(40.0, 450.0, n), rng.uniform(0.0, 2 * np.pi, n)
    t = (1 + np.arange(frames))[:, None] / FS
    return 1e4 * rng.uniform(-1, 1, n) + 50 * np.sin(2 * np.pi * 7 * t + ph) + np.sin(2 * np.pi * f * t + 2 * ph) \
        + rng.uniform(0.01, 1, n) * rng.standard_normal((frames, n))


def _record(hb, mesh, vel, frames=range(FRAMES)):
    for k in frames:
        hb.set_state("n", _velocity_state(hb.ndof, mesh, vel[k]))
        hb.spec_sample("wss")


def _powers(hb, call):
    """The spectrogram and the periodogram of the high-passed and of the raw rows: ``call(kind, *args)``."""
    prm = sp.highpass_design(FS, 25.0)
    w, wp = sp.window_values("blackmanharris", K), sp.window_values("blackmanharris", FRAMES)
    out = {}
    for filtered in (True, False):
        hb.spec_filter("wss", prm["b"], prm["a"], prm["zi"], prm["padlen"]) if filtered else hb.spec_filter("wss")
        out["spectrogram", filtered] = call("spectrogram", ("spectrogram", filtered), K, NOV, NFFT, w, "spectrum", FS)
        out["periodogram", filtered] = call("periodogram", ("periodogram", filtered), wp, "density", FS)
    return out


@pytest.fixture(scope="module")
def driven(cyl):
    """333 frames of a prescribed time-varying velocity; 150 dofs drawn with replacement, their three components stacked, and
    the magnitudes of 87 more: 537 rows, no multiple of 128.  One session on all rows: its history and its four powers."""
    hb, mesh, cell, local = cyl
    rng = np.random.default_rng(41)
    nd = 3 * len(cell)
    a, b = rng.choice(nd, 150), rng.choice(nd, 87)
    dofs = np.concatenate([np.tile(a, 3), b]).astype(np.int32)
    comps = np.concatenate([np.repeat([0, 1, 2], 150), np.full(87, 3)]).astype(np.int32)
    vel = _signal(3 * mesh.num_nodes)
    hb.spec_begin_wss(cell, local, MU, dofs, comps, capacity=FRAMES)
    _record(hb, mesh, vel)
    x = hb.spec_export("wss", 0, FRAMES)
    whole = _powers(hb, lambda kind, key, *args: getattr(hb, f"spec_{kind}")("wss", *args))
    again = _powers(hb, lambda kind, key, *args: getattr(hb, f"spec_{kind}")("wss", *args))
    prm = sp.highpass_design(FS, 25.0)
    hb.spec_filter("wss", prm["b"], prm["a"], prm["zi"], prm["padlen"])
    filtered = np.stack([hb.spec_fetch("wss", k, True) for k in (0, 17, FRAMES - 1)])
    hb.spec_end("wss")
    hb.set_state("n", np.zeros(hb.ndof))
    return dofs, comps, vel, x, whole, again, filtered


@pytest.mark.parametrize("filtered", [False, True], ids=["raw", "highpassed"])
def test_transforms_of_the_recorded_rows_against_scipy_and_the_host_session(driven, filtered):
    dofs, comps, vel, x, whole, again, fetched = driven
    assert x.shape == (FRAMES, 537) and np.isfinite(x).all() and (np.abs(x).max(axis=0) > 0).all()
    w, wp = sp.window_values("blackmanharris", K), sp.window_values("blackmanharris", FRAMES)
    host = host_session(x)
    src = x
    if filtered:
        prm = sp.highpass_design(FS, 25.0)
        host.filter(prm["b"], prm["a"], prm["zi"], prm["padlen"])
        src = host.filtered
        assert np.array_equal(fetched, src[[0, 17, FRAMES - 1]])              # launch_band_filter: scipy's filtfilt bit for bit
    got = whole["spectrogram", filtered]
    ref_rows = scipy_spectrogram_rows(src, FS, K, NOV, NFFT, "blackmanharris", "spectrum")
    bound = power_bound(src, ref_rows, w, K, K - NOV, NFFT, "spectrum", FS)
    part = power_bound(src, ref_rows, w, K, K - NOV, NFFT, "spectrum", FS, accumulation_only=True)
    e_ref, e_twin = np.abs(got - ref_rows.mean(axis=0)), np.abs(got - host.spectrogram(K, NOV, NFFT, w, "spectrum", FS))
    print(f"wss {'filtered' if filtered else 'raw'} spectrogram: share of the bound against scipy {(e_ref / bound).max():.3e}, of its "
          f"accumulation part against the host twin {(e_twin / part).max():.3e}")
    assert got.shape == (NFFT // 2 + 1, (FRAMES - NOV) // (K - NOV)) and (got > 0).all()
    assert (e_ref <= bound).all() and (e_twin <= part).all()
    got = whole["periodogram", filtered]
    ref_rows = scipy_periodogram_rows(src, FS, "density")
    bound = power_bound(src, ref_rows, wp, FRAMES, FRAMES, FRAMES, "density", FS)[:, 0]
    part = power_bound(src, ref_rows, wp, FRAMES, FRAMES, FRAMES, "density", FS, accumulation_only=True)[:, 0]
    e_ref, e_twin = np.abs(got - ref_rows.mean(axis=0)[:, 0]), np.abs(got - host.periodogram(wp, "density", FS))
    print(f"wss {'filtered' if filtered else 'raw'} periodogram: share against scipy {(e_ref / bound).max():.3e}, against the host twin "
          f"{(e_twin / part).max():.3e}")
    assert got.shape == (FRAMES // 2 + 1,) and (e_ref <= bound).all() and (e_twin <= part).all()
    # the same calls again: the same bits
    for key in whole:
        assert whole[key].tobytes() == again[key].tobytes(), key
    assert not np.array_equal(whole["spectrogram", True], whole["spectrogram", False])


def test_two_strips_of_rows_carry_the_bits_of_the_unsplit_session(cyl, driven):
    hb, mesh, cell, local = cyl
    dofs, comps, vel, x, whole, _, _ = driven
    carries = {}
    for r0, r1 in ((0, 256), (256, 537)):
        hb.spec_begin_wss(cell, local, MU, dofs[r0:r1], comps[r0:r1], capacity=FRAMES)
        try:
            _record(hb, mesh, vel)
            assert np.array_equal(hb.spec_export("wss", 0, FRAMES), x[:, r0:r1]), (r0, r1)
            total = 537 if r1 == 537 else 0
            carries = _powers(hb, lambda kind, key, *args: getattr(hb, f"spec_{kind}_sum")("wss", *args, r0, total, carries.get(key)))
        finally:
            hb.spec_end("wss")
    hb.set_state("n", np.zeros(hb.ndof))
    for key in whole:
        assert carries[key].shape == whole[key].shape and carries[key].tobytes() == whole[key].tobytes(), key


def test_history_continues_from_exported_frames(cyl, driven):
    hb, mesh, cell, local = cyl
    dofs, comps, vel, x, whole, _, _ = driven
    from vasp_amd.capi import FsiError
    hb.spec_begin_wss(cell, local, MU, dofs, comps, capacity=SPLIT)
    _record(hb, mesh, vel, range(SPLIT))
    pieces = hb.spec_export("wss", 0, 10), hb.spec_export("wss", 10, SPLIT - 10)
    with pytest.raises(FsiError, match="history is full"):
        hb.spec_sample("wss")
    hb.spec_begin_wss(cell, local, MU, dofs, comps, capacity=FRAMES)          # replaces the session: a new history
    try:
        for piece in pieces:
            hb.spec_import("wss", piece)
        _record(hb, mesh, vel, range(SPLIT, FRAMES))
        assert np.array_equal(hb.spec_export("wss", 0, FRAMES), x)
        got = _powers(hb, lambda kind, key, *args: getattr(hb, f"spec_{kind}")("wss", *args))
        for key in whole:
            assert got[key].tobytes() == whole[key].tobytes(), key
    finally:
        hb.spec_end("wss")
        hb.set_state("n", np.zeros(hb.ndof))


def test_the_driver_side_continues_a_saved_history_and_refuses_another_fingerprint(cyl, cylinder_case, tmp_path):
    hb, mesh, cell, local = cyl
    base = dict(cylinder_case[0], results_folder=tmp_path / "a" / "1", spectrogram=["wss"], spectrogram_sampling="All", spectrogram_region="box",
                spectrogram_fsi_region=[-100, 100, -100, 100, -100, 100], save_step=1, save_deg=2, T=0.039, dt=0.001, t=0.0, counter=0,
                restart_folder=None)
    rng = np.random.default_rng(5)
    vs = [rng.standard_normal((mesh.num_nodes, 3)) for _ in range(4)]
    first = sp.SpectrogramRun(hb, mesh, base)
    assert first.rows("wss") == 9 * len(cell)
    for k, v in enumerate(vs[:3]):
        hb.set_state("n", _velocity_state(hb.ndof, mesh, v))
        first.sample(1e-3 * (k + 1), None)
    hp.save_sessions([first], base["results_folder"], 3e-3, 2)
    (base["results_folder"] / "Checkpoint" / "default_variables.json").write_text(json.dumps(dict(t=3e-3, counter=2)))
    saved = first.sessions["wss"].export(0, 3)
    first.sessions["wss"].end()
    again = dict(base, restart_folder=base["results_folder"], results_folder=tmp_path / "b" / "1")
    with pytest.raises(SystemExit, match=r"differs in mu \(saved 0.0035, now 0.004\)"):
        sp.SpectrogramRun(hb, mesh, dict(again, mu_f=4e-3))
    with pytest.raises(SystemExit, match=r"dofs \(saved '"):
        sp.SpectrogramRun(hb, mesh, dict(again, spectrogram_sampling="RandomPoint", spectrogram_n_samples=3 * len(cell)))
    second = sp.SpectrogramRun(hb, mesh, again)
    try:
        assert second.frames == 3 and np.array_equal(second.sessions["wss"].export(0, 3), saved)
        hb.set_state("n", _velocity_state(hb.ndof, mesh, vs[3]))
        second.sample(4e-3, None)
        tau = hb.wall_shear_stress(cell, local, MU)
        assert np.array_equal(second.sessions["wss"].fetch(3), sp.component_rows(tau.reshape(-1, 3), "all"))
    finally:
        second.sessions["wss"].end()
        hb.set_state("n", np.zeros(hb.ndof))


# ---- 6. refusals ------------------------------------------------------------------------------------------------------

def test_every_refusal_has_its_line_and_the_context_still_steps(cylinder_case):
    from vasp_amd.capi import HipBackend
    from vasp_amd.hemodynamics import fluid_boundary_facets
    ns, desc, bc_values, pressure, hook = cylinder_case
    mesh = ns["mesh"]
    _, cell, local = fluid_boundary_facets(mesh, 1)
    hb = HipBackend(desc)
    try:
        lib, ctx = hb.lib, hb.ctx
        fc = np.ascontiguousarray(hb.cell_u2i[cell], dtype=np.int32)
        fl = np.ascontiguousarray(local, dtype=np.int32)
        nf = len(fc)
        dofs, comps = np.array([0, 5, 3 * nf - 1], dtype=np.int32), np.array([0, 3, 2], dtype=np.int32)
        solid = np.ascontiguousarray(hb.cell_u2i[np.nonzero(mesh.cell_markers == ns["dx_s_id"])[0][:1]], dtype=np.int32)
        free_before = hb.device_memory()[0]

        def begin(nf=nf, fc=fc, fl=fl, mu=MU, nrows=3, dofs=dofs, comps=comps, capacity=8, ctx=ctx):
            return lib.fsi_spec_begin_wss(ctx, nf, _ptr(fc), _ptr(fl), mu, nrows, None if dofs is None else _ptr(dofs), _ptr(comps), capacity)

        def refused(rc, text, ctx=ctx):
            said = lib.fsi_last_error(ctx).decode()
            assert rc == 1 and said.startswith("fsi_spec_begin_wss: ") and text in said and "\n" not in said, said

        swap = lambda a, k, v: np.concatenate([a[:k], np.array([v], dtype=np.int32), a[k + 1:]])
        refused(begin(fc=swap(fc, 2, int(solid[0]))), "a facet's cell is not a fluid cell")
        refused(begin(fc=swap(fc, 0, len(hb.cell_u2i))), "facet cell / local index out of range")
        refused(begin(fl=swap(fl, 1, 4)), "facet cell / local index out of range")
        refused(begin(fc=swap(fc, 1, int(fc[0])), fl=swap(fl, 1, int(fl[0]))), "a facet is listed twice")
        refused(begin(dofs=swap(dofs, 1, 3 * nf)), "dof out of range")
        refused(begin(dofs=swap(dofs, 0, -1)), "dof out of range")
        refused(begin(comps=swap(comps, 2, 4)), "component out of range")
        refused(begin(comps=swap(comps, 0, -1)), "component out of range")
        refused(begin(nrows=0), "needs nrows >= 1")
        refused(begin(dofs=None), "needs nrows >= 1")
        refused(begin(capacity=0), "needs a capacity >= 1")
        refused(begin(nf=0), "needs nf > 0 facets and mu > 0")
        refused(begin(mu=0.0), "needs nf > 0 facets and mu > 0")
        total = hb.device_memory()[1]
        refused(begin(capacity=int(total // (8 * 3)) + 1), "the session needs")            # the room check of fsi_spec_begin_rows
        assert lib.fsi_spec_begin_wss(None, nf, _ptr(fc), _ptr(fl), MU, 3, _ptr(dofs), _ptr(comps), 8) == 1
        assert hb.device_memory()[0] >= free_before - (1 << 26)                            # nothing allocated
        assert lib.fsi_spec_sample(ctx, 3) == 1 and "fsi_spec_begin_wss first" in lib.fsi_last_error(ctx).decode()
        assert lib.fsi_spec_sample(ctx, 4) == 1 and "quantity must be 0 (d), 1 (v), 2 (p) or 3 (wss)" in lib.fsi_last_error(ctx).decode()
        # a refused call leaves an open session as it was
        hb.set_state("n", _velocity_state(hb.ndof, mesh, np.random.default_rng(2).standard_normal((mesh.num_nodes, 3))))
        hb.spec_begin_wss(cell, local, MU, dofs, comps, capacity=8)
        hb.spec_sample("wss")
        kept = hb.spec_fetch("wss", 0)
        refused(begin(comps=swap(comps, 2, 4)), "component out of range")
        assert np.array_equal(hb.spec_fetch("wss", 0), kept) and kept.any()
        hb.set_state("n", np.zeros(hb.ndof))
        # and the context still takes a Newton step
        run = dict(ns)
        run["t"] = float(ns["dt"])
        with contextlib.redirect_stdout(io.StringIO()):
            hook("pre_solve")(**run)
        hb.set_dirichlet_values(bc_values())
        hb.set_interface_pressure(float(pressure.P) if pressure is not None else 0.0)
        hist = hb.newton_solve(counter=0, first_step_num=0, **{k: ns[k] for k in ("atol", "rtol", "max_it", "lmbda", "recompute", "recompute_tstep")})
        assert len(hist) >= 1 and np.isfinite(hb.get_state("n")).all()
        hb.spec_sample("wss")
        assert np.array_equal(hb.spec_fetch("wss", 1), np.column_stack([t := hb.wall_shear_stress(cell, local, MU).reshape(-1, 3),
                                                                        sp.component_rows(t, "mag")])[dofs, comps])
    finally:
        hb.close()


def test_a_partitioned_context_is_refused(cylinder_case):
    """A context told that it is one part of a partition (every cell owned, nothing shared: no call of this test reaches a
    collective) takes no wall-shear-stress session."""
    from vasp_amd.capi import HipBackend
    from vasp_amd.hemodynamics import fluid_boundary_facets
    ns, desc = cylinder_case[:2]
    _, cell, local = fluid_boundary_facets(ns["mesh"], 1)
    red = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32)(lambda user, v, n: 0)
    halo = C.CFUNCTYPE(C.c_int, C.c_void_p)(lambda user: 0)

    class FsiComm(C.Structure):
        _fields_ = [("user", C.c_void_p), ("allreduce_sum", type(red)), ("halo_exchange", type(halo))]

    comm = FsiComm(None, red, halo)
    hb = HipBackend(desc)
    try:
        fc = np.ascontiguousarray(hb.cell_u2i[cell], dtype=np.int32)
        fl = np.ascontiguousarray(local, dtype=np.int32)
        dofs, comps = np.array([0, 5], dtype=np.int32), np.array([0, 3], dtype=np.int32)
        hb._check(hb.lib.fsi_set_partition(hb.ctx, len(hb.cell_u2i), 0, None, 0, None, 0, None, None, None, C.byref(comm)))
        rc = hb.lib.fsi_spec_begin_wss(hb.ctx, len(fc), _ptr(fc), _ptr(fl), MU, 2, _ptr(dofs), _ptr(comps), 8)
        assert rc == 1 and hb.lib.fsi_last_error(hb.ctx).decode() == "fsi_spec_begin_wss: partitioned contexts are not supported"
    finally:
        hb.close()


def test_destroy_without_end_leaks_nothing(cylinder_case):
    from vasp_amd.capi import HipBackend
    from vasp_amd.hemodynamics import fluid_boundary_facets
    mesh, desc = cylinder_case[0]["mesh"], cylinder_case[1]
    _, cell, local = fluid_boundary_facets(mesh, 1)
    nd = 3 * len(cell)
    hb = HipBackend(desc)
    free0 = hb.device_memory()[0]
    hb.set_state("n", 1e-4 * np.random.default_rng(4).standard_normal(hb.ndof))
    capacity = (1 << 29) // (16 * 4 * nd) + 1                                  # raw and filtered history: more than 2^29 bytes
    hb.spec_begin_wss(cell, local, MU, np.tile(np.arange(nd), 4), np.repeat([0, 1, 2, 3], nd), capacity=capacity)
    hb.spec_sample("wss")
    assert hb.device_memory()[0] < free0 - (1 << 28)            # the session holds memory ...
    hb.close()                                                  # ... no fsi_spec_end: fsi_destroy frees it
    again = HipBackend(desc)
    try:
        assert again.device_memory()[0] >= free0 - (1 << 26)
    finally:
        again.close()


# ---- 4. and 7. the run and the tool end to end ------------------------------------------------------------------------

RUN = ["-dt", "0.001", "-T", "0.0395", "--theta", "0.51", "--verbose", "False", "--save-step", "1", "--save-deg", "2", "--checkpoint-step", "39"]
SAMPLING = ["--spectrogram-sampling", "All", "--spectrogram-region", "box", "--spectrogram-fsi-region", "-100", "100", "-100", "100", "-100", "100"]


def _child(module, argv, cwd, limit):
    """One child under its own time limit; anything but exit status 0 fails the caller, which then starts nothing more."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", module, *argv], cwd=cwd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        pytest.fail(f"python -m {module} ended with status {r.returncode}:\n" + r.stdout[-3000:] + r.stderr[-3000:], pytrace=False)
    return r.stdout


@pytest.fixture(scope="module")
def finished(tmp_path_factory):
    """40 steps of the cylinder with --hemodynamics and --spectrogram v wss on every dof; a checkpoint in the last step."""
    tmp = tmp_path_factory.mktemp("wss_run")
    results = tmp / "case" / "1"
    log = _child("vasp_amd.monolithic", ["-p", "cylinder", *RUN, "--folder", str(results.parent), "--sub-folder", "1", "--hemodynamics",
                                         "--spectrogram", "v", "wss", *SAMPLING, "--new-arguments", f"mesh_path={CYL}"], tmp, 300)
    return tmp, results, log


def test_a_run_records_the_frames_that_hemodynamics_writes(finished, cylinder_case):
    from vasp_amd.h5lite import read_h5
    from vasp_amd.hemodynamics import fluid_boundary_facets, xdmf_frames
    tmp, results, log = finished
    assert "Solved for timestep 40," in log and "Spectrograms of 40 frames (v, wss; All" in log
    nd = 3 * len(fluid_boundary_facets(cylinder_case[0]["mesh"], 1)[1])
    out = results / "Spectrograms"
    for name in sp.file_names("wss_all", "case", np.float64(3.0), -18).values():
        assert (out / name).exists(), name
    assert len(list(out.iterdir())) == 8 and not list(out.glob("*.wav"))
    manifest = json.loads((results / "Checkpoint" / "sessions" / "sessions.json").read_text())
    entry = manifest["sessions"]["spectrogram"]
    assert entry["frames"] == 40 and entry["quantities"]["wss"]["rows"] == 3 * nd and entry["quantities"]["wss"]["mu"] == MU
    hist = np.fromfile(results / "Checkpoint" / "sessions" / "spectrogram_wss.f64", dtype="<f8").reshape(40, 3 * nd)
    listed = xdmf_frames(results / "Hemodynamic_indices" / "WSS.xdmf")
    assert len(listed) == 40 and listed[-1][1:] == ("WSS.h5", 39)
    series = read_h5(results / "Hemodynamic_indices" / "WSS.h5")["WSS"]
    for k in (0, 39):                                                          # component-major rows against the interleaved vector
        vector = np.asarray(series[f"WSS_{k}"]["vector"].data).reshape(nd, 3)
        assert np.abs(vector).max() > 0 and np.array_equal(hist[k].reshape(3, nd).T, vector), k


def test_the_tool_on_the_finished_folder_whole_and_in_strips(finished, cylinder_case):
    """At save_deg 2 the tool forms the run's own files; with --history-memory for three strips the same bytes again."""
    from vasp_amd import spectrogram_strips as strips
    from vasp_amd.hemodynamics import fluid_boundary_facets
    tmp, results, _ = finished
    rows = 9 * len(fluid_boundary_facets(cylinder_case[0]["mesh"], 1)[1])
    need = lambda r, capacity: sp.host_room(r, capacity)[0]
    size = -(-(-(-rows // 3)) // 128) * 128
    limit = need(size, 41)
    assert rows > 3 * 128 and len(strips.plan_row_strips(rows, 128, 41, limit, need)) == 3
    base = ["--folder", str(results), "--spectrogram", "wss", *SAMPLING]
    log = _child("vasp_amd.postprocess", [*base, "--output-folder", str(tmp / "whole")], tmp, 120)
    assert "Read 40 of 40 frames" in log and "in strips" not in log and "Spectrograms of 40 frames (wss; All" in log
    log = _child("vasp_amd.postprocess", [*base, "--output-folder", str(tmp / "split"), "--history-memory", str(limit)], tmp, 180)
    said = re.findall(r"Spectrograms of wss in strips: (\d+) strips of at most (\d+) rows \((\d+) in all\), the 40 frames read (\d+) times", log)
    assert [tuple(int(x) for x in s) for s in said] == [(3, size, rows, 3)], log[-2000:]
    names = sorted(p.name for p in (tmp / "whole" / "Spectrograms").iterdir())
    assert names == sorted(sp.file_names("wss_all", "case", np.float64(3.0), -18).values())
    assert names == sorted(p.name for p in (tmp / "split" / "Spectrograms").iterdir())
    for name in names:
        whole = (tmp / "whole" / "Spectrograms" / name).read_bytes()
        assert whole == (tmp / "split" / "Spectrograms" / name).read_bytes(), name
        assert whole == (results / "Spectrograms" / name).read_bytes(), name
