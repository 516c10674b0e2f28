"""The snapshot proper orthogonal decomposition on the device (csrc/fsi_pod.hip; fsi_band_pod_gram, fsi_band_pod_modes,
fsi_band_pod_fetch; HipBackend.hi_pass_pod_gram / hi_pass_pod_modes / hi_pass_pod_fetch; ``--hi-pass-pod``) against the NumPy
twin (vasp_amd/hi_pass.py: ``pod_gram``, ``pod_modes``, HostBandSession) and against the ``numpy.longdouble`` restatement of
tests/test_hi_pass_pod.py.

Bounds: those derived in the docstring of tests/test_hi_pass_pod.py.  Device and twin form the same mean - the same ordered sum,
compared bit for bit - and from it the same y_j and a_j bits; they differ in the order inside a slab's row sum (the matrix pipe's,
four rows at a time, against BLAS's) and inside a mode's sum over the frames.  Each lies within ``gram_bound`` / ``mode_bound``
of the restatement, and so within twice it of the other (``sides=2``).  The tests print the largest share of each bound the
device uses.

The shapes: POD_SLAB = 6144 rows are 2048 nodes of a vector, 128 rows a staging chunk, 64 frames a frame block, 16 a tile.
The histories are filled with hi_pass_import: no time step is taken but in the end-to-end run."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_hi_pass_pod import (A, B, LADDER, LD, ZI, gram_bound, mean_bound, mode_bound, node_weights, pod_reference, pod_rows,
                              same_bits, share)
from vasp_amd import hi_pass as hp

pytestmark = pytest.mark.gpu

STENOSIS = GOLDEN / "offset_stenosis" / "offset_stenosis.h5"
SLAB_NODES = hp.POD_SLAB // 3
# rows: 1 - the smallest; 129 - a staging chunk plus one row; one slab exactly; one slab and a second slab of three rows
SHAPES = (("p", 1), ("v", 43), ("v", SLAB_NODES), ("v", SLAB_NODES + 1))
# 2: the minimum; 7: less than one 16-frame step; 50: no multiple of 16; 65: a second frame block of one frame, an off-diagonal
# block pair; 130: three blocks, the pair (0, 2)
FRAMES = (2, 7, 50, 65, 130)
MODES = (1, 17, 64)                                # the minimum, a second wave's tile, the maximum


@pytest.fixture(scope="module")
def hb(cylinder_case):
    from vasp_amd.capi import HipBackend
    backend = HipBackend(cylinder_case[1])
    yield backend
    backend.close()


def _open(hb, q, nodes, x, capacity=None):
    """The session of q on the first ``nodes`` nodes with the history x, and its host twin."""
    hb.hi_pass_begin(q, np.arange(nodes, dtype=np.int32), None, capacity or len(x))
    hb.hi_pass_import(q, x)
    twin = hp.HostBandSession(x.shape[2], capacity or len(x))
    twin.import_(x)
    return twin


def _table(n, nmodes, seed):
    """A table of ``nmodes`` columns for n frames: any table is one, the kernel does not ask where it comes from."""
    return np.random.default_rng(seed).standard_normal((n, nmodes)) / np.sqrt(n)


def _modes(hb, q, count):
    return np.stack([hb.hi_pass_pod_fetch(q, "mode", m) for m in range(count)])


def _weights(nodes, weighted):
    return None if not weighted else node_weights(nodes) if nodes > 1 else np.array([0.75])


def _check_against_twin_and_reference(hb, q, x, w, source="raw", frames=None, label=""):
    """G, the mean and the modes of MODES tables on the device against the twin and the restatement on ``frames`` (the source's
    frames as the host knows them; None: x).  Returns (G, mean, modes of the 64-column table)."""
    frames = x if frames is None else frames
    n, nodes, ncomp = frames.shape
    rows = nodes * ncomp
    hb.hi_pass_pod_gram(q, source, w)
    G, mean = hb.hi_pass_pod_fetch(q, "gram"), hb.hi_pass_pod_fetch(q, "mean")
    assert G.shape == (n, n) and mean.shape == (nodes, ncomp) and same_bits(G, G.T)
    Gt, mt = hp.pod_gram(frames, w)
    assert same_bits(mean, mt)                                                       # the same ordered sum
    dm = np.abs(mean.astype(LD) - frames.astype(LD).sum(axis=0) / LD(n)).astype(np.float64)
    assert (dm <= mean_bound(frames)).all()
    T = _table(n, 64, n + rows)
    ref = pod_reference(frames, w, mean, T)
    one, two = gram_bound(ref, rows), gram_bound(ref, rows, sides=2)
    d_twin, d_ref = np.abs(G - Gt), np.abs(G.astype(LD) - ref["G"]).astype(np.float64)
    assert (d_twin <= two).all() and (d_ref <= one).all()
    shares = dict(G_twin=share(d_twin, two), G=share(d_ref, one))
    full = None
    for nmodes in MODES:
        hb.hi_pass_pod_modes(q, T[:, :nmodes])
        got = _modes(hb, q, nmodes)
        assert got.shape == (nmodes, nodes, ncomp)
        flat = got.reshape(nmodes, -1)
        want = hp.pod_modes(frames, mean, T[:, :nmodes]).reshape(nmodes, -1)
        bm = mode_bound(dict(absmodes=ref["absmodes"][:nmodes]), n)
        d_twin, d_ref = np.abs(flat - want), np.abs(flat.astype(LD) - ref["modes"][:nmodes]).astype(np.float64)
        assert (d_twin <= 2 * bm).all() and (d_ref <= bm).all(), nmodes
        shares[f"modes{nmodes}"] = share(d_ref, bm)
        full = got
    print(f"{label}{q}{nodes} n = {n} {'weights' if w is not None else 'null'}: largest shares of the bounds "
          + ", ".join(f"{k} {v:.3g}" for k, v in shares.items()))
    return G, mean, full


@pytest.mark.parametrize("n", FRAMES, ids=[f"n{n}" for n in FRAMES])
@pytest.mark.parametrize("q,nodes", SHAPES, ids=[f"{q}{n}" for q, n in SHAPES])
def test_device_against_the_twin_within_the_derived_bound(hb, q, nodes, n):
    from vasp_amd.capi import FsiError
    ncomp = 1 if q == "p" else 3
    x = pod_rows(n, (nodes, ncomp), seed=1000 * n + nodes)
    _open(hb, q, nodes, x)
    try:
        got = {}
        for weighted in (False, True):
            w = _weights(nodes, weighted)
            G, mean, modes = _check_against_twin_and_reference(hb, q, x, w)
            # the same calls again give the same bits
            hb.hi_pass_pod_gram(q, "raw", w)
            with pytest.raises(FsiError, match=r"no modes \(fsi_band_pod_modes first\)"):      # the state was replaced whole
                hb.hi_pass_pod_fetch(q, "mode", 0)
            hb.hi_pass_pod_modes(q, _table(n, 64, n + nodes * ncomp))
            assert same_bits(hb.hi_pass_pod_fetch(q, "gram"), G) and same_bits(hb.hi_pass_pod_fetch(q, "mean"), mean)
            assert same_bits(_modes(hb, q, 64), modes)
            got[weighted] = G
        assert not same_bits(got[False], got[True])
        hb.hi_pass_pod_gram(q, "raw", np.ones(nodes))                                 # uniform weights: the bits of NULL
        assert same_bits(hb.hi_pass_pod_fetch(q, "gram"), got[False])
        assert same_bits(hb.hi_pass_export(q, 0, n), x)                               # the raw frames are untouched
    finally:
        hb.hi_pass_end(q)


@pytest.mark.parametrize("q,nodes", (("v", 43), ("p", 1)), ids=["v43", "p1"])
def test_a_strided_view_equals_a_session_of_those_frames(hb, q, nodes):
    """select(3, n, 2): selected frame k is recorded frame 3 + 2 k.  The history is addressed through the stride: G, the mean and
    the modes are those of a session that imported only those frames, bit for bit."""
    n, ncomp = 50, 1 if q == "p" else 3
    x = pod_rows(3 + 2 * n + 1, (nodes, ncomp), seed=77 + nodes)
    w, T = _weights(nodes, True), _table(n, 17, 5)
    twin = _open(hb, q, nodes, x)
    try:
        assert hb.hi_pass_select(q, 3, n, 2) == n == twin.select(3, n, 2)
        view = np.ascontiguousarray(x[3:3 + 2 * n:2])
        G, mean, _ = _check_against_twin_and_reference(hb, q, x, w, frames=view, label="strided ")
        hb.hi_pass_pod_modes(q, T)
        modes = _modes(hb, q, 17)
        assert same_bits(hb.hi_pass_export(q, 0, len(x)), x)
    finally:
        hb.hi_pass_end(q)
    _open(hb, q, nodes, view)
    try:
        hb.hi_pass_pod_gram(q, "raw", w)
        hb.hi_pass_pod_modes(q, T)
        assert same_bits(hb.hi_pass_pod_fetch(q, "gram"), G) and same_bits(hb.hi_pass_pod_fetch(q, "mean"), mean)
        assert same_bits(_modes(hb, q, 17), modes)
    finally:
        hb.hi_pass_end(q)


def test_the_series_is_decomposed_where_it_lies(hb):
    """Import, filter, decompose the filtered series: the twin's G on the device's own filtered frames, within the bound.  The
    same of the fluctuation about a phase average.  The series still stands afterwards, the raw frames are untouched."""
    n, nodes = 50, 43
    x = pod_rows(n, (nodes, 3), seed=12)
    low = hp.design(1e-3, 0.0, 200.0)
    w = _weights(nodes, True)
    _open(hb, "v", nodes, x)
    try:
        for name, make in (("filtered", lambda: hb.hi_pass_filter("v", low["b"], low["a"], low["zi"], low["padlen"])),
                           ("fluctuation", lambda: hb.hi_pass_phase("v", 10))):
            make()
            series = np.stack([hb.hi_pass_fetch("v", "filtered", k) for k in range(n)])
            assert not same_bits(series, x)
            _check_against_twin_and_reference(hb, "v", x, w, source="series", frames=series, label=name + " ")
            assert same_bits(np.stack([hb.hi_pass_fetch("v", "filtered", k) for k in range(n)]), series)      # the series still stands
            assert same_bits(hb.hi_pass_export("v", 0, n), x)
    finally:
        hb.hi_pass_end("v")


# ---- the ladder, with the rows of the twin's (tests/test_hi_pass_pod.py: LADDER) ----------------------------------------------

NO_GRAM = r"fsi_band_pod_fetch: no Gram matrix \(fsi_band_pod_gram first\)"


def _state(hb):
    return hb.hi_pass_pod_fetch("v", "gram"), hb.hi_pass_pod_fetch("v", "mean"), hb.hi_pass_pod_fetch("v", "mode", 0)


@pytest.mark.parametrize("source", hp.POD_SERIES)
@pytest.mark.parametrize("call", list(LADDER))
def test_the_ladder_drops_the_decomposition_with_its_source(hb, cylinder_case, call, source):
    from vasp_amd.capi import FsiError
    mesh = cylinder_case[0]["mesh"]
    nodes = mesh.num_nodes
    x = pod_rows(12, (nodes, 3), seed=20)
    hb.hi_pass_begin("v", np.arange(nodes, dtype=np.int32), None, 13)
    try:
        hb.hi_pass_import("v", x)
        hb.hi_pass_select("v", 2, 8, 1)
        hb.hi_pass_filter("v", B, A, ZI, 0)
        hb.hi_pass_pod_gram("v", source)
        hb.hi_pass_pod_modes("v", np.full((8, 2), 0.5))
        before = _state(hb)
        calls = {"sample": lambda: hb.hi_pass_sample("v"),
                 "import": lambda: hb.hi_pass_import("v", x[:1]),
                 "select": lambda: hb.hi_pass_select("v", 1, 5, 2),
                 "filter": lambda: hb.hi_pass_filter("v", B, A, ZI, 0),
                 "filter_next": lambda: hb.hi_pass_filter_next("v", B, A, ZI, 0),
                 "phase": lambda: hb.hi_pass_phase("v", 2),
                 "amplitude": lambda: hb.hi_pass_amplitude("v", 2),
                 "spi": lambda: hb.hi_pass_spi("v", None, 0, 1),
                 "cells": lambda: hb.hi_pass_cells("v", [3, 11]),
                 "pod_modes": lambda: hb.hi_pass_pod_modes("v", np.ones((8, 1))),
                 "pod_gram": lambda: hb.hi_pass_pod_gram("v", "series" if source == "raw" else "raw")}
        assert set(calls) == set(LADDER)
        calls[call]()
        fate = LADDER[call][hp.POD_SERIES.index(source)]
        if fate == "gone":
            with pytest.raises(FsiError, match=NO_GRAM):
                hb.hi_pass_pod_fetch("v", "gram")
            with pytest.raises(FsiError, match=r"fsi_band_pod_modes: no Gram matrix \(fsi_band_pod_gram first\)"):
                hb.hi_pass_pod_modes("v", np.ones((hb._band["v"]["selected"], 1)))      # a table for the selection that stands now
        elif fate == "new":
            assert not same_bits(hb.hi_pass_pod_fetch("v", "gram"), before[0])
            with pytest.raises(FsiError, match=r"no modes \(fsi_band_pod_modes first\)"):
                hb.hi_pass_pod_fetch("v", "mode", 0)
        elif call == "pod_modes":
            after = _state(hb)
            assert same_bits(after[0], before[0]) and same_bits(after[1], before[1]) and not same_bits(after[2], before[2])
        else:
            assert all(same_bits(a, b) for a, b in zip(_state(hb), before))
    finally:
        hb.hi_pass_end("v")


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_stepping(hb, cylinder_case):
    from vasp_amd.capi import FsiError
    x = pod_rows(12, (65, 3), seed=4)
    for call in (lambda: hb.hi_pass_pod_gram("v"), lambda: hb.hi_pass_pod_modes("v", np.ones((0, 1))), lambda: hb.hi_pass_pod_fetch("v", "gram")):
        with pytest.raises(FsiError, match="fsi_band_begin first"):
            call()
    solid = np.nonzero(np.asarray(cylinder_case[1]["cell_kind"]) == 1)[0][:3]
    hb.hi_pass_begin_cells("strain", solid, 8)
    try:
        hb.hi_pass_import("strain", np.zeros((8, 12, 6)))
        with pytest.raises(FsiError, match="a strain / stress session has no proper orthogonal decomposition") as e:
            hb.hi_pass_pod_gram("strain")
        assert e.value.code == 1
    finally:
        hb.hi_pass_end("strain")
    _open(hb, "v", 65, x, capacity=14)
    try:
        with pytest.raises(FsiError, match=NO_GRAM):
            hb.hi_pass_pod_fetch("v", "gram")
        with pytest.raises(FsiError, match=NO_GRAM):
            hb.hi_pass_pod_fetch("v", "mode", 0)
        with pytest.raises(FsiError, match=r"fsi_band_pod_modes: no Gram matrix \(fsi_band_pod_gram first\)"):
            hb.hi_pass_pod_modes("v", np.ones((12, 1)))
        with pytest.raises(FsiError, match=r"no filtered series \(fsi_band_filter or fsi_band_phase first\)"):
            hb.hi_pass_pod_gram("v", "series")
        assert hb.lib.fsi_band_pod_gram(hb.ctx, 1, 2, None) == 1                      # FSI_RATE_PHASE_MEAN
        assert "series must be FSI_RATE_RAW or FSI_RATE_SERIES" in hb.lib.fsi_last_error(hb.ctx).decode()
        for k, value in ((7, -1.0), (0, np.nan), (64, np.inf)):
            w = np.ones(65)
            w[k] = value
            with pytest.raises(FsiError, match=f"the weight of node {k} is .*: a weight is >= 0 and finite"):
                hb.hi_pass_pod_gram("v", "raw", w)
        with pytest.raises(FsiError, match=NO_GRAM):                                  # the refused calls changed nothing
            hb.hi_pass_pod_fetch("v", "mean")
        hb.hi_pass_pod_gram("v", "raw")
        G = hb.hi_pass_pod_fetch("v", "gram")
        with pytest.raises(FsiError, match=r"no modes \(fsi_band_pod_modes first\)"):
            hb.hi_pass_pod_fetch("v", "mode", 0)
        for T in (np.ones((12, 0)), np.ones((12, 65))):
            with pytest.raises(FsiError, match="needs 1 <= nmodes <= 64 modes and their table"):
                hb.hi_pass_pod_modes("v", T)
        assert hb.lib.fsi_band_pod_modes(hb.ctx, 1, 2, None) == 1 and hb.lib.fsi_band_pod_fetch(hb.ctx, 1, 0, 0, None) == 1
        assert "out is NULL" in hb.lib.fsi_last_error(hb.ctx).decode()
        assert hb.lib.fsi_band_pod_fetch(hb.ctx, 1, 3, 0, None) == 1 and "what must be FSI_POD_GRAM" in hb.lib.fsi_last_error(hb.ctx).decode()
        hb.hi_pass_pod_modes("v", np.ones((12, 2)))
        for index in (-1, 2):
            with pytest.raises(FsiError, match=f"mode {index} out of range, 2 modes stand"):
                hb.hi_pass_pod_fetch("v", "mode", index)
        with pytest.raises(FsiError, match="the weight of node 3 is -2"):
            hb.hi_pass_pod_gram("v", "raw", np.where(np.arange(65) == 3, -2.0, 1.0))
        assert same_bits(hb.hi_pass_pod_fetch("v", "gram"), G) and hb.hi_pass_pod_fetch("v", "mode", 1).shape == (65, 3)      # and left the state
        # a NaN in one row makes every entry of G non-finite, and the eigen step refuses it
        bad = x.copy()
        bad[7, 40, 2] = np.nan
        hb.hi_pass_end("v")
        _open(hb, "v", 65, bad)
        hb.hi_pass_pod_gram("v", "raw")
        Gb = hb.hi_pass_pod_fetch("v", "gram")
        assert not np.isfinite(Gb).any()
        with pytest.raises(RuntimeError, match="the Gram matrix is not finite: a recorded value is NaN or inf"):
            hp.pod_eig(Gb, 195, 3)
        hb.hi_pass_select("v", 0, 1, 1)
        with pytest.raises(FsiError, match="1 selected frames, the decomposition needs at least 2"):
            hb.hi_pass_pod_gram("v", "raw")
    finally:
        hb.hi_pass_end("v")
    with pytest.raises(FsiError, match="fsi_band_begin first"):
        hb.hi_pass_pod_fetch("v", "gram")
    # the context still steps
    ns, _, bc_values, pressure, hook = cylinder_case
    run = dict(ns)
    run["t"] = float(ns["dt"])
    with contextlib.redirect_stdout(io.StringIO()):
        hook("pre_solve")(**run)
    hb.set_dirichlet_values(bc_values())
    hb.set_interface_pressure(float(pressure.P) if pressure is not None else 0.0)
    hist = hb.newton_solve(counter=0, first_step_num=0, **{k: ns[k] for k in ("atol", "rtol", "max_it", "lmbda", "recompute", "recompute_tstep")})
    assert len(hist) >= 1 and np.isfinite(hb.get_state("n")).all()


def test_a_partitioned_context_is_refused(cylinder_case):
    """A context told that it is one part of a partition (every cell owned, nothing shared: no call of this test reaches a
    collective) takes no decomposition: the three entry points refuse it before they look for a session."""
    import ctypes as C
    from vasp_amd.capi import HipBackend, _ptr
    red = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32)(lambda user, v, n: 0)
    halo = C.CFUNCTYPE(C.c_int, C.c_void_p)(lambda user: 0)

    class FsiComm(C.Structure):
        _fields_ = [("user", C.c_void_p), ("allreduce_sum", type(red)), ("halo_exchange", type(halo))]

    comm = FsiComm(None, red, halo)
    backend = HipBackend(cylinder_case[1])
    try:
        backend._check(backend.lib.fsi_set_partition(backend.ctx, len(backend.cell_u2i), 0, None, 0, None, 0, None, None, None, C.byref(comm)))
        out = np.zeros(4)
        for name, call in (("fsi_band_pod_gram", lambda: backend.lib.fsi_band_pod_gram(backend.ctx, 1, 0, None)),
                           ("fsi_band_pod_modes", lambda: backend.lib.fsi_band_pod_modes(backend.ctx, 1, 1, _ptr(out))),
                           ("fsi_band_pod_fetch", lambda: backend.lib.fsi_band_pod_fetch(backend.ctx, 1, 0, 0, _ptr(out)))):
            assert call() == 1 and backend.lib.fsi_last_error(backend.ctx).decode() == f"{name}: partitioned contexts are not supported"
    finally:
        backend.close()


# ---- end to end -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,frames", (("0.0115", 12), ("0.0195", 20)), ids=("12-steps", "20-steps"))
def test_end_to_end_run_and_the_finished_folder_write_the_same_files(tmp_path, T, frames):
    """12 steps on the small stenosis mesh, every one saved: twelve frames are too few for the band, which is named and left out,
    and the decomposition of the raw frames is written; 20 steps: the low-pass band has its 19 frames, and its filtered series is
    decomposed as well.  The run in a fresh process; the finished folder through vasp_amd.postprocess writes the same bytes; the
    written modes are float32 of hi_pass_pod_fetch on the saved frames."""
    from test_gpu_hi_pass import _files
    from vasp_amd import postprocess
    from vasp_amd.h5lite import read_h5
    options = ["--hi-pass", "d", "v", "--hi-pass-bands", "0", "200", "--hi-pass-pod", "--hi-pass-pod-modes", "4"]
    results = tmp_path / "case" / "1"
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "vasp_amd.monolithic", "-p", "offset_stenosis", "-dt", "0.001", "-T", T,
           "--verbose", "False", "--folder", str(results.parent), "--sub-folder", "1", "--save-step", "1", "--save-deg", "2",
           "--checkpoint-step", "1000", *options, "--new-arguments", f"mesh_path={STENOSIS}"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"Hi-pass velocity_pod: proper orthogonal decomposition of {frames} frames (volume weights)" in r.stdout
    banded = frames > 18
    if banded:
        assert f"Hi-pass velocity_0_to_200_pod: proper orthogonal decomposition of {frames} frames (volume weights)" in r.stdout
    else:
        assert "Hi-pass velocity_0_to_200: 12 frames recorded, the filter needs more than 18: nothing written" in r.stdout
    lines = []
    ns = postprocess.run(["--folder", str(results), "--output-folder", str(tmp_path / "again"), *options], out=lines.append)
    backend = ns["backend"]
    try:
        assert any(f"Read {frames} of {frames} frames" in line for line in lines)
        run, again = _files(results / "Visualization_hi_pass"), _files(tmp_path / "again" / "Visualization_hi_pass")
        fields = ["displacement", "velocity"]
        stems = [f"{f}_pod" for f in fields] + ([f"{f}_0_to_200_pod" for f in fields] if banded else [])
        series = {f"{f}_0_to_200.{e}" for f in fields for e in ("h5", "xdmf")} if banded else set()
        assert {k.split(":")[0] for k in run} == {f"{s}{t}" for s in stems for t in ("_modes.h5", "_modes.xdmf", ".csv", "_coefficients.csv")} | series
        assert sorted(run) == sorted(again)
        for name in run:
            assert run[name] == again[name], name
        w = hp.pod_volume_weights(ns["mesh"], 2)
        low = hp.design(1e-3, 0.0, 200.0)
        for name, q in (("displacement", "d"), ("velocity", "v")):
            g = read_h5(results / "Visualization" / f"{name}.h5")["VisualisationVector"]
            x = np.stack([np.asarray(g[str(k)].data) for k in range(frames)])
            assert x.dtype == np.float64
            nodes = len(x[0])
            backend.hi_pass_begin(q, *hp.output_nodes(ns["mesh"], 2, q), frames)
            try:
                backend.hi_pass_import(q, x)
                for stem, source in ((f"{name}_pod", "raw"),) + (((f"{name}_0_to_200_pod", "series"),) if banded else ()):
                    if source == "series":
                        backend.hi_pass_filter(q, low["b"], low["a"], low["zi"], low["padlen"])
                    backend.hi_pass_pod_gram(q, source, w)
                    eig = hp.pod_eig(backend.hi_pass_pod_fetch(q, "gram"), x[0].size, 4)
                    table = hp.pod_table(eig)
                    K = table.shape[1]
                    backend.hi_pass_pod_modes(q, table)
                    modes = np.stack([backend.hi_pass_pod_fetch(q, "mode", m) for m in range(K)])
                    header, *rows = (results / "Visualization_hi_pass" / f"{stem}.csv").read_text().splitlines()
                    assert header.startswith(f"# {hp.POD_COLUMNS}; frames = {frames}, weights = volume, trace = {eig['trace']!r}, floor = {eig['floor']!r}")
                    assert len(rows) == 4 and [float(r.split(",")[1]) for r in rows] == list(eig["lam"])
                    assert K >= 1 and [r.split(",")[4].strip() for r in rows] == ["1"] * K + ["0"] * (4 - K)
                    for m in range(K):
                        written = np.frombuffer(run[f"{stem}_modes.h5:/VisualisationVector/{m}"][2], dtype=np.float32)
                        assert written.shape == (3 * nodes,) and np.array_equal(written, modes[m].reshape(-1).astype(np.float32), equal_nan=True)
            finally:
                backend.hi_pass_end(q)
    finally:
        backend.close()
