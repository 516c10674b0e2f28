"""The band-pass in strips of rows on the device: the exact selection kernel (csrc/fsi_band.hip, k_band_select) against
``np.sort``, the magnitude board filled through attached sessions, ``fsi_band_room`` against the begin call, and
``python -m vasp_amd.postprocess`` unsplit and in strips on one finished run.  Every comparison is bitwise; files are compared
byte for byte, with the modification time the object headers carry pinned by SOURCE_DATE_EPOCH.  A child process that ends
with a time limit, an abort or a fault ends its test: nothing more is started."""
import contextlib
import ctypes as C
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from vasp_amd import hi_pass as hp

pytestmark = pytest.mark.gpu

CYL = GOLDEN / "cylinder" / "cylinder.h5"


@pytest.fixture(scope="module")
def cyl(cylinder_case):
    from vasp_amd.capi import HipBackend
    hb = HipBackend(cylinder_case[1])
    yield hb, cylinder_case[0]["mesh"]
    hb.close()


# ---- 1. fsi_order_statistics against np.sort ---------------------------------------------------------------------------

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4099]      # one lane, a wavefront's edge, a workgroup's edge, several rounds of one


def _inputs(n, rng):
    sub = np.array([5e-324, 2.5e-310, 1e-308, 1e300, 3e-320])
    return {
        "magnitudes": np.abs(rng.standard_normal(n)) * 1e-6,
        "all equal": np.full(n, 0.37),
        "two values": rng.choice([1.5, 2.5], n),
        "subnormals with 1e300": rng.choice(sub, n),
        "negative": -np.abs(rng.standard_normal(n)),
        "both signs": rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n),
        "zero": np.zeros(n),
    }


def _ranks(n):
    """0, n - 1, a rank listed twice, and the 22 neighbours of the table's percentiles."""
    return np.concatenate([[0, n - 1, n // 2, n // 2], hp.percentile_ranks(n)]).astype(np.int64)


@pytest.mark.parametrize("n", SIZES)
def test_order_statistics_are_np_sorts(cyl, n):
    hb, _ = cyl
    rng = np.random.default_rng(100 + n)
    ranks = _ranks(n)
    for name, x in _inputs(n, rng).items():
        got, nans = hb.order_statistics(x, ranks)
        again, _ = hb.order_statistics(x, ranks)
        ref = np.sort(x)[ranks]
        assert got.tobytes() == ref.tobytes(), (n, name, got[:4], ref[:4])
        assert again.tobytes() == got.tobytes() and nans == 0, (n, name)
    # the interpolation of the neighbours is numpy's percentile
    x = np.abs(rng.standard_normal(n))
    got, _ = hb.order_statistics(x, hp.percentile_ranks(n))
    assert hp.percentiles_from_ranks(n, got).tobytes() == np.array([np.percentile(x, q) for q in hp.CSV_PERCENTILES]).tobytes()


def test_a_nan_is_counted_and_orders_last(cyl):
    hb, _ = cyl
    x = np.abs(np.random.default_rng(7).standard_normal(300))
    x[123] = np.nan
    got, nans = hb.order_statistics(x, [0, 150, 298, 299])
    ref = np.sort(x)[[0, 150, 298, 299]]
    assert nans == 1 and got[:3].tobytes() == ref[:3].tobytes() and np.isnan(got[3]) and np.isnan(ref[3])
    x[5] = -np.nan
    assert hb.order_statistics(x, [0, 297])[1] == 2 and hb.order_statistics(x, [0, 297])[0].tobytes() == np.sort(x)[[0, 297]].tobytes()


def test_bad_arguments_of_the_selection_are_refused_with_nothing_written(cyl):
    from vasp_amd.capi import _ptr
    hb, _ = cyl
    lib, ctx = hb.lib, hb.ctx
    x, ranks = np.arange(10.0), np.array([0, 9], dtype=np.int64)
    out, nans = np.full(2, -1.0), C.c_int64(-1)

    def refused(rc, text):
        assert rc == 1 and text in lib.fsi_last_error(ctx).decode(), lib.fsi_last_error(ctx).decode()
        assert (out == -1.0).all() and nans.value == -1

    call = lib.fsi_order_statistics
    refused(call(ctx, 0, _ptr(x), 2, _ptr(ranks), _ptr(out), C.byref(nans)), "1 <= n")
    refused(call(ctx, 10, None, 2, _ptr(ranks), _ptr(out), C.byref(nans)), "1 <= n")
    refused(call(ctx, 10, _ptr(x), 2, _ptr(ranks), None, C.byref(nans)), "1 <= n")
    refused(call(ctx, 10, _ptr(x), 2, _ptr(ranks), _ptr(out), None), "1 <= n")
    refused(call(ctx, 10, _ptr(x), 2, None, _ptr(out), C.byref(nans)), "nranks >= 1")
    refused(call(ctx, 10, _ptr(x), 0, _ptr(ranks), _ptr(out), C.byref(nans)), "nranks >= 1")
    for bad in (-1, 10):
        refused(call(ctx, 10, _ptr(x), 2, _ptr(np.array([0, bad], dtype=np.int64)), _ptr(out), C.byref(nans)), f"rank {bad} out of range")
    many = np.arange(33, dtype=np.int64)
    big = np.full(33, -1.0)
    assert call(ctx, 40, _ptr(np.arange(40.0)), 33, _ptr(many), _ptr(big), C.byref(nans)) == 1 and (big == -1.0).all()
    assert "33 distinct ranks" in lib.fsi_last_error(ctx).decode()
    assert call(None, 10, _ptr(x), 2, _ptr(ranks), _ptr(out), C.byref(nans)) == 1
    # no board: the table, the attach
    v = np.full((1, 2), -1.0)
    n1, m1, a1 = np.full(1, -1, dtype=np.int64), np.full(1, -1.0), np.full(1, -1, dtype=np.int64)
    assert lib.fsi_board_table(ctx, 0, 1, 2, _ptr(ranks), _ptr(v), _ptr(n1), _ptr(m1), _ptr(a1)) == 1
    assert "no board" in lib.fsi_last_error(ctx).decode() and (v == -1.0).all() and n1[0] == -1 and m1[0] == -1.0 and a1[0] == -1
    assert lib.fsi_board_begin(ctx, 0, 5) == 1 and lib.fsi_board_begin(ctx, 5, 0) == 1
    assert hb.order_statistics(x, ranks)[0].tolist() == [0.0, 9.0]          # the context goes on


# ---- 2. the board ------------------------------------------------------------------------------------------------------

def test_board_table_is_np_sort_max_and_argmax_over_the_strips(cyl):
    """257 board nodes through three sessions at offsets 0 (d, 100 nodes), 100 (v, 100 nodes) and 200 (p, 57 nodes): imported
    raw frames, the low-pass filter, an RMS window of 3 frames - so frame 0 is zero on every node, a tie over the whole frame
    -, and node 7 of the second strip carries the rows of node 50 of the first, the largest of both: a tie across two strips."""
    from vasp_amd.capi import FsiError
    hb, mesh = cyl
    frames, board_frames, window = 24, 5, 3
    rng = np.random.default_rng(31)
    t = (1 + np.arange(frames))[:, None, None] * 1e-3
    raw = {}
    for q, n, ncomp in (("d", 100, 3), ("v", 100, 3), ("p", 57, 1)):
        f, ph = rng.uniform(40.0, 450.0, (n, ncomp)), rng.uniform(0.0, 6.28, (n, ncomp))
        raw[q] = 1e-3 * np.sin(2 * np.pi * 1.5 * t + ph) + 1e-4 * np.sin(2 * np.pi * f * t + ph)
    raw["d"][:, 50] *= 7.0
    raw["v"][:, 7] = raw["d"][:, 50]
    prm = hp.design(1e-3, 0.0, 100.0)
    offsets = {"d": 0, "v": 100, "p": 200}
    hb.hi_pass_board_begin(257, board_frames)
    try:
        parts = {}
        for q, x in raw.items():
            nodes = np.arange(x.shape[1], dtype=np.int32)
            hb.hi_pass_begin(q, nodes, None, capacity=frames)
            hb.hi_pass_import(q, x)
            hb.hi_pass_filter(q, prm["b"], prm["a"], prm["zi"], prm["padlen"])
            hb.hi_pass_amplitude(q, window)
            with pytest.raises(FsiError, match="do not lie in the board"):
                hb.hi_pass_board_attach(q, 257 - x.shape[1] + 1)
            hb.hi_pass_board_attach(q, offsets[q])
            before = [hb.hi_pass_fetch(q, "amplitude", k, with_max=True) for k in range(board_frames)]
            parts[q] = np.stack([hb.hi_pass_fetch(q, "magnitude", k) for k in range(board_frames)])
            with pytest.raises(FsiError, match="the attached board has 5 frames"):
                hb.hi_pass_fetch(q, "amplitude", board_frames)
            hb.hi_pass_board_attach(q, -1)
            after = [hb.hi_pass_fetch(q, "amplitude", k, with_max=True) for k in range(board_frames)]
            for (a, m, i), (b, n, j) in zip(before, after):                  # what a fetch returns does not change
                assert a.tobytes() == b.tobytes() and (m, i) == (n, j)
        whole = np.concatenate([parts["d"], parts["v"], parts["p"]], axis=1)
        assert whole.shape == (board_frames, 257) and not whole[0].any() and (whole[1:] > 0).all()
        ranks = np.concatenate([[0, 256, 128, 128], hp.percentile_ranks(257)]).astype(np.int64)
        values, nans, mx, am = hb.hi_pass_board_table(0, board_frames, ranks)
        assert values.tobytes() == np.sort(whole, axis=1)[:, ranks].tobytes() and not nans.any()
        assert mx.tobytes() == whole.max(axis=1).tobytes() and am.tolist() == whole.argmax(axis=1).tolist()
        assert am.tolist() == [0, 50, 50, 50, 50] and (whole[1:, 50] == whole[1:, 107]).all()
        again = hb.hi_pass_board_table(0, board_frames, ranks)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (values, nans, mx, am)))
        part = hb.hi_pass_board_table(2, 2, ranks[:3])
        assert part[0].tobytes() == values[2:4, :3].tobytes() and part[3].tolist() == [50, 50]
        # the 13-column table formed on the board is amplitude_row's of the whole frames
        table = hp.board_table(type("Board", (), {"table": staticmethod(hb.hi_pass_board_table)}), board_frames, 257, 1e-3, 0.0)
        ref = np.stack([hp.amplitude_row(k * 1e-3 + 0.0, whole[k], whole[k].max(), int(whole[k].argmax())) for k in range(board_frames)])
        assert table.tobytes() == ref.tobytes()
        with pytest.raises(FsiError, match="first \\+ count <= the board's 5 frames"):
            hb.hi_pass_board_table(4, 2, ranks)
    finally:
        for q in raw:
            with contextlib.suppress(Exception):
                hb.hi_pass_end(q)
        hb.hi_pass_board_end()
    with pytest.raises(FsiError, match="no board"):
        hb.hi_pass_board_table(0, 1, [0])


def test_a_board_that_does_not_fit_is_refused_before_anything_is_allocated(cyl):
    """2^31 nodes x 2^20 frames: the room rule's text, from the host; the board that stood is still open."""
    from vasp_amd.capi import FsiError
    hb, _ = cyl
    hb.hi_pass_board_begin(4, 2)
    try:
        with pytest.raises(FsiError) as e:
            hb.hi_pass_board_begin(1 << 31, 1 << 20)
        assert re.search(r"fsi_board_begin: the board needs \d+ bytes \(2147483648 nodes x 1048576 frames\), the device has \d+ bytes free of "
                         r"which \d+ stay with the context$", str(e.value))
        values, nans, mx, am = hb.hi_pass_board_table(0, 2, [0, 3])
        assert not values.any() and not nans.any() and not mx.any() and am.tolist() == [0, 0]
    finally:
        hb.hi_pass_board_end()


# ---- 3. fsi_band_room and the begin call -------------------------------------------------------------------------------

def test_band_room_agrees_with_the_begin_call(cyl):
    from vasp_amd.capi import FsiError
    hb, mesh = cyl
    nodes = hp.output_nodes(mesh, 2, "v")
    rows = 3 * len(nodes[0])
    need1, available = hb.hi_pass_room(rows, 1)
    assert need1 == hp.host_room(rows, 1)[0] == 8 * rows * 72              # the host twin states the same bytes
    fits = (available // (8 * rows) - 70) // 2                              # the largest capacity with need <= available
    need, avail = hb.hi_pass_room(rows, fits)
    over, _ = hb.hi_pass_room(rows, fits + 1)
    print(f"room: {rows} rows, available {avail} bytes, capacity {fits} needs {need}, capacity {fits + 1} needs {over}")
    assert need <= avail < over and need == hp.host_room(rows, fits)[0]
    with pytest.raises(FsiError) as e:
        hb.hi_pass_begin("v", *nodes, capacity=fits + 1)
    said = re.search(r"needs (\d+) bytes .* has (\d+) bytes free of which (\d+) stay", str(e.value))
    assert int(said.group(1)) == over and abs(int(said.group(2)) - int(said.group(3)) - avail) <= 1
    hb.hi_pass_begin("v", *nodes, capacity=fits)
    hb.hi_pass_end("v")
    cells = 5
    assert hb.hi_pass_room(24 * cells, 9)[0] == 8 * 24 * cells * (18 + 70)


# ---- 4. the whole tool -------------------------------------------------------------------------------------------------

RUN = ["-dt", "0.001", "-T", "0.0395", "--theta", "0.51", "--verbose", "False", "--save-step", "1", "--save-deg", "2", "--checkpoint-step", "50"]
# the bands of the issue, 0 - 100 Hz (a low-pass) and 25 - 400 Hz; a cascade takes no band from 0 Hz (hi_pass.stage_refusal),
# so --hi-pass-multiband runs on bands of its own
ALL = ["--hi-pass", "d", "v", "p", "--hi-pass-tensor", "strain", "stress", "--hi-pass-bands", "0", "100", "25", "400", "--hi-pass-amplitude",
       "--hi-pass-window", "8", "--hi-pass-tensor-window", "8", "--hi-pass-point-ids", "0", "5"]
CASCADE = ["--hi-pass", "v", "--hi-pass-bands", "25", "400", "50", "300", "--hi-pass-multiband", "--hi-pass-amplitude", "--hi-pass-window", "8",
           "--hi-pass-point-ids", "0", "5"]
TREES = ("Visualization_hi_pass", "Visualization_separate_domain")


def _child(module, argv, cwd, limit):
    """One child under its own time limit; anything but exit status 0 fails the caller, which then starts nothing more."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""), SOURCE_DATE_EPOCH="1700000000")
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", module, *argv], cwd=cwd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        pytest.fail(f"python -m {module} ended with status {r.returncode}:\n" + r.stdout[-3000:] + r.stderr[-3000:], pytrace=False)
    return r.stdout


@pytest.fixture(scope="module")
def finished(tmp_path_factory):
    """The results folder of a 40-step cylinder run at save_deg 2: 40 frames, enough for a band-pass (padlen + 1 = 34)."""
    tmp = tmp_path_factory.mktemp("strips")
    results = tmp / "case" / "1"
    log = _child("vasp_amd.monolithic", ["-p", "cylinder", *RUN, "--folder", str(results.parent), "--sub-folder", "1",
                                         "--new-arguments", f"mesh_path={CYL}"], tmp, 300)
    assert "Solved for timestep 40," in log
    return results


def _limit(results, options, strips_wanted=3):
    """--history-memory such that the largest quantity of ``options`` needs exactly ``strips_wanted`` strips: its board and a
    session of a third of its rows, in fsi_band_room's bytes (the host twin's, which test 3 compares with the device's)."""
    from vasp_amd import hi_pass_strips as strips
    from vasp_amd import postprocess
    with contextlib.redirect_stdout(io.StringIO()):
        ns, mesh, source, indices, _ = postprocess.prepare(["--folder", str(results), *options])
    source.close()
    need = lambda rows, capacity: hp.host_room(rows, capacity)[0]
    jobs = strips.jobs(mesh, ns)
    big = max(jobs, key=lambda j: j.units * j.rows_per_unit)
    limit = big.board_bytes(True) + need(-(-big.units // strips_wanted) * big.rows_per_unit, len(indices) + 1)
    assert len(strips.plan_strips(big.units, big.rows_per_unit, len(indices) + 1, big.board_bytes(True), limit, need)) == strips_wanted
    return limit, big


def _same_bytes(a, b):
    names = {}
    for tree in TREES:
        names[tree] = sorted(p.name for p in (a / tree).iterdir())
        assert names[tree] == sorted(p.name for p in (b / tree).iterdir()) and names[tree], tree
        for name in names[tree]:
            assert (a / tree / name).read_bytes() == (b / tree / name).read_bytes(), name
    return names


def test_strips_write_the_unsplit_files_byte_for_byte(finished, tmp_path):
    limit, big = _limit(finished, ALL)
    assert big.kind == "tensor"
    base = ["--folder", str(finished), *ALL]
    log = _child("vasp_amd.postprocess", [*base, "--output-folder", str(tmp_path / "whole")], tmp_path, 120)
    assert "Read 40 of 40 frames" in log and "in strips:" not in log
    log = _child("vasp_amd.postprocess", [*base, "--output-folder", str(tmp_path / "split"), "--history-memory", str(limit)], tmp_path, 180)
    said = re.findall(r"Hi-pass (\w+) in strips: (\d+) strips of at most (\d+) (\w+) \((\d+) in all\), the 40 frames read (\d+) times", log)
    assert [s[0] for s in said] == ["displacement", "velocity", "pressure", "GreenLagrangeStrain", "TrueStress"], log[-2000:]
    by = {s[0]: s for s in said}
    assert by["TrueStress"][1] == "3" and by["GreenLagrangeStrain"][1] == "3" and by["TrueStress"][3] == "cells" and int(by["TrueStress"][4]) == big.units
    assert all(int(s[5]) == 2 * int(s[1]) for s in said)                    # two series, one board: every strip read once per series
    names = _same_bytes(tmp_path / "whole", tmp_path / "split")
    hi = names["Visualization_hi_pass"]
    assert len([n for n in hi if n.endswith(".h5")]) == 2 * (3 * 2 + 2 * 3) and len([n for n in hi if n.endswith(".csv")]) == 2 * 5
    assert len(names["Visualization_separate_domain"]) == 6
    log = _child("vasp_amd.postprocess", [*base, "--output-folder", str(tmp_path / "again"), "--history-memory", str(limit)], tmp_path, 180)
    _same_bytes(tmp_path / "split", tmp_path / "again")


def test_a_multiband_cascade_in_strips(finished, tmp_path):
    limit, big = _limit(finished, CASCADE)
    base = ["--folder", str(finished), *CASCADE]
    _child("vasp_amd.postprocess", [*base, "--output-folder", str(tmp_path / "whole")], tmp_path, 120)
    log = _child("vasp_amd.postprocess", [*base, "--output-folder", str(tmp_path / "split"), "--history-memory", str(limit)], tmp_path, 180)
    assert f"Hi-pass velocity in strips: 3 strips of at most {-(-big.units // 3)} nodes ({big.units} in all), the 40 frames read 9 times" in log
    names = _same_bytes(tmp_path / "whole", tmp_path / "split")
    assert "velocity_stop_25_to_400_stop_50_to_300.h5" in names["Visualization_hi_pass"]
    assert "velocity_stop_25_to_400_stop_50_to_300.csv" in names["Visualization_hi_pass"]
