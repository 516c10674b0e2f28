"""Host side of the band-pass in strips of rows (``vasp_amd.hi_pass_strips``): numpy's percentile from two order statistics,
frames of a growing HDF5 series reserved and filled later, the planner, and ``python -m vasp_amd.postprocess`` unsplit and in
strips with a backend that has no device sessions.  Every comparison is bitwise; files are compared byte for byte, with the
modification time the object headers carry pinned by SOURCE_DATE_EPOCH."""
import contextlib
import io

import numpy as np
import pytest

from conftest import GOLDEN
from vasp_amd import hi_pass as hp
from vasp_amd import hi_pass_strips as strips
from vasp_amd.h5lite import open_h5

CYL = GOLDEN / "cylinder" / "cylinder.h5"
OPTIONS = ["--hi-pass", "d", "v", "p", "--hi-pass-bands", "0", "100", "--hi-pass-amplitude", "--hi-pass-window", "8",
           "--hi-pass-point-ids", "0", "5"]
TREES = ("Visualization_hi_pass", "Visualization_separate_domain")


# ---- 1. the percentile twin --------------------------------------------------------------------------------------------

def _inputs(n, scale, rng):
    x = rng.random(n) * scale
    tied = x.copy()
    tied[: n // 3] = tied[0]
    return {"random": x, "a third tied": tied, "all equal": np.full(n, x[0])}


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 255, 256, 257, 1000, 4099, 100003])
def test_percentiles_from_ranks_gives_numpys_bits(n):
    rng = np.random.default_rng(n)
    ranks = hp.percentile_ranks(n)
    assert ranks.shape == (22,) and ranks.min() == 0 and ranks.max() == n - 1
    for scale in (1e-9, 1.0, 1e6):
        for name, x in _inputs(n, scale, rng).items():
            ref = np.array([np.percentile(x, q) for q in hp.CSV_PERCENTILES])
            got = hp.percentiles_from_ranks(n, np.sort(x)[ranks])
            assert got.tobytes() == ref.tobytes(), (n, scale, name)
    # frames stacked in front, as the table takes them
    x = rng.random((3, n))
    got = hp.percentiles_from_ranks(n, np.sort(x, axis=1)[:, ranks])
    assert got.tobytes() == np.array([[np.percentile(row, q) for q in hp.CSV_PERCENTILES] for row in x]).tobytes()


def test_a_nan_gives_numpys_row():
    x = np.random.default_rng(0).random(50)
    x[7] = np.nan
    with np.errstate(invalid="ignore"):
        ref = np.array([np.percentile(x, q) for q in hp.CSV_PERCENTILES])
    got = hp.percentiles_from_ranks(50, np.sort(x)[hp.percentile_ranks(50)])
    assert np.isnan(ref).all() and np.isnan(got).all()
    # the host board's table, whole: the rows of amplitude_row, with numpy's NaN row
    board = hp.HostBoard(50, 2)
    board.store(0, 0, x)
    clean = np.where(np.isnan(x), 0.25, x)
    board.store(1, 0, clean[:20])
    board.store(1, 20, clean[20:])
    table = hp.board_table(board, 2, 50, 0.5, 1.0)
    ref1 = hp.amplitude_row(1.5, clean, clean.max(), int(np.argmax(clean)))
    assert table[1].tobytes() == ref1.tobytes() and np.isnan(table[0, 1:3]).all() and np.isnan(table[0, 4:12]).all() and table[0, 0] == 1.0


# ---- 2. H5Series.reserve -----------------------------------------------------------------------------------------------

BLOCKS = ((23, 37), (5, 23), (0, 5))           # three uneven blocks of 37 rows, filled last block first


def test_a_reserved_dataset_series_is_the_appended_file(tmp_path, monkeypatch):
    monkeypatch.setenv("SOURCE_DATE_EPOCH", "1700000000")
    rng = np.random.default_rng(4)
    frames = rng.standard_normal((6, 37, 3)).astype(np.float32)
    static = lambda: hp.HiPassWriter(tmp_path, np.zeros((37, 3)), np.zeros((2, 4), dtype=np.int32))
    a = static().open("appended")
    for k, f in enumerate(frames):
        a.append(str(k), f)
    a.close()
    r = static().open("reserved")
    addr = [r.reserve(str(k), (37, 3), np.float32) for k in range(6)]
    for lo, hi in BLOCKS:
        for k in (3, 0, 5, 1, 4, 2):
            r.fill(addr[k], 4 * 3 * lo, frames[k, lo:hi])
    r.close()
    assert (tmp_path / "reserved.h5").read_bytes() == (tmp_path / "appended.h5").read_bytes()
    with open_h5(tmp_path / "reserved.h5") as lazy:
        assert all(np.array_equal(lazy["VisualisationVector"][str(k)].data, frames[k]) for k in range(6))
    with pytest.raises(Exception, match="exists"):
        s = static().open("twice")
        s.reserve("0", (3,), np.float64)
        s.reserve("0", (3,), np.float64)


def test_a_reserved_tensor_group_series_is_the_appended_file(tmp_path, monkeypatch):
    from vasp_amd.hi_pass_tensor import TensorWriter
    monkeypatch.setenv("SOURCE_DATE_EPOCH", "1700000000")
    rng = np.random.default_rng(5)
    cells = 37
    geometry, topology = rng.random((4 * cells, 3)), np.arange(4 * cells).reshape(cells, 4)
    for ncomp, name in ((9, "tensor"), (1, "scalar")):
        frames = rng.standard_normal((4, cells, 4 * ncomp))
        (tmp_path / "a").mkdir(exist_ok=True)
        (tmp_path / "r").mkdir(exist_ok=True)
        a = TensorWriter(tmp_path / "a", geometry, topology).open(name, ncomp)
        for f in frames:
            a.append(f)
        a.close(0.5, 0.0)
        r = TensorWriter(tmp_path / "r", geometry, topology).open(name, ncomp)
        addr = [r.reserve() for _ in frames]
        for lo, hi in BLOCKS:
            for k in (2, 0, 3, 1):
                r.fill(addr[k], lo, frames[k, lo:hi])
        r.close(0.5, 0.0)
        for ext in (".h5", ".xdmf"):
            assert (tmp_path / "r" / (name + ext)).read_bytes() == (tmp_path / "a" / (name + ext)).read_bytes(), (name, ext)
        with open_h5(tmp_path / "r" / f"{name}.h5") as lazy:
            for k in range(4):
                assert np.array_equal(lazy[name][f"{name}_{k}"]["vector"].data.reshape(-1), frames[k].reshape(-1).astype(np.float32))
            assert "cell_dofs" in lazy[name][f"{name}_0"] and "cell_dofs" not in lazy[name][f"{name}_1"]


# ---- 3. the planner ----------------------------------------------------------------------------------------------------

NEED = lambda rows, capacity: hp.host_room(rows, capacity)[0]


@pytest.mark.parametrize("units,per,capacity,board", [(2500, 3, 25, 480000), (2500, 1, 25, 0), (317, 24, 41, 8 * 317 * 4 * 40), (7, 3, 100, 0),
                                                      (1000003, 3, 1501, 0)])
def test_the_planner_returns_the_fewest_strips_that_fit(units, per, capacity, board):
    one = NEED(per, capacity)
    for want in (1, 2, 3, 5, units):
        size = -(-units // want)
        limit = board + NEED(size * per, capacity)          # a strip of `size` units just fits
        plan = strips.plan_strips(units, per, capacity, board, limit, NEED)
        assert plan[0][0] == 0 and plan[-1][1] == units and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))       # whole units, none cut
        sizes = [i1 - i0 for i0, i1 in plan]
        assert min(sizes) >= 1 and len(set(sizes[:-1])) <= 1 and sizes[-1] <= sizes[0]
        assert NEED(sizes[0] * per, capacity) <= limit - board
        k = len(plan)
        assert k == -(-units // size)
        if k > 1:                               # one strip fewer does not fit
            assert NEED(-(-units // (k - 1)) * per, capacity) > limit - board
    with pytest.raises(SystemExit, match=rf"rows of one node need {one} bytes .*may take {board + one - 1}"):
        strips.plan_strips(units, per, capacity, board, board + one - 1, NEED)
    if board:
        with pytest.raises(SystemExit, match=rf"board .* alone needs {board} bytes.* may take {board - 1} .*dropping --hi-pass-amplitude needs none"):
            strips.plan_strips(units, per, capacity, board, board - 1, NEED)


def test_three_strips_with_a_shorter_last_one():
    assert strips.plan_strips(2500, 3, 25, 480000, 480000 + NEED(3 * 834, 25), NEED) == [(0, 834), (834, 1668), (1668, 2500)]


# ---- 4. the whole tool on the host backend -----------------------------------------------------------------------------

def _post(argv, factory):
    from vasp_amd import postprocess
    lines = []
    with contextlib.redirect_stdout(io.StringIO()):
        ns = postprocess.run(argv, backend_factory=factory, out=lines.append)
    return ns, lines


@pytest.fixture(scope="module")
def finished(tmp_path_factory):
    """24 saved frames of the cylinder, written by a run with a backend without device sessions: (results, the stub)."""
    from test_session_restart import _Stub
    from vasp_amd import monolithic
    folder = tmp_path_factory.mktemp("strips") / "case"
    with contextlib.redirect_stdout(io.StringIO()):
        monolithic.run(["-p", "cylinder", "-dt", "0.001", "-T", "0.0235", "--theta", "0.51", "--folder", str(folder), "--sub-folder", "1",
                        "--save-step", "1", "--save-deg", "2", "--checkpoint-step", "5", "--verbose", "False",
                        "--new-arguments", f"mesh_path={CYL}"], backend_factory=_Stub, out=lambda *a: None)
    return folder / "1", _Stub


def _same_bytes(a, b):
    for tree in TREES:
        names = sorted(p.name for p in (a / tree).iterdir())
        assert names == sorted(p.name for p in (b / tree).iterdir()) and names, tree
        for name in names:
            assert (a / tree / name).read_bytes() == (b / tree / name).read_bytes(), name
    return names


def test_strips_write_the_unsplit_files_byte_for_byte(finished, tmp_path, monkeypatch):
    monkeypatch.setenv("SOURCE_DATE_EPOCH", "1700000000")
    results, stub = finished
    base = ["--folder", str(results), *OPTIONS]
    ns, lines = _post([*base, "--output-folder", str(tmp_path / "whole")], stub)
    assert not ns["strips"] and not any("in strips:" in line for line in lines)
    # d and v: 2500 nodes x 3 rows over 25 frames in three strips of 834, 834, 832 nodes beside a board of 2500 x 24
    limit = 8 * 2500 * 24 + NEED(3 * 834, 25)
    assert NEED(3 * 1250, 25) > NEED(3 * 834, 25)
    ns, lines = _post([*base, "--output-folder", str(tmp_path / "split"), "--history-memory", str(limit)], stub)
    assert ns["strips"]
    said = [line for line in lines if "in strips" in line]
    assert len(said) == 3 and "displacement in strips: 3 strips of at most 834 nodes (2500 in all), the 24 frames read 3 times" in said[0]
    assert "velocity in strips: 3 strips" in said[1] and "pressure in strips: 1 strips of at most 2500 nodes" in said[2]
    assert all("s reading" in line and "s filtering" in line and "s on tables" in line for line in said)
    _same_bytes(tmp_path / "whole", tmp_path / "split")
    names = sorted(p.name for p in (tmp_path / "split" / "Visualization_hi_pass").iterdir())
    assert len([n for n in names if n.endswith(".h5")]) == 6 and len([n for n in names if n.endswith(".csv")]) == 3
    assert sorted(p.name for p in (tmp_path / "split" / "Visualization_separate_domain").iterdir()) == sorted(
        f"{f}_point_id_{i}.csv" for f in ("displacement", "velocity", "pressure") for i in (0, 5))
    table = np.loadtxt(tmp_path / "split" / "Visualization_hi_pass" / "velocity_0_to_100.csv", delimiter=",")
    assert table.shape == (24, 13) and np.isfinite(table).all() and (table[:, 3] > 0).any()


def test_history_memory_leaves_no_trace_when_everything_fits(finished, tmp_path, monkeypatch):
    monkeypatch.setenv("SOURCE_DATE_EPOCH", "1700000000")
    results, stub = finished
    base = ["--folder", str(results), *OPTIONS]
    _, plain = _post([*base, "--output-folder", str(tmp_path / "plain")], stub)
    fits = 3 * 8 * 2500 * 24 + NEED(3 * 2500, 25) * 2 + NEED(2500, 25)          # the three histories and their boards, to the byte
    ns, lines = _post([*base, "--output-folder", str(tmp_path / "given"), "--history-memory", str(fits)], stub)
    assert not ns["strips"]
    path = lambda line: line.replace(str(tmp_path / "given"), "").replace(str(tmp_path / "plain"), "")
    assert [path(x) for x in lines if not x.startswith("Read ")] == [path(x) for x in plain if not x.startswith("Read ")]
    _same_bytes(tmp_path / "plain", tmp_path / "given")
    ns, _ = _post([*base, "--output-folder", str(tmp_path / "less"), "--history-memory", str(fits - 1)], stub)
    assert ns["strips"]
    from vasp_amd import postprocess
    with pytest.raises(SystemExit, match="--history-memory must be a number of bytes >= 1"):
        postprocess.run([*base, "--history-memory", "0"], backend_factory=stub, out=lambda *a: None)


def _never(desc):
    raise AssertionError("a backend was built")


def test_refusals_of_the_strip_passes_come_before_any_backend(finished, tmp_path):
    results, _ = finished
    base = ["--folder", str(results), "--output-folder", str(tmp_path / "no"), *OPTIONS]
    from vasp_amd import postprocess
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(SystemExit, match=r"board of amplitude magnitudes alone needs 480000 bytes.*dropping --hi-pass-amplitude needs none"):
            postprocess.run([*base, "--history-memory", "479999"], backend_factory=_never, out=lambda *a: None)
        with pytest.raises(SystemExit, match=rf"the 3 rows of one node need {NEED(3, 25)} bytes over 25 frames beside the board's 480000"):
            postprocess.run([*base, "--history-memory", str(480000 + NEED(3, 25) - 1)], backend_factory=_never, out=lambda *a: None)
    assert not (tmp_path / "no").exists()
