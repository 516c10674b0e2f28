"""Host side of the spectrogram in strips of rows (``vasp_amd.spectrogram_strips``): the planner, the carried sums of the host
session against its unsplit calls, and ``python -m vasp_amd.postprocess --spectrogram`` unsplit and in strips with a backend
that has no device sessions.  Every comparison is bitwise; files are compared byte for byte."""
import contextlib
import io

import numpy as np
import pytest

from conftest import GOLDEN
from vasp_amd import spectrogram as sg
from vasp_amd import spectrogram_strips as strips

CYL = GOLDEN / "cylinder" / "cylinder.h5"
BOX = ["--spectrogram-region", "box", "--spectrogram-fsi-region", "-100", "100", "-100", "100", "-100", "100"]
OPTIONS = ["--spectrogram", "d", "v", "p", "--spectrogram-sampling", "All", *BOX]
NEED = lambda rows, capacity: sg.host_room(rows, capacity)[0]


# ---- 1. the planner ----------------------------------------------------------------------------------------------------

def test_the_host_room_is_the_begin_calls_formula():
    """csrc/fsi_sessions.hip, spec_room, term for term: histories, row lists, 64 bins of tables, the means of capacity / 4."""
    for rows, capacity, mag in ((1, 1, False), (423, 49, False), (300, 41, True), (4500000, 5001, False)):
        nsamp = 3 * rows if mag else rows
        ref = 8.0 * rows * (2.0 * capacity + 2.0 * 33) + 16.0 * nsamp + 16.0 * 64 * capacity + 8.0 * rows * (capacity / 4.0 + 2.0)
        assert sg.host_room(rows, capacity, mag)[0] == int(ref) and ref == int(ref)
    assert NEED(4500000, 5001) > 400e9                      # the whole 1.5 M-node mesh, three components, 5000 frames


@pytest.mark.parametrize("rows,granule,capacity", [(423, 128, 49), (7500, 128, 25), (128, 128, 25), (129, 128, 25), (100, 128, 25), (1, 4096, 3),
                                                   (4500000, 128, 5001), (10000, 4096, 25)])
def test_the_planner_returns_the_fewest_equal_strips_on_the_granule(rows, granule, capacity):
    up = lambda k: min(rows, -(-(-(-rows // k)) // granule) * granule)
    for want in (1, 2, 3, 5, rows):
        size = up(want)
        limit = NEED(size, capacity)                        # a strip of `size` rows just fits
        plan = strips.plan_row_strips(rows, granule, capacity, limit, NEED)
        assert plan[0][0] == 0 and plan[-1][1] == rows and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))
        sizes = [r1 - r0 for r0, r1 in plan]
        assert min(sizes) >= 1 and len(set(sizes[:-1])) <= 1 and sizes[-1] <= sizes[0] == size
        assert all(r0 % granule == 0 for r0, _ in plan) and (len(plan) == 1 or sizes[0] % granule == 0)
        assert NEED(sizes[0], capacity) <= limit
        k = len(plan)
        assert k == -(-rows // size)
        if k > 1:                                           # one strip fewer does not fit
            assert NEED(up(k - 1), capacity) > limit
    one = NEED(min(granule, rows), capacity)
    with pytest.raises(SystemExit, match=rf"{min(granule, rows)} rows, the fewest .* need {one} bytes over {capacity} frames, the histories may take {one - 1}$"):
        strips.plan_row_strips(rows, granule, capacity, one - 1, NEED)


def test_three_strips_with_a_shorter_last_one_and_the_two_refusals():
    assert strips.plan_row_strips(423, 128, 49, NEED(256, 49), NEED) == [(0, 256), (256, 423)]
    assert strips.plan_row_strips(423, 128, 49, NEED(256, 49) - 1, NEED) == [(0, 128), (128, 256), (256, 384), (384, 423)]
    assert strips.plan_row_strips(700, 128, 49, NEED(256, 49), NEED) == [(0, 256), (256, 512), (512, 700)]
    with pytest.raises(SystemExit, match=rf"128 rows.* need {NEED(128, 49)} bytes over 49 frames, the histories may take {NEED(128, 49) - 1}"):
        strips.plan_row_strips(423, 128, 49, NEED(128, 49) - 1, NEED)              # not one granule of a longer list
    with pytest.raises(SystemExit, match=rf"100 rows.* need {NEED(100, 49)} bytes over 49 frames, the histories may take 5"):
        strips.plan_row_strips(100, 128, 49, 5, NEED)                               # not even the whole of a shorter one


# ---- 2. the host session's carried sums --------------------------------------------------------------------------------

ROWS, FRAMES, CHUNK = 423, 40, 128
CUTS = ((0, 128), (128, 384), (384, 423))
FS = 1000.0


def _history(rng):
    t = np.arange(FRAMES)[:, None] / FS
    f = rng.uniform(30.0, 400.0, ROWS)[None, :]
    return 1e4 * rng.standard_normal(ROWS)[None, :] + np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28, ROWS)[None, :]) + 0.1 * rng.standard_normal((FRAMES, ROWS))


def _session(x, chunk=CHUNK):
    s = sg.HostSpecSession(x.shape[1], FRAMES + 1, chunk)
    for frame in x:
        s.sample(frame)
    return s


@pytest.fixture(scope="module")
def history():
    return _history(np.random.default_rng(11))


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("scaling", ["spectrum", "density"])
def test_carried_sums_give_the_unsplit_bytes(history, scaling, filtered):
    hp = sg.highpass_design(FS, 25.0)
    K, nov, nfft = 16, 12, 32
    w, wp = sg.window_values("blackmanharris", K), sg.window_values("blackmanharris", FRAMES)
    whole = _session(history)
    assert whole.granule == CHUNK and sg.HostSpecSession(3, 2).granule == sg.HOST_CHUNK == 32 * sg.ROWS
    if filtered:
        whole.filter(hp["b"], hp["a"], hp["zi"], hp["padlen"])
    ref_s, ref_p = whole.spectrogram(K, nov, nfft, w, scaling, FS), whole.periodogram(wp, scaling, FS)
    assert ref_s.shape == (17, 7) and ref_p.shape == (21,) and (ref_s > 0).all()
    cs = cp = None
    for r0, r1 in CUTS:
        s = _session(history[:, r0:r1])
        if filtered:
            s.filter(hp["b"], hp["a"], hp["zi"], hp["padlen"])
        total = ROWS if r1 == ROWS else 0
        cs = s.spectrogram_sum(K, nov, nfft, w, scaling, FS, r0, total, cs)
        cp = s.periodogram_sum(wp, scaling, FS, r0, total, cp)
        if not total:                           # on the way the carry is a sum, not a mean
            assert not np.array_equal(cs, ref_s)
    assert cs.tobytes() == ref_s.tobytes() and cp.tobytes() == ref_p.tobytes()
    # one strip that holds every row is the mean itself
    assert whole.spectrogram_sum(K, nov, nfft, w, scaling, FS, 0, ROWS).tobytes() == ref_s.tobytes()
    assert whole.periodogram_sum(wp, scaling, FS, 0, ROWS).tobytes() == ref_p.tobytes()


def test_a_strip_plan_off_the_granule_is_refused(history):
    K, nov, nfft = 16, 12, 32
    w, wp = sg.window_values("hann", K), sg.window_values("blackmanharris", FRAMES)
    carry_s, carry_p = np.full((17, 7), 3.0), np.full(21, 3.0)
    calls = lambda s, r0, total: (lambda: s.spectrogram_sum(K, nov, nfft, w, "spectrum", FS, r0, total, carry_s),
                                  lambda: s.periodogram_sum(wp, "spectrum", FS, r0, total, carry_p))
    ragged, full = _session(history[:, 128:228]), _session(history[:, 128:256])
    for call in calls(full, 100, 0) + calls(full, -128, 0):
        with pytest.raises(RuntimeError, match="a strip starts at a multiple of 128 rows"):
            call()
    for call in calls(ragged, 128, 0):
        with pytest.raises(RuntimeError, match="100 rows and is not the last strip"):
            call()
    for call in calls(ragged, 128, 229) + calls(full, 128, 128):
        with pytest.raises(RuntimeError, match="the last strip ends at first_row \\+ rows"):
            call()
    with pytest.raises(RuntimeError, match="needs the carry of the rows before first_row"):
        full.spectrogram_sum(K, nov, nfft, w, "spectrum", FS, 128, 0, None)
    with pytest.raises(RuntimeError, match="needs the carry of the rows before first_row"):
        full.periodogram_sum(wp, "spectrum", FS, 128, 0, np.zeros(20))
    assert (carry_s == 3.0).all() and (carry_p == 3.0).all()                        # a refused call leaves the carry as it was
    full.spectrogram_sum(K, nov, nfft, w, "spectrum", FS, 128, 0, carry_s)          # and the session still transforms
    assert (carry_s > 3.0).all()


def test_the_single_row_rule_follows_the_total_row_count():
    """get_psd drops its scaling for one row: a strip of one row of many keeps 'spectrum'."""
    o = sg.options({"fsi_region": [0, 0, 0, 1]})
    assert sg.transform_plan(1, 40, 0.04, o)["psd_scaling"] == "density" and sg.transform_plan(129, 40, 0.04, o)["psd_scaling"] == "spectrum"


# ---- 3. the whole tool on the host backend -----------------------------------------------------------------------------

def _post(argv, factory):
    from vasp_amd import postprocess
    lines = []
    with contextlib.redirect_stdout(io.StringIO()):
        ns = postprocess.run(argv, backend_factory=factory, out=lines.append)
    return ns, lines


@pytest.fixture(scope="module")
def finished(tmp_path_factory):
    """24 saved frames of the cylinder, written by a run with a backend without device sessions: (results, the stub, whose
    host sessions add their rows in chunks of 128)."""
    from test_session_restart import _Stub
    from vasp_amd import monolithic
    folder = tmp_path_factory.mktemp("specstrips") / "case"
    with contextlib.redirect_stdout(io.StringIO()):
        monolithic.run(["-p", "cylinder", "-dt", "0.001", "-T", "0.0235", "--theta", "0.51", "--folder", str(folder), "--sub-folder", "1",
                        "--save-step", "1", "--save-deg", "2", "--checkpoint-step", "5", "--verbose", "False",
                        "--new-arguments", f"mesh_path={CYL}"], backend_factory=_Stub, out=lambda *a: None)
    return folder / "1", type("_Stub128", (_Stub,), dict(spec_host_chunk=CHUNK))


def _same_bytes(a, b):
    names = sorted(p.name for p in (a / "Spectrograms").iterdir())
    assert names == sorted(p.name for p in (b / "Spectrograms").iterdir()) and names
    for name in names:
        assert (a / "Spectrograms" / name).read_bytes() == (b / "Spectrograms" / name).read_bytes(), name
    return names


def _rows(results, stub):
    """Rows of d, v, p under OPTIONS, from the tool's own selection."""
    from vasp_amd import postprocess
    with contextlib.redirect_stdout(io.StringIO()):
        ns, mesh, source, *_ = postprocess.prepare(["--folder", str(results), *OPTIONS], stub, lambda *a: None)
    source.close()
    run = sg.SpectrogramRun(None, mesh, ns, open_sessions=False)
    return {q: run.rows(q) for q in run.quantities}


def test_strips_write_the_unsplit_files_byte_for_byte(finished, tmp_path):
    results, stub = finished
    base = ["--folder", str(results), *OPTIONS]
    ns, lines = _post([*base, "--output-folder", str(tmp_path / "whole")], stub)
    assert not ns["strips"] and not any("in strips" in line for line in lines) and any("Spectrograms of 24 frames" in line for line in lines)
    rows = _rows(results, stub)
    big = max(rows.values())
    assert big >= 6 * CHUNK, rows                                      # several granules of rows
    size = -(-(-(-big // 3)) // CHUNK) * CHUNK                         # three strips of the largest quantity just fit
    limit = NEED(size, 25)
    assert NEED(-(-(-(-big // 2)) // CHUNK) * CHUNK, 25) > limit and -(-big // size) == 3
    ns, lines = _post([*base, "--output-folder", str(tmp_path / "split"), "--history-memory", str(limit)], stub)
    assert ns["strips"]
    said = [line for line in lines if "in strips" in line]
    assert len(said) == 3 and [line.split()[2] for line in said] == ["d", "v", "p"]
    for q, line in zip("dvp", said):
        k = len(strips.plan_row_strips(rows[q], CHUNK, 25, limit, NEED))
        assert f"Spectrograms of {q} in strips: {k} strips of at most" in line and f"({rows[q]} in all), the 24 frames read {k} times" in line
        assert "s reading" in line and "s transforming" in line
    assert max(len(strips.plan_row_strips(rows[q], CHUNK, 25, limit, NEED)) for q in rows) == 3
    names = _same_bytes(tmp_path / "whole", tmp_path / "split")
    assert len(names) == 12                                            # four CSV files per quantity
    # a second run in strips gives the same bytes again
    _post([*base, "--output-folder", str(tmp_path / "again"), "--history-memory", str(limit)], stub)
    _same_bytes(tmp_path / "split", tmp_path / "again")


def test_history_memory_leaves_no_trace_when_the_spectrogram_sessions_fit(finished, tmp_path):
    results, stub = finished
    base = ["--folder", str(results), *OPTIONS]
    rows = _rows(results, stub)
    fits = sum(NEED(r, 25) for r in rows.values())
    _, plain = _post([*base, "--output-folder", str(tmp_path / "plain")], stub)
    ns, lines = _post([*base, "--output-folder", str(tmp_path / "given"), "--history-memory", str(fits)], stub)
    assert not ns["strips"]
    path = lambda line: line.replace(str(tmp_path / "given"), "").replace(str(tmp_path / "plain"), "")
    assert [path(x) for x in lines if not x.startswith("Read ")] == [path(x) for x in plain if not x.startswith("Read ")]
    _same_bytes(tmp_path / "plain", tmp_path / "given")
    ns, _ = _post([*base, "--output-folder", str(tmp_path / "less"), "--history-memory", str(fits - 1)], stub)
    assert ns["strips"]
    _same_bytes(tmp_path / "plain", tmp_path / "less")


def test_a_limit_below_one_granule_is_refused_before_any_backend(finished, tmp_path):
    results, stub = finished

    class _Never(stub):
        def __init__(self, desc):
            raise AssertionError("a backend was built")

    from vasp_amd import postprocess
    one = NEED(CHUNK, 25)
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(SystemExit, match=rf"--history-memory: 128 rows, .* need {one} bytes over 25 frames, the histories may take {one - 1}"):
            postprocess.run(["--folder", str(results), "--output-folder", str(tmp_path / "no"), *OPTIONS, "--history-memory", str(one - 1)],
                            backend_factory=_Never, out=lambda *a: None)
    assert not (tmp_path / "no").exists()
