"""Multiband cascades, frame selections and point traces of the band-pass sessions on the device (csrc/fsi_band.hip:
k_band_filter_next, k_band_trace and the strided k_band_filter; HipBackend.hi_pass_select / _filter_next / _trace;
``--hi-pass-multiband``, ``--hi-pass-point-ids``) against the host restatement of scipy's filtfilt (vasp_amd/hi_pass.py)."""
import numpy as np
import pytest

from test_gpu_hi_pass import DT, FRAMES, STENOSIS, WINDOW, _files, _rows, _run, _signal, _vectors
from vasp_amd import hi_pass as hp

pytestmark = pytest.mark.gpu

CASCADE = ((25.0, 450.0, "bandpass"), (100.0, 150.0, "bandstop"), (200.0, 230.0, "bandstop"))
KEYS = ("b", "a", "zi", "padlen")


def _stages(cascade=CASCADE, dt=DT):
    return [hp.design(dt, lo, hi, btype) for lo, hi, btype in cascade]


def _host(x, stages):
    for prm in stages:
        x = hp.filtfilt_rows(prm["b"], prm["a"], x, prm["zi"], prm["padlen"])
    return x


def _device(hb, q, stages):
    for k, prm in enumerate(stages):
        (hb.hi_pass_filter_next if k else hb.hi_pass_filter)(q, *(prm[key] for key in KEYS))


def _filtered(hb, q, n):
    return np.stack([hb.hi_pass_fetch(q, "filtered", k) for k in range(n)])


@pytest.fixture(scope="module")
def recorded(stenosis_case):
    """As tests/test_gpu_hi_pass.py: a context on the small stenosis mesh driven through fsi_set_state with a prescribed
    signal, every frame sampled by the three sessions."""
    from vasp_amd.capi import HipBackend
    mesh, desc = stenosis_case[0]["mesh"], stenosis_case[1]
    hb = HipBackend(desc)
    states = _signal(hb.ndof)
    for q in "dvp":
        hb.hi_pass_begin(q, *hp.output_nodes(mesh, 2, q), capacity=FRAMES)
    for k in range(FRAMES):
        hb.set_state("n", states[k])
        for q in "dvp":
            hb.hi_pass_sample(q)
    yield hb, mesh, states
    hb.close()


@pytest.fixture()
def whole(recorded):
    """The recorded sessions with every frame selected, whatever the test before left."""
    hb = recorded[0]
    for q in "dvp":
        assert hb.hi_pass_select(q, 0, -1, 1) == FRAMES
    return recorded


def test_cascade_equals_the_staged_host_restatement_bit_for_bit(whole):
    hb, mesh, states = whole
    stages = _stages()
    single = hp.design(DT, 25.0, 1000.0)
    for q in "dvp":
        x = _rows(mesh, states, q)
        y = _host(x, stages)
        _device(hb, q, stages)
        got = _filtered(hb, q, FRAMES)
        print(f"{q}: after three stages max |device - host| = {np.abs(got - y).max():.3e}, max |y| = {np.abs(y).max():.3e}, "
              f"{int((got != y).sum())} of {y.size} values differ")
        assert np.array_equal(got, y), q
        for k in (0, 1, FRAMES // 2, FRAMES - 1):                                    # the raw frames are still what was set
            assert np.array_equal(hb.hi_pass_fetch(q, "raw", k), x[k]), (q, k)
        # a stage leaves nothing behind: the plain single band again
        hb.hi_pass_filter(q, *(single[key] for key in KEYS))
        assert np.array_equal(_filtered(hb, q, FRAMES), _host(x, [single])), q


def test_a_shorter_padlen_follows_a_longer_one_and_the_reverse_is_refused(whole):
    """A low-pass stage (6 coefficients, padlen 18) after a band-pass (33): the series moves down inside its buffer.  The
    reverse would write the head of the extension over the series it is formed from: refused."""
    from vasp_amd.capi import FsiError
    hb, mesh, states = whole
    stages = [hp.design(DT, 25.0, 450.0, "bandpass"), hp.design(DT, 0.0, 200.0), hp.design(DT, 0.0, 120.0)]
    assert [prm["padlen"] for prm in stages] == [33, 18, 18]
    x = _rows(mesh, states, "v")
    _device(hb, "v", stages)
    assert np.array_equal(_filtered(hb, "v", FRAMES), _host(x, stages))
    with pytest.raises(FsiError, match="padlen = 33 after a stage of padlen = 18"):
        hb.hi_pass_filter_next("v", *(stages[0][key] for key in KEYS))
    assert np.array_equal(_filtered(hb, "v", FRAMES), _host(x, stages))                # the refused stage touched nothing


def test_edge_lengths_and_a_partial_wavefront(cylinder_case):
    """65 vertices x 3 = 195 rows (three full wavefronts and three lanes) and a p session of one row, at 34 frames = padlen + 1
    - the tail extension takes every saved sample down to index 0, L = 100 is no multiple of the 8 frames loaded ahead - and at
    38 frames, L = 104."""
    from vasp_amd.capi import HipBackend
    mesh, desc = cylinder_case[0]["mesh"], cylinder_case[1]
    V, N2 = mesh.num_vertices, mesh.num_nodes
    rng = np.random.default_rng(21)
    nodes = np.sort(rng.choice(V, 65, replace=False)).astype(np.int32)
    stages = _stages(CASCADE[:2])
    hb = HipBackend(desc)
    try:
        states = 1e-3 * rng.standard_normal((38, hb.ndof))
        hb.hi_pass_begin("v", nodes, None, 38)
        hb.hi_pass_begin("p", [V - 1], None, 38)
        xv = states[:, 3 * N2:6 * N2].reshape(38, N2, 3)[:, nodes]
        xp = states[:, 6 * N2 + V - 1].reshape(38, 1, 1)
        done = 0
        for n in (34, 38):
            for k in range(done, n):
                hb.set_state("n", states[k])
                hb.hi_pass_sample("v")
                hb.hi_pass_sample("p")
            done = n
            for q, x in (("v", xv), ("p", xp)):
                _device(hb, q, stages)
                got, y = _filtered(hb, q, n), _host(x[:n], stages)
                print(f"{q}, {n} frames: {int((got != y).sum())} of {y.size} values differ")
                assert np.array_equal(got, y), (q, n)
                assert np.array_equal(hb.hi_pass_fetch(q, "raw", n - 1), x[n - 1])
    finally:
        hb.close()


def test_selection(whole):
    from vasp_amd.capi import FsiError
    hb, mesh, states = whole
    stages = _stages(CASCADE[:2])
    single = hp.design(DT, 25.0, 1000.0)
    for q in "dvp":
        x = _rows(mesh, states, q)
        assert hb.hi_pass_select(q, 1, -1, 2) == 36
        _device(hb, q, stages[:1])
        assert np.array_equal(_filtered(hb, q, 36), _host(x[1::2], stages[:1])), q      # filtered frame k is selected frame k
        hb.hi_pass_filter_next(q, *(stages[1][key] for key in KEYS))
        assert np.array_equal(_filtered(hb, q, 36), _host(x[1::2], stages)), q
        with pytest.raises(FsiError, match="frame out of range"):
            hb.hi_pass_fetch(q, "filtered", 36)
        for k in (0, 1, 36, FRAMES - 1):                                              # the raw fetch stays absolute
            assert np.array_equal(hb.hi_pass_fetch(q, "raw", k), x[k]), (q, k)
        # a window inside the history: first 5, 40 frames, every frame
        assert hb.hi_pass_select(q, 5, 40, 1) == 40
        _device(hb, q, stages)
        assert np.array_equal(_filtered(hb, q, 40), _host(x[5:45], stages)), q
        # too few frames left
        assert hb.hi_pass_select(q, 0, -1, 3) == 24
        with pytest.raises(FsiError, match="24 recorded frames, the filter needs more than padlen = 33"):
            hb.hi_pass_filter(q, *(single[key] for key in KEYS))
        with pytest.raises(FsiError, match="fsi_band_filter first"):
            hb.hi_pass_fetch(q, "filtered", 0)
        # every frame, said explicitly: the unselected result
        assert hb.hi_pass_select(q, 0, 72, 1) == 72
        hb.hi_pass_filter(q, *(single[key] for key in KEYS))
        assert np.array_equal(_filtered(hb, q, FRAMES), _host(x, [single])), q


def test_amplitude_of_a_cascade(whole):
    """The bound of test_amplitudes_against_the_host_restatement: the device sums a window's squares running, the reference's
    formula directly; the device may differ from the formula by 4 x the spread between the two on the host, on these rows."""
    from vasp_amd.capi import FsiError
    hb, mesh, states = whole
    stages = _stages()
    for q in "dvp":
        y = _host(_rows(mesh, states, q), stages)
        direct, running = hp.windowed_rms_rows(y, WINDOW), hp.windowed_rms_running(y, WINDOW)
        spread = np.abs(direct - running).max()
        _device(hb, q, stages)
        hb.hi_pass_amplitude(q, WINDOW)
        amp = np.stack([hb.hi_pass_fetch(q, "amplitude", k) for k in range(FRAMES)])
        err = np.abs(amp - direct).max()
        print(f"{q}: host direct vs running spread {spread:.3e}, device vs direct {err:.3e}, device vs running "
              f"{np.abs(amp - running).max():.3e}, max amplitude {direct.max():.3e}")
        assert spread > 0
        assert err <= 4 * spread, q
        assert not np.isnan(amp).any() and (amp >= 0).all()
        # a further stage invalidates the amplitude
        hb.hi_pass_filter_next(q, *(stages[1][key] for key in KEYS))
        with pytest.raises(FsiError, match="fsi_band_amplitude first"):
            hb.hi_pass_fetch(q, "amplitude", 10)


def test_trace(whole):
    hb, mesh, states = whole
    stages = _stages(CASCADE[:2])
    eps = np.finfo(float).eps
    for q in "dvp":
        n = len(hp.output_nodes(mesh, 2, q)[0])
        points = [0, 64, n - 1, 0]              # the first lane, the first of the second wavefront, the last node, a duplicate
        hb.hi_pass_select(q, 1, -1, 2)
        _device(hb, q, stages)
        for what, frames in (("raw", range(1, FRAMES, 2)), ("filtered", range(36))):
            ref = np.stack([hb.hi_pass_fetch(q, what, k) for k in frames])[:, points].transpose(1, 0, 2)
            tr = hb.hi_pass_trace(q, what, points)
            assert tr.shape == (4, 36, 1 + ref.shape[2])
            assert np.array_equal(tr[:, :, 1:], ref), (q, what)
            mag = np.linalg.norm(ref, axis=2) if q != "p" else ref[:, :, 0]          # a scalar's magnitude is the value itself
            dist = np.abs(tr[:, :, 0] - mag).max()
            print(f"{q} {what}: magnitude vs numpy.linalg.norm {dist:.3e}, max {np.abs(mag).max():.3e}")
            assert dist <= 4 * eps * np.abs(mag).max(), (q, what)
            if q == "p":
                assert np.array_equal(tr[:, :, 0], tr[:, :, 1])
        hb.hi_pass_select(q, 0, -1, 1)
        assert np.array_equal(hb.hi_pass_trace(q, "raw", [n - 1])[0, :, 1:], _rows(mesh, states, q)[:, n - 1])


def test_errors_leave_the_session_usable(whole, cylinder_case):
    from vasp_amd.capi import FsiError, HipBackend
    hb, mesh, states = whole
    stages = _stages(CASCADE[:2])
    n = len(hp.output_nodes(mesh, 2, "d")[0])
    with pytest.raises(FsiError, match=r"no filtered series \(fsi_band_filter first\)"):          # the fixture just selected
        hb.hi_pass_filter_next("d", *(stages[1][key] for key in KEYS))
    with pytest.raises(FsiError, match=r"no filtered series \(fsi_band_filter first\)"):
        hb.hi_pass_trace("d", "filtered", [0])
    for bad in ((0, 73, 1), (72, -1, 1), (1, 37, 2), (0, -1, 0), (-1, -1, 1), (0, 0, 1)):
        with pytest.raises(FsiError, match=r"first \+ \(count - 1\) \* stride < the 72 recorded frames"):
            hb.hi_pass_select("d", *bad)
    for bad in ([0, n], [-1]):
        with pytest.raises(FsiError, match="node out of range"):
            hb.hi_pass_trace("d", "raw", bad)
    fresh = HipBackend(cylinder_case[1])
    try:
        with pytest.raises(FsiError, match="fsi_band_begin first"):
            fresh.hi_pass_select("v", 0, -1, 1)
        fresh.hi_pass_begin("v", [0, 1], None, 4)
        with pytest.raises(FsiError, match="the 0 recorded frames"):
            fresh.hi_pass_select("v", 0, -1, 1)
    finally:
        fresh.close()
    # the refused calls changed nothing: every frame is still selected, and the cascade runs
    x = _rows(mesh, states, "d")
    _device(hb, "d", stages)
    assert np.array_equal(_filtered(hb, "d", FRAMES), _host(x, stages))
    assert np.array_equal(hb.hi_pass_trace("d", "filtered", [n - 1])[0, :, 1:], _host(x, stages)[:, n - 1])


# ---- end to end -------------------------------------------------------------------------------------------------------

def test_end_to_end_multiband_run_and_point_traces(tmp_path):
    """--hi-pass d v p with two bands, the cascade of both, two point traces and the amplitudes on the small stenosis mesh, 41
    saved frames, in fresh processes."""
    from vasp_amd.mesh import FsiMesh
    base = ["--hi-pass", "d", "v", "p", "--hi-pass-bands", "25", "450", "100", "150", "--hi-pass-amplitude", "--hi-pass-window", "8"]
    new = ["--hi-pass-multiband", "--hi-pass-pass-stop", "pass", "stop", "--hi-pass-point-ids", "0", "5"]
    res, log = _run(tmp_path, "with", base + new)
    old, _ = _run(tmp_path, "without", base)
    twice, _ = _run(tmp_path, "twice", base + new)
    mesh = FsiMesh.read(STENOSIS)
    states = np.load(res / "hook_states.npy")
    n = len(states)
    assert n == 41 and "Hi-pass fields of 41 frames (d, v, p)" in log
    out = res / "Visualization_hi_pass"
    stages = _stages(CASCADE[:2])
    times = np.arange(n) * 1e-3
    for q, name in hp.VIZ_TYPE.items():
        x = _rows(mesh, states, q)
        assert np.array_equal(_vectors(res / "Visualization" / f"{name}.h5"), x)          # the hook saw what the writer wrote
        viz = f"{name}_pass_25_to_450_stop_100_to_150"
        y = _host(x, stages)
        got = _vectors(out / f"{viz}.h5")
        assert got.dtype == np.float32 and np.array_equal(got, y.astype(np.float32)), q
        direct, running = hp.windowed_rms_rows(y, 8), hp.windowed_rms_running(y, 8)
        spread = np.abs(direct - running).max()
        amp = _vectors(out / f"{viz}_amplitude.h5")
        err = np.abs(amp.astype(np.float64) - direct)
        print(f"{q}: cascade amplitude files vs the reference formula {err.max():.3e}, host spread {spread:.3e}, max {direct.max():.3e}")
        assert (err <= 4 * spread + 0.5 * np.finfo(np.float32).eps * np.abs(direct)).all(), q
        assert np.loadtxt(out / f"{viz}.csv", delimiter=",").shape == (n, 13)
        assert (out / f"{viz}.xdmf").read_text() == hp.xdmf_text(n, 1e-3, 0.0, 8 * mesh.num_cells, mesh.num_nodes,
                                                                 "Scalar" if q == "p" else "Vector", viz)
        for i in (0, 5):
            data = np.loadtxt(res / "Visualization_separate_domain" / f"{name}_point_id_{i}.csv", delimiter=",")
            assert data.shape == (n, 2 if q == "p" else 5)
            np.testing.assert_allclose(data[:, 0], times, rtol=1e-15, atol=0)
            assert np.array_equal(data[:, -x.shape[2]:], x[:, i]), (q, i)                 # the hooked rows: savetxt's %.18e round-trips
            mag = np.linalg.norm(x[:, i], axis=1) if q != "p" else x[:, i, 0]
            assert np.abs(data[:, 1] - mag).max() <= 4 * np.finfo(float).eps * np.abs(mag).max(), (q, i)
    # the per-band files and Visualization/ are those of a run without the three new flags, dataset for dataset
    with_files, old_files = _files(out), _files(old / "Visualization_hi_pass")
    assert not (old / "Visualization_separate_domain").exists()
    assert len(old_files) == 3 * 2 * (2 * (1 + 2 + n) + 1) and set(old_files) < set(with_files)
    assert all(with_files[k] == v for k, v in old_files.items())
    assert all("_pass_25_to_450_stop_100_to_150" in k for k in set(with_files) - set(old_files))
    assert _files(res / "Visualization") == _files(old / "Visualization")
    # a second identical run writes identical files
    assert _files(twice / "Visualization_hi_pass") == with_files
    assert _files(twice / "Visualization_separate_domain") == _files(res / "Visualization_separate_domain")
