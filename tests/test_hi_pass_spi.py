"""The spectral power index under ``--hi-pass-spi``, host side: the NumPy twin of csrc/fsi_spi.hip (``spi_sums``, ``spi_close``,
``spi_rows``, ``spi_nodes``, ``HostBandSession.spi`` / ``spi_fetch``) against ``numpy.fft.rfft``'s one-sided ratio and against a
direct DFT in ``numpy.longdouble``; the cut-off's bin in exact rationals; the options and their refusals; the driver's files with
a stub backend; the C-ABI's new entry points.

The bound on an index (``spi_bound``)
-------------------------------------
One row of n frames: y_j = w_j (x_j - m) with m the mean, X_k = sum_j t_jk y_j with |t_jk| <= 1 a table entry,
Q = sum_j y_j^2, AC = n Q - |X_0|^2, L2 = sum_{1 <= k < kc} |X_k|^2, SPI = 1 - 2 L2 / AC.  With u = 2^-53:

* a bin, as ``power_bound`` of tests/test_spectrogram.py counts it: the table entry, the product t y, the difference x - m and
  the product with w are four roundings, counted as 8; the accumulation is n roundings whatever its order; both on either
  side of a comparison.  The mean is a sum of n terms of size <= max|x| on either side, off by at most dm = 2 n u max|x|, and
  enters y_j with weight |w_j|:

      dX = (2 n + 8) u sum_j |y_j| + sum_j |w_j| dm

* the low bins: dL2 = sum_{1 <= k < kc} (2 |X_k| dX + dX^2);
* the sum of squares: y_j is off by dy_j = 8 u |y_j| + |w_j| dm, its square by 2 |y_j| dy_j + dy_j^2, and the sum of n squares
  by another (2 n + 2) u Q for the squarings and the additions on either side:

      dQ = sum_j (2 |y_j| dy_j + dy_j^2) + (2 n + 2) u Q

* dAC = n dQ + (2 |X_0| dX + dX^2) + 4 u (n Q + |X_0|^2), the last term for the product n Q and the subtraction on either side;
* the index: d(2 L2 / AC) <= (2 dL2 + (2 L2 / AC) dAC) / (AC - dAC), and 2 L2 / AC = 1 - SPI:

      dSPI <= (2 dL2 + (1 - SPI) dAC) / (AC - dAC)

which says something only while AC - dAC > 0: every test asserts that margin on every row that is not constant on purpose.
|X_k|, Q, AC and SPI in the bound are those of the extended-precision DFT, not of the code under test.

``accumulation_only``: the part two evaluations with the same mean and the same y_j bits can differ by - dm = 0, dy_j = 0: what
holds the device to the twin (tests/test_gpu_hi_pass_spi.py), whose mean is the same ordered sum.

Nothing in it is tuned to what the code gives.  On the rows of this file the twin uses at most 5e-3 of the bound against rfft and
against the extended-precision DFT (the tests print the share): the bound is dominated by the mean's error, 4 n^2 u max|x|
sum|y|, which a real evaluation never gets near.
"""
import argparse
import contextlib
import io
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from test_session_restart import CYL, _run, one_modification_time  # noqa: F401  (the fixture holds h5lite's clock)
from vasp_amd import hi_pass as hp
from vasp_amd import spectrogram as sp

U = 2.0 ** -53
ROWS = 130
CASES = ((7, 2), (50, 2), (200, 5), (333, 9))        # (frames, kc): 25 Hz at 1 kHz but for n = 7, whose first bin is at 143 Hz
WINDOWS = ("boxcar", "hann")


# ---- helpers shared with tests/test_gpu_hi_pass_spi.py ------------------------------------------------------------------

def pulsatile_rows(n, shape, seed=3, mean=5.0):
    """(n,) + shape: per row a mean of its own, a pulsatile part of 0.5 and 1.5 cycles over the record and amplitude 0.15 .. 0.45,
    and white noise of 3e-3: an index between 1e-7 and 1e-2 at the cut-offs of CASES."""
    rng = np.random.default_rng(seed)
    t = (np.arange(n) / n).reshape((n,) + (1,) * len(shape))
    amp, ph = rng.uniform(0.15, 0.45, shape), rng.uniform(0, 2 * np.pi, shape)
    return mean * rng.uniform(0.5, 1.5, shape) + amp * np.sin(2 * np.pi * 0.5 * t + ph) + 0.3 * amp * np.sin(2 * np.pi * 1.5 * t + 2 * ph) \
        + 3e-3 * rng.standard_normal((n,) + tuple(shape))


def window_of(name, n):
    return None if name == "boxcar" else sp.window_values(name, n)


def spi_reference(x, w, kc):
    """Every row of frame-major x (n, ...) in ``numpy.longdouble``: the mean, y = w (x - m), the direct DFT of the bins
    0 .. n // 2 and the one-sided ratio.  Returns the ratio and the magnitudes ``spi_bound`` is built from, as float64."""
    x = np.asarray(x, dtype=np.float64)
    n, shape = len(x), x.shape[1:]
    xl = x.reshape(n, -1).astype(np.longdouble)
    wl = np.ones(n, dtype=np.longdouble) if w is None else np.asarray(w, dtype=np.float64).astype(np.longdouble)
    y = wl[:, None] * (xl - xl.sum(axis=0) / np.longdouble(n))
    k = np.arange(n // 2 + 1)
    ang = (np.longdouble(2) * sp.PI_L / np.longdouble(n)) * (np.outer(k, np.arange(n)) % n).astype(np.longdouble)
    re, im = np.cos(ang) @ y, np.sin(ang) @ y
    P = re * re + im * im
    f = np.full(len(k), 2.0, dtype=np.longdouble)
    if n % 2 == 0:
        f[-1] = 1.0
    total = (f[1:, None] * P[1:]).sum(axis=0)
    Q = (y * y).sum(axis=0)
    out = dict(spi=(f[kc:, None] * P[kc:]).sum(axis=0) / total, absX=np.sqrt(P), absy=np.abs(y), Q=Q, AC=np.longdouble(n) * Q - P[0],
               L2=P[1:kc].sum(axis=0), X0sq=P[0], one_sided=total)
    return {key: np.asarray(v, dtype=np.float64).reshape(v.shape[:-1] + shape) for key, v in out.items()}


def spi_bound(x, w, kc, ref, accumulation_only=False):
    """The module docstring's bounds per row: dL2, dX0sq, dQ, dAC, dSPI and the margin AC - dAC."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    aw = np.ones(n) if w is None else np.abs(np.asarray(w, dtype=np.float64))
    absy, absX, Q, AC = ref["absy"], ref["absX"], ref["Q"], ref["AC"]
    dm = np.zeros(x.shape[1:]) if accumulation_only else 2 * n * U * np.abs(x).max(axis=0)
    dX = (2 * n + 8) * U * absy.sum(axis=0) + aw.sum() * dm
    dL2 = (2 * absX[1:kc] * dX[None] + dX[None] ** 2).sum(axis=0)
    dX0 = 2 * absX[0] * dX + dX ** 2
    dQ = (2 * n + 2) * U * Q
    if not accumulation_only:
        dy = 8 * U * absy + aw.reshape((n,) + (1,) * (x.ndim - 1)) * dm[None]
        dQ = dQ + (2 * absy * dy + dy ** 2).sum(axis=0)
    dAC = n * dQ + dX0 + 4 * U * (n * Q + absX[0] ** 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        dSPI = (2 * dL2 + (1 - ref["spi"]) * dAC) / (AC - dAC)
    return dict(dL2=dL2, dX0sq=dX0, dQ=dQ, dAC=dAC, dSPI=dSPI, margin=AC - dAC)


def rfft_ratio(x, w, kc):
    """The one-sided ratio sum_{k >= kc} P_k / sum_{k >= 1} P_k of ``numpy.fft.rfft``, every bin doubled but the Nyquist bin."""
    n = len(x)
    y = x - x.mean(axis=0)
    if w is not None:
        y = np.asarray(w).reshape((n,) + (1,) * (x.ndim - 1)) * y
    P = np.abs(np.fft.rfft(y, axis=0)) ** 2
    f = np.full(P.shape[0], 2.0)
    if n % 2 == 0:
        f[-1] = 1.0
    f = f.reshape((-1,) + (1,) * (x.ndim - 1))
    return (f[kc:] * P[kc:]).sum(axis=0) / (f[1:] * P[1:]).sum(axis=0)


def _session(x, ncomp=3):
    s = hp.HostBandSession(ncomp, len(x))
    s.import_(x)
    return s


# ---- the twin against rfft and an extended-precision DFT ----------------------------------------------------------------------

@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n,kc", CASES, ids=[f"n{n}kc{k}" for n, k in CASES])
def test_twin_against_rfft_and_extended_precision(n, kc, window):
    x = pulsatile_rows(n, (ROWS,), seed=n)
    w = window_of(window, n)
    ref = spi_reference(x, w, kc)
    b = spi_bound(x, w, kc, ref)
    assert (b["margin"] > 0).all() and (ref["AC"] > 0).all()                    # the bound says something on every row
    got = hp.spi_rows(x, w, kc)
    assert got.shape == (ROWS,) and ((got > 0) & (got < 1)).all()
    share_l = np.abs(got - ref["spi"]) / b["dSPI"]
    share_f = np.abs(got - rfft_ratio(x, w, kc)) / b["dSPI"]
    print(f"n = {n}, kc = {kc}, {window}: SPI {got.min():.3g} .. {got.max():.3g}, bound {b['dSPI'].max():.3g}, largest share of it "
          f"against longdouble {share_l.max():.3g}, against rfft {share_f.max():.3g}")
    assert (share_l <= 1).all() and (share_f <= 1).all()
    # the three sums, each against its own bound; Parseval's AC against the one-sided sum it stands for
    L2, X0, Q, _ = hp.spi_sums(x, w, 0, kc)
    assert (np.abs(L2 - ref["L2"]) <= b["dL2"]).all() and (np.abs(Q - ref["Q"]) <= b["dQ"]).all()
    assert (np.abs(X0 - ref["X0sq"]) <= b["dX0sq"]).all()
    H, AC = hp.spi_close(L2, X0, Q, n)
    assert (np.abs(AC - ref["one_sided"]) <= b["dAC"]).all()
    # a session in two slabs forms the same sums but for the order of L2's additions
    s = _session(x[:, :, None], 1)
    if kc > 2:
        s.spi(w, 0, 2)
        s.spi(w, 2, kc - 2)
    else:
        s.spi(w, 0, kc)
    acc = spi_bound(x, w, kc, ref, accumulation_only=True)
    assert (np.abs(s.spi_fetch("rows")[:, 0] - got) <= acc["dSPI"]).all()
    assert np.array_equal(s.spi_fetch("nodes"), s.spi_fetch("rows")[:, 0])


def test_two_tones_have_the_known_answer():
    n, A, B = 240, 0.7, 0.02
    j = np.arange(n)
    x = (5.0 + A * np.sin(2 * np.pi * 3 * j / n) + B * np.sin(2 * np.pi * 40 * j / n + 0.4))[:, None]
    ref = spi_reference(x, None, 6)
    b = spi_bound(x, None, 6, ref)
    assert b["margin"][0] > 0
    got = hp.spi_rows(x, None, 6)[0]
    print(f"two tones: SPI {got!r}, B^2 / (A^2 + B^2) = {B * B / (A * A + B * B)!r}, bound {b['dSPI'][0]:.3g}")
    assert abs(got - B * B / (A * A + B * B)) <= b["dSPI"][0]
    above = spi_bound(x, None, 41, spi_reference(x, None, 41))
    assert above["margin"][0] > 0 and abs(hp.spi_rows(x, None, 41)[0]) <= above["dSPI"][0]
    assert hp.spi_rows(x, None, 1)[0] == 1.0                                      # no low bin: all the power is high


def test_the_cut_off_bin_in_exact_rationals():
    assert hp.spi_low_bins(200, 1e-3, 25) == 5                                   # 5 Hz bins: 25 Hz is bin 5, which counts as high
    assert hp.spi_low_bins(200, 1e-3, 25.0) == 5 and hp.spi_low_bins(200, 3 * 0.0001, 25) == 2 and hp.spi_low_bins(333, 1e-3, 25) == 9
    assert hp.spi_low_bins(7, 1e-3, 25) == 1 and hp.spi_low_bins(160, 1e-3, 406.25) == 65 and hp.spi_low_bins(160, 1e-3, 406.26) == 66
    dt, ulp = Fraction(1, 1000), Fraction(1, 2 ** 48)                             # an ulp of 25.0 is 2^-48
    for k in (1, 2, 5, 17, 99):
        edge = Fraction(k, 200) / dt                                              # bin k of 200 frames, exactly
        assert hp.spi_low_bins(200, dt, edge) == k
        assert hp.spi_low_bins(200, dt, edge - ulp) == k
        assert hp.spi_low_bins(200, dt, edge + ulp) == k + 1
    assert hp.spi_low_bins(200, dt, Fraction(500) - ulp) == 100
    for cutoff in (500, 500.0, Fraction(500), 1e6):
        with pytest.raises(SystemExit, match="at or above the Nyquist frequency 500 Hz"):
            hp.spi_low_bins(200, dt, cutoff)
    with pytest.raises(SystemExit, match="at or above the Nyquist frequency 250 Hz"):
        hp.spi_low_bins(200, 2e-3, 250)
    for cutoff in (0, -3.0):
        with pytest.raises(SystemExit, match="must be a frequency > 0 Hz"):
            hp.spi_low_bins(200, dt, cutoff)
    with pytest.raises(SystemExit, match="hold 1 frames, the index needs at least 2"):
        hp.spi_low_bins(1, dt, 25)
    # whatever the cut-off below Nyquist, the low bins have their mirror pair: kc - 1 <= (n - 1) // 2
    for n in (2, 3, 7, 8):
        assert hp.spi_low_bins(n, dt, Fraction(500) - ulp) - 1 <= (n - 1) // 2


# ---- special rows, the vector rule, the session's refusals -----------------------------------------------------------------------

def test_a_zero_row_gives_zero_and_a_nan_stays_in_its_node():
    n = 50
    x = pulsatile_rows(n, (9, 3), seed=2)
    x[:, 2, :] = 0.0                              # a node at rest
    x[:, 3, 1] = 0.0                              # one silent component
    x[0, 3, 1] = -0.0
    x[7, 5, 2] = np.nan
    x[n - 1, 6, 0] = np.inf
    clean = x.copy()
    clean[:, 5] = clean[:, 6] = 1.0
    s = _session(x)
    s.spi(None, 0, 2)
    rows, nodes = s.spi_fetch("rows"), s.spi_fetch("nodes")
    assert rows.shape == (9, 3) and nodes.shape == (9,)
    assert not rows[2].any() and not np.signbit(rows[2]).any() and nodes[2] == 0.0 and rows[3, 1] == 0.0
    assert np.isnan(rows[5, 2]) and np.isnan(rows[6, 0]) and np.isnan(nodes[5]) and np.isnan(nodes[6])
    finite = np.ones((9, 3), dtype=bool)
    finite[5, 2] = finite[6, 0] = False
    assert np.isfinite(rows[finite]).all() and np.isfinite(np.delete(nodes, [5, 6])).all()
    # the other rows are what they are without the two special values
    keep = np.array([0, 1, 2, 3, 4, 7, 8])
    assert np.array_equal(rows[keep], hp.spi_rows(clean, None, 2)[keep]) and np.array_equal(nodes[keep], hp.spi_nodes(clean, None, 2)[keep])
    assert ((rows[5, :2] > 0) & (rows[5, :2] < 1)).all() and ((rows[6, 1:] > 0) & (rows[6, 1:] < 1)).all()      # the special rows' neighbours
    sums = s.spi_fetch("sums")
    assert sums.shape == (3, 9, 3) and not sums[:, 2].any()


def test_the_vector_rule_sums_the_power():
    n, kc = 200, 5
    x = np.zeros((n, 3, 3))
    x[:, 0, 1] = pulsatile_rows(n, (), seed=8)    # one energetic component, two silent ones
    x[:, 1] = pulsatile_rows(n, (3,), seed=9)
    x[:, 2] = x[:, 1] @ np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])      # node 1 in rotated axes
    rows, nodes = hp.spi_rows(x, None, kc), hp.spi_nodes(x, None, kc)
    assert nodes[0] == rows[0, 1] and rows[0, 0] == 0.0 == rows[0, 2]
    L2, X0, Q, _ = hp.spi_sums(x, None, 0, kc)
    H, AC = hp.spi_close(L2, X0, Q, n)
    assert nodes[1] == ((H[1, 0] + H[1, 1]) + H[1, 2]) / ((AC[1, 0] + AC[1, 1]) + AC[1, 2])
    assert rows[1].min() < nodes[1] < rows[1].max()
    ref = spi_reference(x[:, 1:], None, kc)
    bound = (spi_bound(x[:, 1:], None, kc, ref)["dSPI"] * ref["AC"]).sum(axis=1) / ref["AC"].sum(axis=1)      # the AC-weighted mean of the rows' bounds
    assert abs(nodes[2] - nodes[1]) <= 3 * (bound[0] + bound[1])                  # invariant under the rotation, to rounding


def test_twin_refusals_and_invalidation():
    x = pulsatile_rows(12, (4, 3), seed=4)
    s = hp.HostBandSession(3, 13)
    s.import_(x)
    with pytest.raises(RuntimeError, match=r"no spectral power index \(spi first\)"):
        s.spi_fetch("nodes")
    with pytest.raises(RuntimeError, match="needs bin0 >= 0 and nb >= 1 bins"):
        s.spi(None, 0, 0)
    with pytest.raises(RuntimeError, match=r"a slab out of order: bin0 = 2, no slab stands before it \(bin0 = 0 first\)"):
        s.spi(None, 2, 1)
    with pytest.raises(RuntimeError, match="bins 0 .. 6 of 12 selected frames: a low bin lies below the Nyquist frequency, at most bin 5"):
        s.spi(None, 0, 7)
    s.spi(None, 0, 2)
    with pytest.raises(RuntimeError, match="a slab out of order: bin0 = 3, the next slab starts at bin 2"):
        s.spi(None, 3, 1)
    s.spi(None, 2, 2)                             # the refused slab left the sums standing
    acc = spi_bound(x, None, 4, spi_reference(x, None, 4), accumulation_only=True)
    assert (acc["margin"] > 0).all() and (np.abs(s.spi_fetch("rows") - hp.spi_rows(x, None, 4)) <= acc["dSPI"]).all()
    with pytest.raises(RuntimeError, match="what must be one of rows, nodes, sums"):
        s.spi_fetch("spectrum")
    assert s.select(1, 5, 2) == 5                 # a selection drops the index; the next one is formed on the view
    with pytest.raises(RuntimeError, match=r"no spectral power index \(spi first\)"):
        s.spi_fetch("rows")
    s.spi(sp.window_values("hann", 5), 0, 2)
    assert np.array_equal(s.spi_fetch("nodes"), hp.spi_nodes(x[1:10:2], sp.window_values("hann", 5), 2))
    s.sample(x[0])
    with pytest.raises(RuntimeError, match=r"no spectral power index \(spi first\)"):
        s.spi_fetch("rows")
    one = _session(x[:1])
    with pytest.raises(RuntimeError, match="1 selected frames, the index needs at least 2"):
        one.spi(None, 0, 1)
    tensor = _session(np.zeros((8, 2, 6)), 6)
    with pytest.raises(RuntimeError, match="a strain / stress session has no spectral power index"):
        tensor.spi(None, 0, 2)


# ---- the options and the refusals before a run ---------------------------------------------------------------------------------

def _parameters(extra, hi_pass=("--hi-pass", "v")):
    from vasp_amd.monolithic import parameters
    with contextlib.redirect_stdout(io.StringIO()):
        return parameters(["-p", "cylinder", *hi_pass, "--verbose", "False", "-dt", "0.001", "--save-step", "1", *extra])[2]


def _refusal(extra):
    return hp.hi_pass_refusal(_parameters(extra), 1, None)


def test_each_refusal_has_its_message():
    on = ["--hi-pass-spi"]
    assert hp.spi_options({}) is None
    assert hp.spi_options(dict(hi_pass_spi=True)) == dict(cutoff=25.0, window="boxcar")
    assert hp.spi_options(dict(hi_pass_spi=True, hi_pass_spi_cutoff=40, hi_pass_spi_window="hann")) == dict(cutoff=40.0, window="hann")
    assert _refusal(["-T", "0.0115", *on]) == ""                                    # 12 frames: no band has enough, the index has
    assert "padlen + 1 = 34" in _refusal(["-T", "0.0115"])                         # without the option nothing has changed
    assert _refusal(["-T", "0.0235", *on, "--hi-pass-stride", "2", "--hi-pass-spi-cutoff", "249.9", "--hi-pass-spi-window", "hann"]) == ""
    msg = _refusal(["-T", "0.0235", *on, "--hi-pass-stride", "2", "--hi-pass-spi-cutoff", "250"])
    assert "--hi-pass-spi-cutoff 250 Hz is at or above the Nyquist frequency 250 Hz of frames 0.002 s apart" in msg
    assert "at or above the Nyquist frequency 500 Hz" in _refusal(["-T", "0.0115", *on, "--hi-pass-spi-cutoff", "500"])
    msg = _refusal(["-T", "0.0115", *on, "--hi-pass-start-time", "0.0115"])
    assert "hold 1 frames, the index needs at least 2" in msg
    for sub in (["--hi-pass-spi-cutoff", "30"], ["--hi-pass-spi-window", "hann"]):
        with pytest.raises(SystemExit, match=f"{sub[0]} belongs to --hi-pass-spi"):
            _refusal(["-T", "0.039", *sub])
    with pytest.raises(SystemExit, match="--hi-pass-spi-cutoff must be a frequency > 0 Hz"):
        _refusal(["-T", "0.0115", *on, "--hi-pass-spi-cutoff", "-1"])
    with pytest.raises(SystemExit, match="--hi-pass-spi-window must be one of boxcar, hann"):
        hp.spi_options(dict(hi_pass_spi=True, hi_pass_spi_window="blackman"))
    with pytest.raises(SystemExit):                                                  # argparse knows the two windows
        _refusal(["-T", "0.0115", *on, "--hi-pass-spi-window", "blackman"])
    assert "one rank only" in hp.hi_pass_refusal(_parameters(["-T", "0.0115", *on]), 2, None)
    # without --hi-pass there is no history to form it on
    from vasp_amd import monolithic, postprocess
    with pytest.raises(SystemExit, match="--hi-pass-spi needs --hi-pass with at least one of d, v, p"):
        monolithic._refuse_sessions(["-p", "cylinder", "--hi-pass-spi"], None, 1)
    with pytest.raises(SystemExit, match="--hi-pass-spi needs --hi-pass with at least one of d, v, p"):
        postprocess.prepare(["--folder", str(ROOT), "--hi-pass-spi"])


def test_a_history_in_strips_refuses_the_option(tmp_path):
    from vasp_amd.mesh import FsiMesh
    mesh = FsiMesh.read(CYL)
    ns = dict(_parameters(["-T", "0.0115", "--hi-pass-spi"]), save_deg=2, results_folder=tmp_path, hi_pass_strip=(0, 8))
    with pytest.raises(SystemExit) as e:
        hp.HiPassRun(object(), mesh, ns)
    assert str(e.value) == hp.SPI_STRIPS and "strips of rows" in str(e.value) and str(e.value) != hp.PHASE_STRIPS
    assert not (tmp_path / "Visualization_hi_pass").exists()


# ---- the driver with a stub backend -------------------------------------------------------------------------------------------

def _vectors(path):
    from vasp_amd.h5lite import read_h5
    g = read_h5(path)["VisualisationVector"]
    return np.stack([np.asarray(g[str(k)].data) for k in range(len(g.keys()))])


def _frames(results, name):
    return _vectors(results / "Visualization" / f"{name}.h5")


def _csv(path):
    lines = path.read_text().splitlines()
    return lines[0], [[c.strip() for c in line.split(",")] for line in lines[1:]]


def test_driver_writes_the_index_of_the_saved_frames(tmp_path):
    """40 saved frames 1 ms apart: 25 Hz bins, the default cut-off is bin 1 - no low bin; 60 Hz leaves bins 1 and 2 below."""
    options = ["--hi-pass", "v", "p", "--hi-pass-spi", "--hi-pass-spi-cutoff", "60"]
    ns, lines = _run(tmp_path / "case", options=options)
    results = tmp_path / "case" / "1"
    out = results / "Visualization_hi_pass"
    assert any("Hi-pass velocity_spi_60: spectral power index over 40 frames, 2 bins of 25 Hz below the cut-off (boxcar), written" in line for line in lines)
    names = {p.name for p in out.iterdir()}
    assert {"velocity_spi_60.h5", "velocity_spi_60.xdmf", "pressure_spi_60.h5", "pressure_spi_60.xdmf", "spi.csv"} <= names
    assert {"velocity_25_to_1000.h5", "pressure_25_to_1000.h5"} <= names              # the bands are written as without the option
    header, rows = _csv(out / "spi.csv")
    assert header == "# " + hp.SPI_HEADER and len(hp.SPI_HEADER.split(",")) == 11 and [r[0] for r in rows] == ["velocity", "pressure"]
    for name, row in zip(("velocity", "pressure"), rows):
        x = _frames(results, name)
        assert x.dtype == np.float64 and len(x) == 40
        field = hp.spi_nodes(x, None, 3)
        got = _vectors(out / f"{name}_spi_60.h5")
        assert got.shape == (1, x.shape[1], 1) and np.array_equal(got[0, :, 0], field.astype(np.float32))
        assert 'AttributeType="Scalar"' in (out / f"{name}_spi_60.xdmf").read_text()
        assert len(row) == 11 and row[1:7] == ["60.0", "boxcar", "40", "1000.0", "25.0", "3"]
        assert [float(c) for c in row[7:10]] == [field.min(), field.mean(), field.max()] and int(row[10]) == int(np.argmax(field))
        assert 0 < field.min() and field.max() < 1
    # a Hann window, a stride and a start time: the index of the selected frames
    options = ["--hi-pass", "v", "--hi-pass-spi", "--hi-pass-spi-window", "hann", "--hi-pass-stride", "2", "--hi-pass-start-time", "0.011"]
    ns, lines = _run(tmp_path / "view" / "case", options=options)
    results = tmp_path / "view" / "case" / "1"
    x = _frames(results, "velocity")[10::2]
    assert len(x) == 15 and hp.spi_low_bins(15, 2e-3, 25) == 1
    got = _vectors(results / "Visualization_hi_pass" / "velocity_spi_25.h5")
    assert np.array_equal(got[0, :, 0], hp.spi_nodes(x, sp.window_values("hann", 15), 1).astype(np.float32))
    _, rows = _csv(results / "Visualization_hi_pass" / "spi.csv")
    assert rows[0][:7] == ["velocity", "25.0", "hann", "15", "500.0", repr(1.0 / (15 * 2e-3)), "1"]


def test_without_the_option_the_files_are_those_of_before(tmp_path):
    base = ["--hi-pass", "v", "--hi-pass-amplitude", "--hi-pass-window", "8", "--hi-pass-point-ids", "0"]
    from test_hi_pass_phase import _outputs
    _run(tmp_path / "without" / "case", options=base)
    _run(tmp_path / "with" / "case", options=base + ["--hi-pass-spi"])
    old, new = _outputs(tmp_path / "without" / "case" / "1"), _outputs(tmp_path / "with" / "case" / "1")
    assert set(old) < set(new) and all(new[k] == v for k, v in old.items())           # what the options of before write: not a byte changed
    assert {k.split("/")[1] for k in set(new) - set(old)} == {"velocity_spi_25.h5", "velocity_spi_25.xdmf", "spi.csv"}


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------

def test_header_binding_and_kernel_source_agree():
    from vasp_amd import capi
    from vasp_amd.monolithic import add_session_arguments
    header = (ROOT / "include" / "vaspfsi.h").read_text()
    lib = capi.load_library()
    for name in ("fsi_band_spi", "fsi_band_spi_fetch"):
        m = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S)
        assert m and name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
    for k, what in enumerate(hp.SPI_WHAT):
        assert re.search(r"#define FSI_SPI_%s %d\b" % (what.upper(), k), header) and capi.HipBackend.SPI_WHAT[what] == k
    src = (ROOT / "vasp_amd" / "csrc" / "fsi_spi.hip").read_text()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("#include")[1:][-1].lower()
    assert "fsi_spi.hip" in (ROOT / "vasp_amd" / "csrc" / "Makefile").read_text()
    tiles = (ROOT / "vasp_amd" / "csrc" / "fsi_spec.hpp").read_text()
    assert "SPEC_ROWS = 128;" in tiles and "SPEC_BINS = 64;" in tiles and "SPEC_KC = 16;" in tiles      # what the GPU shapes rely on
    ap = argparse.ArgumentParser()
    add_session_arguments(ap)
    ns = vars(ap.parse_args([]))
    assert all(ns[k] is None for k in ("hi_pass_spi", "hi_pass_spi_cutoff", "hi_pass_spi_window"))
    assert hasattr(capi.HipBackend, "hi_pass_spi") and hasattr(capi.HipBackend, "hi_pass_spi_fetch")
    assert hasattr(hp.HostBandSession, "spi") and hasattr(hp.HostBandSession, "spi_fetch")
