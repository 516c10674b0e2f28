"""Band-pass filtered fields and vibration amplitudes of a run: `<results>/Visualization_hi_pass/`, libhdf5-free.

Counterpart of ``vasp-create-hi-pass-viz`` [REF src/vasp/postprocessing/postprocessing_h5py/create_hi_pass_viz.py:29-426],
whose node loops run on the device on a history recorded during the run (``HipBackend.hi_pass_*``, csrc/fsi_band.hip).
This module holds

* the band logic of the reference, verbatim (``band_parameters``), and the filter design, taken from scipy as the reference
  takes it (``design``): a 1-ulp change of ``a`` is visible in the output, so nothing is re-derived;
* the NumPy restatement of the whole chain - scipy's ``filtfilt`` (odd extension, transposed direct form II, ``lfilter_zi``
  scaled by the first / last sample) and the reference's windowed RMS - vectorised over rows.  Every operation is an
  element-wise IEEE operation in scipy's order, so a row's result equals ``scipy.signal.filtfilt`` bit for bit.  It is the
  path of a backend without the device session (``HostBandSession``) and the yardstick of the GPU tests;
* the writer of the reference's files and the driver's side of ``--hi-pass`` (``HiPassRun``): one series per band, with
  ``--hi-pass-multiband`` one more that went through all bands in order, each passed or stopped
  [REF create_hi_pass_viz.py:532-545,191-198,651-657]; a frame window and stride (``--hi-pass-stride``,
  ``--hi-pass-start-time``, ``--hi-pass-end-time``); the raw series of listed nodes (``--hi-pass-point-ids``);
* the phase-averaged decomposition of ``--hi-pass-phase-average`` - what the reference's ``vasp-log-plotter`` forms at probe
  points [REF log_plotter.py:902-989], here per written node (csrc/fsi_phase.hip): its NumPy twin (``phase_average``,
  ``fluctuation_energy``, ``ordered_mean``, ``HostBandSession.phase`` / ``phase_fetch``), the period arithmetic with its
  refusals (``phase_cycle``, ``phase_period``, ``phase_cycles``) and its files (``HiPassRun._write_phase``);
* the spectral power index of ``--hi-pass-spi`` (Khan et al., J. Biomech. 2017), the fraction of a row's non-mean spectral
  power at or above a cut-off frequency, per written node (csrc/fsi_spi.hip): its NumPy twin (``spi_sums``, ``spi_close``,
  ``spi_rows``, ``spi_nodes``, ``HostBandSession.spi`` / ``spi_fetch``), the cut-off's bin in exact rationals
  (``spi_low_bins``), the options with their refusals (``spi_options``) and its files (``HiPassRun._write_spi``);
* the snapshot proper orthogonal decomposition of ``--hi-pass-pod`` - modes, energies and time coefficients of the selected frames
  and of every band's filtered series (csrc/fsi_pod.hip): its NumPy twin (``pod_gram``, ``pod_modes``, ``HostBandSession.pod_gram`` /
  ``pod_modes`` / ``pod_fetch``), the one eigen step of device and twin with its resolution floor (``pod_eig``, ``pod_table``), the
  lumped volumes of the written nodes (``pod_volume_weights``), the options (``pod_options``) and the files (``HiPassRun._write_pod``);
* the strain rate of a session's vector history on mesh cells, which ``--hi-pass-flow-metrics`` closes into dissipation and
  resolution metrics (``vasp_amd/flow_metrics.py``): the NumPy twin of csrc/fsi_rate.hip (``cell_rate``,
  ``HostBandSession.cells`` / ``cell_rate``; in the current configuration of the ALE mesh ``cell_rate_current`` /
  ``HostBandSession.cell_rate_current``, which pairs the field's frames with the displacement session's), and where
  ``HiPassRun.write`` collects the rates;
* the Q-criterion, enstrophy, helicity and kinetic energy of the same history on the same cells and their ordered weighted
  sums, which ``--hi-pass-vortex`` closes into the files of ``vasp_amd/vortex.py``: the NumPy twin of csrc/fsi_vortex.hip
  (``cell_vortex``, ``cell_wsum``, ``HostBandSession.cell_weights`` / ``cell_vortex``; in the current configuration
  ``cell_vortex_current`` / ``HostBandSession.cell_vortex_current``, on the 14-point rule ``vortex_rule``);
* what the four post-processing options share to go through a checkpoint: the manifest and the files of
  ``<results>/Checkpoint/sessions/`` and the checks of a restart (``save_sessions``, ``restart_entry``), and the saving and
  restoring of a recorded history (``SessionRun``);
* the three parameters by which ``vasp_amd.postprocess`` tells the options the frames of a finished folder instead of a run's
  ``T`` and ``save_step``: ``frame_times`` (``saved_times``), ``frame_stride`` (``frame_spacing``), ``frame_start``.  A run
  sets none of them.

* what a band-pass in strips of rows (``hi_pass_strips.py``, for a history larger than the device) needs of this module: the
  strip a ``HiPassRun`` is opened on, the list of the series it writes (``series_list``), numpy's percentile from two order
  statistics (``percentiles_from_ranks``), the board of all strips' amplitude magnitudes and the table formed on it.

What a filter stage and a trace cost on a mesh of the benchmark's size has not been measured.
The reference's ``strain`` / ``stress`` quantities are ``--hi-pass-tensor`` (``hi_pass_tensor.py``), on the sessions of this module.
"""
from __future__ import annotations

import hashlib
import json
import os
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np

from .h5lite import Dataset, Group, H5Series
from .mesh import FsiMesh

ORDER = 5                                       # butter_bandpass(order=5) [REF spectrograms.py:502]
VIZ_TYPE = {"d": "displacement", "v": "velocity", "p": "pressure"}      # [REF create_hi_pass_viz.py:86-91]
RMS_REFRESH = 64                                # csrc/fsi_band.hpp: BAND_RMS_REFRESH
CSV_HEADER = ("time (s), 95th percentile amplitude, 5th percentile amplitude, maximum amplitude, "
              "minimum amplitude, average amplitude, 90th percentile amplitude, 10th percentile amplitude, "
              "97.5th percentile amplitude, 2.5th percentile amplitude, 99th percentile amplitude, "
              "1st percentile amplitude, ID of node with max amplitude")          # [REF create_hi_pass_viz.py:397-400]
CSV_PERCENTILES = (95, 5, 100, 0, 50, 90, 10, 97.5, 2.5, 99, 1)                   # columns 1 .. 11 [REF :379-389]


# ------------------------------------------------------------------------------------------------
# band logic and design
# ------------------------------------------------------------------------------------------------

def band_parameters(time_between_files: float, lowcut: float, highcut: float) -> dict:
    """The reference's numbers for one band [REF create_hi_pass_viz.py:198-215]: ``fs = int(1 / dt) - 1`` (not 1 / dt),
    ``critical = int(1 / dt) / 2 - 1``, ``highcut`` clipped to it, low-pass when ``lowcut < 0.1``.  ``name`` carries the
    unclipped band, as the file names do (:105)."""
    fs = int(1 / time_between_files) - 1
    critical = int(1 / time_between_files) / 2 - 1
    name = f"{int(np.rint(lowcut))}_to_{int(np.rint(highcut))}"
    highcut = critical if highcut >= critical else highcut
    return dict(fs=fs, critical=critical, lowcut=lowcut, highcut=highcut, btype="lowpass" if lowcut < 0.1 else "bandpass",
                name=name)


def stage_refusal(time_between_files: float, lowcut: float, highcut: float) -> str:
    """Why a band cannot be a stage of a multiband cascade ('' if it can).  There the reference hands the band to scipy as it
    is [REF create_hi_pass_viz.py:193-198] - ``highcut`` is not clipped - and scipy raises unless 0 < Wn < 1."""
    nyq = 0.5 * (int(1 / time_between_files) - 1)
    if 0.0 < lowcut < highcut < nyq:
        return ""
    return (f"--hi-pass-multiband: band {lowcut:g} - {highcut:g} Hz cannot be a stage, it needs 0 < lower < upper < fs / 2 = "
            f"{nyq:g} Hz (a stage's upper frequency is not clipped)")


def design(time_between_files: float, lowcut: float, highcut: float, btype: Optional[str] = None) -> dict:
    """``band_parameters`` plus b, a [REF spectrograms.py:516-529], ``zi = lfilter_zi(b, a)`` and filtfilt's default
    ``padlen = 3 max(len(a), len(b))``.  ``btype`` "bandstop" or "bandpass": a stage of a multiband cascade - the band as it
    is (``highcut`` not clipped, no low-pass below 0.1 Hz), stopped [REF spectrograms.py:522-523] or passed (:528-529)."""
    from scipy.signal import butter, lfilter_zi
    prm = band_parameters(time_between_files, lowcut, highcut)
    nyq = 0.5 * prm["fs"]
    if btype is not None:
        if btype not in ("bandstop", "bandpass"):
            raise ValueError(f"btype must be None, 'bandstop' or 'bandpass', got {btype!r}")
        why = stage_refusal(time_between_files, lowcut, highcut)
        if why:
            raise ValueError(why)
        prm.update(highcut=highcut, btype=btype)
    low, high = prm["lowcut"] / nyq, prm["highcut"] / nyq
    if prm["btype"] == "lowpass":
        b, a = butter(ORDER, high, btype="lowpass")
    else:
        b, a = butter(ORDER, [low, high], btype=prm["btype"])
    prm.update(b=np.asarray(b, dtype=np.float64), a=np.asarray(a, dtype=np.float64), zi=np.asarray(lfilter_zi(b, a)),
               padlen=3 * max(len(a), len(b)))
    return prm


def padlen_of(lowcut: float) -> int:
    """filtfilt's padlen for the order-5 design: 18 for the low-pass (6 coefficients), 33 for the band-pass (11)."""
    return 3 * (ORDER + 1 if lowcut < 0.1 else 2 * ORDER + 1)


# ------------------------------------------------------------------------------------------------
# NumPy restatement: x is frame-major, x[frame] an array of rows of any shape
# ------------------------------------------------------------------------------------------------

def odd_ext(x: np.ndarray, n: int) -> np.ndarray:
    """scipy.signal._arraytools.odd_ext along axis 0."""
    if n < 1:
        return x
    return np.concatenate((2 * x[:1] - x[n:0:-1], x, 2 * x[-1:] - x[-2:-(n + 2):-1]), axis=0)


def lfilter_rows(b: np.ndarray, a: np.ndarray, x: np.ndarray, zi: np.ndarray) -> np.ndarray:
    """scipy.signal.lfilter(b, a, x, axis=0, zi=zi) for len(a) == len(b), a[0] == 1: the transposed direct form II of
    scipy's C loop, ``y = z[0] + b[0] x; z[k] = z[k+1] + x b[k+1] - y a[k+1]; z[-1] = x b[-1] - y a[-1]``, each line
    evaluated left to right.  zi: (len(b) - 1,) + x.shape[1:]."""
    m = len(b) - 1
    z = [np.array(zi[k], dtype=np.float64) for k in range(m)]
    y = np.empty_like(x)
    for j in range(len(x)):
        xj = x[j]
        yj = z[0] + b[0] * xj
        for k in range(m - 1):
            z[k] = z[k + 1] + xj * b[k + 1] - yj * a[k + 1]
        z[m - 1] = xj * b[m] - yj * a[m]
        y[j] = yj
    return y


def filtfilt_rows(b: np.ndarray, a: np.ndarray, x: np.ndarray, zi: Optional[np.ndarray] = None,
                  padlen: Optional[int] = None) -> np.ndarray:
    """scipy.signal.filtfilt(b, a, x, axis=0) with its defaults (padtype "odd", padlen 3 max(len(a), len(b)), method "pad")."""
    b, a = np.asarray(b, dtype=np.float64), np.asarray(a, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    if padlen is None:
        padlen = 3 * max(len(a), len(b))
    if len(x) <= padlen:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
    if zi is None:
        from scipy.signal import lfilter_zi
        zi = lfilter_zi(b, a)
    zi = np.asarray(zi, dtype=np.float64).reshape((-1,) + (1,) * (x.ndim - 1))
    ext = odd_ext(x, padlen)
    y = lfilter_rows(b, a, ext, zi * ext[0])
    y = lfilter_rows(b, a, y[::-1], zi * y[-1])[::-1]
    return np.ascontiguousarray(y[padlen:len(y) - padlen] if padlen > 0 else y)


def windowed_rms(signal_array: np.ndarray, window_size: int) -> np.ndarray:
    """calculate_windowed_rms(signal, window, "flat") [REF postprocessing_h5py_common.py:685-731] of one row:
    ``sqrt(convolve(x^2, ones(w) / w, "valid"))`` placed at ``pad = (n - len_RMS) // 2``, zero elsewhere."""
    sq = np.power(np.asarray(signal_array, dtype=np.float64), 2)
    rms = np.sqrt(np.convolve(sq, np.ones(window_size) / float(window_size), mode="valid"))
    pad = int((len(sq) - len(rms)) / 2)
    out = np.zeros(len(sq))
    out[pad:pad + len(rms)] = rms
    return out


def windowed_rms_rows(y: np.ndarray, window_size: int) -> np.ndarray:
    """``windowed_rms`` of every row of a frame-major array (direct summation, numpy's)."""
    y = np.asarray(y, dtype=np.float64)
    flat = y.reshape(len(y), -1)
    out = np.empty_like(flat)
    for r in range(flat.shape[1]):
        out[:, r] = windowed_rms(flat[:, r], window_size)
    return out.reshape(y.shape)


def windowed_rms_running(y: np.ndarray, window_size: int, refresh: int = RMS_REFRESH) -> np.ndarray:
    """The same amplitudes with the device's summation (csrc/fsi_band.hip, k_band_rms): the sum of squares of the window
    that starts at frame s is summed in order when ``s % refresh == 0`` and advanced from window s - 1 otherwise; clamped
    at zero, divided by the window, square root."""
    y = np.asarray(y, dtype=np.float64)
    n, w = len(y), int(window_size)
    out = np.zeros_like(y)
    pad = (w - 1) // 2
    acc = None
    for s in range(n - w + 1):
        if s % refresh == 0:
            acc = np.zeros_like(y[0])
            for j in range(s, s + w):
                acc = acc + y[j] * y[j]
        else:
            acc = (acc + y[s + w - 1] * y[s + w - 1]) - y[s - 1] * y[s - 1]
        out[s + pad] = np.sqrt(np.fmax(acc, 0.0) / float(w))
    return out


def amplitude_magnitude(amp: np.ndarray) -> np.ndarray:
    """rms_magnitude of one frame [REF create_hi_pass_viz.py:244,341]: ``LA.norm(., axis=1)`` of a vector's amplitudes, the
    amplitude itself for a scalar."""
    amp = np.asarray(amp, dtype=np.float64)
    if amp.ndim == 1 or amp.shape[1] == 1:
        return amp.reshape(-1).copy()
    return np.sqrt((amp[:, 0] * amp[:, 0] + amp[:, 1] * amp[:, 1]) + amp[:, 2] * amp[:, 2])


def phase_average(x: np.ndarray, period: int) -> Tuple[np.ndarray, np.ndarray]:
    """(mean, fluctuation) of whole cycles of ``period`` frames of a frame-major array, as compute_tke forms them
    [REF log_plotter.py:928-989]: ``mean[j] = (((+0.0 + x[j]) + x[period + j]) + ...) / cycles`` - the sum over the cycles in
    cycle order, then a true division - and ``fluctuation[k] = x[k] - mean[k % period]``.  What csrc/fsi_phase.hip computes."""
    x = np.asarray(x, dtype=np.float64)
    period = int(period)
    cycles = len(x) // period if period >= 1 else 0
    if period < 1 or cycles < 1 or cycles * period != len(x):
        raise RuntimeError(f"hi-pass phase: period = {period} frames, {len(x)} selected frames: needs period >= 1 and a selected "
                           "count that is a positive multiple of it")
    with np.errstate(invalid="ignore", over="ignore"):      # an inf in a row makes its mean inf and its fluctuation NaN, quietly
        s = np.zeros(x[:period].shape)
        for c in range(cycles):
            s = s + x[c * period:(c + 1) * period]
        mean = s / float(cycles)
        return mean, (x.reshape((cycles, period) + x.shape[1:]) - mean[None]).reshape(x.shape)


def fluctuation_energy(f: np.ndarray) -> np.ndarray:
    """``0.5 * ((fx fx + fy fy) + fz fz)`` per node of (..., nodes, 3) fluctuations [REF log_plotter.py:981-987]; of a scalar
    (..., nodes, 1) ``0.5 * (f f)``."""
    f = np.asarray(f, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if f.shape[-1] == 3:
            return 0.5 * ((f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2])
        if f.shape[-1] == 1:
            return 0.5 * (f[..., 0] * f[..., 0])
    raise RuntimeError("hi-pass phase_fetch: a strain / stress session has no energy: 0.5 |u'|^2 is that of a vector or a scalar")


def ordered_mean(e: np.ndarray) -> np.ndarray:
    """The sum over axis 0 in order, from +0.0, divided by the count: compute_average_over_cycles [REF log_plotter.py:902-925]
    of cycles stacked along axis 0, and ``numpy.mean(axis=0)`` of frames."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros(e.shape[1:])
        for row in e:
            s = s + row
        return s / float(len(e))


# ------------------------------------------------------------------------------------------------
# spectral power index (csrc/fsi_spi.hip)
# ------------------------------------------------------------------------------------------------

SPI_WHAT = ("rows", "nodes", "sums")            # HipBackend.SPI_WHAT, FSI_SPI_*
SPI_WINDOWS = ("boxcar", "hann")


def _rational(x):
    """A frequency or a time as a rational: an int or a Fraction as it is; a float as the closest rational with a denominator
    up to 10^12 - 0.001 is 1 / 1000, and 3 * 0.0001 = 0.00030000000000000003 is 3 / 10000, not their binary neighbours."""
    from fractions import Fraction
    if isinstance(x, (float, np.floating)):
        return Fraction(float(x)).limit_denominator(10 ** 12)
    return Fraction(x)


def spi_low_bins(n: int, time_between_files, cutoff) -> int:
    """kc, the smallest k >= 1 with ``k / (n * time_between_files) >= cutoff``: bins 1 .. kc - 1 of the length-n DFT lie below
    the cut-off, bin kc and above count as high - a cut-off that falls exactly on a bin counts that bin as high.  Decided in
    exact rational arithmetic (``_rational``).  A cut-off that is not > 0, or at or above the Nyquist frequency
    ``1 / (2 time_between_files)``, and fewer than 2 frames are refused."""
    n, dt, fc = int(n), _rational(time_between_files), _rational(cutoff)
    if n < 2:
        raise SystemExit(f"--hi-pass-spi: the window and stride asked for hold {n} frames, the index needs at least 2")
    if not fc > 0 or not dt > 0:
        raise SystemExit(f"--hi-pass-spi-cutoff must be a frequency > 0 Hz, got {cutoff!r}")
    if fc * 2 * dt >= 1:
        raise SystemExit(f"--hi-pass-spi-cutoff {float(fc):g} Hz is at or above the Nyquist frequency {float(1 / (2 * dt)):g} Hz of frames "
                         f"{float(dt)!r} s apart (dt * save_step * stride): no power lies above it")
    x = fc * n * dt                                 # the cut-off in bins
    kc = x.numerator // x.denominator + (1 if x.numerator % x.denominator else 0)
    return max(1, kc)


def spi_sums(x: np.ndarray, window, bin0: int, nb: int, mean: Optional[np.ndarray] = None):
    """(L2, X0sq, Q, mean) of frame-major x (n, ...) for the bins bin0 .. bin0 + nb - 1 of the length-n DFT: with the ordered
    mean m, ``Y[j] = window[j] (x[j] - m)`` (window None: the boxcar) and ``X_k = sum_j Y[j] exp(-2 pi i j k / n)``:
    ``L2 = sum |X_k|^2`` over the slab's bins k >= 1 in bin order, ``X0sq = |X_0|^2`` (zeros unless the slab holds bin 0),
    ``Q = sum_j Y[j]^2`` in frame order.  What k_spi_power forms, but for the order inside a sum."""
    from .spectrogram import spec_tables
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    with np.errstate(invalid="ignore", over="ignore"):
        if mean is None:
            mean = np.zeros(x.shape[1:])
            for j in range(n):
                mean = mean + x[j]
            mean = mean / float(n)
        y = x - mean[None]
        if window is not None:
            y = np.asarray(window, dtype=np.float64).reshape((n,) + (1,) * (x.ndim - 1)) * y
        flat = y.reshape(n, -1)
        bad = ~np.isfinite(flat).all(axis=0)        # a NaN stays in its row: BLAS is kept away from it
        C, S = spec_tables(n, n, bin0, nb)
        safe = np.where(bad[None], 0.0, flat)
        re, im = C @ safe, S @ safe
        P = re * re + im * im
        P[:, bad] = np.nan
        L2, X0 = np.zeros(flat.shape[1]), np.zeros(flat.shape[1])
        for b in range(nb):
            if bin0 + b == 0:
                X0 = P[b]
            else:
                L2 = L2 + P[b]
        Q = np.zeros(flat.shape[1])
        for j in range(n):
            Q = Q + flat[j] * flat[j]
    shape = x.shape[1:]
    return L2.reshape(shape), X0.reshape(shape), Q.reshape(shape), mean


def spi_close(L2: np.ndarray, X0sq: np.ndarray, Q: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """(H, AC): ``AC = n Q - X0sq``, all power but bin 0, two-sided, by Parseval; ``H = AC - 2 L2``, what lies at or above the
    cut-off."""
    with np.errstate(invalid="ignore", over="ignore"):
        AC = float(n) * np.asarray(Q) - np.asarray(X0sq)
        return AC - 2.0 * np.asarray(L2), AC


def spi_ratio(H: np.ndarray, AC: np.ndarray) -> np.ndarray:
    """``H <= 0 ? 0 : H / AC``: an exactly constant row (AC == 0) gives 0, a NaN stays NaN."""
    H, AC = np.asarray(H, dtype=np.float64), np.asarray(AC, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(H <= 0.0, 0.0, H / np.where(H <= 0.0, 1.0, AC))


def spi_node_ratio(H: np.ndarray, AC: np.ndarray) -> np.ndarray:
    """The index per node of (nodes, ncomp) H and AC: of a vector that of the summed power, ``(H_x + H_y) + H_z`` over
    ``(AC_x + AC_y) + AC_z`` - invariant under a rotation of the axes -, of a scalar the row's."""
    H, AC = np.asarray(H, dtype=np.float64), np.asarray(AC, dtype=np.float64)
    if H.ndim < 2 or H.shape[-1] == 1:
        return spi_ratio(H.reshape(H.shape[0]), AC.reshape(H.shape[0]))
    if H.shape[-1] != 3:
        raise RuntimeError("hi-pass spi: a strain / stress session has no spectral power index: it is that of a vector or a scalar (d, v, p)")
    with np.errstate(invalid="ignore", over="ignore"):
        return spi_ratio((H[..., 0] + H[..., 1]) + H[..., 2], (AC[..., 0] + AC[..., 1]) + AC[..., 2])


def spi_rows(x: np.ndarray, window, kc: int) -> np.ndarray:
    """The spectral power index of every row of frame-major x (n, ...): the fraction of the one-sided power of bins >= 1 that
    lies in the bins >= kc, ``sum_{k >= kc} P_k / sum_{k >= 1} P_k``, formed from the kc lowest bins alone (``spi_sums``,
    ``spi_close``)."""
    L2, X0, Q, _ = spi_sums(x, window, 0, int(kc))
    return spi_ratio(*spi_close(L2, X0, Q, len(x)))


def spi_nodes(x: np.ndarray, window, kc: int) -> np.ndarray:
    """``spi_node_ratio`` of frame-major x (n, nodes, ncomp): (nodes,)."""
    L2, X0, Q, _ = spi_sums(x, window, 0, int(kc))
    return spi_node_ratio(*spi_close(L2, X0, Q, len(x)))


# ------------------------------------------------------------------------------------------------
# snapshot proper orthogonal decomposition (csrc/fsi_pod.hip)
# ------------------------------------------------------------------------------------------------

POD_WHAT = ("gram", "mean", "mode")             # HipBackend.POD_WHAT, FSI_POD_*
POD_SERIES = ("raw", "series")                  # FSI_RATE_RAW, FSI_RATE_SERIES
POD_WEIGHTS = ("volume", "uniform")
POD_SLAB = 6144                                 # rows of a slab of the Gram matrix's row sum (csrc/fsi_pod.hpp)
POD_MAX_MODES = 64


def _pod_weights(weights, x: np.ndarray):
    """None, or the weight of every node shaped to multiply a frame of x (n, nodes, ...): refused if one is negative or not
    finite, naming the first such node."""
    if weights is None:
        return None
    w = np.array(weights, dtype=np.float64).reshape(-1)
    if len(w) != x.shape[1]:
        raise ValueError(f"{len(w)} weights, the frames have {x.shape[1]} nodes")
    bad = np.flatnonzero(~(np.isfinite(w) & (w >= 0)))
    if len(bad):
        raise RuntimeError(f"hi-pass pod_gram: the weight of node {bad[0]} is {w[bad[0]]:g}: a weight is >= 0 and finite")
    return w.reshape((len(w),) + (1,) * (x.ndim - 2))


def pod_gram(x: np.ndarray, weights=None) -> Tuple[np.ndarray, np.ndarray]:
    """``(G, mean)`` of frame-major x (n, nodes, ...): with m the ordered mean over the frames, ``y_j = x_j - m`` and
    ``a_j = w y_j`` rounded once (``weights`` one value >= 0 per node; None: ``a_j`` is ``y_j`` itself),
    ``G[i][j] = sum_r a_i[r] y_j[r]`` over the rows r (node, component).  The rows are added in slabs of ``POD_SLAB``, the
    slabs in ascending order from +0.0; only ``i <= j`` is formed and mirrored, so G is symmetric bit for bit.  What
    k_pod_gram and k_pod_gram_close form, but for the order inside a slab.  A sum over the rows: unlike the spectral power
    index, where a NaN stays in its row, one NaN or inf poisons every entry."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    w = _pod_weights(weights, x)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = np.zeros(x.shape[1:])
        for j in range(n):
            mean = mean + x[j]
        mean = mean / float(n)
        y = x - mean[None]
        a = y if w is None else w[None] * y
        y, a = y.reshape(n, -1), a.reshape(n, -1)
        G = np.zeros((n, n))
        for r0 in range(0, y.shape[1], POD_SLAB):       # a copy: numpy hands a @ a.T of one array to another BLAS routine, with other bits
            G = G + np.array(a[:, r0:r0 + POD_SLAB]) @ y[:, r0:r0 + POD_SLAB].T
    G = np.triu(G)
    return G + np.triu(G, 1).T, mean


def pod_floor(rows: int, trace: float) -> float:
    """``(rows + 2) * 2^-53 * trace``: below it an eigenvalue of the computed Gram matrix is rounding (``pod_eig``)."""
    return (int(rows) + 2) * 2.0 ** -53 * float(trace)


def pod_eig(G: np.ndarray, rows: int, modes: int) -> dict:
    """The eigen step of the snapshot POD, the one of the device path and of the twin: ``G V = V diag(lam)`` by
    ``numpy.linalg.eigh`` with lam descending and, in each column of V, the entry of largest magnitude positive (on a tie the
    first such entry decides).  ``sigma = sqrt(lam)``, ``trace`` the ordered sum of G's diagonal from +0.0.

    The resolution floor.  G is a sum over ``rows`` rows, ``G_ij = sum_r a_i[r] y_j[r]``.  With u = 2^-53 the computed entry is
    off by at most ``(rows + 2) u sum_r |a_i[r] y_j[r]|`` (one rounding each for the product and for a = w y, rows for the
    additions, to first order); by Cauchy-Schwarz in the w inner product that is ``<= (rows + 2) u sqrt(G_ii G_jj)``, so
    ``||dG||_F <= (rows + 2) u sqrt(sum_ij G_ii G_jj) = (rows + 2) u trace``.  By Weyl's inequality every eigenvalue of the
    computed G lies within ``||dG||_2 <= ||dG||_F`` of the exact one: mode m is **resolved** iff
    ``lam_m > (rows + 2) * 2^-53 * trace`` - derived, not measured.  An unresolved mode is neither formed nor written.

    Returns the leading ``min(modes, n)`` modes: ``lam``, ``V`` (n, M), ``sigma`` (0 where lam < 0), ``resolved``, ``fraction``
    ``lam / trace``; ``trace``, ``floor``; ``spectrum`` every eigenvalue.  Raises on a G that is not finite: a Gram matrix sums
    over the rows, so one recorded NaN or inf makes every entry non-finite."""
    G = np.asarray(G, dtype=np.float64)
    n = len(G)
    if G.shape != (n, n) or n < 2:
        raise ValueError(f"pod_eig: G must be (n, n) with n >= 2, got {G.shape}")
    if not np.isfinite(G).all():
        raise RuntimeError("hi-pass pod: the Gram matrix is not finite: a recorded value is NaN or inf (the matrix sums over the "
                           "rows, so one such value reaches every entry)")
    lam, V = np.linalg.eigh(G)
    lam, V = lam[::-1].copy(), V[:, ::-1].copy()
    for m in range(n):
        if V[np.argmax(np.abs(V[:, m])), m] < 0:      # argmax: the first of equal magnitudes
            V[:, m] = -V[:, m]
    trace = 0.0
    for k in range(n):
        trace = trace + float(G[k, k])
    M = max(1, min(int(modes), n))
    floor = pod_floor(rows, trace)
    with np.errstate(invalid="ignore", divide="ignore"):
        fraction = lam[:M] / trace if trace > 0 else np.zeros(M)
    return dict(lam=lam[:M], V=V[:, :M], sigma=np.sqrt(np.maximum(lam[:M], 0.0)), resolved=lam[:M] > floor, fraction=fraction,
                trace=trace, floor=floor, spectrum=lam)


def pod_table(eig: dict) -> np.ndarray:
    """``T[j][m] = V[j][m] / sigma_m`` for the resolved modes of ``pod_eig``, (n, resolved): ``Phi_m = sum_j T[j][m] y_j`` are
    orthonormal in the w inner product, ``Phi_a^T W Phi_b = V_a^T G V_b / (sigma_a sigma_b)``."""
    K = int(np.count_nonzero(eig["resolved"]))
    return np.ascontiguousarray(eig["V"][:, :K] / eig["sigma"][None, :K])


def pod_coefficients(eig: dict) -> np.ndarray:
    """``a_m(j) = sigma_m V[j][m]``, (n, M): ``y_j = sum_m a_m(j) Phi_m``."""
    return eig["V"] * eig["sigma"][None]


def pod_modes(x: np.ndarray, mean: np.ndarray, T: np.ndarray) -> np.ndarray:
    """``Phi_m = sum_j T[j][m] (x_j - mean)`` of frame-major x (n, ...): (modes, ...).  What k_pod_modes forms, but for the order
    inside a sum."""
    x, T = np.asarray(x, dtype=np.float64), np.asarray(T, dtype=np.float64)
    n = len(x)
    if T.ndim != 2 or T.shape[0] != n:
        raise ValueError(f"the table must be (frames, modes) = ({n}, modes), got {T.shape}")
    with np.errstate(invalid="ignore", over="ignore"):
        y = (x - np.asarray(mean)[None]).reshape(n, -1)
        return (T.T @ y).reshape((T.shape[1],) + x.shape[1:])


def pod_volume_weights(mesh, save_deg: int) -> np.ndarray:
    """One weight per written node (``output_nodes``), summed over the cells of the mesh - every quantity of ``--hi-pass`` is
    written on all of it.  ``save_deg`` 2: a cell of volume |K| gives |K| / 32 to each vertex and 7 |K| / 48 to each edge
    midpoint - the P1 lumping of the once-refined cell: a corner tetrahedron of volume |K| / 8 gives a quarter of it to its
    vertex and to each of its three midpoints, and the inner octahedron of volume |K| / 2 is shared equally by its six
    midpoints, so that the weights do not depend on the diagonal it is cut along; 4 / 32 + 6 * 7 / 48 = 1.  ``save_deg`` 1:
    |K| / 4 to each vertex."""
    xk = mesh.coords[mesh.tets]
    vol = np.abs(np.einsum("ij,ij->i", xk[:, 1] - xk[:, 0], np.cross(xk[:, 2] - xk[:, 0], xk[:, 3] - xk[:, 0]))) / 6.0
    if save_deg < 2:
        w = np.zeros(mesh.num_vertices)
        np.add.at(w, mesh.tets, (vol / 4.0)[:, None])
        return w
    w = np.zeros(mesh.num_nodes)
    np.add.at(w, mesh.tet_nodes[:, :4], (vol / 32.0)[:, None])
    np.add.at(w, mesh.tet_nodes[:, 4:], (7.0 * vol / 48.0)[:, None])
    return w


RATE_SERIES = ("raw", "series", "phase_mean")      # HipBackend.RATE_SERIES, FSI_RATE_*


def cell_rate(w: np.ndarray, grad: np.ndarray) -> np.ndarray:
    """The exact mean over a tetrahedron of ``2 S:S``, ``S = sym(grad w)``, of P2 fields w, (cells, 10, 3) in the local node
    order (``mesh.TET_EDGES``), with ``grad`` (cells, 4, 3) the gradients of the barycentric coordinates: the arithmetic of
    k_cell_rate (csrc/fsi_rate.hip) in its order, one IEEE operation per NumPy operation.  ``G_t = grad w`` at vertex t
    (``vertex_gradients``), ``S_t = 0.5 (G_t + G_t^T)`` and
    ``0.1 * (sum_t S_t:S_t + (sum_t S_t):(sum_t S_t))``, since ``int L_a L_b = |K| (1 + delta_ab) / 20``."""
    w, g = np.asarray(w, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    if w.ndim != 3 or w.shape[1:] != (10, 3) or g.shape != (len(w), 4, 3):
        raise RuntimeError(f"cell_rate: w of shape {w.shape} and grad of shape {g.shape}, expected (n, 10, 3) and (n, 4, 3)")
    n = len(w)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.zeros(n)
        T = [[np.zeros(n) for _ in range(3)] for _ in range(3)]
        for G in vertex_gradients(w, g):
            for i in range(3):
                for j in range(3):
                    S = 0.5 * (G[i][j] + G[j][i])
                    q = q + S * S
                    T[i][j] = T[i][j] + S
        p = np.zeros(n)
        for i in range(3):
            for j in range(3):
                p = p + T[i][j] * T[i][j]
        return 0.1 * (q + p)


RULE_A, RULE_B = 0.5854101966249685, 0.1381966011250105      # the degree-2 interior rule of the tetrahedron: on vertex q, on the others


def vertex_gradients(w: np.ndarray, g: np.ndarray) -> list:
    """``G[t][i][j]``, (cells,) each: the gradient of P2 fields w (cells, 10, 3) at vertex t, ``g`` (cells, 4, 3) the gradients
    of the barycentric coordinates - it is linear on the cell, so the four vertices determine it.  The arithmetic of
    vertex_gradient_of (csrc/fsi_cell.hpp) in its order: the one expression ``cell_rate``, ``cell_rate_current`` and
    ``cell_vortex`` share, as their kernels do.  (wss_dg1_cell, csrc/fsi_wss.hpp, has the same expression compiled with
    contraction; it is no twin of this.)"""
    from .mesh import TET_EDGES
    n = len(w)
    G = [[[None] * 3 for _ in range(3)] for _ in range(4)]
    for t in range(4):
        for i in range(3):
            for j in range(3):
                s = np.zeros(n)
                for a in range(4):
                    s = s + w[:, a, i] * ((3.0 if a == t else -1.0) * g[:, a, j])
                for e in range(6):
                    p, r = int(TET_EDGES[e][0]), int(TET_EDGES[e][1])
                    s = s + (w[:, 4 + e, i] * 4.0) * ((1.0 if p == t else 0.0) * g[:, r, j] + (1.0 if r == t else 0.0) * g[:, p, j])
                G[t][i][j] = s
    return G


def cell_rate_current(v: np.ndarray, d: np.ndarray, grad: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(rate, volume_ratio, min_jacobian)`` of one frame, (cells,) each: the mean of ``2 S:S`` over the **deformed** cell,
    ``S = sym(grad_X v F^-1)``, ``F = I + grad_X d``, of P2 fields v on the mesh ``x = X + d(X)`` - v and d (cells, 10, 3) in
    the local node order, ``grad`` (cells, 4, 3) the gradients of the barycentric coordinates of the undeformed cells; the
    deformed cell's volume over the undeformed; the smallest ``det F`` at the rule's points.  The arithmetic of
    k_cell_rate_current (csrc/fsi_rate.hip) in its order, one IEEE operation per NumPy operation.

    With ``G_t``, ``D_t`` the vertex gradients of v and d: at the four points of the degree-2 interior rule (``RULE_A`` on
    vertex q, ``RULE_B`` on the others) ``G_q = b (sum_t G_t) + (a - b) G_q`` - exact, the gradient being linear on the cell -
    and ``D_q`` likewise; ``F_q = I + D_q``, ``J_q = det F_q``, ``L_q = G_q adj(F_q) / J_q``, ``S_q = 0.5 (L_q + L_q^T)``,
    ``e_q = 2 S_q:S_q``; ``rate = (sum_q J_q e_q) / (sum_q J_q)``, ``volume_ratio = 0.25 sum_q J_q`` and ``min_jacobian``
    from +inf by ``m = J_q if J_q < m else m``, which a NaN never replaces.  With d = 0 the integrand is quadratic, the rule
    exact and ``rate`` is ``cell_rate`` to rounding.  Nothing is clamped: ``J_q = 0`` gives inf or NaN, a negative ``J_q`` is
    carried through."""
    v, d, g = np.asarray(v, dtype=np.float64), np.asarray(d, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    if v.ndim != 3 or v.shape[1:] != (10, 3) or d.shape != v.shape or g.shape != (len(v), 4, 3):
        raise RuntimeError(f"cell_rate_current: v of shape {v.shape}, d of shape {d.shape} and grad of shape {g.shape}, expected (n, 10, 3) "
                           "twice and (n, 4, 3)")
    n = len(v)
    qab = RULE_A - RULE_B
    with np.errstate(all="ignore"):
        D, G = vertex_gradients(d, g), vertex_gradients(v, g)
        TG, TD = [[None] * 3 for _ in range(3)], [[None] * 3 for _ in range(3)]
        for T, X in ((TG, G), (TD, D)):
            for i in range(3):
                for j in range(3):
                    s = np.zeros(n)
                    for t in range(4):
                        s = s + X[t][i][j]
                    T[i][j] = s
        num, den, m = np.zeros(n), np.zeros(n), np.full(n, np.inf)
        for q in range(4):
            gq, F = [[None] * 3 for _ in range(3)], [[None] * 3 for _ in range(3)]
            for i in range(3):
                for j in range(3):
                    gq[i][j] = RULE_B * TG[i][j] + qab * G[q][i][j]
                    dq = RULE_B * TD[i][j] + qab * D[q][i][j]
                    F[i][j] = 1.0 + dq if i == j else dq
            A = [[F[1][1] * F[2][2] - F[1][2] * F[2][1], F[0][2] * F[2][1] - F[0][1] * F[2][2], F[0][1] * F[1][2] - F[0][2] * F[1][1]],
                 [F[1][2] * F[2][0] - F[1][0] * F[2][2], F[0][0] * F[2][2] - F[0][2] * F[2][0], F[0][2] * F[1][0] - F[0][0] * F[1][2]],
                 [F[1][0] * F[2][1] - F[1][1] * F[2][0], F[0][1] * F[2][0] - F[0][0] * F[2][1], F[0][0] * F[1][1] - F[0][1] * F[1][0]]]
            J = (F[0][0] * A[0][0] + F[0][1] * A[1][0]) + F[0][2] * A[2][0]
            L = [[((gq[i][0] * A[0][j] + gq[i][1] * A[1][j]) + gq[i][2] * A[2][j]) / J for j in range(3)] for i in range(3)]
            e = np.zeros(n)
            for i in range(3):
                for j in range(3):
                    S = 0.5 * (L[i][j] + L[j][i])
                    e = e + S * S
            num = num + J * (2.0 * e)
            den = den + J
            m = np.where(J < m, J, m)
        return num / den, 0.25 * den, m


VORTEX_FIELDS = ("Q", "enstrophy", "helicity", "abs_helicity", "speed2")      # HipBackend.VORTEX_FIELDS, FSI_VORTEX_*


def vortex_tables() -> Tuple[np.ndarray, np.ndarray]:
    """``(60 M, 420 MM)`` in integers, (10, 4) and (10, 10), local node order.  ``M[a][t]``: the mean over the cell of P2 basis
    function a times barycentric coordinate t - vertex a: 0 at t == a, else -1; edge {p, r}: 4 at t in {p, r}, else 2.
    ``MM``: the P2 mass matrix over the volume - vertex-vertex 6 and 1; vertex-edge -4 if the vertex is an end of the edge,
    else -6; edge-edge 32, 16 if they share a vertex, 8 if they are opposite.  Both from
    ``mean(prod L_i^alpha_i) = 6 prod alpha_i! / (|alpha| + 3)!``."""
    from .mesh import TET_EDGES
    ends = [{a} for a in range(4)] + [{int(p), int(r)} for p, r in TET_EDGES]
    M = np.array([[(0 if a == t else -1) if a < 4 else (4 if t in ends[a] else 2) for t in range(4)] for a in range(10)])
    MM = np.empty((10, 10), dtype=np.int64)
    for a in range(10):
        for b in range(10):
            if a < 4 and b < 4:
                MM[a, b] = 6 if a == b else 1
            elif a < 4 or b < 4:
                MM[a, b] = -4 if ends[min(a, b)] <= ends[max(a, b)] else -6
            else:
                MM[a, b] = 32 if a == b else 16 if ends[a] & ends[b] else 8
    return M, MM


VORTEX_M = vortex_tables()[0] / 60.0         # one true division each: the constants of csrc/fsi_vortex.hip
VORTEX_MM = vortex_tables()[1] / 420.0


def cell_vortex(w: np.ndarray, grad: np.ndarray) -> np.ndarray:
    """(5, cells), the rows ``VORTEX_FIELDS``: exact means over a tetrahedron of P2 fields w, (cells, 10, 3) in the local node
    order (``mesh.TET_EDGES``), with ``grad`` (cells, 4, 3) the gradients of the barycentric coordinates - the arithmetic of
    k_cell_vortex (csrc/fsi_vortex.hip) in its order, one IEEE operation per NumPy operation.

    With ``G_t = grad w`` at vertex t (``vertex_gradients``), ``T = sum_t G_t`` and
    ``omega_t = (G_t[2][1] - G_t[1][2], G_t[0][2] - G_t[2][0], G_t[1][0] - G_t[0][1])``: the gradient is linear on the cell, so
    the mean of a product of two of its entries is ``0.05 (sum_t f_t h_t + (sum_t f_t)(sum_t h_t))``, and

        Q             -0.5 sum_ij mean(G_ij G_ji) = 0.5 (|Omega|^2 - |S|^2)
        enstrophy     mean(|omega|^2)
        helicity      mean(w . omega) = sum_t sum_i (sum_a M[a][t] w[a][i]) omega_t[i]            (``VORTEX_M``)
        abs_helicity  |helicity|: the absolute value of the cell mean, **not** the cell mean of |w . omega|
        speed2        mean(|w|^2) = sum_i sum_a w[a][i] (sum_b MM[a][b] w[b][i])                  (``VORTEX_MM``)

    Nothing is clamped; NaN and inf propagate."""
    w, g = np.asarray(w, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    if w.ndim != 3 or w.shape[1:] != (10, 3) or g.shape != (len(w), 4, 3):
        raise RuntimeError(f"cell_vortex: w of shape {w.shape} and grad of shape {g.shape}, expected (n, 10, 3) and (n, 4, 3)")
    n = len(w)
    with np.errstate(all="ignore"):
        Gs = vertex_gradients(w, g)
        qd, ed, h = np.zeros(n), np.zeros(n), np.zeros(n)
        T = [[np.zeros(n) for _ in range(3)] for _ in range(3)]
        for t in range(4):
            G = Gs[t]
            for i in range(3):
                for j in range(3):
                    qd = qd + G[i][j] * G[j][i]
                    T[i][j] = T[i][j] + G[i][j]
            om = [G[2][1] - G[1][2], G[0][2] - G[2][0], G[1][0] - G[0][1]]
            for i in range(3):
                ed = ed + om[i] * om[i]
            for i in range(3):
                u = np.zeros(n)
                for a in range(10):
                    u = u + VORTEX_M[a][t] * w[:, a, i]
                h = h + u * om[i]
        qp = np.zeros(n)
        for i in range(3):
            for j in range(3):
                qp = qp + T[i][j] * T[j][i]
        W = [T[2][1] - T[1][2], T[0][2] - T[2][0], T[1][0] - T[0][1]]
        ep = np.zeros(n)
        for i in range(3):
            ep = ep + W[i] * W[i]
        s2 = np.zeros(n)
        for i in range(3):
            for a in range(10):
                u = np.zeros(n)
                for b in range(10):
                    u = u + VORTEX_MM[a][b] * w[:, b, i]
                s2 = s2 + w[:, a, i] * u
        return np.stack([-0.5 * (0.05 * (qd + qp)), 0.05 * (ed + ep), h, np.abs(h), s2])


VORTEX_CURRENT_FIELDS = VORTEX_FIELDS + ("volume_ratio",)      # HipBackend.VORTEX_CURRENT_FIELDS, FSI_VORTEX_* and FSI_VORTEX_VOLUME_RATIO

# The 14-point positive interior rule of degree 5 on the tetrahedron (the constants of csrc/fsi_vortex.hip): 1 - 3 a on one
# vertex and a on the others for a = A1 (weight W1) and a = A2 (W2), 0.5 - B on the two ends of an edge and B on the other two (W3)
VORTEX_RULE_A1, VORTEX_RULE_W1 = 0.31088591926330060980, 0.11268792571801585080
VORTEX_RULE_A2, VORTEX_RULE_W2 = 0.092735250310891226402, 0.073493043116361949544
VORTEX_RULE_B, VORTEX_RULE_W3 = 0.045503704125649649492, 0.042546020777081466438


def vortex_rule() -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(lam, om, basis)``: (14, 4) barycentrics, (14,) weights and (14, 10) values of the P2 basis at the points, local node
    order - ``lam_a (2 lam_a - 1)`` at a vertex, ``(4 lam_r) lam_s`` on the edge {r, s} -, each entry by the operations that
    form it in RuleTable (csrc/fsi_vortex.hip)."""
    from .mesh import TET_EDGES
    edges = [(int(r), int(s)) for r, s in TET_EDGES]
    lam, om, basis = np.empty((14, 4)), np.empty(14), np.empty((14, 10))
    for p in range(14):
        for t in range(4):
            if p < 4:
                lam[p, t] = 1.0 - 3.0 * VORTEX_RULE_A1 if t == p else VORTEX_RULE_A1
            elif p < 8:
                lam[p, t] = 1.0 - 3.0 * VORTEX_RULE_A2 if t == p - 4 else VORTEX_RULE_A2
            else:
                lam[p, t] = 0.5 - VORTEX_RULE_B if t in edges[p - 8] else VORTEX_RULE_B
        om[p] = VORTEX_RULE_W1 if p < 4 else VORTEX_RULE_W2 if p < 8 else VORTEX_RULE_W3
        for a in range(4):
            basis[p, a] = lam[p, a] * (2.0 * lam[p, a] - 1.0)
        for e, (r, s) in enumerate(edges):
            basis[p, 4 + e] = (4.0 * lam[p, r]) * lam[p, s]
    return lam, om, basis


VORTEX_RULE_LAM, VORTEX_RULE_OM, VORTEX_RULE_BASIS = vortex_rule()


def cell_vortex_current(w: np.ndarray, d: np.ndarray, grad: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``(means, numerators)`` of one frame, (6, cells) each, the rows ``VORTEX_CURRENT_FIELDS``: ``cell_vortex`` on the mesh
    ``x = X + d(X)`` - w and d (cells, 10, 3) P2 fields in the local node order, ``grad`` (cells, 4, 3) the gradients of the
    barycentric coordinates of the **undeformed** cells.  The arithmetic of k_cell_vortex_current (csrc/fsi_vortex.hip) in its
    order, one IEEE operation per NumPy operation.

    With ``G_t``, ``D_t`` the vertex gradients of w and d, at the 14 points p of the degree-5 rule (``vortex_rule``):
    ``G_p = ((lam_0 G_0 + lam_1 G_1) + lam_2 G_2) + lam_3 G_3`` - exact, the gradient being linear on the cell - and ``D_p``
    likewise; ``F_p = I + D_p``, ``A_p = adj F_p``, ``J_p = det F_p``, ``L_p = (G_p A_p) * (1 / J_p)``,
    ``v_p = sum_a N_a(lam_p) w[a]``, ``omega_p`` the axial vector of ``L_p - L_p^T``, and

        f_0 = -0.5 sum_ij L_ij L_ji      f_1 = |omega_p|^2      f_2 = v_p . omega_p      f_4 = |v_p|^2

    ``Jbar = sum_p om_p J_p`` is the deformed cell's volume over the undeformed, exact for a P2 displacement; the numerators
    ``n_f = sum_p (om_p J_p) f_p`` and ``n_3 = |n_2|`` are integrals over the deformed cell per undeformed volume, the means
    ``r_f = n_f / Jbar`` and ``r_3 = |r_2|`` those over the deformed cell; row 5 of both is ``Jbar``.  With d = 0 every
    integrand is of degree <= 4, the rule exact and the means are ``cell_vortex`` to rounding.  Nothing is clamped: ``J_p = 0``
    gives inf or NaN, a negative ``J_p`` is carried through."""
    w, d, g = np.asarray(w, dtype=np.float64), np.asarray(d, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    if w.ndim != 3 or w.shape[1:] != (10, 3) or d.shape != w.shape or g.shape != (len(w), 4, 3):
        raise RuntimeError(f"cell_vortex_current: w of shape {w.shape}, d of shape {d.shape} and grad of shape {g.shape}, expected (n, 10, 3) "
                           "twice and (n, 4, 3)")
    n = len(w)
    with np.errstate(all="ignore"):
        D, G = vertex_gradients(d, g), vertex_gradients(w, g)
        n0, n1, n2, n4, jb = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        for p in range(14):
            l0, l1, l2, l3 = (float(x) for x in VORTEX_RULE_LAM[p])
            gp, F = [[None] * 3 for _ in range(3)], [[None] * 3 for _ in range(3)]
            for i in range(3):
                for j in range(3):
                    gp[i][j] = ((l0 * G[0][i][j] + l1 * G[1][i][j]) + l2 * G[2][i][j]) + l3 * G[3][i][j]
                    dp = ((l0 * D[0][i][j] + l1 * D[1][i][j]) + l2 * D[2][i][j]) + l3 * D[3][i][j]
                    F[i][j] = 1.0 + dp if i == j else dp
            A = [[F[1][1] * F[2][2] - F[1][2] * F[2][1], F[0][2] * F[2][1] - F[0][1] * F[2][2], F[0][1] * F[1][2] - F[0][2] * F[1][1]],
                 [F[1][2] * F[2][0] - F[1][0] * F[2][2], F[0][0] * F[2][2] - F[0][2] * F[2][0], F[0][2] * F[1][0] - F[0][0] * F[1][2]],
                 [F[1][0] * F[2][1] - F[1][1] * F[2][0], F[0][1] * F[2][0] - F[0][0] * F[2][1], F[0][0] * F[1][1] - F[0][1] * F[1][0]]]
            J = (F[0][0] * A[0][0] + F[0][1] * A[1][0]) + F[0][2] * A[2][0]
            rJ = 1.0 / J
            L = [[((gp[i][0] * A[0][j] + gp[i][1] * A[1][j]) + gp[i][2] * A[2][j]) * rJ for j in range(3)] for i in range(3)]
            q = np.zeros(n)
            for i in range(3):
                for j in range(3):
                    q = q + L[i][j] * L[j][i]
            om = [L[2][1] - L[1][2], L[0][2] - L[2][0], L[1][0] - L[0][1]]
            e, h, s2 = np.zeros(n), np.zeros(n), np.zeros(n)
            for i in range(3):
                e = e + om[i] * om[i]
            for i in range(3):
                v = np.zeros(n)
                for a in range(10):
                    v = v + float(VORTEX_RULE_BASIS[p][a]) * w[:, a, i]
                h = h + v * om[i]
                s2 = s2 + v * v
            wj = float(VORTEX_RULE_OM[p]) * J
            jb = jb + wj
            n0 = n0 + wj * (-0.5 * q)
            n1 = n1 + wj * e
            n2 = n2 + wj * h
            n4 = n4 + wj * s2
        r2 = n2 / jb
        return np.stack([n0 / jb, n1 / jb, r2, np.abs(r2), n4 / jb, jb]), np.stack([n0, n1, n2, np.abs(n2), n4, jb])


def cell_wsum(values: np.ndarray, weights: np.ndarray) -> np.ndarray:
    """``sum_c weights[c] * values[..., c]`` in the bracket of k_cell_wsum and k_cell_wsum_close (csrc/fsi_vortex.hip):
    ``p_c = weights[c] * values[c]``, one rounding; the cells in groups of 256 consecutive ones, +0.0 past the last; inside
    each 64 of a group a balanced tree over adjacent pairs (strides 1, 2, 4, 8, 16, 32); the group's four sums of 64 as
    ``((s0 + s1) + s2) + s3``; the groups from +0.0 in ascending order.  ``values`` (n,) gives a scalar array, (k, n) gives (k,)."""
    v, wt = np.asarray(values, dtype=np.float64), np.asarray(weights, dtype=np.float64).reshape(-1)
    if v.ndim not in (1, 2) or v.shape[-1] != len(wt) or len(wt) < 1:
        raise RuntimeError(f"cell_wsum: values of shape {v.shape} and {len(wt)} weights, expected (n,) or (k, n) and n > 0 weights")
    with np.errstate(all="ignore"):
        p = np.atleast_2d(wt * v)
        k, n = p.shape
        groups = (n + 255) // 256
        x = np.zeros((k, groups * 256))
        x[:, :n] = p
        x = x.reshape(k, groups, 4, 64)
        for _ in range(6):
            x = x[..., 0::2] + x[..., 1::2]
        x = x[..., 0]
        part = ((x[..., 0] + x[..., 1]) + x[..., 2]) + x[..., 3]
        s = np.zeros(k)
        for b in range(groups):
            s = s + part[:, b]
        return s[0] if v.ndim == 1 else s


def pass_stop_list(band_list, words=None) -> List[str]:
    """"pass" or "stop" per band of a multiband cascade: the reference's rule - a band wider than 1000 Hz passes, a narrower
    one is stopped [REF create_hi_pass_viz.py:541-545] - or the words given (``--hi-pass-pass-stop``)."""
    if words is None:
        return ["pass" if hi - lo > 1000 else "stop" for lo, hi in band_list]
    words = [words] if isinstance(words, str) else [str(w) for w in words]
    if len(words) != len(band_list):
        raise SystemExit(f"--hi-pass-pass-stop takes one word per band: {len(words)} words for {len(band_list)} bands")
    bad = [w for w in words if w not in ("pass", "stop")]
    if bad:
        raise SystemExit(f"--hi-pass-pass-stop takes the words pass and stop, got {bad}")
    return words


def multiband_name(viz_type: str, band_list, words) -> str:
    """The reference's chained file name [REF create_hi_pass_viz.py:102-103]."""
    for (lo, hi), word in zip(band_list, words):
        viz_type = f"{viz_type}_{word}_{int(np.rint(lo))}_to_{int(np.rint(hi))}"
    return viz_type


class HostHistory:
    """The recording half of a host session: the raw frames, up to the capacity declared at begin, and their filtfilt."""
    what = ""

    def __init__(self, shape, capacity: int):
        self.shape, self.capacity = shape, int(capacity)
        self.raw: List[np.ndarray] = []
        self.filtered = None

    def sample(self, frame: np.ndarray) -> None:
        if len(self.raw) >= self.capacity:
            raise RuntimeError(f"{self.what} history is full (capacity declared at begin)")
        self.raw.append(np.array(frame, dtype=np.float64).reshape(self.shape))
        self.filtered = None

    def filter(self, b=None, a=None, zi=None, padlen: int = 0) -> None:
        self.filtered = None if b is None else filtfilt_rows(b, a, np.stack(self.raw), zi, padlen)

    def export(self, first: int, count: int) -> np.ndarray:
        """Raw frames ``first .. first + count - 1``, frame-major: what ``HipBackend.<prefix>_export`` returns."""
        if first < 0 or count < 1 or first + count > len(self.raw):
            raise RuntimeError(f"{self.what} export: needs first >= 0, count >= 1 and first + count <= the {len(self.raw)} recorded frames")
        return np.stack(self.raw[first:first + count])

    def import_(self, frames) -> None:
        """Append exported frames as that many samples would have; past the capacity nothing is appended."""
        frames = np.asarray(frames, dtype=np.float64)
        if len(self.raw) + len(frames) > self.capacity:
            raise RuntimeError(f"{self.what} import: {len(self.raw)} recorded frames + {len(frames)} exceed the capacity of {self.capacity}")
        for frame in frames:
            self.sample(frame)

    def end(self) -> None:
        pass


class HostBandSession(HostHistory):
    """The session of one quantity on the host, method for method ``HipBackend.hi_pass_*`` without the quantity argument:
    for a backend that has no device session."""
    what = "hi-pass"

    def __init__(self, ncomp: int, capacity: int):
        super().__init__((-1, ncomp), capacity)
        self.ncomp = ncomp
        self.board, self.board_node0 = None, -1
        self.cell_conn = self.cell_grad = self.cell_weight = None
        self.frames_changed()

    # The ladder of FsiCtx::Band (csrc/fsi_context.hpp), function for function: recorded frames -> selection ->
    # series -> amplitude, the spectral power index hanging on the selection, the proper orthogonal decomposition on the
    # selection (of the raw frames) or on the series (of the series).  A method that replaces a link calls that link's function,
    # once, and resets nothing by hand.
    def frames_changed(self) -> None:
        self.view = slice(None)
        self.selection_changed()

    def selection_changed(self) -> None:
        self.spi_state = None
        self.pod_state = None
        self.series_changed(None)

    def series_changed(self, series, phase_mean=None, phase_period: int = 0) -> None:
        self.filtered, self.phase_mean, self.phase_period = series, phase_mean, phase_period
        if self.pod_state is not None and self.pod_state["source"] == "series":
            self.pod_state = None                   # the decomposition was of the series that is replaced
        self.amplitude_changed(None)

    def amplitude_changed(self, amp) -> None:
        self.amp = amp

    def sample(self, frame: np.ndarray) -> None:
        super().sample(frame)
        self.frames_changed()

    def selected(self) -> np.ndarray:
        return np.stack(self.raw)[self.view]

    def series(self, name: str):
        """The (frames, nodes, ncomp) array of 'raw' (the selected raw frames), 'series' (the filtered series or the fluctuation,
        without guard frames) or 'phase_mean' (the period's mean frames), None where it does not stand: the one place that says
        where a series lies (series_view in csrc/fsi_sessions.hip).  Refusing is the caller's, under its own name."""
        return self.selected() if name == "raw" else self.filtered if name == "series" else self.phase_mean

    def select(self, first: int = 0, count: int = -1, stride: int = 1) -> int:
        frames = len(self.raw)
        fits = stride >= 1 and 0 <= first < frames and (count == -1 or (count >= 1 and first + (count - 1) * stride < frames))
        if not fits:
            raise RuntimeError(f"hi-pass select: needs stride >= 1, first >= 0, count >= 1 or -1 and first + (count - 1) * stride "
                               f"< the {frames} recorded frames")
        count = (frames - 1 - first) // stride + 1 if count == -1 else count
        self.view = slice(first, first + (count - 1) * stride + 1, stride)
        self.selection_changed()
        return count

    def filter(self, b, a, zi, padlen: int) -> None:
        self.series_changed(filtfilt_rows(b, a, self.selected(), zi, padlen))

    def phase(self, period: int) -> None:
        """The selected frames, whole cycles of ``period`` frames, into their mean over the cycles and the fluctuation about
        it (``phase_average``); the fluctuation becomes the filtered series.  A refused call changes nothing."""
        mean, fluct = phase_average(self.selected(), period)
        self.series_changed(fluct, mean, int(period))

    def phase_fetch(self, what: str, frame: int = 0) -> np.ndarray:
        """'mean' of phase ``frame`` (n, ncomp); 'energy' of fluctuation frame ``frame``, 'energy_cycle_mean' at phase ``frame``,
        'energy_time_mean' (``frame`` 0): (n,) each, summed in order from +0.0 and divided by the count."""
        if what not in PHASE_WHAT:
            raise RuntimeError(f"hi-pass phase_fetch: what must be one of {', '.join(PHASE_WHAT)}")
        if self.phase_mean is None:
            raise RuntimeError("hi-pass phase_fetch: no phase average (phase first)")
        P, n = self.phase_period, len(self.filtered)
        limit = n if what == "energy" else 1 if what == "energy_time_mean" else P
        if not 0 <= frame < limit:
            raise RuntimeError(f"hi-pass phase_fetch: frame {frame} out of range, this kind has {limit}")
        if what == "mean":
            return self.phase_mean[frame]
        if what == "energy":
            return fluctuation_energy(self.filtered[frame])
        return ordered_mean(fluctuation_energy(self.filtered[frame::P] if what == "energy_cycle_mean" else self.filtered))

    def spi(self, window, bin0: int, nb: int, Ct=None, St=None) -> None:
        """One slab of the spectral power index of the selected raw frames: the ``nb`` lowest bins from ``bin0``, ``window``
        (n,) or None for the boxcar (``spi_sums``).  A slab with ``bin0`` > 0 adds onto the slabs before it.  The twin of
        fsi_band_spi: it refuses what that refuses (``Ct`` / ``St`` are the device's: the twin forms its own tables)."""
        bin0, nb = int(bin0), int(nb)
        if self.ncomp not in (1, 3):
            raise RuntimeError("hi-pass spi: a strain / stress session has no spectral power index: it is that of a vector or a scalar (d, v, p)")
        x = self.selected() if self.raw else np.empty((0,))
        n, state = len(x), self.spi_state
        if n < 2:
            raise RuntimeError(f"hi-pass spi: {n} selected frames, the index needs at least 2 (select)")
        if nb < 1 or bin0 < 0:
            raise RuntimeError("hi-pass spi: needs bin0 >= 0 and nb >= 1 bins")
        if nb - 1 > (n - 1) // 2 - bin0:
            raise RuntimeError(f"hi-pass spi: bins {bin0} .. {bin0 + nb - 1} of {n} selected frames: a low bin lies below the Nyquist "
                               f"frequency, at most bin {(n - 1) // 2}")
        if bin0 > 0 and (state is None or state["next"] != bin0):
            raise RuntimeError(f"hi-pass spi: a slab out of order: bin0 = {bin0}, " +
                               ("no slab stands before it (bin0 = 0 first)" if state is None else f"the next slab starts at bin {state['next']}"))
        if window is not None and len(window) != n:
            raise ValueError(f"the window has {len(window)} values, {n} frames are selected")
        L2, X0, Q, mean = spi_sums(x, window, bin0, nb, None if bin0 == 0 else state["mean"])
        if bin0 == 0:
            self.spi_state = dict(L2=L2, X0=X0, Q=Q, mean=mean, n=n, next=nb)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                state.update(L2=state["L2"] + L2, next=bin0 + nb)

    def spi_fetch(self, what: str = "nodes") -> np.ndarray:
        """'rows' the index of every row (n, ncomp), 'nodes' the power-summed index of every node (n,), 'sums' L2, X0^2, Q of
        every row (3, n, ncomp), of the slabs run so far.  The twin of fsi_band_spi_fetch."""
        if what not in SPI_WHAT:
            raise RuntimeError(f"hi-pass spi_fetch: what must be one of {', '.join(SPI_WHAT)}")
        state = self.spi_state
        if state is None:
            raise RuntimeError("hi-pass spi_fetch: no spectral power index (spi first)")
        if what == "sums":
            return np.stack([state["L2"], state["X0"], state["Q"]])
        H, AC = spi_close(state["L2"], state["X0"], state["Q"], state["n"])
        return spi_ratio(H, AC) if what == "rows" else spi_node_ratio(H, AC)

    def pod_gram(self, series: str = "raw", weights=None) -> None:
        """The Gram matrix of the proper orthogonal decomposition of the selected frames: 'raw' the selected raw frames, 'series'
        the filtered series or the fluctuation; ``weights`` one value >= 0 per node or None (``pod_gram``).  Replaces a
        decomposition that stood, its modes included.  The twin of fsi_band_pod_gram: it refuses what that refuses."""
        if self.ncomp not in (1, 3):
            raise RuntimeError("hi-pass pod_gram: a strain / stress session has no proper orthogonal decomposition: it is that of a "
                               "vector or a scalar (d, v, p)")
        if series not in POD_SERIES:
            raise RuntimeError(f"hi-pass pod_gram: series must be one of {', '.join(POD_SERIES)}")
        n = len(range(*self.view.indices(len(self.raw))))
        if n < 2:
            raise RuntimeError(f"hi-pass pod_gram: {n} selected frames, the decomposition needs at least 2 (select)")
        if series == "series" and self.filtered is None:
            raise RuntimeError("hi-pass pod_gram: no filtered series (filter or phase first)")
        G, mean = pod_gram(self.series(series), weights)
        self.pod_state = dict(source=series, G=G, mean=mean, n=n, modes=None)

    def pod_modes(self, table) -> None:
        """The modes ``Phi_m = sum_j table[j, m] y_j`` of the decomposition whose Gram matrix stands, ``table`` (frames, nmodes)
        with 1 <= nmodes <= 64 (``pod_modes``).  The twin of fsi_band_pod_modes."""
        if self.pod_state is None:
            raise RuntimeError("hi-pass pod_modes: no Gram matrix (pod_gram first)")
        T = np.asarray(table, dtype=np.float64)
        if T.ndim != 2 or not 1 <= T.shape[1] <= POD_MAX_MODES:
            raise RuntimeError(f"hi-pass pod_modes: needs 1 <= nmodes <= {POD_MAX_MODES} modes and their table (frames, nmodes)")
        self.pod_state["modes"] = pod_modes(self.series(self.pod_state["source"]), self.pod_state["mean"], T)

    def pod_fetch(self, what: str, index: int = 0) -> np.ndarray:
        """'gram' the matrix (frames, frames), 'mean' the mean the frames were taken about (n, ncomp), 'mode' ``index``
        (n, ncomp).  The twin of fsi_band_pod_fetch."""
        if what not in POD_WHAT:
            raise RuntimeError(f"hi-pass pod_fetch: what must be one of {', '.join(POD_WHAT)}")
        state = self.pod_state
        if state is None:
            raise RuntimeError("hi-pass pod_fetch: no Gram matrix (pod_gram first)")
        if what != "mode":
            return state["G"] if what == "gram" else state["mean"]
        if state["modes"] is None:
            raise RuntimeError("hi-pass pod_fetch: no modes (pod_modes first)")
        if not 0 <= index < len(state["modes"]):
            raise RuntimeError(f"hi-pass pod_fetch: mode {index} out of range, {len(state['modes'])} modes stand")
        return state["modes"][index]

    def cells(self, conn, grad) -> np.ndarray:
        """Attach cells for ``cell_rate``: ``conn`` (n, 10) the cells' P2 nodes as indices into the session's nodes, local
        order, ``grad`` (n, 4, 3) the gradients of their barycentric coordinates (what ``HipBackend.hi_pass_cells`` forms from
        the mesh cells and returns).  Replaces an earlier list; a refused call leaves it in place.  Returns ``grad``."""
        if self.ncomp != 3:
            raise RuntimeError("hi-pass cells: the strain rate is that of a vector on P2 nodes: a session of d or v")
        conn, grad = np.asarray(conn), np.asarray(grad, dtype=np.float64)
        if conn.ndim != 2 or conn.shape[1] != 10 or len(conn) < 1 or grad.shape != (len(conn), 4, 3):
            raise RuntimeError(f"hi-pass cells: needs n > 0 cells, conn (n, 10) and grad (n, 4, 3), got {conn.shape} and {grad.shape}")
        nodes = len(self.raw[0]) if self.raw else None
        if conn.min() < 0 or (nodes is not None and conn.max() >= nodes):
            c, a = np.argwhere((conn < 0) | (conn >= (nodes if nodes is not None else conn.max() + 1)))[0]
            raise RuntimeError(f"hi-pass cells: cell {c} has node {conn[c, a]}, which is no node of the session")
        self.cell_conn, self.cell_grad, self.cell_weight = conn.astype(np.int64), grad.copy(), None
        return self.cell_grad

    def _cell_frames(self, what: str, series: str, first: int, step: int, count: int, own: Optional[str] = None):
        """``(x, first, step, count)`` for ``cell_rate``, ``cell_vortex`` and their ``_current`` forms: the frames x of 'raw' (the
        selected frames), 'series' or 'phase_mean', and ``count`` with -1 made as many frames as x has from ``first`` in steps
        of ``step`` - or the refusal of the C-ABI's entry point, prefixed ``what``, in its order: ``own``, the caller's own
        refusal if it has one, comes after those of the series and before those of the frames."""
        if series not in RATE_SERIES:
            raise RuntimeError(f"{what}: series must be one of {', '.join(RATE_SERIES)}")
        if self.cell_conn is None:
            raise RuntimeError(f"{what}: no cell list (cells first)")
        if series == "series" and self.filtered is None:
            raise RuntimeError(f"{what}: no filtered series (filter or phase first)")
        if series == "phase_mean" and self.phase_mean is None:
            raise RuntimeError(f"{what}: no phase average (phase first)")
        if own is not None:
            raise RuntimeError(own)
        x = self.series(series)
        first, step, count = int(first), int(step), int(count)
        if count == -1 and step >= 1:
            count = (len(x) - 1 - first) // step + 1
        if step < 1 or count < 1:
            raise RuntimeError(f"{what}: needs step >= 1 and count >= 1, got step = {step}, count = {count}")
        if not 0 <= first < len(x) or first + (count - 1) * step >= len(x):
            raise RuntimeError(f"{what}: frames {first}, {first} + {step}, ... ({count} of them) fall outside the series of {len(x)} frames")
        if self.cell_conn.max() >= x.shape[1]:
            raise RuntimeError(f"{what}: the cell list names node {self.cell_conn.max()}, the session has {x.shape[1]}")
        return x, first, step, count

    def cell_rate(self, series: str, first: int = 0, step: int = 1, count: int = -1) -> np.ndarray:
        """Per attached cell ``(((+0.0 + r[first]) + r[first + step]) + ...) / count`` with ``r[k] = cell_rate`` of frame k of
        'raw' (the selected frames), 'series' (the filtered series or the fluctuation) or 'phase_mean'; ``count`` -1: as many
        frames as the series has.  The twin of fsi_band_cell_rate."""
        x, first, step, count = self._cell_frames("hi-pass cell_rate", series, first, step, count)
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.zeros(len(self.cell_conn))
            for k in range(first, first + count * step, step):
                s = s + cell_rate(x[k][self.cell_conn], self.cell_grad)
            return s / float(count)

    def cell_weights(self, weights) -> None:
        """One weight per attached cell for the sums of ``cell_vortex``; None drops them, as a new cell list does.  The twin of
        fsi_band_cell_weights."""
        if self.cell_conn is None:
            raise RuntimeError("hi-pass cell_weights: no cell list (cells first)")
        if weights is None:
            self.cell_weight = None
            return
        w = np.array(weights, dtype=np.float64).reshape(-1)
        if len(w) != len(self.cell_conn):
            raise ValueError(f"{len(w)} weights, the session has {len(self.cell_conn)} cells")
        self.cell_weight = w

    def cell_vortex(self, series: str, first: int = 0, step: int = 1, count: int = -1, cells: bool = True, sums: bool = False):
        """``(cells, sums)``: (5, n) or None, per attached cell and row of ``VORTEX_FIELDS``
        ``(((+0.0 + r[first]) + r[first + step]) + ...) / count`` with ``r[k] = cell_vortex`` of frame k of the series, the
        frames as ``cell_rate`` takes them - row 3 is the mean over the frames of the absolute value of each frame's cell mean
        of the helicity, not of the cell mean of |w . omega|; and (5,) or None, ``cell_wsum`` of those rows with the weights of
        ``cell_weights``.  The twin of fsi_band_cell_vortex: it refuses what that refuses."""
        return self._cell_vortex("hi-pass cell_vortex", False, series, None, first, step, count, cells, sums)

    def _cell_vortex(self, what: str, current: bool, series: str, geometry, first: int, step: int, count: int, cells: bool, sums: bool):
        """``cell_vortex`` and, ``current``, ``cell_vortex_current``: the ordered means of the rows, and the sums of those means
        (``current``: of the means of the numerators)."""
        own = (f"{what}: neither cells nor sums asked for" if not cells and not sums else
               f"{what}: sums without weights (cell_weights first)" if sums and self.cell_weight is None else None)
        x, first, step, count = self._cell_frames(what, series, first, step, count, own)
        geo = self._cell_geometry(what, series, geometry) if current else None
        conn, grad = self.cell_conn, self.cell_grad
        with np.errstate(all="ignore"):
            sr = sn = np.zeros((len(VORTEX_CURRENT_FIELDS if current else VORTEX_FIELDS), len(conn)))
            for k in range(first, first + count * step, step):
                r, num = cell_vortex_current(x[k][conn], geo[k][conn], grad) if current else (cell_vortex(x[k][conn], grad),) * 2
                sr, sn = sr + r, sn + num
            out, num = sr / float(count), sn / float(count)
        return (out if cells else None), (cell_wsum(num, self.cell_weight) if sums else None)

    def _cell_geometry(self, what: str, series: str, geometry) -> np.ndarray:
        """The frames of ``geometry``, the twin session of d, that go with the frames of ``series`` of this session - for
        ``cell_rate_current`` and ``cell_vortex_current``: the recorded d frames at this session's selection for 'raw' and
        'series', ``geometry``'s phase means for 'phase_mean' - or the refusal of the C-ABI's entry point, prefixed ``what``."""
        g = geometry
        if not isinstance(g, HostBandSession) or g.ncomp != 3 or not g.raw:
            raise RuntimeError(f"{what}: no session of d: the current configuration is x = X + d")
        if g.raw[0].shape != self.raw[0].shape:
            raise RuntimeError(f"{what}: the session of d is on {len(g.raw[0])} nodes, the session of the quantity on {len(self.raw[0])}: both "
                               "must be opened on the same node list")
        if len(g.raw) != len(self.raw):
            raise RuntimeError(f"{what}: the session of d has recorded {len(g.raw)} frames, the session of the quantity {len(self.raw)}: both "
                               "must hold the same frames")
        if series != "phase_mean":
            return np.stack(g.raw)[self.view]
        if g.phase_mean is None:
            raise RuntimeError(f"{what}: the session of d has no phase average (phase of d first)")
        if g.phase_period != self.phase_period:
            raise RuntimeError(f"{what}: the phase average of d has a period of {g.phase_period} frames, that of the quantity {self.phase_period}")
        if g.view.indices(len(g.raw)) != self.view.indices(len(self.raw)):
            raise RuntimeError(f"{what}: the phase average of d is over another selection of frames than that of the quantity")
        return g.phase_mean

    def cell_vortex_current(self, series: str, geometry, first: int = 0, step: int = 1, count: int = -1, cells: bool = True,
                            sums: bool = False):
        """``cell_vortex`` in the current configuration: ``(cells, sums)``, (6, n) or None - per attached cell and row of
        ``VORTEX_CURRENT_FIELDS`` the ordered mean over the frames of the means of ``cell_vortex_current`` - and (6,) or None,
        ``cell_wsum`` with the weights of ``cell_weights`` of the same ordered means of its **numerators**: with the undeformed
        volumes as weights and one frame, the integrals over the current fluid domain and, last, its volume.  ``geometry`` and
        the pairing of the frames as ``cell_rate_current`` has them.  The twin of fsi_band_cell_vortex_current: it refuses what
        that refuses."""
        return self._cell_vortex("hi-pass cell_vortex_current", True, series, geometry, first, step, count, cells, sums)

    def cell_rate_current(self, series: str, geometry, first: int = 0, step: int = 1, count: int = -1):
        """``cell_rate`` in the current configuration: ``(rate, volume_ratio, min_jacobian)`` per attached cell, the ordered
        means over the frames of the first two of ``cell_rate_current`` and the smallest of the third.  ``geometry``: the
        twin session of d, on the same nodes and recorded frames.  Frame k of 'raw' and of 'series' is paired with the
        recorded d frame of the same absolute index - ``geometry``'s own selection does not matter -, phase j of 'phase_mean'
        with ``geometry``'s phase mean j.  The twin of fsi_band_cell_rate_current: it refuses what that refuses."""
        what = "hi-pass cell_rate_current"
        x, first, step, count = self._cell_frames(what, series, first, step, count)
        geo = self._cell_geometry(what, series, geometry)
        with np.errstate(invalid="ignore", over="ignore"):
            n = len(self.cell_conn)
            s, sv, m = np.zeros(n), np.zeros(n), np.full(n, np.inf)
            for k in range(first, first + count * step, step):
                r, vol, mk = cell_rate_current(x[k][self.cell_conn], geo[k][self.cell_conn], self.cell_grad)
                s, sv, m = s + r, sv + vol, np.where(mk < m, mk, m)
            return s / float(count), sv / float(count), m

    def end(self) -> None:
        self.cell_conn = self.cell_grad = self.cell_weight = None

    def filter_next(self, b, a, zi, padlen: int) -> None:
        if self.filtered is None:
            raise RuntimeError("hi-pass filter_next: no filtered series (filter first)")
        self.series_changed(filtfilt_rows(b, a, self.series("series"), zi, padlen))

    def trace(self, what: str, points) -> np.ndarray:
        """(points, frames, 1 + ncomp): the magnitude, then the row of each listed node over the selected frames."""
        if what == "filtered" and self.filtered is None:
            raise RuntimeError("hi-pass trace: no filtered series (filter first)")
        x = self.series("raw" if what == "raw" else "series")
        pts = np.asarray(points, dtype=np.int64).reshape(-1)
        if len(pts) and (pts.min() < 0 or pts.max() >= x.shape[1]):
            raise RuntimeError("hi-pass trace: node out of range")
        rows = x[:, pts].transpose(1, 0, 2)
        mag = np.stack([amplitude_magnitude(r) for r in rows])
        return np.concatenate([mag[:, :, None], rows], axis=2)

    def amplitude(self, window: int) -> None:
        self.amplitude_changed(self.filtered if window == 0 else windowed_rms_running(self.filtered, window))

    def board_attach(self, node0: int, board=None) -> None:
        """From now on an 'amplitude' or 'magnitude' fetch of frame k also stores its magnitudes into ``board`` (a
        ``HostBoard``) at ``[k, node0:node0 + n]``; ``node0`` -1 detaches."""
        self.board, self.board_node0 = (None, -1) if node0 < 0 else (board, int(node0))

    def fetch(self, what: str, frame: int, with_max: bool = False):
        if what == "raw":
            return self.raw[frame]
        if what == "filtered":
            return self.filtered[frame]
        mag = amplitude_magnitude(self.amp[frame])
        if self.board is not None:
            self.board.store(frame, self.board_node0, mag)
        out = mag if what == "magnitude" else self.amp[frame]
        return (out, float(mag.max()), int(np.argmax(mag))) if with_max else out


class DeviceSession:
    """``HipBackend.<prefix>_*`` of one quantity behind the host session's method names."""

    def __init__(self, backend, prefix: str, q: str):
        self.backend, self.prefix, self.q = backend, prefix, q

    def __getattr__(self, name: str):
        call = getattr(self.backend, f"{self.prefix}_{name.rstrip('_')}")       # import_ -> <prefix>_import
        return lambda *args, **kwargs: call(self.q, *args, **kwargs)

    def cell_rate_current(self, series: str, geometry, *args, **kwargs):
        """The host session's signature: on the device the geometry is the session of d the context holds."""
        return self.backend.hi_pass_cell_rate_current(self.q, series, *args, **kwargs)

    def cell_vortex_current(self, series: str, geometry, *args, **kwargs):
        """The host session's signature: on the device the geometry is the session of d the context holds."""
        return self.backend.hi_pass_cell_vortex_current(self.q, series, *args, **kwargs)


# ------------------------------------------------------------------------------------------------
# session state through a checkpoint: <results>/Checkpoint/sessions/
# ------------------------------------------------------------------------------------------------

MANIFEST = "sessions.json"
SLAB_BYTES = 1 << 28                            # host memory of one export / import call of a history


def sessions_folder(results) -> Path:
    return Path(str(results)) / "Checkpoint" / "sessions"


def sha256_of(*arrays) -> str:
    """SHA-256 of the listed arrays' shapes, types and bytes (None: an absent list)."""
    h = hashlib.sha256()
    for a in arrays:
        if a is None:
            h.update(b"none;")
            continue
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape};".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def checkpoint_position(v: dict) -> Tuple[float, int]:
    """(t, counter) of ``<restart_folder>/Checkpoint/default_variables.json``: where the restarted time loop starts."""
    path = Path(str(v["restart_folder"])) / "Checkpoint" / "default_variables.json"
    if not path.exists():
        raise SystemExit(f"--restart-folder: {path} not found")
    meta = json.loads(path.read_text())
    return float(meta["t"]), int(meta["counter"])


def restart_refusal(v: dict, key: str, words: str) -> str:
    """Why the option ``key`` cannot continue from ``v["restart_folder"]`` ('' if it can): there is no saved state for it
    (``words``: the option's own sentence, which names --restart-folder), or the state belongs to another checkpoint."""
    path = sessions_folder(v["restart_folder"]) / MANIFEST
    manifest = json.loads(path.read_text()) if path.exists() else None
    if manifest is None or key not in manifest.get("sessions", {}):
        return (f"{words}: the run in {v['restart_folder']} saved no state for the option (looked for "
                f"{'an entry ' + repr(key) + ' in ' if manifest is not None else ''}{path})")
    t, counter = checkpoint_position(v)
    if int(manifest["counter"]) != counter or float(manifest["t"]) != t:
        return (f"--restart-folder: the session state in {path} belongs to counter = {manifest['counter']}, t = {manifest['t']!r}, the "
                f"checkpoint beside it to counter = {counter}, t = {t!r}: one of the two was written by another run")
    return ""


def restart_entry(v: dict, key: str, words: str) -> Optional[dict]:
    """None without --restart-folder, else the saved entry of the option ``key``; SystemExit with ``restart_refusal``."""
    if not v.get("restart_folder"):
        return None
    why = restart_refusal(v, key, words)
    if why:
        raise SystemExit(why)
    return json.loads((sessions_folder(v["restart_folder"]) / MANIFEST).read_text())["sessions"][key]


def check_fingerprint(option: str, what: str, saved: dict, now: dict) -> None:
    """SystemExit naming every field in which what was recorded differs from what the restarted run would record."""
    bad = [f"{k} (saved {saved.get(k)!r}, now {now.get(k)!r})" for k in now if saved.get(k) != now.get(k)]
    if bad:
        raise SystemExit(f"{option}: the saved state of {what} was recorded otherwise than this run would record, it differs in "
                         + ", ".join(bad))


def frame_times(v: dict, key: str, words: str) -> Tuple[List[float], int]:
    """(times, saved): the times of the frames a run with the parameters ``v`` hands to the option ``key`` - under
    --restart-folder those its saved state holds, then those the time loop saves from the checkpoint on - and how many of
    them are saved ones."""
    entry = restart_entry(v, key, words)
    if entry is None:
        return saved_times(v), 0
    t, counter = checkpoint_position(v)
    past = [float(x) for x in entry["times"]]
    return past + saved_times(dict(v, t=t, counter=counter)), len(past)


def save_sessions(sessions, results, t: float, counter: int) -> None:
    """Every session's ``save`` into ``<results>/Checkpoint/sessions/``, then the manifest of what they wrote - last, under a
    temporary name and renamed, so that a manifest always describes complete files.  It names the checkpoint it belongs to
    and lists the running sessions only: a saved session that this run does not continue has missed frames."""
    folder = sessions_folder(results)
    folder.mkdir(parents=True, exist_ok=True)
    entries = {s.key: s.save(folder, t, counter) for s in sessions}
    manifest = dict(t=float(t), counter=int(counter), sessions={k: e for k, e in entries.items() if e is not None})
    tmp = folder / ("tmp_" + MANIFEST)
    tmp.write_text(json.dumps(manifest))
    os.replace(tmp, folder / MANIFEST)


def save_array(path: Path, a: np.ndarray) -> str:
    """``a`` to ``path`` (.npy) through a temporary name; returns the SHA-256 the manifest keeps of it."""
    tmp = path.with_name("tmp_" + path.name)
    with open(tmp, "wb") as f:
        np.save(f, np.ascontiguousarray(a, dtype=np.float64))
    os.replace(tmp, path)
    return sha256_of(a)


def load_array(path: Path, sha256: str, option: str) -> np.ndarray:
    if not path.exists():
        raise SystemExit(f"{option}: {path} not found")
    a = np.load(path)
    if sha256_of(a) != sha256:
        raise SystemExit(f"{option}: {path} is not the file the manifest beside it describes (SHA-256 differs)")
    return a


class SessionRun:
    """What the driver's sides of ``--hi-pass`` and ``--spectrogram`` share: per quantity one session, on the device or, for a
    backend without ``<prefix>_<begin>``, on the host; one recorded frame per saved frame; every session ended after ``write``."""
    prefix, begin = "", "begin"                     # HipBackend.<prefix>_<begin> opens the device session

    key = option = words = ""                       # the manifest's key, the option and its sentence about --restart-folder
    reads = None                                    # the fields of dvp_["n"] the sessions read, of d, v, p: None - the quantities asked for

    def open_sessions(self, backend, ns: dict, begin_args, host_session) -> None:
        """``begin_args(q)``: the device session's arguments before the capacity; ``host_session(q, capacity)``: its host twin.
        Under --restart-folder the saved histories are checked against ``fingerprint(q)`` and imported."""
        self.device = hasattr(backend, f"{self.prefix}_{self.begin}")
        self.frames = self.saved = 0                # recorded frames, and how many of them the history files hold
        self.times: List[float] = []
        self.sessions = {}
        entry = restart_entry(ns, self.key, self.words)
        if entry is not None:
            missing = [q for q in self.quantities if q not in entry["quantities"]]
            if missing:
                raise SystemExit(f"{self.option} {' '.join(missing)}: the run in {ns['restart_folder']} recorded "
                                 f"{' '.join(entry['quantities']) or 'none'}; a quantity added at a restart has no past")
            for q in self.quantities:
                check_fingerprint(self.option, q, entry["quantities"][q], self.fingerprint(q))
            self.times = [float(x) for x in entry["times"]]
            self.frames = self.saved = int(entry["frames"])
        capacity = self.frames + expected_frames(ns) + 1
        for q in self.quantities:
            if self.device:
                self.sessions[q] = DeviceSession(backend, self.prefix, q)
                self.begin_session(self.sessions[q], q, begin_args(q), capacity)
            else:
                self.sessions[q] = host_session(q, capacity)
        if self.saved:
            folder = sessions_folder(ns["restart_folder"])
            for q in self.quantities:
                self._read_history(folder / f"{self.file_stem}_{q}.f64", q)

    def begin_session(self, session, q: str, args, capacity: int) -> None:
        """Open the device session of ``q``: ``HipBackend.<prefix>_<begin>(q, *args, capacity)``."""
        getattr(session, self.begin)(*args, capacity)

    def sample(self, t: float, state) -> None:
        """Record dvp_["n"]; ``state``: a callable giving the host copy, used only without the device session."""
        for q, s in self.sessions.items():
            s.sample() if self.device else s.sample(self._host_frame(q, state()))
        self.frames += 1
        self.times.append(float(t))

    def _slab(self, q: str) -> int:
        return max(1, SLAB_BYTES // (8 * self.rows(q)))

    def _read_history(self, path: Path, q: str) -> None:
        """The first ``saved`` frames of a history file into the session, a slab at a time; bytes beyond them are the stale
        tail of a save that ended before its manifest."""
        rows, need = self.rows(q), 8 * self.rows(q) * self.saved
        have = path.stat().st_size if path.exists() else 0
        if have < need:
            raise SystemExit(f"{self.option}: {path} holds {have} bytes, the {self.saved} frames of {rows} rows the manifest "
                             f"beside it names need {need}")
        with open(path, "rb") as f:
            for k in range(0, self.saved, self._slab(q)):
                count = min(self._slab(q), self.saved - k)
                self.sessions[q].import_(np.fromfile(f, dtype="<f8", count=count * rows).reshape(count, rows))

    def save(self, folder, t: float, counter: int) -> dict:
        """The frames recorded since the last save appended to ``<file_stem>_<q>.f64`` (little-endian FP64 [frame][row]), a
        slab at a time; returns the manifest's entry."""
        for q, s in self.sessions.items():
            path = Path(folder) / f"{self.file_stem}_{q}.f64"
            with open(path, "r+b" if self.saved and path.exists() else "wb") as f:
                f.seek(8 * self.rows(q) * self.saved)        # whatever lies beyond the last manifest's count is overwritten
                for k in range(self.saved, self.frames, self._slab(q)):
                    f.write(np.ascontiguousarray(s.export(k, min(self._slab(q), self.frames - k)), dtype="<f8").tobytes())
                f.truncate()
        self.saved = self.frames
        return dict(frames=self.frames, times=list(self.times), quantities={q: self.fingerprint(q) for q in self.quantities})

    def finish(self, out=print) -> None:
        try:
            self.write(out)
        finally:
            for s in self.sessions.values():
                s.end()


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------

def xdmf_text(num_ts: int, time_between_files: float, start_t: float, n_elements: int, n_nodes: int, att_type: str,
              viz_type: str) -> str:
    """The text create_xdmf_file writes [REF postprocessing_h5py_common.py:543-579]."""
    n_dim = {"Scalar": "1", "Vector": "3"}[att_type]
    text = f'''<?xml version="1.0"?>
<!DOCTYPE Xdmf SYSTEM "Xdmf.dtd" []>
<Xdmf Version="3.0" xmlns:xi="http://www.w3.org/2001/XInclude">
  <Domain>
    <Grid Name="TimeSeries_{viz_type}" GridType="Collection" CollectionType="Temporal">
      <Grid Name="mesh" GridType="Uniform">
        <Topology NumberOfElements="{n_elements}" TopologyType="Tetrahedron" NodesPerElement="4">
          <DataItem Dimensions="{n_elements} 4" NumberType="UInt" Format="HDF">{viz_type}.h5:/Mesh/0/mesh/topology</DataItem>
        </Topology>
        <Geometry GeometryType="XYZ">
          <DataItem Dimensions="{n_nodes} 3" Format="HDF">{viz_type}.h5:/Mesh/0/mesh/geometry</DataItem>
        </Geometry>
'''
    for idx in range(num_ts):
        text += f'''        <Time Value="{idx * time_between_files + start_t}" />
        <Attribute Name="{viz_type}" AttributeType="{att_type}" Center="Node">
          <DataItem Dimensions="{n_nodes} {n_dim}" Format="HDF">{viz_type}.h5:/VisualisationVector/{idx}</DataItem>
        </Attribute>
      </Grid>
'''
        if idx < num_ts - 1:
            text += f'''      <Grid>
        <xi:include xpointer="xpointer(//Grid[@Name=&quot;TimeSeries_{viz_type}&quot;]/Grid[1]/*[self::Topology or self::Geometry])" />
'''
    return text + "    </Grid>\n  </Domain>\n</Xdmf>\n"


class HiPassWriter:
    """``<results>/Visualization_hi_pass/``: per series ``<viz_type>.h5`` with ``Mesh/0/mesh/{geometry f32, topology i32}``
    and ``VisualisationVector/<k>`` f32 (n, 3) or (n, 1) - h5py's defaults, as the reference creates them
    [REF create_hi_pass_viz.py:179-189,236,328] - the XDMF of ``xdmf_text``, and the amplitude table ``<viz_type>.csv``."""

    def __init__(self, folder, geometry: np.ndarray, topology: np.ndarray):
        self.folder = Path(folder)
        self.folder.mkdir(parents=True, exist_ok=True)
        self.geometry = np.ascontiguousarray(geometry, dtype=np.float32)
        self.topology = np.ascontiguousarray(topology, dtype=np.int32)

    def open(self, viz_type: str) -> H5Series:
        meshg, zero, inner, root = Group(), Group(), Group(), Group()
        inner["geometry"] = Dataset(self.geometry)
        inner["topology"] = Dataset(self.topology)
        zero["mesh"] = inner
        meshg["0"] = zero
        root["Mesh"] = meshg
        return H5Series(self.folder / f"{viz_type}.h5", root, "VisualisationVector")

    def write_series(self, viz_type: str, frames, num_ts: int, ncomp: int, time_between_files: float, start_t: float) -> None:
        """frames: an iterable of num_ts (n, ncomp) arrays; one frame in memory at a time."""
        series = self.open(viz_type)
        try:
            k = 0
            for k, frame in enumerate(frames):
                arr = np.asarray(frame).reshape(len(self.geometry), ncomp)
                series.append(str(k), arr.astype(np.float32))
            if k + 1 != num_ts:
                raise ValueError(f"{viz_type}: {k + 1} frames, expected {num_ts}")
        finally:
            series.close()
        self.write_xdmf(viz_type, num_ts, ncomp, time_between_files, start_t)

    def write_xdmf(self, viz_type: str, num_ts: int, ncomp: int, time_between_files: float, start_t: float) -> None:
        (self.folder / f"{viz_type}.xdmf").write_text(xdmf_text(num_ts, time_between_files, start_t, len(self.topology),
                                                                len(self.geometry), "Scalar" if ncomp == 1 else "Vector", viz_type))

    def write_table(self, viz_type: str, table: np.ndarray) -> None:
        np.savetxt(self.folder / f"{viz_type}.csv", table, delimiter=",", header=CSV_HEADER)


def amplitude_row(t: float, mag: np.ndarray, mx: float, argmax: int) -> np.ndarray:
    """One row of the amplitude table [REF create_hi_pass_viz.py:378-390]; the maximum and its node come from the device."""
    row = np.empty(13)
    row[0] = t
    row[1:12] = [np.percentile(mag, q) for q in CSV_PERCENTILES]
    row[3] = mx
    row[12] = argmax
    return row


def percentile_ranks(n: int) -> np.ndarray:
    """The 22 zero-based ranks of the order statistics ``np.percentile(., q)`` of n values interpolates between, per q of
    ``CSV_PERCENTILES`` the lower and the upper neighbour: ``vi = q / 100 * (n - 1)``, ``floor(vi)`` and one more, at most n - 1."""
    vi = np.true_divide(np.asarray(CSV_PERCENTILES, dtype=np.float64), 100) * (n - 1)
    lo = np.floor(vi).astype(np.int64)
    return np.stack([lo, np.minimum(lo + 1, n - 1)], axis=1).reshape(-1)


def percentiles_from_ranks(n: int, lo_hi_values) -> np.ndarray:
    """``[np.percentile(x, q) for q in CSV_PERCENTILES]`` of n values x, bit for bit, from ``np.sort(x)[percentile_ranks(n)]``
    (shape (..., 22): frames may be stacked in front): numpy's ``method="linear"``, ``a + (b - a) * t`` with ``t = vi - lo``
    and, where ``t >= 0.5``, ``b - (b - a) * (1 - t)``.  A NaN among the values makes the row NaN, as numpy does when the
    array holds one (NaNs sort last, so the largest order statistic shows it)."""
    v = np.asarray(lo_hi_values, dtype=np.float64)
    v = v.reshape(v.shape[:-1] + (len(CSV_PERCENTILES), 2))
    vi = np.true_divide(np.asarray(CSV_PERCENTILES, dtype=np.float64), 100) * (n - 1)
    t = vi - np.floor(vi)
    a, b = v[..., 0], v[..., 1]
    diff = b - a
    out = a + diff * t
    upper = np.broadcast_to(t >= 0.5, out.shape)
    out[upper] = (b - diff * (1 - t))[upper]
    out[np.isnan(v).any(axis=(-1, -2))] = np.nan
    return out


def host_room(rows: int, capacity: int) -> Tuple[int, int]:
    """(need, available) of a host session, in the numbers of the device's (``HipBackend.hi_pass_room``, fsi_band_room): the
    history, the filtered series with its guard frames, three work frames and the row lists; the host is not asked what it
    has - ``--history-memory`` is the limit of a backend without the device sessions."""
    return 8 * int(rows) * (2 * int(capacity) + 2 * 33 + 4), 1 << 62


class HostBoard:
    """``board[frame][node]`` of amplitude magnitudes on the host: the twin of the device's board (``DeviceBoard``), filled by
    the fetches of attached ``HostBandSession``s."""

    def __init__(self, nodes: int, frames: int):
        self.a = np.full((int(frames), int(nodes)), np.nan)

    def attach(self, session, node0: int) -> None:
        session.board_attach(node0, self)

    def store(self, frame: int, node0: int, mag: np.ndarray) -> None:
        self.a[frame, node0:node0 + len(mag)] = mag

    def table(self, first: int, count: int, ranks):
        """(order statistics (count, len(ranks)), NaN counts, maxima, first nodes of the maxima) of ``count`` frames."""
        ranks = np.asarray(ranks, dtype=np.int64)
        x = self.a[first:first + count]
        values = np.stack([np.partition(row, np.unique(ranks))[ranks] for row in x])
        return values, np.isnan(x).sum(axis=1), x.max(axis=1), x.argmax(axis=1)

    def end(self) -> None:
        self.a = None


class DeviceBoard:
    """The board of the device (``HipBackend.hi_pass_board_*``, fsi_board_*) behind ``HostBoard``'s method names."""

    def __init__(self, backend, nodes: int, frames: int):
        self.backend = backend
        backend.hi_pass_board_begin(nodes, frames)

    def attach(self, session, node0: int) -> None:
        session.board_attach(node0)

    def table(self, first: int, count: int, ranks):
        return self.backend.hi_pass_board_table(first, count, ranks)

    def end(self) -> None:
        self.backend.hi_pass_board_end()


def board_table(board, n: int, nodes: int, dt_files: float, t0: float) -> np.ndarray:
    """The 13-column amplitude table of n board frames: ``amplitude_row`` of every frame, its percentiles interpolated from
    the board's order statistics (``percentiles_from_ranks``), its maximum and the node of it from the board."""
    values, nans, mx, am = board.table(0, n, percentile_ranks(nodes))
    table = np.empty((n, 13))
    table[:, 0] = np.arange(n) * dt_files + t0
    table[:, 1:12] = percentiles_from_ranks(nodes, values)
    table[np.asarray(nans) > 0, 1:12] = np.nan
    table[:, 3] = mx
    table[:, 12] = am
    return table


# ------------------------------------------------------------------------------------------------
# the driver's side
# ------------------------------------------------------------------------------------------------

def quantities(v: dict) -> List[str]:
    q = v.get("hi_pass") or []
    q = [q] if isinstance(q, str) else list(q)
    bad = [x for x in q if x not in VIZ_TYPE]
    if bad:
        raise SystemExit(f"--hi-pass takes d, v and / or p, got {bad}")
    return [x for x in ("d", "v", "p") if x in q]


def bands(v: dict) -> List[Tuple[float, float]]:
    flat = v.get("hi_pass_bands")
    flat = [25, 1000] if flat is None else list(np.atleast_1d(flat))
    if len(flat) == 0 or len(flat) % 2:
        raise SystemExit("--hi-pass-bands takes pairs of a lower and an upper frequency")
    return [(float(flat[2 * i]), float(flat[2 * i + 1])) for i in range(len(flat) // 2)]


def saved_times(v: dict) -> List[float]:
    """The times of the frames the time loop of ``monolithic`` saves with these parameters (``while t <= T + dt / 10``, a
    frame when ``counter % save_step == 0``) - or, where ``v["frame_times"]`` lists them, the frames a finished folder hands
    over (``vasp_amd.postprocess``)."""
    if v.get("frame_times") is not None:
        return [float(t) for t in v["frame_times"]]
    dt, T, step = float(v["dt"]), float(v["T"]), int(v["save_step"])
    t, counter, times = float(v.get("t", 0.0)), int(v.get("counter", 0)), []
    while t <= T + dt / 10:
        t += dt
        if counter % step == 0:
            times.append(t)
        counter += 1
    return times


def expected_frames(v: dict) -> int:
    """Frames the time loop saves with these parameters."""
    return len(saved_times(v))


def frame_spacing(v: dict) -> float:
    """Seconds between two frames the sessions are handed: ``dt * save_step`` in a run; times ``v["frame_stride"]`` where a
    finished folder is read on every S-th frame (``vasp_amd.postprocess --stride``)."""
    spacing = float(v["dt"]) * int(v["save_step"])
    return spacing * int(v["frame_stride"]) if v.get("frame_stride") is not None else spacing


def frame_start(v: dict, default: float = 0.0) -> float:
    """The time the written files start at: ``default`` in a run and on a finished folder read without ``--start-time``, else
    ``v["frame_start"]`` (``vasp_amd.postprocess --start-time``, the reference's ``start_t``)."""
    return float(v["frame_start"]) if v.get("frame_times") is not None and v.get("frame_start") is not None else default


def multiband(v: dict) -> List[str]:
    """[] without ``--hi-pass-multiband``, else "pass" / "stop" per band of ``--hi-pass-bands``.  Fewer than two bands are
    refused, as the reference asserts [REF create_hi_pass_viz.py:100-101]."""
    if not v.get("hi_pass_multiband"):
        if v.get("hi_pass_pass_stop") is not None:
            raise SystemExit("--hi-pass-pass-stop belongs to --hi-pass-multiband")
        return []
    band_list = bands(v)
    if len(band_list) < 2:
        raise SystemExit(f"--hi-pass-multiband needs at least two bands in --hi-pass-bands, got {len(band_list)}")
    return pass_stop_list(band_list, v.get("hi_pass_pass_stop"))


def point_ids(v: dict) -> List[int]:
    ids = v.get("hi_pass_point_ids")
    ids = [] if ids is None else list(np.atleast_1d(ids))
    bad = [i for i in ids if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or i < 0]
    if bad:
        raise SystemExit(f"--hi-pass-point-ids takes indices >= 0 into the written nodes, got {bad}")
    return [int(i) for i in ids]


def frame_window(v: dict) -> Tuple[int, float, Optional[float]]:
    """(stride, start time, end time or None) of ``--hi-pass-stride``, ``--hi-pass-start-time``, ``--hi-pass-end-time``."""
    stride = v.get("hi_pass_stride")
    stride = 1 if stride is None else stride
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 1:
        raise SystemExit(f"--hi-pass-stride must be an integer >= 1, got {stride!r}")
    t0, t1 = v.get("hi_pass_start_time"), v.get("hi_pass_end_time")
    t0 = 0.0 if t0 is None else float(t0)
    t1 = None if t1 is None else float(t1)
    if t0 < 0.0 or (t1 is not None and t1 < t0):
        raise SystemExit(f"--hi-pass-start-time / --hi-pass-end-time: need 0 <= start <= end, got {t0:g} and {t1}")
    return int(stride), t0, t1


def select_frames(times, dt: float, stride: int, t0: float, t1: Optional[float]) -> Tuple[int, int]:
    """(first, count) of the saved frames k with ``k % stride == 0`` and ``t0 <= t_k <= t1`` (t1 None: no upper limit; the
    comparisons allow dt / 10, as the time loop's own does): frames first, first + stride, ..."""
    keep = [k for k in range(0, len(times), stride) if times[k] >= t0 - dt / 10 and (t1 is None or times[k] <= t1 + dt / 10)]
    return (keep[0], len(keep)) if keep else (0, 0)


def hi_pass_refusal(v: dict, world: int, backend_cls) -> str:
    """Why ``--hi-pass`` cannot run with the resolved parameters ``v`` ('' if it can)."""
    quantities(v)
    if not v.get("save_step"):
        return "--hi-pass records the saved frames: it needs --save-step"
    if v.get("restart_folder"):
        why = restart_refusal(v, HiPassRun.key, HiPassRun.words)
        if why:
            return why
    if world > 1:
        return "--hi-pass runs on one rank only (WORLD_SIZE > 1)"
    stride, t0, t1 = frame_window(v)
    words, _ = multiband(v), point_ids(v)
    whole = stride == 1 and t0 == 0.0 and t1 is None
    times, past = frame_times(v, HiPassRun.key, HiPassRun.words)
    frames = select_frames(times, float(v["dt"]), stride, t0, t1)[1]
    saves = f"saves {frames} frames" if whole else f"saves {frames} frames in the window and stride asked for"
    if v.get("restart_folder"):
        saves += f" ({past} saved before the restart and {len(times) - past} to come)"
    from .flow_metrics import refusal as metrics_refusal
    why = metrics_refusal(v, quantities(v))
    if why:
        return why
    from .vortex import refusal as vortex_refusal
    why = vortex_refusal(v, quantities(v))
    if why:
        return why
    cycle = phase_cycle(v)
    if cycle is not None:
        try:
            phase_cycles(v, phase_period(cycle, frame_spacing(v) * stride), frames)
        except SystemExit as e:
            return str(e)
    spi = spi_options(v)
    if spi is not None:
        try:
            spi_low_bins(frames, frame_spacing(v) * stride, spi["cutoff"])
        except SystemExit as e:
            return str(e)
    pod = pod_options(v)
    if pod is not None and frames < 2:
        return f"--hi-pass-pod: the run {saves}, the decomposition needs at least 2"
    for lo, hi in bands(v):
        # with a phase average, an index or a decomposition a band the frames do not suffice for is named when the files are
        # written and left out
        if frames < padlen_of(lo) + 1 and cycle is None and spi is None and pod is None:
            return (f"--hi-pass: the run {saves}, the filter of band {lo:g} - {hi:g} Hz needs at least "
                    f"padlen + 1 = {padlen_of(lo) + 1}")
    if words:
        dt_files = frame_spacing(v) * stride
        for lo, hi in bands(v):
            why = stage_refusal(dt_files, lo, hi)
            if why:
                return why
        if frames < 3 * (2 * ORDER + 1) + 1:        # a stage is a band-pass or band-stop: 11 coefficients whatever the band
            return f"--hi-pass-multiband: the run {saves}, a stage needs at least padlen + 1 = {3 * (2 * ORDER + 1) + 1}"
    window = int(v.get("hi_pass_window") or 250)
    if window < 1:
        return "--hi-pass-window must be at least 1"
    if v.get("hi_pass_amplitude") and frames < window:
        return f"--hi-pass-amplitude: the run {saves}, fewer than the window of {window} (--hi-pass-window)"
    return ""


def output_nodes(mesh: FsiMesh, save_deg: int, quantity: str):
    """(nodes, nodes_b) of the rows the Visualization writer writes for ``save_deg`` (vasp_amd/output.py), in its order:
    the vertices, for save_deg 2 then the edge nodes - whose pressure is the mean of the edge's two vertices."""
    V, N2 = mesh.num_vertices, mesh.num_nodes
    if save_deg < 2:
        return np.arange(V, dtype=np.int32), None
    if quantity != "p":
        return np.arange(N2, dtype=np.int32), None
    e = np.asarray(mesh.edges)
    return (np.concatenate([np.arange(V), e[:, 0]]).astype(np.int32),
            np.concatenate([np.full(V, -1), e[:, 1]]).astype(np.int32))


PHASE_WHAT = ("mean", "energy", "energy_cycle_mean", "energy_time_mean")      # HipBackend.PHASE_WHAT, FSI_PHASE_*
METRICS_STRIPS = ("--hi-pass-flow-metrics: the history goes through the session in strips of rows, which do not keep a cell's 30 rows "
                  "together (give it room with --history-memory, or fewer frames with --stride)")
PHASE_STRIPS = ("--hi-pass-phase-average: the history goes through the session in strips of rows, which form no phase average "
                "(give it room with --history-memory, or fewer frames with --stride)")


SPI_STRIPS = ("--hi-pass-spi: the history goes through the session in strips of rows, on which no spectral power index is formed "
              "(give it room with --history-memory, or fewer frames with --stride)")
SPI_TABLE_BYTES = 1 << 27                       # cos and sin columns of one slab of low bins (HiPassRun._write_spi)
SPI_HEADER = ("quantity, cut-off (Hz), window, frames, sampling rate (Hz), bin width (Hz), low bins kc, minimum SPI, mean SPI, "
              "maximum SPI, ID of node with max SPI")


def spi_options(v: dict) -> Optional[dict]:
    """None without ``--hi-pass-spi``, else ``cutoff`` (``--hi-pass-spi-cutoff``, 25 Hz) and ``window``
    (``--hi-pass-spi-window``, boxcar)."""
    for key in ("hi_pass_spi_cutoff", "hi_pass_spi_window"):
        if v.get(key) is not None and not v.get("hi_pass_spi"):
            raise SystemExit(f"--{key.replace('_', '-')} belongs to --hi-pass-spi")
    if not v.get("hi_pass_spi"):
        return None
    cutoff = v.get("hi_pass_spi_cutoff")
    cutoff = 25.0 if cutoff is None else cutoff
    if isinstance(cutoff, bool) or not isinstance(cutoff, (int, float, np.integer, np.floating)) or not cutoff > 0:
        raise SystemExit(f"--hi-pass-spi-cutoff must be a frequency > 0 Hz, got {cutoff!r}")
    window = v.get("hi_pass_spi_window")
    window = "boxcar" if window is None else window
    if window not in SPI_WINDOWS:
        raise SystemExit(f"--hi-pass-spi-window must be one of {', '.join(SPI_WINDOWS)}, got {window!r}")
    return dict(cutoff=float(cutoff), window=str(window))


POD_STRIPS = ("--hi-pass-pod: the history goes through the session in strips of rows, on which no proper orthogonal decomposition is "
              "formed (give it room with --history-memory, or fewer frames with --stride)")
POD_COLUMNS = "mode, eigenvalue, energy fraction, cumulative fraction, resolved (0: below the floor, neither formed nor written)"


def pod_options(v: dict) -> Optional[dict]:
    """None without ``--hi-pass-pod``, else ``modes`` (``--hi-pass-pod-modes``, 10, from 1 to 64) and ``weights``
    (``--hi-pass-pod-weights``, volume)."""
    for key in ("hi_pass_pod_modes", "hi_pass_pod_weights"):
        if v.get(key) is not None and not v.get("hi_pass_pod"):
            raise SystemExit(f"--{key.replace('_', '-')} belongs to --hi-pass-pod")
    if not v.get("hi_pass_pod"):
        return None
    modes = v.get("hi_pass_pod_modes")
    modes = 10 if modes is None else modes
    if isinstance(modes, bool) or not isinstance(modes, (int, np.integer)) or not 1 <= modes <= POD_MAX_MODES:
        raise SystemExit(f"--hi-pass-pod-modes must be an integer from 1 to {POD_MAX_MODES}, got {modes!r}")
    weights = v.get("hi_pass_pod_weights")
    weights = "volume" if weights is None else weights
    if weights not in POD_WEIGHTS:
        raise SystemExit(f"--hi-pass-pod-weights must be one of {', '.join(POD_WEIGHTS)}, got {weights!r}")
    return dict(modes=int(modes), weights=str(weights))


def pod_energy_counts(spectrum: np.ndarray, trace: float) -> Tuple[int, int]:
    """The number of leading modes whose eigenvalues, added in order, reach 90 % and 99 % of the trace (0, 0 for a trace of 0)."""
    if not trace > 0:
        return 0, 0
    cum = np.cumsum(np.asarray(spectrum, dtype=np.float64)) / trace
    return tuple(int(min(np.count_nonzero(cum < level) + 1, len(cum))) for level in (0.9, 0.99))


def phase_cycle(v: dict) -> Optional[float]:
    """None without ``--hi-pass-phase-average``, else the cycle length in seconds: ``--hi-pass-cycle`` or the resolved
    parameters' ``T_Cycle``; without either the run is refused."""
    for key in ("hi_pass_cycle", "hi_pass_start_cycle", "hi_pass_end_cycle"):
        if v.get(key) is not None and not v.get("hi_pass_phase_average"):
            raise SystemExit(f"--{key.replace('_', '-')} belongs to --hi-pass-phase-average")
    if not v.get("hi_pass_phase_average"):
        return None
    cycle = v.get("hi_pass_cycle")
    cycle = v.get("T_Cycle") if cycle is None else cycle
    if cycle is None:
        raise SystemExit("--hi-pass-phase-average needs the length of a cycle: give --hi-pass-cycle SECONDS (the parameters hold no T_Cycle)")
    if isinstance(cycle, bool) or not isinstance(cycle, (int, float, np.integer, np.floating)) or not cycle > 0:
        raise SystemExit(f"--hi-pass-cycle must be a number of seconds > 0, got {cycle!r}")
    return float(cycle)


def phase_period(cycle: float, time_between_files: float) -> int:
    """Frames of a cycle, ``cycle / time_between_files``.  The reference rounds the ratio [REF log_plotter.py:944-946], and a
    ratio that is no integer makes its phases drift from cycle to cycle: here one further than 1e-6 (relative) from an integer
    is refused, with both numbers."""
    ratio = cycle / time_between_files
    period = int(np.rint(ratio))
    if period < 1 or abs(ratio - period) > 1e-6 * ratio:
        raise SystemExit(f"--hi-pass-phase-average: a cycle of {cycle!r} s is {ratio!r} frames of {time_between_files!r} s "
                         "(dt * save_step * stride), not a whole number of them: the phases would drift from cycle to cycle "
                         "(choose --hi-pass-cycle, --save-step or --hi-pass-stride so that it is)")
    return period


def phase_cycles(v: dict, period: int, frames: int) -> Tuple[int, int]:
    """(first, last) cycle that is averaged, 1-based and inclusive as in the reference [REF log_plotter.py:928-946]:
    ``--hi-pass-start-cycle`` (default 1) and ``--hi-pass-end-cycle`` (default: the last whole cycle) among the whole cycles
    of ``period`` frames that ``frames`` selected frames hold."""
    whole = frames // period
    if whole < 1:
        raise SystemExit(f"--hi-pass-phase-average: the window and stride asked for hold {frames} frames, fewer than one whole "
                         f"cycle of {period}")
    c0, c1 = v.get("hi_pass_start_cycle"), v.get("hi_pass_end_cycle")
    c0, c1 = 1 if c0 is None else c0, whole if c1 is None else c1
    for c in (c0, c1):
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
            raise SystemExit(f"--hi-pass-start-cycle / --hi-pass-end-cycle must be integers, got {c!r}")
    if not 1 <= c0 <= c1 <= whole:
        raise SystemExit(f"--hi-pass-start-cycle {c0} / --hi-pass-end-cycle {c1}: need 1 <= start <= end <= {whole}, the whole "
                         f"cycles of {period} frames among the {frames} frames of the window and stride asked for")
    return int(c0), int(c1)


TRACE_HEADER = {1: "time (s), Magnitude", 3: "time (s), Magnitude, X Component, Y Component, Z Component"}      # [REF postprocessing_h5py_common.py:482]


class HiPassRun(SessionRun):
    """The driver's side of ``--hi-pass``: one session per quantity on the Visualization writer's nodes, one recorded frame
    per saved frame, and at the end per band the filtered series, with ``--hi-pass-amplitude`` its amplitude and table; with
    ``--hi-pass-multiband`` one more series that went through all bands in order; with ``--hi-pass-point-ids`` the recorded
    series of those nodes; with ``--hi-pass-phase-average`` the mean over the cardiac cycles, the fluctuation about it and the
    velocity's turbulent kinetic energy (``_write_phase``); with ``--hi-pass-spi`` the spectral power index of the recorded
    frames (``_write_spi``).  With ``--hi-pass-flow-metrics`` and ``--hi-pass-vortex`` the velocity session also serves the
    cell quantities of ``flow_metrics.FlowMetrics`` and ``vortex.VortexMetrics``.  All of it on the saved frames k with ``k % stride == 0`` and ``T0 <= t_k <= T1``
    (``--hi-pass-stride``, ``--hi-pass-start-time``, ``--hi-pass-end-time``; every selected frame is kept, where the reference
    drops the last ones, postprocessing_h5py_common.py:285,307).  Times in the files are ``T0 + k * time_between_files``, T0
    being the reference's ``start_t``; ``time_between_files`` is dt * save_step * stride, the spacing of the selected frames
    (the reference takes dt * stride and notes the doubt, :621-634)."""
    prefix = file_stem = key = "hi_pass"
    option, words = "--hi-pass", "--hi-pass cannot be used with --restart-folder"

    def __init__(self, backend, mesh: FsiMesh, ns: dict):
        from .output import refine_topology
        self.backend, self.mesh = backend, mesh
        self.save_deg = int(ns["save_deg"])
        self.quantities = quantities(ns)
        self.bands = bands(ns)
        self.pass_stop = multiband(ns)
        self.point_ids = point_ids(ns)
        self.stride, self.t0, self.t1 = frame_window(ns)
        self.t0 = frame_start(ns, self.t0)
        self.amplitude = bool(ns.get("hi_pass_amplitude"))
        self.window = int(ns.get("hi_pass_window") or 250)
        self.dt = float(ns["dt"])
        self.dt_sample = frame_spacing(ns)
        self.dt_files = self.dt_sample * self.stride
        cycle = phase_cycle(ns)
        self.period = None if cycle is None else phase_period(cycle, self.dt_files)
        self.cycle_range = {key: ns.get(key) for key in ("hi_pass_start_cycle", "hi_pass_end_cycle")}
        self.spi = spi_options(ns)
        self.spi_lines: List[str] = []
        self.pod = pod_options(ns)
        self.pod_weights = pod_volume_weights(mesh, self.save_deg) if self.pod is not None and self.pod["weights"] == "volume" else None
        self.nodes = {q: output_nodes(mesh, self.save_deg, q) for q in self.quantities}
        if self.save_deg >= 2:
            geometry, topology = mesh.node_coords, refine_topology(mesh)
        else:
            geometry, topology = mesh.coords, mesh.tets
        for q in self.quantities:
            n = len(self.nodes[q][0])
            bad = [i for i in self.point_ids if i >= n]
            if bad:
                raise SystemExit(f"--hi-pass-point-ids: {bad} out of range, {VIZ_TYPE[q]} is written on {n} nodes")
        # a strip (vasp_amd.hi_pass_strips): the session is opened on nodes i0 .. i1 - 1 of the one quantity asked for
        self.strip = ns.get("hi_pass_strip")
        if self.strip is not None:
            if self.period is not None:
                raise SystemExit(PHASE_STRIPS)
            if ns.get("hi_pass_flow_metrics"):
                raise SystemExit(METRICS_STRIPS)
            if ns.get("hi_pass_vortex"):
                from .vortex import VORTEX_STRIPS
                raise SystemExit(VORTEX_STRIPS)
            if self.spi is not None:
                raise SystemExit(SPI_STRIPS)
            if self.pod is not None:
                raise SystemExit(POD_STRIPS)
            i0, i1 = self.strip
            self.nodes = {q: tuple(None if a is None else a[i0:i1] for a in ab) for q, ab in self.nodes.items()}
        self.writer = HiPassWriter(Path(ns["results_folder"]) / "Visualization_hi_pass", geometry, topology)
        self.trace_folder = Path(ns["results_folder"]) / "Visualization_separate_domain"      # [REF create_hi_pass_viz.py:565,639]
        self.metrics = None
        if ns.get("hi_pass_flow_metrics"):
            from . import flow_metrics
            why = flow_metrics.refusal(ns, self.quantities)
            if why:
                raise SystemExit(why)
            self.metrics = flow_metrics.FlowMetrics(mesh, ns)
        self.vortex = None
        if ns.get("hi_pass_vortex") or ns.get("hi_pass_vortex_series") or ns.get("hi_pass_vortex_configuration"):
            from . import vortex
            why = vortex.refusal(ns, self.quantities)
            if why:
                raise SystemExit(why)
            self.vortex = vortex.VortexMetrics(mesh, ns)
        self.open_sessions(backend, ns, lambda q: self.nodes[q],
                           lambda q, capacity: HostBandSession(1 if q == "p" else 3, capacity))

    def rows(self, q: str) -> int:
        return len(self.nodes[q][0]) * (1 if q == "p" else 3)

    def fingerprint(self, q: str) -> dict:
        return dict(save_deg=self.save_deg, dt_sample=self.dt_sample, rows=self.rows(q), nodes=sha256_of(*self.nodes[q]))

    def _host_frame(self, q: str, state: np.ndarray) -> np.ndarray:
        frame = self._whole_host_frame(q, state)
        return frame if self.strip is None else frame[self.strip[0]:self.strip[1]]

    def _whole_host_frame(self, q: str, state: np.ndarray) -> np.ndarray:
        d, v, p = self.mesh.split(state)
        V = self.mesh.num_vertices
        if q == "p":
            if self.save_deg >= 2:
                e = self.mesh.edges
                p = np.concatenate([p, 0.5 * (p[e[:, 0]] + p[e[:, 1]])])
            return p[:, None]
        f = d if q == "d" else v
        return f if self.save_deg >= 2 else f[:V]

    def _write_filtered(self, out, session, viz: str, n: int, ncomp: int, rms: bool) -> None:
        """The session's filtered series as ``viz`` and, with --hi-pass-amplitude, its amplitude (the windowed RMS, or for
        ``rms`` False - the reference's low-pass case - the series itself) and table."""
        self.writer.write_series(viz, (session.fetch("filtered", k) for k in range(n)), n, ncomp, self.dt_files, self.t0)
        if not self.amplitude:
            return
        if rms and n < self.window:
            out(f"Hi-pass {viz}: {n} frames recorded, fewer than the window of {self.window}: no amplitude written")
            return
        session.amplitude(self.window if rms else 0)
        table = np.empty((n, 13))

        def amp_frames():
            for k in range(n):
                amp, mx, am = session.fetch("amplitude", k, True)
                table[k] = amplitude_row(k * self.dt_files + self.t0, amplitude_magnitude(amp), mx, am)
                yield amp

        self.writer.write_series(f"{viz}_amplitude", amp_frames(), n, ncomp, self.dt_files, self.t0)
        self.writer.write_table(viz, table)

    def _write_traces(self, session, q: str, n: int, ids=None, local=None, what: str = "raw", suffix: str = "") -> None:
        """``<viz_type>_point_id_<id>.csv``: time, magnitude and components of the recorded rows of each listed node
        [REF postprocessing_h5py_common.py:470-483], the times being T0 + k * time_between_files, one per frame.  ``ids``
        with ``local``: the ids among ``point_ids`` that a strip holds, and their indices into the strip's nodes.  ``what``
        "filtered" with a ``suffix`` of the file's name: the same of the filtered series (the fluctuation of a phase average)."""
        ids, local = (self.point_ids, self.point_ids) if ids is None else (ids, local)
        self.trace_folder.mkdir(parents=True, exist_ok=True)
        trace = np.asarray(session.trace(what, local))
        for i, rows in zip(ids, trace):
            data = np.empty((n, rows.shape[1] + 1 if q != "p" else 2))
            data[:, 0] = self.t0 + np.arange(n) * self.dt_files
            data[:, 1:] = rows if q != "p" else rows[:, :1]
            np.savetxt(self.trace_folder / f"{VIZ_TYPE[q]}{suffix}_point_id_{i}.csv", data, delimiter=",", header=TRACE_HEADER[1 if q == "p" else 3])

    def series_list(self, q: str, n: int, out) -> List[Tuple[str, List[dict], bool]]:
        """(viz, stages, rms) of every series ``q`` is written as on n frames, in the order they are written: per band its
        one filter, then with --hi-pass-multiband the chain of all bands.  ``stages``: the designs ``apply`` runs in order;
        ``rms``: the amplitude is the windowed RMS (False - the reference's low-pass case: the series itself).  A series the
        frames do not suffice for is named through ``out`` and left out."""
        series = []
        for lo, hi in self.bands:
            prm = design(self.dt_files, lo, hi)
            viz = f"{VIZ_TYPE[q]}_{prm['name']}"
            if n <= prm["padlen"]:
                out(f"Hi-pass {viz}: {n} frames recorded, the filter needs more than {prm['padlen']}: nothing written")
                continue
            series.append((viz, [prm], prm["btype"] != "lowpass"))
        if not self.pass_stop:
            return series
        # the recorded rows through all bands in order [REF create_hi_pass_viz.py:191-198].  Its amplitude is the windowed
        # RMS, as a band-pass's: the reference itself raises NameError here (filter_type_single is undefined, :222)
        viz = multiband_name(VIZ_TYPE[q], self.bands, self.pass_stop)
        stages = [design(self.dt_files, lo, hi, "bandpass" if word == "pass" else "bandstop")
                  for (lo, hi), word in zip(self.bands, self.pass_stop)]
        if n <= max(prm["padlen"] for prm in stages):
            out(f"Hi-pass {viz}: {n} frames recorded, the filter needs more than {max(prm['padlen'] for prm in stages)}: nothing written")
            return series
        series.append((viz, stages, True))
        return series

    def _write_phase(self, out, session, q: str, first: int, n: int) -> None:
        """``--hi-pass-phase-average``: the mean over the cycles, the fluctuation about it with - under --hi-pass-amplitude -
        its windowed RMS (the turbulence intensity) and, of the velocity, the turbulent kinetic energy 0.5 |u'|^2 per frame,
        averaged over the cycles and averaged over time [REF log_plotter.py:902-989].  Cycle c is selected frames
        (c - 1) P ... c P - 1 of the ``n`` frames of the window; the files of the cycle range start at its first frame's time."""
        P, name, ncomp = self.period, VIZ_TYPE[q], 1 if q == "p" else 3
        try:
            c0, c1 = phase_cycles(self.cycle_range, P, n)
        except SystemExit as why:                 # a run that was stopped early: named and left out, as a band without its frames
            out(f"Hi-pass {name}: {why}: no phase average written")
            return
        m, skipped = (c1 - c0 + 1) * P, (c0 - 1) * P
        session.select(first + skipped * self.stride, m, self.stride)
        session.phase(P)
        t0 = self.t0
        self.writer.write_series(f"{name}_phase_mean", (session.phase_fetch("mean", j) for j in range(P)), P, ncomp, self.dt_files, t0)
        self.t0 = t0 + skipped * self.dt_files
        try:
            if self.point_ids:
                self._write_traces(session, q, m, what="filtered", suffix="_fluctuation")
            self._write_filtered(out, session, f"{name}_fluctuation", m, ncomp, True)
            if q == "v":
                self.writer.write_series(f"{name}_tke", (session.phase_fetch("energy", k) for k in range(m)), m, 1, self.dt_files, self.t0)
        finally:
            self.t0 = t0
        if q == "v":
            self.writer.write_series(f"{name}_tke_phase_mean", (session.phase_fetch("energy_cycle_mean", j) for j in range(P)), P, 1,
                                     self.dt_files, t0)
            self.writer.write_series(f"{name}_tke_avg", [session.phase_fetch("energy_time_mean", 0)], 1, 1, self.dt_files, t0)
            if self.metrics is not None:      # R(u') over the frames of the chosen cycles, at each phase, and R of the phase means
                rate, geometry = self.metrics.rate, self.sessions.get("d")
                self.metrics.phase = dict(fluctuation=rate(session, geometry, "series"), mean=rate(session, geometry, "phase_mean"),
                                          cycle_mean=np.stack([rate(session, geometry, "series", j, P, m // P) for j in range(P)]))
            if self.vortex is not None:
                self.vortex.collect_phase(session, P, self.sessions.get("d"))
        out(f"Hi-pass {name}: phase average over cycles {c0} to {c1} of {P} frames written")

    def _write_spi(self, out, session, q: str, n: int) -> None:
        """``--hi-pass-spi``: ``<viz_type>_spi_<cutoff>``, one scalar frame with the spectral power index of every written
        node over the ``n`` selected raw frames - of d and v the index of the power summed over the components -, and the
        quantity's line of ``spi.csv``.  The kc lowest bins go through the session in slabs of at most ``SPI_TABLE_BYTES``
        of tables, a multiple of 64 bins."""
        cutoff, window = self.spi["cutoff"], self.spi["window"]
        name = f"{VIZ_TYPE[q]}_spi_{int(np.rint(cutoff))}"
        try:
            kc = spi_low_bins(n, self.dt_files, cutoff)
        except SystemExit as why:                 # a run that was stopped early: named and left out, as a band without its frames
            out(f"Hi-pass {name}: {why}: no index written")
            return
        from .spectrogram import window_values
        w = None if window == "boxcar" else window_values(window, n)
        slab = max(64, SPI_TABLE_BYTES // (16 * n) // 64 * 64)
        for bin0 in range(0, kc, slab):
            session.spi(w, bin0, min(slab, kc - bin0))
        field = np.asarray(session.spi_fetch("nodes"), dtype=np.float64).reshape(-1)
        self.writer.write_series(name, [field], 1, 1, self.dt_files, self.t0)
        finite = np.isfinite(field)
        good = field[finite]
        stats = (float(good.min()), float(good.mean()), float(good.max()), int(np.flatnonzero(finite)[np.argmax(good)])) if len(good) else \
            (float("nan"), float("nan"), float("nan"), -1)
        fs, width = 1.0 / self.dt_files, 1.0 / (n * self.dt_files)
        self.spi_lines.append(f"{VIZ_TYPE[q]}, {cutoff!r}, {window}, {n}, {fs!r}, {width!r}, {kc}, {stats[0]!r}, {stats[1]!r}, {stats[2]!r}, {stats[3]}")
        out(f"Hi-pass {name}: spectral power index over {n} frames, {kc - 1} bins of {width:g} Hz below the cut-off ({window}), written; "
            f"mean {stats[1]:.6g}, maximum {stats[2]:.6g} at node {stats[3]}")

    def _write_pod(self, out, session, q: str, n: int, series: str, stem: str) -> None:
        """``--hi-pass-pod``: the snapshot proper orthogonal decomposition of the ``n`` selected raw frames (``series`` 'raw') or
        of the series that stands ('series').  ``<stem>_modes``: one dataset per resolved mode, the xdmf time being the mode
        number; ``<stem>.csv``: eigenvalue, energy fraction, cumulative fraction and resolved flag per mode, its header line
        with the frames, the weights, the trace, the floor and the modes that 90 % and 99 % of the energy take;
        ``<stem>_coefficients.csv``: the time and a_1 .. a_M.  The Gram matrix and the modes are the session's, the eigen step
        between them is ``pod_eig`` on the host."""
        ncomp, want = 1 if q == "p" else 3, self.pod["modes"]
        if n < 2:
            out(f"Hi-pass {stem}: {n} frames recorded, the decomposition needs at least 2: nothing written")
            return
        M = min(want, n - 1)
        if M < want:
            out(f"Hi-pass {stem}: --hi-pass-pod-modes {want} clipped to {M}, the {n} frames less one")
        session.pod_gram(series, self.pod_weights)
        try:
            eig = pod_eig(np.asarray(session.pod_fetch("gram")), self.rows(q), M)
        except RuntimeError as why:               # a NaN or an inf among the recorded values: named and left out
            out(f"Hi-pass {stem}: {why}: no decomposition written")
            return
        T = pod_table(eig)
        K = T.shape[1]
        if K:
            session.pod_modes(T)
            self.writer.write_series(f"{stem}_modes", (session.pod_fetch("mode", m) for m in range(K)), K, ncomp, 1, 1)
        k90, k99 = pod_energy_counts(eig["spectrum"], eig["trace"])
        header = (f"# {POD_COLUMNS}; frames = {n}, weights = {self.pod['weights']}, trace = {eig['trace']!r}, floor = {eig['floor']!r}, "
                  f"modes for 90 % = {k90}, modes for 99 % = {k99}")
        lines, cum = [header], 0.0
        for m in range(M):
            cum = cum + float(eig["fraction"][m])
            lines.append(f"{m + 1}, {float(eig['lam'][m])!r}, {float(eig['fraction'][m])!r}, {cum!r}, {int(eig['resolved'][m])}")
        (self.writer.folder / f"{stem}.csv").write_text("\n".join(lines) + "\n")
        table = np.empty((n, M + 1))
        table[:, 0] = self.t0 + np.arange(n) * self.dt_files
        table[:, 1:] = pod_coefficients(eig)
        np.savetxt(self.writer.folder / f"{stem}_coefficients.csv", table, delimiter=",",
                   header="time (s), " + ", ".join(f"a_{m + 1}" for m in range(M)))
        out(f"Hi-pass {stem}: proper orthogonal decomposition of {n} frames ({self.pod['weights']} weights), {K} of {M} modes resolved and "
            f"written; mode 1 carries {float(eig['fraction'][0]):.6g} of the energy, {k90} modes 90 %, {k99} modes 99 %")

    @staticmethod
    def apply(session, stages) -> None:
        """The session's filtered series after ``stages``: the first on the selected frames, every further one on the series."""
        for k, prm in enumerate(stages):
            (session.filter_next if k else session.filter)(prm["b"], prm["a"], prm["zi"], prm["padlen"])

    def write(self, out) -> None:
        first, n = select_frames(self.times, self.dt, self.stride, self.t0, self.t1)
        if n == 0:
            out(f"Hi-pass: none of the {self.frames} recorded frames lies in the window and stride asked for: nothing written")
            return
        order = list(self.sessions)
        if any(m is not None and m.configuration == "current" for m in (self.metrics, self.vortex)):
            # d first: by the time the velocity's phase mean is paired with the displacement's, d holds its phase average
            order.sort(key=lambda q: q != "d")
        for q in order:
            session = self.sessions[q]
            ncomp = 1 if q == "p" else 3
            session.select(first, n, self.stride)
            if self.point_ids:
                self._write_traces(session, q, n)
            metrics = self.metrics if q == "v" else None
            if metrics is not None:            # the fluid cells stay attached through the filters and the phase average
                metrics.attach(session, self.device)
                metrics.raw = metrics.rate(session, self.sessions.get("d"), "raw")
            vortex = self.vortex if q == "v" else None
            if vortex is not None:             # the same cells, with their volumes as weights; the per-frame files are written here
                vortex.attach(session, self.device, attached=metrics is not None)
                vortex.collect(session, n, self.dt_files, self.t0, self.sessions.get("d"))
            for viz, stages, rms in self.series_list(q, n, out):
                self.apply(session, stages)
                self._write_filtered(out, session, viz, n, ncomp, rms)
                if metrics is not None and len(stages) == 1:
                    metrics.bands[stages[0]["name"]] = metrics.rate(session, self.sessions.get("d"), "series")
                if self.pod is not None and len(stages) == 1:      # of a band's filtered series; the chain of all bands is not decomposed
                    self._write_pod(out, session, q, n, "series", f"{viz}_pod")
            if self.spi is not None:            # on the selection of the bands, before the phase average narrows it to whole cycles
                self._write_spi(out, session, q, n)
            if self.pod is not None:            # of the selected raw frames, on the selection of the bands
                self._write_pod(out, session, q, n, "raw", f"{VIZ_TYPE[q]}_pod")
            if self.period is not None:
                self._write_phase(out, session, q, first, n)
            if metrics is not None:
                metrics.write(out, self.dt_files, self.t0)
            if vortex is not None:
                vortex.write(out, self.dt_files, self.t0)
        if self.spi_lines:
            (self.writer.folder / "spi.csv").write_text("# " + SPI_HEADER + "\n" + "\n".join(self.spi_lines) + "\n")
        out(f"Hi-pass fields of {n} frames ({', '.join(self.quantities)}) written to {self.writer.folder}")
