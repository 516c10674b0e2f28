"""Average spectrograms, power spectra, chromagrams and the spectral bandedness index of a run: `<results>/Spectrograms/`.

Counterpart of ``vasp-create-spectrograms-chromagrams`` and ``vasp-create-spectrum``
[REF src/vasp/postprocessing/postprocessing_h5py/create_spectrograms_chromagrams.py:21-219, create_spectrum.py:19-72,
spectrograms.py:160-329,381-499,558-583,685-745,796-814], whose row loops around ``scipy.signal.spectrogram`` /
``periodogram`` run on the device on a history recorded during the run (``HipBackend.spec_*``, csrc/fsi_spec.hip).  Because
the transform is a matrix product on the FP64 matrix pipe, the sample can be every node of the region (``sampling All``) or
a seeded draw; the reference's unseeded draw of 1000 nodes exists only because its row loop is slow.  This module holds

* the region and sampling rules of ``read_spectrogram_data`` on the nodes of the run's own output (``select_nodes``);
* the window arithmetic, the chroma filter bank (a restatement of the librosa formula the reference carries), the
  chromagram and the SBI;
* ``HostSpecSession``: the device session in NumPy - the same table, the same explicit detrend, the same order of the
  sum over the rows - for a backend without ``spec_begin`` and as the yardstick of the GPU tests;
* the pipeline, the writer of the reference's CSV files and the driver's side of ``--spectrogram`` (``SpectrogramRun``).

Two of the reference's habits are kept on purpose: with a single row ``get_psd`` ignores the scaling it is given and
returns scipy's default ``"density"`` (spectrograms.py:418-419), and the periodogram's window is always ``blackmanharris``
whatever ``--spectrogram-window`` says (:410-419).

Times: the frames are ``dt * save_step`` apart; ``T = frames * dt * save_step``, ``start_t = 0`` (the reference's default),
``fs = frames / T``.

``--stride`` and a time window are those of ``vasp_amd.postprocess`` on a finished folder: the spacing, ``T`` and ``start_t`` then
come from the frames that were read.

A history larger than the device: on a finished folder the rows go through the session in strips
(``vasp_amd.spectrogram_strips``); the three mean powers are sums over blocks of rows in a fixed order, so the sum is carried
from strip to strip (``spectrogram_sum`` / ``periodogram_sum``) and the files are those of one session on all rows.

The wall shear stress (``--spectrogram wss``): the rows are components or magnitudes of the DG1 function on the boundary mesh
of the fluid that ``--hemodynamics`` writes (``hemodynamics.fluid_boundary_facets``; dof 3 f + k is vertex k of facet f, at that
vertex's coordinate), recorded on the device at every saved frame by the kernel of the hemodynamics session's arithmetic
(``HipBackend.spec_begin_wss``, k_spec_wss_sample in csrc/fsi_hemo.hip): no second tool run and no pass over ``WSS.h5``.  The
reference's own ``wss`` path reads a file nothing writes and keeps one entry of the vector as its magnitude
[REF spectrograms.py:215-217,255-257; postprocessing_h5py_common.py:342-343]; the rows here are what the rest of it implies.
The region is the dofs inside the sphere or box (``interface_only`` is ignored, as the reference takes ``sphere_ids`` alone);
``domain`` is refused: the boundary mesh carries no cell markers.  There is no host recording path for it.
It is a quantity where the parameters hold ``mu_f``, the viscosity it is formed with (``quantities``).

``--spectrogram-region domain`` samples the cells of a marker and asks for at least one of the two sampling-domain ids.

``PointList`` also writes the reference's sound file, ``<quantity>_sound_<case>.wav`` (``sonify_point``, ``sound_of``).

Not done: the PNG figures.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

from .hemodynamics import FACET_VERTS, fluid_boundary_facets
from .hi_pass import DeviceSession, HostHistory, SessionRun, expected_frames, frame_spacing, frame_start, frame_times, output_nodes, restart_refusal, sha256_of
from .mesh import FsiMesh

HP_ORDER = 6                                    # filter_time_data(order=6, btype="highpass") [REF spectrograms.py:558]
HP_PADLEN = 3 * (HP_ORDER + 1)                  # filtfilt's default for 7 coefficients
N_CHROMA = 24                                   # [REF create_spectrograms_chromagrams.py:112]
MIN_COLOR = {"d": -42, "v": -20, "p": -5, "wss": -18}      # [REF spectrograms.py:133-150]
FIELD_OF = {"d": "d", "v": "v", "p": "p", "wss": "v"}     # the field of dvp_["n"] a quantity's rows are formed from
REGIONS = ("sphere", "box", "domain")
COMPONENTS = ("all", "x", "y", "z", "mag")
SAMPLINGS = ("RandomPoint", "PointList", "All")
ROWS = 128                                      # csrc/fsi_spec.hpp: SPEC_ROWS
HOST_CHUNK = 32 * ROWS                          # columns of one C @ Y product of the host session (mean_power)
PI_L = np.longdouble("3.14159265358979323846264338327950288")


# ------------------------------------------------------------------------------------------------
# options
# ------------------------------------------------------------------------------------------------

def add_arguments(ap, coerce) -> None:
    """The ``--spectrogram*`` options of ``vasp_amd.monolithic`` (defaults: ``options``)."""
    ap.add_argument("--spectrogram", dest="spectrogram", nargs="+", default=None, metavar="Q",
                    help="record d, v, p and / or wss (the wall shear stress) at every saved frame on the device and write the average spectrogram, "
                         "chromagram, SBI and power spectrum of a region to <results>/Spectrograms/ (what "
                         "vasp-create-spectrograms-chromagrams and vasp-create-spectrum write afterwards)")
    ap.add_argument("--spectrogram-region", dest="spectrogram_region", default=None,
                    help="sphere (default), box or domain (the nodes of the cells marked --spectrogram-fluid-sampling-domain-id / "
                         "--spectrogram-solid-sampling-domain-id, of which at least one must be given; not for wss)")
    ap.add_argument("--spectrogram-fluid-sampling-domain-id", dest="spectrogram_fluid_sampling_domain_id", type=int, default=None,
                    help="cell marker of the fluid region that --spectrogram-region domain samples (default 1)")
    ap.add_argument("--spectrogram-solid-sampling-domain-id", dest="spectrogram_solid_sampling_domain_id", type=int, default=None,
                    help="cell marker of the solid region that --spectrogram-region domain samples (default 2)")
    ap.add_argument("--spectrogram-fsi-region", dest="spectrogram_fsi_region", nargs="+", type=coerce, default=None,
                    help="x y z r of the sphere, or x_min x_max y_min y_max z_min z_max of the box (default: the problem's fsi_region)")
    ap.add_argument("--spectrogram-interface-only", dest="spectrogram_interface_only", action="store_const", const=True, default=None)
    ap.add_argument("--spectrogram-component", dest="spectrogram_component", default=None, help="all (default), x, y, z or mag")
    ap.add_argument("--spectrogram-sampling", dest="spectrogram_sampling", default=None,
                    help="RandomPoint (default: n-samples region nodes drawn with --spectrogram-seed), PointList or All (every region node)")
    ap.add_argument("--spectrogram-n-samples", dest="spectrogram_n_samples", type=int, default=None, help="default 1000")
    ap.add_argument("--spectrogram-point-ids", dest="spectrogram_point_ids", nargs="+", type=coerce, default=None)
    ap.add_argument("--spectrogram-seed", dest="spectrogram_seed", type=int, default=None, help="seed of the draw (default 0)")
    ap.add_argument("--spectrogram-lowcut", dest="spectrogram_lowcut", type=float, default=None, help="high-pass cut-off in Hz (default 25)")
    ap.add_argument("--spectrogram-overlap-frac", dest="spectrogram_overlap_frac", type=float, default=None, help="default 0.75")
    ap.add_argument("--spectrogram-window", dest="spectrogram_window", default=None,
                    help="a parameter-free scipy.signal.get_window name (default blackmanharris)")
    ap.add_argument("--spectrogram-num-windows-per-sec", dest="spectrogram_num_windows_per_sec", type=coerce, default=None, help="default 4")
    ap.add_argument("--spectrogram-min-color", dest="spectrogram_min_color", type=coerce, default=None,
                    help="lower clamp of the log spectrogram (default: -42 for d, -20 for v, -5 for p, -18 for wss)")


def quantities(v: dict) -> List[str]:
    q = v.get("spectrogram") or []
    q = [q] if isinstance(q, str) else list(q)
    # the wall shear stress is formed with the fluid's viscosity: it is a quantity only where the parameters hold mu_f, as
    # those of every run and of every finished folder do
    bad = [x for x in q if x not in MIN_COLOR or (x == "wss" and v.get("mu_f") is None)]
    if bad:
        raise SystemExit(f"--spectrogram takes d, v and / or p, and wss where the parameters hold the viscosity mu_f, got {bad}")
    return [x for x in ("d", "v", "p", "wss") if x in q]


def fields(v: dict) -> List[str]:
    """The fields of dvp_["n"] the asked quantities read: the wall shear stress is formed from the velocity."""
    return sorted({FIELD_OF[q] for q in quantities(v)})


def options(v: dict) -> dict:
    """The resolved ``spectrogram_*`` parameters with the reference's defaults [REF spectrograms.py:56-105]."""
    get = lambda key, default: default if v.get("spectrogram_" + key) is None else v["spectrogram_" + key]
    o = dict(region=str(get("region", "sphere")), fsi_region=get("fsi_region", v.get("fsi_region")),
             interface_only=bool(get("interface_only", False)), component=str(get("component", "all")),
             sampling=str(get("sampling", "RandomPoint")), n_samples=int(get("n_samples", 1000)),
             point_ids=get("point_ids", None), seed=int(get("seed", 0)), lowcut=float(get("lowcut", 25)),
             overlap_frac=float(get("overlap_frac", 0.75)), window=str(get("window", "blackmanharris")),
             num_windows_per_sec=get("num_windows_per_sec", 4), min_color=get("min_color", None),
             fluid_sampling_domain_id=int(get("fluid_sampling_domain_id", 1)),        # [REF spectrograms.py:66-71]
             solid_sampling_domain_id=int(get("solid_sampling_domain_id", 2)))
    # domain samples the cells of a marker: which one is the user's to say - at least one of the two ids must be given (the
    # other keeps the reference's default), since 1 and 2 by default would silently be the whole fluid or the whole solid
    named = any(v.get("spectrogram_" + k) is not None for k in ("fluid_sampling_domain_id", "solid_sampling_domain_id"))
    if o["region"] not in REGIONS or (o["region"] == "domain" and not named):
        raise SystemExit(f"--spectrogram-region takes sphere or box, or domain together with --spectrogram-fluid-sampling-domain-id and / or "
                         f"--spectrogram-solid-sampling-domain-id, got {o['region']!r}")
    if o["region"] == "domain" and "wss" in quantities(v):
        raise SystemExit("--spectrogram wss with --spectrogram-region domain: the boundary mesh the wall shear stress lives on carries no "
                         "cell markers; use sphere or box")
    if o["component"] not in COMPONENTS:
        raise SystemExit(f"--spectrogram-component takes one of {', '.join(COMPONENTS)}, got {o['component']!r}")
    if o["sampling"] not in SAMPLINGS:
        raise SystemExit(f"--spectrogram-sampling takes one of {', '.join(SAMPLINGS)}, got {o['sampling']!r}")
    fr = None if o["fsi_region"] is None else [float(x) for x in np.atleast_1d(o["fsi_region"])]
    if o["region"] == "domain":
        fr = None                                 # no sphere or box cut: the markers alone [REF spectrograms.py:235-241]
    elif fr is None or len(fr) != (4 if o["region"] == "sphere" else 6):
        raise SystemExit("--spectrogram-fsi-region takes x y z r for a sphere and x_min x_max y_min y_max z_min z_max for a box")
    o["fsi_region"] = fr
    if o["point_ids"] is not None:
        o["point_ids"] = [int(x) for x in np.atleast_1d(o["point_ids"])]
    if o["sampling"] == "PointList" and not o["point_ids"]:
        raise SystemExit("--spectrogram-sampling PointList needs --spectrogram-point-ids")
    if o["sampling"] == "RandomPoint" and o["n_samples"] < 1:
        raise SystemExit("--spectrogram-n-samples must be at least 1")
    if not 0.0 <= o["overlap_frac"] < 1.0:
        raise SystemExit("--spectrogram-overlap-frac must be in [0, 1)")
    try:
        window_values(o["window"], 8)
    except Exception as e:
        raise SystemExit(f"--spectrogram-window: {o['window']!r} is not a parameter-free scipy.signal.get_window name ({e})")
    return o


# ------------------------------------------------------------------------------------------------
# window arithmetic
# ------------------------------------------------------------------------------------------------

def shift_bit_length(x: int) -> int:
    """The smallest power of two >= x [REF spectrograms.py:381-394]."""
    return 1 << (int(x) - 1).bit_length()


def window_values(name: str, n: int) -> np.ndarray:
    """``scipy.signal.get_window(name, n)`` (periodic), as scipy's spectrogram and periodogram call it."""
    from scipy.signal import get_window
    return np.asarray(get_window(str(name), int(n)), dtype=np.float64)


def window_plan(n: int, T: float, num_windows_per_sec, overlap_frac: float) -> dict:
    """The segment sizes of ``create_spectrogram_composite`` / ``get_spectrogram`` for n frames over T seconds
    [REF create_spectrograms_chromagrams.py:50, spectrograms.py:446-453]: ``num_windows`` stays the float numpy makes of it
    (the file names print it so), ``nseg`` is scipy's count of whole segments."""
    num_windows = np.round(num_windows_per_sec * T) + 3
    per = int(n / num_windows)
    nperseg = shift_bit_length(per) if per >= 1 else 0
    noverlap = int(overlap_frac * nperseg)
    step = nperseg - noverlap
    nseg = (n - noverlap) // step if nperseg >= 1 and step >= 1 and n >= nperseg else 0
    return dict(num_windows=num_windows, nperseg=nperseg, noverlap=noverlap, nfft=2 * nperseg, nseg=int(nseg))


def highpass_design(fs: float, lowcut: float) -> dict:
    """``butter(6, lowcut / (fs / 2), "highpass")`` [REF spectrograms.py:516-525,558], ``lfilter_zi`` and filtfilt's padlen."""
    from scipy.signal import butter, lfilter_zi
    b, a = butter(HP_ORDER, lowcut / (0.5 * fs), btype="highpass")
    return dict(b=np.asarray(b, dtype=np.float64), a=np.asarray(a, dtype=np.float64), zi=np.asarray(lfilter_zi(b, a)),
                padlen=3 * max(len(a), len(b)))


# ------------------------------------------------------------------------------------------------
# chroma, SBI
# ------------------------------------------------------------------------------------------------

def chroma_filterbank(sr: float, n_fft: int, n_chroma: int = N_CHROMA, ctroct: float = 5.0, octwidth: float = 2.0) -> np.ndarray:
    """The chroma filter bank of the reference's tools (the librosa chroma filter at tuning 0, [REF chroma_filters.py:397-531]),
    written from its definition; (n_chroma, n_fft // 2 + 1), float32 as the reference's.

    FFT bin k > 0 has the pitch ``p_k = n_chroma log2(f_k / 27.5 Hz)`` in chroma steps, ``f_k = k sr / n_fft``; the 0 Hz bin is put
    1.5 octaves below bin 1.  Chroma class c answers to bin k with ``exp(-2 (d / s_k)^2)``: d is p_k - c wrapped into
    [-n_chroma / 2, n_chroma / 2), s_k the distance to the next bin's pitch but at least one step (1 for the last bin).  Every
    bin's column is scaled to unit Euclidean length, then weighted by ``exp(-((p_k / n_chroma - ctroct) / octwidth)^2 / 2)``, the
    preference for the octaves around ``ctroct``; class 0 is C, a quarter octave above A."""
    classes = np.arange(n_chroma, dtype=np.float64)[:, None]
    pitch = np.empty(n_fft)
    pitch[1:] = n_chroma * np.log2(np.arange(1, n_fft) * (sr / n_fft) / 27.5)
    pitch[0] = pitch[1] - 1.5 * n_chroma
    spacing = np.ones(n_fft)
    spacing[:-1] = np.maximum(np.diff(pitch), 1.0)
    half = n_chroma // 2
    wrapped = np.mod(pitch[None, :] - classes + half, n_chroma) - half
    bank = np.exp(-2.0 * np.square(wrapped / spacing[None, :]))
    bank /= np.linalg.norm(bank, axis=0)[None, :]
    bank *= np.exp(-0.5 * np.square((pitch / n_chroma - ctroct) / octwidth))[None, :]
    from_c = (np.arange(n_chroma) + n_chroma // 4) % n_chroma            # row c of the result is the class a quarter octave above c
    return bank[from_c, :n_fft // 2 + 1].astype(np.float32)


def chromagram(Pxx: np.ndarray, fs: float, n_fft: int, n_chroma: int = N_CHROMA) -> np.ndarray:
    """The chroma filter bank applied to a (bins, segments) power, every segment's classes scaled to sum 1 - the reference's
    ``norm="sum"`` [REF spectrograms.py:685-727], which the entropy below needs."""
    energy = chroma_filterbank(fs, n_fft, n_chroma) @ Pxx
    return energy / energy.sum(axis=0, keepdims=True)


def sbi(chroma: np.ndarray, n_chroma: int = N_CHROMA) -> np.ndarray:
    """Spectral bandedness index per segment, ``1 + sum_c c log c / log n_chroma``: 0 for a flat chromagram, 1 for a single
    class [REF spectrograms.py:730-745]."""
    return 1.0 + (chroma * np.log(chroma)).sum(axis=0) / np.log(n_chroma)


# ------------------------------------------------------------------------------------------------
# the device's arithmetic in NumPy
# ------------------------------------------------------------------------------------------------

def spec_tables(K: int, nfft: int, bin0: int, nb: int):
    """C, S (nb, K): cos / sin(2 pi (j k mod nfft) / nfft) for the bins k = bin0 .. bin0 + nb - 1, the angle formed in
    extended precision and the value rounded to FP64 once - what fsi_sessions.hip uploads."""
    m = np.arange(nfft, dtype=np.longdouble)
    ang = (np.longdouble(2) * PI_L) * m / np.longdouble(nfft)
    cosm, sinm = np.cos(ang).astype(np.float64), np.sin(ang).astype(np.float64)
    jk = np.outer(np.arange(bin0, bin0 + nb, dtype=np.int64), np.arange(K, dtype=np.int64)) % nfft
    return cosm[jk], sinm[jk]


def block_sums(P: np.ndarray) -> np.ndarray:
    """(bins, rows) -> (bins, row blocks): the sum over the rows of every block of ROWS rows in k_spec_power's order - in a
    lane the block's eight 16-row tiles one after the other, then a four-step butterfly over the 16 lanes."""
    nb, rows = P.shape
    nblk = -(-rows // ROWS)
    full = np.zeros((nb, nblk * ROWS))
    full[:, :rows] = P
    tiles = full.reshape(nb, nblk, ROWS // 16, 16)
    lane = np.zeros((nb, nblk, 16))
    for a in range(ROWS // 16):
        lane = lane + tiles[:, :, a, :]
    for half in (8, 4, 2, 1):
        lane = lane[:, :, :half] + lane[:, :, half:2 * half]
    return lane[:, :, 0]


def sum_power(x: np.ndarray, K: int, step: int, nseg: int, nfft: int, window: np.ndarray, scaling: str, fs: float,
              carry: Optional[np.ndarray] = None, total_rows: int = 0, max_table_bytes: int = 1 << 27,
              chunk: int = HOST_CHUNK) -> np.ndarray:
    """(nfft // 2 + 1, nseg): ``carry`` (None: zeros) plus the sums, over the blocks of ROWS rows of x (frames, rows) in index
    order, of the one-sided power of nseg segments of K frames, ``step`` apart - fsi_spec.hip operation for operation except
    the order inside a dot product (BLAS here, the matrix pipe's there); divided by ``total_rows`` where that is > 0.  The
    rows go through ``C @ Y`` in chunks of ``chunk`` columns: rows handed over in strips that start at multiples of it form
    the same products and, the carry handed on, the same sum."""
    x = np.asarray(x, dtype=np.float64)
    rows = x.shape[1]
    w = np.asarray(window, dtype=np.float64)
    sw = sw2 = 0.0
    for v in w:
        sw += float(v)
        sw2 += float(v) * float(v)
    scale = 1.0 / (fs * sw2) if scaling == "density" else 1.0 / (sw * sw)
    nbins = nfft // 2 + 1
    last_single = nfft // 2 if nfft % 2 == 0 else -1
    out = np.empty((nbins, nseg))
    slab = max(1, min(nbins, max_table_bytes // (16 * K)))
    for seg in range(nseg):
        xs = x[seg * step:seg * step + K]
        acc = np.zeros(rows)
        for j in range(K):
            acc = acc + xs[j]
        Y = w[:, None] * (xs - (acc / float(K))[None, :])
        for bin0 in range(0, nbins, slab):
            nb = min(slab, nbins - bin0)
            C, S = spec_tables(K, nfft, bin0, nb)
            parts = []
            for r0 in range(0, rows, chunk):
                Yc = np.ascontiguousarray(Y[:, r0:r0 + chunk])      # the same operand whatever rows lie beside the chunk
                re, im = C @ Yc, S @ Yc
                parts.append(block_sums((re * re + im * im) * scale))
            part = np.concatenate(parts, axis=1)
            g = np.arange(bin0, bin0 + nb)
            part = np.where(((g == 0) | (g == last_single))[:, None], part, 2.0 * part)
            tot = np.zeros(nb) if carry is None else np.array(carry[bin0:bin0 + nb, seg], dtype=np.float64)
            for k in range(part.shape[1]):
                tot = tot + part[:, k]
            out[bin0:bin0 + nb, seg] = tot / float(total_rows) if total_rows > 0 else tot
    return out


def mean_power(x: np.ndarray, K: int, step: int, nseg: int, nfft: int, window: np.ndarray, scaling: str, fs: float,
               max_table_bytes: int = 1 << 27, chunk: int = HOST_CHUNK) -> np.ndarray:
    """(nfft // 2 + 1, nseg): the average over the rows of x (frames, rows) of the one-sided power: ``sum_power`` of one strip
    that holds every row."""
    return sum_power(x, K, step, nseg, nfft, window, scaling, fs, None, np.asarray(x).shape[1], max_table_bytes, chunk)


def host_room(rows: int, capacity: int, magnitude: bool = False) -> Tuple[int, int]:
    """(need, available) of a host session, in the numbers of the device's (``HipBackend.spec_room``, fsi_spec_room): the raw
    and the filtered history with its guard frames, the row lists (three entries per row of magnitudes), 64 bins of a
    periodogram's tables and the means of capacity / 4 segments; the host is not asked what it has - ``--history-memory`` is
    the limit of a backend without the device sessions."""
    rows, capacity = int(rows), int(capacity)
    return (8 * rows * (2 * capacity + 2 * 33) + 16 * (3 * rows if magnitude else rows) + 16 * 64 * capacity
            + 2 * rows * capacity + 16 * rows), 1 << 62


class HostSpecSession(HostHistory):
    """The session of one quantity on the host, method for method ``HipBackend.spec_*`` without the quantity argument.
    ``granule``: the rows a strip of a longer row list must start at a multiple of for the carried sums to be those of one
    session on all rows - the column chunk of ``sum_power``."""
    what = "spectrogram"
    granule = HOST_CHUNK

    def __init__(self, nrows: int, capacity: int, chunk: int = HOST_CHUNK):
        super().__init__(int(nrows), capacity)
        self.nrows = int(nrows)
        self.granule = int(chunk)

    def fetch(self, frame: int, filtered: bool = False) -> np.ndarray:
        return self.filtered[frame] if filtered else self.raw[frame]

    def _source(self) -> np.ndarray:
        return self.filtered if self.filtered is not None else np.stack(self.raw)

    def _carried(self, name: str, shape, first_row: int, total_rows: int, carry):
        """The refusals of fsi_spec_*_sum in the host's granule; the carry a sum starts from (None: zeros)."""
        g = self.granule
        if first_row < 0 or first_row % g:
            raise RuntimeError(f"spectrogram {name}: first_row = {first_row}, a strip starts at a multiple of {g} rows")
        if total_rows == 0 and self.nrows % g:
            raise RuntimeError(f"spectrogram {name}: the session has {self.nrows} rows and is not the last strip (total_rows = 0), "
                               f"needs a multiple of {g}")
        if total_rows != 0 and total_rows != first_row + self.nrows:
            raise RuntimeError(f"spectrogram {name}: total_rows = {total_rows}, the last strip ends at first_row + rows = "
                               f"{first_row} + {self.nrows}")
        if first_row == 0:
            return None
        if carry is None or np.shape(carry) != shape:
            raise RuntimeError(f"spectrogram {name}: needs the carry of the rows before first_row, of shape {shape}")
        return carry

    @staticmethod
    def _handed_on(carry, result: np.ndarray) -> np.ndarray:
        if carry is None:
            return result
        carry[...] = result                     # in place, as the device call updates the caller's array
        return carry

    def spectrogram_sum(self, nperseg: int, noverlap: int, nfft: int, window, scaling: str, fs: float, first_row: int,
                        total_rows: int = 0, carry=None) -> np.ndarray:
        x = self._source()
        step = nperseg - noverlap
        nseg = (len(x) - noverlap) // step
        start = self._carried("spectrogram_sum", (nfft // 2 + 1, nseg), int(first_row), int(total_rows), carry)
        return self._handed_on(carry, sum_power(x, nperseg, step, nseg, nfft, window, scaling, fs, start, int(total_rows), chunk=self.granule))

    def periodogram_sum(self, window, scaling: str, fs: float, first_row: int, total_rows: int = 0, carry=None) -> np.ndarray:
        x = self._source()
        start = self._carried("periodogram_sum", (len(x) // 2 + 1,), int(first_row), int(total_rows), carry)
        res = sum_power(x, len(x), len(x), 1, len(x), window, scaling, fs, None if start is None else np.asarray(start)[:, None],
                        int(total_rows), chunk=self.granule)[:, 0]
        return self._handed_on(carry, res)

    def spectrogram(self, nperseg: int, noverlap: int, nfft: int, window, scaling: str, fs: float) -> np.ndarray:
        return self.spectrogram_sum(nperseg, noverlap, nfft, window, scaling, fs, 0, self.nrows)

    def periodogram(self, window, scaling: str, fs: float) -> np.ndarray:
        return self.periodogram_sum(window, scaling, fs, 0, self.nrows)


class DeviceSpecSession(DeviceSession):
    """``HipBackend.spec_*`` of one quantity behind the host session's method names; its granule is the row block of
    k_spec_power."""
    granule = ROWS

    def __init__(self, backend, q: str):
        super().__init__(backend, "spec", q)


def component_rows(values: np.ndarray, component: str) -> np.ndarray:
    """The rows of one frame from the (nodes, ncomp) values at the sampled nodes: a component, the three stacked
    component-major, or the magnitude; a scalar has one."""
    values = np.asarray(values, dtype=np.float64)
    if values.ndim == 1 or values.shape[1] == 1:
        return values.reshape(-1)
    if component == "all":
        return values.T.reshape(-1)
    if component == "mag":
        return np.sqrt((values[:, 0] * values[:, 0] + values[:, 1] * values[:, 1]) + values[:, 2] * values[:, 2])
    return values[:, "xyz".index(component)].copy()


# ------------------------------------------------------------------------------------------------
# region and sampling rules
# ------------------------------------------------------------------------------------------------

def degree_of(quantity: str, save_deg: int) -> int:
    """The output the rows live on: the run's save_deg, the pressure at degree 1 (the reference's choice when no degree is
    given [REF create_spectrograms_chromagrams.py:237])."""
    return 1 if quantity == "p" else int(save_deg)


def region_ids(mesh: FsiMesh, deg: int, quantity: str, v: dict, o: dict) -> np.ndarray:
    """Ids, on the degree-``deg`` output node list, of the nodes the spectrogram of ``quantity`` may sample
    [REF spectrograms.py:221-266]: solid nodes for d, fluid nodes for v and p, the nodes the two share with
    ``interface_only``; of those, the ones strictly inside the sphere or the open box.  Region ``domain``
    [REF spectrograms.py:235-241, postprocessing_h5py_common.py:59-87]: the fluid and the solid nodes are those of the cells
    whose marker equals the fluid / the solid sampling id, and nothing is cut."""
    cells = mesh.tet_nodes if deg >= 2 else mesh.tets
    coords = mesh.node_coords if deg >= 2 else mesh.coords
    as_list = lambda x: list(x) if isinstance(x, (list, tuple)) else [x]
    domain = o["region"] == "domain"
    fluid = np.unique(cells[np.isin(mesh.cell_markers, [o["fluid_sampling_domain_id"]] if domain else as_list(v["dx_f_id"]))])
    solid = np.unique(cells[np.isin(mesh.cell_markers, [o["solid_sampling_domain_id"]] if domain else as_list(v["dx_s_id"]))])
    if o["interface_only"]:
        ids = np.intersect1d(fluid, solid)
    else:
        ids = solid if quantity == "d" else fluid
    if domain:
        return ids
    return np.intersect1d(inside_region(coords, o), ids)


def inside_region(coords: np.ndarray, o: dict) -> np.ndarray:
    """Indices of the points strictly inside the sphere or the open box of ``o`` [REF spectrograms.py:221-250]."""
    fr = o["fsi_region"]
    if o["region"] == "sphere":
        inside = np.where(np.linalg.norm(coords - np.array(fr[:3]), axis=1) < fr[3])[0]
    else:
        inside = np.where((coords[:, 0] > fr[0]) & (coords[:, 0] < fr[1]) & (coords[:, 1] > fr[2]) & (coords[:, 1] < fr[3])
                          & (coords[:, 2] > fr[4]) & (coords[:, 2] < fr[5]))[0]
    return inside


def viscosity(v: dict) -> float:
    """The viscosity ``--hemodynamics`` passes: ``mu_f``, its first entry when it is a list."""
    return float(v["mu_f"][0] if isinstance(v["mu_f"], (list, tuple)) else v["mu_f"])


def select_wss(mesh: FsiMesh, v: dict, o: dict) -> dict:
    """The sampled rows of the wall shear stress: ``ids``, the sampled DG1 dofs of the boundary mesh of the fluid (dof 3 f + k:
    vertex k of facet f of ``fluid_boundary_facets``, at that vertex's coordinate), the row lists ``dofs`` / ``comps`` (0 .. 2, 3
    the magnitude; ``all`` stacks the components component-major), the whole facet list ``facet_cells`` / ``facet_local`` and
    ``mu``.  The region is the dofs inside the sphere or box; ``interface_only`` is ignored [REF spectrograms.py:255-257]."""
    _, cells, local = fluid_boundary_facets(mesh, v["dx_f_id"])
    nd = 3 * len(cells)
    region = inside_region(mesh.coords[mesh.tets[cells[:, None], FACET_VERTS[local]].reshape(-1)], o) if nd else np.zeros(0, dtype=np.int64)
    if len(region) == 0:
        raise SystemExit(f"--spectrogram wss: no nodes found in the specified fsi region: {o['fsi_region']}")
    comp = o["component"]
    suffix = ""
    if o["sampling"] == "RandomPoint":
        ids = np.random.default_rng(o["seed"]).choice(region, o["n_samples"])
        name = f"wss_{comp}_n_samples_{o['n_samples']}"
    elif o["sampling"] == "PointList":
        ids = np.array(o["point_ids"], dtype=np.int64)
        if ((ids < 0) | (ids >= nd)).any():
            raise SystemExit(f"--spectrogram-point-ids: ids must be in 0 .. {nd - 1} (the DG1 dofs of the boundary mesh of wss)")
        name, suffix = f"wss_{comp}", f"_PointList_{o['point_ids']}"
    else:
        ids, name = region, f"wss_{comp}"
    ids = np.asarray(ids, dtype=np.int64)
    if comp == "all":
        dofs, comps = np.tile(ids, 3), np.repeat(np.arange(3), len(ids))
    else:
        dofs, comps = ids, np.full(len(ids), ("x", "y", "z", "mag").index(comp))
    return dict(ids=ids, dofs=dofs.astype(np.int32), comps=comps.astype(np.int32), facet_cells=np.asarray(cells, dtype=np.int64),
                facet_local=np.asarray(local, dtype=np.int32), mu=viscosity(v), name=name, case_suffix=suffix, degree=None)


def select_nodes(mesh: FsiMesh, save_deg: int, quantity: str, v: dict, o: dict) -> dict:
    """The sampled rows of one quantity: ``ids`` on the output node list, the (nodes, nodes_b) a session is opened on, and
    the two name parts of the files [REF spectrograms.py:268-287].  RandomPoint draws n_samples region nodes with
    replacement, as the reference does, from ``numpy.random.default_rng(seed)``; All is every region node once.  The wall
    shear stress has rows of its own (``select_wss``)."""
    if quantity == "wss":
        return select_wss(mesh, v, o)
    deg = degree_of(quantity, save_deg)
    region = region_ids(mesh, deg, quantity, v, o)
    if len(region) == 0:
        raise SystemExit(f"--spectrogram {quantity}: no nodes found in the specified fsi region: {o['fsi_region']}")
    comp = o["component"]
    suffix = ""
    if o["sampling"] == "RandomPoint":
        ids = np.random.default_rng(o["seed"]).choice(region, o["n_samples"])
        name = f"{quantity}_{comp}_n_samples_{o['n_samples']}"
    elif o["sampling"] == "PointList":
        ids = np.array(o["point_ids"], dtype=np.int64)
        limit = mesh.num_nodes if deg >= 2 else mesh.num_vertices
        if ((ids < 0) | (ids >= limit)).any():
            raise SystemExit(f"--spectrogram-point-ids: ids must be in 0 .. {limit - 1} (the degree-{deg} output of {quantity})")
        name, suffix = f"{quantity}_{comp}", f"_PointList_{o['point_ids']}"
    else:
        ids, name = region, f"{quantity}_{comp}"
    nodes, nodes_b = output_nodes(mesh, deg, quantity)
    return dict(ids=np.asarray(ids, dtype=np.int64), nodes=nodes[ids], nodes_b=None if nodes_b is None else nodes_b[ids],
                name=name, case_suffix=suffix, degree=deg)


# ------------------------------------------------------------------------------------------------
# pipeline and files
# ------------------------------------------------------------------------------------------------

def transform_plan(nrows: int, n: int, T: float, o: dict) -> dict:
    """What the three transforms of n frames over T seconds are called with: the segment sizes and the window of the
    spectrograms, the high-pass, the periodogram's window and scaling.  ``nrows`` is the number of all rows, wherever they
    are held: with a single one ``get_psd`` drops the scaling it is given."""
    fs = n / T
    plan = window_plan(n, T, o["num_windows_per_sec"], o["overlap_frac"])
    return dict(plan=plan, fs=fs, n=n, nrows=nrows, window=window_values(o["window"], plan["nperseg"]), hp=highpass_design(fs, o["lowcut"]),
                psd_window=window_values("blackmanharris", n), psd_scaling="spectrum" if nrows > 1 else "density")


def session_powers(session, tp: dict, strip=None, carries=None):
    """The three mean powers the pipeline takes from a session (``HostSpecSession`` or its device twin behind the same
    calls) that holds n frames: the spectrogram of the high-passed rows, that of the raw rows and the raw rows' periodogram.
    ``strip``: None where the session holds all ``tp["nrows"]`` rows; else ``(first_row, last)`` of a session that holds the
    rows from ``first_row`` on - ``carries``, the three sums over the rows before (None for the first strip), are handed on
    through the ``_sum`` calls, and the last strip returns the means."""
    plan, fs, hp = tp["plan"], tp["fs"], tp["hp"]
    K, nov, nfft = plan["nperseg"], plan["noverlap"], plan["nfft"]
    if strip is None:
        spectrogram = lambda k: session.spectrogram(K, nov, nfft, tp["window"], "spectrum", fs)
        periodogram = lambda k: session.periodogram(tp["psd_window"], tp["psd_scaling"], fs)
    else:
        first_row, total = int(strip[0]), tp["nrows"] if strip[1] else 0
        c = [None, None, None] if carries is None else carries
        spectrogram = lambda k: session.spectrogram_sum(K, nov, nfft, tp["window"], "spectrum", fs, first_row, total, c[k])
        periodogram = lambda k: session.periodogram_sum(tp["psd_window"], tp["psd_scaling"], fs, first_row, total, c[k])
    session.filter(hp["b"], hp["a"], hp["zi"], hp["padlen"])
    P_filtered = spectrogram(0)
    session.filter()
    P_raw = spectrogram(1)
    return [P_filtered, P_raw, periodogram(2)]


def results(powers, tp: dict, start_t: float, min_color) -> dict:
    """``create_spectrogram_composite`` and ``create_spectrum`` from the three mean powers of ``session_powers``: the clamped
    log spectrogram of the high-passed rows, the chromagram and SBI of the raw rows' spectrogram, and the log of the raw
    rows' average periodogram."""
    P_filtered, P_raw, P_psd = powers
    plan, fs, n = tp["plan"], tp["fs"], tp["n"]
    K, nov, nfft = plan["nperseg"], plan["noverlap"], plan["nfft"]
    freqs = np.fft.rfftfreq(nfft, 1 / fs)
    bins = np.arange(K / 2, n - K / 2 + 1, K - nov) / float(fs) + start_t

    def scaled(P):                      # get_spectrogram's guard and spectrogram_scaling [REF spectrograms.py:471,491-497]
        P = np.array(P)
        P[P < 0] = 1e-16
        with np.errstate(divide="ignore"):
            L = np.log(P)
        L[L < min_color] = min_color
        return L

    chroma = chromagram(np.exp(scaled(P_raw)), fs, nfft)
    with np.errstate(divide="ignore"):
        log_psd = np.log(P_psd)
    return dict(plan=plan, fs=fs, freqs=freqs, bins=bins, spectrogram=scaled(P_filtered), chroma=chroma, sbi=sbi(chroma),
                psd_freqs=np.fft.rfftfreq(n, 1 / fs), psd=log_psd, power_filtered=P_filtered, power_raw=P_raw, power_psd=P_psd,
                psd_scaling=tp["psd_scaling"])


def pipeline(session, nrows: int, n: int, T: float, start_t: float, o: dict, min_color) -> dict:
    """The three mean powers of a session that holds n frames of nrows rows (``session_powers``), turned into what the files
    hold (``results``)."""
    tp = transform_plan(nrows, n, T, o)
    return results(session_powers(session, tp), tp, start_t, min_color)


def sound_of(filtered: np.ndarray):
    """``sonify_point`` [REF spectrograms.py:817-852] on the high-passed rows, (frames, rows): every row divided by the largest
    value of the whole matrix, the rows added in order from zero, the sum divided by their number.  ``np.max(DataFrame)``
    means different things across pandas versions (a scalar, or a per-column reduction); the reading taken here is one
    signed scalar maximum over all values.  None where that maximum is not finite or not > 0."""
    x = np.asarray(filtered, dtype=np.float64)
    m = float(np.max(x)) if x.size else float("nan")
    if not (np.isfinite(m) and m > 0.0):
        return None
    y2 = np.zeros(x.shape[0])
    for r in range(x.shape[1]):
        y2 += x[:, r] / m
    return y2 / x.shape[1]


def write_sound(folder, name: str, case: str, fs: float, filtered: np.ndarray, out=print):
    """``<name>_sound_<case>.wav``: ``scipy.io.wavfile.write(path, int(fs), y2)`` in float64, as the reference writes it; no
    file and one line where ``sound_of`` gives none."""
    from scipy.io import wavfile
    y2 = sound_of(filtered)
    if y2 is None:
        out(f"Spectrograms: the high-passed rows of {name} have no finite maximum > 0, no sound file written")
        return None
    folder = Path(folder)
    folder.mkdir(parents=True, exist_ok=True)
    path = folder / f"{name}_sound_{case}.wav"
    wavfile.write(path, int(fs), y2)
    return path


def file_names(name: str, case: str, num_windows, min_color) -> Dict[str, str]:
    """[REF create_spectrograms_chromagrams.py:192,203,214; create_spectrum.py:60]"""
    stem = f"{name}_{case}_{num_windows}_windows"
    return dict(spectrogram=f"{stem}_thresh{min_color}_spectrogram.csv", chromagram=f"{stem}_chromagram.csv", sbi=f"{stem}_SBI.csv",
                psd=f"{name}_psd_no_filter_{case}.csv")


def write_files(folder, name: str, case: str, res: dict, min_color) -> Dict[str, Path]:
    """The four CSV files, readable by whatever reads the reference's [REF create_spectrograms_chromagrams.py:197-219;
    create_spectrum.py:68-69]: comma-separated ``np.savetxt`` tables; spectrogram and chromagram under a ``# `` header line of
    the segment times with two decimals, one row per frequency / chroma class with the frequency / the class's place in
    linspace(0, 1, 24) in front; SBI as (time, SBI) rows; the spectrum as (frequency, log power) rows."""
    folder = Path(folder)
    folder.mkdir(parents=True, exist_ok=True)
    paths = {k: folder / f for k, f in file_names(name, case, res["plan"]["num_windows"], min_color).items()}
    times = ",".join(f"{t:.2f}" for t in res["bins"])
    classes = np.linspace(0, 1, len(res["chroma"]))
    tables = dict(spectrogram=(np.column_stack([res["freqs"], res["spectrogram"]]), times),
                  chromagram=(np.column_stack([classes, res["chroma"]]), times),
                  sbi=(np.column_stack([res["bins"], res["sbi"]]), "t (s), SBI"),
                  psd=(np.column_stack([res["psd_freqs"], res["psd"]]), "Freqs(Hz),spectrum"))
    for key, (table, header) in tables.items():
        np.savetxt(paths[key], table, delimiter=",", header=header)
    return paths


# ------------------------------------------------------------------------------------------------
# the driver's side
# ------------------------------------------------------------------------------------------------

def spectrogram_refusal(v: dict, world: int, backend_cls) -> str:
    """Why ``--spectrogram`` cannot run with the resolved parameters ``v`` ('' if it can); as ``hi_pass_refusal``."""
    quantities(v)
    o = options(v)
    if not v.get("save_step"):
        return "--spectrogram records the saved frames: it needs --save-step"
    if v.get("restart_folder"):
        why = restart_refusal(v, SpectrogramRun.key, SpectrogramRun.words)
        if why:
            return why
    if world > 1:
        return "--spectrogram runs on one rank only (WORLD_SIZE > 1)"
    if "wss" in quantities(v) and backend_cls is not None and not hasattr(backend_cls, "spec_begin_wss"):
        return f"--spectrogram wss needs a backend with spec_begin_wss ({getattr(backend_cls, '__name__', backend_cls)} has none)"
    times, past = frame_times(v, SpectrogramRun.key, SpectrogramRun.words)
    frames = len(times)
    if frames < HP_PADLEN + 1:
        split = f" ({past} saved before the restart and {frames - past} to come)" if v.get("restart_folder") else ""
        return f"--spectrogram: the run saves {frames} frames{split}, the high-pass filter needs at least padlen + 1 = {HP_PADLEN + 1}"
    T = frames * frame_spacing(v)
    plan = window_plan(frames, T, o["num_windows_per_sec"], o["overlap_frac"])
    if plan["nseg"] < 2:
        return (f"--spectrogram: {frames} frames over {T:g} s in {plan['num_windows']:g} windows (--spectrogram-num-windows-per-sec) give "
                f"segments of {plan['nperseg']} frames and {plan['nseg']} of them: a spectrogram needs at least two")
    return ""


def host_chunk(backend) -> int:
    """The column chunk of the host sessions of a backend (or backend class) without ``spec_begin``: HOST_CHUNK unless it
    names its own (``spec_host_chunk``)."""
    return int(getattr(backend, "spec_host_chunk", HOST_CHUNK))


class SpectrogramRun(SessionRun):
    """The driver's side of ``--spectrogram``: per quantity one session on the sampled nodes, one recorded frame per saved
    frame, and at the end the four files.  A backend without ``spec_begin`` records and transforms on the host - but not
    the wall shear stress, which is an error without ``spec_begin_wss``.  ``PointList`` also writes the sound file, in this
    unsplit path only: a list of points never needs strips."""
    prefix, file_stem, key = "spec", "spectrogram", "spectrogram"
    option, words = "--spectrogram", "--spectrogram cannot be used with --restart-folder"
    reads = staticmethod(fields)                    # the fields of dvp_["n"] the sessions read, from the parameters

    def __init__(self, backend, mesh: FsiMesh, ns: dict, open_sessions: bool = True):
        """``open_sessions`` False: everything but the sessions - the strips of ``spectrogram_strips`` open their own."""
        self.backend, self.mesh = backend, mesh
        self.quantities = quantities(ns)
        if "wss" in self.quantities and backend is not None and not hasattr(backend, "spec_begin_wss"):
            raise SystemExit(f"--spectrogram wss needs a backend with spec_begin_wss ({type(backend).__name__} has none)")
        self.opts = options(ns)
        self.save_deg = int(ns["save_deg"])
        self.dt_files = frame_spacing(ns)
        self.start_t = frame_start(ns)
        self.expected = expected_frames(ns)          # the frames the run saves, or a finished folder hands over
        self.folder = Path(ns["results_folder"]) / "Spectrograms"
        self.case = str(ns.get("case") or Path(ns["results_folder"]).parent.name)     # "case": the folder that was read, where the files go elsewhere
        self.sel = {q: select_nodes(mesh, self.save_deg, q, ns, self.opts) for q in self.quantities}     # an empty region ends the run here
        if open_sessions:
            self.open_sessions(backend, ns, self.begin_args,
                               lambda q, capacity: HostSpecSession(self.rows(q), capacity, host_chunk(backend)))

    def begin_args(self, q: str, r0: int = 0, r1: Optional[int] = None):
        """The arguments of the begin call before the capacity; of the wall shear stress: of its rows ``[r0, r1)``."""
        sel = self.sel[q]
        if q == "wss":
            return sel["facet_cells"], sel["facet_local"], sel["mu"], sel["dofs"][r0:r1], sel["comps"][r0:r1]
        return sel["nodes"], sel["nodes_b"], self.opts["component"]

    def begin_session(self, session, q: str, args, capacity: int) -> None:
        if q == "wss":                              # an entry point of its own: the quantity is in its name
            self.backend.spec_begin_wss(*args, capacity)
        else:
            super().begin_session(session, q, args, capacity)

    def rows(self, q: str) -> int:
        return len(self.sel[q]["ids"]) * (3 if q != "p" and self.opts["component"] == "all" else 1)

    def fingerprint(self, q: str) -> dict:
        sel = self.sel[q]
        if q == "wss":
            return dict(dt_sample=self.dt_files, component=self.opts["component"], rows=self.rows(q), mu=sel["mu"],
                        facets=sha256_of(sel["facet_cells"], sel["facet_local"]), dofs=sha256_of(sel["dofs"]), comps=sha256_of(sel["comps"]))
        return dict(save_deg=self.save_deg, dt_sample=self.dt_files, component="x" if q == "p" else self.opts["component"],
                    rows=self.rows(q), nodes=sha256_of(sel["nodes"], sel["nodes_b"]))

    def min_color(self, q: str):
        return MIN_COLOR[q] if self.opts["min_color"] is None else self.opts["min_color"]

    def _host_frame(self, q: str, state: np.ndarray) -> np.ndarray:
        d, v, p = self.mesh.split(state)
        s = self.sel[q]
        if q == "p":
            a = p[s["nodes"]]
            if s["nodes_b"] is not None:
                b = s["nodes_b"]
                a = np.where(b < 0, a, 0.5 * (a + p[np.maximum(b, 0)]))
            return a
        return component_rows((d if q == "d" else v)[s["nodes"]], self.opts["component"])

    def write(self, out) -> None:
        n = self.frames
        T = n * self.dt_files
        plan = window_plan(n, T, self.opts["num_windows_per_sec"], self.opts["overlap_frac"]) if n else dict(nseg=0)
        if n <= HP_PADLEN or plan["nseg"] < 2:
            out(f"Spectrograms: {n} frames recorded, too few for the high-pass filter (more than {HP_PADLEN}) and two segments: "
                "nothing written")
            return
        for q, session in self.sessions.items():
            res = pipeline(session, self.rows(q), n, T, self.start_t, self.opts, self.min_color(q))
            write_files(self.folder, self.sel[q]["name"], self.case + self.sel[q]["case_suffix"], res, self.min_color(q))
            if self.opts["sampling"] == "PointList":      # the rows are few: fetched, and added on the host
                hp = highpass_design(res["fs"], self.opts["lowcut"])
                session.filter(hp["b"], hp["a"], hp["zi"], hp["padlen"])
                filtered = np.stack([np.asarray(session.fetch(k, True)).reshape(-1) for k in range(n)])
                session.filter()
                write_sound(self.folder, self.sel[q]["name"], self.case + self.sel[q]["case_suffix"], res["fs"], filtered, out)
        out(f"Spectrograms of {n} frames ({', '.join(self.quantities)}; {self.opts['sampling']}, "
            f"{', '.join(str(self.rows(q)) for q in self.quantities)} rows) written to {self.folder}")
