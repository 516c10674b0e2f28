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
* the writer of the reference's files and the driver's side of ``--hi-pass`` (``HiPassRun``).

Not done: the reference's ``strain`` / ``stress`` quantities, its ``multiband`` mode, ``--stride`` and the point traces.
"""
from __future__ import annotations

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


def design(time_between_files: float, lowcut: float, highcut: float) -> dict:
    """``band_parameters`` plus b, a [REF spectrograms.py:516-529], ``zi = lfilter_zi(b, a)`` and filtfilt's default
    ``padlen = 3 max(len(a), len(b))``."""
    from scipy.signal import butter, lfilter_zi
    prm = band_parameters(time_between_files, lowcut, highcut)
    nyq = 0.5 * prm["fs"]
    low, high = prm["lowcut"] / nyq, prm["highcut"] / nyq
    if prm["btype"] == "lowpass":
        b, a = butter(ORDER, high, btype="lowpass")
    else:
        b, a = butter(ORDER, [low, high], btype="bandpass")
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

    def end(self) -> None:
        pass


class HostBandSession(HostHistory):
    """The session of one quantity on the host, method for method ``HipBackend.hi_pass_*`` without the quantity argument:
    for a backend that has no device session."""
    what = "hi-pass"

    def __init__(self, ncomp: int, capacity: int):
        super().__init__((-1, ncomp), capacity)
        self.ncomp, self.amp = ncomp, None

    def sample(self, frame: np.ndarray) -> None:
        super().sample(frame)
        self.amp = None

    def filter(self, b, a, zi, padlen: int) -> None:
        super().filter(b, a, zi, padlen)
        self.amp = None

    def amplitude(self, window: int) -> None:
        self.amp = self.filtered if window == 0 else windowed_rms_running(self.filtered, window)

    def fetch(self, what: str, frame: int, with_max: bool = False):
        if what == "raw":
            return self.raw[frame]
        if what == "filtered":
            return self.filtered[frame]
        mag = amplitude_magnitude(self.amp[frame])
        out = mag if what == "magnitude" else self.amp[frame]
        return (out, float(mag.max()), int(np.argmax(mag))) if with_max else out


class DeviceSession:
    """``HipBackend.<prefix>_*`` of one quantity behind the host session's method names."""

    def __init__(self, backend, prefix: str, q: str):
        self.backend, self.prefix, self.q = backend, prefix, q

    def __getattr__(self, name: str):
        call = getattr(self.backend, f"{self.prefix}_{name}")
        return lambda *args: call(self.q, *args)


class SessionRun:
    """What the driver's sides of ``--hi-pass`` and ``--spectrogram`` share: per quantity one session, on the device or, for a
    backend without ``<prefix>_begin``, on the host; one recorded frame per saved frame; every session ended after ``write``."""
    prefix = ""

    def open_sessions(self, backend, ns: dict, begin_args, host_session) -> None:
        """``begin_args(q)``: the device session's arguments before the capacity; ``host_session(q, capacity)``: its host twin."""
        self.device = hasattr(backend, self.prefix + "_begin")
        self.frames = 0
        self.sessions = {}
        capacity = expected_frames(ns) + 1
        for q in self.quantities:
            if self.device:
                self.sessions[q] = DeviceSession(backend, self.prefix, q)
                self.sessions[q].begin(*begin_args(q), capacity)
            else:
                self.sessions[q] = host_session(q, capacity)

    def sample(self, t: float, state) -> None:
        """Record dvp_["n"]; ``state``: a callable giving the host copy, used only without the device session."""
        for q, s in self.sessions.items():
            s.sample() if self.device else s.sample(self._host_frame(q, state()))
        self.frames += 1

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


def expected_frames(v: dict) -> int:
    """Frames the time loop of ``monolithic`` saves with these parameters (``while t <= T + dt / 10``, a frame when
    ``counter % save_step == 0``)."""
    dt, T, step = float(v["dt"]), float(v["T"]), int(v["save_step"])
    t, counter, n = float(v.get("t", 0.0)), int(v.get("counter", 0)), 0
    while t <= T + dt / 10:
        t += dt
        n += counter % step == 0
        counter += 1
    return n


def hi_pass_refusal(v: dict, world: int, backend_cls) -> str:
    """Why ``--hi-pass`` cannot run with the resolved parameters ``v`` ('' if it can)."""
    quantities(v)
    if not v.get("save_step"):
        return "--hi-pass records the saved frames: it needs --save-step"
    if v.get("restart_folder"):
        return "--hi-pass does not carry its history through a checkpoint: it cannot be used with --restart-folder"
    if world > 1:
        return "--hi-pass runs on one rank only (WORLD_SIZE > 1)"
    frames = expected_frames(v)
    for lo, hi in bands(v):
        if frames < padlen_of(lo) + 1:
            return (f"--hi-pass: the run saves {frames} frames, the filter of band {lo:g} - {hi:g} Hz needs at least "
                    f"padlen + 1 = {padlen_of(lo) + 1}")
    window = int(v.get("hi_pass_window") or 250)
    if window < 1:
        return "--hi-pass-window must be at least 1"
    if v.get("hi_pass_amplitude") and frames < window:
        return f"--hi-pass-amplitude: the run saves {frames} frames, fewer than the window of {window} (--hi-pass-window)"
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


class HiPassRun(SessionRun):
    """The driver's side of ``--hi-pass``: one session per quantity on the Visualization writer's nodes, one recorded frame
    per saved frame, and at the end per band the filtered series, with ``--hi-pass-amplitude`` its amplitude and table.
    Times in the files are ``k * time_between_files + 0.0``, the reference's default start time; ``time_between_files`` is
    dt * save_step, the spacing of the frames (the reference takes dt * stride and notes the doubt, :621-634)."""
    prefix = "hi_pass"

    def __init__(self, backend, mesh: FsiMesh, ns: dict):
        from .output import refine_topology
        self.backend, self.mesh = backend, mesh
        self.save_deg = int(ns["save_deg"])
        self.quantities = quantities(ns)
        self.bands = bands(ns)
        self.amplitude = bool(ns.get("hi_pass_amplitude"))
        self.window = int(ns.get("hi_pass_window") or 250)
        self.dt_files = float(ns["dt"]) * int(ns["save_step"])
        if self.save_deg >= 2:
            geometry, topology = mesh.node_coords, refine_topology(mesh)
        else:
            geometry, topology = mesh.coords, mesh.tets
        self.writer = HiPassWriter(Path(ns["results_folder"]) / "Visualization_hi_pass", geometry, topology)
        self.open_sessions(backend, ns, lambda q: output_nodes(mesh, self.save_deg, q),
                           lambda q, capacity: HostBandSession(1 if q == "p" else 3, capacity))

    def _host_frame(self, q: str, state: np.ndarray) -> np.ndarray:
        d, v, p = self.mesh.split(state)
        V = self.mesh.num_vertices
        if q == "p":
            if self.save_deg >= 2:
                e = self.mesh.edges
                p = np.concatenate([p, 0.5 * (p[e[:, 0]] + p[e[:, 1]])])
            return p[:, None]
        f = d if q == "d" else v
        return f if self.save_deg >= 2 else f[:V]

    def write(self, out) -> None:
        n = self.frames
        for q, session in self.sessions.items():
            ncomp = 1 if q == "p" else 3
            for lo, hi in self.bands:
                prm = design(self.dt_files, lo, hi)
                viz = f"{VIZ_TYPE[q]}_{prm['name']}"
                if n <= prm["padlen"]:
                    out(f"Hi-pass {viz}: {n} frames recorded, the filter needs more than {prm['padlen']}: nothing written")
                    continue
                session.filter(prm["b"], prm["a"], prm["zi"], prm["padlen"])
                self.writer.write_series(viz, (session.fetch("filtered", k) for k in range(n)), n, ncomp, self.dt_files, 0.0)
                if not self.amplitude:
                    continue
                lowpass = prm["btype"] == "lowpass"
                if not lowpass and n < self.window:
                    out(f"Hi-pass {viz}: {n} frames recorded, fewer than the window of {self.window}: no amplitude written")
                    continue
                session.amplitude(0 if lowpass else self.window)
                table = np.empty((n, 13))

                def amp_frames():
                    for k in range(n):
                        amp, mx, am = session.fetch("amplitude", k, True)
                        table[k] = amplitude_row(k * self.dt_files + 0.0, amplitude_magnitude(amp), mx, am)
                        yield amp

                self.writer.write_series(f"{viz}_amplitude", amp_frames(), n, ncomp, self.dt_files, 0.0)
                self.writer.write_table(viz, table)
        out(f"Hi-pass fields of {n} frames ({', '.join(self.quantities)}) written to {self.writer.folder}")
