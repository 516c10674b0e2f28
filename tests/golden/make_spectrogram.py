"""Writes tests/golden/spectrogram/chroma.npz: what the reference's own chroma filter bank gives for two (fs, n_fft) pairs,
the chromagram and the spectral bandedness index made of it as the reference makes them (``np.dot``, columns normalised to sum
1, one minus the normalised entropy), each with the spectrogram it was applied to, and the window count / segment length /
FFT length for a handful of (frames, seconds).  Recorded results only.

Only the filter bank comes out of a reference function.  The window arithmetic (``plans``) does not: the reference computes
it inside ``create_spectrogram_composite`` and ``get_spectrogram``, which cannot be loaded without h5py, pandas and
matplotlib, so this script states their three lines again (``round(per_sec T) + 3``, ``1 << (int(n / windows) -
1).bit_length()``, ``int(frac nperseg)``, twice nperseg) independently of vasp_amd.  The test that reads ``plans`` therefore
compares two readings of the reference, not the reference itself; it guards the arithmetic against drifting.  The filter bank is the reference's ``chroma_filters.py``, which needs nothing but NumPy; it is loaded by path:

    python tests/golden/make_spectrogram.py <reference tree>/src/vasp/postprocessing/postprocessing_h5py/chroma_filters.py
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np

# (sampling rate, n_fft, segments)
PAIRS = ((1000.0, 512, 9), (2944.2, 128, 5))
# (frames, seconds, windows per second, overlap fraction)
PLANS = ((1501, 1.501, 4, 0.75), (2944, 0.951, 4, 0.75), (400, 0.4, 4, 0.75), (10000, 2.0, 4, 0.5), (41, 0.041, 4, 0.75), (700, 0.7, 10, 0.9))


def spectrum(fs: float, n_fft: int, nseg: int, seed: int) -> np.ndarray:
    """A positive (n_fft / 2 + 1, nseg) spectrogram: a 1 / f floor, two drifting lines, seven decades between peak and floor."""
    rng = np.random.default_rng(seed)
    f = np.fft.rfftfreq(n_fft, 1 / fs)[:, None]
    k = np.arange(nseg)[None, :]
    lines = np.exp(-0.5 * ((f - (0.11 + 0.01 * k) * fs) / (0.01 * fs)) ** 2) + 0.3 * np.exp(-0.5 * ((f - (0.27 - 0.005 * k) * fs) / (0.02 * fs)) ** 2)
    return (1e-7 / (1.0 + f) + lines) * np.exp(0.2 * rng.standard_normal((len(f), nseg)))


def main(path: str):
    spec = importlib.util.spec_from_file_location("chroma_filters", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for i, (fs, n_fft, nseg) in enumerate(PAIRS):
        fb = mod.chroma_filterbank(sr=fs, n_fft=n_fft, tuning=0.0, n_chroma=24, ctroct=5, octwidth=2)
        P = spectrum(fs, n_fft, nseg, 40 + i)
        chroma = np.dot(fb, P)
        chroma = chroma / np.sum(chroma, axis=0)
        entropy = -np.sum(chroma * np.log(chroma), axis=0) / np.log(24)
        out.update({f"fb{i}": fb, f"P{i}": P, f"chroma{i}": chroma, f"sbi{i}": 1 - entropy})
    plans = []
    for n, T, per_sec, frac in PLANS:
        num_windows = np.round(per_sec * T) + 3
        nperseg = 1 << (int(n / num_windows) - 1).bit_length()
        plans.append((n, T, per_sec, frac, num_windows, nperseg, int(frac * nperseg), 2 * nperseg))
    out["plans"] = np.array(plans, dtype=np.float64)
    dst = Path(__file__).resolve().parent / "spectrogram" / "chroma.npz"
    dst.parent.mkdir(exist_ok=True)
    np.savez_compressed(dst, **out)
    print(dst, dst.stat().st_size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
