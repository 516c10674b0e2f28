"""Writes tests/golden/hi_pass/filtfilt.npz: generated rows (a slow carrier, a tone three decades below it, noise), the
order-5 Butterworth coefficients scipy designed for them and ``scipy.signal.filtfilt`` of every row, for the parameter sets
of tests/test_hi_pass.py.  The stored results equal the NumPy restatement (vasp_amd/hi_pass.py) bit for bit; the test holds
the restatement to them with the stored coefficients, so it bites whatever scipy is installed.

    python tests/golden/make_hi_pass.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

# (time between frames, lowcut, highcut, frames)
CASES = ((1e-4, 25.0, 1000.0, 1500), (3.3964e-4, 25.0, 1000.0, 400), (1e-3, 25.0, 1000.0, 64), (1e-3, 0.0, 200.0, 40),
         (3.3964e-4, 0.05, 500.0, 120))
ROWS = 4


def rows(dt: float, n: int, seed: int) -> np.ndarray:
    """(n, ROWS) frame-major: carrier 1e-3 at 1.2 Hz, a tone of 1e-6 at 180 + 30 r Hz, noise of 1e-8."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) * dt
    return np.stack([1e-3 * np.sin(2 * np.pi * 1.2 * t + r) + 1e-6 * np.sin(2 * np.pi * (180 + 30 * r) * t + 0.3 * r)
                     + 1e-8 * rng.standard_normal(n) for r in range(ROWS)], axis=1)


def main():
    from scipy.signal import filtfilt
    from vasp_amd.hi_pass import design, filtfilt_rows
    out = {}
    for i, (dt, lo, hi, n) in enumerate(CASES):
        prm = design(dt, lo, hi)
        x = rows(dt, n, 100 + i)
        y = np.stack([filtfilt(prm["b"], prm["a"], x[:, r]) for r in range(ROWS)], axis=1)
        assert np.array_equal(y, filtfilt_rows(prm["b"], prm["a"], x, prm["zi"], prm["padlen"])), (dt, lo, hi)
        out.update({f"x{i}": x, f"y{i}": y, f"b{i}": prm["b"], f"a{i}": prm["a"], f"zi{i}": prm["zi"]})
    path = Path(__file__).resolve().parent / "hi_pass" / "filtfilt.npz"
    path.parent.mkdir(exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
