"""Writes tests/golden/tke/compute_tke.npz: generated velocities (a pulsatile mean with the cycle's period, a fluctuation two
decades below it; one -0.0, one row with a NaN and one with an inf) and what the reference's own ``compute_tke`` and
``compute_average_over_cycles`` (src/vasp/postprocessing/log_plotter.py of a VaSP checkout) return for them, for the
(period, cycles) of tests/test_hi_pass_phase.py and for a start / end cycle range inside a longer record.  The test holds the
NumPy twin of the device (vasp_amd/hi_pass.py: HostBandSession.phase / phase_fetch) to the stored results bit for bit.

    python tests/golden/make_tke.py <VaSP checkout>
"""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np

CASES = ((4, 3), (1, 5), (5, 1), (3, 11))       # (period, cycles)
RANGE = (4, 6, 2, 4)                            # period, recorded cycles, start cycle, end cycle (1-based, inclusive)
NODES = 5


def velocities(period: int, cycles: int, seed: int) -> np.ndarray:
    """(cycles * period, NODES, 3), frame-major."""
    rng = np.random.default_rng(seed)
    n = cycles * period
    phase = 2 * np.pi * (np.arange(n) % period) / period
    u = 0.3 * np.sin(phase)[:, None, None] * rng.uniform(0.5, 1.5, (1, NODES, 3)) + 3e-3 * rng.standard_normal((n, NODES, 3))
    u[0, 0, 0] = -0.0
    u[n // 2, 1, 1] = np.nan
    u[n - 1, 2, 2] = np.inf
    return u


def load_log_plotter(checkout: Path):
    """The reference's module by its path; matplotlib, which it imports for its figures, need not be installed."""
    try:
        import matplotlib.pyplot  # noqa: F401
    except ImportError:
        for name in ("matplotlib", "matplotlib.pyplot", "matplotlib.axes"):
            sys.modules[name] = types.ModuleType(name)
        sys.modules["matplotlib.axes"].Axes = object
    spec = importlib.util.spec_from_file_location("log_plotter", checkout / "src" / "vasp" / "postprocessing" / "log_plotter.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def reference(lp, u: np.ndarray, period: int, start=None, end=None) -> dict:
    """compute_tke per node, as the reference is handed its probe points, stacked back to [frame][node]; then
    compute_average_over_cycles of the [frame][node] energies of the cycles in range, and their mean over the frames."""
    probes = {i: {"velocity": np.ascontiguousarray(u[:, i])} for i in range(u.shape[1])}
    res = lp.compute_tke(probes, period, start, end)
    mean = np.stack([res[i][0] for i in range(u.shape[1])], axis=1)
    fluct = np.stack([res[i][1] for i in range(u.shape[1])], axis=1)
    tke = np.stack([res[i][2] for i in range(u.shape[1])], axis=1)
    c0 = 1 if start is None else start
    c1 = len(u) // period if end is None else end
    in_range = np.ascontiguousarray(tke[(c0 - 1) * period:c1 * period])
    cycle_mean = lp.compute_average_over_cycles(in_range, period).reshape(period, u.shape[1])
    return dict(mean=mean, fluct=fluct, tke=tke, tke_cycle_mean=cycle_mean, tke_time_mean=np.mean(in_range, axis=0))


def main():
    lp = load_log_plotter(Path(sys.argv[1]))
    out = {}
    with np.errstate(all="ignore"):
        for i, (period, cycles) in enumerate(CASES):
            u = velocities(period, cycles, 200 + i)
            out[f"u{i}"] = u
            out.update({f"{k}{i}": v for k, v in reference(lp, u, period).items()})
        period, cycles, start, end = RANGE
        u = velocities(period, cycles, 300)
        out["u_range"] = u
        out.update({f"{k}_range": v for k, v in reference(lp, u, period, start, end).items()})
    path = Path(__file__).resolve().parent / "tke" / "compute_tke.npz"
    path.parent.mkdir(exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
