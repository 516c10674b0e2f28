"""Writes tests/golden/hi_pass/cell_twin_bits.npz: seeded P2 fields on 7 tetrahedra and what the NumPy twins of the cell kernels
(vasp_amd/hi_pass.py: ``cell_rate``, ``cell_rate_current``, ``cell_vortex``, ``cell_wsum``) return for them.  The stored
results were recorded before the twins' shared pieces were merged into one (``vertex_gradients``), from the commit
"Test the wall-shear, hemodynamics and stress kernels per cell"; tests/test_hi_pass_cell_rate.py holds the twins to them bit
for bit.  Running this again records whatever the twins of the checkout give: do that only to pin a deliberate change.

    python tests/golden/make_cell_twin_bits.py

The cells: 0, 5, 6 ordinary; 1 with a NaN and 2 with an inf in w; 3 with w all zeros, every other one -0.0; 4 with a
displacement grown until exactly one of the four ``J_q`` is negative.  In every other cell every ``J_q > 0``.
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from vasp_amd import hi_pass as hp  # noqa: E402

CELLS, NAN_CELL, INF_CELL, ZERO_CELL, FOLDED_CELL = 7, 1, 2, 3, 4


def jacobians(d: np.ndarray, grad: np.ndarray) -> np.ndarray:
    """(cells, 4): det(I + D_q) at the points of the degree-2 interior rule, in plain NumPy (for choosing the inputs only)."""
    D = np.array(hp.vertex_gradients(d, grad)).transpose(3, 0, 1, 2)                    # (cells, 4, 3, 3)
    Dq = hp.RULE_B * D.sum(axis=1, keepdims=True) + (hp.RULE_A - hp.RULE_B) * D
    return np.linalg.det(np.eye(3) + Dq)


def inputs():
    rng = np.random.default_rng(20261020)
    rows = np.eye(3) + 0.3 * rng.standard_normal((CELLS, 3, 3))                          # the gradients of L_1 .. L_3
    grad = np.concatenate([-((rows[:, :1] + rows[:, 1:2]) + rows[:, 2:3]), rows], axis=1)
    w = rng.standard_normal((CELLS, 10, 3))
    d = 0.01 * rng.standard_normal((CELLS, 10, 3))
    weights = rng.uniform(0.5, 2.0, CELLS)
    w[NAN_CELL, 6, 1] = np.nan
    w[INF_CELL, 2, 0] = np.inf
    w[ZERO_CELL] = np.where(np.arange(30).reshape(10, 3) % 2 == 0, 0.0, -0.0)
    shape = rng.standard_normal((10, 3))
    for scale in np.arange(0.05, 5.0, 0.05):
        d[FOLDED_CELL] = scale * shape
        if (jacobians(d, grad)[FOLDED_CELL] < 0).sum() == 1:
            break
    J = jacobians(d, grad)
    assert (J[FOLDED_CELL] < 0).sum() == 1 and (np.delete(J, FOLDED_CELL, axis=0) > 0).all()
    return w, d, grad, weights


def main():
    w, d, grad, weights = inputs()
    with np.errstate(all="ignore"):
        rate = hp.cell_rate(w, grad)
        rate_current, volume_ratio, min_jacobian = hp.cell_rate_current(w, d, grad)
        vortex = hp.cell_vortex(w, grad)
        finite = np.isfinite(vortex).all(axis=0)
        out = dict(w=w, d=d, grad=grad, weights=weights, rate=rate, rate_current=rate_current, volume_ratio=volume_ratio,
                   min_jacobian=min_jacobian, vortex=vortex, wsum=hp.cell_wsum(vortex, weights),
                   wsum_finite=hp.cell_wsum(vortex[:, finite], weights[finite]))
    assert min_jacobian[FOLDED_CELL] < 0 and (np.delete(min_jacobian, FOLDED_CELL) > 0).all()
    assert np.isnan(rate[NAN_CELL]) and not np.isfinite(rate[INF_CELL]) and not rate[ZERO_CELL]
    path = Path(__file__).resolve().parent / "hi_pass" / "cell_twin_bits.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")
    for k in ("rate", "rate_current", "volume_ratio", "min_jacobian", "wsum", "wsum_finite"):
        print(k, out[k])


if __name__ == "__main__":
    main()
