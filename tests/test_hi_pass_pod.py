"""The snapshot proper orthogonal decomposition under ``--hi-pass-pod``, host side: the NumPy twin of csrc/fsi_pod.hip
(``pod_gram``, ``pod_modes``, ``HostBandSession.pod_gram`` / ``pod_modes`` / ``pod_fetch``) against a restatement in
``numpy.longdouble``; the one eigen step (``pod_eig``, ``pod_table``) on a planted structure; the lumped volumes; the options and
their refusals; the twin's ladder; the driver's files on the host backend; the C-ABI's new entry points.

The quantities, as include/vaspfsi.h defines them: m[r] the ordered mean of row r over the n frames, a double; y_j = x_j - m,
a_j = w y_j, G_ij = sum_r a_i[r] y_j[r], Phi_m[r] = sum_j T[j][m] y_j[r].  The restatement (``pod_reference``) takes the
doubles x, m, w and T as given and forms y, a, G and Phi in ``numpy.longdouble``.  With u = 2^-53 and
gamma(k) = k u / (1 - k u), the error of k roundings compounded (Higham, Accuracy and Stability, lemma 3.1):

* the mean (``mean_bound``): n - 1 additions and one division, n roundings: |m - mean(x)| <= gamma(n) sum_j |x_j[r]| / n;
* a Gram entry (``gram_bound``): a term a_i[r] y_j[r] carries the roundings of y_i, of a_i = w y_i, of y_j and of the product,
  four; a term then goes through the additions of its slab, at most min(R, POD_SLAB) - 1 whatever their order, and through one
  addition per slab, ``slabs`` of them (the first onto +0.0).  With k = R + slabs + 4 >= 4 + min(R, POD_SLAB) - 1 + slabs:

      |G_ij - G_ij(exact)| <= gamma(R + slabs + 4) sum_r |a_i[r] y_j[r]|

  This holds for the twin (BLAS inside a slab), for the device (the matrix pipe, four rows at a time) and between the two
  (twice it: either side);
* a mode value (``mode_bound``): y_j and the product, two roundings, and n - 1 additions in any order:

      |Phi_m[r] - Phi_m[r](exact)| <= gamma(n + 1) sum_j |T[j][m] y_j[r]|

The sums of magnitudes are formed in double from the restatement's y and a (their own rounding, a relative 1e-16 k, is covered
by the factor 1 + 1e-9 on every bound).  Nothing is tuned to what the code gives; the tests print the largest share of each
bound that is used.

The planted structure and the orthonormality check build their tolerances from quantities the test computes in extended
precision; they are derived at the tests.
"""
import argparse
import contextlib
import io
import re

import numpy as np
import pytest

from conftest import ROOT
from test_session_restart import CYL, _run, one_modification_time  # noqa: F401  (the fixture holds h5lite's clock)
from vasp_amd import hi_pass as hp

U = 2.0 ** -53
LD = np.longdouble
SLACK = 1.0 + 1e-9


def gamma(k) -> float:
    return k * U / (1.0 - k * U)


# ---- helpers shared with tests/test_gpu_hi_pass_pod.py ------------------------------------------------------------------

def pod_rows(n, shape, seed=3, mean=2.0):
    """(n,) + shape: per row a mean of its own, five coherent structures of decaying energy and white noise of 1e-3."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / max(n, 1)
    x = mean * rng.uniform(0.5, 1.5, shape)[None] + 1e-3 * rng.standard_normal((n,) + tuple(shape))
    for k in range(5):
        c = np.cos(2 * np.pi * (k + 1) * t + rng.uniform(0, 2 * np.pi)) * 0.5 ** k
        x = x + c.reshape((n,) + (1,) * len(shape)) * rng.standard_normal(shape)[None]
    return x


def node_weights(nodes, seed=1):
    """Non-uniform weights with a zero among them."""
    w = np.random.default_rng(seed).uniform(0.25, 1.75, nodes)
    w[nodes // 2] = 0.0
    return w


def row_weights(weights, x):
    """The weight of every row of a frame of x (n, nodes, ncomp), flat; None: ones."""
    rows = int(np.prod(x.shape[1:]))
    return np.ones(rows) if weights is None else np.repeat(np.asarray(weights, dtype=np.float64), rows // x.shape[1])


def pod_reference(x, weights, mean, T=None):
    """The module docstring's restatement in ``numpy.longdouble`` from the doubles x (n, nodes, ncomp), weights, mean and T:
    ``G``, ``absG`` = sum_r |a_i y_j| (double), and with T ``modes`` (m, rows) and ``absmodes`` = sum_j |T y| (double)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    y = x.reshape(n, -1).astype(LD) - np.asarray(mean, dtype=np.float64).reshape(-1).astype(LD)[None]
    a = y if weights is None else row_weights(weights, x).astype(LD)[None] * y
    out = dict(G=np.dot(a, y.T), absG=np.abs(a).astype(np.float64) @ np.abs(y).astype(np.float64).T, y=y, a=a)
    if T is not None:
        T = np.asarray(T, dtype=np.float64)
        out.update(modes=np.dot(T.T.astype(LD), y), absmodes=np.abs(T.T) @ np.abs(y).astype(np.float64))
    return out


def mean_bound(x):
    n = len(x)
    return SLACK * gamma(n) * np.abs(x).sum(axis=0) / n


def gram_bound(ref, rows, sides=1):
    """``sides`` 2: between two evaluations that both round."""
    slabs = -(-rows // hp.POD_SLAB)
    return SLACK * sides * gamma(rows + slabs + 4) * ref["absG"]


def mode_bound(ref, n, sides=1):
    return SLACK * sides * gamma(n + 1) * ref["absmodes"]


def share(diff, bound) -> float:
    diff, bound = np.asarray(diff, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(diff == 0, 0.0, diff / bound))) if diff.size else 0.0


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[a == 0]), np.signbit(b[b == 0]))


def _session(x, ncomp=3, capacity=None):
    s = hp.HostBandSession(ncomp, capacity or len(x))
    s.import_(x)
    return s


# ---- the twin against extended precision ----------------------------------------------------------------------------------

# (frames, nodes): 2051 nodes of a vector are 6153 rows, a second slab of nine
CASES = ((2, 1), (7, 43), (50, 130), (65, 2051))


@pytest.mark.parametrize("weighted", (False, True), ids=("null", "weights"))
@pytest.mark.parametrize("n,nodes", CASES, ids=[f"n{n}r{3 * k}" for n, k in CASES])
def test_twin_against_extended_precision(n, nodes, weighted):
    x = pod_rows(n, (nodes, 3), seed=n + nodes)
    w = node_weights(nodes) if weighted and nodes > 1 else (np.array([0.75]) if weighted else None)
    rows = 3 * nodes
    G, mean = hp.pod_gram(x, w)
    assert G.shape == (n, n) and mean.shape == (nodes, 3) and same_bits(G, G.T)
    exact = x.astype(LD).sum(axis=0) / LD(n)
    dm = np.abs(mean.astype(LD) - exact).astype(np.float64)
    assert (dm <= mean_bound(x)).all()
    eig = hp.pod_eig(G, rows, min(n, 8))
    T = hp.pod_table(eig)
    assert T.shape[1] >= 1 and eig["resolved"][:T.shape[1]].all()
    ref = pod_reference(x, w, mean, T)
    dG = np.abs(G.astype(LD) - ref["G"]).astype(np.float64)
    bG = gram_bound(ref, rows)
    assert (dG <= bG).all()
    modes = hp.pod_modes(x, mean, T)
    assert modes.shape == (T.shape[1], nodes, 3)
    dP = np.abs(modes.reshape(len(modes), -1).astype(LD) - ref["modes"]).astype(np.float64)
    bP = mode_bound(ref, n)
    assert (dP <= bP).all()
    print(f"n = {n}, rows = {rows}, {'weights' if weighted else 'null'}: largest share of the bound, mean {share(dm, mean_bound(x)):.3g}, "
          f"G {share(dG, bG):.3g}, modes {share(dP, bP):.3g}; {T.shape[1]} resolved modes")
    # the session forms the same bits
    s = _session(x)
    s.pod_gram("raw", w)
    s.pod_modes(T)
    assert same_bits(s.pod_fetch("gram"), G) and same_bits(s.pod_fetch("mean"), mean)
    assert all(same_bits(s.pod_fetch("mode", m), modes[m]) for m in range(len(modes)))


def test_uniform_weights_give_the_bits_of_none():
    x = pod_rows(12, (2051, 3), seed=5)
    G, mean = hp.pod_gram(x, None)
    G1, mean1 = hp.pod_gram(x, np.ones(2051))
    assert same_bits(G, G1) and same_bits(mean, mean1) and same_bits(G, G.T)
    G2, _ = hp.pod_gram(x, node_weights(2051))
    assert same_bits(G2, G2.T) and not same_bits(G2, G)
    for bad, value in ((3, -1.0), (5, np.nan), (0, np.inf)):
        w = np.ones(2051)
        w[bad] = value
        with pytest.raises(RuntimeError, match=f"the weight of node {bad} is .*: a weight is >= 0 and finite"):
            hp.pod_gram(x, w)


# ---- a planted structure --------------------------------------------------------------------------------------------------

def _orthonormal(vectors, inner):
    """Gram-Schmidt, twice, in ``numpy.longdouble`` under the inner product ``inner``."""
    out = []
    for v in vectors:
        v = v.astype(LD)
        for _ in range(2):
            for q in out:
                v = v - inner(q, v) * q
        out.append(v / np.sqrt(inner(v, v)))
    return out


def _planted(n=24, nodes=400, seed=11):
    """x = mean + sum_m c_m(j) Phi_m: three modes orthonormal in the w inner product, coefficient vectors orthogonal to each
    other and to the constant, of squared lengths 4 : 2 : 1 - everything in ``numpy.longdouble``, x rounded to double."""
    rng = np.random.default_rng(seed)
    w = node_weights(nodes, seed)
    wr = np.repeat(w, 3).astype(LD)
    Phi = _orthonormal(list(rng.standard_normal((3, 3 * nodes))), lambda a, b: (wr * a * b).sum())
    ones = np.ones(n)
    Q = _orthonormal([ones] + list(rng.standard_normal((3, n))), lambda a, b: (a * b).sum())[1:]
    E = np.array([4.0, 2.0, 1.0], dtype=LD) * LD(0.37)
    C = np.stack([np.sqrt(E[m]) * Q[m] for m in range(3)], axis=1)                  # (n, 3)
    mean = rng.uniform(0.5, 1.5, 3 * nodes).astype(LD)
    Yp = np.dot(C, np.stack(Phi))                                                   # (n, rows), exact fluctuation
    x = (mean[None] + Yp).astype(np.float64).reshape(n, nodes, 3)
    return dict(x=x, w=w, wr=wr, Phi=np.stack(Phi), Q=np.stack(Q, axis=1), E=E, Gp=np.dot(C, C.T), Yp=Yp, n=n, nodes=nodes)


def _sign_rule(v):
    return v if v[np.argmax(np.abs(v))] > 0 else -v


def test_a_planted_structure_comes_back():
    """Eigenvalues by Weyl, modes by Davis-Kahan.  With dG = ||G - G_p||_F (G_p the planted Gram matrix, in extended precision),
    res_m = ||G v_m - lam_m v_m||_2 of the host's eigh (so an exact eigenvalue of G lies within res_m of lam_m) and gap the
    smallest distance between two planted eigenvalues, zero included:

      |lam_m - E_m| <= dG + res_m                                            (Weyl)
      sin theta(v_m, q_m) <= s_m = (dG + res_m) / (gap - dG - res_m)          (Davis-Kahan)

    The computed mode is Y^T v_m / sigma_m + e with Y = Y_p + dY the doubles y_j against the planted fluctuation and |e| within
    the mode bound.  Y_p^T v_m = Phi_p^T diag(sqrt E) Q^T v_m, and the w norm of Phi_p^T z is |z|, so in the w norm

      ||Phi_m - Phi_p,m||_w <= max_c |sqrt(E_m) c / sigma_m - 1| + sqrt(E_1) s_m / sigma_m + ||dY||_w,F / sigma_m + ||bound||_w

    with c between sqrt(1 - s_m^2) and 1, ||dY||_w,F^2 = sum_j ||dy_j||_w^2.  Every term is computed here, in extended
    precision; none is a constant."""
    p = _planted()
    x, w, n, rows = p["x"], p["w"], p["n"], 3 * p["nodes"]
    G, mean = hp.pod_gram(x, w)
    eig = hp.pod_eig(G, rows, 8)
    lam, V = eig["lam"], eig["V"]
    assert list(eig["resolved"]) == [True] * 3 + [False] * 5                         # modes 4 and above fall under the floor
    dG = float(np.sqrt(((G.astype(LD) - p["Gp"]) ** 2).sum()))
    E = p["E"].astype(np.float64)
    gap = float(min(E[0] - E[1], E[1] - E[2], E[2]))
    T = hp.pod_table(eig)
    assert T.shape == (n, 3)
    modes = hp.pod_modes(x, mean, T).reshape(3, -1)
    ref = pod_reference(x, w, mean, T)
    bound_w = np.sqrt((p["wr"][None] * mode_bound(ref, n).astype(LD) ** 2).sum(axis=1)).astype(np.float64)
    dY = ref["y"] - p["Yp"]
    dY_w = float(np.sqrt((p["wr"][None] * dY * dY).sum()))
    for m in range(3):
        res = float(np.sqrt(((np.dot(G.astype(LD), V[:, m].astype(LD)) - LD(lam[m]) * V[:, m].astype(LD)) ** 2).sum()))
        assert gap - dG - res > 0
        tol_lam = dG + res
        assert abs(lam[m] - E[m]) <= tol_lam
        s = (dG + res) / (gap - dG - res)
        q = _sign_rule(p["Q"][:, m].astype(np.float64))
        ql, vl = p["Q"][:, m], V[:, m].astype(LD)                                     # sin theta as the part of v off q, in extended precision
        off = vl - np.dot(vl, ql) * ql
        sin = float(np.sqrt((off * off).sum() / (vl * vl).sum()))
        assert sin <= s
        sigma = float(eig["sigma"][m])
        tol = max(abs(np.sqrt(E[m]) * c / sigma - 1) for c in (np.sqrt(1 - s * s), 1.0)) + np.sqrt(E[0]) * s / sigma + dY_w / sigma + bound_w[m]
        sign = 1.0 if np.dot(q, p["Q"][:, m].astype(np.float64)) > 0 else -1.0      # the sign rule on the planted coefficients
        d = modes[m].astype(LD) - LD(sign) * p["Phi"][m]
        err = float(np.sqrt((p["wr"] * d * d).sum()))
        print(f"planted mode {m + 1}: |lam - E| = {abs(lam[m] - E[m]):.3g} <= {tol_lam:.3g}; sin theta {sin:.3g} <= {s:.3g}; "
              f"||Phi - Phi_p||_w = {err:.3g} <= {tol:.3g}")
        assert err <= tol
    assert eig["floor"] == (rows + 2) * U * eig["trace"] and (lam[3:] <= eig["floor"]).all()
    assert abs(eig["trace"] - float(E.sum())) <= np.sqrt(n) * dG + n * U * float(E.sum())
    assert hp.pod_energy_counts(eig["spectrum"], eig["trace"]) == (3, 3)              # 4/7, 6/7, 7/7


def test_modes_are_orthonormal_in_the_w_inner_product():
    """With T = V / sigma as doubles, Phi_e = sum_j T y_j exact and G_e the exact Gram matrix of the doubles y:
    Phi_e,a^T W Phi_e,b = T_a^T G_e T_b.  The computed G is within B_G (``gram_bound``) of G_e entry by entry, the computed Phi
    within B_P (``mode_bound``) of Phi_e.  So

      |Phi_a^T W Phi_b - delta_ab| <= |T_a|^T B_G |T_b|                                     the Gram bound over sigma_a sigma_b
                                    + |T_a^T G T_b - delta_ab|                              the measured residual of eigh
                                    + sum_r w (|Phi_a| B_P,b + B_P,a |Phi_b| + 3 B_P,a B_P,b)   the mode bound

    (|Phi_e| <= |Phi| + B_P gives the 3).  The middle term is what eigh, the square root and the division leave of
    V^T G V = diag(sigma^2), measured in extended precision."""
    for n, nodes, weighted in ((30, 700, True), (9, 2051, False)):
        x = pod_rows(n, (nodes, 3), seed=n)
        w = node_weights(nodes) if weighted else None
        G, mean = hp.pod_gram(x, w)
        eig = hp.pod_eig(G, 3 * nodes, n)
        T = hp.pod_table(eig)
        K = T.shape[1]
        assert 5 <= K < n                                                            # the mean is gone: at most n - 1
        modes = hp.pod_modes(x, mean, T).reshape(K, -1)
        ref = pod_reference(x, w, mean, T)
        wr = row_weights(w, x).astype(LD)
        got = np.dot(modes.astype(LD) * wr[None], modes.astype(LD).T)
        BG, BP = gram_bound(ref, 3 * nodes), mode_bound(ref, n)
        term_g = np.abs(T).T @ BG @ np.abs(T)
        term_e = np.abs(np.dot(np.dot(T.T.astype(LD), G.astype(LD)), T.astype(LD)) - np.eye(K)).astype(np.float64)
        A = np.abs(modes)
        wd = wr.astype(np.float64)
        term_p = (A * wd) @ BP.T + (BP * wd) @ A.T + 3 * (BP * wd) @ BP.T
        tol = SLACK * (term_g + term_e + term_p)
        diff = np.abs(got - np.eye(K)).astype(np.float64)
        print(f"n = {n}, {K} modes: largest |Phi_a^T W Phi_b - delta| = {diff.max():.3g}, largest share of the tolerance {share(diff, tol):.3g} "
              f"(Gram {term_g.max():.3g}, eigh {term_e.max():.3g}, modes {term_p.max():.3g})")
        assert (diff <= tol).all()


# ---- the eigen step ---------------------------------------------------------------------------------------------------------

def test_the_sign_rule_and_the_refusals_of_the_eigen_step():
    G = np.array([[2.0, 1.0], [1.0, 2.0]])                                           # eigenvectors (1, 1) and (1, -1) / sqrt 2: ties
    eig = hp.pod_eig(G, 10, 2)
    assert np.allclose(eig["lam"], [3.0, 1.0]) and eig["trace"] == 4.0 and eig["floor"] == 12 * U * 4.0
    assert eig["V"][0, 0] > 0 and eig["V"][0, 1] > 0 and eig["V"][1, 1] < 0            # on a tie the first entry decides
    assert np.allclose(np.abs(eig["V"]), np.sqrt(0.5)) and list(eig["resolved"]) == [True, True]
    assert np.allclose(hp.pod_coefficients(eig), eig["V"] * np.sqrt(eig["lam"])[None])
    x = pod_rows(9, (40, 3), seed=2)
    G, _ = hp.pod_gram(x)
    eig = hp.pod_eig(G, 120, 64)
    assert len(eig["lam"]) == 9 and (np.diff(eig["spectrum"]) <= 0).all()
    for m in range(9):
        assert eig["V"][np.argmax(np.abs(eig["V"][:, m])), m] > 0
    assert not eig["resolved"][8] and eig["resolved"][:8].all()                      # the mean took one direction
    assert hp.pod_table(eig).shape == (9, 8)
    for bad in (np.nan, np.inf):
        x[4, 7, 1] = bad
        Gb, _ = hp.pod_gram(x)
        assert not np.isfinite(Gb).any()                                             # one bad row poisons every entry
        with pytest.raises(RuntimeError, match="the Gram matrix is not finite: a recorded value is NaN or inf"):
            hp.pod_eig(Gb, 120, 3)


# ---- the lumped volumes -----------------------------------------------------------------------------------------------------

def test_volume_weights_sum_to_the_volume():
    from vasp_amd.flow_metrics import cell_volumes
    from vasp_amd.mesh import FsiMesh
    mesh = FsiMesh.read(CYL)
    vol = cell_volumes(mesh, np.arange(mesh.num_cells))
    total = float(vol.astype(LD).sum())
    for deg, count in ((1, mesh.num_vertices), (2, mesh.num_nodes)):
        w = hp.pod_volume_weights(mesh, deg)
        assert w.shape == (count,) and (w > 0).all()
        # each cell's shares and each node's sum are a few roundings: 16 of them per cell and node suffice
        assert abs(float(w.astype(LD).sum()) - total) <= 16 * U * (mesh.num_cells + count) * vol.max()
    k = int(np.argmax(vol))
    one = FsiMesh.from_arrays(mesh.coords[mesh.tets[k]], np.arange(4)[None], np.array([1]))
    w = hp.pod_volume_weights(one, 2)
    assert np.allclose(w[:4], vol[k] / 32, rtol=1e-14) and np.allclose(w[4:], 7 * vol[k] / 48, rtol=1e-14) and len(w) == 10


# ---- the options and the refusals before a run ---------------------------------------------------------------------------------

def _parameters(extra, hi_pass=("--hi-pass", "v")):
    from vasp_amd.monolithic import parameters
    with contextlib.redirect_stdout(io.StringIO()):
        return parameters(["-p", "cylinder", *hi_pass, "--verbose", "False", "-dt", "0.001", "--save-step", "1", *extra])[2]


def _refusal(extra):
    return hp.hi_pass_refusal(_parameters(extra), 1, None)


def test_each_refusal_has_its_message(tmp_path):
    on = ["--hi-pass-pod"]
    assert hp.pod_options({}) is None
    assert hp.pod_options(dict(hi_pass_pod=True)) == dict(modes=10, weights="volume")
    assert hp.pod_options(dict(hi_pass_pod=True, hi_pass_pod_modes=64, hi_pass_pod_weights="uniform")) == dict(modes=64, weights="uniform")
    assert _refusal(["-T", "0.039", *on, "--hi-pass-pod-modes", "3", "--hi-pass-pod-weights", "uniform"]) == ""
    assert "the decomposition needs at least 2" in _refusal(["-T", "0.0115", *on, "--hi-pass-start-time", "0.0115"])
    for sub in (["--hi-pass-pod-modes", "3"], ["--hi-pass-pod-weights", "uniform"]):
        with pytest.raises(SystemExit, match=f"{sub[0]} belongs to --hi-pass-pod"):
            _refusal(["-T", "0.039", *sub])
    for modes in ("0", "65"):
        with pytest.raises(SystemExit, match="--hi-pass-pod-modes must be an integer from 1 to 64"):
            _refusal(["-T", "0.039", *on, "--hi-pass-pod-modes", modes])
    with pytest.raises(SystemExit, match="--hi-pass-pod-weights must be one of volume, uniform"):
        hp.pod_options(dict(hi_pass_pod=True, hi_pass_pod_weights="mass"))
    with pytest.raises(SystemExit):                                                  # argparse knows the two
        _refusal(["-T", "0.039", *on, "--hi-pass-pod-weights", "mass"])
    assert "one rank only" in hp.hi_pass_refusal(_parameters(["-T", "0.039", *on]), 2, None)      # partitions
    from vasp_amd import monolithic, postprocess
    with pytest.raises(SystemExit, match="--hi-pass-pod needs --hi-pass with at least one of d, v, p"):
        monolithic._refuse_sessions(["-p", "cylinder", "--hi-pass-pod"], None, 1)
    with pytest.raises(SystemExit, match="--hi-pass-pod needs --hi-pass with at least one of d, v, p"):
        postprocess.prepare(["--folder", str(ROOT), "--hi-pass-pod"])
    # a history in strips of rows
    from vasp_amd.mesh import FsiMesh
    ns = dict(_parameters(["-T", "0.039", *on]), save_deg=2, results_folder=tmp_path, hi_pass_strip=(0, 8))
    with pytest.raises(SystemExit) as e:
        hp.HiPassRun(object(), FsiMesh.read(CYL), ns)
    assert str(e.value) == hp.POD_STRIPS and "strips of rows" in str(e.value) and str(e.value) != hp.SPI_STRIPS
    assert not (tmp_path / "Visualization_hi_pass").exists()


# ---- the twin's refusals and its ladder ----------------------------------------------------------------------------------------

B, A, ZI = np.array([0.25, 0.25]), np.array([1.0, -0.5]), np.array([0.75])      # a stable two-tap low-pass of gain 1 and its zi


def test_twin_refusals():
    x = pod_rows(12, (6, 3), seed=4)
    s = _session(x, capacity=13)
    for call in (lambda: s.pod_fetch("gram"), lambda: s.pod_fetch("mode", 0)):
        with pytest.raises(RuntimeError, match=r"pod_fetch: no Gram matrix \(pod_gram first\)"):
            call()
    with pytest.raises(RuntimeError, match=r"pod_modes: no Gram matrix \(pod_gram first\)"):
        s.pod_modes(np.ones((12, 1)))
    with pytest.raises(RuntimeError, match="series must be one of raw, series"):
        s.pod_gram("phase_mean")
    with pytest.raises(RuntimeError, match=r"no filtered series \(filter or phase first\)"):
        s.pod_gram("series")
    with pytest.raises(RuntimeError, match="the weight of node 2 is -1"):
        s.pod_gram("raw", [1, 1, -1, 1, np.nan, 1])
    assert s.pod_state is None                                                       # the refused calls changed nothing
    s.pod_gram("raw")
    with pytest.raises(RuntimeError, match=r"no modes \(pod_modes first\)"):
        s.pod_fetch("mode", 0)
    for T in (np.ones((12, 0)), np.ones((12, 65))):
        with pytest.raises(RuntimeError, match="needs 1 <= nmodes <= 64 modes"):
            s.pod_modes(T)
    s.pod_modes(np.ones((12, 2)))
    with pytest.raises(RuntimeError, match="mode 2 out of range, 2 modes stand"):
        s.pod_fetch("mode", 2)
    with pytest.raises(RuntimeError, match="what must be one of gram, mean, mode"):
        s.pod_fetch("energies")
    s.pod_gram("raw")                                                                # replaces the state whole, the modes included
    with pytest.raises(RuntimeError, match=r"no modes \(pod_modes first\)"):
        s.pod_fetch("mode", 0)
    s.select(0, 1, 1)
    with pytest.raises(RuntimeError, match="1 selected frames, the decomposition needs at least 2"):
        s.pod_gram("raw")
    with pytest.raises(RuntimeError, match="a strain / stress session has no proper orthogonal decomposition"):
        _session(np.zeros((8, 2, 6)), 6).pod_gram("raw")


# the call -> what it leaves of a decomposition of the raw frames and of one of the series
LADDER = {"sample": ("gone", "gone"), "import": ("gone", "gone"), "select": ("gone", "gone"),
          "filter": ("stays", "gone"), "filter_next": ("stays", "gone"), "phase": ("stays", "gone"),
          "amplitude": ("stays", "stays"), "spi": ("stays", "stays"), "cells": ("stays", "stays"), "pod_modes": ("stays", "stays"),
          "pod_gram": ("new", "new")}
LADDER_X = pod_rows(12, (8, 3), seed=20)
LADDER_CONN = np.random.default_rng(20).integers(0, 8, (2, 10))
LADDER_GRAD = np.random.default_rng(21).standard_normal((2, 4, 3))
LADDER_CALLS = {"sample": lambda s: s.sample(LADDER_X[0]),
                "import": lambda s: s.import_(LADDER_X[:1]),
                "select": lambda s: s.select(1, 5, 2),
                "filter": lambda s: s.filter(B, A, ZI, 0),
                "filter_next": lambda s: s.filter_next(B, A, ZI, 0),
                "phase": lambda s: s.phase(2),
                "amplitude": lambda s: s.amplitude(2),
                "spi": lambda s: s.spi(None, 0, 1),
                "cells": lambda s: s.cells(LADDER_CONN, LADDER_GRAD),
                "pod_modes": lambda s: s.pod_modes(np.ones((8, 1)))}


def ladder_state(s):
    """(G, mean, mode 0) of the decomposition that stands, or the refusal's text."""
    try:
        return s.pod_fetch("gram"), s.pod_fetch("mean"), s.pod_fetch("mode", 0)
    except RuntimeError as e:
        return str(e)


@pytest.mark.parametrize("source", hp.POD_SERIES)
@pytest.mark.parametrize("call", list(LADDER))
def test_the_ladder_drops_the_decomposition_with_its_source(call, source):
    s = _session(LADDER_X, capacity=13)
    s.select(2, 8, 1)
    s.filter(B, A, ZI, 0)
    s.pod_gram(source)
    s.pod_modes(np.full((8, 2), 0.5))
    before = ladder_state(s)
    assert isinstance(before, tuple)
    fate = LADDER[call][hp.POD_SERIES.index(source)]
    if call == "pod_gram":
        s.pod_gram("series" if source == "raw" else "raw")
        assert ladder_state(s).endswith("no modes (pod_modes first)") and not same_bits(s.pod_fetch("gram"), before[0])
        return
    LADDER_CALLS[call](s)
    after = ladder_state(s)
    if fate == "gone":
        assert after == "hi-pass pod_fetch: no Gram matrix (pod_gram first)"
    elif call == "pod_modes":
        assert same_bits(after[0], before[0]) and same_bits(after[1], before[1]) and not same_bits(after[2], before[2])
    else:
        assert all(same_bits(a, b) for a, b in zip(after, before))


# ---- the driver on the host backend -------------------------------------------------------------------------------------------

def _vectors(path):
    from vasp_amd.h5lite import read_h5
    g = read_h5(path)["VisualisationVector"]
    return np.stack([np.asarray(g[str(k)].data) for k in range(len(g.keys()))])


def _frames(results, name):
    return _vectors(results / "Visualization" / f"{name}.h5")


def test_driver_writes_modes_energies_and_coefficients(tmp_path):
    """40 saved frames: the decomposition of the raw frames and of the band's filtered series, five modes each."""
    options = ["--hi-pass", "v", "p", "--hi-pass-pod", "--hi-pass-pod-modes", "5"]
    ns, lines = _run(tmp_path / "case", options=options)
    results = tmp_path / "case" / "1"
    out = results / "Visualization_hi_pass"
    names = {p.name for p in out.iterdir()}
    stems = [f"{f}{band}_pod" for f in ("velocity", "pressure") for band in ("", "_25_to_1000")]
    assert {f"{s}{tail}" for s in stems for tail in ("_modes.h5", "_modes.xdmf", ".csv", "_coefficients.csv")} <= names
    assert {"velocity_25_to_1000.h5", "pressure_25_to_1000.h5"} <= names              # the bands are written as without the option
    for s in stems:
        assert any(f"Hi-pass {s}: proper orthogonal decomposition of 40 frames (volume weights), 5 of 5 modes resolved and written" in line
                   for line in lines), s
    from vasp_amd.mesh import FsiMesh
    w = hp.pod_volume_weights(FsiMesh.read(CYL), 2)
    for name, ncomp in (("velocity", 3), ("pressure", 1)):
        x = _frames(results, name)
        assert x.dtype == np.float64 and len(x) == 40
        G, mean = hp.pod_gram(x, w)
        eig = hp.pod_eig(G, x[0].size, 5)
        modes = hp.pod_modes(x, mean, hp.pod_table(eig))
        got = _vectors(out / f"{name}_pod_modes.h5")
        assert got.shape == (5, x.shape[1], ncomp) and np.array_equal(got, modes.reshape(got.shape).astype(np.float32))      # float32 of the fetched modes
        xdmf = (out / f"{name}_pod_modes.xdmf").read_text()
        assert [float(t) for t in re.findall(r'<Time Value="([^"]+)"', xdmf)] == [1, 2, 3, 4, 5]      # the time is the mode number
        header, *rows = (out / f"{name}_pod.csv").read_text().splitlines()
        k90, k99 = hp.pod_energy_counts(eig["spectrum"], eig["trace"])
        assert header == (f"# {hp.POD_COLUMNS}; frames = 40, weights = volume, trace = {eig['trace']!r}, floor = {eig['floor']!r}, "
                          f"modes for 90 % = {k90}, modes for 99 % = {k99}")
        cols = [[c.strip() for c in r.split(",")] for r in rows]
        assert [c[0] for c in cols] == ["1", "2", "3", "4", "5"] and all(len(c) == 5 and c[4] == "1" for c in cols)
        assert [float(c[1]) for c in cols] == list(eig["lam"]) and [float(c[2]) for c in cols] == list(eig["fraction"])
        assert np.allclose([float(c[3]) for c in cols], np.cumsum(eig["fraction"]), rtol=1e-15)
        coef = np.loadtxt(out / f"{name}_pod_coefficients.csv", delimiter=",")
        first = (out / f"{name}_pod_coefficients.csv").read_text().splitlines()[0]
        assert first == "# time (s), a_1, a_2, a_3, a_4, a_5" and coef.shape == (40, 6)
        assert np.array_equal(coef[:, 1:], hp.pod_coefficients(eig)) and np.allclose(coef[:, 0], np.arange(40) * 1e-3, atol=1e-15)
    # uniform weights, a window of the frames and more modes than the frames allow: clipped, with a printed line
    options = ["--hi-pass", "v", "--hi-pass-pod", "--hi-pass-pod-weights", "uniform", "--hi-pass-pod-modes", "64", "--hi-pass-start-time", "0.003"]
    ns, lines = _run(tmp_path / "view" / "case", options=options)
    results = tmp_path / "view" / "case" / "1"
    x = _frames(results, "velocity")[2:]
    assert len(x) == 38
    assert any("Hi-pass velocity_pod: --hi-pass-pod-modes 64 clipped to 37, the 38 frames less one" in line for line in lines)
    G, mean = hp.pod_gram(x)
    eig = hp.pod_eig(G, x[0].size, 37)
    got = _vectors(results / "Visualization_hi_pass" / "velocity_pod_modes.h5")
    K = int(eig["resolved"].sum())
    assert 1 <= len(got) == K and np.array_equal(got, hp.pod_modes(x, mean, hp.pod_table(eig)).astype(np.float32))
    header, *rows = (results / "Visualization_hi_pass" / "velocity_pod.csv").read_text().splitlines()
    assert "frames = 38, weights = uniform" in header and len(rows) == 37 and [r.split(",")[4].strip() for r in rows] == ["1"] * K + ["0"] * (37 - K)


def test_without_the_option_the_files_are_those_of_before(tmp_path):
    base = ["--hi-pass", "v", "--hi-pass-amplitude", "--hi-pass-window", "8", "--hi-pass-point-ids", "0"]
    from test_hi_pass_phase import _outputs
    _run(tmp_path / "without" / "case", options=base)
    _run(tmp_path / "with" / "case", options=base + ["--hi-pass-pod"])
    old, new = _outputs(tmp_path / "without" / "case" / "1"), _outputs(tmp_path / "with" / "case" / "1")
    assert set(old) < set(new) and all(new[k] == v for k, v in old.items())           # what the options of before write: not a byte changed
    added = {k.split("/")[1].split(":")[0] for k in set(new) - set(old)}
    assert added == {f"velocity{band}_pod{tail}" for band in ("", "_25_to_1000") for tail in ("_modes.h5", "_modes.xdmf", ".csv", "_coefficients.csv")}


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------

def test_header_binding_and_kernel_source_agree():
    from vasp_amd import capi
    from vasp_amd.monolithic import add_session_arguments
    header = (ROOT / "include" / "vaspfsi.h").read_text()
    lib = capi.load_library()
    for name in ("fsi_band_pod_gram", "fsi_band_pod_modes", "fsi_band_pod_fetch"):
        m = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S)
        assert m and name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
        assert header[header.rfind("/*", 0, m.start()):].startswith("/* Replaces: nothing in the reference"), name
    for k, what in enumerate(hp.POD_WHAT):
        assert re.search(r"#define FSI_POD_%s %d\b" % (what.upper(), k), header) and capi.HipBackend.POD_WHAT[what] == k
    src = (ROOT / "vasp_amd" / "csrc" / "fsi_pod.hip").read_text()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("#include")[1:][-1].lower()
    assert "fsi_pod.hip" in (ROOT / "vasp_amd" / "csrc" / "Makefile").read_text()
    sizes = (ROOT / "vasp_amd" / "csrc" / "fsi_pod.hpp").read_text()
    assert f"POD_SLAB = {hp.POD_SLAB};" in sizes and "POD_CHUNK = 128;" in sizes and "POD_FB = 64;" in sizes      # what the GPU shapes rely on
    assert f"POD_MAX_MODES = {hp.POD_MAX_MODES};" in sizes and hp.POD_SLAB % 3 == 0 and hp.POD_SLAB % 128 == 0
    ap = argparse.ArgumentParser()
    add_session_arguments(ap)
    ns = vars(ap.parse_args([]))
    assert all(ns[k] is None for k in ("hi_pass_pod", "hi_pass_pod_modes", "hi_pass_pod_weights"))
    for name in ("pod_gram", "pod_modes", "pod_fetch"):
        assert hasattr(capi.HipBackend, f"hi_pass_{name}") and hasattr(hp.HostBandSession, name)


TAIL = ", the device has 1000000 bytes free of which 62500 stay with the context"      # "%.0f" of 62500.5 rounds to even
ROOM_TEXTS = (
    ("fsi_band_pod_gram", "the Gram matrix needs", "12 x 12 entries, 2 slabs x 1 tiles of partial sums, 6153 rows of means and weights",
     "fsi_band_pod_gram: the Gram matrix needs 123456789012 bytes (12 x 12 entries, 2 slabs x 1 tiles of partial sums, 6153 rows of means and "
     "weights)" + TAIL),
    ("fsi_band_pod_modes", "the modes need", "5 modes x 6153 rows and their table of 12 frames",
     "fsi_band_pod_modes: the modes need 123456789012 bytes (5 modes x 6153 rows and their table of 12 frames)" + TAIL),
)


@pytest.mark.parametrize("fn,subject,layout,text", ROOM_TEXTS, ids=[r[0] for r in ROOM_TEXTS])
def test_a_room_refusal_names_both_byte_counts(fn, subject, layout, text):
    """The two allocating entry points refuse through the room rule's one format (csrc/fsi_room.hpp, through the kernel shim)."""
    from test_hi_pass_ladder import room_text
    assert room_text(fn, subject, 123456789012.0, layout, 1000000, 62500.5) == text
    src = (ROOT / "vasp_amd" / "csrc" / "fsi_sessions.hip").read_text()
    assert f'room_for(ctx, "{fn}", "{subject}"' in src
