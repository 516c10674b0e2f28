"""The per-cell references of tests/post_cells.py on the CPU, so that a failure of tests/test_gpu_post_cell_kernels.py is one of the
kernel: every builder against oracle.post_oracle (and the FP64 restatement of tests/test_hemodynamics.py) on exactly the inputs of
the GPU tests, all 15 facet masks, the closed forms, the branches of the principal-value formula, every measured constant (the FP64
oracle within K / 4) and the two conditions on the principal-value bound."""
import re

import numpy as np
import pytest

import kernel_shim as ks
import post_cells as pc
from oracle import post_oracle
from test_hemodynamics import hemo_reference as hemo_fp64
from test_hemodynamics import twssg_projection as twssg_fp64

LD = pc.LD
CASES = ("hand3", "shapes", "tube")


def test_the_shim_reaches_every_launch_but_the_calibration():
    src = ks.LIB_PATH.parent / "csrc"
    declared = set(re.findall(r"\b(launch_\w+)\(", (src / "fsi_kernels.hpp").read_text() + (src / "fsi_product.hpp").read_text()))
    reached = set(re.findall(r"\b(launch_\w+)\(", (src / "fsi_kernel_shim.hip").read_text()))
    assert declared - reached == {"launch_calibration"}


def test_pivoted_solve_is_the_solve():
    rng = np.random.default_rng(1)
    M = rng.standard_normal((50, 4, 4))
    M[::5, 0, 0] = 0.0                                   # a zero pivot in first place: the rows must be exchanged
    B = rng.standard_normal((50, 4, 3))
    X = pc.solve_pivoted(M, B)
    assert X.dtype == LD
    assert np.abs(X.astype(np.float64) - np.linalg.solve(M, B)).max() <= 1e-9 * np.abs(X).max()
    assert np.abs(np.einsum("nij,njk->nik", M.astype(LD), X) - B).max() <= 1e-15 * float(np.abs(X).max())


def test_shape_family():
    q = pc.shape_quality(pc.shape_points())
    assert np.allclose(q[:2], 1.0) and np.all((q[2:] > 5e-4) & (q[2:] < 2e-3))
    case = pc.cases("shapes")
    _, det, _ = ks.geometry_reference(case.coords, case.tets)
    sg = np.sign(det.astype(np.float64)).reshape(3, 2)
    assert np.all(sg[:, 0] == -sg[:, 1]) and np.all(sg != 0)                             # every shape in both orientations
    assert set(case.region[case.kind == 1]) == {0, 1, 2}
    tube = pc.cases("tube")
    assert {0, 1, 2} == set(tube.region[pc.stress_lists("tube")])


# ---- wall shear stress --------------------------------------------------------------------------------------------------------------
def test_the_references_rule_is_exact_and_the_twelve_point_rule_is_not():
    w, lam = pc.midpoint_rule()
    exact = (1 + np.eye(3, dtype=LD)) / 12
    assert np.abs(np.einsum("q,qa,qb->ab", 2 * w, lam, lam) - exact).max() <= 2.0 ** -64 / 4
    _, dM3 = pc.rule_defect()
    assert 2 * pc.U64 < np.abs(dM3).max() < 8 * pc.U64                  # 6.7e-15 of 1 / 12
    # so the oracle with its own rule is several times further from the reference than with the exact one, on several facets only
    h = pc.wss_inputs("hand3")
    own = pc.cell_ratios(pc.wss_oracle64(h["case"], h["cells"], h["masks"], h["U"], pc.MU_WSS, rule="triangle12"), h["ref"])
    one = np.isin(h["masks"], (1, 2, 4, 8))
    assert own[one].max() <= pc.K_WSS["hand3"] / 4 < own[~one & (h["masks"] > 0)].max()


def test_wss_builder_agrees_with_the_oracle_on_every_mask():
    r = pc.measure_wss_ratios()
    for name in CASES:
        w = pc.wss_inputs(name)
        assert set(w["masks"]) == set(range(16))
        print(f"RATIO wss oracle FP64 {name}: random {r[name, 'random']:.2f}  " + "  ".join(f"{f} {r[name, f]:.2f}" for f in pc.K_WSS_FIELD))
        assert r[name, "random"] <= pc.K_WSS[name] / 4
        for f, K in pc.K_WSS_FIELD.items():
            assert r[name, f] <= K / 4
        # mask 0 and the vertices on no set facet: exact zeros in the reference
        ref = w["ref"]
        for k, m in enumerate(w["masks"]):
            if m == 0:
                assert np.all(ref[k] == 0)
            elif m in (1, 2, 4, 8):
                assert np.all(ref[k, int(np.log2(m))] == 0) and np.all(np.abs(ref[k]).sum(axis=1)[pc.FVERTS[int(np.log2(m))]] > 0)
            else:
                assert np.all(np.abs(ref[k]).sum(axis=1) > 0)


def test_wss_oracle_from_the_geometry_array_is_the_oracle_from_the_coordinates():
    """the geometry path added to oracle.post_oracle for these tests: on the hand-built cells both give the same traction (up to the
    rounding of the geometry array), for all 15 masks"""
    w = pc.wss_inputs("hand3")
    case, cells, masks = w["case"], w["cells"].astype(np.int64), w["masks"]
    a = pc.wss_oracle64(case, cells, masks, w["U"], pc.MU_WSS, rule="triangle12")
    fc = np.array([i for i in range(len(cells)) for f in range(4) if masks[i] >> f & 1])
    fl = np.array([f for i in range(len(cells)) for f in range(4) if masks[i] >> f & 1])
    b = post_oracle.wall_shear_stress(case.coords, case.tets[cells], case.tet_nodes[cells], w["U"][3 * case.N2:6 * case.N2].reshape(-1, 3),
                                      fc, fl, pc.MU_WSS)
    for k in range(len(fc)):
        assert np.abs(a[fc[k], pc.FVERTS[fl[k]]] - b[k]).max() <= 1e-11 * np.abs(b).max()


@pytest.mark.parametrize("name", CASES)
def test_wss_closed_forms(name):
    """in extended precision the builder gives no traction for a rigid motion and the known constant one for the shear on one facet"""
    for field in ("translation", "rotation"):
        w = pc.wss_inputs(name, field)
        s = pc.gradient_scale(w["case"].geom[w["cells"]], w["v"], pc.MU_WSS)
        # the nodal values of the field are FP64 numbers: a rotation's are rounded, which the gradient passes on at 2^-53 of its terms
        assert np.all(np.abs(w["ref"]).reshape(len(s), -1).max(axis=1) <= 4 * pc.U64 * s)
    w = pc.wss_inputs(name, "shear")
    geom = w["case"].geom[w["cells"]]
    s = pc.gradient_scale(geom, w["v"], pc.MU_WSS)
    for f in range(4):
        sel = np.flatnonzero(w["masks"] == 1 << f)
        want = pc.shear_traction(geom[sel], f, pc.MU_WSS)
        got = w["ref"][sel][:, pc.FVERTS[f]]
        assert np.abs(got - want[:, None, :]).reshape(len(sel), -1).max(axis=1).max() <= (4 * pc.U64 * s[sel]).max()
        assert np.all(np.abs(got - want[:, None, :]).reshape(len(sel), -1).max(axis=1) <= 4 * pc.U64 * s[sel])


# ---- hemodynamics -------------------------------------------------------------------------------------------------------------------
def test_twssg_projection_closed_form_and_restatement():
    rng = np.random.default_rng(2)
    D = rng.standard_normal((20, 3, 3))
    got = pc.twssg_projection(D)
    assert np.abs(got.astype(np.float64) - twssg_fp64(D, np.ones(20))).max() <= 1e-13
    # the same vector at the three vertices projects to its norm at each of them
    c = rng.standard_normal((20, 1, 3)) * np.ones((1, 3, 1))
    got = pc.twssg_projection(c)
    assert np.abs(got - np.sqrt((c.astype(LD) ** 2).sum(axis=2))).max() <= 1e-17
    # and the kernel's closed inverse is the same projection: 6 sum_b (4 delta_ab - 1) sum_q w_q lambda_qb |D_q|
    tw, tl = (a.astype(LD) for a in pc.triangle_tables())
    nq = np.sqrt((np.einsum("qk,nki->nqi", tl, D.astype(LD)) ** 2).sum(axis=2))
    r = np.einsum("q,qb,nq->nb", tw, tl, nq)
    assert np.abs(6 * (4 * r - r.sum(axis=1, keepdims=True)) - pc.twssg_projection(D)).max() <= 1e-13


def test_hemo_builder_agrees_with_the_restatement():
    """three samples on zero accumulators: the sums are those of tests/test_hemodynamics.hemo_reference (FP64), the first sample's
    TWSSG is |tau_1| / dt projected"""
    rng = np.random.default_rng(3)
    n, nf, dt = 7, 30, 2.5e-3
    masks = np.array([1, 2, 4, 8, 3, 15, 0])
    fidx = rng.permutation(nf)[:4 * n].reshape(n, 4)
    acc = pc.hemo_start(nf, None)
    taus, facets = [], [(i, f) for i in range(n) for f in range(4) if masks[i] >> f & 1]
    for s in range(3):
        b = rng.standard_normal((n, 4, 3))
        acc = pc.hemo_reference(acc, b, np.zeros(n), masks, fidx, dt)
        taus.append(np.array([b[i][pc.FVERTS[f]] for i, f in facets]))
        if s == 0:
            first = {k: acc[k].copy() for k in ("sum_twssg", "sum_mag")}
    ref = hemo_fp64(taus, dt, np.ones(len(facets)))
    dofs = np.array([3 * fidx[i, f] + np.arange(3) for i, f in facets])
    assert np.abs(acc["sum_mag"][dofs].astype(np.float64) / 3 - ref["TAWSS"]).max() <= 1e-13
    assert np.abs(acc["sum_twssg"][dofs].astype(np.float64) / 3 - ref["TWSSG"]).max() <= 1e-10
    out, _ = pc.hemo_finish_reference(3, acc["sum_tau"], acc["sum_mag"], acc["sum_twssg"])
    for k, name in enumerate(("TAWSS", "OSI", "RRT", "ECAP", "TWSSG")):
        assert np.abs(out[k][dofs].astype(np.float64) - ref[name]).max() <= 1e-9 * np.abs(ref[name]).max()
    assert np.abs(first["sum_twssg"][dofs] - pc.twssg_projection(taus[0].astype(LD) / LD(dt))).max() == 0
    untouched = np.setdiff1d(np.arange(3 * nf), dofs.ravel())
    assert len(untouched) and all(np.all(acc[k][untouched] == 0) for k in ("sum_tau", "tau_prev", "sum_mag", "sum_twssg"))
    assert all(np.all(acc["err"][k][untouched] == 0) for k in acc["err"])


def test_hemo_finish_classes():
    st = np.array([[0.0, 0, 0], [0.0, 0, 0], [3.0, 0, 4.0], [1.0, 2.0, 2.0]])
    sm = np.array([2.0, 0.0, 5.0, 4.0])
    out, bound = pc.hemo_finish_reference(1, st, sm, np.ones(4))
    tawss, osi, rrt, ecap, _ = out
    assert osi[0] == 0.5 and np.isposinf(rrt[0]) and ecap[0] == 0.25
    assert np.isnan(osi[1]) and np.isnan(ecap[1]) and np.isposinf(rrt[1]) and tawss[1] == 0
    assert osi[2] == 0 and rrt[2] == LD(1) / 5 and bound[1, 2] > 0
    assert abs(float(osi[3]) - 0.125) < 1e-18
    assert np.all(bound[~np.isfinite(out)] == 0)


# ---- principal values ---------------------------------------------------------------------------------------------------------------
def test_closed_form_is_the_oracles_and_finds_the_largest_eigenvalue():
    fam = pc.principal_families()
    T = fam["separated"]
    # two FP64 evaluations of the same formula in another order of operations (I1 ** 3 for I1 I1 I1, 27 / 2 for 13.5): each is
    # within K_PRINCIPAL / 4 of the a-priori bound of the extended-precision value, so they are within half of K_PRINCIPAL of each other
    both = pc.principal_bound(T) + pc.principal_bound(T, u=pc.U80)
    assert np.all(np.abs(pc.closed_form(T, np.float64) - post_oracle.kopp_max_eigenvalue(T)) <= pc.K_PRINCIPAL / 2 * both)
    # in extended precision the closed form is the largest eigenvalue: within its own a-priori bound at 2^-64 plus the error of the
    # polished eigenvalue - a Newton step divides the cubic's value, about 8 operations on terms of |T|^3, by its slope
    # (lambda - lambda_2)(lambda - lambda_3) >= (0.3 |T|)^2 on this family: 8 / 0.09 < 128 units of 2^-64 |T|
    true = pc.true_max_eigenvalue(T)
    assert np.all(np.abs(pc.closed_form(T) - true) <= pc.principal_bound(T, u=pc.U80) + 128 * pc.U80 * np.abs(T).max(axis=(1, 2)))
    assert np.abs(true.astype(np.float64) - np.linalg.eigvalsh(T)[:, -1]).max() <= 1e-12 * np.abs(T).max()


def test_closed_form_branches_on_the_exact_tensors():
    T = np.concatenate([pc.principal_families()["exact"], pc.principal_families()["zero_rule"]])
    l64, l80 = pc.closed_form(T, np.float64, True), pc.closed_form(T, LD, True)
    assert np.array_equal(l64[1], l80[1]) and np.array_equal(l64[2], l80[2])          # p and q: the same branches
    # the discriminant's branch: the same, but for the multiples of I - there p is the perturbed 2e-16, the discriminant
    # 27 I2^2 (p - I2) / 4 + ... rounds it away in FP64 and keeps it in extended precision, and it does not matter: q is an exact zero,
    # and atan2(r, 0) is pi / 2 for every r > 0
    differ = l64[3] != l80[3]
    I1 = np.trace(T, axis1=1, axis2=2)
    q = 13.5 * pc._det3(T) + I1 ** 3 - 4.5 * I1 * 0.5 * (I1 ** 2 - (T * T).sum(axis=(1, 2)))
    assert np.all(q[differ] == 0) and list(np.flatnonzero(differ)) == [0, 1, 2]
    taken = np.stack(l64[1:])
    assert taken.any(axis=1).all() and (~taken).any(axis=1).all()                      # every branch is taken and is not taken somewhere
    lam = l80[0]
    pert = np.sqrt(LD(2e-16)) * 2 * np.cos(LD(np.pi) / 6) / 3
    for k, a in enumerate((1.0, 4.0, -2.0)):
        assert abs(lam[k] - (a + pert)) <= 4 * 2.0 ** -64 * 4
    assert abs(float(lam[0]) - (1 + 8.16e-9)) < 1e-11
    assert [float(x) for x in lam[3:9]] == [2.0, 2.0, 3.0, -1.0, 3.0, 1.0]
    t = 2.0 ** -27
    assert abs(float(lam[9]) / t - 1) > 1.09                                            # 2^-27 I: 110 % off, and that is the contract
    # the zero rule of k_tensor_principal
    z = pc.principal_families()["zero_rule"]
    ref = pc.principal_reference(pc.amplitudes_of(z))
    assert np.all(ref[:4] == 0) and np.all(ref[4:] != 0)
    assert abs(float(pc.closed_form(z[3:4])[0]) - 8.2e-9) < 1e-10                       # what the stress kernels give a tensor at rest
    offdiag = ref[5]                                                                   # one off-diagonal entry of 1e-8: eigenvalue 1e-8
    assert abs(float(offdiag) - 1e-8) < 1e-20
    diag = float(ref[4])                                                               # one diagonal entry of 1e-8
    assert abs(abs(diag - 1e-8) / 1e-8 - 0.089) < 1e-3


def test_principal_constant_and_the_two_conditions():
    r = pc.measure_principal_ratios()
    print("RATIO principal oracle FP64: " + "  ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert set(r) == {"separated", "near_double", "hydrostatic", "exact", "zero_rule"}          # no family left out
    assert max(r.values()) <= pc.K_PRINCIPAL / 4
    T = pc.principal_families()["separated"]
    lam = np.sort(np.linalg.eigvalsh(T), axis=1)
    assert np.all(np.diff(lam, axis=1).min(axis=1) >= 0.3 * np.abs(T).max(axis=(1, 2)))         # gaps of the tensor's own order
    b = pc.principal_check_bound(T)
    print(f"RATIO principal bound on the separated family / (2^-53 max|T|): {float((b / (pc.U64 * np.abs(T).max(axis=(1, 2)))).max()):.1f}")
    assert np.all(b < 64 * pc.U64 * np.abs(T).max(axis=(1, 2)))
    # the exact tensors are all compared, and tightly: a few units in the last place of the value
    E = pc.principal_families()["exact"]
    assert len(E) == len(pc.EXACT_NAMES)
    assert np.all(pc.principal_check_bound(E) <= 16 * pc.U64 * np.maximum(np.abs(pc.closed_form(E)), np.abs(E).max(axis=(1, 2))))
    nd = pc.principal_families()["near_double"]
    lam = np.sort(np.linalg.eigvalsh(nd), axis=1)
    gap = np.diff(lam, axis=1).min(axis=1) / np.abs(nd).max(axis=(1, 2))
    assert np.all((gap > 2e-7) & (gap < 5e-6))
    # the hydrostatic family is the conditioned case: FP64 is off by far more than 64 x 2^-53 there, within the bound
    H = pc.principal_families()["hydrostatic"]
    err = np.abs(post_oracle.kopp_max_eigenvalue(H) - pc.closed_form(H))
    assert err.max() > 1e3 * 64 * pc.U64 * 1e6 * 1e-3 and np.all(err <= pc.principal_check_bound(H))


# ---- stress and strain ------------------------------------------------------------------------------------------------------------------
def test_second_piola_in_extended_precision_is_the_oracles():
    rng = np.random.default_rng(4)
    g = 0.05 * rng.standard_normal((30, 3, 3))
    for model, extra in ((0, ()), (1, (1.0e5, 5.0e4, 1.0e4))):
        a = post_oracle.second_piola(g, 3.0e5, 2.0e6, model, *extra)
        b = post_oracle.second_piola(g.astype(LD), 3.0e5, 2.0e6, model, *extra)
        assert a.dtype == np.float64 and b.dtype == LD
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    assert np.all(post_oracle.second_piola(np.zeros((1, 3, 3), dtype=LD), 3.0e5, 2.0e6, 0) == 0)


def test_stress_builder_agrees_with_the_oracle():
    r = pc.measure_stress_ratios()
    for (name, disp), (s, e, p) in r.items():
        print(f"RATIO stress oracle FP64 {name} {disp}: stress {s:.4g}  strain {e:.4g}  principal / bound {p:.4f}")
        assert s <= pc.K_STRESS_BY[name, disp] / 4 and e <= pc.K_STRAIN_BY[name, disp] / 4 and p <= 0.25
    assert set(r) == set(pc.K_STRESS_BY) == set(pc.K_STRAIN_BY)


@pytest.mark.parametrize("name", CASES)
def test_stress_reference_at_rest_and_under_mooney_rivlin(name):
    z = pc.stress_inputs(name, "zero")["ref"]
    assert np.all(z["stress"] == 0) and np.all(z["strain"] == 0)
    rest = pc.closed_form(np.zeros((1, 3, 3)))[0]
    # a constant is projected onto itself up to the rounding of the FP64 tables (the barycentric coordinates of a point sum to 1 within
    # 2^-53 there)
    assert np.abs(z["pstress"] - rest).max() <= 8 * pc.U64 * rest and np.abs(z["pstrain"] - rest).max() <= 8 * pc.U64 * rest
    s = pc.stress_inputs(name, "large")
    mr = np.flatnonzero(s["case"].region[s["cells"]] == 2)
    assert len(mr)
    T = s["ref"]["stress"][mr].astype(np.float64)
    dev = T - np.trace(T, axis1=2, axis2=3)[..., None, None] / 3 * np.eye(3)
    print(f"RATIO mooney-rivlin {name}: |deviator| / |mean stress| {np.abs(dev).max() / np.abs(np.trace(T, axis1=2, axis2=3) / 3).max():.3f}")
