"""One application of the block preconditioner (vasp_amd/csrc/fsi_precond.hip, precondition_block) on a live context, stage by
stage against its host restatement (tests/block_apply.py), on the cylinder fixture (1 647 tets).

Stage-local: after an application the work vectors in ctx->blk hold what every stage left; each stage is restated from the
DEVICE's own input of that stage, so errors do not compound and a failure names its stage.  End to end: the returned vector
against the restatement run from r alone.  Bound, per stage and field in 2-norms:  |device - R_hi| <= 16 |R_lo - R_hi|, R_hi the
restatement one precision above the device's vectors of that stage (float64 for FP32 sweeps, longdouble for FP64 ones), R_lo
the restatement in the device's precision with every row summed in the reversed order; 16 is the factor test_live_chebyshev_intervals
gives a restatement's own sensitivity.  Copies and sums of two vectors are held to the bit, single products to the derived
bounds of test_live_pressure_step_by_hand.  The exact coarse solve of the solid cycle is FP32 block cyclic reduction on an
ill-conditioned level: stage-local, its answer is held to the 2e-2 of test_exact_coarse_solve_matches_a_dense_factorisation
against a dense solve of A_c + bcr_shift blockdiag(A_c) and handed to the restated cycle; end to end R_lo solves that level in
float32 and R_hi in float64.

The test prints every share |device - R_hi| / |R_lo - R_hi| and, for the default configuration, the ratio by which each
deliberate error of the restatement is caught (device outside the bound of the wrong restatement)."""
import numpy as np
import pytest

import block_apply as ba
import chain_consumers as cc
import kernel_shim as ks
from test_gpu_dropped_sweeps import make_ctx, two_chain_configuration

pytestmark = pytest.mark.gpu

FACTOR = 16.0
EPS = 2.0 ** -53
LD, F32, F64 = np.longdouble, np.float32, np.float64
BLOCKS = ("solid", "fluid", "schur", "disp")
FAULTS = ([("short", b) for b in BLOCKS] + [("shifted", b) for b in BLOCKS] + [("no_restart", "solid"), ("no_restart", "disp")]
          + [("gauss_seidel", None), ("dd_from_dv", None), ("prhs_from_xf", None), ("stale_xs", None)] + [("lmax", b) for b in BLOCKS])


@pytest.fixture(scope="module", autouse=True)
def shim():
    return cc.load()


def norm(a):
    return float(np.linalg.norm(np.asarray(a, dtype=LD)))


def share(dev, hi, lo):
    """|device - R_hi| / |R_lo - R_hi| in 2-norms (0 when the device equals R_hi)"""
    err, own = norm(dev.astype(LD) - hi.astype(LD)), norm(lo.astype(LD) - hi.astype(LD))
    return 0.0 if err == 0.0 else err / own if own > 0.0 else np.inf


def product_excess(R, w, c, dev, ref, extra, scale=None):
    """largest |dev - ref| / bound of y = c - scale (R w): bound (L + extra) eps (scale |R| |w| + |c|), L the row's entries"""
    absR = ba.Rows(R.n, R.rowptr, R.cols, np.abs(R.vals), ncols=R.ncols)
    S = absR(np.abs(w).astype(F64))
    if scale is not None:
        S = S * np.abs(scale)
    L = np.diff(R.rowptr)
    bound = (L + extra) * 2 * EPS * (S + np.abs(c))
    err = np.abs(dev.astype(LD) - ref.astype(LD)).astype(F64)
    ok = bound > 0
    worst = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    return np.inf if np.any(err[~ok] > 0) else worst


class Device:
    """what one application left in ctx->blk, and its result in solver order"""

    def __init__(self, hb, D, r_user, z_user):
        N2, V = D["N2"], D["V"]
        blk = ks.ctx_array(hb.ctx, "blk")
        for name in ("rd", "rv", "rp", "vs", "tp", "dp", "dv", "td", "xs", "xf"):
            setattr(self, name, ba.blk_vector(blk, N2, V, name))
        self.r = ba.to_solver(D, r_user)
        self.z = np.empty_like(z_user)
        self.z[D["user2solver"]] = z_user
        self.zd, self.zv, self.zp = ba.split(D, self.z)
        s = D["solid"]
        if s["mode"] == "cycle":
            nc = D["info"]["sbmg_nc"]
            w = ks.ctx_array(hb.ctx, "sbmg_work").reshape(5, nc, 4)
            self.crhs = w[4, :, :3].reshape(-1).copy()
            self.xc = hb.solid_coarse_solve(self.crhs.astype(F64)) if s["coarse"] == "exact" else None


def stage_shares(D, dev, fault=ba.NO_FAULT, xs_stale=None, own=None, only=None):
    """every stage from the device's own inputs: name -> (figure, kind); kind "chain": |device - R_hi| / |R_lo - R_hi|, held to 16;
    "product": the share of the derived bound; "exact": the number of entries that differ.  With a fault: the same figures for
    the wrong restatement R_hi, of the stage `only`, against the |R_lo - R_hi| of the right one (own, filled by the run without)"""
    f, out = D["flags"], {}
    own = {} if own is None else own
    want = lambda name: only is None or name == only      # noqa: E731

    def chain(name, device, run):
        if not want(name):
            return
        if fault.kind is None:
            hi, lo = run(False, False, fault), run(True, True, fault)
            own[name] = norm(lo.astype(LD) - hi.astype(LD))
            out[name] = (share(device, hi, lo), "chain")
        else:
            out[name] = (norm(device.astype(LD) - run(False, False, fault).astype(LD)) / max(own[name], 1e-300), "chain")
    rd0, rv0, rp0 = ba.split(D, dev.r)
    if only is None:
        out["split rv"] = (int(np.sum(cc.bits(dev.rv) != cc.bits(rv0))), "exact")
        out["split rp"] = (int(np.sum(cc.bits(dev.rp) != cc.bits(rp0))), "exact")
        out["xs off the solid nodes"] = (int(np.sum(cc.bits(dev.xs[~D["solid_rows"]]) != 0)), "exact")
        out["merge v"] = (int(np.sum(cc.bits(dev.zv) != cc.bits(dev.dv))), "exact")
        out["merge p"] = (int(np.sum(cc.bits(dev.zp) != cc.bits(dev.dp))), "exact")
    xc = getattr(dev, "xc", None)
    solid = lambda lo, rev, flt: ba.solid_predictor(D, dev.rv, lo, rev, flt, coarse_solution=xc)      # noqa: E731
    chain("solid predictor", dev.xs[D["solid_rows"]], lambda lo, rev, flt: solid(lo, rev, flt)["xs"][D["solid_rows"]])
    if D["solid"]["mode"] == "cycle" and only is None:
        chain("solid coarse rhs", dev.crhs, lambda lo, rev, flt: solid(lo, rev, flt)["crhs"])
        if xc is not None:
            ref = np.linalg.solve(D["solid"]["Ac_shifted"], dev.crhs.astype(F64))
            out["solid coarse solve"] = (norm(xc - ref) / norm(ref) / 2e-2, "product")
    chain("fluid predictor", dev.xf, lambda lo, rev, flt: ba.fluid_predictor(D, ba.fluid_rhs(D, dev.rv, dev.xs, lo, rev, flt), lo, rev, flt))
    if want("vs = xs + xf"):
        xs = np.where(D["solid_rows"], dev.xs, xs_stale) if fault.kind == "stale_xs" else dev.xs
        out["vs = xs + xf"] = (int(np.sum(cc.bits(dev.vs) != cc.bits(xs + dev.xf))), "exact")
    p = D["pres"]
    if want("pressure rhs"):
        w = dev.xf if ((f["experiment"] & 1) and p["pv32"]) or fault.kind == "prhs_from_xf" else dev.vs
        out["pressure rhs"] = (product_excess(p["Apv"], w, dev.rp, dev.tp, ba.pressure_rhs(D, dev.rp, dev.vs, dev.xf, False, False, fault), 5), "product")
    chain("Schur chain", dev.dp, lambda lo, rev, flt: ba.schur_chain(D, dev.tp, lo, rev, flt))
    if want("velocity correction"):
        out["velocity correction"] = (product_excess(p["Avp"], dev.dp, dev.vs, dev.dv, ba.velocity_correction(D, dev.vs, dev.dp, False), 8,
                                                     p["vv_dinv"]), "product")
    a = D["adv"]
    td_dev = dev.rd if a["is_db"] else dev.td
    if want("displacement rhs"):
        v = dev.xs if a["is_db"] and (f["dd_early"] or f["two_chains"]) and fault.kind != "dd_from_dv" else dev.dv
        if a["is_db"] and f["experiment"] & 2:
            out["displacement rhs"] = (int(np.sum(cc.bits(td_dev) != cc.bits(rd0))), "exact")
        else:
            out["displacement rhs"] = (product_excess(a["A"], v, rd0, td_dev, ba.disp_rhs(D, rd0, dev.xs, dev.dv, False, False, fault), 5), "product")
    chain("displacement block", dev.zd, lambda lo, rev, flt: ba.displacement_block(D, td_dev, lo, rev, flt)["dd"])
    return out


def end_to_end_shares(D, dev):
    hi, lo = ba.application(D, dev.r, False), ba.application(D, dev.r, True, reverse=True)
    parts = lambda z: dict(zip(("d", "v", "p"), ba.split(D, z)))      # noqa: E731
    h, l, z = parts(hi["z"]), parts(lo["z"]), parts(dev.z)
    return {f"end to end {k}": (share(z[k], h[k], l[k]), "chain") for k in ("d", "v", "p")}


def held(shares, label, worst):
    """prints every figure, notes the largest per stage in `worst` and returns the stages outside their bounds"""
    bad = []
    for name, (v, kind) in shares.items():
        limit = {"chain": FACTOR, "product": 1.0, "exact": 0}[kind]
        print(f"[{label}] {name}: {v:.3g} of {limit:g} ({kind})")
        worst[name] = max(worst.get(name, 0.0), float(v))
        if not v <= limit:
            bad.append(f"{name}: {v:.3g} > {limit:g}")
    return bad


def right_hand_sides(D, n, seed):
    """three random vectors in user order whose solid and fluid rows differ in magnitude, each another way"""
    rng = np.random.default_rng(seed)
    solver = D["user2solver"]
    node = np.minimum(solver // 6, D["N2"] - 1)
    solid = D["solid_rows"][3 * node] & (solver < 6 * D["N2"])
    return [rng.standard_normal(n) * np.where(solid, a, b) for a, b in ((1.0, 1.0e3), (1.0e3, 1.0), (1.0e-2, 3.0))]


@pytest.mark.parametrize("variant", list(cc.VARIANTS))
@pytest.mark.parametrize("storage", ["fp64", "mixed"])
def test_application_stage_by_stage(storage, variant, cylinder_case, capsys):
    """Three right-hand sides in turn on one context (the second and third would meet a stale xs), every stage from the device's
    own inputs and the result end to end; the default configuration also on the event-sampled single stream (the same bits as
    on two streams), after a refresh of the same Jacobian (the zero fill of xs happens again), and against every deliberately
    wrong restatement.  The one-chain variants take the Gauss-Seidel coupling; tiles=0, fused_sweeps=0 and solid_fused=0 change
    the kernels and meet the same restatement.

    Measured on an MI355X, largest share of 16 over the three applications, both storages, all 18 variants.  Chains whose
    sweeps the cycle keeps short: solid predictor (two-level cycle) 0.40 - 1.90, its coarse right-hand side 0.54 - 1.77, fluid
    predictor 0.94 - 1.76, Schur chain 0.71 - 2.06, displacement block 0.72 - 1.70.  The one-level solid chains of 300 sweeps
    come closest: solid_fp32=0 (FP64 against longdouble) 10.8, solid_fused=0 8.71, solid_mg=0 8.65, solid_block_jacobi=0 4.38;
    end to end their velocity part follows (8.71, 8.65, 4.41) and the pressure reaches 4.88; every other end-to-end share lies
    between 0.36 and 2.47.  Single products, share of the derived bound: pressure rhs <= 0.011, velocity correction <= 0.115,
    displacement rhs <= 0.090; the exact coarse solve 1.4e-5 of its 2e-2.  Copies, the sum xs + xf and the zeros of xs off the
    solid nodes: to the bit.  Deliberate errors (default configuration, fp64 / mixed storage), factor by which the device lies
    outside the bound: one sweep short 9.6e4 / 1.1e5 (solid), 2.9e5 / 3.0e5 (fluid), 3.8e12 / 2.6e12 (Schur), 1.1e4 / 1.0e4
    (displacement); coefficients shifted by one sweep 2.0e5 / 2.4e5, 7.5e4 / 7.9e4, 3.2e12 / 2.2e12, 1.0e4 / 9.8e3; tail not
    restarted 1.2e6 / 1.5e6 (solid), 2.3e5 / 2.2e5 (displacement); Gauss-Seidel coupling 5.7e5 / 5.9e5; displacement block fed
    dv 1.6e12; pressure rhs from xf 6.7e12; stale xs: 4 160 entries of vs differ; lmax of one block without one 1.6x widening
    step of the self-test (the number of steps a refresh took is not kept) 7.3e6 / 8.6e6, 6.4e5 / 6.8e5, 6.5e13 / 4.4e13,
    5.3e4 / 5.0e4."""
    from bench import FP64_STORAGE_ENV
    env = FP64_STORAGE_ENV if storage == "fp64" else {}
    tune = cc.VARIANTS[variant]
    hb = make_ctx(cylinder_case, env, tune)
    label = f"{storage} {variant}"
    try:
        hb.apply_preconditioner(np.random.default_rng(0).standard_normal(hb.ndof))      # the refresh and its self-test applications
        for k, v in tune.items():
            assert hb.tuning()[k] == v, k
        if variant == "default":
            missing = [k for k, v in two_chain_configuration(hb).items() if not v]
            assert not missing, f"not the two-chain configuration: {missing}"
        D = ba.live_apply_data(hb)
        f = D["flags"]
        one_chain = ("prec_streams=0", "tiles=0", "fused_sweeps=0", "solid_mg=0", "solid_fused=0", "solid_block_jacobi=0", "solid_fp32=0",
                     "scalar_dd=0", "sweeps_fp32=0", "pv_fp32=0", "one_sweep")
        assert f["two_chains"] == (0 if variant in one_chain else 1)
        assert f["cheb_its_p"] > 0 and f["cheb_its_d"] > 0 and f["debug_prec_apply"] == 0
        rhs = right_hand_sides(D, hb.ndof, 11)
        bad, worst, devs, zs, owns = [], {}, [], [], []
        with capsys.disabled():
            print()
            for k, r in enumerate(rhs):                # the second and third find a stale xs
                z = hb.apply_preconditioner(r)
                assert np.isfinite(z).all() and np.abs(z).max() > 0
                dev = Device(hb, D, r, z)
                devs.append(dev)
                zs.append(z)
                owns.append({})
                bad += [f"application {k}: {b}" for b in held(stage_shares(D, dev, own=owns[-1]), f"{label} #{k}", worst)]
                bad += [f"application {k}: {b}" for b in held(end_to_end_shares(D, dev), f"{label} #{k}", worst)]
            assert ba.ctx_apply_info(hb.ctx)["xs_zeroed"] == (1 if f["solid_fp32"] else 0)
            if variant == "default":
                # the sampled application: one stream, event pairs - the same bits, and the same stages
                hb.timers(reset=True)
                z = hb.apply_preconditioner(rhs[0])
                assert np.array_equal(z, zs[0]), "sampled (one stream) against unsampled (two streams)"
                bad += [f"sampled: {b}" for b in held(stage_shares(D, Device(hb, D, rhs[0], z)), f"{label} sampled", worst)]
                # a new Jacobian's refresh uses ctx->blk as scratch: the zero fill of xs must happen again
                hb.assemble_jacobian()
                z = hb.apply_preconditioner(rhs[1])
                dev = Device(hb, D, rhs[1], z)
                assert np.array_equal(z, zs[1]), "the same Jacobian refreshed: the same application"
                assert not np.any(dev.xs[~D["solid_rows"]]) and ba.ctx_apply_info(hb.ctx)["xs_zeroed"] == 1
                # the bound can tell: the device lies outside the bound of every deliberately wrong restatement
                for kind, block in FAULTS:
                    name = {"solid": "solid predictor", "fluid": "fluid predictor", "schur": "Schur chain", "disp": "displacement block",
                            "gauss_seidel": "fluid predictor", "dd_from_dv": "displacement rhs", "prhs_from_xf": "pressure rhs",
                            "stale_xs": "vs = xs + xf"}[block or kind]
                    v, how = stage_shares(D, devs[1], ba.Fault(kind, block), xs_stale=devs[0].vs, own=owns[1], only=name)[name]
                    ratio = v / {"chain": FACTOR, "product": 1.0, "exact": 0.5}[how]
                    print(f"[{label}] wrong restatement {kind} {block or ''}: {name} off by {ratio:.3g} x its bound")
                    if not ratio > 1.0:
                        bad.append(f"the wrong restatement '{kind} {block}' is inside the bound ({ratio:.3g})")
            print(f"[{label}] largest: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
        assert not bad, "\n".join(bad)
    finally:
        hb.close()
