"""The recycled GCR solve (vasp_amd/csrc/fsi_krylov.hip: gs_pass, gcr_project_entry, gcr_make_room, gcr_orthogonalise, gcr_store,
gcr_flush, judge_fp64_cycle, judge_fp32_cycle, run_cycles) and its kept store on a live context, through the test shim's
shim_ctx_solve_gcr / shim_ctx_krylov_info / shim_ctx_krylov_columns.  Single context only: the `host` and `rccl` reduced passes
of a partitioned run, and BiCGStab, are out of scope.

The solver's safety nets turn a wiring error into slowness, so nothing here replays the device's iteration path.  After EVERY
solve (Ctx.solve) the properties of tests/gcr_solve.py are checked: check_store on the fetched store; `relres` against
true_residual - where the solve took an FP64 verdict (it launched more products than iterations) to the a-priori bound of an
FP64 product over |b|, where gcr_verdict_due says none was due (FP64 store, first cycle, rtol >= 1e-8) to 0.1 rtol, the
threshold at which judge_fp64_cycle itself calls the pairs suspect; the host residual meets rtol; the sentinel tail of x is
intact.  The cases add what each path must leave behind: a fresh store, recycling (a repeated right-hand side and one
inside span(Q) cost no iteration: the entry projection alone leaves about 1e-10, six decades below the 1e-4 asked for, where a
wrong stride, offset or born mask leaves O(1)), rotation at capacities 8 and 40, the flush batch and the window ring, the
default storage policy, and the ends that are not convergence.

On a rotated store the repeated right-hand side is no longer inside the kept space (its answer was built from directions that
have been retired), so there the zero-iteration property is asserted for the right-hand side inside span(Q) alone; the
repeated and the perturbed one are solved and held to the properties above.

The host twin (gcr_solve.gcr_twin with the device's preconditioner as M) is used for what a property cannot say: that a
case is rightly designed (cases c and d: it converges without a restart and makes the directions the case needs), and the
iteration band of case c, [min - s - 1, max + s + 1] of the twins' counts with longdouble and float64 inner products, s their
spread.

Cylinder fixture (1 647 tets), zero state with the boundary data of t = 1e-3.  Measured on an MI355X: see MEASURED below and
NOTEBOOK.md ("The recycled GCR solve on a live context").
"""
import numpy as np
import pytest

import gcr_solve as gs
import kernel_shim as ks

pytestmark = pytest.mark.gpu

FSI_ERR_LINEAR = 4
FILL = -7.25
WEAK = dict(its_solid=1, its_fluid=1, its_schur=1, its_disp=1)       # case d: one sweep per block (set_chebyshev)
# case c: what makes the twin rotate the store more than twice at 1e-10 without a restart.  Capacity 8: the default
# preconditioner (33 directions).  Capacity 40: the default makes 29, one sweep per block 76, one sweep on intervals of
# kappa 1.2 makes 89.
ROTATION = {8: None, 40: dict(WEAK, kappa_solid=1.2, kappa_fluid=1.2, kappa_schur=1.2, kappa_disp=1.2)}
# case e: a tuning with which the 1e-11 solve loses the FP32 store every time (one Gram-Schmidt pass whatever it cancels, cycles
# driven to round-off on the FP32 recurrence); four runs out of four fell back in the same iteration
FALL_BACK = {"f32_cycle_floor": 1e-12, "orth_floor32": 1e30, "gcr_reorth": 1e-30}

MEASURED = """
MI355X, cylinder fixture: ndof 15 352, ndof % 4 = 0 (so ldq = ldz = ndof: this fixture has no padding rows), |b| 7.775e-4.
Iterations, host twin (longdouble / float64 inner products) against the device:
  c  capacity 8, default preconditioner, 1e-10        33 / 33    device 33   (made 33, 13 retirements of 2)
  c  capacity 40, one sweep, kappa 1.2, 1e-10         89 / 89    device 89   (made 89, 5 retirements of 10)
  d  one sweep per block, 1e-6                        47         device 47 (FP64 store) and 47 (FP32 store, hot_next 15)
a: 17 iterations to 1e-6, 12 more to 1e-10.  b: 0, 0, and 8 for the perturbed right-hand side against 17 on a fresh store (one
sweep per block: 16 against 47, FP64 and FP32 store alike).  On the rotated stores: 7 / 0 / 13 (capacity 8), 19 / 0 / 30 (40).
e: the defaults converge by refinement (22 iterations, two cycles, no fall-back); FALL_BACK falls back (206 iterations, six
verdicts, two directions left in an FP64 store).  Worst |relres - host| over what is allowed: 5.4e-5 of the a-priori bound
(a verdict at round-off level, 1.4e-15 against 1.2e-15), 1.1e-9 of the 0.1 rtol of an answer read from the recurrence.
The file runs in 8 s.  Against four wiring errors planted in fsi_krylov.hip, every access in bounds, it fails each time: a
retired KQ column not zeroed (free-column check; capacity 8 misses 1e-10 at 9.3e-9), the window's staging area two entries
early (FP32 solves refuse or fall back at once), |r|^2 read from gcr_out + 2 (relres 0 against 0.87), the exact q written
one window column on (bitwise window check).
"""


class Ctx:
    """a live context with its Jacobian assembled once, the equilibrated system in solver ordering on the host, and the
    record of the solves made on it"""

    def __init__(self, case, tuning, chebyshev=None):
        from test_gpu_parity import boundary_data
        from vasp_amd.capi import HipBackend, FsiError
        self.hb = hb = HipBackend(case[1], tuning=tuning)
        if chebyshev:
            hb.set_chebyshev(**chebyshev)
        g, P = boundary_data(case, 1e-3)
        hb.set_dirichlet_values(g)
        hb.set_interface_pressure(P)
        hb.assemble_residual()
        hb.assemble_jacobian()
        ctx = self.ctx = hb.ctx
        self.A = gs.Csr(ks.ctx_array(ctx, "rowptr"), ks.ctx_array(ctx, "cols"), ks.ctx_array(ctx, "A"))
        self.n = hb.ndof
        assert self.A.n == self.n
        # the physical right-hand side as fsi_solve forms it: a solve that may not iterate forms bs, refuses, and touches nothing
        with pytest.raises(FsiError) as e:
            hb.solve(lin_rtol=0.5, lin_max_it=0)
        assert e.value.code == FSI_ERR_LINEAR, str(e.value)
        self.b = ks.ctx_array(ctx, "bs")
        host = np.zeros(self.n)
        host[ks.ctx_array(ctx, "user2solver").astype(np.int64)] = hb.get_state("b")
        assert np.array_equal(self.b, host * ks.ctx_array(ctx, "rowscale")), "bs is not rowscale * b in solver ordering"
        self.bnorm = gs.norm(self.b)
        info = self.info()
        assert info["hw"] == 0 and info["made"] == 0 and info["ndof"] == self.n
        assert info["ldq"] == (self.n + 3) // 4 * 4 and info["ldz"] == (self.n + 1) // 2 * 2
        self.log = []
        self.worst_ratio = 0.0

    def close(self):
        self.hb.close()

    def info(self):
        return ks.ctx_krylov_info(self.ctx)

    def store(self):
        info = self.info()
        return (info,) + ks.ctx_krylov_columns(self.ctx, info)

    def precondition(self, r):
        return ks.ctx_precondition(self.ctx, r)

    def twin(self, rtol, dots, b=None):
        info = self.info()
        return gs.gcr_twin(self.A, self.precondition, self.b if b is None else b, rtol, 4000, info["cap"], info["gcr_escape"], dots)

    def solve(self, rhs, rtol, what, max_it=4000, expect=0):
        """one solve_gcr and the properties that hold after every solve; returns a record"""
        before = self.info()
        rc, msg, x, iters, relres, products = ks.ctx_solve_gcr(self.ctx, rhs, rtol, max_it, FILL)
        info, Q, Z, Qh = self.store()
        rec = dict(what=what, rc=rc, msg=msg, x=x[:self.n].copy(), iters=iters, relres=relres, products=products, info=info, before=before,
                   Q=Q, Z=Z, Qh=Qh, rtol=rtol)
        self.log.append(rec)
        assert np.all(x[self.n:] == FILL), f"{what}: the solve wrote behind x"
        gs.check_store(info, Q, Z, Qh)
        assert rc == expect, f"{what}: status {rc} ({msg}), expected {expect}"
        bn = gs.norm(rhs)
        if rc != 0 or bn == 0.0 or not np.isfinite(bn):
            return rec
        r, bound = gs.true_residual(self.A, rhs, rec["x"])
        host = gs.norm(r) / bn
        verdicts = products - iters
        fp64 = before["kry_fp32"] == 0 and info["kry_fp32"] == 0
        rec.update(host=host, verdicts=verdicts, bound=bound / bn)
        assert verdicts >= 0
        if verdicts > 0:
            kind, allowed = "verdict", bound / bn
        else:
            # nothing but the recurrence was read: only an FP64 store may do that, and only where gcr_verdict_due says so
            assert fp64, f"{what}: an FP32 store returned without the FP64 verdict"
            assert not ks.gcr_verdict_due_ref(rtol, relres * bn, bn, 0, iters, info["gcr_stagnated"], info["gcr_stalled"],
                                              info["nfree"] == 0 and info["hw"] == info["cap"], before["kry_fp32_policy"] == 3,
                                              before["f64_suspect"]), f"{what}: a verdict was due and none was taken"
            kind, allowed = "recurrence", 0.1 * rtol
        ratio = abs(relres - host) / allowed
        self.worst_ratio = max(self.worst_ratio, ratio)
        print(f"  [{what}] rtol {rtol:.0e}: {iters} iterations, {verdicts} verdicts, relres {relres:.3e} ({kind}), host {host:.3e}, "
              f"|relres - host| / allowed {ratio:.3g}, hw {info['hw']} made {info['made']} free {info['nfree']} "
              f"fp32 {info['kry_fp32']} policy {info['kry_fp32_policy']} restarts {info['gcr_restarts']}")
        assert ratio <= 1.0, f"{what}: relres {relres:.6e} against the host's {host:.6e}: {ratio:.3g} of what the {kind} allows"
        assert host <= rtol, f"{what}: the host residual {host:.3e} misses rtol {rtol:.1e} (relres {relres:.3e})"
        return rec

    def in_span(self, seed):
        """sum_j c_j Q_j over the live columns of the store, random c of order one"""
        info, Q, Z, Qh = self.store()
        live = [s for s in range(info["hw"]) if info["born"][s] >= 0]
        c = np.random.default_rng(seed).standard_normal(len(live))
        return c @ Q[live][:, :self.n].astype(np.float64)

    def perturbed(self, seed):
        """the physical right-hand side with every entry moved by 1e-3 of itself, b_i (1 + 1e-3 g_i), g standard normal: the
        perturbation lives in the rows and on the scales of the physical one (the rows of the equilibrated system differ by
        twelve decades, and the constrained rows carry zeros), as the right-hand sides of consecutive Newton iterations do.
        White noise of norm 1e-3 |b| over all rows is no neighbour of b in that sense: host twin and device agree that the kept
        space does not help with it (23 iterations on a fresh store, 24 on the kept one; NOTEBOOK.md)."""
        g = np.random.default_rng(seed).standard_normal(self.n)
        return self.b * (1.0 + 1e-3 * g)


def make(case, tuning, chebyshev=None):
    c = Ctx(case, tuning, chebyshev)
    print(f"\ncontext {tuning} {chebyshev or ''}: ndof {c.n}, ndof % 4 = {c.n % 4}, ldq {c.info()['ldq']}, ldz {c.info()['ldz']}, "
          f"cap {c.info()['cap']}, |b| {c.bnorm:.3e}")
    return c


@pytest.fixture(scope="module", autouse=True)
def shim():
    return ks.load()


@pytest.fixture(scope="module")
def fresh64(cylinder_case):
    c = make(cylinder_case, {"krylov_fp32": 0})
    c.steps = {}
    yield c
    c.close()


def case_a(c):
    """the two solves of case a, once per context"""
    if "a" not in c.steps:
        a1 = c.solve(c.b, 1e-6, "a: fresh store")
        a2 = c.solve(c.b, 1e-10, "a: tightened")
        c.steps["a"] = (a1, a2)
    return c.steps["a"]


def fresh_iterations(case, tuning, chebyshev, seed):
    """what the perturbed right-hand side of case b costs on an empty store of a context made the same way"""
    c = Ctx(case, tuning, chebyshev)
    try:
        return c.solve(c.perturbed(seed), 1e-6, "b: perturbed by 1e-3, fresh store")["iters"]
    finally:
        c.close()


def case_b(c, first_fresh, rotated=False):
    """the three solves of case b on the store as it stands; first_fresh: the iterations of a fresh solve of the perturbed
    right-hand side to 1e-6 (fresh_iterations)"""
    tag = "b (rotated)" if rotated else "b"
    s0 = c.info()
    if rotated:
        c.solve(c.b, 1e-4, f"{tag}: same right-hand side")
    else:
        again = c.solve(c.b, 1e-4, f"{tag}: same right-hand side")
        assert again["iters"] == 0, again["iters"]
        assert (again["info"]["hw"], again["info"]["made"]) == (s0["hw"], s0["made"])
    s1 = c.info()
    inside = c.solve(c.in_span(21), 1e-4, f"{tag}: inside span(Q)")
    assert inside["iters"] == 0, inside["iters"]
    assert (inside["info"]["hw"], inside["info"]["made"], inside["info"]["born"]) == (s1["hw"], s1["made"], s1["born"])
    pert = c.solve(c.perturbed(22), 1e-6, f"{tag}: perturbed by 1e-3")
    if pert["info"]["gcr_restarts"] == s1["gcr_restarts"]:
        assert pert["info"]["made"] == s1["made"] + pert["iters"]
    if not rotated:
        print(f"  [{tag}] perturbed right-hand side: {pert['iters']} iterations on the kept store, {first_fresh} on a fresh one")
        assert 0 < pert["iters"] < first_fresh, (pert["iters"], first_fresh)
        assert pert["info"]["hw"] == s1["hw"] + pert["iters"]
    return inside, pert


def test_fresh_fp64_store(fresh64):
    """case a: every iteration makes one direction and nothing is retired, dropped or restarted"""
    a1, a2 = case_a(fresh64)
    assert a1["iters"] > 0 and a2["iters"] > 0
    assert a1["info"]["made"] == a1["iters"] == a1["info"]["hw"]
    assert a2["info"]["made"] == a1["iters"] + a2["iters"] == a2["info"]["hw"]
    assert a2["info"]["gcr_restarts"] == 0 and a2["info"]["nfree"] == 0 and a2["info"]["kry_fp32"] == 0
    assert a1["Q"].dtype == np.float64


def test_recycling(fresh64, cylinder_case):
    """case b, after case a on the same store"""
    case_a(fresh64)
    case_b(fresh64, fresh_iterations(cylinder_case, {"krylov_fp32": 0}, None, 22))
    assert fresh64.info()["gcr_restarts"] == 0


def test_ends_that_are_not_convergence(fresh64):
    """case f: host refusals; the store is untouched by the first two and consistent after the third, and the context goes on"""
    c = fresh64
    case_a(c)
    s0 = c.store()

    def untouched():
        s = c.store()
        return all(s[0][k] == s0[0][k] for k in ("hw", "made", "born", "free", "hot_slots", "kry_fp32")) and \
            all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(s[1:3], s0[1:3]))
    zero = c.solve(np.zeros(c.n), 1e-6, "f: zero right-hand side")
    assert zero["iters"] == 0 and zero["relres"] == 0.0 and zero["products"] == 0
    assert not zero["x"].any() and not np.signbit(zero["x"]).any()
    assert untouched()
    c.solve(c.b, 1e-6, "f: after the zero right-hand side")
    s0 = c.store()
    bad = c.b.copy()
    bad[c.n // 2] = np.nan
    nan = c.solve(bad, 1e-6, "f: NaN right-hand side", expect=FSI_ERR_LINEAR)
    assert "non-finite right-hand side" in nan["msg"], nan["msg"]
    assert nan["iters"] == 0 and nan["products"] == 0 and untouched()
    c.solve(c.b, 1e-6, "f: after the NaN right-hand side")
    # a right-hand side the store does not hold, so that three iterations are not enough
    rhs = c.perturbed(23)[::-1].copy()
    made = c.info()["made"]
    short = c.solve(rhs, 1e-10, "f: max_it 3", max_it=3, expect=FSI_ERR_LINEAR)
    assert "no convergence" in short["msg"], short["msg"]
    assert short["iters"] == 3 and short["info"]["made"] == made + 3
    assert gs.norm(gs.true_residual(c.A, rhs, short["x"])[0]) <= gs.norm(rhs)
    c.solve(c.b, 1e-6, "f: after max_it 3")


@pytest.mark.parametrize("cap", [8, 40])
def test_rotation(cap, cylinder_case):
    """case c: capacity 8 (the least fsi_create takes: ring 4, batch 2) and 40 (ring 20, batch 10), driven to 1e-10"""
    c = make(cylinder_case, {"krylov_fp32": 0, "krylov_capacity": cap}, ROTATION[cap])
    try:
        assert c.info()["cap"] == cap and ks.gcr_ring(cap) == cap // 2 and ks.gcr_retire_batch(cap) == cap // 4
        twins = [c.twin(1e-10, dots) for dots in ("longdouble", "float64")]
        counts = [t["iters"] for t in twins]
        for t in twins:      # conditions on the case, not on the device
            assert t["restarts"] == 0 and t["relres"] <= 1e-10, (t["restarts"], t["relres"])
            assert t["store"].made > 2 * cap, (t["store"].made, cap)
            gs.check_store(dict(t["info"], ndof=c.n), t["Q"][:t["store"].hw], t["P"][:t["store"].hw])
        dev = c.solve(c.b, 1e-10, f"c: capacity {cap}")
        s = max(counts) - min(counts)
        print(f"  capacity {cap}: twin iterations {counts[0]} (longdouble) {counts[1]} (float64), device {dev['iters']}")
        assert dev["info"]["gcr_restarts"] == 0
        assert dev["info"]["made"] == dev["iters"] > 2 * cap
        assert dev["info"]["hw"] == cap
        assert min(counts) - s - 1 <= dev["iters"] <= max(counts) + s + 1, (counts, dev["iters"])
        case_b(c, None, rotated=True)
        print(f"  capacity {cap}: worst |relres - host| / allowed {c.worst_ratio:.3g}")
    finally:
        c.close()


@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
def test_flush_batch_and_window_ring(fp32, cylinder_case):
    """case d: a preconditioner of one or two sweeps per block, so that one cycle makes more than GCR_FLUSH_BATCH + 8 directions:
    the flush inside the cycle, and with FP32 storage a window that has turned into a ring"""
    c = make(cylinder_case, {"krylov_fp32": fp32}, WEAK)
    try:
        if fp32 == 0:        # the condition on the case (the twin keeps FP64 columns, so it is asked once)
            t = c.twin(1e-6, "float64")
            print(f"  weak preconditioner: twin iterations {t['iters']}")
            assert t["restarts"] == 0 and t["relres"] <= 1e-6 and t["iters"] >= 40, (t["restarts"], t["relres"], t["iters"])
        d = c.solve(c.b, 1e-6, f"d: weak preconditioner, krylov_fp32 {fp32}")
        info = d["info"]
        assert d["verdicts"] <= 1, "more than one cycle"
        assert d["iters"] > ks.GCR_FLUSH_BATCH + 8 and info["made"] == d["iters"] == info["hw"]
        assert info["kry_fp32"] == fp32 and d["Q"].dtype.itemsize == (4 if fp32 else 8)
        assert c.hb.timers()["q_elem_bytes"] == (4 if fp32 else 8)
        if fp32:
            assert info["window_cols"] == ks.GCR_WINDOW
            assert info["hot_next"] == d["iters"] % ks.GCR_WINDOW                      # wrapped: more than 32 were put
            newest = sorted(range(info["hw"]), key=lambda s: info["born"][s])[-ks.GCR_WINDOW:]
            assert sorted(info["hot_slots"]) == sorted(newest)                         # all 32 columns, the latest directions
        else:
            assert info["window_cols"] == 0
        case_b(c, fresh_iterations(cylinder_case, {"krylov_fp32": fp32}, WEAK, 22))
    finally:
        c.close()


@pytest.mark.parametrize("tuning", [{}, FALL_BACK], ids=["defaults", "fall_back"])
def test_default_policy(tuning, cylinder_case):
    """case e: krylov_fp32 = 2.  A first solve at 1e-4 selects FP32 storage; 1e-11 on the same store either converges by
    refinement (the defaults do) or falls back to FP64 (FALL_BACK does) - whichever, the properties hold, and a solve at 1e-6
    follows."""
    c = make(cylinder_case, dict({"krylov_fp32": 2}, **tuning))
    try:
        e1 = c.solve(c.b, 1e-4, "e: selects the storage")
        assert e1["info"]["kry_fp32"] == 1 and e1["info"]["kry_fp32_policy"] == 2 and e1["Q"].dtype == np.float32
        e2 = c.solve(c.b, 1e-11, "e: 1e-11 on the FP32 store")
        info = e2["info"]
        fell = info["kry_fp32_failures_total"] - e1["info"]["kry_fp32_failures_total"]
        print(f"  case e: fell back {fell} times, restarts {info['gcr_restarts']}")
        if tuning:
            assert fell == 1
        if fell:
            assert fell == 1 and info["kry_fp32"] == 0 and info["kry_fp32_policy"] == 3
            assert e2["Q"].dtype == np.float64 and c.hb.timers()["q_elem_bytes"] == 8
            assert info["made"] <= e2["iters"] and info["made"] == info["hw"]         # only directions made after the reset
        else:
            assert info["kry_fp32"] == 1 and info["kry_fp32_policy"] == 2
            assert info["made"] == e1["iters"] + e2["iters"]
        c.solve(c.perturbed(24), 1e-6, "e: afterwards")
        print(f"  case e: worst |relres - host| / allowed {c.worst_ratio:.3g}")
    finally:
        c.close()
