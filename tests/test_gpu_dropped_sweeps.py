"""The last sweep of every Chebyshev chain of the block preconditioner is not launched (vasp_amd/csrc/fsi_precond.hip): its
product feeds an r and a d that nobody reads, and the chain's consumer forms x + d itself.  Bit for bit: (i) each consumer
kernel's x + d form against the kernel it extends, applied to the host's float32 x + d; (ii) one whole application of a context
against a context with FsiTuning.experiment bit 2, which launches every sweep, in both storage modes, on the event-sampled
single chain and on the two streams - in the default configuration and with each tuning field that selects another branch of
precondition_block (chain_consumers.VARIANTS)."""
import numpy as np
import pytest

import chain_consumers as cc
import kernel_shim as ks

pytestmark = pytest.mark.gpu

NODES = (1, 5, 257)


@pytest.fixture(scope="module", autouse=True)
def shim():
    return cc.load()


def with_tail(a, fill):
    """a flat copy of `a` with the shim's tail of sentinels behind it"""
    a = np.ascontiguousarray(a).ravel()
    return np.concatenate([a, np.full(cc.tail(), fill, dtype=a.dtype)])


# ---- the consumer kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nn", NODES)
def test_unpad_adds_the_direction(nn):
    rng = np.random.default_rng(100 + nn)
    x4, d4 = cc.vec4_pairs(rng, nn)
    want = with_tail(np.full(3 * nn, 9.0), 7.0)
    ks.call("shim_unpad_from_f32", nn, cc.host_sum(x4, d4).ravel(), want)
    got = with_tail(np.full(3 * nn, 9.0), 7.0)
    ks.call("shim_unpad_from_f32_xd", nn, x4.ravel(), d4.ravel(), got)
    cc.same_bits(got, want, f"unpad_from_f32 x + d, nn={nn}")
    assert (got[3 * nn:] == 7.0).all()
    cc.same_bits(got[:3 * nn], cc.host_sum(x4, d4)[:, :3].astype(np.float64).ravel(), "the sum, then the conversion")


@pytest.mark.parametrize("nn", NODES)
def test_merge_adds_the_direction(nn):
    rng = np.random.default_rng(200 + nn)
    V = nn // 2 + 1
    x4, d4 = cc.vec4_pairs(rng, nn)
    zv, zp = rng.standard_normal(3 * nn), rng.standard_normal(V)
    want = with_tail(np.full(6 * nn + V, 9.0), 7.0)
    ks.call("shim_merge_f32d", nn, V, cc.host_sum(x4, d4).ravel(), zv, zp, want)
    got = with_tail(np.full(6 * nn + V, 9.0), 7.0)
    ks.call("shim_merge_f32d_xd", nn, V, x4.ravel(), d4.ravel(), zv, zp, got)
    cc.same_bits(got, want, f"merge_f32d x + d, nn={nn}")
    assert (got[6 * nn + V:] == 7.0).all()
    z = got[:6 * nn].reshape(nn, 6)
    cc.same_bits(z[:, :3], cc.host_sum(x4, d4)[:, :3].astype(np.float64), "displacement part")
    cc.same_bits(z[:, 3:], zv.reshape(nn, 3), "velocity part")


@pytest.mark.parametrize("nn", NODES)
def test_scatter_adds_the_direction_and_leaves_the_other_nodes(nn):
    rng = np.random.default_rng(300 + nn)
    nfull_nodes = 2 * nn + 3
    snode = rng.permutation(nfull_nodes)[:nn].astype(np.int32)      # not ascending; nn + 3 nodes are not solid
    x4, d4 = cc.vec4_pairs(rng, nn)
    full0 = rng.standard_normal(3 * nfull_nodes)
    want = full0.copy()
    ks.call("shim_scatter3_f32", nn, 3 * nfull_nodes, snode, cc.host_sum(x4, d4).ravel(), want)
    got = with_tail(full0, 7.0)
    ks.call("shim_scatter3_f32_xd", nn, 3 * nfull_nodes, snode, x4.ravel(), d4.ravel(), got)
    cc.same_bits(got[:3 * nfull_nodes], want, f"scatter3_f32 x + d, nS={nn}")
    assert (got[3 * nfull_nodes:] == 7.0).all()
    other = np.setdiff1d(np.arange(nfull_nodes), snode)
    assert len(other) == nn + 3
    cc.same_bits(got[:3 * nfull_nodes].reshape(-1, 3)[other], full0.reshape(-1, 3)[other], "non-solid entries untouched")
    cc.same_bits(got[:3 * nfull_nodes].reshape(-1, 3)[snode], cc.host_sum(x4, d4)[:, :3].astype(np.float64), "solid entries")


def prolong_case(rng, nn):
    """a fine level of nn nodes over nc coarse ones: vertices (weights 1, 0), midpoints (1/2, 1/2) and general weights; every
    third row from row 1 on is switched off (d0 == 0, resp. flagged); coarse vectors with garbage in the pad lane"""
    nc = nn // 2 + 1
    par = rng.integers(0, nc, (nn, 2)).astype(np.int32)
    pw = np.where(rng.random((nn, 1)) < 0.4, np.float32([1.0, 0.0]), np.float32([0.5, 0.5])).astype(np.float32)
    gen = rng.random(nn) < 0.3
    pw[gen] = rng.uniform(-1, 1, (int(gen.sum()), 2)).astype(np.float32)
    off = np.arange(nn) % 3 == 1
    xc4, dc4 = cc.vec4_pairs(rng, nc, pad=3.5)
    return nc, par.ravel(), pw.ravel(), off, xc4, dc4


@pytest.mark.parametrize("nn", NODES)
def test_mg_prolong_adds_the_coarse_direction(nn):
    rng = np.random.default_rng(400 + nn)
    nc, par, pw, off, xc4, dc4 = prolong_case(rng, nn)
    d0 = np.where(off, 0.0, rng.uniform(0.5, 2.0, nn)).astype(np.float32)
    assert nn == 1 or (d0 == 0).any()
    want = np.full(4 * nn, 9.0, dtype=np.float32)
    ks.call("shim_mg_prolong", nn, nc, par, pw, d0, cc.host_sum(xc4, dc4).ravel(), want)
    got = with_tail(np.full(4 * nn, 9.0, dtype=np.float32), 7.0)
    ks.call("shim_mg_prolong_xd", nn, nc, par, pw, d0, xc4.ravel(), dc4.ravel(), got)
    cc.same_bits(got[:4 * nn], want, f"mg_prolong x + d, N2={nn}")
    assert (got[4 * nn:] == 7.0).all()
    e = got[:4 * nn].reshape(nn, 4)
    cc.same_bits(e[:, 3], np.zeros(nn, dtype=np.float32), "pad lanes")
    cc.same_bits(e[d0 == 0], np.zeros((int((d0 == 0).sum()), 4), dtype=np.float32), "rows with d0 == 0")
    assert nn == 1 or np.any(e[d0 != 0, :3] != 0)


@pytest.mark.parametrize("nn", NODES)
def test_sbmg_prolong_adds_the_coarse_direction(nn):
    rng = np.random.default_rng(500 + nn)
    nc, par, pw, off, xc4, dc4 = prolong_case(rng, nn)
    flag = off.astype(np.uint8)
    assert nn == 1 or flag.any()
    want = np.full(4 * nn, 9.0, dtype=np.float32)
    ks.call("shim_sbmg_prolong", nn, nc, par, pw, flag, cc.host_sum(xc4, dc4).ravel(), want, None, None, 0)
    got = with_tail(np.full(4 * nn, 9.0, dtype=np.float32), 7.0)
    ks.call("shim_sbmg_prolong_xd", nn, nc, par, pw, flag, xc4.ravel(), dc4.ravel(), got)
    cc.same_bits(got[:4 * nn], want, f"sbmg_prolong x + d, nS={nn}")
    assert (got[4 * nn:] == 7.0).all()
    e = got[:4 * nn].reshape(nn, 4)
    cc.same_bits(e[:, 3], np.zeros(nn, dtype=np.float32), "pad lanes")
    cc.same_bits(e[flag != 0], np.zeros((int(flag.sum()), 4), dtype=np.float32), "flagged rows")
    assert nn == 1 or np.any(e[flag == 0, :3] != 0)


# ---- one whole application ---------------------------------------------------------------------------------------------------------
def two_chain_configuration(hb):
    """what precondition_block's two-chain condition asks of a context, read through tuning(), timers() and the shim's views"""
    t, tm = hb.tuning(), hb.timers()
    info, co = ks.ctx_info(hb.ctx), ks.ctx_coarse(hb.ctx)
    flags = int(tm["sweep_flags"])
    return {
        "prec_streams": t["prec_streams"] == 1, "sweeps_fp32": t["sweeps_fp32"] == 1,
        "tiled fused sweeps": bool(flags & 1), "solid fp32": bool(flags & 4), "solid block-Jacobi fused": bool(flags & 8),
        "solid two-level cycle": bool(flags & 16) and info["sbmg_ready"] == 1,
        "displacement two-level cycle": bool(flags & 32) and info["mg_ready"] == 1,
        "scalar displacement block": int(tm["disp_scalar"]) & 1 == 1 and co["dd_is_scalar"] == 1.0,
        "A_dv per component": co["adv_is_db"] == 1.0, "FP32 pressure products": co["pv32_ok"] == 1.0,
        "Schur sweeps": t["its_schur"] > 0, "displacement sweeps": t["its_disp"] > 0, "Schur vectors fit": 4 * info["V"] <= 3 * info["N2"],
    }


def make_ctx(case, env, tuning):
    from vasp_amd.capi import HipBackend
    from test_gpu_parity import boundary_data, random_state
    ns, desc = case[0], case[1]
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        hb = HipBackend(desc, tuning=tuning) if tuning else HipBackend(desc)
    g, P = boundary_data(case, 1e-3)
    U, U1 = random_state(ns["mesh"], hb.ndof, seed=3)
    hb.set_state("n", U)
    hb.set_state("n-1", U1)
    hb.set_dirichlet_values(g)
    hb.set_interface_pressure(P)
    hb.assemble_residual()
    hb.assemble_jacobian()
    return hb


@pytest.mark.parametrize("variant", list(cc.VARIANTS))
@pytest.mark.parametrize("storage", ["fp64", "mixed"])
def test_application_keeps_its_bits_without_the_last_sweeps(storage, variant, cylinder_case):
    """The cylinder fixture (1 647 tets) is the smallest mesh under tests/golden; the default configuration runs both two-level
    cycles and the two chains on it, which the test checks before it relies on it.  Every other variant sets FsiTuning fields
    on both contexts and so takes another branch of precondition_block; the context with experiment bit 2 launches every sweep."""
    from bench import FP64_STORAGE_ENV
    env = FP64_STORAGE_ENV if storage == "fp64" else {}
    tune = cc.VARIANTS[variant]
    base = tune.get("experiment", 0)
    new = make_ctx(cylinder_case, env, tune)
    old = make_ctx(cylinder_case, env, dict(tune, experiment=base | cc.EXPERIMENT_ALL_SWEEPS))
    try:
        assert new.tuning()["experiment"] == base and old.tuning()["experiment"] == base | cc.EXPERIMENT_ALL_SWEEPS
        for k, v in tune.items():
            assert new.tuning()[k] == v and (k == "experiment" or old.tuning()[k] == v), k
        assert new.tuning()["sweeps_fp16"] == (0 if storage == "fp64" else 1)
        rng = np.random.default_rng(11)
        r0, r1, r2 = (rng.standard_normal(new.ndof) for _ in range(3))
        for hb in (new, old):
            hb.apply_preconditioner(r0)            # the refresh and its self-test applications
            missing = [k for k, v in two_chain_configuration(hb).items() if not v] if variant == "default" else []
            assert not missing, f"not the two-chain configuration: {missing}"
            hb.timers(reset=True)                  # counters from zero; the next 16 applications are sampled: one chain, event pairs
        z1n, z1o = new.apply_preconditioner(r1), old.apply_preconditioner(r1)
        assert np.isfinite(z1n).all() and np.abs(z1n).max() > 0
        assert np.array_equal(z1n, z1o), "application 1 (one chain, sampled sweeps)"
        for hb in (new, old):
            for _ in range(16):
                hb.apply_preconditioner(r2)
        z2n, z2o = new.apply_preconditioner(r1), old.apply_preconditioner(r1)
        assert np.isfinite(z2n).all() and np.abs(z2n).max() > 0
        assert np.array_equal(z2n, z2o), "application 18 (two streams in the default configuration)"
        tn, to = new.timers(), old.timers()
        apps = 18
        assert tn["precond_applies"] == apps and to["precond_applies"] == apps
        for name, per in zip(("inner_vv_iters", "inner_schur_iters", "inner_dd_iters"), cc.dropped_per_application(variant, storage)):
            print(f"{storage} {variant}: {name} old {to[name]} new {tn[name]}")
            assert to[name] - tn[name] == per * apps, (name, to[name], tn[name])
            assert tn[name] > 0 or (variant == "one_sweep" and tn[name] == 0)      # chains of one sweep launch none
    finally:
        new.close()
        old.close()
