"""The consumers of a Chebyshev chain's result in their x + d form (vasp_amd/csrc/fsi_block.hip: k_unpad_from_f32, k_merge_f32d,
k_scatter3_f32, k_mg_prolong, k_sbmg_prolong with a direction): ctypes signatures of their shim entry points and the vectors
the tests feed them.  The preconditioner does not launch the last sweep of a chain; the consumer forms x + d as that sweep
would have (one FP32 addition per entry, before any conversion).  Tested on the CPU in tests/test_chain_consumer_vectors.py;
the GPU tests are tests/test_gpu_dropped_sweeps.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

import kernel_shim as ks

# argument codes as in kernel_shim._SIGS: p pointer, i int32, l int64, f float, d double
SIGS = {
    "shim_unpad_from_f32_xd": "lppp", "shim_merge_f32d_xd": "llppppp", "shim_scatter3_f32_xd": "llpppp",
    "shim_mg_prolong_xd": "llpppppp", "shim_sbmg_prolong_xd": "llpppppp",
}
_CT = {"p": C.c_void_p, "i": C.c_int32, "l": C.c_int64, "f": C.c_float, "d": C.c_double}
EXPERIMENT_ALL_SWEEPS = 4          # FsiTuning.experiment bit 2: every chain launches its last sweep
# fine-level product sweeps a default application does not launch, as (inner_vv_iters, inner_schur_iters, inner_dd_iters)
# count them: fluid predictor + solid cycle, Schur complement, displacement cycle
DROPPED_PER_APPLICATION = (2, 1, 1)

# FsiTuning variants of the whole-application test, applied to both contexts: every branch of precondition_block that a
# tuning field selects.  "one_sweep": chains of one sweep, of which nothing is launched - the consumer adds the first direction.
VARIANTS = {
    "default": {}, "prec_streams=0": dict(prec_streams=0), "tiles=0": dict(tiles=0), "fused_sweeps=0": dict(fused_sweeps=0),
    "solid_mg=0": dict(solid_mg=0), "solid_fused=0": dict(solid_fused=0), "solid_block_jacobi=0": dict(solid_block_jacobi=0),
    "solid_fp32=0": dict(solid_fp32=0), "solid_coarse_exact=0": dict(solid_coarse_exact=0), "dd_mg=0": dict(dd_mg=0),
    "scalar_dd=0": dict(scalar_dd=0), "sweeps_fp32=0": dict(sweeps_fp32=0), "cheb4=7": dict(cheb4=7), "pv_fp32=0": dict(pv_fp32=0),
    "sbmg_post=0": dict(sbmg_post=0), "experiment=1": dict(experiment=1), "experiment=2": dict(experiment=2),
    "one_sweep": dict(solid_mg=0, dd_mg=0, its_solid=1, its_fluid=1, its_schur=1, its_disp=1),
}


def dropped_per_application(variant: str, storage: str):
    """DROPPED_PER_APPLICATION of a variant: a chain that runs through the unfused FP64 solve (cheb_solve_op) launches every
    sweep.  solid_fp32=0: the solid predictor; sweeps_fp32=0: the fluid predictor and the displacement block; fused_sweeps=0
    with FP64 Schur values (the FP64 storage mode): the Schur solve."""
    if variant == "solid_fp32=0":
        return (1, 1, 1)
    if variant == "sweeps_fp32=0":
        return (1, 1, 0)
    if variant == "fused_sweeps=0" and storage == "fp64":
        return (2, 0, 1)
    return DROPPED_PER_APPLICATION


def load():
    """the shim with the signatures of the x + d entry points set (ks.call then runs them)"""
    lib = ks.load()
    for name, sig in SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = [_CT[c] for c in sig]
        fn.restype = C.c_int
    return lib


def tail() -> int:
    """elements behind every output of these entry points that the launch must leave alone"""
    return int(ks.load().shim_tail())


# (x, d) pairs every vector starts with, as far as it is long enough: sums that cancel to +0 and to -0, signed zeros, sums
# that round (a tie to even that keeps x, a tie that goes up, an addend below half an ulp, one just above), a sum that
# overflows no exponent but changes it, a subnormal result
SPECIAL = np.array([
    (1.5, -1.5), (-3.25e7, 3.25e7), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0),
    (1.0, 2.0 ** -24), (1.0 + 2.0 ** -23, 2.0 ** -24), (1.0, 2.0 ** -25), (1.0, 2.0 ** -24 + 2.0 ** -40),
    (1.0e8, 1.0), (-16777216.0, -1.0), (0.75, 0.75), (1.0e-38, -0.9e-38), (3.0, -2.0 ** -23),
], dtype=np.float32)


def xd_pairs(rng, n):
    """two float32 vectors of n entries, mixed signs, magnitudes over twelve decades, the SPECIAL pairs in front (at a random
    offset when there is room, so that they meet different components)"""
    mag = lambda: (10.0 ** rng.uniform(-6, 6, n)) * rng.standard_normal(n)      # noqa: E731
    x, d = mag().astype(np.float32), mag().astype(np.float32)
    same = rng.random(n) < 0.3                     # a third of the pairs of like magnitude: sums that lose bits or cancel partly
    d[same] = (x[same] * rng.uniform(-2, 2, int(same.sum()))).astype(np.float32)
    k = min(n, len(SPECIAL))
    o = int(rng.integers(0, n - k + 1))
    x[o:o + k], d[o:o + k] = SPECIAL[:k, 0], SPECIAL[:k, 1]
    return x, d


def vec4_pairs(rng, nn, pad=0.0):
    """(x4, d4) [nn][4] float32 whose first three components are xd_pairs; the pad lane holds `pad` in both"""
    x, d = xd_pairs(rng, 3 * nn)
    x4, d4 = np.full((nn, 4), pad, dtype=np.float32), np.full((nn, 4), pad, dtype=np.float32)
    x4[:, :3], d4[:, :3] = x.reshape(nn, 3), d.reshape(nn, 3)
    return x4, d4


def host_sum(x, d):
    """x + d as the last sweep forms it: one float32 addition per entry"""
    x, d = np.asarray(x), np.asarray(d)
    assert x.dtype == np.float32 and d.dtype == np.float32
    s = x + d
    assert s.dtype == np.float32
    return s


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want, what):
    got, want = bits(got).ravel(), bits(want).ravel()
    assert got.shape == want.shape, f"{what}: {got.shape} against {want.shape}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} entries differ in their bits, first at {bad[0]}"
