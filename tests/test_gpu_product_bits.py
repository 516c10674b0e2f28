"""The monolithic product (vasp_amd/csrc/fsi_product.hip) against the bits of the commit before its kernels were built from
shared pieces and its host state became one type: every form of the product, through the test shim, must give the y that
tests/golden/product_bits.npz holds - recorded on an MI355X with that commit by tests/golden/make_product_bits.py - with equal
``uint64`` views.  The other product tests bound the kernels against extended precision; this one holds their accumulation order.

Synthetic cases, regenerated from their seeds (the file holds a SHA-256 of every input array: a mismatch there means the
generators drifted, not the kernels): N37_V20 and N1100_V400 of test_gpu_product_kernels.py with the matrix whose d rows are in
the pair pattern, N4097 of test_gpu_compact_drows.py with every other node coupled and with none.  Forms: six value rows with
and without the node graph (k_spmv_prow / the k_spmv<0, .> tail), pair form, split form, the padded FP32 copy with six rows, and
with value rows 3 .. 5 and FP32 pair values.

Live contexts on the cylinder fixture after one assembled Jacobian: host::spmv with working = 0 and 1 under the default tuning,
with compact_drows = 0, and with the FP32 basis pinned; also the form each context chose at its refresh and the two counters.

A y longer than 8192 entries is stored as the first 8 bytes of the SHA-256 of every 16 entries (all 30 products whole are 3.7 MB;
the file has to stay below the size a committed file may have); a difference is then reported by block, not by entry.  Held whole,
entry by entry: the six forms of N37_V20 (242 entries) and of N1100_V400 (7 000).  Held as digests only: the six forms of each of
N4097-alternating and N4097-none (26 082 entries), and both products of each of the three live contexts."""
import hashlib
from pathlib import Path

import numpy as np
import pytest

import kernel_shim as ks
import test_gpu_compact_drows as cd
import test_gpu_product_kernels as pk

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "product_bits.npz"
FORMS = ("six", "six_nograph", "pair", "split", "pad_six", "pad_pair")
SYNTHETIC = ("N37_V20", "N1100_V400", "N4097-alternating", "N4097-none")
# name: (tuning, forms chosen at the refresh (FP64, FP32 copy), (op32_products, drows_products) added by working = 0, by working = 1).
# krylov_fp32 = 2 (the default) starts every context on an FP64 basis: its working product is the FP64 one until a solve decides.
SIX64, PAIR64, SPLIT64, SIX32, PAIR32 = range(5)          # ProductForm of fsi_product_host.hpp
LIVE = {
    "default": ({}, (SPLIT64, PAIR32), (0, 1), (0, 1)),
    "compact0": (dict(compact_drows=0), (SIX64, SIX32), (0, 0), (0, 0)),
    "fp32": (dict(krylov_fp32=1, operator_fp32=1), (SPLIT64, PAIR32), (0, 1), (1, 1)),
}
BLOCK = 16


def stored(y):
    """what the golden file holds of y: its bits, or a digest per BLOCK entries of a long one"""
    bits = np.ascontiguousarray(y, dtype=np.float64).view(np.uint64)
    if len(bits) <= 8192:
        return bits
    pad = np.concatenate([bits, np.zeros(-len(bits) % BLOCK, dtype=np.uint64)]).reshape(-1, BLOCK)
    return np.array([int.from_bytes(hashlib.sha256(row.tobytes()).digest()[:8], "little") for row in pad], dtype=np.uint64)


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + a.tobytes()).hexdigest()


def synthetic_case(name):
    """(case dict with N2, V, g, rowptr, cols, x; its matrix with the d rows in the pair pattern)"""
    if name.startswith("N4097"):
        c = cd.graph("N4097")
        return c, cd.matrix(c, cd.coupled_nodes(c["N2"], name.split("-")[1]))
    c = pk.case(name)
    return c, c["Ap"]


def input_hashes(c, A):
    arrays = dict(zip(("nadj_ptr", "nadj", "padj_ptr", "padj", "vrank"), c["g"]), rowptr=c["rowptr"], cols=c["cols"], A=A, x=c["x"])
    return {k: sha(v) for k, v in arrays.items()}


def synthetic_products(c, A):
    """{form: y} of one case, every y starting as NaN"""
    N2, V, rowptr, cols, x = c["N2"], c["V"], c["rowptr"], c["cols"], c["x"]
    nadj_ptr, nadj, _, _, vrank = c["g"]
    graph, npairs, n = (vrank, nadj_ptr, nadj), len(nadj), 6 * N2 + V
    ad64 = ks.drows_extract(N2, rowptr, A, nadj_ptr)[0]
    _, _, dd, _, doff, dv = cd.split(c, A)
    p32, ptail, tail_src, _ = ks.pad_layout(N2, rowptr)
    ys = {f: np.full(n, np.nan) for f in FORMS}
    ks.call("shim_spmv_node6", N2, V, rowptr, cols, A, *graph, npairs, x, ys["six"], None)
    ks.call("shim_spmv_node6", N2, V, rowptr, cols, A, None, None, None, npairs, x, ys["six_nograph"], None)
    ks.call("shim_spmv_node6", N2, V, rowptr, cols, A, *graph, npairs, x, ys["pair"], ad64)
    dv = np.where(np.isnan(dv), 7.0e300, dv)
    assert cd.shim("shim_spmv_node6s", N2, V, rowptr, cols, A, *graph, npairs, x, ys["split"], dd, dv, len(dv) // 3, doff) == 0
    for form, v_rows_only in (("pad_six", False), ("pad_pair", True)):
        cols32, A32, written = ks.pad_copy(N2, rowptr, cols, A, v_rows_only)
        A32[~written] = np.nan
        ad32 = ad64.astype(np.float32) if v_rows_only else None
        ks.call("shim_spmv_node6p", N2, V, p32, cols32, A32, len(A32), rowptr, cols, ptail - tail_src, *graph, npairs, x, ys[form], ad32)
    for f, y in ys.items():
        assert not np.isnan(y).any(), f"{f}: y entries not written"
    return ys


def live_products(case, name):
    """(info, hash of the assembled matrix, x, {working: (y, op32_products added, drows_products added)}) of one context"""
    from test_gpu_parity import boundary_data, random_state
    from vasp_amd.capi import HipBackend
    hb = HipBackend(case[1], tuning=LIVE[name][0])
    try:
        g, P = boundary_data(case, 1e-3)
        U, U1 = random_state(case[0]["mesh"], hb.ndof, seed=4)
        hb.set_state("n", U)
        hb.set_state("n-1", U1)
        hb.set_dirichlet_values(g)
        hb.set_interface_pressure(P)
        hb.assemble_residual()
        hb.assemble_jacobian()
        x = np.random.default_rng(21).standard_normal(hb.ndof)
        out = {}
        for working in (0, 1):
            y = np.full(hb.ndof, np.nan)
            rc, op32, dr = ks.ctx_spmv(hb.ctx, working, x, y)
            assert rc == 0 and not np.isnan(y).any()
            out[working] = (y, op32, dr)
        return ks.ctx_info(hb.ctx), sha(ks.ctx_array(hb.ctx, "A")), x, out
    finally:
        hb.close()


def record(cylinder_case):
    """everything the golden file holds, from the library of this checkout"""
    out = {}
    for name in SYNTHETIC:
        c, A = synthetic_case(name)
        for k, h in input_hashes(c, A).items():
            out[f"{name}/sha/{k}"] = np.array(h)
        for f, y in synthetic_products(c, A).items():
            out[f"{name}/{f}"] = stored(y)
    for name in LIVE:
        _, hA, x, ys = live_products(cylinder_case, name)
        out[f"live-{name}/sha/A"] = np.array(hA)
        out[f"live-{name}/sha/x"] = np.array(sha(x))
        for working, (y, _, _) in ys.items():
            out[f"live-{name}/working{working}"] = stored(y)
    return out


def same_bits(got, gold, what):
    got = stored(got)
    assert got.shape == gold.shape, f"{what}: {got.shape} against {gold.shape}"
    bad = np.flatnonzero(got != gold)
    unit = "entries" if len(got) <= 8192 else f"blocks of {BLOCK} entries"
    assert not len(bad), f"{what}: {len(bad)} of {len(got)} {unit} differ from the recorded bits; first at {int(bad[0])}"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", SYNTHETIC)
def test_synthetic_products_give_the_recorded_bits(gold, name):
    c, A = synthetic_case(name)
    for k, h in input_hashes(c, A).items():
        assert h == str(gold[f"{name}/sha/{k}"]), f"{name}: the regenerated input {k} is not the recorded one (the generator drifted)"
    for f, y in synthetic_products(c, A).items():
        same_bits(y, gold[f"{name}/{f}"], f"{name}, {f}")


@pytest.mark.parametrize("name", LIVE)
def test_live_products_give_the_recorded_bits(gold, cylinder_case, name):
    _, forms, *counters = LIVE[name]
    info, hA, x, ys = live_products(cylinder_case, name)
    assert sha(x) == str(gold[f"live-{name}/sha/x"]), "the regenerated x is not the recorded one (the generator drifted)"
    assert hA == str(gold[f"live-{name}/sha/A"]), "the assembled matrix is not the recorded one: not the product's doing"
    for working, (y, op32, dr) in ys.items():
        assert (op32, dr) == counters[working], (working, op32, dr)
        same_bits(y, gold[f"live-{name}/working{working}"], f"{name}, working = {working}")
    assert (info["product_form64"], info["product_form32"]) == forms, info
