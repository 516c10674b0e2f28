"""The displacement rows of the outer product without the zero dv values (vasp_amd/csrc/fsi_product.hip): the split pair form
a Jacobian refresh builds - k_drows_extract with its node classification, k_drows_offsets, k_drows_gather_dv - and the product
that reads it, k_spmv_node6s, through the test shim (shim_drows_split, shim_spmv_node6s).

The reference of the product is the six-value kernel k_spmv_node6c on the same inputs: the new product must give the same
numbers, ``np.array_equal`` (which lets only the sign of a zero differ).  It is also held against the extended-precision host
product of tests/test_gpu_product_kernels.py with the bound those tests use for k_spmv_node6c, (L + 8) eps S.  The arrays of the
split form are checked entry by entry against the six-value pair form restated in tests/kernel_shim.py.

Synthetic node graphs: N2 in {1, 7, 9, 4097} (no multiple of the eight XCD shares), node degrees 1, 63, 64, 65 and 130 (the
64-lane loop boundary), all nodes uncoupled, all coupled, coupled nodes first, last and alternating, nodes and a whole case
without pressure columns, a fluid row with a single non-zero dv, and a d row with a foreign entry (the form is refused).

A live context at the end: three time steps of the cylinder fixture give the states and Krylov counts that the parent commit
gave (tests/golden/krylov_zeros_cylinder.npz, recorded with it), bit for bit."""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest

import kernel_shim as ks
from test_gpu_product_kernels import EPS        # the product tests' bound is (L + 8) * EPS * S with their EPS

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
_NEW = {"shim_drows_split": "l" + "p" * 9 + "l", "shim_spmv_node6s": "ll" + "p" * 6 + "l" + "pppp" + "l" + "p"}


def shim(name, *args):
    """one of this file's shim entry points (bound here: tests/kernel_shim.py lists the older ones)"""
    fn = getattr(ks.load(), name)
    if fn.argtypes is None:
        fn.argtypes = [ks._CT[c] for c in _NEW[name]]
        fn.restype = C.c_int
    rc = fn(*[ks._arg(a) for a in args])
    if rc not in (0, ks.LAUNCH_REFUSED):
        raise RuntimeError(f"{name}: {ks.load().shim_last_error().decode()}")
    return rc


# name: (N2, V, mono_graph knobs).  Degree 1 is a diag_only node; the heavy nodes get the degree named plus one (their own rank,
# unless it is among the neighbours drawn; the edges test below holds the degrees that matter)
CASES = {
    "N1": (1, 1, {}),
    "N7": (7, 3, dict(diag_only=[2])),
    "N9_V0": (9, 0, dict(heavy=[4], heavy_deg=[9])),
    "N4097": (4097, 1500, dict(max_deg=10, heavy=[0, 1000, 2000, 3000, 4096], heavy_deg=[62, 63, 64, 129, 128], diag_only=[7, 4095],
                               no_padj=range(40, 60))),
}
PATTERNS = ("none", "all", "first", "last", "alternating")


def coupled_nodes(N2, pattern):
    r = np.arange(N2)
    return {"none": r < 0, "all": r >= 0, "first": r < (N2 + 1) // 2, "last": r >= N2 // 2, "alternating": r % 2 == 0}[pattern]


@functools.lru_cache(maxsize=None)
def graph(name):
    N2, V, kw = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 11)
    g = ks.mono_graph(N2, V, rng, **kw)
    rowptr, cols, _ = ks.expand_cols(N2, *g)
    entry, slot = ks.drows_entries(N2, rowptr, g[0])
    nnz = int(rowptr[-1])
    A = rng.uniform(-1, 1, nnz)
    A[entry[slot < 0]] = 0.0                                         # the d rows in the pair pattern
    x = rng.standard_normal(6 * N2 + V)
    return dict(N2=N2, V=V, g=g, rowptr=rowptr, cols=cols, entry=entry, slot=slot, A=A, x=x)


def matrix(c, coupled):
    """the case's matrix with the dv entries of the uncoupled nodes' d rows set to zero"""
    A = c["A"].copy()
    node = (np.searchsorted(c["rowptr"], c["entry"], side="right") - 1) // 6
    dv = (c["slot"] >= 0) & (c["slot"] % 6 >= 3)
    A[c["entry"][dv & ~coupled[node]]] = 0.0
    return A


def split(c, A, dvcap=None):
    """the split form as the shim builds it from A: (flag, ad64, dd, cdeg, doff, dv), every output starting as a sentinel"""
    N2, rowptr, nadj_ptr = c["N2"], c["rowptr"], c["g"][0]
    npairs = int(nadj_ptr[-1])
    dvcap = npairs if dvcap is None else dvcap
    ad64, dd, dv = np.full(6 * npairs, np.nan), np.full(3 * npairs, np.nan), np.full(3 * dvcap, np.nan)
    cdeg, doff, flag = np.full(N2, -5, dtype=np.int32), np.full(N2 + 1, -9, dtype=np.int64), np.zeros(1, dtype=np.int32)
    shim("shim_drows_split", N2, rowptr, np.ascontiguousarray(A[:rowptr[6 * N2]]), nadj_ptr, ad64, flag, dd, cdeg, doff, dv, dvcap)
    return int(flag[0]), ad64, dd, cdeg, doff, dv


def check_split(c, A, coupled, got):
    """the arrays of the split form against the six-value pair form of the same matrix (bitwise) and the classification"""
    N2, nadj_ptr = c["N2"], c["g"][0]
    flag, ad64, dd, cdeg, doff, dv = got
    ref, bad = ks.drows_extract(N2, c["rowptr"], A, nadj_ptr)
    assert not bad and flag == 0
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)      # noqa: E731
    np.testing.assert_array_equal(bits(ad64), bits(ref))
    ref6 = ref.reshape(-1, 6)
    np.testing.assert_array_equal(bits(dd), bits(ref6[:, :3].ravel()))
    deg = np.diff(nadj_ptr)
    np.testing.assert_array_equal(cdeg, np.where(coupled, deg, 0))
    start = np.concatenate([[0], np.cumsum(np.where(coupled, deg, 0))])
    np.testing.assert_array_equal(doff[:N2], np.where(coupled, start[:N2], -1))
    assert doff[N2] == start[N2]
    pair_node = np.repeat(np.arange(N2), deg)
    want = ref6[coupled[pair_node], 3:].ravel()
    np.testing.assert_array_equal(bits(dv[:len(want)]), bits(want))
    assert np.isnan(dv[len(want):]).all(), "k_drows_gather_dv wrote behind the coupled pairs"


def products(c, A, got):
    """(the split product, the six-value product) of the same matrix; y starts as NaN"""
    N2, V, rowptr, cols, x = c["N2"], c["V"], c["rowptr"], c["cols"], c["x"]
    nadj_ptr, nadj, _, _, vrank = c["g"]
    _, ad64, dd, _, doff, dv = got
    n = 6 * N2 + V
    y6, ys = np.full(n, np.nan), np.full(n, np.nan)
    ks.call("shim_spmv_node6", N2, V, rowptr, cols, A, vrank, nadj_ptr, nadj, len(nadj), x, y6, ad64)
    dv = np.where(np.isnan(dv), 7.0e300, dv)                      # what no coupled node owns must not be read: it would show
    assert shim("shim_spmv_node6s", N2, V, rowptr, cols, A, vrank, nadj_ptr, nadj, len(nadj), x, ys, dd, dv, len(dv) // 3, doff) == 0
    assert not np.isnan(y6).any() and not np.isnan(ys).any()
    return ys, y6


def test_the_cases_reach_the_edges():
    big = graph("N4097")
    deg = np.diff(big["g"][0])
    assert {1, 63, 64, 65, 130} <= set(deg.tolist()), sorted(set(deg.tolist()))[-6:]
    assert all(CASES[k][0] % 8 for k in CASES)
    pdeg = np.diff(big["g"][2])
    assert (pdeg == 0).any() and (pdeg > 0).any() and CASES["N9_V0"][1] == 0


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", CASES)
def test_split_form_and_product(name, pattern):
    c = graph(name)
    coupled = coupled_nodes(c["N2"], pattern)
    A = matrix(c, coupled)
    got = split(c, A)
    check_split(c, A, coupled, got)
    ys, y6 = products(c, A, got)
    assert np.array_equal(ys, y6), (f"{int((ys != y6).sum())} entries differ from k_spmv_node6c; first at "
                                    f"{int(np.flatnonzero(ys != y6)[0])}")
    ref, S, L = ks.csr_product(c["rowptr"], c["cols"], A, c["x"])
    ks.check(ys, ref, (L + 8) * EPS * S, "k_spmv_node6s against the host product")


def test_a_single_dv_entry_on_a_fluid_row_couples_its_node():
    c = graph("N4097")
    coupled = coupled_nodes(c["N2"], "first")
    A = matrix(c, coupled)
    r = c["N2"] - 3                                                  # an uncoupled node: one dv entry of its d_z row comes back
    node = (np.searchsorted(c["rowptr"], c["entry"], side="right") - 1) // 6
    mine = np.flatnonzero((node == r) & (c["slot"] >= 0) & (c["slot"] % 6 == 5))
    assert len(mine) and not coupled[r]
    A[c["entry"][mine[-1]]] = 2.0 ** -40
    coupled = coupled.copy()
    coupled[r] = True
    got = split(c, A)
    check_split(c, A, coupled, got)
    ys, y6 = products(c, A, got)
    assert np.array_equal(ys, y6)


def test_a_foreign_entry_in_a_d_row_refuses_the_form():
    """the verdict of the extraction (flag bit 0) is what a refresh reads: the split form is not adopted, the full product runs"""
    c = graph("N7")
    A = matrix(c, coupled_nodes(c["N2"], "alternating"))
    off = c["entry"][c["slot"] < 0]
    A[off[len(off) // 2]] = 2.0 ** -60
    flag = split(c, A)[0]
    assert flag == 1
    N2, V, rowptr, cols, x = c["N2"], c["V"], c["rowptr"], c["cols"], c["x"]
    nadj_ptr, nadj, _, _, vrank = c["g"]
    y = np.full(6 * N2 + V, np.nan)
    ks.call("shim_spmv_node6", N2, V, rowptr, cols, A, vrank, nadj_ptr, nadj, len(nadj), x, y, None)
    ref, S, L = ks.csr_product(rowptr, cols, A, x)
    ks.check(y, ref, (L + 8) * EPS * S, "the full product of the matrix with the foreign entry")


def test_split_product_without_its_arrays_is_refused():
    c = graph("N7")
    A = matrix(c, coupled_nodes(c["N2"], "all"))
    _, ad64, dd, _, doff, dv = split(c, A)
    N2, V, rowptr, cols, x = c["N2"], c["V"], c["rowptr"], c["cols"], c["x"]
    nadj_ptr, nadj, _, _, vrank = c["g"]
    for ptr, nb, d, o in ((None, nadj, dd, doff), (nadj_ptr, None, dd, doff), (nadj_ptr, nadj, None, doff), (nadj_ptr, nadj, dd, None)):
        y = np.full(6 * N2 + V, 17.0)
        rc = shim("shim_spmv_node6s", N2, V, rowptr, cols, A, vrank, ptr, nb, len(nadj), x, y, d, dv, len(dv) // 3, o)
        assert rc == ks.LAUNCH_REFUSED and np.all(y == 17.0)


# ---- a live context: the parent commit's numbers ------------------------------------------------------------------------------
CONFIGS = ("tight",          # driven to round-off: FP64 basis, FP64 products in the iterations
           "shipped")        # HipBackend's defaults and the problem's own tolerances: what the storage policy picks


def three_cylinder_steps(case, config):
    """three time steps of the cylinder fixture: (states [3][ndof], (Krylov iterations, solves, Newton iterations) after each)"""
    from test_gpu_parity import boundary_data
    from vasp_amd.capi import HipBackend
    ns = case[0]
    if config == "tight":
        kw = dict(atol=1e-11, rtol=1e-14, max_it=30, recompute=20, recompute_tstep=20)
        hb = HipBackend(case[1], lin_rtol=1e-11)
    else:
        kw = {k: ns[k] for k in ("atol", "rtol", "max_it", "recompute", "recompute_tstep")}
        hb = HipBackend(case[1])
    states, counts = [], []
    newton = 0
    for k in range(3):
        g, P = boundary_data(case, 1e-3 * (k + 1))
        hb.set_dirichlet_values(g)
        hb.set_interface_pressure(P)
        hist = hb.newton_solve(counter=k, first_step_num=0, lmbda=1.0, **kw)
        newton += len(hist)
        hb.shift()
        t = hb.timers()
        states.append(hb.get_state("n").copy())
        counts.append((int(t["krylov_iters"]), int(t["krylov_solves"]), newton))
    flags = int(hb.timers()["sweep_flags"])
    hb.close()
    return np.array(states), np.array(counts, dtype=np.int64), flags


@pytest.mark.parametrize("config", CONFIGS)
def test_cylinder_three_steps_give_the_parents_bits(cylinder_case, config):
    gold = np.load(GOLDEN / "krylov_zeros_cylinder.npz")
    states, counts, flags = three_cylinder_steps(cylinder_case, config)
    assert flags & 64, "the pair form was not adopted: the split product did not run"
    np.testing.assert_array_equal(counts, gold[f"{config}_counts"])
    ref = gold[f"{config}_states"]
    for k in range(len(ref)):                                        # (the shipped run keeps its last state only)
        got = states[len(states) - len(ref) + k]
        assert np.array_equal(got, ref[k]), f"{config}, state {k}: {int((got != ref[k]).sum())} entries differ from the parent's"
