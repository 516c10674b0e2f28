"""The Jacobian kernels of fsi_assembly.hip on an MI355X through libfsi_kernel_shim.so, one launch_jacobian at a time: the three
bodies of k_jacobian - (linear, 1 wave), (nonlinear, 1), (nonlinear, 2) - and k_jacobian_mfma with 1 and 2 waves per SIMD.

Reference: the complex-step element matrices of the project's oracle in extended precision (np.clongdouble, step 1e-40) from the same
FP64 geometry array, tables and state.  On cells that share no node (kernel_shim.element_cases("jac"), launched colour by colour
through the cell lists) every matrix entry receives one contribution and is compared with its element entry under the bound of its
(row field, column field) block, kernel_shim.K_JACOBIAN: |got - ref| <= K_B 2^-53 max_B |ref|, fluid and solid cells apart.  Entries of
blocks the reference has zero - the d rows of the nonlinear part, every column but d on a solid cell - keep their prefill bit for
bit.  The matrix-pipe and vector variants must agree with each other entry by entry under the same bounds.  One launch without
colours over the first 2000 cells of the tube, which share nodes, is compared with the summed element matrices of the FP64 C oracle
under the summed bounds, K + K / 4 for the oracle's own quarter (tests/test_kernel_references.py).

vals is prefilled with values of the size of the entry they will receive (random sign and factor in 0.5 .. 1), so that a kernel
that stores instead of adding is off by the prefill, and the rounding of the addition, u (|prefill| + |sum|) per contribution,
stays below the bound of the small blocks.

Largest error / bound observed on an MI355X per variant, kind and (row field, column field) block (the tests print every figure; -s
shows them).  One and two waves per SIMD gave the same figures; no block came near its bound:

    linear-1               fluid (d,d) 0.16  (v,v) 0.23                                   solid (d,d) 0.10  (d,v) 0.13  (v,v) 0.12
    nonlinear-1, -2        fluid (v,d) 0.13  (v,v) 0.20  (v,p) 0.21  (p,d) 0.17  (p,v) 0.16     solid (v,d) 0.11
    mfma-1, -2             fluid (v,d) 0.21  (v,v) 0.43  (v,p) 0.25  (p,d) 0.17  (p,v) 0.16     solid (v,d) 0.13
    mfma against vector    fluid (v,d) 0.21  (v,v) 0.55  (v,p) 0.30  (p,d) 0.10  (p,v) 0.12     solid (v,d) 0.19
    2000 cells that share nodes (FP64 C oracle, summed K + K / 4)      linear 0.18   nonlinear 0.24   mfma 0.31
"""
import numpy as np
import pytest

import kernel_shim as ks

pytestmark = pytest.mark.gpu

LD = ks.LD
NAN = float("nan")
F = ("d", "v", "p")
# (part, jac_waves, jac_mfma) of the five launch variants
VARIANTS = {"linear-1": (ks.PART_LINEAR, 1, 0), "nonlinear-1": (ks.PART_NONLINEAR, 1, 0), "nonlinear-2": (ks.PART_NONLINEAR, 2, 0),
            "mfma-1": (ks.PART_NONLINEAR, 1, 1), "mfma-2": (ks.PART_NONLINEAR, 2, 1)}


def run_jacobian(case, variant, prefill, colours=None):
    """one launch_jacobian: vals after (prefill before); colours: lists of cell ids, None for one launch over all cells"""
    part, waves, mfma = VARIANTS[variant]
    es, (sc, fl, so) = case.es, case.params
    nnz = int(es.rowptr[-1])
    vals = np.concatenate([prefill, np.full(ks.TAIL, NAN)])
    if colours is None:
        nc, cells, ptr = 0, None, None
    else:
        nc = len(colours)
        cells = np.concatenate([np.sort(c) for c in colours]).astype(np.int32)
        ptr = np.concatenate([[0], np.cumsum([len(c) for c in colours])]).astype(np.int64)
    ks.call("shim_elem_jacobian", part, waves, mfma, case.C, es.ndof, es.N2, case.geom, es.cell_dofs, case.kind, case.region, es.cell_rank,
            es.enbr, es.epnbr, sc, fl, so, case.Us, case.U1s, es.rowptr, es.nadj_ptr, nc, cells, ptr, vals)
    assert ks.tail_untouched(vals, nnz, NAN)
    return vals[:nnz]


def prefill_for(size, rng):
    """random values of the size of the entries they meet (size: |sum of the contributions| per entry), 0.37 x where that is zero"""
    s = rng.uniform(0.5, 1.0, len(size)) * rng.choice([-1.0, 1.0], len(size))
    return s * np.where(size > 0, size, 0.37).astype(np.float64)


def report(what, got, ref, kind, K):
    q = ks.block_ratios(got, ref, kind)
    for k, name in enumerate(("fluid", "solid")):
        print(f"RATIO {what} {name}: " + "  ".join(f"({F[i]},{F[j]}) {q[k, i, j] / K[k, i, j]:.3f}" for i in range(3) for j in range(3) if K[k, i, j]))


@pytest.fixture(scope="module")
def coloured():
    """the "jac" case, its reference, and the element matrices each variant leaves: {variant: [C][64][64] vals - prefill at the entries'
    positions, in extended precision}, with the untouched-prefill check done on the way"""
    case = ks.element_cases("jac")
    ref = case.jacobian_reference()
    es = case.es
    pos = ks.element_positions(es)
    assert len(np.unique(pos)) == pos.size == es.rowptr[-1]                  # cells that share no node: one contribution per entry, every entry met
    cells = np.arange(case.C)
    colours = [cells[1:2], cells[np.r_[0, 2:65]], cells[65:]]                # 1, 64 and the rest, ascending inside a colour
    out = {}
    for v, (part, _, _) in VARIANTS.items():
        r = ref[0 if part == ks.PART_LINEAR else 1]
        K = ks.K_JACOBIAN[0 if part == ks.PART_LINEAR else 1]
        # an entry the reference has zero inside a block that is not gets a prefill of the block's size
        size = np.abs(r).astype(np.float64)
        blockmax = (ks.block_bound(r, case.kind, np.ones((2, 3, 3))) / ks.U64).astype(np.float64)
        pre = np.empty(int(es.rowptr[-1]))
        pre[pos.ravel()] = prefill_for(np.where(size > 0, size, blockmax).ravel(), np.random.default_rng(len(v)))
        vals = run_jacobian(case, v, pre.copy(), colours)
        keep = (ks.block_bound(r, case.kind, K) == 0)
        assert keep.any() and np.all(r[keep] == 0)
        bad = vals[pos][keep].view(np.uint64) != pre[pos][keep].view(np.uint64)
        assert not bad.any(), f"{v}: {bad.sum()} entries of blocks the reference has zero were written"
        out[v] = (vals.astype(LD)[pos] - pre.astype(LD)[pos], pre[pos])
    return case, ref, out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_jacobian_cell_by_cell(coloured, variant):
    case, ref, out = coloured
    p = 0 if VARIANTS[variant][0] == ks.PART_LINEAR else 1
    r, K = ref[p], ks.K_JACOBIAN[p]
    got, pre = out[variant]
    report(f"jacobian {variant}", got, r, case.kind, K)
    bound = ks.block_bound(r, case.kind, K) + ks.U64 * (np.abs(pre) + 2 * np.abs(r))          # the block bound and the one addition to the prefill
    bound[ks.block_bound(r, case.kind, K) == 0] = 0
    err = np.abs(got - r)
    for k, name in enumerate(("fluid", "solid")):
        sel = case.kind == k
        worst = ks.worst_ratio(err[sel], bound[sel])
        print(f"RATIO jacobian {variant} {name} with the prefill's rounding: {worst:.3f}")
        assert worst <= 1.0, f"{variant}, {name} cells: an entry is at {worst:.2f} of its bound"


@pytest.mark.parametrize("waves", [1, 2])
def test_matrix_pipe_and_vector_variants_agree(coloured, waves):
    """k_jacobian_mfma against k_jacobian<PART_NONLINEAR> entry by entry, under the block bounds (both add to their own prefill: its
    rounding is added for both)"""
    case, ref, out = coloured
    r, K = ref[1], ks.K_JACOBIAN[1]
    (a, pa), (b, pb) = out[f"mfma-{waves}"], out[f"nonlinear-{waves}"]
    report(f"mfma-{waves} against nonlinear-{waves}", a, b, case.kind, K)
    bound = ks.block_bound(r, case.kind, K) + ks.U64 * (np.abs(pa) + np.abs(pb) + 4 * np.abs(r))
    bound[ks.block_bound(r, case.kind, K) == 0] = 0
    worst = ks.worst_ratio(np.abs(a - b), bound)
    print(f"RATIO mfma-{waves} against nonlinear-{waves}: {worst:.3f}")
    assert worst <= 1.0


@pytest.fixture(scope="module")
def shared():
    """the first 2000 cells of the tube (they share nodes: up to some 30 contributions per entry) and the FP64 C oracle's element
    matrices summed at their positions: per part (sum, sum of |terms|, summed block bounds with the oracle's quarter, contributions)"""
    case = ks.element_cases("tube").prefix(2000)
    es = case.es
    pos = ks.element_positions(es).ravel()
    J = case.jacobian_reference(case.oracle(impl="c"))
    nnz = int(es.rowptr[-1])
    sums = []
    for p in (0, 1):
        total, size, bound = np.zeros(nnz, dtype=LD), np.zeros(nnz, dtype=LD), np.zeros(nnz, dtype=LD)
        np.add.at(total, pos, J[p].astype(LD).ravel())
        np.add.at(size, pos, np.abs(J[p]).astype(LD).ravel())
        np.add.at(bound, pos, 1.25 * ks.block_bound(J[p], case.kind, ks.K_JACOBIAN[p]).ravel())
        sums.append((total, size, bound))
    n = np.bincount(pos, minlength=nnz)
    assert n.max() > 8 and n.min() >= 1                                       # every entry is met, the diagonal blocks of shared nodes many times
    return case, sums, n


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_jacobian_on_cells_that_share_nodes(shared, variant):
    """ncolours == 0: one launch over all cells, the contributions of an entry added by atomics in any order: n additions cost
    (n + 1) u (|prefill| + sum |terms|) on top of the summed block bounds.  Entries all of whose contributions are zero in
    the reference keep their prefill bit for bit."""
    case, sums, n = shared
    total, size, bound = sums[0 if VARIANTS[variant][0] == ks.PART_LINEAR else 1]
    pre = prefill_for(size.astype(np.float64), np.random.default_rng(5))
    vals = run_jacobian(case, variant, pre.copy(), None)
    quiet = size == 0
    assert quiet.any() and np.array_equal(vals[quiet].view(np.uint64), pre[quiet].view(np.uint64)), f"{variant}: an entry nothing adds to changed"
    full = bound + (n + 1) * ks.U64 * (np.abs(pre) + size)
    err = np.abs(vals.astype(LD) - pre.astype(LD) - total)
    worst = ks.worst_ratio(err[~quiet], full[~quiet])
    print(f"RATIO jacobian {variant} on 2000 cells that share nodes: {worst:.3f}")
    assert worst <= 1.0
