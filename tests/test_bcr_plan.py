"""Host logic of the solid cycle's exact coarse solve (vasp_amd/csrc/fsi_bcr.hip): the planner on real wall graphs, no device.

The level is solved by block cyclic reduction over breadth-first levels of the solid vertices; what the planner must deliver is
(i) a numbering in which the operator is block tridiagonal - every edge of the graph joins equal or neighbouring levels - with
blocks of one cross-section of the wall, and (ii) sizes that decide whether the method is used at all.  The arithmetic of the
reduction itself is restated in numpy on that numbering (``kernel_shim.bcr_reference``) and solved against a dense factorisation; the HIP
kernels are held to the same dense solve on the GPU (tests/test_gpu_parity.py::test_exact_coarse_solve_*)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from vasp_amd import capi
from kernel_shim import bcr_reference


def wall_graph(tets):
    """Vertex graph of the SOLID cells of a generated offset-stenosis mesh: (nc, cptr, ccol) with a self loop per vertex."""
    from vasp_amd.meshgen import generate
    m = generate(tets, seed=0)
    solid = m["tets"][m["cell_markers"] == 2]
    verts = np.unique(solid)
    loc = -np.ones(len(m["coords"]), dtype=np.int64)
    loc[verts] = np.arange(len(verts))
    t = loc[solid]
    r = np.repeat(t, 4, axis=1).ravel()
    c = np.tile(t, (1, 4)).ravel()
    G = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(len(verts), len(verts)))
    G.sum_duplicates()
    G.sort_indices()
    return len(verts), G.indptr.astype(np.int64), G.indices.astype(np.int32), m["shape"]


def plan(nc, cptr, ccol):
    lib = capi.load_library()
    stats = np.zeros(8, dtype=np.int64)
    pos, level = np.empty(nc, dtype=np.int32), np.empty(nc, dtype=np.int32)
    rc = lib.fsi_bcr_plan_graph(nc, capi._ptr(cptr), capi._ptr(ccol), capi._ptr(stats), capi._ptr(pos), capi._ptr(level))
    assert rc == 0
    keys = ("usable", "blocks", "max_block", "levels", "bytes32", "bytes64", "setup_flops", "launches")
    return dict(zip(keys, (int(v) for v in stats))), pos, level


@pytest.mark.parametrize("tets", [6000, 48000])
def test_planner_numbers_a_vessel_wall_block_tridiagonally(tets):
    nc, cptr, ccol, (ncs, nr, nx) = wall_graph(tets)
    st, pos, level = plan(nc, cptr, ccol)
    assert st["usable"] == 1 and st["blocks"] == level.max() + 1
    # every edge joins equal or neighbouring levels; pos is a permutation that ascends with the level
    rows = np.repeat(np.arange(nc), np.diff(cptr))
    assert np.abs(level[rows] - level[ccol]).max() <= 1
    assert np.array_equal(np.sort(pos), np.arange(nc))
    order = np.argsort(pos)
    assert np.all(np.diff(level[order]) >= 0)
    # blocks are cross-sections of the wall: two rings of the O-grid plus the cell centres between two stations
    ring = 4 * ncs
    assert st["max_block"] <= 3 * 3 * ring and st["blocks"] >= nx
    assert st["levels"] == int(np.ceil(np.log2(st["blocks"]))) and st["launches"] == 2 * st["levels"] + 1
    # operators: about five dense blocks per BFS level, FP32
    m = 3 * np.bincount(level)
    assert 2.0 * 4 * (m.astype(float) ** 2).sum() < st["bytes32"] < 8.0 * 4 * (m.astype(float) ** 2).sum()


def test_reduction_on_the_planners_numbering_solves_the_system():
    """A random positive definite 3x3-block operator on the 6 000-tet wall graph, renumbered by the planner: block tridiagonal
    (no entry outside the three block diagonals), and the reduction as scheduled (FP32 operators) solves it to FP32 accuracy."""
    nc, cptr, ccol, _ = wall_graph(6000)
    st, pos, level = plan(nc, cptr, ccol)
    rng = np.random.default_rng(0)
    nb = len(ccol)
    vals = rng.standard_normal((nb, 3, 3)) * 0.2
    B = sp.bsr_matrix((vals, ccol, cptr), shape=(3 * nc, 3 * nc)).tocsr()
    A = (B @ B.T + 4.0 * sp.identity(3 * nc)).toarray()            # SPD; pattern: two rings of the graph ...
    G = sp.csr_matrix((np.ones(nb), ccol, cptr), shape=(nc, nc))
    mask = sp.kron(G, np.ones((3, 3))).toarray() > 0
    A = np.where(mask, A, 0.0) + 30.0 * np.eye(3 * nc)              # ... cut back to the graph itself (kept definite by the shift)
    perm = np.empty(3 * nc, dtype=np.int64)
    for c in range(3):
        perm[3 * pos + c] = 3 * np.arange(nc) + c
    Ap = A[np.ix_(perm, perm)]
    m = 3 * np.bincount(level)
    off = np.concatenate([[0], np.cumsum(m)])
    K = len(m)
    for k in range(K):                                              # nothing outside the three block diagonals
        lo, hi = off[max(k - 1, 0)], off[min(k + 2, K)]
        assert not Ap[off[k]:off[k + 1], :lo].any() and not Ap[off[k]:off[k + 1], hi:].any()
    solve = bcr_reference(Ap, off)
    rhs = rng.standard_normal(3 * nc)
    x = solve(rhs)
    assert np.linalg.norm(Ap @ x - rhs) <= 2e-6 * np.linalg.norm(rhs)


def test_planner_declines_a_graph_that_is_not_a_thin_wall():
    """A 3-D block of vertices has breadth-first levels of thousands of unknowns: dense operators would cost more than the
    sweeps they replace, and the planner says so instead of building them."""
    n = 30
    idx = np.arange(n ** 3).reshape(n, n, n)
    pairs = []
    for ax in range(3):
        a = np.take(idx, np.arange(n - 1), axis=ax).ravel()
        b = np.take(idx, np.arange(1, n), axis=ax).ravel()
        pairs += [(a, b), (b, a)]
    r = np.concatenate([p[0] for p in pairs] + [np.arange(n ** 3)])
    c = np.concatenate([p[1] for p in pairs] + [np.arange(n ** 3)])
    G = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n ** 3, n ** 3))
    G.sort_indices()
    st, _, _ = plan(n ** 3, G.indptr.astype(np.int64), G.indices.astype(np.int32))
    assert st["usable"] == 0 and st["max_block"] > 2000
