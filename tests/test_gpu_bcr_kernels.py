"""The exact coarse solve of the solid cycle by block cyclic reduction (vasp_amd/csrc/fsi_bcr.hip), one launch function at a
time through the test shim, then whole solves on synthetic tube graphs and on a live context, against FP64 restatements
(tests/kernel_shim.py: gj_inverse, bcr_reference, bcr_task_apply, tube_graph).

Bitwise, where nothing accumulates:
    k_bcr_fill       f * double(v) with f = 1 + shift on a node's own block (ld < 0), 1 elsewhere; dst = -1 skipped
    k_bcr_gather     b[3 pos[i] + c] = double(rc4[4 i + c]), the pad lane never read
    k_bcr_scatter    xc4[4 i + c] = float(x[3 pos[i] + c]), the pad lane written as 0
    k_bcr_copy32     the FP32 operator is float(X) of the FP64 inverse; nothing past m columns of an ld32 row
    k_bcr_gemm       o32 is float(c) of the stored FP64 value when both are written; nothing outside M x N
    whole solve      rc4 / xc4 path == float(FP64 path on double(rc4)); a repeated solve, and a refresh with the same values after
                     a failed one, give the same bits
Bounded, where it accumulates (eps = 2^-52, u = 2^-24, sums of magnitudes in FP64):
    inverse (FP64)   |X - A^-1| <= 8 (m + 32) eps |A^-1| |A| |A^-1|  elementwise, A^-1 from LAPACK (its own error is of the
                     same form and far below), and |A X - I| <= 8 (m + 32) eps |A| |X|: a Gauss-Jordan step contributes a few
                     eps |A^-1||A||A^-1|, over m pivots and the 32-wide panels
    gemm             |C - ref| <= (K1 + K2 + 8) eps (|alpha| sum |a||b| + |beta c|), ref in extended precision; an o32-only
                     product: that plus one FP32 ulp of ref
    apply            |y - ref| <= (ldw + 8) eps sum |w| |in| (+ eps |b_old| forward), ref of the FP32 weights in extended
                     precision
    whole solve      (a) every FP32 operator of the arena within one FP32 ulp of float(its FP64 definition from bcr_reference)
                         plus 64 (L + 1) kappa eps max |W| for the FP64 set-up (L reduction levels, kappa = cond_2 of the level)
                     (b) the GPU solve against bcr_task_apply of the GPU's own FP32 operators (FP64 vectors):
                         (maxld + 8) (2 L + 1) eps times that application carried out with |W| and |rhs|
                     (c) against a dense FP64 solve of A + shift blockdiag(A): normwise backward error
                         |A x - r| / (|A|_2 |x|) <= 8 (L + 1) u (the FP32 operators), so |x - x*| / |x*| <= kappa 8 (L + 1) u

Non-symmetric operators throughout (a transposed operand or inverse fails); block sizes at and around the 32-wide panels and
the 64 x 64 / 16-row tiles, batches that mix sizes (the k0 >= m early exit of k_bcr_panel), K not a multiple of 4, leading
dimensions wider than the operands, LDS vectors of 6 000 unknowns.  A vanished, non-finite or FP32-overflowing pivot / operator
must raise the flag (ready = 0) and the next good refresh must clear it."""
import numpy as np
import pytest
import scipy.linalg as sla

import kernel_shim as ks

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
U32 = 2.0 ** -24
SENT32 = np.float32(-7.25)
SENT64 = 12345.678


def ld4(c):
    return (c + 3) & ~3


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- launch_bcr_invert ----------------------------------------------------------------------------------------------------------
def block(m, kind, rng):
    """definite: B B^T / m + I plus a skew part; dominant: non-symmetric, strictly diagonally dominant"""
    B = rng.standard_normal((m, m))
    if kind == "definite":
        S = rng.standard_normal((m, m))
        return B @ B.T / m + np.eye(m) + 0.3 * (S - S.T) / np.sqrt(m)
    return B + np.diag(np.abs(B).sum(axis=1) + 1.0)


def run_invert(blocks, ld32s=None, o32=True):
    ms = [len(A) for A in blocks]
    desc, n64, n32, offs = ks.bcr_inverse_layout(ms, ld32s if o32 else [-1] * len(ms))
    a64 = np.full(n64, np.nan)                                   # the panel scratch must be written before it is read
    for A, o in zip(blocks, offs):
        a64[o:o + A.size] = A.ravel()
    a32 = np.full(max(n32, 1), SENT32, dtype=np.float32)
    flag = np.zeros(1, dtype=np.int32)
    ks.call("shim_bcr_invert", len(blocks), desc, a64, n64, a32, max(n32, 1), flag)
    X = [a64[o:o + m * m].reshape(m, m) for o, m in zip(offs, ms)]
    return X, a32, desc, int(flag[0])


def check_inverse(A, X, what):
    m = len(A)
    ref = np.linalg.inv(A)
    ai, aa = np.abs(ref), np.abs(A)
    ks.check(X, ref, 8 * (m + 32) * EPS * (ai @ aa @ ai), what + " inverse")
    ks.check(A @ X, np.eye(m), 8 * (m + 32) * EPS * (aa @ np.abs(X)), what + " A X - I")


def check_copy32(X, a32, d, what):
    o32, m, ld32 = int(d[1]), int(d[4]), int(d[5])
    rows = a32[o32:o32 + m * ld32].reshape(m, ld32)
    assert np.array_equal(rows[:, :m], X.astype(np.float32)), what + ": FP32 copy is not float(X)"
    assert (rows[:, m:] == SENT32).all(), what + ": written past m columns"


SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 97, 216, 432, 1998]


@pytest.mark.parametrize("kind", ["definite", "dominant"])
def test_inverse_one_size_at_a_time(kind):
    rng = np.random.default_rng(1 if kind == "definite" else 2)
    for m in SIZES:
        A = block(m, kind, rng)
        (X,), a32, desc, flag = run_invert([A], ld32s=[ld4(m) + 4])
        assert flag == 0, m
        check_inverse(A, X, f"{kind} m={m}")
        check_copy32(X, a32, desc[0], f"{kind} m={m}")


@pytest.mark.parametrize("kind", ["definite", "dominant"])
def test_inverse_of_a_batch_of_mixed_sizes(kind):
    """one launch sequence for blocks of every size: the smaller ones run out of panels first (k_bcr_panel's early exit) while
    the larger ones go on; a block without an FP32 copy is left alone by k_bcr_copy32"""
    rng = np.random.default_rng(3)
    ms = [33, 1, 97, 2, 64, 31, 432, 3, 65, 216, 32, 63]
    blocks = [block(m, kind, rng) for m in ms]
    ld32s = [ld4(m) + 8 * (k % 2) for k, m in enumerate(ms)]
    ld32s[4] = -1
    X, a32, desc, flag = run_invert(blocks, ld32s=ld32s)
    assert flag == 0
    for A, Xk, d in zip(blocks, X, desc):
        check_inverse(A, Xk, f"{kind} batch m={len(A)}")
        if d[1] >= 0:
            check_copy32(Xk, a32, d, f"{kind} batch m={len(A)}")
    desc32 = desc[desc[:, 1] >= 0]
    used = np.zeros(len(a32), dtype=bool)
    for d in desc32:
        used[d[1]:d[1] + d[4] * d[5]] = True
    assert (a32[~used] == SENT32).all()


def _bad_blocks(rng):
    out = []
    for k in (0, 31, 32, 33):                                       # an exactly zero pivot at k
        A = block(40, "dominant", rng)
        A[k, :] = 0.0
        out.append((f"zero row {k}", A))
    A = block(40, "dominant", rng)                                  # a pivot that vanishes only after elimination: 1 - 1 * 1
    A[:2, :] = 0.0
    A[:2, :2] = 1.0
    A[:2, 2:] = 0.01 * rng.standard_normal((2, 38))
    A[1, 2:] = A[0, 2:]
    out.append(("pivot vanishes after elimination", A))
    for v in (np.nan, np.inf):
        A = block(40, "dominant", rng)
        A[17, 5] = v
        out.append((f"{v} entry", A))
    out.append(("FP64-finite inverse beyond FLT_MAX", 1e-39 * np.eye(40)))
    return out


def test_inverse_flag():
    """the flag is raised by a vanished or non-finite pivot and by an inverse that is finite in FP64 but not in FP32 (the
    operator the solve would stream); a good batch leaves it 0, and the good blocks of a flagged batch are still inverted"""
    rng = np.random.default_rng(4)
    good = [block(m, "dominant", rng) for m in (33, 40, 5)]
    assert run_invert(good)[3] == 0
    assert ks.gj_inverse(_bad_blocks(rng)[4][1])[1]                  # (the restatement agrees that this one breaks down)
    for what, B in _bad_blocks(rng):
        X, a32, desc, flag = run_invert([good[0], B, good[2]])
        assert flag == 1, what
        for k in (0, 2):
            check_inverse(good[k], X[k], what + ": good block")
            check_copy32(X[k], a32, desc[k], what + ": good block")


# ---- launch_bcr_gemm -------------------------------------------------------------------------------------------------------------
MS = [1, 15, 16, 17, 63, 64, 65, 130]
KS = [0, 1, 3, 4, 5, 32, 433]
ALPHAS, BETAS = [-1.0, 1.0, 0.37], [0.0, 1.0, -0.5]


def gemm_case(ntasks, seed):
    """ntasks products in one arena: A1 [M][K1] (lda1 = K1 + pad), B1 [K1][N] (ldb1 = N + pad), the same for the second product
    (absent as a2 = -1 or K2 = 0 in some), C [M][ldc] and / or an FP32 [M][ld32] output; C prefilled with NaN where beta = 0"""
    rng = np.random.default_rng(seed)
    a64, idesc, ddesc, regions = [np.zeros(0)], [], [], []
    n64, n32 = 0, 0

    def put(arr):
        nonlocal n64
        o = n64
        a64.append(np.ravel(arr))
        n64 += arr.size
        return o
    for t in range(ntasks):
        M, N = MS[t % len(MS)], MS[(3 * t + 1) % len(MS)]
        K1, K2 = KS[t % len(KS)], KS[(2 * t + 3) % len(KS)]
        alpha, beta = ALPHAS[(t // 2) % 3], BETAS[(t // 3) % 3]
        mode = t % 3                                               # 0: c only, 1: o32 only, 2: both
        if mode == 1:
            beta = 0.0
        p1, p2 = 1 + t % 3, 2 - t % 2
        A1 = rng.standard_normal((M, max(K1, 1) + p1)); B1 = rng.standard_normal((max(K1, 1), N + p2))
        A2 = rng.standard_normal((M, max(K2, 1) + p2)); B2 = rng.standard_normal((max(K2, 1), N + p1))
        oa1, ob1, oa2, ob2 = put(A1), put(B1), put(A2), put(B2)
        if t % 5 == 4:
            oa2 = -1                                               # second product absent
        ldc = N + (t % 4)
        C0 = rng.standard_normal((M, ldc))
        C0[:, N:] = SENT64
        if beta == 0.0:
            C0[:, :N] = np.nan                                     # must not be read
        oc = put(C0) if mode != 1 else -1
        ld32 = N + 4 - (t % 4) if mode != 0 else 0
        o32 = -1
        if mode != 0:
            o32 = n32
            n32 += M * ld32 + 3
        idesc.append([oa1, ob1, oa2, ob2, oc, o32, M, N, K1, K2, A1.shape[1], B1.shape[1], A2.shape[1], B2.shape[1], ldc, ld32])
        ddesc.append([alpha, beta])
        regions.append(dict(A1=A1[:, :K1], B1=B1[:K1, :N], A2=A2[:, :K2] if oa2 >= 0 else None, B2=B2[:K2, :N], C0=C0.copy(), M=M,
                            N=N, K1=K1, K2=K2 if oa2 >= 0 else 0, alpha=alpha, beta=beta, oc=oc, ldc=ldc, o32=o32, ld32=ld32))
    return (np.concatenate(a64), np.asarray(idesc, dtype=np.int64), np.asarray(ddesc, dtype=np.float64), max(n32, 1), regions)


def run_gemm(a64, idesc, ddesc, n32):
    a64 = a64.copy()
    a32 = np.full(n32, SENT32, dtype=np.float32)
    flag = np.zeros(1, dtype=np.int32)
    ks.call("shim_bcr_gemm", len(idesc), idesc, ddesc, a64, len(a64), a32, n32, flag)
    return a64, a32, int(flag[0])


@pytest.mark.parametrize("seed", [0, 1])
def test_gemm_batch_of_shapes(seed):
    a64_in, idesc, ddesc, n32, regions = gemm_case(24, seed)
    a64, a32, flag = run_gemm(a64_in, idesc, ddesc, n32)
    assert flag == 0
    touched64 = np.zeros(len(a64), dtype=bool)
    touched32 = np.zeros(n32, dtype=bool)
    for t, r in enumerate(regions):
        M, N, ld = r["M"], r["N"], np.longdouble
        prod = np.zeros((M, N), dtype=ld)
        S = np.zeros((M, N))
        for A, B in ((r["A1"], r["B1"]), (r["A2"], r["B2"])):
            if A is not None and A.shape[1] > 0:
                prod += A.astype(ld) @ B.astype(ld)
                S += np.abs(A) @ np.abs(B)
        ref = r["alpha"] * prod
        bound = (r["K1"] + r["K2"] + 8) * EPS * abs(r["alpha"]) * S
        if r["beta"] != 0.0 and r["oc"] >= 0:
            ref = ref + r["beta"] * r["C0"][:, :N].astype(ld)
            bound = bound + 8 * EPS * np.abs(r["beta"] * r["C0"][:, :N])
        ref = ref.astype(np.float64)
        what = f"gemm {t}: M={M} N={N} K=({r['K1']},{r['K2']}) alpha={r['alpha']} beta={r['beta']}"
        if r["oc"] >= 0:
            C = a64[r["oc"]:r["oc"] + M * r["ldc"]].reshape(M, r["ldc"])
            touched64[r["oc"]:r["oc"] + M * r["ldc"]] = True
            ks.check(C[:, :N], ref, bound, what)
            assert (C[:, N:] == SENT64).all(), what + ": written past N"
        if r["o32"] >= 0:
            O = a32[r["o32"]:r["o32"] + M * r["ld32"]].reshape(M, r["ld32"])
            touched32[r["o32"]:r["o32"] + M * r["ld32"]] = True
            if r["oc"] >= 0:
                assert np.array_equal(O[:, :N], C[:, :N].astype(np.float32)), what + ": o32 is not float(c)"
            else:
                ks.check(O[:, :N], ref, bound + ulp32(ref), what + " (o32)")
            assert (O[:, N:] == SENT32).all(), what + ": o32 written past N"
    assert np.array_equal(a64[~touched64], a64_in[~touched64]), "an operand or a gap was written"
    assert (a32[~touched32] == SENT32).all()


def test_gemm_flags_an_operator_beyond_flt_max():
    """an FP32 output that overflows (finite in FP64) raises the flag; the same product without the FP32 output does not"""
    A, B = np.full((5, 3), 1e20), np.full((3, 6), 1e20)
    a64 = np.concatenate([A.ravel(), B.ravel(), np.zeros(30)])
    for o32, want in ((0, 1), (-1, 0)):
        idesc = np.array([[0, 15, -1, -1, 33, o32, 5, 6, 3, 0, 3, 6, 0, 0, 6, 6]], dtype=np.int64)
        out, a32, flag = run_gemm(a64, idesc, np.array([[1.0, 0.0]]), 32)
        assert flag == want
        np.testing.assert_allclose(out[33:63], 3e40, rtol=4 * EPS)


# ---- launch_bcr_apply ------------------------------------------------------------------------------------------------------------
ROWS = [1, 2, 3, 4, 5, 15, 16, 17, 65, 433]


def apply_case(forward, widths, seed, pad=0):
    """one task per (rows, segment lengths): inputs from the first part of the vectors (b and x mixed), outputs behind them,
    disjoint; W FP32 with the padding columns up to ldw zero (as the planner's arena holds them)"""
    rng = np.random.default_rng(seed)
    nin = max(sum(w) for _, w in widths) + 64
    nout = sum(r for r, _ in widths)
    n = nin + nout + 7
    b, x = rng.standard_normal(n), rng.standard_normal(n)
    tdesc, Ws, w0, out = [], [], 0, nin
    for t, (rows, lens) in enumerate(widths):
        cols = sum(lens)
        ldw = ld4(cols) + pad
        segs, o = [], int(rng.integers(0, nin - cols + 1))
        for k, L in enumerate(lens):
            segs.append([o, L, (t + k) % 2])
            o += L
        W = np.zeros((rows, ldw), dtype=np.float32)
        W[:, :cols] = rng.standard_normal((rows, cols)).astype(np.float32)
        tdesc.append([w0, rows, ldw, out, len(lens)] + sum(segs + [[0, 0, 0]] * (3 - len(segs)), []))
        Ws.append(W.ravel())
        w0 += W.size
        out += rows
    return np.asarray(tdesc, dtype=np.int64), np.concatenate(Ws), b, x


def check_apply(forward, tdesc, W, b0, x0):
    b, x = b0.copy(), x0.copy()
    ks.call("shim_bcr_apply", int(forward), len(tdesc), tdesc, W, len(W), b, x, len(b))
    written = np.zeros(len(b), dtype=bool)
    for t in tdesc:
        rows, ldw, out = int(t[1]), int(t[2]), int(t[3])
        Wt = W[t[0]:t[0] + rows * ldw].reshape(rows, ldw).astype(np.float64)
        v = np.concatenate([(x0 if t[7 + 3 * k] else b0)[t[5 + 3 * k]:t[5 + 3 * k] + t[6 + 3 * k]] for k in range(int(t[4]))])
        cols = len(v)
        prod = (Wt[:, :cols].astype(np.longdouble) @ v.astype(np.longdouble))
        bound = (ldw + 8) * EPS * (np.abs(Wt[:, :cols]) @ np.abs(v))
        what = f"{'forward' if forward else 'backward'} rows={rows} ldw={ldw} nseg={t[4]}"
        if forward:
            ref = (b0[out:out + rows] + prod).astype(np.float64)
            ks.check(b[out:out + rows], ref, bound + EPS * np.abs(ref), what)
        else:
            ks.check(x[out:out + rows], prod.astype(np.float64), bound, what)
        written[out:out + rows] = True
    kept = b if not forward else x
    assert np.array_equal(kept, b0 if not forward else x0), "the other vector was written"
    mine, mine0 = (b, b0) if forward else (x, x0)
    assert np.array_equal(mine[~written], mine0[~written]), "written outside the tasks' rows"


@pytest.mark.parametrize("forward", [True, False])
def test_apply_rows_and_widths(forward):
    widths = [(r, lens) for r, lens in zip(ROWS * 3, [[1], [3], [2, 3], [5, 1, 7], [33], [30, 33], [66, 3], [3, 216, 30],
                                                       [130], [255], [257], [216, 432], [3, 3, 3], [1, 1], [17, 0, 5], [64],
                                                       [100, 100, 100], [13, 2], [432, 30, 33], [65], [7, 9], [31], [4, 4],
                                                       [2, 2, 2], [40], [1], [6], [11, 3], [99], [3, 432]])]
    tdesc, W, b, x = apply_case(forward, widths, 10 + forward)
    check_apply(forward, tdesc, W, b, x)
    tdesc, W, b, x = apply_case(forward, widths[:10], 20 + forward, pad=8)      # ldw beyond the operator's columns
    check_apply(forward, tdesc, W, b, x)


@pytest.mark.parametrize("forward", [True, False])
def test_apply_with_the_widest_input(forward):
    """three segments of 2 000 unknowns: 6 000 doubles (48 KB) of LDS per workgroup, the planner's largest task"""
    widths = [(r, [2000, 2000, 2000]) for r in (1, 17, 433)] + [(65, [1998, 3]), (5, [300])]
    tdesc, W, b, x = apply_case(forward, widths, 30 + forward)
    check_apply(forward, tdesc, W, b, x)


# ---- fill / gather / scatter -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0.0, 2e-4, 0.5])
def test_fill_scales_only_a_nodes_own_block(shift):
    rng = np.random.default_rng(int(shift * 1e4) + 5)
    nblk = 3000
    ldabs = rng.integers(3, 40, nblk)
    ld = np.where(rng.random(nblk) < 0.3, -ldabs, ldabs).astype(np.int32)
    size = 2 * ldabs + 3
    dst = np.concatenate([[0], np.cumsum(size + 2)[:-1]]).astype(np.int64)
    dst[rng.random(nblk) < 0.1] = -1
    n64 = int((size + 2).sum())
    cvals = rng.standard_normal(9 * nblk).astype(np.float32)
    a64 = np.full(n64, SENT64)
    ks.call("shim_bcr_fill", nblk, cvals, dst, ld, shift, a64, n64)
    ref = np.full(n64, SENT64)
    for e in np.flatnonzero(dst >= 0):
        f = 1.0 + shift if ld[e] < 0 else 1.0
        for c in range(3):
            ref[dst[e] + c * ldabs[e] + np.arange(3)] = f * cvals[9 * e + 3 * c:9 * e + 3 * c + 3].astype(np.float64)
    assert np.array_equal(a64, ref)


def test_gather_and_scatter_go_through_pos():
    rng = np.random.default_rng(6)
    nc, n = 5000, 3 * 5007
    pos = rng.permutation(n // 3)[:nc].astype(np.int32)
    rc4 = rng.standard_normal(4 * nc).astype(np.float32)
    rc4[3::4] = np.nan                                              # the pad lane is not read
    b = np.full(n, SENT64)
    ks.call("shim_bcr_gather", nc, pos, rc4, b, n)
    ref = np.full(n, SENT64)
    for c in range(3):
        ref[3 * pos.astype(np.int64) + c] = rc4[c::4].astype(np.float64)
    assert np.array_equal(b, ref)
    x = rng.standard_normal(n)
    xc4 = np.full(4 * nc, np.nan, dtype=np.float32)
    ks.call("shim_bcr_scatter", nc, pos, x, n, xc4)
    want = np.zeros((nc, 4), dtype=np.float32)
    for c in range(3):
        want[:, c] = x[3 * pos.astype(np.int64) + c].astype(np.float32)
    assert np.array_equal(xc4, want.ravel())


# ---- the whole solve on tube graphs (shim_bcr_run) ------------------------------------------------------------------------------
TUBES = {
    "K1": [[1]],
    "K2": [[1, 144]],
    "K3": [[72, 1, 144]],
    "K5": [[10, 11, 22, 72, 144]],
    "K8": [[11, 10, 1, 22, 72, 144, 11, 10]],
    "K9": [[10, 11, 22, 72, 144, 72, 22, 11, 1]],
    "K17": [[1, 10, 11, 22, 10, 1, 11, 22, 10, 1, 11, 22, 10, 11, 1, 10, 22]],
    "two tubes": [[1, 10, 11, 22, 72], [22, 11, 10, 1, 10, 11, 144, 1]],
}
VALUES = [(1e2, 0.3, 0.0), (1e5, 0.01, 2e-4), (1e2, 0.3, 0.5)]       # (kappa, skew, shift)


def solve_case(name, kappa, skew, shift, seed=0):
    rng = np.random.default_rng(seed)
    g = ks.tube_graph(TUBES[name], rng)
    v = ks.tube_values(g, kappa, rng, skew=skew)
    A = ks.tube_dense(g, v, shift)
    off = np.concatenate([[0], np.cumsum(g["m"])])
    return g, v, A, off, rng


def nlevels(g):
    return int(np.ceil(np.log2(len(g["m"])))) if len(g["m"]) > 1 else 0


@pytest.mark.parametrize("kappa,skew,shift", VALUES)
@pytest.mark.parametrize("name", list(TUBES))
def test_whole_solve_on_tubes(name, kappa, skew, shift):
    g, v, A, off, rng = solve_case(name, kappa, skew, shift)
    n, nc = len(A), g["nc"]
    L = nlevels(g)
    r = rng.standard_normal((4, n))
    r[3] = A @ np.ones(n)                                           # a smooth right-hand side
    rc = rng.standard_normal((nc, 4)).astype(np.float32)
    rc[:, 3] = np.nan                                               # the pad lane
    rc_solve_order = np.zeros(n)
    for c in range(3):
        rc_solve_order[3 * g["pos"].astype(np.int64) + c] = rc[:, c]
    rhs = np.vstack([r, rc_solve_order, 2 * r[0] - 3 * r[1], r[0]])
    rc4 = np.tile(rc.ravel(), (len(rhs), 1))
    out = ks.bcr_run(g, [v], shift, rhs=rhs, rc4=rc4, arena=True)
    st = out["stats"]
    assert st["planned"] == 1 and out["ready"][0] == 1, (st, out["ready"])
    assert st["blocks"] == len(g["m"]) and st["max_block"] == g["m"].max() and st["levels"] == L
    assert np.array_equal(out["pos"], g["pos"])
    x = out["x"][0]
    # (a) the FP32 operators against their FP64 definitions
    _, ops = ks.bcr_reference(A, off, operators=True)
    tasks, a32 = out["tasks"], out["arena32"]
    assert len(tasks) == len(ops)
    kap = np.linalg.cond(A)
    for t, (lv, kind, blk, W64, segs) in zip(tasks, ops):
        assert (t[14], t[15], t[3]) == (lv, kind, off[blk]), (t, lv, kind, blk)
        Wg = ks.bcr_task_operator(t, a32)
        assert Wg.shape == W64.shape
        ks.check(Wg, W64, ulp32(W64) + 64 * (L + 1) * kap * EPS * np.abs(W64).max(), f"{name}: operator level {lv} kind {kind}")
        pad = np.asarray(a32[t[0]:t[0] + t[1] * t[2]]).reshape(t[1], t[2])[:, Wg.shape[1]:]
        assert (pad == 0).all()
    # (b) the GPU's solve is the FP64 application of its own FP32 operators
    maxld = int(tasks[:, 2].max())
    gam = (maxld + 8) * (2 * L + 1) * EPS
    mags = []
    for k in range(len(rhs)):
        ref = ks.bcr_task_apply(tasks, a32, rhs[k])
        mags.append(ks.bcr_task_apply(tasks, a32, rhs[k], absolute=True))
        ks.check(x[k], ref, gam * mags[k], f"{name}: solve {k} against its own operators")
    # (c) end to end against a dense solve of the same operator
    lu = sla.lu_factor(A)
    anorm = np.linalg.norm(A, 2)
    for k in range(4):
        xr = sla.lu_solve(lu, rhs[k])
        be = np.linalg.norm(A @ x[k] - rhs[k]) / (anorm * np.linalg.norm(x[k]))
        assert be <= 8 * (L + 1) * U32, (name, k, be)
        assert np.linalg.norm(x[k] - xr) <= kap * 8 * (L + 1) * U32 * np.linalg.norm(xr), (name, k)
    # the production interface: float(FP64 path on the FP32-rounded right-hand side), pad lane 0
    xc4 = out["xc4"][0].reshape(len(rhs), nc, 4)
    want = np.zeros((nc, 4), dtype=np.float32)
    for c in range(3):
        want[:, c] = x[4][3 * g["pos"].astype(np.int64) + c].astype(np.float32)
    for k in range(len(rhs)):
        assert np.array_equal(xc4[k], want), k
    # linear and bitwise repeatable
    ks.check(x[5], 2 * x[0] - 3 * x[1], 2 * gam * (mags[5] + 2 * mags[0] + 3 * mags[1]), f"{name}: linearity")
    assert np.array_equal(x[6], x[0])


def test_rings_of_666_nodes_are_solved_and_667_declined():
    rng = np.random.default_rng(7)
    g = ks.tube_graph([[666, 1, 666]], rng)
    v = ks.tube_values(g, 1e2, rng)
    A = ks.tube_dense(g, v, 2e-4)
    rhs = rng.standard_normal((1, len(A)))
    out = ks.bcr_run(g, [v], 2e-4, rhs=rhs)
    assert out["stats"]["planned"] == 1 and out["stats"]["max_block"] == 1998 and out["ready"][0] == 1
    x = out["x"][0, 0]
    be = np.linalg.norm(A @ x - rhs[0]) / (np.linalg.norm(A, 2) * np.linalg.norm(x))
    assert be <= 8 * (nlevels(g) + 1) * U32, be
    g = ks.tube_graph([[667, 1, 667]], rng)
    out = ks.bcr_run(g, [np.zeros((len(g["ccol"]), 9), dtype=np.float32)], 0.0, rhs=np.zeros((1, 3 * g["nc"])))
    assert out["stats"]["planned"] == 0 and out["stats"]["usable"] == 0 and out["stats"]["max_block"] == 2001
    assert out["ready"][0] == -1 and np.isnan(out["x"]).all()


def test_ready_falls_and_recovers_with_the_values():
    """a zero row, a NaN coupling and a diagonal block whose inverse overflows FP32 each leave the solve not ready; the next
    refresh with good values is ready again and solves bit for bit as before"""
    rng = np.random.default_rng(8)
    g = ks.tube_graph([[11, 1, 10, 22, 1, 10]], rng)
    v = ks.tube_values(g, 1e2, rng)
    row = np.repeat(np.arange(g["nc"]), np.diff(g["cptr"]))
    single = np.flatnonzero(g["ring"] == 4)[0]                     # a single-node ring (level 1): eliminated at the first level
    assert g["level"][single] % 2 == 1
    zero = v.copy()
    zero[row == single] = 0.0
    nanc = v.copy()
    e = np.flatnonzero((row == 5) & (g["ccol"] != 5))[0]
    nanc[e, 4] = np.nan
    tiny = v.copy()
    own = np.flatnonzero((row == single) & (g["ccol"] == single))[0]
    tiny[own] = (1e-39 * np.eye(3)).astype(np.float32).ravel()     # D^-1 = 1e39 I: finite in FP64, inf in FP32
    tiny[(row == single) & (g["ccol"] != single)] *= 1e-30
    sets = [v, zero, v, nanc, v, tiny, v]
    rhs = rng.standard_normal((1, 3 * g["nc"]))
    out = ks.bcr_run(g, sets, 2e-4, rhs=rhs)
    assert list(out["ready"]) == [1, 0, 1, 0, 1, 0, 1]
    x = out["x"][:, 0]
    for s in (2, 4, 6):
        assert np.array_equal(x[s], x[0]), s
    assert np.isnan(x[[1, 3, 5]]).all()


# ---- a live context -----------------------------------------------------------------------------------------------------------
def test_live_context_solve_is_the_shims(stenosis_case):
    """fsi_solid_coarse_solve on a context's own coarse level is bit for bit shim_bcr_run on the values read back from it, with
    the context's shift"""
    import contextlib
    import io
    from vasp_amd.capi import HipBackend, _ptr
    ns, desc, bc_values, pressure, hook = stenosis_case
    with contextlib.redirect_stdout(io.StringIO()):
        ns["t"] = 0.01
        hook("pre_solve")(**ns)
    g0, P = bc_values(), float(pressure.P)
    hb = HipBackend(stenosis_case[1])
    try:
        hb.set_dirichlet_values(g0); hb.set_interface_pressure(P)
        hb.assemble_residual()
        hb.assemble_jacobian()
        info = hb.solid_coarse_info()
        assert info["ready"] == 1, info
        nc, nb = info["nodes"], info["blocks3x3"]
        cptr, ccol, cvals = np.empty(nc + 1, dtype=np.int64), np.empty(nb, dtype=np.int32), np.empty(9 * nb, dtype=np.float32)
        assert hb.lib.fsi_solid_coarse_matrix(hb.ctx, _ptr(cptr), _ptr(ccol), _ptr(cvals)) == 0
        rng = np.random.default_rng(9)
        rhs = rng.standard_normal(3 * nc)
        x_live = hb.solid_coarse_solve(rhs)
        shift = hb.tuning()["bcr_shift"]
    finally:
        hb.close()
    g = dict(nc=nc, cptr=cptr, ccol=ccol)
    rc4 = np.zeros((nc, 4), dtype=np.float32)
    rc4[:, :3] = rhs.reshape(nc, 3).astype(np.float32)
    out = ks.bcr_run(g, [cvals], shift, rc4=rc4.ravel()[None, :])
    assert out["ready"][0] == 1
    x_shim = out["xc4"][0, 0].reshape(nc, 4)[:, :3].astype(np.float64).ravel()
    assert np.array_equal(x_live, x_shim)
