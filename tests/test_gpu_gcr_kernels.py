"""The Gram-Schmidt kernels of the recycled GCR (vasp_amd/csrc/fsi_gcr.hip) and the deterministic reductions of fsi_solver.hip,
one launch at a time through the test shim, against numpy on the exact inputs the kernel sees.

An FP32 store is drawn in float32 and upcast: the kernel converts to double exactly, so the reference has no storage error and
the bound of an FP64-accumulated sum is the accumulation alone, 64 eps64 sum |terms| (the kernels' summation depth is far below
64 at these sizes).  Large entries are planted in the rows a kernel treats apart - the n mod 4 tail, the first and last rows of
the float4 stream and of a grid-stride pass, the first column of an 8-column group - so that a dropped, doubled or misplaced
element misses the bound by orders of magnitude."""
import numpy as np
import pytest

import kernel_shim as ks

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NT_N, NT_M = 3_000_001, 48           # FP32 store above the 512 MiB stream_once threshold: the non-temporal instantiations
SENTINEL = 1234.5678


def ldq_of(n, pad=0):
    return (n + 3) // 4 * 4 + pad


def planted_rows(n):
    """rows the kernels handle apart: the n mod 4 tail, the first / last row of the float4 stream, and the rows at the edges of a
    grid-stride pass for the grid sizes the launchers choose (256 threads x 4 rows per block)"""
    rows = {0, n - 1, n // 2}
    n4 = n >> 2
    rows.update(range(4 * n4, n))
    if n4:
        rows.update({4 * n4 - 1, 4 * n4 - 4})
    for blocks in (1, 128, 245, 293, 1024, 2048):
        for k in (1, 2):
            e = 4 * 256 * blocks * k
            rows.update({e - 1, e, e + 3})
    return np.array(sorted(r for r in rows if 0 <= r < n), dtype=np.int64)


def draw_store(rng, n, m, fp32, ldq):
    dt = np.float32 if fp32 else np.float64
    Q = np.full((m, ldq), np.nan, dtype=dt)          # padding rows hold NaN: a read of them shows in every sum
    Q[:, :n] = rng.standard_normal((m, n)).astype(dt)
    rows = planted_rows(n)
    for k0 in range(0, m, 8):
        Q[k0, rows] = dt(3.0e3)                      # first column of every 8-column group
    return Q


def draw_vec(rng, n, planted=1.0e3):
    v = rng.standard_normal(n)
    v[planted_rows(n)] *= planted
    return v


def fsum_rows(Q, v):
    """(sum q_i v_i, sum |q_i v_i|) per column in extended precision"""
    vl = v.astype(np.longdouble)
    out, mag = np.zeros(len(Q)), np.zeros(len(Q))
    for k in range(len(Q)):
        p = Q[k].astype(np.longdouble) * vl
        out[k], mag[k] = p.sum(), np.abs(p).sum()
    return out, mag


def check(got, ref, bound, what):
    got, ref, bound = np.atleast_1d(got), np.atleast_1d(ref), np.atleast_1d(bound)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {bad.sum()} of {len(got)} outside the bound; first at {i}: got {got[i]!r}, "
                             f"reference {ref[i]!r}, error {err[i]:.3e} > bound {bound[i]:.3e}")


def run_dots(fp32, n, m, with_r, pad=0, seed=0):
    rng = np.random.default_rng(seed + 7 * n + m)
    ldq = ldq_of(n, pad)
    Q = draw_store(rng, n, m, fp32, ldq)
    w = draw_vec(rng, n)
    r = draw_vec(rng, n) if with_r else None
    out = np.full(m + 3, SENTINEL)
    ks.call("shim_gcr_dots", int(fp32), Q, ldq, n, m, w, r, out, len(out))
    ref, mag = fsum_rows(Q[:, :n], w)
    check(out[:m], ref, 64 * EPS * mag, f"Q_k . w (fp32={fp32}, n={n}, m={m})")
    ww, wwm = fsum_rows(w[None, :], w)
    check(out[m], ww, 64 * EPS * wwm, "w . w")
    if with_r:
        wr, wrm = fsum_rows(w[None, :], r)
        check(out[m + 1], wr, 64 * EPS * wrm, "w . r")
    else:
        assert out[m + 1] == 0.0, "r = nullptr must give out[m + 1] = 0"
    assert out[m + 2] == SENTINEL, "the kernel wrote past out[m + 1]"


DOT_N = [1, 3, 4, 5, 4095, 4097, 1_000_003]
DOT_M = [0, 1, 7, 8, 9, 16, 17, 180]


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", DOT_N)
@pytest.mark.parametrize("m", DOT_M)
def test_gcr_dots_match_extended_precision_sums(fp32, n, m):
    if n > 5000 and m > 17:
        m = 24                                  # keeps the host reference small; 24 still spans three column groups
    run_dots(fp32, n, m, with_r=(m % 2 == 0))


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "fp64"])
def test_gcr_dots_ignore_padding_rows_and_take_r(fp32):
    run_dots(fp32, 4097, 9, with_r=True, pad=12)
    run_dots(fp32, 5, 17, with_r=False, pad=4)


def test_gcr_dots_non_temporal_store():
    assert NT_M * ldq_of(NT_N) * 4 > 512 * 2**20
    run_dots(True, NT_N, NT_M, with_r=True)


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "fp64"])
def test_gcr_dots_at_the_row_part_cap(fp32):
    """m <= 8 leaves two y-groups, so dots_t allows 1024 row parts; n = 4096 * 1024 + 5 asks for 1025: the cap holds and the
    grid-stride loop of every part takes four passes"""
    run_dots(fp32, 4096 * 1024 + 5, 8, with_r=True)


def run_axpy(fp32, n, m, with_r, pad=0, seed=1):
    rng = np.random.default_rng(seed + 11 * n + m)
    ldq = ldq_of(n, pad)
    Q = draw_store(rng, n, m, fp32, ldq)
    h = rng.standard_normal(m)
    w = draw_vec(rng, n)
    r = draw_vec(rng, n) if with_r else None
    w0 = w.copy()
    out = np.full(3, SENTINEL)
    ks.call("shim_gcr_axpy", int(fp32), Q, ldq, n, m, h, w, r, out, len(out))
    ref, mag = w0.astype(np.longdouble), np.abs(w0)
    for k in range(m):                                # column by column: the host memory stays flat at the large stores
        qk = Q[k, :n].astype(np.float64)
        ref = ref - np.longdouble(h[k]) * qk.astype(np.longdouble)
        mag = mag + abs(h[k]) * np.abs(qk)
    check(w, np.asarray(ref, dtype=np.float64), (m + 8) * EPS * mag, f"w - Q h (fp32={fp32}, n={n}, m={m})")
    ww, wwm = fsum_rows(w[None, :], w)               # the norms are of the w' the kernel wrote
    check(out[0], ww, 64 * EPS * wwm, "|w'|^2")
    if with_r:
        wr, wrm = fsum_rows(w[None, :], r)
        check(out[1], wr, 64 * EPS * wrm, "w' . r")
    else:
        assert out[1] == 0.0
    assert out[2] == SENTINEL


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4095, 4097, 1_000_003])
@pytest.mark.parametrize("m", [0, 4, 5, 6, 7])
def test_gcr_axpy_matches_the_projection(fp32, n, m):
    run_axpy(fp32, n, m, with_r=(n % 2 == 1), pad=4 if n == 4097 else 0)


def test_gcr_axpy_grid_stride_and_non_temporal_store():
    run_axpy(True, NT_N, NT_M, with_r=True)          # 2930 row blocks > the 2048-block cap: the grid-stride loop runs
    run_axpy(False, 2_500_003, 5, with_r=False)


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n,slot", [(1, 0), (5, 3), (4097, 2), (1_000_003, 4)])
def test_gcr_update_writes_one_column(fp32, n, slot):
    rng = np.random.default_rng(n + slot)
    ncols, ldq, ldz = 5, ldq_of(n, 4), (n + 1) // 2 * 2 + 2
    dt = np.float32 if fp32 else np.float64
    Q = rng.standard_normal((ncols, ldq)).astype(dt)
    Z = rng.standard_normal((ncols, ldz))
    Q0, Z0 = Q.copy(), Z.copy()
    w, z, r = draw_vec(rng, n), rng.standard_normal(n), draw_vec(rng, n)
    r0 = r.copy()
    qd = np.full(n, np.nan)
    inv_wn, alpha = 1.0 / 3.7, -0.83
    out = np.full(2, SENTINEL)
    ks.call("shim_gcr_update", int(fp32), Q, ldq, Z, ldz, ncols, slot, n, w, z, inv_wn, alpha, r, qd, out, len(out))
    q = w * inv_wn                                    # one FP64 multiply, round to nearest even, as in the kernel
    np.testing.assert_array_equal(qd, q)
    # the store holds (QT)q: the conversion of the FP64 product, round to nearest even (v_cvt_f32_f64)
    np.testing.assert_array_equal(Q[slot, :n], q.astype(dt))
    np.testing.assert_array_equal(Z[slot, :n], z)
    others = [k for k in range(ncols) if k != slot]
    np.testing.assert_array_equal(Q[others], Q0[others])
    np.testing.assert_array_equal(Z[others], Z0[others])
    np.testing.assert_array_equal(Q[slot, n:], Q0[slot, n:])
    np.testing.assert_array_equal(Z[slot, n:], Z0[slot, n:])
    ref = r0 - alpha * q                              # the kernel may fuse the multiply-add: one rounding either way
    check(r, ref, 2 * EPS * (np.abs(r0) + np.abs(alpha * q)), "r - alpha q")
    rr, rrm = fsum_rows(r[None, :], r)
    check(out[0], rr, 64 * EPS * rrm, "|r'|^2")
    assert out[1] == SENTINEL


FLUSH_KNEW = [0, 1, 3, 4, 5, 8, 9, 16, 17, 31, 32]


@pytest.mark.parametrize("knew", FLUSH_KNEW)
@pytest.mark.parametrize("n", [1, 4097, 200_001])
def test_gcr_flush_accumulates_x_and_overwrites_the_new_directions(knew, n):
    rng = np.random.default_rng(100 * knew + n)
    width = ks.load().shim_gcr_flush_width(knew)
    assert width == (0 if knew == 0 else 4 if knew <= 4 else 8 if knew <= 8 else 16 if knew <= 16 else 32)
    m = 40
    ncols, ldz = m + 3, (n + 1) // 2 * 2
    Z = np.full((ncols, ldz), np.nan)                 # the padding row of an odd n and the columns past m are never read
    Z[:m, :n] = rng.standard_normal((m, n))
    Z[::8, planted_rows(n)] *= 1.0e3
    Z[m:, :n] = 5.0
    Z0 = Z.copy()
    y = rng.standard_normal(m)
    cn = np.full((max(width, 1), m), np.nan)          # rows knew .. width - 1 are computed and must not be written
    cn[:knew] = rng.standard_normal((knew, m))
    cn = np.ascontiguousarray(cn[:width]) if width else np.zeros(0)
    slots = rng.permutation(m)[:knew].astype(np.int32)      # non-contiguous, out of order, among the read columns
    x = rng.standard_normal(n)
    x0 = x.copy()
    ks.call("shim_gcr_flush", Z, ldz, ncols, n, m, y, cn if width else None, slots if knew else None, knew, x)
    raw = Z0[:m, :n]
    check(x, x0 + y @ raw, 64 * EPS * (np.abs(x0) + np.abs(y) @ np.abs(raw)), "x += Z y")
    for k in range(knew):
        check(Z[slots[k], :n], cn[k] @ raw, 64 * EPS * (np.abs(cn[k]) @ np.abs(raw)), f"Z_slot[{k}] = Z cn[{k}] of the raw store")
    keep = [j for j in range(ncols) if j not in set(slots.tolist())]
    np.testing.assert_array_equal(Z[keep], Z0[keep])
    np.testing.assert_array_equal(Z[:, n:], Z0[:, n:])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4095, 4097, 1_000_003])
def test_dot_and_hashed_sum(n):
    rng = np.random.default_rng(n)
    x, y = draw_vec(rng, n), draw_vec(rng, n)
    out = np.full(2, SENTINEL)
    ks.call("shim_dot", x, y, n, out)
    ref, mag = fsum_rows(x[None, :], y)
    check(out[0], ref, 64 * EPS * mag, f"x . y (n={n})")
    assert out[1] == SENTINEL
    for first, stride in ((0, 1), (1, 3)):
        cnt = (n - first + stride - 1) // stride if n > first else 0
        i = np.arange(cnt, dtype=np.uint64)
        h = (i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)          # wraps mod 2^64 as the kernel's uint64 product
        wgt = 1.0 + h.astype(np.float64) * (1.0 / 16777216.0)
        v = x[first::stride][:cnt]
        a, b = np.full(2, SENTINEL), np.full(2, SENTINEL)
        ks.call("shim_hashed_sum", x, n, first, stride, cnt, a)
        ks.call("shim_hashed_sum", x, n, first, stride, cnt, b)
        ref, mag = fsum_rows((v * wgt)[None, :], np.ones(cnt)) if cnt else (np.zeros(1), np.zeros(1))
        check(a[0], ref, 64 * EPS * mag, f"hashed sum (n={n}, first={first}, stride={stride})")
        assert a[0].tobytes() == b[0].tobytes(), "launch_hashed_sum is not bitwise reproducible"
        assert a[1] == SENTINEL
