"""The slot a Krylov iteration has just taken beyond the store's high-water mark is neither cleared nor read
(vasp_amd/csrc/fsi_gcr.hip, fsi_gcr_host.hpp, fsi_krylov.hip): k_gcr_dots and k_gcr_axpy are told how many leading columns hold
data and take the others as zeros.

GPU: launch_gcr_dots_lead / launch_gcr_axpy_lead with the last of m columns marked empty, against the unchanged
launch_gcr_dots / launch_gcr_axpy on the same store with that column zeroed - every output equal (``np.array_equal``).  The empty
column's memory holds NaN, so a stray read shows in the result.  n in {4096 .. 4099} (the n mod 4 tails), m in {1, 2, 4, 5, 8, 9,
17} (the four-column groups of the update and the eight-column groups of the products, with the empty column first, inside and
last in its group), with and without r, FP64 and FP32 columns.

Without a GPU: the store's bookkeeping of that slot (GcrStore::lead, abandon) through the shim's host-only store - a slot taken
and abandoned is zeroed before any later pass scans it."""
import ctypes as C

import numpy as np
import pytest

import kernel_shim as ks

_NEW = {"shim_gcr_dots_lead": "iplliipppl", "shim_gcr_axpy_lead": "iplliippppl"}
NS = (4096, 4097, 4098, 4099)
MS = (1, 2, 4, 5, 8, 9, 17)


def shim(name, *args):
    fn = getattr(ks.load(), name)
    if fn.argtypes is None:
        fn.argtypes = [ks._CT[c] for c in _NEW[name]]
        fn.restype = C.c_int
    if fn(*[ks._arg(a) for a in args]) != 0:
        raise RuntimeError(f"{name}: {ks.load().shim_last_error().decode()}")


def store(n, m, fp32, seed):
    """(Q with the last column zero, Q with it NaN, w, r, ldq): columns of unit size, entries behind n in a column's padding NaN
    in both (nobody may read them)"""
    rng = np.random.default_rng(seed)
    ldq = (n + 3) & ~3
    Q = np.full((m, ldq), np.nan, dtype=np.float32 if fp32 else np.float64)
    Q[:, :n] = rng.standard_normal((m, n)) / np.sqrt(n)
    Qz, Qn = Q.copy(), Q.copy()
    Qz[m - 1, :n] = 0.0
    Qn[m - 1, :] = np.nan
    return Qz, Qn, rng.standard_normal(n), rng.standard_normal(n), ldq


@pytest.mark.gpu
@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_empty_last_column_is_zeros_unread(n, m, fp32):
    Qz, Qn, w, r, ldq = store(n, m, fp32, 1000 * m + n + fp32)
    for rr in (r, None):
        what = f"n {n} m {m} {'fp32' if fp32 else 'fp64'} {'with' if rr is not None else 'without'} r"
        # the products
        ref, out = np.full(m + 3, -3.5), np.full(m + 3, -3.5)
        ks.call("shim_gcr_dots", fp32, Qz, ldq, n, m, w, rr, ref, len(ref))
        shim("shim_gcr_dots_lead", fp32, Qn, ldq, n, m, m - 1, w, rr, out, len(out))
        assert np.array_equal(out, ref), f"k_gcr_dots, {what}: {out} against {ref}"
        assert out[m - 1] == 0.0 and out[m + 2] == -3.5
        # the update, with the coefficients the host hands back: the products above
        h = ref[:m].copy()
        wz, wn_ = w.copy(), w.copy()
        ref2, out2 = np.full(3, -3.5), np.full(3, -3.5)
        ks.call("shim_gcr_axpy", fp32, Qz, ldq, n, m, h, wz, rr, ref2, len(ref2))
        shim("shim_gcr_axpy_lead", fp32, Qn, ldq, n, m, m - 1, h, wn_, rr, out2, len(out2))
        assert np.array_equal(wn_, wz), f"k_gcr_axpy, {what}: {int((wn_ != wz).sum())} entries of w differ"
        assert np.array_equal(out2, ref2), f"k_gcr_axpy, {what}: {out2} against {ref2}"
    # all columns marked as data: the old entry points' own results
    out = np.full(m + 3, -3.5)
    shim("shim_gcr_dots_lead", fp32, Qz, ldq, n, m, m, w, r, out, len(out))
    assert np.array_equal(out, _dots(fp32, Qz, ldq, n, m, w, r))


def _dots(fp32, Q, ldq, n, m, w, r):
    out = np.full(m + 3, -3.5)
    ks.call("shim_gcr_dots", fp32, Q, ldq, n, m, w, r, out, len(out))
    return out


# ---- without a GPU: the store's bookkeeping of the fresh slot --------------------------------------------------------------------
OPS = dict(ks.GCR_STORE_OPS, lead=10, abandon=11)


def store_op(cap, op, arg=0):
    res = np.full(cap + 2, -7, dtype=np.int32)
    born, free, hot = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int32), np.zeros(32, dtype=np.int32)
    scal = np.zeros(4, dtype=np.int64)
    ks.call("shim_gcr_store_op", OPS[op], arg, res, born, free, hot, scal)
    return [int(v) for v in res[:2]], int(scal[0])


class Columns:
    """the q columns as the device holds them: never written (NaN), written, or zeroed - driven by what fsi_krylov.hip does with
    the store's answers"""

    def __init__(self, cap):
        self.cap, self.col = cap, ["garbage"] * cap

    def scan(self):
        """a Gram-Schmidt pass: the kernels read the leading lead() of the hw columns"""
        (lead, _), hw = store_op(self.cap, "lead")
        assert hw - 1 <= lead <= hw
        read = self.col[:lead]
        assert "garbage" not in read, f"a pass over {lead} of {hw} columns reads a column nobody wrote: {self.col[:hw]}"
        return lead, hw

    def take(self):
        (slot, clear), hw = store_op(self.cap, "take")
        return slot, clear

    def store(self, slot):                     # gcr_store: the update kernel writes the column, then set_born
        self.col[slot] = "q"
        store_op(self.cap, "set_born", slot)

    def abandon(self, slot):                   # the breakdown return of gcr_cycle
        (col, _), _ = store_op(self.cap, "abandon", slot)
        if col >= 0:
            self.col[col] = "zero"
        return col


def test_a_slot_taken_and_abandoned_is_cleared_before_it_is_scanned_again():
    cap = 8
    store_op(cap, "init", cap)
    c = Columns(cap)
    assert c.scan() == (0, 0)
    # two ordinary iterations: the fresh slot is the last column and is not read until it has been written
    for k in range(2):
        slot, clear = c.take()
        assert (slot, clear) == (k, 1)
        assert c.scan() == (k, k + 1)
        c.store(slot)
        assert c.scan() == (k + 1, k + 1)
    # an iteration that breaks down after its pass: the column is named for zeroing, once, and later passes read it as data
    slot, clear = c.take()
    assert (slot, clear) == (2, 1) and c.scan() == (2, 3)
    assert c.abandon(slot) == 2 and c.abandon(slot) == -1
    assert c.scan() == (3, 3) and c.col[2] == "zero"
    # the next iteration takes the next fresh slot: the abandoned one is inside the scanned range now
    slot, clear = c.take()
    assert (slot, clear) == (3, 1) and c.scan() == (3, 4)
    c.store(slot)
    # fill the store, retire, and take a retired slot: its column is zero already, nothing is fresh, abandoning names nothing
    while True:
        (full, _), _ = store_op(cap, "full")
        if full:
            break
        slot, clear = c.take()
        assert clear == 1
        c.scan()
        c.store(slot)
    (nret, first), _ = store_op(cap, "retire", 2)
    assert nret >= 1
    slot, clear = c.take()
    assert clear == 0 and c.scan() == (cap, cap)
    c.col[slot] = "zero"                       # (gcr_make_room zeroes what it retires)
    assert c.abandon(slot) == -1
    # a reset forgets a fresh slot
    store_op(cap, "reset")
    c = Columns(cap)
    slot, clear = c.take()
    assert c.scan() == (0, 1)
    store_op(cap, "reset")
    assert c.scan() == (0, 0)
