"""CPU self-tests of the host-side references the kernel tests build on (tests/kernel_shim.py), so that a failure of
tests/test_gpu_gcr_kernels.py or tests/test_gpu_sweep_kernels.py is one of a kernel, not of its reference."""
import numpy as np
import pytest

import kernel_shim as ks
from vasp_amd import capi


@pytest.mark.parametrize("n,rows_per_tile", [(1, 256), (37, 256), (1000, 128), (1100, 256), (1100, 128), (300, 32), (300, 64)])
def test_tile_builder_covers_every_entry_once(n, rows_per_tile):
    rowptr, cols = ks.local_graph(n, np.random.default_rng(n), reach=48, max_deg=90, diag_only=[0, n - 1])
    uptr, ulist, ploc, max_nu = ks.build_tiles(rowptr, cols, rows_per_tile, ks.TILE_LIMIT)
    nt = (n + rows_per_tile - 1) // rows_per_tile
    assert len(uptr) == nt + 1 and uptr[0] == 0 and uptr[-1] == len(ulist)
    assert max_nu == np.diff(uptr).max()
    row = np.repeat(np.arange(n), np.diff(rowptr))
    tile = row // rows_per_tile
    np.testing.assert_array_equal(ulist[uptr[tile] + ploc], cols)          # every local index names its own column
    for t in range(nt):
        u = ulist[uptr[t]:uptr[t + 1]]
        assert np.all(np.diff(u) > 0)                                    # sorted, distinct
        e0, e1 = rowptr[t * rows_per_tile], rowptr[min(n, (t + 1) * rows_per_tile)]
        np.testing.assert_array_equal(u, np.unique(cols[e0:e1]))         # exactly the tile's columns
    # the launch the tiled kernels get: xcd_span(nt) logical workgroups, each tile taken by exactly one (as fsi_xcd_order says)
    lib = capi.load_library()
    span = lib.fsi_xcd_order(nt, None)
    out = np.full(max(span, 1), -7, dtype=np.int64)
    assert lib.fsi_xcd_order(nt, capi._ptr(out)) == span
    mine = [ks.xcd_unit(L, nt) for L in range(span)]
    np.testing.assert_array_equal(out[:span], mine)
    taken = sorted(t for t in mine if t >= 0)
    assert taken == list(range(nt))


def test_tile_builder_refuses_a_tile_over_the_limit():
    rowptr = np.array([0, 5], dtype=np.int64)
    cols = np.arange(5, dtype=np.int32)
    assert ks.build_tiles(rowptr, cols, 256, 5) is not None
    assert ks.build_tiles(rowptr, cols, 256, 4) is None


def test_fp16_record_emulation_round_trips():
    """the bit layout the shim documents: h1 = half | loc << 16, h3 = (h0 | h1 << 16, h2 | loc << 16), sb = 5 words of halves +
    the column; every finite half bit pattern survives pack / unpack, and the float32 -> half rounding is to nearest even"""
    bits = np.arange(65536, dtype=np.uint32)
    finite = np.isfinite(bits.astype(np.uint16).view(np.float16))
    halves = bits[finite].astype(np.uint16).view(np.float16).astype(np.float32)
    n = len(halves)
    loc = (np.arange(n) * 7919 % 65536).astype(np.uint16)
    rec = ks.pack_h1(halves, loc)
    v, l2 = ks.unpack_h1(rec)
    np.testing.assert_array_equal(rec & 0xFFFF, bits[finite])
    np.testing.assert_array_equal(v.astype(np.float32).view(np.uint32), halves.view(np.uint32))
    np.testing.assert_array_equal(l2, loc)
    m = n // 3
    v3, l3 = ks.unpack_h3(ks.pack_h3(halves[:3 * m], loc[:m]))
    np.testing.assert_array_equal(v3.ravel().astype(np.float32).view(np.uint32), halves[:3 * m].view(np.uint32))
    np.testing.assert_array_equal(l3, loc[:m])
    k = n // 9
    col = (np.arange(k) * 104729).astype(np.int32)
    vs, cs = ks.unpack_sb(ks.pack_sb(halves[:9 * k], col))
    np.testing.assert_array_equal(vs.ravel().astype(np.float32).view(np.uint32), halves[:9 * k].view(np.uint32))
    np.testing.assert_array_equal(cs, col)
    # round to nearest, ties to even: 1 + 2^-11 is halfway between 1 and 1 + 2^-10 and goes to 1; 1 + 3 * 2^-11 goes up
    t = np.array([1 + 2**-11, 1 + 3 * 2**-11, 65519.0, 65520.0, 2**-25, 3 * 2**-26], dtype=np.float32)
    np.testing.assert_array_equal(ks.half_value(ks.half_bits(t)), [1.0, 1 + 2**-9, 65504.0, np.inf, 0.0, 2**-24])


def test_tile_limit_is_the_librarys():
    """the synthetic limit cases build a tile of exactly TILE_LIMIT distinct neighbours: it must be the library's tile_limit()"""
    assert ks.load().shim_tile_limit() == ks.TILE_LIMIT
