"""CPU: the numpy restatement of the FP32 records (tests/fp32_records.py) - word layout, exact round trip of every float bit
pattern that occurs (signed zeros, subnormals, infinities, NaN payloads) and of the full index ranges."""
import numpy as np

import fp32_records as fr


def special_floats(rng, n):
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.finfo(np.float32).max, np.finfo(np.float32).tiny,
                        1e-45, -1e-45, 0.1, 1 / 3], dtype=np.float32)
    v = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    v[:len(special)] = special
    v[len(special)] = np.array([0x7FC01234], dtype=np.uint32).view(np.float32)[0]      # a NaN with a payload
    return v


def test_f3_layout_and_round_trip():
    rng = np.random.default_rng(2)
    n = 777
    v = special_floats(rng, 3 * n)
    loc = rng.integers(0, 65536, n).astype(np.uint16)
    rec = fr.pack_f3(v, loc)
    assert rec.shape == (4 * n,)
    r4 = rec.reshape(-1, 4)
    for c in range(3):
        np.testing.assert_array_equal(r4[:, c], v[c::3].view(np.uint32))
    np.testing.assert_array_equal(r4[:, 3], loc.astype(np.uint32))
    v3, l3 = fr.unpack_f3(rec)
    np.testing.assert_array_equal(v3.reshape(-1).view(np.uint32), v.view(np.uint32))
    np.testing.assert_array_equal(l3, loc)


def test_sb_f32_layout_and_round_trip():
    rng = np.random.default_rng(3)
    nb = 513
    v = special_floats(rng, 9 * nb)
    col = rng.integers(0, 2**31 - 1, nb).astype(np.int32)
    col[:2] = (0, 2**31 - 1)
    rec = fr.pack_sb_f32(v, col)
    assert rec.shape == (10 * nb,)
    r10 = rec.reshape(-1, 10)
    # the 40-byte record is read as five 8-byte words: (a0 a1) (a2 a3) (a4 a5) (a6 a7) (a8 column)
    w = rec.view(np.uint64).reshape(-1, 5)
    np.testing.assert_array_equal(w[:, 4] >> np.uint64(32), col.astype(np.uint64))
    np.testing.assert_array_equal(r10[:, :9], v.view(np.uint32).reshape(-1, 9))
    vs, cs = fr.unpack_sb_f32(rec)
    np.testing.assert_array_equal(vs.reshape(-1).view(np.uint32), v.view(np.uint32))
    np.testing.assert_array_equal(cs, col)


def test_signatures_cover_the_new_entry_points():
    assert set(fr.SIGS) == {"shim_pack_f3", "shim_pack_sb_f32", "shim_sweep_tiled_r3", "shim_sweep_tiled_a1", "shim_sweep_sb_r",
                            "shim_sweep_schur_tiled_f64"}
    assert all(set(s) <= set("pilfd") for s in fr.SIGS.values())
