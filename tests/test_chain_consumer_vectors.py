"""CPU checks of tests/chain_consumers.py: the vectors the x + d consumer tests use hold what those tests are about."""
import numpy as np
import pytest

import chain_consumers as cc


def test_special_pairs_cancel_and_round():
    x, d = cc.SPECIAL[:, 0], cc.SPECIAL[:, 1]
    s = cc.host_sum(x, d)
    exact = x.astype(np.float64) + d.astype(np.float64)
    zero = s == 0
    assert (zero & ~np.signbit(s)).sum() >= 3 and (zero & np.signbit(s)).sum() >= 1, "sums that are +0 and a sum that is -0"
    assert (zero & (x != 0)).sum() >= 2, "pairs that cancel"
    rounded = s.astype(np.float64) != exact
    assert rounded.sum() >= 5, "sums that round"
    assert (rounded & (s == x)).any() and (rounded & (s != x)).any(), "rounded back to x, and rounded away from it"
    tiny = np.finfo(np.float32).tiny
    assert ((s != 0) & (np.abs(s) < tiny)).any(), "a subnormal sum"


@pytest.mark.parametrize("nn", [1, 5, 257])
def test_vectors_are_mixed_and_reproducible(nn):
    x4, d4 = cc.vec4_pairs(np.random.default_rng(nn), nn, pad=2.5)
    y4, e4 = cc.vec4_pairs(np.random.default_rng(nn), nn, pad=2.5)
    cc.same_bits(x4, y4, "x")
    cc.same_bits(d4, e4, "d")
    assert x4.shape == (nn, 4) and (x4[:, 3] == 2.5).all() and (d4[:, 3] == 2.5).all()
    x, d = x4[:, :3].ravel(), d4[:, :3].ravel()
    k = min(3 * nn, len(cc.SPECIAL))
    hit = [i for i in range(3 * nn - k + 1) if np.array_equal(cc.bits(x[i:i + k]), cc.bits(cc.SPECIAL[:k, 0]))
           and np.array_equal(cc.bits(d[i:i + k]), cc.bits(cc.SPECIAL[:k, 1]))]
    assert hit, "the special pairs are in the vector"
    if nn >= 5:
        assert (x > 0).any() and (x < 0).any() and (d > 0).any() and (d < 0).any()
        s = cc.host_sum(x, d)
        assert (s.astype(np.float64) != x.astype(np.float64) + d.astype(np.float64)).any()
    if nn == 257:
        nz = np.abs(x[x != 0]).astype(np.float64)
        assert nz.max() / nz.min() > 1e6


def test_same_bits_tells_the_zeros_apart():
    cc.same_bits(np.float32([0.0, -0.0]), np.float32([0.0, -0.0]), "zeros")
    with pytest.raises(AssertionError):
        cc.same_bits(np.float32([0.0]), np.float32([-0.0]), "zeros")
    with pytest.raises(AssertionError):
        cc.same_bits(np.float64([0.0]), np.float64([-0.0]), "zeros")
