"""Host-only: the sample queue's per-pixel sums (csrc/pt_queue.hpp queue_sums), in float32 numpy.

The contract is the xor butterfly's lane 0 (pt_render's order).  queue_sums_tree forms lane 0's tree alone — no lane but
the first of a pixel's group is stored — with several pixels packed into one register as the tree narrows.  Both, and the
plain half-lane tree between them, must give the same bits for every g = 1 … 64 (the powers of two a launch can have),
every count of a launch from 1 to 512 (below, at and above g: idle lanes, one slot per lane, sequential per-lane sums
first) and every number of pixels a wave may own, on values of mixed magnitude with ±0, denormals and infinities."""
import numpy as np
import pytest

import queue_sums_ref as qs


@pytest.mark.parametrize("group_log2", range(7))
def test_lane0_of_the_butterfly_is_the_half_lane_tree(group_log2):
    g = 1 << group_log2
    for count in qs.COUNTS:
        for seed in range(4):
            v = qs.adversarial(1, count, 1000 * group_log2 + 10 * count + seed)[0]
            a, b = qs.butterfly_lane0(v, g), qs.half_tree_lane0(v, g)
            assert qs.same_bits(b, a), (g, count, seed)
            # (both on one machine: even a NaN's bits agree)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (g, count, seed)


@pytest.mark.parametrize("group_log2", range(7))
def test_packed_wave_tree_has_the_butterflys_bits(group_log2):
    for count in qs.COUNTS:
        for npix in qs.pixel_counts(count):
            v = qs.adversarial(npix, count, 77 * group_log2 + 3 * count + npix)
            assert qs.same_bits(qs.wave_tree(v, group_log2), qs.contract(v, group_log2)), (group_log2, count, npix)


def test_inputs_are_adversarial():
    v = qs.adversarial(8, 64, 5)
    w = v.view(np.uint32)
    assert (w == 0x80000000).any() and (w == 0).any() and np.isinf(v).any()
    assert ((w & 0x7F800000) == 0).sum() > (w << 1 == 0).sum()          # denormals besides the zeros
    fin = np.abs(v[np.isfinite(v) & (v != 0)]).astype(np.float64)
    assert fin.max() / fin.min() > 1e30
    sums = qs.contract(v, 6)
    assert np.isnan(sums).any() and np.isfinite(sums).any()


def test_minus_zero_becomes_plus_zero():
    v = np.full((1, 3, 3), -0.0, np.float32)
    for gl in range(7):
        assert not np.signbit(qs.wave_tree(v, gl)).any() and not np.signbit(qs.contract(v, gl)).any()
