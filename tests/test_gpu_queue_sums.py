"""GPU (-m gpu): the sample queue's per-pixel sums without LDS permutes (csrc/pt_queue.hpp queue_sums_tree).

1. rt_debug_queue_sums — one wave, its slots filled from an array — against the numpy butterfly (tests/queue_sums_ref.py),
   as uint32: every group size, the counts of the host test, one pixel / the most a wave may own / one number in between,
   on the host test's adversarial values.  (Where the butterfly's sum is a NaN — a pixel with +inf and -inf — the device's
   must be one; its bits are not pinned.)
2. Frames of the fused path against the direct path pt_render, bits with ==, with the options as test_gpu_lane_merge sets
   them: ragged and tiny frames (partly filled waves), both policies, counts below / at / above a pixel's lane group and a
   wave's queue, wave fill off and on, sample moments off and on (the moments plane of both paths against the float64
   two-pass truth, within tests/moments_ref.py's tolerance), a sharded context, counting builds (which keep the butterfly),
   on C2, C3, the all-kinds scene and the small C5 that runs pt_samples_w."""
import numpy as np
import pytest

import cases
import queue_sums_ref as qs
from test_gpu_moments import sample_luminances, truth_and_tolerance

pytestmark = pytest.mark.gpu
rt = cases.rt
R = rt.raytracer

COUNTS = (1, 3, 16, 24, 33, 64, 65, 200)


# ---- 1. the unit probe ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["ieee", "rocm-opencl"])
@pytest.mark.parametrize("count", qs.COUNTS)
def test_probe_has_the_butterflys_bits(count, arith):
    t = rt.RayTracer(8, 8, scene=rt.workloads.get("c1", width=8, height=8).scene, seed=cases.SEED)
    t.setArith(arith)
    try:
        for group_log2 in range(7):
            for npix in qs.pixel_counts(count):
                v = qs.adversarial(npix, count, 77 * group_log2 + 3 * count + npix)
                got = t.debugQueueSums(v, group_log2)
                ref = qs.contract(v, group_log2)
                key = (count, group_log2, npix)
                assert np.array_equal(got[:, 3], np.full(npix, count, np.float32)), key
                assert qs.same_bits(got[:, :3], ref), (key, got[:, :3].view(np.uint32), ref.view(np.uint32))
    finally:
        t.close()


def test_probe_rejects_what_a_wave_cannot_own():
    t = rt.RayTracer(8, 8, scene=rt.workloads.get("c1", width=8, height=8).scene, seed=cases.SEED)
    try:
        for npix, count, gl in ((17, 1, 0), (2, 257, 6), (1, 513, 6), (1, 8, 7)):
            with pytest.raises(R.RtError):
                t.debugQueueSums(np.zeros((npix, count, 3), np.float32), gl)
    finally:
        t.close()


# ---- 2. frames --------------------------------------------------------------------------------------------------------
_WORKLOADS = {}
_LUM = {}


def _workload(case, size):
    if (case, size) not in _WORKLOADS:
        w, h = (7, 5) if size == "tiny" else (96, 64) if case == "c5" else (61, 37)
        kw = {"c2": {}, "all_kinds": {}, "c3": dict(tex_size=64), "c5": dict(segments=24, rings=16)}[case]   # (C5: test_gpu_lookahead's)
        wl = rt.workloads.get(case, width=w, height=h, **kw)
        _WORKLOADS[case, size] = (wl.scene, wl.camera, wl.width, wl.height)
    return _WORKLOADS[case, size]


def _luminances(t, key, cam, w, h):
    """float64 luminance of samples 0 .. max(COUNTS) - 1 of every pixel, traced once per scene, size and policy."""
    if key not in _LUM:
        _LUM[key] = sample_luminances(t, cam, w, h, max(COUNTS))
    return _LUM[key]


def _compare(t, key, cam, w, h, counts, fills=(0, 1), moments=(0, 1)):
    for fill in fills:
        t.setOption(t.OPT_WAVE_FILL, fill)
        for mom in moments:
            t.setOption(t.OPT_MOMENTS, mom)
            first = 0 if mom else 3
            for count in counts:
                got = []
                for share, queue in ((1, 1), (0, 0)):   # fused path with the sample queue; direct path pt_render
                    t.setOption(t.OPT_PREFIX_SHARING, share)
                    t.setOption(t.OPT_SAMPLE_QUEUE, queue)
                    t.clear()
                    t.renderSamples(cam, first, count)
                    t.sync()
                    got.append((t.readLinear().copy(), t.moments() if mom else None, t.sampleCounts() if mom else None))
                what = key + (fill, mom, count)
                assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32)), what
                if mom:
                    assert np.array_equal(got[0][2], got[1][2]), what
                    ref, tol = truth_and_tolerance(_luminances(t, key, cam, w, h), got[0][2])
                    for path, (_, m2, _) in zip(("fused", "direct"), got):
                        assert (np.abs(m2.astype(np.float64) - ref) <= tol).all() and (m2 >= 0).all(), what + (path,)
    assert t.walkOverflow() == 0


@pytest.mark.parametrize("arith", ["ieee", "rocm-opencl"])
@pytest.mark.parametrize("size", ["ragged", "tiny"])
@pytest.mark.parametrize("case", ["c2", "c3", "all_kinds", "c5"])
def test_fused_frames_equal_the_direct_path(case, size, arith):
    scene, cam, w, h = _workload(case, size)
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    try:
        _compare(t, (case, size, arith), cam, w, h, COUNTS)
    finally:
        t.close()


@pytest.mark.parametrize("arith", ["ieee", "rocm-opencl"])
def test_sharded_context_rank_1_of_3(arith):
    scene, cam, w, h = _workload("c2", "ragged")
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    t.setShard(1, 3)
    try:
        _compare(t, ("c2", "ragged", arith), cam, w, h, COUNTS, moments=(0,))   # (a sharded context keeps no moments: RT_EINVAL)
    finally:
        t.close()


@pytest.mark.parametrize("case", ["c2", "all_kinds"])
def test_counting_builds_equal_the_direct_path(case):
    scene, cam, w, h = _workload(case, "ragged")
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith("rocm-opencl")
    t.enableCounters(True)
    try:
        _compare(t, (case, "ragged", "rocm-opencl"), cam, w, h, (3, 33, 64, 200), moments=(0,))
    finally:
        t.close()
