"""GPU (-m gpu): the tagged forms of sqrt and normalize (csrc/pt_arith.hpp "tagged forms") and the sphere scan that
compares with the best hit inside the root block (csrc/pt_device.hpp sphere_take), which the sample queue
pt_samples_q<COUNT = false, ACCEL = false, GEOM 0 | 1> runs under the ROCm-OpenCL policies.

1. rt_debug_builtin ops 10, 11 against ops 4, 2 (the untagged forms, which tests/test_gpu_ref950.py pins to the
   reference's real OpenCL build), as uint32.  The probe kernel runs record i in thread i, so a wave is 64 consecutive
   records and the wave's choice of arm is the test's to make: waves with every lane in the fast range (more than half
   of the records of each op), waves with exactly one lane outside it — at lane 0, 31 or 63 — and waves with every lane
   outside.  The mixed and all-outside waves prove the slow arm: a correctly rounded sqrt there (what a speculated
   __builtin_sqrtf turns into) differs from the 3-ulp expansion in the in-range lanes of a mixed wave.
2. Frames of the fused path (pt_prefix + the tagged pt_samples_q) against the direct path pt_render, which keeps the
   untagged code, bits with ==: C2, C3 and the all-kinds scene, ragged and tiny, policies 0, 1, 2, counts below / at /
   above a wave's 64 lanes, sample moments off and on; C2 with more materials than the LDS table holds; C2 scaled down.

   The scaled scene.  RT_MIN_DISTANCE = 1e-3 is absolute: at a scale of 1e-20 every root is below it and the frame is
   black on every path (the CPU oracle under `ieee`: lit fraction 0.000 at 1e-10 and at 1e-20, 0.024 at 1e-5, 0.389 at
   1e-4, 0.44 from 1e-3 up).  A root t = b ± sqrt(dis) is accepted only for t >= 1e-3, so b² >= 2.5e-7 or dis >= 2.5e-7,
   and the computed dis = fma(b, b, -cc) is a multiple of the last bit of b² or cc — 2^-46 · 2.5e-7 > 1e-21 at the
   least — or zero: a denormal discriminant cannot belong to an accepted hit at any scale, and squared lengths under
   normalize are those of a unit normal plus a table vector, whatever the scale.  Denormal operands are therefore
   part 1's to prove; the frame is taken at 1e-4, the smallest decade at which the direct path still lights more than
   a tenth of the pixels (asserted), where the discriminants are down at 1e-8 ... 1e-12 and most roots straddle
   RT_MIN_DISTANCE."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
rt = cases.rt

WAVE = 64
FLT_MIN = np.float32(2.0 ** -126)


def _bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def _waves(fast, outside, rng):
    """Records of one probe run.  fast(n) → n records inside the fast range; outside: records outside it (or at its
    edge).  → (records, number of all-in-range waves, number of waves)."""
    mixed = []
    for rec in outside:
        for lane in (0, 31, 63):
            w = fast(WAVE)
            w[lane] = rec
            mixed.append(w)
    n_out = max(2, (len(outside) + WAVE - 1) // WAVE)
    all_out = [outside[rng.integers(0, len(outside), WAVE)] for _ in range(n_out)]
    for k, rec in enumerate(outside):        # every outside record at least once among the all-outside waves
        all_out[k // WAVE][k % WAVE] = rec
    n_fast = len(mixed) + len(all_out) + 4   # more than half of the records
    all_in = [fast(WAVE) for _ in range(n_fast)]
    order = [all_in[0]] + mixed + all_out + all_in[1:]   # (a 256-thread block holds four waves: kinds side by side)
    return np.concatenate(order).astype(np.float32), n_fast, len(order)


def _sqrt_records():
    rng = np.random.default_rng(5)

    def fast(n):
        v = np.zeros((n, 8), np.float32)
        v[:, 0] = np.abs(rng.standard_normal(n)).astype(np.float32) * np.exp2(rng.integers(-40, 40, n)).astype(np.float32) + FLT_MIN
        v[::7, 0] = FLT_MIN                                      # the edge itself is inside: the expansion scales x < FLT_MIN
        v[3::11, 0] = np.nextafter(FLT_MIN, np.float32(1.0))
        return v
    edge = np.concatenate([np.array([0.0, -0.0, -2.5, np.inf], np.float32),
                           _bits(0x007FFFFF,    # the largest denormal = FLT_MIN's neighbour below
                                 0x00400000,    # a mid denormal
                                 0x00000001,    # the smallest
                                 0x00800000,    # FLT_MIN
                                 0x00800001,    # its neighbour above
                                 0x7FC00000)])  # a quiet NaN
    outside = np.zeros((len(edge), 8), np.float32)
    outside[:, 0] = edge
    return _waves(fast, outside, rng)


def _normalize_records():
    rng = np.random.default_rng(6)

    def fast(n):
        v = np.zeros((n, 8), np.float32)
        v[:, :3] = rng.standard_normal((n, 3)).astype(np.float32) * np.exp2(rng.integers(-12, 12, (n, 1))).astype(np.float32)
        v[::9, :3] = (np.float32(2.0 ** -63), 0.0, 0.0)          # squared length exactly FLT_MIN: a normal number
        return v
    outside = np.zeros((12, 8), np.float32)
    outside[1, :3] = 1e-30                                        # squared length below FLT_MIN
    outside[2, :3] = (1e-30, -3e-31, 0.0)
    outside[3, :3] = 1e30                                         # squared length infinite
    outside[4, :3] = (-2e30, 1e25, 3.0)
    outside[5, :3] = (np.inf, 1.0, -2.0)
    outside[6, :3] = (-np.inf, np.inf, 0.0)
    outside[7, :3] = (np.nan, 1.0, 2.0)
    outside[8, :3] = (0.5, 0.25, np.nan)
    outside[9, :3] = (np.float32(2.0 ** -64), 0.0, 0.0)           # squared length 2^-128: a denormal
    outside[10, :3] = (0.0, np.float32(2.0 ** -63), 0.0)          # exactly FLT_MIN again (the fast range's edge, inside)
    outside[11, :3] = (0.0, -0.0, 0.0)
    return _waves(fast, outside, rng)


PROBES = {"sqrt": (10, 4, _sqrt_records), "normalize": (11, 2, _normalize_records)}


@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("name", sorted(PROBES))
def test_tagged_form_has_the_untagged_forms_bits(name, policy):
    tagged, plain, make = PROBES[name]
    v, n_fast, n_waves = make()
    assert len(v) == n_waves * WAVE and 2 * n_fast >= n_waves     # the fast arm is what most of the test runs
    t = rt.RayTracer(8, 8, scene=rt.workloads.get("c1", width=8, height=8).scene)
    t.setArith(policy)
    try:
        a, b = t.debugBuiltin(tagged, v).view(np.uint32), t.debugBuiltin(plain, v).view(np.uint32)
    finally:
        t.close()
    bad = (a != b).any(axis=1)
    assert not bad.any(), (name, policy, int(bad.sum()), np.flatnonzero(bad)[:8], v[bad][:4], a[bad][:4], b[bad][:4])


# ---- 2. frames --------------------------------------------------------------------------------------------------------
COUNTS = (1, 3, 64, 65)
_KW = {"c2": {}, "all_kinds": {}, "c3": dict(tex_size=64)}


def _workload(case, size):
    w, h = (7, 5) if size == "tiny" else (61, 37)
    return rt.workloads.get(case, width=w, height=h, **_KW[case])


def _both_paths(t, cam, first, count, mom):
    got = []
    for share, queue in ((1, 1), (0, 0)):   # fused path with the sample queue; direct path pt_render
        t.setOption(t.OPT_PREFIX_SHARING, share)
        t.setOption(t.OPT_SAMPLE_QUEUE, queue)
        t.clear()
        t.renderSamples(cam, first, count)
        t.sync()
        got.append((t.readLinear().copy(), t.sampleCounts().copy() if mom else None))
    return got


def _compare(scene, cam, w, h, policy, what, counts=COUNTS, moments=(0, 1), lit_at_least=None):
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(policy)
    try:
        for mom in moments:
            t.setOption(t.OPT_MOMENTS, mom)
            for count in counts:
                (fused, nf), (direct, nd) = _both_paths(t, cam, 0 if mom else 3, count, mom)
                key = what + (policy, mom, count)
                if lit_at_least is not None:   # (a black frame would compare equal whatever the code does)
                    lit = float((direct[..., :3] > 0).any(axis=2).mean())
                    assert lit >= lit_at_least, key + ("vacuous: lit fraction", lit)
                same = fused.view(np.uint32) == direct.view(np.uint32)
                assert same.all(), key + (int((~same).any(axis=2).sum()),)
                if mom:
                    assert np.array_equal(nf, nd), key
        assert t.walkOverflow() == 0
    finally:
        t.close()


@pytest.mark.parametrize("policy", [0, 1, 2])
@pytest.mark.parametrize("size", ["ragged", "tiny"])
@pytest.mark.parametrize("case", ["c2", "c3", "all_kinds"])
def test_fused_frames_equal_the_direct_path(case, size, policy):
    wl = _workload(case, size)
    _compare(wl.scene, wl.camera, wl.width, wl.height, policy, (case, size))


@pytest.mark.parametrize("policy", [0, 1, 2])
def test_more_materials_than_the_lds_table_holds(policy):
    wl = _workload("c2", "ragged")
    for k in range(70):   # 79 materials: stage_materials stages none, every colour comes from the global records
        wl.scene.addMaterial(rt._abi.T_DIFFUSE, (0.1 + 0.01 * k, 0.5, 0.9), 1.0)
    _compare(wl.scene, wl.camera, wl.width, wl.height, policy, ("c2", "79 materials"))


@pytest.mark.parametrize("policy", [0, 1, 2])
def test_scaled_down_scene(policy):
    wl = _workload("c2", "ragged")
    s = np.float32(1e-4)
    wl.scene.spheres["pos"] *= s
    wl.scene.spheres["r"] *= s
    wl.scene.planes["pos"] *= s
    cam = wl.camera.copy()
    cam[:3] *= s
    _compare(wl.scene, cam, wl.width, wl.height, policy, ("c2", "scaled 1e-4"), lit_at_least=0.1)
