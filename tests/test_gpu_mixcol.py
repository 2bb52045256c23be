"""GPU (-m gpu): mixCol's minimum in its tagged form (csrc/pt_arith.hpp vmin<FAST>: the bare v_min_f32, no canonicalising
of the operands) and the sample queue's carried state written in place (csrc/pt_samples_q_kernel.hpp SIP_*, MAT_*), which
pt_samples_q<COUNT = false, ACCEL = false, GEOM 0 | 1> runs; DESIGN §2 and §5, profiles/r29_experiments.md.

1. rt_debug_builtin op 12 (tagged) against op 6 (the untagged min: __ocml_min_f32 under policies 1 and 2, which
   tests/test_gpu_ref950.py pins to the reference's real OpenCL build), as uint32, record i in thread i as in
   tests/test_gpu_fast_builtins.py.  Operands: +0 and -0 in both orders, equal values, denormals (0x00000001 and 0x007FFFFF
   among them), FLT_MIN, 1, values above 1, +inf and -inf, negative values, a quiet NaN as first operand, as second and as
   both — every ordered pair of the pool in every channel, then waves whose 64 lanes draw all six words from the pool at
   random.  Signalling NaNs are left out: they are outside the tagged form's contract.  The untagged min quiets one (that
   is all its canonicalising instructions do), the bare instruction's answer to one is not part of what the contract
   promises, and no colour can hold one that did not come in through rt_set_scene — where a NaN colour is as
   much outside the renderer's contract as a NaN radiance is.
2. Frames of the fused path (pt_prefix + pt_samples_q) against the direct path pt_render, which keeps the untagged code
   and carries no state, linear frames with ==: C2 and the all-kinds scene ragged and tiny, C3 ragged, policies 0, 1, 2,
   counts (spp, first) = (1, 0), (5, 3), (64, 0), (200, 7) — the 64-sample instantiation, the generic one, a count above a
   wave's lanes; C2 with more materials than the LDS table holds (load_material's global arm); and a C2 whose colours and
   extra_data hold 0, a denormal, 1 and 2.5, with the light's colour below the path colour in one channel, above it in
   another and equal to it in the third, so that the minimum selects each operand and meets ties (rt_set_scene accepted
   every one of these values as given: none was replaced)."""
import numpy as np
import pytest

import cases
from oracle import Oracle

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi

WAVE = 64
OP_MIN, OP_MIN_TAGGED = 6, 12


def _bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


QNAN = 0x7FC00000
POOL = np.concatenate([
    _bits(0x00000000, 0x80000000,                  # +0, -0
          0x00000001, 0x007FFFFF, 0x00400000,      # the smallest, the largest and a mid denormal
          0x80000001, 0x807FFFFF,                  # negative denormals
          0x00800000, 0x00800001,                  # FLT_MIN and its neighbour above
          0x7F800000, 0xFF800000,                  # +inf, -inf
          0x7F7FFFFF,                              # FLT_MAX
          QNAN, 0xFFC00001),                       # quiet NaNs (one negative, with a payload)
    np.array([1.0, 1.0000001, 2.5, 0.5, 0.9, 1e-40, 3e38, -1.0, -2.5, -1e-40, -0.15, 1e-20], np.float32)])


def _min_records():
    rng = np.random.default_rng(29)
    n = len(POOL)
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()                # every ordered pair: both orders, and every value with itself
    pairs = np.zeros((n * n, 8), np.float32)
    for ch in range(3):                            # the same pairs in every channel, in another order each
        o = np.roll(np.arange(n * n), 17 * ch)
        pairs[:, ch], pairs[:, 3 + ch] = POOL[ii[o]], POOL[jj[o]]
    n_mixed = 40 * WAVE
    mixed = np.zeros((n_mixed, 8), np.float32)
    mixed[:, :6] = POOL[rng.integers(0, n, (n_mixed, 6))]
    v = np.concatenate([pairs, mixed])
    pad = (-len(v)) % WAVE
    return np.concatenate([v, v[:pad]]) if pad else v


@pytest.mark.parametrize("policy", [0, 1, 2])
def test_tagged_min_has_the_untagged_mins_bits(policy):
    v = _min_records()
    assert 2000 <= len(v) <= 8000 and len(v) % WAVE == 0
    w = v.view(np.uint32)
    is_nan = (w[:, :6] & 0x7FFFFFFF) > 0x7F800000
    assert not (is_nan & ((w[:, :6] & 0x00400000) == 0)).any()          # quiet NaNs only
    assert is_nan[:, 0].any() and is_nan[:, 3].any() and (is_nan[:, 0] & is_nan[:, 3]).any()
    t = rt.RayTracer(8, 8, scene=rt.workloads.get("c1", width=8, height=8).scene)
    t.setArith(policy)
    try:
        a, b = t.debugBuiltin(OP_MIN_TAGGED, v).view(np.uint32), t.debugBuiltin(OP_MIN, v).view(np.uint32)
    finally:
        t.close()
    bad = (a != b).any(axis=1)
    print("policy %d: %d records, %d differ" % (policy, len(v), int(bad.sum())))
    assert not bad.any(), (policy, int(bad.sum()), np.flatnonzero(bad)[:8], w[bad][:4], a[bad][:4], b[bad][:4])
    # not vacuous: the answer is the first operand in some records and the second in others, and a number beside a NaN
    assert (b[:, 0] != w[:, 0]).any() and (b[:, 0] != w[:, 3]).any()
    if policy != 0:   # (policy 0 compares and selects: beside a NaN it returns its first operand)
        one_nan = is_nan[:, 0] & ~is_nan[:, 3]
        assert np.array_equal(b[one_nan, 0], w[one_nan, 3])


# ---- 2. frames --------------------------------------------------------------------------------------------------------
COUNTS = ((1, 0), (5, 3), (64, 0), (200, 7))   # (spp, first)
_KW = {"c2": {}, "all_kinds": {}, "c3": dict(tex_size=64)}
_GEOM = {"c2": 0, "all_kinds": None, "c3": 1}   # (the all-kinds scene: whatever the plan gives it)


def _workload(case, size):
    w, h = (7, 5) if size == "tiny" else (61, 37)
    return rt.workloads.get(case, width=w, height=h, **_KW[case])


def _compare(scene, cam, w, h, policy, what, geom=None, lit_at_least=None):
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(policy)
    try:
        for spp, first in COUNTS:
            frames = []
            for share, queue in ((1, 1), (0, 0)):   # fused path with the sample queue; direct path pt_render
                t.setOption(t.OPT_PREFIX_SHARING, share)
                t.setOption(t.OPT_SAMPLE_QUEUE, queue)
                t.clear()
                t.renderSamples(cam, first, spp)
                t.sync()
                frames.append(t.readLinear().copy())
                if share:   # the queue family ran, without counters
                    facts, plan = t.lastSamplePlan()
                    assert plan["family"] == A.PLAN_QUEUE and facts["count_enabled"] == 0, what + (policy, spp, facts, plan)
                    if geom is not None:
                        assert plan["geom"] == geom and plan["accel"] == 0, what + (policy, spp, plan)
                    if spp == 64:
                        assert plan["count_log2"] == 6, what + (policy, plan)
            fused, direct = frames
            key = what + (policy, spp, first)
            if lit_at_least is not None:   # (a black frame would compare equal whatever the code does)
                lit = float((direct[..., :3] > 0).any(axis=2).mean())
                assert lit >= lit_at_least, key + ("vacuous: lit fraction", lit)
            same = fused.view(np.uint32) == direct.view(np.uint32)
            assert same.all(), key + (int((~same).any(axis=2).sum()),)
        assert t.walkOverflow() == 0
    finally:
        t.close()


@pytest.mark.parametrize("policy", [0, 1, 2])
@pytest.mark.parametrize("case,size", [("c2", "ragged"), ("c2", "tiny"), ("all_kinds", "ragged"), ("all_kinds", "tiny"), ("c3", "ragged")])
def test_fused_frames_equal_the_direct_path(case, size, policy):
    wl = _workload(case, size)
    _compare(wl.scene, wl.camera, wl.width, wl.height, policy, (case, size), geom=_GEOM[case])


@pytest.mark.parametrize("policy", [0, 1, 2])
def test_more_materials_than_the_lds_table_holds(policy):
    wl = _workload("c2", "ragged")
    for k in range(70):   # 79 materials: none is staged, every colour and type comes from the global records
        wl.scene.addMaterial(A.T_DIFFUSE, (0.1 + 0.01 * k, 0.5, 0.9), 1.0)
    _compare(wl.scene, wl.camera, wl.width, wl.height, policy, ("c2", "79 materials"), geom=0)


def _edge_colours():
    """C2 (assets/scenes/c2_cornell.scene) with colours and extra_data of 0, 1e-40 (a denormal), 1 and 2.5.  The path colour
    starts at 1: past the green sphere (extra_data 2.5) it is 2.5, so the light's (0.5, 2.5, 1) is below it in the first
    channel, never below it in the second, and ties with an untouched 1 in the third."""
    wl = _workload("c2", "ragged")
    m = wl.scene.materials
    assert len(m) == 9 and int(m["type"][7]) == A.T_LIGHT
    m["color"][1][:3] = (0.9, 0.8, 1e-40)   # brass mirror: a denormal channel
    m["extra_data"][1] = 1e-40              # ... and a denormal attenuation: denormal path colours from here on
    m["color"][3][:3] = (2.5, 1e-40, 0.0)   # red diffuse: above every path colour, a denormal, and 0
    m["color"][4][:3] = (1.0, 2.5, 0.15)    # green diffuse
    m["extra_data"][4] = 2.5                # ... which raises the path colour above 1
    m["color"][6][:3] = (0.0, 1.0, 2.5)     # tinted crystal (its extra_data stays a refractive index)
    m["color"][7][:3] = (0.5, 2.5, 1.0)     # the light
    m["color"][8][:3] = (1.0, 0.9, 2.5)     # floor: ties with an untouched path colour in the first channel
    m["extra_data"][8] = 1.0
    return wl


@pytest.fixture(scope="module")
def edge_workload():
    wl = _edge_colours()
    t = rt.RayTracer(8, 8, scene=wl.scene, seed=cases.SEED)   # (the table of the seed every tracer here uses)
    try:
        table = t.getRandomTable()
    finally:
        t.close()
    img, _ = Oracle().render(wl.scene, wl.camera, table, wl.width, wl.height, 2, count=4, threads=4)
    lit = float((img[..., :3] > 0).any(axis=2).mean())
    print("edge colours: the CPU oracle lights %.3f of the pixels at %dx%d" % (lit, wl.width, wl.height))
    assert lit >= 0.1, lit
    return wl


@pytest.mark.parametrize("policy", [0, 1, 2])
def test_colours_that_make_the_minimum_select_each_operand(edge_workload, policy):
    wl = edge_workload
    _compare(wl.scene, wl.camera, wl.width, wl.height, policy, ("c2", "edge colours"), geom=0, lit_at_least=0.1)
