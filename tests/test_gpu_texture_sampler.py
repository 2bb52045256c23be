"""GPU (-m gpu): texture_rgb of csrc/pt_device.hpp on the scenes of tests/texture_cases.py (a sample's radiance is the
texel) — textures that are not square, 1 to 3 layers, uv inside, across and far outside [0, 1], at exactly 0 and 1 and
at +-1e30.

Policy 0: every pixel of samples 0 and 1 bit for bit against the CPU oracle (which tests/test_texture_sampler_host.py
pins to the float64 definition), through the probe kernel and through the fused frame with the acceleration structures
off and on.  Policies 1 and 2: against the float64 reference of tests/texture_ref.py with the host test's bound — their
contracted getTextureUV moves uv by ulps, so this is their first independent check of the textured path.  Under every
policy the feature record's albedo is the float32 texel at the record's own uv, bit for bit, and that uv is the float64
geometry's within its bound.  The wave-fixed kernels see a texture that is not square through the lazy texel of GEOM 0."""
import numpy as np
import pytest

import cases
import chain_ref
import texture_cases as TC
import texture_ref as R
from test_texture_sampler_host import all_pixels, built_case, check_radiance
from test_gpu_wave_fixed import SIZES, _frame, _same, _textured_c2

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
POLICIES = (rt.ARITH_IEEE, rt.ARITH_ROCM_OCL_NOCONTRACT, rt.ARITH_ROCM_OCL)
# |uv - float64 uv| / (2^-24 max(1, |uv|max)) of the CPU oracle's hit records over all cases: largest 9.27 (5x3-far; 6.5 on
# 5x3-straddle-slant).  The bound is twice that.
C_UV = 19.0


@pytest.fixture(scope="module", params=TC.CASES, ids=TC.case_id)
def tracer(request):
    s, cam, uv_max, fh = built_case(request.param)
    t = rt.RayTracer(TC.W, TC.H, scene=s, seed=cases.SEED)
    yield TC.case_id(request.param), t, s, cam, uv_max, fh
    t.setArith(rt.ARITH_IEEE)
    t.close()


def test_policy_0_is_the_oracle_bit_for_bit(tracer, oracle):
    name, t, s, cam, uv_max, fh = tracer
    t.setArith(rt.ARITH_IEEE)
    table = t.getRandomTable()
    exp = []
    for sample in (0, 1):
        xs, ys, ss = all_pixels(sample)
        got = t.traceSamples(cam, xs, ys, ss)
        e, _ = oracle.samples(s, cam, table, TC.W, TC.H, xs, ys, ss)
        assert np.array_equal(got.view(np.uint32), e.view(np.uint32)), (name, sample)
        exp.append(e)
    # the radiance is the texel whatever the sample, so the mean of 4 samples is the texel too, exactly
    assert np.array_equal(exp[0].view(np.uint32), exp[1].view(np.uint32)), name
    for accel in (0, 1):
        t.setOption(t.OPT_ACCEL, accel)
        t.clear()
        t.renderSamples(cam, 0, 4)
        t.sync()
        frame = np.ascontiguousarray(t.readLinear()[..., :3]).reshape(-1, 3)
        assert np.array_equal(frame.view(np.uint32), exp[0].view(np.uint32)), (name, "fused, accel %d" % accel)
    t.setOption(t.OPT_ACCEL, 1)


@pytest.mark.parametrize("policy", POLICIES[1:])
def test_policies_1_and_2_are_the_float64_texel(tracer, policy):
    name, t, s, cam, uv_max, fh = tracer
    t.setArith(policy)
    for sample in (0, 1):
        got = t.traceSamples(cam, *all_pixels(sample))
        check_radiance(got.reshape(TC.H, TC.W, 3), s, fh, uv_max, (name, "policy %d" % policy, sample))


@pytest.mark.parametrize("policy", POLICIES)
def test_feature_albedo_is_the_texel_at_the_records_uv(tracer, policy):
    name, t, s, cam, uv_max, fh = tracer
    t.setArith(policy)
    t.renderFeatures(cam)
    t.sync()
    rec = t.featureRecords()
    hit = (rec["flags"] & A.FEATURE_HIT) != 0
    quad = hit & (rec["material"] == 0)
    keep = fh["edge"] >= R.EDGE_MARGIN
    assert np.array_equal(quad[keep], fh["hit"][keep]), name
    r = rec[quad]
    alb = chain_ref.texel(s, r["u"], r["v"], r["tex"])
    assert np.array_equal(r["albedo"].view(np.uint32), alb.view(np.uint32)), (name, policy)
    k = quad & keep
    assert np.array_equal(rec["tex"][k], fh["tex"][k].astype(np.uint32)), name
    bound = C_UV * 2.0 ** -24 * max(1.0, uv_max)
    eu, ev = np.abs(rec["u"][k] - fh["u"][k]).max(), np.abs(rec["v"][k] - fh["v"][k]).max()
    print("%s policy %d: |u - u64| %.3g, |v - v64| %.3g, bound %.3g" % (name, policy, eu, ev, bound))
    assert max(eu, ev) <= bound, (name, policy, eu, ev, bound)


@pytest.mark.parametrize("arith", ["ieee", "rocm-opencl"])
def test_wave_fixed_kernels_fetch_from_a_texture_that_is_not_square(arith):
    """C2 with one textured sphere (u = v = 0, layer 0) and a 5 x 3 two-layer texture: the 64-sample instantiation's lazy
    texel is texel (0, 0) of layer 0 — the frame is the direct path's, and another frame than with that texel changed."""
    w, h = SIZES["ragged"]
    frames = []
    for other in (False, True):
        wl = _textured_c2(w, h)
        tex = TC.random_texture("5x3")[:2].copy()
        if other:
            tex[0, 0, 0, :3] = 1.0 - tex[0, 0, 0, :3]
        wl.scene.setTextures(tex)
        t = rt.RayTracer(w, h, scene=wl.scene, seed=cases.SEED)
        t.setArith(arith)
        try:
            frames.append(_frame(t, wl.camera, 0, 64, True))
            assert t.waveFixedStats()[0] == 1
            assert _same(frames[-1], _frame(t, wl.camera, 0, 64, False))
        finally:
            t.close()
    assert (frames[0].view(np.uint32) != frames[1].view(np.uint32)).any()
    # no other texel matters: with every other texel of layer 0 and all of layer 1 changed the frame stays (a wrong row
    # stride, a u / v swap or a wrong layer would show)
    wl = _textured_c2(w, h)
    changed = TC.random_texture("5x3")[:2].copy()
    changed[0, :, 1:, :3] = 0.5
    changed[0, 1:, :, :3] = 0.5
    changed[1] = 0.25
    wl.scene.setTextures(changed)
    t = rt.RayTracer(w, h, scene=wl.scene, seed=cases.SEED)
    t.setArith(arith)
    try:
        assert _same(_frame(t, wl.camera, 0, 64, True), frames[0])
    finally:
        t.close()
