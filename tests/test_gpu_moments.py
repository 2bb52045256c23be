"""GPU (-m gpu): the per-pixel sample moments (RT_OPT_MOMENTS) and rt_denoise_moments.  Every path that adds to the
accumulator must leave M2 = sum (l(s_j) - mean)^2 of exactly the samples the pixel holds — checked against the float64
two-pass moment of traceSamples' radiances (bit-exact per sample under the context's own policy) — without moving a bit
of the accumulator, the image or the counts; the filter must follow its restatement (tests/moments_ref.py) and beat the
spatial estimate from 16 spp on.

Figures of an MI355X run are in DESIGN.md, "Measured variance"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import denoise_vg_ref as V
import moments_ref as M

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
R = rt.raytracer
ROOT = cases.ROOT
CLI = os.path.join(ROOT, "host", "rt_cli")
ASSETS = os.path.join(ROOT, "assets")
EINVAL, ESTATE = -1, -4
OPT_MOMENTS = 12


def read_accum(t):
    import torch
    t.sync()
    return torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().copy()


def sample_luminances(t, cam, w, h, n):
    """float64 luminance of samples 0 .. n-1 of every pixel → (h, w, n)."""
    ys, xs = np.mgrid[0:h, 0:w]
    s = t.traceSamples(cam, np.repeat(xs.reshape(-1), n), np.repeat(ys.reshape(-1), n), np.tile(np.arange(n), w * h))
    return (s.astype(np.float64) @ V.LUM).reshape(h, w, n)


def truth_and_tolerance(lum, counts):
    """Per pixel: the two-pass M2 of its first counts[p] samples and the issue's tolerance for it."""
    h, w, nmax = lum.shape
    counts = np.broadcast_to(np.asarray(counts), (h, w))
    use = np.arange(nmax)[None, None, :] < counts[..., None]
    k = np.maximum(counts, 1)
    mean = np.where(use, lum, 0.0).sum(-1) / k
    m2 = np.where(use, (lum - mean[..., None]) ** 2, 0.0).sum(-1)
    lmax = np.where(use, lum, 0.0).max(-1)
    return m2, M.tolerance(m2, counts, lmax)


def both_ways(t, render):
    """`render(t)` after a clear with the option off and on: accumulator, resolved image and counts must not differ in a
    bit → (accumulator, moments)."""
    got = []
    for on in (0, 1):
        t.setOption(OPT_MOMENTS, on)
        t.clear()
        render(t)
        t.resolve()
        got.append((read_accum(t), t.transferImage(), t.sampleCounts()))
    for a, b in zip(got[0], got[1]):
        assert a.tobytes() == b.tobytes()
    return got[1][0], t.moments()


def assert_moments(m2, lum, counts, what):
    ref, tol = truth_and_tolerance(lum, counts)
    err = np.abs(m2.astype(np.float64) - ref)
    worst = np.unravel_index(np.argmax(err - tol), err.shape)
    print("%s: max |M2 - truth| %.3g, worst pixel %s: %.9g vs %.9g (tol %.3g); max M2 %.4g" %
          (what, err.max(), worst, m2[worst], ref[worst], tol[worst], ref.max()))
    assert (err <= tol).all(), what
    assert (m2 >= 0).all()


CONFIGS = {
    "default": [],
    "queue0": [(R.OPT_SAMPLE_QUEUE, 0)],
    "sharing0": [(R.OPT_PREFIX_SHARING, 0)],
    "tree0": [(R.OPT_PREFIX_TREE, 0)],
    "tree2": [(R.OPT_PREFIX_TREE, 2)],
}
COUNTS = (1, 2, 3, 5, 24, 64)
_lum_cache = {}


def _tracer(wl, policy=0, config="default"):
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    if policy:
        t.setArith(policy)
    for o, v in CONFIGS[config]:
        t.setOption(o, v)
    return t


# ---- 1. every path ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("policy", [0, 2])
def test_every_path_c2(policy, config):
    w, h = 24, 16
    wl = rt.workloads.get("c2", width=w, height=h)
    t = _tracer(wl, policy, config)
    try:
        if policy not in _lum_cache:
            _lum_cache[policy] = sample_luminances(t, wl.camera, w, h, max(COUNTS))
        lum = _lum_cache[policy]
        for n in COUNTS:
            acc, m2 = both_ways(t, lambda t: t.renderSamples(wl.camera, 0, n))
            assert (acc[..., 3] == n).all()
            assert_moments(m2, lum, n, "c2 policy %d %s n %d" % (policy, config, n))
            if n == 1:
                assert (m2 == 0).all()
            if config != "sharing0":     # a fused launch: the pixels pt_prefix finished hold M2 == 0 exactly
                _, _, light, heavy = t.liveList()
                live = light + heavy
                assert 0 < live < w * h, "the frame must hold live and finished pixels"
                assert (m2 == 0).sum() >= w * h - live
                t.renderFeatures(wl.camera)
                sky = ~t.features()["hit"]
                assert sky.any() and (m2[sky] == 0).all()
    finally:
        t.close()


# ---- 2. trees really built ----------------------------------------------------------------------------------------------

def _glass_wall():
    """One large dielectric sphere right in front of the camera: every pixel's first random event is glass."""
    s = rt.SceneCreator()
    s.addMaterial(A.T_DIELECTRIC, (1, 1, 1), 1.5)
    s.addMaterial(A.T_DIFFUSE, (0.8, 0.7, 0.6), 0.9)
    s.addMaterial(A.T_LIGHT, (1, 1, 1), 0)
    s.addMaterial(A.T_DIELECTRIC, (1, 0.9, 0.9), 2.4)
    s.addSphere((0, 0, 0), 5.9, 0)
    s.addSphere((0.5, 0.3, 1.0), 1.5, 3)
    s.addSphere((0, 250, 0), 120, 2)
    s.addPlane((0, -7, 0), (0, 1, 0), 1)
    return s, rt.Camera(60, 16 / 9, (0, 0, -6), 0.0, 0.0).transferData()


def test_glass_wall_with_trees():
    w, h, n = 16, 12, 24
    scene, cam = _glass_wall()
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    try:
        t.setOption(R.OPT_PREFIX_TREE, 2)
        lum = sample_luminances(t, cam, w, h, n)
        acc, m2 = both_ways(t, lambda t: t.renderSamples(cam, 0, n))
        assert_moments(m2, lum, n, "glass wall, trees, n %d" % n)
        assert (m2 > 0).sum() > w * h // 2
    finally:
        t.close()


# ---- 3. merging across launches -----------------------------------------------------------------------------------------

def test_moments_merge_across_launches():
    w, h = 24, 16
    wl = rt.workloads.get("c2", width=w, height=h)
    t = _tracer(wl)
    try:
        lum = sample_luminances(t, wl.camera, w, h, 32)
        hits0 = t.prefixCacheStats()[0]

        def three_calls(t):
            t.renderSamples(wl.camera, 0, 3)
            t.renderSamples(wl.camera, 3, 5)
            t.renderSamples(wl.camera, 8, 24)
        acc, m2 = both_ways(t, three_calls)
        assert t.prefixCacheStats()[0] >= hits0 + 2, "pt_final_replay must have run"
        assert (acc[..., 3] == 32).all()
        assert_moments(m2, lum, 32, "c2 3 + 5 + 24 samples")
    finally:
        t.close()


def test_moments_of_a_call_split_into_two_launches():
    w, h, n = 8, 6, 520     # 512 + 8
    wl = rt.workloads.get("c2", width=w, height=h)
    t = _tracer(wl)
    try:
        lum = sample_luminances(t, wl.camera, w, h, n)
        acc, m2 = both_ways(t, lambda t: t.renderSamples(wl.camera, 0, n))
        assert (acc[..., 3] == n).all()
        assert_moments(m2, lum, n, "c2 520 samples in one call")
    finally:
        t.close()


# ---- 4. mesh kernels ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["c3", "c5", "c5_no_slices"])
def test_mesh_kernels(case):
    if case == "c3":
        wl = rt.workloads.get("c3", width=32, height=20, tex_size=64)
    else:
        wl = rt.workloads.get("c5", width=24, height=16, segments=24, rings=16)
    t = _tracer(wl)
    try:
        if case == "c5_no_slices":
            t.setOption(R.OPT_WALK_SLICES, 0)
        lum = sample_luminances(t, wl.camera, wl.width, wl.height, 64)
        for n in (8, 64):
            acc, m2 = both_ways(t, lambda t: t.renderSamples(wl.camera, 0, n))
            assert_moments(m2, lum, n, "%s n %d" % (case, n))
            assert (m2 > 0).any()
    finally:
        t.close()


# ---- 5. adaptive --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", ["default", "sharing0"])
def test_adaptive_moments(config):
    w, h = 40, 24
    wl = rt.workloads.get("c2", width=w, height=h)
    t = _tracer(wl, 0, config)
    try:
        lum = sample_luminances(t, wl.camera, w, h, 32)
        acc, m2 = both_ways(t, lambda t: t.renderAdaptive(wl.camera, 0.05, batch=4, min_spp=8, max_spp=32))
        counts = t.sampleCounts()
        assert len(np.unique(counts)) > 1
        assert_moments(m2, lum, counts, "c2 adaptive %s, counts %s" % (config, np.unique(counts)))
        # a later renderSamples on top of the adaptive frame keeps merging
        t.renderSamples(wl.camera, 32, 8)
        lum2 = np.concatenate([lum, sample_luminances(t, wl.camera, w, h, 40)[..., 32:]], axis=-1)
        full = counts == 32
        assert full.any()
        ref, tol = truth_and_tolerance(lum2, 40)
        assert (np.abs(t.moments().astype(np.float64) - ref)[full] <= tol[full]).all()
    finally:
        t.close()


# ---- 7. the filter against the restatement ------------------------------------------------------------------------------

def _against_restatement(t, wl, iterations=5, **kw):
    args = dict(A.DENOISE_VARIANCE_DEFAULTS)
    args.update(iterations=iterations)
    args.update(kw)
    acc, m2 = read_accum(t), t.moments()
    t.renderFeatures(wl.camera)
    feats = t.features()
    got = t.denoiseMoments(**args)
    v0, vl = t.variance(0), t.variance(1)
    exp, lin, v0_ref, vl_ref = M.filter_moments(acc, m2, feats, **args)
    has = acc[..., 3] > 0
    assert np.array_equal(got[~has], np.zeros_like(got[~has]))
    assert (got[has, 3] == 1).all()
    e_c = np.abs(got[has, :3].astype(np.float64) ** 2 - lin[has]).max() if has.any() else 0.0
    e_v0 = (np.abs(v0 - v0_ref) / np.maximum(1.0, v0_ref)).max()
    e_vl = (np.abs(vl - vl_ref) / np.maximum(1.0, vl_ref)).max()
    print("%dx%d L=%d %s: linear colour %.3g, v0 %.3g, v(L) %.3g (bound 2e-5 each)" %
          (wl.width, wl.height, iterations, kw, e_c, e_v0, e_vl))
    assert e_c <= 2e-5 and e_v0 <= 2e-5 and e_vl <= 2e-5
    return got, v0, vl


@pytest.fixture(scope="module")
def c2():
    wl = rt.workloads.get("c2", width=244, height=138)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    t.setOption(OPT_MOMENTS, 1)
    yield wl, t
    t.close()


@pytest.mark.parametrize("spp,iterations", [(4, 5), (16, 5), (4, 1), (16, 8)])
def test_filter_matches_the_restatement_c2(c2, spp, iterations):
    wl, t = c2
    t.renderFrame(wl.camera, spp)
    got, v0, _ = _against_restatement(t, wl, iterations=iterations)
    # every pixel is above the threshold: v0 is the measured variance, not the 7x7 estimate
    spatial = t.denoiseVariance()
    assert not np.array_equal(v0, t.variance(0)) and not np.array_equal(got, spatial)


@pytest.mark.parametrize("size", [(37, 23), (7, 5), (1, 1)])
def test_filter_matches_the_restatement_on_tiny_frames(size):
    wl = rt.workloads.get("c2", width=size[0], height=size[1])
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        t.setOption(OPT_MOMENTS, 1)
        for spp in (4, 16):
            t.renderFrame(wl.camera, spp)
            for iterations in (1, 5, 8):
                _against_restatement(t, wl, iterations=iterations)
    finally:
        t.close()


def test_below_the_threshold_it_is_the_variance_guided_filter(c2):
    wl, t = c2
    for spp in (2, 3):
        t.renderFrame(wl.camera, spp)
        t.renderFeatures(wl.camera)
        a = (t.denoiseMoments(), t.variance(0), t.variance(1))
        b = (t.denoiseVariance(), t.variance(0), t.variance(1))
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_filter_matches_the_restatement_on_a_mixed_adaptive_frame(c2):
    wl, t = c2
    t.renderAdaptive(wl.camera, 0.05, batch=1, min_spp=2, max_spp=8)
    counts = t.sampleCounts()
    assert (counts < 4).any() and (counts >= 4).any()
    _, v0, _ = _against_restatement(t, wl)
    t.denoiseVarianceOnDevice()
    spatial = t.variance(0)
    assert np.array_equal(v0[counts < 4], spatial[counts < 4]) and not np.array_equal(v0[counts >= 4], spatial[counts >= 4])


# ---- 8. quality ---------------------------------------------------------------------------------------------------------

def gamma_rmse(a, b):
    return float(np.sqrt(((a[..., :3].astype(np.float64) - b[..., :3]) ** 2).mean()))


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_measured_variance_beats_the_spatial_estimate(name):
    """e_m < e_v at 16 spp, e_m <= 0.85 e_v at 64 spp (CPU restatement at 128x72: 0.90 / 0.84 and 0.71 / 0.68), and
    e_m < e_noisy at 4, 16 and 64 spp; the comparison with rt_denoise is printed, not asserted."""
    wl = rt.workloads.get(name, width=256, height=144)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        truth = t.renderFrame(wl.camera, 2048)
        t.setOption(OPT_MOMENTS, 1)
        for spp in (4, 16, 64):
            noisy = t.renderFrame(wl.camera, spp)
            plain = t.denoise(camera=wl.camera)
            vg = t.denoiseVariance()
            mv = t.denoiseMoments()
            e_n, e_p, e_v, e_m = (gamma_rmse(x, truth) for x in (noisy, plain, vg, mv))
            print("%s %d spp gamma RMSE: noisy %.4f, denoise %.4f, denoiseVariance %.4f, denoiseMoments %.4f "
                  "(measured / spatial %.3f, measured / plain %.3f)" % (name, spp, e_n, e_p, e_v, e_m, e_m / e_v, e_m / e_p))
            assert e_m < e_n
            if spp == 16:
                assert e_m < e_v
            if spp == 64:
                assert e_m <= 0.85 * e_v
    finally:
        t.close()


# ---- 9. nothing else moves, and the state machine -----------------------------------------------------------------------

def test_nothing_else_moves(c2):
    wl, t = c2
    t.renderFrame(wl.camera, 4)
    t.render(wl.camera)
    t.renderAgain(wl.camera)
    t.renderFeatures(wl.camera)
    before = (t.transferImage(), read_accum(t), t.featureRecords(), t.moments())
    cnt0 = t.sample_counter
    t.denoiseMomentsOnDevice()
    t.sync()
    out = t.denoisedImage()
    after = (t.transferImage(), read_accum(t), t.featureRecords(), t.moments())
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    assert t.sample_counter == cnt0 == 1
    assert t.denoiseMoments().tobytes() == out.tobytes()
    d = t.deviceMoments()
    assert d and d != t.deviceVariance(0)


def test_compat_path_leaves_valid_moments_untouched():
    wl = rt.workloads.get("c2", width=64, height=40)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        t.setOption(OPT_MOMENTS, 1)
        t.renderFrame(wl.camera, 8)
        m0, a0 = t.moments(), read_accum(t)
        assert (m0 > 0).any()
        t.render(wl.camera)
        for _ in range(20):      # more than one look-ahead batch
            t.renderAgain(wl.camera)
        assert t.lookaheadStats()[0] >= 1
        assert t.moments().tobytes() == m0.tobytes() and read_accum(t).tobytes() == a0.tobytes()
        # and they go on merging afterwards
        t.renderSamples(wl.camera, 8, 8)
        lum = sample_luminances(t, wl.camera, wl.width, wl.height, 16)
        assert_moments(t.moments(), lum, 16, "8 + 8 samples around renderAgain")
    finally:
        t.close()


def test_state_machine_and_error_cases():
    wl = rt.workloads.get("c2", width=64, height=40)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    lib, ctx = t._lib, t._ctx
    try:
        P = A.DenoiseVarianceParams
        ok = P(5, 4.0, 0.5, 0.5, 0.2, A.DENOISE_SPLIT_OBJECTS)
        m = np.empty((wl.height, wl.width), np.float32)
        d = C.c_void_p()

        def state():
            return (lib.rt_read_moments(ctx, m.ctypes.data, m.nbytes), lib.rt_device_moments(ctx, C.byref(d)),
                    lib.rt_denoise_moments(ctx, C.byref(ok)))
        t.renderFrame(wl.camera, 4)
        t.renderFeatures(wl.camera)
        assert state() == (ESTATE,) * 3                   # the option is off
        for bad in (2, -1, 12):
            assert lib.rt_set_option(ctx, OPT_MOMENTS, bad) == EINVAL
        t.setOption(OPT_MOMENTS, 1)
        assert state() == (ESTATE,) * 3                   # on, but no clear yet
        t.renderSamples(wl.camera, 4, 4)                  # (nothing writes the buffer meanwhile)
        assert state() == (ESTATE,) * 3
        t.clear()
        assert state() == (0, 0, 0) and d.value
        assert (m == 0).all()
        t.renderSamples(wl.camera, 0, 4)
        assert state() == (0, 0, 0) and (m > 0).any()
        t.setOption(OPT_MOMENTS, 1)                       # the same value again: nothing changes
        assert state() == (0, 0, 0)
        # every bad parameter rt_denoise_variance refuses
        for it in (0, 9, 100):
            assert lib.rt_denoise_moments(ctx, C.byref(P(it, 4.0, 0.5, 0.5, 0.2, 1))) == EINVAL, it
        for k in range(4):
            for bad in (0.0, -1.0, float("nan"), -np.inf):
                s = [4.0, 0.5, 0.5, 0.2]
                s[k] = bad
                assert lib.rt_denoise_moments(ctx, C.byref(P(5, *s, 1))) == EINVAL, (k, bad)
        assert lib.rt_denoise_moments(ctx, C.byref(P(5, 4.0, 0.5, 0.5, 0.2, 2))) == EINVAL
        assert lib.rt_denoise_moments(ctx, None) == EINVAL
        assert lib.rt_denoise_moments(None, C.byref(ok)) == EINVAL
        assert lib.rt_read_moments(ctx, None, m.nbytes) == EINVAL
        assert lib.rt_read_moments(ctx, m.ctypes.data, m.nbytes - 4) == EINVAL
        assert lib.rt_read_moments(None, m.ctypes.data, m.nbytes) == EINVAL
        assert lib.rt_device_moments(ctx, None) == EINVAL
        # sharded contexts, both ways
        assert lib.rt_set_shard(ctx, 0, 2, 8, 8) == EINVAL
        assert state() == (0, 0, 0)
        t.setOption(OPT_MOMENTS, 0)
        assert state() == (ESTATE,) * 3                   # toggled
        t.setShard(0, 2)
        assert lib.rt_set_option(ctx, OPT_MOMENTS, 1) == EINVAL
        assert lib.rt_set_option(ctx, OPT_MOMENTS, 0) == 0
        t.setShard(0, 1)
        t.setOption(OPT_MOMENTS, 1)
        assert state() == (ESTATE,) * 3                   # toggled back: invalid until the next clear
        t.renderAdaptive(wl.camera, 0.05, batch=4, min_spp=8, max_spp=16)
        assert state() == (0, 0, 0)
        # no features: ESTATE of rt_denoise_variance's own
        t.resize(wl.width + 8, wl.height)
        m = np.empty((wl.height, wl.width + 8), np.float32)
        assert state() == (ESTATE,) * 3                   # after resize
        t.clear()
        assert state() == (0, 0, ESTATE)                  # the moments are back, the features are not
        with pytest.raises(rt.RtError):
            t.denoiseMoments()
        t.renderFrame(wl.camera, 4)
        assert t.denoiseMoments(camera=wl.camera).shape == (wl.height, wl.width + 8, 4)
        assert t.sampleVariance().shape == (wl.height, wl.width + 8)
    finally:
        t.close()


def test_sample_variance_is_m2_over_n_n_minus_1():
    wl = rt.workloads.get("c2", width=32, height=20)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        t.setOption(OPT_MOMENTS, 1)
        t.renderFrame(wl.camera, 1)
        assert (t.sampleVariance() == 0).all()
        t.renderFrame(wl.camera, 5)
        assert np.array_equal(t.sampleVariance(), (t.moments().astype(np.float64) / 20.0).astype(np.float32))
    finally:
        t.close()


# ---- 10. the CLI against the Python path --------------------------------------------------------------------------------

def test_cli_measured_matches_python_path(built, tmp_path):
    w, h, spp = 200, 120, 8
    scene = "c2_cornell.scene"
    raw = str(tmp_path / "f.f32")
    aov = str(tmp_path / "aov")
    cmd = [CLI, "--scene", os.path.join(ASSETS, "scenes", scene), "--size", "%dx%d" % (w, h), "--spp", str(spp),
           "--camera=-8,-1,-8,45,0", "--raw", raw, "--denoise", "--variance-guided", "--measured", "--aov", aov]
    subprocess.run(cmd, check=True, cwd=ROOT)
    got = np.fromfile(raw, np.float32).reshape(h, w, 4)
    s = rt.SceneCreator()
    s.loadScene(os.path.join(ASSETS, "scenes", scene), base_dir=ASSETS)
    t = rt.RayTracer(w, h, scene=s)
    try:
        cam = rt.Camera(60, np.float32(w) / np.float32(h), (-8, -1, -8), 45.0, 0.0)
        t.setOption(OPT_MOMENTS, 1)
        t.renderFrame(cam, spp)
        exp = t.denoiseMoments(camera=cam)
        v0 = t.variance(0)
        sv = t.sampleVariance()
        spatial = t.denoiseVariance()
    finally:
        t.close()
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert not np.array_equal(got.view(np.uint32), spatial.view(np.uint32))
    head = b"Pf\n%d %d\n-1.0\n" % (w, h)
    for name, ref in (("_samplevar.pfm", sv), ("_variance.pfm", v0)):
        pfm = open(aov + name, "rb").read()
        assert pfm.startswith(head)
        data = np.frombuffer(pfm[len(head):], np.float32)
        assert np.array_equal(data.view(np.uint32), ref.reshape(-1).view(np.uint32)), name
    assert (sv > 0).any()
