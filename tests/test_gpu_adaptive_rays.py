"""GPU (-m gpu): adaptive sampling for caller-supplied rays and ray sets (rt_render_adaptive_rays, rt_render_adaptive_variance_rays).
Every pixel of such a frame must hold, bit for bit, what the fixed sequence rt_clear; rt_render_rays / rt_render_ray_sets(k batch,
c_k) for k = 0 .. holds after as many rounds as the pixel got — the first time the four ray kernel families run under a block
mask — and the stopping decisions must follow the header's estimators, rebuilt on the host.  The rays' direction bits come from
the library itself (test_gpu_ray_sets.primary_batch), so the camera calls are available as twins: a camera's own primary rays
must give rt_render_adaptive's frame, sets of max_spp camera blocks rt_render_adaptive_cameras'.

Frame 52 x 27: neither side is a multiple of the 8 x 8 block and 52 is no multiple of a wave's pixels, so waves straddle block
edges and row ends.  batch 8, min_spp 16, max_spp 44: the last round is a partial one of 4.  Sets of 5 distinct records: 5 does
not divide 8, so a wrong cyclic offset changes bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_variance_ref as AV
import cases
import denoise_vg_ref as V
import moments_ref as M
import test_gpu_adaptive_cameras as AC
import test_gpu_ray_sets as RS

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
R = rt.raytracer
T = rt.RayTracer
rays_mod = rt.rays
EINVAL, ESTATE = -1, -4
FIXED, QUEUE = A.CAMERA_PLAN_FIXED, A.CAMERA_PLAN_QUEUE

W, H = 52, 27
BATCH, MIN_SPP, MAX_SPP = 8, 16, 44
K = 5
BLOCK = (8, 8)
KW = dict(batch=BATCH, min_spp=MIN_SPP, max_spp=MAX_SPP, block=BLOCK)
CAMERA = rt.Camera(60, np.float32(W) / np.float32(H), (-8, -1, -8), 45.0, 0.0)
ROUNDS = AC.rounds_of(MAX_SPP, BATCH)

SCENES = RS.SCENES       # workload arguments → the (ACCEL, GEOM) row of the queue: all five rows run masked
CASES = [(name, p) for name in sorted(SCENES) for p in ((0, 1, 2) if name in ("c2", "all_kinds") else (0, 2))]
case_id = lambda c: "%s-a%d" % c
MODES = {   # options on top of the defaults → the family the rounds must run
    "queue": (dict(OPT_WAVE_FILL=1), QUEUE),
    "queue-fill0": (dict(OPT_WAVE_FILL=0), QUEUE),      # a wave owns several rays: masks cut through them
    "fixed": (dict(OPT_SAMPLE_QUEUE=0), FIXED),
}
DEFAULTS = dict(OPT_WAVE_FILL=1, OPT_SAMPLE_QUEUE=1, OPT_MAX_THREADS_PER_LAUNCH=1 << 30, OPT_MOMENTS=0, OPT_PREFIX_SHARING=1)

read_accum, same_bits = RS.read_accum, RS.same_bits


def blocks_for(n):
    return RS.blocks_for(n, W, H, CAMERA)


class Frame:
    """One (scene, policy): the camera's primary rays and sets of K records per ray (blocks_for(K)'s primary rays), on the
    host and on the device, with the policy's own direction bits; the fixed sequence of each kind, computed once under the
    default options and never written again."""

    def __init__(self, t):
        self.blocks = blocks_for(K)
        self.batch = RS.primary_batch(t, CAMERA.transferData())
        self.sets = RS.block_sets(t, self.blocks)
        assert len({self.sets[:, j].tobytes() for j in range(K)}) == K
        self.d = {"rays": RS.to_device(self.batch), "sets": RS.to_device(self.sets)}
        self.refs = {}

    def size(self, kind):
        return 0 if kind == "rays" else K

    def fixed_round(self, t, kind, first, c):
        if kind == "rays":
            t.renderRays(self.d[kind], first, c)
        else:
            t.renderRaySets(self.d[kind], K, first, c)

    def camera_of(self, kind, j):
        """the camera block whose primary rays sample j of every pixel starts along"""
        return CAMERA.transferData() if kind == "rays" else self.blocks[j % K]

    def ref(self, t, kind):
        if kind not in self.refs:
            sums = []
            for first, c in ROUNDS:
                t.clear()
                self.fixed_round(t, kind, first, c)
                sums.append(read_accum(t))
            self.refs[kind] = AC.cumulative(sums)
        return self.refs[kind]

    def lum(self, t, kind):
        """(H, W, MAX_SPP) float64: every sample's luminance, for the variance rule's host restatement"""
        if ("lum", kind) not in self.refs:
            ys, xs = np.mgrid[0:H, 0:W]
            xs, ys = xs.reshape(-1), ys.reshape(-1)
            lum = np.empty((H, W, MAX_SPP))
            for j in range(MAX_SPP):
                s = t.traceSamples(self.camera_of(kind, j), xs, ys, np.full(len(xs), j))
                lum[..., j] = (s.astype(np.float64) @ AV.LUM).reshape(H, W)
            lum.setflags(write=False)
            self.refs["lum", kind] = lum
        return self.refs["lum", kind]


_tracers, _frames = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_tracers():
    yield
    _frames.clear()
    for t in _tracers.values():
        t.close()
    _tracers.clear()


def configured(case, kind, mode="queue"):
    """The scene's tracer under (policy, mode), the frame of (scene, policy), its fixed sequence of `kind`, the family and
    the queue row the rounds must run."""
    name, policy = case
    if name not in _tracers:
        kw, _ = SCENES[name]
        wl = rt.workloads.get(name, width=W, height=H, **kw)
        _tracers[name] = T(W, H, scene=wl.scene, seed=cases.SEED)
    t = _tracers[name]
    for k, v in DEFAULTS.items():
        t.setOption(getattr(T, k), v)
    t.setArith(policy)
    if case not in _frames:
        _frames[case] = Frame(t)
    fr = _frames[case]
    ref = fr.ref(t, kind)
    options, family = MODES[mode]
    for k, v in options.items():
        t.setOption(getattr(T, k), v)
    return t, fr, ref, family, SCENES[name][1]


def adaptive(t, fr, kind, thr, variance=False, **kw):
    f = t.renderAdaptiveVarianceRays if variance else t.renderAdaptiveRays
    return f(fr.d[kind], thr, set_size=fr.size(kind), **dict(KW, **kw))


def frame_state(t, variance=False):
    t.sync()
    return [read_accum(t), t.sampleCounts(), t.blockError(), t.transferImage()] + ([t.pixelError()] if variance else [])


def pick_threshold(accs, halves):
    """The median of the host's positive block errors after round 2: stops some blocks early, keeps others running."""
    e = A.block_error_reference(accs[2], halves[2], *BLOCK)
    assert (e > 0).any()
    return float(np.median(e[e > 0]))


# ---- 1. threshold 0 is the fixed sequence -------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rays", "sets"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_threshold_zero_is_the_fixed_sequence(case, kind):
    t, fr, (accs, _), family, row = configured(case, kind)
    t.clear()
    for first, c in ROUNDS:
        fr.fixed_round(t, kind, first, c)
    fixed = read_accum(t)
    assert same_bits(fixed, accs[-1]) and fixed[..., :3].any()      # the per-round sums compose exactly
    t.resolve()
    fixed_img = t.transferImage()
    st = adaptive(t, fr, kind, 0.0)
    got = read_accum(t)
    facts, plan = t.lastRayPlan()
    assert (plan["family"], plan["accel"], plan["geom"]) == (family,) + row
    assert plan == R.plan_camera_samples(**facts) and facts["n"] == W * H and facts["count"] == MAX_SPP % BATCH
    assert same_bits(got, fixed)
    assert same_bits(t.transferImage(), fixed_img)
    assert st == dict(rounds=len(ROUNDS), pixel_samples=W * H * MAX_SPP, blocks=7 * 4, blocks_at_max=7 * 4)
    assert (t.sampleCounts() == MAX_SPP).all()
    assert t.walkOverflow() == 0


# ---- 2. truncation identity and estimator -------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("kind", ["rays", "sets"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_truncation_identity_and_estimator(case, kind, mode):
    t, fr, (accs, halves), family, row = configured(case, kind, mode)
    thr = pick_threshold(accs, halves)
    st = adaptive(t, fr, kind, thr)
    _, plan = t.lastRayPlan()
    assert plan["family"] == family and (family == FIXED or (plan["accel"], plan["geom"]) == row)
    AC.check_truncated_frame(t, st, thr, accs, halves, BATCH, MIN_SPP, MAX_SPP)
    assert t.walkOverflow() == 0


def check_variance_frame(t, run, thr, accs, lum, what):
    """The variance rule's frame `run(threshold, max_spp)` renders: truncation identity, estimator against the device's own
    state with test_gpu_adaptive_variance's tolerances, decisions."""
    st = run(thr, MAX_SPP)
    got, counts = read_accum(t), t.sampleCounts()
    assert np.array_equal(counts, got[..., 3].astype(np.uint32))
    assert st["pixel_samples"] == int(counts.astype(np.int64).sum())
    blocks = AC.block_of_pixels(counts, *BLOCK)
    bc = blocks.max(-1)
    assert ((blocks == bc[..., None]) | (blocks < 0)).all()
    assert (bc >= MIN_SPP).all() and (bc <= MAX_SPP).all() and ((bc % BATCH == 0) | (bc == MAX_SPP)).all()
    assert st["rounds"] == -(-int(bc.max()) // BATCH) and st["blocks"] == bc.size
    assert len(np.unique(bc)) > 1
    rnd = -(-counts.astype(np.int64) // BATCH) - 1
    expect = np.take_along_axis(np.stack(accs), rnd[None, ..., None].repeat(4, -1), 0)[0]
    assert same_bits(got, expect)
    # the estimator: pixel errors within 4 ulp of the binary32 formula on the device's own state, block errors their means,
    # the moments within moments_ref.tolerance of the two-pass truth
    perr, err, m2 = t.pixelError(), t.blockError(), t.moments()
    f32 = AV.pixel_error_f32(got, m2)
    ulps = np.abs(perr.astype(np.float64) - f32.astype(np.float64)) / np.spacing(np.abs(f32)).astype(np.float64)
    use = np.arange(MAX_SPP)[None, None, :] < counts[..., None]
    mean = np.where(use, lum, 0.0).sum(-1) / counts
    truth = np.where(use, (lum - mean[..., None]) ** 2, 0.0).sum(-1)
    tol = M.tolerance(truth, counts, np.where(use, lum, 0.0).max(-1))
    dev = np.abs(m2.astype(np.float64) - truth)
    print("%s: threshold %.6g, counts %s, pixel error within %.3g ulp, max |M2 - truth| %.3g (max excess over the tolerance %.3g)"
          % (what, thr, np.unique(bc).tolist(), ulps.max(), dev.max(), (dev - tol).max()))
    assert (ulps <= 4).all() and ((perr == 0) == (f32 == 0)).all() and (perr >= 0).all()
    np.testing.assert_allclose(err, AV.block_error(perr, *BLOCK), rtol=1e-5, atol=0)
    assert (dev <= tol).all() and (m2 >= 0).all()
    # decisions: a block that stopped below max_spp had converged; a block still running after round k had not
    last = -(-bc // BATCH) - 1
    thr32 = np.float32(thr)
    assert (err[bc < MAX_SPP] < thr32).all()
    assert st["blocks_at_max"] == int(((bc == MAX_SPP) & ~(err < thr32)).sum())
    pairs = 0
    for k in range(MIN_SPP // BATCH - 1, int(last.max())):
        running = last > k
        if not running.any():
            continue
        cut = run(thr, (k + 1) * BATCH)
        assert cut["rounds"] == k + 1
        e = t.blockError()[running]
        near = np.abs(e.astype(np.float64) - thr) <= 1e-4 * thr
        assert (e[~near] >= thr32).all(), k
        pairs += e.size
    assert pairs > 0


@pytest.mark.parametrize("case,kind", [(c, "sets") for c in CASES] + [(("c2", 2), "rays")], ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_variance_truncation_estimator_and_decisions(case, kind):
    t, fr, (accs, _), _, _ = configured(case, kind)
    lum = fr.lum(t, kind)
    errs = AV.block_errors_per_round(accs, lum, BATCH, MAX_SPP, *BLOCK)
    thr = float(np.float32(AV.middle_threshold(errs[2])))
    t.setOption(T.OPT_MOMENTS, 1)
    run = lambda th, max_spp: adaptive(t, fr, kind, th, variance=True, max_spp=max_spp)
    check_variance_frame(t, run, thr, accs, lum, "%s %s" % (case_id(case), kind))
    _, plan = t.lastRayPlan()
    assert plan["family"] == FIXED and plan["moments"] == 1      # the known price: moments run the fixed-lane kernels
    assert t.walkOverflow() == 0


# ---- 3. equalities with the camera calls --------------------------------------------------------------------------------

def assert_twins(got, got_st, want, want_st):
    names = ("accumulator", "counts", "block errors", "image", "pixel errors")
    assert len(np.unique(want[1])) > 1, "the threshold stops some blocks early"
    differ = [n for n, g, w in zip(names, got, want) if not same_bits(g, w)]
    assert not differ and got_st == want_st, (differ, got_st, want_st)


@pytest.mark.parametrize("policy", [0, 2])
def test_camera_twins(policy):
    t, fr, (accs, halves), _, _ = configured(("c2", policy), "rays")
    thr = pick_threshold(accs, halves)
    cam = CAMERA.transferData()
    blocks = blocks_for(MAX_SPP)
    d44 = RS.to_device(RS.block_sets(t, blocks))          # set_size == max_spp: block j is the camera of sample j
    cams_kw = dict(batch=BATCH, min_spp=MIN_SPP, block=BLOCK)
    # the Dammertz rule: a camera's own primary rays / sets of max_spp camera blocks
    want_st, want = t.renderAdaptive(cam, thr, **KW), frame_state(t)
    t.clear()
    got_st, got = adaptive(t, fr, "rays", thr), frame_state(t)
    assert_twins(got, got_st, want, want_st)
    want_st, want = t.renderAdaptiveCameras(blocks, thr, **cams_kw), frame_state(t)
    t.clear()
    got_st, got = t.renderAdaptiveRays(d44, thr, set_size=MAX_SPP, **KW), frame_state(t)
    assert_twins(got, got_st, want, want_st)
    # the variance rule, pixel errors compared as bits; the threshold: the middle of the block errors after round 2.
    # A ray launch that keeps moments runs the fixed-lane kernels (plan_camera_samples), whose M2 is Welford's merge over the
    # lanes; rt_render_adaptive_variance with prefix sharing on runs the queue kernel, whose M2 is a two-pass sum over its
    # LDS slots — the same quantity in another rounding (moments_ref.tolerance).  Its bit-for-bit twin is the fixed-lane
    # family on both sides: prefix sharing off, which changes no bit of an accumulator.
    t.setOption(T.OPT_MOMENTS, 1)
    t.setOption(T.OPT_PREFIX_SHARING, 0)
    t.renderAdaptiveVariance(cam, 0.0, batch=BATCH, min_spp=MIN_SPP, max_spp=3 * BATCH, block=BLOCK)
    vthr = float(np.float32(AV.middle_threshold(t.blockError())))
    want_st, want = t.renderAdaptiveVariance(cam, vthr, **KW), frame_state(t, True)
    t.clear()
    got_st, got = adaptive(t, fr, "rays", vthr, variance=True), frame_state(t, True)
    assert_twins(got, got_st, want, want_st)
    want_st, want = t.renderAdaptiveVarianceCameras(blocks, vthr, **cams_kw), frame_state(t, True)
    t.clear()
    got_st, got = t.renderAdaptiveVarianceRays(d44, vthr, set_size=MAX_SPP, **KW), frame_state(t, True)
    assert_twins(got, got_st, want, want_st)
    t.setOption(T.OPT_PREFIX_SHARING, 1)


# ---- 4. masked rays do no work ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rays", "sets"])
def test_masked_rays_do_no_work(kind):
    t, fr, (accs, halves), _, _ = configured(("c2", 2), kind)
    thr = pick_threshold(accs, halves)
    t.enableCounters(True)
    try:
        t.resetCounters()
        st = adaptive(t, fr, kind, thr)
        n = int(t.counters().samples)
        _, plan = t.lastRayPlan()
    finally:
        t.enableCounters(False)
    counts = t.sampleCounts()
    assert plan["family"] == FIXED and plan["count"] == 1          # the counting fixed-lane kernel
    assert n == st["pixel_samples"] == int(counts.astype(np.int64).sum())
    assert n < W * H * MAX_SPP and (counts < MAX_SPP).any()


# ---- 5. moments ---------------------------------------------------------------------------------------------------------

def test_moments_follow_the_sample_luminances():
    kind = "sets"
    t, fr, (accs, halves), _, _ = configured(("c2", 2), kind)
    thr = pick_threshold(accs, halves)
    st0 = adaptive(t, fr, kind, thr)
    plain = read_accum(t), t.transferImage(), t.sampleCounts()
    assert t.lastRayPlan()[1]["moments"] == 0
    t.setOption(T.OPT_MOMENTS, 1)
    st1 = adaptive(t, fr, kind, thr)
    kept = read_accum(t), t.transferImage(), t.sampleCounts()
    m2 = t.moments()
    _, plan = t.lastRayPlan()
    assert plan["family"] == FIXED and plan["moments"] == 1
    assert st0 == st1 and all(a.tobytes() == b.tobytes() for a, b in zip(plain, kept))
    counts = kept[2]
    assert len(np.unique(counts)) > 1 and (m2 >= 0).all()
    # the float64 two-pass M2 of the luminances of the samples each pixel holds, on a seeded subset of the pixels
    rng = np.random.RandomState(23)
    xs, ys = rng.randint(0, W, 200), rng.randint(0, H, 200)
    n = counts[ys, xs].astype(np.int64)
    lum = np.stack([t.traceSamples(fr.camera_of(kind, j), xs, ys, np.full(len(xs), j)).astype(np.float64) @ V.LUM
                    for j in range(int(n.max()))], axis=1)
    use = np.arange(lum.shape[1])[None, :] < n[:, None]
    mean = np.where(use, lum, 0.0).sum(-1) / n
    ref = np.where(use, (lum - mean[:, None]) ** 2, 0.0).sum(-1)
    tol = M.tolerance(ref, n, np.where(use, lum, 0.0).max(-1))
    err = np.abs(m2[ys, xs].astype(np.float64) - ref)
    print("max |M2 - truth| %.3g (tolerance there %.3g), max M2 %.4g, counts %s" % (err.max(), tol[err.argmax()], ref.max(), np.unique(n)))
    assert (err <= tol).all() and ref.max() > 0 and len(np.unique(n)) > 1
    # the variance form leaves valid moments: the measured-variance filter runs directly after it, on the rays' own guides
    adaptive(t, fr, kind, 0.05, variance=True)
    t.renderFeaturesRays(fr.d["rays"])
    dn = t.denoiseMoments()
    assert dn.shape == (H, W, 4) and np.isfinite(dn).all() and dn[..., :3].any()


# ---- 6. split launches --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rays", "sets"])
def test_split_launches_change_no_bit(kind):
    t, fr, (accs, halves), _, _ = configured(("c2", 2), kind)
    thr = pick_threshold(accs, halves)
    st, whole = adaptive(t, fr, kind, thr), frame_state(t)
    t.setOption(T.OPT_MAX_THREADS_PER_LAUNCH, 4096)
    st_split, split = adaptive(t, fr, kind, thr), frame_state(t)
    facts, _ = t.lastRayPlan()
    assert facts["n"] < W * H            # several slot ranges per round
    assert len(np.unique(whole[1])) > 1 and st == st_split
    assert all(same_bits(a, b) for a, b in zip(whole, split))


# ---- 7. errors and state ------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_untouched():
    wl = rt.workloads.get("c1", width=W, height=H)
    t = T(W, H, scene=wl.scene, seed=cases.SEED)
    try:
        with pytest.raises(rt.RtError) as ei:
            t.blockError()                            # no adaptive frame yet
        assert ei.value.code == ESTATE
        batch = RS.primary_batch(t, CAMERA.transferData())
        d = RS.to_device(batch)
        d5 = RS.to_device(np.repeat(batch.reshape(-1, 1), K, axis=1))
        t.renderFrame(wl.camera, 8)
        before, before_img = read_accum(t), t.transferImage()
        lib, ctx = t._lib, t._ctx
        n = W * H
        p = A.AdaptiveParams(BATCH, MIN_SPP, MAX_SPP, 0.1, 8, 8)
        st = A.AdaptiveStats()
        ptr, ptr5 = C.c_void_p(d.data_ptr()), C.c_void_p(d5.data_ptr())
        call = lambda f, *a: f(ctx, *a, C.byref(p), C.byref(st))
        for f in (lib.rt_render_adaptive_rays, lib.rt_render_adaptive_variance_rays):
            assert f(None, ptr, n, 0, C.byref(p), C.byref(st)) == EINVAL
        f = lib.rt_render_adaptive_rays
        assert f(ctx, ptr, n, 0, None, C.byref(st)) == EINVAL and f(ctx, ptr, n, 0, C.byref(p), None) == EINVAL
        for bad_n in (0, n - 1, n + 1, W * (H - 1)):                         # one ray per pixel
            assert call(f, ptr, bad_n, 0) == EINVAL, bad_n
        assert call(f, C.c_void_p(d.data_ptr() + 8), n, 0) == EINVAL          # misaligned d_rays
        assert call(f, ptr5, n, A.RAY_SET_MAX + 1) == EINVAL                  # set_size above the maximum
        assert call(f, None, n, 0) == EINVAL                                  # nothing uploaded
        t.uploadRays(batch)
        assert call(f, None, n, K) == EINVAL                                  # n records uploaded, n x 5 asked for
        assert call(lib.rt_render_adaptive_variance_rays, ptr, n, 0) == ESTATE    # the variance form with moments off
        bad = [dict(batch=0), dict(batch=513), dict(min_spp=8), dict(min_spp=20), dict(max_spp=15), dict(block=(6, 8)),
               dict(block=(8, 0)), dict(block=(512, 8))]
        for b in bad:                                                         # check_adaptive's refusals
            with pytest.raises(rt.RtError) as ei:
                t.renderAdaptiveRays(d, 0.1, **dict(KW, **b))
            assert ei.value.code == EINVAL, b
        for thr in (-1.0, float("nan"), float("inf")):
            with pytest.raises(rt.RtError) as ei:
                t.renderAdaptiveRays(d, thr, **KW)
            assert ei.value.code == EINVAL, thr
        t.setShard(0, 2, 8, 8)
        for size, dd in ((0, d), (K, d5)):
            with pytest.raises(rt.RtError) as ei:
                t.renderAdaptiveRays(dd, 0.1, set_size=size, **KW)
            assert ei.value.code == EINVAL
        t.setShard(0, 1, 8, 8)
        with pytest.raises(ValueError):
            t.renderAdaptiveRays(d[:-1], 0.1, **KW)                           # the Python checks, before any library call
        with pytest.raises(ValueError):
            t.renderAdaptiveRays(d, 0.1, set_size=K, **KW)
        assert same_bits(read_accum(t), before) and same_bits(t.transferImage(), before_img)
        with pytest.raises(rt.RtError) as ei:
            t.blockError()                            # still none
        assert ei.value.code == ESTATE
        raw = C.c_void_p()
        assert lib.rt_create(0, W, H, C.byref(raw)) == 0
        assert f(raw, ptr, n, 0, C.byref(p), C.byref(st)) == ESTATE           # no scene
        lib.rt_destroy(raw)

        # a good call after the bad ones — the uploaded records (None), then a numpy batch; blockError and pixelError follow
        # the header's validity rules
        st = t.renderAdaptiveRays(None, 0.1, **KW)
        first = read_accum(t)
        assert st["blocks"] == 7 * 4 and t.blockError().shape == (4, 7)
        with pytest.raises(rt.RtError) as ei:
            t.pixelError()                            # the last adaptive call was not a variance one
        assert ei.value.code == ESTATE
        assert t.renderAdaptiveRays(batch, 0.1, **KW) == st and same_bits(read_accum(t), first)
        assert t.deviceRays()[1] == n                 # the uploaded rays stay as they are
        t.setOption(T.OPT_MOMENTS, 1)
        t.renderAdaptiveVarianceRays(d5, 0.1, set_size=K, **KW)
        assert t.pixelError().shape == (H, W)
        t.renderAdaptiveRays(d, 0.1, **KW)
        with pytest.raises(rt.RtError) as ei:
            t.pixelError()                            # a later Dammertz call invalidates them
        assert ei.value.code == ESTATE
        t.resize(40, 30)
        with pytest.raises(rt.RtError) as ei:
            t.blockError()
        assert ei.value.code == ESTATE
    finally:
        t.close()


def test_a_kept_prefix_survives_and_the_last_plan_is_the_last_rounds():
    wl = rt.workloads.get("c2", width=W, height=H)
    t = T(W, H, scene=wl.scene, seed=cases.SEED)
    try:
        d = RS.to_device(RS.primary_batch(t, CAMERA.transferData()))
        counter = C.c_uint32()
        t._check(t._lib.rt_sample_counter(t._ctx, C.byref(counter)))
        before = counter.value
        t.clear()
        t.renderSamples(wl.camera, 0, 16)
        st = t.renderAdaptiveRays(d, 0.0, batch=16, min_spp=32, max_spp=40, block=BLOCK)
        facts, plan = t.lastRayPlan()
        t.renderSamples(wl.camera, 16, 16)
        t.sync()
        assert t.prefixCacheStats() == (1, 1)      # the second fused call reused the prefix the rounds left alone
        assert st["rounds"] == 3 and facts["count"] == 8 and plan["family"] == QUEUE
        t._check(t._lib.rt_sample_counter(t._ctx, C.byref(counter)))
        assert counter.value == before             # the sample counter stays as it is
    finally:
        t.close()


# ---- 8. rt_cli ----------------------------------------------------------------------------------------------------------

def test_cli_adaptive_projection_matches_the_python_path(built, tmp_path):
    w, h, spp, k, thr = 64, 40, 40, 4, 0.0625
    scene = os.path.join(cases.ROOT, "assets", "scenes", "c2_cornell.scene")
    raw, cnt, raw_v = str(tmp_path / "f.f32"), str(tmp_path / "c.u32"), str(tmp_path / "v.f32")
    cli = os.path.join(cases.ROOT, "host", "rt_cli")
    base = [cli, "--scene", scene, "--size", "%dx%d" % (w, h), "--camera=-8,-1,-8,45,0", "--projection", "ortho", "--extent", "12",
            "--ray-sets", str(k), "--adaptive", repr(thr), "--batch", "8", "--min-spp", "16", "--spp", str(spp)]
    out = subprocess.run(base + ["--counts", cnt, "--raw", raw], check=True, cwd=cases.ROOT, capture_output=True, text=True,
                         timeout=120).stdout
    assert "adaptive caller-supplied ray sets" in out
    out = subprocess.run(base + ["--adaptive-rule", "variance", "--denoise", "--variance-guided", "--measured", "--raw", raw_v,
                                 "--aov", str(tmp_path / "aov")], check=True, cwd=cases.ROOT, capture_output=True, text=True,
                         timeout=120).stdout
    assert "(variance rule)" in out and "measured" in out
    got_v = np.fromfile(raw_v, np.float32).reshape(h, w, 4)
    assert np.isfinite(got_v).all() and got_v[..., :3].any() and os.path.getsize(str(tmp_path / "aov_error.pfm")) > w * h * 4
    got = np.fromfile(raw, np.float32).reshape(h, w, 4)
    got_counts = np.fromfile(cnt, np.uint32).reshape(h, w)
    s = rt.SceneCreator()
    s.loadScene(scene, base_dir=os.path.join(cases.ROOT, "assets"))
    t = T(w, h, scene=s)
    try:
        kw = dict(pos=(-8, -1, -8), w=w, h=h, extent=12.0, yaw=45.0, pitch=0.0)
        sets = rays_mod.ray_sets(rays_mod.orthographic_rays, rt.Camera.sampleOffsets(k), **kw)
        t.renderAdaptiveRays(sets, thr, set_size=k, batch=8, min_spp=16, max_spp=spp)
        exp, exp_counts = t.transferImage(), t.sampleCounts()
    finally:
        t.close()
    print("pixels equal to the Python path's: %.4f, counts equal: %.4f" %
          ((got.view(np.uint32) == exp.view(np.uint32)).all(-1).mean(), (got_counts == exp_counts).mean()))
    assert same_bits(got, exp)
    assert np.array_equal(got_counts, exp_counts) and got_counts.min() >= 16 and got_counts.max() <= spp
    # the other refusals of a projection frame stay
    assert subprocess.run(base + ["--aa"], cwd=cases.ROOT, capture_output=True).returncode == 2
    assert subprocess.run(base + ["--progressive"], cwd=cases.ROOT, capture_output=True).returncode == 2
