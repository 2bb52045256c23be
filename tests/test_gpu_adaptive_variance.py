"""GPU (-m gpu): adaptive sampling under the variance-driven stopping rule (rt_render_adaptive_variance and its cameras
form).  Every pixel of such a frame must hold, bit for bit, what the fixed sequence holds after as many rounds as the pixel
got; the pixel and block errors must be the header's estimator applied to the device's own accumulator and moments; the
moments must be the two-pass truth of exactly the samples held; and every stopping decision must follow the block error
the device itself reports — checked round by round by running the frame again, cut off after that round.

The thresholds come from the host restatement (tests/adaptive_variance_ref.py) applied to the fixed sequence's sums and the
float64 two-pass moments of traceSamples' luminances, as midpoints between two neighbouring block errors."""
import ctypes as C

import numpy as np
import pytest

import adaptive_variance_ref as AV
import cases
import moments_ref as M

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
T = rt.RayTracer
EINVAL, ESTATE = -1, -4

BATCH, MIN_SPP, MAX_SPP = 16, 32, 104      # 104 = 6 x 16 + 8: the last round is a partial one
BLOCK = (8, 8)
KW = dict(batch=BATCH, min_spp=MIN_SPP, max_spp=MAX_SPP, block=BLOCK)

SCENES = {
    # frame sizes that are not multiples of the block: edge blocks hold fewer pixels
    "c1": lambda: rt.workloads.get("c1", width=64, height=64),
    "c2": lambda: rt.workloads.get("c2", width=244, height=138),
    "c3": lambda: rt.workloads.get("c3", width=100, height=65),
    "glass": lambda: rt.workloads.get("c5", width=66, height=50),
}
# (scene, arithmetic policy, prefix sharing): both policies everywhere, prefix sharing off on C2
CASES = [(s, a, 1) for s in sorted(SCENES) for a in (rt.ARITH_IEEE, rt.ARITH_ROCM_OCL)] + \
        [("c2", rt.ARITH_IEEE, 0), ("c2", rt.ARITH_ROCM_OCL, 0)]
case_id = lambda c: "%s-arith%d-share%d" % c


def read_accum(t):
    import torch
    t.sync()
    return torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().copy()


def rounds_of(max_spp, batch):
    return [(k * batch, min(batch, max_spp - k * batch)) for k in range(-(-max_spp // batch))]


def block_of_pixels(counts, bw, bh):
    h, w = counts.shape
    by, bx = -(-h // bh), -(-w // bw)
    pad = np.full((by * bh, bx * bw), -1, dtype=np.int64)
    pad[:h, :w] = counts
    return pad.reshape(by, bh, bx, bw).transpose(0, 2, 1, 3).reshape(by, bx, bh * bw)


class Reference:
    """The fixed sequence of one (scene, policy, camera blocks), computed once and never written again: the accumulator
    after every round, the resolved image after the last, every sample's luminance, and the host's block errors."""

    def __init__(self, t, blocks, cameras):
        w, h = t.width, t.height
        n = len(blocks)
        self.accs = []
        t.setOption(T.OPT_MOMENTS, 0)
        t.clear()
        for first, c in rounds_of(n, BATCH):
            if cameras:
                t.renderSamplesCameras(blocks[first:first + c], first)
            else:
                t.renderSamples(blocks[0], first, c)
            self.accs.append(read_accum(t))
        t.resolve()
        self.image = t.transferImage()
        ys, xs = np.mgrid[0:h, 0:w]
        xs, ys = xs.reshape(-1), ys.reshape(-1)
        lum = np.empty((h, w, n))
        for j in range(n):
            s = t.traceSamples(blocks[j], xs, ys, np.full(len(xs), j))
            lum[..., j] = (s.astype(np.float64) @ AV.LUM).reshape(h, w)
        self.lum = lum
        self.errs = AV.block_errors_per_round(self.accs, lum, BATCH, n, *BLOCK)
        # float32 values, so that the device compares with exactly the number the test compares with
        self.thr_middle = float(np.float32(AV.middle_threshold(self.errs[3])))
        self.thr_p10 = float(np.float32(AV.percentile_threshold(self.errs[-1], 10)))
        for a in self.accs + [self.image, self.lum] + self.errs:
            a.setflags(write=False)


_tracers, _refs = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_tracers():
    yield
    for _, t in _tracers.values():
        t.close()
    _tracers.clear()
    _refs.clear()


def configured(case):
    """The scene's tracer under (policy, sharing) with the moments ON, and the reference of (scene, policy)."""
    name, arith, sharing = case
    if name not in _tracers:
        wl = SCENES[name]()
        _tracers[name] = (wl, T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED))
    wl, t = _tracers[name]
    t.setArith(arith)
    t.setOption(T.OPT_PREFIX_SHARING, 1)
    if (name, arith) not in _refs:      # (the sums do not depend on prefix sharing, bit for bit: tests/test_gpu_parity.py)
        same = np.tile(np.asarray(wl.camera, np.float32), (MAX_SPP, 1))
        _refs[name, arith] = Reference(t, same, cameras=False)
    t.setOption(T.OPT_PREFIX_SHARING, sharing)
    t.setOption(T.OPT_MOMENTS, 1)
    return wl, t, _refs[name, arith]


def truth_and_tolerance(lum, counts):
    """Per pixel: the two-pass M2 of its first counts[p] samples and the project's tolerance for it (moments_ref)."""
    h, w, nmax = lum.shape
    counts = np.broadcast_to(np.asarray(counts), (h, w))
    use = np.arange(nmax)[None, None, :] < counts[..., None]
    mean = np.where(use, lum, 0.0).sum(-1) / np.maximum(counts, 1)
    m2 = np.where(use, (lum - mean[..., None]) ** 2, 0.0).sum(-1)
    lmax = np.where(use, lum, 0.0).max(-1)
    return m2, M.tolerance(m2, counts, lmax)


def check_estimator(t, got, counts, lum, what):
    """3: the errors against the device's own state, the moments against the two-pass truth → (block errors, pixel errors)."""
    perr, err, m2 = t.pixelError(), t.blockError(), t.moments()
    f32 = AV.pixel_error_f32(got, m2)
    ulps = np.abs(perr.astype(np.float64) - f32.astype(np.float64)) / np.spacing(np.abs(f32)).astype(np.float64)
    mean = AV.block_error(perr, *BLOCK)
    ref, tol = truth_and_tolerance(lum, counts)
    dev = np.abs(m2.astype(np.float64) - ref)
    print("%s: pixel error max %.4g, within %.3g ulp of the binary32 formula; block error / mean of pixel errors - 1: %.3g; "
          "max |M2 - truth| %.3g (max excess over the tolerance %.3g)" %
          (what, perr.max(), ulps.max(), np.abs(err / np.where(mean > 0, mean, 1.0) - (mean > 0)).max(), dev.max(),
           (dev - tol).max()))
    assert (ulps <= 4).all()
    assert ((perr == 0) == (f32 == 0)).all() and (perr >= 0).all()
    np.testing.assert_allclose(err, mean, rtol=1e-5, atol=0)
    assert (dev <= tol).all() and (m2 >= 0).all()
    return err, perr


def check_frame(t, run, thr, ref, max_spp=MAX_SPP, what=""):
    """2 to 4 for the frame `run(threshold, max_spp)` renders: truncation identity, estimator, decisions."""
    st = run(thr, max_spp)
    got, counts = read_accum(t), t.sampleCounts()
    assert np.array_equal(counts, got[..., 3].astype(np.uint32))
    assert st["pixel_samples"] == int(counts.astype(np.int64).sum())

    # 2. counts: uniform per block, within [min_spp, max_spp], whole rounds unless at max_spp
    blocks = block_of_pixels(counts, *BLOCK)
    bc = blocks.max(-1)
    assert ((blocks == bc[..., None]) | (blocks < 0)).all()
    assert (bc >= MIN_SPP).all() and (bc <= max_spp).all()
    assert ((bc % BATCH == 0) | (bc == max_spp)).all()
    assert st["rounds"] == -(-int(bc.max()) // BATCH)
    assert st["blocks"] == bc.size
    assert len(np.unique(bc)) > 1                     # the threshold was picked to stop some blocks early
    # every pixel holds the fixed sequence's accumulator after its own number of rounds, bit for bit
    rnd = -(-counts.astype(np.int64) // BATCH) - 1
    expect = np.take_along_axis(np.stack(ref.accs), rnd[None, ..., None].repeat(4, -1), 0)[0]
    assert np.array_equal(got.view(np.uint32), expect.view(np.uint32))

    # 3. the estimator, against the device's own state
    err, _ = check_estimator(t, got, counts, ref.lum, what)

    # 4. decisions: every block that stopped below max_spp had converged, exactly ...
    last = -(-bc // BATCH) - 1
    thr32 = np.float32(thr)
    assert (err[bc < max_spp] < thr32).all()
    assert st["blocks_at_max"] == int(((bc == max_spp) & ~(err < thr32)).sum())
    hist = np.bincount(last.reshape(-1), minlength=len(rounds_of(max_spp, BATCH)))
    host_stop, _, host_at_max, _ = AV.simulate(ref.errs, BATCH, MIN_SPP, max_spp, thr)
    print("%s: threshold %.6g, stop-round histogram %s (host restatement %s), %d blocks at max unconverged (host %d), "
          "%d zero-error blocks" % (what, thr, hist.tolist(), np.bincount(host_stop.reshape(-1), minlength=len(hist)).tolist(),
                                    st["blocks_at_max"], host_at_max, int((err == 0).sum())))
    # ... and at every round boundary past min_spp a block still running after it had not: the frame cut off after round k
    # reports the errors of round k for exactly those blocks
    pairs = skipped = 0
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
        skipped += int(near.sum())
    assert pairs > 0 and skipped <= 0.01 * pairs, (skipped, pairs)
    return bc, err


# ---- 1. threshold 0 is the fixed sequence -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_threshold_zero_is_the_fixed_sequence(case):
    wl, t, ref = configured(case)
    fixed = ref.accs[-1]
    assert fixed[..., :3].any()
    st = t.renderAdaptiveVariance(wl.camera, 0.0, **KW)
    got = read_accum(t)
    img = t.transferImage()
    assert np.array_equal(got.view(np.uint32), fixed.view(np.uint32))
    assert np.array_equal(img.view(np.uint32), ref.image.view(np.uint32))
    assert st["rounds"] == len(ref.accs)
    assert st["pixel_samples"] == wl.width * wl.height * MAX_SPP
    assert st["blocks"] == -(-wl.width // 8) * -(-wl.height // 8)
    assert st["blocks_at_max"] == st["blocks"]
    assert (t.sampleCounts() == MAX_SPP).all()
    check_estimator(t, got, MAX_SPP, ref.lum, case_id(case) + " threshold 0")
    # the Dammertz call at the same rounds
    st_d = t.renderAdaptive(wl.camera, 0.0, **KW)
    assert st_d == st
    assert np.array_equal(read_accum(t).view(np.uint32), got.view(np.uint32))
    assert np.array_equal(t.transferImage().view(np.uint32), img.view(np.uint32))


# ---- 2 to 4. truncation identity, estimator, decisions ------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_truncation_estimator_and_decisions(case):
    wl, t, ref = configured(case)
    run = lambda thr, max_spp: t.renderAdaptiveVariance(wl.camera, thr, batch=BATCH, min_spp=MIN_SPP, max_spp=max_spp, block=BLOCK)
    check_frame(t, run, ref.thr_middle, ref, what=case_id(case) + " middle")


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "c2"], ids=case_id)
def test_low_threshold_leaves_blocks_at_max(case):
    """The 10th percentile of the positive block errors after the last round: most blocks with noise run to max_spp."""
    wl, t, ref = configured(case)
    run = lambda thr, max_spp: t.renderAdaptiveVariance(wl.camera, thr, batch=BATCH, min_spp=MIN_SPP, max_spp=max_spp, block=BLOCK)
    bc, err = check_frame(t, run, ref.thr_p10, ref, what=case_id(case) + " 10th percentile")
    assert (bc == MAX_SPP).any() and (bc < MAX_SPP).any()
    assert ((bc == MAX_SPP) & ~(err < np.float32(ref.thr_p10))).any()


# ---- 5. min_spp == batch ------------------------------------------------------------------------------------------------

def test_min_spp_equal_to_batch_decides_after_round_zero():
    """Sky, a light and a mirror only: every pixel is finished in closed form, all its samples are equal, every moment is
    0 — and with min_spp == batch, which the Dammertz rule refuses, every block stops after round 0."""
    s = rt.SceneCreator()
    s.addMaterial(A.T_LIGHT, (1.0, 0.9, 0.8), 0.0)
    s.addMaterial(A.T_REFLECTIVE, (0.8, 0.8, 0.9), 0.0)
    s.addSphere((0.0, 0.0, 6.0), 1.5, 0)
    s.addSphere((2.5, 0.5, 5.0), 1.0, 1)
    w, h = 120, 90
    cam = rt.workloads._camera(w, h, (0, 0, 0), 0.0)
    t = T(w, h, scene=s, seed=cases.SEED)
    try:
        t.setOption(T.OPT_MOMENTS, 1)
        for arith, sharing in [(a, sh) for a in (rt.ARITH_IEEE, rt.ARITH_ROCM_OCL) for sh in (1, 0)]:
            t.setArith(arith)
            t.setOption(T.OPT_PREFIX_SHARING, sharing)
            st = t.renderAdaptiveVariance(cam, 1e-3, batch=16, min_spp=16, max_spp=512, block=BLOCK)
            assert st["rounds"] == 1 and st["blocks_at_max"] == 0
            assert st["pixel_samples"] == w * h * 16
            assert (t.sampleCounts() == 16).all()
            print("arith %d sharing %d: max block error %.3g, max M2 %.3g" % (arith, sharing, t.blockError().max(), t.moments().max()))
            assert (t.blockError() == 0).all() and (t.pixelError() == 0).all() and (t.moments() == 0).all()
            before = read_accum(t), t.transferImage(), t.pixelError(), t.blockError()
            assert before[0][..., :3].any()
            with pytest.raises(rt.RtError) as ei:
                t.renderAdaptive(cam, 1e-3, batch=16, min_spp=16, max_spp=512, block=BLOCK)
            assert ei.value.code == EINVAL
            after = read_accum(t), t.transferImage(), t.pixelError(), t.blockError()
            for a, b in zip(before, after):
                assert a.tobytes() == b.tobytes()
    finally:
        t.close()


# ---- 6. cameras ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arith", [rt.ARITH_IEEE, rt.ARITH_ROCM_OCL])
def test_identical_blocks_equal_the_one_camera_call(arith):
    wl, t, ref = configured(("c2", arith, 1))
    same = np.tile(np.asarray(wl.camera, np.float32), (MAX_SPP, 1))
    thr = ref.thr_middle
    want_st = t.renderAdaptiveVariance(wl.camera, thr, **KW)
    want = read_accum(t), t.sampleCounts(), t.transferImage()
    want_err, want_perr = check_estimator(t, want[0], want[1], ref.lum, "one camera")
    t.clear()
    got_st = t.renderAdaptiveVarianceCameras(same, thr, batch=BATCH, min_spp=MIN_SPP, block=BLOCK)
    got = read_accum(t), t.sampleCounts(), t.transferImage()
    assert len(np.unique(want[1])) > 1
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    assert got_st == want_st
    # the camera kernels sum a launch's moments in their own order: the errors agree to the estimator's tolerances
    err, perr = check_estimator(t, got[0], got[1], ref.lum, "identical blocks")
    print("identical blocks against one camera: block errors differ by at most %.3g relative, pixel errors equal in %d of %d" %
          (np.abs(err / np.where(want_err > 0, want_err, 1.0) - (want_err > 0)).max(), int((perr == want_perr).sum()), perr.size))


@pytest.mark.parametrize("arith", [rt.ARITH_IEEE, rt.ARITH_ROCM_OCL])
def test_jittered_blocks(arith):
    """Camera.sampleBlocks' pixel jitter: 2 to 4 with renderSamplesCameras as the fixed sequence."""
    wl, t, _ = configured(("c2", arith, 1))
    cam = rt.Camera(60, np.float32(wl.width) / np.float32(wl.height), (-8, -1, -8), 45.0, 0.0)
    blocks = cam.sampleBlocks(MAX_SPP, 0, wl.width, wl.height)
    assert len({b.tobytes() for b in blocks}) == MAX_SPP
    key = ("c2-jittered", arith)
    if key not in _refs:
        _refs[key] = Reference(t, blocks, cameras=True)
        t.setOption(T.OPT_MOMENTS, 1)
    ref = _refs[key]
    run = lambda thr, max_spp: t.renderAdaptiveVarianceCameras(blocks[:max_spp], thr, batch=BATCH, min_spp=MIN_SPP, block=BLOCK)
    # threshold 0: the fixed camera sequence
    st = run(0.0, MAX_SPP)
    assert np.array_equal(read_accum(t).view(np.uint32), ref.accs[-1].view(np.uint32))
    assert np.array_equal(t.transferImage().view(np.uint32), ref.image.view(np.uint32))
    assert st["rounds"] == len(ref.accs) and st["blocks_at_max"] == st["blocks"]
    check_frame(t, run, ref.thr_middle, ref, what="c2 jittered arith%d" % arith)


# ---- 7. state -----------------------------------------------------------------------------------------------------------

def test_state_and_error_cases():
    wl = rt.workloads.get("c1", width=64, height=48)
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    lib, ctx = t._lib, t._ctx
    try:
        good = dict(batch=16, min_spp=32, max_spp=64, block=(8, 8))
        same = np.tile(np.asarray(wl.camera, np.float32), (64, 1))
        e = np.empty((wl.height, wl.width), np.float32)
        d = C.c_void_p()

        def pixel_error_state():
            return lib.rt_read_pixel_error(ctx, e.ctypes.data, e.nbytes), lib.rt_device_pixel_error(ctx, C.byref(d))

        def code_of(call):
            with pytest.raises(rt.RtError) as ei:
                call()
            return ei.value.code

        assert pixel_error_state() == (ESTATE, ESTATE)                # before the first call
        t.renderFrame(wl.camera, 8)
        before = read_accum(t), t.transferImage(), t.sampleCounts()

        def untouched():
            after = read_accum(t), t.transferImage(), t.sampleCounts()
            return all(a.tobytes() == b.tobytes() for a, b in zip(before, after))

        # RT_OPT_MOMENTS 0: RT_ESTATE, and the call does not switch the option on
        assert code_of(lambda: t.renderAdaptiveVariance(wl.camera, 0.1, **good)) == ESTATE
        assert code_of(lambda: t.renderAdaptiveVarianceCameras(same, 0.1, batch=16, min_spp=32)) == ESTATE
        assert "RT_OPT_MOMENTS" in lib.rt_last_error(ctx).decode()
        assert code_of(t.moments) == ESTATE
        assert untouched() and pixel_error_state() == (ESTATE, ESTATE)
        # a sharded context (which cannot have the moments on): RT_EINVAL
        t.setShard(0, 2, 8, 8)
        assert code_of(lambda: t.renderAdaptiveVariance(wl.camera, 0.1, **good)) == EINVAL
        assert code_of(lambda: t.renderAdaptiveVarianceCameras(same, 0.1, batch=16, min_spp=32)) == EINVAL
        t.setShard(0, 1, 8, 8)
        t.setOption(T.OPT_MOMENTS, 1)
        # every parameter rule
        bad = [dict(batch=0), dict(batch=513), dict(min_spp=8), dict(min_spp=40), dict(batch=1, min_spp=1),
               dict(max_spp=31), dict(batch=512, min_spp=1024, max_spp=65537), dict(block=(6, 8)), dict(block=(8, 0)),
               dict(block=(512, 8))]
        for b in bad:
            kw = dict(good, **b)
            assert code_of(lambda: t.renderAdaptiveVariance(wl.camera, 0.1, **kw)) == EINVAL, b
        for thr in (-1.0, float("nan"), float("inf")):
            assert code_of(lambda: t.renderAdaptiveVariance(wl.camera, thr, **good)) == EINVAL, thr
            assert code_of(lambda: t.renderAdaptiveVarianceCameras(same, thr, batch=16, min_spp=32)) == EINVAL, thr
        assert code_of(lambda: t.renderAdaptiveVarianceCameras(same, 0.1, batch=16, min_spp=24)) == EINVAL
        cam = np.ascontiguousarray(wl.camera, dtype=np.float32)
        p = A.AdaptiveParams(16, 32, 64, 0.1, 8, 8)
        st = A.AdaptiveStats()
        assert lib.rt_render_adaptive_variance(ctx, None, C.byref(p), C.byref(st)) == EINVAL
        assert lib.rt_render_adaptive_variance(ctx, cam.ctypes.data, None, C.byref(st)) == EINVAL
        assert lib.rt_render_adaptive_variance(ctx, cam.ctypes.data, C.byref(p), None) == EINVAL
        assert lib.rt_render_adaptive_variance_cameras(ctx, None, 64, C.byref(p), C.byref(st)) == EINVAL
        assert lib.rt_render_adaptive_variance_cameras(ctx, same.ctypes.data, 63, C.byref(p), C.byref(st)) == EINVAL
        assert untouched() and pixel_error_state() == (ESTATE, ESTATE)
        assert code_of(t.blockError) == ESTATE

        # a good call: min_spp == batch is allowed, the errors can be read, the moments are valid
        t.renderAdaptiveVariance(wl.camera, 0.1, batch=16, min_spp=16, max_spp=64)
        assert pixel_error_state() == (0, 0) and d.value
        assert d.value == t.devicePixelError() and d.value != t.deviceMoments()
        assert t.pixelError().shape == (48, 64) and t.blockError().shape == (6, 8) and t.moments().shape == (48, 64)
        assert lib.rt_read_pixel_error(ctx, e.ctypes.data, e.nbytes - 4) == EINVAL
        assert lib.rt_read_pixel_error(ctx, None, e.nbytes) == EINVAL
        assert lib.rt_device_pixel_error(ctx, None) == EINVAL
        # a failed call of either rule leaves them readable, a later Dammertz call does not
        assert code_of(lambda: t.renderAdaptiveVariance(wl.camera, 0.1, **dict(good, batch=0))) == EINVAL
        assert code_of(lambda: t.renderAdaptive(wl.camera, 0.1, **dict(good, min_spp=16))) == EINVAL
        assert pixel_error_state() == (0, 0)
        t.renderAdaptive(wl.camera, 0.1, **good)
        assert pixel_error_state() == (ESTATE, ESTATE)
        assert t.blockError().shape == (6, 8)
        t.renderAdaptiveVarianceCameras(same, 0.1, batch=16, min_spp=32)
        assert pixel_error_state() == (0, 0)
        t.renderAdaptiveCameras(same, 0.1, batch=16, min_spp=32)
        assert pixel_error_state() == (ESTATE, ESTATE)
        t.renderAdaptiveVariance(wl.camera, 0.1, **good)
        assert pixel_error_state() == (0, 0)
        # the option switched off: the call is refused, what the last call left stays
        t.setOption(T.OPT_MOMENTS, 0)
        assert code_of(lambda: t.renderAdaptiveVariance(wl.camera, 0.1, **good)) == ESTATE
        assert pixel_error_state() == (0, 0)
        t.setOption(T.OPT_MOMENTS, 1)
        t.resize(40, 30)
        e = np.empty((30, 40), np.float32)
        assert pixel_error_state() == (ESTATE, ESTATE)                # after rt_resize
        assert code_of(t.blockError) == ESTATE
        t.renderAdaptiveVariance(wl.camera, 0.1, **good)
        assert pixel_error_state() == (0, 0) and t.pixelError().shape == (30, 40)
    finally:
        t.close()


def test_denoise_moments_follows_directly():
    wl = rt.workloads.get("c2", width=64, height=40)
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        t.setOption(T.OPT_MOMENTS, 1)
        t.renderAdaptiveVariance(wl.camera, 0.05, batch=4, min_spp=4, max_spp=32)
        counts = t.sampleCounts()
        assert len(np.unique(counts)) > 1
        args = dict(A.DENOISE_VARIANCE_DEFAULTS)
        acc, m2 = read_accum(t), t.moments()
        t.renderFeatures(wl.camera)
        feats = t.features()
        got = t.denoiseMoments(**args)
        v0, vl = t.variance(0), t.variance(1)
        exp, lin, v0_ref, vl_ref = M.filter_moments(acc, m2, feats, **args)
        assert (acc[..., 3] > 0).all() and (got[..., 3] == 1).all()
        e_c = np.abs(got[..., :3].astype(np.float64) ** 2 - lin).max()
        e_v0 = (np.abs(v0 - v0_ref) / np.maximum(1.0, v0_ref)).max()
        e_vl = (np.abs(vl - vl_ref) / np.maximum(1.0, vl_ref)).max()
        print("denoiseMoments after renderAdaptiveVariance: linear colour %.3g, v0 %.3g, v(L) %.3g (bound 2e-5 each)" % (e_c, e_v0, e_vl))
        assert e_c <= 2e-5 and e_v0 <= 2e-5 and e_vl <= 2e-5
        # the filter moved neither the accumulator nor the errors
        assert read_accum(t).tobytes() == acc.tobytes() and t.pixelError().shape == counts.shape
    finally:
        t.close()


def test_cli_variance_rule_matches_the_python_path(built, tmp_path):
    import os
    import subprocess
    w, h = 120, 72
    scene = os.path.join(cases.ROOT, "assets", "scenes", "c2_cornell.scene")
    raw, aov, cnt = str(tmp_path / "f.f32"), str(tmp_path / "aov"), str(tmp_path / "c.u32")
    cmd = [os.path.join(cases.ROOT, "host", "rt_cli"), "--scene", scene, "--size", "%dx%d" % (w, h), "--camera=-8,-1,-8,45,0",
           "--adaptive", "0.05", "--adaptive-rule", "variance", "--batch", "16", "--min-spp", "16", "--spp", "104",
           "--raw", raw, "--aov", aov, "--counts", cnt]
    out = subprocess.run(cmd, check=True, cwd=cases.ROOT, capture_output=True, text=True, timeout=120)
    assert "(variance rule)" in out.stdout
    s = rt.SceneCreator()
    s.loadScene(scene, base_dir=os.path.join(cases.ROOT, "assets"))
    t = T(w, h, scene=s)
    try:
        cam = rt.Camera(60, np.float32(w) / np.float32(h), (-8, -1, -8), 45.0, 0.0)
        t.setOption(T.OPT_MOMENTS, 1)
        t.renderAdaptiveVariance(cam, 0.05, batch=16, min_spp=16, max_spp=104)
        img, perr, counts = t.transferImage(), t.pixelError(), t.sampleCounts()
    finally:
        t.close()
    assert len(np.unique(counts)) > 1 and (counts == 16).any()
    assert np.array_equal(np.fromfile(raw, np.float32).view(np.uint32), img.reshape(-1).view(np.uint32))
    assert np.array_equal(np.fromfile(cnt, np.uint32), counts.reshape(-1))
    head = b"Pf\n%d %d\n-1.0\n" % (w, h)
    pfm = open(aov + "_error.pfm", "rb").read()
    assert pfm.startswith(head)
    assert np.array_equal(np.frombuffer(pfm[len(head):], np.float32).view(np.uint32), perr.reshape(-1).view(np.uint32))


# ---- 8. the shared loop was not disturbed -------------------------------------------------------------------------------

def test_dammertz_rule_is_the_same_with_and_without_moments():
    wl, t, ref = configured(("c2", rt.ARITH_ROCM_OCL, 1))
    got = []
    for on in (0, 1):
        t.setOption(T.OPT_MOMENTS, on)
        st = t.renderAdaptive(wl.camera, 0.02, **KW)
        got.append((read_accum(t), t.blockError(), t.sampleCounts(), t.transferImage(), st))
    assert len(np.unique(got[0][2])) > 1
    for a, b in zip(got[0][:4], got[1][:4]):
        assert a.tobytes() == b.tobytes()
    assert got[0][4] == got[1][4]
    # and it still is the truncated fixed sequence
    rnd = -(-got[0][2].astype(np.int64) // BATCH) - 1
    expect = np.take_along_axis(np.stack(ref.accs), rnd[None, ..., None].repeat(4, -1), 0)[0]
    assert np.array_equal(got[0][0].view(np.uint32), expect.view(np.uint32))
