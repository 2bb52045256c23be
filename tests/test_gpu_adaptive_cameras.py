"""GPU (-m gpu): adaptive sampling through per-sample cameras (rt_render_adaptive_cameras).  Every pixel of such a frame
must hold, bit for bit, what the fixed sequence rt_clear; rt_render_spp_cameras(blocks + 12 k batch, k batch, c_k) for
k = 0 .. holds after as many rounds as the pixel got — the first time the camera kernels run under a block mask — and the
stopping decisions must follow the block error of the header's estimator, rebuilt on the host from the rounds' sums.
All blocks of a frame differ, so a wrong block offset, mask or ring table in any round changes bits."""
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
T = rt.RayTracer
EINVAL, ESTATE = -1, -4
FIXED, QUEUE = A.CAMERA_PLAN_FIXED, A.CAMERA_PLAN_QUEUE

BATCH, MIN_SPP, MAX_SPP = 32, 64, 232      # 232 = 7 x 32 + 8: the last round is a partial one
BLOCK = (8, 8)

SCENES = {
    # frame sizes that are multiples neither of the 8 x 8 decision block nor of the 64 x 4 tile
    "c2": lambda: rt.workloads.get("c2", width=244, height=138),
    "c3": lambda: rt.workloads.get("c3", width=200, height=130),
    "glass": lambda: rt.workloads.get("c5", width=132, height=100),
}
MODES = {   # arithmetic policy, options on top of the defaults, the camera kernel the rounds must run
    "ieee": (rt.ARITH_IEEE, {}, QUEUE),
    "ocl": (rt.ARITH_ROCM_OCL, {}, QUEUE),
    "ocl-fill0": (rt.ARITH_ROCM_OCL, dict(OPT_WAVE_FILL=0), QUEUE),      # a wave owns several slots: masks cut through them
    "ocl-fixed": (rt.ARITH_ROCM_OCL, dict(OPT_SAMPLE_QUEUE=0), FIXED),
}


def read_accum(t):
    import torch
    t.sync()
    return torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().copy()


def offset_blocks(wl, n, seed=5):
    """n different camera blocks: the workload's camera with the lower left corner moved inside the pixel, per sample."""
    cam = np.asarray(wl.camera, dtype=np.float32)
    d = np.random.RandomState(seed).uniform(-0.5, 0.5, (n, 2)).astype(np.float32)
    b = np.tile(cam, (n, 1))
    b[:, 3:6] = cam[3:6] + (d[:, 0:1] / np.float32(wl.width)) * cam[6:9] + (d[:, 1:2] / np.float32(wl.height)) * cam[9:12]
    assert len({r.tobytes() for r in b}) == n
    return b


def rounds_of(max_spp, batch):
    return [(k * batch, min(batch, max_spp - k * batch)) for k in range(-(-max_spp // batch))]


def round_sums(t, blocks, batch):
    """Each round's exact per-pixel sum: rt_clear; rt_render_spp_cameras(blocks[first:first+c], first) adds it to zeros."""
    out = []
    for first, c in rounds_of(len(blocks), batch):
        t.clear()
        t.renderSamplesCameras(blocks[first:first + c], first)
        out.append(read_accum(t))
    return out


def cumulative(sums):
    """float32 sums in round order: what the accumulator (all rounds) and the half accumulator (even rounds) hold after
    each round."""
    acc, half = np.zeros_like(sums[0]), np.zeros_like(sums[0])
    accs, halves = [], []
    for k, s in enumerate(sums):
        acc = acc + s
        if k % 2 == 0:
            half = half + s
        accs.append(acc)
        halves.append(half)
    for a in accs + halves:
        a.setflags(write=False)
    return accs, halves


def pick_threshold(accs, halves, block=BLOCK):
    """A threshold that stops some blocks early and keeps others running: the median of the host's block errors after
    round 3."""
    e = A.block_error_reference(accs[3], halves[3], *block)
    return float(np.median(e[e > 0])) if (e > 0).any() else 1e-3


def block_of_pixels(counts, bw, bh):
    h, w = counts.shape
    by, bx = -(-h // bh), -(-w // bw)
    pad = np.full((by * bh, bx * bw), -1, dtype=np.int64)
    pad[:h, :w] = counts
    return pad.reshape(by, bh, bx, bw).transpose(0, 2, 1, 3).reshape(by, bx, bh * bw)


DEFAULTS = dict(OPT_WAVE_FILL=None, OPT_SAMPLE_QUEUE=1, OPT_MAX_THREADS_PER_LAUNCH=1 << 30, OPT_MOMENTS=0)
_cache = {}


@pytest.fixture(scope="module", params=sorted(SCENES))
def scene(request):
    wl = SCENES[request.param]()
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    yield request.param, wl, t, offset_blocks(wl, MAX_SPP)
    t.close()


def configured(scene, mode, fill):
    """The scene's tracer under `mode`, and the cumulative reference of (scene, policy) — traced under the defaults."""
    name, wl, t, blocks = scene
    arith, options, family = MODES[mode]
    for k, v in DEFAULTS.items():
        t.setOption(getattr(T, k), fill if v is None else v)
    t.setArith(arith)
    key = (name, arith)
    if key not in _cache:
        _cache[key] = cumulative(round_sums(t, blocks, BATCH))
    for k, v in options.items():
        t.setOption(getattr(T, k), v)
    return wl, t, blocks, _cache[key], family


@pytest.fixture
def fill(request):
    """RT_OPT_WAVE_FILL of this test's tracers (conftest: by the test's name); the module's shared tracers follow it."""
    import zlib
    return zlib.crc32(request.node.nodeid.encode()) & 1


# ---- 1. threshold 0 is the fixed camera sequence ------------------------------------------------------------------------

@pytest.mark.parametrize("mode", sorted(MODES))
def test_threshold_zero_is_the_fixed_camera_sequence(scene, mode, fill):
    wl, t, blocks, (accs, _), family = configured(scene, mode, fill)
    t.clear()
    for first, c in rounds_of(MAX_SPP, BATCH):
        t.renderSamplesCameras(blocks[first:first + c], first)
    fixed = read_accum(t)
    assert np.array_equal(fixed.view(np.uint32), accs[-1].view(np.uint32))   # the per-round sums compose exactly
    assert fixed[..., :3].any()
    t.resolve()
    fixed_img = t.transferImage()
    st = t.renderAdaptiveCameras(blocks, 0.0, batch=BATCH, min_spp=MIN_SPP, block=BLOCK)
    got = read_accum(t)
    facts, plan = t.lastCameraPlan()
    assert plan["family"] == family and facts["count"] == MAX_SPP % BATCH
    assert np.array_equal(got.view(np.uint32), fixed.view(np.uint32))
    assert np.array_equal(t.transferImage().view(np.uint32), fixed_img.view(np.uint32))
    assert st["rounds"] == len(accs)
    assert st["pixel_samples"] == wl.width * wl.height * MAX_SPP
    assert st["blocks"] == -(-wl.width // 8) * -(-wl.height // 8)
    assert st["blocks_at_max"] == st["blocks"]
    assert (t.sampleCounts() == MAX_SPP).all()


# ---- 2. truncation identity and estimator -------------------------------------------------------------------------------

def check_truncated_frame(t, st, thr, accs, halves, batch, min_spp, max_spp, block=BLOCK):
    got = read_accum(t)
    counts = t.sampleCounts()
    err = t.blockError()
    assert np.array_equal(counts, got[..., 3].astype(np.uint32))
    assert st["pixel_samples"] == int(counts.astype(np.int64).sum())

    # counts: uniform per block, within [min_spp, max_spp], whole rounds unless at max_spp
    blocks = block_of_pixels(counts, *block)
    bc = blocks.max(-1)
    assert ((blocks == bc[..., None]) | (blocks < 0)).all()
    assert (bc >= min_spp).all() and (bc <= max_spp).all()
    assert ((bc % batch == 0) | (bc == max_spp)).all()
    assert st["rounds"] == -(-int(bc.max()) // batch)
    assert len(np.unique(bc)) > 1                     # the threshold was picked to stop some blocks early

    # every pixel holds the fixed sequence's accumulator after its own number of rounds, bit for bit
    rnd = -(-counts.astype(np.int64) // batch) - 1
    stack = np.stack(accs)
    expect = np.take_along_axis(stack, rnd[None, ..., None].repeat(4, -1), 0)[0]
    assert np.array_equal(got.view(np.uint32), expect.view(np.uint32))

    # the estimator: the device's block errors are the host's after each block's last round ...
    host = [None] + [A.block_error_reference(accs[k], halves[k], *block) for k in range(1, len(accs))]
    last = -(-bc // batch) - 1
    exp_err = np.choose(last, [np.zeros_like(host[1])] + host[1:])
    np.testing.assert_allclose(err, exp_err, rtol=1e-5, atol=1e-7)
    # ... every block that stopped below max_spp had converged ...
    below = bc < max_spp
    assert (err[below] < thr).all()
    # ... and at every earlier round past min_spp a still-running block had not (ties within 1e-4 thr skipped)
    for k in range(1, len(accs)):
        if (k + 1) * batch < min_spp:
            continue
        running = last > k
        e = host[k][running]
        near = np.abs(e - thr) <= 1e-4 * thr
        assert (e[~near] >= thr).all(), k
    assert st["blocks_at_max"] == int(((bc == max_spp) & ~(err < thr)).sum())
    return got, counts, err


@pytest.mark.parametrize("mode", sorted(MODES))
def test_truncation_identity_and_estimator(scene, mode, fill):
    wl, t, blocks, (accs, halves), family = configured(scene, mode, fill)
    thr = pick_threshold(accs, halves)
    st = t.renderAdaptiveCameras(blocks, thr, batch=BATCH, min_spp=MIN_SPP, block=BLOCK)
    assert t.lastCameraPlan()[1]["family"] == family
    check_truncated_frame(t, st, thr, accs, halves, BATCH, MIN_SPP, MAX_SPP)


# ---- 3. identical blocks equal renderAdaptive ---------------------------------------------------------------------------

def test_identical_blocks_equal_render_adaptive():
    wl = SCENES["c2"]()
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        t.setArith(rt.ARITH_ROCM_OCL)
        same = np.tile(np.asarray(wl.camera, np.float32), (MAX_SPP, 1))
        accs, halves = cumulative(round_sums(t, same, BATCH))
        thr = pick_threshold(accs, halves)
        want_st = t.renderAdaptive(wl.camera, thr, batch=BATCH, min_spp=MIN_SPP, max_spp=MAX_SPP, block=BLOCK)
        want = read_accum(t), t.sampleCounts(), t.blockError(), t.transferImage()
        t.clear()
        got_st = t.renderAdaptiveCameras(same, thr, batch=BATCH, min_spp=MIN_SPP, block=BLOCK)
        got = read_accum(t), t.sampleCounts(), t.blockError(), t.transferImage()
        assert len(np.unique(want[1])) > 1
        for g, w in zip(got, want):
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
        assert got_st == want_st
    finally:
        t.close()


# ---- 4. masked pixels do no work ----------------------------------------------------------------------------------------

def test_masked_pixels_do_no_work():
    wl = rt.workloads.get("c1", width=160, height=120)
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        blocks = offset_blocks(wl, MAX_SPP)
        accs, halves = cumulative(round_sums(t, blocks, BATCH))
        thr = pick_threshold(accs, halves)
        t.enableCounters(True)
        t.resetCounters()
        st = t.renderAdaptiveCameras(blocks, thr, batch=BATCH, min_spp=MIN_SPP, block=BLOCK)
        n = int(t.counters().samples)
        _, plan = t.lastCameraPlan()
        t.enableCounters(False)
        counts = t.sampleCounts()
        assert plan["family"] == FIXED and plan["count"] == 1          # the counting fixed-lane kernel
        assert n == st["pixel_samples"] == int(counts.astype(np.int64).sum())
        assert n < wl.width * wl.height * MAX_SPP
        assert (counts < MAX_SPP).any() and (counts > MIN_SPP).any()
    finally:
        t.close()


# ---- 5. per-sample truth ------------------------------------------------------------------------------------------------

def test_single_samples_match_the_accumulator(oracle, table):
    wl = rt.workloads.get("c2", width=160, height=90)
    batch, min_spp, max_spp = 32, 64, 200
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        blocks = offset_blocks(wl, max_spp)
        st = t.renderAdaptiveCameras(blocks, 0.02, batch=batch, min_spp=min_spp, block=BLOCK)
        assert st["rounds"] >= 2
        acc = read_accum(t)
        counts = t.sampleCounts()
        rng = np.random.RandomState(11)
        xs, ys = rng.randint(0, wl.width, 24), rng.randint(0, wl.height, 24)
        # sample j of the 24 pixels through block j, for every j some pixel holds
        top = int(counts[ys, xs].max())
        rad = np.stack([t.traceSamples(blocks[j], xs, ys, np.full(24, j)) for j in range(top)], axis=1)   # (24, top, 3)
        checked = 0
        for i, (x, y) in enumerate(zip(xs, ys)):
            n = int(counts[y, x])
            assert acc[y, x, 3] == n and min_spp <= n <= max_spp
            np.testing.assert_allclose(acc[y, x, :3], rad[i, :n].astype(np.float64).sum(0), rtol=1e-6, atol=1e-6)
            for j in rng.choice(n, 8, replace=False):      # eight of them against the CPU oracle, bit for bit
                exp, _ = oracle.samples(wl.scene, blocks[j], table, wl.width, wl.height, [x], [y], [j])
                assert np.array_equal(rad[i, j].view(np.uint32), np.asarray(exp, np.float32).reshape(3).view(np.uint32)), (x, y, j)
                checked += 1
        assert checked == 24 * 8
    finally:
        t.close()


# ---- 6. moments ---------------------------------------------------------------------------------------------------------

def test_moments_follow_the_sample_luminances():
    wl = rt.workloads.get("c2", width=160, height=90)
    batch, min_spp, max_spp = 16, 32, 96
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        blocks = offset_blocks(wl, max_spp)
        accs, halves = cumulative(round_sums(t, blocks, batch))
        thr = pick_threshold(accs, halves)
        st0 = t.renderAdaptiveCameras(blocks, thr, batch=batch, min_spp=min_spp, block=BLOCK)
        plain = read_accum(t), t.transferImage(), t.sampleCounts()
        assert t.lastCameraPlan()[1]["moments"] == 0
        t.setOption(T.OPT_MOMENTS, 1)
        st1 = t.renderAdaptiveCameras(blocks, thr, batch=batch, min_spp=min_spp, block=BLOCK)
        kept = read_accum(t), t.transferImage(), t.sampleCounts()
        m2 = t.moments()
        _, plan = t.lastCameraPlan()
        assert plan["family"] == FIXED and plan["moments"] == 1
        assert st0 == st1
        for a, b in zip(plain, kept):
            assert a.tobytes() == b.tobytes()
        counts = kept[2]
        assert len(np.unique(counts)) > 1 and (m2 >= 0).all()
        # the float64 two-pass M2 of the luminances of the samples each pixel holds, on a seeded subset of the pixels
        rng = np.random.RandomState(23)
        xs, ys = rng.randint(0, wl.width, 200), rng.randint(0, wl.height, 200)
        n = counts[ys, xs].astype(np.int64)
        lum = np.stack([t.traceSamples(blocks[j], xs, ys, np.full(len(xs), j)).astype(np.float64) @ V.LUM
                        for j in range(int(n.max()))], axis=1)                       # (200, max n)
        use = np.arange(lum.shape[1])[None, :] < n[:, None]
        mean = np.where(use, lum, 0.0).sum(-1) / n
        ref = np.where(use, (lum - mean[:, None]) ** 2, 0.0).sum(-1)
        tol = M.tolerance(ref, n, np.where(use, lum, 0.0).max(-1))
        err = np.abs(m2[ys, xs].astype(np.float64) - ref)
        print("max |M2 - truth| %.3g (tolerance there %.3g), max M2 %.4g, counts %s" %
              (err.max(), tol[err.argmax()], ref.max(), np.unique(n)))
        assert (err <= tol).all() and ref.max() > 0 and len(np.unique(n)) > 1
    finally:
        t.close()


# ---- 7. ring reuse ------------------------------------------------------------------------------------------------------

def test_more_rounds_than_the_context_has_camera_tables():
    wl = rt.workloads.get("c1", width=64, height=48)
    batch, min_spp, max_spp = 2, 4, 14           # 7 rounds through a ring of 4 tables
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        blocks = offset_blocks(wl, max_spp)
        sums = round_sums(t, blocks, batch)
        assert len(sums) == 7 and len({s.tobytes() for s in sums}) == 7
        accs, _ = cumulative(sums)
        st = t.renderAdaptiveCameras(blocks, 0.0, batch=batch, min_spp=min_spp, block=BLOCK)
        got = read_accum(t)
        assert st["rounds"] == 7 and (got[..., 3] == max_spp).all()
        assert np.array_equal(got.view(np.uint32), accs[-1].view(np.uint32))
    finally:
        t.close()


# ---- 8. split launches --------------------------------------------------------------------------------------------------

def test_split_launches_change_no_bit():
    wl = SCENES["c2"]()
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        t.setArith(rt.ARITH_ROCM_OCL)
        blocks = offset_blocks(wl, MAX_SPP)
        key = ("c2", rt.ARITH_ROCM_OCL)
        if key not in _cache:
            _cache[key] = cumulative(round_sums(t, blocks, BATCH))
        thr = pick_threshold(*_cache[key])
        st = t.renderAdaptiveCameras(blocks, thr, batch=BATCH, min_spp=MIN_SPP, block=BLOCK)
        whole = read_accum(t), t.sampleCounts(), t.blockError(), t.transferImage()
        t.setOption(T.OPT_MAX_THREADS_PER_LAUNCH, 4096)
        st_split = t.renderAdaptiveCameras(blocks, thr, batch=BATCH, min_spp=MIN_SPP, block=BLOCK)
        facts, _ = t.lastCameraPlan()
        split = read_accum(t), t.sampleCounts(), t.blockError(), t.transferImage()
        assert facts["n"] < wl.width * wl.height / 100          # many slot ranges per round
        assert len(np.unique(whole[1])) > 1
        for a, b in zip(whole, split):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert st == st_split
    finally:
        t.close()


# ---- 9. arguments and state ---------------------------------------------------------------------------------------------

def test_bad_arguments_leave_the_context_untouched():
    wl = rt.workloads.get("c1", width=64, height=48)
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        with pytest.raises(rt.RtError) as ei:
            t.blockError()                            # no adaptive frame yet
        assert ei.value.code == ESTATE
        t.renderFrame(wl.camera, 8)
        before, before_img = read_accum(t), t.transferImage()
        good = dict(batch=16, min_spp=32, block=(8, 8))
        blocks = offset_blocks(wl, 64)
        bad = [dict(batch=0), dict(batch=513), dict(min_spp=16), dict(min_spp=40), dict(max_spp=31),
               dict(batch=512, min_spp=1024, max_spp=65537), dict(block=(6, 8)), dict(block=(8, 0)),
               dict(block=(512, 8))]
        for b in bad:
            kw = dict(good, **b)
            n = kw.pop("max_spp", 64)
            with pytest.raises(rt.RtError) as ei:
                t.renderAdaptiveCameras(np.tile(blocks[:1], (n, 1)), 0.1, **kw)
            assert ei.value.code == EINVAL, b
        for thr in (-1.0, float("nan"), float("inf")):
            with pytest.raises(rt.RtError) as ei:
                t.renderAdaptiveCameras(blocks, thr, **good)
            assert ei.value.code == EINVAL, thr
        lib, ctx = t._lib, t._ctx
        p = A.AdaptiveParams(16, 32, 64, 0.1, 8, 8)
        st = A.AdaptiveStats()
        bp = blocks.ctypes.data
        assert lib.rt_render_adaptive_cameras(ctx, None, 64, C.byref(p), C.byref(st)) == EINVAL
        assert lib.rt_render_adaptive_cameras(ctx, bp, 64, None, C.byref(st)) == EINVAL
        assert lib.rt_render_adaptive_cameras(ctx, bp, 64, C.byref(p), None) == EINVAL
        assert lib.rt_render_adaptive_cameras(None, bp, 64, C.byref(p), C.byref(st)) == EINVAL
        for n in (0, 32, 63):                          # block j is the camera of sample j: n_cameras must be max_spp
            assert lib.rt_render_adaptive_cameras(ctx, bp, n, C.byref(p), C.byref(st)) == EINVAL, n
        t.setShard(0, 2, 8, 8)
        with pytest.raises(rt.RtError) as ei:
            t.renderAdaptiveCameras(blocks, 0.1, **good)
        assert ei.value.code == EINVAL
        t.setShard(0, 1, 8, 8)
        assert np.array_equal(read_accum(t).view(np.uint32), before.view(np.uint32))
        assert np.array_equal(t.transferImage().view(np.uint32), before_img.view(np.uint32))
        with pytest.raises(rt.RtError) as ei:
            t.blockError()                            # still none
        assert ei.value.code == ESTATE
        raw = C.c_void_p()
        assert lib.rt_create(0, 16, 8, C.byref(raw)) == 0
        assert lib.rt_render_adaptive_cameras(raw, bp, 64, C.byref(p), C.byref(st)) == ESTATE      # no scene
        lib.rt_destroy(raw)

        # a good call after the bad ones, then a resize forgets the block errors
        st = t.renderAdaptiveCameras(blocks, 0.1, **good)
        assert st["blocks"] == 6 * 8 and t.blockError().shape == (6, 8)
        t.resize(40, 30)
        with pytest.raises(rt.RtError) as ei:
            t.blockError()
        assert ei.value.code == ESTATE
    finally:
        t.close()


def test_a_kept_prefix_survives_and_the_last_plan_is_the_last_rounds():
    wl = rt.workloads.get("c2", width=64, height=36)
    blocks = offset_blocks(wl, 40)
    t = T(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        t.clear()
        t.renderSamples(wl.camera, 0, 16)
        st = t.renderAdaptiveCameras(blocks, 0.0, batch=16, min_spp=32, block=BLOCK)
        facts, plan = t.lastCameraPlan()
        t.renderSamples(wl.camera, 16, 16)
        t.sync()
        assert t.prefixCacheStats() == (1, 1)      # the second fused call reused the prefix the rounds left alone
        assert st["rounds"] == 3 and facts["count"] == 8 and plan["family"] == QUEUE
    finally:
        t.close()


# ---- 10. rt_cli ---------------------------------------------------------------------------------------------------------

def test_cli_adaptive_cameras_frame_matches_python_path(built, tmp_path):
    w, h, spp, thr = 100, 60, 40, 0.0625
    scene = os.path.join(cases.ROOT, "assets", "scenes", "c2_cornell.scene")
    raw, cnt = str(tmp_path / "f.f32"), str(tmp_path / "c.u32")
    subprocess.run([os.path.join(cases.ROOT, "host", "rt_cli"), "--scene", scene, "--size", "%dx%d" % (w, h), "--camera=-8,-1,-8,45,0",
                    "--aa", "--adaptive-cameras", repr(thr), "--batch", "8", "--min-spp", "16", "--spp", str(spp),
                    "--counts", cnt, "--raw", raw], check=True, cwd=cases.ROOT, timeout=120)
    got = np.fromfile(raw, np.float32).reshape(h, w, 4)
    got_counts = np.fromfile(cnt, np.uint32).reshape(h, w)
    s = rt.SceneCreator()
    s.loadScene(scene, base_dir=os.path.join(cases.ROOT, "assets"))
    t = T(w, h, scene=s)
    try:
        cam = rt.Camera(60, np.float32(w) / np.float32(h), (-8, -1, -8), 45.0, 0.0)
        t.renderAdaptiveCameras(cam.sampleBlocks(spp, width=w, height=h), thr, batch=8, min_spp=16)
        exp, exp_counts = t.transferImage(), t.sampleCounts()
        plain = t.renderFrame(cam, spp)
    finally:
        t.close()
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)) and not np.array_equal(exp, plain)
    assert np.array_equal(got_counts, exp_counts) and got_counts.min() >= 16 and got_counts.max() <= spp
