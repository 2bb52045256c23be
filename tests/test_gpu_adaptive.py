"""GPU (-m gpu): adaptive sampling (rt_render_adaptive).  Every pixel of an adaptive frame must hold, bit for bit, what
the fixed sequence rt_clear; rt_render_spp(cam, k*batch, c_k) for k = 0 .. holds after as many rounds as the pixel got,
and the stopping decisions must follow the block error of the header's estimator, rebuilt here on the host from the
rounds' sums."""
import ctypes as C

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi

BATCH, MIN_SPP, MAX_SPP = 32, 64, 232      # 232 = 7 x 32 + 8: the last round is a partial one
BLOCK = (8, 8)


def glass_scene(width, height):
    """C5 (the dielectric uv-sphere mesh) on a small frame."""
    return rt.workloads.get("c5", width=width, height=height)


SCENES = {
    # frame sizes that are not multiples of the block: edge blocks hold fewer pixels
    "c1": lambda: rt.workloads.get("c1", width=256, height=256),
    "c2": lambda: rt.workloads.get("c2", width=244, height=138),
    "c3": lambda: rt.workloads.get("c3", width=200, height=130),
    "glass": lambda: glass_scene(132, 100),
}
MODES = [(arith, sharing) for arith in (rt.ARITH_IEEE, rt.ARITH_ROCM_OCL) for sharing in (1, 0)]


def read_accum(t):
    import torch
    t.sync()
    return torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().copy()


def rounds_of(max_spp, batch):
    return [(k * batch, min(batch, max_spp - k * batch)) for k in range(-(-max_spp // batch))]


def round_sums(t, cam, batch, max_spp):
    """Each round's exact per-pixel sum: rt_clear; rt_render_spp(cam, k*b, c) adds it to a zero accumulator."""
    out = []
    for first, c in rounds_of(max_spp, batch):
        t.clear()
        t.renderSamples(cam, first, c)
        out.append(read_accum(t))
    return out


def cumulative(sums):
    """float32 sums in round order: what the accumulator (all rounds) and the half accumulator (even rounds) hold
    after each round."""
    acc, half = np.zeros_like(sums[0]), np.zeros_like(sums[0])
    accs, halves = [], []
    for k, s in enumerate(sums):
        acc = acc + s
        if k % 2 == 0:
            half = half + s
        accs.append(acc)
        halves.append(half)
    return accs, halves


_cache = {}


@pytest.fixture(scope="module", params=sorted(SCENES))
def scene(request):
    wl = SCENES[request.param]()
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    yield request.param, wl, t
    t.close()


def configured(scene, mode):
    name, wl, t = scene
    arith, sharing = mode
    t.setArith(arith)
    t.setOption(t.OPT_PREFIX_SHARING, sharing)
    key = (name, arith)      # the sums do not depend on prefix sharing (bit for bit: tests/test_gpu_parity.py)
    if key not in _cache:
        sums = round_sums(t, wl.camera, BATCH, MAX_SPP)
        _cache[key] = cumulative(sums)
    return wl, t, _cache[key]


def block_of_pixels(counts, bw, bh):
    h, w = counts.shape
    by, bx = -(-h // bh), -(-w // bw)
    pad = np.full((by * bh, bx * bw), -1, dtype=np.int64)
    pad[:h, :w] = counts
    blocks = pad.reshape(by, bh, bx, bw).transpose(0, 2, 1, 3).reshape(by, bx, bh * bw)
    return blocks


def pick_threshold(accs, halves):
    """A threshold that stops some blocks early and keeps others running: the median of the host's block errors
    after round 3."""
    e = A.block_error_reference(accs[3], halves[3], *BLOCK)
    return float(np.median(e[e > 0])) if (e > 0).any() else 1e-3


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "arith%d-share%d" % m)
def test_threshold_zero_is_the_fixed_sequence(scene, mode):
    wl, t, (accs, _) = configured(scene, mode)
    # the fixed sequence itself, round after round into one accumulator
    t.clear()
    for first, c in rounds_of(MAX_SPP, BATCH):
        t.renderSamples(wl.camera, first, c)
    fixed = read_accum(t)
    assert np.array_equal(fixed.view(np.uint32), accs[-1].view(np.uint32))   # the per-round sums compose exactly
    t.resolve()
    fixed_img = t.transferImage()
    st = t.renderAdaptive(wl.camera, 0.0, batch=BATCH, min_spp=MIN_SPP, max_spp=MAX_SPP, block=BLOCK)
    got = read_accum(t)
    assert np.array_equal(got.view(np.uint32), fixed.view(np.uint32))
    assert np.array_equal(t.transferImage().view(np.uint32), fixed_img.view(np.uint32))
    assert st["rounds"] == len(accs)
    assert st["pixel_samples"] == wl.width * wl.height * MAX_SPP
    assert st["blocks"] == -(-wl.width // 8) * -(-wl.height // 8)
    assert st["blocks_at_max"] == st["blocks"]
    assert (t.sampleCounts() == MAX_SPP).all()


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "arith%d-share%d" % m)
def test_truncation_identity_and_estimator(scene, mode):
    wl, t, (accs, halves) = configured(scene, mode)
    thr = pick_threshold(accs, halves)
    st = t.renderAdaptive(wl.camera, thr, batch=BATCH, min_spp=MIN_SPP, max_spp=MAX_SPP, block=BLOCK)
    got = read_accum(t)
    counts = t.sampleCounts()
    err = t.blockError()
    assert np.array_equal(counts, got[..., 3].astype(np.uint32))
    assert st["pixel_samples"] == int(counts.astype(np.int64).sum())

    # counts: uniform per block, within [min_spp, max_spp], whole rounds unless at max_spp
    blocks = block_of_pixels(counts, *BLOCK)
    bc = blocks.max(-1)
    assert ((blocks == bc[..., None]) | (blocks < 0)).all()
    assert (bc >= MIN_SPP).all() and (bc <= MAX_SPP).all()
    assert ((bc % BATCH == 0) | (bc == MAX_SPP)).all()
    assert st["rounds"] == -(-int(bc.max()) // BATCH)
    assert len(np.unique(bc)) > 1 or thr == 0      # the threshold was picked to stop some blocks early

    # every pixel holds the fixed sequence's accumulator after its own number of rounds, bit for bit
    rnd = -(-counts.astype(np.int64) // BATCH) - 1
    stack = np.stack(accs)
    expect = np.take_along_axis(stack, rnd[None, ..., None].repeat(4, -1), 0)[0]
    assert np.array_equal(got.view(np.uint32), expect.view(np.uint32))

    # the estimator: the device's block errors are the host's after each block's last round ...
    host = [None] + [A.block_error_reference(accs[k], halves[k], *BLOCK) for k in range(1, len(accs))]
    last = -(-bc // BATCH) - 1
    exp_err = np.choose(last, [np.zeros_like(host[1])] + host[1:])
    np.testing.assert_allclose(err, exp_err, rtol=1e-5, atol=1e-7)
    # ... every block that stopped below max_spp had converged ...
    below = bc < MAX_SPP
    assert (err[below] < thr).all()
    # ... and at every earlier round past min_spp a still-running block had not (ties within 1e-4 skipped)
    for k in range(1, len(accs)):
        if (k + 1) * BATCH < MIN_SPP:
            continue
        running = last > k
        e = host[k][running]
        near = np.abs(e - thr) <= 1e-4 * thr
        assert (e[~near] >= thr).all(), k
    assert st["blocks_at_max"] == int(((bc == MAX_SPP) & ~(err < thr)).sum())


def test_trivial_blocks_stop_at_min_spp():
    """Sky, a light and a mirror only: every pixel is finished in closed form (REC_FINAL), so all its samples are
    equal and every block stops as soon as it may."""
    s = rt.SceneCreator()
    s.addMaterial(A.T_LIGHT, (1.0, 0.9, 0.8), 0.0)
    s.addMaterial(A.T_REFLECTIVE, (0.8, 0.8, 0.9), 0.0)
    s.addSphere((0.0, 0.0, 6.0), 1.5, 0)
    s.addSphere((2.5, 0.5, 5.0), 1.0, 1)
    w, h = 120, 90
    cam = rt.workloads._camera(w, h, (0, 0, 0), 0.0)
    t = rt.RayTracer(w, h, scene=s, seed=cases.SEED)
    try:
        for arith, sharing in MODES:
            t.setArith(arith)
            t.setOption(t.OPT_PREFIX_SHARING, sharing)
            st = t.renderAdaptive(cam, 1e-3, batch=16, min_spp=48, max_spp=512, block=BLOCK)
            assert st["blocks_at_max"] == 0
            assert st["rounds"] == 3
            assert (t.sampleCounts() == 48).all()
            assert (t.blockError() < 1e-3).all()
    finally:
        t.close()


def test_masked_pixels_do_no_work():
    wl = rt.workloads.get("c1", width=160, height=120)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        for sharing in (1, 0):
            t.setOption(t.OPT_PREFIX_SHARING, sharing)
            t.enableCounters(True)
            t.resetCounters()
            st = t.renderAdaptive(wl.camera, 1e-3, batch=32, min_spp=64, max_spp=256, block=BLOCK)
            n = int(t.counters().samples)
            t.enableCounters(False)
            counts = t.sampleCounts()
            assert n == st["pixel_samples"] == int(counts.astype(np.int64).sum())
            assert n < wl.width * wl.height * 256      # the sky stopped at min_spp
            assert (counts == 64).any()
    finally:
        t.close()


def test_single_samples_match_the_accumulator(oracle, table):
    wl = rt.workloads.get("c2", width=160, height=90)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        st = t.renderAdaptive(wl.camera, 0.02, batch=32, min_spp=64, max_spp=200, block=BLOCK)
        assert st["rounds"] >= 2
        acc = read_accum(t)
        counts = t.sampleCounts()
        rng = np.random.RandomState(11)
        xs, ys = rng.randint(0, wl.width, 24), rng.randint(0, wl.height, 24)
        for x, y in zip(xs, ys):
            n = int(counts[y, x])
            ss = np.arange(n)
            got = t.traceSamples(wl.camera, np.full(n, x), np.full(n, y), ss)
            sub = rng.choice(n, 8, replace=False)
            exp, _ = oracle.samples(wl.scene, wl.camera, table, wl.width, wl.height, np.full(8, x), np.full(8, y), ss[sub])
            assert np.array_equal(got[sub].view(np.uint32), exp.view(np.uint32))
            np.testing.assert_allclose(acc[y, x, :3], got.astype(np.float64).sum(0), rtol=1e-6, atol=1e-6)
            assert acc[y, x, 3] == n
    finally:
        t.close()


def test_bad_arguments_leave_the_context_untouched():
    wl = rt.workloads.get("c1", width=64, height=48)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        with pytest.raises(rt.RtError) as ei:
            t.blockError()                            # no adaptive frame yet
        assert ei.value.code == -4
        t.renderFrame(wl.camera, 8)
        before = read_accum(t)
        good = dict(batch=16, min_spp=32, max_spp=64, block=(8, 8))
        bad = [dict(batch=0), dict(batch=513), dict(min_spp=16), dict(min_spp=40), dict(max_spp=31),
               dict(batch=512, min_spp=1024, max_spp=65537), dict(block=(6, 8)), dict(block=(8, 0)),
               dict(block=(512, 8))]
        for b in bad:
            kw = dict(good, **b)
            with pytest.raises(rt.RtError) as ei:
                t.renderAdaptive(wl.camera, 0.1, **kw)
            assert ei.value.code == -1, b
        for thr in (-1.0, float("nan"), float("inf")):
            with pytest.raises(rt.RtError) as ei:
                t.renderAdaptive(wl.camera, thr, **good)
            assert ei.value.code == -1, thr
        lib, ctx = t._lib, t._ctx
        cam = np.ascontiguousarray(wl.camera, dtype=np.float32)
        p = A.AdaptiveParams(16, 32, 64, 0.1, 8, 8)
        st = A.AdaptiveStats()
        assert lib.rt_render_adaptive(ctx, None, C.byref(p), C.byref(st)) == -1
        assert lib.rt_render_adaptive(ctx, cam.ctypes.data, None, C.byref(st)) == -1
        assert lib.rt_render_adaptive(ctx, cam.ctypes.data, C.byref(p), None) == -1
        t.setShard(0, 2, 8, 8)
        with pytest.raises(rt.RtError) as ei:
            t.renderAdaptive(wl.camera, 0.1, **good)
        assert ei.value.code == -1
        t.setShard(0, 1, 8, 8)
        assert np.array_equal(read_accum(t).view(np.uint32), before.view(np.uint32))
        with pytest.raises(rt.RtError):
            t.blockError()                            # still none
        out = np.empty(wl.width * wl.height - 1, np.uint32)
        assert lib.rt_read_sample_counts(ctx, out.ctypes.data, out.nbytes) == -1

        # a good call after the bad ones, then a resize forgets the block errors
        st = t.renderAdaptive(wl.camera, 0.1, **good)
        assert t.blockError().shape == (6, 8)
        t.resize(40, 30)
        with pytest.raises(rt.RtError) as ei:
            t.blockError()
        assert ei.value.code == -4
    finally:
        t.close()
