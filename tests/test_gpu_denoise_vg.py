"""GPU (-m gpu): the variance-guided denoiser (rt_denoise_variance: pt_dn_variance + pt_atrous_vg).  The device must
follow the header's statement (tests/denoise_vg_ref.py) in colour and in both variance buffers, beat rt_denoise at 1
and 4 spp, and touch nothing but the denoise buffers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import denoise_vg_ref as V

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
ROOT = cases.ROOT
CLI = os.path.join(ROOT, "host", "rt_cli")
ASSETS = os.path.join(ROOT, "assets")
EINVAL, ESTATE = -1, -4
INF = np.inf


def cam_block(wl):
    return rt.raytracer._cam_block(wl.camera)


def read_accum(t):
    import torch
    t.sync()
    return torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().copy()


@pytest.fixture(scope="module")
def c2():
    wl = rt.workloads.get("c2", width=244, height=138)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    yield wl, t
    t.close()


SIGMAS = {
    "default": dict(),
    "all_inf": dict(sigma_luminance=INF, sigma_normal=INF, sigma_position=INF, sigma_albedo=INF),
    "no_split": dict(split_objects=False),
}


def _against_restatement(t, wl, iterations=5, **kw):
    args = dict(A.DENOISE_VARIANCE_DEFAULTS)
    args.update(iterations=iterations)
    args.update(kw)
    acc = read_accum(t)
    t.renderFeatures(wl.camera)
    feats = t.features()
    got = t.denoiseVariance(**args)
    v0, vl = t.variance(0), t.variance(1)
    exp, v0_ref, vl_ref = V.filter_frame(acc, feats, **args)
    has = acc[..., 3] > 0
    assert np.array_equal(got[~has], np.zeros_like(got[~has]))
    assert (got[has, 3] == 1).all()
    lin_got = got[has, :3].astype(np.float64) ** 2
    e_c = np.abs(lin_got - exp[has, :3] ** 2).max() if has.any() else 0.0
    e_v0 = (np.abs(v0 - v0_ref) / np.maximum(1.0, v0_ref)).max()
    e_vl = (np.abs(vl - vl_ref) / np.maximum(1.0, vl_ref)).max()
    print("%dx%d L=%d %s: linear colour %.3g, v0 %.3g, v(L) %.3g (bound 2e-5 each)" %
          (wl.width, wl.height, iterations, kw, e_c, e_v0, e_vl))
    assert e_c <= 2e-5
    assert e_v0 <= 2e-5 and e_vl <= 2e-5
    miss = has & ~feats["hit"]
    sky = got[miss, :3]
    if miss.any() and (acc[miss, :3] == 0).all():      # a black sky stays black: no hit pixel leaked into it
        assert (sky == 0).all()
    return got, acc, feats


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("sig", sorted(SIGMAS))
def test_filter_matches_the_restatement_c2(c2, sig, spp):
    wl, t = c2
    t.renderFrame(wl.camera, spp)
    _against_restatement(t, wl, **SIGMAS[sig])


@pytest.mark.parametrize("iterations", [1, 3, 8])
def test_filter_matches_the_restatement_iterations(c2, iterations):
    wl, t = c2
    t.renderFrame(wl.camera, 4)
    _against_restatement(t, wl, iterations=iterations)


def test_filter_matches_the_restatement_adaptive(c2):
    wl, t = c2
    t.renderAdaptive(wl.camera, 0.05, batch=4, min_spp=8, max_spp=32)
    counts = t.sampleCounts()
    assert len(np.unique(counts)) > 1
    for sig in sorted(SIGMAS):
        _against_restatement(t, wl, **SIGMAS[sig])


def test_miss_pixels_never_mix_with_hits(c2):
    """Brighten the misses in the accumulator's stead: with the hit pixels' keys apart from the misses', a second run
    whose sky is 7 gives the same hit pixels to the bit and a sky of exactly 7."""
    import torch
    wl, t = c2
    t.renderFrame(wl.camera, 4)
    t.renderFeatures(wl.camera)
    hit = t.features()["hit"]
    assert hit.any() and (~hit).any()
    one = t.denoiseVariance()
    assert (one[~hit, :3] == 0).all()      # the sky of C2 is black, so its variance is 0 before and after
    acc = torch.as_tensor(t.deviceAccum(), device="cuda")
    keep = acc.clone()
    m = torch.as_tensor(~hit, device="cuda")
    try:
        acc[..., :3][m] = 7.0 * acc[..., 3:4].expand(-1, -1, 3)[m]
        torch.cuda.synchronize()
        two = t.denoiseVariance()
    finally:
        acc.copy_(keep)
        torch.cuda.synchronize()
    assert np.array_equal(one[hit].view(np.uint32), two[hit].view(np.uint32))
    assert np.abs(two[~hit, :3].astype(np.float64) ** 2 - 7.0).max() <= 1e-5


@pytest.mark.parametrize("sig", ["default", "all_inf"])
def test_filter_matches_the_restatement_c3(sig):
    wl = rt.workloads.get("c3", width=200, height=130, tex_size=256)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        t.renderFrame(wl.camera, 4)
        _against_restatement(t, wl, **SIGMAS[sig])
    finally:
        t.close()


@pytest.mark.parametrize("size", [(37, 23), (7, 5), (1, 1)])
def test_filter_matches_the_restatement_on_tiny_frames(size):
    """Frames smaller than a tile, than the 7x7 window and than the late steps: staging and the in-frame
    renormalisation."""
    wl = rt.workloads.get("c2", width=size[0], height=size[1])
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        t.renderFrame(wl.camera, 4)
        for sig in sorted(SIGMAS):
            _against_restatement(t, wl, **SIGMAS[sig])
        _against_restatement(t, wl, iterations=8)
    finally:
        t.close()


def gamma_rmse(a, b):
    return float(np.sqrt(((a[..., :3].astype(np.float64) - b[..., :3]) ** 2).mean()))


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_variance_guided_beats_the_plain_filter_at_low_counts(name):
    """RMSE(denoiseVariance) < RMSE(denoise) at 1 and 4 spp, and <= 0.5 x at 1 spp (the CPU restatement of the issue
    measured 0.27 and 0.26 there)."""
    wl = rt.workloads.get(name, width=256, height=144)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        truth = t.renderFrame(wl.camera, 2048)
        for spp in (1, 4):
            noisy = t.renderFrame(wl.camera, spp)
            plain = t.denoise(camera=wl.camera)
            vg = t.denoiseVariance()
            e_n, e_p, e_v = gamma_rmse(noisy, truth), gamma_rmse(plain, truth), gamma_rmse(vg, truth)
            print("%s %d spp gamma RMSE: noisy %.4f, denoise %.4f, denoiseVariance %.4f (ratio %.3f)" %
                  (name, spp, e_n, e_p, e_v, e_v / e_p))
            assert e_v < e_p
            if spp == 1:
                assert e_v <= 0.5 * e_p
    finally:
        t.close()


def test_nothing_else_moves(c2):
    wl, t = c2
    t.renderFrame(wl.camera, 4)
    t.render(wl.camera)
    t.renderAgain(wl.camera)
    t.renderFeatures(wl.camera)
    img0, acc0, cnt0, rec0 = t.transferImage(), read_accum(t), t.sample_counter, t.featureRecords()
    plain0 = t.denoise()
    t.denoiseVarianceOnDevice()
    t.sync()
    vg0, va0, vb0 = t.denoisedImage(), t.variance(0), t.variance(1)
    img1, acc1, cnt1, rec1 = t.transferImage(), read_accum(t), t.sample_counter, t.featureRecords()
    assert img0.tobytes() == img1.tobytes() and acc0.tobytes() == acc1.tobytes() and cnt0 == cnt1 == 1
    assert rec0.tobytes() == rec1.tobytes()
    buf = np.empty_like(img0)
    assert t._lib.rt_read_image(t._ctx, buf.ctypes.data, buf.nbytes) == 0
    assert buf.tobytes() == img0.tobytes()
    assert vg0.tobytes() != plain0.tobytes()
    # the two filters share the ping-pong and the output buffer and leave nothing behind for each other
    assert t.denoise().tobytes() == plain0.tobytes()
    assert t.denoiseVariance().tobytes() == vg0.tobytes()
    assert t.variance(0).tobytes() == va0.tobytes() and t.variance(1).tobytes() == vb0.tobytes()
    assert t.denoiseVariance().tobytes() == vg0.tobytes()


def test_variance_first_then_denoise():
    """rt_denoise_variance as the context's FIRST denoise call makes the buffers rt_denoise needs as well."""
    wl = rt.workloads.get("c2", width=64, height=40)
    a = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    b = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        for t in (a, b):
            t.renderFrame(wl.camera, 2)
            t.renderFeatures(wl.camera)
        va = a.denoiseVariance()
        pa = a.denoise()
        pb = b.denoise()
        vb = b.denoiseVariance()
        assert va.tobytes() == vb.tobytes() and pa.tobytes() == pb.tobytes()
        d = a.deviceVariance(0)
        assert d and d != a.deviceVariance(1)
    finally:
        a.close()
        b.close()


def test_error_cases():
    wl = rt.workloads.get("c2", width=64, height=40)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    lib, ctx = t._lib, t._ctx
    try:
        P = A.DenoiseVarianceParams
        ok = P(5, 4.0, 0.5, 0.5, 0.2, A.DENOISE_SPLIT_OBJECTS)
        var = np.empty((wl.height, wl.width), np.float32)
        img = np.empty((wl.height, wl.width, 4), np.float32)
        d = C.c_void_p()
        # nothing made yet
        assert lib.rt_denoise_variance(ctx, C.byref(ok)) == ESTATE
        for which in (0, 1):
            assert lib.rt_read_variance(ctx, which, var.ctypes.data, var.nbytes) == ESTATE
            assert lib.rt_device_variance(ctx, which, C.byref(d)) == ESTATE
        t.renderFrame(wl.camera, 2)
        t.renderFeatures(wl.camera)
        # bad arguments
        for it in (0, 9, 100):
            assert lib.rt_denoise_variance(ctx, C.byref(P(it, 4.0, 0.5, 0.5, 0.2, 1))) == EINVAL, it
        for k in range(4):
            for bad in (0.0, -1.0, float("nan"), -np.inf):
                s = [4.0, 0.5, 0.5, 0.2]
                s[k] = bad
                assert lib.rt_denoise_variance(ctx, C.byref(P(5, *s, 1))) == EINVAL, (k, bad)
        assert lib.rt_denoise_variance(ctx, C.byref(P(5, 4.0, 0.5, 0.5, 0.2, 2))) == EINVAL
        assert lib.rt_denoise_variance(ctx, None) == EINVAL
        assert lib.rt_denoise_variance(None, C.byref(ok)) == EINVAL
        assert lib.rt_read_variance(ctx, 2, var.ctypes.data, var.nbytes) == EINVAL
        assert lib.rt_read_variance(ctx, -1, var.ctypes.data, var.nbytes) == EINVAL
        assert lib.rt_read_variance(ctx, 0, None, var.nbytes) == EINVAL
        assert lib.rt_read_variance(ctx, 0, var.ctypes.data, var.nbytes - 4) == EINVAL
        assert lib.rt_device_variance(ctx, 2, C.byref(d)) == EINVAL
        assert lib.rt_device_variance(ctx, 0, None) == EINVAL
        # still nothing filtered: the failed calls made nothing, and rt_denoise makes no variance
        assert lib.rt_read_variance(ctx, 0, var.ctypes.data, var.nbytes) == ESTATE
        assert lib.rt_read_denoised(ctx, img.ctypes.data, img.nbytes) == ESTATE
        t.denoiseOnDevice()
        assert lib.rt_read_variance(ctx, 0, var.ctypes.data, var.nbytes) == ESTATE
        assert lib.rt_device_variance(ctx, 1, C.byref(d)) == ESTATE
        assert lib.rt_denoise_variance(ctx, C.byref(P(1, INF, INF, INF, INF, 0))) == 0
        for which in (0, 1):
            assert lib.rt_read_variance(ctx, which, var.ctypes.data, var.nbytes) == 0
            assert lib.rt_device_variance(ctx, which, C.byref(d)) == 0 and d.value
        assert lib.rt_read_denoised(ctx, img.ctypes.data, img.nbytes) == 0
        # a sharded context
        t.setShard(0, 2)
        assert lib.rt_denoise_variance(ctx, C.byref(ok)) == EINVAL
        t.setShard(0, 1)
        assert lib.rt_denoise_variance(ctx, C.byref(ok)) == 0
        # after rt_resize nothing is left
        t.resize(wl.width + 8, wl.height)
        var = np.empty((wl.height, wl.width + 8), np.float32)
        assert lib.rt_denoise_variance(ctx, C.byref(ok)) == ESTATE
        assert lib.rt_read_variance(ctx, 0, var.ctypes.data, var.nbytes) == ESTATE
        assert lib.rt_device_variance(ctx, 0, C.byref(d)) == ESTATE
        with pytest.raises(rt.RtError):
            t.denoiseVariance()
        with pytest.raises(rt.RtError):
            t.variance(1)
    finally:
        t.close()


def test_cli_variance_guided_matches_python_path(built, tmp_path):
    w, h, spp = 200, 120, 8
    scene = "c2_cornell.scene"
    raw = str(tmp_path / "f.f32")
    aov = str(tmp_path / "aov")
    cmd = [CLI, "--scene", os.path.join(ASSETS, "scenes", scene), "--size", "%dx%d" % (w, h), "--spp", str(spp),
           "--camera=-8,-1,-8,45,0", "--raw", raw, "--denoise", "--variance-guided", "--aov", aov]
    subprocess.run(cmd, check=True, cwd=ROOT)
    got = np.fromfile(raw, np.float32).reshape(h, w, 4)
    s = rt.SceneCreator()
    s.loadScene(os.path.join(ASSETS, "scenes", scene), base_dir=ASSETS)
    t = rt.RayTracer(w, h, scene=s)
    try:
        cam = rt.Camera(60, np.float32(w) / np.float32(h), (-8, -1, -8), 45.0, 0.0)
        t.renderFrame(cam, spp)
        exp = t.denoiseVariance(camera=cam)
        v0 = t.variance(0)
        plain = t.denoise()
    finally:
        t.close()
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert not np.array_equal(got.view(np.uint32), plain.view(np.uint32))
    pfm = open(aov + "_variance.pfm", "rb").read()
    head = b"Pf\n%d %d\n-1.0\n" % (w, h)
    assert pfm.startswith(head)
    data = np.frombuffer(pfm[len(head):], np.float32)
    assert np.array_equal(data.view(np.uint32), v0.reshape(-1).view(np.uint32))
    assert os.path.isfile(aov + "_normal.pfm") and os.path.isfile(aov + "_depth.pfm")
