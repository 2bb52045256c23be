"""GPU (-m gpu): first-hit feature buffers (rt_render_features) and the edge-avoiding à-trous denoiser (rt_denoise).
The features must be, bit for bit, what rt_debug_hit(kind 3) returns for (camera origin, the record's direction)
under every arithmetic policy; the filter must follow the header's statement (tests/denoise_ref.py); and neither call
may touch the image, the accumulator or the sample counter."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import denoise_ref as R

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
ROOT = cases.ROOT
CLI = os.path.join(ROOT, "host", "rt_cli")
ASSETS = os.path.join(ROOT, "assets")
POLICIES = (rt.ARITH_IEEE, rt.ARITH_ROCM_OCL_NOCONTRACT, rt.ARITH_ROCM_OCL)
EINVAL, ESTATE = -1, -4

SCENES = {
    "c1": lambda: rt.workloads.get("c1", width=96, height=80),
    "c2": lambda: rt.workloads.get("c2", width=244, height=138),
    "c3": lambda: rt.workloads.get("c3", width=200, height=130, tex_size=256),   # textured cube
    "c4": lambda: rt.workloads.get("c4", width=160, height=96, n_spheres=3000),   # sphere BVH
    "c5": lambda: rt.workloads.get("c5", width=96, height=64),                     # mesh BVH
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def cam_block(wl):
    return rt.raytracer._cam_block(wl.camera)


def read_accum(t):
    import torch
    t.sync()
    return torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().copy()


def primary_dirs(cam, w, h):
    """primary_ray's direction under policy 0 in float32: normalize(ver * t + (hor * s + llc)), dot = (x² + y²) + z²,
    correctly rounded sqrt and divisions."""
    f = np.float32
    ys, xs = np.mgrid[0:h, 0:w]
    s = (xs.astype(f) / f(w))[..., None]
    tt = (ys.astype(f) / f(h))[..., None]
    llc, hor, ver = cam[3:6], cam[6:9], cam[9:12]
    v = (ver * tt + (hor * s + llc).astype(f)).astype(f)
    d2 = ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]).astype(f) + v[..., 2] * v[..., 2]).astype(f)
    return (v / np.sqrt(d2)[..., None]).astype(f)


def texel(scene, u, v, tex):
    """texture_rgb (pt_device.hpp) on the host in float32: bilinear, edge clamp."""
    f = np.float32
    T = scene.textures
    layers, H, W = T.shape[:3]
    layer = np.where(tex < layers, tex, 0)
    # the texel coordinate, clamped to [-1, W] before floor, NaN counts as -1
    with np.errstate(invalid="ignore", over="ignore"):
        uu, vv = (u * f(W) - f(0.5)).astype(f), (v * f(H) - f(0.5)).astype(f)
        uu = np.where(uu >= -1, np.where(uu > f(W), f(W), uu), f(-1)).astype(f)
        vv = np.where(vv >= -1, np.where(vv > f(H), f(H), vv), f(-1)).astype(f)
    fu, fv = np.floor(uu), np.floor(vv)
    a, b = (uu - fu).astype(f), (vv - fv).astype(f)
    i0, j0 = fu.astype(np.int64), fv.astype(np.int64)
    i1, j1 = np.clip(i0 + 1, 0, W - 1), np.clip(j0 + 1, 0, H - 1)
    i0, j0 = np.clip(i0, 0, W - 1), np.clip(j0, 0, H - 1)
    t00, t10, t01, t11 = (T[layer, jj, ii, :3] for jj, ii in ((j0, i0), (j0, i1), (j1, i0), (j1, i1)))
    w00, w10, w01, w11 = ((f(1) - a) * (f(1) - b))[:, None], (a * (f(1) - b))[:, None], ((f(1) - a) * b)[:, None], (a * b)[:, None]
    return ((((w00 * t00).astype(f) + (w10 * t10).astype(f)).astype(f) + (w01 * t01).astype(f)).astype(f)
            + (w11 * t11).astype(f)).astype(f)


@pytest.fixture(scope="module", params=sorted(SCENES))
def scene(request):
    wl = SCENES[request.param]()
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    yield request.param, wl, t
    t.setArith(rt.ARITH_IEEE)
    t.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_features_equal_the_hit_probe_bit_for_bit(scene, policy, oracle):
    name, wl, t = scene
    t.setArith(policy)
    cam = cam_block(wl)
    t.renderFeatures(wl.camera)
    rec = t.featureRecords().reshape(-1)
    n = len(rec)
    hit = (rec["flags"] & A.FEATURE_HIT) != 0
    assert hit.any() and (rec["flags"] & ~np.uint32(A.FEATURE_HIT) == 0).all()
    rays = np.concatenate([np.repeat(cam[None, :3], n, 0), rec["dir"]], axis=1).astype(np.float32)
    probe = t.debugHit(3, rays)
    assert np.array_equal(probe[:, 0] > 0, hit)
    h = probe[hit]
    r = rec[hit]
    assert np.array_equal(bits(r["t"]), bits(h[:, 1]))
    assert np.array_equal(bits(r["pos"]), bits(h[:, 2:5]))
    assert np.array_equal(bits(r["normal"]), bits(h[:, 5:8]))
    assert np.array_equal(bits(r["u"]), bits(h[:, 8])) and np.array_equal(bits(r["v"]), bits(h[:, 9]))
    assert np.array_equal(r["tex"], bits(h[:, 10])) and np.array_equal(r["material"], bits(h[:, 11]))
    # the miss records
    m = rec[~hit]
    assert (m["t"] == np.inf).all() and (m["pos"] == 0).all() and (m["normal"] == 0).all() and (m["albedo"] == 0).all()
    assert (m["object"] == A.NO_ID).all() and (m["material"] == A.NO_ID).all() and (m["face"] == A.NO_ID).all()
    assert (m["u"] == 0).all() and (m["v"] == 0).all() and (m["tex"] == 0).all()
    # faces: mesh hits only
    kind = r["object"] >> 30
    assert (r["face"][kind != 3] == A.NO_ID).all()
    if (kind == 3).any():
        assert (r["face"][kind == 3] < np.max(wl.scene.meshes["face_count"])).all()
    # albedo: the material colour, or the path's texel
    mats = wl.scene.materials
    typ = mats["type"][r["material"]]
    tx = typ == A.T_TEXTURED
    assert np.array_equal(bits(r["albedo"][~tx]), bits(mats["color"][r["material"][~tx], :3]))
    if tx.any():
        assert np.array_equal(bits(r["albedo"][tx]), bits(texel(wl.scene, r["u"][tx], r["v"][tx], r["tex"][tx])))
    if name == "c3":
        assert tx.any()
    if policy == rt.ARITH_IEEE:
        dirs = primary_dirs(cam, wl.width, wl.height).reshape(-1, 3)
        assert np.array_equal(bits(rec["dir"]), bits(dirs))
        # and the CPU oracle's hitScene on a sample of the pixels
        sel = np.random.default_rng(5).choice(n, size=min(n, 1500), replace=False)
        o = oracle.hit(3, wl.scene, rays[sel], np.zeros(len(sel), np.uint32))
        assert np.array_equal(o[:, 0] > 0, hit[sel])
        oh, rs = o[hit[sel]], rec[sel][hit[sel]]
        assert np.array_equal(bits(rs["t"]), bits(oh[:, 1]))
        assert np.array_equal(bits(rs["pos"]), bits(oh[:, 2:5])) and np.array_equal(bits(rs["normal"]), bits(oh[:, 5:8]))
        assert np.array_equal(rs["material"], bits(oh[:, 11]))
        mesh = (rs["object"] >> 30) == 3
        assert np.array_equal(bits(rs["u"][mesh]), bits(oh[mesh, 8])) and np.array_equal(rs["tex"][mesh], bits(oh[mesh, 10]))
    assert t.walkOverflow() == 0


def test_object_ids_are_consistent(scene):
    name, wl, t = scene
    t.setArith(rt.ARITH_IEEE)
    t.renderFeatures(wl.camera)
    r = t.featureRecords().reshape(-1)
    r = r[(r["flags"] & A.FEATURE_HIT) != 0]
    kind, idx = r["object"] >> 30, r["object"] & 0x3FFFFFFF
    s = wl.scene
    for k, arr in ((0, s.spheres), (1, s.planes), (2, s.lenses)):
        sel = kind == k
        if sel.any():
            assert (idx[sel] < len(arr)).all()
            assert np.array_equal(arr["mat_ID"][idx[sel]], r["material"][sel]), k
    sel = kind == 3
    if sel.any():
        models = s.models
        for mi, mat in zip(idx[sel], r["material"][sel]):
            owner = (models["mesh_anchor"] <= mi) & (mi < models["mesh_anchor"] + models["mesh_count"])
            assert owner.any() and mat in models["mat_ID"][owner]
    sel = kind == 0
    if sel.any():
        # relative to the magnitudes the float32 hit point o + t d is formed from (|o| + t), and to the radius
        sp = s.spheres[idx[sel]]
        d = np.linalg.norm(r["pos"][sel].astype(np.float64) - sp["pos"][:, :3], axis=1)
        scale = np.linalg.norm(cam_block(wl)[:3]) + r["t"][sel] + sp["r"]
        # (near-grazing hits lose digits in the discriminant b*b - c of the reference's root: most hits, not all)
        err = np.abs(d - sp["r"]) / scale
        assert (err <= 1e-5).mean() >= 0.95 and (err <= 1e-3).all()   # C4 (3 000 small spheres): 97.7 %


@pytest.fixture(scope="module")
def c2():
    wl = rt.workloads.get("c2", width=244, height=138)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    yield wl, t
    t.close()


def test_nothing_else_moves(c2):
    wl, t = c2
    t.renderFrame(wl.camera, 4)
    t.render(wl.camera)
    t.renderAgain(wl.camera)
    img0, acc0, cnt0 = t.transferImage(), read_accum(t), t.sample_counter
    t.renderFeatures(wl.camera)
    t.denoiseOnDevice(iterations=5)
    t.sync()
    img1, acc1, cnt1 = t.transferImage(), read_accum(t), t.sample_counter
    assert img0.tobytes() == img1.tobytes() and acc0.tobytes() == acc1.tobytes() and cnt0 == cnt1 == 1
    buf = np.empty_like(img0)
    assert t._lib.rt_read_image(t._ctx, buf.ctypes.data, buf.nbytes) == 0
    assert buf.tobytes() == img0.tobytes()


SIGMAS = {
    "default": dict(),
    "all_inf": dict(sigma_color=np.inf, sigma_normal=np.inf, sigma_position=np.inf, sigma_albedo=np.inf),
    "no_split": dict(split_objects=False),
}


def _against_restatement(t, wl, iterations=5, **kw):
    args = dict(A.DENOISE_DEFAULTS)
    args.update(iterations=iterations)
    args.update(kw)
    acc = read_accum(t)
    t.renderFeatures(wl.camera)
    feats = t.features()
    got = t.denoise(**args)
    exp = R.atrous(acc, feats, **args)
    has = acc[..., 3] > 0
    assert np.array_equal(got[~has], np.zeros_like(got[~has]))
    assert (got[has, 3] == 1).all()
    lin_got = got[has, :3].astype(np.float64) ** 2
    assert np.abs(lin_got - exp[has, :3] ** 2).max() <= 2e-5
    miss = has & ~feats["hit"]
    assert (got[miss, :3] == 0).all()


@pytest.mark.parametrize("sig", sorted(SIGMAS))
def test_filter_matches_the_restatement_c2(c2, sig):
    wl, t = c2
    t.renderFrame(wl.camera, 4)
    _against_restatement(t, wl, **SIGMAS[sig])


@pytest.mark.parametrize("iterations", [1, 3, 8])
def test_filter_matches_the_restatement_iterations(c2, iterations):
    wl, t = c2
    t.renderFrame(wl.camera, 4)
    _against_restatement(t, wl, iterations=iterations, sigma_color=0.3)


def test_filter_matches_the_restatement_adaptive(c2):
    wl, t = c2
    t.renderAdaptive(wl.camera, 0.05, batch=4, min_spp=8, max_spp=32)
    counts = t.sampleCounts()
    assert len(np.unique(counts)) > 1
    for sig in sorted(SIGMAS):
        _against_restatement(t, wl, **SIGMAS[sig])


@pytest.mark.parametrize("sig", sorted(SIGMAS))
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
    """Frames smaller than a tile, than the halo and than the late steps: staging, the out-of-frame key and the empty
    tiles of the sparse classes."""
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
def test_denoised_16spp_is_closer_to_the_truth(name):
    wl = rt.workloads.get(name, width=256, height=144)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        truth = t.renderFrame(wl.camera, 2048)
        noisy = t.renderFrame(wl.camera, 16)
        den = t.denoise(camera=wl.camera)
        assert gamma_rmse(den, truth) < gamma_rmse(noisy, truth)
    finally:
        t.close()


def test_error_cases():
    wl = rt.workloads.get("c2", width=64, height=40)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    lib, ctx = t._lib, t._ctx
    try:
        P = A.DenoiseParams
        ok = P(5, 0.5, 0.5, 0.5, 0.2, A.DENOISE_SPLIT_OBJECTS)
        img = np.empty((wl.height, wl.width, 4), np.float32)
        feats = np.empty((wl.height, wl.width), A.FEATURE)
        d = C.c_void_p()
        # nothing made yet
        assert lib.rt_denoise(ctx, C.byref(ok)) == ESTATE
        assert lib.rt_read_features(ctx, feats.ctypes.data, feats.nbytes) == ESTATE
        assert lib.rt_device_features(ctx, C.byref(d)) == ESTATE
        assert lib.rt_read_denoised(ctx, img.ctypes.data, img.nbytes) == ESTATE
        assert lib.rt_device_denoised(ctx, C.byref(d)) == ESTATE
        t.renderFrame(wl.camera, 2)
        t.renderFeatures(wl.camera)
        # bad arguments
        for it in (0, 9, 100):
            assert lib.rt_denoise(ctx, C.byref(P(it, 0.5, 0.5, 0.5, 0.2, 1))) == EINVAL, it
        for k in range(4):
            for bad in (0.0, -1.0, float("nan"), -np.inf):
                s = [0.5, 0.5, 0.5, 0.2]
                s[k] = bad
                assert lib.rt_denoise(ctx, C.byref(P(5, *s, 1))) == EINVAL, (k, bad)
        assert lib.rt_denoise(ctx, C.byref(P(5, 0.5, 0.5, 0.5, 0.2, 2))) == EINVAL
        assert lib.rt_denoise(ctx, None) == EINVAL
        assert lib.rt_render_features(ctx, None) == EINVAL
        assert lib.rt_read_features(ctx, None, feats.nbytes) == EINVAL
        assert lib.rt_read_features(ctx, feats.ctypes.data, feats.nbytes - 80) == EINVAL
        assert lib.rt_device_features(ctx, None) == EINVAL
        assert lib.rt_read_denoised(ctx, None, img.nbytes) == EINVAL
        assert lib.rt_device_denoised(ctx, None) == EINVAL
        assert lib.rt_denoise(None, C.byref(ok)) == EINVAL
        # still nothing denoised: the failed calls made nothing
        assert lib.rt_read_denoised(ctx, img.ctypes.data, img.nbytes) == ESTATE
        assert lib.rt_denoise(ctx, C.byref(P(1, np.inf, np.inf, np.inf, np.inf, 0))) == 0
        assert lib.rt_read_denoised(ctx, img.ctypes.data, img.nbytes) == 0
        assert lib.rt_device_denoised(ctx, C.byref(d)) == 0 and d.value
        assert lib.rt_device_features(ctx, C.byref(d)) == 0 and d.value
        # a sharded context
        t.setShard(0, 2)
        assert lib.rt_render_features(ctx, cam_block(wl).ctypes.data) == EINVAL
        assert lib.rt_denoise(ctx, C.byref(ok)) == EINVAL
        t.setShard(0, 1)
        assert lib.rt_denoise(ctx, C.byref(ok)) == 0
        # after rt_resize nothing is left
        t.resize(wl.width + 8, wl.height)
        img = np.empty((wl.height, wl.width + 8, 4), np.float32)
        feats = np.empty((wl.height, wl.width + 8), A.FEATURE)
        assert lib.rt_denoise(ctx, C.byref(ok)) == ESTATE
        assert lib.rt_read_features(ctx, feats.ctypes.data, feats.nbytes) == ESTATE
        assert lib.rt_read_denoised(ctx, img.ctypes.data, img.nbytes) == ESTATE
        with pytest.raises(rt.RtError):
            t.denoise()
    finally:
        t.close()


def test_second_render_features_replaces_the_first(c2):
    wl, t = c2
    other = rt.workloads.get("c2", width=244, height=138)
    other_cam = rt.Camera(60, np.float32(244) / np.float32(138), (-7, -1, -9), 30.0, 5.0)
    t.renderFeatures(wl.camera)
    a = t.featureRecords()
    t.renderFeatures(other_cam)
    b = t.featureRecords()
    u = rt.RayTracer(other.width, other.height, scene=other.scene, seed=cases.SEED)
    try:
        u.renderFeatures(other_cam)
        assert u.featureRecords().tobytes() == b.tobytes()
    finally:
        u.close()
    assert a.tobytes() != b.tobytes()


def test_python_denoise_with_camera_equals_the_two_calls(c2):
    wl, t = c2
    other_cam = rt.Camera(60, np.float32(244) / np.float32(138), (-7, -1, -9), 30.0, 5.0)
    t.renderFrame(wl.camera, 8)
    t.renderFeatures(other_cam)
    one = t.denoise(camera=wl.camera)
    t.renderFeatures(other_cam)
    t.renderFeatures(wl.camera)
    t.denoiseOnDevice()
    two = t.denoisedImage()
    assert one.tobytes() == two.tobytes()
    f = t.features()
    assert set(f) >= {"position", "depth", "normal", "albedo", "object", "material", "face", "direction", "uv", "hit"}
    assert f["position"].shape == (138, 244, 3) and f["uv"].shape == (138, 244, 2) and f["hit"].dtype == bool


@pytest.mark.parametrize("mode", ["fixed", "progressive", "adaptive"])
def test_cli_denoise_matches_python_path(built, mode, tmp_path):
    w, h, spp = 200, 120, 8
    scene = "c2_cornell.scene"
    raw = str(tmp_path / "f.f32")
    aov = str(tmp_path / "aov")
    cmd = [CLI, "--scene", os.path.join(ASSETS, "scenes", scene), "--size", "%dx%d" % (w, h), "--spp", str(spp),
           "--camera=-8,-1,-8,45,0", "--raw", raw, "--denoise", "--aov", aov]
    if mode == "progressive":
        cmd.append("--progressive")
    if mode == "adaptive":
        cmd += ["--adaptive", "0.05", "--batch", "4", "--min-spp", "8", "--spp", "32"]
    subprocess.run(cmd, check=True, cwd=ROOT)
    got = np.fromfile(raw, np.float32).reshape(h, w, 4)
    s = rt.SceneCreator()
    s.loadScene(os.path.join(ASSETS, "scenes", scene), base_dir=ASSETS)
    t = rt.RayTracer(w, h, scene=s)
    try:
        cam = rt.Camera(60, np.float32(w) / np.float32(h), (-8, -1, -8), 45.0, 0.0)
        if mode == "adaptive":
            t.renderAdaptive(cam, 0.05, batch=4, min_spp=8, max_spp=32)
        else:
            t.renderFrame(cam, spp)
        exp = t.denoise(camera=cam)
        f = t.features()
    finally:
        t.close()
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    for name, arr, ch in (("normal", f["normal"], 3), ("albedo", f["albedo"], 3), ("depth", f["depth"], 1)):
        pfm = open(aov + "_%s.pfm" % name, "rb").read()
        head = b"%s\n%d %d\n-1.0\n" % (b"PF" if ch == 3 else b"Pf", w, h)
        assert pfm.startswith(head)
        data = np.frombuffer(pfm[len(head):], np.float32)
        assert np.array_equal(data.view(np.uint32), np.ascontiguousarray(arr, np.float32).reshape(-1).view(np.uint32))
