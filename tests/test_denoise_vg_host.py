"""CPU: the variance-guided denoiser's surface that needs no device — the header's rt_denoise_variance_params in plain
C, the exports, rt_cli's new flags, the properties of the host restatement (tests/denoise_vg_ref.py) that
tests/test_gpu_denoise_vg.py checks the device against, and one oracle-backed check that the formulation beats the
plain à-trous filter on a 1-spp frame."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import denoise_ref as R
import denoise_vg_ref as V

rt = cases.rt
A = rt._abi
ROOT = cases.ROOT
CLI = os.path.join(ROOT, "host", "rt_cli")
NEW = ("rt_denoise_variance", "rt_read_variance", "rt_device_variance")


def test_header_compiles_in_plain_c_with_the_params_layout(built, tmp_path):
    src = tmp_path / "vg.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_amd.h"\n'
                   'int main(void) {\n'
                   '    rt_denoise_variance_params p = {5, 4.0f, 0.1f, 2.0f, 0.2f, RT_DENOISE_SPLIT_OBJECTS};\n'
                   '    float v[4]; void *d = NULL;\n'
                   '    printf("%zu %zu %d %d %d %.17g %d %d\\n", sizeof p, sizeof(rt_denoise_params),\n'
                   '           rt_denoise_variance(NULL, &p), rt_read_variance(NULL, 0, v, sizeof v),\n'
                   '           rt_device_variance(NULL, 1, &d), (double)RT_DENOISE_VARIANCE_EPS,\n'
                   '           (int)offsetof(rt_denoise_variance_params, sigma_luminance),\n'
                   '           (int)offsetof(rt_denoise_variance_params, flags));\n'
                   '    return 0;\n'
                   '}\n')
    exe = tmp_path / "vg"
    pkg = os.path.dirname(rt.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lrt_amd", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.split()
    assert got[:5] == ["24", "24", "-1", "-1", "-1"]      # a NULL context is an error, not a crash
    assert float(got[5]) == float(np.float32(1e-4)) == V.EPS and got[6:] == ["4", "20"]
    assert C.sizeof(A.DenoiseVarianceParams) == 24
    assert A.DenoiseVarianceParams.sigma_luminance.offset == 4 and A.DenoiseVarianceParams.flags.offset == 20
    assert A.DENOISE_VARIANCE_DEFAULTS == dict(iterations=5, sigma_luminance=4.0, sigma_normal=0.1, sigma_position=2.0,
                                               sigma_albedo=0.2, split_objects=True)
    assert rt.load_library().rt_abi_version() == 3


def test_library_exports_the_new_symbols(built):
    lib = C.CDLL(rt.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in rt.raytracer.SYMBOLS
    assert rt.load_library().rt_denoise_variance.argtypes is not None
    for m in ("denoiseVariance", "denoiseVarianceOnDevice", "variance"):
        assert callable(getattr(rt.RayTracer, m))


def _cli(*args):
    return subprocess.run([CLI, "--scene", os.path.join(ROOT, "assets", "scenes", "c1_sphere.scene"), *args],
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [
    ["--denoise", "--variance-guided"],
    ["--variance-guided", "--denoise", "--sigma-luminance", "8"],
    ["--denoise", "--variance-guided", "--sigma-luminance=inf", "--denoise-iterations", "3"],
    ["--denoise", "--variance-guided", "--sigma", "0.5,0.1,inf,0.2", "--sigma-luminance", "1e-3"],
    ["--adaptive", "0.05", "--denoise", "--variance-guided", "--aov", "aov"],
    ["--denoise", "--progressive", "--variance-guided"],
])
def test_cli_accepts_variance_guided_flags(built, tmp_path, args):
    out = _cli(*args, "--dump-scene", str(tmp_path / "scene.bin"))
    assert out.returncode == 0, out.stderr
    assert (tmp_path / "scene.bin").stat().st_size > 0


@pytest.mark.parametrize("args", [
    ["--variance-guided"],                                           # without --denoise
    ["--variance-guided", "--sigma-luminance", "4"],
    ["--sigma-luminance", "4"],
    ["--denoise", "--sigma-luminance", "4"],                         # without --variance-guided
    ["--denoise", "--variance-guided", "--sigma-luminance", "0"],
    ["--denoise", "--variance-guided", "--sigma-luminance", "-1"],
    ["--denoise", "--variance-guided", "--sigma-luminance", "nan"],
    ["--denoise", "--variance-guided", "--sigma-luminance", "4x"],
    ["--denoise", "--variance-guided", "--sigma-luminance", ""],
    ["--denoise", "--variance-guided", "--sigma-luminance", "4,4"],
    ["--denoise", "--variance-guided=1"],
    ["--denoise", "--variance-guided", "--sigma", "0.5,0.5,0.5"],
    ["--denoise", "--variance-guided", "--denoise-iterations", "9"],
])
def test_cli_rejects_bad_variance_guided_flags(built, tmp_path, args):
    out = _cli(*args, "--dump-scene", str(tmp_path / "scene.bin"))
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "--denoise" in out.stderr


def _frame(h=23, w=37, seed=1):
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 9, size=(h, w)).astype(np.float32)
    acc = np.empty((h, w, 4), np.float32)
    acc[..., :3] = rng.random((h, w, 3), dtype=np.float32) * n[..., None]
    acc[..., 3] = n
    return acc, rng


def _guides(h, w, rng, hit=None, obj=None):
    return dict(normal=rng.standard_normal((h, w, 3)).astype(np.float32),
                position=rng.standard_normal((h, w, 3)).astype(np.float32),
                albedo=rng.random((h, w, 3), dtype=np.float32),
                hit=np.ones((h, w), bool) if hit is None else hit,
                object=np.zeros((h, w), np.uint32) if obj is None else obj)


def _run(acc, g, **kw):
    return V.filter_linear(acc, g["normal"], g["position"], g["albedo"], g["hit"], g["object"], **kw)


@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_restatement_keeps_a_constant_image_constant(iterations):
    h, w = 29, 41
    acc, rng = _frame(h, w)
    acc[..., :3] = np.float32(0.25) * acc[..., 3:4]         # c0 = 0.25 everywhere, exactly
    g = _guides(h, w, rng, obj=rng.integers(0, 3, (h, w)).astype(np.uint32))
    c, v0, vl = _run(acc, g, iterations=iterations, sigma_luminance=4.0, sigma_normal=0.5, sigma_position=0.7,
                     sigma_albedo=0.2)
    # (the weighted mean of equal float64 values may round one ulp off them: v0 <= (2^-53)^2, not 0 to the bit)
    assert v0.max() <= 1e-30 and vl.max() <= 1e-30
    assert np.abs(c - R.initial_colour(acc)).max() <= 1e-15


def _b3_squared(v, iterations):
    """The variance that the plain B3 à-trous blur carries along: at step s the stencil h (x) h dilated by s with the
    in-frame weights renormalised, applied to v with the SQUARED normalised weights."""
    v = np.asarray(v, dtype=np.float64)
    h, w = v.shape
    for i in range(iterations):
        s = 1 << i
        k = np.outer(R.H5, R.H5)
        pad = 2 * s
        P = np.zeros((h + 2 * pad, w + 2 * pad))
        M = np.zeros((h + 2 * pad, w + 2 * pad))
        P[pad:pad + h, pad:pad + w] = v
        M[pad:pad + h, pad:pad + w] = 1.0
        num = np.zeros((h, w))
        den = np.zeros((h, w))
        for a in range(5):
            for b in range(5):
                oy, ox = pad + (a - 2) * s, pad + (b - 2) * s
                num += k[a, b] ** 2 * P[oy:oy + h, ox:ox + w]
                den += k[a, b] * M[oy:oy + h, ox:ox + w]
        v = num / den ** 2
    return v


@pytest.mark.parametrize("iterations", [1, 2, 4, 6])
def test_restatement_without_edge_terms_is_the_b3_blur(iterations):
    h, w = 37, 53   # smaller than 2 * 2^5 in one direction: most taps of the late steps fall outside the frame
    acc, rng = _frame(h, w, seed=iterations)
    g = _guides(h, w, rng)
    c, v0, vl = _run(acc, g, iterations=iterations, split_objects=False)
    assert np.abs(c - R.b3_blur(R.initial_colour(acc), iterations)).max() <= 1e-12
    assert np.abs(vl - _b3_squared(v0, iterations)).max() <= 1e-12
    # and v0 is then the plain (1/n-normalised) variance of the luminance over the in-frame 7x7 window
    l = V.luminance(R.initial_colour(acc))
    assert abs(v0[10, 20] - l[7:14, 17:24].var()) <= 1e-12
    assert abs(v0[0, 0] - l[0:4, 0:4].var()) <= 1e-12
    assert abs(v0[h - 1, w - 2] - l[h - 4:h, w - 5:w].var()) <= 1e-12


def test_restatement_never_mixes_hit_and_miss_pixels():
    h, w = 31, 47
    acc, rng = _frame(h, w, seed=7)
    hit = rng.random((h, w)) < 0.5
    acc[~hit, :3] = 0.0        # the sky is black
    g = _guides(h, w, rng, hit=hit, obj=np.where(hit, 5, A.NO_ID).astype(np.uint32))
    for split in (True, False):
        kw = dict(iterations=5, sigma_luminance=4.0, sigma_normal=2.0, split_objects=split)
        c, v0, vl = _run(acc, g, **kw)
        assert (c[~hit] == 0).all() and (v0[~hit] == 0).all() and (vl[~hit] == 0).all()
        # brighten the misses' input and no hit pixel moves, neither its colour nor its variances
        acc2 = acc.copy()
        acc2[~hit, :3] = 7.0 * acc2[~hit, 3:4]
        c2, v02, vl2 = _run(acc2, g, **kw)
        assert np.array_equal(c[hit], c2[hit]) and np.array_equal(v0[hit], v02[hit])
        # (the unit-neighbour blur vt_p has no edge stopping, but the misses' variance stays 0: a flat region)
        assert np.array_equal(vl[hit], vl2[hit])
        assert np.allclose(c2[~hit], 7.0)


def test_restatement_estimates_the_variance_of_gaussian_noise():
    h = w = 64
    s = 0.05
    rng = np.random.default_rng(20171)
    acc = np.empty((h, w, 4), np.float32)
    grey = (0.5 + s * rng.standard_normal((h, w))).astype(np.float32)
    acc[..., :3] = grey[..., None]      # l(c) = grey: the luminance weights sum to 1
    acc[..., 3] = 1.0
    g = _guides(h, w, rng)
    for k in ("normal", "position", "albedo"):
        g[k][:] = g[k][0, 0]            # constant guides
    _, v0, _ = _run(acc, g, iterations=1, sigma_luminance=4.0, sigma_normal=0.1, sigma_position=2.0, sigma_albedo=0.2)
    # the 49-tap estimate is biased by 1/49 (less at the frame's edge); the sampling error at 64 x 64 is about 2 %
    assert abs(v0.mean() / s ** 2 - 1.0) <= 0.10


def test_output_is_gamma_with_alpha_and_zero_without_samples():
    h, w = 12, 14
    acc, rng = _frame(h, w, seed=4)
    acc[3, 4] = 0.0
    g = _guides(h, w, rng)
    out, v0, vl = V.filter_frame(acc, g, iterations=2, sigma_luminance=4.0)
    lin, v0b, vlb = _run(acc, g, iterations=2, sigma_luminance=4.0)
    assert (out[3, 4] == 0).all()
    has = acc[..., 3] > 0
    assert np.allclose(out[has, :3] ** 2, lin[has]) and (out[has, 3] == 1).all()
    assert np.array_equal(v0, v0b) and np.array_equal(vl, vlb) and (vl >= 0).all() and (v0 >= 0).all()


def primary_dirs(cam, w, h):
    """primary_ray's direction under policy IEEE in float32: normalize(ver * t + (hor * s + llc))."""
    f = np.float32
    ys, xs = np.mgrid[0:h, 0:w]
    s = (xs.astype(f) / f(w))[..., None]
    tt = (ys.astype(f) / f(h))[..., None]
    llc, hor, ver = cam[3:6], cam[6:9], cam[9:12]
    v = (ver * tt + (hor * s + llc).astype(f)).astype(f)
    d2 = ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]).astype(f) + v[..., 2] * v[..., 2]).astype(f)
    return (v / np.sqrt(d2)[..., None]).astype(f)


def gamma_rmse(lin, truth):
    return float(np.sqrt(((np.sqrt(lin) - np.sqrt(truth)) ** 2).mean()))


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_variance_guided_beats_the_plain_filter_at_1spp(name, oracle, table):
    w, h = 128, 72
    wl = rt.workloads.get(name, width=w, height=h)
    cam = rt.raytracer._cam_block(wl.camera)
    one = oracle.linear_sum(wl.scene, cam, table, w, h, (0, 0, w, h), 0, 1)
    truth = oracle.linear_sum(wl.scene, cam, table, w, h, (0, 0, w, h), 0, 256) / 256.0
    acc = np.concatenate([one, np.ones((h, w, 1))], axis=-1).astype(np.float32)
    rays = np.concatenate([np.repeat(cam[None, :3], w * h, 0), primary_dirs(cam, w, h).reshape(-1, 3)], axis=1)
    o = oracle.hit(3, wl.scene, rays.astype(np.float32), np.zeros(w * h, np.uint32))
    hit = (o[:, 0] > 0).reshape(h, w)
    mat = np.where(hit.reshape(-1), o[:, 11].copy().view(np.uint32), A.NO_ID).astype(np.uint32)
    colour = wl.scene.materials["color"][np.where(hit.reshape(-1), mat, 0), :3]
    g = dict(normal=np.where(hit[..., None], o[:, 5:8].reshape(h, w, 3), 0),
             position=np.where(hit[..., None], o[:, 2:5].reshape(h, w, 3), 0),
             albedo=np.where(hit[..., None], colour.reshape(h, w, 3), 0), hit=hit, object=mat.reshape(h, w))
    kw = dict(A.DENOISE_VARIANCE_DEFAULTS)
    vg, v0, vl = _run(acc, g, **kw)
    plain = R.atrous_linear(acc, g["normal"], g["position"], g["albedo"], g["hit"], g["object"], **A.DENOISE_DEFAULTS)
    e_noisy, e_plain, e_vg = gamma_rmse(R.initial_colour(acc), truth), gamma_rmse(plain, truth), gamma_rmse(vg, truth)
    print("%s 1 spp %dx%d gamma RMSE: noisy %.4f, rt_denoise defaults %.4f, variance-guided %.4f" %
          (name, w, h, e_noisy, e_plain, e_vg))
    assert e_vg < e_plain
