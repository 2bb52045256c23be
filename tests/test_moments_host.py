"""CPU: the per-pixel sample moments' surface that needs no device — the header in plain C, the exports, the merge rule
(rt_moments_merge is the very function the kernels call) against the float64 two-pass moment, the host restatement of
rt_denoise_moments (tests/moments_ref.py) against the one of rt_denoise_variance, rt_cli's --measured, and one
oracle-backed check that filtering on MEASURED variance beats the spatial estimate from 16 spp on."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import denoise_ref as R
import denoise_vg_ref as V
import moments_ref as M
from test_denoise_vg_host import gamma_rmse, primary_dirs

rt = cases.rt
A = rt._abi
ROOT = cases.ROOT
CLI = os.path.join(ROOT, "host", "rt_cli")
NEW = ("rt_read_moments", "rt_device_moments", "rt_moments_merge", "rt_denoise_moments")


def test_header_compiles_in_plain_c(built, tmp_path):
    src = tmp_path / "mom.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_amd.h"\n'
                   'int main(void) {\n'
                   '    rt_denoise_variance_params p = {5, 4.0f, 0.1f, 2.0f, 0.2f, RT_DENOISE_SPLIT_OBJECTS};\n'
                   '    float a[3] = {1.0f, 2.0f, 3.0f}, b[3] = {4.0f, 5.0f, 6.0f}, m[4], out = -1.0f; void *d = NULL;\n'
                   '    int rc = rt_moments_merge(0u, a, 7.0f, 3u, b, 0.25f, &out);\n'
                   '    printf("%d %d %u %d %d %d %d %.9g %d\\n", RT_OPT_MOMENTS, RT_ABI_VERSION, RT_DENOISE_MOMENTS_MIN_COUNT,\n'
                   '           rt_read_moments(NULL, m, sizeof m), rt_device_moments(NULL, &d), rt_denoise_moments(NULL, &p),\n'
                   '           rc, (double)out, rt_moments_merge(1u, a, 0.0f, 1u, NULL, 0.0f, &out));\n'
                   '    return 0;\n'
                   '}\n')
    exe = tmp_path / "mom"
    pkg = os.path.dirname(rt.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lrt_amd", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    # a NULL context / pointer is an error, not a crash; nA == 0 hands M2B back
    assert out.stdout.split() == ["12", "3", "4", "-1", "-1", "-1", "0", "0.25", "-1"]
    assert A.DENOISE_MOMENTS_MIN_COUNT == M.MIN_COUNT == 4


def test_library_exports_the_new_symbols(built):
    lib = C.CDLL(rt.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in rt.raytracer.SYMBOLS
    assert rt.load_library().rt_abi_version() == 3
    assert rt.raytracer.OPT_MOMENTS == rt.RayTracer.OPT_MOMENTS == 12
    for m in ("moments", "deviceMoments", "sampleVariance", "denoiseMoments", "denoiseMomentsOnDevice"):
        assert callable(getattr(rt.RayTracer, m))


# ---- the merge rule ----------------------------------------------------------------------------------------------------

def _fold(samples):
    """One-sample states folded in one after the other with rt_moments_merge; the running sum in float32 as the
    fixed-lane kernels keep it → float32 M2."""
    s = np.zeros(3, np.float32)
    m2 = np.float32(0)
    for k, x in enumerate(np.asarray(samples, np.float32)):
        m2 = rt.raytracer.moments_merge(k, s, m2, 1, x, 0.0)
        s = (s + x).astype(np.float32)
    return m2, s


def _radiances(rng, n, scale=1.0):
    # path-tracer-like: mostly dim, some bright, some exactly black
    x = (rng.random((n, 3)) ** 3 * scale).astype(np.float32)
    x[rng.random(n) < 0.2] = 0.0
    return x


def test_merge_with_an_empty_side_is_exact(built):
    f = np.float32
    a, b = np.array([0.3, 0.7, 0.1], f), np.array([9.0, 1.0, 4.0], f)
    for m2 in (0.0, 1e-30, 0.123456789, 3.5e7):
        assert rt.raytracer.moments_merge(0, a, 55.0, 7, b, m2) == f(m2)     # nA == 0: M2B, whatever the A side holds
        assert rt.raytracer.moments_merge(7, b, m2, 0, a, 55.0) == f(m2)     # nB == 0: M2A
    assert rt.raytracer.moments_merge(0, a, 1.0, 0, b, 2.0) == f(2.0)
    lib = rt.load_library()
    out = C.c_float()
    v = (C.c_float * 3)(1, 2, 3)
    assert lib.rt_moments_merge(1, None, 0.0, 1, v, 0.0, C.byref(out)) == -1
    assert lib.rt_moments_merge(1, v, 0.0, 1, v, 0.0, None) == -1


@pytest.mark.parametrize("n,scale", [(2, 1.0), (3, 1.0), (5, 40.0), (24, 1.0), (64, 1.0), (64, 300.0), (512, 1.0)])
def test_folding_single_samples_is_the_two_pass_moment(built, n, scale):
    rng = np.random.default_rng(1000 + n)
    for _ in range(8):
        x = _radiances(rng, n, scale)
        got, _ = _fold(x)
        ref = M.m2_two_pass(x)
        tol = M.tolerance(ref, n, (x.astype(np.float64) @ V.LUM).max())
        assert abs(float(got) - ref) <= tol, (got, ref, tol)
        xd, k = x.astype(np.float64), n // 2
        assert abs(M.merge(k, xd[:k].sum(0), M.m2_two_pass(xd[:k]), n - k, xd[k:].sum(0), M.m2_two_pass(xd[k:])) -
                   ref) <= 1e-9 * max(ref, 1e-30)   # the float64 rule itself


def test_any_split_into_two_launches_agrees_with_the_unsplit_value(built):
    rng = np.random.default_rng(64)
    x = _radiances(rng, 64, 2.0)
    ref = M.m2_two_pass(x)
    tol = M.tolerance(ref, 64, (x.astype(np.float64) @ V.LUM).max())
    whole, _ = _fold(x)
    assert abs(float(whole) - ref) <= tol
    for k in range(0, 65):
        (ma, sa), (mb, sb) = _fold(x[:k]), _fold(x[k:])
        got = rt.raytracer.moments_merge(k, sa, ma, 64 - k, sb, mb)
        assert abs(float(got) - ref) <= tol, (k, got, ref, tol)


def test_equal_samples_have_no_moment(built):
    f = np.float32
    x = np.tile(np.array([[0.9, 1.05, 0.8]], f), (64, 1))      # luminance about 1
    l = float(x[0].astype(np.float64) @ V.LUM)
    assert 0.9 < l < 1.1
    got, s = _fold(x)
    assert float(got) <= 64e-12
    a, b = _fold(x[:24]), _fold(x[24:])
    assert float(rt.raytracer.moments_merge(24, a[1], a[0], 40, b[1], b[0])) <= 64e-12
    # the form the header rules out, sum l^2 - n m^2 in binary32: four orders of magnitude above the bound
    lf = (f(0.2126) * x[:, 0] + f(0.7152) * x[:, 1] + f(0.0722) * x[:, 2]).astype(f)
    s1, s2 = f(0), f(0)
    for v in lf:
        s1, s2 = f(s1 + v), f(s2 + f(v * v))
    naive = abs(float(f(s2 - f(f(64) * f(f(s1 / f(64)) * f(s1 / f(64)))))))
    assert naive >= 1e4 * 64e-12, naive


# ---- the filter's restatement -------------------------------------------------------------------------------------------

def test_restatement_given_the_spatial_estimate_is_the_variance_guided_filter():
    h, w = 23, 37
    rng = np.random.default_rng(5)
    n = rng.integers(0, 9, size=(h, w)).astype(np.float32)
    acc = np.empty((h, w, 4), np.float32)
    acc[..., :3] = rng.random((h, w, 3), dtype=np.float32) * n[..., None]
    acc[..., 3] = n
    g = (rng.standard_normal((h, w, 3)).astype(np.float32), rng.standard_normal((h, w, 3)).astype(np.float32),
         rng.random((h, w, 3), dtype=np.float32), rng.random((h, w)) < 0.8, rng.integers(0, 3, (h, w)).astype(np.uint32))
    for kw in (dict(A.DENOISE_VARIANCE_DEFAULTS), dict(iterations=3, sigma_luminance=np.inf, sigma_normal=0.5),
               dict(iterations=1, sigma_luminance=1.0, split_objects=False)):
        c, v0, vl = V.filter_linear(acc, *g, **kw)
        assert np.array_equal(M.spatial_v0(acc, *g, **kw), v0)
        c2, vl2 = M.filter_linear_given_v0(acc, v0, *g, **kw)
        assert np.array_equal(c, c2) and np.array_equal(vl, vl2)
    # measured_v0: the threshold, n = 0 included
    m2 = rng.random((h, w))
    v = M.measured_v0(m2, n, v0)
    assert np.array_equal(v[n < 4], v0[n < 4]) and np.array_equal(v[n >= 4], m2[n >= 4] / (n * (n - 1.0))[n >= 4])
    assert (n == 0).any() and (n >= 4).any()


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_measured_variance_beats_the_spatial_estimate_from_16spp(name, oracle, table):
    w, h = 128, 72
    wl = rt.workloads.get(name, width=w, height=h)
    cam = rt.raytracer._cam_block(wl.camera)
    truth = oracle.linear_sum(wl.scene, cam, table, w, h, (0, 0, w, h), 0, 1024) / 1024.0
    rays = np.concatenate([np.repeat(cam[None, :3], w * h, 0), primary_dirs(cam, w, h).reshape(-1, 3)], axis=1)
    o = oracle.hit(3, wl.scene, rays.astype(np.float32), np.zeros(w * h, np.uint32))
    hit = (o[:, 0] > 0).reshape(h, w)
    mat = np.where(hit.reshape(-1), o[:, 11].copy().view(np.uint32), A.NO_ID).astype(np.uint32)
    colour = wl.scene.materials["color"][np.where(hit.reshape(-1), mat, 0), :3]
    g = (np.where(hit[..., None], o[:, 5:8].reshape(h, w, 3), 0), np.where(hit[..., None], o[:, 2:5].reshape(h, w, 3), 0),
         np.where(hit[..., None], colour.reshape(h, w, 3), 0), hit, mat.reshape(h, w))
    kw = dict(A.DENOISE_VARIANCE_DEFAULTS)
    ys, xs = np.mgrid[0:h, 0:w]
    spp = 64
    s, _ = oracle.samples(wl.scene, cam, table, w, h, np.repeat(xs.reshape(-1), spp), np.repeat(ys.reshape(-1), spp),
                          np.tile(np.arange(spp), w * h))
    s = s.reshape(h, w, spp, 3)
    for n, bound in ((16, 1.0), (64, 0.85)):
        part = s[:, :, :n].astype(np.float64)
        acc = np.concatenate([part.sum(2), np.full((h, w, 1), float(n))], axis=-1).astype(np.float32)
        spatial, v0, _ = V.filter_linear(acc, *g, **kw)
        measured, _ = M.filter_linear_given_v0(acc, M.measured_v0(M.m2_two_pass(part), acc[..., 3], v0), *g, **kw)
        plain = R.atrous_linear(acc, *g, **A.DENOISE_DEFAULTS)
        e_noisy, e_plain = gamma_rmse(R.initial_colour(acc), truth), gamma_rmse(plain, truth)
        e_spatial, e_measured = gamma_rmse(spatial, truth), gamma_rmse(measured, truth)
        print("%s %d spp %dx%d gamma RMSE: noisy %.4f, rt_denoise %.4f, spatial variance %.4f, measured variance %.4f "
              "(measured / spatial %.2f)" % (name, n, w, h, e_noisy, e_plain, e_spatial, e_measured, e_measured / e_spatial))
        if n == 16:
            assert e_measured < e_spatial
        else:
            assert e_measured <= bound * e_spatial


# ---- rt_cli -------------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([CLI, "--scene", os.path.join(ROOT, "assets", "scenes", "c1_sphere.scene"), *args],
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [
    ["--denoise", "--variance-guided", "--measured"],
    ["--measured", "--variance-guided", "--denoise", "--sigma-luminance", "8", "--aov", "aov"],
    ["--adaptive", "0.05", "--denoise", "--variance-guided", "--measured"],
])
def test_cli_accepts_measured(built, tmp_path, args):
    out = _cli(*args, "--dump-scene", str(tmp_path / "scene.bin"))
    assert out.returncode == 0, out.stderr
    assert (tmp_path / "scene.bin").stat().st_size > 0


def test_cli_measured_fails_on_the_missing_device_not_on_usage(built, tmp_path):
    try:
        rt.RayTracer(8, 8).close()
        device = True
    except rt.RtError as e:
        assert e.code == -2     # RT_ENODEVICE
        device = False
    out = _cli("--size", "16x12", "--spp", "4", "--denoise", "--variance-guided", "--measured")
    assert out.returncode != 2 and "usage" not in out.stderr, (out.returncode, out.stderr)
    assert (out.returncode == 0) == device, (out.returncode, out.stderr)


@pytest.mark.parametrize("args", [
    ["--measured"],
    ["--denoise", "--measured"],                                     # without --variance-guided
    ["--variance-guided", "--measured"],                             # without --denoise
    ["--denoise", "--variance-guided", "--measured=1"],
])
def test_cli_rejects_measured_alone(built, tmp_path, args):
    out = _cli(*args, "--dump-scene", str(tmp_path / "scene.bin"))
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "--measured" in out.stderr
