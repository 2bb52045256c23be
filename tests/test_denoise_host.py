"""CPU: the feature-buffer / denoiser surface that needs no device — the header's rt_feature and rt_denoise_params in
plain C, the exports, the Python dtype, rt_cli's new flags, and the host restatement of the filter
(tests/denoise_ref.py) that tests/test_gpu_denoise.py checks the device against."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import denoise_ref as R

rt = cases.rt
A = rt._abi
ROOT = cases.ROOT
CLI = os.path.join(ROOT, "host", "rt_cli")
NEW = ("rt_render_features", "rt_read_features", "rt_device_features", "rt_denoise", "rt_read_denoised",
       "rt_device_denoised")
OFFSETS = {"pos": 0, "t": 12, "normal": 16, "object": 28, "albedo": 32, "material": 44, "dir": 48, "face": 60,
           "u": 64, "v": 68, "tex": 72, "flags": 76}


def test_header_compiles_in_plain_c_with_the_feature_layout(built, tmp_path):
    src = tmp_path / "features.c"
    offs = " ".join("(int)offsetof(rt_feature, %s)," % f for f in OFFSETS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_amd.h"\n'
                   'int main(void) {\n'
                   '    rt_denoise_params p = {5, 0.5f, 0.5f, 0.5f, 0.2f, RT_DENOISE_SPLIT_OBJECTS};\n'
                   '    rt_feature f[1]; float img[4]; void *d = NULL;\n'
                   '    int o[] = {%s};\n'
                   '    size_t k;\n'
                   '    printf("%%zu %%zu %%d %%d %%d %%d %%d %%d", sizeof(rt_feature), sizeof p,\n'
                   '           rt_render_features(NULL, NULL), rt_read_features(NULL, f, sizeof f),\n'
                   '           rt_device_features(NULL, &d), rt_denoise(NULL, &p), rt_read_denoised(NULL, img, sizeof img),\n'
                   '           rt_device_denoised(NULL, &d));\n'
                   '    for (k = 0; k < sizeof o / sizeof o[0]; k++) printf(" %%d", o[k]);\n'
                   '    printf("\\n");\n'
                   '    return 0;\n'
                   '}\n' % offs)
    exe = tmp_path / "features"
    pkg = os.path.dirname(rt.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lrt_amd", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.split()
    assert got[:8] == ["80", "24"] + ["-1"] * 6      # a NULL context is an error, not a crash
    assert [int(v) for v in got[8:]] == list(OFFSETS.values())
    assert C.sizeof(A.DenoiseParams) == 24


def test_feature_dtype_matches_the_header():
    assert A.FEATURE.itemsize == 80
    for name, off in OFFSETS.items():
        assert A.FEATURE.fields[name][1] == off, name


def test_library_exports_the_new_symbols(built):
    lib = C.CDLL(rt.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in rt.raytracer.SYMBOLS
    assert rt.load_library().rt_denoise.argtypes is not None


def _cli(*args):
    return subprocess.run([CLI, "--scene", os.path.join(ROOT, "assets", "scenes", "c1_sphere.scene"), *args],
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [
    ["--denoise"],
    ["--denoise", "--denoise-iterations", "1"],
    ["--denoise", "--denoise-iterations=8", "--sigma", "0.5,0.1,inf,0.2"],
    ["--denoise", "--progressive", "--sigma=1e-3,2,3,4"],
    ["--adaptive", "0.05", "--denoise", "--aov", "aov"],
    ["--aov", "x"],
])
def test_cli_accepts_denoise_flags(built, tmp_path, args):
    out = _cli(*args, "--dump-scene", str(tmp_path / "scene.bin"))
    assert out.returncode == 0, out.stderr
    assert (tmp_path / "scene.bin").stat().st_size > 0


@pytest.mark.parametrize("args", [
    ["--denoise", "--denoise-iterations", "0"],
    ["--denoise", "--denoise-iterations", "9"],
    ["--denoise", "--denoise-iterations", "2x"],
    ["--denoise", "--denoise-iterations", ""],
    ["--denoise", "--sigma", "0.5,0.5,0.5"],
    ["--denoise", "--sigma", "0.5,0.5,0.5,0.5,0.5"],
    ["--denoise", "--sigma", "0.5,0,0.5,0.5"],
    ["--denoise", "--sigma", "0.5,-1,0.5,0.5"],
    ["--denoise", "--sigma", "nan,1,1,1"],
    ["--denoise", "--sigma", "1,1,1,x"],
    ["--denoise", "--sigma", "1;1;1;1"],
    ["--denoise", "--sigma", "1,1,1,1,"],
    ["--denoise-iterations", "3"],                 # denoise-only flags without --denoise
    ["--sigma", "1,1,1,1"],
    ["--aov="],
])
def test_cli_rejects_bad_denoise_flags(built, tmp_path, args):
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


@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_restatement_keeps_a_constant_image_constant(iterations):
    h, w = 29, 41
    acc, rng = _frame(h, w)
    acc[..., :3] = np.float32(0.3) * acc[..., 3:4]          # c0 = 0.3 everywhere (up to float32 division)
    g = _guides(h, w, rng, obj=rng.integers(0, 3, (h, w)).astype(np.uint32))
    out = R.atrous_linear(acc, g["normal"], g["position"], g["albedo"], g["hit"], g["object"], iterations=iterations,
                          sigma_color=0.1, sigma_normal=0.5, sigma_position=0.7, sigma_albedo=0.2)
    assert np.abs(out - R.initial_colour(acc)).max() <= 1e-6


@pytest.mark.parametrize("iterations", [1, 2, 4, 6])
def test_restatement_without_edge_terms_is_the_b3_blur(iterations):
    h, w = 37, 53   # smaller than 2 * 2^5 in one direction: most taps of the late steps fall outside the frame
    acc, rng = _frame(h, w, seed=iterations)
    g = _guides(h, w, rng)
    for split in (True, False):
        out = R.atrous_linear(acc, g["normal"], g["position"], g["albedo"], g["hit"], g["object"],
                              iterations=iterations, split_objects=split)
        assert np.abs(out - R.b3_blur(R.initial_colour(acc), iterations)).max() <= 1e-12


def test_restatement_never_mixes_hit_and_miss_pixels():
    h, w = 31, 47
    acc, rng = _frame(h, w, seed=7)
    hit = rng.random((h, w)) < 0.5
    acc[~hit, :3] = 0.0        # the sky is black
    g = _guides(h, w, rng, hit=hit, obj=np.where(hit, 5, A.NO_ID).astype(np.uint32))
    for split in (True, False):
        out = R.atrous_linear(acc, g["normal"], g["position"], g["albedo"], g["hit"], g["object"], iterations=5,
                              split_objects=split)
        assert (out[~hit] == 0).all()
        # and a hit pixel only ever averages hit pixels: brighten the misses' input and nothing on the hits moves
        acc2 = acc.copy()
        acc2[~hit, :3] = 7.0 * acc2[~hit, 3:4]
        out2 = R.atrous_linear(acc2, g["normal"], g["position"], g["albedo"], g["hit"], g["object"], iterations=5,
                               split_objects=split)
        assert np.array_equal(out[hit], out2[hit])
        assert np.allclose(out2[~hit], 7.0)


def test_restatement_split_objects_keeps_objects_apart():
    h, w = 20, 30
    acc, rng = _frame(h, w, seed=3)
    obj = np.where(np.arange(w)[None, :] < 13, 1, 2).astype(np.uint32).repeat(h, 0)
    acc[obj[..., None].repeat(4, -1)[..., 0] == 2, :3] = 0.0
    g = _guides(h, w, rng, obj=obj)
    out = R.atrous_linear(acc, g["normal"], g["position"], g["albedo"], g["hit"], g["object"], iterations=4)
    assert (out[obj == 2] == 0).all() and (out[obj == 1] > 0).all()
    mixed = R.atrous_linear(acc, g["normal"], g["position"], g["albedo"], g["hit"], g["object"], iterations=4,
                            split_objects=False)
    assert (mixed[obj == 2] > 0).any()


def test_output_is_gamma_with_alpha_and_zero_without_samples():
    h, w = 12, 14
    acc, rng = _frame(h, w, seed=4)
    acc[3, 4] = 0.0
    g = _guides(h, w, rng)
    out = R.atrous(acc, g, iterations=2, sigma_color=1.0)
    lin = R.atrous_linear(acc, g["normal"], g["position"], g["albedo"], g["hit"], g["object"], iterations=2,
                          sigma_color=1.0)
    assert (out[3, 4] == 0).all()
    has = acc[..., 3] > 0
    assert np.allclose(out[has, :3] ** 2, lin[has]) and (out[has, 3] == 1).all()
