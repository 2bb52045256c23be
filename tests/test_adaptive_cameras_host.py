"""CPU: adaptive sampling through per-sample cameras (rt_render_adaptive_cameras) — what needs no device: the header's
declaration as plain C, the export and its ctypes prototype, and rt_cli's argument rules for --adaptive-cameras."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases

rt = cases.rt
A = rt._abi
ROOT = cases.ROOT
CLI = os.path.join(ROOT, "host", "rt_cli")
SYMBOL = "rt_render_adaptive_cameras"


def test_header_declares_the_call_in_plain_c(built, tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include <stdio.h>\n#include "rt_amd.h"\n'
                   'int main(void) {\n'
                   '    rt_adaptive_params p = {64, 128, 1024, 0.01f, 8, 8};\n'
                   '    rt_adaptive_stats s = {0, 0, 0, 0};\n'
                   '    static float cams[12 * 1024];\n'
                   '    int (*f)(rt_context *, const float *, uint32_t, const rt_adaptive_params *, rt_adaptive_stats *) =\n'
                   '        rt_render_adaptive_cameras;\n'
                   '    printf("%d\\n", f(NULL, cams, 1024u, &p, &s));\n'
                   '    return 0;\n'
                   '}\n')
    exe = tmp_path / "use"
    pkg = os.path.dirname(rt.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lrt_amd", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["-1"]          # a NULL context is RT_EINVAL, not a crash


def test_library_exports_the_symbol_and_abi_binds_it(built):
    assert hasattr(C.CDLL(rt.LIB_PATH), SYMBOL)
    assert SYMBOL in rt.raytracer.SYMBOLS
    lib = rt.load_library()
    vp = C.c_void_p
    assert lib.rt_render_adaptive_cameras.argtypes == [vp, vp, C.c_uint32, C.POINTER(A.AdaptiveParams), C.POINTER(A.AdaptiveStats)]
    p, st = A.AdaptiveParams(64, 128, 1024, 0.01, 8, 8), A.AdaptiveStats()
    cams = np.zeros((1024, 12), np.float32)
    assert lib.rt_render_adaptive_cameras(None, cams.ctypes.data, 1024, C.byref(p), C.byref(st)) == -1
    assert callable(rt.RayTracer.renderAdaptiveCameras)


def _cli(tmp_path, *args):
    # --dump-scene is the host-only mode: the arguments are parsed and checked, no device is needed
    return subprocess.run([CLI, "--scene", os.path.join(ROOT, "assets", "scenes", "c1_sphere.scene"), *args,
                           "--dump-scene", str(tmp_path / "scene.bin")], capture_output=True, text=True, timeout=120)


LENS = ["--aperture", "0.1", "--focus", "4"]


@pytest.mark.parametrize("args", [
    ["--aa", "--adaptive-cameras", "0.05"],
    ["--aa", "--adaptive-cameras=0", "--batch", "8", "--min-spp", "16", "--spp", "40", "--counts", "c.u32"],
    LENS + ["--adaptive-cameras", "0.01", "--batch", "32", "--spp", "100"],
    ["--aa"] + LENS + ["--adaptive-cameras", "0.01", "--batch", "512", "--spp", "65536"],
    ["--aa", "--adaptive-cameras", "0.02", "--denoise", "--aa-guides", "16", "--aov", "x"],
])
def test_cli_accepts_adaptive_cameras(built, tmp_path, args):
    out = _cli(tmp_path, *args)
    assert out.returncode == 0, out.stderr
    assert (tmp_path / "scene.bin").stat().st_size > 0


@pytest.mark.parametrize("args", [
    ["--adaptive-cameras", "0.05"],                                          # no per-sample cameras to adapt
    ["--adaptive-cameras", "0.05", "--batch", "16"],
    ["--aa", "--adaptive-cameras", "0.05", "--progressive"],
    ["--aa", "--adaptive-cameras", "0.05", "--adaptive", "0.05"],
    LENS + ["--adaptive-cameras", "0.05", "--adaptive", "0.05"],
    ["--aa", "--adaptive-cameras", "-1"],                                    # bad numbers
    ["--aa", "--adaptive-cameras", "nan"],
    ["--aa", "--adaptive-cameras", "inf"],
    ["--aa", "--adaptive-cameras", "x"],
    ["--aa", "--adaptive-cameras", "0.1", "--batch", "0"],
    ["--aa", "--adaptive-cameras", "0.1", "--batch", "513", "--spp", "2048"],
    ["--aa", "--adaptive-cameras", "0.1", "--batch", "16", "--min-spp", "24"],
    ["--aa", "--adaptive-cameras", "0.1", "--batch", "16", "--min-spp", "16"],
    ["--aa", "--adaptive-cameras", "0.1", "--batch", "16", "--min-spp", "64", "--spp", "32"],
    ["--aa", "--adaptive-cameras", "0.1", "--batch", "512", "--spp", "65537"],
    ["--aa", "--batch", "16"],                                               # adaptive-only flags with neither adaptive flag
    ["--aa", "--min-spp", "32"],
    ["--aa", "--counts", "c.pgm"],
    ["--batch", "16"],
])
def test_cli_rejects_bad_adaptive_cameras_flags(built, tmp_path, args):
    out = _cli(tmp_path, *args)
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "usage" in out.stderr and "--adaptive-cameras THRESHOLD" in out.stderr      # the usage text names the flag
    assert not (tmp_path / "scene.bin").exists()


def test_cli_still_refuses_one_camera_adaptive_with_per_sample_cameras(built, tmp_path):
    for flags in (["--aa", "--adaptive", "0.01"], LENS + ["--adaptive", "0.01"], ["--aa", "--progressive"]):
        out = _cli(tmp_path, *flags)
        assert out.returncode == 2 and "use --spp" in out.stderr and "usage" not in out.stderr, (flags, out.stderr)
