"""CPU: progressive anti-aliasing (rt_render_again_cameras) — what needs no device: the header as plain C, the export and
its ctypes prototype, RT_AGAIN_CAMERAS_MAX in the header and in _abi, the C++ façade's renderAgainCameras, and rt_cli's
argument rules for --progressive-cameras."""
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
SYMBOL = "rt_render_again_cameras"
PKG = os.path.dirname(rt.LIB_PATH)
LINK = ["-L", PKG, "-lrt_amd", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
LINK_HOST = LINK + ["-lz"]          # (host/scene.cpp reads PNGs)


def test_header_is_plain_c_and_a_null_context_is_einval(built, tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include <stdio.h>\n#include "rt_amd.h"\n'
                   'int main(void) {\n'
                   '    static float cams[12 * 3];\n'
                   '    int (*f)(rt_context *, const float *, uint32_t) = rt_render_again_cameras;\n'
                   '    printf("%d %u %d\\n", f(NULL, cams, 3u), (unsigned)RT_AGAIN_CAMERAS_MAX, RT_ABI_VERSION);\n'
                   '    return 0;\n'
                   '}\n')
    exe = tmp_path / "use"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)] + LINK, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["-1", "4096", "3"]        # RT_EINVAL, not a crash; the cap; the ABI version stays


def test_library_exports_the_symbol_and_abi_binds_it(built):
    assert hasattr(C.CDLL(rt.LIB_PATH), SYMBOL)
    assert SYMBOL in rt.raytracer.SYMBOLS
    lib = rt.load_library()
    assert lib.rt_render_again_cameras.argtypes == [C.c_void_p, C.c_void_p, C.c_uint32]
    cams = np.zeros((3, 12), np.float32)
    assert lib.rt_render_again_cameras(None, cams.ctypes.data, 3) == -1
    assert A.AGAIN_CAMERAS_MAX == 4096
    assert callable(rt.RayTracer.renderAgainCameras)
    assert lib.rt_abi_version() == 3


def test_cpp_facade_compiles_and_links(built, tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "raytracer.h"\n'
                   'int main(int argc, char **) {\n'
                   '    void (RayTracer::*f)(const std::vector<float> &) = &RayTracer::renderAgainCameras;\n'
                   '    if (argc > 100) {\n'
                   '        RayTracer t(8, 8, "kernels/raytracer.cl");\n'
                   '        (t.*f)(std::vector<float>(36, 0.0f));\n'
                   '    }\n'
                   '    return f ? 0 : 1;\n'
                   '}\n')
    exe = tmp_path / "use"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"),
                    str(src), os.path.join(ROOT, "host", "librt_host.a"), "-o", str(exe)] + LINK_HOST, check=True)
    assert subprocess.run([str(exe)], timeout=120).returncode == 0


def _cli(tmp_path, *args):
    # --dump-scene is the host-only mode: the arguments are parsed and checked, no device is needed
    return subprocess.run([CLI, "--scene", os.path.join(ROOT, "assets", "scenes", "c1_sphere.scene"), *args,
                           "--dump-scene", str(tmp_path / "scene.bin")], capture_output=True, text=True, timeout=120)


LENS = ["--aperture", "0.1", "--focus", "4"]


@pytest.mark.parametrize("args", [
    ["--aa", "--progressive-cameras"],
    ["--aa", "--progressive-cameras", "--spp", "20", "--lookahead", "8"],
    LENS + ["--progressive-cameras", "--lookahead", "0"],
    ["--aa"] + LENS + ["--progressive-cameras", "--spp", "5000", "--lookahead", "64"],
])
def test_cli_accepts_progressive_cameras(built, tmp_path, args):
    out = _cli(tmp_path, *args)
    assert out.returncode == 0, out.stderr
    assert (tmp_path / "scene.bin").stat().st_size > 0


@pytest.mark.parametrize("args", [
    ["--progressive-cameras"],                                          # no camera flag
    ["--progressive-cameras", "--lookahead", "8"],
    ["--aa", "--progressive-cameras", "--adaptive", "0.01"],
    ["--aa", "--progressive-cameras", "--adaptive-cameras", "0.01"],
    ["--aa", "--progressive-cameras", "--denoise"],
    ["--aa", "--progressive-cameras", "--progressive"],
    LENS + ["--progressive-cameras", "--progressive"],
    ["--aa", "--progressive-cameras", "--lookahead", "1"],              # 1 is no batch size
    ["--aa", "--progressive-cameras", "--lookahead", "65"],
    ["--aperture", "0.1", "--progressive-cameras"],                     # a lens has a focus distance
])
def test_cli_rejects_bad_progressive_cameras_flags(built, tmp_path, args):
    out = _cli(tmp_path, *args)
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "usage" in out.stderr and "--progressive-cameras" in out.stderr          # the usage text names the flag


def test_cli_keeps_its_older_refusals(built, tmp_path):
    for flags in (["--aa", "--progressive"], LENS + ["--progressive"], ["--aa", "--adaptive", "0.01"]):
        out = _cli(tmp_path, *flags)
        assert out.returncode == 2 and "use --spp" in out.stderr and "usage" not in out.stderr, (flags, out.stderr)
    assert _cli(tmp_path, "--lookahead", "8").returncode == 2           # the flag belongs to a progressive mode
