"""CPU: the adaptive-sampling surface that needs no device — header and exports, rt_cli's new flags, and the host
reference of the block error that tests/test_gpu_adaptive.py checks the device against."""
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
NEW = ("rt_render_adaptive", "rt_read_sample_counts", "rt_read_block_error")


def test_header_structs_compile_in_plain_c(built, tmp_path):
    src = tmp_path / "adaptive.c"
    src.write_text('#include <stdio.h>\n#include "rt_amd.h"\n'
                   'int main(void) {\n'
                   '    rt_adaptive_params p = {64, 128, 1024, 0.01f, 8, 8};\n'
                   '    rt_adaptive_stats s = {0, 0, 0, 0};\n'
                   '    uint32_t c[1]; float e[1];\n'
                   '    printf("%zu %zu %d %d %d\\n", sizeof p, sizeof s, rt_render_adaptive(NULL, NULL, &p, &s),\n'
                   '           rt_read_sample_counts(NULL, c, sizeof c), rt_read_block_error(NULL, e, sizeof e));\n'
                   '    return 0;\n'
                   '}\n')
    exe = tmp_path / "adaptive"
    pkg = os.path.dirname(rt.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lrt_amd", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    # a NULL context is an error, not a crash
    assert out.stdout.split() == [str(C.sizeof(A.AdaptiveParams)), str(C.sizeof(A.AdaptiveStats)), "-1", "-1", "-1"]
    assert (C.sizeof(A.AdaptiveParams), C.sizeof(A.AdaptiveStats)) == (24, 24)


def test_library_exports_the_new_symbols(built):
    lib = C.CDLL(rt.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in rt.raytracer.SYMBOLS
    lib = rt.load_library()
    assert lib.rt_render_adaptive.argtypes is not None


def _cli(*args):
    return subprocess.run([CLI, "--scene", os.path.join(ROOT, "assets", "scenes", "c1_sphere.scene"), *args],
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [
    ["--adaptive", "0.05"],
    ["--adaptive", "0", "--batch", "32", "--spp", "100"],
    ["--adaptive=0.01", "--batch", "32", "--min-spp", "64", "--spp", "1024", "--counts", "c.pgm"],
    ["--adaptive", "0.01", "--batch", "1", "--spp", "2"],
    ["--adaptive", "0.01", "--batch", "512", "--spp", "65536"],
])
def test_cli_accepts_adaptive_flags(built, tmp_path, args):
    # --dump-scene is the host-only mode: the arguments are parsed and checked, no device is needed
    out = _cli(*args, "--dump-scene", str(tmp_path / "scene.bin"))
    assert out.returncode == 0, out.stderr
    assert (tmp_path / "scene.bin").stat().st_size > 0


@pytest.mark.parametrize("args", [
    ["--adaptive", "-1"],
    ["--adaptive", "nan"],
    ["--adaptive", "x"],
    ["--adaptive", "0.1", "--batch", "0"],
    ["--adaptive", "0.1", "--batch", "513", "--spp", "2048"],
    ["--adaptive", "0.1", "--batch", "16", "--min-spp", "24"],        # not a multiple of batch
    ["--adaptive", "0.1", "--batch", "16", "--min-spp", "16"],        # below 2 x batch
    ["--adaptive", "0.1", "--batch", "16", "--min-spp", "64", "--spp", "32"],   # max below min
    ["--adaptive", "0.1", "--batch", "512", "--spp", "65537"],
    ["--adaptive", "0.1", "--progressive"],
    ["--batch", "16"],                                                 # adaptive-only flags without --adaptive
    ["--min-spp", "32"],
    ["--counts", "c.pgm"],
])
def test_cli_rejects_bad_adaptive_flags(built, tmp_path, args):
    out = _cli(*args, "--dump-scene", str(tmp_path / "scene.bin"))
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "--adaptive THRESHOLD" in out.stderr


def _acc(rgb, n):
    rgb = np.asarray(rgb, np.float32)
    out = np.empty(rgb.shape[:-1] + (4,), np.float32)
    out[..., :3] = rgb * np.float32(n)
    out[..., 3] = n
    return out


def test_block_error_reference_by_hand():
    # one pixel: I = (0.5, 0.25, 0.25), A = (0.25, 0.25, 0.5) → e = (0.25 + 0 + 0.25) / sqrt(1) = 0.5
    acc = _acc([[[0.5, 0.25, 0.25]]], 4)
    half = _acc([[[0.25, 0.25, 0.5]]], 2)
    assert A.block_error_reference(acc, half, 8, 8)[0, 0] == pytest.approx(0.5)
    # I = (1, 2, 1): sqrt 2 in the denominator
    acc = _acc([[[1.0, 2.0, 1.0]]], 8)
    half = _acc([[[1.0, 1.0, 1.0]]], 4)
    assert A.block_error_reference(acc, half, 1, 1)[0, 0] == pytest.approx(1.0 / 2.0)


def test_block_error_reference_zero_denominator_and_equal_halves():
    acc = np.zeros((2, 2, 4), np.float32)
    acc[..., 3] = 4
    half = np.zeros((2, 2, 4), np.float32)
    half[..., 3] = 2
    half[0, 0, 0] = 1.0           # black mean, non-black half: the denominator is still 0 → e = 0
    assert (A.block_error_reference(acc, half, 2, 2) == 0).all()
    same = _acc(np.full((2, 2, 3), 0.3), 8)
    assert (A.block_error_reference(same, _acc(np.full((2, 2, 3), 0.3), 4), 2, 2) == 0).all()
    # a pixel without samples (0 / 0) counts as 0, not NaN
    empty = np.zeros((1, 1, 4), np.float32)
    assert A.block_error_reference(empty, empty, 1, 1)[0, 0] == 0


def test_block_error_reference_edge_blocks_average_in_frame_pixels_only():
    h, w = 5, 7                   # 4 x 4 blocks: 2 x 2 of them, three of them cut by the frame edge
    rng = np.random.RandomState(0)
    i = rng.uniform(0.1, 1.0, (h, w, 3)).astype(np.float32)
    a = rng.uniform(0.1, 1.0, (h, w, 3)).astype(np.float32)
    acc, half = _acc(i, 16), _acc(a, 8)
    got = A.block_error_reference(acc, half, 4, 4)
    assert got.shape == (2, 2)
    ii, aa = acc[..., :3] / acc[..., 3:], half[..., :3] / half[..., 3:]
    e = np.abs(ii - aa).sum(-1) / np.sqrt(ii.sum(-1))
    for by in range(2):
        for bx in range(2):
            blk = e[4 * by:4 * by + 4, 4 * bx:4 * bx + 4]
            assert got[by, bx] == pytest.approx(blk.mean(), rel=1e-6)
    assert got[1, 1] == pytest.approx(e[4, 4:].mean(), rel=1e-6)      # 1 x 3 in-frame pixels


def test_render_adaptive_rejects_a_null_context(built):
    lib = rt.load_library()
    p = A.AdaptiveParams(64, 128, 1024, 0.01, 8, 8)
    st = A.AdaptiveStats()
    cam = np.zeros(12, np.float32)
    assert lib.rt_render_adaptive(None, cam.ctypes.data, C.byref(p), C.byref(st)) == -1
