"""CPU: the surface of the variance-driven stopping rule that needs no device — header and exports, rt_cli's
--adaptive-rule, and the host restatement (tests/adaptive_variance_ref.py) that tests/test_gpu_adaptive_variance.py
measures the device against, checked by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_variance_ref as AV
import cases

rt = cases.rt
A = rt._abi
ROOT = cases.ROOT
CLI = os.path.join(ROOT, "host", "rt_cli")
NEW = ("rt_render_adaptive_variance", "rt_render_adaptive_variance_cameras", "rt_read_pixel_error", "rt_device_pixel_error")


def test_header_compiles_in_plain_c_with_the_new_declarations(built, tmp_path):
    src = tmp_path / "variance.c"
    src.write_text('#include <stdio.h>\n#include "rt_amd.h"\n'
                   'int main(void) {\n'
                   '    rt_adaptive_params p = {16, 16, 1024, 0.01f, 8, 8};\n'
                   '    rt_adaptive_stats s = {0, 0, 0, 0};\n'
                   '    float cam[12] = {0}; float e[1]; void *d = NULL;\n'
                   '    printf("%zu %zu %d %d %d %d %d\\n", sizeof p, sizeof s, rt_abi_version(),\n'
                   '           rt_render_adaptive_variance(NULL, cam, &p, &s),\n'
                   '           rt_render_adaptive_variance_cameras(NULL, cam, 1, &p, &s),\n'
                   '           rt_read_pixel_error(NULL, e, sizeof e), rt_device_pixel_error(NULL, &d));\n'
                   '    return 0;\n'
                   '}\n')
    exe = tmp_path / "variance"
    pkg = os.path.dirname(rt.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lrt_amd", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    # the structs and the ABI version are the Dammertz calls'; a NULL context is an error, not a crash
    assert out.stdout.split() == ["24", "24", "3", "-1", "-1", "-1", "-1"]


def test_library_exports_and_binds_the_new_symbols(built):
    raw = C.CDLL(rt.LIB_PATH)
    for s in NEW:
        assert hasattr(raw, s), s
        assert s in rt.raytracer.SYMBOLS
    lib = rt.load_library()
    for s in NEW:
        assert getattr(lib, s).argtypes is not None, s
    for m in ("renderAdaptiveVariance", "renderAdaptiveVarianceCameras", "pixelError", "devicePixelError"):
        assert callable(getattr(rt.RayTracer, m))


def test_null_context_calls_give_einval(built):
    lib = rt.load_library()
    p = A.AdaptiveParams(16, 32, 1024, 0.01, 8, 8)
    st = A.AdaptiveStats()
    cam = np.zeros(12, np.float32)
    e = np.zeros(4, np.float32)
    d = C.c_void_p()
    assert lib.rt_render_adaptive_variance(None, cam.ctypes.data, C.byref(p), C.byref(st)) == -1
    assert lib.rt_render_adaptive_variance_cameras(None, cam.ctypes.data, 1, C.byref(p), C.byref(st)) == -1
    assert lib.rt_read_pixel_error(None, e.ctypes.data, e.nbytes) == -1
    assert lib.rt_device_pixel_error(None, C.byref(d)) == -1


# ---- the restatement by hand --------------------------------------------------------------------------------------------

def _state(samples):
    """(n, 3) samples of one pixel → its (1, 1, 4) accumulator and (1, 1) two-pass moment."""
    s = np.asarray(samples, dtype=np.float64)
    acc = np.zeros((1, 1, 4))
    acc[0, 0, :3] = s.sum(0)
    acc[0, 0, 3] = len(s)
    l = s @ AV.LUM
    return acc, np.array([[((l - l.mean()) ** 2).sum()]])


def test_pixel_error_of_one_pixel_by_hand():
    # grey samples 1 and 3 (luminance = the grey value): mean 2, M2 = 2, n = 2 → sqrt(2 / 2) / sqrt(2)
    acc, m2 = _state([[1, 1, 1], [3, 3, 3]])
    assert m2[0, 0] == pytest.approx(2.0)
    assert AV.pixel_error(acc, m2)[0, 0] == pytest.approx(1.0 / np.sqrt(2.0))
    # four samples 0, 0, 4, 4: mean 2, M2 = 16, variance of the mean 16 / 12 → sqrt(4 / 3) / sqrt(2)
    acc, m2 = _state([[0, 0, 0], [0, 0, 0], [4, 4, 4], [4, 4, 4]])
    assert AV.pixel_error(acc, m2)[0, 0] == pytest.approx(np.sqrt(4.0 / 3.0) / np.sqrt(2.0))
    # a coloured pixel: the luminance weights enter both the moment and the mean
    acc, m2 = _state([[1, 0, 0], [0, 1, 0]])
    l = np.array([0.2126, 0.7152])
    exp = np.sqrt(((l - l.mean()) ** 2).sum() / 2.0) / np.sqrt(l.mean())
    assert AV.pixel_error(acc, m2)[0, 0] == pytest.approx(exp)
    # the binary32 form agrees to rounding
    assert AV.pixel_error_f32(acc, m2)[0, 0] == pytest.approx(exp, rel=1e-6)
    assert AV.pixel_error_f32(acc, m2).dtype == np.float32


def test_pixel_error_is_zero_without_luminance_samples_or_spread():
    # L = 0 with a non-zero moment (cannot come from non-negative samples, but the rule is stated for it)
    acc = np.zeros((1, 1, 4))
    acc[0, 0, 3] = 4
    for f in (AV.pixel_error, AV.pixel_error_f32):
        assert f(acc, np.array([[1.0]]))[0, 0] == 0
        # n = 1 and n = 0
        one = np.array([[[0.5, 0.5, 0.5, 1.0]]])
        assert f(one, np.array([[0.0]]))[0, 0] == 0
        assert f(one, np.array([[3.0]]))[0, 0] == 0
        assert f(np.zeros((1, 1, 4)), np.array([[0.0]]))[0, 0] == 0
        # equal samples: M2 = 0 → 0
        same = np.array([[[0.3 * 8, 0.3 * 8, 0.3 * 8, 8.0]]])
        assert f(same, np.array([[0.0]]))[0, 0] == 0
        # a negative moment (rounding) counts as none
        assert f(same, np.array([[-1e-9]]))[0, 0] == 0
    acc, m2 = _state([[0.3, 0.3, 0.3]] * 8)
    assert m2[0, 0] == 0 and AV.pixel_error(acc, m2)[0, 0] == 0


def test_block_error_edge_blocks_average_in_frame_pixels_only():
    h, w = 5, 7                   # 4 x 4 blocks: 2 x 2 of them, three of them cut by the frame edge
    e = np.random.RandomState(0).uniform(0.1, 1.0, (h, w))
    got = AV.block_error(e, 4, 4)
    assert got.shape == (2, 2)
    for by in range(2):
        for bx in range(2):
            assert got[by, bx] == pytest.approx(e[4 * by:4 * by + 4, 4 * bx:4 * bx + 4].mean(), rel=1e-12)
    assert got[0, 1] == pytest.approx(e[:4, 4:].mean())            # 4 x 3
    assert got[1, 0] == pytest.approx(e[4, :4].mean())             # 1 x 4
    assert got[1, 1] == pytest.approx(e[4, 4:].mean())             # 1 x 3 in-frame pixels
    # zeros of in-frame pixels count, the padding does not
    z = np.zeros((h, w))
    z[4, 6] = 3.0
    assert AV.block_error(z, 4, 4)[1, 1] == pytest.approx(1.0)


def test_round_simulation_by_hand():
    # batch 16, min 32, max 104: counts 16, 32, 48, ..., 96, 104.  Four blocks:
    #   0: always below the threshold → stops at min_spp (round 1), not before
    #   1: converges after round 3
    #   2: never converges → at max, unconverged
    #   3: converges in the very last round → at max, but converged
    errs = [np.array([0.0, 9.0, 9.0, 9.0]), np.array([0.0, 9.0, 9.0, 9.0]), np.array([5.0, 9.0, 9.0, 9.0]),
            np.array([5.0, 0.5, 9.0, 9.0]), np.array([5.0, 0.1, 9.0, 9.0]), np.array([5.0, 0.1, 9.0, 9.0]),
            np.array([5.0, 0.1, 9.0, 0.5])]
    assert AV.round_counts(16, 104) == [16, 32, 48, 64, 80, 96, 104]
    stop, final, at_max, rounds = AV.simulate(errs, 16, 32, 104, 1.0)
    assert stop.tolist() == [1, 3, 6, 6]
    assert final.tolist() == [0.0, 0.5, 9.0, 0.5]
    assert (at_max, rounds) == (1, 7)
    # threshold 0 never stops early, and every block ends at max unconverged
    stop, _, at_max, rounds = AV.simulate(errs, 16, 32, 104, 0.0)
    assert stop.tolist() == [6] * 4 and (at_max, rounds) == (4, 7)
    # min_spp == batch: round 0 decides
    stop, _, at_max, rounds = AV.simulate(errs, 16, 16, 104, 1.0)
    assert stop.tolist() == [0, 3, 6, 6]
    # an error equal to the threshold has not converged
    stop, _, _, _ = AV.simulate([np.array([1.0]), np.array([1.0]), np.array([0.5])], 16, 16, 48, 1.0)
    assert stop.tolist() == [2]


def test_thresholds_are_no_element_of_the_set():
    e = np.array([0.0, 0.4, 0.1, 0.3, 0.2, 0.0])
    assert AV.middle_threshold(e) == pytest.approx(0.25)
    assert AV.middle_threshold(e[:-2]) == pytest.approx(0.2)        # 0.1, 0.3, 0.4: an odd count → below the median element
    for t in (AV.middle_threshold(e), AV.middle_threshold(e[1:]), AV.percentile_threshold(e, 10)):
        assert t not in e.tolist()


# ---- rt_cli -------------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([CLI, "--scene", os.path.join(ROOT, "assets", "scenes", "c1_sphere.scene"), *args],
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [
    ["--adaptive", "0.05", "--adaptive-rule", "variance", "--batch", "16", "--min-spp", "16"],
    ["--adaptive", "0.05", "--adaptive-rule=variance"],
    ["--adaptive-rule", "variance", "--adaptive", "0.05", "--batch", "1", "--min-spp", "2", "--spp", "2"],
    ["--adaptive", "0.05", "--adaptive-rule", "dammertz", "--batch", "16", "--min-spp", "32"],
    ["--adaptive-cameras", "0.05", "--adaptive-rule", "variance", "--aa", "--batch", "16", "--min-spp", "16", "--spp", "64"],
    ["--adaptive", "0.05", "--adaptive-rule", "variance", "--denoise", "--variance-guided", "--measured", "--aov", "a"],
])
def test_cli_accepts_the_adaptive_rule(built, tmp_path, args):
    # --dump-scene is the host-only mode: the arguments are parsed and checked, no device is needed
    out = _cli(*args, "--dump-scene", str(tmp_path / "scene.bin"))
    assert out.returncode == 0, out.stderr
    assert (tmp_path / "scene.bin").stat().st_size > 0


@pytest.mark.parametrize("args", [
    ["--adaptive-rule", "variance"],                                                      # alone
    ["--adaptive-rule", "variance", "--spp", "64"],
    ["--adaptive-rule", "variance", "--progressive"],
    ["--adaptive", "0.1", "--adaptive-rule", "x"],
    ["--adaptive", "0.1", "--adaptive-rule"],
    ["--adaptive", "0.1", "--adaptive-rule", "variance", "--batch", "16", "--min-spp", "24"],   # not a multiple of batch
    ["--adaptive", "0.1", "--adaptive-rule", "variance", "--min-spp", "1", "--batch", "1"],     # one sample has no variance
    ["--adaptive", "0.1", "--adaptive-rule", "dammertz", "--batch", "16", "--min-spp", "16"],   # the Dammertz rule keeps 2 x batch
    ["--adaptive", "0.1", "--adaptive-rule", "variance", "--batch", "16", "--min-spp", "32", "--spp", "16"],
])
def test_cli_rejects_bad_adaptive_rule_flags(built, tmp_path, args):
    out = _cli(*args, "--dump-scene", str(tmp_path / "scene.bin"))
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "--adaptive THRESHOLD" in out.stderr and "--adaptive-rule dammertz|variance" in out.stderr
