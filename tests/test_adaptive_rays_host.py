"""CPU: the host side of adaptive sampling for caller-supplied rays (rt_render_adaptive_rays, rt_render_adaptive_variance_rays)
— the header's declarations in plain C, the exported and bound symbols, NULL-context calls, _abi's argument checks (no device
needed) and rt_cli's usage rules for --projection with --adaptive.  The kernels find the pixel of ray i with a plain 32-bit
division, so there is no reciprocal whose domain would have to be walked here."""
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
NEW = ("rt_render_adaptive_rays", "rt_render_adaptive_variance_rays")


def test_header_compiles_in_plain_c_with_the_new_declarations(built, tmp_path):
    src = tmp_path / "adaptive_rays.c"
    src.write_text('#include <stdio.h>\n#include "rt_amd.h"\n'
                   'int main(void) {\n'
                   '    rt_adaptive_params p = {8, 16, 44, 0.01f, 8, 8};\n'
                   '    rt_adaptive_stats s = {0, 0, 0, 0};\n'
                   '    int (*a)(rt_context *, const void *, size_t, uint32_t, const rt_adaptive_params *, rt_adaptive_stats *) = rt_render_adaptive_rays;\n'
                   '    printf("%d %d %d\\n", rt_abi_version(), a(NULL, NULL, 1404, 0, &p, &s),\n'
                   '           rt_render_adaptive_variance_rays(NULL, NULL, 1404, RT_RAY_SET_MAX, &p, &s));\n'
                   '    return 0;\n'
                   '}\n')
    exe = tmp_path / "adaptive_rays"
    pkg = os.path.dirname(rt.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lrt_amd", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["3", "-1", "-1"]     # the ABI version stays; a NULL context is an error, not a crash


def test_library_exports_and_binds_the_new_symbols(built):
    raw = C.CDLL(rt.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    for s in NEW:
        assert hasattr(raw, s), s
        assert s in rt.raytracer.SYMBOLS
        assert "int %s(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t set_size" % s in header
    lib = rt.load_library()
    for s in NEW:
        assert len(getattr(lib, s).argtypes) == 6, s
    for m in ("renderAdaptiveRays", "renderAdaptiveVarianceRays"):
        assert callable(getattr(rt.RayTracer, m))


def test_defaults_are_those_of_the_camera_calls():
    import inspect
    for rays, twin in (("renderAdaptiveRays", "renderAdaptive"), ("renderAdaptiveVarianceRays", "renderAdaptiveVariance")):
        a = inspect.signature(getattr(rt.RayTracer, rays)).parameters
        b = inspect.signature(getattr(rt.RayTracer, twin)).parameters
        assert a["set_size"].default == 0
        for k in ("batch", "min_spp", "max_spp", "block"):
            assert a[k].default == b[k].default, (rays, k)


def test_null_context_calls_give_einval(built):
    lib = rt.load_library()
    p = A.AdaptiveParams(8, 16, 44, 0.01, 8, 8)
    st = A.AdaptiveStats()
    buf = np.zeros((4, 8), np.float32)
    for s in NEW:
        assert getattr(lib, s)(None, buf.ctypes.data, 4, 0, C.byref(p), C.byref(st)) == -1
        assert getattr(lib, s)(None, None, 4, 2, C.byref(p), C.byref(st)) == -1


def test_abi_checks_refuse_what_they_must(monkeypatch):
    torch = pytest.importorskip("torch")
    w, h = 6, 4
    n = w * h
    for k in (-1, A.RAY_SET_MAX + 1):
        with pytest.raises(ValueError):
            A.check_adaptive_set_size(k)
    assert A.check_adaptive_set_size(0) == 0 and A.check_adaptive_set_size(A.RAY_SET_MAX) == A.RAY_SET_MAX
    host = torch.zeros((n, 8), dtype=torch.float32)
    bad = [
        (np.zeros((n, 8), np.float32), 0),                       # not a tensor
        (host, 0),                                               # not on the device
        (torch.zeros((n, 3, 8), dtype=torch.float32), 3),        # sets, not on the device
        (torch.zeros((n, 8), dtype=torch.float64), 0),           # wrong type
        (torch.zeros((n, 7), dtype=torch.float32), 0),           # wrong shape
        (torch.zeros((n * 3 + 1, 8), dtype=torch.float32), 3),   # no whole sets
        (host, A.RAY_SET_MAX + 1),                               # set size out of range
        (host, -1),
    ]
    for t, k in bad:
        with pytest.raises(ValueError):
            A.check_adaptive_rays(t, k, w, h)

    # one ray per pixel: the count rule on its own — host tensors, with the tensor rules (pinned above and in
    # test_ray_sets_host.py) reduced to their counts
    monkeypatch.setattr(A, "check_rays", lambda x: int(x.shape[0]))
    monkeypatch.setattr(A, "check_ray_sets", lambda x, kk: int(x.shape[0]) // kk)
    for rows, k, ok in ((n, 0, True), (n - 1, 0, False), (n + w, 0, False), (n * 3, 3, True), (n * 3, 1, False), (n * 6, 3, False)):
        t = torch.zeros((rows, 8), dtype=torch.float32)
        if ok:
            assert A.check_adaptive_rays(t, k, w, h) == n
        else:
            with pytest.raises(ValueError):
                A.check_adaptive_rays(t, k, w, h)


def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=120, cwd=ROOT)


def test_cli_usage_rules_for_adaptive_projection_frames(built, tmp_path):
    scene = os.path.join(ROOT, "assets", "scenes", "c2_cornell.scene")
    dump = str(tmp_path / "scene.bin")
    base = ["--scene", scene, "--size", "32x20", "--projection", "ortho", "--extent", "12", "--dump-scene", dump]
    # accepted (the host-only --dump-scene mode ends after the usage rules, before any device is touched)
    ok = [["--adaptive", "0.05"],
          ["--ray-sets", "4", "--adaptive", "0.05", "--batch", "8", "--min-spp", "16", "--spp", "40", "--counts", "c.u32"],
          ["--adaptive", "0.05", "--adaptive-rule", "variance", "--batch", "8", "--min-spp", "8"],
          ["--ray-sets", "4", "--adaptive", "0.05", "--adaptive-rule", "variance", "--denoise", "--variance-guided", "--measured"],
          ["--spp", "8", "--denoise", "--variance-guided", "--measured"]]      # --measured on a fixed-count projection frame
    for extra in ok:
        r = run_cli(*(base + extra))
        assert r.returncode == 0, (extra, r.stderr)
    # the other refusals stay
    bad = [["--adaptive", "0.05", "--aa"], ["--adaptive", "0.05", "--progressive"], ["--progressive"], ["--aa"],
           ["--adaptive-cameras", "0.05", "--aa"], ["--progressive-cameras", "--aa"],
           ["--adaptive", "0.05", "--batch", "8", "--min-spp", "8"],              # the Dammertz rule needs two batches
           ["--adaptive", "0.05", "--measured"],                                  # --measured belongs to --denoise --variance-guided
           ["--batch", "8"], ["--adaptive-rule", "variance"]]                     # adaptive-only flags
    for extra in bad:
        r = run_cli(*(base + extra))
        assert r.returncode == 2, (extra, r.returncode)
