"""CPU: the host side of the hemisphere gather (rt_render_hemispheres) — the header, the prototype and the exported symbol,
_abi.check_hemisphere_target and _abi.check_gather's refusals (no device needed), the Python wrappers' checks before any
library call, the façade's methods, rt_cli's --gather usage rules and the documents."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases

rt = cases.rt
A = rt._abi
ROOT = cases.ROOT
F32 = np.float32


def test_header_prototype_and_symbol(built):
    header = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    assert re.search(r"^int rt_render_hemispheres\(rt_context \*ctx, const void \*d_features, size_t n, const rt_hemisphere_params \*p,\s+"
                     r"uint32_t first_sample, uint32_t n_samples, void \*d_accum\);", header, re.M)
    assert re.search(r"^#define RT_ABI_VERSION %d$" % A.RT_ABI_VERSION, header, re.M) and A.RT_ABI_VERSION == 3   # additive
    assert "rt_render_hemispheres" in rt.raytracer.SYMBOLS
    lib = rt.load_library()
    assert len(lib.rt_render_hemispheres.argtypes) == 7
    p = A.HemisphereParams(16, 0, 7, 0.0, float("inf"))
    assert lib.rt_render_hemispheres(None, None, 1, C.byref(p), 0, 16, None) == -1           # a NULL context: RT_EINVAL
    exported = subprocess.run(["nm", "-D", "--defined-only", rt.raytracer.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T rt_render_hemispheres$", exported, re.M)
    for name in ("renderHemispheres", "irradiance"):
        assert hasattr(rt.RayTracer, name)


def test_check_hemisphere_target():
    import torch
    n = 12
    host = torch.zeros((n, 4), dtype=torch.float32)
    with pytest.raises(ValueError) as e:                       # right shape and dtype, wrong place: the last rule
        A.check_hemisphere_target(host, n)
    assert "device tensor" in str(e.value)
    for bad in (np.zeros((n, 4), F32), None, host.double(), host.int(), torch.zeros((n, 3)), torch.zeros((n + 1, 4)), torch.zeros((4 * n,)),
                torch.zeros((n, 4, 1)), torch.zeros((n, 8))[:, ::2], torch.zeros((2 * n, 4))[::2]):
        with pytest.raises(ValueError) as e:
            A.check_hemisphere_target(bad, n)
        if isinstance(bad, torch.Tensor) and (bad.dtype != torch.float32 or tuple(bad.shape) != (n, 4)):
            assert "shape" in str(e.value)

    # a view one float into a buffer is contiguous, (n, 4) float32 and 4 bytes off a 16-byte boundary
    off = torch.zeros((4 * n + 1,), dtype=torch.float32)[1:].reshape(n, 4)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    with pytest.raises(ValueError):
        A.check_hemisphere_target(off, n)


def test_check_gather_restates_every_refusal():
    """One case per RT_EINVAL row of rt_render_hemispheres that the Python layer can meet.  The tensors live on the host, so
    a call that passes the argument rules ends at the check of the first tensor ('device tensor')."""
    import torch
    n, k, w, h = 12, 4, 4, 3
    feats = torch.zeros((n, A.FEATURE_FLOATS), dtype=torch.float32)
    out = torch.zeros((n, 4), dtype=torch.float32)
    good = dict(features=None, n=n, k=k, flags=A.HEMI_FACE_FORWARD, offset=1e-3, first_sample=0, n_samples=None, out=None, width=w, height=h)
    assert A.check_gather(**good) == (k, 1, 0, k)                                # n_samples None: k; nothing else to refuse
    assert A.check_gather(**dict(good, first_sample=3, n_samples=11)) == (k, 1, 3, 11)
    assert A.check_gather(**dict(good, first_sample=A.MAX_SAMPLE, n_samples=1)) == (k, 1, A.MAX_SAMPLE, 1)

    def refused(**change):
        with pytest.raises(ValueError) as e:
            A.check_gather(**dict(good, **change))
        return str(e.value)

    assert "device tensor" in refused(out=out) and "device tensor" in refused(features=feats)
    assert "records" in refused(n=0, width=0) and "records" in refused(n=A.MAX_RAYS + 1, width=A.MAX_RAYS + 1, height=1)
    assert "rays, not 0" in refused(k=0) and "rays, not" in refused(k=A.RAY_SET_MAX + 1)
    big = 1 << 20
    assert "2^31" in refused(n=big, k=4096, width=big, height=1) and "2^31" not in refused(n=big, k=2048, width=big, height=1, out=out)
    assert "flags" in refused(flags=2) and "flags" in refused(flags=A.HEMI_FACE_FORWARD | 0x80000000)
    for bad in (float("inf"), float("-inf"), float("nan"), 1e39):
        assert "finite" in refused(offset=bad)
    assert "samples" in refused(n_samples=0) and "samples" in refused(n_samples=-1) and "samples" in refused(first_sample=-1)
    assert "samples" in refused(first_sample=A.MAX_SAMPLE, n_samples=2) and "samples" in refused(n_samples=A.MAX_SAMPLE + 2)
    assert "4 x 3" in refused(n=11)                                               # NULL features with n != W * H
    # (records of another number than the frame's need an external target: on the device the rule is reached, here the
    # host tensor is refused first — tests/test_gpu_gather.py meets it through the library)
    with pytest.raises(ValueError):
        A.check_gather(**dict(good, features=torch.zeros((n + 1, 20)), n=n + 1, out=None))
    assert "sharded" in refused(world=2)
    assert "shape" in refused(out=torch.zeros((n + 1, 4))) and "shape" in refused(out=torch.zeros((n, 3)))
    # the occlusion form's checker still refuses what it refused (the shared rules moved, its own stayed)
    with pytest.raises(ValueError) as e:
        A.check_hemispheres(None, n, k, 1, 0.0, None, None, w, h)
    assert "needs counts" in str(e.value)


class NoLibrary:
    """A library whose every entry point fails the test: the wrappers' own checks must come first."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def test_wrappers_validate_before_any_library_call():
    import torch
    t = rt.RayTracer.__new__(rt.RayTracer)            # no context, no device: only what the checks read
    t.width, t.height, t._device, t._ctx, t._lib = 4, 3, 0, None, NoLibrary()
    feats = torch.zeros((12, A.FEATURE_FLOATS), dtype=torch.float32)
    for kw in (dict(k=0), dict(k=A.RAY_SET_MAX + 1), dict(k=-3), dict(offset=float("inf")), dict(offset=float("nan")), dict(n_samples=0),
               dict(n_samples=-5), dict(first_sample=A.MAX_SAMPLE, n_samples=2), dict(n_samples=A.MAX_SAMPLE + 2), dict(first_sample=-1),
               dict(features=feats), dict(out=torch.zeros((12, 4))), dict(out=np.zeros((12, 4), F32))):
        with pytest.raises(ValueError):
            t.renderHemispheres(**kw)
    for args in ((0,), (A.RAY_SET_MAX + 1,), (4, 0), (4, -1), (4, 1, 0, float("inf")), (4, 1, 0, float("nan")), (256, 257)):
        with pytest.raises(ValueError):
            t.irradiance(*args)
    with pytest.raises(AssertionError):               # and a call that passes them does reach the library
        t.renderHemispheres(None, 4)


def test_facade_and_cli(built):
    header = open(os.path.join(ROOT, "host", "raytracer.h")).read()
    assert "renderHemispheres(" in header and "irradiance(" in header
    symbols = subprocess.run(["nm", "-C", os.path.join(ROOT, "host", "librt_host.a")], capture_output=True, text=True, check=True).stdout
    assert "RayTracer::renderHemispheres(" in symbols and "RayTracer::irradiance(" in symbols
    cli = os.path.join(ROOT, "host", "rt_cli")

    def run(*args):
        return subprocess.run([cli, "--scene", os.path.join(ROOT, "no_such.scene")] + list(args), capture_output=True, text=True)

    for args in (("--gather", "8"), ("--gather-spp", "2"), ("--aov", "p", "--gather-spp", "2"),          # --gather goes with --aov
                 ("--aov", "p", "--gather", "0"), ("--aov", "p", "--gather", "4097"), ("--aov", "p", "--gather", "8", "--gather-spp", "0"),
                 ("--aov", "p", "--gather", "4096", "--gather-spp", "17"),                               # more than 65536 samples
                 ("--aov", "p", "--gather", "8", "--follow", "mirror"),
                 ("--aov", "p", "--aa", "--gather", "8", "--aa-guides", "4")):
        p = run(*args)
        assert p.returncode == 2 and "--gather" in p.stderr and "rt_render_hemispheres" in p.stderr, args
    for args in (("--aov", "p", "--gather", "8"), ("--aov", "p", "--gather", "8", "--gather-spp", "3"), ("--aov", "p", "--gather", "4096", "--gather-spp", "16")):
        p = run(*args)                                 # passes the usage rules: fails later, not as usage
        assert p.returncode != 2 and "usage:" not in p.stderr, args


def test_documents():
    readme = open(os.path.join(ROOT, "README.md"), encoding="utf-8").read()
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    assert "rt_render_hemispheres" in readme and "renderHemispheres" in readme
    m = re.search(r"^### Hemisphere gather \(`rt_render_hemispheres`.*?(?=^### |\Z)", design, re.M | re.S)
    assert m, "DESIGN.md has no 'Hemisphere gather' section"
    section = m.group(0)
    for word in ("pt_samples_q_hemi", "pt_render_hemi", "hemisphere_frame", "hemisphere_dir", "Contract", "VGPR", "scratch", "queries_bench.py --gather"):
        assert word in section, word
