"""CPU: the host side of the hemisphere queries (rt_occluded_hemispheres) — the header, the prototype and the exported
symbol, _abi.check_hemispheres' refusals (one per RT_EINVAL rule of the header, no device needed), the float64 reference
wrapper tests/hemisphere_ref.py, the façade's methods and rt_cli's --ao-device usage rules."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import hemisphere_ref as H

rt = cases.rt
A = rt._abi
ROOT = cases.ROOT
F32 = np.float32


def test_header_prototype_and_symbol(built):
    header = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    assert re.search(r"^int rt_occluded_hemispheres\(rt_context \*ctx, const void \*d_features, size_t n, const rt_hemisphere_params \*p,\s+"
                     r"void \*d_counts, void \*d_rays_out\);", header, re.M)
    assert re.search(r"^#define RT_HEMI_FACE_FORWARD 1u", header, re.M) and A.HEMI_FACE_FORWARD == 1
    assert re.search(r"^#define RT_ABI_VERSION %d$" % A.RT_ABI_VERSION, header, re.M)      # additive: the version stays
    # the struct as the header lays it out: k, flags, seed (8-byte aligned), offset, t_max — 24 bytes
    assert [f[0] for f in A.HemisphereParams._fields_] == ["k", "flags", "seed", "offset", "t_max"]
    assert C.sizeof(A.HemisphereParams) == 24 and A.HemisphereParams.seed.offset == 8 and A.HemisphereParams.t_max.offset == 20
    assert "rt_occluded_hemispheres" in rt.raytracer.SYMBOLS
    lib = rt.load_library()
    assert len(lib.rt_occluded_hemispheres.argtypes) == 6
    p = A.HemisphereParams(16, 0, 7, 0.0, float("inf"))
    assert lib.rt_occluded_hemispheres(None, None, 1, C.byref(p), None, None) == -1         # a NULL context: RT_EINVAL
    for name in ("occludedHemispheres", "spawnHemispheres", "ambientOcclusion"):
        assert hasattr(rt.RayTracer, name)


def test_check_hemispheres_restates_every_refusal():
    """One case per RT_EINVAL row of rt_occluded_hemispheres that the Python layer can meet (a NULL ctx or p cannot
    arise there).  The tensors live on the host here, so every call that passes the argument rules ends at the check of
    the first tensor: 'device tensor' in the message tells the two apart."""
    import torch
    n, k, w, h = 12, 4, 4, 3
    feats = torch.zeros((n, A.FEATURE_FLOATS), dtype=torch.float32)
    counts = torch.zeros((n,), dtype=torch.int32)
    rays = torch.zeros((n * k, 8), dtype=torch.float32)
    good = dict(features=None, n=n, k=k, flags=A.HEMI_FACE_FORWARD, offset=1e-3, counts=counts, rays_out=None, width=w, height=h)

    def refused(**change):
        kw = dict(good)
        kw.update(change)
        with pytest.raises(ValueError) as e:
            A.check_hemispheres(**kw)
        return str(e.value)

    assert "device tensor" in refused()                                      # the rules pass; the host tensor does not
    assert "needs counts" in refused(counts=None)                            # both outputs NULL
    assert "records" in refused(n=0, width=0) and "records" in refused(n=A.MAX_RAYS + 1, width=A.MAX_RAYS + 1, height=1)
    assert "rays, not 0" in refused(k=0) and "rays, not" in refused(k=A.RAY_SET_MAX + 1)
    big = 1 << 20
    assert "2^31" in refused(n=big, k=4096, width=big, height=1)             # n * k above 2^31
    assert "2^31" not in refused(n=big, k=2048, width=big, height=1)         # exactly 2^31 is allowed
    assert "flags" in refused(flags=2) and "flags" in refused(flags=A.HEMI_FACE_FORWARD | 0x80000000)
    for bad in (float("inf"), float("-inf"), float("nan"), 1e39):            # (1e39 is not finite in binary32)
        assert "finite" in refused(offset=bad)
    assert "4 x 3" in refused(n=11)                                          # NULL features with n != W * H
    assert "sharded" in refused(world=2)
    # tensors of the wrong kind, shape or alignment
    assert "shape" in refused(features=feats, n=n + 1, counts=torch.zeros((n + 1,), dtype=torch.int32))
    assert "int32" in refused(counts=counts.float()) or "out must be" in refused(counts=counts.float())
    for bad in (np.zeros((n, 20), F32), feats.double(), torch.zeros((n, 19)), torch.zeros((2 * n, 20))[::2]):
        with pytest.raises(ValueError):
            A.check_hemispheres(**dict(good, features=bad))
    for bad in (rays.double(), torch.zeros((n * k, 7)), torch.zeros((n, k + 1, 8)), torch.zeros((n * k + k, 8))):
        with pytest.raises(ValueError):
            A.check_hemispheres(**dict(good, rays_out=bad))


def test_reference_wrapper_masks_faces_and_counts_by_record():
    recs = H.generator_records()
    mask = H.valid_mask(recs)
    assert mask.sum() == len(recs) - 4 and not mask[-5:-1].any() and mask[-1]      # zero, NaN, inf, no hit flag
    k, seed = 5, 11
    m0, plain = H.hemisphere_rays(recs, k, seed)
    m1, faced = H.hemisphere_rays(recs, k, seed, offset=1e-3, face_forward=True)
    assert np.array_equal(m0, mask) and np.array_equal(m1, mask) and plain.shape == (len(recs), k)
    assert not plain[~mask].view(np.uint8).any() and not faced[~mask].view(np.uint8).any()
    assert (plain["x"][mask] == np.arange(len(recs))[mask, None]).all() and (plain["y"] == 0).all()
    # the counter is i * k + t whatever lies before record i: the last record alone, moved to slot 0, gives other rays,
    # and the uniforms of slot (i, t) are workloads.uniforms(n * k, 0, seed)[i * k + t]
    last = len(recs) - 1
    u = rt.workloads.uniforms(len(recs) * k, 0, seed)[last * k:, :2].astype(np.float64)
    up = (plain["d"][last].astype(np.float64) * (0, 1, 0)).sum(-1)             # the last record's normal is +y
    assert np.abs(up - np.sqrt(1 - u[:, 0])).max() < 1e-6
    # face-forward: a hemisphere about -normal where the normal looks along dir, about the normal elsewhere
    for sets, ff in ((plain, False), (faced, True)):
        unit = H.unit_normals(recs, ff)
        cos = (sets["d"].astype(np.float64) * unit[:, None, :]).sum(-1)
        assert cos[mask].min() > 0
    with np.errstate(invalid="ignore"):
        along = (recs["normal"].astype(np.float64) * recs["dir"].astype(np.float64)).sum(1) > 0
    assert along[mask].any() and (~along[mask]).any()
    same = (np.abs(plain["d"] - faced["d"]).max(axis=(1, 2)) < 1e-6)
    assert not same[mask & along].any() and same[mask & ~along].all()
    lift = faced["o"][mask].astype(np.float64) - recs["pos"][mask].astype(np.float64)[:, None, :]
    assert np.abs(lift - 1e-3 * H.unit_normals(recs, True)[mask][:, None, :]).max() < 1e-6
    padded = H.generator_records(400)
    assert len(padded) == 400 and padded[:len(recs)].tobytes() == recs.tobytes()
    assert 0 < (~H.valid_mask(padded)[len(recs):]).sum() < 100                    # misses in between


def test_facade_and_cli(built):
    header = open(os.path.join(ROOT, "host", "raytracer.h")).read()
    assert "occludedHemispheres(" in header and "ambientOcclusion(" in header
    symbols = subprocess.run(["nm", "-C", os.path.join(ROOT, "host", "librt_host.a")], capture_output=True, text=True, check=True).stdout
    assert "RayTracer::occludedHemispheres(" in symbols and "RayTracer::ambientOcclusion(" in symbols
    cli = os.path.join(ROOT, "host", "rt_cli")

    def run(*args):
        return subprocess.run([cli, "--scene", os.path.join(ROOT, "no_such.scene")] + list(args), capture_output=True, text=True)

    for args in (("--ao-device",), ("--aov", "p", "--ao-device"),                                   # without --ao
                 ("--aov", "p", "--ao", "4", "--ao-device", "--follow", "mirror"),
                 ("--aov", "p", "--aa", "--ao", "4", "--ao-device", "--aa-guides", "4"),
                 ("--ao", "4", "--ao-device")):                                                    # --ao goes with --aov
        p = run(*args)
        assert p.returncode == 2 and "--ao-device" in p.stderr and "rt_occluded_hemispheres" in p.stderr, args
    p = run("--aov", "p", "--ao", "4", "--ao-device")              # passes the usage rules: fails later, not as usage
    assert p.returncode != 2 and "usage:" not in p.stderr
