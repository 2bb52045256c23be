"""CPU: what the wave's fixed cost (profiles/r16_experiments.md) changes and a host can check — the exports,
the layout of the staged scene block restated from a scene's arrays (its VALUES are compared on the GPU,
tests/test_gpu_wave_fixed.py), and queue_stage's division-free tile quotient, in float32 as the device rounds it, against
`//` for every divisor a frame can have and every reciprocal v_rcp_f32 may return."""
import ctypes as C
import os
import re

import numpy as np

import cases
import wave_fixed_ref as W

rt = cases.rt
A = rt._abi
f32 = np.float32
CSRC = os.path.join(cases.ROOT, "opencl-raytracing_amd", "csrc")


def _define(text, name):
    return re.search(r"#define\s+%s\s+\(?\s*(\d+)" % name, text).group(1)


def test_library_exports_the_debug_getters(built):
    lib = C.CDLL(rt.LIB_PATH)
    for s in ("rt_debug_wave_fixed", "rt_debug_stage_block", "rt_debug_queue_pixels", "rt_debug_queue_occupancy",
              "rt_debug_plan_samples", "rt_debug_last_sample_plan"):
        assert hasattr(lib, s), s
        assert s in rt.raytracer.SYMBOLS
    for m in ("waveFixedStats", "stageBlock", "queueOccupancy", "planSamples", "lastSamplePlan"):
        assert callable(getattr(rt.RayTracer, m))


def test_the_layout_helper_has_the_kernels_caps():
    types = open(os.path.join(CSRC, "pt_types.hpp")).read()
    assert (A.LDS_MATERIALS, A.LDS_WINNERS, A.LDS_PLANES) == tuple(
        int(_define(types, n)) for n in ("PT_LDS_MATERIALS", "PT_LDS_WINNERS", "PT_LDS_PLANES"))
    kernels = "".join(open(os.path.join(CSRC, f)).read() for f in ("pt_kernels.hip", "pt_queue.hpp"))
    assert 1 << int(re.search(r"#define PT_XY_FAST_MAX_TILES \(1u << (\d+)\)", kernels).group(1)) == W.XY_FAST_MAX_TILES
    # the block follows the materials in their allocation, 16-byte aligned: a material is 48 bytes
    assert A.MATERIAL.itemsize == 48 and A.MATERIAL.itemsize % 16 == 0
    # every part has its switch, default on
    for name in ("PT_Q_COUNT64", "PT_STAGE_COPY", "PT_TEXEL_LAZY", "PT_STAGE_XY_FAST"):
        assert re.search(r"#ifndef %s\n#define %s 1\b" % (name, name), kernels), name


def test_stage_block_layout_of_real_scenes():
    for name, kw in (("c2", {}), ("all_kinds", {}), ("c3", dict(tex_size=8))):
        s = rt.workloads.get(name, width=16, height=16, **kw).scene
        nm, ns, npl = len(s.materials), len(s.spheres), len(s.planes)
        assert nm <= A.LDS_MATERIALS and ns <= A.LDS_WINNERS and npl <= A.LDS_PLANES
        m0, w0, p0, rows = A.stage_block_layout(nm, ns, npl)
        assert (m0, w0, p0, rows) == (0, 2 * nm, 2 * nm + 2 * ns, 2 * nm + 2 * ns + npl)
        b = W.stage_block(s)
        assert b.shape == (rows, 4) and b.dtype == f32
        words = b.view(np.uint32)
        assert np.array_equal(words[m0 + 1:w0:2, 0], s.materials["type"].astype(np.uint32))
        assert np.array_equal(b[m0:w0:2, 3], s.materials["extra_data"])
        assert np.array_equal(b[w0:p0:2, 3], s.spheres["r"])
        assert np.array_equal(words[w0 + 1:p0:2, 0], s.spheres["mat_ID"]) and not words[w0 + 1:p0:2, 1:].any()
        assert np.array_equal(words[p0:, 3], s.planes["mat_ID"])
        # glass constants: 1 / extra and Schlick's r0 of both ratios, in float32
        k = int(np.flatnonzero(s.materials["type"] == A.T_DIELECTRIC)[0]) if (s.materials["type"] == A.T_DIELECTRIC).any() else None
        if k is not None:
            e = f32(s.materials["extra_data"][k])
            inv = f32(1.0) / e
            assert b[2 * k + 1, 1] == inv
            assert b[2 * k + 1, 2] == ((f32(1.0) - e) / (f32(1.0) + e)) ** 2 and b[2 * k + 1, 3] == ((f32(1.0) - inv) / (f32(1.0) + inv)) ** 2


def test_a_set_over_its_cap_has_no_rows():
    s = rt.workloads.get("c2", width=16, height=16).scene
    nm, ns, npl = len(s.materials), len(s.spheres), len(s.planes)
    assert A.stage_block_layout(A.LDS_MATERIALS, ns, npl)[3] == 2 * A.LDS_MATERIALS + 2 * ns + npl
    assert A.stage_block_layout(A.LDS_MATERIALS + 1, ns, npl) == (0, 0, 2 * ns, 2 * ns + npl)
    assert A.stage_block_layout(nm, A.LDS_WINNERS + 1, npl) == (0, 2 * nm, 2 * nm, 2 * nm + npl)
    assert A.stage_block_layout(nm, ns, A.LDS_PLANES + 1) == (0, 2 * nm, 2 * nm + 2 * ns, 2 * nm + 2 * ns)
    assert A.stage_block_layout(A.LDS_MATERIALS + 1, A.LDS_WINNERS + 1, A.LDS_PLANES + 1)[3] == 0
    for _ in range(A.LDS_MATERIALS):
        s.addMaterial(A.T_DIFFUSE, (0.5, 0.5, 0.5), 1.0)
    b = W.stage_block(s)   # materials left out: sphere and plane records only
    assert b.shape == (2 * ns + npl, 4) and np.array_equal(b[0:2 * ns:2, 3], s.spheres["r"])


def test_tile_quotient_is_exact_for_every_divisor_and_reciprocal():
    """stage_xy: ty = (uint32)(((float)t + 0.5f) * rcp((float)tiles_x)) == t // tiles_x for t < 2^20 — every divisor up to
    RT_MAX_DIM / 8 + 1 (the default 8 x 8 tiles) and a sample of larger ones (smaller tiles), each with the correctly
    rounded reciprocal and its two neighbours (v_rcp_f32 is within 1 ulp), at t = 0, 1, around every kind of multiple of
    the divisor and at the top of the range."""
    top = W.XY_FAST_MAX_TILES - 1
    header = open(os.path.join(cases.ROOT, "include", "rt_amd.h")).read()
    max_div = int(_define(header, "RT_MAX_DIM")) // 8 + 1
    divisors = list(range(1, max_div + 1)) + [4095, 4096, 4097, 16383, 16384, 65535, 65536, 99991, 1 << 19, top, top + 1]
    rng = np.random.RandomState(5)
    for d in divisors:
        kmax = top // d
        ks = np.unique(np.concatenate([np.arange(0, min(kmax, 3) + 1), [kmax // 2, kmax - 1, kmax], rng.randint(0, kmax + 1, 24)]))
        ks = ks[(ks >= 0)].astype(np.int64)
        t = np.concatenate([ks * d - 1, ks * d, ks * d + 1, ks * d + d // 2, [0, 1, d - 1, d, d + 1, top - 1, top]])
        t = np.unique(t[(t >= 0) & (t <= top)]).astype(np.uint32)
        exact = f32(1.0) / f32(d)
        for rcp in (np.nextafter(exact, f32(0)), exact, np.nextafter(exact, f32(2))):
            q = W.tile_quotient(t, d, rcp)
            assert np.array_equal(q, t // np.uint32(d)), (d, float(rcp), t[q != t // np.uint32(d)][:4])


def test_tile_quotient_exhaustive_for_the_headline_frame():
    """1920 x 1080 in 8 x 8 tiles: every tile index, and every index up to the bound for that divisor."""
    d = 1920 // 8
    t = np.arange(W.XY_FAST_MAX_TILES, dtype=np.uint32)
    exact = f32(1.0) / f32(d)
    for rcp in (np.nextafter(exact, f32(0)), exact, np.nextafter(exact, f32(2))):
        assert np.array_equal(W.tile_quotient(t, d, rcp), t // np.uint32(d))


# ---- the LDS granule -----------------------------------------------------------------------------------------------------
def pixels_per_wave(count, waves, static_f4, granule, slots=512, max_pixels=16, min_samples=384):
    """queue_pixels_per_wave (csrc/pt_kernels.hip) restated: a CU's 160 KiB of LDS shared by 4 x waves one-wave workgroups,
    the share rounded DOWN to the allocation granule; the 5-per-SIMD budget where a wave would own fewer than 384 samples."""
    def fit(w):
        budget = 163840 // (4 * w) // granule * granule
        p = (budget - 16 * static_f4 - 15) // (96 + 12 * count)   # (5 + 1 float4 of record and coordinates, 12 bytes a sample)
        return min(p, slots // count, max_pixels)
    p = fit(waves)
    if p * count < min_samples:
        p = max(p, fit(5))
    return max(p, 1)


def test_pixels_per_wave_under_both_granules(built):
    kernels = open(os.path.join(CSRC, "pt_kernels.hip")).read()
    shipped = int(re.search(r"#define PT_LDS_GRANULE (\d+)u", kernels).group(1))
    assert shipped in (1024, 1280)
    c2 = rt.workloads.get("c2", width=16, height=16).scene
    static_c2 = A.stage_block_layout(len(c2.materials), len(c2.spheres), len(c2.planes))[3]
    for static_f4 in (0, static_c2, 2 * 64 + 2 * 64 + 16):
        for waves in (5, 6):
            for count in (16, 32, 64, 128, 256):
                for granule in (1024, 1280):
                    got = rt.raytracer.queue_pixels(count, waves, static_f4, granule)
                    assert got == pixels_per_wave(count, waves, static_f4, granule), (count, waves, static_f4, granule)
                    # the request never exceeds the granule-rounded share of its occupancy (or of 5 per SIMD)
                    lds = 16 * static_f4 + ((got * (96 + 12 * count) + 15) & ~15)
                    assert got == 1 or lds <= max(163840 // (4 * waves) // granule * granule, 163840 // 20 // granule * granule)
                assert rt.raytracer.queue_pixels(count, waves, static_f4, 0) == rt.raytracer.queue_pixels(count, waves, static_f4, shipped)
    # the headline: C2 at 64 spp owns 6 pixels under either granule.  At 32 spp a share of 6 144 bytes holds 11 pixels = 352
    # samples, fewer than the 384 below which the 5-per-SIMD budget is taken: 15 pixels; a share of 6 400 bytes holds 12 =
    # 384 samples and stays at 6 per SIMD
    assert [rt.raytracer.queue_pixels(64, 6, static_c2, g) for g in (1024, 1280)] == [6, 6]
    assert [pixels_per_wave(32, 6, static_c2, g, min_samples=0) for g in (1024, 1280)] == [11, 12]
    assert [rt.raytracer.queue_pixels(32, 6, static_c2, g) for g in (1024, 1280)] == [15, 12]
    # 5 waves per SIMD: 8 192 bytes is a multiple of 1 024 but not of 1 280 — the share shrinks to 7 680
    assert pixels_per_wave(16, 5, 0, 1024) >= pixels_per_wave(16, 5, 0, 1280)
    for bad in ((0, 6, 0, 0), (64, 0, 0, 0), (64, 9, 0, 0), (64, 6, 0, 8), (64, 6, 100000, 0)):
        try:
            rt.raytracer.queue_pixels(*bad)
            assert False, bad
        except rt.raytracer.RtError:
            pass
