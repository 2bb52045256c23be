"""CPU: feature records through per-sample cameras (rt_render_features_cameras) — the header's new declarations as plain
C and the exported symbols, the launcher's plan (rt_debug_plan_feature_cameras, the launcher's own function) against its
restatement, and the properties of the reduction's numpy restatement (tests/feature_cameras_ref.py) on synthetic
records: the n = 1 identity, the tie rule, miss-dominant pixels, signed zeros and the padded lane, sums across groups."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import feature_cameras_ref as F

rt = cases.rt
A = rt._abi
ROOT = cases.ROOT
f32 = np.float32
EINVAL = -1
NEW_SYMBOLS = ("rt_render_features_cameras", "rt_read_feature_coverage", "rt_device_feature_coverage",
               "rt_debug_plan_feature_cameras")


def test_header_compiles_as_plain_c_and_the_symbols_are_exported(built, tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "rt_amd.h"\n'
                   "int use(rt_context *c, const float *cams, float *cov, size_t bytes) {\n"
                   "    rt_feature_chain_params p = {RT_FOLLOW_REFLECTIVE, RT_FEATURE_CHAIN_MAX};\n"
                   "    uint32_t plan[3]; void *d = 0;\n"
                   "    if (rt_debug_plan_feature_cameras(61, 37, RT_FEATURE_CAMERAS_MAX, plan)) return 1;\n"
                   "    if (rt_render_features_cameras(c, cams, 16u, &p) || rt_render_features_cameras(c, cams, 1u, 0)) return 2;\n"
                   "    if (rt_device_feature_coverage(c, &d)) return 3;\n"
                   "    return rt_read_feature_coverage(c, cov, bytes) + (int)RT_FEATURE_MIXED;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)
    lib = rt.load_library()
    for s in NEW_SYMBOLS:
        assert s in rt.raytracer.SYMBOLS and getattr(lib, s)
    assert lib.rt_abi_version() == 3
    assert A.FEATURE_MIXED == F.MIXED == 4 and A.FEATURE_CAMERAS_MAX == F.CAMERAS_MAX == 64


# ---- the plan ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1, 1), (61, 37), (1920, 1080), (16384, 16384)], ids=lambda s: "%dx%d" % s)
def test_the_plan_equals_its_restatement(built, size):
    w, h = size
    for n in range(1, 65):
        got = rt.plan_feature_cameras(w, h, n)
        assert got == F.plan(w, h, n), (w, h, n)
        glog2, groups, threads = got
        assert threads == 256 and (1 << glog2) >= n and (glog2 == 0 or (1 << (glog2 - 1)) < n)
        assert groups * (256 >> glog2) >= w * h > (groups - 1) * (256 >> glog2) and groups < 2 ** 32
    assert rt.RayTracer.planFeatureCameras(w, h, 16) == rt.plan_feature_cameras(w, h, 16)


def test_hand_written_plan_rows(built):
    assert rt.plan_feature_cameras(1, 1, 1) == (0, 1, 256)
    assert rt.plan_feature_cameras(61, 37, 16) == (4, 142, 256)            # 2257 pixels, 16 to a workgroup
    assert rt.plan_feature_cameras(61, 37, 3) == (2, 36, 256)              # 64 to a workgroup
    assert rt.plan_feature_cameras(1920, 1080, 16) == (4, 129600, 256)
    assert rt.plan_feature_cameras(16384, 16384, 64) == (6, 1 << 26, 256)


def test_the_plan_refuses_what_no_launch_can_have(built):
    lib = rt.load_library()
    out = (C.c_uint32 * 3)()
    for w, h, n in ((0, 4, 1), (4, 0, 1), (-1, 4, 1), (16385, 4, 1), (4, 16385, 1), (4, 4, 0), (4, 4, 65), (4, 4, 0xFFFFFFFF)):
        assert lib.rt_debug_plan_feature_cameras(w, h, n, out) == EINVAL, (w, h, n)
        with pytest.raises(rt.RtError):
            rt.plan_feature_cameras(w, h, n)
    assert lib.rt_debug_plan_feature_cameras(4, 4, 4, None) == EINVAL
    assert lib.rt_debug_plan_feature_cameras(16384, 16384, 64, out) == 0


# ---- the restatement on synthetic records --------------------------------------------------------------------------------

def hit_record(obj, pos=(1.0, 2.0, 3.0), t=4.0, normal=(0.0, 1.0, 0.0), albedo=(0.5, 0.25, 0.125), chain=0, material=7, face=A.NO_ID,
               direction=(0.0, 0.0, 1.0), uv=(0.0, 0.0), tex=0, cut=False):
    r = np.zeros((), A.FEATURE)
    r["pos"], r["t"], r["normal"], r["albedo"] = pos, t, normal, albedo
    r["object"], r["material"], r["face"], r["dir"] = obj, material, face, direction
    r["u"], r["v"], r["tex"] = uv[0], uv[1], tex
    r["flags"] = A.FEATURE_HIT | (A.FEATURE_CUT if cut else 0) | (chain << 8)
    return r


def miss_record(chain=0, direction=(0.0, 0.0, 1.0)):
    r = np.zeros((), A.FEATURE)
    r["t"] = np.inf
    r["object"] = r["material"] = r["face"] = A.NO_ID
    r["dir"] = direction
    r["flags"] = chain << 8
    return r


def one_pixel(samples):
    rec = np.array(samples, dtype=A.FEATURE).reshape(len(samples), 1)
    out, cov = F.aggregate(rec, len(samples))
    return out[0], cov[0]


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def test_one_sample_is_the_record_itself():
    rng = np.random.RandomState(3)
    rec = np.zeros((1, 50), A.FEATURE)
    raw = rng.randint(0, 2 ** 32, size=(50, 20), dtype=np.uint64).astype(np.uint32)
    rec[0] = raw.view(A.FEATURE).reshape(50)
    rec["flags"] &= ~np.uint32(A.FEATURE_MIXED)
    finite = np.isfinite(rec["pos"]).all(-1) & np.isfinite(rec["t"]) & np.isfinite(rec["normal"]).all(-1) & np.isfinite(rec["albedo"]).all(-1)
    rec = rec[:, finite[0]]
    assert rec.shape[1] >= 40
    out, cov = F.aggregate(rec, 1)
    assert out.tobytes() == rec[0].tobytes()
    hit = (rec[0]["flags"] & A.FEATURE_HIT) != 0
    assert hit.any() and (~hit).any()
    assert np.array_equal(cov, np.stack([hit.astype(f32), np.ones(len(hit), f32)], -1))


@pytest.mark.parametrize("n", [2, 4, 16, 64])
def test_identical_samples_of_a_power_of_two_are_the_record_itself(n):
    for r in (hit_record(5, pos=(0.1, -0.7, 1e-3), t=3.3, normal=(-0.0, 0.6, 0.8), albedo=(0.3, 0.7, 0.9), chain=0x1234), miss_record(3)):
        out, cov = one_pixel([r] * n)
        assert out.tobytes() == np.asarray(r).tobytes()
        assert cov.tolist() == [1.0 if r["flags"] & 1 else 0.0, 1.0]


def test_two_groups_of_equal_size_the_one_with_the_smallest_j_wins():
    a, b = hit_record(1, material=11, direction=(1.0, 0.0, 0.0)), hit_record(2, material=22, direction=(0.0, 1.0, 0.0))
    for order, first in (([a, b], a), ([b, a], b), ([a, b, b, a], a), ([b, a, a, b], b), ([b, b, a, a], b), ([a, a, b, b], a)):
        out, cov = one_pixel(order)
        assert out["object"] == first["object"] and out["material"] == first["material"]
        assert out["dir"].tobytes() == order[0]["dir"].tobytes()                  # j* = 0: the smallest j of the winner
        assert out["flags"] == first["flags"] | A.FEATURE_MIXED
        assert cov.tolist() == [1.0, 0.5]


def test_three_way_ties_and_the_representative_inside_the_winner():
    a, b, c = hit_record(1), hit_record(2), miss_record()
    out, cov = one_pixel([c, a, b])                       # three groups of one: the miss holds j = 0
    assert out["object"] == A.NO_ID and out["flags"] == A.FEATURE_MIXED and out["t"] == np.inf
    assert bits(cov).tolist() == bits([f32(2) / f32(3), f32(1) / f32(3)]).tolist()
    out, cov = one_pixel([b, c, a, a, c, b])              # three groups of two
    assert out["object"] == 2 and cov.tolist() == [f32(4) / f32(6), f32(2) / f32(6)]
    # a larger group beats a smaller one that holds j = 0, and its representative is ITS smallest j
    a1, a2 = hit_record(1, direction=(1.0, 0.0, 0.0), uv=(0.25, 0.5)), hit_record(1, direction=(0.0, 1.0, 0.0), uv=(0.75, 0.5))
    out, cov = one_pixel([b, a2, a1])
    assert out["object"] == 1 and out["dir"].tolist() == [0.0, 1.0, 0.0] and out["u"] == f32(0.75)
    assert out["flags"] & A.FEATURE_MIXED and cov.tolist() == [1.0, f32(2) / f32(3)]
    # the chain word is part of the key: the same object behind different chains is two groups
    out, cov = one_pixel([hit_record(1, chain=0x10001), hit_record(1, chain=0x20001), hit_record(1, chain=0x20001)])
    assert out["flags"] == (A.FEATURE_HIT | A.FEATURE_MIXED | (0x20001 << 8)) and cov[1] == f32(2) / f32(3)
    # CUT is not: it rides on the representative
    out, cov = one_pixel([hit_record(1, cut=True), hit_record(1)])
    assert out["flags"] == A.FEATURE_HIT | A.FEATURE_CUT and cov.tolist() == [1.0, 1.0]


def test_a_miss_dominant_pixel_keeps_the_miss_values():
    out, cov = one_pixel([miss_record(direction=(0.0, 1.0, 0.0)), hit_record(1), miss_record(), miss_record()])
    assert out["t"] == np.inf and not out["pos"].any() and not out["normal"].any() and not out["albedo"].any()
    assert bits(out["pos"]).tolist() == [0, 0, 0]                                     # +0, not a sum
    assert out["object"] == out["material"] == out["face"] == A.NO_ID and out["dir"].tolist() == [0.0, 1.0, 0.0]
    assert out["flags"] == A.FEATURE_MIXED and cov.tolist() == [0.25, 0.75]
    assert (out["flags"] & 1 != 0) == bool(out["t"] < np.inf)


def test_negative_zero_components_and_the_padded_lane():
    nz = hit_record(1, pos=(-0.0, -0.0, 5.0), normal=(-0.0, 1.0, -0.0))
    out, _ = one_pixel([nz])                                  # g = 1: no addition at all
    assert bits(out["pos"]).tolist() == bits([-0.0, -0.0, 5.0]).tolist()
    out, _ = one_pixel([nz, nz])                              # g = 2, no padding: (-0) + (-0) = -0, / 2 = -0
    assert bits(out["pos"]).tolist() == bits([-0.0, -0.0, 5.0]).tolist()
    assert bits(out["normal"]).tolist() == bits([-0.0, 1.0, -0.0]).tolist()
    out, _ = one_pixel([nz, nz, nz])                          # g = 4: lane 3 holds +0, and (-0) + (+0) = +0
    assert bits(out["pos"]).tolist() == bits([0.0, 0.0, f32(15.0) / f32(3.0)]).tolist()
    out, cov = one_pixel([nz, miss_record()])                 # a missed sample's lane holds +0 as well
    assert bits(out["pos"]).tolist() == bits([0.0, 0.0, 5.0]).tolist() and cov.tolist() == [0.5, 0.5]


def test_sums_run_over_the_hits_of_every_group_in_butterfly_order():
    rng = np.random.RandomState(11)
    n, g = 6, 8
    vals = (rng.standard_normal((n, 10)) * [1e3, 1.0, 1e-3, 50.0, 1.0, 1.0, 1.0, 0.5, 0.5, 0.5]).astype(f32)
    objs = [1, 2, 1, A.NO_ID, 3, 1]
    samples = [miss_record() if o == A.NO_ID else hit_record(o, pos=v[:3], t=v[3], normal=v[4:7], albedo=v[7:]) for o, v in zip(objs, vals)]
    out, cov = one_pixel(samples)
    assert out["object"] == 1 and cov.tolist() == [f32(5) / f32(6), 0.5]
    lanes = np.zeros((g, 10), f32)
    lanes[:n] = vals
    lanes[3] = 0.0
    # the tree written out: offsets 4, 2, 1
    s4 = [f32(lanes[l] + lanes[l ^ 4]) for l in range(8)]
    s2 = [f32(s4[l] + s4[l ^ 2]) for l in range(8)]
    s1 = f32(s2[0] + s2[1])
    exp = (s1 / f32(5)).astype(f32)
    got = np.concatenate([out["pos"], [out["t"]], out["normal"], out["albedo"]]).astype(f32)
    assert bits(got).tolist() == bits(exp).tolist()
    # and it is not the left-to-right sum of the dominant group alone
    alone = (vals[[0, 2, 5]].sum(0, dtype=f32) / f32(3)).astype(f32)
    assert bits(got).tolist() != bits(alone).tolist()


def test_census_counts_what_it_says():
    a, b, c = hit_record(1), hit_record(2), miss_record()
    pixels = [[a, a, a, a], [a, a, b, b], [a, b, b, b], [a, c, a, a]]        # pure; tied; mixed; mixed with a miss
    rec = np.ascontiguousarray(np.array(pixels, dtype=A.FEATURE).T)           # [n = 4, P = 4]
    assert F.census(rec) == dict(mixed=3, hit_and_miss=1, ties=1)


def test_sample_blocks_is_untouched():
    """The guide pass takes Camera.sampleBlocks as it is: block j of n blocks from sample 0 is what renderFrameCameras sees."""
    cam = rt.Camera(60, 16.0 / 9.0, pos=(-8.0, -1.0, -8.0), y=45.0, p=0.0)
    blocks = cam.sampleBlocks(16, 0, 96, 54, True, 0.05, 8.0)
    assert blocks.shape == (16, 12) and blocks.dtype == np.float32
    assert np.array_equal(cam.sampleBlocks(4, 0, 96, 54, True, 0.05, 8.0), blocks[:4])
    assert np.array_equal(cam.sampleBlocks(3, 0, 96, 54, False, 0.0, 1.0), np.repeat(cam.transferData()[None], 3, 0))


def test_cli_refuses_aa_guides_without_its_frame_or_its_use(built):
    cli = os.path.join(cases.ROOT, "host", "rt_cli")
    for flags in (["--aa-guides", "16", "--denoise"], ["--aa", "--aa-guides", "16"], ["--aa", "--aa-guides", "0", "--denoise"],
                  ["--aa", "--aa-guides", "65", "--denoise"]):
        p = subprocess.run([cli, "--size", "16x8", "--spp", "1"] + flags, capture_output=True, text=True, cwd=cases.ROOT)
        assert p.returncode == 2, flags
