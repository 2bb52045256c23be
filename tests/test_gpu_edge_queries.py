"""GPU (-m gpu): the degenerate scenes of tests/edge_scenes.py through every entry point that is not a trace kernel — the
feature kernels (pt_features, pt_features_chain, pt_features_rays, pt_features_cameras), the any-hit search behind
rt_occluded_rays, the hemisphere rays of rt_occluded_hemispheres and the caller-supplied-ray sample kernels — at 48 x 32,
under the three arithmetic policies, with the ray batch of tests/edge_rays.py: primary rays, rays that start ON surfaces,
axis-parallel directions, the zero direction and directions of length 1.1, 2 and 1e-3, from the eye, from sphere centres
and from plane points.  tests/test_edge_queries_host.py pins the CPU side of every comparison to the compiled reference.

All comparisons are on bit patterns, NaN matching NaN in float fields; rt_walk_overflow is 0 after every step.

RT_FEATURE_CHAIN_MAX is 29: rt_render_features_chain refuses max_chain 30 (include/rt_amd.h), so the long chains run with
(FOLLOW_ALL, 29) on the device — 30 searches per pixel, the kernel's loop bound — and the test asserts the refusal of 30;
the host replay of tests/test_edge_queries_host.py runs at 30."""
import numpy as np
import pytest

import cases
import chain_ref as CH
import edge_rays as ER
import edge_scenes as E
import hemisphere_ref as HR
import ray_queries_ref as Q
from test_gpu_hemispheres import RAY_BOUND

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
R = rt.raytracer
T = rt.RayTracer
rays_mod = rt.rays
F32 = np.float32
EINVAL = -1
POLICIES = [0, 1, 2]
FOLLOW_ALL = rt.FOLLOW_ALL
CHAINS = ((0, 0), (FOLLOW_ALL, 3), (FOLLOW_ALL, A.FEATURE_CHAIN_MAX))
K = 8
INF = float("inf")
POISON = 0xDEADBEEF
FLOAT_FIELDS = ("pos", "t", "normal", "albedo", "dir", "u", "v")
WORD_FIELDS = ("object", "material", "face", "tex", "flags")


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def same_floats(a, b):
    """element-wise: the same bits, or NaN on both sides"""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same_floats(a, b, what):
    same = same_floats(a, b)
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist())


def assert_same_records(got, exp, what, fields=FLOAT_FIELDS + WORD_FIELDS):
    got, exp = np.asarray(got).reshape(-1), np.asarray(exp).reshape(-1)
    assert got.shape == exp.shape, what
    for f in fields:
        a, b = got[f].reshape(len(got), -1), exp[f].reshape(len(exp), -1)
        same = (same_floats(a, b) if f in FLOAT_FIELDS else a == b).all(1)
        assert same.all(), "%s: field %s differs in %d of %d records, first %d: %r != %r" % (
            what, f, (~same).sum(), len(same), np.nonzero(~same)[0][0], a[~same][0], b[~same][0])


def accel_settings(name):
    return (1, 0, 2) if name in E.SPHERE_BVH else (1, 0)


def rays_to_device(batch):
    import torch
    d = torch.from_numpy(rays_mod.as_floats(batch).copy()).cuda()
    torch.cuda.synchronize()
    return d


def intersect(t, d_rays, follow=0, max_chain=0):
    """→ ((n,) FEATURE on the host, the (n, 20) device tensor)"""
    out = t.intersectRays(d_rays, follow, max_chain)
    t.sync()
    return A.feature_records(out), out


def occluded(t, d_rays, set_size=1, t_max=INF, bounds=None):
    """occludedRays into a poisoned output → (n_sets,) uint32"""
    import torch
    n = int(d_rays.shape[0]) // set_size
    out = torch.full((n,), POISON - (1 << 32), dtype=torch.int32, device="cuda")
    b = None if bounds is None else torch.from_numpy(np.ascontiguousarray(bounds, dtype=F32)).cuda()
    torch.cuda.synchronize()
    assert t.occludedRays(d_rays, set_size, t_max, b, out=out) is out
    t.sync()
    return out.cpu().numpy().view(np.uint32)


def hemispheres(t, feats, n, counts=True, rays=True, **kw):
    """One rt_occluded_hemispheres call into poisoned outputs → (counts (n,) uint32 | None, rays (n, K) RAY | None, the
    device tensor of the rays | None)"""
    import torch
    c = torch.full((n,), POISON - (1 << 32), dtype=torch.int32, device="cuda") if counts else None
    r = torch.full((n * K, 8), POISON - (1 << 32), dtype=torch.int32, device="cuda").view(torch.float32) if rays else None
    torch.cuda.synchronize()
    if counts:
        assert t.occludedHemispheres(feats, K, out=c, rays_out=r, **kw) is c
    else:
        kw.pop("t_max", None)
        assert t.spawnHemispheres(feats, K, out=r, **kw) is r
    t.sync()
    return (c.cpu().numpy().view(np.uint32) if counts else None, r.cpu().numpy().view(A.RAY).reshape(n, K) if rays else None, r)


def read_accum(t):
    import torch
    t.sync()
    return torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().copy().reshape(-1, 4)


def primary_batch(t, camera):
    """The camera's primary rays with the selected policy's own direction bits, ids = pixel coordinates → RAY (h * w,)"""
    t.renderFeatures(camera)
    rec = t.featureRecords()
    ys, xs = np.mgrid[0:E.H, 0:E.W]
    return rays_mod.pack_rays(np.asarray(camera, F32)[0:3], rec["dir"].reshape(-1, 3), ids=np.stack([xs.ravel(), ys.ravel()], axis=1))


# ---- one context per scene, and the host side of a scene made once --------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(E.SCENES))
def tracer(request):
    s, cam = E.get(request.param)
    t = T(E.W, E.H, scene=s, seed=cases.SEED)
    yield request.param, t, s, np.asarray(cam, F32).reshape(12)
    t.setArith(rt.ARITH_IEEE)
    t.close()     # (asserts that no walk ended on its loop bound: tests/conftest.py)


@pytest.fixture
def ready(tracer, request):
    """The scene's context under the test's policy, default options before and after"""
    name, t, s, cam = tracer
    t.setArith(request.node.callspec.params["policy"])
    yield name, t, s, cam
    t.setOption(T.OPT_ACCEL, 1)
    t.setOption(T.OPT_SAMPLE_QUEUE, 1)
    assert t.walkOverflow() == 0


_edge = {}
_oracle_replays = {}


def edge_batch(oracle, name):
    """(rays (n, 6), RAY records, the oracle's hitScene records (n, 12)): the same batch under every policy"""
    if name not in _edge:
        s, cam = E.get(name)
        rays6 = ER.edge_rays(oracle, s, cam)
        out = ER.scene_hits(oracle, s, rays6)
        for a in (rays6, out):
            a.setflags(write=False)
        _edge[name] = rays6, rays_mod.pack_rays(rays6[:, :3], rays6[:, 3:]), out
    return _edge[name]


# ---- a. feature records from the camera -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_feature_records_are_the_host_replay(ready, policy, oracle, table):
    name, t, s, cam = ready
    first = None
    for follow, max_chain in CHAINS:
        frames = []
        for accel in (1, 0):
            t.setOption(T.OPT_ACCEL, accel)
            if max_chain:
                t.renderFeaturesChain(cam, follow, max_chain)
            else:
                t.renderFeatures(cam)
            frames.append(t.featureRecords().reshape(-1).copy())
            assert t.walkOverflow() == 0, (name, follow, max_chain, accel)
        rec = frames[0]
        assert_same_records(frames[1], rec, "RT_OPT_ACCEL 0 against 1, chain %d" % max_chain)
        exp, chain = CH.replay(CH.DeviceProbes(t), s, cam[:3], rec["dir"], follow, max_chain, identify=CH.identify_by_probe)
        assert_same_records(rec, exp, "device probes, chain %d" % max_chain)
        if policy == rt.ARITH_IEEE:
            key = (name, follow, max_chain)
            if key not in _oracle_replays:
                _oracle_replays[key] = CH.replay(CH.OracleProbes(oracle, s, table), s, cam[:3], rec["dir"].copy(), follow, max_chain,
                                                 identify=CH.identify_by_probe)[0]
            assert_same_records(rec, _oracle_replays[key], "CPU oracle, chain %d" % max_chain)
        f = A.split_features(rec)
        n = f["chain_length"]
        print(name, policy, "chain", max_chain, "hits", int(f["hit"].sum()), "longest", int(n.max()), "cut", int(f["cut"].sum()))
        assert np.array_equal(f["hit"], rec["t"] < np.inf) and f["hit"].any()
        for r, c in zip(rec, chain):
            assert (int(r["flags"]) >> 8) & 31 == len(c) and int(r["flags"]) & 0xFFFF0000 == rt.feature_chain_signature(c) & 0xFFFF0000
        if max_chain == 0:
            first = rec
            for fo, mc in ((FOLLOW_ALL, 0), (0, A.FEATURE_CHAIN_MAX)):          # (follow, 0) is the first-hit record
                t.renderFeaturesChain(cam, fo, mc)
                assert_same_records(t.featureRecords(), first, "(follow, max_chain) = (%d, %d)" % (fo, mc))
        if name == "facing_mirrors" and max_chain:
            assert n.max() == max_chain and f["cut"].sum() >= 1000 and (n[f["cut"]] == max_chain).all()
        if name == "lenses" and max_chain:
            assert n.max() >= 3
    with pytest.raises(R.RtError) as e:                                            # the documented limit: 29 followed vertices
        t.renderFeaturesChain(cam, FOLLOW_ALL, A.FEATURE_CHAIN_MAX + 1)
    assert e.value.code == EINVAL
    assert_same_records(t.featureRecords(), rec, "after the refused call")          # a failed call makes nothing


# ---- b. nearest hits of the edge rays -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_nearest_hits_of_the_edge_rays(ready, policy, oracle, table):
    name, t, s, cam = ready
    rays6, batch, out = edge_batch(oracle, name)
    d = rays_to_device(batch)
    recs = []
    for accel in accel_settings(name):
        t.setOption(T.OPT_ACCEL, accel)
        recs.append(intersect(t, d)[0])
        assert t.walkOverflow() == 0, (name, accel)
        assert_same_records(recs[-1], recs[0], "RT_OPT_ACCEL %d against 1" % accel)
    t.setOption(T.OPT_ACCEL, 1)
    rec = recs[0]
    hit = (rec["flags"] & A.FEATURE_HIT) != 0
    assert (rec["flags"] & ~np.uint32(A.FEATURE_HIT) == 0).all()
    assert np.isposinf(rec["t"][~hit]).all() and (rec["t"][hit] < np.inf).all()
    assert (rec["object"][~hit] == A.NO_ID).all() and (rec["material"][~hit] == A.NO_ID).all()
    assert_same_floats(rec["dir"], rays6[:, 3:], "dir as given")
    for n in (1, 63, 65):                                                          # sub-batches from the middle
        a = (len(batch) - n) // 2 + 3
        sub, _ = intersect(t, rays_to_device(batch[a:a + n]))
        assert_same_records(sub, rec[a:a + n], "a sub-batch of %d" % n)
    print(name, policy, "records", len(rec), "hits", int(hit.sum()))
    if policy == rt.ARITH_IEEE:
        o_hit = out[:, 0] > 0
        assert np.array_equal(hit, o_hit), np.flatnonzero(hit != o_hit)[:10]
        for field, cols in (("t", out[:, 1]), ("pos", out[:, 2:5]), ("normal", out[:, 5:8]), ("u", out[:, 8]), ("v", out[:, 9])):
            assert_same_floats(rec[field][hit], cols[hit], field)
        assert np.array_equal(rec["tex"][hit], CH.bits(out[hit, 10])) and np.array_equal(rec["material"][hit], CH.bits(out[hit, 11]))
        obj, face = CH.identify_by_probe(CH.OracleProbes(oracle, s, table), s, rays6[hit], out[hit], np.ones(int(hit.sum()), bool))
        assert np.array_equal(rec["object"][hit], obj), np.flatnonzero(rec["object"][hit] != obj)[:10]
        assert np.array_equal(rec["face"][hit], face), np.flatnonzero(rec["face"][hit] != face)[:10]


# ---- c. occlusion is its definition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_occlusion_is_its_definition(ready, policy, oracle):
    name, t, s, cam = ready
    rays6, batch, out = edge_batch(oracle, name)
    d = rays_to_device(batch)
    rec, _ = intersect(t, d)
    tt = rec["t"].astype(F32)
    hit = (rec["flags"] & A.FEATURE_HIT) != 0
    bounds = Q.cycled_bounds(tt)
    want = Q.occluded(tt, bounds)
    assert want.sum() >= 1000 and (hit & ~want).sum() >= 1000
    sizes = (3, 64, 100)
    for accel in accel_settings(name):
        t.setOption(T.OPT_ACCEL, accel)
        got = occluded(t, d, bounds=bounds)
        assert set(np.unique(got)) <= {0, 1}
        differ = np.flatnonzero(got.astype(bool) != want)
        print(name, policy, "accel", accel, "records", len(batch), "occluded", int(want.sum()), "differ", len(differ))
        assert not len(differ), (name, policy, accel, differ[:10].tolist(), rays6[differ[:4]].tolist(), tt[differ[:4]], bounds[differ[:4]])
        any_hit = occluded(t, d)                                                   # no bounds, t_max +inf: the hit flag
        assert np.array_equal(any_hit.astype(bool), hit), np.flatnonzero(any_hit.astype(bool) != hit)[:10]
        for k in sizes:
            m = len(batch) // k * k
            counts = occluded(t, d[:m], set_size=k, bounds=bounds[:m])
            assert np.array_equal(counts, got[:m].reshape(-1, k).sum(1)), (name, policy, accel, k)
            counts = occluded(t, d[:m], set_size=k)
            assert np.array_equal(counts, any_hit[:m].reshape(-1, k).sum(1)), (name, policy, accel, k)
        if policy == rt.ARITH_IEEE:
            t_ref = np.where(out[:, 0] > 0, out[:, 1], F32(np.inf)).astype(F32)
            b_ref = Q.cycled_bounds(t_ref)
            assert np.array_equal(occluded(t, d, bounds=b_ref).astype(bool), Q.occluded(t_ref, b_ref))
        assert t.walkOverflow() == 0, (name, accel)


# ---- d. hemispheres --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_hemisphere_counts_and_rays(ready, policy, oracle):
    name, t, s, cam = ready
    rays6, batch, _ = edge_batch(oracle, name)
    t.renderFeatures(cam)
    own = t.featureRecords().reshape(-1).copy()
    edge, d_edge = intersect(t, rays_to_device(batch))
    for what, rec, feats in (("the frame's records", own, None), ("the edge rays' records", edge, d_edge)):
        n = len(rec)
        mask = HR.valid_mask(rec)
        assert mask.sum() >= 500, (what, int(mask.sum()))
        for accel in (1, 0):
            t.setOption(T.OPT_ACCEL, accel)
            tag = (name, policy, what, accel)
            kw = dict(seed=7, offset=0.0, face_forward=True)
            fused, none, _ = hemispheres(t, feats, n, True, False, t_max=INF, **kw)
            both, dumped, d_rays = hemispheres(t, feats, n, True, True, t_max=INF, **kw)
            _, spawned, _ = hemispheres(t, feats, n, False, True, **kw)
            assert none is None and spawned.tobytes() == dumped.tobytes(), tag
            assert np.array_equal(fused, both), tag
            want = occluded(t, d_rays, K, INF)
            assert np.array_equal(fused[mask], want[mask]), (tag, np.flatnonzero(mask & (fused != want))[:10])
            assert not fused[~mask].any() and not dumped[~mask].view(np.uint8).any(), tag
            assert fused.max() <= K
            print(name, policy, what, "accel", accel, "valid", int(mask.sum()), "of", n, "occluded", int(fused.sum()), "of", int(mask.sum()) * K)
            assert t.walkOverflow() == 0, tag
        # the rays are the float64 generator's, as tests/test_gpu_hemispheres.py compares them
        _, got, _ = hemispheres(t, feats, n, False, True, seed=7, offset=0.0, face_forward=False)
        ref_mask, ref = HR.hemisphere_rays(rec, K, 7, 0.0, False)
        assert np.array_equal(ref_mask, mask)
        assert not got[~mask].view(np.uint8).any()
        assert (got["x"][mask] == np.arange(n, dtype=np.uint32)[mask, None]).all() and (got["y"] == 0).all()
        dd = got["d"][mask].astype(np.float64)
        cos = (dd * HR.unit_normals(rec, False)[mask][:, None, :]).sum(-1)
        dev_d = np.abs(dd - ref["d"][mask]).max()
        dev_o = np.abs(got["o"][mask].astype(np.float64) - ref["o"][mask]).max()
        dev_len = np.abs(np.sqrt((dd * dd).sum(-1)) - 1.0).max()
        print(name, policy, what, "max |d - ref| %.3g  |o - ref| %.3g  ||d| - 1| %.3g  min cos %.3g (bound %.3g)" % (dev_d, dev_o, dev_len, cos.min(), RAY_BOUND))
        assert cos.min() > 0
        assert dev_d <= RAY_BOUND and dev_o <= RAY_BOUND and dev_len <= RAY_BOUND, (name, policy, what)
        assert (got["o"][mask] == rec["pos"][mask][:, None, :]).all()               # offset 0: the origin is the point itself
    if name == "plane_normals":
        length = np.linalg.norm(own["normal"].astype(np.float64), axis=1)
        assert (np.abs(length[HR.valid_mask(own)] - 3.0) < 1e-6).sum() >= 100      # the (0, 3, 0) floor is among them


# ---- e. the caller-ray sample kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_ray_sample_kernels_are_the_frame(ready, policy):
    import torch
    name, t, s, cam = ready
    batch = primary_batch(t, cam)
    d = rays_to_device(batch)
    d_sets = rays_to_device(np.repeat(batch, 4))
    npix = E.W * E.H
    for queue in (1, 0):
        t.setOption(T.OPT_SAMPLE_QUEUE, queue)
        for n in (1, 8, 64):
            tag = (name, policy, queue, n)
            t.clear()
            t.renderSamples(cam, 0, n)
            want = read_accum(t)
            assert (want[:, 3] == n).all() and np.nan_to_num(want[:, :3]).any(), tag
            out = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            t.renderRays(d, 0, n, out=out)
            t.sync()
            assert_same_floats(out.cpu().numpy(), want, tag + ("renderRays",))
            out.zero_()
            torch.cuda.synchronize()
            t.renderRaySets(d_sets, 4, 0, n, out=out)
            t.sync()
            assert_same_floats(out.cpu().numpy(), want, tag + ("renderRaySets",))
            t.clear()
            t.renderSamplesCameras(np.tile(cam, (n, 1)), 0)
            assert_same_floats(read_accum(t), want, tag + ("renderSamplesCameras",))
            assert t.walkOverflow() == 0, tag


# ---- f. the per-sample feature reduction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_four_identical_cameras_reduce_to_the_chain_record(ready, policy):
    name, t, s, cam = ready
    for follow, max_chain in ((0, 0), (FOLLOW_ALL, 3)):
        t.renderFeaturesChain(cam, follow, max_chain)
        one = t.featureRecords().reshape(-1).copy()
        t.renderFeaturesCameras(np.tile(cam, (4, 1)), follow, max_chain)
        got, cov = t.featureRecords().reshape(-1), t.featureCoverage().reshape(-1, 2)
        assert_same_records(got, one, "discrete fields, chain %d" % max_chain, ("object", "material", "face", "u", "v", "tex", "dir", "flags"))
        assert not (got["flags"] & A.FEATURE_MIXED).any()
        assert (cov[:, 1] * 4 == 4).all()
        hit = (one["flags"] & A.FEATURE_HIT) != 0
        assert np.array_equal(cov[:, 0] * 4, np.where(hit, 4.0, 0.0).astype(F32))
        assert t.walkOverflow() == 0
