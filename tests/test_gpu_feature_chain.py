"""GPU (-m gpu): feature records that follow mirror and glass chains to the first rough hit (rt_render_features_chain:
pt_features_chain) and RT_DENOISE_SPLIT_CHAINS.  The records must be, bit for bit, what iterating rt_debug_hit(kind 3)
and rt_debug_material on the host gives (tests/chain_ref.py) under every arithmetic policy — under policy IEEE also what
the CPU oracle gives — on frames whose chains are long, cut, leave the scene and end on the light; the three filters must
follow the header's statement with the pair key; and the call may touch nothing but the feature records."""
import ctypes as C

import numpy as np
import pytest

import cases
import chain_ref as CH
import denoise_ref as R
import denoise_vg_ref as V
import moments_ref as M

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi
POLICIES = (rt.ARITH_IEEE, rt.ARITH_ROCM_OCL_NOCONTRACT, rt.ARITH_ROCM_OCL)
EINVAL, ESTATE = -1, -4

SCENES = {
    "c2": lambda: rt.workloads.get("c2", width=64, height=36),
    "all_kinds": lambda: rt.workloads.get("all_kinds", width=60, height=40),     # lens, textured terminals
    "c5": lambda: rt.workloads.get("c5", width=48, height=27),                   # mesh BVH, a dielectric mesh
}
# (scene, follow mask, max_chain)
REPLAYS = [("c2", 3, 29), ("c2", 7, 29), ("c2", 7, 2), ("all_kinds", 7, 29), ("c5", 4, 29)]


def cam_block(wl):
    return rt.raytracer._cam_block(wl.camera)


def read_accum(t):
    import torch
    t.sync()
    return torch.as_tensor(t.deviceAccum(), device="cuda").cpu().numpy().copy()


@pytest.fixture(scope="module")
def tracers():
    made = {}

    def get(name):
        if name not in made:
            wl = SCENES[name]()
            made[name] = (wl, rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED))
        return made[name]

    yield get
    for _, t in made.values():
        t.setArith(rt.ARITH_IEEE)
        t.close()


# ---- 1. the identity case -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", ["c2", "all_kinds"])
def test_nothing_followed_is_render_features_bit_for_bit(tracers, name, policy):
    wl, t = tracers(name)
    t.setArith(policy)
    t.renderFeatures(wl.camera)
    first = t.featureRecords()
    assert ((first["flags"] & A.FEATURE_HIT) != 0).any()
    for follow, max_chain in ((0, 29), (7, 0), (0, 0)):
        t.renderFeatures(rt.Camera(60, 1.5, (-7, -1, -9), 30.0, 5.0))     # something else in the buffer first
        t.renderFeaturesChain(wl.camera, follow, max_chain)
        assert t.featureRecords().tobytes() == first.tobytes(), (follow, max_chain)


# ---- 2. + 3. the replay, and what the frames must cover ----------------------------------------------------------------

FIELDS = ("dir", "flags", "t", "pos", "normal", "object", "material", "face", "u", "v", "tex", "albedo")


def assert_records_equal(got, exp, what):
    for f in FIELDS:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(exp[f])
        same = a.view(np.uint32) == b.view(np.uint32)
        assert same.all(), "%s: field %s differs in %d records, first %d: %r != %r" % (
            what, f, (~same.reshape(len(got), -1).all(1)).sum(), np.nonzero(~same.reshape(len(got), -1).all(1))[0][0],
            a[~same.reshape(len(got), -1).all(1)][0], b[~same.reshape(len(got), -1).all(1)][0])
    assert got.tobytes() == exp.tobytes(), what


def coverage(wl, rec):
    f = A.split_features(rec)
    n = f["chain_length"]
    types = wl.scene.materials["type"]
    return dict(chain1=int((n >= 1).sum()), chain2=int((n >= 2).sum()), sky=int((~f["hit"] & (n >= 1)).sum()),
                light=int((f["hit"] & (n >= 1) & (types[np.where(f["hit"], f["material"], 0)] == A.T_LIGHT)).sum()),
                cut=int(f["cut"].sum()), longest=int(n.max()))


# what each replay case must cover, so that none passes on empty chains (CPU oracle: 253, 151, 65, 8; 97; 110)
REQUIRED = {
    ("c2", 7, 29): dict(chain1=100, chain2=50, sky=20, light=1),
    ("c2", 7, 2): dict(cut=30),
    ("c5", 4, 29): dict(chain1=50),
}

_oracle_cache = {}


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("case", REPLAYS, ids=lambda c: "%s-mask%d-max%d" % c)
def test_records_equal_the_host_replay_bit_for_bit(tracers, case, policy, oracle, table):
    name, follow, max_chain = case
    wl, t = tracers(name)
    t.setArith(policy)
    cam = cam_block(wl)
    t.renderFeaturesChain(wl.camera, follow, max_chain)
    rec = t.featureRecords().reshape(-1)
    exp, chain = CH.replay(CH.DeviceProbes(t), wl.scene, cam[:3], rec["dir"], follow, max_chain)
    cov = coverage(wl, rec)
    print("%s mask %d max_chain %d policy %d: %s" % (name, follow, max_chain, policy, cov))
    assert_records_equal(rec, exp, "device probes")
    # the flags against the chain's own objects, through the library's signature
    for r, c in zip(rec, chain):
        fl = int(r["flags"])
        assert (fl >> 8) & 31 == len(c) <= max_chain
        assert fl & 0xFFFF0000 == rt.feature_chain_signature(c) & 0xFFFF0000
        assert not (fl & A.FEATURE_CUT) or (len(c) == max_chain and fl & A.FEATURE_HIT)
        assert (fl & A.FEATURE_HIT != 0) == bool(r["t"] < np.inf)
    for key, least in REQUIRED.get(case, {}).items():
        assert cov[key] >= least, (key, cov[key], least)
    if case == ("c2", 7, 2):
        assert cov["longest"] == 2
    if name == "all_kinds":
        f = A.split_features(rec)
        types = wl.scene.materials["type"]
        tex = f["hit"] & (types[np.where(f["hit"], f["material"], 0)] == A.T_TEXTURED)
        assert tex.any() and (f["face"][tex] != A.NO_ID).all() and (f["chain_length"] >= 1).any()
    if policy == rt.ARITH_IEEE:
        if case not in _oracle_cache:
            dirs = rec["dir"].copy()
            _oracle_cache[case] = CH.replay(CH.OracleProbes(oracle, wl.scene, table), wl.scene, cam[:3], dirs, follow, max_chain)[0]
        assert_records_equal(rec, _oracle_cache[case], "CPU oracle")
    assert t.walkOverflow() == 0


# ---- 4. the denoisers -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=POLICIES, ids=lambda p: "policy%d" % p)
def frame(request):
    """C2 96x54, 4 spp with sample moments, rendered under each arithmetic policy in turn: the accumulator, the moments
    and every feature record the filters of this section read come from that policy's kernel set."""
    wl = rt.workloads.get("c2", width=96, height=54)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    t.setArith(request.param)
    t.setOption(t.OPT_MOMENTS, 1)
    t.renderFrame(wl.camera, 4)
    acc, m2 = read_accum(t), t.moments()
    yield wl, t, acc, m2
    t.close()


def run_filter(t, which, **kw):
    if which == "atrous":
        return t.denoise(**dict(A.DENOISE_DEFAULTS, **kw)), None, None
    got = (t.denoiseVariance if which == "variance" else t.denoiseMoments)(**dict(A.DENOISE_VARIANCE_DEFAULTS, **kw))
    return got, t.variance(0), t.variance(1)


def restate(which, acc, m2, feats, split_objects, split_chains):
    g = CH.with_pair_key(feats, split_objects, split_chains)
    if which == "atrous":
        return R.atrous(acc, g, **dict(A.DENOISE_DEFAULTS, split_objects=True))[..., :3] ** 2, None, None
    kw = dict(A.DENOISE_VARIANCE_DEFAULTS, split_objects=True)
    if which == "variance":
        out, v0, vl = V.filter_frame(acc, g, **kw)
        return out[..., :3] ** 2, v0, vl
    _, lin, v0, vl = M.filter_moments(acc, m2, g, **kw)
    return lin, v0, vl


@pytest.mark.parametrize("split_objects", [True, False])
@pytest.mark.parametrize("which", ["atrous", "variance", "moments"])
def test_filters_match_the_restatement_on_chain_records(frame, which, split_objects):
    """Tolerances: those of tests/test_gpu_denoise.py, test_gpu_denoise_vg.py and test_gpu_moments.py for the same filters
    (2e-5 on the linear colour, 2e-5 relative to max(1, v) on both variance buffers)."""
    wl, t, acc, m2 = frame
    t.renderFeaturesChain(wl.camera, rt.FOLLOW_ALL)
    feats = t.features()
    assert (feats["chain_length"] >= 2).sum() >= 100
    outs = {}
    for split_chains in (False, True):
        got, v0, vl = run_filter(t, which, split_objects=split_objects, split_chains=split_chains)
        lin, v0_ref, vl_ref = restate(which, acc, m2, feats, split_objects, split_chains)
        assert (got[..., 3] == 1).all()
        e_c = np.abs(got[..., :3].astype(np.float64) ** 2 - lin).max()
        print("%s split_objects %d split_chains %d: linear colour %.3g (bound 2e-5)" % (which, split_objects, split_chains, e_c))
        assert e_c <= 2e-5
        if v0 is not None:
            e_v0 = (np.abs(v0 - v0_ref) / np.maximum(1.0, v0_ref)).max()
            e_vl = (np.abs(vl - vl_ref) / np.maximum(1.0, vl_ref)).max()
            print("    v0 %.3g, v(L) %.3g (bound 2e-5 each)" % (e_v0, e_vl))
            assert e_v0 <= 2e-5 and e_vl <= 2e-5
        outs[split_chains] = got
    assert outs[False].tobytes() != outs[True].tobytes()      # the flag does something on chain records


@pytest.mark.parametrize("which", ["atrous", "variance", "moments"])
def test_split_chains_changes_nothing_on_first_hit_records(frame, which):
    wl, t, acc, m2 = frame
    t.renderFeatures(wl.camera)
    assert (t.featureRecords()["flags"] >> 8 == 0).all()
    for split_objects in (True, False):
        off = run_filter(t, which, split_objects=split_objects, split_chains=False)
        on = run_filter(t, which, split_objects=split_objects, split_chains=True)
        for a, b in zip(off, on):
            assert (a is None and b is None) or a.tobytes() == b.tobytes()


def test_unknown_denoise_flags_are_still_errors(frame):
    wl, t, acc, m2 = frame
    lib, ctx = t._lib, t._ctx
    t.renderFeaturesChain(wl.camera, rt.FOLLOW_ALL)
    for flags in (2, 8, 3, 6, 7, 0x80000000, 0x100):
        assert lib.rt_denoise(ctx, C.byref(A.DenoiseParams(5, 0.5, 0.5, 0.5, 0.2, flags))) == EINVAL, flags
        for fn in (lib.rt_denoise_variance, lib.rt_denoise_moments):
            assert fn(ctx, C.byref(A.DenoiseVarianceParams(5, 4.0, 0.5, 0.5, 0.2, flags))) == EINVAL, flags
    for flags in (0, 1, 4, 5):
        assert lib.rt_denoise(ctx, C.byref(A.DenoiseParams(1, 0.5, 0.5, 0.5, 0.2, flags))) == 0, flags
        for fn in (lib.rt_denoise_variance, lib.rt_denoise_moments):
            assert fn(ctx, C.byref(A.DenoiseVarianceParams(1, 4.0, 0.5, 0.5, 0.2, flags))) == 0, flags
    t.sync()


# ---- 5. state and validation ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("policy", POLICIES)
def test_error_cases_and_state(policy):
    wl = rt.workloads.get("c2", width=64, height=36)
    lib = rt.load_library()
    P = A.FeatureChainParams
    cam = cam_block(wl)
    raw = C.c_void_p()
    assert lib.rt_create(0, 16, 8, C.byref(raw)) == 0
    try:
        assert lib.rt_render_features_chain(raw, cam.ctypes.data, C.byref(P(7, 29))) == ESTATE     # no scene yet
    finally:
        lib.rt_destroy(raw)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    ctx = t._ctx
    try:
        t.setArith(policy)
        feats = np.empty((wl.height, wl.width), A.FEATURE)
        for follow, max_chain in ((8, 29), (0x10, 1), (0x80000007, 4), (7, 30), (0, 30), (7, 0xFFFFFFFF)):
            assert lib.rt_render_features_chain(ctx, cam.ctypes.data, C.byref(P(follow, max_chain))) == EINVAL, (follow, max_chain)
        assert lib.rt_render_features_chain(ctx, cam.ctypes.data, None) == EINVAL
        assert lib.rt_render_features_chain(ctx, None, C.byref(P(7, 29))) == EINVAL
        assert lib.rt_render_features_chain(None, cam.ctypes.data, C.byref(P(7, 29))) == EINVAL
        # the failed calls made nothing
        assert lib.rt_read_features(ctx, feats.ctypes.data, feats.nbytes) == ESTATE
        t.setShard(0, 2)
        assert lib.rt_render_features_chain(ctx, cam.ctypes.data, C.byref(P(7, 29))) == EINVAL
        t.setShard(0, 1)
        for follow, max_chain in ((7, 29), (1, 1), (4, 0), (0, 0)):
            assert lib.rt_render_features_chain(ctx, cam.ctypes.data, C.byref(P(follow, max_chain))) == 0
        assert lib.rt_read_features(ctx, feats.ctypes.data, feats.nbytes) == 0
        d = C.c_void_p()
        assert lib.rt_device_features(ctx, C.byref(d)) == 0 and d.value
        # after rt_resize nothing is left; a chain call makes the records of the new frame
        t.resize(wl.width + 8, wl.height)
        feats = np.empty((wl.height, wl.width + 8), A.FEATURE)
        assert lib.rt_read_features(ctx, feats.ctypes.data, feats.nbytes) == ESTATE
        assert lib.rt_denoise(ctx, C.byref(A.DenoiseParams(5, 0.5, 0.5, 0.5, 0.2, 5))) == ESTATE
        t.renderFeaturesChain(wl.camera, rt.FOLLOW_ALL, 29)
        assert t.featureRecords().shape == (wl.height, wl.width + 8)
    finally:
        t.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_nothing_else_moves(policy):
    wl = rt.workloads.get("c2", width=64, height=36)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        t.setArith(policy)
        t.setOption(t.OPT_MOMENTS, 1)
        t.renderFrame(wl.camera, 4)
        t.render(wl.camera)
        t.renderAgain(wl.camera)
        before = t.transferImage(), read_accum(t), t.sample_counter, t.moments(), t.sampleCounts()
        t.renderFeaturesChain(wl.camera, rt.FOLLOW_ALL, 29)
        t.renderFeaturesChain(wl.camera, rt.FOLLOW_REFLECTIVE, 2)
        t.sync()
        after = t.transferImage(), read_accum(t), t.sample_counter, t.moments(), t.sampleCounts()
        assert before[2] == after[2] == 1
        for a, b in zip(before, after):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
        # and the next sample is the one the counter says
        t.renderAgain(wl.camera)
        assert t.sample_counter == 2
    finally:
        t.close()


# ---- 6. quality on the device ---------------------------------------------------------------------------------------------

def gamma_rmse(a, b, sel):
    return float(np.sqrt(((a[..., :3].astype(np.float64) - b[..., :3])[sel] ** 2).mean()))


@pytest.mark.parametrize("policy", POLICIES)
def test_chain_guides_with_split_beat_the_noisy_frame_on_the_chain_pixels(policy):
    """C2 256x144, 4 spp, rt_denoise_variance (defaults), truth 2048 spp: gamma RMSE of the noisy frame and of the filter
    guided by first-hit records, by chain records, and by chain records with RT_DENOISE_SPLIT_CHAINS, on the whole frame
    and on the pixels with a chain.  Asserted: chain-guided with split is below noisy on the chain pixels."""
    wl = rt.workloads.get("c2", width=256, height=144)
    t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=cases.SEED)
    try:
        t.setArith(policy)
        truth = t.renderFrame(wl.camera, 2048)
        noisy = t.renderFrame(wl.camera, 4)
        by_first = t.denoiseVariance(camera=wl.camera)
        t.renderFeaturesChain(wl.camera, rt.FOLLOW_ALL)
        sub = t.features()["chain_length"] >= 1
        by_chain = t.denoiseVariance()
        by_split = t.denoiseVariance(split_chains=True)
        assert sub.sum() >= 2000
        rows = {}
        print("\npolicy %d\n| pixels | noisy | first-hit guides | chain guides | chain guides, split |" % policy)
        print("|---|---:|---:|---:|---:|")
        for name, sel in (("whole frame", np.ones_like(sub)), ("chain >= 1 (%d)" % sub.sum(), sub)):
            rows[name] = [gamma_rmse(x, truth, sel) for x in (noisy, by_first, by_chain, by_split)]
            print("| %s | %.4f | %.4f | %.4f | %.4f |" % ((name,) + tuple(rows[name])))
        e = rows["chain >= 1 (%d)" % sub.sum()]
        assert e[3] < e[0]
    finally:
        t.close()


# ---- 7. rt_cli ------------------------------------------------------------------------------------------------------------

def test_cli_follow_matches_python_path(built, tmp_path):
    """rt_cli has no switch for the arithmetic policy: one run, under the default policy."""
    import os
    import subprocess
    w, h, spp = 96, 54, 4
    root = cases.ROOT
    assets = os.path.join(root, "assets")
    raw, aov = str(tmp_path / "f.f32"), str(tmp_path / "aov")
    subprocess.run([os.path.join(root, "host", "rt_cli"), "--scene", os.path.join(assets, "scenes", "c2_cornell.scene"),
                    "--size", "%dx%d" % (w, h), "--spp", str(spp), "--camera=-8,-1,-8,45,0", "--raw", raw, "--denoise",
                    "--variance-guided", "--follow", "mirror,glass,dielectric", "--max-chain", "3", "--split-chains",
                    "--aov", aov], check=True, cwd=root, timeout=120)
    got = np.fromfile(raw, np.float32).reshape(h, w, 4)
    s = rt.SceneCreator()
    s.loadScene(os.path.join(assets, "scenes", "c2_cornell.scene"), base_dir=assets)
    t = rt.RayTracer(w, h, scene=s)
    try:
        cam = rt.Camera(60, np.float32(w) / np.float32(h), (-8, -1, -8), 45.0, 0.0)
        t.renderFrame(cam, spp)
        t.renderFeaturesChain(cam, rt.FOLLOW_ALL, 3)
        exp = t.denoiseVariance(split_chains=True)
        f = t.features()
    finally:
        t.close()
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert f["cut"].any() and (f["chain_length"] == 3).any()
    chain = np.stack([f["chain_length"], f["chain_signature"] >> 16, f["cut"]], axis=-1).astype(np.float32)
    for name, arr, ch in (("normal", f["normal"], 3), ("depth", f["depth"], 1), ("chain", chain, 3)):
        pfm = open(aov + "_%s.pfm" % name, "rb").read()
        head = b"%s\n%d %d\n-1.0\n" % (b"PF" if ch == 3 else b"Pf", w, h)
        assert pfm.startswith(head)
        data = np.frombuffer(pfm[len(head):], np.float32)
        assert np.array_equal(data.view(np.uint32), np.ascontiguousarray(arr, np.float32).reshape(-1).view(np.uint32)), name
