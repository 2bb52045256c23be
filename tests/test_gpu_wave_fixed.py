"""GPU (-m gpu): the fixed cost a wave of the sample queue pays around its sample loop (csrc/pt_queue.hpp: the instantiation
for exactly 64 samples per pixel, the scene's LDS tables copied from the context's staged block, the texel set-up kept in
its branch, queue_stage's coordinates without the division) changes no bit.

Frames of the fused path against the direct path pt_render with == as uint32, as tests/test_gpu_queue_sums.py compares them:
C2, C3, the all-kinds scene and a C2 with one sphere textured (one texture layer: the GEOM 0 kernel fetches the texel);
61 x 37 and 7 x 5 (a wave with fewer than four pixels, with one, a partial last wave); counts 1, 63, 64, 65, 128 (64 takes
the specialised kernel — asserted through rt_debug_wave_fixed — its neighbours do not); first sample 0 and 7; policies
`ieee` and `rocm-opencl`; moments off and on; wave fill off and on; two calls of 64 on one accumulator; rank 1 of 3 of a
sharded context; and a staged block that must not go stale: another scene, another policy and back, more materials than
the LDS table holds, the prefix-cache hit path — each against a fresh context.  Under `ieee` the block itself is compared
with its numpy restatement (tests/wave_fixed_ref.py)."""
import numpy as np
import pytest

import cases
import wave_fixed_ref as W

pytestmark = pytest.mark.gpu
rt = cases.rt
A = rt._abi

COUNTS = (1, 63, 64, 65, 128)
SIZES = {"ragged": (61, 37), "tiny": (7, 5)}
_SCENES = {}


def _textured_c2(w, h, textured=True):
    """C2 with the red diffuse sphere (material 3) t_textured and a one-layer texture: a sphere hit has u = v = 0 and layer 0."""
    wl = rt.workloads.get("c2", width=w, height=h)
    if textured:
        wl.scene.materials["type"][3] = A.T_TEXTURED
    wl.scene.setTextures(rt.workloads.checker_texture(8, 2))
    return wl


def _workload(case, size):
    if (case, size) not in _SCENES:
        w, h = SIZES[size]
        if case == "c2_textured":
            wl = _textured_c2(w, h)
        else:
            wl = rt.workloads.get(case, width=w, height=h, **({"tex_size": 64} if case == "c3" else {}))
        _SCENES[case, size] = (wl.scene, wl.camera, w, h)
    return _SCENES[case, size]


def _frame(t, cam, first, count, fused, calls=1):
    t.setOption(t.OPT_PREFIX_SHARING, 1 if fused else 0)
    t.setOption(t.OPT_SAMPLE_QUEUE, 1 if fused else 0)
    t.clear()
    for k in range(calls):
        t.renderSamples(cam, first + k * count, count)
    t.sync()
    return t.readLinear().copy()


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _compare(t, cam, key, counts=COUNTS, firsts=(0, 7), fills=(0, 1), moments=(0, 1), specialised=None):
    """specialised: True = a launch of 64 without moments must take the count-specialised kernel (a scene without a BVH),
    None = it may; no other launch ever does."""
    for mom in moments:
        t.setOption(t.OPT_MOMENTS, mom)
        for first in (firsts if not mom else firsts[:1]):
            for count in counts:
                direct = _frame(t, cam, first, count, False)
                direct_n = t.sampleCounts() if mom else None
                for fill in fills:
                    t.setOption(t.OPT_WAVE_FILL, fill)
                    before = t.waveFixedStats()[0]
                    fused = _frame(t, cam, first, count, True)
                    took = t.waveFixedStats()[0] - before
                    what = key + (mom, first, count, fill)
                    assert _same(fused, direct), what
                    if mom:
                        assert np.array_equal(t.sampleCounts(), direct_n), what
                        assert np.isfinite(t.moments()).all() and (t.moments() >= 0).all(), what
                    if count == 64 and not mom:
                        assert took == 1 if specialised else took in (0, 1), what
                    else:
                        assert took == 0, what
    t.setOption(t.OPT_MOMENTS, 0)


@pytest.mark.parametrize("arith", ["ieee", "rocm-opencl"])
@pytest.mark.parametrize("size", ["ragged", "tiny"])
@pytest.mark.parametrize("case", ["c2", "c3", "all_kinds", "c2_textured"])
def test_fused_frames_equal_the_direct_path(case, size, arith):
    scene, cam, w, h = _workload(case, size)
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    try:
        _compare(t, cam, (case, size, arith), specialised=True)   # (none of the four scenes has a BVH at these sizes)
    finally:
        t.close()


def test_a_64_sample_launch_on_c2_runs_the_specialised_kernel():
    scene, cam, w, h = _workload("c2", "ragged")
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith("rocm-opencl")
    try:
        assert t.waveFixedStats()[0] == 0
        for n, count in enumerate((64, 64, 64)):
            t.renderSamples(cam, 64 * n, count)
            assert t.waveFixedStats()[0] == n + 1
        for count in (63, 65, 32, 128, 1):
            t.renderSamples(cam, 200, count)
            assert t.waveFixedStats()[0] == 3, count
        t.enableCounters(True)   # a counting build keeps the generic kernel
        t.renderSamples(cam, 300, 64)
        assert t.waveFixedStats()[0] == 3
        t.enableCounters(False)
        t.setOption(t.OPT_MOMENTS, 1)   # and so do moments
        t.clear()
        t.renderSamples(cam, 0, 64)
        assert t.waveFixedStats()[0] == 3
        t.sync()
    finally:
        t.close()


@pytest.mark.parametrize("arith", ["ieee", "rocm-opencl"])
def test_the_textured_sphere_fetches_its_texel(arith):
    """The lazy texel is really fetched under GEOM 0: the frame differs from the same scene with that sphere diffuse."""
    w, h = SIZES["ragged"]
    frames = []
    for textured in (True, False):
        wl = _textured_c2(w, h, textured)
        t = rt.RayTracer(w, h, scene=wl.scene, seed=cases.SEED)
        t.setArith(arith)
        try:
            frames.append(_frame(t, wl.camera, 0, 64, True))
            assert t.waveFixedStats()[0] == 1
            assert _same(frames[-1], _frame(t, wl.camera, 0, 64, False))
        finally:
            t.close()
    assert (frames[0].view(np.uint32) != frames[1].view(np.uint32)).any()


@pytest.mark.parametrize("arith", ["ieee", "rocm-opencl"])
def test_two_calls_of_64_on_one_accumulator(arith):
    scene, cam, w, h = _workload("c2", "ragged")
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    try:
        before = t.waveFixedStats()[0]
        hits = t.prefixCacheStats()[0]
        fused = _frame(t, cam, 0, 64, True, calls=2)
        assert t.waveFixedStats()[0] == before + 2
        assert t.prefixCacheStats()[0] == hits + 1   # (the second call reuses the kept prefix)
        assert _same(fused, _frame(t, cam, 0, 64, False, calls=2))   # (not one call of 128: that is another summation order)
    finally:
        t.close()


@pytest.mark.parametrize("arith", ["ieee", "rocm-opencl"])
def test_sharded_context_rank_1_of_3(arith):
    """world == 3: queue_stage keeps slot_to_pixel."""
    scene, cam, w, h = _workload("c2", "ragged")
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    t.setShard(1, 3)
    try:
        _compare(t, cam, ("c2", "rank 1 of 3", arith), counts=(63, 64, 65), moments=(0,), specialised=True)
    finally:
        t.close()


# ---- the staged block never goes stale ---------------------------------------------------------------------------------
def _scene_b(w, h):
    """C2 with other extra_data (glass and mirror constants) and other colours."""
    wl = rt.workloads.get("c2", width=w, height=h)
    m = wl.scene.materials
    m["extra_data"][m["type"] == A.T_DIELECTRIC] += np.float32(0.27)
    m["extra_data"][m["type"] == A.T_REFLECTIVE] *= np.float32(0.5)
    m["color"][:, :3] = (m["color"][:, :3] * np.float32(0.6) + np.float32(0.2)).astype(np.float32)
    return wl


def _fresh(scene, cam, w, h, arith, count=64):
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    try:
        return _frame(t, cam, 0, count, True)
    finally:
        t.close()


@pytest.mark.parametrize("arith", ["ieee", "rocm-opencl"])
def test_another_scene_rebuilds_the_block(arith):
    scene_a, cam, w, h = _workload("c2", "ragged")
    wl_b = _scene_b(w, h)
    t = rt.RayTracer(w, h, scene=scene_a, seed=cases.SEED)
    t.setArith(arith)
    try:
        a = _frame(t, cam, 0, 64, True)
        builds = t.waveFixedStats()[1]
        assert builds >= 1
        if arith == "ieee":
            assert W.same_block(t.stageBlock(), W.stage_block(scene_a))
        t.setScene(wl_b.scene)
        with pytest.raises(rt.raytracer.RtError):
            t.stageBlock()   # (not built for this scene yet)
        b = _frame(t, cam, 0, 64, True)
        assert t.waveFixedStats()[1] > builds
        if arith == "ieee":
            assert W.same_block(t.stageBlock(), W.stage_block(wl_b.scene))
        assert _same(b, _frame(t, cam, 0, 64, False))
        assert _same(b, _fresh(wl_b.scene, cam, w, h, arith))
        assert not _same(a, b)
        t.setScene(scene_a)
        assert _same(_frame(t, cam, 0, 64, True), a)
    finally:
        t.close()


def test_another_policy_rebuilds_the_block():
    """ieee -> rocm-opencl -> ieee: the block holds the policy's divisions."""
    scene, cam, w, h = _workload("c2", "ragged")
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    try:
        blocks = []
        for arith in ("ieee", "rocm-opencl", "ieee"):
            t.setArith(arith)
            builds = t.waveFixedStats()[1]
            got = _frame(t, cam, 0, 64, True)
            assert t.waveFixedStats()[1] > builds, arith
            blocks.append(t.stageBlock())
            assert _same(got, _frame(t, cam, 0, 64, False)), arith
            assert _same(got, _fresh(scene, cam, w, h, arith)), arith
        assert W.same_block(blocks[0], W.stage_block(scene)) and W.same_block(blocks[2], W.stage_block(scene))
        assert blocks[1].shape == blocks[0].shape
    finally:
        t.close()


@pytest.mark.parametrize("arith", ["ieee", "rocm-opencl"])
def test_more_materials_than_the_table_holds(arith):
    w, h = SIZES["ragged"]
    wl = rt.workloads.get("c2", width=w, height=h)
    for k in range(A.LDS_MATERIALS):
        wl.scene.addMaterial(A.T_DIFFUSE, (0.1 + 0.01 * k, 0.5, 0.9), 1.0)
    t = rt.RayTracer(w, h, scene=wl.scene, seed=cases.SEED)
    t.setArith(arith)
    try:
        _compare(t, wl.camera, ("c2", "no material table", arith), counts=(63, 64), firsts=(0,), moments=(0,), specialised=True)
        _frame(t, wl.camera, 0, 64, True)   # (the options _compare set last ask for a rebuild: the next fused launch's)
        block = t.stageBlock()   # sphere and plane records only
        assert block.shape == (2 * len(wl.scene.spheres) + len(wl.scene.planes), 4)
        assert W.same_block(block, W.stage_block(wl.scene))
    finally:
        t.close()


@pytest.mark.parametrize("arith", ["ieee", "rocm-opencl"])
def test_the_prefix_cache_hit_path_builds_nothing_and_changes_nothing(arith):
    scene, cam, w, h = _workload("c2", "ragged")
    t = rt.RayTracer(w, h, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    try:
        first = _frame(t, cam, 0, 64, True)
        hits, builds = t.prefixCacheStats()[0], t.waveFixedStats()[1]
        t.clear()
        t.renderSamples(cam, 0, 64)   # a second identical call: the kept prefix, the kept block
        t.sync()
        assert t.prefixCacheStats()[0] == hits + 1 and t.waveFixedStats()[1] == builds
        again = t.readLinear()
        assert _same(again, first)
        assert _same(again, _fresh(scene, cam, w, h, arith))
    finally:
        t.close()
