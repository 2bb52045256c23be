"""GPU (-m gpu): the fused launcher runs the plan that plan_samples makes (csrc/pt_kernels.hip; its table is pinned on the
CPU, tests/test_sample_plan_host.py).  After fused calls on tiny frames of every kind of scene, rt_debug_last_sample_plan's
facts are what the scene's arrays and the options say, its plan is rt_debug_plan_samples of those facts, and
rt_sample_grid_stats' workgroup count grew by the plan's grid — under counters off / on, moments off / on, both wave-fill
modes, 8 and 64 samples per call, a call that traces the prefix and one that reuses it; then a hit whose live counts have
become known (the exact grid) and a look-ahead batch."""
import pytest

import cases
import sample_plan_ref as R

pytestmark = pytest.mark.gpu
rt = cases.rt
plan_samples = rt.raytracer.plan_samples

W, H = 32, 16    # 8 tiles of 8 x 8: 512 slots, two workgroups of pt_prefix
SCENES = {"c2": {}, "c3": dict(tex_size=8), "c4": dict(n_spheres=2000), "c5": dict(segments=16, rings=10), "all_kinds": {}}
_WORKLOADS = {}


def _workload(name):
    if name not in _WORKLOADS:
        wl = rt.workloads.get(name, width=W, height=H, **SCENES[name])
        _WORKLOADS[name] = (wl.scene, wl.camera)
    return _WORKLOADS[name]


def _tracer(name, fill=1):
    scene, cam = _workload(name)
    t = rt.RayTracer(W, H, scene=scene, seed=cases.SEED)
    t.setOption(t.OPT_WAVE_FILL, fill)       # (explicit: the facts below name it)
    t.setOption(t.OPT_PREFIX_CACHE, 1)       # (explicit: the environment must not matter here)
    t.setOption(t.OPT_EXACT_GRID, 1)
    return t, scene, cam


def _check_last(t, want_facts, before):
    """The last launch's facts are `want_facts`, its plan is theirs, and the grid statistics grew by that plan's launch."""
    facts, plan = t.lastSamplePlan()
    assert facts == want_facts
    assert plan == plan_samples(**facts) == R.plan(facts), facts
    after = t.sampleGridStats()
    assert (after[0] - before[0], after[2] - before[2]) == (1, plan["grid_units"]), plan
    assert t.liveList()[:2] == (facts["seg_cap"], plan["pixels_per_wave"])
    return plan


@pytest.mark.parametrize("moments", [0, 1])
@pytest.mark.parametrize("counters", [0, 1])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_launch_runs_the_plan_of_its_facts(name, counters, moments):
    t, scene, cam = _tracer(name)
    try:
        with pytest.raises(rt.RtError):
            t.lastSamplePlan()               # no fused launch yet
        cu = t.deviceInfo()["cu_count"]
        t.enableCounters(bool(counters))
        t.setOption(t.OPT_MOMENTS, moments)
        families = set()
        for spp in (8, 64):
            for fill in (1, 0):
                t.setOption(t.OPT_WAVE_FILL, fill)
                want = R.facts_of(scene, W * H, spp, cu_count=cu, count_enabled=counters, moments=moments, wave_fill=fill)
                before = t.sampleGridStats()
                t.clear()
                t.renderSamples(cam, 0, spp)       # traces the prefix
                plan = _check_last(t, want, before)
                before = t.sampleGridStats()
                t.renderSamples(cam, spp, spp)     # reuses it (not under counters); its counts are not known yet
                assert _check_last(t, want, before) == plan
                assert t.prefixCacheStats()[0] > 0 or counters
                families.add(plan["family"])
                assert plan["moments"] == moments and plan["count"] == counters and plan["grid_units"] > 0
        assert families == ({R.WALK} if name == "c5" and not counters else {R.QUEUE})
        t.sync()
    finally:
        t.close()


def test_a_hit_whose_counts_are_known_plans_the_exact_grid():
    t, scene, cam = _tracer("c2", fill=0)
    try:
        cu = t.deviceInfo()["cu_count"]
        t.clear()
        t.renderSamples(cam, 0, 64)              # miss
        t.renderSamples(cam, 64, 64)             # hit: the copy of the counters is under way
        t.sync()
        assert t.lastSamplePlan()[0]["exact"] == 0
        before = t.sampleGridStats()
        t.renderSamples(cam, 128, 64)            # hit: the counts are known
        cap, per, light, heavy = t.liveList()
        assert 0 < light + heavy <= W * H
        want = R.facts_of(scene, W * H, 64, cu_count=cu, wave_fill=0, exact=1, count_light=light, count_heavy=heavy)
        plan = _check_last(t, want, before)
        after = t.sampleGridStats()
        assert plan["grid_units"] == rt.sample_units(cap, per, light, heavy) == after[3] and after[1] - before[1] == 1
        assert plan["grid_units"] <= -(-cap // per) + 1 and plan["count_log2"] == 6
    finally:
        t.close()


def test_a_lookahead_batch_runs_the_plan_of_its_facts():
    t, scene, cam = _tracer("all_kinds")
    try:
        cu = t.deviceInfo()["cu_count"]
        t.setOption(t.OPT_LOOKAHEAD, 5)
        t.render(cam)                            # the direct kernel: no plan
        with pytest.raises(rt.RtError):
            t.lastSamplePlan()
        before = t.sampleGridStats()
        t.renderAgain(cam)                       # one fused launch for the next 5 samples
        assert t.lookaheadStats()[0] == 1
        plan = _check_last(t, R.facts_of(scene, W * H, 5, cu_count=cu), before)
        assert (plan["family"], plan["geom"], plan["count_log2"]) == (R.QUEUE, 1, R.GENERIC)
    finally:
        t.close()
