"""GPU: a setScene call that fails validation leaves the context's scene as it was, and a scene that replaces one with
walk jobs renders as on a fresh context.  32 x 24 at 4 spp: the linear frame is the accumulator divided by 4, an exact
operation, so equal bits there are equal bits in the accumulator."""
import numpy as np
import pytest

import cases

rt = cases.rt
W, H, SPP = 32, 24, 4
RT_ERANGE = -5   # include/rt_amd.h


def accum(t, camera):
    t.clear()
    t.renderSamples(camera, 0, SPP)
    return t.readLinear().view(np.uint32)


@pytest.mark.gpu
def test_failed_and_successful_scene_replacement(built):
    mesh = rt.workloads.get("c5", segments=16, rings=10, width=W, height=H, spp=SPP)
    kinds = rt.workloads.get("all_kinds", width=W, height=H, spp=SPP)
    t = rt.RayTracer(W, H, scene=mesh.scene)
    first = accum(t, mesh.camera)
    assert t.lastSamplePlan()[0]["walk_jobs"] == 1            # the scene has walk jobs
    assert first[..., :3].any()

    bad = rt.SceneCreator()
    bad.addMaterial(rt._abi.T_DIFFUSE, (1, 1, 1), 1)
    bad.addSphere((0, 0, 5), 1, 3)
    with pytest.raises(rt.RtError) as e:
        t.setScene(bad)
    assert e.value.code == RT_ERANGE and "sphere 0: material 3 does not exist" in str(e.value)
    assert np.array_equal(accum(t, mesh.camera), first)       # the old scene still renders, bit for bit

    t.setScene(kinds.scene)
    replaced = accum(t, kinds.camera)
    t.close()
    fresh = rt.RayTracer(W, H, scene=kinds.scene)
    assert np.array_equal(replaced, accum(fresh, kinds.camera))
    fresh.close()
