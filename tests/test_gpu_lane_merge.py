"""The sample queue's loop updates its per-lane state in place (pt_samples_q: no separate "continue" path, refills
and hits write the loop-carried registers directly): frames must stay bit-identical to the direct path pt_render,
which traces every sample from the camera, under the IEEE and the rocm-opencl policies, at sample counts below,
at, and above a wave's queue, on the headline scenes, the all-kinds scene and random scenes."""
import numpy as np
import pytest

import cases
from test_gpu_fuzz import random_scene

pytestmark = pytest.mark.gpu
rt = cases.rt

SPPS = ((1, 0), (5, 3), (64, 0), (200, 7))


def _scene(case):
    if case.startswith("random"):
        s, cam = random_scene(int(case[len("random"):]))
        return s, cam, 160, 90
    wl = rt.workloads.get(case, width=320, height=180)
    return wl.scene, wl.camera, wl.width, wl.height


@pytest.mark.parametrize("arith", ["ieee", "rocm-opencl"])
@pytest.mark.parametrize("case", ["c2", "c3", "all_kinds", "random103", "random111", "random118"])
def test_sample_queue_frames_equal_direct_path(case, arith):
    scene, cam, W, H = _scene(case)
    t = rt.RayTracer(W, H, scene=scene, seed=cases.SEED)
    t.setArith(arith)
    t.resetCounters()
    for spp, first in SPPS:
        frames = []
        for share, queue in ((1, 1), (0, 0)):   # fused path with the sample queue; direct path pt_render
            t.setOption(t.OPT_PREFIX_SHARING, share)
            t.setOption(t.OPT_SAMPLE_QUEUE, queue)
            t.clear()
            t.renderSamples(cam, first, spp)
            t.sync()
            frames.append(t.readLinear().copy())
        assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32)), (case, arith, spp)
    assert t.walkOverflow() == 0
    t.close()
