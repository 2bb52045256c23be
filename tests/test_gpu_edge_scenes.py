"""GPU (-m gpu): the degenerate scenes of tests/edge_scenes.py (VERDICT.md "What's weak" #2) through the trace kernels.

Policy 0: every pixel of samples 0-3 bit for bit against the CPU oracle (which tests/test_edge_scenes_host.py pins to the
compiled reference), the fused 8-sample frame with the acceleration structures on against off, bit for bit, the counters
of both equal to the oracle's, and no walk on its loop bound.  Policies 1 and 2, where oracle/_ref/gfx950 is present:
samples 0-3 bit for bit against the reference's kernel file as ROCm's OpenCL tool chain builds it (NaN matches NaN) —
the 2.5-ulp division and the library's normalize need not agree with IEEE on 0 / 0, x / 0 and normalize(0), and these
scenes are where the paths meet them."""
import os
import sys

import numpy as np
import pytest

import cases
import edge_scenes as E
from test_edge_scenes_host import SAMPLES, all_pixels, oracle_samples

sys.path.insert(0, os.path.join(cases.ROOT, "oracle"))
import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
rt = cases.rt
HSACO = {1: orc.REF950_HSACO_NOCONTRACT, 2: orc.REF950_HSACO}
needs_ref950 = pytest.mark.skipif(
    not (orc.ReferenceGfx950.available() and orc.ReferenceGfx950.available(orc.REF950_HSACO_NOCONTRACT)),
    reason="oracle/_ref/gfx950 (gfx950 builds of the reference) not present")
FUSED = 8


@pytest.fixture(scope="module", params=sorted(E.SCENES))
def tracer(request):
    s, cam = E.get(request.param)
    t = rt.RayTracer(E.W, E.H, scene=s, seed=cases.SEED)
    t.resetCounters()
    yield request.param, t, s, cam
    t.setArith(rt.ARITH_IEEE)
    t.close()     # (asserts that no walk ended on its loop bound: tests/conftest.py)


def test_policy_0_is_the_oracle_bit_for_bit(tracer, oracle):
    name, t, s, cam = tracer
    t.setArith(rt.ARITH_IEEE)
    table = t.getRandomTable()
    exp, _ = oracle_samples(oracle, name, table)
    for k in range(SAMPLES):
        got = t.traceSamples(cam, *all_pixels(k))
        same = (got.view(np.uint32) == exp[k].view(np.uint32)).all(axis=1)
        assert same.all(), (name, k, int((~same).sum()))
    _, ocn = oracle.render(s, cam, table, E.W, E.H, 2, count=FUSED, threads=4)
    od = ocn.as_dict()
    od["image_reads"] = 0      # the fused path never re-reads the image
    frames = []
    for accel in (1, 0):
        t.setOption(t.OPT_ACCEL, accel)
        t.enableCounters(True)
        t.resetCounters()
        t.clear()
        t.renderSamples(cam, 0, FUSED)
        t.sync()
        frames.append(t.readLinear().copy())
        assert t.counters().as_dict() == od, (name, accel)
        t.enableCounters(False)
        t.clear()
        t.renderSamples(cam, 0, FUSED)     # and the kernels that do not count
        t.sync()
        assert np.array_equal(t.readLinear().view(np.uint32), frames[-1].view(np.uint32)), (name, accel)
        assert t.walkOverflow() == 0, (name, accel)
    t.setOption(t.OPT_ACCEL, 1)
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32)), name
    # the fused mean is the mean of the oracle's samples (float64 sum of the first four against the frame of four)
    t.clear()
    t.renderSamples(cam, 0, SAMPLES)
    t.sync()
    lin = t.readLinear()[..., :3].reshape(-1, 3).astype(np.float64)
    mean = exp.astype(np.float64).mean(axis=0)
    assert np.abs(lin - mean).max() <= 1e-5 * max(1.0, np.abs(mean).max()), name


@needs_ref950
@pytest.mark.parametrize("policy", [1, 2])
def test_policies_1_and_2_are_the_rocm_opencl_build_bit_for_bit(tracer, policy):
    name, t, s, cam = tracer
    ref = orc.ReferenceGfx950(HSACO[policy])
    t.setArith(policy)
    t.setOption(t.OPT_PREFIX_TREE, 2)
    table = t.getRandomTable()
    try:
        for k in range(SAMPLES):
            _, last = ref.render(s, cam, table, E.W, E.H, k, 1, want_last=True)
            theirs = np.ascontiguousarray(last[..., :3]).reshape(-1, 3)
            t.clear()
            t.renderSamples(cam, k, 1)      # through pt_prefix + the sample kernels
            t.sync()
            mine = np.ascontiguousarray(t.readLinear()[..., :3]).reshape(-1, 3)
            probe = t.traceSamples(cam, *all_pixels(k))     # and through the probe kernel
            for what, a in (("fused", mine), ("probe", probe)):
                same = ((a.view(np.uint32) == theirs.view(np.uint32)) | (np.isnan(a) & np.isnan(theirs))).all(axis=1)
                assert same.all(), (name, policy, k, what, int((~same).sum()), np.nonzero(~same)[0][:8].tolist())
        assert t.walkOverflow() == 0
    finally:
        t.setOption(t.OPT_PREFIX_TREE, 1)
