"""CPU: the feature, occlusion and fixed-lane ray kernels (csrc/pt_kernels.hip: pt_features*, pt_occluded*, pt_render_rays,
pt_render_raysets) are shells around shared texts — feature_chain, PT_OCCLUDED_COUNTS, render_rays_fixed (DESIGN §5,
profiles/r31_experiments.md) — and every shell inlines its body afresh.  What a change to a body may cost each of them is read
from the compiler's output, as tests/test_sphere_scan_host.py does: the device code of the three arithmetic policies is
compiled as shipped (tools/isa_stats.py --json) and, per kernel, there is no scratch, no spilled VGPR, and the VGPR count
allows at least the waves per SIMD the kernel had before the bodies were shared (512 VGPRs per lane in granules of 8, at most
8 waves; the steps were equal under the three policies).  The number of kernels per policy is pinned too, so that a shell
that is no longer instantiated shows."""
import json
import os
import subprocess
import sys

import pytest

import cases

ISA = os.path.join(cases.ROOT, "tools", "isa_stats.py")
FAMILIES = ("pt_features", "pt_occluded", "pt_render_rays", "pt_render_raysets")
KERNELS_PER_POLICY = 104
# waves per SIMD by VGPR count before the kernels shared their bodies
WAVES = {
    "pt_features<false>": 8, "pt_features<true>": 7,
    "pt_features_chain<false>": 7, "pt_features_chain<true>": 5,
    "pt_features_rays<false>": 7, "pt_features_rays<true>": 5,
    "pt_features_cameras<false>": 5, "pt_features_cameras<true>": 4,
    "pt_occluded<false>": 8, "pt_occluded<true>": 8,
    "pt_occluded_hemi<false, false>": 8, "pt_occluded_hemi<false, true>": 8,
    "pt_occluded_hemi<true, false>": 8, "pt_occluded_hemi<true, true>": 8,
    # <COUNT, ACCEL>
    "pt_render_rays<false, false>": 5, "pt_render_rays<false, true>": 4,
    "pt_render_rays<true, false>": 5, "pt_render_rays<true, true>": 3,
    "pt_render_raysets<false, false>": 5, "pt_render_raysets<false, true>": 4,
    "pt_render_raysets<true, false>": 5, "pt_render_raysets<true, true>": 4,
}


def waves_per_simd(vgpr):
    return min(8, 512 // max(8, (vgpr + 7) // 8 * 8))


@pytest.fixture(scope="module")
def builds():
    procs = [subprocess.Popen([sys.executable, ISA, "--arith", str(k), "--json"], stdout=subprocess.PIPE, text=True,
                              env=dict(os.environ, ISA_EXTRA_FLAGS="")) for k in (0, 1, 2)]
    outs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0, 0]
    return [json.loads(o) for o in outs]


def test_every_kernel_is_still_instantiated(builds):
    for k, build in enumerate(builds):
        assert len(build) == KERNELS_PER_POLICY, (k, len(build))
        named = sorted(n.split("::", 1)[1] for n in build if n.split("::", 1)[1].startswith(FAMILIES))
        assert named == sorted(WAVES), (k, sorted(set(named) ^ set(WAVES)))


@pytest.mark.parametrize("policy", [0, 1, 2])
def test_no_scratch_no_spill_and_no_occupancy_step_lost(builds, policy):
    build = builds[policy]
    for name, before in sorted(WAVES.items()):
        k = build["pt_a%d::%s" % (policy, name)]
        waves = waves_per_simd(k["vgpr"])
        print("policy %d  %-40s vgpr %3d  waves %d (before: %d)  scratch %d  spilled %d  VALU %4d  SALU %4d" %
              (policy, name, k["vgpr"], waves, before, k["scratch"], k["spilled_vgprs"], k["valu"], k["salu"]))
        assert k["scratch"] == 0 and k["spilled_vgprs"] == 0, (policy, name, k["scratch"], k["spilled_vgprs"])
        assert waves >= before, (policy, name, k["vgpr"], waves, before)
