"""CPU: the switch that makes an interaction of the sample queue gather only the random-table entries its material reads
(csrc/pt_queue.hpp PT_RND_BY_USE, pt_device.hpp fetch_rnd_by_use, profiles/r22_experiments.md) is live and confined — read
from the compiler's listing, not from the source text: the device code of arithmetic policy 2 is compiled as shipped and with
the switch off (tools/isa_stats.py, two compilations side by side), and the two are compared kernel by kernel.  Were the
kernel to fall back to the two unconditional gathers, no kernel would differ and this fails; were the change to leak into
another kernel — the camera rows, the mesh rows (GEOM 1), the counting builds, the ACCEL rows, pt_samples_w — that fails too."""
import json
import os
import re
import subprocess
import sys

import cases

FAMILY = "pt_samples_q<false, false, 0, "   # COUNT = false, ACCEL = false, GEOM = 0
VGPR_BUDGET = 80                         # __launch_bounds__(64, 6): 512 / 6, in the allocation granule of 8


def _isa(extra):
    env = dict(os.environ, ISA_EXTRA_FLAGS=extra)
    return subprocess.Popen([sys.executable, os.path.join(cases.ROOT, "tools", "isa_stats.py"), "--arith", "2", "--json"],
                            stdout=subprocess.PIPE, env=env, text=True)


def _is_cam(name):
    """pt_samples_q<COUNT, ACCEL, GEOM, WAVES, MOMENTS, COUNT_LOG2, CAM>: the last template argument."""
    args = re.search(r"<(.*)>", name).group(1).split(", ")
    return len(args) == 7 and args[6] == "true"


def test_the_switch_changes_the_mesh_free_queue_kernels_without_camera_and_nothing_else():
    procs = [_isa(""), _isa("-DPT_RND_BY_USE=0")]
    outs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0]
    on, off = (json.loads(o) for o in outs)
    assert sorted(on) == sorted(off)
    differ = sorted(k for k in on if on[k] != off[k])
    touched = sorted(k for k in on if FAMILY in k and not _is_cam(k))
    assert len(touched) == 3, touched          # generic, MOMENTS, COUNT_LOG2 = 6
    assert differ == touched, (differ, touched)
    for k in touched:
        assert on[k]["scratch"] == 0 and on[k]["spilled_vgprs"] == 0 and on[k]["scratch_ops"] == 0, (k, on[k])
        assert on[k]["vgpr"] <= VGPR_BUDGET, (k, on[k]["vgpr"])
        # the same two gathers, each in a branch of its own, and no read of the type: no vector-memory or LDS instruction more
        assert on[k]["vmem"] <= off[k]["vmem"] and on[k]["lds"] <= off[k]["lds"], (k, on[k], off[k])
