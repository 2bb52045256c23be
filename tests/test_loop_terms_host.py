"""CPU: the switch that makes the sample queue ask "is the table staged?" of the scene's counts (csrc/pt_queue.hpp
PT_TABLES_BY_COUNT, DESIGN §8, profiles/r20_experiments.md) is live and confined — read from the compiler's listing, not from
the source text: the device code of arithmetic policy 2 is compiled as shipped and with the switch off (tools/isa_stats.py,
two compilations side by side), and the two are compared kernel by kernel.  Were the tag to fall back to the pointer test,
by the switch or by a rewrite, no kernel would differ and this fails; were it to leak into another kernel, that fails too."""
import json
import os
import subprocess
import sys

import cases

TOUCHED = "pt_samples_q<false, false, "   # COUNT = false, ACCEL = false: the instantiations that copy the staged block


def _isa(extra):
    env = dict(os.environ, ISA_EXTRA_FLAGS=extra)
    return subprocess.Popen([sys.executable, os.path.join(cases.ROOT, "tools", "isa_stats.py"), "--arith", "2", "--json"],
                            stdout=subprocess.PIPE, env=env, text=True)


def test_the_switch_changes_the_queue_kernels_without_counters_and_nothing_else():
    procs = [_isa(""), _isa("-DPT_TABLES_BY_COUNT=0")]
    outs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0]
    on, off = (json.loads(o) for o in outs)
    assert sorted(on) == sorted(off)
    differ = sorted(k for k in on if on[k] != off[k])
    touched = sorted(k for k in on if TOUCHED in k)
    assert len(touched) == 8, touched          # GEOM 0 | 1 x generic, MOMENTS, COUNT_LOG2 = 6, CAM
    assert differ == touched, (differ, touched)
    for k in touched:
        # registers and scratch are the pointer test's; both arms of every presence test exist either way
        for field in ("vgpr", "scratch", "spilled_vgprs", "vmem", "lds", "lds_static"):
            assert on[k][field] == off[k][field], (k, field, on[k][field], off[k][field])
    # the headline instantiation (C2 at 64 spp): the presence tests are scalar compares — more SALU, no more VALU
    head = [k for k in touched if k.endswith("<false, false, 0, 6, false, 6, false>")]
    assert len(head) == 1, touched
    assert on[head[0]]["salu"] > off[head[0]]["salu"] and on[head[0]]["valu"] <= off[head[0]]["valu"]
