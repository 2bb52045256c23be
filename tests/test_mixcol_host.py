"""CPU: mixCol's minimum without canonicalising moves (csrc/pt_arith.hpp vmin<FAST>, -DPT_MIXCOL_FAST) and the carried
state written in place (-DPT_STATE_IN_PLACE) are live and confined (profiles/r29_experiments.md) — read
from the compiler's listing, not from the source text: the device code of arithmetic policy 2 is compiled as shipped and with
both switches off (tools/isa_stats.py, side by side, as tests/test_loop_terms_host.py does) and compared kernel by kernel;
policy 0, whose minimum compares and selects and has no tagged form, is compiled once for its register budget."""
import json
import os
import subprocess
import sys

import pytest

import cases

TOUCHED = "pt_samples_q<false, false, "   # COUNT = false, ACCEL = false: GEOM 0 | 1 x generic, MOMENTS, COUNT_LOG2 = 6, CAM
HEAD = "<false, false, 0, 6, false, 6, false>"   # C2 at 64 spp


def _isa(arith, extra):
    env = dict(os.environ, ISA_EXTRA_FLAGS=extra)
    return subprocess.Popen([sys.executable, os.path.join(cases.ROOT, "tools", "isa_stats.py"), "--arith", str(arith), "--json"],
                            stdout=subprocess.PIPE, env=env, text=True)


def _opcodes(arith, extra, kernel_suffix):
    """Static opcode histogram of one kernel from the listing the --json run left behind (isa_stats.kernels)."""
    sys.path.insert(0, os.path.join(cases.ROOT, "tools"))
    import isa_stats
    tag = ("_" + "_".join(e.lstrip("-D").replace("=", "") for e in extra.split())) if extra else ""
    path = os.path.join(cases.ROOT, "build", "pt_kernels_a%d_gfx950%s.s" % (arith, tag))
    ks = [k for k in isa_stats.kernels(path).values() if k["demangled"].endswith("pt_samples_q" + kernel_suffix)]
    assert len(ks) == 1, [k["demangled"] for k in ks]
    return ks[0]["ops"]


def _count(ops, prefix):
    return sum(n for o, n in ops.items() if o.startswith(prefix))


@pytest.fixture(scope="module")
def builds():
    off_flags = "-DPT_MIXCOL_FAST=0 -DPT_STATE_IN_PLACE=0"
    procs = [_isa(2, ""), _isa(2, off_flags), _isa(0, "")]
    outs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0, 0]
    on, off, ieee = (json.loads(o) for o in outs)
    return on, off, ieee, off_flags


def test_the_switches_change_the_queue_kernels_without_counters_and_nothing_else(builds):
    on, off, _, _ = builds
    assert sorted(on) == sorted(off)                      # the same kernel names in both builds
    differ = sorted(k for k in on if on[k] != off[k])
    touched = sorted(k for k in on if TOUCHED in k)
    assert len(touched) == 8, touched
    assert differ == touched, (differ, touched)


def test_no_scratch_no_spill_and_no_register_more(builds):
    on, off, ieee, _ = builds
    for name, ks in (("policy 2", on), ("policy 2, switches off", off), ("policy 0", ieee)):
        bad = sorted(k for k, v in ks.items() if TOUCHED in k and (v["scratch"] or v["spilled_vgprs"] or v["scratch_ops"]))
        assert not bad, (name, bad)
    for k in on:
        if TOUCHED in k:
            assert on[k]["vgpr"] <= off[k]["vgpr"], (k, on[k]["vgpr"], off[k]["vgpr"])


def test_the_headline_kernel_lost_its_canonicalising_moves(builds):
    _, _, _, off_flags = builds
    ops_on, ops_off = _opcodes(2, "", HEAD), _opcodes(2, off_flags, HEAD)
    max_on, max_off = _count(ops_on, "v_max_f32"), _count(ops_off, "v_max_f32")
    mov_on, mov_off = _count(ops_on, "v_mov_b32"), _count(ops_off, "v_mov_b32")
    print("headline kernel: v_max_f32 %d -> %d, v_mov_b32 %d -> %d, v_min_f32 %d -> %d" %
          (max_off, max_on, mov_off, mov_on, _count(ops_off, "v_min_f32"), _count(ops_on, "v_min_f32")))
    assert max_on <= max_off - 12, (max_on, max_off)      # two sites x three minima x two operands
    assert _count(ops_on, "v_min_f32") == _count(ops_off, "v_min_f32")
    assert mov_on < mov_off, (mov_on, mov_off)
