"""CPU: the brute-force sphere scan that asks the wave first (csrc/pt_device.hpp sphere_take<FAST>, -DPT_SPHERE_ANY_FIRST,
DESIGN §5 and §8, profiles/r30_experiments.md) is live and confined — read from the compiler's listing, not from the source
text, as tests/test_loop_terms_host.py does: the device code of arithmetic policy 2 is compiled as shipped and with the switch
at 0 (tools/isa_stats.py --json --digest, side by side), policy 0 both ways, and the builds are compared kernel by kernel.
The switch moves instructions behind a branch and changes almost no total, so "differs" is asked of a hash of each kernel's
instructions, operands included.

The property itself is read from the headline kernel's listing (tools/isa_stats.py --listing): in the inner loop that holds
the second s_load_dwordx16 (the next batch of four spheres), the common path is the one a wave takes when no lane needs a
sphere's roots — every s_cbranch_vccz and s_cbranch_execz taken, from the loop's header to its back-edge.  Shipped, that path
holds one compare per sphere, each directly in front of its s_cbranch_vccz; with the switch at 0 it holds four per sphere and
no s_cbranch_vccz at all."""
import json
import os
import re
import subprocess
import sys

import pytest

import cases

OFF = "-DPT_SPHERE_ANY_FIRST=0"
HEAD = "pt_samples_q<false, false, 0, 6, false, 6, false>"   # C2 at 64 spp
# hit_primitives<..., FAST> with PT_ROOT_UPDATE: FAST = PT_OCL && !COUNT && !ACCEL && GEOM != 2
TOUCHED = sorted(["pt_a2::pt_samples_q<false, false, %d, 6, %s>" % (g, rest) for g in (0, 1)
                  for rest in ("false, -1, false", "true, -1, false", "false, 6, false", "false, -1, true")] +
                 ["pt_a2::pt_samples_q_%s<false, %d, 6>" % (k, g) for k in ("rays", "raysets") for g in (0, 1)])
ISA = os.path.join(cases.ROOT, "tools", "isa_stats.py")


def _isa(arith, extra):
    env = dict(os.environ, ISA_EXTRA_FLAGS=extra)
    return subprocess.Popen([sys.executable, ISA, "--arith", str(arith), "--json", "--digest"], stdout=subprocess.PIPE, env=env, text=True)


@pytest.fixture(scope="module")
def builds():
    procs = [_isa(2, ""), _isa(2, OFF), _isa(0, ""), _isa(0, OFF)]
    outs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0, 0, 0]
    return [json.loads(o) for o in outs]


def test_the_switch_changes_the_twelve_tagged_scans_and_nothing_else(builds):
    on, off, on0, off0 = builds
    assert sorted(on) == sorted(off) and sorted(on0) == sorted(off0)       # the same kernel names
    assert len(TOUCHED) == 12 and all(k in on for k in TOUCHED), [k for k in TOUCHED if k not in on]
    differ = sorted(k for k in on if on[k] != off[k])
    assert differ == TOUCHED, (sorted(set(differ) - set(TOUCHED)), sorted(set(TOUCHED) - set(differ)))
    assert [k for k in on0 if on0[k] != off0[k]] == []                       # policy 0 has no tagged scan


def test_no_register_no_scratch_and_no_instruction_more(builds):
    on, off, _, _ = builds
    for k in TOUCHED:
        for field in ("vgpr", "sgpr", "scratch", "spilled_vgprs", "scratch_ops", "vmem", "lds", "lds_static"):
            assert on[k][field] == off[k][field], (k, field, on[k][field], off[k][field])
        assert on[k]["valu"] <= off[k]["valu"] and on[k]["salu"] <= off[k]["salu"], (k, on[k]["valu"], off[k]["valu"], on[k]["salu"], off[k]["salu"])
        print("%-60s vgpr %3d sgpr %3d  VALU %4d / %4d  SALU %4d / %4d" %
              (k, on[k]["vgpr"], on[k]["sgpr"], on[k]["valu"], off[k]["valu"], on[k]["salu"], off[k]["salu"]))


def _listing(extra):
    """Labels and instructions of the headline kernel.  tools/isa_stats.py keeps one listing per (policy, extra flags) under
    build/ and compiles only when a source is newer: after the `builds` fixture — which the test below takes for that
    reason — this call reads the listing that fixture's run left; run without it, it would compile first (half a minute)."""
    env = dict(os.environ, ISA_EXTRA_FLAGS=extra)
    out = subprocess.run([sys.executable, ISA, "--arith", "2", "--listing", HEAD], stdout=subprocess.PIPE, env=env, text=True, check=True).stdout
    lines = out.strip().split("\n")
    assert lines[0] == "; pt_a2::" + HEAD and not any(l.startswith("; ") for l in lines[1:]), lines[0]
    return lines[1:]


def _common_path(code):
    """The instructions from the header of the loop that holds the second s_load_dwordx16 to that loop's back-edge, every
    s_cbranch_vccz and s_cbranch_execz taken and no other conditional branch: what a wave issues when no lane needs roots."""
    loads = [i for i, l in enumerate(code) if l.startswith("s_load_dwordx16")]
    assert len(loads) == 2, loads
    label = {l.split(":")[0]: i for i, l in enumerate(code) if l.startswith(".LBB")}
    # the loop's header: the nearest label above the load that is not "in Loop: Header=..." of another one
    head = max(i for l, i in label.items() if i < loads[1] and "in Loop:" not in code[i])
    name = code[head].split(":")[0]
    path, i, seen = [], head + 1, set()
    while i != head:
        assert i not in seen and i < len(code), ("the path does not come back to the header", code[head], len(path))
        seen.add(i)
        ins = code[i]
        if ins.startswith(".LBB"):
            assert "Header=" + name[2:] in ins, ("the path left the loop", ins)
            i += 1
            continue
        path.append(ins)
        op, _, arg = ins.partition(" ")
        if op in ("s_cbranch_vccz", "s_cbranch_execz", "s_branch"):
            i = label[arg.strip()]
        else:
            i += 1
    return path


def _compares_and_their_successors(path):
    real = [p for p in path if not p.startswith(("s_waitcnt", "s_nop"))]
    return [(p.split()[0], real[k + 1].split()[0]) for k, p in enumerate(real[:-1]) if p.startswith("v_cmp")]


def test_one_compare_per_sphere_on_the_common_path(builds):
    on, off = _common_path(_listing("")), _common_path(_listing(OFF))
    c_on, c_off = _compares_and_their_successors(on), _compares_and_their_successors(off)
    n_vccz = lambda path: sum(p.startswith("s_cbranch_vccz") for p in path)
    valu = lambda path: sum(p.startswith("v_") for p in path)
    salu = lambda path: sum(bool(re.match(r"s_(?!waitcnt|nop|load)", p)) for p in path)
    print("common path of one batch of four spheres: VALU %d -> %d, SALU %d -> %d, compares %d -> %d" %
          (valu(off), valu(on), salu(off), salu(on), len(c_off), len(c_on)))
    assert len(c_on) == 4 and n_vccz(on) == 4, (c_on, n_vccz(on))
    assert all(c == ("v_cmp_lt_f32_e32", "s_cbranch_vccz") for c in c_on), c_on       # `0 < dis`, then the wave's branch
    assert len(c_off) == 16 and n_vccz(off) == 0, (c_off, n_vccz(off))
    assert valu(off) - valu(on) == 12, (valu(off), valu(on))                           # three compares a sphere, nothing else
