"""CPU: the two switches of the stored frame (csrc/pt_sample.hpp PT_ACCUM_STORE, csrc/pt_queue.hpp PT_SUMS_ADDR; DESIGN §5 "A cleared frame is
stored") are live and confined — read from the compiler's listings (tools/isa_stats.py), not from the source text.  Policy 2
is compiled as shipped, with either switch off and with both off, policy 0 as shipped and with both off; the builds are
compared kernel by kernel through the digest of their instructions.

The kernels that may differ are the ones a qualifying launch runs (launch_fused_any): pt_final_replay, pt_prefix without
counters and without a BVH walk (with and without the tree phase), and the two pt_samples_q<false, false, 0 | 1, …,
COUNT_LOG2 = 6> kernels: five per policy.  The moments rows, the camera rows, the ray forms, the counting builds and everything
with a BVH walk keep their code, as the issue lists them.  The generic-count kernels keep theirs by this change's own choice:
built with the store arm, C3's kernel at 256 samples measured 0.5 % slower (profiles/r32_experiments.md), so a call stores
only at exactly 64 samples per pixel."""
import json
import os
import re
import subprocess
import sys

import pytest

import cases

ISA = os.path.join(cases.ROOT, "tools", "isa_stats.py")
OFF = {"store": "-DPT_ACCUM_STORE=0", "addr": "-DPT_SUMS_ADDR=0"}
BOTH_OFF = OFF["store"] + " " + OFF["addr"]
HEADLINE = "pt_samples_q<false, false, 0, 6, false, 6, false>"


def _names(ns):
    queue = ["%s::pt_samples_q<false, false, %d, 6, false, 6, false>" % (ns, geom) for geom in (0, 1)]
    first = ["%s::pt_final_replay" % ns, "%s::pt_prefix<false, false, false>" % ns, "%s::pt_prefix<false, false, true>" % ns]
    return sorted(queue), sorted(first)


def _isa(arith, extra, *more):
    env = dict(os.environ, ISA_EXTRA_FLAGS=extra)
    return subprocess.Popen([sys.executable, ISA, "--arith", str(arith)] + list(more), stdout=subprocess.PIPE, env=env, text=True)


@pytest.fixture(scope="module")
def builds():
    """{(policy, flags): the --json --digest dump}: six compilations side by side."""
    keys = [(2, ""), (2, OFF["store"]), (2, OFF["addr"]), (2, BOTH_OFF), (0, ""), (0, BOTH_OFF)]
    procs = [_isa(a, extra, "--json", "--digest") for a, extra in keys]
    outs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0] * len(keys)
    return {k: json.loads(o) for k, o in zip(keys, outs)}


def _differ(a, b):
    assert sorted(a) == sorted(b)
    return sorted(k for k in a if a[k]["code_sha1"] != b[k]["code_sha1"])


@pytest.mark.parametrize("policy", [2, 0])
def test_the_switches_change_the_kernels_of_a_qualifying_launch_and_nothing_else(builds, policy):
    on, off = builds[policy, ""], builds[policy, BOTH_OFF]
    queue, first = _names("pt_a%d" % policy)
    assert all(k in on for k in queue + first), sorted(set(queue + first) - set(on))
    assert _differ(on, off) == sorted(queue + first)
    for k in queue + first:
        # no scratch, no spilled register, and not a register more than without the switches
        assert on[k]["scratch"] == 0 and on[k]["spilled_vgprs"] == 0, (k, on[k])
        assert on[k]["vgpr"] <= off[k]["vgpr"] and on[k]["sgpr"] <= off[k]["sgpr"], (k, on[k], off[k])
        print("%-60s VGPR %3d -> %3d  SGPR %3d -> %3d  VALU %4d -> %4d  VMEM %2d -> %2d  LDS %2d -> %2d" % (
            k, off[k]["vgpr"], on[k]["vgpr"], off[k]["sgpr"], on[k]["sgpr"], off[k]["valu"], on[k]["valu"], off[k]["vmem"],
            on[k]["vmem"], off[k]["lds"], on[k]["lds"]))


def test_each_switch_alone_changes_its_own_kernels(builds):
    off = builds[2, BOTH_OFF]
    queue, first = _names("pt_a2")
    # PT_SUMS_ADDR 0 leaves the store arm: every kernel of a qualifying launch
    assert _differ(builds[2, OFF["addr"]], off) == sorted(queue + first)
    # PT_ACCUM_STORE 0 leaves the sums' addresses: the two queue kernels
    assert _differ(builds[2, OFF["store"]], off) == queue
    # and each is live in the shipped build
    assert _differ(builds[2, ""], builds[2, OFF["store"]]) == sorted(queue + first)
    assert _differ(builds[2, ""], builds[2, OFF["addr"]]) == queue


def _epilogue(extra):
    """The headline kernel's epilogue, from the label behind its last loop to the end, as basic blocks: [[opcode, …], …] (a
    block ends at a label and behind a branch)."""
    p = _isa(2, extra, "--listing", HEADLINE)
    code = p.communicate()[0].split("\n")
    assert p.returncode == 0 and code[0].endswith(HEADLINE), code[:1]
    label = re.compile(r"\.LBB\d+_\d+:")
    loops = [i for i, line in enumerate(code) if label.match(line) and "Loop" in line]
    start = next(i for i in range(loops[-1] + 1, len(code)) if label.match(code[i]) and "Loop" not in code[i])
    assert loops[-1] > len(code) // 2
    blocks = [[]]
    for line in code[start:]:
        if not line:
            continue
        if label.match(line):
            blocks.append([])
            continue
        op = line.split()[0]
        blocks[-1].append(op)
        if op.startswith(("s_cbranch", "s_branch", "s_endpgm")):
            blocks.append([])
    blocks = [b for b in blocks if b]
    assert blocks[-1][-1] == "s_endpgm"
    return blocks


def _arms(blocks):
    """Of the blocks that write the accumulator: (those that store without a load, those that load and then store)."""
    writers = [b for b in blocks if "global_store_dwordx4" in b]
    store = [b for b in writers if "global_load_dwordx4" not in b]
    add = [b for b in writers if "global_load_dwordx4" in b and b.index("global_load_dwordx4") < b.index("global_store_dwordx4")]
    assert len(store) + len(add) == len(writers)
    return store, add


def test_the_headline_epilogue_stores_without_a_load_and_issues_less(builds):
    on, off = _epilogue(""), _epilogue(BOTH_OFF)
    assert sum(op.startswith("v_permlane16_swap") for b in on for op in b) == 6   # two passes of the tree, three channels
    # whatever the order of the blocks: each of the two passes ends in a block that stores with no load in it (and no wait
    # for vector memory: there is nothing to wait for) and in one that loads, adds and stores
    store, add = _arms(on)
    assert len(store) == 2 and len(add) == 2, (store, add)
    for b in store:
        assert not any(op.startswith(("global_load", "flat_load", "buffer_load")) for op in b), b
    # the parent's epilogue has the add arm alone
    store_off, add_off = _arms(off)
    assert len(store_off) == 0 and len(add_off) == 2, (store_off, add_off)
    valu = [sum(op.startswith("v_") for b in blocks for op in b) for blocks in (on, off)]
    lds = [sum(op.startswith("ds_read") for b in blocks for op in b) for blocks in (on, off)]
    print("headline epilogue, static VALU instructions: %d shipped, %d with both switches off" % tuple(valu))
    print("headline epilogue, LDS reads: %d shipped, %d with both switches off" % tuple(lds))
    assert valu[0] < valu[1], valu
