#!/usr/bin/env python3
"""tools/compat_bench.py [--runs 3] [--spp 64] [--root DIR] [--lib FILE] [--only NAME] [--waste] [--cameras]
Progressive (compat) path timing: render + (spp-1) x renderAgain, one host sync per call, exactly the reference's
interactive loop (src/raytracer.cpp:127-165) — with look-ahead off (RT_OPT_LOOKAHEAD 0: one direct launch per call) and
with the library's default (one fused launch per 16 samples whose frames the calls hand out), in ONE process, the two
alternating, --runs timed sequences each after a warmed one, at 1080p for C2, C3 and C5 and at 1200x800 for all_kinds.
Per configuration: every run's sequence time (host clock around calls that each end in a device synchronise), and the
per-call times of the last run split into the calls that launched a batch and the calls that were served a frame, with the
device time of each (rt_kernel_ms_history: the launch for a batch call, the copy for a served call).
--root DIR imports the package (and its librt_amd.so) from another checkout of the project — a library from before the
option is timed as it is, so that two checkouts can be alternated process by process.
--lib FILE loads a variant build of librt_amd.so (tools/build_variant.sh), e.g. the pixel-major ring.
--waste: what a batch costs when the camera moves right after it — render + renderAgain (launches a batch) + render with
another camera, against the same with look-ahead off.
--cameras: progressive anti-aliasing (rt_render_again_cameras) instead — C2 and C5 at 1080p, policy 2 unless --arith says
otherwise, render + --calls (default 128) calls per sequence, --runs (here default 5) rounds after a warmed one with the
configurations alternating inside each round; per configuration the time per call by the host's clock, synchronise
included, as median (min .. max) over the rounds:
    a          plain renderAgain, look-ahead 16, the unjittered camera — the loop without anti-aliasing
    b          renderAgain with a freshly jittered block on every call (look-ahead 16: never a batch) — anti-aliasing before
               rt_render_again_cameras
    c K        renderAgainCameras over a table of 64 jittered blocks, look-ahead K = 0, 16, 64
and, for c 16 and c 64, the device time of a batch launch and of one frame copy (the start-image copy is such a copy)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--lib", default="")
ap.add_argument("--only", default="")
ap.add_argument("--waste", action="store_true")
ap.add_argument("--arith", type=int, default=None, help="RT_OPT_ARITH (default: the library's)")
ap.add_argument("--cameras", action="store_true")
ap.add_argument("--calls", type=int, default=128)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import numpy as np  # noqa: E402
import opencl_raytracing_amd as rt  # noqa: E402

if args.lib:
    rt.load_library(os.path.abspath(args.lib))
HAS = hasattr(rt.RayTracer, "OPT_LOOKAHEAD")
CASES = (("c2", 1920, 1080, {}), ("c3", 1920, 1080, {}), ("c5", 1920, 1080, {}), ("all_kinds", 1200, 800, {}))


def sequence(t, cam, spp):
    """→ (sequence seconds, per-call seconds of render + the renderAgain calls)"""
    calls = []
    t0 = time.perf_counter()
    t.render(cam)
    calls.append(time.perf_counter() - t0)
    for _ in range(spp - 1):
        c0 = time.perf_counter()
        t.renderAgain(cam)
        calls.append(time.perf_counter() - c0)
    return time.perf_counter() - t0, calls


def ms(v):
    return "%.3f" % (1e3 * v)


def jittered(block, n, w, h):
    """n blocks about `block`: Camera.sampleBlocks' pixel jitter applied to a camera block"""
    block = np.asarray(block, np.float32)
    off = rt.Camera.sampleOffsets(n)
    out = np.tile(block, (n, 1))
    for j in range(n):
        out[j, 3:6] = block[3:6] + (off[j, 0] / np.float32(w)) * block[6:9] + (off[j, 1] / np.float32(h)) * block[9:12]
    return out


def cameras_bench():
    runs = args.runs if "--runs" in sys.argv else 5
    for name, w, h in (("c2", 1920, 1080), ("c5", 1920, 1080)):
        if args.only and name != args.only:
            continue
        wl = rt.workloads.get(name, width=w, height=h)
        t = rt.RayTracer(w, h, scene=wl.scene)
        t.setArith(2 if args.arith is None else args.arith)
        table = jittered(wl.camera, 64, w, h)
        fresh = jittered(wl.camera, args.calls + 1, w, h)

        def run(label):
            """→ (seconds per call of the calls after render, device ms of those calls)"""
            kind, k = label[0], int(label.split()[1]) if " " in label else 16
            t.setOption(t.OPT_LOOKAHEAD, k)
            t.render(wl.camera if kind == "a" else fresh[0] if kind == "b" else table[0])
            t0 = time.perf_counter()
            for i in range(1, args.calls + 1):
                if kind == "a":
                    t.renderAgain(wl.camera)
                elif kind == "b":
                    t.renderAgain(fresh[i])
                else:
                    t.renderAgainCameras(table)
            dt = (time.perf_counter() - t0) / args.calls
            return dt, t.kernelMsHistory(64)

        labels = ["a", "b", "c 0", "c 16", "c 64"]
        res, dev = {x: [] for x in labels}, {}
        for x in labels:
            run(x)                                   # warm: code objects, the ring, the camera tables
        for _ in range(runs):
            for x in labels:                         # alternating inside the round
                dt, dev[x] = run(x)
                res[x].append(1e3 * dt)
        out = {"workload": name, "size": [w, h], "calls": args.calls, "rounds": runs, "per_call_ms": {}}
        for x in labels:
            v = res[x]
            out["per_call_ms"][x] = [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
            print("%s %dx%d %s: %.4f ms per call (%.4f .. %.4f)" % (name, w, h, x, np.median(v), min(v), max(v)), flush=True)
        for x in ("c 16", "c 64"):
            # (the last 64 calls' device times: the few large ones are batch launches, the rest frame copies)
            d = sorted(dev[x])
            out[x + " device_ms"] = {"batch_launch": round(d[-1], 4), "frame_copy": round(float(np.median(d)), 4)}
            print("%s %s: batch launch %.4f ms, one frame copy %.4f ms on the device" % (name, x, d[-1], float(np.median(d))), flush=True)
        st = t.lookaheadStats()
        out["lookahead_stats"] = list(st)
        print("RESULT " + json.dumps(out), flush=True)
        t.close()


if args.cameras:
    cameras_bench()
    sys.exit(0)

for name, w, h, kw in CASES:
    if args.only and name != args.only:
        continue
    wl = rt.workloads.get(name, width=w, height=h, **kw)
    t = rt.RayTracer(w, h, scene=wl.scene)
    if args.arith is not None:
        t.setArith(args.arith)
    default_k = rt.lookahead_plan(w, h) if HAS else None
    configs = [("lookahead 0", 0), ("lookahead %d" % default_k, default_k)] if HAS else [("as built", None)]
    cam2 = np.array(wl.camera, dtype=np.float32)
    cam2[0] += np.float32(0.25)

    def select(k):
        if k is not None:
            t.setOption(t.OPT_LOOKAHEAD, k)

    res = {label: [] for label, _ in configs}
    last = {}
    for label, k in configs:                       # warm every configuration (code objects, the ring's allocation)
        select(k)
        sequence(t, wl.camera, args.spp)
    for _ in range(args.runs):
        for label, k in configs:                   # alternating
            select(k)
            dt, calls = sequence(t, wl.camera, args.spp)
            res[label].append(dt)
            last[label] = (calls, t.kernelMsHistory(64)[-(args.spp - 1):], k)
    out = {"workload": name, "size": [w, h], "spp": args.spp, "root": os.path.abspath(args.root), "sequence_ms": {}}
    for label, _ in configs:
        out["sequence_ms"][label] = [round(1e3 * v, 3) for v in res[label]]
        calls, dev, k = last[label]
        again = calls[1:]
        line = "%s %dx%d %d calls, %s: sequence %s ms" % (name, w, h, args.spp, label, " ".join(ms(v) for v in res[label]))
        if k:
            batch = [i for i in range(len(again)) if i % k == 0]
            served = [i for i in range(len(again)) if i % k]
            stat = lambda idx, a: float(np.median([a[i] for i in idx]))   # noqa: E731
            out[label] = {"batch_call_ms": round(1e3 * stat(batch, again), 3), "batch_device_ms": round(stat(batch, dev), 3),
                          "served_call_ms": round(1e3 * stat(served, again), 3), "served_copy_device_ms": round(stat(served, dev), 3)}
            line += "; batch call %.3f ms (launch on the device %.3f), served call %.3f ms (copy on the device %.3f)" % (
                1e3 * stat(batch, again), stat(batch, dev), 1e3 * stat(served, again), stat(served, dev))
        else:
            out[label] = {"call_ms": round(1e3 * float(np.median(again)), 3), "device_ms": round(float(np.median(dev)), 3)}
            line += "; call %.3f ms (kernel on the device %.3f)" % (1e3 * float(np.median(again)), float(np.median(dev)))
        print(line, flush=True)
    if args.waste and HAS:
        # the camera moves right after a batch: render, renderAgain (batch / direct), render elsewhere
        waste = {}
        for label, k in configs:
            select(k)
            v = []
            for r in range(args.runs + 1):
                t.render(wl.camera)
                c0 = time.perf_counter()
                t.renderAgain(wl.camera)
                c1 = time.perf_counter()
                t.render(cam2)
                if r:
                    v.append(c1 - c0)
            waste[label] = [round(1e3 * x, 3) for x in v]
            print("%s: renderAgain followed by a camera change, %s: %s ms" % (name, label, " ".join(ms(x) for x in v)), flush=True)
        out["wasted_batch_call_ms"] = waste
    print("RESULT " + json.dumps(out), flush=True)
    t.close()
