#!/usr/bin/env python3
"""tools/prefix_cache_bench.py [--workload c2] [--spp N] [--steps 20] [--warmup 5] [--arith 2] [--cameras 2] [--cache 0|1]
What a MOVING camera pays for the prefix cache (RT_OPT_PREFIX_CACHE): bench.py's step — clear, one fused call, resolve —
with the camera alternating between `--cameras` blocks (the workload's, and copies whose first float is one ulp
further on), so that with 2 or more every call traces its prefix in full while the cache is on.  --cameras 1 is the camera
at rest.  Prints one JSON line: wall time per step, the means of the two stages' HIP-event times over the timed steps,
the context's hit / miss counts and a hash of the last frame."""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import opencl_raytracing_amd as rt

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="c2")
ap.add_argument("--spp", type=int, default=0)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--arith", type=int, default=2)
ap.add_argument("--cameras", type=int, default=2)
ap.add_argument("--cache", type=int, default=None, help="RT_OPT_PREFIX_CACHE (default: the library's)")
args = ap.parse_args()

wl = rt.workloads.get(args.workload)
spp = args.spp or wl.spp
cams = [np.array(wl.camera, dtype=np.float32)]
for _ in range(1, args.cameras):
    c = cams[-1].copy()
    c[0] = np.nextafter(c[0], np.float32(np.inf))
    cams.append(c)
t = rt.RayTracer(wl.width, wl.height, scene=wl.scene, seed=rt.workloads.SEED)
t.setArith(args.arith)
if args.cache is not None:
    t.setOption(t.OPT_PREFIX_CACHE, args.cache)


def step(k):
    t.clear()
    t.renderSamples(cams[k % len(cams)], 0, spp)
    t.resolve()


for k in range(args.warmup):
    step(k)
t.sync()
stats = t.prefixCacheStats if hasattr(t, "prefixCacheStats") else (lambda: (0, 0))   # (a library from before the cache)
h0, m0 = stats()
t0 = time.perf_counter()
for k in range(args.steps):
    step(args.warmup + k)
t.sync()
wall = time.perf_counter() - t0
h1, m1 = stats()
launches = min(64, args.steps * -(-spp // 512))
first, second = t.stageMsHistory(launches)
print(json.dumps({"workload": args.workload, "size": [wl.width, wl.height], "spp": spp, "cameras": len(cams),
                  "cache": args.cache, "steps": args.steps, "ms_per_step": round(wall / args.steps * 1e3, 4),
                  "first_stage_ms": round(float(np.mean(first)), 4), "second_stage_ms": round(float(np.mean(second)), 4),
                  "hits": h1 - h0, "misses": m1 - m0, "walk_overflow": t.walkOverflow(),
                  "image": hashlib.sha1(t.readLinear().tobytes()).hexdigest()[:16]}))
t.close()
