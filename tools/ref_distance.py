#!/usr/bin/env python3
"""tools/ref_distance.py [--hsaco default|nocontract] [--out FILE] — GPU box.

How far is the arithmetic contract this build is pinned to ("reference source + IEEE-plain builtins,
no FMA": oracle/ref_shim.cpp = oracle/pt_oracle.c = the HIP kernels, bit for bit) from what the
reference computes when ROCm's own OpenCL tool chain builds kernels/raytracer.cl for gfx950 with its
real builtin library (oracle/_ref/gfx950/, see oracle/Makefile)?  Same scene arrays, camera block and
random table go to both; per pixel-sample the two either agree bit for bit or take different paths
(the table index is a hash of the ray direction, raytracer.cl:113-125).

For each non-textured workload: per-sample frames (samples 0..3) compared bit-wise, and the spp-sample
mean image compared against the Monte-Carlo noise floor (our own samples [spp, 2·spp) as the yardstick).
Prints one JSON object."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import opencl_raytracing_amd as rt  # noqa: E402
import oracle as orc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--hsaco", default="default", choices=["default", "nocontract"])
ap.add_argument("--out", default="")
ap.add_argument("--workloads", default="c1,c2,c4small,c5small")
args = ap.parse_args()
hsaco = orc.REF950_HSACO if args.hsaco == "default" else orc.REF950_HSACO_NOCONTRACT
ref = orc.ReferenceGfx950(hsaco)

SPECS = {
    "c1": ("c1", dict(width=256, height=256), 16),
    "c2": ("c2", dict(width=1920, height=1080), 64),
    "c4small": ("c4", dict(width=480, height=270, n_spheres=2000), 16),   # brute force in the reference: keep it small
    "c5small": ("c5", dict(width=480, height=270, segments=24, rings=16), 16),
}
res = {"hsaco": os.path.basename(hsaco), "workloads": {}}
for name in args.workloads.split(","):
    wname, kw, spp = SPECS[name]
    try:
        wl = rt.workloads.get(wname, **kw)
    except TypeError:
        kw = {k: v for k, v in kw.items() if k in ("width", "height")}
        wl = rt.workloads.get(wname, **kw)
    W, H = wl.width, wl.height
    t = rt.RayTracer(W, H, scene=wl.scene, seed=rt.workloads.SEED)
    table = t.getRandomTable()

    def ours(first, count):
        t.clear()
        t.renderSamples(wl.camera, first, count)
        t.sync()
        return t.readLinear()[..., :3].astype(np.float64) * count   # mean → sum

    per_sample = []
    for k in range(4):
        acc, last = ref.render(wl.scene, wl.camera, table, W, H, k, 1, want_last=True)
        mine = ours(k, 1).astype(np.float32)
        same = (mine.view(np.uint32) == last[..., :3].view(np.uint32)).all(axis=2)
        per_sample.append(float(same.mean()))
    a = ref.render(wl.scene, wl.camera, table, W, H, 0, spp)[..., :3].astype(np.float64) / spp
    b = ours(0, spp) / spp
    b2 = ours(spp, spp) / spp           # an independent estimate from the same renderer: the noise yardstick
    d_ref, d_noise = np.abs(a - b), np.abs(b2 - b)
    rel = lambda x, y: float(abs(x.mean() - y.mean()) / max(y.mean(), 1e-12))
    res["workloads"][name] = {
        "frame": "%dx%d" % (W, H), "spp": spp,
        "bit_identical_pixel_fraction_samples_0_3": [round(x, 5) for x in per_sample],
        "mean_image": {
            "pixels_within_1e-4_rel": float((d_ref <= 1e-4 * np.maximum(np.abs(a), 1e-6)).mean()),
            "mean_abs_diff_vs_rocm_opencl_build": float(d_ref.mean()),
            "mean_abs_diff_between_two_own_sample_sets": float(d_noise.mean()),
            "frame_mean_rel_diff_vs_rocm_opencl_build": rel(a, b),
            "frame_mean_rel_diff_between_two_own_sample_sets": rel(b2, b),
        },
    }
    t.close()
txt = json.dumps(res, indent=1)
print(txt)
if args.out:
    open(args.out, "w").write(txt + "\n")
