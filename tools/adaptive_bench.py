"""Adaptive sampling against fixed sample counts at equal quality (DESIGN.md "Adaptive sampling").

For each scene: a fixed 4096-spp frame is the ground truth; fixed 256 / 1024 spp frames and adaptive frames
(max_spp 1024, batch 64, 8x8 blocks, a few thresholds) are timed with device events around the whole call on the
tracer's stream, and their RMSE against the ground truth is measured in gamma space (the displayed image).

    python tools/adaptive_bench.py [--scenes c2,c5] [--size 1920x1080] [--thresholds 0.05,0.02,0.01] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opencl_raytracing_amd as rt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c2,c5")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--thresholds", default="0.05,0.02,0.01")
    ap.add_argument("--truth-spp", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--min-spp", type=int, default=128)
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    w, h = (int(v) for v in a.size.split("x"))
    rows = []
    for name in a.scenes.split(","):
        wl = rt.workloads.get(name, width=w, height=h)
        t = rt.RayTracer(w, h, scene=wl.scene, seed=rt.workloads.SEED)
        stream = torch.cuda.Stream()
        t.setStream(stream.cuda_stream)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            r = fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), r

        t.renderFrameOnDevice(wl.camera, 64)   # warm-up (code objects, LDS sizing, buffers)
        t.renderAdaptive(wl.camera, 0.05, batch=a.batch, min_spp=a.min_spp, max_spp=a.max_spp)
        _, truth = timed(lambda: t.renderFrame(wl.camera, a.truth_spp))
        truth = truth[..., :3].astype(np.float64)

        def rmse(img):
            return float(np.sqrt(((img[..., :3].astype(np.float64) - truth) ** 2).mean()))

        for spp in (256, 1024):
            ms, _ = timed(lambda: t.renderFrameOnDevice(wl.camera, spp))
            rows.append(dict(scene=name, mode="fixed", spp=spp, ms=ms, mean_spp=float(spp), rounds=1,
                             rmse=rmse(t.transferImage())))
        for thr in (float(v) for v in a.thresholds.split(",")):
            ms, st = timed(lambda: t.renderAdaptive(wl.camera, thr, batch=a.batch, min_spp=a.min_spp, max_spp=a.max_spp))
            rows.append(dict(scene=name, mode="adaptive", threshold=thr, ms=ms,
                             mean_spp=st["pixel_samples"] / float(w * h), rounds=st["rounds"],
                             blocks_at_max=st["blocks_at_max"], blocks=st["blocks"], rmse=rmse(t.transferImage())))
        t.setStream(None)
        t.close()
    print("| scene | run | ms | mean spp | rounds | RMSE (gamma) |")
    print("|---|---|---:|---:|---:|---:|")
    for r in rows:
        run = "fixed %d" % r["spp"] if r["mode"] == "fixed" else "adaptive thr %g" % r["threshold"]
        print("| %s | %s | %.1f | %.1f | %d | %.5f |" % (r["scene"], run, r["ms"], r["mean_spp"], r["rounds"], r["rmse"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
