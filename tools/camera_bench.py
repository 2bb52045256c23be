"""Per-sample camera blocks (rt_render_spp_cameras) against the routes that existed before it (DESIGN.md §5 "Per-sample
cameras").

For each scene:samples of --scenes, device events around the whole sequence of calls, warm, --rounds rounds with the
configurations alternating inside every round; median and (min .. max) per configuration:
    A        a host loop of n rt_render_spp(block_j, j, 1) — the only way to give every sample a camera without the call
    B        rt_render_spp(camera, 0, n) with RT_OPT_PREFIX_SHARING 0 — the from-the-camera kernel with fixed lanes
    C jit    rt_render_spp_cameras with n pixel-jittered blocks
    C same   rt_render_spp_cameras with n copies of the camera block
    fused    rt_render_spp(camera, 0, n) as shipped (prefix sharing): what anti-aliasing is priced against
--rmse SCENE: gamma-space RMSE of a 64-sample frame against a 4096-sample JITTERED truth, rendered with jitter and without
(samples 4096 .. 4159 both times, so neither frame shares a sample with the truth).

    python tools/camera_bench.py [--scenes c2:64,c3:256,c5:64] [--size 1920x1080] [--rounds 5] [--policy 2] [--rmse c2] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opencl_raytracing_amd as rt  # noqa: E402

f32 = np.float32


def jitter_blocks(block, n, first, width, height):
    """Camera.sampleBlocks' pixel jitter applied to a 12-float camera block: llc' = llc + (dx / w) hor + (dy / h) ver."""
    off = rt.Camera.sampleOffsets(n, first)
    out = np.tile(np.asarray(block, dtype=f32), (n, 1))
    llc, hor, ver = out[0, 3:6].copy(), out[0, 6:9].copy(), out[0, 9:12].copy()
    for j in range(n):
        v = llc + (off[j, 0] / f32(width)) * hor
        out[j, 3:6] = v + (off[j, 1] / f32(height)) * ver
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c2:64,c3:256,c5:64")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--policy", type=int, default=2)
    ap.add_argument("--rmse", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    w, h = (int(v) for v in a.size.split("x"))
    T = rt.RayTracer
    result = {"size": [w, h], "policy": a.policy, "rounds": a.rounds, "scenes": {}}
    for item in [s for s in a.scenes.split(",") if s]:
        name, n = item.split(":")
        n = int(n)
        wl = rt.workloads.get(name, width=w, height=h)
        t = T(w, h, scene=wl.scene, seed=rt.workloads.SEED)
        t.setArith(a.policy)
        stream = torch.cuda.Stream()
        t.setStream(stream.cuda_stream)
        jit, same = jitter_blocks(wl.camera, n, 0, w, h), np.tile(wl.camera, (n, 1))

        def loop():
            for j in range(n):
                t.renderSamples(jit[j], j, 1)

        def fixed():
            t.setOption(T.OPT_PREFIX_SHARING, 0)
            t.renderSamples(wl.camera, 0, n)

        configs = [("A", loop), ("B", fixed), ("C jit", lambda: t.renderSamplesCameras(jit, 0)),
                   ("C same", lambda: t.renderSamplesCameras(same, 0)), ("fused", lambda: t.renderSamples(wl.camera, 0, n))]
        ms = {k: [] for k, _ in configs}
        for r in range(a.rounds + 1):   # (round 0 warms every configuration up)
            for k, fn in configs:
                t.setOption(T.OPT_PREFIX_SHARING, 1)
                t.clear()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if r:
                    ms[k].append(e0.elapsed_time(e1))
        _, plan = t.lastCameraPlan()
        row = {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()}
        row["plan"] = plan
        result["scenes"][item] = row
        print("%s %dx%d, %d samples, policy %d, %d rounds (ms: median, min .. max); camera plan: family %d accel %d geom %d, %d pixels per wave" %
              (name, w, h, n, a.policy, a.rounds, plan["family"], plan["accel"], plan["geom"], plan["pixels_per_wave"]))
        for k, _ in configs:
            print("  %-7s %8.3f  (%.3f .. %.3f)" % (k, row[k]["median"], row[k]["min"], row[k]["max"]))
        print("  C jit / A %.3f, C jit / B %.3f, C jit / fused %.2f" % (row["C jit"]["median"] / row["A"]["median"],
              row["C jit"]["median"] / row["B"]["median"], row["C jit"]["median"] / row["fused"]["median"]), flush=True)
        t.close()
    if a.rmse:
        wl = rt.workloads.get(a.rmse, width=w, height=h)
        t = T(w, h, scene=wl.scene, seed=rt.workloads.SEED)
        t.setArith(a.policy)
        truth = t.renderFrameCameras(jitter_blocks(wl.camera, 4096, 0, w, h))[..., :3].astype(np.float64)
        t.clear()
        t.renderSamplesCameras(jitter_blocks(wl.camera, 64, 4096, w, h), 4096)
        t.resolve()
        with_jitter = t.transferImage()
        t.clear()
        t.renderSamples(wl.camera, 4096, 64)
        t.resolve()
        without = t.transferImage()
        t.close()
        rmse = lambda img: float(np.sqrt(((img[..., :3].astype(np.float64) - truth) ** 2).mean()))
        result["rmse"] = dict(scene=a.rmse, truth_spp=4096, spp=64, jittered=rmse(with_jitter), unjittered=rmse(without))
        print("%s %dx%d: gamma RMSE of 64 samples against the 4096-sample jittered truth: jittered %.5f, unjittered %.5f" %
              (a.rmse, w, h, result["rmse"]["jittered"], result["rmse"]["unjittered"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
