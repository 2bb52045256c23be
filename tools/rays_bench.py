"""Caller-supplied rays (rt_render_rays) against the from-the-camera routes (DESIGN.md §5 "Caller-supplied rays").

For each scene of --scenes, at --size and --spp, device events around each call, warm, --rounds rounds with the
configurations alternating inside every round; median and (min .. max) per configuration:
    rays     rt_render_rays on the camera's own primary rays (a device tensor; directions = renderFeatures' `dir`), into the
             accumulator
    rays8x8  the same rays sorted into the camera kernels' pixel order (8 x 8 tiles), into an external buffer
    cameras  rt_render_spp_cameras with --spp copies of the camera block: the same from-the-camera work plus a block gather
             and a normalize per refill
    fused    rt_render_spp as shipped (prefix sharing), for orientation
--pano SCENE: an equirectangular --pano-size frame of SCENE at --spp through rt_render_rays — the new capability's own figure.
On a checkout without rt_render_rays only `cameras` and `fused` are measured (the parent's side of the comparison).

    python tools/rays_bench.py [--scenes c2,c5] [--size 1920x1080] [--spp 64] [--rounds 5] [--policy 2] [--pano c2] [--pano-size 2048x1024] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opencl_raytracing_amd as rt  # noqa: E402


def timed(t, stream, configs, rounds):
    """→ {name: [ms per round]}; round 0 warms every configuration up"""
    import torch
    ms = {k: [] for k, _ in configs}
    for r in range(rounds + 1):
        for k, fn in configs:
            t.clear()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r:
                ms[k].append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    return {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c2,c5")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--policy", type=int, default=2)
    ap.add_argument("--pano", default="c2")
    ap.add_argument("--pano-size", default="2048x1024")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    T = rt.RayTracer
    have_rays = hasattr(T, "renderRays")
    w, h = (int(v) for v in a.size.split("x"))
    n = a.spp
    result = {"size": [w, h], "spp": n, "policy": a.policy, "rounds": a.rounds, "have_rays": have_rays, "scenes": {}}
    for name in [s for s in a.scenes.split(",") if s]:
        wl = rt.workloads.get(name, width=w, height=h)
        t = T(w, h, scene=wl.scene, seed=rt.workloads.SEED)
        t.setArith(a.policy)
        stream = torch.cuda.Stream()
        t.setStream(stream.cuda_stream)
        same = np.tile(wl.camera, (n, 1))
        configs = [("cameras", lambda: t.renderSamplesCameras(same, 0)), ("fused", lambda: t.renderSamples(wl.camera, 0, n))]
        if have_rays:
            t.renderFeatures(wl.camera)
            ys, xs = np.mgrid[0:h, 0:w]
            batch = rt.rays.pack_rays(wl.camera[0:3], t.featureRecords()["dir"].reshape(-1, 3),
                                      ids=np.stack([xs.ravel(), ys.ravel()], axis=1))
            d = torch.from_numpy(rt.rays.as_floats(batch).copy()).cuda()
            torch.cuda.synchronize()
            configs.insert(0, ("rays", lambda: t.renderRays(d, 0, n)))
            # the same rays in the order the camera kernels take their pixels (8 x 8 tiles, row-major inside a tile), into an
            # external buffer: what the order of a batch is worth where the paths read memory (C5's mesh walk)
            tiles = (ys.ravel() // 8 * ((w + 7) // 8) + xs.ravel() // 8) * 64 + (ys.ravel() % 8) * 8 + xs.ravel() % 8
            dt = torch.from_numpy(rt.rays.as_floats(batch[np.argsort(tiles, kind="stable")]).copy()).cuda()
            out = torch.zeros((w * h, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            configs.insert(1, ("rays8x8", lambda: t.renderRays(dt, 0, n, out=out)))
        row = stats(timed(t, stream, configs, a.rounds))
        if have_rays:
            row["plan"] = t.lastRayPlan()[1]
        result["scenes"][name] = row
        print("%s %dx%d, %d samples, policy %d, %d rounds (ms: median, min .. max)" % (name, w, h, n, a.policy, a.rounds))
        for k, _ in configs:
            print("  %-8s %8.3f  (%.3f .. %.3f)" % (k, row[k]["median"], row[k]["min"], row[k]["max"]))
        if have_rays:
            print("  rays / cameras %.4f, rays8x8 / cameras %.4f" % (row["rays"]["median"] / row["cameras"]["median"],
                                                                   row["rays8x8"]["median"] / row["cameras"]["median"]), flush=True)
        t.close()
    if a.pano and have_rays:
        pw, ph = (int(v) for v in a.pano_size.split("x"))
        wl = rt.workloads.get(a.pano, width=pw, height=ph)
        t = T(pw, ph, scene=wl.scene, seed=rt.workloads.SEED)
        t.setArith(a.policy)
        stream = torch.cuda.Stream()
        t.setStream(stream.cuda_stream)
        d = torch.from_numpy(rt.rays.as_floats(rt.rays.equirect_rays(wl.camera[0:3], pw, ph, yaw=45.0)).copy()).cuda()
        torch.cuda.synchronize()
        row = stats(timed(t, stream, [("equirect", lambda: t.renderRays(d, 0, n))], a.rounds))
        t.resolve()
        img = t.transferImage()
        row["finite"] = bool(np.isfinite(img).all())
        row["mean"] = float(img[..., :3].mean())
        result["pano"] = dict(scene=a.pano, size=[pw, ph], **row)
        print("%s equirect %dx%d, %d samples: %.3f ms (%.3f .. %.3f), %.1f Msamples/s; finite %s, mean %.4f" %
              (a.pano, pw, ph, n, row["equirect"]["median"], row["equirect"]["min"], row["equirect"]["max"],
               pw * ph * n / row["equirect"]["median"] / 1e3, row["finite"], row["mean"]), flush=True)
        t.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
