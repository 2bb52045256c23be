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

--sets K: ray sets (rt_render_ray_sets; DESIGN.md §5 "Ray sets") instead — the pinhole's own rays through --spp jittered
camera blocks (Camera.sampleBlocks, pixel jitter only; directions formed on the device in float32, their last bits do not
matter to a timing), everything into the accumulator:
    loop     (A) what a caller writes without ray sets: --spp single-sample rt_render_rays calls over --spp sample-major
             batches, batch j = every pixel's ray through block j
    sets     (B) one rt_render_ray_sets call, set_size K (block j mod K at sample j)
    sets16   (B') the same call with set_size 16 (only if K > 16)
    rays     (C) rt_render_rays with the unjittered rays: what anti-aliasing costs
    cameras  (D) rt_render_spp_cameras with the jittered blocks
On a checkout without rt_render_ray_sets `loop`, `rays` and `cameras` are measured (the parent's side).

    python tools/rays_bench.py [--scenes c2,c5] [--size 1920x1080] [--spp 64] [--rounds 5] [--policy 2] [--pano c2] [--pano-size 2048x1024] [--json out.json]
    python tools/rays_bench.py --sets 64 [--scenes c2,c5] [--size 1920x1080] [--spp 64] [--rounds 5] [--policy 2] [--json out.json]
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


def device_rays(block, w, h):
    """the pinhole block's primary rays as an (w * h, 8) float32 device tensor of rt_ray bits, ids = pixel coordinates"""
    import torch
    cam = torch.as_tensor(np.asarray(block, np.float32), device="cuda")
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    s, t = (xs.reshape(-1).float() / w)[:, None], (ys.reshape(-1).float() / h)[:, None]
    d = cam[3:6][None, :] + s * cam[6:9][None, :] + t * cam[9:12][None, :]
    d = d / d.norm(dim=1, keepdim=True)
    out = torch.empty((w * h, 8), dtype=torch.float32, device="cuda")
    out[:, 0:3], out[:, 4:7] = cam[0:3][None, :], d
    out[:, 3] = xs.reshape(-1).int().view(torch.float32)
    out[:, 7] = ys.reshape(-1).int().view(torch.float32)
    return out


def bench_sets(a, result):
    import torch
    T = rt.RayTracer
    have_sets = hasattr(T, "renderRaySets")
    w, h = (int(v) for v in a.size.split("x"))
    n, k = a.spp, a.sets
    result.update(have_sets=have_sets, set_size=k)
    for name in [s for s in a.scenes.split(",") if s]:
        wl = rt.workloads.get(name, width=w, height=h)
        t = T(w, h, scene=wl.scene, seed=rt.workloads.SEED)
        t.setArith(a.policy)
        stream = torch.cuda.Stream()
        t.setStream(stream.cuda_stream)
        pos, yaw, pitch = a.camera[name]
        cam = rt.Camera(60, np.float32(w) / np.float32(h), pos, yaw, pitch)
        assert np.array_equal(cam.transferData(), wl.camera), "the workload's camera"
        blocks = cam.sampleBlocks(n, width=w, height=h)
        batches = [device_rays(blocks[j % k], w, h) for j in range(n)]          # sample-major: batch j for sample j
        central = device_rays(wl.camera, w, h)
        torch.cuda.synchronize()

        def loop():
            for j in range(n):
                t.renderRays(batches[j], j, 1)
        configs = [("loop", loop), ("rays", lambda: t.renderRays(central, 0, n)), ("cameras", lambda: t.renderSamplesCameras(blocks, 0))]
        if have_sets:
            sets = torch.stack(batches[:k], dim=1).contiguous()                  # (w * h, k, 8): ray-major
            configs.insert(1, ("sets", lambda: t.renderRaySets(sets, k, 0, n)))
            if k > 16:
                sets16 = sets[:, :16].contiguous()
                configs.insert(2, ("sets16", lambda: t.renderRaySets(sets16, 16, 0, n)))
            torch.cuda.synchronize()
        row = stats(timed(t, stream, configs, a.rounds))
        if have_sets:
            row["plan"] = t.lastRayPlan()[1]
        result["scenes"][name] = row
        print("%s %dx%d, %d samples, sets of %d, policy %d, %d rounds (ms: median, min .. max)" % (name, w, h, n, k, a.policy, a.rounds))
        for c, _ in configs:
            print("  %-8s %8.3f  (%.3f .. %.3f)" % (c, row[c]["median"], row[c]["min"], row[c]["max"]))
        if have_sets:
            print("  sets / loop %.4f, sets / rays %.4f, sets / cameras %.4f" % tuple(row["sets"]["median"] / row[c]["median"]
                                                                                   for c in ("loop", "rays", "cameras")), flush=True)
        t.close()
        del batches, central


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
    ap.add_argument("--sets", type=int, default=0)
    a = ap.parse_args()
    if a.sets:
        # the workloads' cameras (workloads.py): a Camera object makes the jittered blocks
        a.camera = {"c1": ((0, 0, 0), 0.0, 0.0), "c2": ((-8, -1, -8), 45.0, 0.0), "c3": ((-6, -2, -7), 40.0, 8.0),
                    "c4": ((-8, -1, -8), 45.0, 0.0), "c5": ((-7, 0, -7), 45.0, 8.0), "all_kinds": ((-8, -1, -8), 45.0, 0.0)}
        w, h = (int(v) for v in a.size.split("x"))
        result = {"size": [w, h], "spp": a.spp, "policy": a.policy, "rounds": a.rounds, "scenes": {}}
        bench_sets(a, result)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(result, f, indent=1)
        return
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
