"""The ray queries (rt_occluded_rays, rt_intersect_rays) against the only way to ask the occlusion question without them:
rt_render_features_rays on the same records (DESIGN.md §5 "Ray queries").

For each scene of --scenes at --size, device events around each call, warm, --rounds rounds with the configurations
alternating inside every round; median and (min .. max) per configuration.  Two batches of W x H records:
    primary  the camera's own primary rays
    hemi     one cosine-weighted hemisphere ray from every pixel's first hit, its origin on the surface (the primary ray
             again where the pixel missed)
and per batch
    features   rt_render_features_rays (first hits; 80 bytes per ray into the context's records) — what a caller has to run
               to learn whether anything lies in front of a bound
    occ_inf    rt_occluded_rays, t_max = +inf (any hit)
    occ_1      rt_occluded_rays, t_max = 1.0
    intersect  rt_intersect_rays into a buffer of the caller's, for orientation
then `ao16`: one rt_occluded_rays call with set_size 16 — 16 hemisphere rays per pixel, the capability's own figure.
The hemisphere rays are made on the device with torch's generator (a timing needs no particular bits).  On a checkout
without the ray queries only `features` is measured (the parent's side of the comparison).

    python tools/queries_bench.py [--scenes c2,c4,c5] [--size 1920x1080] [--rounds 5] [--policy 2] [--ao 16] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opencl_raytracing_amd as rt  # noqa: E402


def timed(stream, configs, rounds):
    """→ {name: [ms per round]}; round 0 warms every configuration up"""
    import torch
    ms = {k: [] for k, _ in configs}
    for r in range(rounds + 1):
        for k, fn in configs:
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


def hemisphere_on_device(pos, normal, incoming, k, gen):
    """(n, 3) hit points, normals and incoming directions on the device → (n, k, 8) rt_ray bits: cosine-weighted
    directions about the normal turned to the side the ray came from"""
    import torch
    n = pos.shape[0]
    nr = normal / normal.norm(dim=1, keepdim=True).clamp_min(1e-30)
    nr = torch.where((nr * incoming).sum(1, keepdim=True) > 0, -nr, nr)
    axis = torch.nn.functional.one_hot(nr.abs().argmin(dim=1), 3).to(nr.dtype)
    tan = torch.linalg.cross(nr, axis)
    tan = tan / tan.norm(dim=1, keepdim=True).clamp_min(1e-30)
    bit = torch.linalg.cross(nr, tan)
    u = torch.rand((n, k, 2), device=pos.device, generator=gen)
    rad, phi = u[..., 0].sqrt(), 2 * np.pi * u[..., 1]
    d = ((rad * phi.cos())[..., None] * tan[:, None, :] + (rad * phi.sin())[..., None] * bit[:, None, :] +
         (1 - u[..., 0]).clamp_min(1e-7).sqrt()[..., None] * nr[:, None, :])
    d = d / d.norm(dim=-1, keepdim=True)
    out = torch.zeros((n, k, 8), dtype=torch.float32, device=pos.device)
    out[..., 0:3], out[..., 4:7] = pos[:, None, :], d
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c2,c4,c5")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--policy", type=int, default=2)
    ap.add_argument("--ao", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    T = rt.RayTracer
    have = hasattr(T, "occludedRays")
    w, h = (int(v) for v in a.size.split("x"))
    result = {"size": [w, h], "policy": a.policy, "rounds": a.rounds, "have_queries": have, "scenes": {}}
    for name in [s for s in a.scenes.split(",") if s]:
        wl = rt.workloads.get(name, width=w, height=h)
        t = T(w, h, scene=wl.scene, seed=rt.workloads.SEED)
        t.setArith(a.policy)
        stream = torch.cuda.Stream()
        t.setStream(stream.cuda_stream)
        t.renderFeatures(wl.camera)
        rec = t.featureRecords().reshape(-1)
        ys, xs = np.mgrid[0:h, 0:w]
        prim = rt.rays.pack_rays(wl.camera[0:3], rec["dir"], ids=np.stack([xs.ravel(), ys.ravel()], axis=1))
        primary = torch.from_numpy(rt.rays.as_floats(prim).copy()).cuda()
        hit = torch.from_numpy((rec["flags"] & 1) != 0).cuda()
        pos, nrm, inc = (torch.from_numpy(np.ascontiguousarray(rec[f])).cuda() for f in ("pos", "normal", "dir"))
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        nrm = torch.where(hit[:, None], nrm, torch.tensor([0.0, 1.0, 0.0], device="cuda")[None, :])
        hemi = torch.where(hit[:, None], hemisphere_on_device(pos, nrm, inc, 1, gen)[:, 0, :], primary).contiguous()
        row = {"hit_share": float(hit.float().mean())}
        out_n = torch.empty((w * h,), dtype=torch.int32, device="cuda")
        out_f = torch.empty((w * h, 20), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for label, batch in (("primary", primary), ("hemi", hemi)):
            configs = [("features", lambda b=batch: t.renderFeaturesRays(b))]
            if have:
                configs += [("occ_inf", lambda b=batch: t.occludedRays(b, out=out_n)),
                            ("occ_1", lambda b=batch: t.occludedRays(b, t_max=1.0, out=out_n)),
                            ("intersect", lambda b=batch: t.intersectRays(b, out=out_f))]
            row[label] = stats(timed(stream, configs, a.rounds))
            if have:
                t.occludedRays(batch, out=out_n)
                t.sync()
                row[label]["occluded_share"] = float(out_n.float().mean())
        if have and a.ao:
            sets = hemisphere_on_device(pos, nrm, inc, a.ao, gen)
            sets = torch.where(hit[:, None, None], sets, primary[:, None, :].expand(-1, a.ao, -1)).contiguous()
            torch.cuda.synchronize()
            row["ao"] = stats(timed(stream, [("ao%d" % a.ao, lambda: t.occludedRays(sets, a.ao, out=out_n))], a.rounds))
            t.sync()
            row["ao"]["mean_open"] = float(1.0 - out_n.float().mean() / a.ao)
            del sets
        row["walk_overflow"] = t.walkOverflow()
        result["scenes"][name] = row
        print("%s %dx%d, policy %d, %d rounds (ms: median, min .. max); %.1f %% of the primary rays hit" %
              (name, w, h, a.policy, a.rounds, 100 * row["hit_share"]))
        for label in ("primary", "hemi"):
            for c, v in row[label].items():
                if isinstance(v, dict):
                    print("  %-8s %-10s %8.3f  (%.3f .. %.3f)" % (label, c, v["median"], v["min"], v["max"]))
            if have:
                f = row[label]["features"]["median"]
                print("  %-8s occ_inf / features %.3f, occ_1 / features %.3f; %.1f %% occluded at +inf" %
                      (label, row[label]["occ_inf"]["median"] / f, row[label]["occ_1"]["median"] / f, 100 * row[label]["occluded_share"]))
        if "ao" in row:
            v = row["ao"]["ao%d" % a.ao]
            print("  ao%-6d %8.3f  (%.3f .. %.3f): %.0f Mrays/s, mean openness %.3f" %
                  (a.ao, v["median"], v["min"], v["max"], w * h * a.ao / v["median"] / 1e3, row["ao"]["mean_open"]), flush=True)
        t.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
