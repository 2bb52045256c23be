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

With the hemisphere queries (rt_occluded_hemispheres, DESIGN.md §5 "Hemisphere queries") --ao K adds, over the same W x H
first-hit records and alternating inside every round:
    fused        occludedHemispheres: the K rays of every record made in registers, counts only
    spawn        spawnHemispheres alone: the same rays written to memory, no search
    occ_dumped   rt_occluded_rays with set_size K over the very rays `spawn` wrote — pt_occluded on identical work
    spawn_occ    spawn, then that query: what a caller pays who wants the rays as well
and, by the host's clock over --host-rounds rounds (default --rounds; seconds each at 1080p x 16, so no warm-up round), `host_path`: the first-hit
records as they lie on the host -> rays.hemisphere_sets -> upload -> rt_occluded_rays -> sync, which is what rt_cli --ao K and
every user of hemisphere_sets ran before.  The fused counts are checked against occ_dumped's on the way.

With the hemisphere gather (rt_render_hemispheres, DESIGN.md §5 "Hemisphere gather") --gather K is a mode of its own:
nothing of the above runs, and over the same W x H first-hit records, K samples per record (every direction once),
alternating inside every round:
    fused        renderHemispheres into an external target: the rays made at the sample queue's refill, none stored
    spawn_sets   spawnHemispheres, then renderRaySets over the rays it wrote: the two calls the fused one replaces
    sets_only    renderRaySets alone over those rays, for orientation
with the bytes the two-call sequence moves through memory for its rays (32 B x W x H x K written, then read once per
sample).  The two targets are compared on the way: equal bytes on the records that have a hemisphere.

    python tools/queries_bench.py [--scenes c2,c4,c5] [--size 1920x1080] [--rounds 5] [--policy 2] [--ao 16] [--json out.json]
    python tools/queries_bench.py --gather 64 [--scenes c2,c5] [--size 1920x1080] [--rounds 5] [--policy 2]
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


def hemisphere_rows(t, stream, rec, k, rounds, host_rounds):
    """The rows of rt_occluded_hemispheres over the (n,) FEATURE records `rec` → {configuration: statistics}"""
    import time
    import torch
    n = len(rec)
    feats = torch.from_numpy(np.ascontiguousarray(rec).view(np.float32).reshape(n, 20).copy()).cuda()
    counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    counts2 = torch.empty((n,), dtype=torch.int32, device="cuda")
    dumped = torch.empty((n * k, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    kw = dict(k=k, seed=7, offset=0.0, face_forward=True)
    t.spawnHemispheres(feats, out=dumped, **kw)
    t.sync()

    def spawn_occ():
        t.spawnHemispheres(feats, out=dumped, **kw)
        t.occludedRays(dumped, k, out=counts2)

    configs = [("fused", lambda: t.occludedHemispheres(feats, out=counts, **kw)),
               ("occ_dumped", lambda: t.occludedRays(dumped, k, out=counts2)),
               ("spawn", lambda: t.spawnHemispheres(feats, out=dumped, **kw)),
               ("spawn_occ", spawn_occ)]
    row = stats(timed(stream, configs, rounds))
    t.sync()
    valid = torch.from_numpy((rec["flags"] & 1) != 0).cuda()
    row["counts_equal"] = bool((counts[valid] == counts2[valid]).all()) and not bool(counts[~valid].any())
    row["mean_open"] = float(1.0 - counts.float().mean() / k)
    del dumped
    if host_rounds > 0:
        hit = (rec["flags"] & 1) != 0
        ms = []
        for r in range(host_rounds):
            t.sync()
            t0 = time.perf_counter()
            normal = rec["normal"][hit]
            facing = (normal * rec["dir"][hit]).sum(1) > 0
            sets = rt.rays.hemisphere_sets(rec["pos"][hit], np.where(facing[:, None], -normal, normal), k, 7)
            d = torch.from_numpy(rt.rays.as_floats(sets).reshape(-1, 8)).cuda()
            out = t.occludedRays(d, k)
            t.sync()
            ms.append((time.perf_counter() - t0) * 1e3)
            del sets, d, out
        row.update(stats({"host_path": ms}))
    return row


def gather_rows(t, stream, rec, k, rounds):
    """The rows of rt_render_hemispheres over the (n,) FEATURE records `rec`, k samples per record → {configuration: statistics}"""
    import torch
    n = len(rec)
    feats = torch.from_numpy(np.ascontiguousarray(rec).view(np.float32).reshape(n, 20).copy()).cuda()
    dumped = torch.empty((n * k, 8), dtype=torch.float32, device="cuda")
    fused, twin = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    kw = dict(k=k, seed=7, offset=1e-3, face_forward=True)

    def spawn_sets():
        t.spawnHemispheres(feats, out=dumped, **kw)
        t.renderRaySets(dumped, k, 0, k, out=twin)

    # the comparison first, on fresh targets: one call each
    t.renderHemispheres(feats, first_sample=0, n_samples=k, out=fused, **kw)
    spawn_sets()
    t.sync()
    valid = torch.from_numpy(((rec["flags"] & 1) != 0) & np.isfinite(rec["normal"]).all(1) & (rec["normal"] != 0).any(1)).cuda()
    row = {"targets_equal": bool((fused[valid].view(torch.int32) == twin[valid].view(torch.int32)).all()) and not bool(fused[~valid].any()),
           "valid_share": float(valid.float().mean()),
           "mean_radiance": float((fused[valid][:, :3].sum(1) / (3.0 * fused[valid][:, 3])).mean()) if bool(valid.any()) else 0.0,
           "ray_bytes_written": 32 * n * k, "ray_bytes_read": 32 * n * k}
    configs = [("fused", lambda: t.renderHemispheres(feats, first_sample=0, n_samples=k, out=fused, **kw)),
               ("spawn_sets", spawn_sets),
               ("sets_only", lambda: t.renderRaySets(dumped, k, 0, k, out=twin))]
    row.update(stats(timed(stream, configs, rounds)))
    t.sync()
    return row


def gather_mode(a, w, h):
    """--gather K: the fused gather against the two calls it replaces, per scene"""
    import torch
    result = {"size": [w, h], "policy": a.policy, "rounds": a.rounds, "gather": a.gather, "scenes": {}}
    for name in [s for s in a.scenes.split(",") if s]:
        wl = rt.workloads.get(name, width=w, height=h)
        t = rt.RayTracer(w, h, scene=wl.scene, seed=rt.workloads.SEED)
        t.setArith(a.policy)
        stream = torch.cuda.Stream()
        t.setStream(stream.cuda_stream)
        t.renderFeatures(wl.camera)
        r = gather_rows(t, stream, t.featureRecords().reshape(-1), a.gather, a.rounds)
        r["walk_overflow"] = t.walkOverflow()
        result["scenes"][name] = r
        print("%s %dx%d, policy %d, %d rounds (ms: median, min .. max); gather of %d samples along %d directions from %.1f %% of the pixels" %
              (name, w, h, a.policy, a.rounds, a.gather, a.gather, 100 * r["valid_share"]))
        for c in ("fused", "spawn_sets", "sets_only"):
            print("  gather%-4d %-10s %9.3f  (%.3f .. %.3f)" % (a.gather, c, r[c]["median"], r[c]["min"], r[c]["max"]))
        print("  spawn_sets / fused %.3f, sets_only / fused %.3f; the sequence writes %.2f GB of rays and reads %.2f GB; targets equal: %s" %
              (r["spawn_sets"]["median"] / r["fused"]["median"], r["sets_only"]["median"] / r["fused"]["median"],
               r["ray_bytes_written"] / 1e9, r["ray_bytes_read"] / 1e9, r["targets_equal"]), flush=True)
        t.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c2,c4,c5")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--policy", type=int, default=2)
    ap.add_argument("--ao", type=int, default=16)
    ap.add_argument("--host-rounds", type=int, default=None)
    ap.add_argument("--gather", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    T = rt.RayTracer
    have = hasattr(T, "occludedRays")
    w, h = (int(v) for v in a.size.split("x"))
    if a.gather:
        return gather_mode(a, w, h)
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
        if hasattr(T, "occludedHemispheres") and a.ao:
            row["hemi_ao"] = hemisphere_rows(t, stream, rec, a.ao, a.rounds, a.rounds if a.host_rounds is None else a.host_rounds)
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
        if "hemi_ao" in row:
            r = row["hemi_ao"]
            for c in ("fused", "spawn", "occ_dumped", "spawn_occ", "host_path"):
                if c in r:
                    print("  ao%-3d %-10s %9.3f  (%.3f .. %.3f)" % (a.ao, c, r[c]["median"], r[c]["min"], r[c]["max"]))
            print("  fused / occ_dumped %.3f, spawn_occ / fused %.2f%s; counts equal: %s" %
                  (r["fused"]["median"] / r["occ_dumped"]["median"], r["spawn_occ"]["median"] / r["fused"]["median"],
                   ", host_path / fused %.0f" % (r["host_path"]["median"] / r["fused"]["median"]) if "host_path" in r else "",
                   r["counts_equal"]), flush=True)
        t.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
