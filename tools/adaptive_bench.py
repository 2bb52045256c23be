"""Adaptive sampling against fixed sample counts at equal quality (DESIGN.md "Adaptive sampling").

For each scene: a fixed 4096-spp frame is the ground truth; fixed 256 / 1024 spp frames and adaptive frames
(max_spp 1024, batch 64, 8x8 blocks, a few thresholds) are timed with device events around the whole call on the
tracer's stream, and their RMSE against the ground truth is measured in gamma space (the displayed image).

    python tools/adaptive_bench.py [--scenes c2,c5] [--size 1920x1080] [--thresholds 0.05,0.02,0.01] [--json out.json]

--cameras runs the experiment on ANTI-ALIASED frames (DESIGN.md "Adaptive sampling through per-sample cameras"): every
sample has a camera block of its own (the workload's camera with Camera.sampleOffsets' pixel jitter), the ground truth is
a jittered --truth-spp frame (renderFrameCameras), the fixed runs are renderSamplesCameras frames of 256 and 1024 samples
and the adaptive runs are renderAdaptiveCameras frames — the thresholds and threshold 0, the price of the rounds
themselves.  The configurations alternate inside each of --rounds rounds (default 5) and the times are reported as
median (min .. max).  Per adaptive run the record also holds every round's launch time (the device events round each
round's camera launch, kernelMsHistory) beside the share of the decision blocks that round traced.

--rule variance compares the two stopping rules (DESIGN.md "Variance-driven stopping rule") at EQUAL pixel-sample budgets:
for each --thresholds value the Dammertz frame (renderAdaptive) is rendered, then the variance rule's threshold is found by
bisection so that renderAdaptiveVariance spends the same pixel samples within 2 %, and for both the gamma RMSE against the
--truth-spp frame, the pixel samples, the rounds and the whole call's time (median (min .. max) of --runs) are reported;
the sample moments are on for both, batch / min_spp / max_spp are shared.  It ends with the cameras form at threshold 0
(every block in every round, --cameras-spp jittered samples): renderAdaptiveCameras without and with moments and
renderAdaptiveVarianceCameras — what the fixed-lane camera kernel the moments ask for costs.
--rays [--sets K] runs the experiment on a frame of CALLER-SUPPLIED rays (DESIGN.md "Adaptive sampling for caller-supplied
rays"): an equirectangular panorama about the workload's camera position (rays.equirect_rays), with --sets K anti-aliased by K
jittered records per pixel (rays.ray_sets over Camera.sampleOffsets(K); 1080p x 16 records are 1.06 GB).  The ground truth is
a fixed --truth-spp renderRays / renderRaySets frame, the fixed runs are such frames of 256 and 1024 samples, and the adaptive
runs are renderAdaptiveRays and — with the sample moments on, whose ray launches run the fixed-lane kernels —
renderAdaptiveVarianceRays frames at the --thresholds; the configurations alternate inside each of --rounds rounds.
The merge kernels' own time per round comes from a kernel trace:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/adaptive_bench.py --rule variance --merge-rounds 20
renders 20 two-round threshold-0 frames per rule and scene (every block active in round 0 and in round 1), and
    python tools/adaptive_bench.py --merge-trace DIR/.../*_kernel_trace.csv
prints per merge kernel and round the median (min .. max) of its dispatches.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opencl_raytracing_amd as rt  # noqa: E402


def jitter_blocks(block, n, width, height):
    """Camera.sampleBlocks' pixel jitter applied to a 12-float camera block: llc' = llc + (dx / w) hor + (dy / h) ver."""
    f32 = np.float32
    off = rt.Camera.sampleOffsets(n, 0)
    out = np.tile(np.asarray(block, dtype=f32), (n, 1))
    llc, hor, ver = out[0, 3:6].copy(), out[0, 6:9].copy(), out[0, 9:12].copy()
    for j in range(n):
        v = llc + (off[j, 0] / f32(width)) * hor
        out[j, 3:6] = v + (off[j, 1] / f32(height)) * ver
    return out


def spread(v):
    v = sorted(v)
    return "%.1f (%.1f .. %.1f)" % (v[len(v) // 2], v[0], v[-1])


def merge_trace_main(path):
    """--merge-trace: per merge kernel and round (the dispatches of a two-round frame alternate) its time in a rocprofv3 trace."""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "pt_adaptive_merge" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        name = "pt_adaptive_merge_variance" if "pt_adaptive_merge_variance" in r["Kernel_Name"] else "pt_adaptive_merge"
        grid = r.get("Grid_Size_X", r.get("Grid_Size", "?"))
        by.setdefault((name, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("| kernel | grid (work-items) | round | dispatches | us: median (min .. max) |")
    print("|---|---:|---:|---:|---:|")
    for (name, grid), us in sorted(by.items()):
        for k in (0, 1):
            v = sorted(us[k::2])
            if v:
                print("| %s | %s | %d | %d | %.1f (%.1f .. %.1f) |" % (name, grid, k, len(v), v[len(v) // 2], v[0], v[-1]))


def rule_main(a):
    """--rule variance: the two stopping rules at equal pixel-sample budgets."""
    import torch
    w, h = (int(v) for v in a.size.split("x"))
    rows, cam_rows = [], []
    for name in a.scenes.split(","):
        wl = rt.workloads.get(name, width=w, height=h)
        t = rt.RayTracer(w, h, scene=wl.scene, seed=rt.workloads.SEED)
        t.setArith(2 if a.policy is None else a.policy)
        stream = torch.cuda.Stream()
        t.setStream(stream.cuda_stream)
        kw = dict(batch=a.batch, min_spp=a.min_spp, max_spp=a.max_spp)
        calls = {"dammertz": lambda thr: t.renderAdaptive(wl.camera, thr, **kw),
                 "variance": lambda thr: t.renderAdaptiveVariance(wl.camera, thr, **kw)}

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            r = fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), r

        t.setOption(t.OPT_MOMENTS, 1)
        t.renderFrameOnDevice(wl.camera, 64)   # warm-up (code objects, LDS sizing, buffers)
        if a.merge_rounds:
            two = dict(batch=a.batch, min_spp=2 * a.batch, max_spp=2 * a.batch)
            for _ in range(a.merge_rounds):
                t.renderAdaptive(wl.camera, 0.0, **two)
                t.renderAdaptiveVariance(wl.camera, 0.0, **two)
            t.setStream(None)
            t.close()
            continue
        for c in calls.values():
            c(0.05)
        truth = t.renderFrame(wl.camera, a.truth_spp)[..., :3].astype(np.float64)

        def measure(rule, thr, against=None):
            ms, st = [], None
            for _ in range(a.runs):
                m, st = timed(lambda: calls[rule](thr))
                ms.append(m)
            img = t.transferImage()[..., :3].astype(np.float64)
            rec = dict(scene=name, rule=rule, threshold=thr, ms=ms, pixel_samples=st["pixel_samples"],
                       mean_spp=st["pixel_samples"] / float(w * h), rounds=st["rounds"], blocks_at_max=st["blocks_at_max"],
                       blocks=st["blocks"], rmse=float(np.sqrt(((img - truth) ** 2).mean())))
            if against:
                rec["budget_ratio"] = st["pixel_samples"] / float(against)
            return rec

        for thr in (float(v) for v in a.thresholds.split(",")):
            d = measure("dammertz", thr)
            lo, hi = 1e-5, 10.0          # the samples fall as the threshold rises: bisect its logarithm
            for _ in range(24):
                mid = float(np.sqrt(lo * hi))
                ps = calls["variance"](mid)["pixel_samples"]
                if abs(ps / float(d["pixel_samples"]) - 1.0) <= 0.005:
                    break
                lo, hi = (mid, hi) if ps > d["pixel_samples"] else (lo, mid)
            rows += [d, measure("variance", mid, against=d["pixel_samples"])]

        # the cameras form at threshold 0: equal work, so the difference is the camera kernel the moments select (and the merge)
        blocks = jitter_blocks(wl.camera, a.cameras_spp, w, h)
        ckw = dict(batch=a.batch, min_spp=2 * a.batch)
        forms = [("renderAdaptiveCameras, moments off", 0, lambda: t.renderAdaptiveCameras(blocks, 0.0, **ckw)),
                 ("renderAdaptiveCameras, moments on", 1, lambda: t.renderAdaptiveCameras(blocks, 0.0, **ckw)),
                 ("renderAdaptiveVarianceCameras", 1, lambda: t.renderAdaptiveVarianceCameras(blocks, 0.0, **ckw))]
        recs = [dict(scene=name, form=f[0], ms=[]) for f in forms]
        for rnd in range(a.runs + 1):             # (the first pass warms the camera tables and code objects up)
            for f, r in zip(forms, recs):
                t.setOption(t.OPT_MOMENTS, f[1])
                ms, st = timed(f[2])
                if rnd:
                    r["ms"].append(ms)
                r.update(rounds=st["rounds"], family=t.lastCameraPlan()[1]["family"])
        cam_rows += recs
        t.setStream(None)
        t.close()
    if a.merge_rounds:
        return
    print("| scene | rule | threshold | ms: median (min .. max) of %d | pixel samples | vs Dammertz | mean spp | rounds | at max | RMSE (gamma) |" % a.runs)
    print("|---|---|---:|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print("| %s | %s | %.5g | %s | %d | %s | %.1f | %d | %d of %d | %.5f |" %
              (r["scene"], r["rule"], r["threshold"], spread(r["ms"]), r["pixel_samples"],
               "%+.2f %%" % (100 * (r["budget_ratio"] - 1)) if "budget_ratio" in r else "", r["mean_spp"], r["rounds"],
               r["blocks_at_max"], r["blocks"], r["rmse"]))
    print()
    print("| scene | cameras form, threshold 0, %d samples | camera kernel family | rounds | ms: median (min .. max) of %d |" % (a.cameras_spp, a.runs))
    print("|---|---|---:|---:|---:|")
    for r in cam_rows:
        print("| %s | %s | %d | %d | %s |" % (r["scene"], r["form"], r["family"], r["rounds"], spread(r["ms"])))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(rules=rows, cameras=cam_rows), f, indent=1)


def rays_main(a):
    """--rays [--sets K]: the experiment on an equirectangular frame of caller-supplied rays, both stopping rules."""
    import torch
    w, h = (int(v) for v in a.size.split("x"))
    thresholds = [float(v) for v in a.thresholds.split(",")]
    rows = []
    for name in a.scenes.split(","):
        wl = rt.workloads.get(name, width=w, height=h)
        t = rt.RayTracer(w, h, scene=wl.scene, seed=rt.workloads.SEED)
        t.setArith(2 if a.policy is None else a.policy)
        stream = torch.cuda.Stream()
        t.setStream(stream.cuda_stream)
        kw = dict(pos=np.asarray(wl.camera, np.float32)[:3], w=w, h=h, yaw=a.yaw)
        host = rt.rays.ray_sets(rt.rays.equirect_rays, rt.Camera.sampleOffsets(a.sets), **kw) if a.sets else rt.rays.equirect_rays(**kw)
        d = torch.from_numpy(rt.rays.as_floats(host).copy()).cuda()
        del host
        torch.cuda.synchronize()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            r = fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), r

        def fixed(spp):
            t.clear()
            if a.sets:
                t.renderRaySets(d, a.sets, 0, spp)
            else:
                t.renderRays(d, 0, spp)
            t.resolve()

        akw = dict(set_size=a.sets, batch=a.batch, min_spp=a.min_spp, max_spp=a.max_spp)
        calls = {"dammertz": lambda thr: t.renderAdaptiveRays(d, thr, **akw), "variance": lambda thr: t.renderAdaptiveVarianceRays(d, thr, **akw)}
        fixed(64)                                           # warm-up (code objects, buffers)
        calls["dammertz"](thresholds[0])
        t.setOption(t.OPT_MOMENTS, 1)
        calls["variance"](thresholds[0])
        t.setOption(t.OPT_MOMENTS, 0)
        fixed(a.truth_spp)
        truth = t.transferImage()[..., :3].astype(np.float64)

        def rmse():
            return float(np.sqrt(((t.transferImage()[..., :3].astype(np.float64) - truth) ** 2).mean()))

        configs = [("fixed", spp) for spp in (256, 1024)] + [(rule, thr) for rule in ("dammertz", "variance") for thr in thresholds]
        recs = {c: dict(scene=name, mode=c[0], ms=[]) for c in configs}
        for rnd in range(a.rounds):
            for c in configs:
                r = recs[c]
                t.setOption(t.OPT_MOMENTS, 1 if c[0] == "variance" else 0)
                if c[0] == "fixed":
                    ms, _ = timed(lambda: fixed(c[1]))
                    r["ms"].append(ms)
                    if rnd == 0:
                        r.update(spp=c[1], mean_spp=float(c[1]), rounds=1, rmse=rmse(), family=t.lastRayPlan()[1]["family"])
                    continue
                ms, st = timed(lambda: calls[c[0]](c[1]))
                r["ms"].append(ms)
                if rnd == 0:
                    r.update(threshold=c[1], mean_spp=st["pixel_samples"] / float(w * h), rounds=st["rounds"],
                             blocks_at_max=st["blocks_at_max"], blocks=st["blocks"], rmse=rmse(), family=t.lastRayPlan()[1]["family"])
        rows += [recs[c] for c in configs]
        t.setStream(None)
        t.close()
    print("equirect %s, %s, truth %d spp" % (a.size, "sets of %d" % a.sets if a.sets else "one record per ray", a.truth_spp))
    print("| scene | run | kernel family | ms: median (min .. max) of %d | mean spp | rounds | RMSE (gamma) |" % a.rounds)
    print("|---|---|---:|---:|---:|---:|---:|")
    for r in rows:
        run = "fixed %d" % r["spp"] if r["mode"] == "fixed" else "%s thr %g" % (r["mode"], r["threshold"])
        print("| %s | %s | %s | %s | %.1f | %d | %.5f |" % (r["scene"], run, "queue" if r["family"] else "fixed lanes", spread(r["ms"]),
                                                         r["mean_spp"], r["rounds"], r["rmse"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


def cameras_main(a):
    """--cameras: the experiment on anti-aliased frames."""
    import torch
    w, h = (int(v) for v in a.size.split("x"))
    thresholds = [float(v) for v in a.thresholds.split(",")]
    rows = []
    for name in a.scenes.split(","):
        wl = rt.workloads.get(name, width=w, height=h)
        t = rt.RayTracer(w, h, scene=wl.scene, seed=rt.workloads.SEED)
        if a.policy is not None:
            t.setArith(a.policy)
        stream = torch.cuda.Stream()
        t.setStream(stream.cuda_stream)
        blocks = jitter_blocks(wl.camera, max(a.truth_spp, a.max_spp), w, h)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            r = fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), r

        def fixed(spp):
            t.clear()
            t.renderSamplesCameras(blocks[:spp], 0)
            t.resolve()

        def adaptive(thr):
            return t.renderAdaptiveCameras(blocks[:a.max_spp], thr, batch=a.batch, min_spp=a.min_spp)

        fixed(64)                                           # warm-up (code objects, camera tables, buffers)
        adaptive(thresholds[0])
        truth = t.renderFrameCameras(blocks[:a.truth_spp])[..., :3].astype(np.float64)

        def rmse():
            return float(np.sqrt(((t.transferImage()[..., :3].astype(np.float64) - truth) ** 2).mean()))

        configs = [("fixed", spp) for spp in (256, 1024)] + [("adaptive", thr) for thr in thresholds + [0.0]]
        recs = {c: dict(scene=name, mode=c[0], ms=[]) for c in configs}
        for rnd in range(a.rounds):
            for c in configs:
                r = recs[c]
                if c[0] == "fixed":
                    ms, _ = timed(lambda: fixed(c[1]))
                    r["ms"].append(ms)
                    if rnd == 0:
                        r.update(spp=c[1], mean_spp=float(c[1]), rounds=1, rmse=rmse())
                    continue
                ms, st = timed(lambda: adaptive(c[1]))
                r["ms"].append(ms)
                launch = t.kernelMsHistory(st["rounds"])    # one camera launch per round, oldest first
                r.setdefault("round_ms", []).append(launch)
                if rnd == 0:
                    counts = t.sampleCounts().astype(np.int64)
                    by, bx = -(-h // 8), -(-w // 8)
                    pad = np.zeros((by * 8, bx * 8), np.int64)
                    pad[:h, :w] = counts
                    bc = pad.reshape(by, 8, bx, 8).max(axis=(1, 3))
                    r.update(threshold=c[1], mean_spp=st["pixel_samples"] / float(w * h), rounds=st["rounds"],
                             blocks_at_max=st["blocks_at_max"], blocks=st["blocks"], rmse=rmse(),
                             active_share=[float((bc > k * a.batch).mean()) for k in range(st["rounds"])])
        rows += [recs[c] for c in configs]
        t.setStream(None)
        t.close()
    print("| scene | run | ms: median (min .. max) of %d | mean spp | rounds | RMSE (gamma) |" % a.rounds)
    print("|---|---|---:|---:|---:|---:|")
    for r in rows:
        run = "fixed %d" % r["spp"] if r["mode"] == "fixed" else "adaptive thr %g" % r["threshold"]
        print("| %s | %s | %s | %.1f | %d | %.5f |" % (r["scene"], run, spread(r["ms"]), r["mean_spp"], r["rounds"], r["rmse"]))
    print()
    print("| scene | run | round | active blocks | launch ms (median) | ms per 1 % active |")
    print("|---|---|---:|---:|---:|---:|")
    for r in rows:
        if r["mode"] != "adaptive":
            continue
        per_round = np.median(np.asarray(r["round_ms"], dtype=np.float64), axis=0)
        for k, (share, ms) in enumerate(zip(r["active_share"], per_round)):
            print("| %s | thr %g | %d | %.1f %% | %.2f | %.3f |" % (r["scene"], r["threshold"], k, 100 * share, ms, ms / (100 * share)))
        print("| %s | thr %g | all | | %.1f of %.1f in launches | |" % (r["scene"], r["threshold"], per_round.sum(), sorted(r["ms"])[len(r["ms"]) // 2]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


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
    ap.add_argument("--cameras", action="store_true", help="anti-aliased frames: per-sample cameras (see the module text)")
    ap.add_argument("--rays", action="store_true", help="a frame of caller-supplied rays: an equirectangular panorama (see the module text)")
    ap.add_argument("--sets", type=int, default=0, help="--rays: K jittered records per pixel (ray sets); 0: one record per ray")
    ap.add_argument("--yaw", type=float, default=45.0, help="--rays: the panorama's yaw in degrees")
    ap.add_argument("--rounds", type=int, default=5, help="--cameras, --rays: repeats, the configurations alternating inside each")
    ap.add_argument("--policy", type=int, default=None, help="--cameras: arithmetic policy (default: the tracer's)")
    ap.add_argument("--rule", choices=("dammertz", "variance"), default="dammertz",
                    help="variance: compare the two stopping rules at equal pixel-sample budgets (see the module text)")
    ap.add_argument("--runs", type=int, default=3, help="--rule variance: timed repeats of every configuration")
    ap.add_argument("--cameras-spp", type=int, default=256, help="--rule variance: samples of the cameras-form comparison")
    ap.add_argument("--merge-rounds", type=int, default=0,
                    help="--rule variance: only render this many two-round threshold-0 frames per rule, for a kernel trace")
    ap.add_argument("--merge-trace", default=None, help="summarise the merge kernels of a rocprofv3 kernel-trace CSV and exit")
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace_main(a.merge_trace)
    if a.rays:
        return rays_main(a)
    if a.rule == "variance":
        return rule_main(a)
    if a.cameras:
        return cameras_main(a)
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
