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
    ap.add_argument("--rounds", type=int, default=5, help="--cameras: repeats, the configurations alternating inside each")
    ap.add_argument("--policy", type=int, default=None, help="--cameras: arithmetic policy (default: the tracer's)")
    a = ap.parse_args()
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
