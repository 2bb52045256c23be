"""Feature buffers + à-trous denoiser against fixed sample counts (DESIGN.md "Feature buffers and denoising").

For each scene: a fixed 4096-spp frame is the ground truth.  For 1 / 4 / 16 / 64 spp it reports the gamma-space RMSE
of the noisy frame and of the denoised frame (default sigmas), the device time of rt_render_features and of rt_denoise
(events on the tracer's stream, median of --reps), and the smallest fixed spp (a power of two) whose noisy RMSE reaches
the denoised 16-spp RMSE.  --sweep instead scores a grid of sigmas at 16 spp (the choice of the defaults).
--variance-guided instead prints, per scene and spp, the RMSE and the device time of rt_denoise and of rt_denoise_variance
(default parameters each) side by side, on the same frames in the same run.
--measured prints that table with a fourth filter, rt_denoise_moments (the variance-guided filter on the variance measured
from the per-pixel sample moments, RT_OPT_MOMENTS), its device time, and what keeping the moments costs the frame: the
two stages of the fused 64-spp call (rt_stage_ms_history, median of --reps) with the option off and on.
--chain prints, per scene, the device time of rt_render_features and of rt_render_features_chain (all three glass-like
types followed, median of --reps), how many pixels have a chain, and per spp the RMSE of rt_denoise_variance guided by the
first-hit records, by the chain records, and by the chain records with RT_DENOISE_SPLIT_CHAINS — on the whole frame and
on the pixels with a chain — with the filter's device time without and with the flag.
--aa-guides is about the guides of anti-aliased frames (rt_render_features_cameras): per scene the device time of that call
at 16 blocks (median and min .. max of --reps), 16 x the single-camera rt_render_features time of the same run, and per
sample count (jittered frames of 4 / 16 / 64 samples through rt_render_spp_cameras, truth a jittered --truth-spp frame) the
RMSE of rt_denoise and rt_denoise_variance guided by the central records and by the 16-block records, on the whole frame
and on the pixels with RT_FEATURE_MIXED; then a depth-of-field row (C2, aperture 0.05, focus 8).  With --profile-only it
runs just the 16-block call --reps times per scene, and --trace FILE then prints the two kernels' times from such a run.
--profile-only runs just the denoise (with --variance-guided: rt_denoise_variance), --reps times, for a `rocprofv3 --kernel-trace --stats` run; --trace FILE turns
such a run's kernel_trace.csv into per-iteration times.

    python tools/denoise_bench.py [--scenes c2,c3,c5] [--size 1920x1080] [--json out.json] [--sweep | --variance-guided | --measured | --chain | --aa-guides]
"""
import argparse
import csv
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opencl_raytracing_amd as rt  # noqa: E402

D = rt._abi.DENOISE_DEFAULTS


def per_iteration(trace, iterations):
    """Per-iteration pt_atrous times (us, median) from a rocprofv3 kernel_trace.csv of --profile-only runs."""
    rows = [r for r in csv.DictReader(open(trace)) if "pt_atrous" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    us = us[len(us) % iterations:]
    return [float(np.median(us[i::iterations])) for i in range(iterations)]


# the cameras of the workloads (workloads.py): position, yaw, pitch — Camera.sampleBlocks needs the Camera, not its block
POSES = {"c2": ((-8, -1, -8), 45.0, 0.0), "c3": ((-6, -2, -7), 40.0, 8.0), "c5": ((-7, 0, -7), 45.0, 8.0)}
GUIDE_BLOCKS = 16


def guide_kernels(trace):
    """Times (us: median, min, max) of pt_features_cameras and pt_features_cameras_finish from a rocprofv3 kernel_trace.csv
    of --aa-guides --profile-only runs, per kernel name."""
    out = {}
    for r in csv.DictReader(open(trace)):
        if "pt_features_cameras" in r["Kernel_Name"]:
            key = "pt_features_cameras_finish" if "finish" in r["Kernel_Name"] else r["Kernel_Name"].split("(")[0]
            out.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: dict(n=len(v), median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c2,c3,c5")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--truth-spp", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--variance-guided", action="store_true")
    ap.add_argument("--measured", action="store_true")
    ap.add_argument("--chain", action="store_true")
    ap.add_argument("--aa-guides", action="store_true")
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.trace and a.aa_guides:
        print(json.dumps(guide_kernels(a.trace), indent=1))
        return
    if a.trace:
        print(json.dumps({"pt_atrous_us_per_iteration": per_iteration(a.trace, D["iterations"])}))
        return
    import torch
    w, h = (int(v) for v in a.size.split("x"))
    rows, sweep = [], []
    for name in a.scenes.split(","):
        wl = rt.workloads.get(name, width=w, height=h)
        t = rt.RayTracer(w, h, scene=wl.scene, seed=rt.workloads.SEED)
        stream = torch.cuda.Stream()
        t.setStream(stream.cuda_stream)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def dev(buf):
            return torch.as_tensor(buf, device="cuda")[..., :3].double()

        t.renderFrameOnDevice(wl.camera, 16)   # warm-up (code objects, buffers)
        t.renderFeatures(wl.camera)
        t.denoiseOnDevice()
        if a.variance_guided:
            t.denoiseVarianceOnDevice()
        if a.aa_guides:
            pos, yaw, pitch = POSES[name]
            cam = rt.Camera(60, np.float32(w) / np.float32(h), pos, yaw, pitch)
            assert np.array_equal(cam.transferData(), wl.camera)
            variants = [(name, 0.0)] + ([(name + " aperture 0.05 focus 8", 0.05)] if name == "c2" else [])
            for label, aperture in variants:
                def blocks(n):
                    return cam.sampleBlocks(n, 0, w, h, True, aperture, 8.0)
                guides = blocks(GUIDE_BLOCKS)
                t.renderFeaturesCameras(guides)                   # warm-up (code object, coverage buffer, camera tables)
                if a.profile_only:
                    for _ in range(a.reps):
                        t.renderFeaturesCameras(guides)
                    t.sync()
                    continue
                ms_g = [timed(lambda: t.renderFeaturesCameras(guides)) for _ in range(a.reps)]
                ms_1 = [timed(lambda: t.renderFeatures(wl.camera)) for _ in range(a.reps)]
                t.renderFeaturesCameras(guides)
                mixed_np = t.features()["mixed"]
                mixed = torch.as_tensor(mixed_np, device="cuda")
                t.clear()
                t.renderSamplesCameras(blocks(a.truth_spp), 0)
                t.resolve()
                t.sync()
                truth_aa = dev(t.deviceImage()).clone()

                def rmse2(buf):
                    t.sync()
                    d2 = (dev(buf) - truth_aa) ** 2
                    return float(torch.sqrt(d2.mean())), float(torch.sqrt(d2[mixed].mean()))

                for spp in (4, 16, 64):
                    t.clear()
                    t.renderSamplesCameras(blocks(spp), 0)
                    t.resolve()
                    r = dict(scene=label, spp=spp, mixed=int(mixed_np.sum()), rmse_noisy=rmse2(t.deviceImage()),
                             ms_guides=float(np.median(ms_g)), ms_guides_min=float(min(ms_g)), ms_guides_max=float(max(ms_g)),
                             ms_features=float(np.median(ms_1)), ms_features_min=float(min(ms_1)), ms_features_max=float(max(ms_1)))
                    for guide in ("central", "blocks"):
                        if guide == "central":
                            t.renderFeatures(wl.camera)
                        else:
                            t.renderFeaturesCameras(guides)
                        t.denoiseOnDevice()
                        r["rmse_denoise_" + guide] = rmse2(t.deviceDenoised())
                        t.denoiseVarianceOnDevice()
                        r["rmse_variance_" + guide] = rmse2(t.deviceDenoised())
                    rows.append(r)
            t.setStream(None)
            t.close()
            continue
        if a.profile_only:
            for _ in range(a.reps):
                t.denoiseVarianceOnDevice() if a.variance_guided else t.denoiseOnDevice()
            t.sync()
            t.setStream(None)
            t.close()
            continue
        t.renderFrameOnDevice(wl.camera, a.truth_spp)
        t.sync()
        truth = dev(t.deviceImage()).clone()

        def rmse(buf):
            t.sync()
            return float(torch.sqrt(((dev(buf) - truth) ** 2).mean()))

        if a.sweep:
            t.renderFrameOnDevice(wl.camera, 16)
            noisy = rmse(t.deviceImage())
            grid = itertools.product((0.25, 0.5, 1.0, 2.0, np.inf), (0.1, 0.3, 0.5, 1.0), (0.1, 0.25, 0.5, 1.0, 2.0),
                                     (0.05, 0.2, 0.5, np.inf))
            for sc, sn, sx, sa in grid:
                t.denoiseOnDevice(D["iterations"], sc, sn, sx, sa, True)
                sweep.append(dict(scene=name, sigma=[sc, sn, sx, sa], rmse=rmse(t.deviceDenoised()), noisy=noisy))
            t.setStream(None)
            t.close()
            continue
        if a.chain:
            ms_f = float(np.median([timed(lambda: t.renderFeatures(wl.camera)) for _ in range(a.reps)]))
            ms_c = float(np.median([timed(lambda: t.renderFeaturesChain(wl.camera, rt.FOLLOW_ALL)) for _ in range(a.reps)]))
            f = t.features()
            sub = torch.as_tensor(f["chain_length"] >= 1, device="cuda")
            stats = dict(chain1=int((f["chain_length"] >= 1).sum()), chain2=int((f["chain_length"] >= 2).sum()),
                         longest=int(f["chain_length"].max()), sky=int((~f["hit"] & (f["chain_length"] >= 1)).sum()))

            def rmse2(buf):
                t.sync()
                d2 = ((dev(buf) - truth) ** 2)
                return float(torch.sqrt(d2.mean())), (float(torch.sqrt(d2[sub].mean())) if stats["chain1"] else 0.0)

            for spp in (1, 4, 16):
                t.renderFrameOnDevice(wl.camera, spp)
                noisy = rmse2(t.deviceImage())
                t.renderFeatures(wl.camera)
                t.denoiseVarianceOnDevice()
                first = rmse2(t.deviceDenoised())
                t.renderFeaturesChain(wl.camera, rt.FOLLOW_ALL)
                ms_v = float(np.median([timed(lambda: t.denoiseVarianceOnDevice()) for _ in range(a.reps)]))
                chain = rmse2(t.deviceDenoised())
                ms_s = float(np.median([timed(lambda: t.denoiseVarianceOnDevice(split_chains=True)) for _ in range(a.reps)]))
                split = rmse2(t.deviceDenoised())
                rows.append(dict(scene=name, spp=spp, ms_features=ms_f, ms_features_chain=ms_c, rmse_noisy=noisy,
                                 rmse_first_hit=first, rmse_chain=chain, rmse_chain_split=split, ms_denoise_variance=ms_v,
                                 ms_denoise_variance_split=ms_s, **stats))
            t.setStream(None)
            t.close()
            continue
        if a.measured:
            def frame_ms(on):   # the fused call's two stages, median of reps: camera and scene rest, so the prefix is kept
                t.setOption(t.OPT_MOMENTS, on)
                first, second = [], []
                for _ in range(a.reps + 1):
                    t.renderFrameOnDevice(wl.camera, 64)
                    t.sync()
                    f, s2 = t.stageMsHistory(1)
                    first.append(float(f[-1]))
                    second.append(float(s2[-1]))
                return float(np.median(first[1:])), float(np.median(second[1:]))
            off, on = frame_ms(0), frame_ms(1)
            for spp in (2, 4, 16, 64):
                t.renderFrameOnDevice(wl.camera, spp)
                noisy = rmse(t.deviceImage())
                ms_d = float(np.median([timed(lambda: t.denoiseOnDevice()) for _ in range(a.reps)]))
                den = rmse(t.deviceDenoised())
                ms_v = float(np.median([timed(lambda: t.denoiseVarianceOnDevice()) for _ in range(a.reps)]))
                vg = rmse(t.deviceDenoised())
                ms_m = float(np.median([timed(lambda: t.denoiseMomentsOnDevice()) for _ in range(a.reps)]))
                rows.append(dict(scene=name, spp=spp, rmse_noisy=noisy, rmse_denoised=den, rmse_variance_guided=vg,
                                 rmse_moments=rmse(t.deviceDenoised()), ms_denoise=ms_d, ms_denoise_variance=ms_v,
                                 ms_denoise_moments=ms_m, frame64_ms_moments_off=off, frame64_ms_moments_on=on))
            t.setStream(None)
            t.close()
            continue
        if a.variance_guided:
            for spp in (1, 4, 16, 64):
                t.renderFrameOnDevice(wl.camera, spp)
                noisy = rmse(t.deviceImage())
                ms_d = float(np.median([timed(lambda: t.denoiseOnDevice()) for _ in range(a.reps)]))
                den = rmse(t.deviceDenoised())
                ms_v = float(np.median([timed(lambda: t.denoiseVarianceOnDevice()) for _ in range(a.reps)]))
                rows.append(dict(scene=name, spp=spp, rmse_noisy=noisy, rmse_denoised=den,
                                 rmse_variance_guided=rmse(t.deviceDenoised()), ms_denoise=ms_d, ms_denoise_variance=ms_v))
            t.setStream(None)
            t.close()
            continue
        ms_f = float(np.median([timed(lambda: t.renderFeatures(wl.camera)) for _ in range(a.reps)]))
        ms_d = float(np.median([timed(lambda: t.denoiseOnDevice()) for _ in range(a.reps)]))
        den16 = None
        for spp in (1, 4, 16, 64):
            t.renderFrameOnDevice(wl.camera, spp)
            noisy = rmse(t.deviceImage())
            t.denoiseOnDevice()
            den = rmse(t.deviceDenoised())
            if spp == 16:
                den16 = den
            rows.append(dict(scene=name, spp=spp, rmse_noisy=noisy, rmse_denoised=den, ms_features=ms_f,
                             ms_denoise=ms_d))
        match = None
        for spp in (32, 64, 128, 256, 512, 1024, 2048):
            t.renderFrameOnDevice(wl.camera, spp)
            if rmse(t.deviceImage()) <= den16:
                match = spp
                break
        for r in rows:
            if r["scene"] == name:
                r["fixed_spp_matching_denoised_16"] = match
        t.setStream(None)
        t.close()
    if a.profile_only:
        return
    if a.aa_guides:
        print("| scene | MIXED pixels | rt_render_features_cameras, %d blocks: ms (min .. max) | rt_render_features ms (min .. max) | %d x that |"
              % (GUIDE_BLOCKS, GUIDE_BLOCKS))
        print("|---|---:|---:|---:|---:|")
        for label in dict.fromkeys(r["scene"] for r in rows):
            r = next(r for r in rows if r["scene"] == label)
            print("| %s | %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.3f |" % (
                label.upper(), r["mixed"], r["ms_guides"], r["ms_guides_min"], r["ms_guides_max"], r["ms_features"],
                r["ms_features_min"], r["ms_features_max"], GUIDE_BLOCKS * r["ms_features"]))
        print()
        print("| scene | spp | pixels | RMSE noisy | rt_denoise, central guides | rt_denoise, %d-block guides | rt_denoise_variance, central | rt_denoise_variance, %d-block |"
              % (GUIDE_BLOCKS, GUIDE_BLOCKS))
        print("|---|---:|---|---:|---:|---:|---:|---:|")
        for r in rows:
            for k, what in ((0, "whole frame"), (1, "MIXED")):
                print("| %s | %d | %s | %.4f | %.4f | %.4f | %.4f | %.4f |" % (
                    r["scene"].upper(), r["spp"], what, r["rmse_noisy"][k], r["rmse_denoise_central"][k], r["rmse_denoise_blocks"][k],
                    r["rmse_variance_central"][k], r["rmse_variance_blocks"][k]))
        out = rows
    elif a.sweep:
        by = {}
        for r in sweep:
            by.setdefault(tuple(r["sigma"]), []).append(r["rmse"] / r["noisy"])
        ranked = sorted(by.items(), key=lambda kv: float(np.mean(kv[1])))
        print("| sigma c, n, x, a | RMSE ratio denoised / noisy per scene (16 spp) | mean |")
        print("|---|---|---:|")
        for k, v in ranked[:12]:
            print("| %s | %s | %.3f |" % (", ".join("%g" % x for x in k), ", ".join("%.3f" % x for x in v), np.mean(v)))
        out = sweep
    elif a.chain:
        print("| scene | pixels with a chain (>= 2 vertices, longest, ending in the sky) | rt_render_features ms | rt_render_features_chain ms |")
        print("|---|---|---:|---:|")
        for name in a.scenes.split(","):
            r = next(r for r in rows if r["scene"] == name)
            print("| %s | %d (%d, %d, %d) | %.3f | %.3f |" % (name.upper(), r["chain1"], r["chain2"], r["longest"], r["sky"],
                                                          r["ms_features"], r["ms_features_chain"]))
        print()
        print("| scene | spp | pixels | RMSE noisy | first-hit guides | chain guides | chain guides, split | filter ms | filter ms, split |")
        print("|---|---:|---|---:|---:|---:|---:|---:|---:|")
        for r in rows:
            for k, what in ((0, "whole frame"), (1, "chain >= 1")):
                print("| %s | %d | %s | %.4f | %.4f | %.4f | %.4f | %.3f | %.3f |" %
                      (r["scene"].upper(), r["spp"], what, r["rmse_noisy"][k], r["rmse_first_hit"][k], r["rmse_chain"][k],
                       r["rmse_chain_split"][k], r["ms_denoise_variance"], r["ms_denoise_variance_split"]))
        out = rows
    elif a.measured:
        print("| scene | spp | RMSE noisy | RMSE rt_denoise | RMSE rt_denoise_variance | RMSE rt_denoise_moments | rt_denoise ms | rt_denoise_variance ms | rt_denoise_moments ms |")
        print("|---|---:|---:|---:|---:|---:|---:|---:|---:|")
        for r in rows:
            print("| %s | %d | %.4f | %.4f | %.4f | %.4f | %.3f | %.3f | %.3f |" %
                  (r["scene"].upper(), r["spp"], r["rmse_noisy"], r["rmse_denoised"], r["rmse_variance_guided"], r["rmse_moments"],
                   r["ms_denoise"], r["ms_denoise_variance"], r["ms_denoise_moments"]))
        print()
        print("| scene | 64 spp frame, moments off: first + second stage ms | moments on |")
        print("|---|---:|---:|")
        for name in a.scenes.split(","):
            r = next(r for r in rows if r["scene"] == name)
            print("| %s | %.3f + %.3f | %.3f + %.3f |" % ((name.upper(),) + tuple(r["frame64_ms_moments_off"]) + tuple(r["frame64_ms_moments_on"])))
        out = rows
    elif a.variance_guided:
        print("| scene | spp | RMSE noisy | RMSE rt_denoise | RMSE rt_denoise_variance | rt_denoise ms | rt_denoise_variance ms |")
        print("|---|---:|---:|---:|---:|---:|---:|")
        for r in rows:
            print("| %s | %d | %.4f | %.4f | %.4f | %.3f | %.3f |" % (r["scene"].upper(), r["spp"], r["rmse_noisy"], r["rmse_denoised"],
                                                                   r["rmse_variance_guided"], r["ms_denoise"], r["ms_denoise_variance"]))
        out = rows
    else:
        print("| scene | spp | RMSE noisy | RMSE denoised | features ms | denoise ms | fixed spp matching denoised 16 |")
        print("|---|---:|---:|---:|---:|---:|---:|")
        for r in rows:
            m = r["fixed_spp_matching_denoised_16"]
            print("| %s | %d | %.5f | %.5f | %.3f | %.3f | %s |" % (r["scene"], r["spp"], r["rmse_noisy"], r["rmse_denoised"],
                                                                 r["ms_features"], r["ms_denoise"], m if m else "> 2048"))
        out = rows
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
