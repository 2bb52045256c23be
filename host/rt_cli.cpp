// rt_cli.cpp — headless driver replacing the reference's GLFW application
// (main.cpp:62-116 render loop, :262-289 screenshot) for the trace path:
//   rt_cli --scene assets/scenes/c2_cornell.scene --size 1920x1080 --spp 64
//          --camera=-8,-1,-8,45,0 [--fov 60] [--seed 12648430] [--progressive [--lookahead N]]
//          [--out frame.tga] [--pfm frame.pfm] [--raw frame.f32] [--device 0]
//          [--adaptive THRESHOLD [--batch N] [--min-spp N] [--counts F.pgm|F.u32]]
//          [--adaptive-rule dammertz|variance]
//          [--denoise [--denoise-iterations N] [--sigma c,n,x,a] [--variance-guided [--sigma-luminance S] [--measured]]]
//              [--follow mirror,glass,dielectric [--max-chain N] [--split-chains]]]
//          [--aov PREFIX] [--aa] [--aperture R --focus D] [--aa-guides N]
//          [--adaptive-cameras THRESHOLD [--batch N] [--min-spp N] [--counts F.pgm|F.u32]]
//          [--progressive-cameras [--lookahead N]]
//          [--projection equirect|fisheye|ortho [--fov-deg F] [--extent E] [--ray-sets K] [--adaptive THRESHOLD ...]]
// --projection renders --spp samples through caller-supplied rays instead of the pinhole camera (host/rays.h →
// rt_upload_rays + rt_render_rays into the accumulator): an equirectangular panorama about --camera's position and yaw, an
// equidistant fisheye of --fov-deg degrees (default 180) or an orthographic view --extent world units wide (default 10)
// along --camera's direction.  It goes with --spp, --denoise (plain or --variance-guided, with or without --follow), --aov
// and the image outputs — the guides then come from rt_render_features_rays — and is refused with every other way to spend
// the samples (--progressive, --aa, --aperture, --adaptive-cameras, ...).
// --projection P [--ray-sets K] --adaptive THRESHOLD renders such a frame adaptively (rt_render_adaptive_rays; with
// --adaptive-rule variance rt_render_adaptive_variance_rays): --adaptive's rounds, --batch, --min-spp, --spp (the maximum,
// default 1024) and --counts over the frame's rays, with --ray-sets K sample s through record s mod K; --aov writes
// PREFIX_error.pfm under the variance rule as for the pinhole, and --denoise --variance-guided --measured filters on the
// moments the rule measured.
// --ray-sets K (1 .. RT_RAY_SET_MAX, only with --projection) anti-aliases such a frame: K records per pixel, jittered inside
// the pixel by the Halton points of Camera::sampleOffsets(K) (rays::ray_sets), sample s through record s mod K
// (rt_render_ray_sets); the guides of --denoise / --aov still come from the central rays.
// --aa jitters every sample's primary rays inside their pixels (Halton points, Camera::sampleBlocks) and --aperture R
// --focus D looks through a thin lens of radius R focused at distance D along the view direction: one camera block per
// sample, traced by rt_render_spp_cameras.  Both go with --spp (the fused path) and are refused with --progressive and
// --adaptive, whose samples share one camera; --denoise is allowed, its guides stay the unjittered camera's first hits
// unless --aa-guides N (1 .. 64; with --aa or --aperture, and --denoise or --aov) asks for the guides that belong to such a
// frame: the records of the run's first N sample cameras (its jitter, aperture and focus) reduced to one per pixel
// (rt_render_features_cameras; --follow / --max-chain are honoured), which the filter and --aov then use; --aov also writes
// PREFIX_coverage.pfm: per pixel (share of the N samples that hit, share in the dominant group, 0).
// --adaptive-cameras THRESHOLD (with --aa or --aperture R --focus D; refused with --adaptive and --progressive) renders such
// a frame adaptively (rt_render_adaptive_cameras): --adaptive's rounds, --batch, --min-spp, --spp (the maximum, default 1024)
// and --counts, with sample j of every pixel through block j of the run's --spp sample cameras; --denoise, --aov and
// --aa-guides work as with --spp.
// --adaptive-rule variance (with --adaptive or --adaptive-cameras; default dammertz) stops a block by the standard error of
// its pixels' means, measured from the per-pixel sample moments (rt_render_adaptive_variance, ..._variance_cameras): the
// moments are switched on before anything is accumulated, --min-spp may then equal --batch (default batch, at least 2), and
// --aov also writes PREFIX_error.pfm, the pixel errors the rule decided on; --denoise --variance-guided --measured filters
// on the same moments.
// --progressive-cameras (with --aa or --aperture R --focus D; refused with --progressive, --adaptive, --adaptive-cameras and
// --denoise) renders such a frame like the interactive app: render(block 0) + (spp - 1) x renderAgainCameras(table), the
// table being the run's first min(spp, 4096) sample cameras, sample s through block s mod that (rt_render_again_cameras);
// --lookahead N is accepted with it, and the image is the same whatever N.
// --progressive renders like the interactive app (render + spp-1 × renderAgain, one launch
// per sample, or with look-ahead — --lookahead N, 0 or 2 .. 64, default the library's 16 — one fused launch per N samples
// whose frames the calls hand out: the same image either way); the default is the fused path (all samples in one launch).  --adaptive renders
// rounds of --batch samples (default 64) until every 8x8 block's error is below THRESHOLD, with
// at least --min-spp (default 2 x batch) and at most --spp (default 1024 here) samples per pixel; --counts writes the
// per-pixel sample counts (16-bit PGM for a .pgm name, raw uint32 otherwise).  --denoise filters the rendered frame
// with the edge-avoiding à-trous denoiser (rt_denoise: --denoise-iterations, default 5; --sigma colour, normal,
// position, albedo, each > 0, inf = term off) guided by the first-hit features, and --out / --pfm / --raw then write the
// denoised frame.  The denoiser reads the linear accumulator; --progressive keeps its running mean in the image only, so
// there the same samples 0..spp-1 are first accumulated with the fused path.  --aov writes the feature buffers as
// PREFIX_normal.pfm, PREFIX_albedo.pfm and PREFIX_depth.pfm (the hit's t, +inf where the primary ray misses).
// --denoise --variance-guided selects the variance-guided filter for low sample counts instead (rt_denoise_variance:
// --sigma-luminance, default 4, > 0, inf = term off; --sigma keeps its four values, of which the colour one is unused);
// --aov then also writes PREFIX_variance.pfm, its 7x7 luminance-variance estimate v0.
// --denoise --variance-guided --measured keeps the per-pixel sample moments while accumulating (RT_OPT_MOMENTS) and filters
// on the variance measured from them wherever a pixel holds >= 4 samples (rt_denoise_moments); --aov then also writes
// PREFIX_samplevar.pfm, the measured variance of every pixel's mean luminance, M2 / (n (n - 1)) (0 where n < 2).
// --follow mirror,glass,dielectric (any of the three, comma-separated; with --denoise and / or --aov) guides the filter by the records at the
// end of every pixel's mirror / glass chain instead of the first hit (rt_render_features_chain: reflective, refractive
// and — by rayRefract's rule — dielectric hits are followed, at most --max-chain of them, default and maximum 29);
// --split-chains adds RT_DENOISE_SPLIT_CHAINS, so that pixels whose chains differ in length or objects never mix.
// --aov then writes the chain's records and also PREFIX_chain.pfm: per pixel (followed vertices, the signature's upper
// half as a number 0 .. 65535, 1 where the chain was cut at --max-chain).
// --ao K [--ao-distance D] (with --aov, first-hit guides: not with --follow or --aa-guides) adds ambient occlusion by the ray
// queries: K cosine-weighted hemisphere rays from every pixel's first hit (rays::hemisphere_sets, origin on the surface),
// one rt_occluded_rays call with set_size K and the bound D (default +inf: any hit), PREFIX_ao.pfm = 1 - count / K and 1
// where the pixel's primary ray missed.  The rays take 32 B x W x H x K of host and of device memory, and take the place of
// the uploaded rays of a --projection frame (nothing after this step reads those).
// --ao K --ao-device asks the device for the same picture instead (rt_occluded_hemispheres over the context's feature
// records, face-forward, seed --seed): the K rays of every pixel are made in the kernel's registers, so there are no host
// rays, no upload, and the uploaded rays stay.  The rays are those of the float64 generator to 1e-6, numbered by pixel
// (the host path numbers them by hit), so the two pictures agree as two estimates do, not bit for bit.
// --gather K [--gather-spp N] (with --aov, first-hit guides as --ao) adds an irradiance bake: radiance gathered along K
// device-made cosine-weighted directions from every pixel's first hit, each followed N times (default 1), in one
// rt_render_hemispheres call over the context's feature records (face-forward, seed --seed, origins lifted by 1e-3);
// PREFIX_irradiance.pfm = pi * rgb / count, three channels, 0 where the pixel's primary ray missed.  No ray is stored.
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "raytracer.h"
#include "rays.h"

static void check_rc(int rc) {
    if (rc) {
        std::cerr << "rt_cli: librt_amd error " << rc << std::endl;
        std::exit(1);
    }
}

static void usage() {
    std::cerr << "usage: rt_cli --scene FILE [--size WxH] [--spp N] [--camera=x,y,z,yaw,pitch] [--fov DEG] "
                 "[--seed N] [--progressive [--lookahead N]] [--progressive-cameras [--lookahead N]] [--out F.tga] [--pfm F.pfm] [--raw F.f32] [--device N] "
                 "[--adaptive THRESHOLD [--batch N] [--min-spp N] [--counts F.pgm|F.u32]] "
                 "[--denoise [--denoise-iterations N] [--sigma c,n,x,a] [--variance-guided [--sigma-luminance S] [--measured]] "
                 "[--follow mirror,glass,dielectric [--max-chain N] [--split-chains]]] "
                 "[--aov PREFIX] [--aa] [--aperture R --focus D] [--aa-guides N] "
                 "[--adaptive-cameras THRESHOLD [--batch N] [--min-spp N] [--counts F.pgm|F.u32]] "
                 "[--adaptive-rule dammertz|variance] [--projection equirect|fisheye|ortho [--fov-deg F] [--extent E] [--ray-sets K] "
                 "[--adaptive THRESHOLD ...]] [--ao K [--ao-distance D] [--ao-device]] [--gather K [--gather-spp N]]\n"
                 "  --ao K (1 .. 4096, with --aov): PREFIX_ao.pfm from K hemisphere rays per first hit, bound D (default inf);"
                 " its rays take 32 B x W x H x K of host and of device memory, unless --ao-device has the device make them"
                 " in registers (rt_occluded_hemispheres)\n"
                 "  --gather K (1 .. 4096, with --aov): PREFIX_irradiance.pfm from K device-made directions per first hit, N samples"
                 " each (rt_render_hemispheres)\n";
    std::exit(2);
}

// a whole decimal number in [lo, hi], or usage()
static long parse_int(const char *v, long lo, long hi) {
    char *end = nullptr;
    long x = std::strtol(v, &end, 10);
    if (!*v || *end || x < lo || x > hi) usage();
    return x;
}

// --sigma c,n,x,a: four numbers > 0 (inf allowed), or usage()
static void parse_sigmas(const char *v, float out[4]) {
    const char *p = v;
    for (int k = 0; k < 4; k++) {
        char *end = nullptr;
        out[k] = std::strtof(p, &end);
        if (end == p || !(out[k] > 0.0f)) usage();
        if (k < 3 && *end != ',') usage();
        p = end + (k < 3 ? 1 : 0);
    }
    if (*p) usage();
}

// --follow: a comma-separated list of mirror / glass / dielectric → RT_FOLLOW_* bits (at least one), or usage()
static uint32_t parse_follow(const char *v) {
    uint32_t mask = 0;
    std::string s = v;
    size_t at = 0;
    while (at <= s.size()) {
        size_t end = s.find(',', at);
        if (end == std::string::npos) end = s.size();
        const std::string word = s.substr(at, end - at);
        if (word == "mirror") mask |= RT_FOLLOW_REFLECTIVE;
        else if (word == "glass") mask |= RT_FOLLOW_REFRACTIVE;
        else if (word == "dielectric") mask |= RT_FOLLOW_DIELECTRIC;
        else usage();
        at = end + 1;
    }
    return mask;
}

// PFM of `ch` (1 or 3) channels taken from records of `stride` floats at offset `off`; rows bottom-up as the image's
static void write_pfm(const std::string &path, const float *data, size_t stride, size_t off, int ch, int w, int h) {
    std::ofstream f(path, std::ios::binary);
    f << (ch == 3 ? "PF" : "Pf") << "\n" << w << " " << h << "\n-1.0\n";
    for (size_t i = 0; i < (size_t)w * h; i++) f.write((const char *)(data + i * stride + off), ch * sizeof(float));
}

static void write_counts(const std::string &path, const std::vector<uint32_t> &c, int w, int h) {
    std::ofstream f(path, std::ios::binary);
    if (path.size() >= 4 && path.compare(path.size() - 4, 4, ".pgm") == 0) {
        // binary 16-bit PGM: big-endian samples, top row first (image row 0 is the bottom of the picture)
        f << "P5\n" << w << " " << h << "\n65535\n";
        std::string row((size_t)w * 2, '\0');
        for (int y = h - 1; y >= 0; y--) {
            for (int x = 0; x < w; x++) {
                uint32_t v = std::min<uint32_t>(c[(size_t)y * w + x], 65535u);
                row[2 * x] = (char)(v >> 8);
                row[2 * x + 1] = (char)(v & 0xFF);
            }
            f.write(row.data(), row.size());
        }
    } else {
        f.write((const char *)c.data(), c.size() * sizeof(uint32_t));
    }
}

int main(int argc, char **argv) {
    std::string scene_path = "assets/scenes/c2_cornell.scene", out_tga   // (the façade's own default is the reference's path, assets/scenes/scene.scene)
        , out_pfm, out_raw, dump_scene;
    int w = 1200, h = 800, spp = 16, device = 0, fov = 60;  // the reference's window is 1200x800 (main.cpp:9-12)
    float cam[5] = {0, 0, 0, 0, 0};
    unsigned long long seed = 0xC0FFEE;
    bool progressive = false, progressive_cameras = false;
    long lookahead = -1;   // (-1: the library's default)
    bool adaptive = false, adaptive_cameras = false, spp_given = false, rule_given = false, rule_variance = false;
    float threshold = 0.0f;
    long batch = 0, min_spp = 0;
    std::string out_counts;
    // rt_denoise defaults, the same as the Python surface's (opencl-raytracing_amd/_abi.py DENOISE_DEFAULTS)
    bool denoise = false;
    long dn_iterations = 0;
    float sigmas[4] = {0.5f, 0.1f, 2.0f, 0.2f};
    bool sigmas_given = false;
    bool variance_guided = false, sigma_l_given = false, measured = false;
    float sigma_l = 4.0f;
    std::string aov_prefix;
    uint32_t follow = 0;
    long max_chain = -1;   // (-1: RT_FEATURE_CHAIN_MAX)
    bool split_chains = false;
    bool aa = false, focus_given = false;
    float aperture = 0.0f, focus = 1.0f;
    long aa_guides = 0;   // (0: the central, unjittered records)
    std::string projection;
    float fov_deg = 180.0f, extent = 10.0f;
    bool fov_deg_given = false, extent_given = false;
    long ray_set = 0;   // (0: one record per pixel)
    long ao = 0;        // (0: no ambient occlusion)
    float ao_distance = INFINITY;
    bool ao_distance_given = false;
    bool ao_device = false;   // (the rays of --ao made on the device)
    long gather = 0;          // (0: no irradiance bake)
    long gather_spp = 0;      // (0: not given, 1)
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&](const char *name) -> const char * {
            size_t n = std::strlen(name);
            if (a.compare(0, n, name) == 0 && a.size() > n && a[n] == '=') return argv[i] + n + 1;
            if (a == name && i + 1 < argc) return argv[++i];
            return nullptr;
        };
        const char *v;
        if ((v = val("--scene"))) scene_path = v;
        else if ((v = val("--size"))) { if (std::sscanf(v, "%dx%d", &w, &h) != 2) usage(); }
        else if ((v = val("--spp"))) { spp = std::atoi(v); spp_given = true; }
        else if ((v = val("--camera"))) { if (std::sscanf(v, "%f,%f,%f,%f,%f", cam, cam + 1, cam + 2, cam + 3, cam + 4) != 5) usage(); }
        else if ((v = val("--fov"))) fov = std::atoi(v);
        else if ((v = val("--seed"))) seed = std::strtoull(v, nullptr, 0);
        else if ((v = val("--out"))) out_tga = v;
        else if ((v = val("--pfm"))) out_pfm = v;
        else if ((v = val("--raw"))) out_raw = v;
        else if ((v = val("--device"))) device = std::atoi(v);
        else if ((v = val("--dump-scene"))) dump_scene = v;
        else if ((v = val("--adaptive-rule"))) {
            const std::string r = v;
            if (r != "dammertz" && r != "variance") usage();
            rule_given = true;
            rule_variance = r == "variance";
        }
        else if ((v = val("--adaptive-cameras"))) {
            char *end = nullptr;
            threshold = std::strtof(v, &end);
            if (!*v || *end || !(threshold >= 0.0f) || !std::isfinite(threshold)) usage();
            adaptive_cameras = true;
        }
        else if ((v = val("--adaptive"))) {
            char *end = nullptr;
            threshold = std::strtof(v, &end);
            if (!*v || *end || !(threshold >= 0.0f) || !std::isfinite(threshold)) usage();
            adaptive = true;
        }
        else if ((v = val("--batch"))) batch = parse_int(v, 1, 512);
        else if ((v = val("--min-spp"))) min_spp = parse_int(v, 1, (long)RT_MAX_SAMPLE + 1);
        else if ((v = val("--counts"))) out_counts = v;
        else if ((v = val("--lookahead"))) { lookahead = parse_int(v, 0, 64); if (lookahead == 1) usage(); }
        else if ((v = val("--denoise-iterations"))) dn_iterations = parse_int(v, 1, RT_DENOISE_MAX_ITERATIONS);
        else if ((v = val("--sigma-luminance"))) {
            char *end = nullptr;
            sigma_l = std::strtof(v, &end);
            if (!*v || *end || !(sigma_l > 0.0f)) usage();
            sigma_l_given = true;
        }
        else if ((v = val("--sigma"))) { parse_sigmas(v, sigmas); sigmas_given = true; }
        else if ((v = val("--follow"))) follow = parse_follow(v);
        else if ((v = val("--max-chain"))) max_chain = parse_int(v, 0, RT_FEATURE_CHAIN_MAX);
        else if ((v = val("--ao"))) ao = parse_int(v, 1, (long)RT_RAY_SET_MAX);
        else if ((v = val("--gather"))) gather = parse_int(v, 1, (long)RT_RAY_SET_MAX);
        else if ((v = val("--gather-spp"))) gather_spp = parse_int(v, 1, (long)RT_MAX_SAMPLE + 1);
        else if ((v = val("--ao-distance"))) {
            char *end = nullptr;
            ao_distance = std::strtof(v, &end);
            ao_distance_given = true;
            if (!*v || *end || !(ao_distance > 0.0f)) usage();
        }
        else if ((v = val("--aov"))) { aov_prefix = v; if (aov_prefix.empty()) usage(); }
        else if ((v = val("--aperture"))) {
            char *end = nullptr;
            aperture = std::strtof(v, &end);
            if (!*v || *end || !(aperture > 0.0f) || !std::isfinite(aperture)) usage();
        }
        else if ((v = val("--focus"))) {
            char *end = nullptr;
            focus = std::strtof(v, &end);
            if (!*v || *end || !(focus > 0.0f) || !std::isfinite(focus)) usage();
            focus_given = true;
        }
        else if ((v = val("--projection"))) {
            projection = v;
            if (projection != "equirect" && projection != "fisheye" && projection != "ortho") usage();
        }
        else if ((v = val("--fov-deg"))) {
            char *end = nullptr;
            fov_deg = std::strtof(v, &end);
            if (!*v || *end || !(fov_deg > 0.0f) || !(fov_deg <= 360.0f)) usage();
            fov_deg_given = true;
        }
        else if ((v = val("--extent"))) {
            char *end = nullptr;
            extent = std::strtof(v, &end);
            if (!*v || *end || !(extent > 0.0f) || !std::isfinite(extent)) usage();
            extent_given = true;
        }
        else if ((v = val("--ray-sets"))) ray_set = parse_int(v, 1, RT_RAY_SET_MAX);
        else if ((v = val("--aa-guides"))) aa_guides = parse_int(v, 1, RT_FEATURE_CAMERAS_MAX);
        else if (a == "--aa") aa = true;
        else if (a == "--ao-device") ao_device = true;
        else if (a == "--denoise") denoise = true;
        else if (a == "--variance-guided") variance_guided = true;
        else if (a == "--measured") measured = true;
        else if (a == "--split-chains") split_chains = true;
        else if (a == "--progressive") progressive = true;
        else if (a == "--progressive-cameras") progressive_cameras = true;
        else usage();
    }
    if (spp < 1 || w < 1 || h < 1) usage();
    if (adaptive_cameras && (adaptive || progressive)) usage();            // one way to spend the samples
    if (!adaptive && !adaptive_cameras && (batch || min_spp || !out_counts.empty() || rule_given)) usage();   // adaptive-only flags
    if (!denoise && (dn_iterations || sigmas_given || variance_guided || sigma_l_given)) usage();   // denoise-only flags
    if ((sigma_l_given || measured) && !variance_guided) usage();
    if (follow && !denoise && aov_prefix.empty()) usage();                 // --follow guides --denoise and / or fills --aov
    if ((max_chain >= 0 || split_chains) && !follow) usage();
    if (split_chains && !denoise) usage();
    if (ao && (aov_prefix.empty() || follow || aa_guides)) usage();        // --ao fills --aov from first-hit records
    if ((ao_distance_given || ao_device) && !ao) usage();
    if (gather && (aov_prefix.empty() || follow || aa_guides)) usage();    // --gather fills --aov from first-hit records
    if (gather_spp && !gather) usage();
    if (gather && (uint64_t)gather * (uint64_t)std::max(gather_spp, 1L) > (uint64_t)RT_MAX_SAMPLE + 1u) usage();
    if (max_chain < 0) max_chain = RT_FEATURE_CHAIN_MAX;
    if (progressive_cameras && (progressive || adaptive || adaptive_cameras || denoise)) usage();   // one way to spend the samples; the running mean lives in the image
    if (!progressive && !progressive_cameras && lookahead >= 0) usage();   // progressive-only flag
    if ((aperture > 0.0f) != focus_given) usage();                         // a lens has a radius and a focus distance
    const bool cameras = aa || aperture > 0.0f;
    if (cameras && (progressive || adaptive)) {
        std::cerr << "rt_cli: --aa and --aperture give every sample a camera of its own; --progressive and --adaptive trace "
                     "all samples through one camera: use --spp" << std::endl;
        return 2;
    }
    if ((adaptive_cameras || progressive_cameras) && !cameras) usage();    // need the per-sample cameras of --aa / --aperture
    if (cameras && spp > (long)RT_MAX_SAMPLE + 1) usage();
    if (aa_guides && (!cameras || (!denoise && aov_prefix.empty()))) usage();   // guides of a per-sample-camera frame, for --denoise / --aov
    const bool rays_frame = !projection.empty();
    if (rays_frame && (cameras || progressive || progressive_cameras || adaptive_cameras)) usage();   // one way to spend the samples
    if (fov_deg_given && projection != "fisheye") usage();
    if (ray_set && !rays_frame) usage();   // ray sets belong to a projection (--aa is the pinhole camera's)
    if (extent_given && projection != "ortho") usage();
    if (!dn_iterations) dn_iterations = 5;
    if (adaptive || adaptive_cameras) {
        if (progressive) usage();
        if (!batch) batch = 64;
        if (!min_spp) min_spp = rule_variance ? std::max(batch, 2L) : 2 * batch;
        if (!spp_given) spp = 1024;
        if (min_spp < (rule_variance ? std::max(batch, 2L) : 2 * batch) || min_spp % batch || spp < min_spp || spp > (long)RT_MAX_SAMPLE + 1) usage();
    }

    Camera camera(fov, (float)w / (float)h, rth::vec3(cam[0], cam[1], cam[2]), cam[3], cam[4]);
    if (!dump_scene.empty()) {
        // host-only mode (no GPU): the arrays rt_set_scene would receive + the camera block, for parity
        // checks of the parser / OBJ reader / camera against other host implementations
        SceneCreator sc;
        try {
            sc.loadScene(scene_path);
            sc.loadTextures();
        } catch (const SceneError &e) {
            std::cerr << e.what() << std::endl;
            return 1;
        }
        rt_scene_desc d = sc.describe();
        std::ofstream f(dump_scene, std::ios::binary);
        uint32_t counts[12] = {d.material_count, d.sphere_count, d.plane_count, d.lens_count, d.vertex_count, d.uv_count,
                               d.index_count, d.mesh_count, d.model_count, (uint32_t)sc.texW(), (uint32_t)sc.texH(),
                               (uint32_t)sc.texLayers()};
        f.write((const char *)counts, sizeof counts);
        f.write((const char *)camera.transferData(), 12 * sizeof(float));
        f.write((const char *)d.materials, sizeof(rt_material) * d.material_count);
        f.write((const char *)d.spheres, sizeof(rt_sphere) * d.sphere_count);
        f.write((const char *)d.planes, sizeof(rt_plane) * d.plane_count);
        f.write((const char *)d.lenses, sizeof(rt_lens) * d.lens_count);
        f.write((const char *)d.vertices, sizeof(rt_float3) * d.vertex_count);
        f.write((const char *)d.uvs, sizeof(rt_float2) * d.uv_count);
        f.write((const char *)d.indices, sizeof(uint32_t) * d.index_count);
        f.write((const char *)d.meshes, sizeof(rt_mesh) * d.mesh_count);
        f.write((const char *)d.models, sizeof(rt_model) * d.model_count);
        if (sc.texLayers()) f.write((const char *)sc.texels(), sizeof(float) * 4 * sc.texW() * sc.texH() * sc.texLayers());
        return f ? 0 : 1;
    }
    RayTracer tracer(w, h, "kernels/raytracer.cl", scene_path, device, seed);
    if (measured || rule_variance) tracer.setMoments(true);   // before anything is accumulated: every path below starts with a clear

    auto t0 = std::chrono::steady_clock::now();
    const float *img;
    rt_adaptive_stats st{};
    if (adaptive && !rays_frame) {
        rt_adaptive_params p{(uint32_t)batch, (uint32_t)min_spp, (uint32_t)spp, threshold, 8, 8};
        st = rule_variance ? tracer.renderAdaptiveVariance(&camera, p) : tracer.renderAdaptive(&camera, p);
        img = tracer.lastImage();
    } else if (adaptive_cameras) {
        rt_adaptive_params p{(uint32_t)batch, (uint32_t)min_spp, (uint32_t)spp, threshold, 8, 8};
        const std::vector<float> blocks = camera.sampleBlocks((uint32_t)spp, 0, w, h, aa, aperture, focus);
        st = rule_variance ? tracer.renderAdaptiveVarianceCameras(blocks, p) : tracer.renderAdaptiveCameras(blocks, p);
        img = tracer.lastImage();
    } else if (progressive) {
        if (lookahead >= 0) tracer.setLookahead((int)lookahead);
        tracer.render(&camera);
        for (int s = 1; s < spp; s++) tracer.renderAgain(&camera);
        img = tracer.transferImage();
    } else if (progressive_cameras) {
        if (lookahead >= 0) tracer.setLookahead((int)lookahead);
        const std::vector<float> table = camera.sampleBlocks((uint32_t)std::min<long>(spp, (long)RT_AGAIN_CAMERAS_MAX), 0, w, h, aa, aperture, focus);
        check_rc(rt_render(tracer.context(), table.data()));
        for (int s = 1; s < spp; s++) tracer.renderAgainCameras(table);
        img = tracer.transferImage();
    } else if (rays_frame) {
        const float pos[3] = {cam[0], cam[1], cam[2]};
        auto generate = [&](rays::Offset off) {
            return projection == "equirect" ? rays::equirect(pos, w, h, cam[3], off)
                   : projection == "fisheye" ? rays::fisheye(pos, w, h, fov_deg, cam[3], cam[4], off)
                                             : rays::orthographic(pos, w, h, extent, cam[3], cam[4], off);
        };
        if (adaptive) {   // the frame's rays (or its sets of --ray-sets records) under --adaptive's rounds
            rt_adaptive_params p{(uint32_t)batch, (uint32_t)min_spp, (uint32_t)spp, threshold, 8, 8};
            tracer.uploadRays(ray_set ? rays::ray_sets(generate, Camera::sampleOffsets((uint32_t)ray_set)) : generate(rays::Offset{}));
            st = rule_variance ? tracer.renderAdaptiveVarianceRays((uint32_t)ray_set, p) : tracer.renderAdaptiveRays((uint32_t)ray_set, p);
            img = tracer.lastImage();
            if (ray_set && (denoise || !aov_prefix.empty())) tracer.uploadRays(generate(rays::Offset{}));   // the guides' central rays
        } else if (ray_set) {
            img = tracer.renderFrameRaySets(rays::ray_sets(generate, Camera::sampleOffsets((uint32_t)ray_set)), (uint32_t)ray_set, (uint32_t)spp);
            if (denoise || !aov_prefix.empty()) tracer.uploadRays(generate(rays::Offset{}));   // the guides' central rays
        } else {
            img = tracer.renderFrameRays(generate(rays::Offset{}), (uint32_t)spp);
        }
    } else if (cameras) {
        img = tracer.renderFrameCameras(camera.sampleBlocks((uint32_t)spp, 0, w, h, aa, aperture, focus));
    } else {
        img = tracer.renderFrame(&camera, (uint32_t)spp);
    }
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (adaptive || adaptive_cameras) {
        std::cout << w << "x" << h << (adaptive_cameras ? " adaptive per-sample cameras threshold " : rays_frame ? (ray_set ? " adaptive caller-supplied ray sets threshold " : " adaptive caller-supplied rays threshold ") : " adaptive threshold ") << threshold << (rule_variance ? " (variance rule)" : "") << " batch " << batch << " spp " << min_spp
                  << ".." << spp << ": " << st.rounds << " rounds, mean " << (double)st.pixel_samples / ((double)w * h)
                  << " spp, " << st.blocks_at_max << " of " << st.blocks << " blocks at max, " << sec * 1e3
                  << " ms incl. read-back" << std::endl;
        if (!out_counts.empty()) write_counts(out_counts, tracer.sampleCounts(), w, h);
    } else {
        std::cout << w << "x" << h << " " << spp << " spp " << (progressive ? "progressive" : progressive_cameras ? "progressive per-sample cameras" : rays_frame ? (ray_set ? "caller-supplied ray sets" : "caller-supplied rays") : cameras ? "per-sample cameras" : "fused") << ": " << sec * 1e3
                  << " ms incl. read-back, " << (double)w * h * spp / sec / 1e6 << " Msamples/s" << std::endl;
    }

    if (rays_frame) { if (denoise || !aov_prefix.empty()) tracer.renderFeaturesRays(follow, follow ? (uint32_t)max_chain : 0u); }
    else if (aa_guides) tracer.renderFeaturesCameras(camera.sampleBlocks((uint32_t)aa_guides, 0, w, h, aa, aperture, focus), follow,
                                                follow ? (uint32_t)max_chain : 0u);
    else if (follow) tracer.renderFeaturesChain(&camera, follow, (uint32_t)max_chain);
    else if (denoise || !aov_prefix.empty()) tracer.renderFeatures(&camera);
    if (denoise) {
        if (progressive) {   // the running mean of --progressive lives in the image: accumulate the same samples
            check_rc(rt_clear(tracer.context()));
            tracer.renderSamples(&camera, 0, (uint32_t)spp);
        }
        const uint32_t dn_flags = RT_DENOISE_SPLIT_OBJECTS | (split_chains ? RT_DENOISE_SPLIT_CHAINS : 0u);
        rt_denoise_params dp{(uint32_t)dn_iterations, sigmas[0], sigmas[1], sigmas[2], sigmas[3], dn_flags};
        rt_denoise_variance_params vp{(uint32_t)dn_iterations, sigma_l, sigmas[1], sigmas[2], sigmas[3], dn_flags};
        auto d0 = std::chrono::steady_clock::now();
        img = measured ? tracer.denoiseMoments(nullptr, vp) : variance_guided ? tracer.denoiseVariance(nullptr, vp) : tracer.denoise(nullptr, dp);
        if (aa_guides) std::cout << "guides: " << aa_guides << " sample cameras per pixel" << std::endl;
        if (follow)
            std::cout << "guides: chains through follow mask " << follow << ", at most " << max_chain << " vertices"
                      << (split_chains ? ", split" : "") << std::endl;
        std::cout << "denoised" << (measured ? " (variance-guided, measured)" : variance_guided ? " (variance-guided)" : "") << ": " << dn_iterations
                  << " iterations, sigma " << (variance_guided ? sigma_l : sigmas[0]) << "," << sigmas[1] << ","
                  << sigmas[2] << "," << sigmas[3] << ": "
                  << std::chrono::duration<double>(std::chrono::steady_clock::now() - d0).count() * 1e3
                  << " ms incl. read-back" << std::endl;
    }
    if (!aov_prefix.empty()) {
        std::vector<rt_feature> f = tracer.features();
        const float *fd = (const float *)f.data();
        const size_t stride = sizeof(rt_feature) / sizeof(float);
        write_pfm(aov_prefix + "_normal.pfm", fd, stride, offsetof(rt_feature, normal) / sizeof(float), 3, w, h);
        write_pfm(aov_prefix + "_albedo.pfm", fd, stride, offsetof(rt_feature, albedo) / sizeof(float), 3, w, h);
        write_pfm(aov_prefix + "_depth.pfm", fd, stride, offsetof(rt_feature, t) / sizeof(float), 1, w, h);
        if (follow) {
            std::vector<float> ch(f.size() * 3);
            for (size_t i = 0; i < f.size(); i++) {
                ch[3 * i] = (float)RT_FEATURE_CHAIN_LENGTH(f[i].flags);
                ch[3 * i + 1] = (float)(RT_FEATURE_CHAIN_SIGNATURE(f[i].flags) >> 16);
                ch[3 * i + 2] = (f[i].flags & RT_FEATURE_CUT) ? 1.0f : 0.0f;
            }
            write_pfm(aov_prefix + "_chain.pfm", ch.data(), 3, 0, 3, w, h);
        }
        if (aa_guides) {
            const std::vector<float> cv = tracer.featureCoverage();
            std::vector<float> c3(f.size() * 3, 0.0f);
            for (size_t i = 0; i < f.size(); i++) {
                c3[3 * i] = cv[2 * i];
                c3[3 * i + 1] = cv[2 * i + 1];
            }
            write_pfm(aov_prefix + "_coverage.pfm", c3.data(), 3, 0, 3, w, h);
        }
        if (ao && ao_device) {   // ambient occlusion with the rays made on the device: no host rays, no upload
            auto a0 = std::chrono::steady_clock::now();
            const std::vector<float> open = tracer.ambientOcclusion((uint32_t)ao, ao_distance, seed);
            std::cout << "ambient occlusion: " << ao << " device-made rays per pixel, bound " << ao_distance << ": "
                      << std::chrono::duration<double>(std::chrono::steady_clock::now() - a0).count() * 1e3 << " ms incl. read-back" << std::endl;
            write_pfm(aov_prefix + "_ao.pfm", open.data(), 1, 0, 1, w, h);
        } else if (ao) {   // ambient occlusion: K hemisphere rays per first hit, counted by one occlusion query
            std::vector<float> points, normals;
            std::vector<size_t> pixel;
            for (size_t i = 0; i < f.size(); i++)
                if (f[i].flags & RT_FEATURE_HIT) {
                    pixel.push_back(i);
                    points.insert(points.end(), f[i].pos, f[i].pos + 3);
                    // (the record's normal is the hit routine's: turned to the side the ray came from)
                    const float *nr = f[i].normal, *dr = f[i].dir;
                    const float side = nr[0] * dr[0] + nr[1] * dr[1] + nr[2] * dr[2] > 0.0f ? -1.0f : 1.0f;
                    for (int c = 0; c < 3; c++) normals.push_back(side * nr[c]);
                }
            std::vector<float> open((size_t)w * h, 1.0f);
            if (!pixel.empty()) {
                auto a0 = std::chrono::steady_clock::now();
                const std::vector<uint32_t> count = tracer.occludedRays(rays::hemisphere_sets(points, normals, (uint32_t)ao, seed), (uint32_t)ao, ao_distance);
                for (size_t j = 0; j < pixel.size(); j++) open[pixel[j]] = 1.0f - (float)count[j] / (float)ao;
                std::cout << "ambient occlusion: " << ao << " rays from each of " << pixel.size() << " hits, bound " << ao_distance << ": "
                          << std::chrono::duration<double>(std::chrono::steady_clock::now() - a0).count() * 1e3 << " ms incl. ray generation and read-back" << std::endl;
            }
            write_pfm(aov_prefix + "_ao.pfm", open.data(), 1, 0, 1, w, h);
        }
        if (gather) {   // irradiance: radiance gathered along device-made hemisphere rays, in one call
            const long each = std::max(gather_spp, 1L);
            auto g0 = std::chrono::steady_clock::now();
            const std::vector<float> e = tracer.irradiance((uint32_t)gather, (uint32_t)each, seed);
            std::cout << "irradiance: " << gather << " device-made directions per pixel, " << each << " samples each: "
                      << std::chrono::duration<double>(std::chrono::steady_clock::now() - g0).count() * 1e3 << " ms incl. read-back" << std::endl;
            write_pfm(aov_prefix + "_irradiance.pfm", e.data(), 3, 0, 3, w, h);
        }
        if (rule_variance) write_pfm(aov_prefix + "_error.pfm", tracer.pixelError().data(), 1, 0, 1, w, h);
        if (denoise && variance_guided) write_pfm(aov_prefix + "_variance.pfm", tracer.variance(0).data(), 1, 0, 1, w, h);
        if (denoise && measured) {
            const std::vector<float> m2 = tracer.moments();
            const std::vector<uint32_t> n = tracer.sampleCounts();
            std::vector<float> sv(m2.size());
            for (size_t i = 0; i < sv.size(); i++) sv[i] = n[i] >= 2u ? (float)((double)m2[i] / ((double)n[i] * ((double)n[i] - 1.0))) : 0.0f;
            write_pfm(aov_prefix + "_samplevar.pfm", sv.data(), 1, 0, 1, w, h);
        }
    }

    if (!out_raw.empty()) {
        std::ofstream f(out_raw, std::ios::binary);
        f.write((const char *)img, (size_t)w * h * 4 * sizeof(float));
    }
    if (!out_pfm.empty()) {  // PFM stores rows bottom-up; image row 0 is the bottom of the picture already
        std::ofstream f(out_pfm, std::ios::binary);
        f << "PF\n" << w << " " << h << "\n-1.0\n";
        for (size_t i = 0; i < (size_t)w * h; i++) f.write((const char *)(img + 4 * i), 3 * sizeof(float));
    }
    if (!out_tga.empty()) {
        // uncompressed 24-bit TGA, the header of main.cpp:266; bottom-up rows, BGR bytes
        short header[9] = {0, 2, 0, 0, 0, 0, (short)w, (short)h, 24};
        std::ofstream f(out_tga, std::ios::binary);
        f.write((const char *)header, sizeof header);
        std::string row((size_t)w * 3, '\0');
        for (int y = 0; y < h; y++) {
            for (int x = 0; x < w; x++) {
                const float *p = img + 4 * ((size_t)y * w + x);
                for (int c = 0; c < 3; c++) {
                    float v = p[2 - c];
                    v = v < 0 ? 0 : (v > 1 ? 1 : v);
                    row[3 * x + c] = (char)(unsigned char)std::lround(v * 255.0f);
                }
            }
            f.write(row.data(), row.size());
        }
    }
    return 0;
}
