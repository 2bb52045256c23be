// raytracer.h — RayTracer with the reference's public surface (include/raytracer.h:17-47,
// src/raytracer.cpp:24-174 of antoni-wojcik/OpenCL-Raytracing) over the C ABI of
// librt_amd.so (include/rt_amd.h).  No OpenCL / OpenGL: the image lives in HBM and is
// read back on request.  Errors print the library's message and exit(-1), as the
// reference does (src/kernelgl.cpp:47-56), unless exceptions are enabled with
// RayTracer::throwOnError(true).
#pragma once
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "../include/rt_amd.h"
#include "camera.h"
#include "scene.h"

struct Screen;  // the reference's display quad (include/screen.h) — out of scope, kept as an opaque name

struct RayTracerError : std::runtime_error {
    int code;
    RayTracerError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

class RayTracer {
    int width, height;
    rt_context *ctx = nullptr;
    SceneCreator scene;
    std::vector<float> pixels;  // last transferImage(): gamma-space RGBA32F, row 0 = y 0
    static bool throw_on_error;

    void check(int rc) const;
    void upload();

public:
    // the reference's constructor loads this path, relative to the working directory (src/raytracer.cpp:95); the
    // repository ships its own file of that name (assets/scenes/scene.scene)
    static const char *defaultScenePath() { return "assets/scenes/scene.scene"; }
    static void throwOnError(bool on) { throw_on_error = on; }

    // kernel_path is accepted for source compatibility with
    // RayTracer(w, h, "kernels/raytracer.cl") and ignored: the kernels are in librt_amd.so.
    RayTracer(int w, int h, const char *kernel_path);
    RayTracer(int w, int h, const char *kernel_path, const std::string &scene_path, int device = 0,
              uint64_t seed = 0xC0FFEE);
    RayTracer(int w, int h, SceneCreator &&scene_, int device = 0, uint64_t seed = 0xC0FFEE);
    ~RayTracer();
    RayTracer(const RayTracer &) = delete;
    RayTracer &operator=(const RayTracer &) = delete;

    void render(const Camera *camera);       // sample_counter = 0, kernel `trace`
    void renderAgain(const Camera *camera);  // ++sample_counter, kernel `retrace`
    // The reference binds a GL texture here (src/raytracer.cpp:167-174); this one reads the image
    // back and returns it (both arguments may be null).
    const float *transferImage(Screen *screen = nullptr, const char *shader_tex_id = nullptr);
    void setTime(float time);  // declared, never defined in the reference (raytracer.h:45): a stub
    void resize(int w, int h);

    // native additions
    void renderSamples(const Camera *camera, uint32_t first_sample, uint32_t n_samples);  // fused, asynchronous
    const float *renderFrame(const Camera *camera, uint32_t spp);  // clear + fused + resolve + read back
    // per-sample camera blocks (rt_render_spp_cameras, asynchronous): sample first_sample + j of every pixel through block j
    // of `blocks` (n x 12 floats, e.g. Camera::sampleBlocks: pixel jitter, depth of field); adds to the accumulator like
    // renderSamples.  renderFrameCameras: clear + that from sample 0 + resolve + read back
    void renderSamplesCameras(const std::vector<float> &blocks, uint32_t first_sample);
    const float *renderFrameCameras(const std::vector<float> &blocks);
    // renderAgain through a cyclic schedule of camera blocks (rt_render_again_cameras): the call that makes sample s looks
    // through block s mod n of `blocks` (n x 12 floats) — renderAgain's bits for that block, served from look-ahead batches
    // while the calls repeat one table
    void renderAgainCameras(const std::vector<float> &blocks);
    // caller-supplied rays (rt_upload_rays, rt_render_rays, rt_render_features_rays; host/rays.h makes panoramas, fisheye and
    // orthographic views and cube maps): uploadRays copies a batch into the context's ray buffer; renderRays traces samples
    // first_sample .. +n_samples-1 of the uploaded rays into the accumulator (the batch holds w x h rays, ray i = pixel i),
    // asynchronously like renderSamples; renderFeaturesRays writes the feature records that belong to such a frame, so that
    // denoise(nullptr, ...) works on it
    void uploadRays(const std::vector<rt_ray> &batch);
    void renderRays(uint32_t first_sample, uint32_t n_samples);
    void renderFeaturesRays(uint32_t follow = 0, uint32_t max_chain = 0);
    const float *renderFrameRays(const std::vector<rt_ray> &batch, uint32_t spp);  // upload + clear + renderRays + resolve + read back
    // ray queries (rt_intersect_rays, rt_occluded_rays): the geometric questions beside renderRays, for ANY batch.  The
    // image, the accumulator and the feature records stay as they are — but BOTH CALLS REPLACE THE UPLOADED RAYS: the batch
    // goes through uploadRays into the context's ray buffer, so a caller who uploaded a frame's rays before (renderRays,
    // renderFeaturesRays, the adaptive ray calls) uploads them again afterwards.  The device buffers the query writes come
    // from the library (rt_device_alloc); the calls wait for the query and return its results.  intersectRays: ray i's
    // rt_feature record as renderFeaturesRays / renderFeaturesChain writes it.  occludedRays: `records` holds sets of set_size
    // records, ray-major (rays::hemisphere_sets makes them); → per set the number of records whose first hit lies below its
    // bound, (*bounds)[k] or, with bounds null, t_max for every record (+inf: any hit)
    std::vector<rt_feature> intersectRays(const std::vector<rt_ray> &batch, uint32_t follow = 0, uint32_t max_chain = 0);
    std::vector<uint32_t> occludedRays(const std::vector<rt_ray> &records, uint32_t set_size = 1, float t_max = INFINITY,
                                       const std::vector<float> *bounds = nullptr);
    // hemisphere queries (rt_occluded_hemispheres): per feature record the number of occluded rays among p.k cosine-weighted
    // rays about its normal, the rays being made on the device — no host rays, no upload, and the uploaded rays stay.
    // d_features: n rt_feature records in device memory (rt_device_alloc + rt_intersect_rays), or null: the context's own
    // w x h records (renderFeatures & co. first).  The call waits for the query.  ambientOcclusion: 1 - count / k per pixel
    // of the context's records (1 on a miss), about the normal turned to face the viewer, rays bounded by `distance`
    std::vector<uint32_t> occludedHemispheres(const rt_hemisphere_params &p, const void *d_features = nullptr, size_t n = 0);
    std::vector<float> ambientOcclusion(uint32_t k = 16, float distance = INFINITY, uint64_t seed = 0, float offset = 0.0f);
    // hemisphere gather (rt_render_hemispheres, asynchronous): radiance along the same rays, sample s of record i along
    // hemisphere ray s mod p.k, ADDED to d_accum — n x 4 floats of sums and counts in device memory (rt_device_alloc) — or,
    // with d_accum null, to the accumulator (the context's own records then).  No ray reaches memory.  irradiance: pi * rgb /
    // count per pixel of the context's records, three floats each (0 on a miss), k directions about the normal turned to
    // face the viewer, each followed spp_per_direction times; it waits for the gather
    void renderHemispheres(const rt_hemisphere_params &p, uint32_t first_sample, uint32_t n_samples, void *d_accum = nullptr,
                           const void *d_features = nullptr, size_t n = 0);
    std::vector<float> irradiance(uint32_t k = 16, uint32_t spp_per_direction = 1, uint64_t seed = 0, float offset = 1e-3f);
    // ray sets (rt_render_ray_sets; rays::ray_sets makes them): the uploaded records are w x h sets of set_size records,
    // ray-major, and sample s of pixel i starts at record s mod set_size of its set — anti-aliasing for any projection
    void renderRaySets(uint32_t set_size, uint32_t first_sample, uint32_t n_samples);
    const float *renderFrameRaySets(const std::vector<rt_ray> &sets, uint32_t set_size, uint32_t spp);  // upload + clear + renderRaySets + resolve + read back
    // adaptive frame (rt_render_adaptive) + read back like renderFrame; the image is then transferImage()'s
    rt_adaptive_stats renderAdaptive(const Camera *camera, const rt_adaptive_params &params);
    // the same through per-sample camera blocks (rt_render_adaptive_cameras): sample j of every pixel through block j of
    // `blocks` (params.max_spp x 12 floats, e.g. Camera::sampleBlocks)
    rt_adaptive_stats renderAdaptiveCameras(const std::vector<float> &blocks, const rt_adaptive_params &params);
    // both under the variance-driven stopping rule (rt_render_adaptive_variance, ..._variance_cameras): setMoments(true)
    // first; pixelError() reads the W x H standard errors the rule decided on
    rt_adaptive_stats renderAdaptiveVariance(const Camera *camera, const rt_adaptive_params &params);
    rt_adaptive_stats renderAdaptiveVarianceCameras(const std::vector<float> &blocks, const rt_adaptive_params &params);
    // adaptive frames of caller-supplied rays (rt_render_adaptive_rays, rt_render_adaptive_variance_rays): the uploaded
    // records are w x h rays (set_size 0) or w x h ray-major sets of set_size records, sample s along record s mod set_size;
    // rounds, stopping rules and stats are those of renderAdaptive / renderAdaptiveVariance (setMoments(true) first)
    rt_adaptive_stats renderAdaptiveRays(uint32_t set_size, const rt_adaptive_params &params);
    rt_adaptive_stats renderAdaptiveVarianceRays(uint32_t set_size, const rt_adaptive_params &params);
    std::vector<float> pixelError();
    std::vector<uint32_t> sampleCounts();  // per-pixel sample counts, row-major
    const float *lastImage() const { return pixels.data(); }  // what the last read-back returned
    // first-hit feature records of every pixel (rt_render_features, asynchronous) and their read-back
    void renderFeatures(const Camera *camera);
    std::vector<rt_feature> features();
    // the records at the end of every pixel's mirror / glass chain instead (rt_render_features_chain, asynchronous): hits
    // whose material type is in `follow` (RT_FOLLOW_* bits) are followed, at most max_chain of them; features() and the
    // denoisers with a null camera then work on these
    void renderFeaturesChain(const Camera *camera, uint32_t follow, uint32_t max_chain = RT_FEATURE_CHAIN_MAX);
    // the guides of a renderFrameCameras frame (rt_render_features_cameras, asynchronous): the records of the n <= 64 camera
    // blocks of `blocks` (n x 12 floats, e.g. Camera::sampleBlocks) reduced to one record per pixel — the dominant group's
    // discrete fields, position / depth / normal / albedo averaged over the hit samples, RT_FEATURE_MIXED where the samples
    // disagree; follow / max_chain as renderFeaturesChain (0, 0: first hits).  featureCoverage: W x H x (hit share,
    // dominant share) of that call
    void renderFeaturesCameras(const std::vector<float> &blocks, uint32_t follow = 0, uint32_t max_chain = 0);
    std::vector<float> featureCoverage();
    // features for `camera` (unless it is null: then the last ones) + rt_denoise + read back into the image that
    // transferImage() / lastImage() return; the accumulator is left as it was
    const float *denoise(const Camera *camera, const rt_denoise_params &params);
    // the same with the variance-guided filter for low sample counts (rt_denoise_variance); variance(0) is its 7x7
    // luminance-variance estimate v0, variance(1) the filtered variance v(L), W x H floats each
    const float *denoiseVariance(const Camera *camera, const rt_denoise_variance_params &params);
    std::vector<float> variance(int which = 0);
    // RT_OPT_MOMENTS: the context keeps every pixel's centred second luminance moment M2 beside the accumulator, from the
    // next renderFrame / renderAdaptive (rt_clear) on; moments() reads the W x H floats.  denoiseMoments is
    // denoiseVariance on the variance MEASURED from them, M2 / (n (n - 1)), wherever a pixel holds >= 4 samples
    // (rt_denoise_moments); variance() serves it as well
    void setMoments(bool on);
    std::vector<float> moments();
    const float *denoiseMoments(const Camera *camera, const rt_denoise_variance_params &params);
    // RT_OPT_PREFIX_CACHE: while camera and scene rest, renderSamples keeps the traced prefix from call to call (default
    // on; same pixels either way); the counts of fused launches that reused it / traced it in full
    void setPrefixCache(bool on);
    void prefixCacheStats(uint64_t &hits, uint64_t &misses) const;
    // RT_OPT_LOOKAHEAD: while the camera rests, renderAgain computes the images after the next `samples` samples (2 .. 64,
    // default 16) in one fused launch and hands them out call by call; 0 = every call runs the direct kernel.  Same
    // pixels either way.  The counts since construction: look-ahead launches, calls served from a look-ahead frame,
    // calls that ran the direct kernel, frames computed and dropped.
    void setLookahead(int samples);
    struct LookaheadStats { uint64_t batches, served, direct, discarded; };
    LookaheadStats lookaheadStats() const;
    // RT_OPT_EXACT_GRID: while renderSamples reuses the kept prefix, its sample kernel is launched with exactly the
    // workgroups that own a live pixel (default on; same pixels either way).  The counts since construction: fused
    // launches, those sized by the known live list, workgroups launched in all, workgroups of the last exact launch.
    void setExactGrid(bool on);
    struct SampleGridStats { uint64_t launches, exact, workgroups, live_last; };
    SampleGridStats sampleGridStats() const;
    uint32_t sampleCounter() const;
    rt_context *context() { return ctx; }
    SceneCreator &sceneCreator() { return scene; }
    int getWidth() const { return width; }
    int getHeight() const { return height; }
};
