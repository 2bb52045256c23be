// raytracer.cpp — see raytracer.h.
#include "raytracer.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <iostream>

bool RayTracer::throw_on_error = false;

void RayTracer::check(int rc) const {
    if (rc == RT_OK) return;
    std::string msg = rt_last_error(ctx);
    if (throw_on_error) throw RayTracerError(rc, msg);
    std::cerr << msg << std::endl;  // KernelGL::processError: message, then exit(-1)
    std::exit(-1);
}

void RayTracer::upload() {
    rt_scene_desc d = scene.describe();
    check(rt_set_scene(ctx, &d));
    check(rt_set_textures(ctx, scene.texels(), scene.texW(), scene.texH(), scene.texLayers()));
}

RayTracer::RayTracer(int w, int h, const char *kernel_path) : RayTracer(w, h, kernel_path, defaultScenePath()) {}

RayTracer::RayTracer(int w, int h, const char *, const std::string &scene_path, int device, uint64_t seed)
    : width(w), height(h) {
    check(rt_create(device, w, h, &ctx));
    check(rt_set_seed(ctx, seed));
    try {
        scene.loadScene(scene_path);  // the reference hard-codes its path, src/raytracer.cpp:95
        scene.loadTextures();
    } catch (const SceneError &e) {
        if (throw_on_error) throw;
        std::cerr << e.what() << std::endl;  // processError of src/scene.cpp:29-32
        std::exit(-1);
    }
    upload();
}

RayTracer::RayTracer(int w, int h, SceneCreator &&scene_, int device, uint64_t seed)
    : width(w), height(h), scene(std::move(scene_)) {
    check(rt_create(device, w, h, &ctx));
    check(rt_set_seed(ctx, seed));
    upload();
}

RayTracer::~RayTracer() { rt_destroy(ctx); }

void RayTracer::render(const Camera *camera) { check(rt_render(ctx, camera->transferData())); }
void RayTracer::renderAgain(const Camera *camera) { check(rt_render_again(ctx, camera->transferData())); }

const float *RayTracer::transferImage(Screen *, const char *) {
    pixels.resize((size_t)width * height * 4);
    check(rt_read_image(ctx, pixels.data(), pixels.size() * sizeof(float)));
    return pixels.data();
}

void RayTracer::setTime(float) {}

void RayTracer::resize(int w, int h) {
    check(rt_resize(ctx, w, h));
    width = w;
    height = h;
}

void RayTracer::renderSamples(const Camera *camera, uint32_t first_sample, uint32_t n_samples) {
    check(rt_render_spp(ctx, camera->transferData(), first_sample, n_samples));
}

const float *RayTracer::renderFrame(const Camera *camera, uint32_t spp) {
    check(rt_clear(ctx));
    check(rt_render_spp(ctx, camera->transferData(), 0, spp));
    check(rt_resolve(ctx));
    return transferImage();
}

void RayTracer::renderSamplesCameras(const std::vector<float> &blocks, uint32_t first_sample) {
    check(rt_render_spp_cameras(ctx, blocks.data(), first_sample, (uint32_t)(blocks.size() / 12)));
}

void RayTracer::uploadRays(const std::vector<rt_ray> &batch) { check(rt_upload_rays(ctx, batch.data(), batch.size())); }

void RayTracer::renderRays(uint32_t first_sample, uint32_t n_samples) {
    check(rt_render_rays(ctx, nullptr, (size_t)width * height, first_sample, n_samples, nullptr));
}

void RayTracer::renderFeaturesRays(uint32_t follow, uint32_t max_chain) {
    const rt_feature_chain_params p{follow, max_chain};
    check(rt_render_features_rays(ctx, nullptr, (size_t)width * height, &p));
}

namespace {
// a block of device memory for the results of a ray query, from the library (the façade has no HIP runtime of its own)
struct DeviceBlock {
    rt_context *ctx;
    void *p = nullptr;
    DeviceBlock(rt_context *c, size_t bytes, int *rc) : ctx(c) { *rc = rt_device_alloc(c, bytes, &p); }
    ~DeviceBlock() { (void)rt_device_free(ctx, p); }
    DeviceBlock(const DeviceBlock &) = delete;
    DeviceBlock &operator=(const DeviceBlock &) = delete;
};
}  // namespace

std::vector<rt_feature> RayTracer::intersectRays(const std::vector<rt_ray> &batch, uint32_t follow, uint32_t max_chain) {
    uploadRays(batch);
    std::vector<rt_feature> out(batch.size());
    int rc = RT_OK;
    DeviceBlock d(ctx, out.size() * sizeof(rt_feature), &rc);
    check(rc);
    const rt_feature_chain_params p{follow, max_chain};
    check(rt_intersect_rays(ctx, nullptr, batch.size(), &p, d.p));
    check(rt_device_copy(ctx, out.data(), d.p, out.size() * sizeof(rt_feature), 0));   // (behind the query on the stream)
    return out;
}

std::vector<uint32_t> RayTracer::occludedRays(const std::vector<rt_ray> &records, uint32_t set_size, float t_max,
                                              const std::vector<float> *bounds) {
    if (set_size == 0 || records.empty() || records.size() % set_size || (bounds && bounds->size() != records.size()))
        throw RayTracerError(RT_EINVAL, "occludedRays takes whole sets of set_size records and one bound per record");
    uploadRays(records);
    std::vector<uint32_t> out(records.size() / set_size);
    int rc = RT_OK;
    DeviceBlock d(ctx, out.size() * sizeof(uint32_t), &rc);
    check(rc);
    if (!bounds) {
        check(rt_occluded_rays(ctx, nullptr, out.size(), set_size, nullptr, t_max, d.p));
    } else {
        DeviceBlock b(ctx, bounds->size() * sizeof(float), &rc);
        check(rc);
        check(rt_device_copy(ctx, b.p, bounds->data(), bounds->size() * sizeof(float), 1));
        check(rt_occluded_rays(ctx, nullptr, out.size(), set_size, static_cast<const float *>(b.p), t_max, d.p));
        check(rt_sync(ctx));   // (the bounds are read until the query has run)
    }
    check(rt_device_copy(ctx, out.data(), d.p, out.size() * sizeof(uint32_t), 0));
    return out;
}

std::vector<uint32_t> RayTracer::occludedHemispheres(const rt_hemisphere_params &p, const void *d_features, size_t n) {
    if (!d_features) n = (size_t)width * height;
    if (n == 0) throw RayTracerError(RT_EINVAL, "occludedHemispheres takes at least one feature record");
    std::vector<uint32_t> out(n);
    int rc = RT_OK;
    DeviceBlock d(ctx, out.size() * sizeof(uint32_t), &rc);
    check(rc);
    check(rt_occluded_hemispheres(ctx, d_features, n, &p, d.p, nullptr));
    check(rt_device_copy(ctx, out.data(), d.p, out.size() * sizeof(uint32_t), 0));   // (behind the query on the stream)
    return out;
}

std::vector<float> RayTracer::ambientOcclusion(uint32_t k, float distance, uint64_t seed, float offset) {
    const rt_hemisphere_params p{k, RT_HEMI_FACE_FORWARD, seed, offset, distance};
    const std::vector<uint32_t> counts = occludedHemispheres(p);
    std::vector<float> out(counts.size());
    for (size_t i = 0; i < counts.size(); i++) out[i] = 1.0f - (float)counts[i] / (float)k;
    return out;
}

void RayTracer::renderHemispheres(const rt_hemisphere_params &p, uint32_t first_sample, uint32_t n_samples, void *d_accum,
                                  const void *d_features, size_t n) {
    if (!d_features) n = (size_t)width * height;
    check(rt_render_hemispheres(ctx, d_features, n, &p, first_sample, n_samples, d_accum));
}

std::vector<float> RayTracer::irradiance(uint32_t k, uint32_t spp_per_direction, uint64_t seed, float offset) {
    const size_t n = (size_t)width * height;
    if (n == 0 || spp_per_direction == 0) throw RayTracerError(RT_EINVAL, "irradiance takes a frame and at least one sample per direction");
    std::vector<float> acc(4 * n, 0.0f), out(3 * n, 0.0f);
    int rc = RT_OK;
    DeviceBlock d(ctx, acc.size() * sizeof(float), &rc);
    check(rc);
    check(rt_device_copy(ctx, d.p, acc.data(), acc.size() * sizeof(float), 1));   // the gather adds: it starts from zero
    const rt_hemisphere_params p{k, RT_HEMI_FACE_FORWARD, seed, offset, INFINITY};
    renderHemispheres(p, 0, (uint32_t)std::min<uint64_t>((uint64_t)k * spp_per_direction, UINT32_MAX), d.p);
    check(rt_device_copy(ctx, acc.data(), d.p, acc.size() * sizeof(float), 0));   // (behind the gather on the stream)
    const float pi = 3.14159265358979323846f;
    for (size_t i = 0; i < n; i++)
        if (acc[4 * i + 3] > 0.0f)
            for (int c = 0; c < 3; c++) out[3 * i + c] = (pi * acc[4 * i + c]) / acc[4 * i + 3];
    return out;
}

const float *RayTracer::renderFrameRays(const std::vector<rt_ray> &batch, uint32_t spp) {
    uploadRays(batch);
    check(rt_clear(ctx));
    renderRays(0, spp);
    check(rt_resolve(ctx));
    return transferImage();
}

void RayTracer::renderRaySets(uint32_t set_size, uint32_t first_sample, uint32_t n_samples) {
    check(rt_render_ray_sets(ctx, nullptr, (size_t)width * height, set_size, first_sample, n_samples, nullptr));
}

const float *RayTracer::renderFrameRaySets(const std::vector<rt_ray> &sets, uint32_t set_size, uint32_t spp) {
    uploadRays(sets);
    check(rt_clear(ctx));
    renderRaySets(set_size, 0, spp);
    check(rt_resolve(ctx));
    return transferImage();
}

void RayTracer::renderAgainCameras(const std::vector<float> &blocks) {
    check(rt_render_again_cameras(ctx, blocks.data(), (uint32_t)(blocks.size() / 12)));
}

const float *RayTracer::renderFrameCameras(const std::vector<float> &blocks) {
    check(rt_clear(ctx));
    renderSamplesCameras(blocks, 0);
    check(rt_resolve(ctx));
    return transferImage();
}

rt_adaptive_stats RayTracer::renderAdaptive(const Camera *camera, const rt_adaptive_params &params) {
    rt_adaptive_stats st{};
    check(rt_render_adaptive(ctx, camera->transferData(), &params, &st));
    transferImage();
    return st;
}

rt_adaptive_stats RayTracer::renderAdaptiveCameras(const std::vector<float> &blocks, const rt_adaptive_params &params) {
    rt_adaptive_stats st{};
    check(rt_render_adaptive_cameras(ctx, blocks.empty() ? nullptr : blocks.data(), (uint32_t)(blocks.size() / 12), &params, &st));
    transferImage();
    return st;
}

rt_adaptive_stats RayTracer::renderAdaptiveVariance(const Camera *camera, const rt_adaptive_params &params) {
    rt_adaptive_stats st{};
    check(rt_render_adaptive_variance(ctx, camera->transferData(), &params, &st));
    transferImage();
    return st;
}

rt_adaptive_stats RayTracer::renderAdaptiveVarianceCameras(const std::vector<float> &blocks, const rt_adaptive_params &params) {
    rt_adaptive_stats st{};
    check(rt_render_adaptive_variance_cameras(ctx, blocks.empty() ? nullptr : blocks.data(), (uint32_t)(blocks.size() / 12), &params, &st));
    transferImage();
    return st;
}

rt_adaptive_stats RayTracer::renderAdaptiveRays(uint32_t set_size, const rt_adaptive_params &params) {
    rt_adaptive_stats st{};
    check(rt_render_adaptive_rays(ctx, nullptr, (size_t)width * height, set_size, &params, &st));
    transferImage();
    return st;
}

rt_adaptive_stats RayTracer::renderAdaptiveVarianceRays(uint32_t set_size, const rt_adaptive_params &params) {
    rt_adaptive_stats st{};
    check(rt_render_adaptive_variance_rays(ctx, nullptr, (size_t)width * height, set_size, &params, &st));
    transferImage();
    return st;
}

std::vector<float> RayTracer::pixelError() {
    std::vector<float> e((size_t)width * height);
    check(rt_read_pixel_error(ctx, e.data(), e.size() * sizeof(float)));
    return e;
}

std::vector<uint32_t> RayTracer::sampleCounts() {
    std::vector<uint32_t> c((size_t)width * height);
    check(rt_read_sample_counts(ctx, c.data(), c.size() * sizeof(uint32_t)));
    return c;
}

void RayTracer::renderFeatures(const Camera *camera) {
    check(rt_render_features(ctx, camera->transferData()));
}

void RayTracer::renderFeaturesChain(const Camera *camera, uint32_t follow, uint32_t max_chain) {
    const rt_feature_chain_params p{follow, max_chain};
    check(rt_render_features_chain(ctx, camera->transferData(), &p));
}

void RayTracer::renderFeaturesCameras(const std::vector<float> &blocks, uint32_t follow, uint32_t max_chain) {
    const rt_feature_chain_params p{follow, max_chain};
    check(rt_render_features_cameras(ctx, blocks.empty() ? nullptr : blocks.data(), (uint32_t)(blocks.size() / 12), &p));
}

std::vector<float> RayTracer::featureCoverage() {
    std::vector<float> c((size_t)width * height * 2);
    check(rt_read_feature_coverage(ctx, c.data(), c.size() * sizeof(float)));
    return c;
}

std::vector<rt_feature> RayTracer::features() {
    std::vector<rt_feature> f((size_t)width * height);
    check(rt_read_features(ctx, f.data(), f.size() * sizeof(rt_feature)));
    return f;
}

const float *RayTracer::denoise(const Camera *camera, const rt_denoise_params &params) {
    if (camera) renderFeatures(camera);
    check(rt_denoise(ctx, &params));
    pixels.resize((size_t)width * height * 4);
    check(rt_read_denoised(ctx, pixels.data(), pixels.size() * sizeof(float)));
    return pixels.data();
}

const float *RayTracer::denoiseVariance(const Camera *camera, const rt_denoise_variance_params &params) {
    if (camera) renderFeatures(camera);
    check(rt_denoise_variance(ctx, &params));
    pixels.resize((size_t)width * height * 4);
    check(rt_read_denoised(ctx, pixels.data(), pixels.size() * sizeof(float)));
    return pixels.data();
}

std::vector<float> RayTracer::variance(int which) {
    std::vector<float> v((size_t)width * height);
    check(rt_read_variance(ctx, which, v.data(), v.size() * sizeof(float)));
    return v;
}

void RayTracer::setMoments(bool on) { check(rt_set_option(ctx, RT_OPT_MOMENTS, on ? 1 : 0)); }

std::vector<float> RayTracer::moments() {
    std::vector<float> m((size_t)width * height);
    check(rt_read_moments(ctx, m.data(), m.size() * sizeof(float)));
    return m;
}

const float *RayTracer::denoiseMoments(const Camera *camera, const rt_denoise_variance_params &params) {
    if (camera) renderFeatures(camera);
    check(rt_denoise_moments(ctx, &params));
    pixels.resize((size_t)width * height * 4);
    check(rt_read_denoised(ctx, pixels.data(), pixels.size() * sizeof(float)));
    return pixels.data();
}

void RayTracer::setPrefixCache(bool on) { check(rt_set_option(ctx, RT_OPT_PREFIX_CACHE, on ? 1 : 0)); }

void RayTracer::setLookahead(int samples) { check(rt_set_option(ctx, RT_OPT_LOOKAHEAD, samples)); }

RayTracer::LookaheadStats RayTracer::lookaheadStats() const {
    LookaheadStats s{};
    check(rt_lookahead_stats(ctx, &s.batches, &s.served, &s.direct, &s.discarded));
    return s;
}

void RayTracer::prefixCacheStats(uint64_t &hits, uint64_t &misses) const {
    check(rt_prefix_cache_stats(ctx, &hits, &misses));
}

void RayTracer::setExactGrid(bool on) { check(rt_set_option(ctx, RT_OPT_EXACT_GRID, on ? 1 : 0)); }

RayTracer::SampleGridStats RayTracer::sampleGridStats() const {
    SampleGridStats s{};
    check(rt_sample_grid_stats(ctx, &s.launches, &s.exact, &s.workgroups, &s.live_last));
    return s;
}

uint32_t RayTracer::sampleCounter() const {
    uint32_t v = 0;
    rt_sample_counter(ctx, &v);
    return v;
}
