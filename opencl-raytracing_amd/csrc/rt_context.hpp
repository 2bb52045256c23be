// rt_context.hpp — the context behind the C ABI (include/rt_amd.h) and the helpers every translation unit of
// librt_amd.so shares: rt_amd.hip (host side: C ABI, scene upload from scene_prep.hpp, policy-free kernels), rt_denoise.hip
// (the denoisers, policy-free) and pt_kernels.hip (the path-tracing kernels and their launchers, compiled once per
// arithmetic policy).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "pt_types.hpp"

// Owns one device array: freed by release(), by reassignment and on destruction.  A group of them is reset by
// assigning {} to it.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {   // (the old array dies with `o`: at once for `= {}`)
        std::swap(p, o.p);
        std::swap(n, o.n);
        return *this;
    }
    ~DevBuf() { release(); }
    // exactly `count` uninitialised elements
    hipError_t alloc(size_t count) {
        release();
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        n = count;
        return e;
    }
    // tail_bytes: uninitialised room behind the array, in the same allocation (the staged scene block behind the materials)
    hipError_t upload(const T *src, size_t count, size_t tail_bytes = 0) {
        release();
        size_t alloc = count ? count : 1;  // empty arrays become 1-element dummies (src/scene.cpp:41-44)
        hipError_t e = hipMalloc((void **)&p, alloc * sizeof(T) + tail_bytes);
        if (e != hipSuccess) { p = nullptr; return e; }
        n = count;
        if (count) e = hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
        else e = hipMemset(p, 0, sizeof(T));
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

namespace pt { struct KernelSet; }

#define ACCEL_MIN_SPHERES 64
#define RT_SPP_PER_LAUNCH 512u   // samples per pixel of one trace launch (rt_render_spp splits larger calls); = QUEUE_SLOTS below
// The sample queue's launch constants (the queue itself: pt_queue.hpp): what the planners (plan_samples, plan_camera_samples,
// pt_kernels.hip) size a launch by and the kernels of both policy units (pt_kernels.hip, pt_gather.hip) are compiled for.
#ifndef QUEUE_SLOTS
#define QUEUE_SLOTS 512   // upper bound of samples a wave owns; the launch picks pixels_per_wave
#endif
#ifndef QUEUE_MAX_PIXELS
#define QUEUE_MAX_PIXELS 16
#endif
#ifndef PT_Q_WAVES
#define PT_Q_WAVES 6  // waves per SIMD the register allocator must leave room for: 6 = 80 VGPRs (A/B on C2: 5 → 2.62 ms, 6 → 2.48)
#endif
#ifndef PT_Q_WAVES_ACCEL
#define PT_Q_WAVES_ACCEL 5  // scenes that mix BVH meshes with small ones (every other mesh scene runs pt_samples_w), and scenes with a sphere BVH
                            // next to lenses / small meshes: 96 VGPRs (at 6 waves per SIMD = 80 VGPRs these instantiations spill 21 registers)
#endif
#ifndef PT_Q_WAVES_SPHERE_BVH
#define PT_Q_WAVES_SPHERE_BVH 6  // scenes whose only BVH is the sphere BVH (C4 at 8 spp, r02: 5 → 76.9 ms, 6 → 71.8 ms)
#endif
static_assert(QUEUE_SLOTS >= RT_SPP_PER_LAUNCH, "rt_render_spp's launches must fit a wave's sample queue");
#define RT_LOOKAHEAD_MAX 64                     // largest RT_OPT_LOOKAHEAD: frames of one look-ahead batch
#define RT_LOOKAHEAD_MAX_BYTES (1ull << 30)     // budget of a context's look-ahead ring: a batch holds as many frames as fit
#ifndef MESH_BVH_MIN_FACES
#define MESH_BVH_MIN_FACES 32
#endif

struct rt_context {
    int device = 0;
    int width = 0, height = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    static constexpr int EV_RING = 64;   // event pairs of the last EV_RING render calls
    hipEvent_t ev[EV_RING][3] = {};      // [0] before the call, [1] after it, [2] between the fused call's two stages
    uint64_t ev_count = 0;
    std::string error;
    std::string dev_name, dev_arch;
    int cu_count = 0;

    DevBuf<rt_material> materials;
    DevBuf<rt_sphere> spheres;
    DevBuf<float4> sph4;
    uint32_t sphere_batches = 0;
    DevBuf<float4> faces;
    DevBuf<uint32_t> mesh_face_base;
    DevBuf<float4> mbvh_nodes, mbvh_faces;
    DevBuf<uint32_t> mbvh_face_idx, mesh_bvh_root;
    bool have_mesh_bvh = false;
    DevBuf<float4> bvh_nodes, bvh_sph;
    DevBuf<uint32_t> bvh_idx;
    DevBuf<float4> bvh_links;
    uint32_t bvh_node_count = 0;
    float bvh_lo[3] = {0, 0, 0}, bvh_hi[3] = {0, 0, 0}, bvh_rmax = 0;
    int accel = 1;  // RT_OPT_ACCEL: 0 brute force, 1 BVH for >= ACCEL_MIN_SPHERES spheres, 2 always BVH
    int arith = 0;  // RT_OPT_ARITH: the arithmetic policy (pt_arith.hpp) whose kernels render
    const pt::KernelSet *ks = nullptr;   // that policy's launchers
    // host copies of what depends on the policy (re-derived by rt_set_option(RT_OPT_ARITH)): the spheres' test records
    // hold r*r (policies 0, 1) or r (policy 2), the per-face normals are computed ON THE DEVICE with the policy's
    // cross / normalize for policies 1, 2
    std::vector<rt_sphere> h_spheres;
    std::vector<uint32_t> h_bvh_idx;
    std::vector<float4> h_faces, h_mbvh_faces;
    DevBuf<rt_plane> planes;
    DevBuf<rt_lens> lenses;
    DevBuf<rt_float3> vertices;
    DevBuf<rt_float2> uvs;
    DevBuf<uint32_t> indices;
    DevBuf<rt_mesh> meshes;
    DevBuf<rt_model> models;
    DevBuf<float> table;
    DevBuf<float4> tex;
    int tex_w = 1, tex_h = 1, tex_layers = 0;
    bool have_scene = false;
    bool scene_uses_textures = false;
    uint32_t max_texture_id = 0;

    // frame: reallocated and zeroed by alloc_frame
    DevBuf<float4> image, accum;
    // counter block (COUNTER_REPLICAS rows, then 32 words): made once by rt_create, dies with the context
    DevBuf<unsigned long long> counters;
    uint32_t *d_walk_overflow = nullptr;   // one word of sticky PT_OVF_* bits, inside `counters`
    // fused-path slot buffers, made whole by ensure_slots when the shard outgrows them: reset by alloc_frame
    struct Slots {
        DevBuf<pt::PixelRec> recs;      // per owned pixel slot: shared path prefix (fused path)
        DevBuf<uint32_t> live;          // slots that need per-sample work + [capacity] = their count
        size_t capacity = 0;
        // shared decision trees of dielectric-first pixels (pt_types.hpp): both or none (tree_capacity 0)
        DevBuf<pt::PixelTree> trees;    // tree_capacity of them
        DevBuf<pt::PixelRec> tree_wait; // glass vertices waiting for the next level: PT_TREE_WAITS per tree
        size_t tree_capacity = 0;
        // the pixels pt_prefix finished: workgroup b's at finals[256 b …], final_n[b] of them (pt_final_replay)
        DevBuf<pt::FinalPix> finals;
        DevBuf<uint32_t> final_n;
    } slots;
    // What the last pt_prefix left in `slots`, kept for as long as it stays true (launch_fused): a fused call that finds
    // the entry valid and its key unchanged launches pt_final_replay instead of pt_prefix and runs the sample kernel
    // over the buffers as they lie.
    //  * What pt_prefix writes — the records, the ordered live list and its counters, the decision trees, the finished
    //    list — is a function of the scene (DeviceScene: geometry, materials, textures, random table, RT_OPT_ACCEL, the
    //    policy's records), the policy's kernels, and these FrameParams fields: cam, w, h, tile_*_log2, tiles_x,
    //    tiles_total, rank, world, slot_begin, slot_end, seg_cap, trees, tree_wait, tree_count, tree_cap and the block
    //    mask.  trace_prefix and tree_step take no FrameParams at all (pt_device.hpp); `first` is not read; `count` and
    //    `group_log2` enter the finished pixels' closed-form sum only, which pt_final_replay forms anew per call.
    //  * The sample kernels (pt_samples_q, pt_samples_w, pt_samples) READ recs, live, live_count and the trees and write
    //    the accumulator (and the work counters) only, so a launch leaves the entry as it found it.
    //  * Key: (generation, the camera block's 12 floats as bits, trees on / off — tree_cap follows PT_TREE_MIN_SAMPLES).
    //    `generation` is bumped (prefix_changed()) by every entry point that can change anything else on the list above
    //    or reallocates the buffers: scene, textures, random table / seed, every rt_set_option, shard, frame size,
    //    stream, counters on / off, ensure_slots growing.  When in doubt, bump.
    //  * A look-ahead launch (launch_lookahead) is an ordinary fused launch as far as the slot buffers go: its pt_prefix
    //    differs only in NOT adding the finished pixels' sums (accum == NULL), its sample kernel only in what it does with the
    //    slots' radiances (queue_replay), and pt_final_retrace reads the finished list.  So it hits, misses and leaves an
    //    entry under the same key, and an rt_render_spp call with the same camera afterwards may reuse its prefix.
    //  * A launch that writes the buffers only partly or for another purpose — a block mask (adaptive rounds), counters
    //    enabled, a frame cut into several slot ranges, an error — takes the full path and leaves the entry invalid.
    struct PrefixCache {
        bool enabled = true;            // RT_OPT_PREFIX_CACHE (rt_create: the environment's RT_PREFIX_CACHE=0 turns it off)
        bool valid = false;
        uint64_t generation = 0;        // now
        uint64_t key_generation = 0;    // the entry's
        uint32_t key_cam[12] = {};
        bool key_tree_on = false;
        uint64_t hits = 0, misses = 0;  // fused launches served from the entry / traced in full (rt_prefix_cache_stats)
        // The entry's live counters as the HOST knows them (RT_OPT_EXACT_GRID): while the entry is valid nothing writes
        // the live-count block, so a launch that hits may be sized for the live list instead of for "every pixel is live".
        //  * The first launch that HITS the entry enqueues an asynchronous copy of the block into `sample_grid.h_counts`
        //    (pinned, owned by the context) with `sample_grid.counts_ev` behind it — not the miss: a camera that moves with
        //    every frame never hits and never pays for a copy.  Later hits only query the event, never wait on it; from
        //    the first query that finds it complete the counts are known and rt_sample_units sizes the launch.
        //  * The counts are part of the entry: EVERY fused launch that is not a hit drops them (launch_fused), and whatever
        //    invalidates or re-keys the entry — prefix_changed(), another camera, trees on / off, a masked, counting or
        //    split launch — makes the next launch such a one.  A copy still in flight then lands in the pinned block
        //    unread; a later copy follows it on the same stream (rt_set_stream synchronises the old one first).
        enum { COUNTS_UNKNOWN, COUNTS_IN_FLIGHT, COUNTS_KNOWN } counts_state = COUNTS_UNKNOWN;
        uint32_t count_light = 0, count_heavy = 0;   // live_count[0], live_count[LIVE_HEAVY_COUNTER], unclamped
    } prefix_cache;
    void prefix_changed() { prefix_cache.generation++; }
    // The staged scene block: the LDS tables of stage_materials (pt_device.hpp) as the selected policy's kernels compute
    // them, lds_static_used(...) float4 BEHIND the materials array in the same allocation (stage_block_of; rt_set_scene
    // leaves the room) — pt_samples_q without counters and without a BVH walk copies it instead of computing it per wave.
    // Whatever can change a word of it (the scene's materials, spheres or planes; the arithmetic policy, whose divisions
    // it holds) bumps the prefix generation already, so launch_fused rebuilds it when `generation` is not the prefix
    // cache's — a superset of the reasons, one tiny kernel each, and nothing of the prefix cache is touched.
    struct StageBlock {
        uint64_t generation = ~0ull;    // prefix_cache.generation the block was built at
        uint64_t builds = 0;            // (rt_debug_wave_fixed)
    } stage_block;
    // RT_OPT_EXACT_GRID and rt_sample_grid_stats; the pinned block and the event are made by rt_create and die with the context
    struct SampleGrid {
        bool exact = true;              // RT_OPT_EXACT_GRID (rt_create: the environment's RT_EXACT_GRID=0 turns it off)
        uint32_t *h_counts = nullptr;   // pinned: LIVE_COUNT_STRIDE words, the target of the counts' copy
        hipEvent_t counts_ev = nullptr;
        uint64_t launches = 0;          // fused launches that reached the sample stage
        uint64_t exact_launches = 0;    // … sized by the known counts (a launch of zero workgroups included)
        uint64_t workgroups = 0;        // sample-kernel workgroups launched, all launches together
        uint64_t live_last = 0;         // workgroups of the last EXACT launch's kernel that own a pixel (= its grid)
        // what the last launch's sample stage was chosen from and what was chosen (plan_samples, pt_kernels.hip);
        // pixels_per_wave 0: no launch yet (rt_debug_last_sample_plan, rt_debug_live_list)
        rt_sample_facts last_facts = {};
        rt_sample_plan last_plan = {};
        uint64_t count64_launches = 0;  // sample-stage launches whose plan was pt_samples_q<…, COUNT_LOG2 = 6> (rt_debug_wave_fixed)
    } sample_grid;
    // Look-ahead for rt_render_again (RT_OPT_LOOKAHEAD): while the camera rests, ONE fused launch traces the next `pending`
    // samples and replays the gamma-space running mean per pixel, the image after each sample going to a frame of `ring`;
    // the following calls hand those frames out, one device copy each.  The ring is allocated on the first batch, reset by
    // alloc_frame, freed with the context.  The frames are valid while nothing they were computed from has changed: the
    // camera bits, the prefix generation (scene, seed, options, shard, size, stream, counters — prefix_changed()), the
    // IMAGE EPOCH (bumped by whatever else writes the image: rt_render, rt_resolve, rt_render_adaptive, a direct
    // rt_render_again, alloc_frame) and the sample counter being the batch's next index.
    struct Lookahead {
        int k = 16;                     // RT_OPT_LOOKAHEAD: 0 off, 2 .. 64 samples per batch
        DevBuf<float4> ring;            // ring_frames frames of W x H, frame-major
        size_t ring_frames = 0;
        bool ring_failed = false;       // the allocation failed for this frame size / option: direct path until either changes
        uint32_t pending = 0;           // frames of the last batch not handed out yet
        uint32_t batch_frames = 0;      // frames the last batch computed
        uint32_t next_frame = 0;        // the ring frame handed out next …
        uint32_t next_sample = 0;       // … which is the image after this sample
        uint64_t key_generation = 0, key_epoch = 0;
        uint32_t key_cam[12] = {};
        bool have_last_cam = false;     // the camera block of the previous rt_render / rt_render_again call
        uint32_t last_cam[12] = {};
        // rt_render_again_cameras: the same rule over a cyclic TABLE of blocks.  `last_table` is the host copy of the table
        // the previous such call was given (n x 12 words; dropped by a plain rt_render_again, which in turn finds no
        // `last_cam` after a table call); a batch launched by a table call is keyed by that table (`key_is_table`, key_cam
        // unused) and handed out to table calls only.
        bool have_last_table = false;
        std::vector<uint32_t> last_table;
        bool key_is_table = false;
        uint64_t batches = 0, served = 0, direct = 0, discarded = 0;   // rt_lookahead_stats
    } lookahead;
    uint64_t image_epoch = 0;
    bool wave_fill = true;              // RT_OPT_WAVE_FILL
    int prefix_tree = 1;                // RT_OPT_PREFIX_TREE: 0 off, 1 from PT_TREE_MIN_SAMPLES samples per call on, 2 always
    bool prefix_sharing = true;
    bool sample_queue = true;
    DevBuf<uint2> walk_jobs;         // (mesh, model material) of every model's meshes in hit order; empty unless
                                     // every one of them has a BVH (pt_samples_w)
    bool walk_slices = true;         // RT_OPT_WALK_SLICES
    uint32_t accum_count = 0;
    // rt_clear under RT_OPT_ACCUM_STORE 1 records the clear instead of enqueuing it: the accumulator is LOGICALLY zero while
    // clear_pending is set, and its bytes are whatever they were.  A qualifying fused launch (launch_fused_any, pt_kernels.hip)
    // stores its sums and ends the state; everything else that reads, writes or hands out the accumulator, and every wait
    // for the stream, calls materialise_clear first.
    bool accum_store = true;         // RT_OPT_ACCUM_STORE
    bool clear_pending = false;
    uint64_t clears_stored = 0, clears_materialised = 0;   // how the recorded clears ended (rt_accum_store_stats)
    uint32_t sample_counter = 0;
    bool count_enabled = false;

    // adaptive sampling (rt_render_adaptive), made whole on its first call and when the blocks outgrow them: reset by
    // alloc_frame and by a failed allocation
    struct Adaptive {
        DevBuf<float4> scratch;         // W x H: the current round's sums (zero outside it)
        DevBuf<float4> half;            // W x H: the sums of the even rounds; made by the first call of the Dammertz rule
        DevBuf<uint32_t> block_active;  // per decision block: traced by the next round
        DevBuf<float> block_err;        // per decision block: its error after the last round it was traced in
        DevBuf<unsigned long long> stats;   // pt_adaptive_merge's counter rows (rt_amd.hip)
        DevBuf<float> m2_scratch;       // W x H: the current round's moments (zero outside it); only with RT_OPT_MOMENTS 1
        DevBuf<float> pixel_err;        // W x H: rt_render_adaptive_variance's pixel errors; made by the first call of that rule
        size_t block_capacity = 0;
        uint32_t blocks = 0;            // blocks of the last completed rt_render_adaptive call (0: none)
        bool variance = false;          // that call was of the variance rule: pixel_err describes the frame
    } adaptive;
    // first-hit features (rt_render_features), allocated on its first call: reset by alloc_frame
    struct Features {
        DevBuf<rt_feature> records;     // W x H
        bool ready = false;             // written since the frame was (re)allocated
        // rt_render_features_cameras, allocated on its first call: W x H x (hit share, dominant share) — two uint32 counts
        // between pt_features_cameras and its finishing pass, two floats after it
        DevBuf<float2> coverage;
        bool coverage_ready = false;    // `coverage` describes the records that lie in `records`
    } features;
    // denoiser (rt_denoise), allocated on its first call: reset by alloc_frame and by a failed allocation
    struct Denoise {
        DevBuf<float4> pingpong[2];     // W x H: the à-trous iterations' ping-pong buffers (linear colour, count)
        DevBuf<float4> out;             // W x H: the last rt_denoise result, gamma RGBA
        bool ready = false;             // written since the frame was (re)allocated
        // rt_denoise_variance, allocated on ITS first call (with the three above when rt_denoise has not run yet; its
        // iterations ping-pong (linear colour, variance) through `pingpong` and its result goes to `out`)
        DevBuf<float> var[2];           // W x H each: v0 (the 7x7 estimate) and v(L) (the filtered variance)
        bool var_ready = false;         // both written since the frame was (re)allocated
    } denoise;

    // per-pixel sample moments (RT_OPT_MOMENTS): the centred second moment of every pixel's sample luminances, kept beside
    // the accumulator by every call that adds to it (pt_moments.hpp).  Allocated by the first rt_clear / rt_render_adaptive
    // with the option on; reset by alloc_frame.  `valid`: zeroed together with the accumulator and updated by every launch
    // since — set by rt_clear and rt_render_adaptive while the option is 1, dropped when the option's value changes and
    // by alloc_frame.  While it is false every launch gets a NULL moment pointer and nothing writes the buffer.
    struct Moments {
        bool on = false;
        bool valid = false;
        DevBuf<float> m2;               // W x H
        float *target() const { return on && valid ? m2.p : nullptr; }   // what a launch that adds to `accum` updates
    } moments;

    // Per-sample camera blocks (rt_render_spp_cameras), made whole by the first such call and freed with the context.
    // "Host pointer, copied at the call", and the call is asynchronous: a launch's blocks go through a table of their own in
    // a ring of RING tables of RT_SPP_PER_LAUNCH blocks each — copied into the PINNED host table k at the call, from there
    // to device table k on the stream, read by the launch's kernels, `read[k]` recorded behind them.  A launch that comes
    // round to table k again waits (on the host) for read[k] first: four launches of 512 samples per pixel ahead of the
    // device, which no caller reaches with the stream busy for milliseconds per launch.
    struct Cameras {
        static constexpr uint32_t RING = 4;
        DevBuf<float> table;            // RING x RT_SPP_PER_LAUNCH x 12 floats
        float *h_table = nullptr;       // pinned, the same shape
        hipEvent_t read[RING] = {};
        uint64_t launches = 0;          // launches that took a table (the next one takes table launches % RING)
        // what the last launch was chosen from and what was chosen (plan_camera_samples, pt_kernels.hip); block_size 0: no
        // launch yet (rt_debug_last_camera_plan)
        rt_camera_facts last_facts = {};
        rt_camera_plan last_plan = {};
    } cameras;

    // Caller-supplied rays (rt_upload_rays, rt_render_rays): the context's own ray buffer — `count` rays uploaded, room for
    // buf.n; grown on demand (the old array is freed by DevBuf, which waits for the device), never touched by alloc_frame or
    // rt_set_scene: rays belong to neither a frame size nor a scene — freed with the context.
    struct Rays {
        DevBuf<rt_ray> buf;
        size_t count = 0;
        // what the last ray launch was chosen from and what was chosen (plan_camera_samples with n = the range's rays);
        // block_size 0: no launch yet (rt_debug_last_ray_plan)
        rt_camera_facts last_facts = {};
        rt_camera_plan last_plan = {};
    } rays;

    int rank = 0, world = 1, tile_w_log2 = 3, tile_h_log2 = 3;
    uint32_t max_threads_per_launch = 1u << 30;
};

namespace rtamd {
using namespace pt;

// records the message on the context (or, for ctx == nullptr, as the last rt_create failure) and returns `code`
int fail(rt_context *ctx, int code, const char *fmt, ...);
// Copies the `need` bytes of device buffer `src` into the caller's `dst` of `bytes` bytes and waits for them: EINVAL
// unless the sizes match, then ESTATE unless `src` is `ready` (written by a `producer` call since the frame was made).
int read_back(rt_context *ctx, void *dst, size_t bytes, const void *src, size_t need, const char *what, bool ready = true,
              const char *producer = nullptr);

#define HIP_TRY(ctx, expr)                                                                        \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail(ctx, RT_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// The pending rt_clear, enqueued now (rt_context::clear_pending): the memset rt_clear enqueues under RT_OPT_ACCUM_STORE 0, on
// the context's stream, in front of whatever the caller is about to enqueue or wait for.
inline int materialise_clear(rt_context *ctx) {
    if (!ctx->clear_pending) return RT_OK;
    HIP_TRY(ctx, hipMemsetAsync(ctx->accum.p, 0, (size_t)ctx->width * ctx->height * sizeof(float4), ctx->stream));
    ctx->clear_pending = false;
    ctx->clears_materialised++;
    return RT_OK;
}
// every wait for the context's stream: a pending clear is ordered before it returns
inline int sync_stream(rt_context *ctx) {
    const int rc = materialise_clear(ctx);
    if (rc != RT_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}
#define SYNC_TRY(ctx)                         \
    do {                                      \
        const int rc_ = sync_stream(ctx);     \
        if (rc_ != RT_OK) return rc_;         \
    } while (0)
#define CLEAR_TRY(ctx)                        \
    do {                                      \
        const int rc_ = materialise_clear(ctx); \
        if (rc_ != RT_OK) return rc_;         \
    } while (0)

inline DeviceScene device_scene(const rt_context *ctx) {
    DeviceScene s;
    s.materials = ctx->materials.p;
    s.spheres = ctx->spheres.p;
    s.sph4 = ctx->sph4.p;
    s.sphere_batches = ctx->sphere_batches;
    s.material_count = (uint32_t)ctx->materials.n;
    s.faces = ctx->faces.p;
    s.mesh_face_base = ctx->mesh_face_base.p;
    s.mbvh_nodes = ctx->mbvh_nodes.p;
    s.mbvh_faces = ctx->mbvh_faces.p;
    s.mbvh_face_idx = ctx->mbvh_face_idx.p;
    s.mesh_bvh_root = (ctx->have_mesh_bvh && ctx->accel != 0) ? ctx->mesh_bvh_root.p : nullptr;
    bool use_bvh = ctx->bvh_node_count && (ctx->accel == 2 || (ctx->accel == 1 && ctx->spheres.n >= ACCEL_MIN_SPHERES));
    s.bvh_nodes = ctx->bvh_nodes.p;
    s.bvh_sph = ctx->bvh_sph.p;
    s.bvh_idx = ctx->bvh_idx.p;
    s.bvh_links = ctx->bvh_links.p;
    s.bvh_node_count = use_bvh ? ctx->bvh_node_count : 0;
    for (int k = 0; k < 3; k++) { s.bvh_lo[k] = ctx->bvh_lo[k]; s.bvh_hi[k] = ctx->bvh_hi[k]; }
    s.bvh_rmax = ctx->bvh_rmax;
    s.walk_overflow = ctx->d_walk_overflow;
    s.planes = ctx->planes.p;
    s.lenses = ctx->lenses.p;
    s.vertices = ctx->vertices.p;
    s.uvs = ctx->uvs.p;
    s.indices = ctx->indices.p;
    s.meshes = ctx->meshes.p;
    s.models = ctx->models.p;
    s.table = ctx->table.p;
    s.tex = ctx->tex.p;
    s.tex_w = ctx->tex_w;
    s.tex_h = ctx->tex_h;
    s.tex_layers = ctx->tex_layers;
    s.tex_wf = (float)ctx->tex_w;
    s.tex_hf = (float)ctx->tex_h;
    s.sphere_count = (uint32_t)ctx->spheres.n;
    s.plane_count = (uint32_t)ctx->planes.n;
    s.lens_count = (uint32_t)ctx->lenses.n;
    s.model_count = (uint32_t)ctx->models.n;
    return s;
}

struct Shard {
    uint32_t tiles_x, tiles_total, owned_tiles, slots;
};
inline Shard shard_of(const rt_context *ctx, int rank, int world) {
    Shard s;
    uint32_t tw = 1u << ctx->tile_w_log2, th = 1u << ctx->tile_h_log2;
    s.tiles_x = (ctx->width + tw - 1) / tw;
    uint32_t tiles_y = (ctx->height + th - 1) / th;
    s.tiles_total = s.tiles_x * tiles_y;
    s.owned_tiles = s.tiles_total > (uint32_t)rank ? (s.tiles_total - rank + world - 1) / world : 0;
    s.slots = s.owned_tiles * tw * th;
    return s;
}

// frame parameters for the shard (rank of world); rank < 0 → the context's own shard
inline FrameParams frame_params(const rt_context *ctx, const float cam[12], uint32_t first, uint32_t count, uint32_t glog2,
                         int rank = -1, int world = 1) {
    if (rank < 0) { rank = ctx->rank; world = ctx->world; }
    FrameParams fp;
    memcpy(fp.cam, cam, sizeof fp.cam);
    Shard sh = shard_of(ctx, rank, world);
    fp.w = ctx->width;
    fp.h = ctx->height;
    fp.tile_w_log2 = ctx->tile_w_log2;
    fp.tile_h_log2 = ctx->tile_h_log2;
    fp.tiles_x = sh.tiles_x;
    fp.tiles_total = sh.tiles_total;
    fp.rank = (uint32_t)rank;
    fp.world = (uint32_t)world;
    fp.slot_begin = 0;
    fp.slot_end = sh.slots;
    fp.first = first;
    fp.count = count;
    fp.group_log2 = glog2;
    fp.seg_cap = 0;
    fp.store = 0;
    fp.trees = nullptr;
    fp.tree_wait = nullptr;
    fp.tree_count = nullptr;
    fp.tree_cap = 0;
    fp.lds_face_f4 = 0;
    fp.block_active = nullptr;
    fp.blk_w_log2 = fp.blk_h_log2 = 0;
    fp.blocks_x = 0;
    fp.la_ring = nullptr;
    fp.la_image = nullptr;
    fp.m2 = nullptr;
    {
        volatile float c = (float)count;
        volatile float q = 1.0f / c;
        fp.inv_count = count ? q : 0.0f;
    }
    return fp;
}

inline void apply_mask(FrameParams &fp, const BlockMask *mask) {
    if (!mask) return;
    fp.block_active = mask->active;
    fp.blk_w_log2 = mask->w_log2;
    fp.blk_h_log2 = mask->h_log2;
    fp.blocks_x = mask->blocks_x;
}

// kernels come in (COUNT, ACCEL) instantiations; scenes without any BVH run the ACCEL = false ones
inline bool scene_has_accel(const DeviceScene &sc) { return sc.bvh_node_count != 0 || sc.mesh_bvh_root != nullptr; }

inline int ensure_slots(rt_context *ctx, size_t slots) {
    rt_context::Slots &s = ctx->slots;
    if (slots <= s.capacity) return RT_OK;
    s = {};
    ctx->prefix_changed();
    // live list: whole pt_prefix workgroups' worth of entries, then the block of counters
    size_t entries = slots + 256u;
    HIP_TRY(ctx, s.recs.alloc(entries));
    HIP_TRY(ctx, s.live.alloc(entries + LIVE_COUNT_STRIDE));
    HIP_TRY(ctx, s.finals.alloc(entries));
    HIP_TRY(ctx, s.final_n.alloc(entries / 256u + 1u));
    // decision trees for a quarter of the slots (a frame with more dielectric-first pixels keeps plain records for the rest)
    const size_t trees = slots / 4 + 256;
    if (s.trees.alloc(trees) == hipSuccess && s.tree_wait.alloc(trees * PT_TREE_WAITS) == hipSuccess) {
        s.tree_capacity = trees;
    } else {   // not fatal: the frame renders without shared trees
        (void)hipGetLastError();
        s.trees.release();
        s.tree_wait.release();
    }
    s.capacity = slots;
    return RT_OK;
}

// ---- steps of the fused launch that are the same under every policy (launch_fused_any, pt_kernels.hip) ------------------
// What plan_samples reads, for the slot range fp holds.  exact: the host knows the live list's counters.
inline rt_sample_facts sample_facts(const rt_context *ctx, const DeviceScene &sc, const FrameParams &fp, bool exact) {
    rt_sample_facts f = {};
    f.count = fp.count;
    f.glog2 = fp.group_log2;
    f.n = fp.slot_end - fp.slot_begin;
    f.seg_cap = fp.seg_cap;
    f.material_count = sc.material_count;
    f.sphere_count = sc.sphere_count;
    f.plane_count = sc.plane_count;
    f.lens_count = sc.lens_count;
    f.model_count = sc.model_count;
    f.sphere_bvh = sc.bvh_node_count != 0;
    f.mesh_bvh = sc.mesh_bvh_root != nullptr;
    f.walk_jobs = (uint32_t)ctx->walk_jobs.n;
    f.faces = ctx->h_faces.empty() ? 0u : (uint32_t)(ctx->h_faces.size() / 3u - 1u);   // (the array ends with one dummy record)
    f.cu_count = ctx->cu_count > 0 ? (uint32_t)ctx->cu_count : 0u;
    f.count_enabled = ctx->count_enabled;
    f.sample_queue = ctx->sample_queue;
    f.walk_slices = ctx->walk_slices;
    f.wave_fill = ctx->wave_fill;
    f.moments = fp.m2 != nullptr;   // (the launch keeps the sample moments)
    f.exact = exact;
    f.count_light = exact ? ctx->prefix_cache.count_light : 0u;
    f.count_heavy = exact ? ctx->prefix_cache.count_heavy : 0u;
    return f;
}

// The prefix cache (rt_context::PrefixCache): is the last launch's pt_prefix still good for this one?  Until the launch has
// gone through (prefix_keep) the entry is invalid, so an error on the way leaves it so.
inline bool prefix_lookup(rt_context::PrefixCache &pc, bool keepable, bool tree_on, const uint32_t cam_bits[12]) {
    const bool hit = pc.enabled && pc.valid && keepable && pc.key_generation == pc.generation && pc.key_tree_on == tree_on &&
                     memcmp(pc.key_cam, cam_bits, sizeof pc.key_cam) == 0;
    pc.valid = false;
    return hit;
}

// the slot buffers hold this camera's whole prefix
inline void prefix_keep(rt_context::PrefixCache &pc, bool tree_on, const uint32_t cam_bits[12]) {
    pc.valid = true;
    pc.key_generation = pc.generation;
    pc.key_tree_on = tree_on;
    memcpy(pc.key_cam, cam_bits, sizeof pc.key_cam);
}

// The entry's live counters on the host (rt_context::PrefixCache, RT_OPT_EXACT_GRID): dropped with the entry by every
// launch that does not hit; learnt by an asynchronous copy that the FIRST hit enqueues and later hits only ask after.
// *exact: this launch may be sized by them.
inline int learn_live_counts(rt_context *ctx, bool hit, const uint32_t *live_count, bool *exact) {
    using PC = rt_context::PrefixCache;
    PC &pc = ctx->prefix_cache;
    rt_context::SampleGrid &sg = ctx->sample_grid;
    *exact = false;
    if (!hit) pc.counts_state = PC::COUNTS_UNKNOWN;
    else if (sg.exact && pc.counts_state == PC::COUNTS_UNKNOWN) {
        HIP_TRY(ctx, hipMemcpyAsync(sg.h_counts, live_count, LIVE_COUNT_STRIDE * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(sg.counts_ev, ctx->stream));
        pc.counts_state = PC::COUNTS_IN_FLIGHT;
    } else if (sg.exact && pc.counts_state == PC::COUNTS_IN_FLIGHT) {
        const hipError_t q = hipEventQuery(sg.counts_ev);
        if (q == hipSuccess) {
            pc.count_light = sg.h_counts[0];
            pc.count_heavy = sg.h_counts[LIVE_HEAVY_COUNTER];
            pc.counts_state = PC::COUNTS_KNOWN;
        } else {
            (void)hipGetLastError();   // (not ready is no error of this launch)
            if (q != hipErrorNotReady) return fail(ctx, RT_EHIP, "hipEventQuery: %s", hipGetErrorString(q));
        }
    }
    *exact = hit && sg.exact && pc.counts_state == PC::COUNTS_KNOWN;
    return RT_OK;
}

// What plan_camera_samples reads, for the slot range fp holds (rt_render_spp_cameras).
inline rt_camera_facts camera_facts(const rt_context *ctx, const DeviceScene &sc, const FrameParams &fp) {
    rt_camera_facts f = {};
    f.count = fp.count;
    f.glog2 = fp.group_log2;
    f.n = fp.slot_end - fp.slot_begin;
    f.material_count = sc.material_count;
    f.sphere_count = sc.sphere_count;
    f.plane_count = sc.plane_count;
    f.lens_count = sc.lens_count;
    f.model_count = sc.model_count;
    f.sphere_bvh = sc.bvh_node_count != 0;
    f.mesh_bvh = sc.mesh_bvh_root != nullptr;
    f.faces = ctx->h_faces.empty() ? 0u : (uint32_t)(ctx->h_faces.size() / 3u - 1u);   // (as sample_facts)
    f.cu_count = ctx->cu_count > 0 ? (uint32_t)ctx->cu_count : 0u;
    f.count_enabled = ctx->count_enabled;
    f.sample_queue = ctx->sample_queue;
    f.wave_fill = ctx->wave_fill;
    f.moments = fp.m2 != nullptr;
    return f;
}

inline uint32_t group_log2_for(uint32_t count) {
    uint32_t g = 0;
    while ((1u << g) < count && g < 6) g++;
    return g;
}

}  // namespace rtamd
