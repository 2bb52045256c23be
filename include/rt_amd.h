/*
 * rt_amd.h — C ABI of the MI355X (gfx950) path tracer: librt_amd.so.
 *
 * This is the drop-in boundary for ONE hot path of antoni-wojcik/OpenCL-Raytracing:
 * the per-pixel Monte-Carlo trace loop (kernels `trace` / `retrace`,
 * kernels/raytracer.cl:496-532 and everything they reach, :93-494).  The
 * reference has no FFI layer; its boundary is the C++ class API
 * (include/raytracer.h:17-47, include/scene.h:83-153, include/camera.h:20-53)
 * plus the OpenCL kernel argument lists (src/raytracer.cpp:108-121,
 * src/scene.cpp:89-108).  Every entry point below names the reference
 * interface it replaces.  Plain pointers and sizes only: no C++ types, no
 * torch types.  All file:line citations are relative to the reference repo.
 *
 * Conventions
 *   - every function returns 0 on success, a negative RT_E* code on failure;
 *     rt_last_error() gives the message (reference: print + exit(-1),
 *     src/kernelgl.cpp:47-56, src/scene.cpp:29-32);
 *   - calls on one context must be serialised by the caller (reference: single
 *     GL thread, src/raytracer.cpp:134-140);
 *   - host arrays are copied at the call, the caller keeps ownership;
 *   - "device" pointers are HIP device addresses of the context's GPU;
 *   - the library never falls back to a CPU path: without a usable gfx950
 *     device rt_create() fails with RT_ENODEVICE.
 */
#ifndef RT_AMD_H
#define RT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 3

/* error codes */
#define RT_OK 0
#define RT_EINVAL (-1)    /* bad argument                                    */
#define RT_ENODEVICE (-2) /* no HIP device / wrong architecture              */
#define RT_EHIP (-3)      /* a HIP runtime call failed                       */
#define RT_ESTATE (-4)    /* call order violated (e.g. render before scene)  */
#define RT_ERANGE (-5)    /* index inside the scene points outside an array  */

/* kernel constants, kernels/raytracer.cl:1-7 (duplicated src/raytracer.cpp:21) */
#define RT_TRIANGLE_EPSILON 0.0000001f
#define RT_MIN_DISTANCE 0.001f
#define RT_MAX_DISTANCE 1000.0f
#define RT_DEPTH 30
#define RT_RANDOM_BUFFER_SIZE 100000
#define RT_RANDOM_TABLE_FLOATS (4 * RT_RANDOM_BUFFER_SIZE)

/* API limits: keep the 64-bit table index of raytracer.cl:115,122 below 2^32 */
#define RT_MAX_DIM 16384
#define RT_MAX_SAMPLE 65535u

/* ---- device data layouts (byte-identical to the reference's structs) ---- */

/* cl_float3 / OpenCL float3: 16 bytes, align 16 (include/scene.h:34,42,...) */
typedef struct rt_float3 { float x, y, z, w; } rt_float3;
typedef struct rt_float2 { float x, y; } rt_float2;

/* enum MatType, kernels/raytracer.cl:23, include/scene.h:30 */
enum rt_mat_type {
    RT_REFRACTIVE = 0,
    RT_REFLECTIVE = 1,
    RT_DIELECTRIC = 2,
    RT_DIFFUSE = 3,
    RT_TEXTURED = 4,
    RT_LIGHT = 5
};

/* Material, raytracer.cl:25-29 / scene.h:32-39 — 48 bytes */
typedef struct rt_material {
    int32_t type;
    int32_t _pad0[3];
    rt_float3 color;
    float extra_data;
    int32_t _pad1[3];
} rt_material;

/* Sphere, raytracer.cl:40-44 / scene.h:41-47 — 32 bytes */
typedef struct rt_sphere {
    rt_float3 pos;
    float r;
    uint32_t mat_ID;
    uint32_t _pad[2];
} rt_sphere;

/* Plane, raytracer.cl:46-50 / scene.h:49-55 — 48 bytes */
typedef struct rt_plane {
    rt_float3 pos;
    rt_float3 normal;
    uint32_t mat_ID;
    uint32_t _pad[3];
} rt_plane;

/* Lens, raytracer.cl:52-59 / scene.h:57-64 — 64 bytes */
typedef struct rt_lens {
    rt_float3 pos;
    rt_float3 p1;
    rt_float3 p2;
    float r1;
    float r2;
    uint32_t mat_ID;
    uint32_t _pad;
} rt_lens;

/* Mesh, raytracer.cl:61-66 / scene.h:66-73 — 16 bytes */
typedef struct rt_mesh {
    uint32_t vertex_anchor;
    uint32_t index_anchor;
    uint32_t face_count;
    uint32_t texture_ID;
} rt_mesh;

/* Model, raytracer.cl:68-72 / scene.h:75-81 — 12 bytes */
typedef struct rt_model {
    uint32_t mesh_anchor;
    uint32_t mesh_count;
    uint32_t mat_ID;
} rt_model;

/*
 * The nine arrays + counts the kernel reads: Scene, raytracer.cl:74-91, filled
 * by createScene (:541-558) from SceneCreator::setKernelArgs (src/scene.cpp:89-108).
 * The uv array is indexed with the vertex index (raytracer.cl:97-99): uv_count
 * must be 0 or equal to vertex_count (a short uv array is zero-filled on upload).
 */
typedef struct rt_scene_desc {
    const rt_material *materials;
    const rt_sphere *spheres;
    const rt_plane *planes;
    const rt_lens *lenses;
    const rt_float3 *vertices;
    const rt_float2 *uvs;
    const uint32_t *indices;
    const rt_mesh *meshes;
    const rt_model *models;
    uint32_t material_count;
    uint32_t sphere_count;
    uint32_t plane_count;
    uint32_t lens_count;
    uint32_t vertex_count;
    uint32_t uv_count;
    uint32_t index_count;
    uint32_t mesh_count;
    uint32_t model_count;
    uint32_t _pad;
} rt_scene_desc;

/*
 * Work counters of one render call (data dependent, exact, deterministic).
 * They price the reference kernel's logical global-memory traffic
 * (SURVEY §8d "algorithmic bytes"); see rt_counters_bytes().
 */
typedef struct rt_counters {
    uint64_t samples;       /* pixel-samples traced (camera block 48 B, image write 16 B) */
    uint64_t bounces;       /* hitScene calls, raytracer.cl:449                          */
    uint64_t t_sphere;      /* hitSphere calls  (32 B each)                              */
    uint64_t t_plane;       /* hitPlane calls   (48 B)                                   */
    uint64_t t_lens;        /* hitLens calls    (64 B)                                   */
    uint64_t t_model;       /* hitModel calls   (12 B)                                   */
    uint64_t t_mesh;        /* hitMeshOut calls (16 B)                                   */
    uint64_t t_tri;         /* hitTriangle calls (3 idx + 3 vtx = 60 B)                  */
    uint64_t h_tri;         /* triangle hits reaching the uv fetch :281 (36 B)           */
    uint64_t h_bounce;      /* bounces that hit something (material 48 B)                */
    uint64_t n_scatter;     /* randomVec table reads :113 (12 B)                         */
    uint64_t n_dielectric;  /* random() table reads :120 (4 B)                           */
    uint64_t n_texfetch;    /* bilinear texture fetches :105 (4 texels x 16 B)           */
    uint64_t image_reads;   /* retrace read of the previous pixel :524 (16 B)            */
} rt_counters;

typedef struct rt_context rt_context;

/* ---- lifetime ------------------------------------------------------------ */

/* ABI version of the loaded library (== RT_ABI_VERSION it was built with). */
int rt_abi_version(void);

/* Message of the last failure on ctx (or of the last failed rt_create when
 * ctx is NULL).  Replaces KernelGL::processError, src/kernelgl.cpp:47-56. */
const char *rt_last_error(const rt_context *ctx);

/* Replaces RayTracer::RayTracer(w,h,kernel_path) minus scene loading
 * (src/raytracer.cpp:24-36) and KernelGL::initialiseOpenCL
 * (src/kernelgl.cpp:58-93).  `device` is a HIP ordinal (the reference
 * hard-wires OpenCL GPU index 1, kernelgl.cpp:76).  Allocates the W×H RGBA32F
 * image (raytracer.cpp:54,60), the 12-float camera block (:64-65) and the
 * 400 000-float random table (:69-93, seeded as rt_set_seed(ctx, 0xC0FFEE)). */
int rt_create(int device, int width, int height, rt_context **out);

/* Replaces RayTracer::~RayTracer (src/raytracer.cpp:38-40). */
void rt_destroy(rt_context *ctx);

/* RayTracer::resize — declared, never defined (include/raytracer.h:46).
 * Reallocates the image; resets the sample counter. */
int rt_resize(rt_context *ctx, int width, int height);

/* Run on this hipStream_t (0 = the context's own stream).  The reference
 * creates a fresh cl::CommandQueue per call (src/raytracer.cpp:134). */
int rt_set_stream(rt_context *ctx, void *hip_stream);

/* ---- inputs -------------------------------------------------------------- */

/* Replaces SceneCreator::setupBuffers/createScene/setKernelArgs
 * (src/scene.cpp:46-108) and the createScene kernel (raytracer.cl:541-558).
 * Validates every index the kernel would dereference (RT_ERANGE). */
int rt_set_scene(rt_context *ctx, const rt_scene_desc *scene);

/* Replaces SceneCreator::loadTextures' upload (src/scene.cpp:164,173): `layers`
 * RGBA32F images of w×h texels, layer-major.  layers==0 installs the 1×1×1
 * dummy the reference creates for model-free scenes (scene.cpp:187-189). */
int rt_set_textures(rt_context *ctx, const float *rgba, int w, int h, int layers);

/* Replaces the random-table fill of RayTracer::createCLBuffers
 * (src/raytracer.cpp:69-93), which is unseeded (std::random_device).  The
 * table has the same layout and distribution (100 000 points uniform in the
 * unit ball, then 100 000 U[0,1)) but is a pure function of `seed`
 * (Philox-4x32-10; DESIGN.md "random table"). */
int rt_set_seed(rt_context *ctx, uint64_t seed);

/* Inject a caller-made table (n must be RT_RANDOM_TABLE_FLOATS). */
int rt_set_random_table(rt_context *ctx, const float *table, size_t n);

/* Copy the table currently on the device to `out` (n floats). */
int rt_get_random_table(rt_context *ctx, float *out, size_t n);

/* Host-only: fill `out[400000]` with the table rt_set_seed(seed) would
 * upload.  Needs no device and no context. */
int rt_make_random_table(uint64_t seed, float *out, size_t n);

/*
 * Frame sharding for multi-GPU rendering (new; the reference is single
 * device, src/kernelgl.cpp:76).  The frame is cut into tile_w×tile_h tiles,
 * numbered row-major; this context renders tiles t with t % world == rank
 * and leaves every other pixel of its buffers at zero, so an element-wise
 * sum over ranks (RCCL reduce) is the full frame.  Pixels keep their
 * whole-frame coordinates (they enter the table index, raytracer.cl:115,122),
 * so every pixel is bit-identical to the unsharded render.
 * Default: rank 0 of 1, 64×4 tiles.
 */
int rt_set_shard(rt_context *ctx, int rank, int world, int tile_w, int tile_h);

/* Compact exchange of a sharded accumulator (new).  rt_shard_slots: number of pixel
 * slots every rank of `world` packs (whole tiles, the same for all ranks).
 * rt_pack_accum: this rank's owned accumulator pixels → d_packed (device, slots × 16 B,
 * slot order).  rt_unpack_accum: scatter the packed pixels of rank `src_rank` of
 * `world` into this context's accumulator.  gather(packed) + unpack on rank 0 moves
 * 1/world of the frame per rank over xGMI instead of a full-frame reduce. */
int rt_shard_slots(rt_context *ctx, int world, uint32_t *slots_out);
int rt_pack_accum(rt_context *ctx, void *d_packed, size_t bytes);
int rt_unpack_accum(rt_context *ctx, const void *d_packed, size_t bytes, int src_rank, int world);

/* ---- rendering ----------------------------------------------------------- */

/* Replaces RayTracer::render (src/raytracer.cpp:127-144) + kernel `trace`
 * (raytracer.cl:496-510): sample_counter = 0; image = sqrt(getCol(sample 0)). */
int rt_render(rt_context *ctx, const float camera[12]);

/* Replaces RayTracer::renderAgain (src/raytracer.cpp:146-165) + kernel
 * `retrace` (raytracer.cl:512-532): ++sample_counter; running mean kept in
 * gamma space, bit-identical to the reference's arithmetic.
 * Synchronous; when it returns, the image (rt_device_image, rt_read_image) is the
 * image after that sample and the accumulator is untouched.  While the calls repeat
 * one camera block, RT_OPT_LOOKAHEAD lets ONE fused launch compute the images after
 * the next K samples; the calls then hand them out, bit for bit what the direct
 * kernel would have written (see the option). */
int rt_render_again(rt_context *ctx, const float camera[12]);

/* Value of RayTracer::sample_counter (include/raytracer.h:21). */
int rt_sample_counter(const rt_context *ctx, uint32_t *out);

/*
 * Native fused path (new): samples first_sample .. first_sample+n-1 of every
 * owned pixel in ONE launch, each sample bit-identical to what `trace` /
 * `retrace` would have traced, summed per pixel in linear space in a fixed
 * order, added to the linear accumulator (RGB sum, and the sample count in the
 * 4th channel, so accumulators of several ranks can simply be summed).
 * rt_clear() zeroes it; rt_resolve() writes image = sqrt(sum / count), alpha 1.
 * 64 spp: rt_clear; rt_render_spp(cam, 0, 64); rt_resolve.
 * A call of more than 512 samples per pixel is executed as consecutive launches of 512 (the accumulator is the sum of
 * their sums; results within a launch are summed in a fixed order).
 * WHEN the clear happens (RT_OPT_ACCUM_STORE 1, the default): rt_clear records it and returns.  The clear is ordered before
 * the work of the next library call on this context and before rt_sync returns — never later, possibly not sooner: a fused
 * rt_render_spp launch that writes every pixel of the frame stores its sums instead of adding them to zeros (the same bits),
 * and every other call, rt_device_accum and rt_sync included, enqueues the memset first.  A caller that works on the
 * accumulator through a pointer it obtained BEFORE the rt_clear, on the context's stream, calls rt_sync (or rt_device_accum
 * again) after the rt_clear first.
 */
int rt_clear(rt_context *ctx);
int rt_render_spp(rt_context *ctx, const float camera[12], uint32_t first_sample, uint32_t n_samples);
int rt_resolve(rt_context *ctx);

/*
 * Per-sample camera blocks (new): samples first_sample .. first_sample+n-1 of every owned pixel, sample first_sample+j
 * traced from cameras[12*j .. 12*j+11] (host pointer, copied at the call).  The reference's `retrace` takes a camera block
 * and a sample index per call and its host may move the camera between calls (src/raytracer.cpp:146-165), so this is, per
 * pixel-sample, what the reference computes — with the host's camera a function of the sample index: pixel jitter
 * (anti-aliasing), a lens (depth of field), a moving camera (motion blur).
 *   - Sample first_sample+j of pixel (x, y) is bit for bit the radiance rt_trace_samples returns for (block j, x, y,
 *     first_sample+j) under the selected arithmetic policy.
 *   - The samples of a pixel are summed in rt_render_spp's fixed order — lane l of the pixel's g lanes adds its samples
 *     l, l+g, ... one after the other, then the xor butterfly, g = 2^ceil(log2(min(n, 64))) — and the sum is added to the
 *     linear accumulator, the count to its 4th channel.  With n identical blocks the accumulator therefore equals
 *     rt_render_spp(block, first_sample, n)'s, bit for bit.
 *   - A call of more than 512 samples runs as consecutive launches of 512, as rt_render_spp's does.
 *   - Asynchronous on the context's stream.  The image, the sample counter, the feature records and pending look-ahead
 *     frames stay as they are, as under rt_render_spp; so does a kept prefix (RT_OPT_PREFIX_CACHE): these launches use none of
 *     its buffers.
 *   - Sharded contexts, RT_OPT_MOMENTS, enabled counters, RT_OPT_MAX_THREADS_PER_LAUNCH and RT_OPT_ACCEL are honoured as by
 *     rt_render_spp; no option changes a bit.  RT_OPT_PREFIX_SHARING, _TREE and _CACHE have nothing to act on: samples that
 *     look through different cameras share no path prefix.
 * RT_EINVAL: a NULL pointer, samples beyond RT_MAX_SAMPLE.  RT_ESTATE: no scene set.
 */
int rt_render_spp_cameras(rt_context *ctx, const float *cameras, uint32_t first_sample, uint32_t n_samples);

/*
 * Caller-supplied rays (new): paths that start at rays the caller computed — an equirectangular panorama, a fisheye or
 * orthographic view, a cube-map probe, a bake from surface points, a radiance query along arbitrary rays — instead of at a
 * pinhole camera block.
 *   o      the origin.
 *   d      the direction, used AS GIVEN and not normalised (the reference leaves refracted directions unnormalised too: the
 *          hit routines take any length).
 *   x, y   the ray's random stream: they take the values the pixel coordinates take in the table index.
 * The contract is stated for finite components, a non-zero d and x, y < RT_MAX_DIM.  The library does not validate device
 * data; every table index is reduced mod RT_RANDOM_BUFFER_SIZE in 32 bits, so any 32-bit id is memory-safe.
 */
typedef struct rt_ray {
    float o[3];
    uint32_t x;
    float d[3];
    uint32_t y;
}
#if defined(__GNUC__) || defined(__clang__)
__attribute__((aligned(16)))
#endif
rt_ray;

#define RT_MAX_RAYS (1u << 28)   /* rays of one rt_render_rays call */

/* Copies n rays (host pointer) into the context's own ray buffer, on the context's stream.  The buffer grows on demand and
 * survives rt_resize and a scene change.  RT_EINVAL: a NULL pointer, n 0 or above RT_MAX_RAYS. */
int rt_upload_rays(rt_context *ctx, const rt_ray *host, size_t n);
/* Device address of the uploaded rays and their count (NULL and 0 before the first upload). */
int rt_device_rays(rt_context *ctx, void **d_rays, size_t *n);

/*
 * Samples first_sample .. first_sample+n_samples-1 of ray i, for every i < n_rays.  d_rays: n_rays rt_ray records on the
 * device, 16-byte aligned (NULL: the uploaded rays, of which there must be at least n_rays); d_accum: n_rays x 4 floats on
 * the device (NULL: the context's accumulator, and then n_rays == W*H, ray i being pixel i, row-major).
 *   - Sample s of ray i is, bit for bit under the selected arithmetic policy, the radiance rt_trace_samples returns for a
 *     camera whose primary ray at pixel (x_i, y_i) has exactly these origin and direction bits.
 *   - The samples of a ray are summed in rt_render_spp's fixed order — lane l of the ray's g lanes adds its samples l, l+g, ...
 *     one after the other, then the xor butterfly — and the sum is ADDED to d_accum[i], the count to its 4th channel: the
 *     caller zeroes the buffer, consecutive calls add.  More than 512 samples run as launches of 512, as elsewhere.
 *   - Asynchronous on the context's stream (the caller orders its own writes of d_rays / d_accum before it).
 *   - With d_accum NULL rt_clear, rt_resolve, rt_read_image / rt_read_linear, the denoisers and RT_OPT_MOMENTS work on the frame
 *     unchanged; the sample moments are updated exactly as rt_render_spp_cameras updates them.  An external d_accum keeps none.
 *   - The image, the sample counter, the feature records, a kept prefix and pending look-ahead frames stay untouched, as
 *     under rt_render_spp_cameras.  Enabled counters, RT_OPT_SAMPLE_QUEUE, RT_OPT_ACCEL, RT_OPT_WAVE_FILL and
 *     RT_OPT_MAX_THREADS_PER_LAUNCH are honoured; none changes a bit.  The prefix options have nothing to act on.
 * RT_EINVAL: n_rays 0 or above RT_MAX_RAYS, samples beyond RT_MAX_SAMPLE, NULL d_rays with fewer than n_rays rays uploaded,
 * NULL d_accum with n_rays != W*H, a sharded context (the caller shards a batch itself).  RT_ESTATE: no scene set.  A failed
 * call changes nothing.
 */
int rt_render_rays(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t first_sample, uint32_t n_samples, void *d_accum);

/*
 * Ray sets (new): anti-aliasing and depth of field for caller-supplied rays — rt_render_rays with a SET of set_size records
 * per ray instead of one, so that every sample of a ray can have its own origin and direction (a jittered panorama, a lens
 * in front of a fisheye), as rt_render_spp_cameras gives every sample of a pinhole frame its own camera block.
 * d_rays: n_rays x set_size rt_ray records on the device, 16-byte aligned and RAY-MAJOR: the set of ray i is records
 * i*set_size .. i*set_size + set_size-1, and sample s (the absolute sample index) of ray i starts at record
 * i*set_size + (s mod set_size) — rt_render_again_cameras' cyclic rule, under which a call cut into launches needs no offset.
 * (Ray-major because the lanes of a queue refill hold consecutive samples of one ray: they read one contiguous stretch of
 * 32-byte records; sample-major they would stand n_rays * 32 bytes apart.)
 *   - Sample s of ray i is, bit for bit under the selected arithmetic policy, the radiance rt_render_rays traces for that
 *     single record at sample s: the record's own origin, its own direction used as given, its own (x, y) random-stream ids.
 *     Every record is a full rt_ray.
 *   - The samples of a ray are summed in rt_render_spp's fixed order and ADDED to d_accum[i], the count to its 4th channel
 *     (d_accum NULL: the context's accumulator, and then n_rays == W*H; rt_resolve, the three denoisers and RT_OPT_MOMENTS work
 *     unchanged).  More than 512 samples run as launches of 512.  So set_size 1 is rt_render_rays bit for bit, a set of
 *     identical records is too, and sets built from the primary rays of camera blocks are rt_render_spp_cameras of those blocks.
 *   - d_rays NULL: the uploaded records (rt_upload_rays), of which there must be at least n_rays*set_size.
 *   - Asynchronous on the context's stream.  The image, the sample counter, the feature records, a kept prefix and pending
 *     look-ahead frames stay untouched.  Counters, RT_OPT_SAMPLE_QUEUE, RT_OPT_ACCEL, RT_OPT_WAVE_FILL,
 *     RT_OPT_MAX_THREADS_PER_LAUNCH and RT_OPT_MOMENTS are honoured exactly as by rt_render_rays; none changes a bit.
 *   - Record addresses are formed in 64 bits.  rt_debug_last_ray_plan also reports these launches.
 *   - Memory: a record is 32 bytes, so 1080p x 16 records is 1.06 GB.  Calls add: a large sample count can be rendered in
 *     chunks over one reused buffer (refill it between the calls, in stream order).
 * RT_EINVAL: everything rt_render_rays refuses (a sharded context included), set_size 0 or above RT_RAY_SET_MAX,
 * n_rays*set_size above 2^31.  RT_ESTATE: no scene set.  A failed call changes nothing.
 */
#define RT_RAY_SET_MAX 4096u
int rt_render_ray_sets(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t set_size, uint32_t first_sample,
                       uint32_t n_samples, void *d_accum);

/*
 * Progressive anti-aliasing (new): rt_render_again through a CYCLIC SCHEDULE of camera blocks.  `cameras` is a host pointer to
 * n_cameras x 12 floats, copied during the call; the call that makes sample s = sample_counter + 1 looks through block
 * s mod n_cameras (a caller who starts with rt_render(ctx, cameras) has sample 0 through block 0).
 *   - The image, the sample counter and every other piece of state after the call are, bit for bit, what
 *     rt_render_again(ctx, cameras + 12 * (s % n_cameras)) leaves with RT_OPT_LOOKAHEAD 0.  Synchronous; one entry in the
 *     event history per call.  The accumulator, the feature records, the sample moments and a kept prefix stay untouched.
 *   - Look-ahead through the table: the context keeps a copy of the table of the previous rt_render_again_cameras call.  A
 *     call whose table equals it (n_cameras and every bit), with no batch pending and RT_OPT_LOOKAHEAD = K >= 2, traces the
 *     next K' = rt_lookahead_plan(w, h, K, sample_counter) samples in ONE camera launch — sample s + j through block
 *     (s + j) mod n_cameras — and leaves K' images in the ring; this call and the next K' - 1 equal calls hand them out as
 *     rt_render_again does.  The first call with a new table runs the direct kernel and is remembered, so a caller who
 *     changes the table on every call never pays for a batch.
 *   - Pending frames are dropped by everything that drops them for rt_render_again, by a table that differs in any bit or
 *     in n_cameras, and by a plain rt_render_again between two table calls; a pending plain batch is dropped by this call,
 *     and a plain rt_render_again that follows a table call repeats no plain call and runs direct.
 *   - The direct kernel (same bits) also runs with counters enabled, on a sharded context, with RT_OPT_SAMPLE_QUEUE 0, where
 *     RT_OPT_MAX_THREADS_PER_LAUNCH splits the frame into several slot ranges, and where K' < 2.  RT_OPT_PREFIX_SHARING does
 *     not matter (camera launches share no prefix), nor does RT_OPT_MOMENTS (the compat path keeps no moments).
 *   - rt_lookahead_stats counts these batches, served calls, direct calls and discarded frames with rt_render_again's.
 * RT_EINVAL: a NULL pointer, n_cameras 0 or above RT_AGAIN_CAMERAS_MAX, the sample counter at RT_MAX_SAMPLE.  RT_ESTATE: no
 * scene set.  A failed call changes nothing.
 */
#define RT_AGAIN_CAMERAS_MAX 4096u
int rt_render_again_cameras(rt_context *ctx, const float *cameras, uint32_t n_cameras);

/*
 * Adaptive sampling (new): render until every decision block of block_w x block_h pixels has converged.
 * Round k (k = 0, 1, ...) traces samples k*batch .. k*batch+c-1, c = min(batch, max_spp - k*batch), of every pixel of
 * a still-active block, so a pixel whose count is n holds exactly samples 0 .. n-1 and each round adds, bit for bit,
 * what rt_render_spp(cam, k*batch, c) would have added to it.  From round 1 on, with I the linear mean of all of a
 * pixel's samples and A the linear mean of its even rounds' samples (0, 2, 4, ...), the pixel's error is
 * e = (|I.r-A.r| + |I.g-A.g| + |I.b-A.b|) / sqrt(I.r + I.g + I.b) (0 when the root is 0) and a block's error is the
 * mean e of its in-frame pixels (Dammertz et al. 2010, computed in linear space).  A block stays active while its
 * count < min_spp, or while its error >= threshold and its count < max_spp.  The call is a self-contained
 * rt_clear + rounds + rt_resolve: the image and the linear accumulator (sample counts in its 4th channel) end in
 * the state those calls leave.  Synchronous (one counter is read back per round).  Unsharded contexts only.
 */
typedef struct rt_adaptive_params {
    uint32_t batch;      /* samples per pixel per round, 1 .. 512                                           */
    uint32_t min_spp;    /* every pixel gets at least this many: >= 2*batch, a multiple of batch             */
    uint32_t max_spp;    /* no pixel gets more: >= min_spp, <= RT_MAX_SAMPLE + 1                              */
    float threshold;     /* a block stops when its error is < threshold; 0 = never stop early                */
    uint32_t block_w, block_h; /* decision block: powers of two, 1 .. 256 (8 x 8 suggested)                  */
} rt_adaptive_params;

typedef struct rt_adaptive_stats {
    uint32_t rounds;            /* launches of the sample pipeline                                           */
    uint64_t pixel_samples;     /* sum of all per-pixel counts                                               */
    uint32_t blocks, blocks_at_max; /* blocks in the frame; blocks that reached max_spp unconverged          */
} rt_adaptive_stats;

int rt_render_adaptive(rt_context *ctx, const float camera[12], const rt_adaptive_params *p, rt_adaptive_stats *out);
/* Per-pixel sample counts (accum.w) of the accumulator: W*H uint32, row-major; bytes = W*H*4. */
int rt_read_sample_counts(rt_context *ctx, uint32_t *counts, size_t bytes);
/* Block errors of the last adaptive call (of either stopping rule), ceil(W/block_w) * ceil(H/block_h) floats, row-major; a block
 * holds its error after the last round it was traced in.  RT_ESTATE before the first call / after rt_resize. */
int rt_read_block_error(rt_context *ctx, float *err, size_t bytes);

/*
 * Adaptive sampling through per-sample camera blocks (new): rt_render_adaptive for anti-aliased, defocused or moving
 * frames.  `cameras` is a host pointer to n_cameras x 12 floats, copied during the call; n_cameras must equal
 * p->max_spp: block j is the camera of sample j.  Round k traces samples k*batch .. k*batch+c-1 of every pixel of a
 * still-active block through blocks k*batch .. k*batch+c-1, so a pixel whose count is n holds exactly samples 0 .. n-1
 * through blocks 0 .. n-1 and each round adds, bit for bit, what rt_render_spp_cameras(cameras + 12*k*batch, k*batch, c)
 * would have added to it.
 *   - Parameters, estimator, stopping rule, rt_adaptive_stats, rt_read_sample_counts and rt_read_block_error are
 *     rt_render_adaptive's.  With max_spp identical blocks the accumulator, the counts, the block errors and the stats
 *     therefore equal rt_render_adaptive(block, p)'s, bit for bit.
 *   - A self-contained clear + rounds + resolve like rt_render_adaptive: synchronous, unsharded contexts only; it starts the
 *     sample moments when RT_OPT_MOMENTS is 1 and drops pending look-ahead frames.  The feature records and a kept prefix
 *     (RT_OPT_PREFIX_CACHE) stay as they are: camera launches use none of the prefix buffers.
 *   - Options as under rt_render_spp_cameras, none changes a bit: RT_OPT_SAMPLE_QUEUE 0, enabled counters and RT_OPT_MOMENTS 1
 *     run the fixed-lane camera kernel; RT_OPT_ACCEL, RT_OPT_WAVE_FILL and RT_OPT_MAX_THREADS_PER_LAUNCH are honoured.
 * RT_EINVAL: what rt_render_adaptive gives, a NULL `cameras`, n_cameras != max_spp.  RT_ESTATE: no scene set.  A failed
 * call changes nothing.
 */
int rt_render_adaptive_cameras(rt_context *ctx, const float *cameras, uint32_t n_cameras, const rt_adaptive_params *p,
                               rt_adaptive_stats *out);

/*
 * Adaptive sampling with a stopping rule driven by MEASURED variance (new): rt_render_adaptive and
 * rt_render_adaptive_cameras with the standard error of every pixel's mean, taken from the sample moments, in place of the
 * half-buffer estimate.  RT_OPT_MOMENTS must be 1: the calls do not switch it on.
 *   - The rounds are rt_render_adaptive's (rt_render_adaptive_cameras' for the cameras form, n_cameras == max_spp): round
 *     k traces samples k*batch .. k*batch+c-1 of every pixel of a still-active block, so every pixel holds, bit for bit,
 *     the accumulator of the fixed-count frame with its own count.  A self-contained clear + rounds + resolve, synchronous,
 *     unsharded contexts only; rt_adaptive_stats means the same; rt_read_sample_counts and rt_read_block_error serve it.
 *   - Estimator.  After a round, for a pixel with n = accum.w samples, I = accum.rgb / n, L = l(I) (the luminance of
 *     rt_denoise_variance) and M2 its merged moment (rt_moments_merge, taken in before the round's sums are added):
 *       e_p = sqrt(M2 / (n (n - 1))) / sqrt(L),   0 where n < 2, L <= 0 or M2 <= 0
 *     — the standard error of the pixel's mean luminance over the root of that mean.  By the delta method e_p / 2 is the
 *     standard error of the displayed (sqrt-space) luminance: that is what `threshold` means, and it does not depend on
 *     `batch`.  A block's error is the mean e_p of its in-frame pixels.  Division and square root are correctly rounded
 *     whatever the arithmetic policy.
 *   - A block stays active while its count < min_spp, or while (threshold == 0 or its error >= threshold) and its count <
 *     max_spp.  Decisions are taken from round 0 on.  The block errors and the pixel errors hold the values of the last
 *     round a block was traced in.
 *   - Parameters: batch 1 .. 512; min_spp a multiple of batch, >= batch and >= 2 (no half buffer exists, so there is no
 *     2 * batch rule); max_spp in min_spp .. RT_MAX_SAMPLE + 1; threshold finite and >= 0; blocks as rt_render_adaptive's.
 *   - Afterwards the moments are valid, so rt_denoise_moments can follow directly.  The half buffer of the Dammertz rule is
 *     neither read nor written, and a context that only ever uses this rule never allocates it.
 * rt_read_pixel_error: the W*H pixel errors, row-major; bytes = W*H*4.  rt_device_pixel_error: their device address.  Both
 * give RT_ESTATE unless the last completed adaptive call since the frame was (re)allocated was one of these two: a later
 * rt_render_adaptive / rt_render_adaptive_cameras or rt_resize invalidates them.
 * RT_ESTATE: RT_OPT_MOMENTS is 0; no scene set.  RT_EINVAL: everything else rt_render_adaptive / rt_render_adaptive_cameras
 * refuse, a sharded context included.  A failed call changes nothing.
 */
int rt_render_adaptive_variance(rt_context *ctx, const float camera[12], const rt_adaptive_params *p, rt_adaptive_stats *out);
int rt_render_adaptive_variance_cameras(rt_context *ctx, const float *cameras, uint32_t n_cameras,
                                        const rt_adaptive_params *p, rt_adaptive_stats *out);
int rt_read_pixel_error(rt_context *ctx, float *err, size_t bytes);      /* W*H floats, row-major */
int rt_device_pixel_error(rt_context *ctx, void **d_err);

/*
 * Adaptive sampling for caller-supplied rays (new): rt_render_adaptive and rt_render_adaptive_variance for frames made of
 * rays — a panorama, a fisheye or orthographic view, a cube-map face, a bake.  d_rays has the meaning it has in
 * rt_render_rays / rt_render_ray_sets: device memory, 16-byte aligned, or NULL for the uploaded records.  n_rays must equal
 * W*H: ray i is pixel (i mod W, i div W), the target is the context's accumulator, and the decision blocks are the frame's
 * block_w x block_h blocks exactly as for the camera calls.
 *   set_size 0                    one record per ray: the rounds run rt_render_rays' kernels.
 *   set_size 1 .. RT_RAY_SET_MAX  ray-major sets under rt_render_ray_sets' cyclic rule — sample s starts at record
 *                                 s mod set_size, so set_size and max_spp need no relation: rt_render_ray_sets' kernels.
 *   - Round k traces samples k*batch .. k*batch+c-1 of every pixel of a still-active block, and adds to it, bit for bit,
 *     what rt_render_rays(d_rays, n_rays, k*batch, c, NULL) / rt_render_ray_sets(d_rays, n_rays, set_size, k*batch, c, NULL)
 *     would add.  So a batch of a camera's own primary rays gives rt_render_adaptive's accumulator, counts, block errors,
 *     image and stats bit for bit, and sets built from camera blocks 0 .. max_spp-1 with set_size == max_spp give
 *     rt_render_adaptive_cameras'; the variance form equals its twins likewise, pixel errors included.
 *   - Parameters, estimators, stopping rules, rt_adaptive_stats, rt_read_sample_counts, rt_read_block_error and — for the
 *     variance form — rt_read_pixel_error / rt_device_pixel_error are those of the existing calls of the same rule.
 *   - A self-contained clear + rounds + resolve: synchronous, unsharded contexts only; it starts the sample moments when
 *     RT_OPT_MOMENTS is 1 and drops pending look-ahead frames.  The sample counter, the feature records, a kept prefix and
 *     the uploaded rays stay as they are.
 *   - Counters, RT_OPT_SAMPLE_QUEUE, RT_OPT_ACCEL, RT_OPT_WAVE_FILL and RT_OPT_MAX_THREADS_PER_LAUNCH are honoured as by
 *     rt_render_rays, none changes a bit; with RT_OPT_MOMENTS 1 (always, for the variance form) the launches run the
 *     fixed-lane ray kernels.  Only an owned ray of an active block is staged, traced, summed and counted.
 *     rt_debug_last_ray_plan reports the last round; plan and grid are those of the unmasked launch.
 * RT_EINVAL: what rt_render_adaptive refuses (a sharded context included) and what rt_render_rays / rt_render_ray_sets
 * refuse — n_rays != W*H, a misaligned d_rays, NULL d_rays with fewer than n_rays (x set_size) records uploaded, set_size
 * above RT_RAY_SET_MAX.  RT_ESTATE: no scene set; the variance form with RT_OPT_MOMENTS 0.  A failed call changes nothing.
 */
int rt_render_adaptive_rays(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t set_size, const rt_adaptive_params *p,
                            rt_adaptive_stats *out);
int rt_render_adaptive_variance_rays(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t set_size,
                                     const rt_adaptive_params *p, rt_adaptive_stats *out);

/*
 * First-hit feature buffers (new; the reference has no such entry point).  One record per pixel of the frame,
 * row-major W x H in the layout of rt_read_image: the pixel's primary ray (no jitter, raytracer.cl:500-505, so one
 * first hit per pixel) through the same nearest-hit search and winner rebuild as the trace kernels, under the
 * selected arithmetic policy — bit for bit what rt_debug_hit(kind 3) returns for (camera origin, dir).
 * On a miss: t = +inf, pos / normal / albedo 0, object and material 0xFFFFFFFF, face 0xFFFFFFFF, u = v = tex = 0,
 * flags 0; the direction is always written.  80 bytes, five 16-byte groups.
 */
typedef struct rt_feature {
    float pos[3];       /* hit point                                                                          */
    float t;            /* ray parameter of the nearest hit (+inf: miss)                                      */
    float normal[3];    /* the hit routine's normal, unchanged (not turned to face the ray)                   */
    uint32_t object;    /* kind in bits 31..30 (0 sphere, 1 plane, 2 lens, 3 mesh), index in bits 29..0      */
    float albedo[3];    /* material colour; for RT_TEXTURED the bilinear texel the path fetches at (u, v)      */
    uint32_t material;  /* mat_ID of the hit                                                                  */
    float dir[3];       /* primary ray direction, as the selected policy computes it                          */
    uint32_t face;      /* face index inside the mesh for a mesh hit, else 0xFFFFFFFF                         */
    float u, v;         /* texture coordinates (mesh hits; 0 otherwise)                                       */
    uint32_t tex;       /* texture id (mesh hits; 0 otherwise)                                                */
    uint32_t flags;     /* RT_FEATURE_HIT; after rt_render_features_chain also RT_FEATURE_CUT and the chain fields;
                           after rt_render_features_cameras also RT_FEATURE_MIXED                            */
} rt_feature;
#define RT_FEATURE_HIT 1u

/* Render the feature record of every pixel for `camera` (asynchronous on the context's stream; replaces the
 * previous features).  Leaves the image, the accumulator and the sample counter untouched.  Unsharded contexts only.
 * rt_read_features: bytes = W*H*80.  rt_device_features: the device address of the W x H records.  Both give
 * RT_ESTATE until rt_render_features has run since the frame was (re)allocated. */
int rt_render_features(rt_context *ctx, const float camera[12]);
int rt_read_features(rt_context *ctx, rt_feature *out, size_t bytes);
int rt_device_features(rt_context *ctx, void **d_features);

/*
 * Feature records that follow mirror and glass chains to the first rough hit (new).  The primary ray is not jittered
 * and reflective / refractive interactions draw no random number (raytracer.cl:362-391), so every pixel has ONE
 * deterministic chain.  Start with the primary ray:
 *   1. take the nearest hit (the search of rt_render_features);
 *   2. if the hit's material type is selected in `follow` and fewer than `max_chain` vertices have been followed so
 *      far, apply that material's interaction — the device's own scatter; a followed RT_DIELECTRIC goes through the
 *      RT_REFRACTIVE branch, i.e. rayRefract's rule: refract where the discriminant is > 0, else reflect, no random
 *      number — and continue from the hit point;
 *   3. otherwise that hit is the TERMINAL.  A miss ends the chain.
 * The result REPLACES the context's feature records, in the same layout, so rt_read_features, rt_device_features and
 * the three denoisers work on it unchanged:
 *   pos, normal, albedo, material, object, face, u, v, tex describe the terminal exactly as rt_render_features fills
 *     them for a first hit (the miss values on a terminal miss);
 *   t is the fp32 sum of the segments' t in path order ((t0 + t1) + t2 ...), +inf on a miss: hit == (t < inf) holds;
 *   dir stays the primary direction;
 *   flags: bit 0 RT_FEATURE_HIT (the terminal exists), bit 1 RT_FEATURE_CUT (the terminal has a followed type, but
 *     max_chain >= 1 vertices had been followed), bits 8..12 the number of followed vertices (RT_FEATURE_CHAIN_LENGTH),
 *     bits 16..31 the upper half of the chain signature (RT_FEATURE_CHAIN_SIGNATURE).
 * Signature: h = 0; for each followed vertex in path order h = (h ^ object) * 0x9E3779B1 (mod 2^32), `object` the id an
 * rt_feature record holds.  rt_feature_chain_signature is the very function the kernel calls (host-only, no context).
 * With follow == 0 or max_chain == 0 the records equal rt_render_features', bit for bit, flags included.
 * RT_EINVAL: unknown follow bits, max_chain > RT_FEATURE_CHAIN_MAX, a NULL pointer, a sharded context.  State rules,
 * asynchrony and what stays untouched: as rt_render_features.
 */
#define RT_FOLLOW_REFLECTIVE 1u
#define RT_FOLLOW_REFRACTIVE 2u
#define RT_FOLLOW_DIELECTRIC 4u   /* by rayRefract's rule: refract where the discriminant is > 0, else reflect; no random number */
#define RT_FEATURE_CHAIN_MAX 29u
#define RT_FEATURE_CUT 2u
#define RT_FEATURE_CHAIN_LENGTH(flags) (((flags) >> 8) & 31u)
#define RT_FEATURE_CHAIN_SIGNATURE(flags) ((flags) & 0xFFFF0000u)   /* == signature & 0xFFFF0000 */
typedef struct rt_feature_chain_params { uint32_t follow; uint32_t max_chain; } rt_feature_chain_params;
int rt_render_features_chain(rt_context *ctx, const float camera[12], const rt_feature_chain_params *p);

/*
 * Feature records for caller-supplied rays (new): the guides that belong to an rt_render_rays frame.  d_rays: n_rays == W*H
 * rt_ray records on the device (NULL: the uploaded rays), ray i being pixel i, row-major; p NULL = first hits.  Record i is,
 * bit for bit, what rt_render_features_chain writes for a camera whose primary ray at that pixel has these origin and
 * direction bits; `dir` is the direction as given.  The call replaces the context's feature records, so the denoisers work
 * on a panorama.  State rules and errors as rt_render_features_chain, plus RT_EINVAL for n_rays != W*H and for NULL d_rays
 * with fewer than n_rays rays uploaded.
 */
int rt_render_features_rays(rt_context *ctx, const void *d_rays, size_t n_rays, const rt_feature_chain_params *p);
int rt_feature_chain_signature(const uint32_t *objects, uint32_t n, uint32_t *sig_out);   /* host-only, no context */

/*
 * Ray queries (new): the two geometric questions beside the radiance query rt_render_rays — for bakes, pickers, visibility
 * passes.  Both are asynchronous on the context's stream and leave the context as it is: its feature records with their
 * ready and coverage state (on a fresh context rt_read_features is still RT_ESTATE afterwards), the image, the accumulator,
 * the sample counter, the moments, a kept prefix, pending look-ahead frames and the counters.  RT_ESTATE: no scene set.  A
 * failed call writes nothing.
 *
 * rt_intersect_rays: nearest hits for ANY batch.  Record i of d_out (n_rays rt_feature records on the device, 16-byte
 * aligned) is, bit for bit, the record rt_render_features_rays / rt_render_features_chain would write for ray i (p NULL =
 * first hits): the 80-byte layout, the miss values, the chain flags and `dir` as given.  n_rays: 1 .. RT_MAX_RAYS; d_rays
 * NULL = the uploaded rays, at least n_rays of them.  Record i depends on ray i only — not on its slot, its neighbours or
 * the length of the batch.  RT_EINVAL: a NULL ctx or d_out, a misaligned pointer, n_rays 0 or above RT_MAX_RAYS, NULL
 * d_rays with too few rays uploaded, unknown follow bits, max_chain above RT_FEATURE_CHAIN_MAX, a sharded context.
 */
int rt_intersect_rays(rt_context *ctx, const void *d_rays, size_t n_rays, const rt_feature_chain_params *p, void *d_out);

/*
 * rt_occluded_rays: occlusion (any hit).  d_rays: n_rays * set_size rt_ray records, ray-major as in rt_render_ray_sets — the
 * set of entry i is records i*set_size .. i*set_size + set_size-1; NULL = the uploaded records; set_size 1 ..
 * RT_RAY_SET_MAX, 1 being the plain per-ray query; the fields x, y of a record are not read.  With F(r) the first-hit record
 * rt_render_features_rays writes for r under the selected arithmetic policy (p NULL; F(r).t = +inf on a miss), record k
 * with bound b_k — d_tmax[k] (n_rays * set_size floats on the device), or t_max for every record where d_tmax is NULL —
 *   is occluded  iff  F(record k).t < b_k   in binary32.
 * A NaN bound, a bound <= RT_MIN_DISTANCE or a negative one never occludes; +inf asks for any hit; a hit at exactly b_k does
 * not occlude.  Directions are used as given, so t is in units of |d|; the guard against self-intersection is the hit
 * routines' own RT_MIN_DISTANCE.  The query is geometric: glass and lights occlude like anything else.
 * d_out[i] (n_rays uint32 on the device) = the number of occluded records of set i — 0 or 1 for set_size 1; OVERWRITTEN, not
 * added to.  The search stops at the first primitive that reports a t below min(b_k, RT_MAX_DISTANCE), which is exact: the
 * nearest hit is below the bound iff some sphere, plane, lens or mesh reports a t below it (a mesh reports its first
 * front-facing face in face order, as ever).  RT_OPT_ACCEL is honoured and changes no bit; rt_walk_overflow reports these
 * walks too.
 * RT_EINVAL: everything rt_render_ray_sets refuses for its ray arguments (n_rays 0 or above RT_MAX_RAYS, set_size 0 or above
 * RT_RAY_SET_MAX, n_rays * set_size above 2^31, a misaligned d_rays, too few uploaded records, a sharded context), a NULL
 * d_out, a d_out or d_tmax that is not 4-byte aligned.
 */
int rt_occluded_rays(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t set_size, const float *d_tmax, float t_max,
                     void *d_out);

/*
 * Hemisphere queries (new): ambient occlusion and visibility or irradiance bakes from hit points, with the rays made on the
 * device.  For each of the n rt_feature records at d_features (device, 16-byte aligned — typically rt_intersect_rays' output;
 * NULL: the context's own W*H records, RT_ESTATE while rt_read_features would be) the kernel makes p->k cosine-weighted
 * rays about the record's normal in registers and
 *   d_counts   (n uint32, OVERWRITTEN) receives the number of occluded rays among record i's k — or is NULL: no search runs
 *              (the spawn form);
 *   d_rays_out (n * k rt_ray records, ray-major, 16-byte aligned, OVERWRITTEN) receives the rays — ready for
 *              rt_render_ray_sets, rt_occluded_rays or any later query — or is NULL: no ray reaches memory (the fused form).
 * One of the two at least.  Record i is VALID when it has RT_FEATURE_HIT and the squared length of its normal is, in
 * binary32, a finite number above 0.  Ray t of a valid record:
 *   n^ = normal / |normal|, of -normal under RT_HEMI_FACE_FORWARD where dot(normal, record.dir) > 0;
 *   the tangent frame of rays::hemisphere_sets: axis = the world axis of the smallest |component| of the normal, ties to
 *     the lower index; tan = unit(n^ x axis), bit = n^ x tan;
 *   (u, v) = the first two 24-bit uniforms of Philox-4x32-10 on the counter (i*k + t, 0, 0, 0) with the key (seed lo, seed hi)
 *     (workloads.uniforms(n*k, 0, seed)[i*k + t, :2]);
 *   d = unit(sqrt(u) cos(2 pi v) tan + sqrt(u) sin(2 pi v) bit + sqrt(1 - u) n^),  o = pos + offset * n^,  x = i, y = 0
 * — Malley's method as host/rays.h states it, evaluated in binary32: a direction lies within 1e-6 per component of the
 * float64 generators' (measured: 1.8e-7, DESIGN.md "Hemisphere queries"), an origin within two roundings of pos + offset *
 * n^, and the rays are deterministic: the same call gives the same bytes.  An invalid record counts 0 and its k records of
 * d_rays_out are all-zero bytes: not rays.
 * For every valid record d_counts[i] equals, bit for bit, what rt_occluded_rays(d_rays_out, n, k, NULL, p->t_max, .) writes
 * for set i, under every arithmetic policy and RT_OPT_ACCEL setting, whether d_rays_out was given or not.
 * Asynchronous on the context's stream; the context stays as it is, as under the ray queries; rt_walk_overflow reports these
 * walks too.  RT_EINVAL: a NULL ctx or p, both outputs NULL, n 0 or above RT_MAX_RAYS, k 0 or above RT_RAY_SET_MAX, n * k above
 * 2^31, a misaligned pointer (16 bytes; d_counts 4), unknown flag bits, a non-finite offset, NULL d_features with n != W*H, a
 * sharded context.  RT_ESTATE: no scene set; NULL d_features without ready records.  A failed call writes nothing.
 */
#define RT_HEMI_FACE_FORWARD 1u   /* use -normal where dot(normal, record.dir) > 0 */
typedef struct rt_hemisphere_params {
    uint32_t k;        /* rays per record, 1 .. RT_RAY_SET_MAX                       */
    uint32_t flags;    /* RT_HEMI_FACE_FORWARD; any other bit: RT_EINVAL            */
    uint64_t seed;
    float offset;      /* origin = pos + offset * unit normal; finite               */
    float t_max;       /* the bound of every ray, with rt_occluded_rays' meaning    */
} rt_hemisphere_params;
int rt_occluded_hemispheres(rt_context *ctx, const void *d_features, size_t n, const rt_hemisphere_params *p,
                            void *d_counts, void *d_rays_out);

/*
 * Hemisphere gather (new): radiance along the same rays — a final gather from hit points, for irradiance bakes, light maps
 * and probes, in one call and without a ray buffer.  d_features and p as in rt_occluded_hemispheres (p->t_max is not read);
 * d_accum: n x 4 floats on the device, 16-byte aligned, or NULL for the context's accumulator (n must be W*H then, record i
 * is pixel i, and rt_resolve, the denoisers and RT_OPT_MOMENTS work as after rt_render_ray_sets).
 * With R the n * k records rt_occluded_hemispheres' spawn form writes for the same d_features, n and p, the call ADDS to
 * d_accum[i], for every VALID record i, what rt_render_ray_sets(ctx, R, n, p->k, first_sample, n_samples, d_accum) adds for
 * set i — bit for bit in all four channels, under every arithmetic policy, RT_OPT_ACCEL, RT_OPT_SAMPLE_QUEUE,
 * RT_OPT_WAVE_FILL and RT_OPT_MAX_THREADS_PER_LAUNCH, with counters on or off: absolute sample s starts at hemisphere ray
 * s mod k (Philox counter i*k + s mod k), under the random stream (i, 0), with the sample index s; the samples are summed in
 * rt_render_spp's fixed order, more than RT_SPP_PER_LAUNCH of them as launches of that many.  An INVALID record adds nothing:
 * d_accum[i] (count included) and its moment keep their bytes, nothing is traced for it and the counters do not see it —
 * enabled counters receive what rt_render_ray_sets would add over the valid sets alone.  No ray reaches memory.  With d_accum
 * NULL the sample moments are updated as rt_render_ray_sets updates them; an external d_accum keeps none.
 * accum.rgb / accum.w is the mean incoming radiance under the cosine-weighted density: irradiance is pi times it, and the
 * mean times the record's albedo is the diffuse one-bounce radiance.
 * Asynchronous on the context's stream; the image, the sample counter, the feature records, a kept prefix and pending
 * look-ahead frames stay as they are, as under rt_render_rays; rt_debug_last_ray_plan reports these launches.
 * RT_EINVAL: a NULL ctx or p, n 0 or above RT_MAX_RAYS, k 0 or above RT_RAY_SET_MAX, n * k above 2^31, a misaligned pointer,
 * unknown flag bits, a non-finite offset, n_samples 0 or samples beyond RT_MAX_SAMPLE, NULL d_features or NULL d_accum with
 * n != W*H, a sharded context.  RT_ESTATE: no scene set; NULL d_features without ready records.  A failed call changes nothing.
 */
int rt_render_hemispheres(rt_context *ctx, const void *d_features, size_t n, const rt_hemisphere_params *p,
                          uint32_t first_sample, uint32_t n_samples, void *d_accum);

/*
 * Device memory for a host that has no HIP runtime of its own (new) — the buffers the ray queries write into, as the C++
 * façade of host/ makes them.  rt_device_alloc: `bytes` > 0 of memory on the context's device (hipMalloc's alignment), owned by the
 * caller until rt_device_free (NULL is fine; waits for the work that uses the block).  rt_device_copy: `bytes` from `src` to
 * `dst`, to_device != 0: host to device, 0: device to host — ordered on the context's stream behind the calls before it, and
 * complete on return.  RT_EINVAL: a NULL ctx, a NULL pointer to fill or copy, bytes 0 for an allocation.  RT_EHIP: no memory.
 */
int rt_device_alloc(rt_context *ctx, size_t bytes, void **d_out);
int rt_device_free(rt_context *ctx, void *d_ptr);
int rt_device_copy(rt_context *ctx, void *dst, const void *src, size_t bytes, int to_device);

/*
 * Feature records through per-sample cameras (new): the guides that belong to an rt_render_spp_cameras frame.  One call
 * renders the feature records of n_cameras camera blocks per pixel (cameras[12*j .. 12*j+11], host pointer, copied at the
 * call) and reduces them on the device to ONE record per pixel, in rt_feature's layout, plus a two-channel coverage buffer.
 * Per-sample record: for pixel (x, y) and block j, r_j is bit for bit the record rt_render_features_chain(block j, p)
 *   writes for that pixel under the selected arithmetic policy (p NULL = {0, 0}: rt_render_features' record).
 * Key: key_j = (r_j.object, r_j.flags >> 8); the object is 0xFFFFFFFF on a miss, so misses with equal chain words form a
 *   group too.
 * Dominant group and representative: group the n samples by key.  The dominant group is the one with the most samples;
 *   among equally large groups the one that contains the smallest j wins.  The representative j* is the smallest j inside
 *   the dominant group, m the dominant group's size, c the number of samples with RT_FEATURE_HIT.
 * Output record (it REPLACES the context's feature records, so rt_read_features, rt_device_features, the three denoisers
 * and the AOV writers work on it unchanged):
 *   object, material, face, u, v, tex, dir are r_j*'s values, bit for bit;
 *   flags is r_j*'s flags, or'ed with RT_FEATURE_MIXED when m < n;
 *   if r_j* is a miss, pos, t, normal, albedo hold r_j*'s miss values (0, +inf, 0, 0);
 *   if r_j* is a hit, each of the ten floats of pos, t, normal, albedo is S / (float)c: S the sum over ALL hit samples,
 *     whatever their group, taken by the xor butterfly of rt_render_spp over g = 2^ceil(log2 n) lanes — lane j holds sample
 *     j's value, a lane whose sample missed or with j >= n holds +0.0f, offsets g/2, g/4, ..., 1 — and the division the
 *     correctly rounded binary32 quotient under EVERY arithmetic policy.  t of a chain record is its path length, as
 *     rt_render_features_chain defines it.
 * Coverage buffer: W*H*2 floats, row-major, ((float)c / (float)n, (float)m / (float)n), correctly rounded: the anti-aliased
 *   alpha and the purity of the discrete fields.
 * Consequences: n_cameras == 1 gives rt_render_features_chain's record bit for bit and coverage (hit ? 1 : 0, 1); for
 *   n_cameras a power of two, n identical blocks give that record too; hit == (t < inf) still holds; the denoisers' hard
 *   hit / object / chain gates act on the dominant group, their distance terms on the footprint's mean.
 * Why at most 64 blocks: one lane per sample and one pixel per lane group keep the reduction inside a wave; guides carry no
 *   Monte-Carlo noise, only coverage, and 16 blocks are the intended use.
 * Asynchronous on the context's stream.  The image, the accumulator, the sample counter, the moments, a kept prefix and
 * pending look-ahead frames stay untouched, as under rt_render_features.  Unsharded contexts only.
 * rt_read_feature_coverage (bytes = W*H*2*4) and rt_device_feature_coverage give RT_ESTATE until this call has run since the
 * frame was (re)allocated, and again after a later rt_render_features / rt_render_features_chain: the coverage describes the
 * records that lie in the buffer.
 * RT_EINVAL: a NULL cameras or ctx, n_cameras 0 or above RT_FEATURE_CAMERAS_MAX, unknown follow bits, max_chain above
 * RT_FEATURE_CHAIN_MAX, a sharded context, a wrong `bytes`.  RT_ESTATE: no scene set.  A failed call makes nothing.
 * rt_debug_plan_feature_cameras (host-only, no context): the launcher's own plan for a width x height frame and n blocks,
 * out = {log2 of the lanes per pixel, workgroups, threads per workgroup}.  RT_EINVAL: a size outside 1..RT_MAX_DIM, n outside
 * 1..RT_FEATURE_CAMERAS_MAX, a NULL pointer.
 */
#define RT_FEATURE_CAMERAS_MAX 64u
#define RT_FEATURE_MIXED 4u      /* flags bit 2: the pixel's samples fall into more than one group */
int rt_render_features_cameras(rt_context *ctx, const float *cameras, uint32_t n_cameras,
                               const rt_feature_chain_params *p /* NULL = {0, 0}: first hits */);
int rt_read_feature_coverage(rt_context *ctx, float *out, size_t bytes);   /* W*H*2 floats */
int rt_device_feature_coverage(rt_context *ctx, void **d_out);
int rt_debug_plan_feature_cameras(int width, int height, uint32_t n_cameras, uint32_t out[3]); /* host-only */

/*
 * Edge-avoiding à-trous denoiser (new; the reference has no such entry point): Dammertz et al. 2010, "Edge-Avoiding
 * À-Trous Wavelet Transform for fast Global Illumination Filtering", over the linear accumulator, guided by the last
 * rt_render_features call.  With c_p, n_p, x_p, a_p a pixel's colour, normal, position and albedo (the feature
 * record's fp32 values):
 *   c0_p = accum.rgb / accum.w, or 0 where accum.w == 0;
 *   for i = 0 .. L-1, s = 2^i:  c(i+1)_p = sum_q w_pq c(i)_q / sum_q w_pq  over q = p + s*(dx, dy), dx, dy in -2..2
 *     (dy outer, dx inner), taps outside the frame skipped;
 *   w_pq = h[dx] h[dy] e(|c(i)_p - c(i)_q|^2 / (sigma_color 2^-i)^2) e(|n_p - n_q|^2 / sigma_normal^2)
 *          e(|x_p - x_q|^2 / sigma_position^2) e(|a_p - a_q|^2 / sigma_albedo^2),
 *     h = (1/16, 1/4, 3/8, 1/4, 1/16), e(z) = exp(-z); a sigma of +inf switches its term off;
 *     w_pq = 0 when the hit flags of p and q differ, and with RT_DENOISE_SPLIT_OBJECTS also when their object ids
 *     differ, and with RT_DENOISE_SPLIT_CHAINS also when their `flags >> 8` (chain length and signature of
 *     rt_render_features_chain; 0 in first-hit records, where the flag changes nothing) differ — the pair (key, flags >> 8)
 *     is compared, so a mirror's silhouette stays a hard edge even where it reflects the surface behind it (the centre tap
 *     always has weight > 0);
 *   output RGBA = (sqrt(c(L)_p), 1) where accum.w > 0, else 0 (as rt_resolve), into a buffer of its own.
 * Asynchronous on the context's stream; one launch per iteration.  Leaves the image, the accumulator and the sample
 * counter untouched.  RT_EINVAL: iterations outside 1..8, a sigma <= 0 or NaN, unknown flags, a NULL pointer, a
 * sharded context; RT_ESTATE: no features since the frame was (re)allocated.
 * rt_read_denoised: bytes = W*H*16.  rt_device_denoised: the device address of the W x H x 4 floats.  Both give
 * RT_ESTATE until rt_denoise has run since the frame was (re)allocated.
 */
typedef struct rt_denoise_params {
    uint32_t iterations;    /* L, 1 .. 8 (5 suggested)                                                       */
    float sigma_color, sigma_normal, sigma_position, sigma_albedo;   /* > 0; +inf = term off                  */
    uint32_t flags;         /* RT_DENOISE_SPLIT_OBJECTS | RT_DENOISE_SPLIT_CHAINS                             */
} rt_denoise_params;
#define RT_DENOISE_SPLIT_OBJECTS 1u
#define RT_DENOISE_SPLIT_CHAINS 4u   /* (2u stays an unknown bit: callers that probed it keep their RT_EINVAL) */
#define RT_DENOISE_MAX_ITERATIONS 8u

int rt_denoise(rt_context *ctx, const rt_denoise_params *p);
int rt_read_denoised(rt_context *ctx, float *rgba, size_t bytes);
int rt_device_denoised(rt_context *ctx, void **d_rgba);

/*
 * Variance-guided denoiser for low sample counts (new): the spatial half of SVGF, Schied et al. 2017, "Spatiotemporal
 * Variance-Guided Filtering".  Notation as for rt_denoise: c0_p = accum.rgb / accum.w, or 0 where accum.w == 0; n, x, a
 * the feature record's normal, position and albedo; e(z) = exp(-z); h = (1/16, 1/4, 3/8, 1/4, 1/16); key_p the object
 * id with RT_DENOISE_SPLIT_OBJECTS, else the hit flag.  New: l(c) = 0.2126 c.r + 0.7152 c.g + 0.0722 c.b;
 * k = (1/4, 1/2, 1/4); eps = RT_DENOISE_VARIANCE_EPS.
 * The guide weight is g_pq = e(|n_p-n_q|^2/sigma_normal^2 + |x_p-x_q|^2/sigma_position^2 + |a_p-a_q|^2/sigma_albedo^2),
 * and 0 when key_q != key_p, with RT_DENOISE_SPLIT_CHAINS also when `flags >> 8` of the two records differ (as for
 * rt_denoise); a sigma of +inf switches its term off.
 *   1. Variance estimate, 7x7: over the taps q = p + (dx, dy), dx, dy in -3..3, inside the frame,
 *        M0 = sum g_pq,  m = sum g_pq l(c0_q) / M0,  v0_p = sum g_pq (l(c0_q) - m)^2 / M0
 *      (the two-pass form, not M2/M0 - m^2, which in binary32 cancels to noise of the order of eps on flat regions;
 *      the centre tap has weight 1, so M0 >= 1).
 *   2. For i = 0 .. L-1, s = 2^i:
 *        vt_p = sum k[dx] k[dy] v(i)_q / sum k[dx] k[dy] over the 3x3 UNIT neighbours of p inside the frame (no edge
 *          stopping);
 *        d_p = sigma_luminance sqrt(vt_p) + eps;
 *        w_pq = h[dx] h[dy] g_pq e(|l(c(i)_p) - l(c(i)_q)| / d_p) over q = p + s*(dx, dy), dx, dy in -2..2 (dy outer,
 *          dx inner), taps outside the frame skipped; sigma_luminance = +inf switches the luminance term off;
 *        c(i+1)_p = sum w c(i)_q / sum w;   v(i+1)_p = sum w^2 v(i)_q / (sum w)^2.
 *   3. Output RGBA = (sqrt(c(L)_p), 1) where accum.w > 0, else 0, into the SAME buffer rt_denoise writes, so
 *      rt_read_denoised and rt_device_denoised serve both.  v0 and v(L) are kept as W x H floats.
 * A filter for LOW sample counts (1 .. 4 spp): from about 16 spp on the spatial estimate takes illumination gradients
 * for noise and rt_denoise is the better filter (DESIGN.md "Variance-guided filter").
 * Asynchronous on the context's stream; one launch for step 1 and one per iteration.  Leaves the image, the
 * accumulator, the sample counter and the feature records untouched.  RT_EINVAL: iterations outside 1..8, a sigma <= 0
 * or NaN, unknown flags, a NULL pointer, `which` outside 0..1, a sharded context; RT_ESTATE: no features since the frame
 * was (re)allocated.
 * rt_read_variance: which 0: v0, 1: v(L); bytes = W*H*4.  rt_device_variance: the device address of the W x H floats.
 * Both give RT_ESTATE until rt_denoise_variance has run since the frame was (re)allocated.
 */
typedef struct rt_denoise_variance_params {
    uint32_t iterations;    /* L, 1 .. 8 (5 suggested)                                                       */
    float sigma_luminance;  /* > 0 (4 suggested); +inf = term off                                            */
    float sigma_normal, sigma_position, sigma_albedo;   /* as rt_denoise_params                               */
    uint32_t flags;         /* RT_DENOISE_SPLIT_OBJECTS | RT_DENOISE_SPLIT_CHAINS                             */
} rt_denoise_variance_params;
#define RT_DENOISE_VARIANCE_EPS 1e-4f

int rt_denoise_variance(rt_context *ctx, const rt_denoise_variance_params *p);
int rt_read_variance(rt_context *ctx, int which, float *out, size_t bytes);
int rt_device_variance(rt_context *ctx, int which, void **d_out);

/*
 * Per-pixel sample moments (new; RT_OPT_MOMENTS) and the variance-guided filter on MEASURED variance.
 * With l(c) the luminance above and s_0 .. s_(n-1) the samples a pixel's accumulator holds (n = accum.w), the moment
 * buffer keeps M2_p = sum_j (l(s_j) - m_p)^2, m_p = sum_j l(s_j) / n: one float per pixel, W x H, row-major.
 * The moments become VALID at rt_clear and at the start of rt_render_adaptive, rt_render_adaptive_cameras,
 * rt_render_adaptive_variance and rt_render_adaptive_variance_cameras while RT_OPT_MOMENTS is 1 (all zero them on the
 * stream); they become invalid when the option's value changes and after rt_resize.  While they are valid, every call
 * that adds to the accumulator — rt_render_spp and the adaptive calls, on every path they can take — updates them (the
 * two variance-rule calls also READ them, to decide when a block stops); rt_render, rt_render_again and its look-ahead launches never touch them.  While they are invalid nothing
 * writes the buffer, and rt_read_moments, rt_device_moments and rt_denoise_moments give RT_ESTATE.
 * Two partial states (n, RGB sum S, M2) of a pixel are combined in ONE place, by the pairwise update of Chan, Golub &
 * LeVeque 1979 — rt_moments_merge, the very function the kernels call:
 *   nA == 0: M2B exactly;  nB == 0: M2A exactly;
 *   otherwise delta = l(SB)/nB - l(SA)/nA,  M2 = M2A + M2B + delta^2 nA nB / (nA + nB).
 * A launch's own M2B is the centred sum about the launch's mean, sum_j (l(s_j) - l(S_B)/nB)^2 — never sum l^2 - n m^2,
 * which cancels in binary32; a pixel whose samples are all one colour (finished by the prefix stage) has M2B = 0.
 * The summation order inside a launch is not part of the contract: the result is specified to a tolerance.
 * rt_read_moments: bytes = W*H*4.  rt_device_moments: the device address of the W x H floats.
 * rt_moments_merge: host-only, no context.  RT_EINVAL: a NULL pointer.
 * rt_denoise_moments is rt_denoise_variance in every respect — parameters, validation, the buffers written, the outputs
 * behind rt_read_denoised and rt_read_variance, asynchrony, nothing else moves — except step 1:
 *   v0_p = M2_p / (n_p (n_p - 1))  where n_p >= RT_DENOISE_MOMENTS_MIN_COUNT (SVGF's history threshold),
 * the variance of the pixel's MEAN measured from its own samples; elsewhere (n_p = 0 included) the 7x7 estimate.
 * From 4 spp on it is never worse than the spatial estimate and from 16 spp on clearly better (DESIGN.md "Measured
 * variance"); additionally RT_ESTATE while the moments are not valid.
 */
#define RT_DENOISE_MOMENTS_MIN_COUNT 4u
int rt_read_moments(rt_context *ctx, float *m2, size_t bytes);
int rt_device_moments(rt_context *ctx, void **d_m2);
int rt_moments_merge(uint32_t nA, const float sumA[3], float m2A, uint32_t nB, const float sumB[3], float m2B, float *m2_out);
int rt_denoise_moments(rt_context *ctx, const rt_denoise_variance_params *p);

/* Wait for everything queued on the context's stream (reference:
 * queue.finish(), src/raytracer.cpp:140).  rt_render/rt_render_again already
 * return synchronously; rt_render_spp/rt_resolve/rt_clear are asynchronous. */
int rt_sync(rt_context *ctx);

/*
 * Parity probe (new): linear radiance getCol(...) (raytracer.cl:444-486) of
 * `n` individual pixel-samples (x[i], y[i], sample[i]) → out_rgb[3*i..].
 * Bit-exact against the reference per sample.  Host pointers.
 */
int rt_trace_samples(rt_context *ctx, const float camera[12], const uint32_t *x, const uint32_t *y,
                     const uint32_t *sample, size_t n, float *out_rgb);

/* ---- outputs ------------------------------------------------------------- */

/* Replaces RayTracer::transferImage (src/raytracer.cpp:167-174; there the
 * pixels stay in a GL texture): copy the gamma-space RGBA32F image, row 0 =
 * first row the kernel wrote (y = 0), to host memory.  bytes = w*h*16. */
int rt_read_image(rt_context *ctx, float *rgba, size_t bytes);

/* Linear accumulator divided by the sample count (RGBA32F, alpha 1). */
int rt_read_linear(rt_context *ctx, float *rgba, size_t bytes);

/* Device addresses of the W×H×4-float buffers, for zero-copy consumers
 * (RCCL reduce of the radiance buffer, display interop). */
int rt_device_image(rt_context *ctx, void **d_rgba);
int rt_device_accum(rt_context *ctx, void **d_rgba);

/* Tuning / diagnostics switches (new).  Results never depend on them. */
#define RT_OPT_PREFIX_SHARING 1         /* 1 (default): rt_render_spp traces the sample-invariant path
                                           prefix once per pixel; 0: every sample from the camera      */
#define RT_OPT_MAX_THREADS_PER_LAUNCH 2 /* split one render call into several kernel launches           */
#define RT_OPT_SAMPLE_QUEUE 3           /* 1 (default): lanes pull samples from an in-wave queue as their
                                           paths end; 0: one fixed sample set per lane                  */
#define RT_OPT_ACCEL 4                  /* sphere / mesh search: 0 brute force (the reference's loops), 1
                                           (default) conservative BVHs for >= 64 spheres and for meshes of
                                           >= 32 faces, 2 sphere BVH always.  Same winner in every mode
                                           (a set of >= 2^24 spheres, or meshes of >= 2^26 BVH nodes in all,
                                           take the brute-force loops: the walks address 32-bit offsets)      */
#define RT_OPT_WALK_SLICES 5            /* 1 (default): in scenes where every mesh of every model has a BVH, the
                                           lanes' mesh walks advance in interleaved slices; 0: every walk runs in place */
#define RT_OPT_PREFIX_TREE 7            /* a pixel whose first random event is a dielectric surface gets a shared DECISION TREE —
                                           glass has only two outcomes (refract / reflect, raytracer.cl:407-435), so both
                                           continuations are traced once per pixel and every sample only picks its branch with
                                           its own table entry.  1 (default): in calls of >= 24 samples per pixel (below that
                                           the trees cost more than they share); 2: in every call; 0: never — every sample
                                           traces its own way through the glass.  Same result bit for bit in every mode */
#define RT_OPT_WAVE_FILL 8              /* 1 (default): a sample-kernel wave owns fewer pixels when the launch is small (a small
                                           frame, a rank's share of a sharded one), so that the chip's wave slots are filled;
                                           0: always as many pixels per wave as its LDS share holds.  Same result bit for bit */
#define RT_OPT_PREFIX_CACHE 9           /* 1 (default): while the camera block, the scene and every setting stay as they are,
                                           a fused call keeps what its first stage (pt_prefix) left in the context — records,
                                           live list, decision trees — and later calls only add the finished pixels' share of
                                           their samples (pt_final_replay) before the sample kernel runs; a changed camera,
                                           scene, texture, seed, option, shard, frame size or stream traces the prefix anew.
                                           0: every call traces it anew.  A process whose environment holds
                                           RT_PREFIX_CACHE=0 starts its contexts with 0.  Same result bit for bit           */
#define RT_OPT_LOOKAHEAD 10             /* K = 16 (default), 2 .. 64: an rt_render_again call that repeats the camera block of the
                                           previous rt_render / rt_render_again call traces the next K samples in one fused
                                           launch (pt_prefix / the kept prefix + the sample-queue kernel), replays the running mean
                                           per pixel in sample order and stores the image after each sample in a ring of frames
                                           owned by the context (at most RT_LOOKAHEAD_MAX_BYTES = 1 GiB: fewer frames per batch for
                                           large frames, none where two do not fit); this call and the next K - 1 copy their frame
                                           into the image.  Frames still pending are dropped — and the next call starts from the
                                           image as it lies — when the camera block changes, after rt_render, rt_resolve,
                                           rt_render_adaptive, rt_resize, and after any call that changes scene, textures, seed /
                                           table, an option, the shard, the stream or the counters.  Calls run the direct kernel
                                           as before while counters are enabled, on a sharded context, with RT_OPT_PREFIX_SHARING or
                                           RT_OPT_SAMPLE_QUEUE off, or when RT_OPT_MAX_THREADS_PER_LAUNCH splits the frame.
                                           0: every call runs the direct kernel; 1 and values above 64: RT_EINVAL.  A process whose
                                           environment holds RT_LOOKAHEAD=0 starts its contexts with 0.  Same result bit for bit.
                                           The library assumes that nobody else writes the image: a zero-copy consumer that WRITES
                                           through rt_device_image between rt_render_again calls must set this option to 0       */
#define RT_OPT_EXACT_GRID 11            /* 1 (default): while a fused call reuses the kept prefix (RT_OPT_PREFIX_CACHE), the host learns
                                           the length of the live list — one asynchronous 128-byte copy on the first call that
                                           reuses it, never waited for — and from then on launches the sample kernel with exactly
                                           the workgroups that own a pixel (rt_sample_units), none at all for a frame without live
                                           pixels; 0: always the grid for "every pixel is live" (its surplus workgroups leave at
                                           once).  A process whose environment holds RT_EXACT_GRID=0 starts its contexts with 0.
                                           Same result bit for bit                                                          */
#define RT_OPT_MOMENTS 12               /* 0 (default): no sample moments — nothing is allocated and every launch gets a NULL moment
                                           pointer; 1: the context keeps each pixel's centred second luminance moment beside the
                                           accumulator (rt_read_moments; one more pass over a wave's sample slots in the sample
                                           kernels' epilogue, 4 more bytes per pixel).  Any other value: RT_EINVAL.  Unsharded
                                           contexts only: setting 1 on a context with world > 1, and rt_set_shard to world > 1
                                           while it is 1, give RT_EINVAL.  A change of value invalidates the moments until the next
                                           rt_clear / rt_render_adaptive.  rt_render_adaptive_variance(_cameras) need 1 and give
                                           RT_ESTATE otherwise.  Image and accumulator: the same bit for bit                  */
#define RT_OPT_ACCUM_STORE 13           /* 1 (default): rt_clear records the clear instead of enqueuing it, and a fused rt_render_spp
                                           launch that writes every pixel of the frame exactly once — 64 samples per pixel through the
                                           sample queue without a BVH walk, an unsharded, unmasked frame in one slot range, no
                                           counters, no moments — STORES its
                                           sums (0 + sum, the words an add to a zeroed pixel leaves); whatever else reads, writes
                                           or hands out the accumulator, and every wait for the stream, enqueues the memset first
                                           (see rt_clear).  0: rt_clear enqueues the memset at once and every launch adds; a clear
                                           recorded under 1 is enqueued by the change to 0.  Any other value: RT_EINVAL.  Same
                                           result bit for bit                                                                   */
#define RT_OPT_ARITH 6                  /* the ARITHMETIC POLICY of the trace kernels (csrc/pt_arith.hpp).  The reference's
                                           random numbers are table entries indexed by a hash of the ray direction
                                           (raytracer.cl:113-125): one ulp re-routes a path, so "the reference's
                                           result" exists only relative to one definition of the OpenCL builtins, of
                                           `/`, sqrt and of the contraction of a*b+c.  Unlike the other options this
                                           one CHANGES THE RESULT — it selects which build of the reference is matched
                                           bit for bit per pixel-sample:                                          */
#define RT_ARITH_IEEE 0                 /*   (default) plain IEEE-754 builtins, correctly rounded / and sqrt, no fused
                                             multiply-add: the reference compiled -ffp-contract=off for a CPU with the
                                             builtin formulas of oracle/ref_shim.cpp — what the CPU oracle restates   */
#define RT_ARITH_ROCM_OCL_NOCONTRACT 1  /*   the reference built by ROCm's OpenCL tool chain for gfx950 with
                                             -ffp-contract=off: ROCm's builtin library (fma-chain dot / cross / mix,
                                             v_rsq_f32 normalize, ocml pow), 2.5-ulp `/`, 3-ulp sqrt               */
#define RT_ARITH_ROCM_OCL 2             /*   the same with OpenCL's DEFAULT flags: clang also contracts the kernel's
                                             own a*b+c expressions — what an unmodified KernelGL::buildProgram
                                             (src/kernelgl.cpp:95-106, no build options) gets from ROCm's OpenCL    */
int rt_set_option(rt_context *ctx, int option, int value);

/* ---- measurement --------------------------------------------------------- */

/* When enabled, render calls run the counting build of the kernel (slower)
 * and add to the context's counters.  Off by default. */
int rt_enable_counters(rt_context *ctx, int enable);
int rt_reset_counters(rt_context *ctx);
int rt_get_counters(rt_context *ctx, rt_counters *out);

/* Host-only self-check (no device, no context): validates and prepares the scene through the very
 * code rt_set_scene uploads from and verifies the invariants of the prepared arrays — every
 * primitive in exactly one leaf and inside the box of every node above it, split axes and skip
 * links (both walks are threaded), the walk visiting every leaf exactly once in all eight direction
 * octants (mesh trees: as built and through the collapsed links of the packed nodes), smallest-face
 * indices, normal cones, edge bounds, the packed nodes' fields rounded to the safe side, the sphere
 * tree's device arrays, the walk jobs.  Where rt_set_scene builds no tree (a non-finite sphere, the
 * size gates) none is reported.  A scene rt_set_scene would reject gives the same code, the message
 * in `err`.  stats = {sphere nodes, sphere leaves, sphere depth, mesh nodes, mesh leaves, mesh
 * depth, meshes with a BVH, digest}; digest = FNV-1a-64 over the raw bytes of what rt_set_scene
 * uploads or keeps for arithmetic policy 0, each array preceded by its element count as a
 * little-endian uint64: face bases, face records, packed mesh nodes, leaf faces, leaf face indices,
 * mesh roots, walk jobs, sphere boxes, sphere links, sphere leaf indices, then eleven 32-bit words
 * (BVH node count, centre bounds lo[3] hi[3], largest radius, mesh BVHs in use, textures in use,
 * largest texture id). */
int rt_debug_check_accel(const rt_scene_desc *scene, uint64_t stats[8], char *err, size_t err_len);

/* Diagnostics of the sphere search since the last reset (counting build only):
 * out[0] = BVH nodes entered, out[1] = sphere tests actually executed. */
int rt_get_debug_counters(rt_context *ctx, uint64_t out[2]);

/* Sticky flags "a BVH walk left its loop on its iteration bound instead of at the end of the tree" since the last
 * rt_reset_counters(): bit 0 sphere walk, bit 1 mesh walk, bit 2 the walk-slice kernel's outer loop.  Such a walk
 * may return a wrong nearest hit; the bounds are sized so that it cannot happen, and every GPU test and bench.py's
 * parity leg assert 0 here. */
int rt_walk_overflow(rt_context *ctx, uint32_t *flags_out);

/* Algorithmic bytes of the reference kernel for these counters
 * (SURVEY §8d): 32·t_sphere + 48·t_plane + 64·t_lens + 12·t_model +
 * 16·t_mesh + 60·t_tri + 36·h_tri + 48·h_bounce + 12·n_scatter +
 * 4·n_dielectric + 64·n_texfetch + (48+16)·samples + 16·image_reads. */
uint64_t rt_counters_bytes(const rt_counters *c);

/* Milliseconds the last render call's kernel(s) took on the device
 * (hipEvent pair recorded on the launch stream around the launch). */
int rt_last_kernel_ms(rt_context *ctx, float *ms);

/* The same for the last *n_out <= min(cap, 64) render calls, oldest first.  The
 * events are only read here, so a timed loop can run without per-step syncs. */
int rt_kernel_ms_history(rt_context *ctx, float *ms, size_t cap, size_t *n_out);

/* ---- unit probes of the device routines (test instrumentation; no reference counterpart) ----
 * rt_debug_hit: one intersection routine per record, through the same search + winner rebuild the
 * trace kernels inline.  kind 0 hitSphere (raytracer.cl:149), 1 hitPlane (:176), 2 hitLens (:196),
 * 3 hitScene (:322), 4 hitTriangle (:257) on face[i] of mesh prim[i].  rays: n × 6 floats (origin,
 * direction); out12: n × 12 floats {hit, t, p.xyz, normal.xyz, uv.xy, texture_ID bits, mat_ID bits},
 * all zero on a miss — the record layout of oracle/ref_shim.cpp ref_hit.
 * rt_debug_material: routine 0 rayReflect (:362), 1 rayRefract (:369), 2 rayScatter (:393),
 * 3 rayRefractDielectric (:407).  in16: n × 16 floats {ray dir.xyz, hit p.xyz, hit normal.xyz,
 * colour so far.xyz, mat_ID bits, s_seed bits, pixel x bits, pixel y bits}; out9: n × 9 floats
 * {new origin.xyz, new direction.xyz, colour.xyz} (getCol's mixCol is not part of the routines).
 * rt_debug_div3: in4 n × {a.xyz, d} → out6 n × {shared-reciprocal a/d, compiler's a/d}. */
int rt_debug_hit(rt_context *ctx, int kind, const float *rays, const uint32_t *prim, const uint32_t *face, size_t n,
                 float *out12);
int rt_debug_material(rt_context *ctx, int routine, const float *in16, size_t n, float *out9);
int rt_debug_div3(rt_context *ctx, const float *in4, size_t n, float *out6);
/* rt_debug_builtin: ONE builtin of the selected arithmetic policy per record — op 0 dot, 1 cross, 2 normalize,
 * 3 {a0/a1, 1/a0, (a.yz)/a6}, 4 sqrt, 5 mix(a, b, a6), 6 min, 7 sign, 8 pow(a0, 5), 9 the table hash of a.xyz (uint
 * bits); 10 sqrt and 11 normalize in the tagged forms the sample queue runs (csrc/pt_arith.hpp: the WAVE — 64
 * consecutive records — chooses between the bare instruction and the untagged form; same bits as ops 4 and 2,
 * tests/test_gpu_fast_builtins.py); 12 min in the tagged form (no canonicalising of the operands: same bits as op 6
 * for operands that hold no signalling NaN, tests/test_gpu_mixcol.py).  in8: n × 8 floats {a.xyz, b.xyz, t, -}; out4: n × 4 floats.
 * tests/test_gpu_ref950.py compares policies 1 / 2 with probe kernels that call ROCm's OpenCL builtins themselves. */
int rt_debug_builtin(rt_context *ctx, int op, const float *in8, size_t n, float *out4);
/* rt_debug_queue_sums: the sample-queue kernels' per-pixel summation on its own.  ONE wave owns npix pixels of `count`
 * samples each (npix <= 16, npix × count <= 512), finds their radiances in its queue — in3: npix × count × 3 floats,
 * pixel-major — and sums them with 1 << group_log2 lanes per pixel (group_log2 <= 6) as a launch without sample moments
 * does.  out4: npix × 4 floats {sum.rgb, count}, the accumulator after the launch when it was zero before. */
int rt_debug_queue_sums(rt_context *ctx, const float *in3, uint32_t npix, uint32_t count, uint32_t group_log2, float *out4);

/* The two stages of the same calls separately: a fused rt_render_spp call is pt_prefix
 * (first_ms: one work-item per pixel, the sample-invariant path prefix) or, when the call
 * reuses the kept prefix (RT_OPT_PREFIX_CACHE), pt_final_replay in its place, followed by the
 * per-sample kernel (second_ms: pt_samples_q / pt_samples_w, the dominant kernel that
 * bench.py prices against the roofline); a third event is recorded between them.  Calls
 * on the direct path (rt_render, rt_render_again) report first_ms = 0; so does an
 * rt_render_again call that only hands a look-ahead frame out (its copy is second_ms), while
 * the call that launches a look-ahead batch reports the two stages of that launch. */
int rt_stage_ms_history(rt_context *ctx, float *first_ms, float *second_ms, size_t cap, size_t *n_out);

/* Fused launches (rt_render_spp: one per 512 samples per pixel; rt_render_adaptive: one per round; rt_render_again: one
 * per look-ahead batch, RT_OPT_LOOKAHEAD) of this context that reused the kept prefix (RT_OPT_PREFIX_CACHE) and that
 * traced it in full, since rt_create. */
int rt_prefix_cache_stats(rt_context *ctx, uint64_t *hits, uint64_t *misses);

/* rt_clear calls of this context since rt_create whose clear was recorded (RT_OPT_ACCUM_STORE 1) and then ended by a fused
 * launch that STORED its sums (`stored`), or by the memset, enqueued in front of whatever came next (`materialised`). */
int rt_accum_store_stats(rt_context *ctx, uint64_t *stored, uint64_t *materialised);

/* Look-ahead (RT_OPT_LOOKAHEAD) since rt_create: `batches` look-ahead launches; `served` rt_render_again calls whose image
 * came from a look-ahead frame (the launching call included); `direct` rt_render_again calls that ran the direct kernel;
 * `discarded` frames computed and dropped before a call could hand them out.  rt_render_again_cameras calls count with
 * rt_render_again's. */
int rt_lookahead_stats(rt_context *ctx, uint64_t *batches, uint64_t *served, uint64_t *direct, uint64_t *discarded);

/* Host-only (no device, no context): the number of samples the look-ahead launch of an rt_render_again call would trace
 * for a width x height frame with RT_OPT_LOOKAHEAD = option_value at this sample counter — min(option_value,
 * RT_MAX_SAMPLE - sample_counter, frames of the ring budget of 1 GiB), or 0 (the direct kernel) where that is below 2.
 * rt_render_again calls this very function.  RT_EINVAL: an option value the option refuses, a size outside 1..RT_MAX_DIM. */
int rt_lookahead_plan(int width, int height, int option_value, uint32_t sample_counter, uint32_t *batch_out);

/* Host-only (no device, no context): the workgroups (pixel groups, for the fixed-lane kernel) of a sample-kernel launch
 * that own at least one pixel, for a live list of capacity seg_cap whose counters read count_light and count_heavy and
 * pixels_per_unit pixels per workgroup — the host's restatement of the kernels' live_take: both counts clamped to the
 * capacity as the kernels clamp them (light first, heavy to what is left), ceil(heavy / p) units for the heavy part, which
 * the kernels hand out first, then ceil(light / p).  Every unit below the result takes a pixel, none from it on.  The
 * launcher calls this very function (RT_OPT_EXACT_GRID).  RT_EINVAL: pixels_per_unit 0, units_out NULL. */
int rt_sample_units(uint32_t seg_cap, uint32_t pixels_per_unit, uint32_t count_light, uint32_t count_heavy, uint32_t *units_out);

/* Sample-kernel launches of this context's fused calls since rt_create (RT_OPT_EXACT_GRID): `launches` fused launches that
 * reached the sample stage; `exact` of them sized by the known length of the live list (a launch of no workgroup at all
 * included); `workgroups` launched by all of them together; `live_last` the workgroups of the last exact launch, all of
 * which own a pixel.  The direct path (rt_render, rt_render_again without look-ahead) does not count. */
int rt_sample_grid_stats(rt_context *ctx, uint64_t *launches, uint64_t *exact, uint64_t *workgroups, uint64_t *live_last);

/* Test instrumentation: what the last fused launch's sample kernel divided — out = {capacity of the live list (seg_cap),
 * pixels per unit of that launch, the light counter, the heavy counter}, the counters read from the device as they lie
 * (synchronises the stream).  rt_sample_units of these four is the number of workgroups with a pixel.  RT_EINVAL before
 * the first fused launch. */
int rt_debug_live_list(rt_context *ctx, uint32_t out[4]);

/* Test instrumentation, no device needed: pixels a wave of the sample queue owns at `count` samples per pixel with
 * `waves_per_simd` one-wave workgroups per SIMD and `static_float4` float4 of staged tables, when LDS is handed out in blocks
 * of `granule` bytes (0: the granule the launcher uses).  RT_EINVAL: count 0, waves outside 1..8, a granule outside 16..8192. */
int rt_debug_queue_pixels(uint32_t count, uint32_t waves_per_simd, uint32_t static_float4, uint32_t granule, uint32_t *pixels_out);

/* What a fused launch's choice of sample kernel reads (one slot range of one call); flags are 0 / 1. */
typedef struct rt_sample_facts {
    uint32_t count, glog2;              /* samples per pixel of the call, log2 of the lanes per pixel */
    uint32_t n, seg_cap;                /* slots of the range; capacity of its live list (n rounded up to 256) */
    uint32_t material_count, sphere_count, plane_count, lens_count, model_count;
    uint32_t sphere_bvh, mesh_bvh;      /* the launch walks a sphere BVH / per-mesh BVHs */
    uint32_t walk_jobs;                 /* meshes of the walk-slice kernel (0 unless every mesh has a BVH) */
    uint32_t faces;                     /* triangles of all meshes together */
    uint32_t cu_count;
    uint32_t count_enabled, sample_queue, walk_slices, wave_fill, moments;
    uint32_t exact, count_light, count_heavy;   /* the live list's counters are known to the host (else both 0) */
} rt_sample_facts;

#define RT_PLAN_FIXED 0u   /* pt_samples<COUNT, ACCEL> */
#define RT_PLAN_QUEUE 1u   /* pt_samples_q<COUNT, ACCEL, GEOM, WAVES, MOMENTS, COUNT_LOG2> */
#define RT_PLAN_WALK 2u    /* pt_samples_w<MULTI, MOMENTS> */
#define RT_PLAN_GENERIC_COUNT 0xFFFFFFFFu   /* count_log2 of the instantiations for any count (COUNT_LOG2 = -1) */

/* The sample-kernel launch chosen for an rt_sample_facts: the instantiation and its launch geometry.  count (counters on),
 * accel (the scene has a BVH) and moments (the launch keeps them) are set for every family, whether or not its template
 * takes them; geom, count_log2 belong to RT_PLAN_QUEUE and multi to RT_PLAN_WALK (0 elsewhere), waves is 0 for
 * RT_PLAN_FIXED.  grid_units 0: nothing is launched. */
typedef struct rt_sample_plan {
    uint32_t family;
    uint32_t count, accel, geom, waves, moments, count_log2, multi;
    uint32_t pixels_per_wave;           /* pixels per unit of the live list (1 for RT_PLAN_FIXED) */
    uint32_t lds_face_f4;               /* float4 of face records the launch stages in LDS (FrameParams::lds_face_f4) */
    uint32_t lds_bytes;                 /* dynamic LDS of a workgroup */
    uint32_t grid_units, block_size;    /* workgroups, threads of each */
} rt_sample_plan;

/* Test instrumentation, no device needed: the plan the fused launcher makes for `facts` — the launcher calls this very
 * function.  RT_EINVAL: a NULL pointer, count 0, glog2 above 6, seg_cap below n. */
int rt_debug_plan_samples(const rt_sample_facts *facts, rt_sample_plan *plan_out);

/* Test instrumentation: the facts and the plan of the context's last fused launch (its last slot range).  RT_EINVAL before
 * the first one. */
int rt_debug_last_sample_plan(rt_context *ctx, rt_sample_facts *facts_out, rt_sample_plan *plan_out);

/* What a camera launch's choice of kernel reads (one slot range of one launch of rt_render_spp_cameras); flags are 0 / 1. */
typedef struct rt_camera_facts {
    uint32_t count, glog2;              /* blocks (= samples per pixel) of the launch, log2 of the lanes per pixel */
    uint32_t n;                         /* slots of the range */
    uint32_t material_count, sphere_count, plane_count, lens_count, model_count;
    uint32_t sphere_bvh, mesh_bvh;      /* the launch walks a sphere BVH / per-mesh BVHs */
    uint32_t faces;                     /* triangles of all meshes together */
    uint32_t cu_count;
    uint32_t count_enabled, sample_queue, wave_fill, moments;
} rt_camera_facts;

#define RT_CAMERA_PLAN_FIXED 0u   /* pt_render<MODE_ACCUM, COUNT, ACCEL, CAMS = true> */
#define RT_CAMERA_PLAN_QUEUE 1u   /* pt_samples_q<false, ACCEL, GEOM, WAVES, false, -1, CAM = true> */

/* The kernel chosen for an rt_camera_facts and its launch geometry.  count, accel and moments as in rt_sample_plan; geom,
 * waves, lds_face_f4 and lds_bytes belong to RT_CAMERA_PLAN_QUEUE (0 elsewhere).  A queue wave owns the owned, active pixels
 * among pixels_per_wave consecutive slots, so grid_units = ceil(n / pixels_per_wave) exactly. */
typedef struct rt_camera_plan {
    uint32_t family;
    uint32_t count, accel, geom, waves, moments;
    uint32_t pixels_per_wave;           /* slots per wave (1 for RT_CAMERA_PLAN_FIXED) */
    uint32_t lds_face_f4, lds_bytes;
    uint32_t grid_units, block_size;
} rt_camera_plan;

/* Test instrumentation, no device needed: the plan rt_render_spp_cameras' launcher makes for `facts` — the launcher calls
 * this very function.  RT_EINVAL: a NULL pointer, count 0 or above 512, glog2 above 6. */
int rt_debug_plan_camera_samples(const rt_camera_facts *facts, rt_camera_plan *plan_out);

/* Test instrumentation: the facts and the plan of the context's last camera launch (its last slot range).  RT_EINVAL before
 * the first one. */
int rt_debug_last_camera_plan(rt_context *ctx, rt_camera_facts *facts_out, rt_camera_plan *plan_out);

/* Test instrumentation: the facts (n = the rays of the range) and the plan of the context's last ray launch (rt_render_rays or
 * rt_render_ray_sets, its last slot range; after rt_render_adaptive_rays / ..._variance_rays the last round's — a masked launch
 * has the plan and the grid of the unmasked one) — rt_render_spp_cameras' planner, the one rt_debug_plan_camera_samples calls.
 * RT_EINVAL before the first one. */
int rt_debug_last_ray_plan(rt_context *ctx, rt_camera_facts *facts_out, rt_camera_plan *plan_out);

/* Test instrumentation: resident workgroups per compute unit the runtime reports for the headline sample-queue kernel
 * (one wave per workgroup) at `lds_bytes` of dynamic LDS (hipOccupancyMaxActiveBlocksPerMultiprocessor; no kernel runs). */
int rt_debug_queue_occupancy(rt_context *ctx, uint32_t lds_bytes, int *blocks_out);

/* Test instrumentation: out = {sample-kernel launches (one per slot range of a fused call; an empty grid launches nothing) of the instantiation of pt_samples_q written for
 * exactly 64 samples per pixel, builds of the staged scene block (the LDS tables the sample queue copies)} since the
 * context was made. */
int rt_debug_wave_fixed(rt_context *ctx, uint64_t out[2]);

/* Test instrumentation: the staged scene block as it lies on the device — *float4_out float4 (0 for a scene none of whose
 * sets fits its cap) in the layout of the sample kernels' LDS tables: per material (r, g, b, extra_data), (type bits,
 * 1 / extra_data, Schlick's r0 of extra_data, of 1 / extra_data); per sphere (x, y, z, r), (mat_ID bits, 0, 0, 0); per
 * plane (normal, mat_ID bits); a set over its cap (64 materials, 64 spheres, 16 planes) is left out.  Synchronises the
 * stream.  RT_EINVAL: no fused launch since the scene, an option or the shard last changed, or capacity_float4 too small. */
int rt_debug_stage_block(rt_context *ctx, float *out, size_t capacity_float4, uint32_t *float4_out);

/* Name, CU count and arch of the context's device, e.g. "gfx950". */
int rt_device_info(rt_context *ctx, char *name, size_t name_len, int *cu_count, char *arch, size_t arch_len);

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_H */
