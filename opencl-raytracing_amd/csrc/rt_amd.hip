// rt_amd.hip — host side of librt_amd.so (include/rt_amd.h), gfx950 only: the C ABI, scene upload (what is uploaded is
// computed by scene_prep.hpp) and the kernels that carry none of the reference's arithmetic (resolve, pack, unpack).
// The path-tracing kernels live in pt_kernels.hip, compiled once per arithmetic policy (pt_arith.hpp); this file
// picks a policy's launchers at run time (RT_OPT_ARITH).  The denoisers and their kernels live in rt_denoise.hip.
//
// Build: __graft_entry__.build_hip().  No CPU fallback exists: without a gfx950 device rt_create() fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "rt_context.hpp"
#include "pt_kernels.hpp"
#include "pt_moments.hpp"
#include "pt_chain.hpp"
#include "scene_prep.hpp"

using namespace pt;
using namespace rtamd;
using namespace scene_prep;

static_assert(MESH_ROOT_NONE == PT_MESH_BVH_NONE, "scene_prep.hpp and pt_types.hpp name the same \"no BVH\" root");

// =============================== policy-free kernels ===============================

// Multi-GPU exchange: the accumulator pixels a rank owns, packed in slot order (what
// travels over xGMI is 1/world of the frame instead of the whole frame) ...
__global__ __launch_bounds__(256) void pt_pack(FrameParams fp, const float4 *__restrict__ accum,
                                               float4 *__restrict__ packed, uint32_t n_slots) {
    uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= n_slots) return;
    uint32_t x, y;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (slot < fp.slot_end && slot_to_pixel(fp, slot, x, y)) v = accum[(size_t)y * fp.w + x];
    packed[slot] = v;
}
// ... and the inverse on the receiving rank: fp describes the SENDER's shard
__global__ __launch_bounds__(256) void pt_unpack(FrameParams fp, const float4 *__restrict__ packed,
                                                 float4 *__restrict__ accum) {
    uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    uint32_t x, y;
    if (slot < fp.slot_end && slot_to_pixel(fp, slot, x, y)) accum[(size_t)y * fp.w + x] = packed[slot];
}

// image = sqrt(accum.rgb / accum.w), alpha 1; pixels this rank does not own stay 0
__global__ __launch_bounds__(256) void pt_resolve(const float4 *__restrict__ accum, float4 *__restrict__ image,
                                                  uint32_t n, int linear_only) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float4 a = accum[i];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.w > 0.0f) {
        float rx = a.x / a.w, ry = a.y / a.w, rz = a.z / a.w;
        o = linear_only ? make_float4(rx, ry, rz, 1.0f) : make_float4(sqrtf(rx), sqrtf(ry), sqrtf(rz), 1.0f);
    }
    image[i] = o;
}

// rt_render_features_cameras, behind pt_features_cameras (pt_kernels.hip): one work-item per pixel.  That kernel leaves the
// ten floats of pos, t, normal, albedo of a hit record as SUMS over the pixel's hit samples and the coverage words as the
// counts (c hit samples, m samples in the dominant group).  The quotients are taken HERE, in the translation unit that is
// compiled with the correctly rounded divide whatever the arithmetic policy: S / (float)c in place, and the coverage
// ((float)c / (float)n, (float)m / (float)n).
__global__ __launch_bounds__(256) void pt_features_cameras_finish(float4 *__restrict__ rec, float2 *__restrict__ cov, uint32_t pixels,
                                                                  uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    const uint2 cm = reinterpret_cast<const uint2 *>(cov)[i];
    float4 *r = rec + 5 * (size_t)i;
    if (__float_as_uint(r[4].w) & RT_FEATURE_HIT) {
        const float c = (float)cm.x;
        const float4 a = r[0], b = r[1], d = r[2];
        r[0] = make_float4(a.x / c, a.y / c, a.z / c, a.w / c);
        r[1] = make_float4(b.x / c, b.y / c, b.z / c, b.w);
        r[2] = make_float4(d.x / c, d.y / c, d.z / c, d.w);
    }
    cov[i] = make_float2((float)cm.x / (float)n, (float)cm.y / (float)n);
}

// Adaptive sampling (rt_render_adaptive), after each round: one wave per decision block, PT_MERGE_WAVES per workgroup.  A round has traced the active
// blocks into `scratch`, which is zero everywhere else, so scratch = 0 + the launch's per-pixel sum exactly, and
// accum + scratch is, bit for bit, what rt_render_spp of that launch would have made of accum.  Per pixel of an active
// block: accum += scratch, half += scratch in even rounds, scratch = 0; from round 1 on the pixel error (rt_amd.h)
// from I = accum / accum.w and A = half / half.w.  The block error is the mean over its in-frame pixels in a fixed
// order (lane l sums pixels l, l + 64, ... in turn, then an xor butterfly), and lane 0 decides whether the block is
// traced by the next round.  stats (PT_MERGE_REPLICAS rows, summed by the host): [0] blocks active next round,
// [1] blocks stopped at max_spp unconverged, [2] pixel samples of the blocks that stopped.
// With sample moments (RT_OPT_MOMENTS; m2 != NULL) the round's sample kernels have left the launch's own centred second
// moment in m2_scratch — scratch was zero, the merge rule's nA == 0 — and the pixel's state (accum, m2) takes the round's
// (scratch, m2_scratch) in with the merge rule (pt_moments.hpp) BEFORE accum += scratch; m2_scratch is zeroed with scratch.
struct MergeParams {
    uint32_t w, h;
    uint32_t bw_log2, bh_log2, blocks_x, blocks;
    uint32_t round;        // k
    uint32_t count;        // samples every pixel of an active block holds after this round
    uint32_t min_spp, max_spp;
    float threshold;
};

#define PT_MERGE_WAVES 4u       // decision blocks (one wave each) per workgroup
#define PT_MERGE_REPLICAS 64u    // rows of the stats counters, 128 bytes apart: one address took the whole frame's atomics
#define PT_MERGE_STRIDE 16u      // (MI355X, C2 1080p: 190-395 us per round on one row, most of the merge's time)
__global__ __launch_bounds__(64 * PT_MERGE_WAVES) void pt_adaptive_merge(MergeParams mp, float4 *__restrict__ accum, float4 *__restrict__ half,
                                                        float4 *__restrict__ scratch, uint32_t *__restrict__ active,
                                                        float *__restrict__ block_err, unsigned long long *__restrict__ stats,
                                                        float *__restrict__ m2, float *__restrict__ m2_scratch) {
    const uint32_t b = blockIdx.x * PT_MERGE_WAVES + (threadIdx.x >> 6);
    if (b >= mp.blocks || active[b] == 0u) return;   // (uniform over the wave; no workgroup barrier follows)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t bw = 1u << mp.bw_log2, area = bw << mp.bh_log2;
    const uint32_t x0 = (b % mp.blocks_x) << mp.bw_log2, y0 = (b / mp.blocks_x) << mp.bh_log2;
    const bool even = (mp.round & 1u) == 0u;
    float esum = 0.0f;
    uint32_t npx = 0u;
    for (uint32_t i = lane; i < area; i += 64u) {
        const uint32_t x = x0 + (i & (bw - 1u)), y = y0 + (i >> mp.bw_log2);
        if (x >= mp.w || y >= mp.h) continue;
        const size_t p = (size_t)y * mp.w + x;
        const float4 s = scratch[p];
        float4 m = accum[p];
        if (m2) {   // (uniform)
            m2[p] = moments_merge(m.w, m.x, m.y, m.z, m2[p], s.w, s.x, s.y, s.z, m2_scratch[p]);
            m2_scratch[p] = 0.0f;
        }
        m.x += s.x; m.y += s.y; m.z += s.z; m.w += s.w;
        accum[p] = m;
        float4 a = half[p];
        if (even) {
            a.x += s.x; a.y += s.y; a.z += s.z; a.w += s.w;
            half[p] = a;
        }
        scratch[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        npx++;
        if (mp.round >= 1u) {
            const float ix = m.x / m.w, iy = m.y / m.w, iz = m.z / m.w;
            const float ax = a.x / a.w, ay = a.y / a.w, az = a.z / a.w;
            const float den = sqrtf(ix + iy + iz);
            if (den > 0.0f) esum += (fabsf(ix - ax) + fabsf(iy - ay) + fabsf(iz - az)) / den;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        esum += __shfl_xor(esum, off);
        npx += __shfl_xor(npx, off);
    }
    if (lane != 0u) return;
    float err = 0.0f;
    if (mp.round >= 1u) {
        err = esum / (float)npx;
        block_err[b] = err;
    }
    const bool unconverged = mp.round == 0u || mp.threshold == 0.0f || !(err < mp.threshold);
    const bool next = mp.count < mp.max_spp && (mp.count < mp.min_spp || unconverged);
    active[b] = next ? 1u : 0u;
    stats += (size_t)(b % PT_MERGE_REPLICAS) * PT_MERGE_STRIDE;
    if (next) {
        atomicAdd(&stats[0], 1ull);
    } else {
        if (mp.count >= mp.max_spp && unconverged) atomicAdd(&stats[1], 1ull);
        atomicAdd(&stats[2], (unsigned long long)npx * mp.count);
    }
}

// The same pass for the variance-driven rule (rt_render_adaptive_variance): the shape, the pixel order, the butterfly and the
// stats rows are pt_adaptive_merge's, the moments are always kept (m2 != NULL), and no half buffer exists.  Per pixel of
// an active block: (accum, m2) takes (scratch, m2_scratch) in with the merge rule BEFORE accum += scratch, both scratches
// are zeroed, and with n = accum.w, L = l(accum.rgb / n) the pixel error — the standard error of the pixel's mean luminance
// over the root of that mean — is sqrt(M2 / (n (n - 1))) / sqrt(L), 0 where n < 2, L <= 0 or M2 <= 0.  It is written for
// every such pixel in every round, so pixel_err and block_err hold the values of the last round a block was traced in,
// and lane 0 decides from round 0 on.
__global__ __launch_bounds__(64 * PT_MERGE_WAVES) void pt_adaptive_merge_variance(MergeParams mp, float4 *__restrict__ accum,
                                                        float4 *__restrict__ scratch, uint32_t *__restrict__ active,
                                                        float *__restrict__ block_err, unsigned long long *__restrict__ stats,
                                                        float *__restrict__ m2, float *__restrict__ m2_scratch,
                                                        float *__restrict__ pixel_err) {
    const uint32_t b = blockIdx.x * PT_MERGE_WAVES + (threadIdx.x >> 6);
    if (b >= mp.blocks || active[b] == 0u) return;   // (uniform over the wave; no workgroup barrier follows)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t bw = 1u << mp.bw_log2, area = bw << mp.bh_log2;
    const uint32_t x0 = (b % mp.blocks_x) << mp.bw_log2, y0 = (b / mp.blocks_x) << mp.bh_log2;
    float esum = 0.0f;
    uint32_t npx = 0u;
    for (uint32_t i = lane; i < area; i += 64u) {
        const uint32_t x = x0 + (i & (bw - 1u)), y = y0 + (i >> mp.bw_log2);
        if (x >= mp.w || y >= mp.h) continue;
        const size_t p = (size_t)y * mp.w + x;
        const float4 s = scratch[p];
        float4 m = accum[p];
        const float mm = moments_merge(m.w, m.x, m.y, m.z, m2[p], s.w, s.x, s.y, s.z, m2_scratch[p]);
        m2[p] = mm;
        m2_scratch[p] = 0.0f;
        m.x += s.x; m.y += s.y; m.z += s.z; m.w += s.w;
        accum[p] = m;
        scratch[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        npx++;
        float e = 0.0f;
        if (m.w >= 2.0f) {
            const float lum = moments_lum(m.x / m.w, m.y / m.w, m.z / m.w);
            if (lum > 0.0f && mm > 0.0f) e = sqrtf(mm / (m.w * (m.w - 1.0f))) / sqrtf(lum);
        }
        pixel_err[p] = e;
        esum += e;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        esum += __shfl_xor(esum, off);
        npx += __shfl_xor(npx, off);
    }
    if (lane != 0u) return;
    const float err = esum / (float)npx;
    block_err[b] = err;
    const bool unconverged = mp.threshold == 0.0f || !(err < mp.threshold);
    const bool next = mp.count < mp.max_spp && (mp.count < mp.min_spp || unconverged);
    active[b] = next ? 1u : 0u;
    stats += (size_t)(b % PT_MERGE_REPLICAS) * PT_MERGE_STRIDE;
    if (next) {
        atomicAdd(&stats[0], 1ull);
    } else {
        if (mp.count >= mp.max_spp && unconverged) atomicAdd(&stats[1], 1ull);
        atomicAdd(&stats[2], (unsigned long long)npx * mp.count);
    }
}

// ================================== host side ==================================

namespace {

std::mutex g_err_mutex;
std::string g_create_error;

// Philox-4x32-10 random table — see rt_set_seed in rt_amd.h, DESIGN.md "random table"
void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int round = 0; round < 10; round++) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
inline float u24(uint32_t w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }

void make_table(uint64_t seed, float *out) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (uint32_t i = 0; i < RT_RANDOM_BUFFER_SIZE; i++) {
        uint32_t w[4];
        philox4x32_10(i, 0, 0, 0, k0, k1, w);
        out[3 * RT_RANDOM_BUFFER_SIZE + i] = u24(w[3]);
        for (uint32_t attempt = 0;; attempt++) {
            if (attempt) philox4x32_10(i, attempt, 0, 0, k0, k1, w);
            // volatile: keep each product/sum a separately rounded binary32 operation on the host
            volatile float x = 2.0f * u24(w[0]) - 1.0f, y = 2.0f * u24(w[1]) - 1.0f, z = 2.0f * u24(w[2]) - 1.0f;
            volatile float xx = x * x, yy = y * y, zz = z * z;
            volatile float s2 = xx + yy;
            volatile float s3 = s2 + zz;
            if (s3 < 1.0f) {
                out[3 * i] = x;
                out[3 * i + 1] = y;
                out[3 * i + 2] = z;
                break;
            }
        }
    }
}

}  // namespace

namespace rtamd {
int fail(rt_context *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->error = buf;
    else {
        std::lock_guard<std::mutex> lk(g_err_mutex);
        g_create_error = buf;
    }
    return code;
}
}  // namespace rtamd

namespace {

// pending look-ahead frames that no call will hand out any more
void lookahead_drop(rt_context *ctx) {
    rt_context::Lookahead &la = ctx->lookahead;
    la.discarded += la.pending;
    la.pending = 0;
}

// drops them unless they still continue the image as it lies: nothing they were computed from has changed since the batch
void lookahead_validate(rt_context *ctx) {
    const rt_context::Lookahead &la = ctx->lookahead;
    if (la.pending && (la.key_generation != ctx->prefix_cache.generation || la.key_epoch != ctx->image_epoch ||
                       la.next_sample != ctx->sample_counter + 1u))
        lookahead_drop(ctx);
}

int alloc_frame(rt_context *ctx, int w, int h) {
    // what was made for the old frame goes with it
    ctx->slots = {};
    ctx->prefix_changed();
    ctx->image_epoch++;
    lookahead_drop(ctx);
    ctx->lookahead.ring = {};
    ctx->lookahead.ring_frames = 0;
    ctx->lookahead.ring_failed = false;
    ctx->adaptive = {};
    ctx->features = {};
    ctx->denoise = {};
    ctx->moments.m2 = {};
    ctx->moments.valid = false;
    const size_t px = (size_t)w * h;
    HIP_TRY(ctx, ctx->image.alloc(px));
    HIP_TRY(ctx, ctx->accum.alloc(px));
    HIP_TRY(ctx, hipMemset(ctx->image.p, 0, px * sizeof(float4)));
    HIP_TRY(ctx, hipMemset(ctx->accum.p, 0, px * sizeof(float4)));
    ctx->width = w;
    ctx->height = h;
    ctx->accum_count = 0;
    ctx->clear_pending = false;   // (the new accumulator IS zero)
    ctx->sample_counter = 0;
    return RT_OK;
}

int check_ready(rt_context *ctx, const float *cam) {
    if (!ctx) return RT_EINVAL;
    if (!cam) return fail(ctx, RT_EINVAL, "camera block is NULL");
    if (!ctx->have_scene) return fail(ctx, RT_ESTATE, "no scene: call rt_set_scene first");
    if (ctx->scene_uses_textures && (ctx->tex_layers <= 0 || ctx->max_texture_id >= (uint32_t)ctx->tex_layers))
        return fail(ctx, RT_ERANGE, "scene has textured meshes (max texture id %u) but only %d texture layers are set",
                    ctx->max_texture_id, ctx->tex_layers);
    return RT_OK;
}

}  // namespace

namespace rtamd {
int read_back(rt_context *ctx, void *dst, size_t bytes, const void *src, size_t need, const char *what, bool ready,
              const char *producer) {
    if (!dst || bytes != need) return fail(ctx, RT_EINVAL, "%s buffer must be %zu bytes", what, need);
    if (!ready) return fail(ctx, RT_ESTATE, "no %s call since the frame was (re)allocated", producer);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    CLEAR_TRY(ctx);   // (src may be the accumulator or made from it)
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, need, hipMemcpyDeviceToHost, ctx->stream));
    SYNC_TRY(ctx);
    return RT_OK;
}
}  // namespace rtamd

namespace {

// Everything on the device that depends on the arithmetic policy (rt_set_scene, rt_set_option(RT_OPT_ARITH)):
//   * the spheres' test records (centre, w) of the brute-force loop (sph4: whole batches + one dummy batch that the
//     prefetch of the last iteration reads) and of the BVH leaves (bvh_sph): w = r*r, the one rounded binary32 product
//     hitSphere forms (:152), for policies 0 and 1; w = r for policy 2, where the product is contracted into
//     fma(-r, r, dot(oc, oc)) and never exists on its own.  Dummies: w = -inf (discriminant -inf) resp. NaN;
//   * the unit normal of every face record (A, e1, e2, n): host-computed IEEE operations for policy 0
//     (build_face_records), the policy's own cross / rsq-based normalize ON THE DEVICE for policies 1 and 2.
int apply_arith(rt_context *ctx) {
    const bool w_is_radius = ctx->arith == RT_ARITH_ROCM_OCL;
    auto rec = [&](const rt_sphere &s) {
        volatile float r2 = s.r * s.r;
        return make_float4(s.pos.x, s.pos.y, s.pos.z, w_is_radius ? s.r : (float)r2);
    };
    const uint32_t n = (uint32_t)ctx->h_spheres.size();
    const uint32_t batches = (n + PT_SPHERE_BATCH - 1) / PT_SPHERE_BATCH;
    std::vector<float4> v((size_t)(batches + 1) * PT_SPHERE_BATCH, make_float4(0.0f, 0.0f, 0.0f, w_is_radius ? NAN : -INFINITY));
    for (uint32_t i = 0; i < n; i++) v[i] = rec(ctx->h_spheres[i]);
    HIP_TRY(ctx, ctx->sph4.upload(v.data(), v.size()));
    ctx->sphere_batches = batches;
    if (!ctx->h_bvh_idx.empty()) {
        std::vector<float4> leaf(ctx->h_bvh_idx.size());
        for (size_t i = 0; i < leaf.size(); i++) leaf[i] = rec(ctx->h_spheres[ctx->h_bvh_idx[i]]);
        HIP_TRY(ctx, ctx->bvh_sph.upload(leaf.data(), leaf.size()));
    }
    HIP_TRY(ctx, ctx->faces.upload(ctx->h_faces.data(), ctx->h_faces.size()));
    HIP_TRY(ctx, ctx->mbvh_faces.upload(ctx->h_mbvh_faces.data(), ctx->h_mbvh_faces.size()));
    if (ctx->arith != RT_ARITH_IEEE) {
        int rc = ctx->ks->launch_face_normals(ctx, ctx->faces.p, (uint32_t)(ctx->h_faces.size() / 3));
        if (rc == RT_OK) rc = ctx->ks->launch_face_normals(ctx, ctx->mbvh_faces.p, (uint32_t)(ctx->h_mbvh_faces.size() / 3));
        if (rc != RT_OK) return rc;
        SYNC_TRY(ctx);
    }
    return RT_OK;
}

}  // namespace

// ================================== C ABI =====================================

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

const char *rt_last_error(const rt_context *ctx) {
    if (ctx) return ctx->error.c_str();
    std::lock_guard<std::mutex> lk(g_err_mutex);
    return g_create_error.c_str();
}

int rt_make_random_table(uint64_t seed, float *out, size_t n) {
    if (!out || n != RT_RANDOM_TABLE_FLOATS) return fail(nullptr, RT_EINVAL, "table must hold %d floats", RT_RANDOM_TABLE_FLOATS);
    make_table(seed, out);
    return RT_OK;
}

int rt_create(int device, int width, int height, rt_context **out) {
    if (!out) return fail(nullptr, RT_EINVAL, "out is NULL");
    *out = nullptr;
    if (width < 1 || height < 1 || width > RT_MAX_DIM || height > RT_MAX_DIM)
        return fail(nullptr, RT_EINVAL, "frame size %dx%d outside 1..%d", width, height, RT_MAX_DIM);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
        return fail(nullptr, RT_ENODEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= n) return fail(nullptr, RT_ENODEVICE, "device %d out of range (%d visible)", device, n);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, RT_EHIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, RT_ENODEVICE, "device %d is %s; librt_amd.so carries gfx950 code only", device,
                    prop.gcnArchName);
    rt_context *ctx = new (std::nothrow) rt_context();
    if (!ctx) return fail(nullptr, RT_EHIP, "out of host memory");
    ctx->device = device;
    ctx->dev_name = prop.name;
    ctx->dev_arch = prop.gcnArchName;
    ctx->cu_count = prop.multiProcessorCount;
    int rc = RT_OK;
    auto bail = [&](int code) {
        {
            std::lock_guard<std::mutex> lk(g_err_mutex);
            g_create_error = ctx->error;
        }
        rt_destroy(ctx);
        return code;
    };
    if (hipSetDevice(device) != hipSuccess) { ctx->error = "hipSetDevice failed"; return bail(RT_EHIP); }
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) { ctx->error = "hipStreamCreate failed"; return bail(RT_EHIP); }
    ctx->stream = ctx->own_stream;
    for (int i = 0; i < rt_context::EV_RING; i++)
        if (hipEventCreate(&ctx->ev[i][0]) != hipSuccess || hipEventCreate(&ctx->ev[i][1]) != hipSuccess || hipEventCreate(&ctx->ev[i][2]) != hipSuccess) { ctx->error = "hipEventCreate failed"; return bail(RT_EHIP); }
    if (ctx->counters.alloc(COUNTER_REPLICAS * COUNTER_STRIDE + 32) != hipSuccess ||
        hipMemset(ctx->counters.p, 0, (COUNTER_REPLICAS * COUNTER_STRIDE + 32) * sizeof(unsigned long long)) != hipSuccess) { ctx->error = "counter allocation failed"; return bail(RT_EHIP); }
    ctx->d_walk_overflow = reinterpret_cast<uint32_t *>(ctx->counters.p + COUNTER_REPLICAS * COUNTER_STRIDE + 24);

    ctx->arith = RT_ARITH_IEEE;
    ctx->ks = kernel_set_a0();
    // (the environment may switch the prefix cache off for a whole process: A/B of an unchanged caller)
    if (const char *e = getenv("RT_PREFIX_CACHE")) ctx->prefix_cache.enabled = strcmp(e, "0") != 0;
    if (const char *e = getenv("RT_LOOKAHEAD")) { if (strcmp(e, "0") == 0) ctx->lookahead.k = 0; }   // (likewise)
    if (const char *e = getenv("RT_EXACT_GRID")) ctx->sample_grid.exact = strcmp(e, "0") != 0;       // (likewise)
    if (hipHostMalloc((void **)&ctx->sample_grid.h_counts, LIVE_COUNT_STRIDE * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->sample_grid.counts_ev, hipEventDisableTiming) != hipSuccess) { ctx->error = "live-count read-back allocation failed"; return bail(RT_EHIP); }
    if ((rc = alloc_frame(ctx, width, height)) != RT_OK) return bail(rc);
    if ((rc = rt_set_seed(ctx, 0xC0FFEEull)) != RT_OK) return bail(rc);
    if ((rc = rt_set_textures(ctx, nullptr, 0, 0, 0)) != RT_OK) return bail(rc);
    *out = ctx;
    return RT_OK;
}

void rt_destroy(rt_context *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
    for (int i = 0; i < rt_context::EV_RING; i++)
        for (int k = 0; k < 3; k++)
            if (ctx->ev[i][k]) (void)hipEventDestroy(ctx->ev[i][k]);
    if (ctx->sample_grid.counts_ev) (void)hipEventDestroy(ctx->sample_grid.counts_ev);
    if (ctx->sample_grid.h_counts) (void)hipHostFree(ctx->sample_grid.h_counts);
    for (hipEvent_t e : ctx->cameras.read)
        if (e) (void)hipEventDestroy(e);
    if (ctx->cameras.h_table) (void)hipHostFree(ctx->cameras.h_table);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int rt_resize(rt_context *ctx, int width, int height) {
    if (!ctx) return RT_EINVAL;
    if (width < 1 || height < 1 || width > RT_MAX_DIM || height > RT_MAX_DIM)
        return fail(ctx, RT_EINVAL, "frame size %dx%d outside 1..%d", width, height, RT_MAX_DIM);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SYNC_TRY(ctx);
    return alloc_frame(ctx, width, height);
}

int rt_set_stream(rt_context *ctx, void *hip_stream) {
    if (!ctx) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SYNC_TRY(ctx);
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    ctx->prefix_changed();
    ctx->ev_count = 0;
    return RT_OK;
}

int rt_set_scene(rt_context *ctx, const rt_scene_desc *d) {
    if (!ctx) return RT_EINVAL;
    if (!d) return fail(ctx, RT_EINVAL, "scene is NULL");
    ctx->prefix_changed();
    {
        PreparedScene ps;
        std::string err;
        if (int rc = prepare_scene(*d, ps, err)) return fail(ctx, rc, "%s", err.c_str());
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        SYNC_TRY(ctx);
        ctx->have_scene = false;
        // (behind the materials: room for the staged scene block, rt_context::StageBlock)
        HIP_TRY(ctx, ctx->materials.upload(d->materials, d->material_count,
                                           lds_static_used(d->material_count, d->sphere_count, d->plane_count) * sizeof(float4)));
        ctx->stage_block.generation = ~0ull;
        HIP_TRY(ctx, ctx->spheres.upload(d->spheres, d->sphere_count));
        ctx->h_spheres.assign(d->spheres, d->spheres + d->sphere_count);   // the test records follow in apply_arith()
        HIP_TRY(ctx, ctx->mesh_face_base.upload(ps.face_base.data(), ps.face_base.size()));
        HIP_TRY(ctx, ctx->mbvh_nodes.upload(ps.mesh_packed.data(), ps.mesh_packed.size()));
        ctx->have_mesh_bvh = ps.have_mesh_bvh;
        HIP_TRY(ctx, ctx->mbvh_face_idx.upload(ps.leaf_face_idx.data(), ps.leaf_face_idx.size()));
        HIP_TRY(ctx, ctx->mesh_bvh_root.upload(ps.mesh_roots.data(), ps.mesh_roots.size()));
        ctx->walk_jobs.release();
        if (!ps.walk_jobs.empty()) HIP_TRY(ctx, ctx->walk_jobs.upload(ps.walk_jobs.data(), ps.walk_jobs.size()));
        ctx->bvh_node_count = ps.bvh_node_count;
        if (!ps.sphere_nodes.empty()) {   // (without a tree the arrays and bounds of the last one stay, unused: bvh_node_count is 0)
            HIP_TRY(ctx, ctx->bvh_nodes.upload(ps.sphere_boxes.data(), ps.sphere_boxes.size()));
            HIP_TRY(ctx, ctx->bvh_links.upload(ps.sphere_links.data(), ps.sphere_links.size()));
            HIP_TRY(ctx, ctx->bvh_idx.upload(ps.sphere_leaf_idx.data(), ps.sphere_leaf_idx.size()));
            ctx->bvh_rmax = ps.bvh_rmax;
            for (int k = 0; k < 3; k++) { ctx->bvh_lo[k] = ps.bvh_lo[k]; ctx->bvh_hi[k] = ps.bvh_hi[k]; }
        }
        HIP_TRY(ctx, ctx->planes.upload(d->planes, d->plane_count));
        HIP_TRY(ctx, ctx->lenses.upload(d->lenses, d->lens_count));
        HIP_TRY(ctx, ctx->vertices.upload(d->vertices, d->vertex_count));
        if (d->uv_count) HIP_TRY(ctx, ctx->uvs.upload(d->uvs, d->uv_count));
        else {
            std::vector<rt_float2> zeros(d->vertex_count ? d->vertex_count : 1, rt_float2{0.0f, 0.0f});
            HIP_TRY(ctx, ctx->uvs.upload(zeros.data(), d->vertex_count));
        }
        HIP_TRY(ctx, ctx->indices.upload(d->indices, d->index_count));
        HIP_TRY(ctx, ctx->meshes.upload(d->meshes, d->mesh_count));
        HIP_TRY(ctx, ctx->models.upload(d->models, d->model_count));
        ctx->scene_uses_textures = ps.uses_tex;
        ctx->max_texture_id = ps.max_tex;
        // what depends on the arithmetic policy is uploaded by apply_arith() from these: the spheres' and the leaves' test
        // records, the face records and the leaf faces with their normals
        ctx->h_bvh_idx.swap(ps.sphere_leaf_idx);
        ctx->h_faces.swap(ps.faces);
        ctx->h_mbvh_faces.swap(ps.leaf_faces);
    }   // (the upload sources are freed before apply_arith() allocates its records: the host's peak is the builders')
    if (int rc = apply_arith(ctx)) return rc;
    ctx->have_scene = true;
    ctx->sample_counter = 0;
    return RT_OK;
}

int rt_set_textures(rt_context *ctx, const float *rgba, int w, int h, int layers) {
    if (!ctx) return RT_EINVAL;
    ctx->prefix_changed();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SYNC_TRY(ctx);
    if (layers == 0) {
        float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        HIP_TRY(ctx, ctx->tex.upload(&zero, 1));
        ctx->tex_w = ctx->tex_h = 1;
        ctx->tex_layers = 0;
        return RT_OK;
    }
    if (!rgba || w < 1 || h < 1 || layers < 1 || w > 32768 || h > 32768 || layers > 2048)
        return fail(ctx, RT_EINVAL, "bad texture array %dx%dx%d", w, h, layers);
    HIP_TRY(ctx, ctx->tex.upload((const float4 *)rgba, (size_t)w * h * layers));
    ctx->tex_w = w;
    ctx->tex_h = h;
    ctx->tex_layers = layers;
    return RT_OK;
}

int rt_set_random_table(rt_context *ctx, const float *table, size_t n) {
    if (!ctx) return RT_EINVAL;
    if (!table || n != RT_RANDOM_TABLE_FLOATS) return fail(ctx, RT_EINVAL, "table must hold %d floats", RT_RANDOM_TABLE_FLOATS);
    ctx->prefix_changed();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SYNC_TRY(ctx);
    // 2 floats of slack: getVec reads idx..idx+2 with idx < 100000 — inside the table already
    HIP_TRY(ctx, ctx->table.upload(table, n));
    return RT_OK;
}

int rt_set_seed(rt_context *ctx, uint64_t seed) {
    if (!ctx) return RT_EINVAL;
    std::vector<float> t(RT_RANDOM_TABLE_FLOATS);
    make_table(seed, t.data());
    return rt_set_random_table(ctx, t.data(), t.size());
}

int rt_get_random_table(rt_context *ctx, float *out, size_t n) {
    if (!ctx) return RT_EINVAL;
    if (!out || n != RT_RANDOM_TABLE_FLOATS) return fail(ctx, RT_EINVAL, "table must hold %d floats", RT_RANDOM_TABLE_FLOATS);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SYNC_TRY(ctx);
    HIP_TRY(ctx, hipMemcpy(out, ctx->table.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_set_shard(rt_context *ctx, int rank, int world, int tile_w, int tile_h) {
    if (!ctx) return RT_EINVAL;
    auto log2_exact = [](int v) { int l = 0; while ((1 << l) < v) l++; return (1 << l) == v ? l : -1; };
    int lw = log2_exact(tile_w), lh = log2_exact(tile_h);
    if (world < 1 || rank < 0 || rank >= world) return fail(ctx, RT_EINVAL, "rank %d of %d", rank, world);
    if (world > 1 && ctx->moments.on) return fail(ctx, RT_EINVAL, "RT_OPT_MOMENTS is 1: sample moments are kept on unsharded contexts only");
    if (tile_w < 1 || tile_h < 1 || lw < 0 || lh < 0 || lw + lh > 16)
        return fail(ctx, RT_EINVAL, "tile %dx%d: sides must be powers of two, area <= 65536", tile_w, tile_h);
    ctx->prefix_changed();
    ctx->rank = rank;
    ctx->world = world;
    ctx->tile_w_log2 = lw;
    ctx->tile_h_log2 = lh;
    return RT_OK;
}

extern "C++" {
namespace {

#if PT_RING_PIXEL_MAJOR
__global__ __launch_bounds__(256) void pt_ring_handout(const float4 *__restrict__ ring, float4 *__restrict__ image, size_t n,
                                                       uint32_t frames, uint32_t j) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) image[i] = ring[i * frames + j];
}
#endif

// frames a batch of a w x h frame may have at this sample counter: min(option, samples left, frames in the budget); < 2 = none
uint32_t lookahead_frames(int w, int h, int k, uint32_t sample_counter) {
    if (k < 2 || sample_counter >= RT_MAX_SAMPLE) return 0u;
    const uint64_t frame_bytes = (uint64_t)w * (uint64_t)h * sizeof(float4);
    uint64_t n = std::min<uint64_t>((uint64_t)k, RT_MAX_SAMPLE - sample_counter);
    n = std::min<uint64_t>(n, RT_LOOKAHEAD_MAX_BYTES / frame_bytes);
    return n >= 2u ? (uint32_t)n : 0u;
}

// The ring holds kp frames of this frame size — allocated for as many as any batch of this size and option can have.
// false: it cannot be had (not an error: the direct path).
bool lookahead_ring(rt_context *ctx, uint32_t kp) {
    rt_context::Lookahead &la = ctx->lookahead;
    if (la.ring_frames >= kp) return true;
    if (la.ring_failed) return false;
    const uint32_t frames = lookahead_frames(ctx->width, ctx->height, la.k, 0u);
    la.ring_frames = 0;
    if (la.ring.alloc((size_t)frames * ctx->width * ctx->height) != hipSuccess) {
        (void)hipGetLastError();
        la.ring_failed = true;
        return false;
    }
    la.ring_frames = frames;
    return true;
}

// The batch a call that repeats the previous call's camera (rt_render_again) or table (rt_render_again_cameras) may start
// (0: the direct path): the context must be one a look-ahead launch can serve (lookahead_ok, pt_kernels.hip), and the ring
// must exist.  Camera launches share no prefix: RT_OPT_PREFIX_SHARING matters to the plain call only.
uint32_t lookahead_batch_any(rt_context *ctx, bool cameras) {
    rt_context::Lookahead &la = ctx->lookahead;
    if (ctx->count_enabled || ctx->world != 1 || (!cameras && !ctx->prefix_sharing) || !ctx->sample_queue) return 0u;
    uint32_t kp = 0;
    if (rt_lookahead_plan(ctx->width, ctx->height, la.k, ctx->sample_counter, &kp) != RT_OK || kp < 2u) return 0u;
    if ((ctx->max_threads_per_launch >> group_log2_for(kp)) < shard_of(ctx, 0, 1).slots) return 0u;   // several slot ranges
    return lookahead_ring(ctx, kp) ? kp : 0u;
}
uint32_t lookahead_batch(rt_context *ctx, const uint32_t cam_bits[12]) {
    const rt_context::Lookahead &la = ctx->lookahead;
    if (!la.have_last_cam || memcmp(la.last_cam, cam_bits, sizeof la.last_cam) != 0) return 0u;
    return lookahead_batch_any(ctx, false);
}

// a batch of kp frames has just been launched for the samples behind the counter
void lookahead_begin(rt_context *ctx, uint32_t kp, bool table) {
    rt_context::Lookahead &la = ctx->lookahead;
    la.batches++;
    la.pending = la.batch_frames = kp;
    la.next_frame = 0;
    la.next_sample = ctx->sample_counter + 1u;
    la.key_generation = ctx->prefix_cache.generation;   // (after the launch: ensure_slots may have bumped it)
    la.key_epoch = ctx->image_epoch;
    la.key_is_table = table;
}

// Hands the next pending frame out: device copy into the image, then synchronise.  timed: the call has its entry in the
// event history already (it launched the batch).
int lookahead_hand_out(rt_context *ctx, bool timed) {
    rt_context::Lookahead &la = ctx->lookahead;
    const size_t frame_px = (size_t)ctx->width * ctx->height;
    hipEvent_t *evp = ctx->ev[ctx->ev_count % rt_context::EV_RING];
    if (!timed) {
        HIP_TRY(ctx, hipEventRecord(evp[0], ctx->stream));
        HIP_TRY(ctx, hipEventRecord(evp[2], ctx->stream));   // no first stage
    }
#if PT_RING_PIXEL_MAJOR   // (A/B variant: a pixel's frames lie side by side, the hand-out gathers one of them)
    hipLaunchKernelGGL(pt_ring_handout, dim3((unsigned)((frame_px + 255) / 256)), dim3(256), 0, ctx->stream, la.ring.p, ctx->image.p,
                       frame_px, la.batch_frames, la.next_frame);
    HIP_TRY(ctx, hipGetLastError());
#else
    HIP_TRY(ctx, hipMemcpyAsync(ctx->image.p, la.ring.p + (size_t)la.next_frame * frame_px, frame_px * sizeof(float4),
                                hipMemcpyDeviceToDevice, ctx->stream));
#endif
    if (!timed) {
        HIP_TRY(ctx, hipEventRecord(evp[1], ctx->stream));
        ctx->ev_count++;
    }
    la.pending--;
    la.next_frame++;
    la.next_sample++;
    la.served++;
    ctx->sample_counter++;  // src/raytracer.cpp:147
    SYNC_TRY(ctx);
    return RT_OK;
}

void remember_camera(rt_context *ctx, const float camera[12]) {
    memcpy(ctx->lookahead.last_cam, camera, sizeof ctx->lookahead.last_cam);
    ctx->lookahead.have_last_cam = true;
}

}  // namespace
}  // extern "C++"

int rt_lookahead_plan(int width, int height, int option_value, uint32_t sample_counter, uint32_t *batch_out) {
    if (!batch_out) return fail(nullptr, RT_EINVAL, "batch_out is NULL");
    *batch_out = 0;
    if (width < 1 || height < 1 || width > RT_MAX_DIM || height > RT_MAX_DIM)
        return fail(nullptr, RT_EINVAL, "frame size %dx%d outside 1..%d", width, height, RT_MAX_DIM);
    if (option_value < 0 || option_value == 1 || option_value > RT_LOOKAHEAD_MAX)
        return fail(nullptr, RT_EINVAL, "RT_OPT_LOOKAHEAD takes 0 or 2..%d", RT_LOOKAHEAD_MAX);
    *batch_out = lookahead_frames(width, height, option_value, sample_counter);
    return RT_OK;
}

int rt_lookahead_stats(rt_context *ctx, uint64_t *batches, uint64_t *served, uint64_t *direct, uint64_t *discarded) {
    if (!ctx || !batches || !served || !direct || !discarded) return RT_EINVAL;
    lookahead_validate(ctx);   // (frames that can no longer be handed out count as dropped from the change on)
    *batches = ctx->lookahead.batches;
    *served = ctx->lookahead.served;
    *direct = ctx->lookahead.direct;
    *discarded = ctx->lookahead.discarded;
    return RT_OK;
}

int rt_render(rt_context *ctx, const float camera[12]) {
    int rc = check_ready(ctx, camera);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->image_epoch++;
    lookahead_drop(ctx);
    remember_camera(ctx, camera);
    ctx->sample_counter = 0;  // src/raytracer.cpp:128
    if ((rc = ctx->ks->launch_render(ctx, MODE_TRACE, camera, 0, 1, 0, ctx->accum.p, nullptr, nullptr)) != RT_OK) return rc;
    SYNC_TRY(ctx);  // queue.finish(), src/raytracer.cpp:140
    return RT_OK;
}

int rt_render_again(rt_context *ctx, const float camera[12]) {
    int rc = check_ready(ctx, camera);
    if (rc) return rc;
    if (ctx->sample_counter >= RT_MAX_SAMPLE) return fail(ctx, RT_EINVAL, "sample counter limit %u reached", RT_MAX_SAMPLE);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // Look-ahead (RT_OPT_LOOKAHEAD): the image after sample k is a pure function of the image after sample k - 1 and of
    // sample k, so while the camera rests one fused launch computes the next frames and the calls hand them out.
    rt_context::Lookahead &la = ctx->lookahead;
    uint32_t cam_bits[12];
    memcpy(cam_bits, camera, sizeof cam_bits);
    lookahead_validate(ctx);
    if (la.pending && (la.key_is_table || memcmp(la.key_cam, cam_bits, sizeof cam_bits) != 0)) lookahead_drop(ctx);
    la.have_last_table = false;   // (a plain call between two table calls: the next table call repeats none)
    bool timed = false;   // the call has its entry in the event history
    if (!la.pending) {
        const uint32_t kp = lookahead_batch(ctx, cam_bits);
        if (kp) {
            if ((rc = ctx->ks->launch_lookahead(ctx, camera, ctx->sample_counter + 1u, kp, la.ring.p)) != RT_OK) return rc;
            timed = true;
            lookahead_begin(ctx, kp, false);
            memcpy(la.key_cam, cam_bits, sizeof cam_bits);
        }
    }
    remember_camera(ctx, camera);
    if (la.pending) return lookahead_hand_out(ctx, timed);
    ctx->image_epoch++;
    la.direct++;
    ctx->sample_counter++;  // src/raytracer.cpp:147
    if ((rc = ctx->ks->launch_render(ctx, MODE_RETRACE, camera, ctx->sample_counter, 1, 0, ctx->accum.p, nullptr, nullptr)) != RT_OK) return rc;
    SYNC_TRY(ctx);
    return RT_OK;
}

int rt_sample_counter(const rt_context *ctx, uint32_t *out) {
    if (!ctx || !out) return RT_EINVAL;
    *out = ctx->sample_counter;
    return RT_OK;
}

extern "C++" {
namespace {
// The sample moments start anew with the accumulator (rt_clear, rt_render_adaptive) while RT_OPT_MOMENTS is 1: the buffer is
// made on the first such call since the frame was (re)allocated, zeroed on the stream, and valid from here on.
int moments_begin(rt_context *ctx) {
    rt_context::Moments &mo = ctx->moments;
    if (!mo.on) return RT_OK;
    const size_t px = (size_t)ctx->width * ctx->height;
    mo.valid = false;
    if (!mo.m2.p) HIP_TRY(ctx, mo.m2.alloc(px));
    HIP_TRY(ctx, hipMemsetAsync(mo.m2.p, 0, px * sizeof(float), ctx->stream));
    mo.valid = true;
    return RT_OK;
}

// Samples first .. first+c-1 of one camera into `target` (and `m2`): the fused launch, or every sample from the camera where
// prefix sharing is switched off.
int launch_camera_samples(rt_context *ctx, const float camera[12], uint32_t first, uint32_t c, float4 *target, const BlockMask *mask, float *m2) {
    return ctx->prefix_sharing ? ctx->ks->launch_fused(ctx, camera, first, c, group_log2_for(c), target, mask, m2)
                               : ctx->ks->launch_render(ctx, MODE_ACCUM, camera, first, c, group_log2_for(c), target, mask, m2);
}

// A call of more than RT_SPP_PER_LAUNCH samples per pixel runs as consecutive launches of that many (the capacity of a
// wave's sample queue: beyond it a frame would fall back to the fixed-lane kernel, 1.8 x slower — 520 samples took
// 18.4 ms where 512 take 10.2); the target then holds the sum of those launches' sums, on every path alike.
// launch(done, c): samples done .. done+c-1 of the call; the first failure ends it.
template <class Launch>
int for_each_launch(uint32_t n_samples, Launch launch) {
    for (uint32_t done = 0; done < n_samples;) {
        const uint32_t c = n_samples - done < RT_SPP_PER_LAUNCH ? n_samples - done : RT_SPP_PER_LAUNCH;
        const int rc = launch(done, c);
        if (rc != RT_OK) return rc;
        done += c;
    }
    return RT_OK;
}
}  // namespace
}  // extern "C++"

int rt_clear(rt_context *ctx) {
    if (!ctx) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // RT_OPT_ACCUM_STORE 1: the clear is recorded, not enqueued — a fused launch that writes every pixel stores its sums into
    // the frame as it lies (launch_fused_any), and whatever else comes next enqueues the memset first (materialise_clear).
    // A clear that is still pending is enqueued before this one is recorded.
    CLEAR_TRY(ctx);
    if (ctx->accum_store) ctx->clear_pending = true;
    else HIP_TRY(ctx, hipMemsetAsync(ctx->accum.p, 0, (size_t)ctx->width * ctx->height * sizeof(float4), ctx->stream));
    ctx->accum_count = 0;
    return moments_begin(ctx);
}

int rt_render_spp(rt_context *ctx, const float camera[12], uint32_t first_sample, uint32_t n_samples) {
    int rc = check_ready(ctx, camera);
    if (rc) return rc;
    if (n_samples == 0) return RT_OK;
    if ((uint64_t)first_sample + n_samples - 1 > RT_MAX_SAMPLE)
        return fail(ctx, RT_EINVAL, "samples %u..+%u exceed the limit %u", first_sample, n_samples, RT_MAX_SAMPLE);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return for_each_launch(n_samples, [&](uint32_t done, uint32_t c) {
        const int r = launch_camera_samples(ctx, camera, first_sample + done, c, ctx->accum.p, nullptr, ctx->moments.target());
        if (r == RT_OK) ctx->accum_count += c;
        return r;
    });
}

extern "C++" {
namespace {
// the context's camera tables (rt_context::Cameras), made on the first camera call
int ensure_cameras(rt_context *ctx) {
    rt_context::Cameras &cm = ctx->cameras;
    if (cm.table.p) return RT_OK;
    const size_t floats = (size_t)rt_context::Cameras::RING * RT_SPP_PER_LAUNCH * 12u;
    if (!cm.h_table) HIP_TRY(ctx, hipHostMalloc((void **)&cm.h_table, floats * sizeof(float), hipHostMallocDefault));
    for (hipEvent_t &e : cm.read)
        if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(ctx, cm.table.alloc(floats));
    return RT_OK;
}

// One launch's blocks on their way to the device: `c` <= RT_SPP_PER_LAUNCH blocks go into table k of the ring — after the
// table's last reader, through the pinned host table, onto the stream.  The launch then reads `d` (cam0: `h`), and
// camera_table_read records its kernels as the table's reader.  Every call that sends camera blocks goes through these two.
struct CameraTable {
    uint32_t k;
    const float *d, *h;
};
int camera_table_send(rt_context *ctx, const float *blocks, uint32_t c, CameraTable *t) {
    rt_context::Cameras &cm = ctx->cameras;
    t->k = (uint32_t)(cm.launches % rt_context::Cameras::RING);
    const size_t at = (size_t)t->k * RT_SPP_PER_LAUNCH * 12u;
    if (cm.launches >= rt_context::Cameras::RING) HIP_TRY(ctx, hipEventSynchronize(cm.read[t->k]));   // (table k's last reader)
    memcpy(cm.h_table + at, blocks, (size_t)c * 12u * sizeof(float));
    HIP_TRY(ctx, hipMemcpyAsync(cm.table.p + at, cm.h_table + at, (size_t)c * 12u * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    cm.launches++;
    t->d = cm.table.p + at;
    t->h = cm.h_table + at;
    return RT_OK;
}
int camera_table_read(rt_context *ctx, const CameraTable &t) {
    HIP_TRY(ctx, hipEventRecord(ctx->cameras.read[t.k], ctx->stream));
    return RT_OK;
}
}  // namespace
}  // extern "C++"

int rt_render_spp_cameras(rt_context *ctx, const float *cameras, uint32_t first_sample, uint32_t n_samples) {
    int rc = check_ready(ctx, cameras);
    if (rc) return rc;
    if (n_samples == 0) return RT_OK;
    if ((uint64_t)first_sample + n_samples - 1 > RT_MAX_SAMPLE)
        return fail(ctx, RT_EINVAL, "samples %u..+%u exceed the limit %u", first_sample, n_samples, RT_MAX_SAMPLE);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_cameras(ctx)) != RT_OK) return rc;
    return for_each_launch(n_samples, [&](uint32_t done, uint32_t c) {
        CameraTable tb;
        int r = camera_table_send(ctx, cameras + (size_t)done * 12u, c, &tb);
        if (r != RT_OK) return r;
        r = ctx->ks->launch_cameras(ctx, tb.d, tb.h, first_sample + done, c, group_log2_for(c), ctx->accum.p, nullptr,
                                    ctx->moments.target(), nullptr);
        const int rd = camera_table_read(ctx, tb);
        if (rd == RT_OK && r == RT_OK) ctx->accum_count += c;
        return rd != RT_OK ? rd : r;
    });
}

// ---- caller-supplied rays ------------------------------------------------------------------------------------------------
static_assert(sizeof(rt_ray) == 32 && alignof(rt_ray) == 16, "an rt_ray is two float4: (o, x bits), (d, y bits)");

int rt_upload_rays(rt_context *ctx, const rt_ray *host, size_t n) {
    if (!ctx) return RT_EINVAL;
    if (!host || n == 0 || n > RT_MAX_RAYS) return fail(ctx, RT_EINVAL, "rt_upload_rays takes 1 .. %u rays", RT_MAX_RAYS);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rt_context::Rays &ry = ctx->rays;
    if (n > ry.buf.n) {   // grow: a new array first, so that a failed allocation leaves the old rays as they were
        DevBuf<rt_ray> grown;
        if (grown.alloc(n) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, RT_EHIP, "no device memory for %zu rays", n);
        }
        ry.buf = std::move(grown);   // (the old array is freed here: hipFree waits for the launches that read it)
        ry.count = 0;
    }
    HIP_TRY(ctx, hipMemcpyAsync(ry.buf.p, host, n * sizeof(rt_ray), hipMemcpyHostToDevice, ctx->stream));
    ry.count = n;
    return RT_OK;
}

int rt_device_rays(rt_context *ctx, void **d_rays, size_t *n) {
    if (!ctx || !d_rays || !n) return RT_EINVAL;
    *d_rays = ctx->rays.count ? ctx->rays.buf.p : nullptr;
    *n = ctx->rays.count;
    return RT_OK;
}

extern "C++" {
namespace {
const float k_no_camera[12] = {};   // a ray call has no camera block: check_ready's other rules apply
// the ray buffer of a ray call: the caller's, or the uploaded rays (at least n_rays of them); NULL + a recorded RT_EINVAL
const void *ray_source(rt_context *ctx, const void *d_rays, size_t n_rays) {
    if (d_rays) {
        if ((uintptr_t)d_rays % alignof(rt_ray)) { (void)fail(ctx, RT_EINVAL, "d_rays is not 16-byte aligned"); return nullptr; }
        return d_rays;
    }
    if (ctx->rays.count < n_rays) {
        (void)fail(ctx, RT_EINVAL, "%zu rays asked for, %zu uploaded (rt_upload_rays)", n_rays, ctx->rays.count);
        return nullptr;
    }
    return ctx->rays.buf.p;
}
}  // namespace
}  // extern "C++"

extern "C++" {
namespace {
// The rules of the ray arguments alone, which the ray queries share: RT_OK and the number of records in *records_out
int check_ray_records(rt_context *ctx, const char *call, size_t n_rays, uint32_t set_size, bool sets, size_t *records_out) {
    if (ctx->world > 1) return fail(ctx, RT_EINVAL, "rays on a sharded context (rank %d of %d): shard the batch instead", ctx->rank, ctx->world);
    if (n_rays == 0 || n_rays > RT_MAX_RAYS) return fail(ctx, RT_EINVAL, "%s takes 1 .. %u rays", call, RT_MAX_RAYS);
    if (sets && (set_size == 0 || set_size > RT_RAY_SET_MAX)) return fail(ctx, RT_EINVAL, "a ray set holds 1 .. %u records, not %u", RT_RAY_SET_MAX, set_size);
    const size_t records = sets ? n_rays * set_size : n_rays;   // (<= 2^28 * 2^12: no overflow)
    if (records > ((size_t)1 << 31)) return fail(ctx, RT_EINVAL, "%zu rays x %u records exceed 2^31 records", n_rays, set_size);
    *records_out = records;
    return RT_OK;
}

// The argument rules of a ray call (after check_ready): rt_render_rays (sets false), rt_render_ray_sets (set_size 1 ..
// RT_RAY_SET_MAX) and the adaptive ray calls, which pass their whole sample range and a NULL d_accum.  RT_OK and the ray
// buffer in *rays_out, or an RT_* code recorded on the context.
int check_rays_or_sets(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t set_size, bool sets, uint32_t first_sample,
                       uint32_t n_samples, void *d_accum, const void **rays_out) {
    size_t records = 0;
    const int rc = check_ray_records(ctx, sets ? "rt_render_ray_sets" : "rt_render_rays", n_rays, set_size, sets, &records);
    if (rc != RT_OK) return rc;
    if (n_samples && (uint64_t)first_sample + n_samples - 1 > RT_MAX_SAMPLE)
        return fail(ctx, RT_EINVAL, "samples %u..+%u exceed the limit %u", first_sample, n_samples, RT_MAX_SAMPLE);
    if (!d_accum && n_rays != (size_t)ctx->width * ctx->height)
        return fail(ctx, RT_EINVAL, "%zu rays into the accumulator of a %d x %d frame", n_rays, ctx->width, ctx->height);
    if (d_accum && (uintptr_t)d_accum % sizeof(float4)) return fail(ctx, RT_EINVAL, "d_accum is not 16-byte aligned");
    *rays_out = ray_source(ctx, d_rays, records);
    return *rays_out ? RT_OK : RT_EINVAL;
}

// rt_render_rays (set_size 0) and rt_render_ray_sets (set_size 1 .. RT_RAY_SET_MAX): one set of checks, one launch loop
int render_rays_or_sets(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t set_size, bool sets, uint32_t first_sample,
                        uint32_t n_samples, void *d_accum) {
    int rc = check_ready(ctx, k_no_camera);
    if (rc) return rc;
    const void *rays = nullptr;
    if ((rc = check_rays_or_sets(ctx, d_rays, n_rays, set_size, sets, first_sample, n_samples, d_accum, &rays)) != RT_OK) return rc;
    if (n_samples == 0) return RT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    float4 *accum = d_accum ? static_cast<float4 *>(d_accum) : ctx->accum.p;
    // (a set is indexed by the absolute sample, so a later launch needs no offset into it)
    return for_each_launch(n_samples, [&](uint32_t done, uint32_t c) {
        float *m2 = d_accum ? nullptr : ctx->moments.target();
        const int r = ctx->ks->launch_rays(ctx, rays, n_rays, set_size, first_sample + done, c, group_log2_for(c), accum, nullptr, m2);
        if (r == RT_OK && !d_accum) ctx->accum_count += c;
        return r;
    });
}
}  // namespace
}  // extern "C++"

int rt_render_rays(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t first_sample, uint32_t n_samples, void *d_accum) {
    return render_rays_or_sets(ctx, d_rays, n_rays, 0u, false, first_sample, n_samples, d_accum);
}

int rt_render_ray_sets(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t set_size, uint32_t first_sample,
                       uint32_t n_samples, void *d_accum) {
    return render_rays_or_sets(ctx, d_rays, n_rays, set_size, true, first_sample, n_samples, d_accum);
}

int rt_render_again_cameras(rt_context *ctx, const float *cameras, uint32_t n_cameras) {
    if (!ctx) return RT_EINVAL;
    if (!cameras) return fail(ctx, RT_EINVAL, "camera table is NULL");
    if (n_cameras == 0u || n_cameras > RT_AGAIN_CAMERAS_MAX) return fail(ctx, RT_EINVAL, "a camera table holds 1 .. %u blocks", RT_AGAIN_CAMERAS_MAX);
    int rc = check_ready(ctx, cameras);
    if (rc) return rc;
    if (ctx->sample_counter >= RT_MAX_SAMPLE) return fail(ctx, RT_EINVAL, "sample counter limit %u reached", RT_MAX_SAMPLE);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // rt_render_again's look-ahead rule over the table: sample s looks through block s mod n_cameras, so while the calls
    // repeat one table the next samples' blocks are known, and one camera launch computes the images after them.
    rt_context::Lookahead &la = ctx->lookahead;
    const uint32_t s = ctx->sample_counter + 1u;
    const size_t words = (size_t)n_cameras * 12u;
    const bool same = la.have_last_table && la.last_table.size() == words && memcmp(la.last_table.data(), cameras, words * sizeof(uint32_t)) == 0;
    lookahead_validate(ctx);
    if (la.pending && (!la.key_is_table || !same)) lookahead_drop(ctx);
    bool timed = false;   // the call has its entry in the event history
    if (!la.pending && same) {
        const uint32_t kp = lookahead_batch_any(ctx, true);
        if (kp) {
            if ((rc = ensure_cameras(ctx)) != RT_OK) return rc;
            std::vector<float> blocks((size_t)kp * 12u);   // the batch's blocks: (s + j) mod n_cameras
            for (uint32_t j = 0; j < kp; j++) memcpy(&blocks[12u * j], cameras + 12u * (size_t)((s + j) % n_cameras), 12u * sizeof(float));
            // the start image: frame 0 of the ring (FrameParams::cams holds la_image's bytes)
            HIP_TRY(ctx, hipMemcpyAsync(la.ring.p, ctx->image.p, (size_t)ctx->width * ctx->height * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
            CameraTable tb;
            if ((rc = camera_table_send(ctx, blocks.data(), kp, &tb)) != RT_OK) return rc;
            rc = ctx->ks->launch_cameras(ctx, tb.d, tb.h, s, kp, group_log2_for(kp), nullptr, nullptr, nullptr, la.ring.p);
            const int rd = camera_table_read(ctx, tb);
            if (rd != RT_OK) return rd;
            if (rc != RT_OK) return rc;
            timed = true;
            lookahead_begin(ctx, kp, true);
        }
    }
    if (!same) {
        la.last_table.resize(words);
        memcpy(la.last_table.data(), cameras, words * sizeof(uint32_t));
        la.have_last_table = true;
    }
    la.have_last_cam = false;   // (a plain rt_render_again after this call repeats no plain call)
    if (la.pending) return lookahead_hand_out(ctx, timed);
    ctx->image_epoch++;
    la.direct++;
    ctx->sample_counter++;
    if ((rc = ctx->ks->launch_render(ctx, MODE_RETRACE, cameras + 12u * (size_t)(s % n_cameras), ctx->sample_counter, 1, 0, ctx->accum.p, nullptr, nullptr)) != RT_OK) return rc;
    SYNC_TRY(ctx);
    return RT_OK;
}

static int resolve_into(rt_context *ctx, int linear_only) {
    uint32_t n = (uint32_t)ctx->width * ctx->height;
    CLEAR_TRY(ctx);
    hipLaunchKernelGGL(pt_resolve, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->accum.p, ctx->image.p, n,
                       linear_only);
    HIP_TRY(ctx, hipGetLastError());
    return RT_OK;
}

int rt_resolve(rt_context *ctx) {
    if (!ctx) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->image_epoch++;
    return resolve_into(ctx, 0);
}

// ---- adaptive sampling ----------------------------------------------------------------------------------------------

extern "C++" {
namespace {

int ensure_adaptive(rt_context *ctx, size_t blocks) {
    rt_context::Adaptive &a = ctx->adaptive;
    if (a.scratch.p && blocks <= a.block_capacity) return RT_OK;
    a = {};
    const size_t px = (size_t)ctx->width * ctx->height;
    hipError_t e = a.scratch.alloc(px);
    if (e == hipSuccess) e = a.block_active.alloc(blocks);
    if (e == hipSuccess) e = a.block_err.alloc(blocks);
    if (e == hipSuccess) e = a.stats.alloc(PT_MERGE_REPLICAS * PT_MERGE_STRIDE);
    if (e != hipSuccess) {
        a = {};
        return fail(ctx, RT_EHIP, "adaptive buffers: %s", hipGetErrorString(e));
    }
    a.block_capacity = blocks;
    return RT_OK;
}

int log2_pow2(uint32_t v) {
    int l = 0;
    while ((1u << l) < v && l < 31) l++;
    return (1u << l) == v ? l : -1;
}

}  // namespace
}  // extern "C++"

extern "C++" {
namespace {

// The two stopping rules: Dammertz' half-buffer estimate (rt_render_adaptive, rt_render_adaptive_cameras) and the standard
// error of each pixel's mean, measured by the sample moments (rt_render_adaptive_variance, ..._variance_cameras)
enum AdaptiveRule { RULE_DAMMERTZ, RULE_VARIANCE };

// The parameter rules of the adaptive calls (after check_ready): RT_OK, or an RT_* code recorded on the context.
int check_adaptive(rt_context *ctx, AdaptiveRule rule, const rt_adaptive_params *p, const rt_adaptive_stats *out, int *bwl, int *bhl) {
    if (!p || !out) return fail(ctx, RT_EINVAL, "adaptive parameters / stats are NULL");
    if (ctx->world > 1) return fail(ctx, RT_EINVAL, "adaptive rendering of a sharded context (rank %d of %d)", ctx->rank, ctx->world);
    if (rule == RULE_VARIANCE && !ctx->moments.on)
        return fail(ctx, RT_ESTATE, "the variance-driven stopping rule reads the sample moments: set RT_OPT_MOMENTS to 1 first");
    if (p->batch < 1 || p->batch > RT_SPP_PER_LAUNCH)
        return fail(ctx, RT_EINVAL, "batch %u outside 1..%u", p->batch, RT_SPP_PER_LAUNCH);
    if (rule == RULE_VARIANCE) {   // (no half buffer, so one round can decide; a standard error needs two samples)
        if (p->min_spp < std::max(p->batch, 2u) || p->min_spp % p->batch)
            return fail(ctx, RT_EINVAL, "min_spp %u must be a multiple of batch %u, at least it and at least 2", p->min_spp, p->batch);
    } else if (p->min_spp < 2 * p->batch || p->min_spp % p->batch)
        return fail(ctx, RT_EINVAL, "min_spp %u must be a multiple of batch %u and at least twice it", p->min_spp, p->batch);
    if (p->max_spp < p->min_spp || p->max_spp > RT_MAX_SAMPLE + 1u)
        return fail(ctx, RT_EINVAL, "max_spp %u outside min_spp %u .. %u", p->max_spp, p->min_spp, RT_MAX_SAMPLE + 1u);
    if (!(p->threshold >= 0.0f) || !std::isfinite(p->threshold))
        return fail(ctx, RT_EINVAL, "threshold must be finite and >= 0");
    *bwl = log2_pow2(p->block_w), *bhl = log2_pow2(p->block_h);
    if (p->block_w < 1 || p->block_h < 1 || p->block_w > 256 || p->block_h > 256 || *bwl < 0 || *bhl < 0)
        return fail(ctx, RT_EINVAL, "block %ux%u: sides must be powers of two in 1..256", p->block_w, p->block_h);
    return RT_OK;
}

// The round loop of the adaptive calls, the parameters checked (bwl, bhl: check_adaptive's): buffers, clear, rounds —
// launch, the rule's merge kernel, the stats read back, the stop test — and the resolve.  `launch_round(first, c, scratch,
// mask, m2_scratch)` adds samples first .. first+c-1 of every pixel of an active block to `scratch` (and their moments to
// m2_scratch, NULL without RT_OPT_MOMENTS): the one thing in which the two calls of a rule differ.  The rules differ in
// the merge kernel and in the buffer beside the accumulator: `half` (Dammertz) or `pixel_err` (variance; the moments are on).
template <class LaunchRound>
int adaptive_rounds(rt_context *ctx, AdaptiveRule rule, const rt_adaptive_params *p, int bwl, int bhl, rt_adaptive_stats *out,
                    LaunchRound launch_round) {
    int rc;
    const uint32_t bx = ((uint32_t)ctx->width + p->block_w - 1) >> bwl, by = ((uint32_t)ctx->height + p->block_h - 1) >> bhl;
    const uint32_t blocks = bx * by;
    if ((rc = ensure_adaptive(ctx, blocks)) != RT_OK) return rc;
    rt_context::Adaptive &a = ctx->adaptive;
    a.blocks = 0;
    a.variance = false;
    const size_t px = (size_t)ctx->width * ctx->height;
    if (rule == RULE_DAMMERTZ && !a.half.p) HIP_TRY(ctx, a.half.alloc(px));
    if (rule == RULE_VARIANCE && !a.pixel_err.p) HIP_TRY(ctx, a.pixel_err.alloc(px));
    // sample moments (RT_OPT_MOMENTS): the rounds leave theirs in a scratch of its own, made once the option is on
    const bool mom = ctx->moments.on;
    if (mom && !a.m2_scratch.p) HIP_TRY(ctx, a.m2_scratch.alloc(px));
    ctx->image_epoch++;   // (the call ends in a resolve)
    const size_t bytes = px * sizeof(float4);
    ctx->clear_pending = false;   // (a pending rt_clear is this memset)
    HIP_TRY(ctx, hipMemsetAsync(ctx->accum.p, 0, bytes, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(a.scratch.p, 0, bytes, ctx->stream));
    if (rule == RULE_DAMMERTZ) HIP_TRY(ctx, hipMemsetAsync(a.half.p, 0, bytes, ctx->stream));
    else HIP_TRY(ctx, hipMemsetAsync(a.pixel_err.p, 0, bytes / 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(a.block_active.p, 0xFF, blocks * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(a.block_err.p, 0, blocks * sizeof(float), ctx->stream));
    ctx->accum_count = 0;
    if ((rc = moments_begin(ctx)) != RT_OK) return rc;
    if (mom) HIP_TRY(ctx, hipMemsetAsync(a.m2_scratch.p, 0, bytes / 4, ctx->stream));
    float *const m2 = mom ? ctx->moments.m2.p : nullptr, *const m2_scratch = mom ? a.m2_scratch.p : nullptr;
    const BlockMask mask{a.block_active.p, (uint32_t)bwl, (uint32_t)bhl, bx};
    MergeParams mp;
    mp.w = (uint32_t)ctx->width;
    mp.h = (uint32_t)ctx->height;
    mp.bw_log2 = (uint32_t)bwl;
    mp.bh_log2 = (uint32_t)bhl;
    mp.blocks_x = bx;
    mp.blocks = blocks;
    mp.min_spp = p->min_spp;
    mp.max_spp = p->max_spp;
    mp.threshold = p->threshold;
    uint32_t rounds = 0;
    uint64_t at_max = 0, pixel_samples = 0;
    std::vector<unsigned long long> st(PT_MERGE_REPLICAS * PT_MERGE_STRIDE);
    const size_t st_bytes = st.size() * sizeof(unsigned long long);
    for (uint32_t k = 0;; k++) {
        const uint32_t first = k * p->batch;
        const uint32_t c = std::min(p->batch, p->max_spp - first);
        if ((rc = launch_round(first, c, a.scratch.p, &mask, m2_scratch)) != RT_OK) return rc;
        mp.round = k;
        mp.count = first + c;
        HIP_TRY(ctx, hipMemsetAsync(a.stats.p, 0, st_bytes, ctx->stream));
        const dim3 grid((blocks + PT_MERGE_WAVES - 1) / PT_MERGE_WAVES), wg(64 * PT_MERGE_WAVES);
        if (rule == RULE_DAMMERTZ)
            hipLaunchKernelGGL(pt_adaptive_merge, grid, wg, 0, ctx->stream, mp, ctx->accum.p, a.half.p, a.scratch.p, a.block_active.p,
                               a.block_err.p, a.stats.p, m2, m2_scratch);
        else
            hipLaunchKernelGGL(pt_adaptive_merge_variance, grid, wg, 0, ctx->stream, mp, ctx->accum.p, a.scratch.p, a.block_active.p,
                               a.block_err.p, a.stats.p, m2, m2_scratch, a.pixel_err.p);
        HIP_TRY(ctx, hipGetLastError());
        rounds++;
        ctx->accum_count = first + c;
        HIP_TRY(ctx, hipMemcpyAsync(st.data(), a.stats.p, st_bytes, hipMemcpyDeviceToHost, ctx->stream));
        SYNC_TRY(ctx);
        uint64_t still = 0;
        for (uint32_t r = 0; r < PT_MERGE_REPLICAS; r++) {
            still += st[r * PT_MERGE_STRIDE];
            at_max += st[r * PT_MERGE_STRIDE + 1];
            pixel_samples += st[r * PT_MERGE_STRIDE + 2];
        }
        if (still == 0) break;
    }
    if ((rc = resolve_into(ctx, 0)) != RT_OK) return rc;
    SYNC_TRY(ctx);
    a.blocks = blocks;
    a.variance = rule == RULE_VARIANCE;
    out->rounds = rounds;
    out->pixel_samples = pixel_samples;
    out->blocks = blocks;
    out->blocks_at_max = (uint32_t)at_max;
    return RT_OK;
}

}  // namespace
}  // extern "C++"

extern "C++" {
namespace {

// rt_render_adaptive / rt_render_adaptive_variance: every sample through one camera
int render_adaptive(rt_context *ctx, AdaptiveRule rule, const float camera[12], const rt_adaptive_params *p, rt_adaptive_stats *out) {
    int rc = check_ready(ctx, camera), bwl = 0, bhl = 0;
    if (rc) return rc;
    if ((rc = check_adaptive(ctx, rule, p, out, &bwl, &bhl)) != RT_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return adaptive_rounds(ctx, rule, p, bwl, bhl, out, [&](uint32_t first, uint32_t c, float4 *scratch, const BlockMask *mask, float *m2_scratch) {
        return launch_camera_samples(ctx, camera, first, c, scratch, mask, m2_scratch);
    });
}

// rt_render_adaptive_cameras / rt_render_adaptive_variance_cameras: sample j through block j
int render_adaptive_cameras(rt_context *ctx, AdaptiveRule rule, const float *cameras, uint32_t n_cameras, const rt_adaptive_params *p,
                            rt_adaptive_stats *out) {
    int rc = check_ready(ctx, cameras), bwl = 0, bhl = 0;
    if (rc) return rc;
    if ((rc = check_adaptive(ctx, rule, p, out, &bwl, &bhl)) != RT_OK) return rc;
    if (n_cameras != p->max_spp)
        return fail(ctx, RT_EINVAL, "%u camera blocks for max_spp %u: block j is the camera of sample j", n_cameras, p->max_spp);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_cameras(ctx)) != RT_OK) return rc;
    // (a round ends in a stream synchronisation, so the ring's wait returns at once: the tables go the way of
    // rt_render_spp_cameras' all the same)
    return adaptive_rounds(ctx, rule, p, bwl, bhl, out, [&](uint32_t first, uint32_t c, float4 *scratch, const BlockMask *mask, float *m2_scratch) {
        CameraTable tb;
        int r = camera_table_send(ctx, cameras + (size_t)first * 12u, c, &tb);
        if (r != RT_OK) return r;
        r = ctx->ks->launch_cameras(ctx, tb.d, tb.h, first, c, group_log2_for(c), scratch, mask, m2_scratch, nullptr);
        const int rd = camera_table_read(ctx, tb);
        return rd != RT_OK ? rd : r;
    });
}

// rt_render_adaptive_rays / rt_render_adaptive_variance_rays: sample s of pixel i along ray i (set_size 0), or along record
// s mod set_size of ray i's set — the rounds run rt_render_rays' / rt_render_ray_sets' launches under the block mask
int render_adaptive_rays(rt_context *ctx, AdaptiveRule rule, const void *d_rays, size_t n_rays, uint32_t set_size,
                         const rt_adaptive_params *p, rt_adaptive_stats *out) {
    int rc = check_ready(ctx, k_no_camera), bwl = 0, bhl = 0;
    if (rc) return rc;
    if ((rc = check_adaptive(ctx, rule, p, out, &bwl, &bhl)) != RT_OK) return rc;
    // (the call's whole sample range 0 .. max_spp-1 into the context's accumulator: n_rays == W*H)
    const bool sets = set_size != 0u;
    const void *rays = nullptr;
    if ((rc = check_rays_or_sets(ctx, d_rays, n_rays, set_size, sets, 0u, p->max_spp, nullptr, &rays)) != RT_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return adaptive_rounds(ctx, rule, p, bwl, bhl, out, [&](uint32_t first, uint32_t c, float4 *scratch, const BlockMask *mask, float *m2_scratch) {
        return ctx->ks->launch_rays(ctx, rays, n_rays, set_size, first, c, group_log2_for(c), scratch, mask, m2_scratch);
    });
}

}  // namespace
}  // extern "C++"

int rt_render_adaptive(rt_context *ctx, const float camera[12], const rt_adaptive_params *p, rt_adaptive_stats *out) {
    return render_adaptive(ctx, RULE_DAMMERTZ, camera, p, out);
}

int rt_render_adaptive_cameras(rt_context *ctx, const float *cameras, uint32_t n_cameras, const rt_adaptive_params *p,
                               rt_adaptive_stats *out) {
    return render_adaptive_cameras(ctx, RULE_DAMMERTZ, cameras, n_cameras, p, out);
}

int rt_render_adaptive_variance(rt_context *ctx, const float camera[12], const rt_adaptive_params *p, rt_adaptive_stats *out) {
    return render_adaptive(ctx, RULE_VARIANCE, camera, p, out);
}

int rt_render_adaptive_variance_cameras(rt_context *ctx, const float *cameras, uint32_t n_cameras, const rt_adaptive_params *p,
                                        rt_adaptive_stats *out) {
    return render_adaptive_cameras(ctx, RULE_VARIANCE, cameras, n_cameras, p, out);
}

int rt_render_adaptive_rays(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t set_size, const rt_adaptive_params *p,
                            rt_adaptive_stats *out) {
    return render_adaptive_rays(ctx, RULE_DAMMERTZ, d_rays, n_rays, set_size, p, out);
}

int rt_render_adaptive_variance_rays(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t set_size, const rt_adaptive_params *p,
                                     rt_adaptive_stats *out) {
    return render_adaptive_rays(ctx, RULE_VARIANCE, d_rays, n_rays, set_size, p, out);
}

int rt_read_sample_counts(rt_context *ctx, uint32_t *counts, size_t bytes) {
    if (!ctx) return RT_EINVAL;
    const size_t n = (size_t)ctx->width * ctx->height;
    if (!counts || bytes != n * sizeof(uint32_t)) return fail(ctx, RT_EINVAL, "count buffer must be %zu bytes", n * sizeof(uint32_t));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<float4> h(n);
    CLEAR_TRY(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), ctx->accum.p, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    SYNC_TRY(ctx);
    for (size_t i = 0; i < n; i++) counts[i] = (uint32_t)h[i].w;
    return RT_OK;
}

int rt_read_block_error(rt_context *ctx, float *err, size_t bytes) {
    if (!ctx) return RT_EINVAL;
    const rt_context::Adaptive &a = ctx->adaptive;
    if (!a.blocks) return fail(ctx, RT_ESTATE, "no rt_render_adaptive call since the frame was (re)allocated");
    return read_back(ctx, err, bytes, a.block_err.p, a.blocks * sizeof(float), "block error");
}

int rt_read_pixel_error(rt_context *ctx, float *err, size_t bytes) {
    if (!ctx) return RT_EINVAL;
    const rt_context::Adaptive &a = ctx->adaptive;
    const size_t need = (size_t)ctx->width * ctx->height * sizeof(float);
    if (!err || bytes != need) return fail(ctx, RT_EINVAL, "pixel error buffer must be %zu bytes", need);
    if (!a.blocks || !a.variance)
        return fail(ctx, RT_ESTATE, "the last adaptive call on this frame was not rt_render_adaptive_variance(_cameras)");
    return read_back(ctx, err, bytes, a.pixel_err.p, need, "pixel error");
}

int rt_device_pixel_error(rt_context *ctx, void **d_err) {
    if (!ctx || !d_err) return RT_EINVAL;
    const rt_context::Adaptive &a = ctx->adaptive;
    if (!a.blocks || !a.variance)
        return fail(ctx, RT_ESTATE, "the last adaptive call on this frame was not rt_render_adaptive_variance(_cameras)");
    *d_err = a.pixel_err.p;
    return RT_OK;
}

// ---- feature buffers (the denoisers that read them: rt_denoise.hip) ---------------------------------------------------

}  // extern "C"

namespace {
// the follow bits and the chain length of every call that takes rt_feature_chain_params
int check_chain_params(rt_context *ctx, const rt_feature_chain_params *p) {
    if (p->follow & ~(RT_FOLLOW_REFLECTIVE | RT_FOLLOW_REFRACTIVE | RT_FOLLOW_DIELECTRIC))
        return fail(ctx, RT_EINVAL, "unknown follow bits 0x%x", p->follow);
    if (p->max_chain > RT_FEATURE_CHAIN_MAX) return fail(ctx, RT_EINVAL, "max_chain %u above %u", p->max_chain, RT_FEATURE_CHAIN_MAX);
    return RT_OK;
}

// What rt_render_features and rt_render_features_chain share — the state rules, the records' allocation, the frame and
// scene blocks, `ready` — round the one launch in which they differ (`params_ok`: the caller's own argument checks,
// made after check_ready and before the shard check, 0 or an RT_* code already recorded on the context).
template <class Launch>
int render_features_with(rt_context *ctx, const float camera[12], int params_ok, Launch launch) {
    if (params_ok) return params_ok;
    if (ctx->world > 1) return fail(ctx, RT_EINVAL, "features of a sharded context (rank %d of %d)", ctx->rank, ctx->world);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rt_context::Features &f = ctx->features;
    if (!f.records.p) HIP_TRY(ctx, f.records.alloc((size_t)ctx->width * ctx->height));
    const FrameParams fp = frame_params(ctx, camera, 0, 1, 0);
    const DeviceScene sc = device_scene(ctx);
    const int rc = launch(fp, sc, f.records.p);
    if (rc != RT_OK) return rc;
    f.ready = true;
    f.coverage_ready = false;   // (rt_render_features_cameras sets it: the coverage describes ITS records only)
    return RT_OK;
}
}  // namespace

extern "C" {

int rt_render_features(rt_context *ctx, const float camera[12]) {
    const int rc = check_ready(ctx, camera);
    if (rc) return rc;
    return render_features_with(ctx, camera, RT_OK, [&](const FrameParams &fp, const DeviceScene &sc, rt_feature *out) {
        return ctx->ks->launch_features(ctx, fp, sc, out);
    });
}

int rt_render_features_chain(rt_context *ctx, const float camera[12], const rt_feature_chain_params *p) {
    const int rc = check_ready(ctx, camera);
    if (rc) return rc;
    const int ok = p ? check_chain_params(ctx, p) : fail(ctx, RT_EINVAL, "feature chain parameters are NULL");
    return render_features_with(ctx, camera, ok, [&](const FrameParams &fp, const DeviceScene &sc, rt_feature *out) {
        return ctx->ks->launch_features_chain(ctx, fp, sc, p->follow, p->max_chain, out);
    });
}

int rt_render_features_rays(rt_context *ctx, const void *d_rays, size_t n_rays, const rt_feature_chain_params *p) {
    const int rc = check_ready(ctx, k_no_camera);
    if (rc) return rc;
    const rt_feature_chain_params first_hits = {0u, 0u};
    if (!p) p = &first_hits;
    int ok = check_chain_params(ctx, p);
    const void *rays = nullptr;
    if (ok == RT_OK && n_rays != (size_t)ctx->width * ctx->height)
        ok = fail(ctx, RT_EINVAL, "%zu rays for the feature records of a %d x %d frame", n_rays, ctx->width, ctx->height);
    if (ok == RT_OK && !(rays = ray_source(ctx, d_rays, n_rays))) ok = RT_EINVAL;
    return render_features_with(ctx, k_no_camera, ok, [&](const FrameParams &, const DeviceScene &sc, rt_feature *out) {
        return ctx->ks->launch_features_rays(ctx, sc, rays, (uint32_t)n_rays, p->follow, p->max_chain, out);
    });
}

// ---- ray queries: nearest hit and occlusion for any batch; nothing of the context's state moves ---------------------------
int rt_intersect_rays(rt_context *ctx, const void *d_rays, size_t n_rays, const rt_feature_chain_params *p, void *d_out) {
    const int rc = check_ready(ctx, k_no_camera);
    if (rc) return rc;
    const rt_feature_chain_params first_hits = {0u, 0u};
    if (!p) p = &first_hits;
    size_t records = 0;
    const int bad = check_ray_records(ctx, "rt_intersect_rays", n_rays, 0u, false, &records);
    if (bad != RT_OK) return bad;
    if (!d_out || (uintptr_t)d_out % 16u) return fail(ctx, RT_EINVAL, "d_out must be a 16-byte aligned device buffer of rt_feature records");
    const int chain = check_chain_params(ctx, p);
    if (chain != RT_OK) return chain;
    const void *rays = ray_source(ctx, d_rays, n_rays);
    if (!rays) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ctx->ks->launch_features_rays(ctx, device_scene(ctx), rays, (uint32_t)n_rays, p->follow, p->max_chain,
                                         static_cast<rt_feature *>(d_out));
}

int rt_occluded_rays(rt_context *ctx, const void *d_rays, size_t n_rays, uint32_t set_size, const float *d_tmax, float t_max,
                     void *d_out) {
    const int rc = check_ready(ctx, k_no_camera);
    if (rc) return rc;
    size_t records = 0;
    const int bad = check_ray_records(ctx, "rt_occluded_rays", n_rays, set_size, true, &records);
    if (bad != RT_OK) return bad;
    if (!d_out || (uintptr_t)d_out % sizeof(uint32_t)) return fail(ctx, RT_EINVAL, "d_out must be a 4-byte aligned device buffer of n_rays uint32");
    if ((uintptr_t)d_tmax % sizeof(float)) return fail(ctx, RT_EINVAL, "d_tmax is not 4-byte aligned");
    const void *rays = ray_source(ctx, d_rays, records);
    if (!rays) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ctx->ks->launch_occluded(ctx, device_scene(ctx), rays, n_rays, set_size, d_tmax, t_max, static_cast<uint32_t *>(d_out));
}

// rt_occluded_hemispheres: the rays of n feature records made in registers (pt_occluded_hemi); counts, rays or both
int rt_occluded_hemispheres(rt_context *ctx, const void *d_features, size_t n, const rt_hemisphere_params *p, void *d_counts,
                            void *d_rays_out) {
    const int rc = check_ready(ctx, k_no_camera);
    if (rc) return rc;
    if (!p) return fail(ctx, RT_EINVAL, "rt_occluded_hemispheres: the parameters are NULL");
    size_t records = 0;
    const int bad = check_ray_records(ctx, "rt_occluded_hemispheres", n, p->k, true, &records);
    if (bad != RT_OK) return bad;
    if (!d_counts && !d_rays_out) return fail(ctx, RT_EINVAL, "rt_occluded_hemispheres needs d_counts, d_rays_out or both");
    if ((uintptr_t)d_counts % sizeof(uint32_t)) return fail(ctx, RT_EINVAL, "d_counts is not 4-byte aligned");
    if ((uintptr_t)d_rays_out % alignof(rt_ray)) return fail(ctx, RT_EINVAL, "d_rays_out is not 16-byte aligned");
    if ((uintptr_t)d_features % 16u) return fail(ctx, RT_EINVAL, "d_features is not 16-byte aligned");
    if (p->flags & ~RT_HEMI_FACE_FORWARD) return fail(ctx, RT_EINVAL, "unknown hemisphere flags 0x%x", p->flags);
    if (!std::isfinite(p->offset)) return fail(ctx, RT_EINVAL, "the hemisphere offset must be finite");
    if (!d_features) {
        if (n != (size_t)ctx->width * ctx->height)
            return fail(ctx, RT_EINVAL, "the context's feature records are %d x %d, not %zu", ctx->width, ctx->height, n);
        if (!ctx->features.ready) return fail(ctx, RT_ESTATE, "no rt_render_features call since the frame was (re)allocated");
        d_features = ctx->features.records.p;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ctx->ks->launch_occluded_hemi(ctx, device_scene(ctx), static_cast<const rt_feature *>(d_features), n, *p,
                                         static_cast<uint32_t *>(d_counts), d_rays_out);
}

// rt_render_hemispheres: rt_render_ray_sets over the rays the spawn form would write, made in registers instead
// (pt_samples_q_hemi / pt_render_hemi); every check stands before the first launch
int rt_render_hemispheres(rt_context *ctx, const void *d_features, size_t n, const rt_hemisphere_params *p, uint32_t first_sample,
                          uint32_t n_samples, void *d_accum) {
    const int rc = check_ready(ctx, k_no_camera);
    if (rc) return rc;
    if (!p) return fail(ctx, RT_EINVAL, "rt_render_hemispheres: the parameters are NULL");
    size_t records = 0;
    const int bad = check_ray_records(ctx, "rt_render_hemispheres", n, p->k, true, &records);
    if (bad != RT_OK) return bad;
    if ((uintptr_t)d_features % 16u) return fail(ctx, RT_EINVAL, "d_features is not 16-byte aligned");
    if ((uintptr_t)d_accum % sizeof(float4)) return fail(ctx, RT_EINVAL, "d_accum is not 16-byte aligned");
    if (p->flags & ~RT_HEMI_FACE_FORWARD) return fail(ctx, RT_EINVAL, "unknown hemisphere flags 0x%x", p->flags);
    if (!std::isfinite(p->offset)) return fail(ctx, RT_EINVAL, "the hemisphere offset must be finite");
    if (n_samples == 0 || (uint64_t)first_sample + n_samples - 1 > RT_MAX_SAMPLE)
        return fail(ctx, RT_EINVAL, "samples %u..+%u: 1 or more, up to the limit %u", first_sample, n_samples, RT_MAX_SAMPLE);
    const size_t frame = (size_t)ctx->width * ctx->height;
    if (!d_accum && n != frame) return fail(ctx, RT_EINVAL, "%zu records into the accumulator of a %d x %d frame", n, ctx->width, ctx->height);
    if (!d_features) {
        if (n != frame) return fail(ctx, RT_EINVAL, "the context's feature records are %d x %d, not %zu", ctx->width, ctx->height, n);
        if (!ctx->features.ready) return fail(ctx, RT_ESTATE, "no rt_render_features call since the frame was (re)allocated");
        d_features = ctx->features.records.p;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    float4 *accum = d_accum ? static_cast<float4 *>(d_accum) : ctx->accum.p;
    // (a hemisphere ray is chosen by the absolute sample, so a later launch needs no offset)
    return for_each_launch(n_samples, [&](uint32_t done, uint32_t c) {
        float *m2 = d_accum ? nullptr : ctx->moments.target();
        const int r = ctx->ks->launch_hemispheres(ctx, static_cast<const rt_feature *>(d_features), n, *p, first_sample + done, c,
                                                  group_log2_for(c), accum, m2);
        if (r == RT_OK && !d_accum) ctx->accum_count += c;
        return r;
    });
}

// ---- device memory for a host without a HIP runtime of its own (the buffers the ray queries write into) ----------------------
int rt_device_alloc(rt_context *ctx, size_t bytes, void **d_out) {
    if (!ctx) return RT_EINVAL;
    if (!d_out || bytes == 0) return fail(ctx, RT_EINVAL, "rt_device_alloc takes a size above 0 and a place for the pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *d_out = nullptr;
    if (hipMalloc(d_out, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *d_out = nullptr;
        return fail(ctx, RT_EHIP, "no device memory for %zu bytes", bytes);
    }
    return RT_OK;
}

int rt_device_free(rt_context *ctx, void *d_ptr) {
    if (!ctx) return RT_EINVAL;
    if (!d_ptr) return RT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipFree(d_ptr));   // (waits for the work that uses it)
    return RT_OK;
}

int rt_device_copy(rt_context *ctx, void *dst, const void *src, size_t bytes, int to_device) {
    if (!ctx) return RT_EINVAL;
    if (!dst || !src) return fail(ctx, RT_EINVAL, "rt_device_copy: a NULL pointer");
    if (bytes == 0) return RT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, ctx->stream));
    SYNC_TRY(ctx);
    return RT_OK;
}

int rt_render_features_cameras(rt_context *ctx, const float *cameras, uint32_t n_cameras, const rt_feature_chain_params *p) {
    const int rc = check_ready(ctx, cameras);
    if (rc) return rc;
    const rt_feature_chain_params first_hits = {0u, 0u};
    if (!p) p = &first_hits;
    const int ok = n_cameras < 1u || n_cameras > RT_FEATURE_CAMERAS_MAX
                       ? fail(ctx, RT_EINVAL, "%u camera blocks outside 1..%u", n_cameras, RT_FEATURE_CAMERAS_MAX)
                       : check_chain_params(ctx, p);
    // (cameras: the first block fills FrameParams::cam, which pt_features_cameras does not read)
    const int done = render_features_with(ctx, cameras, ok, [&](const FrameParams &fp, const DeviceScene &sc, rt_feature *out) {
        rt_context::Features &f = ctx->features;
        const size_t pixels = (size_t)ctx->width * ctx->height;
        if (!f.coverage.p) HIP_TRY(ctx, f.coverage.alloc(pixels));
        int r = ensure_cameras(ctx);
        if (r != RT_OK) return r;
        // the blocks go through table k of the ring, as a launch of rt_render_spp_cameras sends its own
        CameraTable tb;
        if ((r = camera_table_send(ctx, cameras, n_cameras, &tb)) != RT_OK) return r;
        r = ctx->ks->launch_features_cameras(ctx, fp, sc, tb.d, n_cameras, p->follow, p->max_chain, out,
                                             reinterpret_cast<uint2 *>(f.coverage.p));
        if (r == RT_OK) {
            hipLaunchKernelGGL(pt_features_cameras_finish, dim3((uint32_t)((pixels + 255u) / 256u)), dim3(256), 0, ctx->stream,
                               reinterpret_cast<float4 *>(out), f.coverage.p, (uint32_t)pixels, n_cameras);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) r = fail(ctx, RT_EHIP, "pt_features_cameras_finish: %s", hipGetErrorString(e));
        }
        const int rd = camera_table_read(ctx, tb);
        return rd != RT_OK ? rd : r;
    });
    if (done == RT_OK) ctx->features.coverage_ready = true;
    return done;
}

int rt_read_feature_coverage(rt_context *ctx, float *out, size_t bytes) {
    if (!ctx) return RT_EINVAL;
    const rt_context::Features &f = ctx->features;
    return read_back(ctx, out, bytes, f.coverage.p, (size_t)ctx->width * ctx->height * sizeof(float2), "feature coverage",
                     f.coverage_ready, "rt_render_features_cameras");
}

int rt_device_feature_coverage(rt_context *ctx, void **d_out) {
    if (!ctx || !d_out) return RT_EINVAL;
    if (!ctx->features.coverage_ready)
        return fail(ctx, RT_ESTATE, "no rt_render_features_cameras call since the feature records were last written");
    *d_out = ctx->features.coverage.p;
    return RT_OK;
}

int rt_debug_plan_feature_cameras(int width, int height, uint32_t n_cameras, uint32_t out[3]) {
    if (!out || width < 1 || width > RT_MAX_DIM || height < 1 || height > RT_MAX_DIM || n_cameras < 1u || n_cameras > RT_FEATURE_CAMERAS_MAX)
        return fail(nullptr, RT_EINVAL, "rt_debug_plan_feature_cameras: a size outside 1..%d, a count outside 1..%u or a NULL pointer",
                    RT_MAX_DIM, RT_FEATURE_CAMERAS_MAX);
    const pt::FeatureCamerasPlan p = pt::kernel_set_a2()->plan_feature_cameras((uint32_t)width * (uint32_t)height, n_cameras);   // (host code: the same in every policy)
    out[0] = p.glog2;
    out[1] = p.workgroups;
    out[2] = p.block_size;
    return RT_OK;
}

int rt_feature_chain_signature(const uint32_t *objects, uint32_t n, uint32_t *sig_out) {
    if (!sig_out || (n && !objects)) return fail(nullptr, RT_EINVAL, "rt_feature_chain_signature: a pointer is NULL");
    uint32_t h = 0u;
    for (uint32_t i = 0; i < n; i++) h = chain_signature_step(h, objects[i]);
    *sig_out = h;
    return RT_OK;
}

int rt_read_features(rt_context *ctx, rt_feature *out, size_t bytes) {
    if (!ctx) return RT_EINVAL;
    const rt_context::Features &f = ctx->features;
    return read_back(ctx, out, bytes, f.records.p, (size_t)ctx->width * ctx->height * sizeof(rt_feature), "feature", f.ready,
                     "rt_render_features");
}

int rt_device_features(rt_context *ctx, void **d_features) {
    if (!ctx || !d_features) return RT_EINVAL;
    if (!ctx->features.ready) return fail(ctx, RT_ESTATE, "no rt_render_features call since the frame was (re)allocated");
    *d_features = ctx->features.records.p;
    return RT_OK;
}

int rt_read_moments(rt_context *ctx, float *m2, size_t bytes) {
    if (!ctx) return RT_EINVAL;
    const size_t need = (size_t)ctx->width * ctx->height * sizeof(float);
    if (!m2 || bytes != need) return fail(ctx, RT_EINVAL, "moment buffer must be %zu bytes", need);
    if (!ctx->moments.target()) return fail(ctx, RT_ESTATE, "the sample moments are not valid: set RT_OPT_MOMENTS to 1, then rt_clear or rt_render_adaptive");
    return read_back(ctx, m2, bytes, ctx->moments.m2.p, need, "moment");
}

int rt_device_moments(rt_context *ctx, void **d_m2) {
    if (!ctx || !d_m2) return RT_EINVAL;
    if (!ctx->moments.target()) return fail(ctx, RT_ESTATE, "the sample moments are not valid: set RT_OPT_MOMENTS to 1, then rt_clear or rt_render_adaptive");
    *d_m2 = ctx->moments.m2.p;
    return RT_OK;
}

int rt_moments_merge(uint32_t nA, const float sumA[3], float m2A, uint32_t nB, const float sumB[3], float m2B, float *m2_out) {
    if (!sumA || !sumB || !m2_out) return fail(nullptr, RT_EINVAL, "rt_moments_merge: a pointer is NULL");
    *m2_out = moments_merge((float)nA, sumA[0], sumA[1], sumA[2], m2A, (float)nB, sumB[0], sumB[1], sumB[2], m2B);
    return RT_OK;
}

int rt_sync(rt_context *ctx) {
    if (!ctx) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SYNC_TRY(ctx);
    return RT_OK;
}

int rt_trace_samples(rt_context *ctx, const float camera[12], const uint32_t *x, const uint32_t *y,
                     const uint32_t *sample, size_t n, float *out_rgb) {
    int rc = check_ready(ctx, camera);
    if (rc) return rc;
    if (n == 0) return RT_OK;
    if (!x || !y || !sample || !out_rgb || n > (1u << 28)) return fail(ctx, RT_EINVAL, "bad probe arrays");
    for (size_t i = 0; i < n; i++)
        if (x[i] >= (uint32_t)ctx->width || y[i] >= (uint32_t)ctx->height || sample[i] > RT_MAX_SAMPLE)
            return fail(ctx, RT_EINVAL, "probe %zu (%u,%u,%u) outside the frame / sample range", i, x[i], y[i], sample[i]);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf<uint32_t> d_in;
    DevBuf<float> d_out;
    HIP_TRY(ctx, d_in.alloc(3 * n));
    HIP_TRY(ctx, d_out.alloc(3 * n));
    HIP_TRY(ctx, hipMemcpyAsync(d_in.p, x, n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_in.p + n, y, n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_in.p + 2 * n, sample, n * 4, hipMemcpyHostToDevice, ctx->stream));
    const FrameParams fp = frame_params(ctx, camera, 0, 1, 0);
    if ((rc = ctx->ks->launch_probe(ctx, fp, device_scene(ctx), d_in.p, (uint32_t)n, d_out.p)) != RT_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_rgb, d_out.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    SYNC_TRY(ctx);
    return RT_OK;
}

int rt_read_image(rt_context *ctx, float *rgba, size_t bytes) {
    if (!ctx) return RT_EINVAL;
    return read_back(ctx, rgba, bytes, ctx->image.p, (size_t)ctx->width * ctx->height * sizeof(float4), "image");
}

int rt_read_linear(rt_context *ctx, float *rgba, size_t bytes) {
    if (!ctx) return RT_EINVAL;
    const size_t n = (size_t)ctx->width * ctx->height;
    if (!rgba || bytes != n * sizeof(float4)) return fail(ctx, RT_EINVAL, "image buffer must be %zu bytes", n * sizeof(float4));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf<float4> tmp;
    HIP_TRY(ctx, tmp.alloc(n));
    CLEAR_TRY(ctx);
    hipLaunchKernelGGL(pt_resolve, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->accum.p, tmp.p, (uint32_t)n, 1);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(rgba, tmp.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SYNC_TRY(ctx);
    return RT_OK;
}

int rt_device_image(rt_context *ctx, void **d_rgba) {
    if (!ctx || !d_rgba) return RT_EINVAL;
    *d_rgba = ctx->image.p;
    return RT_OK;
}

int rt_device_accum(rt_context *ctx, void **d_rgba) {
    if (!ctx || !d_rgba) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    CLEAR_TRY(ctx);   // (the caller's own work on the stream may come next)
    *d_rgba = ctx->accum.p;
    return RT_OK;
}

int rt_enable_counters(rt_context *ctx, int enable) {
    if (!ctx) return RT_EINVAL;
    ctx->count_enabled = enable != 0;
    ctx->prefix_changed();
    return RT_OK;
}

// host-only self-check of the acceleration structures: the prepared scene rt_set_scene would upload (scene_prep.hpp)
int rt_debug_check_accel(const rt_scene_desc *d, uint64_t stats[8], char *err, size_t err_len) {
    if (!d || !stats) return RT_EINVAL;
    memset(stats, 0, 8 * sizeof(uint64_t));
    PreparedScene ps;
    std::string msg;
    int rc = prepare_scene(*d, ps, msg);
    if (rc == RT_OK) rc = check_prepared(*d, ps, stats, msg);
    if (rc != RT_OK && err && err_len) snprintf(err, err_len, "%s", msg.c_str());
    return rc;
}

extern "C++" {
namespace {
// upload `bytes` of input, run `launch(d_in, d_out)` (an RT_* code), download `out_bytes`
template <class F>
int debug_roundtrip(rt_context *ctx, const void *in, size_t bytes, void *out, size_t out_bytes, F launch) {
    DevBuf<uint8_t> d_in, d_out;
    HIP_TRY(ctx, d_in.alloc(bytes ? bytes : 16));
    HIP_TRY(ctx, d_out.alloc(out_bytes ? out_bytes : 16));
    HIP_TRY(ctx, hipMemcpyAsync(d_in.p, in, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = launch(d_in.p, d_out.p)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SYNC_TRY(ctx);
    return RT_OK;
}
}  // namespace
}  // extern "C++"

int rt_debug_hit(rt_context *ctx, int kind, const float *rays, const uint32_t *prim, const uint32_t *face, size_t n,
                 float *out12) {
    if (!ctx) return RT_EINVAL;
    if (!ctx->have_scene) return fail(ctx, RT_ESTATE, "no scene: call rt_set_scene first");
    if (n == 0) return RT_OK;
    if (!rays || !out12 || kind < 0 || kind > 4 || n > (1u << 26) || (kind != 3 && !prim) || (kind == 4 && !face))
        return fail(ctx, RT_EINVAL, "bad unit-probe arguments");
    const size_t counts[5] = {ctx->spheres.n, ctx->planes.n, ctx->lenses.n, 0, ctx->meshes.n};
    std::vector<uint32_t> pf(2 * n, 0u);
    for (size_t i = 0; i < n; i++) {
        if (kind != 3) {
            if (prim[i] >= counts[kind]) return fail(ctx, RT_ERANGE, "unit probe %zu: primitive %u does not exist", i, prim[i]);
            pf[i] = prim[i];
        }
        if (kind == 4) pf[n + i] = face[i];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (kind == 4) {  // face indices against the meshes' face counts (host copy of the mesh array)
        std::vector<rt_mesh> meshes(ctx->meshes.n);
        HIP_TRY(ctx, hipMemcpy(meshes.data(), ctx->meshes.p, meshes.size() * sizeof(rt_mesh), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++)
            if (face[i] >= meshes[prim[i]].face_count) return fail(ctx, RT_ERANGE, "unit probe %zu: face %u does not exist", i, face[i]);
    }
    // rays and (prim, face) travel in one buffer: 6 floats + 2 words per record
    std::vector<uint32_t> in(8 * n);
    memcpy(in.data(), rays, 6 * n * sizeof(float));
    memcpy(in.data() + 6 * n, pf.data(), 2 * n * sizeof(uint32_t));
    DeviceScene sc = device_scene(ctx);
    return debug_roundtrip(ctx, in.data(), in.size() * 4, out12, 12 * n * sizeof(float), [&](void *d_in, void *d_out) {
        const float *d_rays = (const float *)d_in;
        const uint32_t *d_prim = (const uint32_t *)d_in + 6 * n, *d_face = d_prim + n;
        return ctx->ks->launch_debug_hit(ctx, sc, kind, d_rays, d_prim, d_face, (uint32_t)n, (float *)d_out);
    });
}

int rt_debug_material(rt_context *ctx, int routine, const float *in16, size_t n, float *out9) {
    if (!ctx) return RT_EINVAL;
    if (!ctx->have_scene) return fail(ctx, RT_ESTATE, "no scene: call rt_set_scene first");
    if (n == 0) return RT_OK;
    if (!in16 || !out9 || routine < 0 || routine > 3 || n > (1u << 26)) return fail(ctx, RT_EINVAL, "bad unit-probe arguments");
    for (size_t i = 0; i < n; i++) {
        uint32_t w[4];
        memcpy(w, in16 + 16 * i + 12, sizeof w);
        if (w[0] >= ctx->materials.n) return fail(ctx, RT_ERANGE, "unit probe %zu: material %u does not exist", i, w[0]);
        if (w[1] > RT_MAX_SAMPLE + RT_DEPTH || w[2] >= RT_MAX_DIM || w[3] >= RT_MAX_DIM)
            return fail(ctx, RT_EINVAL, "unit probe %zu: seed / pixel outside the supported range", i);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceScene sc = device_scene(ctx);
    return debug_roundtrip(ctx, in16, 16 * n * sizeof(float), out9, 9 * n * sizeof(float), [&](void *d_in, void *d_out) {
        return ctx->ks->launch_debug_material(ctx, sc, routine, (const float *)d_in, (uint32_t)n, (float *)d_out);
    });
}

int rt_debug_div3(rt_context *ctx, const float *in4, size_t n, float *out6) {
    if (!ctx || !in4 || !out6 || n > (1u << 28)) return RT_EINVAL;
    if (n == 0) return RT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return debug_roundtrip(ctx, in4, 4 * n * sizeof(float), out6, 6 * n * sizeof(float), [&](void *d_in, void *d_out) {
        return ctx->ks->launch_debug_div3(ctx, (const float *)d_in, (uint32_t)n, (float *)d_out);
    });
}

int rt_debug_queue_sums(rt_context *ctx, const float *in3, uint32_t npix, uint32_t count, uint32_t group_log2, float *out4) {
    if (!ctx || !in3 || !out4) return RT_EINVAL;
    if (npix < 1u || npix > 16u || count < 1u || npix * (uint64_t)count > 512u || group_log2 > 6u)   // (a wave's queue: 16 pixels, 512 slots)
        return fail(ctx, RT_EINVAL, "queue_sums probe: %u pixels of %u samples do not fit one wave's queue", npix, count);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return debug_roundtrip(ctx, in3, (size_t)npix * count * 3 * sizeof(float), out4, (size_t)npix * 4 * sizeof(float), [&](void *d_in, void *d_out) {
        return ctx->ks->launch_debug_queue_sums(ctx, (const float *)d_in, npix, count, group_log2, (float *)d_out);
    });
}

int rt_shard_slots(rt_context *ctx, int world, uint32_t *slots_out) {
    if (!ctx || !slots_out || world < 1) return RT_EINVAL;
    uint32_t tw = 1u << ctx->tile_w_log2, th = 1u << ctx->tile_h_log2;
    uint32_t tiles = ((ctx->width + tw - 1) / tw) * ((ctx->height + th - 1) / th);
    *slots_out = ((tiles + world - 1) / world) * tw * th;  // the same for every rank of `world`
    return RT_OK;
}

int rt_pack_accum(rt_context *ctx, void *d_packed, size_t bytes) {
    if (!ctx || !d_packed) return RT_EINVAL;
    uint32_t n = 0;
    rt_shard_slots(ctx, ctx->world, &n);
    if (bytes != (size_t)n * sizeof(float4)) return fail(ctx, RT_EINVAL, "packed buffer must be %zu bytes", (size_t)n * sizeof(float4));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    float cam0[12] = {0};
    FrameParams fp = frame_params(ctx, cam0, 0, 0, 0);
    CLEAR_TRY(ctx);
    hipLaunchKernelGGL(pt_pack, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, fp, ctx->accum.p, (float4 *)d_packed, n);
    HIP_TRY(ctx, hipGetLastError());
    return RT_OK;
}

int rt_unpack_accum(rt_context *ctx, const void *d_packed, size_t bytes, int src_rank, int world) {
    if (!ctx || !d_packed) return RT_EINVAL;
    if (world < 1 || src_rank < 0 || src_rank >= world) return fail(ctx, RT_EINVAL, "rank %d of %d", src_rank, world);
    uint32_t n = 0;
    rt_shard_slots(ctx, world, &n);
    if (bytes != (size_t)n * sizeof(float4)) return fail(ctx, RT_EINVAL, "packed buffer must be %zu bytes", (size_t)n * sizeof(float4));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    float cam0[12] = {0};
    FrameParams fp = frame_params(ctx, cam0, 0, 0, 0, src_rank, world);  // the SENDER's shard
    CLEAR_TRY(ctx);
    if (fp.slot_end)
        hipLaunchKernelGGL(pt_unpack, dim3((fp.slot_end + 255) / 256), dim3(256), 0, ctx->stream, fp, (const float4 *)d_packed, ctx->accum.p);
    HIP_TRY(ctx, hipGetLastError());
    return RT_OK;
}

int rt_set_option(rt_context *ctx, int option, int value) {
    if (!ctx) return RT_EINVAL;
    ctx->prefix_changed();   // whichever option it is
    switch (option) {
        case RT_OPT_PREFIX_CACHE: ctx->prefix_cache.enabled = value != 0; return RT_OK;
        case RT_OPT_PREFIX_SHARING: ctx->prefix_sharing = value != 0; return RT_OK;
        case RT_OPT_SAMPLE_QUEUE: ctx->sample_queue = value != 0; return RT_OK;
        case RT_OPT_WALK_SLICES: ctx->walk_slices = value != 0; return RT_OK;
        case RT_OPT_WAVE_FILL: ctx->wave_fill = value != 0; return RT_OK;
        case RT_OPT_EXACT_GRID: ctx->sample_grid.exact = value != 0; return RT_OK;
        case RT_OPT_ACCUM_STORE:
            if (value != 0 && value != 1) return fail(ctx, RT_EINVAL, "RT_OPT_ACCUM_STORE takes 0 or 1");
            if (value == 0) {   // (eager from here on: a clear recorded under 1 is enqueued now)
                HIP_TRY(ctx, hipSetDevice(ctx->device));
                CLEAR_TRY(ctx);
            }
            ctx->accum_store = value != 0;
            return RT_OK;
        case RT_OPT_MOMENTS:
            if (value != 0 && value != 1) return fail(ctx, RT_EINVAL, "RT_OPT_MOMENTS takes 0 or 1");
            if (value == 1 && ctx->world > 1)
                return fail(ctx, RT_EINVAL, "sample moments on a sharded context (rank %d of %d)", ctx->rank, ctx->world);
            if ((value != 0) != ctx->moments.on) ctx->moments.valid = false;   // (until the next rt_clear / rt_render_adaptive)
            ctx->moments.on = value != 0;
            return RT_OK;
        case RT_OPT_LOOKAHEAD:
            if (value < 0 || value == 1 || value > RT_LOOKAHEAD_MAX) return fail(ctx, RT_EINVAL, "RT_OPT_LOOKAHEAD takes 0 or 2..%d", RT_LOOKAHEAD_MAX);
            ctx->lookahead.k = value;
            ctx->lookahead.ring_failed = false;
            return RT_OK;
        case RT_OPT_PREFIX_TREE:
            if (value < 0 || value > 2) return fail(ctx, RT_EINVAL, "RT_OPT_PREFIX_TREE takes 0, 1 or 2");
            ctx->prefix_tree = value;
            return RT_OK;
        case RT_OPT_ACCEL:
            if (value < 0 || value > 2) return fail(ctx, RT_EINVAL, "RT_OPT_ACCEL takes 0, 1 or 2");
            ctx->accel = value;
            return RT_OK;
        case RT_OPT_ARITH: {
            const KernelSet *ks = value == RT_ARITH_IEEE ? kernel_set_a0() : value == RT_ARITH_ROCM_OCL_NOCONTRACT ? kernel_set_a1()
                                  : value == RT_ARITH_ROCM_OCL ? kernel_set_a2() : nullptr;
            if (!ks) return fail(ctx, RT_EINVAL, "RT_OPT_ARITH takes RT_ARITH_IEEE (0), RT_ARITH_ROCM_OCL_NOCONTRACT (1) or RT_ARITH_ROCM_OCL (2)");
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            SYNC_TRY(ctx);
            ctx->arith = value;
            ctx->ks = ks;
            ctx->sample_counter = 0;
            return ctx->have_scene ? apply_arith(ctx) : RT_OK;
        }
        case RT_OPT_MAX_THREADS_PER_LAUNCH:
            if (value < 256) return fail(ctx, RT_EINVAL, "max threads per launch must be >= 256");
            ctx->max_threads_per_launch = (uint32_t)value;
            return RT_OK;
        default: return fail(ctx, RT_EINVAL, "unknown option %d", option);
    }
}

int rt_accum_store_stats(rt_context *ctx, uint64_t *stored, uint64_t *materialised) {
    if (!ctx || !stored || !materialised) return RT_EINVAL;
    *stored = ctx->clears_stored;
    *materialised = ctx->clears_materialised;
    return RT_OK;
}

int rt_prefix_cache_stats(rt_context *ctx, uint64_t *hits, uint64_t *misses) {
    if (!ctx || !hits || !misses) return RT_EINVAL;
    *hits = ctx->prefix_cache.hits;
    *misses = ctx->prefix_cache.misses;
    return RT_OK;
}

int rt_sample_units(uint32_t seg_cap, uint32_t pixels_per_unit, uint32_t count_light, uint32_t count_heavy, uint32_t *units_out) {
    if (!units_out) return fail(nullptr, RT_EINVAL, "units_out is NULL");
    *units_out = 0;
    if (pixels_per_unit == 0) return fail(nullptr, RT_EINVAL, "pixels_per_unit is 0");
    // live_take's clamps, then its two parts: the heavy one first
    const uint32_t cnt_l = std::min(count_light, seg_cap);
    const uint32_t cnt_h = std::min(count_heavy, seg_cap - cnt_l);
    const uint32_t units_h = cnt_h / pixels_per_unit + (cnt_h % pixels_per_unit != 0u);
    const uint32_t units_l = cnt_l / pixels_per_unit + (cnt_l % pixels_per_unit != 0u);
    *units_out = units_h + units_l;   // (<= seg_cap: no overflow)
    return RT_OK;
}

int rt_sample_grid_stats(rt_context *ctx, uint64_t *launches, uint64_t *exact, uint64_t *workgroups, uint64_t *live_last) {
    if (!ctx || !launches || !exact || !workgroups || !live_last) return RT_EINVAL;
    *launches = ctx->sample_grid.launches;
    *exact = ctx->sample_grid.exact_launches;
    *workgroups = ctx->sample_grid.workgroups;
    *live_last = ctx->sample_grid.live_last;
    return RT_OK;
}

int rt_debug_live_list(rt_context *ctx, uint32_t out[4]) {
    if (!ctx || !out) return RT_EINVAL;
    const rt_context::Slots &ss = ctx->slots;
    if (!ss.live.p || ctx->sample_grid.last_plan.pixels_per_wave == 0) return fail(ctx, RT_EINVAL, "no fused launch yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t h[LIVE_COUNT_STRIDE];
    HIP_TRY(ctx, hipMemcpyAsync(h, ss.live.p + ss.capacity + 256u, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    SYNC_TRY(ctx);
    out[0] = ctx->sample_grid.last_facts.seg_cap;
    out[1] = ctx->sample_grid.last_plan.pixels_per_wave;
    out[2] = h[0];
    out[3] = h[LIVE_HEAVY_COUNTER];
    return RT_OK;
}

int rt_debug_plan_samples(const rt_sample_facts *facts, rt_sample_plan *plan_out) {
    if (!facts || !plan_out || facts->count < 1u || facts->glog2 > 6u || facts->seg_cap < facts->n) return RT_EINVAL;
    *plan_out = pt::kernel_set_a2()->plan_samples(*facts);   // (host code: the same in every policy)
    return RT_OK;
}

int rt_debug_last_sample_plan(rt_context *ctx, rt_sample_facts *facts_out, rt_sample_plan *plan_out) {
    if (!ctx || !facts_out || !plan_out) return RT_EINVAL;
    if (ctx->sample_grid.last_plan.pixels_per_wave == 0) return fail(ctx, RT_EINVAL, "no fused launch yet");
    *facts_out = ctx->sample_grid.last_facts;
    *plan_out = ctx->sample_grid.last_plan;
    return RT_OK;
}

int rt_debug_plan_camera_samples(const rt_camera_facts *facts, rt_camera_plan *plan_out) {
    if (!facts || !plan_out || facts->count < 1u || facts->count > RT_SPP_PER_LAUNCH || facts->glog2 > 6u) return RT_EINVAL;
    *plan_out = pt::kernel_set_a2()->plan_camera_samples(*facts);   // (host code: the same in every policy)
    return RT_OK;
}

int rt_debug_last_camera_plan(rt_context *ctx, rt_camera_facts *facts_out, rt_camera_plan *plan_out) {
    if (!ctx || !facts_out || !plan_out) return RT_EINVAL;
    if (ctx->cameras.last_plan.block_size == 0) return fail(ctx, RT_EINVAL, "no camera launch yet");
    *facts_out = ctx->cameras.last_facts;
    *plan_out = ctx->cameras.last_plan;
    return RT_OK;
}

int rt_debug_last_ray_plan(rt_context *ctx, rt_camera_facts *facts_out, rt_camera_plan *plan_out) {
    if (!ctx || !facts_out || !plan_out) return RT_EINVAL;
    if (ctx->rays.last_plan.block_size == 0) return fail(ctx, RT_EINVAL, "no ray launch yet");
    *facts_out = ctx->rays.last_facts;
    *plan_out = ctx->rays.last_plan;
    return RT_OK;
}

int rt_debug_queue_pixels(uint32_t count, uint32_t waves_per_simd, uint32_t static_float4, uint32_t granule, uint32_t *pixels_out) {
    if (!pixels_out || count < 1u || waves_per_simd < 1u || waves_per_simd > 8u || static_float4 > PT_LDS_STATIC_FLOAT4 ||
        (granule != 0u && (granule < 16u || granule > 8192u)))
        return RT_EINVAL;
    *pixels_out = pt::kernel_set_a2()->queue_pixels(count, waves_per_simd, static_float4, granule);   // (host code: the same in every policy)
    return RT_OK;
}

int rt_debug_queue_occupancy(rt_context *ctx, uint32_t lds_bytes, int *blocks_out) {
    if (!ctx || !blocks_out) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ctx->ks->queue_occupancy(ctx, lds_bytes, blocks_out);
}

int rt_debug_wave_fixed(rt_context *ctx, uint64_t out[2]) {
    if (!ctx || !out) return RT_EINVAL;
    out[0] = ctx->sample_grid.count64_launches;
    out[1] = ctx->stage_block.builds;
    return RT_OK;
}

int rt_debug_stage_block(rt_context *ctx, float *out, size_t capacity_float4, uint32_t *float4_out) {
    if (!ctx || !float4_out) return RT_EINVAL;
    if (!ctx->have_scene || ctx->stage_block.generation != ctx->prefix_cache.generation)
        return fail(ctx, RT_EINVAL, "the staged scene block is not built (no fused launch since the last change)");
    const uint32_t n = lds_static_used((uint32_t)ctx->materials.n, (uint32_t)ctx->spheres.n, (uint32_t)ctx->planes.n);
    *float4_out = n;
    if (n == 0) return RT_OK;
    if (!out || capacity_float4 < n) return fail(ctx, RT_EINVAL, "the staged scene block holds %u float4", n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(out, reinterpret_cast<const char *>(ctx->materials.p) + stage_block_offset((uint32_t)ctx->materials.n),
                                n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    SYNC_TRY(ctx);
    return RT_OK;
}

int rt_reset_counters(rt_context *ctx) {
    if (!ctx) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(ctx->counters.p, 0, COUNTER_REPLICAS * COUNTER_STRIDE * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_walk_overflow, 0, sizeof(uint32_t), ctx->stream));
    return RT_OK;
}

int rt_get_counters(rt_context *ctx, rt_counters *out) {
    if (!ctx || !out) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<unsigned long long> h(COUNTER_REPLICAS * COUNTER_STRIDE);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), ctx->counters.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    SYNC_TRY(ctx);
    uint64_t *o = (uint64_t *)out;
    for (int i = 0; i < 14; i++) {
        o[i] = 0;
        for (int r = 0; r < COUNTER_REPLICAS; r++) o[i] += h[(size_t)r * COUNTER_STRIDE + i];
    }
    return RT_OK;
}

int rt_get_debug_counters(rt_context *ctx, uint64_t out[2]) {
    if (!ctx || !out) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<unsigned long long> h(COUNTER_REPLICAS * COUNTER_STRIDE);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), ctx->counters.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    SYNC_TRY(ctx);
    out[0] = out[1] = 0;
    for (int r = 0; r < COUNTER_REPLICAS; r++) {
        out[0] += h[(size_t)r * COUNTER_STRIDE + 14];
        out[1] += h[(size_t)r * COUNTER_STRIDE + 15];
    }
#ifdef PT_WSTAT
    {   // diagnostic build: lane census of pt_samples_w (tools/wstat.py)
        unsigned long long v[12];
        if (hipMemcpy(v, ctx->counters.p + COUNTER_REPLICAS * COUNTER_STRIDE + 8, sizeof v, hipMemcpyDeviceToHost) == hipSuccess) {
            const char *names[12] = {"outer iterations", "active lanes", "phase-0 lanes", "phase-1 lanes", "phase-2 lanes", "walk slices",
                                     "walk steps", "node-test lanes", "(unused)", "leaf phases", "leaf lanes", "finished (idle) lanes"};
            for (int k = 0; k < 12; k++) fprintf(stderr, "[wstat] %-24s %llu\n", names[k], v[k]);
            (void)hipMemset(ctx->counters.p + COUNTER_REPLICAS * COUNTER_STRIDE + 8, 0, sizeof v);
        }
    }
#endif
#if PT_STAMPS
    {   // diagnostic build: print the s_memtime shares of pt_samples_q's sections
        unsigned long long st[8];
        if (hipMemcpy(st, ctx->counters.p + COUNTER_REPLICAS * COUNTER_STRIDE, sizeof st, hipMemcpyDeviceToHost) == hipSuccess) {
            const char *names[6] = {"refill", "scatter", "hit:spheres", "hit:planes/lenses/models", "hit:rebuild+material", "loop"};
            double tot = 0;
            for (int k = 0; k < 6; k++) tot += (double)st[k];
            for (int k = 0; k < 6; k++) fprintf(stderr, "[stamps] %-26s %5.1f %%\n", names[k], tot > 0 ? 100.0 * st[k] / tot : 0.0);
        }
    }
#endif
    return RT_OK;
}

int rt_walk_overflow(rt_context *ctx, uint32_t *flags_out) {
    if (!ctx || !flags_out) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(flags_out, ctx->d_walk_overflow, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    SYNC_TRY(ctx);
    return RT_OK;
}

int rt_debug_builtin(rt_context *ctx, int op, const float *in8, size_t n, float *out4) {
    if (!ctx || !in8 || !out4 || op < 0 || op > 12 || n > (1u << 26)) return RT_EINVAL;
    if (n == 0) return RT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return debug_roundtrip(ctx, in8, 8 * n * sizeof(float), out4, 4 * n * sizeof(float), [&](void *d_in, void *d_out) {
        return ctx->ks->launch_debug_builtin(ctx, op, (const float *)d_in, (uint32_t)n, (float *)d_out);
    });
}

uint64_t rt_counters_bytes(const rt_counters *c) {
    if (!c) return 0;
    return 32 * c->t_sphere + 48 * c->t_plane + 64 * c->t_lens + 12 * c->t_model + 16 * c->t_mesh + 60 * c->t_tri +
           36 * c->h_tri + 48 * c->h_bounce + 12 * c->n_scatter + 4 * c->n_dielectric + 64 * c->n_texfetch +
           (48 + 16) * c->samples + 16 * c->image_reads;
}

int rt_kernel_ms_history(rt_context *ctx, float *ms, size_t cap, size_t *n_out) {
    if (!ctx || !ms || !n_out) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t have = ctx->ev_count < (uint64_t)rt_context::EV_RING ? (size_t)ctx->ev_count : (size_t)rt_context::EV_RING;
    size_t n = have < cap ? have : cap;
    for (size_t i = 0; i < n; i++) {  // oldest of the last n first
        hipEvent_t *evp = ctx->ev[(ctx->ev_count - n + i) % rt_context::EV_RING];
        HIP_TRY(ctx, hipEventSynchronize(evp[1]));
        HIP_TRY(ctx, hipEventElapsedTime(&ms[i], evp[0], evp[1]));
    }
    *n_out = n;
    return RT_OK;
}

int rt_stage_ms_history(rt_context *ctx, float *first_ms, float *second_ms, size_t cap, size_t *n_out) {
    if (!ctx || !first_ms || !second_ms || !n_out) return RT_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t have = ctx->ev_count < (uint64_t)rt_context::EV_RING ? (size_t)ctx->ev_count : (size_t)rt_context::EV_RING;
    size_t n = have < cap ? have : cap;
    for (size_t i = 0; i < n; i++) {  // oldest of the last n first
        hipEvent_t *evp = ctx->ev[(ctx->ev_count - n + i) % rt_context::EV_RING];
        HIP_TRY(ctx, hipEventSynchronize(evp[1]));
        HIP_TRY(ctx, hipEventElapsedTime(&first_ms[i], evp[0], evp[2]));
        HIP_TRY(ctx, hipEventElapsedTime(&second_ms[i], evp[2], evp[1]));
    }
    *n_out = n;
    return RT_OK;
}

int rt_last_kernel_ms(rt_context *ctx, float *ms) {
    if (!ctx || !ms) return RT_EINVAL;
    if (ctx->ev_count == 0) return fail(ctx, RT_ESTATE, "no render call has been timed yet");
    size_t n = 0;
    return rt_kernel_ms_history(ctx, ms, 1, &n);
}

int rt_device_info(rt_context *ctx, char *name, size_t name_len, int *cu_count, char *arch, size_t arch_len) {
    if (!ctx) return RT_EINVAL;
    if (name && name_len) snprintf(name, name_len, "%s", ctx->dev_name.c_str());
    if (arch && arch_len) snprintf(arch, arch_len, "%s", ctx->dev_arch.c_str());
    if (cu_count) *cu_count = ctx->cu_count;
    return RT_OK;
}

}  // extern "C"
