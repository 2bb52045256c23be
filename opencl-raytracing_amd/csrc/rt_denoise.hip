// rt_denoise.hip — the denoisers of librt_amd.so (include/rt_amd.h, where the math is written out), gfx950 only:
// rt_denoise (edge-avoiding à-trous), rt_denoise_variance and rt_denoise_moments (the variance-guided filter on the
// 7x7 estimate or on the measured sample moments), their kernels and the accessors of their results.  Everything here
// is policy-free: compiled once, with the IEEE divide, like rt_amd.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "rt_context.hpp"

using namespace rtamd;

// ==================================== kernels ====================================

// One launch per à-trous iteration.  At step s = 2^i the 5x5 stencil only ever couples pixels of one residue class
// (x mod s, y mod s), so a workgroup owns a 16x16 tile of one class's sub-lattice {(rx + s i, ry + s j)}, stages the
// 20x20 lattice points of the tile and its 2-point halo into LDS (colour + the guide's three 16-byte groups of the
// feature record: pos_t, normal_obj, albedo_mat), and every tap is an LDS neighbour at distance <= 2 for every step; an
// iteration re-reads 400/256 = 1.56x its input.  The hit flag is read as t < +inf (the same bit as RT_FEATURE_HIT by
// construction of pt_features).
// A staged point carries a key in pos.w: the object id (split objects) or the hit flag, and PT_DN_OFF for a point
// outside the frame, whose data are zeros — a tap's weight is 0 unless its key equals the centre's (a select, no branch).
// CHAINS (RT_DENOISE_SPLIT_CHAINS, kernels of their own so that the others compile as they did): a staged point also
// carries the record's flags >> 8 — chain length and signature of rt_render_features_chain — in albedo.w, which no term
// reads (there the record holds the material id); a tap then counts only if key AND that word equal the centre's.
// Workgroup ids are remapped so that the s classes of one tile row, which share cache lines, run on one XCD.
#define PT_DN_TILE 16
#define PT_DN_SIDE (PT_DN_TILE + 4)
#define PT_DN_POINTS (PT_DN_SIDE * PT_DN_SIDE)
#define PT_DN_OFF 0xFFFFFFFEu          // key of an out-of-frame point (never an object id: 2^30 - 2 meshes)
#define PT_DN_XCDS 8u
struct DenoiseStep {
    uint32_t w, h;
    uint32_t step_log2;                 // s = 1 << step_log2
    uint32_t tiles_x;                   // 16x16 tiles across the widest sub-lattice
    uint32_t groups;                    // s * s * tiles_x * tiles_y
    float inv_n, inv_x, inv_a;          // 1 / sigma^2 of the guides; 0 = term off
    uint32_t split;                     // RT_DENOISE_SPLIT_OBJECTS
    uint32_t first, last;               // src is the accumulator (c0 = rgb / w) / dst gets (sqrt(c), 1) or 0
    float inv_c;                        // pt_atrous: 4^i / sigma_c^2 of this iteration; 0 = term off
    float sigma_l;                      // pt_atrous_vg: sigma_luminance; unused when lum_on == 0
    uint32_t lum_on;                    // pt_atrous_vg: 0 = sigma_luminance is +inf, the luminance term is off
};

PT_DEV float dn_d2(float4 a, float4 b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return dx * dx + dy * dy + dz * dz;
}
PT_DEV float dn_lum(float4 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }

// the accumulator's mean (rgb / w, w); zeros for a pixel that holds no sample
PT_DEV float4 dn_mean(float4 c) {
    const float cw = c.w;
    return cw > 0.0f ? make_float4(c.x / cw, c.y / cw, c.z / cw, cw) : make_float4(0.0f, 0.0f, 0.0f, cw);
}
// pos of a point outside the frame: zeros, the key PT_DN_OFF in w
PT_DEV float4 dn_off() { return make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(PT_DN_OFF)); }
// the guide of in-frame pixel q, its key in pos.w
template <bool CHAINS>
PT_DEV void dn_guide(const float4 *__restrict__ feat, size_t q, uint32_t split, float4 &p, float4 &n, float4 &a) {
    const float4 *f = feat + 5 * q;
    p = f[0];
    n = f[1];
    a = f[2];
    const bool hit = p.w < INFINITY;
    p.w = __uint_as_float(split ? __float_as_uint(n.w) : (hit ? 0u : 1u));
    if (CHAINS) a.w = __uint_as_float(__float_as_uint(f[4].w) >> 8);
}
// a tap's pair (key, chain word) against the centre's
template <bool CHAINS>
PT_DEV bool dn_same(float4 pq, float4 aq, uint32_t keyp, uint32_t chainp) {
    return __float_as_uint(pq.w) == keyp && (!CHAINS || __float_as_uint(aq.w) == chainp);
}
// what a filter's last iteration writes: (sqrt(c), 1), or 0 for a pixel whose accumulator holds no sample
PT_DEV float4 dn_gamma(float r, float g, float b, float count) {
    return count > 0.0f ? make_float4(sqrtf(r), sqrtf(g), sqrtf(b), 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// One iteration of either filter.  VG = false (rt_denoise): colour.w carries the sample count through the iterations,
// the first edge-stopping term is inv_c |c_p - c_q|^2.  VG = true (rt_denoise_variance): colour.w carries the variance
// v(i) (v0 in the first iteration), a point's luminance rides in normal.w (which the key has already been taken from),
// the first term is |l_p - l_q| / (sigma_l sqrt(vt_p) + eps), and the variance is filtered with the squared weights;
// var0, accum and var_out are read and written by this variant only.
template <bool VG, bool CHAINS>
PT_DEV void dn_atrous(const DenoiseStep &ds, const float4 *__restrict__ src, const float *__restrict__ var0,
                      const float4 *__restrict__ accum, const float4 *__restrict__ feat, float4 *__restrict__ dst,
                      float *__restrict__ var_out) {
    __shared__ float4 s_col[PT_DN_POINTS], s_pos[PT_DN_POINTS], s_nrm[PT_DN_POINTS], s_alb[PT_DN_POINTS];
    // XCD remap: consecutive logical groups (the residue classes rx of one tile) share an XCD
    const uint32_t per_xcd = gridDim.x / PT_DN_XCDS;
    const uint32_t g = (blockIdx.x % PT_DN_XCDS) * per_xcd + blockIdx.x / PT_DN_XCDS;
    if (g >= ds.groups) return;
    const uint32_t sl = ds.step_log2, s = 1u << sl;
    const uint32_t rx = g & (s - 1u);
    uint32_t rem = g >> sl;
    const uint32_t tx = rem % ds.tiles_x;
    rem /= ds.tiles_x;
    const uint32_t ry = rem & (s - 1u), ty = rem >> sl;
    const int i0 = (int)(tx * PT_DN_TILE), j0 = (int)(ty * PT_DN_TILE);
    const int nx = (int)((ds.w - rx + s - 1u) >> sl), ny = (int)((ds.h - ry + s - 1u) >> sl);   // the class's lattice size
    if (i0 >= nx || j0 >= ny) return;   // (uniform over the workgroup, before its barrier)
    for (uint32_t k = threadIdx.x; k < PT_DN_POINTS; k += 256u) {
        const int x = (int)rx + (i0 - 2 + (int)(k % PT_DN_SIDE)) * (int)s;
        const int y = (int)ry + (j0 - 2 + (int)(k / PT_DN_SIDE)) * (int)s;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), p = dn_off(), n = c, a = c;
        float l = 0.0f;
        if (x >= 0 && y >= 0 && x < (int)ds.w && y < (int)ds.h) {
            const size_t q = (size_t)y * ds.w + (size_t)x;
            c = src[q];
            if (ds.first) {
                c = dn_mean(c);
                if (VG) c.w = var0[q];
            }
            if (VG) l = dn_lum(c);
            dn_guide<CHAINS>(feat, q, ds.split, p, n, a);
        }
        if (VG) n.w = l;
        s_col[k] = c;
        s_pos[k] = p;
        s_nrm[k] = n;
        s_alb[k] = a;
    }
    __syncthreads();
    const uint32_t li = threadIdx.x & (PT_DN_TILE - 1u), lj = threadIdx.x / PT_DN_TILE;
    const uint32_t x = rx + (((uint32_t)i0 + li) << sl), y = ry + (((uint32_t)j0 + lj) << sl);
    if (x >= ds.w || y >= ds.h) return;
    // vt_p: the 3x3 binomial of v(i) over the unit neighbours inside the frame, renormalised.  They are not on the
    // stride-s lattice the tile holds, so the centre thread reads them from global memory (v0 / src.w).
    float inv_d = 0.0f;
    if (VG && ds.lum_on) {
        const float kk[3] = {0.25f, 0.5f, 0.25f};
        float sv = 0.0f, sk = 0.0f;
#pragma unroll
        for (int dy = 0; dy < 3; dy++) {
#pragma unroll
            for (int dx = 0; dx < 3; dx++) {
                const int xx = (int)x + dx - 1, yy = (int)y + dy - 1;
                if (xx >= 0 && yy >= 0 && xx < (int)ds.w && yy < (int)ds.h) {
                    const size_t q = (size_t)yy * ds.w + (size_t)xx;
                    const float v = ds.first ? var0[q] : src[q].w;
                    sv += (kk[dx] * kk[dy]) * v;
                    sk += kk[dx] * kk[dy];
                }
            }
        }
        inv_d = 1.0f / (ds.sigma_l * sqrtf(sv / sk) + RT_DENOISE_VARIANCE_EPS);
    }
    const uint32_t ci = (lj + 2u) * PT_DN_SIDE + li + 2u;
    const float4 cp = s_col[ci], pp = s_pos[ci], np = s_nrm[ci], ap = s_alb[ci];
    const uint32_t keyp = __float_as_uint(pp.w), chainp = __float_as_uint(ap.w);
    const float hk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 5; dy++) {
#pragma unroll
        for (int dx = 0; dx < 5; dx++) {
            const uint32_t q = ci + (uint32_t)((dy - 2) * PT_DN_SIDE + (dx - 2));
            const float4 cq = s_col[q], pq = s_pos[q], nq = s_nrm[q], aq = s_alb[q];
            const float z = (VG ? inv_d * fabsf(np.w - nq.w) : ds.inv_c * dn_d2(cp, cq)) + ds.inv_n * dn_d2(np, nq) +
                            ds.inv_x * dn_d2(pp, pq) + ds.inv_a * dn_d2(ap, aq);
            float wt = (hk[dx] * hk[dy]) * __expf(-z);
            wt = dn_same<CHAINS>(pq, aq, keyp, chainp) ? wt : 0.0f;
            sw += wt;
            sr += wt * cq.x;
            sg += wt * cq.y;
            sb += wt * cq.z;
            if (VG) sv += (wt * wt) * cq.w;
        }
    }
    const float r = sr / sw, gg = sg / sw, b = sb / sw, vn = VG ? sv / (sw * sw) : 0.0f;
    const size_t pix = (size_t)y * ds.w + x;
    if (ds.last) {
        dst[pix] = dn_gamma(r, gg, b, VG ? accum[pix].w : cp.w);
        if (VG) var_out[pix] = vn;
    } else {
        dst[pix] = make_float4(r, gg, b, VG ? vn : cp.w);
    }
}

__global__ __launch_bounds__(256) void pt_atrous(DenoiseStep ds, const float4 *__restrict__ src,
                                                 const float4 *__restrict__ feat, float4 *__restrict__ dst) {
    dn_atrous<false, false>(ds, src, nullptr, nullptr, feat, dst, nullptr);
}
__global__ __launch_bounds__(256) void pt_atrous_ch(DenoiseStep ds, const float4 *__restrict__ src,
                                                    const float4 *__restrict__ feat, float4 *__restrict__ dst) {
    dn_atrous<false, true>(ds, src, nullptr, nullptr, feat, dst, nullptr);
}
__global__ __launch_bounds__(256) void pt_atrous_vg(DenoiseStep ds, const float4 *__restrict__ src,
                                                    const float *__restrict__ var0, const float4 *__restrict__ accum,
                                                    const float4 *__restrict__ feat, float4 *__restrict__ dst,
                                                    float *__restrict__ var_out) {
    dn_atrous<true, false>(ds, src, var0, accum, feat, dst, var_out);
}
__global__ __launch_bounds__(256) void pt_atrous_vg_ch(DenoiseStep ds, const float4 *__restrict__ src,
                                                       const float *__restrict__ var0, const float4 *__restrict__ accum,
                                                       const float4 *__restrict__ feat, float4 *__restrict__ dst,
                                                       float *__restrict__ var_out) {
    dn_atrous<true, true>(ds, src, var0, accum, feat, dst, var_out);
}

// Step 1 of the variance-guided filter, the 7x7 two-pass estimate v0: a workgroup owns a 16x16 pixel tile and stages the
// 22x22 points of the tile and its 3-pixel halo as three float4 (pos + key, normal + l(c0), albedo: 23232 bytes, six
// workgroups per CU), then every thread walks its 49 taps twice from LDS: once for M0 and the mean, once for the squared
// deviations.
#define PT_DV_HALO 3
#define PT_DV_SIDE (PT_DN_TILE + 2 * PT_DV_HALO)
#define PT_DV_POINTS (PT_DV_SIDE * PT_DV_SIDE)
struct DenoiseVariance {
    uint32_t w, h;
    uint32_t tiles_x;                   // 16x16 tiles across the frame
    float inv_n, inv_x, inv_a;          // 1 / sigma^2 of the guides; 0 = term off
    uint32_t split;                     // RT_DENOISE_SPLIT_OBJECTS
};

template <bool CHAINS>
PT_DEV void dn_variance(DenoiseVariance dv, const float4 *__restrict__ accum, const float4 *__restrict__ feat,
                        float *__restrict__ var0) {
    __shared__ float4 s_pos[PT_DV_POINTS], s_nrm[PT_DV_POINTS], s_alb[PT_DV_POINTS];
    const uint32_t tx = blockIdx.x % dv.tiles_x, ty = blockIdx.x / dv.tiles_x;
    const int i0 = (int)(tx * PT_DN_TILE), j0 = (int)(ty * PT_DN_TILE);
    for (uint32_t k = threadIdx.x; k < PT_DV_POINTS; k += 256u) {
        const int x = i0 - PT_DV_HALO + (int)(k % PT_DV_SIDE);
        const int y = j0 - PT_DV_HALO + (int)(k / PT_DV_SIDE);
        float4 p = dn_off(), n = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a = n;
        float l = 0.0f;
        if (x >= 0 && y >= 0 && x < (int)dv.w && y < (int)dv.h) {
            const size_t q = (size_t)y * dv.w + (size_t)x;
            l = dn_lum(dn_mean(accum[q]));
            dn_guide<CHAINS>(feat, q, dv.split, p, n, a);
        }
        n.w = l;
        s_pos[k] = p;
        s_nrm[k] = n;
        s_alb[k] = a;
    }
    __syncthreads();
    const uint32_t li = threadIdx.x & (PT_DN_TILE - 1u), lj = threadIdx.x / PT_DN_TILE;
    const uint32_t x = (uint32_t)i0 + li, y = (uint32_t)j0 + lj;
    if (x >= dv.w || y >= dv.h) return;
    const uint32_t ci = (lj + PT_DV_HALO) * PT_DV_SIDE + li + PT_DV_HALO;
    const float4 pp = s_pos[ci], np = s_nrm[ci], ap = s_alb[ci];
    const uint32_t keyp = __float_as_uint(pp.w), chainp = __float_as_uint(ap.w);
    float m0 = 0.0f, m1 = 0.0f;
    for (int dy = -PT_DV_HALO; dy <= PT_DV_HALO; dy++) {
#pragma unroll
        for (int dx = -PT_DV_HALO; dx <= PT_DV_HALO; dx++) {
            const uint32_t q = ci + (uint32_t)(dy * PT_DV_SIDE + dx);
            const float4 pq = s_pos[q], nq = s_nrm[q], aq = s_alb[q];
            const float z = dv.inv_n * dn_d2(np, nq) + dv.inv_x * dn_d2(pp, pq) + dv.inv_a * dn_d2(ap, aq);
            const float g = dn_same<CHAINS>(pq, aq, keyp, chainp) ? __expf(-z) : 0.0f;
            m0 += g;
            m1 += g * nq.w;
        }
    }
    const float m = m1 / m0;
    float m2 = 0.0f;
    for (int dy = -PT_DV_HALO; dy <= PT_DV_HALO; dy++) {
#pragma unroll
        for (int dx = -PT_DV_HALO; dx <= PT_DV_HALO; dx++) {
            const uint32_t q = ci + (uint32_t)(dy * PT_DV_SIDE + dx);
            const float4 pq = s_pos[q], nq = s_nrm[q], aq = s_alb[q];
            const float z = dv.inv_n * dn_d2(np, nq) + dv.inv_x * dn_d2(pp, pq) + dv.inv_a * dn_d2(ap, aq);
            const float g = dn_same<CHAINS>(pq, aq, keyp, chainp) ? __expf(-z) : 0.0f;
            const float d = nq.w - m;
            m2 += g * (d * d);
        }
    }
    var0[(size_t)y * dv.w + x] = m2 / m0;
}
__global__ __launch_bounds__(256) void pt_dn_variance(DenoiseVariance dv, const float4 *__restrict__ accum,
                                                      const float4 *__restrict__ feat, float *__restrict__ var0) {
    dn_variance<false>(dv, accum, feat, var0);
}
__global__ __launch_bounds__(256) void pt_dn_variance_ch(DenoiseVariance dv, const float4 *__restrict__ accum,
                                                         const float4 *__restrict__ feat, float *__restrict__ var0) {
    dn_variance<true>(dv, accum, feat, var0);
}

// Step 1 of rt_denoise_moments, after pt_dn_variance: where a pixel holds at least RT_DENOISE_MOMENTS_MIN_COUNT samples its
// MEASURED variance of the mean, M2 / (n (n - 1)) (the sample moments, RT_OPT_MOMENTS), replaces the 7x7 estimate.
__global__ __launch_bounds__(256) void pt_dn_measured(const float4 *__restrict__ accum, const float *__restrict__ m2,
                                                      float *__restrict__ var0, uint32_t n_px) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_px) return;
    const float n = accum[i].w;
    if (n >= (float)RT_DENOISE_MOMENTS_MIN_COUNT) var0[i] = m2[i] / (n * (n - 1.0f));
}

// ================================== host side ==================================

namespace {

// What both parameter blocks hold: `sigma_own` is the filter's own term (sigma_color / sigma_luminance).
struct Params {
    uint32_t iterations;
    float sigma_own, sigma_normal, sigma_position, sigma_albedo;
    uint32_t flags;
};

// what rt_denoise and the variance-guided entries check alike (`have`: the caller's parameter pointer is not NULL)
int validate(rt_context *ctx, bool have, const Params &p) {
    if (!ctx) return RT_EINVAL;
    if (!have) return fail(ctx, RT_EINVAL, "denoise parameters are NULL");
    if (ctx->world > 1) return fail(ctx, RT_EINVAL, "denoising a sharded context (rank %d of %d)", ctx->rank, ctx->world);
    if (p.iterations < 1 || p.iterations > RT_DENOISE_MAX_ITERATIONS)
        return fail(ctx, RT_EINVAL, "iterations %u outside 1..%u", p.iterations, RT_DENOISE_MAX_ITERATIONS);
    const float sig[4] = {p.sigma_own, p.sigma_normal, p.sigma_position, p.sigma_albedo};
    for (float v : sig)
        if (!(v > 0.0f)) return fail(ctx, RT_EINVAL, "every sigma must be > 0 (+inf switches its term off)");
    if (p.flags & ~(RT_DENOISE_SPLIT_OBJECTS | RT_DENOISE_SPLIT_CHAINS)) return fail(ctx, RT_EINVAL, "unknown denoise flags 0x%x", p.flags);
    if (!ctx->features.ready) return fail(ctx, RT_ESTATE, "no rt_render_features call since the frame was (re)allocated");
    return RT_OK;
}

// The ping-pong pair and `out` are made together, the two variance planes together on the first call that wants
// them; an allocation that fails takes all five with it.
int ensure_buffers(rt_context *ctx, bool with_variance) {
    rt_context::Denoise &d = ctx->denoise;
    const size_t px = (size_t)ctx->width * ctx->height;
    hipError_t e = hipSuccess;
    if (!d.out.p) {
        e = d.pingpong[0].alloc(px);
        if (e == hipSuccess) e = d.pingpong[1].alloc(px);
        if (e == hipSuccess) e = d.out.alloc(px);
    }
    if (with_variance && !d.var[1].p) {
        if (e == hipSuccess) e = d.var[0].alloc(px);
        if (e == hipSuccess) e = d.var[1].alloc(px);
    }
    if (e == hipSuccess) return RT_OK;
    d = {};
    return fail(ctx, RT_EHIP, "denoise buffers: %s", hipGetErrorString(e));
}

// 1 / sigma^2 as the header's formula has it, (sigma 2^-i)^2 for the colour; +inf -> 0 (term off); a sigma so small
// that the reciprocal overflows is held at FLT_MAX (z = 0 still gives 0 at the centre, not inf * 0)
float inv_sq(float sigma, int i = 0) {
    if (std::isinf(sigma)) return 0.0f;
    const double sd = (double)sigma * std::ldexp(1.0, -i);
    return (float)std::min(1.0 / (sd * sd), (double)FLT_MAX);
}

// Iteration i of `iterations`: the step's lattice geometry and guide terms (the filter's own term is the caller's), the
// grid (whole XCD rounds), and where it reads and writes: the accumulator first, `out` last, the ping-pong pair between.
struct StepPlan {
    DenoiseStep ds;
    uint32_t grid;
    const float4 *src;
    float4 *dst;
};
StepPlan plan_step(const rt_context *ctx, const Params &p, uint32_t i) {
    const rt_context::Denoise &d = ctx->denoise;
    StepPlan sp = {};
    DenoiseStep &ds = sp.ds;
    ds.w = (uint32_t)ctx->width;
    ds.h = (uint32_t)ctx->height;
    ds.step_log2 = i;
    const uint32_t s = 1u << i;
    const uint32_t lat_w = (ds.w + s - 1u) >> i, lat_h = (ds.h + s - 1u) >> i;   // the widest / tallest class
    ds.tiles_x = (lat_w + PT_DN_TILE - 1u) / PT_DN_TILE;
    const uint32_t tiles_y = (lat_h + PT_DN_TILE - 1u) / PT_DN_TILE;
    ds.groups = s * s * ds.tiles_x * tiles_y;
    ds.inv_n = inv_sq(p.sigma_normal);
    ds.inv_x = inv_sq(p.sigma_position);
    ds.inv_a = inv_sq(p.sigma_albedo);
    ds.split = (p.flags & RT_DENOISE_SPLIT_OBJECTS) ? 1u : 0u;
    ds.first = i == 0;
    ds.last = i + 1 == p.iterations;
    sp.grid = (ds.groups + PT_DN_XCDS - 1u) / PT_DN_XCDS * PT_DN_XCDS;
    sp.src = i == 0 ? ctx->accum.p : d.pingpong[(i - 1) & 1u].p;
    sp.dst = ds.last ? d.out.p : d.pingpong[i & 1u].p;
    return sp;
}

const float4 *guide(const rt_context *ctx) { return reinterpret_cast<const float4 *>(ctx->features.records.p); }

// rt_denoise_variance and rt_denoise_moments: one filter, two sources of v0 (`measured`: the sample moments where a pixel
// holds enough samples, the 7x7 estimate elsewhere)
int denoise_variance(rt_context *ctx, const rt_denoise_variance_params *vp, bool measured) {
    const Params p = vp ? Params{vp->iterations, vp->sigma_luminance, vp->sigma_normal, vp->sigma_position, vp->sigma_albedo, vp->flags}
                        : Params{};
    int rc = validate(ctx, vp != nullptr, p);
    if (rc) return rc;
    if (measured && !ctx->moments.target())
        return fail(ctx, RT_ESTATE, "the sample moments are not valid: set RT_OPT_MOMENTS to 1, then rt_clear or rt_render_adaptive");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_buffers(ctx, true)) != RT_OK) return rc;
    CLEAR_TRY(ctx);   // (the filters read the accumulator)
    rt_context::Denoise &d = ctx->denoise;
    const uint32_t w = (uint32_t)ctx->width, h = (uint32_t)ctx->height;
    DenoiseVariance dv;
    dv.w = w;
    dv.h = h;
    dv.tiles_x = (w + PT_DN_TILE - 1u) / PT_DN_TILE;
    dv.inv_n = inv_sq(p.sigma_normal);
    dv.inv_x = inv_sq(p.sigma_position);
    dv.inv_a = inv_sq(p.sigma_albedo);
    dv.split = (p.flags & RT_DENOISE_SPLIT_OBJECTS) ? 1u : 0u;
    const bool chains = (p.flags & RT_DENOISE_SPLIT_CHAINS) != 0;
    hipLaunchKernelGGL(chains ? pt_dn_variance_ch : pt_dn_variance, dim3(dv.tiles_x * ((h + PT_DN_TILE - 1u) / PT_DN_TILE)), dim3(256),
                       0, ctx->stream, dv, ctx->accum.p, guide(ctx), d.var[0].p);
    HIP_TRY(ctx, hipGetLastError());
    if (measured) {
        hipLaunchKernelGGL(pt_dn_measured, dim3((w * h + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->accum.p, ctx->moments.m2.p,
                           d.var[0].p, w * h);
        HIP_TRY(ctx, hipGetLastError());
    }
    for (uint32_t i = 0; i < p.iterations; i++) {
        StepPlan sp = plan_step(ctx, p, i);
        sp.ds.lum_on = std::isinf(p.sigma_own) ? 0u : 1u;
        sp.ds.sigma_l = sp.ds.lum_on ? p.sigma_own : 0.0f;
        hipLaunchKernelGGL(chains ? pt_atrous_vg_ch : pt_atrous_vg, dim3(sp.grid), dim3(256), 0, ctx->stream, sp.ds, sp.src, d.var[0].p, ctx->accum.p,
                           guide(ctx), sp.dst, d.var[1].p);
        HIP_TRY(ctx, hipGetLastError());
    }
    d.ready = true;
    d.var_ready = true;
    return RT_OK;
}

}  // namespace

// ================================== C ABI =====================================

extern "C" {

int rt_denoise(rt_context *ctx, const rt_denoise_params *dp) {
    const Params p = dp ? Params{dp->iterations, dp->sigma_color, dp->sigma_normal, dp->sigma_position, dp->sigma_albedo, dp->flags}
                        : Params{};
    int rc = validate(ctx, dp != nullptr, p);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_buffers(ctx, false)) != RT_OK) return rc;
    CLEAR_TRY(ctx);   // (the filter reads the accumulator)
    for (uint32_t i = 0; i < p.iterations; i++) {
        StepPlan sp = plan_step(ctx, p, i);
        sp.ds.inv_c = inv_sq(p.sigma_own, (int)i);
        hipLaunchKernelGGL((p.flags & RT_DENOISE_SPLIT_CHAINS) ? pt_atrous_ch : pt_atrous, dim3(sp.grid), dim3(256), 0, ctx->stream, sp.ds, sp.src, guide(ctx), sp.dst);
        HIP_TRY(ctx, hipGetLastError());
    }
    ctx->denoise.ready = true;
    return RT_OK;
}

int rt_read_denoised(rt_context *ctx, float *rgba, size_t bytes) {
    if (!ctx) return RT_EINVAL;
    const rt_context::Denoise &d = ctx->denoise;
    return read_back(ctx, rgba, bytes, d.out.p, (size_t)ctx->width * ctx->height * sizeof(float4), "image", d.ready, "rt_denoise");
}

int rt_device_denoised(rt_context *ctx, void **d_rgba) {
    if (!ctx || !d_rgba) return RT_EINVAL;
    if (!ctx->denoise.ready) return fail(ctx, RT_ESTATE, "no rt_denoise call since the frame was (re)allocated");
    *d_rgba = ctx->denoise.out.p;
    return RT_OK;
}

int rt_denoise_variance(rt_context *ctx, const rt_denoise_variance_params *p) { return denoise_variance(ctx, p, false); }
int rt_denoise_moments(rt_context *ctx, const rt_denoise_variance_params *p) { return denoise_variance(ctx, p, true); }

int rt_read_variance(rt_context *ctx, int which, float *out, size_t bytes) {
    if (!ctx) return RT_EINVAL;
    if (which < 0 || which > 1) return fail(ctx, RT_EINVAL, "variance buffer %d outside 0..1", which);
    const rt_context::Denoise &d = ctx->denoise;
    return read_back(ctx, out, bytes, d.var[which].p, (size_t)ctx->width * ctx->height * sizeof(float), "variance", d.var_ready,
                     "rt_denoise_variance");
}

int rt_device_variance(rt_context *ctx, int which, void **d_out) {
    if (!ctx || !d_out) return RT_EINVAL;
    if (which < 0 || which > 1) return fail(ctx, RT_EINVAL, "variance buffer %d outside 0..1", which);
    if (!ctx->denoise.var_ready) return fail(ctx, RT_ESTATE, "no rt_denoise_variance call since the frame was (re)allocated");
    *d_out = ctx->denoise.var[which].p;
    return RT_OK;
}

}  // extern "C"
