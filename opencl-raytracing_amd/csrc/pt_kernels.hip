// pt_kernels.hip — the path-tracing kernels and their launchers, compiled ONCE PER ARITHMETIC POLICY
// (-DPT_ARITH=0|1|2, see pt_arith.hpp) into namespaces pt_a0 / pt_a1 / pt_a2 of the same librt_amd.so.
// rt_amd.hip picks a policy's KernelSet at run time (rt_set_option(RT_OPT_ARITH, ...)).
//
// Build (see __graft_entry__.build_hip()), gfx950 only:
//   policy 0: hipcc -c -DPT_ARITH=0 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt ...
//   policy 1: hipcc -c -DPT_ARITH=1 -ffp-contract=off -fno-hip-fp32-correctly-rounded-divide-sqrt ...
//   policy 2: hipcc -c -DPT_ARITH=2 -ffp-contract=off -fno-hip-fp32-correctly-rounded-divide-sqrt ...
// (the contractions of policy 2 are written out as fma calls at the reference's sites; the compiler never contracts)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_device.hpp"
#include "pt_moments.hpp"
#include "pt_chain.hpp"
#include "rt_context.hpp"
#include "pt_kernels.hpp"
#include "pt_sample.hpp"
#include "pt_queue.hpp"

// This is the policy's translation unit: every kernel but those of rt_render_hemispheres, the launchers and planners, and
// the policy's KernelSet.  The device code its sample kernels share with the gather unit (pt_gather.hip: pt_samples_q_hemi,
// pt_render_hemi) lies in headers both include — pt_sample.hpp (what a sample kernel does around its loop), pt_queue.hpp
// (the wave's sample queue) and pt_samples_q_kernel.hpp (the queue kernel's text, forms 0 – 3 here, form 4 there) — so each
// unit reads one text, and a kernel defined here is defined once.  The launchers reach the gather unit's kernels through
// pt::GatherKernels (pt_kernels.hpp).

namespace PT_NS {
using namespace rtamd;

// =============================== device kernels ===============================

// `count` samples of one colour, summed in the kernels' order: lane l of the pixel's g = 2^group_log2 lanes adds its samples
// l, l + g, … one after the other (k or k + 1 of them: the first r = count mod g lanes have one more), then the
// xor butterfly (offsets g/2 … 1).  Before a butterfly step over n lanes the first r lanes hold one value (X)
// and the others another (Y); lane l takes T(l) + T(l + n/2), so the pattern survives with n/2 lanes:
// r <= n/2 → (X + Y, Y + Y, r), else (X + X, X + Y, r − n/2).  Lane 0's value after the last step is the pixel's sum.
// (Until round 3 only counts that are multiples of g took this shortcut; every other count sent its sky pixels
// through the sample kernel: 56 samples per pixel took longer than 64.)
// The ONE place that forms it: pt_prefix and pt_final_replay both call it, so a replayed pixel gets the traced one's bits.
PT_DEV V3 final_sum(V3 col, uint32_t count, uint32_t group_log2) {
    const uint32_t g = 1u << group_log2;
    V3 Y = mk(0.0f, 0.0f, 0.0f);
    for (uint32_t k = 0; k < (count >> group_log2); k++) Y = Y + col;
    V3 X = Y + col;
    uint32_t r = count & (g - 1u);
    for (uint32_t n = g; n > 1u; n >>= 1) {
        const uint32_t h = n >> 1;
        if (r <= h) { X = X + Y; Y = Y + Y; }
        else { Y = X + Y; X = X + X; r -= h; }
    }
    return r ? X : Y;
}

// Direct path: one work-item per (pixel, sample lane), every sample traced from
// the camera.  Lane l of a group of g = 2^group_log2 lanes traces samples
// first+l, first+l+g, ... of its pixel and sums them in that order; the g partial
// sums are combined by an xor butterfly, and the group's lane 0 updates the pixel:
//   MODE_ACCUM   accum += (sum, count)                      (rt_render_spp, prefix sharing off)
//   MODE_TRACE   image = sqrt(radiance(sample first))        (`trace`,  raytracer.cl:496-510)
//   MODE_RETRACE image = sqrt(mix(new, image², k/(k+1)))     (`retrace`, raytracer.cl:512-532)
// CAMS (MODE_ACCUM only; rt_render_spp_cameras' fixed-lane kernel): sample first + j looks through block j of fp.cams instead of
// fp.cam — the primary ray is formed per sample, everything else is the same code.  The other instantiations never read
// the field.
template <int MODE, bool COUNT, bool ACCEL, bool CAMS = false>
__global__ __launch_bounds__(256) void pt_render(DeviceScene sc, FrameParams fp, float4 *__restrict__ accum,
                                                 float4 *__restrict__ image, unsigned long long *counters) {
    __shared__ float4 s_mat[PT_LDS_STATIC_FLOAT4];
    LaneCounters cn;
    if (COUNT) zero_counters(cn);
    Ctx c{sc, stage_materials(sc, s_mat), &cn};
    c.lwin = staged_winners(sc, s_mat);
    c.lpln = staged_planes(sc, s_mat);

    uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    uint32_t g = 1u << fp.group_log2;
    uint32_t slot = fp.slot_begin + (tid >> fp.group_log2);
    uint32_t lane = tid & (g - 1u);
    uint32_t x = 0, y = 0;
    bool valid = slot < fp.slot_end && slot_to_pixel(fp, slot, x, y) && pixel_active(fp, x, y);

    V3 sum = mk(0.0f, 0.0f, 0.0f);
    const bool mom = MODE == MODE_ACCUM && fp.m2 != nullptr;   // (uniform; never in the compat modes)
    LaneMoments lm{0.0f, 0.0f};
    if (valid) {
        Ray r0 = primary_ray(fp.cam, x, y, fp.w, fp.h);
        for (uint32_t s = fp.first + lane; s < fp.first + fp.count; s += g) {
            if (COUNT) cn.c[CN_SAMPLES]++;
            if (CAMS) r0 = primary_ray(fp.cams + 12u * (s - fp.first), x, y, fp.w, fp.h);
            const V3 rad = radiance<COUNT, ACCEL>(c, r0, s, x, y);
            if (mom) moments_fold(lm, sum, rad);
            sum = sum + rad;
        }
    }
    sum = mom ? group_sum_moments(sum, lm, g) : group_sum(sum, g);
    if (valid && lane == 0) {
        size_t pix = (size_t)y * fp.w + x;
        if (MODE == MODE_ACCUM) {
            if (mom) moments_update(accum, fp.m2, pix, sum, fp.count, lm.m2);
            accumulate(accum, pix, sum, fp.count);
        } else if (MODE == MODE_TRACE) {
            image[pix] = make_float4(sqrt1(sum.x), sqrt1(sum.y), sqrt1(sum.z), 1.0f);   // gamma_corr :488
        } else {
            if (COUNT) cn.c[CN_IMAGE_READS]++;
            float4 prev = image[pix];
            V3 o = retrace_step(mk(prev.x, prev.y, prev.z), sum, fp.first);
            image[pix] = make_float4(o.x, o.y, o.z, 1.0f);
        }
    }
    flush_counters<COUNT>(cn, counters, 1);
}

// Caller-supplied rays, fixed lanes (rt_render_rays / rt_render_ray_sets with counters on, RT_OPT_SAMPLE_QUEUE 0 or sample
// moments — as plan_camera_samples decides): pt_render<MODE_ACCUM>'s shape with slot i of the launch's range = ray i of
// fp.rays.  Lane l of the ray's g lanes traces samples first+l, first+l+g, … of the given ray — used as given, not
// normalised — under the random stream (ray.x, ray.y); the g partial sums meet in the same butterfly and lane 0 adds to
// accum[i] (and m2[i]).  SETS: sample s starts at record s mod set_size of the ray's set, loaded INSIDE the sample loop;
// otherwise the ray's one record is loaded ahead of it.
template <bool COUNT, bool ACCEL, bool SETS>
PT_DEV void render_rays_fixed(const DeviceScene &sc, const FrameParams &fp, float4 *__restrict__ accum, unsigned long long *counters) {
    __shared__ float4 s_mat[PT_LDS_STATIC_FLOAT4];
    LaneCounters cn;
    if (COUNT) zero_counters(cn);
    Ctx c{sc, stage_materials(sc, s_mat), &cn};
    c.lwin = staged_winners(sc, s_mat);
    c.lpln = staged_planes(sc, s_mat);

    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t g = 1u << fp.group_log2;
    const uint32_t index = fp.slot_begin + (tid >> fp.group_log2);
    const uint32_t lane = tid & (g - 1u);
    const bool valid = index < fp.slot_end && ray_active(fp, index);   // (an adaptive round: the rays of active blocks only)

    V3 sum = mk(0.0f, 0.0f, 0.0f);
    const bool mom = fp.m2 != nullptr;   // (uniform)
    LaneMoments lm{0.0f, 0.0f};
    if (valid) {
        float4 ro, rd;
        if (!SETS) ro = fp.rays[2u * (size_t)index], rd = fp.rays[2u * (size_t)index + 1u];
        for (uint32_t s = fp.first + lane; s < fp.first + fp.count; s += g) {
            if (COUNT) cn.c[CN_SAMPLES]++;
            if (SETS) {
                const float4 *rec = ray_set_record(fp, index, ray_set_member(fp, s));
                ro = rec[0], rd = rec[1];
            }
            Ray r0;
            r0.o = mk(ro.x, ro.y, ro.z);
            r0.d = mk(rd.x, rd.y, rd.z);
            const V3 rad = radiance<COUNT, ACCEL>(c, r0, s, __float_as_uint(ro.w), __float_as_uint(rd.w));
            if (mom) moments_fold(lm, sum, rad);
            sum = sum + rad;
        }
    }
    sum = mom ? group_sum_moments(sum, lm, g) : group_sum(sum, g);
    if (valid && lane == 0) {
        if (mom) moments_update(accum, fp.m2, (size_t)index, sum, fp.count, lm.m2);
        accumulate(accum, (size_t)index, sum, fp.count);
    }
    flush_counters<COUNT>(cn, counters, 1);
}
template <bool COUNT, bool ACCEL>
__global__ __launch_bounds__(256) void pt_render_rays(DeviceScene sc, FrameParams fp, float4 *__restrict__ accum,
                                                      unsigned long long *counters) {
    render_rays_fixed<COUNT, ACCEL, false>(sc, fp, accum, counters);
}
template <bool COUNT, bool ACCEL>
__global__ __launch_bounds__(256) void pt_render_raysets(DeviceScene sc, FrameParams fp, float4 *__restrict__ accum,
                                                         unsigned long long *counters) {
    render_rays_fixed<COUNT, ACCEL, true>(sc, fp, accum, counters);
}

// Fused path, stage 1: one work-item per owned PIXEL traces the sample-invariant
// prefix of the pixel's paths (pt_device.hpp "shared deterministic prefix").
// A pixel whose paths never meet a random event (sky, direct light, mirror /
// glass chains) is finished here: all its samples are equal, and their sum in the
// order of stage 2 (k sequential adds per lane, then log2(g) doublings) is
// computed in closed form.  Other pixels are appended to the live list.
// A look-ahead launch (launch_fused_any with a ring) passes accum == NULL: the finished pixels are only LISTED then, and
// pt_final_retrace forms their frames; everything else the kernel writes is what an ordinary launch writes.
// TREES: the instantiation that also builds the shared decision trees (RT_OPT_PREFIX_TREE; never in counting builds).
// The tree phase needs some 120 VGPRs against the prefix's 86: a frame without trees keeps the leaner kernel.
#ifndef PT_PREFIX_WAVES
#define PT_PREFIX_WAVES 4   // waves per SIMD pt_prefix is compiled for (profiles/r05_experiments.md)
#endif
template <bool COUNT, bool ACCEL, bool TREES = false>
__global__ __launch_bounds__(256, TREES ? PT_PREFIX_WAVES : 1) void pt_prefix(DeviceScene sc, FrameParams fp, PixelRec *__restrict__ recs,
                                                 uint32_t *__restrict__ live, uint32_t *__restrict__ live_count,
                                                 float4 *__restrict__ accum, unsigned long long *counters,
                                                 FinalPix *__restrict__ finals, uint32_t *__restrict__ final_n) {
    __shared__ float4 s_mat[PT_LDS_STATIC_FLOAT4];
    LaneCounters cn;
    if (COUNT) zero_counters(cn);
    Ctx c{sc, stage_materials(sc, s_mat), &cn};
    c.lwin = staged_winners(sc, s_mat);
    c.lpln = staged_planes(sc, s_mat);

    uint32_t slot = fp.slot_begin + blockIdx.x * 256u + threadIdx.x;
    uint32_t x = 0, y = 0;
    bool valid = slot < fp.slot_end && slot_to_pixel(fp, slot, x, y) && pixel_active(fp, x, y);
    bool is_live = false, is_final = false;
    PixelRec rec;
    rec.p_kind = rec.n_extra = rec.d = rec.out = rec.col = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (valid) {
        Ray r0 = primary_ray(fp.cam, x, y, fp.w, fp.h);
        rec = trace_prefix<COUNT, ACCEL>(c, r0, x, y);
    }
    if (valid) {
        bool final_px = (__float_as_uint(rec.p_kind.w) & 0xFFu) == REC_FINAL;
        if (final_px) {
            is_final = true;
            if (accum) {   // (every sample of a finished pixel is the same colour: the launch's own M2 is 0)
                const V3 fsum = final_sum(xyz(rec.out), fp.count, fp.group_log2);
                if (fp.m2) moments_update(accum, fp.m2, (size_t)y * fp.w + x, fsum, fp.count, 0.0f);
                // (a launch with counters or a BVH walk never stores: accum_store_qualifies)
                if (COUNT || ACCEL) accumulate(accum, (size_t)y * fp.w + x, fsum, fp.count);
                else accumulate_any(fp, accum, (size_t)y * fp.w + x, fsum, fp.count);
            }
            if (COUNT) cn.c[CN_SAMPLES] += 1;  // scaled by count below
        } else {
            is_live = true;
        }
    }
    // Append the live pixels — slot index and record, both at the pixel's position in the live list, so the sample
    // kernels read records without an indirection.  Order within the list is irrelevant to the result but NOT to the
    // speed of the sample kernel, whose waves take the list chunk by chunk in launch order, a wave living as long as
    // its longest path:
    //  * the pixels of a HEAVY workgroup — one in which some pixel's path went through two or more mirror / glass
    //    bounces, or met glass as its first random event: the neighbourhood of mirrors and glass, where samples get
    //    trapped for many bounces whatever their own first vertex is — are stored from the END of the capacity
    //    downwards and taken FIRST (longest processing time first).  In completion order they sat at the end of the
    //    list (their workgroups finish last) and, started last, WERE the sample kernel's tail: leaving out the last
    //    3 % of the list's chunks made C2's frame 10.6 % shorter, the first 3 % 3.6 %, 3 % in the middle 1.8 %
    //    (profiles/r03_experiments.md);
    //  * the others from 0 upwards in the order in which the workgroups finish — consecutive chunks are neighbouring
    //    pixels: dealing the list out in strands costs 10–55 % (texel and table locality).
    // ONE atomic per WORKGROUP either way: the four waves' counts meet in LDS, thread 0 reserves the workgroup's run,
    // each wave takes its part of it (one atomic per wave made 32 400 waves of a 1080p frame queue on a single
    // address: 0.12 of the kernel's 0.20 ms).
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t kb = __float_as_uint(rec.p_kind.w);
    // (bits 8..15: the vertex's bounce index = mirror / glass bounces before it; a final colour's: hits on its way)
    const bool lane_heavy = valid && (((kb >> 8) & 0xFFu) >= 2u || is_glass_vertex(rec));
    const bool wg_heavy = __syncthreads_or(lane_heavy ? 1 : 0) != 0;
    // Pixels whose first random event is a dielectric surface get a shared decision tree (the tree phase below): their
    // two continuations through the glass are traced once per pixel there instead of once per sample.  Their tree
    // indices are reserved with the same one atomic per workgroup.
    const bool glass = TREES && is_live && is_glass_vertex(rec);
    __shared__ uint32_t s_wave_n[4], s_wave_g[4], s_wave_f[4], s_base, s_tree0;
    __shared__ uint32_t s_tpos[256];                                    // live position of the workgroup's tree j
    __shared__ uint32_t s_wn[PT_TREE_LEVELS];                           // [L]: glass vertices waiting for level L
    __shared__ uint16_t s_wait[PT_TREE_LEVELS > 2 ? 2 : 1][256u << (PT_TREE_LEVELS - 1)];   // (heap << 8 | j) of those, by level parity
    unsigned long long m = __ballot(is_live);
    const unsigned long long gm = __ballot(glass);
    const unsigned long long fm = __ballot(is_final);
    if (lane == 0) {
        s_wave_n[wv] = (uint32_t)__popcll(m);
        s_wave_f[wv] = (uint32_t)__popcll(fm);
        if (TREES) s_wave_g[wv] = (uint32_t)__popcll(gm);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = s_wave_n[0] + s_wave_n[1] + s_wave_n[2] + s_wave_n[3];
        s_base = total ? atomicAdd(&live_count[wg_heavy ? LIVE_HEAVY_COUNTER : 0u], total) : 0u;
        if (TREES) {
            const uint32_t trees = s_wave_g[0] + s_wave_g[1] + s_wave_g[2] + s_wave_g[3];
            s_tree0 = trees ? atomicAdd(fp.tree_count, trees) : 0u;
            for (uint32_t l = 0; l < PT_TREE_LEVELS; l++) s_wn[l] = 0u;
        }
    }
    __syncthreads();
    uint32_t pos = 0u;
    if (is_live) {
        uint32_t before = 0;
        for (uint32_t k = 0; k < wv; k++) before += s_wave_n[k];
        pos = s_base + before + lanes_below(m);
        if (wg_heavy) pos = fp.seg_cap - 1u - pos;
        live[pos] = slot;
        recs[pos] = rec;
    }
    // The finished pixels — slot and colour, at [256 b, 256 b + final_n[b]) of the finished list for workgroup b, in ballot
    // order: no atomic (the run's place is the workgroup's own), and the order is irrelevant because a pixel appears once.
    // While camera and scene rest, pt_final_replay forms their sums for the next call's samples from this list.
    // (Not in counting builds: a counting launch is never kept, launch_fused.)
    if (!COUNT && is_final) {
        uint32_t before = 0;
        for (uint32_t k = 0; k < wv; k++) before += s_wave_f[k];
        FinalPix e;
        e.slot = slot;
        e.r = rec.out.x;
        e.g = rec.out.y;
        e.b = rec.out.z;
        finals[blockIdx.x * 256u + before + lanes_below(fm)] = e;
    }
    if (!COUNT && threadIdx.x == 0) final_n[blockIdx.x] = s_wave_f[0] + s_wave_f[1] + s_wave_f[2] + s_wave_f[3];
    flush_counters<COUNT>(cn, counters, fp.count);  // the prefix stands for `count` samples' worth of work
    if (!TREES) return;
    // Tree phase (pt_types.hpp PixelTree): the trees of the workgroup's glass-first pixels, level by level, two
    // work-items per waiting glass vertex (one per continuation: refracted / reflected ray), so that every work-item
    // traces ONE stretch of path.  Tree j of the workgroup is tree s_tree0 + j; a pixel beyond the capacity gets none
    // and continues per sample.  These work-items run in the gaps of the other workgroups' prefix waves: as launches
    // of their own (until round 5), two levels cost 0.09 ms of a 1.43 ms C2 step, each lasting as long as its longest
    // stretch of path with a few thousand waves in flight.
    const uint32_t tree0 = s_tree0;
    const uint32_t nt = tree0 < fp.tree_cap ? min(s_wave_g[0] + s_wave_g[1] + s_wave_g[2] + s_wave_g[3], fp.tree_cap - tree0) : 0u;
    if (nt == 0u) return;   // (workgroup-uniform)
    if (glass) {
        uint32_t before = 0;
        for (uint32_t k = 0; k < wv; k++) before += s_wave_g[k];
        const uint32_t j = before + lanes_below(gm);
        if (j < nt) {
            s_tpos[j] = pos;
            fp.trees[tree0 + j].dec[0].hsh = 0u;   // the tree's leaf counter
        }
    }
    __syncthreads();   // (the records, the positions and the leaf counters are the other work-items')
    for (uint32_t level = 0; level < PT_TREE_LEVELS; level++) {
        const uint32_t items = 2u * (level ? s_wn[level] : nt);
        for (uint32_t t = threadIdx.x; t < items; t += 256u) {
            const uint32_t e = level ? (uint32_t)s_wait[(level - 1u) & 1u][t >> 1] : (1u << 8) | (t >> 1);
            const uint32_t j = e & 0xFFu, heap = e >> 8, which = t & 1u, tree = tree0 + j;
            if (tree_step<ACCEL>(c, fp.trees + tree, tree, heap, which, level + 1u == PT_TREE_LEVELS, recs + s_tpos[j],
                                 fp.tree_wait + (size_t)tree * PT_TREE_WAITS)) {
                const uint32_t k = atomicAdd(&s_wn[level + 1u], 1u);
                s_wait[level & 1u][k] = (uint16_t)(((2u * heap + which) << 8) | j);
            }
        }
        if (level + 1u < PT_TREE_LEVELS) __syncthreads();
    }
}

// Fused path, stage 1 while the prefix is still valid (launch_fused, rt_context::PrefixCache): records, live list,
// counters and trees lie in the slot buffers as the last pt_prefix left them, and all that remains of the first stage is
// the finished pixels' share of THIS call's samples.  One workgroup per pt_prefix workgroup over its run of the
// finished list; final_sum is the function pt_prefix calls, with this call's count and group size.
__global__ __launch_bounds__(256) void pt_final_replay(FrameParams fp, const FinalPix *__restrict__ finals,
                                                       const uint32_t *__restrict__ final_n, float4 *__restrict__ accum) {
    if (threadIdx.x >= min(final_n[blockIdx.x], 256u)) return;
    const FinalPix e = finals[blockIdx.x * 256u + threadIdx.x];
    uint32_t x = 0, y = 0;
    if (!slot_to_pixel(fp, e.slot, x, y)) return;   // (never: pt_prefix stored the slots of valid pixels only)
    const V3 fsum = final_sum(mk(e.r, e.g, e.b), fp.count, fp.group_log2);
    if (fp.m2) moments_update(accum, fp.m2, (size_t)y * fp.w + x, fsum, fp.count, 0.0f);   // (as pt_prefix)
    accumulate_any(fp, accum, (size_t)y * fp.w + x, fsum, fp.count);
}

// Look-ahead launches (FrameParams::la_ring): the finished pixels' part of the fp.count frames.  Every sample of such a pixel
// is the listed colour, so its chain is `count` retrace steps with that colour from the image as it lies, the result of
// step j going to frame j of the ring.  pt_final_replay's grid; runs after pt_prefix and on a prefix-cache hit alike.
__global__ __launch_bounds__(256) void pt_final_retrace(FrameParams fp, const FinalPix *__restrict__ finals,
                                                        const uint32_t *__restrict__ final_n) {
    if (threadIdx.x >= min(final_n[blockIdx.x], 256u)) return;
    const FinalPix e = finals[blockIdx.x * 256u + threadIdx.x];
    uint32_t x = 0, y = 0;
    if (!slot_to_pixel(fp, e.slot, x, y)) return;   // (never: pt_prefix stored the slots of valid pixels only)
    const size_t pix = (size_t)y * fp.w + x;
    const float4 at = fp.la_image[pix];
    V3 prev = mk(at.x, at.y, at.z);
    const V3 sum = mk(0.0f, 0.0f, 0.0f) + mk(e.r, e.g, e.b);   // the sum of a one-sample group, as pt_render forms it
    for (uint32_t j = 0; j < fp.count; j++) {
        prev = retrace_step(prev, sum, fp.first + j);
        fp.la_ring[ring_at(fp, pix, j)] = make_float4(prev.x, prev.y, prev.z, 1.0f);
    }
}

// Fused path, stage 2: one group of g lanes per LIVE pixel; each lane continues
// its samples from the pixel's record.  Same summation order as pt_render.
template <bool COUNT, bool ACCEL>
__global__ __launch_bounds__(256) void pt_samples(DeviceScene sc, FrameParams fp, const PixelRec *__restrict__ recs,
                                                  const uint32_t *__restrict__ live,
                                                  const uint32_t *__restrict__ live_count,
                                                  float4 *__restrict__ accum, unsigned long long *counters) {
    __shared__ float4 s_mat[PT_LDS_STATIC_FLOAT4];
    // A workgroup whose FIRST pixel group lies beyond the live list owns no pixel at all (live_take hands the list out in
    // unit order): it leaves before anything is staged — no barrier, and only zeros to add to the counters.
    {
        uint32_t e0 = 0;
        if (live_take(fp, live_count, (blockIdx.x * 256u) >> fp.group_log2, 1u, e0) == 0u) return;
    }
    LaneCounters cn;
    if (COUNT) zero_counters(cn);
    Ctx c{sc, stage_materials(sc, s_mat), &cn};
    c.lwin = staged_winners(sc, s_mat);
    c.lpln = staged_planes(sc, s_mat);

    uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    uint32_t g = 1u << fp.group_log2;
    uint32_t li = tid >> fp.group_log2;
    uint32_t lane = tid & (g - 1u);
    uint32_t entry = 0;
    bool valid = live_take(fp, live_count, li, 1u, entry) != 0u;
    uint32_t x = 0, y = 0;
    V3 sum = mk(0.0f, 0.0f, 0.0f);
    const bool mom = fp.m2 != nullptr;   // (uniform)
    LaneMoments lm{0.0f, 0.0f};
    if (valid) {
        uint32_t slot = live[entry];
        (void)slot_to_pixel(fp, slot, x, y);
        PixelRec rec = recs[entry];
        for (uint32_t s = fp.first + lane; s < fp.first + fp.count; s += g) {
            if (COUNT) cn.c[CN_SAMPLES]++;
            const V3 rad = radiance_from_rec<COUNT, ACCEL>(c, rec, s, x, y, fp.trees);
            if (mom) moments_fold(lm, sum, rad);
            sum = sum + rad;
        }
    }
    sum = mom ? group_sum_moments(sum, lm, g) : group_sum(sum, g);
    if (valid && lane == 0) {
        if (mom) moments_update(accum, fp.m2, (size_t)y * fp.w + x, sum, fp.count, lm.m2);
        accumulate(accum, (size_t)y * fp.w + x, sum, fp.count);
    }
    flush_counters<COUNT>(cn, counters, 1);
}

// Fused path, stage 2 with the wave's sample queue (pt_queue.hpp): pt_samples_q and its forms.
// ACCEL: the sphere BVH walk is compiled in.  GEOM: 0 = the scene holds spheres and planes only (C1, C2, C4: no
// lens, model or mesh code at all), 1 = everything by brute force or through the sphere BVH, 2 = the mesh BVH
// walk too.  A scene whose only BVH is the sphere BVH (C4) runs <true, 0>: without the mesh walk's registers the
// kernel keeps 6 waves per SIMD.
// COUNT_LOG2 = 6: the launch has exactly 64 samples per pixel and 64 lanes per pixel (fp.count == 64, fp.group_log2 == 6;
// launch_fused picks it for <false, false, …> only) — the queue's index arithmetic and sums are written for that count.
// CAM: the from-the-camera entry (rt_render_spp_cameras; never with COUNT, MOMENTS or a COUNT_LOG2): a refilled lane takes
// the primary ray of its sample's own camera block, depth 0 and path colour (1, 1, 1), and — there is no interaction at
// the camera — passes its first interaction step (`fresh`) and enters the loop at the nearest-hit step; from there the
// body, queue_put and queue_sums are the code of the record-fed instantiations.  recs, live and live_count are NULL.
// The kernel's text is csrc/pt_samples_q_kernel.hpp, included twice below: as pt_samples_q, and as
// pt_samples_q_la<GEOM, WAVES> — CAM_LA, the LOOK-AHEAD form of the camera entry's ACCEL rows (rt_render_again_cameras), which
// ends in queue_replay<true> instead of queue_sums.  The two CAM rows without a BVH walk carry the wave-uniform branch on
// fp.la_ring that the record-fed kernels carry — it costs them neither a register nor scratch.  The three ACCEL rows sit on
// the 96-VGPR budget of their five waves, and there the branch cost the (ACCEL, GEOM 2) row scratch under the ROCm-OpenCL
// policies (8 -> 12 bytes, 3 -> 6 / 4 spilled VGPRs): these rows carry no branch and their look-ahead form is a kernel
// of its own, chosen by the host.  (A second kernel around a shared __device__ body, and an eighth template parameter, were
// both tried: the first moved scalar instructions in a dozen instantiations, the second renames every one of them.  Two
// inclusions of one text leave every other kernel's code as it was — DESIGN.md, "Progressive anti-aliasing".)
#define PT_Q_LOOKAHEAD_FORM 0
#include "pt_samples_q_kernel.hpp"
#undef PT_Q_LOOKAHEAD_FORM
#define PT_Q_LOOKAHEAD_FORM 1
#include "pt_samples_q_kernel.hpp"
#undef PT_Q_LOOKAHEAD_FORM
// … and a third time as pt_samples_q_rays<ACCEL, GEOM, WAVES>, the camera entry fed from a ray buffer (rt_render_rays;
// queue_stage_rays, pt_queue.hpp): a kernel of its own for the same reason — the existing instantiations keep their code.
#define PT_Q_LOOKAHEAD_FORM 2
#include "pt_samples_q_kernel.hpp"
#undef PT_Q_LOOKAHEAD_FORM
// … and a fourth time as pt_samples_q_raysets<ACCEL, GEOM, WAVES>, the ray form with a set of records per ray
// (rt_render_ray_sets; queue_stage_raysets, pt_queue.hpp).  The fifth form, pt_samples_q_hemi, is the gather unit's (pt_gather.hip).
#define PT_Q_LOOKAHEAD_FORM 3
#include "pt_samples_q_kernel.hpp"
#undef PT_Q_LOOKAHEAD_FORM

// The context's staged scene block (rt_context::StageBlock): stage_materials' tables by stage_materials' loops, compiled
// in this translation unit — the divisions are the policy's.  One workgroup.
__global__ __launch_bounds__(64) void pt_stage_block(DeviceScene sc, float4 *__restrict__ block) {
    stage_tables(sc, block, lds_mat_n(sc.material_count), lds_win_n(sc.sphere_count), lds_pln_n(sc.plane_count));
}

// pt_samples_w — the sample queue for scenes in which every mesh of every model has a BVH (C5: one mesh of
// 50 000 faces).  The mesh walk
// is the bulk of such a frame, and its length differs per lane from a handful of nodes (the root is missed)
// to hundreds: run in place, a wave executes the walk loop until its slowest lane is through — rocprofv3
// counted 9 of 64 lanes active per VALU instruction on C5.  Here every lane is a small state machine
//     0 material interaction + spheres/planes/lenses → 1 walking → 2 winner's record, material, next bounce
// and each loop iteration advances EVERY walking lane by at most PT_WALK_STEPS nodes (the threaded walk's
// whole position is one node index), while lanes in the cheap states 0 and 2 pass through them: lanes start
// and finish walks at different times, so the walk loop always has many lanes in it.  Same arithmetic per
// sample as pt_samples_q, same slots, same summation order: bit-identical.
#ifndef PT_WALK_STEPS
#define PT_WALK_STEPS 24u  // A/B: 8 → 122.9 ms, 16 → 118.3, 24 → 116.5, 48 → 118.4
#endif
// The root of the (single) mesh is tested while the lane is still in state 0: a ray that misses the whole mesh (a third of
// C5's walks) goes straight to state 2 instead of idling through a slice, and the cheap states repeat (at most
// PT_W_CHEAP_REPEATS times) while at least PT_W_CHEAP_AGAIN lanes came out of them with no walk to join.  C5 at 4K x 512 spp:
// off 561.8 ms, root test without repeats 571.6, repeats from 4 / 8 / 16 lanes 548.6 / 546.6 / 545.6.  (Ending a slice early once
// 8 / 16 / 24 of its lanes are through: 593.7 / 558.8 / 553.4 vs 548.2 — the fixed slice stays.)
#ifndef PT_W_CHEAP_AGAIN
#define PT_W_CHEAP_AGAIN 8u
#endif
#ifndef PT_W_CHEAP_REPEATS
#define PT_W_CHEAP_REPEATS 4u
#endif
#ifndef PT_W_WAVES
#define PT_W_WAVES 6  // A/B on C5 at 16 spp (round 2, 92 VGPRs): 4 → 116.5 ms, 5 → 110.2, 6 → 116.1 (spills); round 3 (the loop reordered: 79 VGPRs) at 1080p x 64 spp: 5 → 20.87, 6 → 20.65
#endif
#ifndef PT_W_WAVES_MULTI
#define PT_W_WAVES_MULTI 4  // several meshes: the running minimum over the jobs needs 13 more VGPRs — 109, no scratch at 4 waves per SIMD
#endif
template <bool MULTI, bool MOMENTS = false>
__global__ __launch_bounds__(64, MULTI ? PT_W_WAVES_MULTI : PT_W_WAVES) void pt_samples_w(DeviceScene sc, FrameParams fp, const PixelRec *__restrict__ recs,
                                                    const uint32_t *__restrict__ live,
                                                    const uint32_t *__restrict__ live_count,
                                                    float4 *__restrict__ accum, uint32_t pixels_per_wave,
                                                    const uint2 *__restrict__ jobs, uint32_t n_jobs
#ifdef PT_WSTAT
                                                    , unsigned long long *wstat
#endif
                                                    ) {
    extern __shared__ float4 s_dyn[];
    // (as in pt_samples_q: a wave without pixels leaves before anything is staged)
    uint32_t pix0 = 0;
    const uint32_t npix = live_take(fp, live_count, blockIdx.x, pixels_per_wave, pix0);
    if (npix == 0u) return;
    float4 *s_mat = s_dyn;
    Ctx c{sc, stage_materials(sc, s_mat), nullptr};
    c.lwin = staged_winners(sc, s_mat);
    c.lpln = staged_planes(sc, s_mat);
    const WaveQueue q = queue_stage(sc, fp, recs, live, npix, pix0, pixels_per_wave, s_dyn, 0u);

    // The walks of a bounce, in the reference's order: jobs[j] = (mesh index, material of its model), model by
    // model, mesh by mesh.  hitModel's "nearest of my meshes" followed by hitScene's "nearer than the best so
    // far" (:305-320, :349-356) equals ONE running strict-< minimum over this flat list, which is what state 1
    // keeps.  MULTI = false: a single job, its constants wave-uniform.
    const uint32_t mesh0 = jobs[0].x, mat0 = jobs[0].y;
    const uint32_t faces0 = sc.meshes[mesh0].face_count;
    const uint32_t root0 = sc.mesh_bvh_root[mesh0];

    uint32_t next = 0;  // wave-uniform head of the queue
    bool active = false;
    int phase = 0;
    uint32_t idx = 0, depth = 0, bv = 0, bu = 0;   // (see pt_samples_q: hit point and sample / pixel are not carried)
    V3 col = mk(0.0f, 0.0f, 0.0f), out = mk(0.0f, 0.0f, 0.0f);   // col: material colour or texel of the hit
    Ray r;
    r.o = r.d = mk(0.0f, 0.0f, 0.0f);
    V3 hn = mk(0.0f, 0.0f, 0.0f);
    uint32_t hmat = 0;
    float nb_t = RT_MAX_DISTANCE;       // nearest sphere / plane / lens of the current bounce
    uint32_t nb_id = PT_NO_HIT;
    MeshWalk wpos = mesh_walk_start(0);  // the walk's position and its best face so far
    uint32_t wbest = 0;
    float wt = 0.0f, wu = 0.0f, wv = 0.0f;
    uint32_t job = 0;                   // MULTI: the job being walked, and the winning mesh hit so far
    uint32_t nb_face = 0, nb_mat = 0;
    float nb_u = 0.0f, nb_v = 0.0f;

    // MULTI: move `job` on to the next mesh whose ROOT the ray does not miss — the root's node test runs here, in the cheap
    // code, so a bounce costs a walk slice per mesh the ray may touch, not one per mesh of the scene — and set the walk
    // up behind that root; false: no such mesh is left (the bounce's mesh search is over)
    auto enter_job = [&]() {
        while (job < n_jobs) {
            const uint32_t mesh_n = jobs[job].x;
            wbest = sc.meshes[mesh_n].face_count;
            wt = wu = wv = 0.0f;
            wpos = mesh_walk_first(sc, r, sc.mesh_bvh_root[mesh_n], wbest);
            if (wpos.cur != PT_MESH_END) return true;
            job++;
        }
        return false;
    };
#ifdef PT_WSTAT
    WalkStat ws = {0, 0, 0, 0, 0};
    unsigned long long it_n = 0, it_active = 0, it_p0 = 0, it_p1 = 0, it_p2 = 0, it_walk_calls = 0;
#endif
    // every iteration takes samples off the queue, or moves every active lane on (a bounce, or up to
    // PT_WALK_STEPS nodes of a walk that visits each of the < 2^28 nodes at most 3 times)
    for (unsigned long long guard = ((unsigned long long)q.total + 1ull) * (RT_DEPTH + 2ull) * (3ull * (1ull << 28) / PT_WALK_STEPS + 4ull); guard; guard--) {
        // Which lanes are inside a walk, and which want one of the cheap steps (the winner's record after a walk, a new
        // sample from the queue, a material interaction + the primitives that are not models)?  The cheap steps run as
        // soon as ONE lane wants one.  (Holding them back until 8 / 16 / 24 / 32 lanes wait, C5 at 1080p x 64 spp: 21.14 /
        // 21.41 / 21.79 / 22.42 ms against 20.87, 16 with slices of 12 / 8 nodes 20.79 / 21.01 — waiting lanes cost more
        // than sparsely filled cheap steps.)
        const bool walking = active && phase == 1;
        const bool wants_cheap = (active && phase != 1) || (!active && next < q.total);
        const uint32_t n_cheap = (uint32_t)__popcll(__ballot(wants_cheap));
        const bool any_walk = __any(walking);
        if (n_cheap == 0u && !any_walk) break;   // every path is through and the queue is empty
#ifdef PT_WSTAT
        it_n++;
        it_active += __popcll(__ballot(active));
        it_p0 += __popcll(__ballot(active && phase == 0));
        it_p1 += __popcll(__ballot(active && phase == 1));
        it_p2 += __popcll(__ballot(active && phase == 2));
#endif
        if (n_cheap) {
          // (a ray that misses the mesh's root goes from state 0 straight to state 2; the cheap states repeat while at
          // least PT_W_CHEAP_AGAIN lanes came out of them without a walk to join)
          for (uint32_t again = 0;; again++) {
            // ---- state 2: the winner's record, its material
            if (active && phase == 2) {
                Nearest nb;
                nb.t = nb_t;
                nb.id = nb_id;
                if (MULTI) {
                    nb.face = nb_face;
                    nb.mat = nb_mat;
                    nb.u = nb_u;
                    nb.v = nb_v;
                } else if (wbest < faces0 && wt < RT_MAX_DISTANCE && wt < nb.t) {
                    nb.t = wt;
                    nb.id = K_MESH | mesh0;
                    nb.face = wbest;
                    nb.mat = mat0;
                    nb.u = wu;
                    nb.v = wv;
                }
                V3 res;
                bool done = false;
                Hit h;
                h.p = h.n = mk(0.0f, 0.0f, 0.0f);
                h.u = h.v = 0.0f;
                h.tex = h.mat = 0;
                if (!hit_finish<false>(c, r, nb, h)) {
                    res = mk(0.0f, 0.0f, 0.0f);
                    done = true;
                } else {
                    int type;
                    float extra;
                    load_material(c, h.mat, type, extra, col);
                    if (type == RT_LIGHT) {
                        res = vmin(out, col);
                        done = true;
                    } else if (type == RT_TEXTURED) {
                        col = texture_rgb(c.sc, h.u, h.v, h.tex);
                    }
                }
                phase = 0;
                if (done) {
                    queue_put(q, idx, res);
                    active = false;
                } else {   // the next interaction happens here
                    r.o = h.p;
                    hn = h.n;
                    hmat = h.mat;
                }
            }
            // ---- refill idle lanes from the queue
            bool need = !active;
            unsigned long long m = __ballot(need);
            if (m && next < q.total) {
                uint32_t cand = next + lanes_below(m);
                if (need && cand < q.total) {
                    idx = cand;
                    const QueueEntry e = queue_fetch(q, sc, fp, idx);
                    bv = e.bv;
                    bu = e.bu;
                    if ((e.bits & 0xFFu) == REC_FINAL) {  // a leaf of a tree, or count is not a multiple of g
                        queue_put(q, idx, xyz(e.q3));
                    } else {
                        depth = (e.bits >> 8) & 0xFFu;   // (type and extra_data of the record are the material's: re-read below)
                        hn = xyz(e.q1);
                        r.o = xyz(e.q0);
                        r.d = xyz(e.q2);
                        hmat = __float_as_uint(e.q2.w);
                        out = xyz(e.q3);
                        col = xyz(e.q4);
                        active = true;
                        phase = 0;
                    }
                }
                next += (uint32_t)__popcll(m);
            }
            // ---- state 0: one material interaction, then the primitives that are not models
            if (active && phase == 0) {
                Rnd rnd = fetch_rnd_b(sc.table, r.d, depth, bv, bu);
                Hit at;
                at.p = r.o;
                at.n = hn;
                at.u = at.v = 0.0f;
                at.tex = 0;
                at.mat = hmat;
                int type;
                float extra;
                V3 mcol;
                load_material(c, hmat, type, extra, mcol);
                scatter<false>(c, r, out, at, type, extra, col, rnd, false);
                depth++;
                if (depth >= RT_DEPTH) {  // survived DEPTH bounces: returns what it has (:447,485)
                    queue_put(q, idx, out);
                    active = false;
                } else {
                    Nearest nb;
                    hit_primitives<false, true>(c, r, nb);
                    nb_t = nb.t;
                    nb_id = nb.id;
                    if (MULTI) {
                        nb_face = nb_mat = 0;
                        nb_u = nb_v = 0.0f;
                    }
                    wpos = mesh_walk_start(root0);
                    wbest = faces0;
                    wt = wu = wv = 0.0f;
                    job = 0;
                    phase = 1;
                    if (!MULTI) {
                        wpos = mesh_walk_first(sc, r, root0, faces0);
                        if (wpos.cur == PT_MESH_END) phase = 2;
                    } else if (!enter_job()) {
                        phase = 2;
                    }
                }
            }
            if (again >= PT_W_CHEAP_REPEATS) break;
            if ((uint32_t)__popcll(__ballot((active && phase != 1) || (!active && next < q.total))) < PT_W_CHEAP_AGAIN) break;
          }
        }
        // ---- state 1: a slice of the current job's mesh walk
        if (active && phase == 1) {
            uint32_t hits = 0;
            uint32_t mesh_j = mesh0, mat_j = mat0, faces_j = faces0;
            if (MULTI) {
                uint2 jb = jobs[job];
                mesh_j = jb.x;
                mat_j = jb.y;
                faces_j = sc.meshes[mesh_j].face_count;
            }
#ifdef PT_WSTAT
            it_walk_calls++;
            if (mesh_bvh_steps<0>(sc, r, wpos, wbest, wt, wu, wv, PT_WALK_STEPS, hits, nullptr, &ws)) {
#else
            if (mesh_bvh_steps<0>(sc, r, wpos, wbest, wt, wu, wv, PT_WALK_STEPS, hits)) {
#endif
                if (!MULTI) {
                    phase = 2;  // (the one job's result is merged in state 2, straight from the walk's registers)
                } else {
                if (wbest < faces_j && wt < RT_MAX_DISTANCE && wt < nb_t) {  // the running strict-< minimum
                    nb_t = wt;
                    nb_id = K_MESH | mesh_j;
                    nb_face = wbest;
                    nb_mat = mat_j;
                    nb_u = wu;
                    nb_v = wv;
                }
                job++;
                if (!enter_job()) phase = 2;   // (the next mesh whose root the ray does not miss: stay in state 1)
                }
            }
        }
    }
    if (active) atomicOr(sc.walk_overflow, PT_OVF_WALK_SLICES);   // cold: the outer loop ended on its guard with a path unfinished
#ifdef PT_WSTAT
    if (threadIdx.x == 0 && q.npix) {
        unsigned long long v[12] = {it_n, it_active, it_p0, it_p1, it_p2, it_walk_calls, ws.steps, ws.node_lanes, 0ull,
                                    ws.leaf_runs, ws.leaf_lanes, ws.idle_lanes};
        for (int k = 0; k < 12; k++) atomicAdd(&wstat[k], v[k]);
    }
#endif
    if (!MOMENTS && fp.la_ring) queue_replay<false>(q, fp);   // (wave-uniform: a look-ahead launch; never with moments)
    else queue_sums<MOMENTS, true>(q, fp, accum);
}

// parity probe: one work-item per listed pixel-sample
template <bool ACCEL>
__global__ __launch_bounds__(256) void pt_probe(DeviceScene sc, FrameParams fp, const uint32_t *__restrict__ xs,
                                                const uint32_t *__restrict__ ys, const uint32_t *__restrict__ ss,
                                                uint32_t n, float *__restrict__ out) {
    __shared__ float4 s_mat[PT_LDS_STATIC_FLOAT4];
    Ctx c{sc, stage_materials(sc, s_mat), nullptr};
    c.lwin = staged_winners(sc, s_mat);
    c.lpln = staged_planes(sc, s_mat);
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    Ray r0 = primary_ray(fp.cam, xs[i], ys[i], fp.w, fp.h);
#ifdef PT_PROBE_NODES  // diagnostic build (tools/walk_hist.py): the probe returns (BVH nodes tested, mesh walks, bounces) of the sample
    LaneCounters cn;
    zero_counters(cn);
    c.cn = &cn;
    (void)radiance<true, ACCEL>(c, r0, ss[i], xs[i], ys[i]);
    out[3 * i] = (float)cn.c[CN_DBG_BVH_NODES];
    out[3 * i + 1] = (float)cn.c[CN_T_MESH];
    out[3 * i + 2] = (float)cn.c[CN_BOUNCES];
    return;
#endif
    V3 col = radiance<false, ACCEL>(c, r0, ss[i], xs[i], ys[i]);
    out[3 * i] = col.x;
    out[3 * i + 1] = col.y;
    out[3 * i + 2] = col.z;
}

// The feature record of one ray, the body of every pt_features* kernel: the nearest-hit search of the trace kernels
// (hit_primitives + hit_models + hit_finish, the parts of hit_scene, kept apart for the winner's id and face) in a loop of
// at most max_chain + 1 hits (max_chain <= RT_FEATURE_CHAIN_MAX: at most RT_DEPTH).  A hit whose material type is selected
// in `follow` (RT_FOLLOW_*) is followed through scatter() — a dielectric as RT_REFRACTIVE, rayRefract's rule, so no lane
// draws a random number and nothing reads the table — while fewer than max_chain vertices have been followed; the first
// hit that is not is the terminal: position, normal, the material colour or the path's texel, the primary direction as
// given.  t sums the segments in path order; the flags carry RT_FEATURE_CUT, the chain length (bits 8..12) and the upper
// half of the signature (pt_chain.hpp).  follow == 0 or max_chain == 0: the first hit's record with flags RT_FEATURE_HIT.
// The five float4 of the public rt_feature (include/rt_amd.h) go to `sink`, called exactly once: inside the terminal branch
// or at the miss exit, so that the record is never live across the loop (returned by value it cost 18 to 22 VGPRs,
// profiles/r31_experiments.md).
struct FeatureRec { float4 o0, o1, o2, o3, o4; };
struct FeatureStore {   // the sink of the kernels that write memory: five 16-byte stores
    float4 *o;
    PT_DEV void operator()(const FeatureRec &f) const { o[0] = f.o0; o[1] = f.o1; o[2] = f.o2; o[3] = f.o3; o[4] = f.o4; }
};
template <bool ACCEL, class Sink>
PT_DEV void feature_chain(const Ctx &c, Ray r, uint32_t follow, uint32_t max_chain, Sink sink) {
    const V3 d0 = r.d;
    float t_sum = 0.0f;
    uint32_t len = 0u, sig = 0u;
    FeatureRec f;
    for (uint32_t k = 0u; k <= max_chain; k++) {
        Nearest nb;
        hit_primitives<false, ACCEL>(c, r, nb);
        hit_models<false, ACCEL>(c, r, nb);
        Hit h;
        if (!hit_finish<false>(c, r, nb, h)) break;
        int type;
        float extra;
        V3 col;
        load_material(c, h.mat, type, extra, col);
        t_sum = k == 0u ? nb.t : t_sum + nb.t;
        const bool followed = (type == RT_REFLECTIVE && (follow & RT_FOLLOW_REFLECTIVE)) ||
                              (type == RT_REFRACTIVE && (follow & RT_FOLLOW_REFRACTIVE)) ||
                              (type == RT_DIELECTRIC && (follow & RT_FOLLOW_DIELECTRIC));
        if (followed && len < max_chain) {
            sig = pt::chain_signature_step(sig, nb.id);
            len++;
            Rnd none;  // mirror / glass by rayRefract's rule: no random numbers
            none.v = mk(0.0f, 0.0f, 0.0f);
            none.u = 0.0f;
            V3 path = mk(1.0f, 1.0f, 1.0f);   // (the path colour is not needed)
            scatter<false>(c, r, path, h, type == RT_DIELECTRIC ? RT_REFRACTIVE : type, extra, col, none);
            continue;
        }
        if (type == RT_TEXTURED) col = texture_rgb(c.sc, h.u, h.v, h.tex);
        const bool mesh = (nb.id & K_MASK) == K_MESH;
        const uint32_t flags = RT_FEATURE_HIT | (followed && max_chain ? RT_FEATURE_CUT : 0u) | (len << 8) | (sig & 0xFFFF0000u);
        f.o0 = make_float4(h.p.x, h.p.y, h.p.z, t_sum);
        f.o1 = make_float4(h.n.x, h.n.y, h.n.z, __uint_as_float(nb.id));
        f.o2 = make_float4(col.x, col.y, col.z, __uint_as_float(h.mat));
        f.o3 = make_float4(d0.x, d0.y, d0.z, __uint_as_float(mesh ? nb.face : 0xFFFFFFFFu));
        f.o4 = make_float4(h.u, h.v, __uint_as_float(h.tex), __uint_as_float(flags));
        sink(f);
        return;
    }
    // the chain left the scene (a terminal exists whenever the loop runs out: its last pass cannot follow)
    const float none = __uint_as_float(0xFFFFFFFFu);
    f.o0 = make_float4(0.0f, 0.0f, 0.0f, INFINITY);
    f.o1 = make_float4(0.0f, 0.0f, 0.0f, none);
    f.o2 = make_float4(0.0f, 0.0f, 0.0f, none);
    f.o3 = make_float4(d0.x, d0.y, d0.z, none);
    f.o4 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float((len << 8) | (sig & 0xFFFF0000u)));
    sink(f);
}

// First-hit feature buffers (rt_render_features): one work-item per pixel of the whole frame, feature_chain of the
// pixel's primary ray with literal (follow, max_chain) = (0, 0) — one search, no follow test.  A kernel of its own: it is
// the lean one (47 VGPRs without the BVH walk) that the denoisers run every frame.
template <bool ACCEL>
__global__ __launch_bounds__(256) void pt_features(DeviceScene sc, FrameParams fp, float4 *__restrict__ out) {
    __shared__ float4 s_mat[PT_LDS_STATIC_FLOAT4];
    Ctx c{sc, stage_materials(sc, s_mat), nullptr};
    c.lwin = staged_winners(sc, s_mat);
    c.lpln = staged_planes(sc, s_mat);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)fp.w * (uint32_t)fp.h) return;
    const uint32_t x = i % (uint32_t)fp.w, y = i / (uint32_t)fp.w;
    feature_chain<ACCEL>(c, primary_ray(fp.cam, x, y, fp.w, fp.h), 0u, 0u, FeatureStore{out + 5 * (size_t)i});
}

// Feature buffers at the end of the pixel's mirror / glass chain (rt_render_features_chain): feature_chain of the pixel's
// primary ray.  follow == 0 or max_chain == 0: pt_features' record, bit for bit.
template <bool ACCEL>
__global__ __launch_bounds__(256) void pt_features_chain(DeviceScene sc, FrameParams fp, uint32_t follow, uint32_t max_chain,
                                                         float4 *__restrict__ out) {
    __shared__ float4 s_mat[PT_LDS_STATIC_FLOAT4];
    Ctx c{sc, stage_materials(sc, s_mat), nullptr};
    c.lwin = staged_winners(sc, s_mat);
    c.lpln = staged_planes(sc, s_mat);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)fp.w * (uint32_t)fp.h) return;
    const uint32_t x = i % (uint32_t)fp.w, y = i / (uint32_t)fp.w;
    feature_chain<ACCEL>(c, primary_ray(fp.cam, x, y, fp.w, fp.h), follow, max_chain, FeatureStore{out + 5 * (size_t)i});
}

// Feature records for caller-supplied rays (rt_render_features_rays): feature_chain with record i's primary ray read from
// ray i of the buffer (n rays = the frame's pixels, row-major).  `dir` is the direction as given.
template <bool ACCEL>
__global__ __launch_bounds__(256) void pt_features_rays(DeviceScene sc, const float4 *__restrict__ rays, uint32_t n, uint32_t follow,
                                                        uint32_t max_chain, float4 *__restrict__ out) {
    __shared__ float4 s_mat[PT_LDS_STATIC_FLOAT4];
    Ctx c{sc, stage_materials(sc, s_mat), nullptr};
    c.lwin = staged_winners(sc, s_mat);
    c.lpln = staged_planes(sc, s_mat);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 ro = rays[2u * (size_t)i], rd = rays[2u * (size_t)i + 1u];
    Ray r;
    r.o = mk(ro.x, ro.y, ro.z);
    r.d = mk(rd.x, rd.y, rd.z);
    feature_chain<ACCEL>(c, r, follow, max_chain, FeatureStore{out + 5 * (size_t)i});
}

// The counts of an occlusion kernel leave here (pt_occluded, pt_occluded_hemi): lane = record k of set `set`, occ = its
// answer (false for a lane that is not live).  set_size 1: out[k] = 0 | 1, a plain store.  Otherwise out (zeroed on the
// stream before the launch) receives one integer atomicAdd per run of lanes of a wave that share a set — records are
// consecutive, so a set's lanes are — with the run's count from the ballot: integer sums, the same whatever the order.
// Every lane of the wave arrives here: none leaves before the ballots.  (A run ends before the next head; lanes past the
// last record are not occluded.)
// One text as a statement macro, not a function: with it both kernels keep, instruction for instruction, the code they had
// with the tail written out.  As a force-inlined function (five forms were tried) the compiler lays pt_occluded's search out
// under other registers with 4 – 5 more scalar instructions, and pt_occluded<true> took 1.3 % longer over C5's sets of 16
// in two sessions (profiles/r31_experiments.md).  Each argument is evaluated once on the path that uses it.
#define PT_OCCLUDED_COUNTS(live, occ, k, set, set_size, out)                                                          \
    do {                                                                                                              \
        if ((set_size) == 1u) { /* (uniform) */                                                                       \
            if (live) (out)[(size_t)(k)] = (occ) ? 1u : 0u;                                                           \
        } else {                                                                                                      \
            const uint32_t lane_ = threadIdx.x & 63u, set_ = (set);                                                   \
            const uint32_t before_ = (uint32_t)__shfl_up((int)set_, 1);                                               \
            const bool head_ = (live) && (lane_ == 0u || before_ != set_);                                            \
            const unsigned long long occ_m_ = __ballot(occ), heads_ = __ballot(head_);                                \
            if (head_) {                                                                                              \
                const unsigned long long above_ = lane_ == 63u ? 0ull : heads_ >> (lane_ + 1u);                       \
                const uint32_t len_ = above_ ? (uint32_t)__builtin_ctzll(above_) + 1u : 64u - lane_;                  \
                const unsigned long long run_ = (len_ == 64u ? ~0ull : (1ull << len_) - 1ull) << lane_;               \
                const uint32_t count_ = (uint32_t)__popcll(occ_m_ & run_);                                            \
                if (count_) atomicAdd((out) + (size_t)set_, count_);                                                  \
            }                                                                                                         \
        }                                                                                                             \
    } while (0)

// Occlusion queries (rt_occluded_rays): one lane per record k of n sets x set_size records, ray-major.  The record is
// occluded iff pt_features_rays' first-hit t for it is below its bound — tmax[k], or t_max where tmax is NULL —
// (occluded_scene, pt_device.hpp: the search stops at the first report below the bound; no materials, no record).
// The answers leave through PT_OCCLUDED_COUNTS: out[k] = 0 | 1 for set_size 1, otherwise a count per set.  No lane leaves
// before it.
template <bool ACCEL>
__global__ __launch_bounds__(256) void pt_occluded(DeviceScene sc, const float4 *__restrict__ rays, const float *__restrict__ tmax,
                                                   float t_max, uint32_t records, uint32_t set_size, uint32_t *__restrict__ out) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;   // (records <= 2^31: the grid covers them in 32 bits)
    const bool live = k < records;
    Ray r;
    r.o = r.d = mk(0.0f, 0.0f, 0.0f);
    float b = 0.0f;
    if (live) {
        const float4 ro = rays[2u * (size_t)k], rd = rays[2u * (size_t)k + 1u];
        r.o = mk(ro.x, ro.y, ro.z);
        r.d = mk(rd.x, rd.y, rd.z);
        b = tmax ? tmax[(size_t)k] : t_max;
    }
    // B = min(b, MAX_DISTANCE); a NaN bound or one at or below MIN_DISTANCE is below no report
    const float B = b < RT_MAX_DISTANCE ? b : RT_MAX_DISTANCE;
    const bool skip = !live || !(b > RT_MIN_DISTANCE);
    const bool occ = occluded_scene<ACCEL>(sc, r, B, skip);
    PT_OCCLUDED_COUNTS(live, occ, k, k / set_size, set_size, out);
}

// Hemisphere queries (rt_occluded_hemispheres): pt_occluded with its rays made in registers.  Lane k = i * set_size + t
// makes ray t of feature record i (hemisphere_ray, pt_device.hpp: the lanes of a set read the same 80 bytes) and asks
// occluded_scene with the bound t_max, pt_occluded's rule; a record without a hemisphere is skipped and counts 0.  DUMP
// stores the ray (zero bytes for such a record) at rays_out[k].  out NULL: the spawn form, every lane skips the search.
// The counts leave through PT_OCCLUDED_COUNTS, as pt_occluded's do.
template <bool ACCEL, bool DUMP>
__global__ __launch_bounds__(256) void pt_occluded_hemi(DeviceScene sc, const float4 *__restrict__ feats, uint32_t k0, uint32_t k1,
                                                        uint32_t flags, float offset, float t_max, uint32_t records, uint32_t set_size,
                                                        uint32_t *__restrict__ out, float4 *__restrict__ rays_out) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;   // (records <= 2^31: the grid covers them in 32 bits)
    const bool live = k < records;
    const uint32_t set = k / set_size;
    Ray r;
    r.o = r.d = mk(0.0f, 0.0f, 0.0f);
    bool valid = false;
    if (live) {
        valid = hemisphere_ray(feats + 5u * (size_t)set, k, k0, k1, (flags & RT_HEMI_FACE_FORWARD) != 0u, offset, r);
        if (DUMP) {
            rays_out[2u * (size_t)k] = make_float4(r.o.x, r.o.y, r.o.z, __uint_as_float(valid ? set : 0u));
            rays_out[2u * (size_t)k + 1u] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
        }
    }
    if (!out) return;
    const float B = t_max < RT_MAX_DISTANCE ? t_max : RT_MAX_DISTANCE;
    const bool skip = !valid || !(t_max > RT_MIN_DISTANCE);
    const bool occ = occluded_scene<ACCEL>(sc, r, B, skip);
    PT_OCCLUDED_COUNTS(live, occ, k, set, set_size, out);
}

// Feature records through per-sample cameras (rt_render_features_cameras): lane j < n of a pixel's g = 2^glog2 lanes (one
// wave holds whole pixels) looks through block j of fp.cams and takes feature_chain's record into five registers instead of
// memory.  No lane leaves before the cross-lane steps: a lane without a sample (j >= n, or a pixel past the frame) skips the
// search under a branch and carries neutral values.  Then, per pixel:
//   vote   every lane counts the samples that share its key (object, flags >> 8), reading lanes 0 .. n-1 of its group
//          only; the maximum of (count << 6) | (63 - j) by the butterfly is (m, j*): the largest group, the smallest j
//          among equally large ones, and the smallest j inside it;
//   sums   pos, t, normal, albedo of the HIT samples of every group (a lane that missed or has no sample holds +0) by
//          group_sum's tree (offsets g/2 .. 1), and the number of hit samples c the same way.
// Lane j* writes the record: its own discrete fields and direction, RT_FEATURE_MIXED where m < n, the ten sums where it
// hit (its miss values where it did not), and (c, m) as two uint32 into the coverage buffer.  No division here — under
// policies 1 and 2 `/` is the 2.5-ulp expansion: pt_features_cameras_finish (rt_amd.hip) divides, for every policy alike.
template <bool ACCEL>
__global__ __launch_bounds__(256) void pt_features_cameras(DeviceScene sc, FrameParams fp, uint32_t follow, uint32_t max_chain,
                                                           uint32_t n, uint32_t glog2, float4 *__restrict__ out,
                                                           uint2 *__restrict__ cov) {
    __shared__ float4 s_mat[PT_LDS_STATIC_FLOAT4];
    Ctx c{sc, stage_materials(sc, s_mat), nullptr};
    c.lwin = staged_winners(sc, s_mat);
    c.lpln = staged_planes(sc, s_mat);
    const uint32_t g = 1u << glog2;
    const uint32_t pix = blockIdx.x * (256u >> glog2) + (threadIdx.x >> glog2), j = threadIdx.x & (g - 1u);
    const bool in_frame = pix < (uint32_t)fp.w * (uint32_t)fp.h;
    const float none = __uint_as_float(0xFFFFFFFFu);
    // the record of a lane without a sample: a miss that no vote counts and no sum sees
    float4 o0 = make_float4(0.0f, 0.0f, 0.0f, INFINITY), o1 = make_float4(0.0f, 0.0f, 0.0f, none);
    float4 o2 = make_float4(0.0f, 0.0f, 0.0f, none), o3 = make_float4(0.0f, 0.0f, 0.0f, none);
    float4 o4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (in_frame && j < n) {
        const uint32_t x = pix % (uint32_t)fp.w, y = pix / (uint32_t)fp.w;
        feature_chain<ACCEL>(c, primary_ray(fp.cams + 12u * j, x, y, fp.w, fp.h), follow, max_chain,
                             [&](const FeatureRec &f) { o0 = f.o0; o1 = f.o1; o2 = f.o2; o3 = f.o3; o4 = f.o4; });
    }
    // ---- the vote: lanes 0 .. n-1 of the group all hold a sample (or none does, past the frame: nothing is written then)
    const uint32_t flags = __float_as_uint(o4.w), key_o = __float_as_uint(o1.w), key_c = flags >> 8;
    const uint32_t lane0 = (threadIdx.x & 63u) & ~(g - 1u);
    uint32_t same = 0u;
    for (uint32_t s = 0u; s < n; s++)
        same += (__shfl(key_o, (int)(lane0 + s)) == key_o && __shfl(key_c, (int)(lane0 + s)) == key_c) ? 1u : 0u;
    uint32_t best = j < n ? (same << 6) | (63u - j) : 0u;
    const bool hit = (flags & RT_FEATURE_HIT) != 0u;
    uint32_t hits = hit ? 1u : 0u;
    float sum[10] = {hit ? o0.x : 0.0f, hit ? o0.y : 0.0f, hit ? o0.z : 0.0f, hit ? o0.w : 0.0f, hit ? o1.x : 0.0f,
                     hit ? o1.y : 0.0f, hit ? o1.z : 0.0f, hit ? o2.x : 0.0f, hit ? o2.y : 0.0f, hit ? o2.z : 0.0f};
    for (uint32_t off = g >> 1; off > 0u; off >>= 1) {
        best = max(best, (uint32_t)__shfl_xor(best, off));
        hits += __shfl_xor(hits, off);
#pragma unroll
        for (int k = 0; k < 10; k++) sum[k] += __shfl_xor(sum[k], off);
    }
    if (!in_frame || j != 63u - (best & 63u)) return;   // (past every cross-lane step)
    const uint32_t m = best >> 6;
    if (hit) {
        o0 = make_float4(sum[0], sum[1], sum[2], sum[3]);
        o1 = make_float4(sum[4], sum[5], sum[6], o1.w);
        o2 = make_float4(sum[7], sum[8], sum[9], o2.w);
    }
    o4.w = __uint_as_float(flags | (m < n ? RT_FEATURE_MIXED : 0u));
    float4 *o = out + 5 * (size_t)pix;
    o[0] = o0;
    o[1] = o1;
    o[2] = o2;
    o[3] = o3;
    o[4] = o4;
    cov[pix] = make_uint2(hits, m);
}

// ---- unit probes of the device routines (tests only; rt_debug_hit / rt_debug_material / rt_debug_div3) -----------
// One work-item per record; the routines are the very ones the trace kernels inline (hit_primitives' sphere_t /
// plane_t / lens_t, triangle_t, hit_scene + hit_finish, scatter), so a unit vector that matches the oracle here
// pins the arithmetic of the hot loop piece by piece (SURVEY §8c "unit vectors").  Record layouts are those of
// oracle/ref_shim.cpp ref_hit / ref_material.
PT_DEV void put_hit(float *o, bool hit, float t, const Hit &h) {
    for (int k = 0; k < 12; k++) o[k] = 0.0f;
    if (!hit) return;
    o[0] = 1.0f; o[1] = t;
    o[2] = h.p.x; o[3] = h.p.y; o[4] = h.p.z;
    o[5] = h.n.x; o[6] = h.n.y; o[7] = h.n.z;
    o[8] = h.u; o[9] = h.v;
    o[10] = __uint_as_float(h.tex);
    o[11] = __uint_as_float(h.mat);
}
template <bool ACCEL>
__global__ __launch_bounds__(256) void pt_debug_hit(DeviceScene sc, int kind, const float *__restrict__ rays,
                                                    const uint32_t *__restrict__ prim, const uint32_t *__restrict__ face,
                                                    uint32_t n, float *__restrict__ out) {
    __shared__ float4 s_mat[PT_LDS_STATIC_FLOAT4];
    Ctx c{sc, stage_materials(sc, s_mat), nullptr};
    c.lwin = staged_winners(sc, s_mat);
    c.lpln = staged_planes(sc, s_mat);
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.o = mk(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
    r.d = mk(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    Hit h;
    h.p = h.n = mk(0.0f, 0.0f, 0.0f);
    h.u = h.v = 0.0f;
    h.tex = h.mat = 0;
    Nearest nb;
    bool hit = false;
    if (kind == 3) {                      // hitScene :322-360
        hit = hit_scene<false, ACCEL>(c, r, h);
        if (hit) { hit_primitives<false, ACCEL>(c, r, nb); hit_models<false, ACCEL>(c, r, nb); }
    } else {
        // a single primitive through the SAME (t, id) search + winner rebuild the trace kernels use
        uint32_t p = prim[i];
        float t = PT_MISS;
        // (the sphere's test record as apply_arith makes it: w = r under policy 2, whose sphere_disc contracts the product, else r²)
        if (kind == 0) { const rt_sphere &sp = sc.spheres[p]; t = sphere_t(r, make_float4(sp.pos.x, sp.pos.y, sp.pos.z, PT_SPHERE_W_IS_RADIUS ? sp.r : sp.r * sp.r)); nb.id = K_SPHERE | p; }
        else if (kind == 1) { const rt_plane &pl = sc.planes[p]; t = plane_t(r, ld3(pl.pos), ld3(pl.normal)); nb.id = K_PLANE | p; }
        else if (kind == 2) { int which; t = lens_t(r, sc.lenses[p], &which); nb.id = K_LENS | p; }
        else if (kind == 4) {             // hitTriangle :257-289 on face face[i] of mesh p
            const float4 *fr = sc.faces + 3u * ((size_t)sc.mesh_face_base[p] + face[i]);
            float4 q0 = fr[0], q1 = fr[1];
            float4 q2 = fr[2];
            float u, v;
            t = triangle_t(r, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), mk(q1.z, q1.w, q2.x), &u, &v);
            nb.id = K_MESH | p; nb.face = face[i]; nb.u = u; nb.v = v; nb.mat = 0;
        }
        if (t < PT_MISS) {
            nb.t = t;
            hit = hit_finish<false>(c, r, nb, h);
            if (kind == 4) h.mat = h.tex = 0;  // hitTriangle sets neither mat_ID (hitModel does, :314) nor texture_ID (hitMeshOut, :299)
        }
    }
    put_hit(out + 12 * (size_t)i, hit, nb.t, h);
}

__global__ __launch_bounds__(256) void pt_debug_material(DeviceScene sc, int routine, const float *__restrict__ in,
                                                         uint32_t n, float *__restrict__ out) {
    __shared__ float4 s_mat[PT_LDS_STATIC_FLOAT4];
    Ctx c{sc, stage_materials(sc, s_mat), nullptr};
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float *v = in + 16 * (size_t)i;
    Ray r;
    r.o = mk(0.0f, 0.0f, 0.0f);
    r.d = mk(v[0], v[1], v[2]);
    Hit h;
    h.p = mk(v[3], v[4], v[5]);
    h.n = mk(v[6], v[7], v[8]);
    h.u = h.v = 0.0f;
    h.tex = 0;
    h.mat = __float_as_uint(v[12]);
    V3 out_col = mk(v[9], v[10], v[11]);
    uint32_t seed = __float_as_uint(v[13]), gx = __float_as_uint(v[14]), gy = __float_as_uint(v[15]);
    int type;
    float extra;
    V3 col;
    load_material(c, h.mat, type, extra, col);
    // the routine under test decides the branch of scatter(); the material supplies extra_data and — for
    // rayReflect's "*= extra only if t_reflective" (:366) — its own type
    int as_type = routine == 0 ? (type == RT_REFLECTIVE ? RT_REFLECTIVE : -1) : routine == 1 ? RT_REFRACTIVE
                  : routine == 2 ? RT_DIFFUSE : RT_DIELECTRIC;
    Rnd rnd = fetch_rnd(sc.table, r.d, seed, gx, gy);
    if (as_type == -1) {   // rayReflect on a material that is not t_reflective: the reflection tail of scatter()
        float k = 2.0f * dot(r.d, h.n);
        r.o = h.p;
        r.d = normalize(nmad(h.n, k, r.d));
    } else {
        scatter<false>(c, r, out_col, h, as_type, extra, mk(INFINITY, INFINITY, INFINITY), rnd);  // mixCol with +inf = identity
    }
    float *o = out + 9 * (size_t)i;
    o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z;
    o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z;
    o[6] = out_col.x; o[7] = out_col.y; o[8] = out_col.z;
}

// div3 (shared-reciprocal form of three IEEE divisions) against the compiler's divisions: in n × 4 {a.xyz, d} →
// out n × 6 {div3 result, a / d}; `force` = 1 runs the shared-reciprocal sequence even when PT_DIV3 is off
__global__ __launch_bounds__(256) void pt_debug_div3(const float *__restrict__ in, uint32_t n, float *__restrict__ out) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    V3 a = mk(in[4 * i], in[4 * i + 1], in[4 * i + 2]);
    float d = in[4 * i + 3];
    V3 q = a / d, s = q;
    if (div3_in_range(a, d)) {
        float nd = -d, rr = __builtin_amdgcn_rcpf(d);
        float e = __builtin_fmaf(nd, rr, 1.0f);
        rr = __builtin_fmaf(e, rr, rr);
        s = V3{div_shared(a.x, nd, rr), div_shared(a.y, nd, rr), div_shared(a.z, nd, rr)};
    }
    float *o = out + 6 * (size_t)i;
    o[0] = s.x; o[1] = s.y; o[2] = s.z; o[3] = q.x; o[4] = q.y; o[5] = q.z;
}

// queue_sums on its own (rt_debug_queue_sums): ONE wave fills the slot region of its queue from `in` (npix × count × 3
// floats, pixel-major), owns pixels (p, 0) of an npix × 1 frame, and runs the sample kernels' epilogue into `accum`
// (npix float4, zeroed by the caller).  The host checks npix <= QUEUE_MAX_PIXELS and npix × count <= QUEUE_SLOTS.
__global__ __launch_bounds__(64) void pt_debug_queue_sums(const float *__restrict__ in, uint32_t npix, uint32_t count,
                                                          uint32_t group_log2, float4 *__restrict__ accum) {
    __shared__ float4 s_q[QUEUE_MAX_PIXELS * QUEUE_XY_F4 + (QUEUE_SLOTS * 3u + 3u) / 4u];
    WaveQueue q;
    q.rec = nullptr;
    q.xy = (LdsQueueXY)s_q;
    q.slot = (LdsF32)(s_q + QUEUE_MAX_PIXELS * QUEUE_XY_F4);
    q.npix = npix;
    q.count = count;
    q.total = npix * count;
    q.count_log2 = 0xFFu;
    q.inv_count = 0.0f;
    const uint32_t lane = threadIdx.x;
    if (lane < npix) {
        q.xy[lane].x = lane;
        q.xy[lane].y = 0u;
    }
    for (uint32_t i = lane; i < 3u * q.total; i += 64u) q.slot[i] = in[i];
    FrameParams fp = {};
    fp.w = (int)npix;
    fp.h = 1;
    fp.count = count;
    fp.group_log2 = group_log2;
    queue_sums<false>(q, fp, accum);
}

// ================================== launchers ==================================
// All instantiations of a kernel template share a signature: a launch picks its instantiation from an explicit table (the
// tables together ARE the kernels of a policy's code object — an entry more is a kernel more) and goes through the pointer.
using RenderKernel = void (*)(DeviceScene, FrameParams, float4 *, float4 *, unsigned long long *);
static_assert(MODE_ACCUM == 0 && MODE_TRACE == 1 && MODE_RETRACE == 2, "render_kernel's table is indexed by the mode");
static RenderKernel render_kernel(int mode, bool count, bool accel) {   // [MODE][COUNT][ACCEL]
    static const RenderKernel k[3][2][2] = {
        {{pt_render<MODE_ACCUM, false, false>, pt_render<MODE_ACCUM, false, true>}, {pt_render<MODE_ACCUM, true, false>, pt_render<MODE_ACCUM, true, true>}},
        {{pt_render<MODE_TRACE, false, false>, pt_render<MODE_TRACE, false, true>}, {pt_render<MODE_TRACE, true, false>, pt_render<MODE_TRACE, true, true>}},
        {{pt_render<MODE_RETRACE, false, false>, pt_render<MODE_RETRACE, false, true>}, {pt_render<MODE_RETRACE, true, false>, pt_render<MODE_RETRACE, true, true>}}};
    return k[mode][count][accel];
}

// Very long launches are split into slot ranges (RT_OPT_MAX_THREADS_PER_LAUNCH; keeps single kernels short on huge scenes):
// the slots of a range, and where the range that begins at b ends (never b + per, which may pass 2^32).
static uint32_t slots_per_launch(const rt_context *ctx, uint32_t glog2) { return std::max(ctx->max_threads_per_launch >> glog2, 1u); }
static uint32_t range_end(uint32_t b, uint32_t slots, uint32_t per) { return slots - b > per ? b + per : slots; }

// The launch of a call without a first stage: the call's entry in the event history around body(), once per slot range with
// fp.slot_begin / fp.slot_end set.  A failure inside the loop returns its code and leaves the entry unused.
template <class Body>
static int launch_ranges(rt_context *ctx, FrameParams &fp, uint32_t slots, Body body) {
    const uint32_t per = slots_per_launch(ctx, fp.group_log2);
    hipEvent_t *evp = ctx->ev[ctx->ev_count % rt_context::EV_RING];
    HIP_TRY(ctx, hipEventRecord(evp[0], ctx->stream));
    HIP_TRY(ctx, hipEventRecord(evp[2], ctx->stream));   // no first stage
    for (uint32_t b = 0; b < slots; b = fp.slot_end) {
        fp.slot_begin = b;
        fp.slot_end = range_end(b, slots, per);
        const int rc = body();
        if (rc != RT_OK) return rc;
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(evp[1], ctx->stream));
    ctx->ev_count++;
    return RT_OK;
}

// Direct path (every sample from the camera): trace / retrace compat modes, and the fused mode when prefix sharing is switched off.
int launch_render(rt_context *ctx, int mode, const float cam[12], uint32_t first, uint32_t count, uint32_t glog2, float4 *accum,
                  const BlockMask *mask, float *m2) {
    if (mode < MODE_ACCUM || mode > MODE_RETRACE) return fail(ctx, RT_EINVAL, "unknown render mode %d", mode);
    CLEAR_TRY(ctx);
    FrameParams fp = frame_params(ctx, cam, first, count, glog2);
    apply_mask(fp, mask);
    fp.m2 = mode == MODE_ACCUM ? m2 : nullptr;
    const DeviceScene sc = device_scene(ctx);
    const uint32_t slots = fp.slot_end;
    if (slots == 0) return RT_OK;
    const RenderKernel kernel = render_kernel(mode, ctx->count_enabled, scene_has_accel(sc));
    return launch_ranges(ctx, fp, slots, [&]() -> int {
        const uint64_t threads = (uint64_t)(fp.slot_end - fp.slot_begin) << glog2;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, sc, fp, accum, ctx->image.p, ctx->counters.p);
        return RT_OK;
    });
}

// ---- sizing a wave's sample queue (host only; the layout functions and the queue: pt_queue.hpp, the launch constants:
// rt_context.hpp) ----------------------------------------------------------------------------------------------------
#ifndef QUEUE_MIN_SAMPLES
#define QUEUE_MIN_SAMPLES 384u
#endif
// Pixels per wave: as many as the LDS of a CU allows with PT_Q_WAVES(_ACCEL) one-wave workgroups resident per SIMD
// (6: 160 KB / 24 per workgroup); when that leaves a wave fewer than 384 samples (256 spp and up: the queue's tail
// grows) the budget of 5 per SIMD is used instead — the kernel's 80 VGPRs fit either way.
#ifndef PT_LDS_GRANULE
#define PT_LDS_GRANULE 1024u
#endif
__host__ inline uint32_t queue_pixels_per_wave(uint32_t count, uint32_t waves, uint32_t static_float4, uint32_t granule = PT_LDS_GRANULE) {
    auto fit = [&](uint32_t waves_per_simd) {
        uint32_t workgroups = waves_per_simd * 4u;  // resident workgroups per CU: one wave each
        // (LDS is handed out in blocks: a request of 6 584 bytes — 7 pixels of 64 samples — left fewer than 24 workgroups
        // resident although 24 × 6 584 < 160 KiB, and 6 pixels (5 728 bytes) are 4.5 % faster on C2; the budget is
        // therefore rounded DOWN to a multiple of the granule: PT_LDS_GRANULE, or the one rt_debug_queue_pixels asks about)
        uint32_t budget = 163840u / workgroups / granule * granule;
        uint32_t per_wave = budget - static_float4 * (uint32_t)sizeof(float4) - 15u;   // (15: queue_wave_lds_bytes rounds up)
        uint32_t p = per_wave / queue_pixel_bytes(count);
        if (p * count > QUEUE_SLOTS) p = QUEUE_SLOTS / count;
        return p > QUEUE_MAX_PIXELS ? (uint32_t)QUEUE_MAX_PIXELS : p;
    };
    uint32_t p = fit(waves);
    if (p * count < QUEUE_MIN_SAMPLES) {
        uint32_t p5 = fit(5u);
        if (p5 > p) p = p5;
    }
    return p < 1u ? 1u : p;
}
#ifndef PT_UNITS_PER_WAVE_SLOT
#define PT_UNITS_PER_WAVE_SLOT 16u   // waves a sample-kernel launch should have per wave slot of the chip (launch_fused)
#endif
#ifndef PT_TREE_MIN_SAMPLES
#define PT_TREE_MIN_SAMPLES 24u   // samples per call from which the shared decision trees pay (launch_fused; RT_OPT_PREFIX_TREE 1)
#endif
#ifndef PT_LDS_FACE_CAP
#define PT_LDS_FACE_CAP 64u   // faces (48 bytes each) of a scene of small meshes that may be staged in LDS (launch_fused)
#endif
#ifndef PT_Q_COUNT64
#define PT_Q_COUNT64 1       // pt_samples_q<…, COUNT_LOG2 = 6>: launches of exactly 64 samples per pixel with 64 lanes per pixel
                             // (one of the switches of a wave's fixed cost, pt_queue.hpp; plan_samples and queue_kernel read it)
#endif

// ---- the sample stage: facts (sample_facts, camera_facts: rt_context.hpp) → plan → launch -------------------------------
using SampleFacts = rt_sample_facts;
using SamplePlan = rt_sample_plan;
using CameraFacts = rt_camera_facts;
using CameraPlan = rt_camera_plan;

// THE sizing rule of the sample queue, for every way of feeding it (plan_samples, plan_camera_samples): the geometry row
// (accel, geom, waves) by the scene's BVHs and primitive kinds, the pixels a wave owns, and its LDS — the static prefix
// (static_f4: tables, then lds_face_f4 of faces), then the queue.  ppw_cap is what the wave-fill rule allows at most.
struct QueueSize {
    uint32_t accel, geom, waves, pixels_per_wave, ppw_cap, lds_face_f4, static_f4, lds_bytes;
};
template <class Facts>   // (the scene part of either facts, count, n, cu_count, wave_fill; stage_faces: the launch may keep faces in LDS)
static QueueSize queue_size(const Facts &f, bool stage_faces) {
    QueueSize q = {};
    const bool simple_geom = f.lens_count == 0 && f.model_count == 0;   // spheres and planes only
    const bool sphere_bvh_only = f.sphere_bvh && !f.mesh_bvh;
    q.accel = f.sphere_bvh || f.mesh_bvh;
    q.geom = !q.accel || sphere_bvh_only ? (simple_geom ? 0u : 1u) : 2u;
    q.waves = !q.accel ? PT_Q_WAVES : ((sphere_bvh_only && simple_geom) ? PT_Q_WAVES_SPHERE_BVH : PT_Q_WAVES_ACCEL);
    // a wave owns pixels_per_wave live pixels (<= QUEUE_SLOTS samples)
    q.static_f4 = lds_static_used(f.material_count, f.sphere_count, f.plane_count);
    // Small launches (small frames, a rank's share of a sharded frame): fewer pixels per wave, so that there are about
    // PT_UNITS_PER_WAVE_SLOT waves per wave slot of the chip — a wave works through its pixels' samples one batch of
    // 64 after the other, and 4 200 waves of 384 samples leave a third of the slots empty for the whole launch.
    // C2 at 64 spp, 6 pixels per wave vs this rule: 200 x 126 0.314 → 0.140 ms, 320 x 180 0.336 → 0.187, 480 x 270
    // 0.344 → 0.268, 640 x 360 0.419 → 0.369, 960 x 540 0.619 → 0.59; 1080p and up unchanged (6).
    const uint32_t want_units = (f.cu_count ? f.cu_count : 256u) * 4u * 6u * PT_UNITS_PER_WAVE_SLOT;
    const uint32_t ppw_full = (64u + f.count - 1u) / f.count;   // (never fewer than the 64 samples that fill a wave's lanes once)
    q.ppw_cap = !f.wave_fill ? QUEUE_MAX_PIXELS : std::max(f.n / want_units, ppw_full);
    q.pixels_per_wave = std::min(queue_pixels_per_wave(f.count, q.waves, q.static_f4), q.ppw_cap);
    // Face records in LDS for hit_models' candidate loop: scenes whose meshes are all face-scanned (no mesh BVH) and
    // hold at most PT_LDS_FACE_CAP faces together, and only when the copy fits into what the 1 KiB allocation granule
    // leaves over anyway (C3: 576 bytes of a cube into 609 spare ones) — never at the price of a pixel per wave.
    if (PT_FACE_MASK && stage_faces && !simple_geom && !f.mesh_bvh && f.faces > 0 && f.faces <= PT_LDS_FACE_CAP &&
        queue_pixels_per_wave(f.count, q.waves, q.static_f4 + 3u * f.faces) >= q.pixels_per_wave) {
        q.lds_face_f4 = 3u * f.faces;
        q.static_f4 += q.lds_face_f4;
    }
    q.lds_bytes = q.static_f4 * (uint32_t)sizeof(float4) + queue_wave_lds_bytes(q.pixels_per_wave, f.count);
    return q;
}

// plan_samples is THE place that decides which sample kernel a slot range of a fused call runs, with how many pixels per
// wave, how much LDS and how many workgroups: a pure function of the facts (no HIP call, no context), so the table can be
// pinned without a device (rt_debug_plan_samples, tests/test_sample_plan_host.py).  Its own, beside queue_size: the walk
// family's waves and pixels per wave, count_log2, the units of the live list and the exact grid.
static SamplePlan plan_samples(const SampleFacts &f) {
    SamplePlan p = {};
    const QueueSize q = queue_size(f, !f.count_enabled);
    const bool queue = f.sample_queue && f.count <= QUEUE_SLOTS;
    uint32_t ppw = q.pixels_per_wave;
    p.count = f.count_enabled;
    p.accel = q.accel;
    p.moments = f.moments;
    p.lds_face_f4 = q.lds_face_f4;   // (whatever the family: the facts decide it)
    p.block_size = 64u;
    if (queue && f.mesh_bvh && f.walk_jobs && f.walk_slices && !f.count_enabled) {   // every mesh has a BVH: walk slices, sized for their own occupancy
        p.family = RT_PLAN_WALK;
        p.multi = f.walk_jobs != 1u;
        p.waves = p.multi ? PT_W_WAVES_MULTI : PT_W_WAVES;
        ppw = std::min(queue_pixels_per_wave(f.count, p.waves, q.static_f4), q.ppw_cap);
        p.lds_bytes = q.static_f4 * (uint32_t)sizeof(float4) + queue_wave_lds_bytes(ppw, f.count);
    } else if (queue) {
        p.family = RT_PLAN_QUEUE;
        p.geom = q.geom;
        p.waves = q.waves;
        p.lds_bytes = q.lds_bytes;
        // (the count-specialised instantiation: exactly 64 samples on 64 lanes per pixel, no counters, no BVH, no moments)
        const bool count64 = PT_Q_COUNT64 && !p.accel && !p.count && !p.moments && f.count == 64u && f.glog2 == 6u;
        p.count_log2 = count64 ? 6u : RT_PLAN_GENERIC_COUNT;
    } else {
        p.family = RT_PLAN_FIXED;
        p.block_size = 256u;
        ppw = 1u;   // a unit of the live list is one pixel: 2^glog2 lanes
    }
    p.pixels_per_wave = ppw;
    // the units of the live list (its two parts each end in a partial chunk: one unit more than capacity / chunk) — unless the host knows
    // the list's counts: then exactly the units that own a pixel (rt_sample_units restates live_take), and no launch where there is none
    uint32_t units = (f.seg_cap + ppw - 1u) / ppw + 1u;
    if (f.exact) (void)rt_sample_units(f.seg_cap, ppw, f.count_light, f.count_heavy, &units);
    p.grid_units = p.family == RT_PLAN_FIXED ? (uint32_t)((((uint64_t)units << f.glog2) + 255u) / 256u) : units;
    return p;
}

// plan_camera_samples is THE place that decides what a slot range of a camera or ray launch runs (launch_source) — like
// plan_samples a pure function of its facts (rt_debug_plan_camera_samples, tests/test_cameras_host.py), sized by queue_size.
//  * RT_CAMERA_PLAN_QUEUE: the row's camera, ray or ray-set kernel, one wave per pixels_per_wave SLOTS — the grid is exact,
//    ceil(n / pixels_per_wave).  A scene plan_samples would give the walk-slice kernel runs the (1, 2) row, its walks in place.
//  * RT_CAMERA_PLAN_FIXED: pt_render<MODE_ACCUM, COUNT, ACCEL, true> (pt_render_rays, pt_render_raysets) — counting builds,
//    RT_OPT_SAMPLE_QUEUE 0, and launches that keep sample moments (a MOMENTS row of the camera queue would be five more
//    kernels for an option that is off by default; the fixed-lane kernel's moments are the ones rt_render_spp keeps with
//    prefix sharing off).
static CameraPlan plan_camera_samples(const CameraFacts &f) {
    CameraPlan p = {};
    p.count = f.count_enabled;
    p.accel = f.sphere_bvh || f.mesh_bvh;
    p.moments = f.moments;
    if (!f.sample_queue || f.count > QUEUE_SLOTS || f.count_enabled || f.moments) {   // no queue with counters or moments
        p.family = RT_CAMERA_PLAN_FIXED;
        p.pixels_per_wave = 1u;
        p.block_size = 256u;
        p.grid_units = (uint32_t)((((uint64_t)f.n << f.glog2) + 255u) / 256u);
        return p;
    }
    const QueueSize q = queue_size(f, true);
    p.family = RT_CAMERA_PLAN_QUEUE;
    p.geom = q.geom;
    p.waves = q.waves;
    p.pixels_per_wave = q.pixels_per_wave;
    p.lds_face_f4 = q.lds_face_f4;
    p.lds_bytes = q.lds_bytes;
    p.block_size = 64u;
    p.grid_units = (f.n + q.pixels_per_wave - 1u) / q.pixels_per_wave;
    return p;
}

using FixedKernel = void (*)(DeviceScene, FrameParams, const PixelRec *, const uint32_t *, const uint32_t *, float4 *, unsigned long long *);
static FixedKernel fixed_kernel(const SamplePlan &p) {   // [COUNT][ACCEL]
    static const FixedKernel k[2][2] = {{pt_samples<false, false>, pt_samples<false, true>}, {pt_samples<true, false>, pt_samples<true, true>}};
    return k[p.count != 0u][p.accel != 0u];
}
using QueueKernel = void (*)(DeviceScene, FrameParams, const PixelRec *, const uint32_t *, const uint32_t *, float4 *, unsigned long long *, uint32_t);
// The sample queue's five geometry rows: the key (accel, geom, waves) that queue_size yields, once, with every kernel of the
// row — fed from pt_prefix's records, from camera blocks (its look-ahead form: the rows without a BVH walk branch on
// fp.la_ring themselves, the ACCEL rows have pt_samples_q_la), from rays and from ray sets.  (Fed from feature records:
// pt_samples_q_hemi, the gather unit's — gather_kernels below.)
struct QueueRow {
    uint32_t accel, geom, waves;
    QueueKernel recs[2][2];   // [COUNT][MOMENTS]
    QueueKernel cams[2];      // [look-ahead]
    QueueKernel rays, ray_sets;
};
template <bool ACCEL, int GEOM, int WAVES>
static QueueRow queue_row() {
    const QueueKernel cam = pt_samples_q<false, ACCEL, GEOM, WAVES, false, -1, true>;
    QueueKernel cam_la = cam;
    if constexpr (ACCEL) cam_la = pt_samples_q_la<GEOM, WAVES>;   // (constexpr: naming it for the other rows would instantiate it)
    return {ACCEL, GEOM, WAVES,
            {{pt_samples_q<false, ACCEL, GEOM, WAVES, false>, pt_samples_q<false, ACCEL, GEOM, WAVES, true>},
             {pt_samples_q<true, ACCEL, GEOM, WAVES, false>, pt_samples_q<true, ACCEL, GEOM, WAVES, true>}},
            {cam, cam_la}, pt_samples_q_rays<ACCEL, GEOM, WAVES>, pt_samples_q_raysets<ACCEL, GEOM, WAVES>};
}
// The row of a plan — its kernels take any count, so a plan with another count_log2 has none — or NULL with RT_ESTATE recorded
// for the `family` that asked (neither planner asks for a row that is not there).
static const QueueRow *find_queue_row(rt_context *ctx, const char *family, uint32_t accel, uint32_t geom, uint32_t waves,
                                      uint32_t count_log2 = RT_PLAN_GENERIC_COUNT) {
#define PT_QUEUE_ROW(ACCEL, GEOM, WAVES) queue_row<ACCEL, GEOM, WAVES>(),
    static const QueueRow rows[] = {PT_QUEUE_ROWS(PT_QUEUE_ROW)};
#undef PT_QUEUE_ROW
    if (count_log2 == RT_PLAN_GENERIC_COUNT)
        for (const QueueRow &r : rows)
            if (r.accel == accel && r.geom == geom && r.waves == waves) return &r;
    (void)fail(ctx, RT_ESTATE, "no %s instantiation of pt_samples_q for the plan (accel %u, geom %u, %u waves)", family, accel, geom, waves);
    return nullptr;
}
// the record-fed kernel of a queue plan; the two COUNT_LOG2 = 6 kernels stand beside the table
static QueueKernel queue_kernel(rt_context *ctx, const SamplePlan &p) {
#if PT_Q_COUNT64
    static const QueueKernel k64[2] = {pt_samples_q<false, false, 0, PT_Q_WAVES, false, 6>, pt_samples_q<false, false, 1, PT_Q_WAVES, false, 6>};   // [GEOM]
    if (p.count_log2 == 6u && !p.count && !p.accel && !p.moments && p.geom < 2u && p.waves == PT_Q_WAVES) return k64[p.geom];
#endif
    const QueueRow *r = find_queue_row(ctx, "record", p.accel, p.geom, p.waves, p.count_log2);
    return r ? r->recs[p.count != 0u][p.moments != 0u] : nullptr;
}
#ifdef PT_WSTAT   // (the diagnostic build's kernels take their statistics block as one argument more)
using WalkKernel = void (*)(DeviceScene, FrameParams, const PixelRec *, const uint32_t *, const uint32_t *, float4 *, uint32_t, const uint2 *, uint32_t, unsigned long long *);
#else
using WalkKernel = void (*)(DeviceScene, FrameParams, const PixelRec *, const uint32_t *, const uint32_t *, float4 *, uint32_t, const uint2 *, uint32_t);
#endif
static WalkKernel walk_kernel(const SamplePlan &p) {   // [MULTI][MOMENTS]
    static const WalkKernel k[2][2] = {{pt_samples_w<false, false>, pt_samples_w<false, true>}, {pt_samples_w<true, false>, pt_samples_w<true, true>}};
    return k[p.multi != 0u][p.moments != 0u];
}

// the sample kernel over the live list, as planned; an empty grid launches nothing
static int launch_plan(rt_context *ctx, const SamplePlan &p, const DeviceScene &sc, const FrameParams &fp, float4 *accum, uint32_t *live_count) {
    if (p.grid_units == 0u) return RT_OK;
    const rt_context::Slots &ss = ctx->slots;
    const dim3 grid(p.grid_units), block(p.block_size);
    if (p.family == RT_PLAN_WALK) {
#ifdef PT_WSTAT
        hipLaunchKernelGGL(walk_kernel(p), grid, block, p.lds_bytes, ctx->stream, sc, fp, ss.recs.p, ss.live.p, live_count, accum,
                           p.pixels_per_wave, ctx->walk_jobs.p, (uint32_t)ctx->walk_jobs.n, ctx->counters.p + COUNTER_REPLICAS * COUNTER_STRIDE + 8);
#else
        hipLaunchKernelGGL(walk_kernel(p), grid, block, p.lds_bytes, ctx->stream, sc, fp, ss.recs.p, ss.live.p, live_count, accum,
                           p.pixels_per_wave, ctx->walk_jobs.p, (uint32_t)ctx->walk_jobs.n);
#endif
    } else if (p.family == RT_PLAN_QUEUE) {
        const QueueKernel kernel = queue_kernel(ctx, p);
        if (!kernel) return RT_ESTATE;
        hipLaunchKernelGGL(kernel, grid, block, p.lds_bytes, ctx->stream, sc, fp, ss.recs.p, ss.live.p, live_count, accum,
                           ctx->counters.p, p.pixels_per_wave);
    } else hipLaunchKernelGGL(fixed_kernel(p), grid, block, 0, ctx->stream, sc, fp, ss.recs.p, ss.live.p, live_count, accum, ctx->counters.p);
    return RT_OK;
}

// ---- the fused path's first stage and what is kept of it ----------------------------------------------------------------
using PrefixKernel = void (*)(DeviceScene, FrameParams, PixelRec *, uint32_t *, uint32_t *, float4 *, unsigned long long *, FinalPix *, uint32_t *);
static PrefixKernel prefix_kernel(bool count, bool accel, bool trees) {
    static const PrefixKernel plain[2][2] = {{pt_prefix<false, false>, pt_prefix<false, true>}, {pt_prefix<true, false>, pt_prefix<true, true>}};   // [COUNT][ACCEL]
    static const PrefixKernel tree[2] = {pt_prefix<false, false, true>, pt_prefix<false, true, true>};   // [ACCEL] (never in counting builds)
    return trees ? tree[accel] : plain[count][accel];
}
// A miss traces the prefix.  A hit adds the finished pixels' sums for this call's samples (everything else pt_prefix wrote lies
// there still); a look-ahead launch replays the finished pixels into the ring instead, after a traced prefix and a kept one alike.
static void launch_first_stage(rt_context *ctx, const DeviceScene &sc, const FrameParams &fp, bool hit, bool lookahead, float4 *accum, uint32_t *live_count) {
    const rt_context::Slots &ss = ctx->slots;
    const dim3 grid(fp.seg_cap / 256u), block(256);
    if (!hit)
        hipLaunchKernelGGL(prefix_kernel(ctx->count_enabled, scene_has_accel(sc), fp.tree_cap != 0u), grid, block, 0, ctx->stream, sc, fp,
                           ss.recs.p, ss.live.p, live_count, accum, ctx->counters.p, ss.finals.p, ss.final_n.p);
    else if (!lookahead)
        hipLaunchKernelGGL(pt_final_replay, grid, block, 0, ctx->stream, fp, ss.finals.p, ss.final_n.p, accum);
    if (lookahead) hipLaunchKernelGGL(pt_final_retrace, grid, block, 0, ctx->stream, fp, ss.finals.p, ss.final_n.p);
}

// what a look-ahead launch needs: the sample queue, an unsharded frame in one slot range, no counters, no accumulator
static bool lookahead_ok(const rt_context *ctx, const FrameParams &fp, const float4 *accum, const BlockMask *mask, const float *m2) {
    return !accum && !m2 && !mask && !ctx->count_enabled && ctx->world == 1 && ctx->sample_queue && fp.count <= QUEUE_SLOTS &&
           (ctx->max_threads_per_launch >> fp.group_log2) >= fp.slot_end;
}

// the staged scene block, for the sample kernels that copy it: (re)built when anything it holds may have changed
static void refresh_stage_block(rt_context *ctx, const DeviceScene &sc) {
    if (!PT_STAGE_COPY || ctx->stage_block.generation == ctx->prefix_cache.generation) return;
    if (lds_static_used(sc.material_count, sc.sphere_count, sc.plane_count))
        hipLaunchKernelGGL(pt_stage_block, dim3(1), dim3(64), 0, ctx->stream, sc,
                           reinterpret_cast<float4 *>(reinterpret_cast<char *>(ctx->materials.p) + stage_block_offset(sc.material_count)));
    ctx->stage_block.generation = ctx->prefix_cache.generation;
    ctx->stage_block.builds++;
}

// May this slot range of a fused launch STORE its sums (FrameParams::store)?  A clear is pending, the target is the context's
// accumulator, and after the two stages every pixel of the frame has been written exactly once by a kernel with the store arm:
//  * one slot range over an unsharded, unmasked frame: the slots 0 .. slot_end are the pixels of every tile, slot_to_pixel
//    refuses exactly those beyond the frame's edge (and those of seg_cap's rounded-up tail, >= slot_end), so each pixel of
//    the frame is `valid` in exactly one work-item of pt_prefix;
//  * pt_prefix makes a valid pixel either finished — it writes the pixel's sum itself and lists it, and on a prefix-cache
//    hit pt_final_replay writes the listed pixels — or live, appended once to the live list (a pixel with a decision tree
//    is a live pixel whose record says so);
//  * the queue family hands every live-list entry to exactly one wave (live_take; the exact grid launches the units that
//    own one), and queue_sums_tree writes each of the wave's npix pixels once.  An empty grid means no live pixel;
//  * no moments (moments_update reads the accumulator), no counters (the counting kernels keep the add), no BVH walk (their
//    kernels keep the butterfly and the add), no look-ahead (no accumulator), and the COUNT_LOG2 = 6 kernel — 64 samples on
//    64 lanes per pixel: the generic-count kernels keep the add too.
// (in two steps: what the call itself says, known before anything is enqueued, and what the range's plan says)
static bool accum_store_may_qualify(const rt_context *ctx, const FrameParams &fp, const float4 *accum, const BlockMask *mask,
                                    const float4 *ring, const float *m2, bool one_range) {
    return PT_ACCUM_STORE && ctx->accum_store && ctx->clear_pending && accum && accum == ctx->accum.p && !ring && !mask && !m2 &&
           one_range && fp.world == 1u && !ctx->count_enabled && fp.count == 64u && fp.group_log2 == 6u;
}
static bool accum_store_qualifies(const rt_context *ctx, const FrameParams &fp, const SamplePlan &plan, const float4 *accum,
                                  const BlockMask *mask, const float4 *ring, const float *m2, bool one_range) {
    return accum_store_may_qualify(ctx, fp, accum, mask, ring, m2, one_range) && plan.family == RT_PLAN_QUEUE && !plan.accel &&
           !plan.count && !plan.moments && plan.geom < 2u && plan.count_log2 == 6u && plan.waves == PT_Q_WAVES;   // (queue_kernel's k64 test)
}

// Fused path: pt_prefix (one work-item per pixel) + the planned sample kernel (g lanes per live pixel).  While camera and
// scene rest the first stage is pt_final_replay over what the last pt_prefix left (rt_context::PrefixCache).
// ring != NULL: a LOOK-AHEAD launch (rt_render_again, RT_OPT_LOOKAHEAD) — the same two stages over the same slot buffers and
// the same prefix-cache entry, but the `count` samples become `count` frames of the ring (queue_replay, pt_final_retrace)
// and the accumulator is not touched (accum is NULL).
static int launch_fused_any(rt_context *ctx, const float cam[12], uint32_t first, uint32_t count, uint32_t glog2, float4 *accum,
                            const BlockMask *mask, float4 *ring, float *m2) {
    FrameParams fp = frame_params(ctx, cam, first, count, glog2);
    apply_mask(fp, mask);
    fp.m2 = m2;   // (NULL for a look-ahead launch: the compat path keeps no moments)
    if (ring) {
        if (!lookahead_ok(ctx, fp, accum, mask, m2))
            return fail(ctx, RT_EINVAL, "a look-ahead launch needs the sample queue, an unsharded frame in one slot range and no counters");
        fp.la_ring = ring;
        fp.la_image = ctx->image.p;
    }
    const DeviceScene sc = device_scene(ctx);
    const uint32_t slots = fp.slot_end;
    if (slots == 0) return RT_OK;
    int rc = ensure_slots(ctx, slots);
    if (rc) return rc;
    refresh_stage_block(ctx, sc);
    const rt_context::Slots &ss = ctx->slots;
    uint32_t *live_count = ss.live.p + ss.capacity + 256u;
    const uint32_t per = slots_per_launch(ctx, glog2);
    // may this launch's pt_prefix be kept, and is the last one's still good?
    const bool tree_on = ctx->prefix_tree == 2 || (ctx->prefix_tree == 1 && count >= PT_TREE_MIN_SAMPLES);
    const bool keepable = !mask && !ctx->count_enabled && per >= slots;
    uint32_t cam_bits[12];
    memcpy(cam_bits, cam, sizeof cam_bits);
    const bool hit = prefix_lookup(ctx->prefix_cache, keepable, tree_on, cam_bits);   // (a hit is one slot range)
    bool exact = false;
    if ((rc = learn_live_counts(ctx, hit, live_count, &exact)) != RT_OK) return rc;
    rt_context::SampleGrid &sg = ctx->sample_grid;
    // (a pending clear that this call cannot store over is enqueued here, in front of the call's first event as rt_clear's
    // memset always was: the call's entry in the event history keeps timing the kernels alone)
    if (!accum_store_may_qualify(ctx, fp, accum, mask, ring, m2, per >= slots) && (rc = materialise_clear(ctx)) != RT_OK) return rc;
    hipEvent_t *evp = ctx->ev[ctx->ev_count % rt_context::EV_RING];
    HIP_TRY(ctx, hipEventRecord(evp[0], ctx->stream));
    for (uint32_t b = 0; b < slots; b = fp.slot_end) {
        fp.slot_begin = b;
        fp.slot_end = range_end(b, slots, per);
        if (!hit) HIP_TRY(ctx, hipMemsetAsync(live_count, 0, LIVE_COUNT_STRIDE * sizeof(uint32_t), ctx->stream));
        // shared decision trees (RT_OPT_PREFIX_TREE): not in counting builds — the counters price per-sample work
        fp.trees = ss.trees.p;
        fp.tree_wait = ss.tree_wait.p;
        fp.tree_count = live_count + LIVE_TREE_COUNTER;
        // (and not for a handful of samples per call: tracing both continuations of a pixel costs more than the few samples
        // that would share them — C2 at 1 / 8 / 16 / 32 samples per call: 0.321 / 0.457 / 0.609 / 1.031 ms with trees,
        // 0.243 / 0.393 / 0.582 / 1.088 without)
        fp.tree_cap = (tree_on && !ctx->count_enabled) ? (uint32_t)ss.tree_capacity : 0u;   // (0 without the tree buffers)
        // the live list holds whole workgroups of pt_prefix; worst case all n pixels are live
        fp.seg_cap = (fp.slot_end - fp.slot_begin + 255u) / 256u * 256u;
        const SampleFacts facts = sample_facts(ctx, sc, fp, exact);
        const SamplePlan plan = plan_samples(facts);
        fp.lds_face_f4 = plan.lds_face_f4;
        // A cleared frame is stored, not added to (rt_context::clear_pending): this launch qualifies when its two stages write
        // every pixel of the frame exactly once with kernels that have the store arm — see accum_store_qualifies.  The first
        // launch of a call only: it ends the pending state, the later ones add.
        const bool store = accum_store_qualifies(ctx, fp, plan, accum, mask, ring, m2, per >= slots);
        if (store) fp.store = 1u;
        else if ((rc = materialise_clear(ctx)) != RT_OK) return rc;
        launch_first_stage(ctx, sc, fp, hit, ring != nullptr, accum, live_count);
        HIP_TRY(ctx, hipEventRecord(evp[2], ctx->stream));  // (the last slot range's; one range is the normal case)
        if ((rc = launch_plan(ctx, plan, sc, fp, accum, live_count)) != RT_OK) return rc;
        // (the frame now holds this launch's sums.  Had the sample kernel not been launched, the clear would still be pending and
        // the memset that ends it would wipe what the first stage stored: a failed call leaves a cleared frame)
        if (store) ctx->clear_pending = false, ctx->clears_stored++;
        fp.store = 0u;
        sg.last_facts = facts, sg.last_plan = plan;
        sg.launches++;
        sg.workgroups += plan.grid_units;   // (what rt_sample_grid_stats reports)
        if (plan.grid_units && plan.family == RT_PLAN_QUEUE && plan.count_log2 == 6u) sg.count64_launches++;
        if (exact) { sg.exact_launches++; sg.live_last = plan.grid_units; }
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(evp[1], ctx->stream));
    ctx->ev_count++;
    if (hit) ctx->prefix_cache.hits++; else ctx->prefix_cache.misses++;   // (launches that went through)
    if (keepable) prefix_keep(ctx->prefix_cache, tree_on, cam_bits);
    return RT_OK;
}

int launch_fused(rt_context *ctx, const float cam[12], uint32_t first, uint32_t count, uint32_t glog2, float4 *accum, const BlockMask *mask, float *m2) {
    return launch_fused_any(ctx, cam, first, count, glog2, accum, mask, nullptr, m2);
}

int launch_lookahead(rt_context *ctx, const float cam[12], uint32_t first, uint32_t count, float4 *ring) {
    if (!ring || count < 1u) return fail(ctx, RT_EINVAL, "look-ahead launch without a ring");
    return launch_fused_any(ctx, cam, first, count, group_log2_for(count), nullptr, nullptr, ring, nullptr);
}

// ---- samples from a source of their own: per-sample camera blocks, caller-supplied rays, ray sets ---------------------------
// facts (camera_facts, rt_context.hpp: n = the slots of the range) → plan_camera_samples → the row's kernel for the source,
// or the source's fixed-lane kernel.
static RenderKernel camera_render_kernel(bool count, bool accel) {   // [COUNT][ACCEL]
    static const RenderKernel k[2][2] = {{pt_render<MODE_ACCUM, false, false, true>, pt_render<MODE_ACCUM, false, true, true>},
                                         {pt_render<MODE_ACCUM, true, false, true>, pt_render<MODE_ACCUM, true, true, true>}};
    return k[count][accel];
}
typedef void (*RayRenderKernel)(DeviceScene, FrameParams, float4 *, unsigned long long *);
static RayRenderKernel ray_render_kernel(bool count, bool accel, bool sets) {   // [COUNT][ACCEL]
    static const RayRenderKernel k[2][2] = {{pt_render_rays<false, false>, pt_render_rays<false, true>},
                                            {pt_render_rays<true, false>, pt_render_rays<true, true>}};
    static const RayRenderKernel k_sets[2][2] = {{pt_render_raysets<false, false>, pt_render_raysets<false, true>},
                                                 {pt_render_raysets<true, false>, pt_render_raysets<true, true>}};
    return sets ? k_sets[count][accel] : k[count][accel];
}
// the kernels of rt_render_hemispheres: this policy's gather unit has them (pt_gather.hip)
static const pt::GatherKernels &gather_kernels() { return *pt::PT_GATHER_KERNELS(); }

// What feeds a launch of launch_source, on the device.  Cameras: `count` blocks of 12 floats at p, sample first + j through
// block j, over the owned pixels of the (sharded) frame; cam0 is the first block.  Rays: n rt_ray records at p (set_size 0) or
// n sets of set_size records, ray-major, slot = ray index; cam0 is zero but for the set size and its reciprocal in its first
// two words (queue_stage_raysets).  Hemispheres (`hemi`, a ray source): n rt_feature records at p, the sets of set_size
// rays made from them; cam0 holds the HEMI_CAM_* words too.  cam0 fills FrameParams::cam, which no camera kernel reads.
struct SampleSource {
    bool rays, hemi;
    const void *p;
    size_t n;
    uint32_t set_size;
    const float *cam0;
};

// One launch of a camera or ray call: samples first .. first+count-1 of every slot, the sums added to `accum` (and `m2`) at
// the pixel (cameras) or at the ray's index.  Nothing here reads or writes the slot buffers or the prefix cache; the staged
// scene block is the context's, refreshed as launch_fused refreshes it.  The facts and the plan of the last slot range go to
// rt_context::Cameras / Rays.
// mask != NULL (the adaptive calls): only the slots of active decision blocks are staged and traced — the kernels test
// pixel_active / ray_active where they take ownership of a slot, a ray launch then has one ray per pixel of the frame, ray i
// being pixel (i mod W, i div W); the plan and the grid are those of the unmasked launch.
// ring != NULL, cameras only: a LOOK-AHEAD launch (rt_render_again_cameras, RT_OPT_LOOKAHEAD) — the queue family only, accum,
// mask and m2 NULL: the `count` samples become `count` frames of the ring (queue_replay<true>), whose frame 0 holds the image as
// it lies (the caller copied it there on the stream), and the accumulator is not touched.  The facts carry moments = 0.
static int launch_source(rt_context *ctx, const SampleSource &src, uint32_t first, uint32_t count, uint32_t glog2, float4 *accum,
                         const BlockMask *mask, float *m2, float4 *ring) {
    const bool sets = src.set_size != 0u && !src.hemi;
    if (!src.rays) {
        if (!src.p || count < 1u || count > RT_SPP_PER_LAUNCH) return fail(ctx, RT_EINVAL, "a camera launch takes 1 .. %u blocks", RT_SPP_PER_LAUNCH);
    } else {
        if (!src.p || !accum || src.n < 1u || src.n > (1u << 28) || count < 1u || count > RT_SPP_PER_LAUNCH)
            return fail(ctx, RT_EINVAL, "a ray launch takes 1 .. 2^28 rays and 1 .. %u samples", RT_SPP_PER_LAUNCH);
        if (src.set_size > RT_RAY_SET_MAX || (uint64_t)src.n * src.set_size > (1ull << 31))
            return fail(ctx, RT_EINVAL, "a ray-set launch takes sets of 1 .. %u records, 2^31 records in all", RT_RAY_SET_MAX);
        if (mask && src.n != (size_t)ctx->width * ctx->height)   // (ray_active reads the block of pixel i: i must be one)
            return fail(ctx, RT_EINVAL, "a masked ray launch takes one ray per pixel of the %d x %d frame", ctx->width, ctx->height);
    }
    CLEAR_TRY(ctx);   // (these launches add, and a look-ahead launch starts from the image)
    FrameParams fp = src.rays ? frame_params(ctx, src.cam0, first, count, glog2, 0, 1)   // (unsharded: slot = ray index)
                              : frame_params(ctx, src.cam0, first, count, glog2);
    apply_mask(fp, mask);
    fp.m2 = m2;
    if (src.rays) fp.rays = reinterpret_cast<const float4 *>(src.p);   // (a hemisphere source: fp.feats, the same bytes)
    else fp.cams = reinterpret_cast<const float *>(src.p);
    const DeviceScene sc = device_scene(ctx);
    if (ring) {
        if (src.rays || !lookahead_ok(ctx, fp, accum, mask, m2) || plan_camera_samples(camera_facts(ctx, sc, fp)).family != RT_CAMERA_PLAN_QUEUE)
            return fail(ctx, RT_EINVAL, "a look-ahead launch needs the sample queue, an unsharded frame in one slot range and no counters");
        fp.la_ring = ring;   // (la_image's bytes hold `cams`: the start image is the ring's frame 0)
    }
    const uint32_t slots = src.rays ? (uint32_t)src.n : fp.slot_end;
    if (slots == 0) return RT_OK;
    refresh_stage_block(ctx, sc);
    return launch_ranges(ctx, fp, slots, [&]() -> int {
        const CameraFacts facts = camera_facts(ctx, sc, fp);
        const CameraPlan plan = plan_camera_samples(facts);
        const dim3 grid(plan.grid_units), block(plan.block_size);
        fp.lds_face_f4 = plan.lds_face_f4;
        if (plan.family == RT_CAMERA_PLAN_QUEUE) {
            const QueueRow *r = find_queue_row(ctx, src.rays ? "ray" : "camera", plan.accel, plan.geom, plan.waves);
            if (!r) return RT_ESTATE;
            const QueueKernel kernel = !src.rays ? r->cams[ring != nullptr] : src.hemi ? gather_kernels().queue(plan.accel, plan.geom, plan.waves)
                                       : sets ? r->ray_sets : r->rays;
            if (!kernel) return fail(ctx, RT_ESTATE, "no pt_samples_q_hemi for the plan (accel %u, geom %u, %u waves)", plan.accel, plan.geom, plan.waves);
            hipLaunchKernelGGL(kernel, grid, block, plan.lds_bytes, ctx->stream,
                               sc, fp, (const PixelRec *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr, accum,
                               ctx->counters.p, plan.pixels_per_wave);
        } else if (src.rays) {
            hipLaunchKernelGGL(src.hemi ? gather_kernels().fixed(plan.count != 0u, plan.accel != 0u) : ray_render_kernel(plan.count != 0u, plan.accel != 0u, sets),
                               grid, block, 0, ctx->stream, sc, fp, accum, ctx->counters.p);
        } else {
            hipLaunchKernelGGL(camera_render_kernel(plan.count != 0u, plan.accel != 0u), grid, block, 0, ctx->stream, sc, fp, accum,
                               ctx->image.p, ctx->counters.p);
        }
        if (src.rays) ctx->rays.last_facts = facts, ctx->rays.last_plan = plan;
        else ctx->cameras.last_facts = facts, ctx->cameras.last_plan = plan;
        return RT_OK;
    });
}

// rt_render_spp_cameras, rt_render_adaptive_cameras, rt_render_again_cameras: `count` blocks at d_cams, cam0 the first of them
int launch_cameras(rt_context *ctx, const float *d_cams, const float cam0[12], uint32_t first, uint32_t count, uint32_t glog2,
                   float4 *accum, const BlockMask *mask, float *m2, float4 *ring) {
    return launch_source(ctx, {false, false, d_cams, 0u, 0u, cam0}, first, count, glog2, accum, mask, m2, ring);
}
// rt_render_rays (set_size 0: one record per ray), rt_render_ray_sets (1 .. RT_RAY_SET_MAX) and their adaptive forms
int launch_rays(rt_context *ctx, const void *d_rays, size_t n, uint32_t set_size, uint32_t first, uint32_t count, uint32_t glog2,
                float4 *accum, const BlockMask *mask, float *m2) {
    float cam0[12] = {};
    if (set_size) {
        memcpy(&cam0[0], &set_size, sizeof(uint32_t));
        cam0[1] = 1.0f / (float)set_size;
    }
    return launch_source(ctx, {true, false, d_rays, n, set_size, cam0}, first, count, glog2, accum, mask, m2, nullptr);
}
// rt_render_hemispheres: the p.k hemisphere rays of each of the n feature records as the record's ray set, never stored
int launch_hemispheres(rt_context *ctx, const rt_feature *d_features, size_t n, const rt_hemisphere_params &p, uint32_t first,
                       uint32_t count, uint32_t glog2, float4 *accum, float *m2) {
    if (p.k < 1u) return fail(ctx, RT_EINVAL, "a hemisphere launch takes sets of 1 .. %u rays", RT_RAY_SET_MAX);
    const uint32_t words[6] = {p.k, 0u, (uint32_t)p.seed, (uint32_t)(p.seed >> 32), 0u, p.flags};
    float cam0[12] = {};
    memcpy(cam0, words, sizeof words);
    cam0[1] = 1.0f / (float)p.k;
    cam0[HEMI_CAM_OFFSET] = p.offset;
    return launch_source(ctx, {true, true, d_features, n, p.k, cam0}, first, count, glog2, accum, nullptr, m2, nullptr);
}

// ---- policy-dependent precomputation and probes ---------------------------------------------------------------
// hitTriangle's unit normal, normalize(cross(edge1, edge2)) (raytracer.cl:285), depends on the face only: it is kept
// in the face records (A, e1, e2, n).  Policy 0 computes it on the host (rt_amd.hip build_face_records: plain IEEE
// operations); the ROCm-OpenCL policies need the library's cross and its v_rsq_f32-based normalize, which only
// the device can evaluate — one work-item per record, the same two calls the reference makes per test.
__global__ __launch_bounds__(256) void pt_face_normals(float4 *__restrict__ rec, uint32_t n) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float4 q0 = rec[3 * (size_t)i], q1 = rec[3 * (size_t)i + 1], q2 = rec[3 * (size_t)i + 2];
    V3 e1 = mk(q0.w, q1.x, q1.y), e2 = mk(q1.z, q1.w, q2.x);
    V3 nn = normalize(cross(e1, e2));
    rec[3 * (size_t)i + 2] = make_float4(q2.x, nn.x, nn.y, nn.z);
}

// One builtin of this policy per record (tests/test_gpu_ref950.py compares policies 1 / 2 with probe kernels that call
// ROCm's OpenCL builtins themselves, oracle/ref_gfx950_wrap.cl): in n × 8 floats, out n × 4 floats.
__global__ __launch_bounds__(256) void pt_debug_builtin(int op, const float *__restrict__ in, uint32_t n, float *__restrict__ out) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float *a = in + 8 * (size_t)i;
    V3 x = mk(a[0], a[1], a[2]), y = mk(a[3], a[4], a[5]);
    float t = a[6];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (op == 0) o.x = dot(x, y);
    else if (op == 1) { V3 c = cross(x, y); o = make_float4(c.x, c.y, c.z, 0.0f); }
    else if (op == 2) { V3 c = normalize(x); o = make_float4(c.x, c.y, c.z, 0.0f); }
    else if (op == 3) { o.x = a[0] / a[1]; o.y = 1.0f / a[0]; V3 c = x / t; o.z = c.y; o.w = c.z; }
    else if (op == 4) o.x = sqrt1(a[0]);
    else if (op == 5) o = make_float4(mix1(x.x, y.x, t), mix1(x.y, y.y, t), mix1(x.z, y.z, t), 0.0f);
    else if (op == 6) { V3 c = vmin(x, y); o = make_float4(c.x, c.y, c.z, 0.0f); }
    else if (op == 7) o.x = sign1(a[0]);
    else if (op == 8) o.x = pow5(a[0]);
    else if (op == 9) o.x = __uint_as_float(dir_hash(x));
    // the tagged forms of pt_arith.hpp as the sample queue runs them (the wave decides: 64 consecutive records)
    else if (op == 10) o.x = sqrt1<true>(a[0]);
    else if (op == 11) { V3 c = normalize<true>(x); o = make_float4(c.x, c.y, c.z, 0.0f); }
    else if (op == 12) { V3 c = vmin<true>(x, y); o = make_float4(c.x, c.y, c.z, 0.0f); }   // mixCol's min, tagged (op 6: untagged)
    reinterpret_cast<float4 *>(out)[i] = o;
}

namespace {

// The launch of every kernel that takes one lane per item: a flat grid of 256-thread workgroups on the context's stream.
template <class Kernel, class... Args>
int launch_flat(rt_context *ctx, Kernel kernel, size_t items, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((uint32_t)((items + 255u) / 256u)), dim3(256), 0, ctx->stream, args...);
    HIP_TRY(ctx, hipGetLastError());
    return RT_OK;
}

int ks_launch_probe(rt_context *ctx, const FrameParams &fp, const DeviceScene &sc, const uint32_t *d_in, uint32_t n, float *d_out) {
    return launch_flat(ctx, scene_has_accel(sc) ? pt_probe<true> : pt_probe<false>, n, sc, fp, d_in, d_in + n, d_in + 2 * (size_t)n, n, d_out);
}

// rt_render_features: pt_features, one record per pixel
// (the ACCEL choice of launch_fused: the BVH walks are compiled in when the scene has a BVH)
int ks_launch_features(rt_context *ctx, const FrameParams &fp, const DeviceScene &sc, rt_feature *d_out) {
    return launch_flat(ctx, scene_has_accel(sc) ? pt_features<true> : pt_features<false>, (size_t)fp.w * (size_t)fp.h, sc, fp,
                       reinterpret_cast<float4 *>(d_out));
}

// rt_render_features_chain: pt_features_chain, one record per pixel
int ks_launch_features_chain(rt_context *ctx, const FrameParams &fp, const DeviceScene &sc, uint32_t follow, uint32_t max_chain,
                             rt_feature *d_out) {
    return launch_flat(ctx, scene_has_accel(sc) ? pt_features_chain<true> : pt_features_chain<false>, (size_t)fp.w * (size_t)fp.h, sc, fp,
                       follow, max_chain, reinterpret_cast<float4 *>(d_out));
}

// rt_debug_plan_feature_cameras: one lane per sample, g = 2^ceil(log2 n) lanes per pixel, whole pixels per 256-thread
// workgroup (at most 2^28 pixels of 4 .. 256 to a workgroup: the grid fits 32 bits)
FeatureCamerasPlan ks_plan_feature_cameras(uint32_t pixels, uint32_t n) {
    FeatureCamerasPlan p;
    p.glog2 = 0u;
    while ((1u << p.glog2) < n) p.glog2++;
    const uint32_t per_wg = 256u >> p.glog2;
    p.workgroups = (pixels + per_wg - 1u) / per_wg;
    p.block_size = 256u;
    return p;
}

// rt_render_features_cameras: pt_features_cameras on ks_plan_feature_cameras' grid
int ks_launch_features_cameras(rt_context *ctx, FrameParams fp, const DeviceScene &sc, const float *d_cams, uint32_t n,
                               uint32_t follow, uint32_t max_chain, rt_feature *d_out, uint2 *d_cov) {
    if (!d_cams || n < 1u || n > RT_FEATURE_CAMERAS_MAX) return fail(ctx, RT_EINVAL, "a feature launch takes 1 .. %u camera blocks", RT_FEATURE_CAMERAS_MAX);
    fp.cams = d_cams;   // (the union with la_image: la_ring is NULL, nothing reads la_image)
    const FeatureCamerasPlan plan = ks_plan_feature_cameras((uint32_t)fp.w * (uint32_t)fp.h, n);
    float4 *o = reinterpret_cast<float4 *>(d_out);
    hipLaunchKernelGGL(scene_has_accel(sc) ? pt_features_cameras<true> : pt_features_cameras<false>, dim3(plan.workgroups),
                       dim3(plan.block_size), 0, ctx->stream, sc, fp, follow, max_chain, n, plan.glog2, o, d_cov);
    HIP_TRY(ctx, hipGetLastError());
    return RT_OK;
}

// rt_render_features_rays, rt_intersect_rays: pt_features_rays, one record per ray into d_out
int ks_launch_features_rays(rt_context *ctx, const DeviceScene &sc, const void *d_rays, uint32_t n, uint32_t follow, uint32_t max_chain,
                            rt_feature *d_out) {
    if (!d_rays || n < 1u) return fail(ctx, RT_EINVAL, "a feature launch over rays needs a ray buffer");
    return launch_flat(ctx, scene_has_accel(sc) ? pt_features_rays<true> : pt_features_rays<false>, n, sc,
                       reinterpret_cast<const float4 *>(d_rays), n, follow, max_chain, reinterpret_cast<float4 *>(d_out));
}

// rt_occluded_rays: pt_occluded over n sets of set_size records; the counts of sets of more than one record are summed
// into d_out by atomics, so it is zeroed on the stream first
int ks_launch_occluded(rt_context *ctx, const DeviceScene &sc, const void *d_rays, size_t n, uint32_t set_size, const float *d_tmax,
                       float t_max, uint32_t *d_out) {
    const size_t records = n * set_size;
    if (!d_rays || !d_out || n < 1u || set_size < 1u || records > ((size_t)1 << 31))
        return fail(ctx, RT_EINVAL, "an occlusion launch needs rays, an output and at most 2^31 records");
    if (set_size > 1u) HIP_TRY(ctx, hipMemsetAsync(d_out, 0, n * sizeof(uint32_t), ctx->stream));
    return launch_flat(ctx, scene_has_accel(sc) ? pt_occluded<true> : pt_occluded<false>, records, sc,
                       reinterpret_cast<const float4 *>(d_rays), d_tmax, t_max, (uint32_t)records, set_size, d_out);
}

// rt_occluded_hemispheres: pt_occluded_hemi over n feature records x p.k rays.  d_counts (zeroed on the stream first where
// atomics sum into it) and d_rays_out may each be NULL, not both; without d_counts no search runs
int ks_launch_occluded_hemi(rt_context *ctx, const DeviceScene &sc, const rt_feature *d_features, size_t n, const rt_hemisphere_params &p,
                            uint32_t *d_counts, void *d_rays_out) {
    const size_t records = n * p.k;
    if (!d_features || (!d_counts && !d_rays_out) || n < 1u || p.k < 1u || records > ((size_t)1 << 31))
        return fail(ctx, RT_EINVAL, "a hemisphere launch needs records, an output and at most 2^31 rays");
    if (d_counts && p.k > 1u) HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, n * sizeof(uint32_t), ctx->stream));
    const bool accel = d_counts && scene_has_accel(sc);
    auto kernel = d_rays_out ? (accel ? pt_occluded_hemi<true, true> : pt_occluded_hemi<false, true>)
                             : (accel ? pt_occluded_hemi<true, false> : pt_occluded_hemi<false, false>);
    return launch_flat(ctx, kernel, records, sc, reinterpret_cast<const float4 *>(d_features), (uint32_t)p.seed, (uint32_t)(p.seed >> 32),
                       p.flags, p.offset, p.t_max, (uint32_t)records, p.k, d_counts, static_cast<float4 *>(d_rays_out));
}

int ks_launch_debug_hit(rt_context *ctx, const DeviceScene &sc, int kind, const float *d_rays, const uint32_t *d_prim,
                        const uint32_t *d_face, uint32_t n, float *d_out) {
    return launch_flat(ctx, scene_has_accel(sc) ? pt_debug_hit<true> : pt_debug_hit<false>, n, sc, kind, d_rays, d_prim, d_face, n, d_out);
}

int ks_launch_debug_material(rt_context *ctx, const DeviceScene &sc, int routine, const float *d_in, uint32_t n, float *d_out) {
    return launch_flat(ctx, pt_debug_material, n, sc, routine, d_in, n, d_out);
}

int ks_launch_debug_div3(rt_context *ctx, const float *d_in, uint32_t n, float *d_out) {
    return launch_flat(ctx, pt_debug_div3, n, d_in, n, d_out);
}

int ks_launch_debug_queue_sums(rt_context *ctx, const float *d_in, uint32_t npix, uint32_t count, uint32_t glog2, float *d_out) {
    if (npix < 1u || npix > QUEUE_MAX_PIXELS || count < 1u || npix * count > QUEUE_SLOTS || glog2 > 6u)
        return fail(ctx, RT_EINVAL, "queue_sums probe: %u pixels of %u samples do not fit one wave's queue", npix, count);
    HIP_TRY(ctx, hipMemsetAsync(d_out, 0, npix * sizeof(float4), ctx->stream));
    hipLaunchKernelGGL(pt_debug_queue_sums, dim3(1), dim3(64), 0, ctx->stream, d_in, npix, count, glog2, (float4 *)d_out);
    HIP_TRY(ctx, hipGetLastError());
    return RT_OK;
}

int ks_launch_face_normals(rt_context *ctx, float4 *d_records, uint32_t n_records) {
    if (n_records == 0) return RT_OK;
    return launch_flat(ctx, pt_face_normals, n_records, d_records, n_records);
}

int ks_launch_debug_builtin(rt_context *ctx, int op, const float *d_in, uint32_t n, float *d_out) {
    return launch_flat(ctx, pt_debug_builtin, n, op, d_in, n, d_out);
}

// rt_debug_queue_pixels: queue_pixels_per_wave as the launcher calls it, under a granule of the caller's choice (0: PT_LDS_GRANULE)
uint32_t ks_queue_pixels(uint32_t count, uint32_t waves, uint32_t static_float4, uint32_t granule) {
    return queue_pixels_per_wave(count, waves, static_float4, granule ? granule : PT_LDS_GRANULE);
}

// rt_debug_queue_occupancy: what the runtime says about the headline instantiation at a dynamic LDS size — no kernel runs
int ks_queue_occupancy(rt_context *ctx, uint32_t lds_bytes, int *blocks) {
    HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, pt_samples_q<false, false, 0, PT_Q_WAVES, false, -1>, 64, lds_bytes));
    return RT_OK;
}

const pt::KernelSet g_kernel_set = {
    PT_ARITH,
#if PT_ARITH == 0
    "ieee",
#elif PT_ARITH == 1
    "rocm-opencl-nocontract",
#else
    "rocm-opencl",
#endif
    launch_render, launch_fused, launch_lookahead, ks_launch_probe, ks_launch_features, ks_launch_debug_hit, ks_launch_debug_material, ks_launch_debug_div3,
    ks_launch_face_normals, ks_launch_debug_builtin, ks_launch_debug_queue_sums, ks_launch_features_chain,
    ks_queue_pixels, ks_queue_occupancy, plan_samples, launch_cameras, plan_camera_samples, ks_launch_features_cameras,
    ks_plan_feature_cameras, launch_rays, ks_launch_features_rays, ks_launch_occluded, ks_launch_occluded_hemi, launch_hemispheres};

}  // namespace

}  // namespace PT_NS

namespace pt {
const KernelSet *PT_KERNEL_SET() { return &PT_NS::g_kernel_set; }
}  // namespace pt
