// pt_sample.hpp — what a sample kernel does around its sample loop, whatever feeds it: its share of the live list, the lane
// counters, the summation tree of a pixel's lanes, the accumulator update (added or stored), the sample moments, one step
// of the look-ahead chain, and where a ray-set or hemisphere launch finds sample s's ray.  Templates and PT_DEV inline
// functions only, inside the policy's namespace: pt_kernels.hip and pt_gather.hip both include it, and a kernel of either
// unit is made of the same text.  The switches defined here (#ifndef X / #define X default) reach both units.
#pragma once
#include "pt_device.hpp"
#include "pt_moments.hpp"

namespace PT_NS {

// wave (or pixel group) `unit` of a sample kernel → its first entry in the live list and how many of `want` exist.
// The list has two parts (pt_prefix): the HEAVY pixels, stored from the end of the capacity downwards, and the others,
// stored from 0 upwards in the order in which pt_prefix's workgroups finish.  The heavy ones are taken FIRST (longest
// processing time first — see pt_prefix), then the rest in list order.
// Safe by construction, whatever the grid: the counts are clamped to the list's capacity, a unit's start is formed
// in 64 bits and clamped INTO its part (start <= count), so `count - start` cannot wrap and `first + result` never
// leaves the part — a unit beyond the list gets 0 entries.  (Round 2's form `start < cnt ? min(want, cnt - start) : 0`
// is the same function, but an experiment that inlined it into a persistent loop faulted and the cause was never
// established beyond "the guard was optimised away"; this form has no guard to lose.  tests/test_gpu_properties.py
// ::test_live_list_far_shorter_than_the_grid renders an all-sky frame and a frame with ONE live pixel.)
PT_DEV uint32_t live_take(const FrameParams &fp, const uint32_t *__restrict__ live_count, uint32_t unit, uint32_t want,
                          uint32_t &first) {
    const uint32_t cap = fp.seg_cap;
    const uint32_t cnt_l = min(live_count[0], cap);
    const uint32_t cnt_h = min(live_count[LIVE_HEAVY_COUNTER], cap - cnt_l);
    const uint32_t units_h = want ? (cnt_h + want - 1u) / want : 0u;
    const bool heavy = unit < units_h;
    const uint32_t cnt = heavy ? cnt_h : cnt_l;
    const unsigned long long start64 = (unsigned long long)(heavy ? unit : unit - units_h) * want;
    const uint32_t start = (uint32_t)min(start64, (unsigned long long)cnt);
    first = (heavy ? cap - cnt_h : 0u) + start;
    return min(want, cnt - start);
}

template <bool COUNT>
PT_DEV void flush_counters(const LaneCounters &cn, unsigned long long *counters, uint32_t scale) {
    if (!COUNT) return;
    unsigned long long *row = counters + (size_t)(blockIdx.x % COUNTER_REPLICAS) * COUNTER_STRIDE;
#pragma unroll
    for (int i = 0; i < PT_N_COUNTERS; i++) {
        uint32_t v = cn.c[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&row[i], (unsigned long long)v * scale);
    }
}

PT_DEV void zero_counters(LaneCounters &cn) {
#pragma unroll
    for (int i = 0; i < PT_N_COUNTERS; i++) cn.c[i] = 0;
}

// how many set bits of a wave mask belong to lanes below this one (v_mbcnt: no per-lane mask to keep in registers)
PT_DEV uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// xor-butterfly over the g lanes of a pixel group: a fixed summation tree
PT_DEV V3 group_sum(V3 sum, uint32_t g) {
    for (uint32_t off = g >> 1; off > 0; off >>= 1) {
        sum.x += __shfl_xor(sum.x, off);
        sum.y += __shfl_xor(sum.y, off);
        sum.z += __shfl_xor(sum.z, off);
    }
    return sum;
}

PT_DEV void accumulate(float4 *__restrict__ accum, size_t pix, V3 sum, uint32_t count) {
    float4 a = accum[pix];
    a.x += sum.x;
    a.y += sum.y;
    a.z += sum.z;
    a.w += (float)count;
    accum[pix] = a;
}
// A cleared frame is stored, not added to (FrameParams::store; DESIGN §5 "A cleared frame is stored"): the words accumulate
// leaves in a pixel that holds zeros — the same operands in the same order, 0.0f + sum, so every word keeps its bits, a sum
// of -0.0f included — without the load and without the wait for it.  The kernels that take it test fp.store wave-uniformly
// (accumulate_any); everything else keeps accumulate.  PT_ACCUM_STORE 0: no kernel reads the field.
#ifndef PT_ACCUM_STORE
#define PT_ACCUM_STORE 1
#endif
PT_DEV void accumulate_store(float4 *__restrict__ accum, size_t pix, V3 sum, uint32_t count) {
    accum[pix] = make_float4(0.0f + sum.x, 0.0f + sum.y, 0.0f + sum.z, 0.0f + (float)count);
}
PT_DEV void accumulate_any(const FrameParams &fp, float4 *__restrict__ accum, size_t pix, V3 sum, uint32_t count) {
    if (PT_ACCUM_STORE && fp.store) accumulate_store(accum, pix, sum, count);
    else accumulate(accum, pix, sum, count);
}

// ---- per-pixel sample moments (FrameParams::m2, RT_OPT_MOMENTS; pt_moments.hpp) --------------------------------------
// A launch that adds `count` samples of sum `sum` to a pixel merges their centred second moment m2B — about the launch's
// own mean l(sum) / count — with the state the pixel holds BEFORE the launch's accumulate: (accum.w, accum.rgb, m2).
// Called by the one lane that then accumulates, in the kernels' epilogues only.
PT_DEV void moments_update(const float4 *accum, float *m2, size_t pix, V3 sum, uint32_t count, float m2B) {
    const float4 a = accum[pix];
    m2[pix] = moments_merge(a.w, a.x, a.y, a.z, m2[pix], (float)count, sum.x, sum.y, sum.z, m2B);
}

// The fixed-lane kernels (pt_render<MODE_ACCUM>, pt_samples): a lane keeps (n, its partial sum, M2) over its own samples,
// folding each one in as a one-sample state BEFORE it joins the sum; the butterfly then merges the lanes' states pairwise
// while it adds their sums exactly as group_sum does (same operands, same order: the sum keeps its bits).
struct LaneMoments {
    float n, m2;
};
PT_DEV void moments_fold(LaneMoments &lm, V3 sum, V3 s) {
    lm.m2 = moments_merge(lm.n, sum.x, sum.y, sum.z, lm.m2, 1.0f, s.x, s.y, s.z, 0.0f);
    lm.n += 1.0f;
}
PT_DEV V3 group_sum_moments(V3 sum, LaneMoments &lm, uint32_t g) {
    for (uint32_t off = g >> 1; off > 0; off >>= 1) {
        const V3 o = mk(__shfl_xor(sum.x, off), __shfl_xor(sum.y, off), __shfl_xor(sum.z, off));
        const float on = __shfl_xor(lm.n, off), om2 = __shfl_xor(lm.m2, off);
        lm.m2 = moments_merge(lm.n, sum.x, sum.y, sum.z, lm.m2, on, o.x, o.y, o.z, om2);
        lm.n += on;
        sum.x += o.x;
        sum.y += o.y;
        sum.z += o.z;
    }
    return sum;
}

// ONE step of the interactive loop's running mean, kept in gamma space (`retrace`, raytracer.cl:524-528): the image after
// sample s from the image after sample s - 1 and the radiance of sample s — mix(new, prev², s/(s+1)), then gamma_corr.
// The ONE place that forms it: pt_render<MODE_RETRACE> and the look-ahead replays (queue_replay, pt_final_retrace) all
// call it with the policy's `/`, mix1 and sqrt1, so a look-ahead frame has the direct kernel's bits.  `sample` is the
// SUM of a one-sample group, 0.0f + radiance (a radiance of -0 becomes +0 there): every caller forms that sum first.
PT_DEV float retrace_step1(float prev, float sample, uint32_t s) {
    const float lin = prev * prev;
    const float k = (float)s / (float)(s + 1u);
    return sqrt1(mix1(sample, lin, k));   // mix(new, prev², k/(k+1)) :526
}
PT_DEV V3 retrace_step(V3 prev, V3 sample, uint32_t s) {
    return mk(retrace_step1(prev.x, sample.x, s), retrace_step1(prev.y, sample.y, s), retrace_step1(prev.z, sample.z, s));
}

// Where frame j of pixel pix lies in the look-ahead ring (in float4).  Shipped: FRAME-MAJOR, frame after frame, so that a frame
// is handed out as one contiguous device copy.  -DPT_RING_PIXEL_MAJOR=1 builds the A/B variant that keeps a pixel's `count`
// frames side by side (whole-line stores here, a strided hand-out kernel in rt_amd.hip): profiles/r08_experiments.md.
PT_DEV size_t ring_at(const FrameParams &fp, size_t pix, uint32_t j) {
    return PT_RING_PIXEL_MAJOR ? pix * fp.count + j : j * ((size_t)fp.w * fp.h) + pix;
}

// s mod set_size for s <= RT_MAX_SAMPLE and set_size <= RT_RAY_SET_MAX without an integer division: the quotient is
// floor((s + 0.5) · (1 / set_size)) in float — s + 0.5 is exact, the true quotient (s + 0.5) / set_size stands at least
// 0.5 / set_size from every integer, and the two roundings move the product by less than 2^-22 · 2^16 / set_size =
// 0.016 / set_size.  (tests/test_ray_sets_host.py walks the whole domain.)
PT_DEV uint32_t ray_set_member(const FrameParams &fp, uint32_t sample) {
    const uint32_t set_size = __float_as_uint(fp.cam[0]);
    return sample - (uint32_t)(((float)sample + 0.5f) * fp.cam[1]) * set_size;
}
// the two float4 of record `member` of ray `index`'s set; the record index stays below 2^31 and is formed in 64 bits
PT_DEV const float4 *ray_set_record(const FrameParams &fp, uint32_t index, uint32_t member) {
    return fp.rays + 2u * ((size_t)index * __float_as_uint(fp.cam[0]) + member);
}

// Hemisphere gathers (rt_render_hemispheres): a ray-set launch whose sets are MADE — slot i is feature record i of fp.feats,
// sample s starts at hemisphere ray s mod k of the record (Philox counter i · k + s mod k, random stream (i, 0)): the rays
// rt_occluded_hemispheres' spawn form writes, never written.  What the spawn kernel takes as arguments travels in fp.cam
// beside the set size and its reciprocal (ray_set_member reads those two as it does for a ray-set launch):
#define HEMI_CAM_KEY0 2     // the Philox key: the seed's low and high word
#define HEMI_CAM_KEY1 3
#define HEMI_CAM_OFFSET 4   // rt_hemisphere_params::offset
#define HEMI_CAM_FLAGS 5    // rt_hemisphere_params::flags
PT_DEV void hemi_frame_of(const FrameParams &fp, uint32_t index, HemiFrame &fr) {   // (of a record that has a hemisphere)
    hemisphere_frame(fp.feats + 5u * (size_t)index, (__float_as_uint(fp.cam[HEMI_CAM_FLAGS]) & RT_HEMI_FACE_FORWARD) != 0u,
                     fp.cam[HEMI_CAM_OFFSET], fr);
}
// (The key is opaque to the optimiser and waits for the counter: the generator's twenty round keys are launch constants, and
// lifted out of the sample loop they took twenty scalar registers of kernels that have none to spare — they went to VGPR
// lanes, and the (ACCEL, GEOM 2) row spilled one vector register more than its ray-set twin.  DESIGN.md §5 "Hemisphere gather")
PT_DEV V3 hemi_point_of(const FrameParams &fp, uint32_t index, uint32_t sample) {
    uint32_t counter = index * __float_as_uint(fp.cam[0]) + ray_set_member(fp, sample);   // (< 2^31)
    uint32_t k0 = __float_as_uint(fp.cam[HEMI_CAM_KEY0]), k1 = __float_as_uint(fp.cam[HEMI_CAM_KEY1]);
    asm("" : "+s"(k0), "+s"(k1), "+v"(counter));
    return hemisphere_point(counter, k0, k1);
}

}  // namespace PT_NS
