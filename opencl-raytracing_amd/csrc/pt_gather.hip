// pt_gather.hip — the kernels of rt_render_hemispheres (pt_samples_q_hemi, pt_render_hemi), a translation unit of their own
// per arithmetic policy: compiled with pt_kernels.hip's flags, once per policy, and linked beside it.  They are made of the
// device code the other sample kernels are made of — what a sample kernel does around its loop (pt_sample.hpp), the wave's
// queue with its hemisphere entry and its sums (pt_queue.hpp), the queue kernel's text (pt_samples_q_kernel.hpp) — and this
// unit includes those headers as pt_kernels.hip does.  What is the gather's alone is here: the fixed-lane kernel, the fifth
// form of the queue kernel, and the table that instantiates the nine kernels (pt::GatherKernels, pt_kernels.hpp), through
// which launch_hemispheres (pt_kernels.hip) reaches them.  So the policy's own code object holds the kernels it held before
// the gather existed, and tools/isa_stats.py --unit pt_gather lists these.
#include <hip/hip_runtime.h>

#include "pt_device.hpp"
#include "rt_context.hpp"
#include "pt_kernels.hpp"
#include "pt_sample.hpp"
#include "pt_queue.hpp"

namespace PT_NS {
using namespace rtamd;

// Fixed lanes (counters on, RT_OPT_SAMPLE_QUEUE 0 or sample moments): render_rays_fixed (pt_kernels.hip) with the ray made inside the sample
// loop from a frame formed ahead of it.  A record without a hemisphere is an unowned slot: no sample, no sum, no counter.
template <bool COUNT, bool ACCEL>
__global__ __launch_bounds__(256) void pt_render_hemi(DeviceScene sc, FrameParams fp, float4 *__restrict__ accum,
                                                      unsigned long long *counters) {
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
    const bool valid = index < fp.slot_end && hemisphere_valid(fp.feats + 5u * (size_t)index);

    V3 sum = mk(0.0f, 0.0f, 0.0f);
    const bool mom = fp.m2 != nullptr;   // (uniform)
    LaneMoments lm{0.0f, 0.0f};
    if (valid) {
        HemiFrame fr;
        hemi_frame_of(fp, index, fr);
        for (uint32_t s = fp.first + lane; s < fp.first + fp.count; s += g) {
            if (COUNT) cn.c[CN_SAMPLES]++;
            Ray r0;
            r0.o = fr.o;
            r0.d = hemisphere_dir(fr, hemi_point_of(fp, index, s));
            const V3 rad = radiance<COUNT, ACCEL>(c, r0, s, index, 0u);
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

// The queue kernel's text (pt_samples_q_kernel.hpp; pt_kernels.hip includes its forms 0 – 3) a fifth time, as
// pt_samples_q_hemi<ACCEL, GEOM, WAVES>: the ray-set form with the sets made from feature records (rt_render_hemispheres;
// queue_stage_hemi, pt_queue.hpp).
#define PT_Q_LOOKAHEAD_FORM 4
#include "pt_samples_q_kernel.hpp"
#undef PT_Q_LOOKAHEAD_FORM

// ---- the unit's table: the kernels of rt_render_hemispheres and nothing else ----------------------------------------------
namespace {
pt::GatherKernels::Queue gather_queue_kernel(uint32_t accel, uint32_t geom, uint32_t waves) {
    struct Row { uint32_t accel, geom, waves; pt::GatherKernels::Queue kernel; };
#define PT_GATHER_ROW(ACCEL, GEOM, WAVES) {ACCEL, GEOM, WAVES, pt_samples_q_hemi<ACCEL, GEOM, WAVES>},
    static const Row rows[] = {PT_QUEUE_ROWS(PT_GATHER_ROW)};
#undef PT_GATHER_ROW
    for (const Row &r : rows)
        if (r.accel == accel && r.geom == geom && r.waves == waves) return r.kernel;
    return nullptr;
}
pt::GatherKernels::Fixed gather_fixed_kernel(bool count, bool accel) {   // [COUNT][ACCEL]
    static const pt::GatherKernels::Fixed k[2][2] = {{pt_render_hemi<false, false>, pt_render_hemi<false, true>},
                                                 {pt_render_hemi<true, false>, pt_render_hemi<true, true>}};
    return k[count][accel];
}
const pt::GatherKernels g_gather_kernels = {gather_queue_kernel, gather_fixed_kernel};
}  // namespace

}  // namespace PT_NS

namespace pt {
const GatherKernels *PT_GATHER_KERNELS() { return &PT_NS::g_gather_kernels; }
}  // namespace pt
