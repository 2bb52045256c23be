// pt_kernels.hpp — what one arithmetic policy's translation unit (pt_kernels.hip, -DPT_ARITH=k) exports to the host
// side of librt_amd.so: the launchers of its kernels.  All launches go to ctx->stream; every function returns an RT_*
// code and records its message on the context.
#pragma once
#include "rt_context.hpp"

namespace pt {

// the launch of pt_features_cameras (rt_debug_plan_feature_cameras' three words)
struct FeatureCamerasPlan {
    uint32_t glog2, workgroups, block_size;
};

struct KernelSet {
    int arith;             // RT_ARITH_* this set was compiled for
    const char *name;
    // direct path: MODE_ACCUM / MODE_TRACE / MODE_RETRACE (rt_render, rt_render_again, prefix sharing off)
    // `accum`: the accumulator MODE_ACCUM adds to; `mask`: the pixels traced (NULL = every owned pixel); `m2`: the sample
    // moments kept beside `accum` (MODE_ACCUM only; NULL = none, FrameParams::m2)
    int (*launch_render)(rt_context *ctx, int mode, const float cam[12], uint32_t first, uint32_t count, uint32_t glog2,
                         float4 *accum, const BlockMask *mask, float *m2);
    // fused path: pt_prefix + the sample kernel plan_samples chooses (pt_samples_q / pt_samples_w / pt_samples), adding to
    // `accum` (and updating `m2`, as above)
    int (*launch_fused)(rt_context *ctx, const float cam[12], uint32_t first, uint32_t count, uint32_t glog2,
                        float4 *accum, const BlockMask *mask, float *m2);
    // look-ahead (rt_render_again, RT_OPT_LOOKAHEAD): the fused launch for samples first .. first+count-1, but instead of
    // sums into the accumulator the image after each of them — `count` frames of W x H float4, frame-major, into `ring`,
    // starting from the context's image as it lies.  Same slot buffers and prefix-cache entry as launch_fused.
    int (*launch_lookahead)(rt_context *ctx, const float cam[12], uint32_t first, uint32_t count, float4 *ring);
    // rt_trace_samples: d_in = n x, n y, n sample (uint32), d_out = 3 n floats
    int (*launch_probe)(rt_context *ctx, const FrameParams &fp, const DeviceScene &sc, const uint32_t *d_in, uint32_t n, float *d_out);
    // rt_render_features: pt_features (feature_chain with no follow bits), one rt_feature per pixel of the fp.w x fp.h frame
    // into d_out
    int (*launch_features)(rt_context *ctx, const FrameParams &fp, const DeviceScene &sc, rt_feature *d_out);
    // unit probes (rt_debug_hit / rt_debug_material / rt_debug_div3)
    int (*launch_debug_hit)(rt_context *ctx, const DeviceScene &sc, int kind, const float *d_rays, const uint32_t *d_prim,
                            const uint32_t *d_face, uint32_t n, float *d_out);
    int (*launch_debug_material)(rt_context *ctx, const DeviceScene &sc, int routine, const float *d_in, uint32_t n, float *d_out);
    int (*launch_debug_div3)(rt_context *ctx, const float *d_in, uint32_t n, float *d_out);
    // per-face unit normals normalize(cross(e1, e2)) (raytracer.cl:285) with THIS policy's builtins, written into the
    // (A, e1, e2, n) records: n_records records of 3 float4 each
    int (*launch_face_normals)(rt_context *ctx, float4 *d_records, uint32_t n_records);
    // one builtin per record, for tests against oracle/_ref/gfx950's probe kernels: op 0 dot, 1 cross, 2 normalize,
    // 3 a/b, 4 sqrt, 5 mix, 6 min, 7 sign, 8 pow(x,5), 9 the table hash, 10 / 11 / 12 sqrt / normalize / min in their tagged
    // forms;
    // in: n × 8 floats, out: n × 4 floats
    int (*launch_debug_builtin)(rt_context *ctx, int op, const float *d_in, uint32_t n, float *d_out);
    // rt_debug_queue_sums: one wave's queue_sums over npix × count × 3 slot floats into npix float4 (zeroed here)
    int (*launch_debug_queue_sums)(rt_context *ctx, const float *d_in, uint32_t npix, uint32_t count, uint32_t glog2, float *d_out);
    // rt_render_features_chain: pt_features_chain, the record at the end of every pixel's mirror / glass chain (`follow`:
    // RT_FOLLOW_* bits, at most max_chain <= RT_FEATURE_CHAIN_MAX followed vertices) into d_out
    int (*launch_features_chain)(rt_context *ctx, const FrameParams &fp, const DeviceScene &sc, uint32_t follow, uint32_t max_chain,
                                 rt_feature *d_out);
    // rt_debug_queue_pixels: the launcher's queue_pixels_per_wave under an LDS allocation granule (0: the shipped one)
    uint32_t (*queue_pixels)(uint32_t count, uint32_t waves, uint32_t static_float4, uint32_t granule);
    // rt_debug_queue_occupancy: hipOccupancyMaxActiveBlocksPerMultiprocessor of pt_samples_q<false, false, 0, PT_Q_WAVES> at a dynamic LDS size
    int (*queue_occupancy)(rt_context *ctx, uint32_t lds_bytes, int *blocks);
    // rt_debug_plan_samples: the fused launcher's choice of sample kernel and launch geometry — a pure function, no device
    rt_sample_plan (*plan_samples)(const rt_sample_facts &facts);
    // rt_render_spp_cameras: samples first .. first+count-1 (count <= RT_SPP_PER_LAUNCH) of every owned pixel, sample first + j
    // through block j of d_cams (count x 12 floats on the device), summed in launch_fused's order and added to `accum`
    // (updating `m2`): the from-the-camera sample queue, or pt_render<MODE_ACCUM, …, CAMS> where plan_camera_samples says so;
    // mask != NULL (rt_render_adaptive_cameras): the pixels of active decision blocks only, as launch_fused / launch_render;
    // ring != NULL (rt_render_again_cameras): a look-ahead launch — accum, mask and m2 NULL, the queue family only, the image
    // after sample first + j into frame j of `ring`, whose frame 0 holds the start image when the launch begins
    int (*launch_cameras)(rt_context *ctx, const float *d_cams, const float cam0[12], uint32_t first, uint32_t count, uint32_t glog2,
                          float4 *accum, const BlockMask *mask, float *m2, float4 *ring);
    // rt_debug_plan_camera_samples: that launcher's choice of kernel and launch geometry — a pure function, no device
    rt_camera_plan (*plan_camera_samples)(const rt_camera_facts &facts);
    // rt_render_features_cameras: pt_features_cameras, the records of n <= RT_FEATURE_CAMERAS_MAX blocks of d_cams (n x 12
    // floats on the device) per pixel reduced to one record per pixel in d_out — the ten float sums undivided — and the
    // counts (hit samples, dominant group) as two uint32 per pixel in d_cov; pt_features_cameras_finish (rt_amd.hip) divides
    int (*launch_features_cameras)(rt_context *ctx, FrameParams fp, const DeviceScene &sc, const float *d_cams, uint32_t n,
                                   uint32_t follow, uint32_t max_chain, rt_feature *d_out, uint2 *d_cov);
    // rt_debug_plan_feature_cameras: that launcher's geometry for a frame of `pixels` pixels — a pure function, no device
    FeatureCamerasPlan (*plan_feature_cameras)(uint32_t pixels, uint32_t n);
    // rt_render_rays, rt_render_ray_sets: samples first .. first+count-1 (count <= RT_SPP_PER_LAUNCH) of the n <= 2^28 rays at
    // d_rays (rt_ray records on the device), ray i's sum added to accum[i] (updating m2[i]; NULL = no moments).  set_size 0:
    // one record per ray — the sample queue's ray entry, or pt_render_rays where plan_camera_samples says fixed lanes.
    // set_size 1 .. RT_RAY_SET_MAX: n sets of that many records, ray-major; sample s of ray i starts at record
    // i * set_size + s % set_size — pt_samples_q_raysets, or pt_render_raysets for fixed lanes.  Facts and plan go to
    // rt_context::Rays;
    // mask != NULL (rt_render_adaptive_rays; n == W x H, ray i is pixel (i mod W, i div W)): the rays of active decision
    // blocks only, as launch_cameras — the plan and the grid are those of the unmasked launch
    int (*launch_rays)(rt_context *ctx, const void *d_rays, size_t n, uint32_t set_size, uint32_t first, uint32_t count, uint32_t glog2,
                       float4 *accum, const BlockMask *mask, float *m2);
    // rt_render_features_rays, rt_intersect_rays: pt_features_rays, pt_features_chain's record (the same feature_chain) for
    // each of the n rays at d_rays into d_out
    int (*launch_features_rays)(rt_context *ctx, const DeviceScene &sc, const void *d_rays, uint32_t n, uint32_t follow,
                                uint32_t max_chain, rt_feature *d_out);
    // rt_occluded_rays: pt_occluded, for each of the n sets of set_size >= 1 rt_ray records at d_rays (ray-major, at most
    // 2^31 records) the number of records whose first hit lies below the record's bound — d_tmax[k], or t_max where
    // d_tmax is NULL — into d_out[set] (n uint32, overwritten; PT_OCCLUDED_COUNTS)
    int (*launch_occluded)(rt_context *ctx, const DeviceScene &sc, const void *d_rays, size_t n, uint32_t set_size,
                           const float *d_tmax, float t_max, uint32_t *d_out);
    // rt_occluded_hemispheres: pt_occluded_hemi, the p.k hemisphere rays of each of the n feature records at d_features made
    // in registers: their occluded count into d_counts[record] (n uint32, overwritten, through launch_occluded's
    // PT_OCCLUDED_COUNTS; NULL: no search runs) and the rays themselves into d_rays_out (n * p.k rt_ray records, ray-major;
    // NULL: not stored) — one of the two at least
    int (*launch_occluded_hemi)(rt_context *ctx, const DeviceScene &sc, const rt_feature *d_features, size_t n,
                                const rt_hemisphere_params &p, uint32_t *d_counts, void *d_rays_out);
    // rt_render_hemispheres: launch_rays with the sets made — samples first .. first+count-1 of the n feature records at
    // d_features, sample s of record i along hemisphere ray s % p.k of rt_occluded_hemispheres' spawn form (never stored),
    // the sum added to accum[i] (updating m2[i]); a record without a hemisphere is skipped.  pt_samples_q_hemi, or
    // pt_render_hemi for fixed lanes (GatherKernels below); facts and plan go to rt_context::Rays
    int (*launch_hemispheres)(rt_context *ctx, const rt_feature *d_features, size_t n, const rt_hemisphere_params &p,
                              uint32_t first, uint32_t count, uint32_t glog2, float4 *accum, float *m2);
};

// The kernels of rt_render_hemispheres, which a policy keeps in a translation unit of their own (pt_gather.hip: made of the
// headers pt_kernels.hip's sample kernels are made of — pt_sample.hpp, pt_queue.hpp, pt_samples_q_kernel.hpp — with nothing
// instantiated but these): launch_hemispheres launches them through these pointers.
struct GatherKernels {
    using Queue = void (*)(DeviceScene, FrameParams, const PixelRec *, const uint32_t *, const uint32_t *, float4 *, unsigned long long *, uint32_t);
    using Fixed = void (*)(DeviceScene, FrameParams, float4 *, unsigned long long *);
    Queue (*queue)(uint32_t accel, uint32_t geom, uint32_t waves);   // pt_samples_q_hemi of the queue's geometry row; NULL: no such row
    Fixed (*fixed)(bool count, bool accel);                          // pt_render_hemi<COUNT, ACCEL>
};
// defined by pt_gather.hip compiled with -DPT_ARITH=0 / 1 / 2 (as PT_GATHER_KERNELS, pt_arith.hpp)
const GatherKernels *gather_kernels_a0();
const GatherKernels *gather_kernels_a1();
const GatherKernels *gather_kernels_a2();

// defined by pt_kernels.hip compiled with -DPT_ARITH=0 / 1 / 2 (as PT_KERNEL_SET, pt_arith.hpp)
const KernelSet *kernel_set_a0();
const KernelSet *kernel_set_a1();
const KernelSet *kernel_set_a2();

}  // namespace pt
