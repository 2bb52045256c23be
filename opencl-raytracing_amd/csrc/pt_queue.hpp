// pt_queue.hpp — the wave's sample queue: its LDS layout (the launch constants QUEUE_SLOTS, QUEUE_MAX_PIXELS, PT_Q_WAVES* are
// rt_context.hpp's; the host's sizing rule queue_pixels_per_wave is pt_kernels.hip's, beside the planners), WaveQueue, staging and refill for every way of feeding it (pt_prefix's records, camera blocks, a ray
// buffer, ray sets, feature records), the per-pixel sums and the look-ahead replay a wave ends in, and the table of the
// queue's geometry rows.  The kernel text that runs on it is pt_samples_q_kernel.hpp (and pt_samples_w, pt_kernels.hip).
// Templates, PT_DEV / PT_HD inline functions and constants only, inside the policy's namespace: pt_kernels.hip and
// pt_gather.hip both include it.  The switches defined here (#ifndef X / #define X default) reach both units.
#pragma once
#include "rt_context.hpp"
#include "pt_sample.hpp"

namespace PT_NS {

// Fused path, stage 2 with an in-wave SAMPLE QUEUE (default).  Path lengths differ
// wildly between samples (1 bounce into the sky … 30 inside glass), so with one fixed
// sample per lane most lanes of a wave idle while its longest path finishes.  Here a
// wave owns P live pixels = up to QUEUE_SLOTS samples and its 64 lanes pull the next
// sample whenever their path ends: every iteration is "scatter, then nearest hit" for
// all lanes, new samples joining at the scatter step straight from their pixel's
// record (staged in LDS).  A finished sample's radiance goes to its own LDS slot, and
// the slots are summed in exactly the order of pt_render (lane l: samples l, l+g, …;
// then the xor butterfly), so the result does not depend on which lane traced what.
#ifndef PT_REFILL_MIN
#define PT_REFILL_MIN 1   // idle lanes that trigger a refill
#endif
// THE layout of a wave's queue in LDS — the one place that knows it.  The workgroup's dynamic LDS starts with the staged
// tables and face records (queue_static_f4 float4), then the wave's three regions in this order:
//   records      pixels_per_wave x QUEUE_REC_F4 float4   the pixels' PixelRec
//   coordinates  pixels_per_wave x QUEUE_XY_F4 float4    (x, y, rnd_base_v(0, x, y), rnd_base_u(0, x, y))
//   slots        pixels_per_wave x count x 3 floats      one sample's radiance each
// queue_pixels_per_wave and the launcher (pt_kernels.hip) size by these functions and queue_stage carves by them.
#define QUEUE_REC_F4 5u
#define QUEUE_XY_F4 1u
static_assert(sizeof(PixelRec) == QUEUE_REC_F4 * sizeof(float4), "a queue record is a PixelRec");
PT_HD uint32_t queue_pixel_bytes(uint32_t count) { return (QUEUE_REC_F4 + QUEUE_XY_F4) * 16u + count * 3u * 4u; }
PT_HD uint32_t queue_xy_f4(uint32_t pixels_per_wave) { return pixels_per_wave * QUEUE_REC_F4; }                    // float4 from the wave's base
PT_HD uint32_t queue_slot_f4(uint32_t pixels_per_wave) { return pixels_per_wave * (QUEUE_REC_F4 + QUEUE_XY_F4); }   // likewise
PT_HD uint32_t queue_wave_lds_bytes(uint32_t pixels_per_wave, uint32_t count) {
    return (pixels_per_wave * queue_pixel_bytes(count) + 15u) & ~15u;
}
// The static prefix of the dynamic LDS, in front of the wave's queue: stage_materials' tables, then — from float4
// queue_faces_f4 on — the face_f4 float4 of face records of a scene of a few small meshes (fp.lds_face_f4, set by
// launch_fused).  A kernel that cannot stage faces (GEOM == 0, pt_samples_w) passes 0 and never reads the field.
PT_HD uint32_t queue_faces_f4(const DeviceScene &sc) { return lds_static_used(sc.material_count, sc.sphere_count, sc.plane_count); }
PT_HD uint32_t queue_static_f4(const DeviceScene &sc, uint32_t face_f4) { return queue_faces_f4(sc) + face_f4; }

// ---- the wave's sample queue (pt_samples_q, pt_samples_w) -----------------------------------------------------------
// One wave per workgroup: a wave that is through frees its LDS and wave slot at once instead of waiting for three others
// (A/B on C2, waves per workgroup: 4 → 2.42 ms, 2 → 2.42, 1 → 2.34), and lane = threadIdx.x.
// The three regions are carried as LDS-QUALIFIED pointers (like Ctx's staged tables, pt_device.hpp) and every access goes
// through them: as generic pointers in a struct they lose their address space, and the record reads of a refill become
// flat loads — vector-memory instructions, which these kernels are bound by as much as by ALU work.  The 16-byte
// regions are plain aligned structs read and written member by member: the type carries the alignment (which does
// not survive the address-space cast otherwise), and the compiler merges exactly the members a kernel uses into one
// ds_read_b96 / b128, ds_read2_b32 or ds_write_b128.
struct alignas(16) QueueF4 { float x, y, z, w; };
struct alignas(16) QueueXY { uint32_t x, y, bv, bu; };   // bv, bu: rnd_base_v(0, x, y), rnd_base_u(0, x, y)
typedef QueueF4 __attribute__((address_space(3))) *LdsQueueF4;
typedef QueueXY __attribute__((address_space(3))) *LdsQueueXY;
typedef float __attribute__((address_space(3))) *LdsF32;
typedef v4f __attribute__((address_space(3))) *LdsV4Rw;
struct WaveQueue {
    LdsQueueF4 rec;     // [5 p + k]: part k of pixel p's record
    LdsQueueXY xy;      // [p]: pixel p's coordinates and its part of the table index sums
    LdsF32 slot;        // [3 (p count + j) + …]: the radiance of pixel p's sample first + j
    uint32_t npix;      // live pixels this wave owns (<= pixels_per_wave)
    uint32_t count;     // samples per pixel of this launch
    uint32_t total;     // npix x count queue entries
    uint32_t count_log2;  // log2(count) where count is a power of two, else 0xFF
    float inv_count;
};

// The fixed cost a wave pays around its sample loop (profiles/r16_experiments.md), one switch per part
// (the fourth, PT_Q_COUNT64, is read by the planner alone: pt_kernels.hip):
#ifndef PT_TEXEL_LAZY
#define PT_TEXEL_LAZY 1      // GEOM 0: the texel's address arithmetic stays inside the textured branch
#endif
#ifndef PT_STAGE_XY_FAST
#define PT_STAGE_XY_FAST 1   // queue_stage: an unsharded frame's (x, y) without the integer division
#endif
#ifndef PT_STAGE_COPY
#define PT_STAGE_COPY 1      // pt_samples_q<false, false, …> copies the scene's LDS tables from the context's block
#endif
// What a wave issues per iteration of the sample loop and the result does not need (profiles/r20_experiments.md):
#ifndef PT_TABLES_BY_COUNT
#define PT_TABLES_BY_COUNT 1 // pt_samples_q<false, false, …>: "is the table staged?" is asked of the scene's counts, not of the LDS pointer
#endif
#ifndef PT_RND_BY_USE
#define PT_RND_BY_USE 1      // pt_samples_q<false, false, 0, …> without CAM: an interaction gathers only the table entries its material reads (profiles/r22_experiments.md)
#endif

// queue_stage's slot → (x, y).  slot_to_pixel divides the tile index by fp.tiles_x, a launch constant, with the generic
// uint32 division (about 25 VALU instructions).  An unsharded frame (world == 1, so rank == 0 and t = slot >> tpix_log2)
// of at most 2^20 tiles — both wave-uniform — takes the quotient as queue_fetch takes idx / count:
//     ty = (uint32_t)(((float)t + 0.5f) * rcp((float)tiles_x)),   tx = t - ty * tiles_x.
// Exact: t < 2^20 and tiles_x <= tiles_total <= 2^20, so (float)tiles_x, (float)t and t + 0.5 (22 significant bits) are
// exact; v_rcp_f32 is within 1 ulp (relative 2^-23) and the product rounds once (2^-24), so the computed value is within
//     (t + 0.5) / tiles_x · (2^-23 + 2^-24 + 2^-47) < 2^20 · 1.5001 · 2^-23 / tiles_x < 0.19 / tiles_x
// of (t + 0.5) / tiles_x = Q + (r + 0.5) / tiles_x (0 <= r < tiles_x), which lies at least 0.5 / tiles_x away from
// both Q and Q + 1: the truncation is Q.  (tests/test_wave_fixed_host.py restates it for every reciprocal within 1 ulp.)
// The live list holds slots of valid pixels only (pt_prefix), so slot_to_pixel's range checks — whose result queue_stage
// never used — have nothing to say here.  Sharded and larger frames keep slot_to_pixel.
#define PT_XY_FAST_MAX_TILES (1u << 20)
template <bool FAST>
PT_DEV void stage_xy(const FrameParams &fp, uint32_t slot, uint32_t &x, uint32_t &y) {
    if (FAST && PT_STAGE_XY_FAST && fp.world == 1u && fp.tiles_total <= PT_XY_FAST_MAX_TILES) {
        const uint32_t tpix_log2 = fp.tile_w_log2 + fp.tile_h_log2;
        const uint32_t t = slot >> tpix_log2, in = slot & ((1u << tpix_log2) - 1u);
        const uint32_t ty = (uint32_t)(((float)t + 0.5f) * __builtin_amdgcn_rcpf((float)fp.tiles_x)), tx = t - ty * fp.tiles_x;
        x = (tx << fp.tile_w_log2) + (in & ((1u << fp.tile_w_log2) - 1u));
        y = (ty << fp.tile_h_log2) + (in >> fp.tile_w_log2);
    } else {
        (void)slot_to_pixel(fp, slot, x, y);
    }
}

// What every queue_stage* opens and closes with, each said once.  All three fill the caller's WaveQueue in place: returning
// it by value from the carve moved 32 kernels ("A translation unit of their own").
//   queue_carve   the wave's three regions of the workgroup's dynamic LDS, by the layout above (`lds`: the workgroup's dynamic
//                 LDS; face_f4: the float4 of face records the kernel staged in it, queue_static_f4)
//   queue_owned   the counts of an entry that finds its pixels by a ballot, from the owners' mask
//   queue_staged  the wave's fence and barrier behind the staging stores, then the two operands of the refill's idx / count
//                 (CL as in queue_stage).  Called where these lines stood — behind the staging stores: see queue_stage.
PT_DEV void queue_carve(WaveQueue &q, const DeviceScene &sc, uint32_t pixels_per_wave, float4 *lds, uint32_t face_f4) {
    float4 *wave_lds = lds + queue_static_f4(sc, face_f4);
    q.rec = (LdsQueueF4)wave_lds;
    q.xy = (LdsQueueXY)(wave_lds + queue_xy_f4(pixels_per_wave));
    q.slot = (LdsF32)(wave_lds + queue_slot_f4(pixels_per_wave));
}
PT_DEV void queue_owned(WaveQueue &q, const FrameParams &fp, unsigned long long owners) {
    q.npix = (uint32_t)__popcll(owners);
    q.count = fp.count;
    q.total = q.npix * q.count;
}
template <int CL = -1>
PT_DEV void queue_staged(WaveQueue &q, const FrameParams &fp) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    q.inv_count = fp.inv_count;
    q.count_log2 = CL >= 0 ? (uint32_t)CL : (q.count & (q.count - 1u)) == 0u ? (uint32_t)__builtin_ctz(q.count) : 0xFFu;
}

// Stages the records and coordinates of the wave's pixels — the `npix` live-list entries from `pix0` on, which the kernel
// took with live_take before it staged anything (a wave that took none has left by now); `lds` is the workgroup's dynamic
// LDS and face_f4 the float4 of face records the kernel staged in it (queue_static_f4).  Every lane of the wave calls it (contains the wave's fence and barrier).
// CL: the launch's sample count is the compile-time 1 << CL (pt_samples_q's COUNT_LOG2; -1: any count, read from fp).
// XY_FAST: stage_xy's short form (pt_samples_q without counters and without a BVH walk; every other kernel keeps slot_to_pixel).
template <int CL = -1, bool XY_FAST = false>
PT_DEV WaveQueue queue_stage(const DeviceScene &sc, const FrameParams &fp, const PixelRec *__restrict__ recs,
                             const uint32_t *__restrict__ live, uint32_t npix, uint32_t pix0,
                             uint32_t pixels_per_wave, float4 *lds, uint32_t face_f4) {
    WaveQueue q;
    queue_carve(q, sc, pixels_per_wave, lds, face_f4);
    const uint32_t lane = threadIdx.x;
    q.npix = npix;
    q.count = CL >= 0 ? 1u << (CL & 31) : fp.count;
    q.total = q.npix * q.count;
    for (uint32_t i = lane; i < q.npix * QUEUE_REC_F4; i += 64u) {
        uint32_t p = i / QUEUE_REC_F4, part = i - p * QUEUE_REC_F4;
        const float4 t = reinterpret_cast<const float4 *>(recs + pix0 + p)[part];
        // The record part is written whole, through a vector-typed pointer to the same 16 aligned bytes that queue_fetch
        // reads member by member.  The pun is intentional: written member by member, the loop vectoriser interleaves this
        // loop two trips wide (a longer prologue for nothing).  It is safe: clang lets vector types alias their element
        // type, and the wave's fence and barrier below stand between this store and every read.
        *(LdsV4Rw)(q.rec + i) = v4f{t.x, t.y, t.z, t.w};
    }
    if (lane < q.npix) {
        uint32_t x = 0, y = 0;
        stage_xy<XY_FAST>(fp, live[pix0 + lane], x, y);
        // (x, y, and the pixel's part of the two table index sums: rnd_base_v = (sample·2683 + x·3931 + y·2504)·3 and
        // rnd_base_u = sample·2683 + x·3931 + y are linear in uint32 arithmetic, so a refill needs two multiplies, not five)
        q.xy[lane].x = x;
        q.xy[lane].y = y;
        q.xy[lane].bv = rnd_base_v(0u, x, y);
        q.xy[lane].bu = rnd_base_u(0u, x, y);
    }
    // (the wave's fence and barrier, then the two operands of queue_fetch's division — formed here, where the parent kernels
    // formed them: before the staging loop they change the register allocation of every instantiation)
    queue_staged<CL>(q, fp);
    return q;
}

// Queue entry idx → what a lane starts from: the record q0 … q4 (PixelRec's five parts; a pixel with a shared decision
// tree: this sample's leaf), its kind bits, and the sample's part of the two table index sums.
struct QueueEntry {
    float4 q0, q1, q2, q3, q4;
    uint32_t bits, bv, bu;
};
template <int CL = -1>
PT_DEV QueueEntry queue_fetch(const WaveQueue &q, const DeviceScene &sc, const FrameParams &fp, uint32_t idx) {
    // pixel of this queue entry: p = idx / count, exactly, without an integer divide:
    // (idx + 0.5)/count lies >= 0.5/count away from every integer, far more than the rounding
    // of the float product (idx < 8192, count <= 512)
    // (a power-of-two count — wave-uniform — needs a shift; otherwise one float multiply:)
    // (a compile-time count: a shift and a mask, and the record's address by shifts and adds)
    const uint32_t p = CL >= 0 ? idx >> (CL & 31) : q.count_log2 != 0xFFu ? idx >> q.count_log2 : (uint32_t)(((float)idx + 0.5f) * q.inv_count);
    const uint32_t sample = fp.first + (CL >= 0 ? idx & ((1u << (CL & 31)) - 1u) : idx - p * q.count);
    auto part = [&](uint32_t k) {
        const LdsQueueF4 f = q.rec + (QUEUE_REC_F4 * p + k);
        return make_float4(f->x, f->y, f->z, f->w);
    };
    QueueEntry e;
    e.q0 = part(0);
    e.q1 = part(1);
    e.q2 = part(2);
    e.q3 = part(3);
    e.q4 = part(4);
    e.bv = sample * 8049u + q.xy[p].bv;   // = rnd_base_v(sample, x, y)
    e.bu = sample * 2683u + q.xy[p].bu;   // = rnd_base_u(sample, x, y)
    e.bits = __float_as_uint(e.q0.w);
    if ((e.bits & 0xFFu) == REC_TREE) {   // the pixel has a shared decision tree: this sample's leaf
        const float4 *lf = tree_leaf(fp.trees + __float_as_uint(e.q4.w), sc.table, e.bu);
        e.q0 = lf[0]; e.q1 = lf[1]; e.q2 = lf[2]; e.q3 = lf[3]; e.q4 = lf[4];
        e.bits = __float_as_uint(e.q0.w);
    }
    return e;
}

// the finished sample's radiance, into its own slot
PT_DEV void queue_put(const WaveQueue &q, uint32_t idx, V3 rgb) {
    q.slot[3 * idx] = rgb.x;
    q.slot[3 * idx + 1] = rgb.y;
    q.slot[3 * idx + 2] = rgb.z;
}

// Once every sample of the wave is in its slot: the per-pixel sums in pt_render's order (lane l of a pixel's g lanes:
// samples l, l + g, …; then the xor butterfly), added to the accumulator.  Every lane of the wave calls it.
// MOMENTS: the instantiation for launches that keep sample moments (FrameParams::m2 != NULL) — the slots are read a second
// time, for the squared deviations from the pixel's mean.  A template parameter of the two queue kernels, not a branch on
// the pointer like fp.la_ring: read as a kernel argument the pointer holds two SGPRs through the hot loop, where
// pt_samples_q<false, false, 1, 6> of policy 0 parks exactly 64 SGPRs in the lanes of ONE VGPR — the two more took a second
// one and the loop spilled three VGPRs to scratch, with the option off.  The instantiations without moments never read
// the field and compile to what they compiled to before it existed.
//
// Without moments only lane 0 of a pixel's g lanes is used, and after the butterfly step `off` lanes l and l ^ off hold
// the same value (IEEE addition commutes): lane 0's sum is, bit for bit, that of the half-lane tree
//   for off = g/2 … 1, for l < off: T(l) = T(l) + T(l + off)
// (tests/test_queue_sums_host.py).  queue_sums_tree forms that tree without LDS permutes (PT_QUEUE_SUMS_TREE 0: the butterfly):
//   offset 32     at the LDS read: half-wave h takes a pixel of its own and lane i of it forms S(i) and S(i + 32)
//   offset 16     v_permlane16_swap of two such registers (pixels pb, pb+1 | pb+2, pb+3) and one add: four pixels, one per
//                 row of 16 lanes, in row order pb, pb+2, pb+1, pb+3
//   offsets 8 … 1 v_add_f32 with a DPP row shift (lane i takes lane i + off of its row); the lanes outside lane 0's cone
//                 add neighbours or zeros and are never stored
// and the four (g >= 32) or 64 / g rows' first lanes add to the accumulator together.  g <= 16 keeps a pass per 64 / g pixels
// and needs the row shifts only.  All of it runs under the full EXEC mask: a pixel the wave does not own has a trip count
// of 0, never a branch around a cross-lane operation, and reads nothing.
// A NaN in a slot gives a NaN sum in both forms, but its payload is not pinned: the compiler picks the operand order of a
// DPP add.  No radiance is a NaN (no test produces one).
#ifndef PT_QUEUE_SUMS_TREE
#define PT_QUEUE_SUMS_TREE 1
#endif
// lane l of pixel p's g lanes: 0.0f + its slots l, l + g, … in that order (nothing for a pixel the wave does not own)
PT_DEV V3 queue_lane_sum(const WaveQueue &q, uint32_t p, uint32_t l, uint32_t g) {
    V3 sum = mk(0.0f, 0.0f, 0.0f);
    const uint32_t n = p < q.npix ? q.count : 0u;
    for (uint32_t j = l; j < n; j += g) {
        const LdsF32 sl = q.slot + 3u * (p * q.count + j);
        sum = sum + mk(sl[0], sl[1], sl[2]);
    }
    return sum;
}
// v(i) + v(i + OFF) within a row of 16 lanes (one v_add_f32_dpp row_shl:OFF; a lane whose partner lies outside its row adds 0)
template <int OFF>
PT_DEV float row_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + OFF, 0xF, 0xF, false));
}
template <int OFF>
PT_DEV V3 row_add(V3 v) { return mk(row_add<OFF>(v.x), row_add<OFF>(v.y), row_add<OFF>(v.z)); }
// rows (a0 a1 a2 a3), (b0 b1 b2 b3) → (a0 + a1, b0 + b1, a2 + a3, b2 + b3): the swap exchanges a's odd rows with b's even rows
PT_DEV float row_pair_add(float a, float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// count == g == 64 (queue_sums_tree<6>): queue_lane_sum's loop runs exactly one trip for a pixel the wave owns and none
// otherwise — one guarded read, the same operands in the same order (0.0f + slot), no loop
PT_DEV V3 queue_lane_slot64(const WaveQueue &q, uint32_t p, uint32_t l) {
    V3 sum = mk(0.0f, 0.0f, 0.0f);
    if (p < q.npix) {
        const LdsF32 sl = q.slot + 3u * (p * 64u + l);
        sum = sum + mk(sl[0], sl[1], sl[2]);
    }
    return sum;
}
// The sums' addresses once per half-wave (PT_SUMS_ADDR; queue_sums_tree<6, STORE> only, so that no other kernel changes): one LDS
// address per lane, that of slot (half, i); the slots of (pb + half, i), (pb + 2 + half, i), (·, i + 32) and of the second
// pass lie at constant distances from it, which the LDS reads take as immediate offsets.  Ownership is asked once per pixel,
// not once per read, and both reads of a pixel stand under the one test: a pixel the wave does not own still gives
// 0.0f + 0.0f = +0, the value the two guarded reads gave.  The accumulator index y · w + x stays below RT_MAX_DIM² and is
// formed in 32 bits, then scaled and added to the base in one 64-bit step.
#ifndef PT_SUMS_ADDR
#define PT_SUMS_ADDR 1
#endif
static_assert((uint64_t)RT_MAX_DIM * RT_MAX_DIM <= 0xFFFFFFFFull, "a pixel index fits 32 bits (queue_sums_tree, PT_SUMS_ADDR)");
// both slots of lane i of a pixel at `sl` (its slot i): (0.0f + slot i) + (0.0f + slot i + 32), or +0 for a pixel not owned
PT_DEV V3 queue_lane_pair64(LdsF32 sl, bool owned) {
    V3 sum = mk(0.0f, 0.0f, 0.0f);
    if (owned) {
        sum = sum + mk(sl[0], sl[1], sl[2]);
        sum = sum + (mk(0.0f, 0.0f, 0.0f) + mk(sl[96], sl[97], sl[98]));
    }
    return sum;
}
// CL = 6: a launch of 64 samples per pixel with 64 lanes per pixel (at most QUEUE_SLOTS / 64 = 8 pixels: two passes)
// STORE: the instantiation may be launched with fp.store set (pt_samples_q<false, false, 0 | 1, …, COUNT_LOG2 = 6>); every
// other one never reads the field.
template <int CL = -1, bool STORE = false>
PT_DEV void queue_sums_tree(const WaveQueue &q, const FrameParams &fp, float4 *__restrict__ accum) {
    if (CL == 6) {
        static_assert(QUEUE_SLOTS / 64u <= 8u, "two passes of four pixels");
        const uint32_t lane = threadIdx.x, half = lane >> 5, i = lane & 31u, row = lane >> 4;
        const LdsF32 sl0 = q.slot + 3u * (half * 64u + i);   // (PT_SUMS_ADDR: slot i of pixel `half`)
#pragma unroll
        for (uint32_t pb = 0; pb < 8u; pb += 4u) {
            if (pb >= q.npix) break;
            V3 a, b;
            if (STORE && PT_SUMS_ADDR) {
                a = queue_lane_pair64(sl0 + 3u * 64u * pb, pb + half < q.npix);
                b = queue_lane_pair64(sl0 + 3u * 64u * (pb + 2u), pb + 2u + half < q.npix);
            } else {
                a = queue_lane_slot64(q, pb + half, i), b = queue_lane_slot64(q, pb + 2u + half, i);
                a = a + queue_lane_slot64(q, pb + half, i + 32u);   // offset 32
                b = b + queue_lane_slot64(q, pb + 2u + half, i + 32u);
            }
            V3 sum = mk(row_pair_add(a.x, b.x), row_pair_add(a.y, b.y), row_pair_add(a.z, b.z));   // offset 16
            sum = row_add<1>(row_add<2>(row_add<4>(row_add<8>(sum))));
            const uint32_t p = pb + ((row & 1u) << 1 | row >> 1);
            if (p < q.npix && (lane & 15u) == 0u) {
                if (STORE && PT_SUMS_ADDR) accumulate_any(fp, accum, q.xy[p].y * (uint32_t)fp.w + q.xy[p].x, sum, 64u);   // (32-bit index)
                else if (STORE) accumulate_any(fp, accum, (size_t)q.xy[p].y * fp.w + q.xy[p].x, sum, 64u);
                else accumulate(accum, (size_t)q.xy[p].y * fp.w + q.xy[p].x, sum, 64u);
            }
        }
        return;
    }
    const uint32_t lane = threadIdx.x, gl = fp.group_log2;
    if (gl >= 5u) {
        const uint32_t half = lane >> 5, i = lane & 31u, g = 1u << gl, row = lane >> 4;
        for (uint32_t pb = 0; pb < q.npix; pb += 4u) {
            V3 a = queue_lane_sum(q, pb + half, i, g), b = queue_lane_sum(q, pb + 2u + half, i, g);
            if (gl == 6u) {   // offset 32
                a = a + queue_lane_sum(q, pb + half, i + 32u, g);
                b = b + queue_lane_sum(q, pb + 2u + half, i + 32u, g);
            }
            V3 sum = mk(row_pair_add(a.x, b.x), row_pair_add(a.y, b.y), row_pair_add(a.z, b.z));   // offset 16
            sum = row_add<1>(row_add<2>(row_add<4>(row_add<8>(sum))));
            const uint32_t p = pb + ((row & 1u) << 1 | row >> 1);
            if (p < q.npix && (lane & 15u) == 0u) accumulate(accum, (size_t)q.xy[p].y * fp.w + q.xy[p].x, sum, q.count);
        }
    } else {
        const uint32_t g = 1u << gl, ppp = 64u >> gl;
        for (uint32_t pb = 0; pb < q.npix; pb += ppp) {
            const uint32_t p = pb + (lane >> gl), l = lane & (g - 1u);
            V3 sum = queue_lane_sum(q, p, l, g);
            if (gl >= 4u) sum = row_add<8>(sum);
            if (gl >= 3u) sum = row_add<4>(sum);
            if (gl >= 2u) sum = row_add<2>(sum);
            if (gl >= 1u) sum = row_add<1>(sum);
            if (p < q.npix && l == 0u) accumulate(accum, (size_t)q.xy[p].y * fp.w + q.xy[p].x, sum, q.count);
        }
    }
}
// BUTTERFLY: the instantiation keeps the butterfly and is the code it was before the tree existed —
//   the counting builds, whose 14 counters live through the epilogue: with the tree two of them (policy 0 <true, true, 0, 6>,
//   policy 1 <true, true, 1, 5>) spill more registers in the sample loop;
//   the kernels with a BVH walk (pt_samples_q<…, ACCEL = true>, pt_samples_w): their waves live for milliseconds, the
//   epilogue is nothing to them, and with the tree C4 and C5 measured 1.2 % and 0.9 % SLOWER than the parent
//   (profiles/r13_experiments.md) — the walk loops' code moved with the epilogue behind them.
template <bool MOMENTS, bool BUTTERFLY = false, int CL = -1, bool STORE = false>
PT_DEV void queue_sums(const WaveQueue &q, const FrameParams &fp, float4 *__restrict__ accum) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (PT_QUEUE_SUMS_TREE && !MOMENTS && !BUTTERFLY) return queue_sums_tree<CL, STORE>(q, fp, accum);   // (moments need the sum in all g lanes)
    const uint32_t lane = threadIdx.x;
    const uint32_t g = 1u << fp.group_log2, ppp = 64u >> fp.group_log2;
    for (uint32_t pb = 0; pb < q.npix; pb += ppp) {
        uint32_t p = pb + (lane >> fp.group_log2), l = lane & (g - 1u);
        V3 sum = mk(0.0f, 0.0f, 0.0f);
        if (p < q.npix)
            for (uint32_t j = l; j < q.count; j += g) {
                const LdsF32 sl = q.slot + 3u * (p * q.count + j);
                sum = sum + mk(sl[0], sl[1], sl[2]);
            }
        sum = group_sum(sum, g);
        if (MOMENTS) {   // a second pass over the same slots, the sum being in all g lanes
            // the launch's centred second moment about its own mean — never sum l^2 - n m^2 (pt_moments.hpp)
            const float mean = moments_lum(sum.x, sum.y, sum.z) / (float)q.count;
            float dev2 = 0.0f;
            if (p < q.npix)
                for (uint32_t j = l; j < q.count; j += g) {
                    const LdsF32 sl = q.slot + 3u * (p * q.count + j);
                    const float d = moments_lum(sl[0], sl[1], sl[2]) - mean;
                    dev2 += d * d;
                }
            for (uint32_t off = g >> 1; off > 0; off >>= 1) dev2 += __shfl_xor(dev2, off);
            if (p < q.npix && l == 0) moments_update(accum, fp.m2, (size_t)q.xy[p].y * fp.w + q.xy[p].x, sum, q.count, dev2);
        }
        if (p < q.npix && l == 0) accumulate(accum, (size_t)q.xy[p].y * fp.w + q.xy[p].x, sum, q.count);
    }
}

// A look-ahead launch ends here instead (FrameParams::la_ring): the wave's pixels take their `count` retrace steps in
// sample order — pixel p from la_image[pix], step j with the sum of the one-sample group 0.0f + slot[p][j], the image after
// it into frame j of the ring — and nothing is added to the accumulator.  Lane 4 p' + c owns channel c of the wave's pixel
// p' (a wave owns at most QUEUE_MAX_PIXELS = 16 of them): the chain of a channel is sequential by definition, and the four
// lanes of a pixel store its 16 bytes of a frame with one instruction (channel 3 is the alpha of 1).
// Every lane of the wave calls it.
// CAM (a look-ahead launch of the camera entry, rt_render_again_cameras): fp.cams holds the eight bytes la_image would, so
// the start image comes from the RING — the host has copied the image as it lies into frame 0 before the launch, and the
// lane takes its channel from there before its own loop overwrites that element (the same lane owns (pixel, channel) for
// the read and for every write, and no other wave owns the pixel).  Everything after that read is the same code.
static_assert(QUEUE_MAX_PIXELS * 4u <= 64u, "queue_replay maps (pixel, channel) to the wave's lanes");
template <bool CAM = false>
PT_DEV void queue_replay(const WaveQueue &q, const FrameParams &fp) {
    static_assert(!CAM || !PT_RING_PIXEL_MAJOR, "the camera look-ahead's start image is frame 0 of a frame-major ring (one contiguous "
                                                "device copy of the image); the pixel-major A/B layout has no such frame");
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t lane = threadIdx.x, ch = lane & 3u;
    const bool alpha = ch == 3u;
    for (uint32_t pb = 0; pb < q.npix; pb += 16u) {
        const uint32_t p = pb + (lane >> 2);
        if (p >= q.npix) continue;
        const size_t pix = (size_t)q.xy[p].y * fp.w + q.xy[p].x;
        float *out = reinterpret_cast<float *>(fp.la_ring) + ch;
        float prev = CAM ? out[4u * ring_at(fp, pix, 0u)] : reinterpret_cast<const float *>(fp.la_image)[4u * pix + ch];
        const LdsF32 sl = q.slot + 3u * (p * q.count) + (alpha ? 0u : ch);
        for (uint32_t j = 0; j < q.count; j++) {
            prev = retrace_step1(prev, 0.0f + sl[3u * j], fp.first + j);
            out[4u * ring_at(fp, pix, j)] = alpha ? 1.0f : prev;
        }
    }
}

// ---- the queue's entry FROM THE CAMERA (pt_samples_q<…, CAM>; rt_render_spp_cameras) ---------------------------------------
// Sample first + j of a pixel looks through camera block j of fp.cams, so the samples of a pixel share no path prefix:
// there are no records, no live list and no trees.  A wave owns the owned, active pixels among `pixels_per_wave`
// consecutive SLOTS of the launch's range (wave b: slot_begin + b·ppw …) — found and compacted inside the wave by one
// ballot, so the launch needs no list kernel and touches none of the slot buffers (a kept prefix lies as it lay).  A wave
// whose slots hold no such pixel (the slots of a partial tile outside the frame) leaves before anything is staged.
// The queue's LDS layout is queue_stage's, so the sizing rules are shared; of a pixel's record region (80 bytes) the first
// two floats hold its frame coordinates (s, t) = (x / w, y / h) — primary_ray's first part, formed here once per pixel.
// Every lane of the wave calls queue_stage_cam after the ballot (it holds the wave's fence).
PT_DEV WaveQueue queue_stage_cam(const DeviceScene &sc, const FrameParams &fp, bool owns, uint32_t x, uint32_t y,
                                 unsigned long long owners, uint32_t pixels_per_wave, float4 *lds, uint32_t face_f4) {
    WaveQueue q;
    queue_carve(q, sc, pixels_per_wave, lds, face_f4);
    queue_owned(q, fp, owners);
    if (owns) {
        const uint32_t k = lanes_below(owners);   // (< npix <= pixels_per_wave)
        q.xy[k].x = x;
        q.xy[k].y = y;
        q.xy[k].bv = rnd_base_v(0u, x, y);
        q.xy[k].bu = rnd_base_u(0u, x, y);
        q.rec[QUEUE_REC_F4 * k].x = primary_coord(x, fp.w);
        q.rec[QUEUE_REC_F4 * k].y = primary_coord(y, fp.h);
    }
    queue_staged(q, fp);
    return q;
}
// Queue entry idx → (pixel p, sample first + j): the primary ray through block j — the policy's own primary_ray, its second
// part (primary_ray_at) on the staged coordinates — and the sample's part of the two table index sums.  The blocks are GATHERED from global memory here, at the refill — the lanes
// of a refill hold consecutive entries, i.e. mostly consecutive j of one pixel, so a wave reads a contiguous stretch of the
// table (48 bytes per lane) that every wave of the launch reads too: it lives in L2 / the vector L1.  In LDS the table of a
// 512-sample launch would be 24 KiB per wave, four times the queue itself (about 6 KiB at 6 waves per SIMD).
struct CameraEntry {
    Ray r;
    uint32_t bv, bu;
};
// Queue entry idx of an entry without records → (p, j): the wave's pixel p = idx / count (as queue_fetch forms it: a shift
// for a power-of-two count, else one float multiply) and j = idx - p * count; the entry's sample is first + j.  Returned as
// a value: with the sample handed back through a reference 23 kernels moved (as above).
struct QueuePos { uint32_t p, j; };
PT_DEV QueuePos queue_pos(const WaveQueue &q, uint32_t idx) {
    const uint32_t p = q.count_log2 != 0xFFu ? idx >> q.count_log2 : (uint32_t)(((float)idx + 0.5f) * q.inv_count);
    return QueuePos{p, idx - p * q.count};
}
PT_DEV CameraEntry queue_fetch_cam(const WaveQueue &q, const FrameParams &fp, uint32_t idx) {
    const QueuePos at = queue_pos(q, idx);
    const uint32_t p = at.p, j = at.j, sample = fp.first + j;
    const LdsQueueF4 st = q.rec + QUEUE_REC_F4 * p;
    CameraEntry e;
    e.r = primary_ray_at(fp.cams + 12u * j, st->x, st->y);
    e.bv = sample * 8049u + q.xy[p].bv;   // = rnd_base_v(sample, x, y)
    e.bu = sample * 2683u + q.xy[p].bu;   // = rnd_base_u(sample, x, y)
    return e;
}

// ---- the queue's entry FROM A RAY BUFFER (pt_samples_q_rays; rt_render_rays) -----------------------------------------------
// The camera entry with the primary ray given instead of formed: slot i of the launch's range IS ray i of fp.rays (no tiles,
// no shard; an adaptive round's mask is tested by ray_active at the kernel's entry), a wave owns the slots below slot_end among its `pixels_per_wave` consecutive ones, and a ray's `count`
// samples are the queue entries of one "pixel".  The LDS layout is queue_stage's once more, so the sizing rules stay shared:
//   coordinates   (x: the ray index, y: 0, rnd_base_v(0, ray.x, ray.y), rnd_base_u(0, ray.x, ray.y)) — queue_sums forms
//                 y · fp.w + x = the ray index with its code unchanged, and the random stream is the one the ray names;
//   record        of the 80 bytes the first two float4 hold the ray as it lies in the buffer, (o, x bits) and (d, y bits):
//                 two 16-byte loads per ray at staging, two 12-byte LDS reads per refill, no camera block, no normalize.
// Every lane of the wave calls queue_stage_rays after the ballot (it holds the wave's fence).
PT_DEV WaveQueue queue_stage_rays(const DeviceScene &sc, const FrameParams &fp, bool owns, uint32_t index,
                                  unsigned long long owners, uint32_t pixels_per_wave, float4 *lds, uint32_t face_f4) {
    WaveQueue q;
    queue_carve(q, sc, pixels_per_wave, lds, face_f4);
    queue_owned(q, fp, owners);
    if (owns) {
        const uint32_t k = lanes_below(owners);   // (< npix <= pixels_per_wave)
        const float4 ro = fp.rays[2u * (size_t)index], rd = fp.rays[2u * (size_t)index + 1u];
        const uint32_t rx = __float_as_uint(ro.w), ry = __float_as_uint(rd.w);
        q.xy[k].x = index;
        q.xy[k].y = 0u;
        q.xy[k].bv = rnd_base_v(0u, rx, ry);
        q.xy[k].bu = rnd_base_u(0u, rx, ry);
        *(LdsV4Rw)(q.rec + QUEUE_REC_F4 * k) = v4f{ro.x, ro.y, ro.z, ro.w};        // (whole, as queue_stage writes a record part)
        *(LdsV4Rw)(q.rec + QUEUE_REC_F4 * k + 1u) = v4f{rd.x, rd.y, rd.z, rd.w};
    }
    queue_staged(q, fp);
    return q;
}
// Queue entry idx → (ray p, sample first + j): the staged ray as it was given, and the sample's part of the two index sums.
PT_DEV CameraEntry queue_fetch_rays(const WaveQueue &q, const FrameParams &fp, uint32_t idx) {
    const QueuePos at = queue_pos(q, idx);
    const uint32_t p = at.p, sample = fp.first + at.j;
    const LdsQueueF4 st = q.rec + QUEUE_REC_F4 * p;
    CameraEntry e;
    e.r.o = mk(st[0].x, st[0].y, st[0].z);
    e.r.d = mk(st[1].x, st[1].y, st[1].z);
    e.bv = sample * 8049u + q.xy[p].bv;   // = rnd_base_v(sample, ray.x, ray.y)
    e.bu = sample * 2683u + q.xy[p].bu;   // = rnd_base_u(sample, ray.x, ray.y)
    return e;
}

// ---- the queue's entry FROM RAY SETS (pt_samples_q_raysets; rt_render_ray_sets) --------------------------------------------
// The ray entry with a SET of set_size records per ray, ray-major: sample s of ray i starts at record i · set_size +
// (s mod set_size) of fp.rays — its own origin, direction and random-stream ids.  Nothing of a ray can be staged once per
// slot, so staging writes the ray index alone (queue_sums reads x and y, nothing else) and a refill loads its record from
// global memory, as queue_fetch_cam gathers its block: the lanes of a refill hold consecutive samples of one ray, i.e. one
// contiguous stretch of 32-byte records.  Unlike the camera table a record is read by one lane only — it comes from HBM.
// The set size travels in fp.cam, of which a ray launch reads nothing else: cam[0] holds its bits, cam[1] its reciprocal
// (the IEEE quotient 1 / set_size computed on the host, as inv_count is).
PT_DEV WaveQueue queue_stage_raysets(const DeviceScene &sc, const FrameParams &fp, bool owns, uint32_t index,
                                     unsigned long long owners, uint32_t pixels_per_wave, float4 *lds, uint32_t face_f4) {
    WaveQueue q;
    queue_carve(q, sc, pixels_per_wave, lds, face_f4);
    queue_owned(q, fp, owners);
    if (owns) {
        const uint32_t k = lanes_below(owners);   // (< npix <= pixels_per_wave)
        q.xy[k].x = index;
        q.xy[k].y = 0u;
    }
    queue_staged(q, fp);
    return q;
}
// Queue entry idx → (ray p, sample first + j): the sample's own record, and both index sums in full from the record's ids.
PT_DEV CameraEntry queue_fetch_raysets(const WaveQueue &q, const FrameParams &fp, uint32_t idx) {
    const QueuePos at = queue_pos(q, idx);
    const uint32_t p = at.p, sample = fp.first + at.j;
    const float4 *rec = ray_set_record(fp, q.xy[p].x, ray_set_member(fp, sample));
    const float4 ro = rec[0], rd = rec[1];   // (non-temporal loads were tried: no gain, profiles/r24_experiments.md)
    CameraEntry e;
    e.r.o = mk(ro.x, ro.y, ro.z);
    e.r.d = mk(rd.x, rd.y, rd.z);
    e.bv = rnd_base_v(sample, __float_as_uint(ro.w), __float_as_uint(rd.w));
    e.bu = rnd_base_u(sample, __float_as_uint(ro.w), __float_as_uint(rd.w));
    return e;
}

// ---- the queue's entry FROM FEATURE RECORDS (pt_samples_q_hemi; rt_render_hemispheres) ------------------------------------
// The ray-set entry with the set made at the refill instead of loaded: slot i of the launch's range is feature record i of
// fp.feats, and the kernel gives a slot to a lane only where the record has a hemisphere (hemisphere_valid, where the ray
// forms test ray_active) — an invalid record is in no wave's queue.  What a record's k rays share is staged once, in the
// LDS layout of the ray entry:
//   coordinates   (x: the record index, y: 0, rnd_base_v(0, i, 0), rnd_base_u(0, i, 0)): the spawn form's rays name the
//                 random stream (i, 0);
//   record        of the 80 bytes the first four float4 hold the frame — o, n̂, tan, bit, three floats each.
// A refill reads the frame back (four 12-byte LDS reads) and makes ray s mod k in registers: nothing comes from global memory.
PT_DEV WaveQueue queue_stage_hemi(const DeviceScene &sc, const FrameParams &fp, bool owns, uint32_t index,
                                  unsigned long long owners, uint32_t pixels_per_wave, float4 *lds, uint32_t face_f4) {
    WaveQueue q;
    queue_carve(q, sc, pixels_per_wave, lds, face_f4);
    queue_owned(q, fp, owners);
    if (owns) {
        const uint32_t k = lanes_below(owners);   // (< npix <= pixels_per_wave)
        HemiFrame fr;
        hemi_frame_of(fp, index, fr);
        q.xy[k].x = index;
        q.xy[k].y = 0u;
        q.xy[k].bv = rnd_base_v(0u, index, 0u);
        q.xy[k].bu = rnd_base_u(0u, index, 0u);
        *(LdsV4Rw)(q.rec + QUEUE_REC_F4 * k) = v4f{fr.o.x, fr.o.y, fr.o.z, 0.0f};
        *(LdsV4Rw)(q.rec + QUEUE_REC_F4 * k + 1u) = v4f{fr.n.x, fr.n.y, fr.n.z, 0.0f};
        *(LdsV4Rw)(q.rec + QUEUE_REC_F4 * k + 2u) = v4f{fr.tan.x, fr.tan.y, fr.tan.z, 0.0f};
        *(LdsV4Rw)(q.rec + QUEUE_REC_F4 * k + 3u) = v4f{fr.bit.x, fr.bit.y, fr.bit.z, 0.0f};
    }
    queue_staged(q, fp);
    return q;
}
// Queue entry idx → (record p, sample first + j): hemisphere ray s mod k about the staged frame, and the sample's part of the
// two index sums.
PT_DEV CameraEntry queue_fetch_hemi(const WaveQueue &q, const FrameParams &fp, uint32_t idx) {
    const QueuePos at = queue_pos(q, idx);
    const uint32_t p = at.p, sample = fp.first + at.j;
    const LdsQueueF4 st = q.rec + QUEUE_REC_F4 * p;
    HemiFrame fr;
    fr.o = mk(st[0].x, st[0].y, st[0].z);
    fr.n = mk(st[1].x, st[1].y, st[1].z);
    fr.tan = mk(st[2].x, st[2].y, st[2].z);
    fr.bit = mk(st[3].x, st[3].y, st[3].z);
    CameraEntry e;
    e.r.o = fr.o;
    e.r.d = hemisphere_dir(fr, hemi_point_of(fp, q.xy[p].x, sample));
    e.bv = sample * 8049u + q.xy[p].bv;   // = rnd_base_v(sample, i, 0)
    e.bu = sample * 2683u + q.xy[p].bu;   // = rnd_base_u(sample, i, 0)
    return e;
}

// The sample queue's five geometry rows, the key (accel, geom, waves) that queue_size yields: X(ACCEL, GEOM, WAVES) per row,
// for the launchers' table (find_queue_row, pt_kernels.hip) and for the gather unit's (gather_queue_kernel, pt_gather.hip)
#define PT_QUEUE_ROWS(X) \
    X(false, 0, PT_Q_WAVES) X(false, 1, PT_Q_WAVES) X(true, 0, PT_Q_WAVES_SPHERE_BVH) X(true, 1, PT_Q_WAVES_ACCEL) X(true, 2, PT_Q_WAVES_ACCEL)

}  // namespace PT_NS
