// pt_samples_q_kernel.hpp — the text of the sample-queue kernel, included once per FORM of the kernel, inside the policy's
// namespace, after pt_queue.hpp and with PT_Q_LOOKAHEAD_FORM defined — forms 0 – 3 by pt_kernels.hip, form 4 by pt_gather.hip
// (and by nothing else):
//   0  pt_samples_q<COUNT, ACCEL, GEOM, WAVES, MOMENTS, COUNT_LOG2, CAM>, every instantiation there was
//   1  pt_samples_q_la<GEOM, WAVES>: the look-ahead form of the camera entry's ACCEL rows (CAM_LA; see pt_kernels.hip)
//   2  pt_samples_q_rays<ACCEL, GEOM, WAVES>: the camera entry fed from a ray buffer (RAYS; rt_render_rays) — the slots ARE
//      the ray indices, the staged record holds the ray itself, and a refill gathers no camera block and normalises nothing
//   3  pt_samples_q_raysets<ACCEL, GEOM, WAVES>: the ray form with a SET of records per ray (SETS; rt_render_ray_sets) —
//      nothing of a ray is staged but its index, and a refill loads the record of its own sample from global memory
//   4  pt_samples_q_hemi<ACCEL, GEOM, WAVES>: the ray-set form with the sets MADE from feature records (HEMI;
//      rt_render_hemispheres) — a slot is a record index and belongs to a wave only where the record has a hemisphere, its
//      frame is staged, and a refill makes the ray of its own sample in registers
// No include guard: it is meant to be read once per form.
#if PT_Q_LOOKAHEAD_FORM == 4
template <bool ACCEL, int GEOM, int WAVES>
__global__ __launch_bounds__(64, WAVES) void pt_samples_q_hemi(DeviceScene sc, FrameParams fp, const PixelRec *__restrict__ recs,
                                                         const uint32_t *__restrict__ live,
                                                         const uint32_t *__restrict__ live_count,
                                                         float4 *__restrict__ accum, unsigned long long *counters,
                                                         uint32_t pixels_per_wave) {
    constexpr bool COUNT = false, MOMENTS = false, CAM = true, CAM_LA = false, RAYS = true, SETS = false, HEMI = true;
    constexpr int COUNT_LOG2 = -1;
#elif PT_Q_LOOKAHEAD_FORM == 3
template <bool ACCEL, int GEOM, int WAVES>
__global__ __launch_bounds__(64, WAVES) void pt_samples_q_raysets(DeviceScene sc, FrameParams fp, const PixelRec *__restrict__ recs,
                                                            const uint32_t *__restrict__ live,
                                                            const uint32_t *__restrict__ live_count,
                                                            float4 *__restrict__ accum, unsigned long long *counters,
                                                            uint32_t pixels_per_wave) {
    constexpr bool COUNT = false, MOMENTS = false, CAM = true, CAM_LA = false, RAYS = true, SETS = true, HEMI = false;
    constexpr int COUNT_LOG2 = -1;
#elif PT_Q_LOOKAHEAD_FORM == 2
template <bool ACCEL, int GEOM, int WAVES>
__global__ __launch_bounds__(64, WAVES) void pt_samples_q_rays(DeviceScene sc, FrameParams fp, const PixelRec *__restrict__ recs,
                                                         const uint32_t *__restrict__ live,
                                                         const uint32_t *__restrict__ live_count,
                                                         float4 *__restrict__ accum, unsigned long long *counters,
                                                         uint32_t pixels_per_wave) {
    constexpr bool COUNT = false, MOMENTS = false, CAM = true, CAM_LA = false, RAYS = true, SETS = false, HEMI = false;
    constexpr int COUNT_LOG2 = -1;
#elif PT_Q_LOOKAHEAD_FORM == 1
template <int GEOM, int WAVES>
__global__ __launch_bounds__(64, WAVES) void pt_samples_q_la(DeviceScene sc, FrameParams fp, const PixelRec *__restrict__ recs,
                                                       const uint32_t *__restrict__ live,
                                                       const uint32_t *__restrict__ live_count,
                                                       float4 *__restrict__ accum, unsigned long long *counters,
                                                       uint32_t pixels_per_wave) {
    constexpr bool COUNT = false, ACCEL = true, MOMENTS = false, CAM = true, CAM_LA = true, RAYS = false, SETS = false, HEMI = false;
    constexpr int COUNT_LOG2 = -1;
#else
template <bool COUNT, bool ACCEL, int GEOM, int WAVES, bool MOMENTS = false, int COUNT_LOG2 = -1, bool CAM = false>
__global__ __launch_bounds__(64, WAVES) void pt_samples_q(DeviceScene sc, FrameParams fp, const PixelRec *__restrict__ recs,
                                                    const uint32_t *__restrict__ live,
                                                    const uint32_t *__restrict__ live_count,
                                                    float4 *__restrict__ accum, unsigned long long *counters,
                                                    uint32_t pixels_per_wave) {
    constexpr bool CAM_LA = false, RAYS = false, SETS = false, HEMI = false;
#endif
    extern __shared__ float4 s_dyn[];  // 16-byte aligned: no static LDS in this kernel
    // The tagged forms of sqrt and normalize (pt_arith.hpp) and the sphere scan that compares inside the root block
    // (pt_device.hpp sphere_take): this kernel without counters and without a BVH walk only — every other kernel, and
    // every other instantiation of this one, keeps the untagged code.
    constexpr bool FAST = PT_OCL && !COUNT && !ACCEL && GEOM != 2;
    // mixCol's min in its tagged form (pt_arith.hpp vmin<FAST>): the same family, without the ray forms, which keep their code
    constexpr bool MIN_FAST = PT_MIXCOL_FAST && FAST && !RAYS;
    // The carried state written where it is computed (PT_STATE_IN_PLACE, pt_device.hpp), the same family: scatter's arms
    // without the arm that leaves the direction alone (SIP_ARMS), and below the hit section under ONE test of "no hit",
    // with the colour a retiring lane returns in `out` (SIP_HIT: that lane's path colour is dead).
    constexpr bool SIP_ARMS = FAST && !RAYS && (PT_STATE_IN_PLACE & 1), SIP_HIT = FAST && !RAYS && (PT_STATE_IN_PLACE & 2);
    // The presence of the staged tables by count (pt_device.hpp has_materials): the instantiations that copy the staged block, in every policy.
    // (the ray form was written after that A/B was settled: it takes the settled form whatever the switch says, so the
    // switch keeps changing exactly the instantiations it changed — tests/test_loop_terms_host.py)
    constexpr bool BY_COUNT = (PT_TABLES_BY_COUNT || RAYS) && !COUNT && !ACCEL;
    // The table gathers by use (pt_device.hpp fetch_rnd_by_use): a lane reads randomVec's entry at a diffuse or textured vertex,
    // random's at a dielectric one, nothing at a mirror or a refractive one.  The same family, without the camera rows and
    // without meshes: GEOM 1 sits on its budget of 80 VGPRs and spills under policy 0 with the gathers in branches of their
    // own, and C3 gained nothing from them (profiles/r22_experiments.md).  The type that decides it is carried from where it
    // was last known (htype below), so the gathers do not wait for an LDS read.
    constexpr bool BY_USE = PT_RND_BY_USE && !PT_RNG_PREFETCH && !COUNT && !ACCEL && !CAM && GEOM == 0;
    // The wave's share of the live list first (two counters, read through the scalar cache): a wave that owns no pixel —
    // the launch is sized for "every pixel is live" unless the host knows better (launch_fused) — leaves here, before
    // anything is staged: no barrier, no sums, and only zeros to add to the counters.
    static_assert(!CAM || (!COUNT && !MOMENTS && COUNT_LOG2 < 0), "the camera entry has no counting, moment or count-specialised build");
    uint32_t pix0 = 0, npix = 0;
    uint32_t cam_x = 0, cam_y = 0;   // CAM: the pixel of this lane's slot, if the wave owns it
    bool cam_owns = false;
    unsigned long long cam_owners = 0;
    if (RAYS) {   // (slot = ray index: no tiles; cam_x carries it.  An adaptive round's mask is tested here: ray_active)
        cam_x = fp.slot_begin + blockIdx.x * pixels_per_wave + threadIdx.x;
        // (HEMI: slot = record index, owned where the record has a hemisphere; a gather launch has no mask)
        cam_owns = threadIdx.x < pixels_per_wave && cam_x < fp.slot_end &&
                   (HEMI ? hemisphere_valid(fp.feats + 5u * (size_t)cam_x) : ray_active(fp, cam_x));
        cam_owners = __ballot(cam_owns);
        npix = (uint32_t)__popcll(cam_owners);
    } else if (CAM) {
        const uint32_t slot = fp.slot_begin + blockIdx.x * pixels_per_wave + threadIdx.x;
        cam_owns = threadIdx.x < pixels_per_wave && slot < fp.slot_end && slot_to_pixel(fp, slot, cam_x, cam_y) && pixel_active(fp, cam_x, cam_y);
        cam_owners = __ballot(cam_owns);
        npix = (uint32_t)__popcll(cam_owners);
    } else {
        npix = live_take(fp, live_count, blockIdx.x, pixels_per_wave, pix0);
    }
    if (npix == 0u) return;
    float4 *s_mat = s_dyn;
    LaneCounters cn;
    if (COUNT) zero_counters(cn);
    // (without counters and without a BVH walk: the tables by copy from the context's staged block — launch_fused built it)
    Ctx c{sc, PT_STAGE_COPY && !COUNT && !ACCEL ? stage_materials_copy(sc, s_mat) : stage_materials(sc, s_mat), &cn};
    c.lwin = staged_winners(sc, s_mat);
    c.lpln = staged_planes(sc, s_mat);
    if (GEOM != 0 && fp.lds_face_f4) {   // the face records of a scene of a few small meshes (hit_models' candidate loop)
        float4 *s_faces = s_dyn + queue_faces_f4(sc);
        for (uint32_t i = threadIdx.x; i < fp.lds_face_f4; i += blockDim.x) s_faces[i] = sc.faces[i];
        __syncthreads();
        c.lfaces = lds_ptr(s_faces);
    }

    const WaveQueue q = HEMI ? queue_stage_hemi(sc, fp, cam_owns, cam_x, cam_owners, pixels_per_wave, s_dyn, GEOM != 0 ? fp.lds_face_f4 : 0u)
                      : SETS ? queue_stage_raysets(sc, fp, cam_owns, cam_x, cam_owners, pixels_per_wave, s_dyn, GEOM != 0 ? fp.lds_face_f4 : 0u)
                      : RAYS ? queue_stage_rays(sc, fp, cam_owns, cam_x, cam_owners, pixels_per_wave, s_dyn, GEOM != 0 ? fp.lds_face_f4 : 0u)
                      : CAM ? queue_stage_cam(sc, fp, cam_owns, cam_x, cam_y, cam_owners, pixels_per_wave, s_dyn, GEOM != 0 ? fp.lds_face_f4 : 0u)
                            : queue_stage<COUNT_LOG2, !COUNT && !ACCEL>(sc, fp, recs, live, npix, pix0, pixels_per_wave, s_dyn, GEOM != 0 ? fp.lds_face_f4 : 0u);

    uint32_t next = 0;  // wave-uniform head of the queue
    bool active = false;
    bool fresh = false;  // CAM: the lane stands at the camera — no interaction before its first nearest-hit search
    // Per-lane state carried from one iteration to the next, kept small (the kernel sits on its VGPR budget):
    // the hit POINT is not carried — the ray's origin is moved there as soon as the hit is known — and the
    // per-sample part of the table index sums is precomputed (bv, bu) instead of carrying sample, x and y.
    uint32_t idx = 0, depth = 0, bv = 0, bu = 0;
    V3 col = mk(0.0f, 0.0f, 0.0f), out = mk(0.0f, 0.0f, 0.0f);   // col: material colour or texel of the hit
    Ray r;
    r.o = r.d = mk(0.0f, 0.0f, 0.0f);
    V3 hn = mk(0.0f, 0.0f, 0.0f);   // normal and material of the hit the next interaction happens at
    uint32_t hmat = 0;
    uint32_t htype = 0;   // BY_USE: the type of that material (the hit section has read it for the light test; a record holds it)
    Rnd rnd;
    rnd.v = mk(0.0f, 0.0f, 0.0f);
    rnd.u = 0.0f;

#if PT_STAMPS
    c.st_last = __builtin_amdgcn_s_memtime();
#endif
    while (true) {
        PT_STAMP(c, 5);
        // ---- refill idle lanes from the queue
        bool need = !active;
        unsigned long long m = __ballot(need);
        // refill when enough lanes idle (or none is active): the refill step issues for the whole wave
        if (m && next < q.total && ((uint32_t)__popcll(m) >= PT_REFILL_MIN || m == ~0ull)) {
            uint32_t cand = next + lanes_below(m);
            if (CAM) {
                if (need && cand < q.total) {
                    idx = cand;
                    const CameraEntry e = HEMI ? queue_fetch_hemi(q, fp, idx) : SETS ? queue_fetch_raysets(q, fp, idx) : RAYS ? queue_fetch_rays(q, fp, idx) : queue_fetch_cam(q, fp, idx);
                    bv = e.bv;
                    bu = e.bu;
                    depth = 0u;
                    r = e.r;
                    out = mk(1.0f, 1.0f, 1.0f);
                    if (PT_RNG_PREFETCH) rnd = fetch_rnd_b(sc.table, r.d, depth, bv, bu);
                    active = true;
                    fresh = true;
                }
            } else
            if (need && cand < q.total) {
                idx = cand;
                const QueueEntry e = queue_fetch<COUNT_LOG2>(q, sc, fp, idx);
                bv = e.bv;
                bu = e.bu;
                if (COUNT) cn.c[CN_SAMPLES]++;
                // the state of an idle lane is dead: it takes the record whatever its kind, so that the registers are
                // written in place (a final colour's lane stays idle and its state is never read)
                depth = (e.bits >> 8) & 0xFFu;   // (type and extra_data of the record are the material's: re-read below)
                hn = xyz(e.q1);
                r.o = xyz(e.q0);
                r.d = xyz(e.q2);
                hmat = __float_as_uint(e.q2.w);
                if (BY_USE) htype = e.bits >> 16;   // (a vertex record holds its material's type, trace_branch)
                out = xyz(e.q3);
                col = xyz(e.q4);
                if ((e.bits & 0xFFu) == REC_FINAL) {  // a leaf of a tree, or count is not a multiple of g
                    queue_put(q, idx, out);
                } else {
                    if (PT_RNG_PREFETCH) rnd = fetch_rnd_b(sc.table, r.d, depth, bv, bu);
                    active = true;
                }
            }
            next += (uint32_t)__popcll(m);
        }
        if (!__any(active) && next >= q.total) break;
        PT_STAMP(c, 0);
#ifdef PT_EXP_PAD  // timing experiment (tools/pad_experiment.sh): PT_EXP_PAD extra full-rate VALU instructions per iteration
                   // (v_or_b32 x, x, x on a live register: no new VGPR; PT_EXP_PAD_NOP: operand-free v_nop instead).  An
                   // issue-bound loop slows down by their issue time, a latency-bound one does not (profiles/r03_experiments.md)
#define PT_STR2(x) #x
#define PT_STR(x) PT_STR2(x)
#ifdef PT_EXP_PAD_NOP
        asm volatile(".rept " PT_STR(PT_EXP_PAD) "\n\tv_nop\n\t.endr");
#else
        asm volatile(".rept " PT_STR(PT_EXP_PAD) "\n\tv_or_b32 %0, %0, %0\n\t.endr" : "+v"(idx));
#endif
#endif
#ifdef PT_QSTAT  // diagnostic: lane-iterations used / offered (read through rt_get_debug_counters on a BVH-free scene)
        if (COUNT && __any(active)) {   // (an iteration that only refilled final colours is not offered)
            uint32_t na = (uint32_t)__popcll(__ballot(active));
            if (threadIdx.x == 0) cn.c[CN_DBG_BVH_NODES] += na;
            if (threadIdx.x == 0) cn.c[CN_DBG_BVH_TESTS] += 64u;
        }
#endif
        // ---- one material interaction for every active lane
        if (CAM ? active && !fresh : active) {
            if (!PT_RNG_PREFETCH && !BY_USE) rnd = fetch_rnd_b(sc.table, r.d, depth, bv, bu);
            Hit at;   // the vertex this interaction happens at: the ray's origin already stands on it
            at.p = r.o;
            at.n = hn;
            at.u = at.v = 0.0f;
            at.tex = 0;
            at.mat = hmat;
            int type;
            float extra;
            V3 mcol;
            if (BY_USE) fetch_rnd_by_use(rnd, sc.table, r.d, (int)htype, depth, bv, bu);
            load_material<BY_COUNT>(c, hmat, type, extra, mcol);   // extra_data is not carried, nor the type without BY_USE: one LDS read each
            if (BY_USE) type = (int)htype;   // (the same value, and the type's LDS read goes)
            scatter<COUNT, FAST, BY_COUNT, MIN_FAST, SIP_ARMS>(c, r, out, at, type, extra, col, rnd, false);
            depth++;
            if (depth >= RT_DEPTH) {  // survived DEPTH bounces: returns what it has (:447,485)
                queue_put(q, idx, out);
                active = false;
            }
        }
        if (CAM) fresh = false;
        PT_STAMP(c, 1);
        // ---- nearest hit for every lane still active; the table reads of the NEXT material
        // interaction are issued first (they depend on the ray direction only)
        if (active) {
            if (PT_RNG_PREFETCH == 1) rnd = fetch_rnd_b(sc.table, r.d, depth, bv, bu);
            V3 res;   // what a retiring lane returns (SIP_HIT: in `out`, that lane's path colour being dead)
            bool done = false;
            Hit h;   // (every field is written by hit_finish on a hit, and read only then)
            Nearest nb;
            hit_primitives<COUNT, ACCEL, GEOM != 0, FAST>(c, r, nb);
            if (GEOM != 0) hit_models<COUNT, GEOM == 2>(c, r, nb);
            // (SIP_HIT: the test hit_finish makes, made here first — the hit's state is then computed and stored under one
            // condition, not under two equal ones with the miss between them, across which it lived in registers of its own)
            if ((SIP_HIT && nb.id == PT_NO_HIT) || !hit_finish<COUNT, GEOM == 0, BY_COUNT>(c, r, nb, h)) {
                if (SIP_HIT) out = mk(0.0f, 0.0f, 0.0f);
                else res = mk(0.0f, 0.0f, 0.0f);
                done = true;
            } else {
                if (COUNT) cn.c[CN_H_BOUNCE]++;
                // the next interaction happens here (for a light the lane retires below and this state is dead):
                // written in the branch that computed it, so that the registers are updated in place
                r.o = h.p;
                hn = h.n;
                hmat = h.mat;
                int type;
                float extra;
                load_material<BY_COUNT>(c, h.mat, type, extra, col);
                if (BY_USE) htype = (uint32_t)type;
                if (type == RT_LIGHT) {
                    if (SIP_HIT) out = vmin<MIN_FAST>(out, col);
                    else res = vmin<MIN_FAST>(out, col);
                    done = true;
                } else if (type == RT_TEXTURED) {
                    if (COUNT) cn.c[CN_N_TEXFETCH]++;
                    float tu = h.u, tv = h.v;
                    // (GEOM 0: hit_finish leaves u = v = 0 and layer 0, constants — the texel's address arithmetic, four
                    // 64-bit addresses and four weights, was lifted to the kernel's entry and carried through the loop in
                    // 11 VGPRs, for a branch C2 never takes; opaque to the optimiser, the same operations stay in here)
                    // (Nothing but the compiler's present cost model keeps LICM from lifting the asm together with what hangs
                    // on it — it is not volatile and its inputs are loop-invariant: tools/isa_stats.py shows it, as a GEOM 0
                    // kernel back at 71 VGPRs.)
                    if (PT_TEXEL_LAZY && GEOM == 0 && !COUNT && !ACCEL) asm("" : "+v"(tu), "+v"(tv));
                    col = texture_rgb(c.sc, tu, tv, h.tex);
                }
            }
            if (done) {
                queue_put(q, idx, SIP_HIT ? out : res);
                active = false;
            } else if (PT_RNG_PREFETCH == 2) {
                // this lane WILL interact next iteration: its table reads fly during the refill step
                rnd = fetch_rnd_b(sc.table, r.d, depth, bv, bu);
            }
        }
        PT_STAMP(c, 4);
    }
#if PT_STAMPS
    if (threadIdx.x == 0 && q.npix)
        for (int k = 0; k < 6; k++) atomicAdd(&counters[(size_t)COUNTER_REPLICAS * COUNTER_STRIDE + k], c.st[k]);
#endif
    static_assert(!CAM_LA || (CAM && ACCEL), "the look-ahead kernels of the camera entry's ACCEL rows");
    // (wave-uniform: a look-ahead launch; never a counting one, never with moments; of the camera rows those without a BVH walk)
    constexpr bool LA_BRANCH = CAM ? !ACCEL : !COUNT && !MOMENTS;
    if (CAM_LA || (!RAYS && LA_BRANCH && fp.la_ring)) queue_replay<CAM>(q, fp);   // (a ray launch is never a look-ahead launch)
    // (the two COUNT_LOG2 = 6 kernels may be launched on a cleared frame: FrameParams::store.  The generic-count kernels keep
    // the add: with the second arm behind its loop C3's kernel at 256 samples measured 0.5 % slower, profiles/r32_experiments.md)
    else queue_sums<MOMENTS, COUNT || ACCEL, COUNT_LOG2, PT_Q_LOOKAHEAD_FORM == 0 && !COUNT && !ACCEL && !MOMENTS && !CAM && COUNT_LOG2 == 6>(q, fp, accum);
    flush_counters<COUNT>(cn, counters, 1);
}
