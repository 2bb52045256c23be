// scene_prep.hpp — everything rt_set_scene computes on the host before it uploads, and the self-check of exactly that.
// Host only: no HIP runtime call and no rt_context, just the vector types (as mesh_bvh_build.hpp); compiles with a plain
// C++17 compiler given -D__HIP_PLATFORM_AMD__ and ROCm's include directory (tests/host/scene_prep_main.cpp).
//   prepare_scene   validates a scene description and builds the face records, the per-mesh BVHs (one node array,
//                   collapsed links, 48-byte packing), the walk jobs and the sphere BVH in its device layout;
//   check_prepared  verifies the invariants of those structures (rt_debug_check_accel);
//   scene_digest    FNV-1a-64 over what is uploaded.
#pragma once
#include <hip/hip_vector_types.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/rt_amd.h"
#include "mesh_bvh_build.hpp"

#ifndef MESH_BVH_MIN_FACES
#define MESH_BVH_MIN_FACES 32   // (rt_context.hpp carries the same guarded definition for the launch planner)
#endif
#ifndef SPHERE_BVH_LEAF
#define SPHERE_BVH_LEAF 4  // spheres per leaf (<= 7)
#endif
#define BVH_END 0x0FFFFFFFu
#define BVH_ROOT 1u

namespace scene_prep {

constexpr uint32_t MESH_ROOT_NONE = 0xFFFFFFFFu;   // = PT_MESH_BVH_NONE (pt_types.hpp): the mesh has no BVH (face scan)

// Sphere BVH (see hit_spheres_bvh): binned surface-area-heuristic splits (16 bins per axis over the
// centroids; median split when no bin boundary separates them), leaves of <= 4 spheres; children
// are allocated in adjacent pairs (left at an even index, lower coordinates along the split axis),
// every node records its split axis and, per direction octant, the node that follows its subtree in the
// near-before-far order of that octant (the walk is threaded: no stack, no way back up).
struct BvhBuild {
    const rt_sphere *sph;
    std::vector<uint32_t> order;
    std::vector<float4> nodes;   // 4 per node: (lo, A) (hi, B) and the eight skip links (pt_device.hpp hit_spheres_bvh)
    std::vector<float4> leaf_sph;
    std::vector<uint32_t> leaf_idx;

    void bounds(uint32_t b, uint32_t e, float lo[3], float hi[3]) const {
        for (int k = 0; k < 3; k++) { lo[k] = INFINITY; hi[k] = -INFINITY; }
        for (uint32_t i = b; i < e; i++) {
            const rt_sphere &s = sph[order[i]];
            const float c[3] = {s.pos.x, s.pos.y, s.pos.z};
            float r = std::fabs(s.r);
            for (int k = 0; k < 3; k++) {
                lo[k] = std::fmin(lo[k], c[k] - r);
                hi[k] = std::fmax(hi[k], c[k] + r);
            }
        }
    }
    // skip[o]: the node that follows this subtree for a ray of direction octant o (bit k of o: d_k < 0), whose walk
    // enters the nearer child of every inner node first; BVH_END after the last one
    void fill(uint32_t me, const uint32_t skip[8], uint32_t b, uint32_t e, uint32_t depth = 0) {
        float lo[3], hi[3];
        bounds(b, e, lo, hi);
        uint32_t A = 0, B;
        if (e - b <= SPHERE_BVH_LEAF) {
            uint32_t first = (uint32_t)leaf_sph.size();
            for (uint32_t i = b; i < e; i++) {
                const rt_sphere &s = sph[order[i]];
                volatile float r2 = s.r * s.r;
                leaf_sph.push_back(make_float4(s.pos.x, s.pos.y, s.pos.z, r2));
                leaf_idx.push_back(order[i]);
            }
            B = 0x80000000u | ((e - b) << 28) | first;
        } else {
            float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (uint32_t i = b; i < e; i++) {
                const rt_sphere &s = sph[order[i]];
                const float c[3] = {s.pos.x, s.pos.y, s.pos.z};
                for (int k = 0; k < 3; k++) { clo[k] = std::fmin(clo[k], c[k]); chi[k] = std::fmax(chi[k], c[k]); }
            }
            int ax = 0;
            for (int k = 1; k < 3; k++) if (chi[k] - clo[k] > chi[ax] - clo[ax]) ax = k;
            uint32_t mid = b + (e - b) / 2;
            const rt_sphere *sp = sph;
            // binned SAH: cost(split) = area(L)·|L| + area(R)·|R| over 15 boundaries × 3 axes
            constexpr int NB = 16;
            double best_cost = INFINITY;
            int best_ax = -1, best_bin = -1;
            for (int k = 0; k < 3 && depth < 32u; k++) {   // (median splits from level 32 on bound the depth)
                float ext = chi[k] - clo[k];
                if (!(ext > 0.0f)) continue;
                struct Bin { float lo[3], hi[3]; uint32_t n; } bins[NB];
                for (auto &bn : bins) { for (int q = 0; q < 3; q++) { bn.lo[q] = INFINITY; bn.hi[q] = -INFINITY; } bn.n = 0; }
                for (uint32_t i = b; i < e; i++) {
                    const rt_sphere &s = sph[order[i]];
                    const float c[3] = {s.pos.x, s.pos.y, s.pos.z};
                    int bi = (int)((c[k] - clo[k]) / ext * NB);
                    bi = bi < 0 ? 0 : (bi >= NB ? NB - 1 : bi);
                    float r = std::fabs(s.r);
                    for (int q = 0; q < 3; q++) { bins[bi].lo[q] = std::fmin(bins[bi].lo[q], c[q] - r); bins[bi].hi[q] = std::fmax(bins[bi].hi[q], c[q] + r); }
                    bins[bi].n++;
                }
                auto area = [](const float *l, const float *h) {
                    double dx = (double)h[0] - l[0], dy = (double)h[1] - l[1], dz = (double)h[2] - l[2];
                    return dx < 0 ? 0.0 : 2.0 * (dx * dy + dy * dz + dz * dx);
                };
                double right_cost[NB];
                float rl[3] = {INFINITY, INFINITY, INFINITY}, rh[3] = {-INFINITY, -INFINITY, -INFINITY};
                uint32_t rn = 0;
                for (int j = NB - 1; j > 0; j--) {
                    for (int q = 0; q < 3; q++) { rl[q] = std::fmin(rl[q], bins[j].lo[q]); rh[q] = std::fmax(rh[q], bins[j].hi[q]); }
                    rn += bins[j].n;
                    right_cost[j] = rn ? area(rl, rh) * rn : INFINITY;
                }
                float ll[3] = {INFINITY, INFINITY, INFINITY}, lh[3] = {-INFINITY, -INFINITY, -INFINITY};
                uint32_t ln = 0;
                for (int j = 0; j < NB - 1; j++) {
                    for (int q = 0; q < 3; q++) { ll[q] = std::fmin(ll[q], bins[j].lo[q]); lh[q] = std::fmax(lh[q], bins[j].hi[q]); }
                    ln += bins[j].n;
                    if (ln == 0 || ln == e - b) continue;
                    double cost = area(ll, lh) * ln + right_cost[j + 1];
                    if (cost < best_cost) { best_cost = cost; best_ax = k; best_bin = j; }
                }
            }
            if (best_ax >= 0) {
                ax = best_ax;
                float ext = chi[ax] - clo[ax], base = clo[ax];
                int bb = best_bin;
                auto it = std::partition(order.begin() + b, order.begin() + e, [sp, ax, ext, base, bb](uint32_t i) {
                    const float *ci = &sp[i].pos.x;
                    int bi = (int)((ci[ax] - base) / ext * NB);
                    bi = bi < 0 ? 0 : (bi >= NB ? NB - 1 : bi);
                    return bi <= bb;
                });
                mid = (uint32_t)(it - order.begin());
            }
            if (best_ax < 0 || mid == b || mid == e) {  // coincident centroids: median split by index
                mid = b + (e - b) / 2;
                std::nth_element(order.begin() + b, order.begin() + mid, order.begin() + e, [sp, ax](uint32_t i, uint32_t j) {
                    const float *ci = &sp[i].pos.x, *cj = &sp[j].pos.x;
                    return ci[ax] < cj[ax] || (ci[ax] == cj[ax] && i < j);
                });
            }
            uint32_t left = (uint32_t)(nodes.size() / 4);  // even: the root is node 1 and pairs follow, each in one 64-byte stretch
            nodes.resize(nodes.size() + 8);
            A = (uint32_t)ax << 28;
            B = left;
            uint32_t skip_l[8], skip_r[8];
            for (uint32_t o = 0; o < 8; o++) {   // the walk enters child B + ((o >> ax) & 1) first, its sibling next
                bool right_first = ((o >> ax) & 1u) != 0;
                skip_l[o] = right_first ? skip[o] : left + 1u;
                skip_r[o] = right_first ? left : skip[o];
            }
            fill(left, skip_l, b, mid, depth + 1u);
            fill(left + 1, skip_r, mid, e, depth + 1u);
        }
        float bc[3], bh[3];
        bvh_centre_half(lo, hi, bc, bh);
        nodes[4 * (size_t)me] = make_float4(bc[0], bc[1], bc[2], 0.0f);
        nodes[4 * (size_t)me + 1] = make_float4(bh[0], bh[1], bh[2], 0.0f);
        memcpy(&nodes[4 * (size_t)me].w, &A, 4);
        memcpy(&nodes[4 * (size_t)me + 1].w, &B, 4);
        memcpy(&nodes[4 * (size_t)me + 2], skip, 32);
    }
    void build(uint32_t b, uint32_t e) {
        nodes.assign(8, make_float4(0.0f, 0.0f, 0.0f, 0.0f));   // node 0 is padding, the root is node BVH_ROOT
        const uint32_t end[8] = {BVH_END, BVH_END, BVH_END, BVH_END, BVH_END, BVH_END, BVH_END, BVH_END};
        fill(BVH_ROOT, end, b, e);
    }
};

// per-face records (see DeviceScene::faces): the same binary32 operations hitTriangle performs.
// base[m] = first record of mesh m; fr = 3 float4 per face + one dummy record.
inline bool build_face_records(const rt_scene_desc *d, std::vector<uint32_t> &base, std::vector<float4> &fr) {
    base.assign(d->mesh_count ? d->mesh_count : 1, 0u);
    size_t total = 0;
    for (uint32_t m = 0; m < d->mesh_count; m++) { base[m] = (uint32_t)total; total += d->meshes[m].face_count; }
    if (total >= (1ull << 31)) return false;
    fr.assign(3 * (total + 1), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t m = 0; m < d->mesh_count; m++) {
        const rt_mesh &me = d->meshes[m];
        for (uint32_t f = 0; f < me.face_count; f++) {
            const uint32_t *ib = d->indices + me.index_anchor + 3u * f;
            const rt_float3 &A = d->vertices[me.vertex_anchor + ib[0]], &B = d->vertices[me.vertex_anchor + ib[1]],
                            &C = d->vertices[me.vertex_anchor + ib[2]];
            volatile float e1x = B.x - A.x, e1y = B.y - A.y, e1z = B.z - A.z;
            volatile float e2x = C.x - A.x, e2y = C.y - A.y, e2z = C.z - A.z;
            volatile float p1 = e1y * e2z, p2 = e1z * e2y, p3 = e1z * e2x, p4 = e1x * e2z, p5 = e1x * e2y, p6 = e1y * e2x;
            volatile float cx = p1 - p2, cy = p3 - p4, cz = p5 - p6;          // cross(e1, e2)
            volatile float xx = cx * cx, yy = cy * cy, zz = cz * cz;
            volatile float s2 = xx + yy;
            volatile float s3 = s2 + zz;                                        // dot = (x*x + y*y) + z*z
            volatile float len = std::sqrt((float)s3);
            volatile float nx = cx / len, ny = cy / len, nz = cz / len;          // normalize
            float4 *q = &fr[3 * ((size_t)base[m] + f)];
            q[0] = make_float4(A.x, A.y, A.z, e1x);
            q[1] = make_float4(e1y, e1z, e2x, e2y);
            q[2] = make_float4(e2z, nx, ny, nz);
        }
    }
    return true;
}

// What rt_set_scene uploads or keeps in the context, as the host computes it.  Every vector is uploaded whole (the
// placeholders of a scene without mesh BVHs included: one zero node, one zero leaf record).
struct PreparedScene {
    std::vector<uint32_t> face_base;       // per mesh: its first face record
    std::vector<float4> faces;             // 3 per face + one dummy record; normals as arithmetic policy 0 has them
    std::vector<uint32_t> mesh_roots;      // per mesh: its root in mesh_nodes, or MESH_ROOT_NONE
    std::vector<float4> mesh_nodes;        // all trees, 4 float4 per node as MeshBvhBuilder writes them, links collapsed …
    std::vector<float4> mesh_packed;       // … and their 48-byte device form (mesh_node_pack)
    std::vector<uint2> mesh_built_links;   // per node: its (A, B) words before mesh_collapse_links (check_prepared only)
    std::vector<float4> leaf_faces;        // 3 per leaf slot
    std::vector<uint32_t> leaf_face_idx;   // per leaf slot: the face's index within its mesh
    bool have_mesh_bvh = false;
    std::vector<uint2> walk_jobs;          // (mesh, model material) in hit order; empty unless every model mesh has a BVH and they number < 2^16
    // sphere BVH; all empty where none is built (no sphere, a non-finite sphere, >= 2^24 spheres)
    std::vector<float4> sphere_nodes;      // 4 per node as BvhBuild writes them
    std::vector<float4> sphere_boxes;      // device layout (hit_spheres_bvh): (centre, B) per node …
    std::vector<float4> sphere_links;      // … and per node and octant (skip | axis << 28, half extent)
    std::vector<uint32_t> sphere_leaf_idx;
    uint32_t bvh_node_count = 0;           // 0 also where the tree outgrows the walk's 32-bit byte offsets
    float bvh_lo[3] = {0, 0, 0}, bvh_hi[3] = {0, 0, 0}, bvh_rmax = 0;   // bounds of the centres, largest |r| (with a tree)
    bool uses_tex = false;
    uint32_t max_tex = 0;
};

inline int prep_fail(std::string &err, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

// every pointer and index the builders and the kernels dereference; → uses_tex, max_tex
inline int validate_scene(const rt_scene_desc *d, bool &uses_tex, uint32_t &max_tex, std::string &err) {
    struct { const void *p; uint32_t n; const char *name; } arrs[] = {
        {d->materials, d->material_count, "materials"}, {d->spheres, d->sphere_count, "spheres"},
        {d->planes, d->plane_count, "planes"}, {d->lenses, d->lens_count, "lenses"},
        {d->vertices, d->vertex_count, "vertices"}, {d->uvs, d->uv_count, "uvs"},
        {d->indices, d->index_count, "indices"}, {d->meshes, d->mesh_count, "meshes"},
        {d->models, d->model_count, "models"}};
    for (auto &a : arrs)
        if (a.n && !a.p) return prep_fail(err, RT_EINVAL, "%s: count %u but NULL pointer", a.name, a.n);
    if (d->uv_count != 0 && d->uv_count != d->vertex_count)
        return prep_fail(err, RT_EINVAL, "uv_count (%u) must be 0 or vertex_count (%u)", d->uv_count, d->vertex_count);
    // validate every index the kernels dereference
    for (uint32_t i = 0; i < d->material_count; i++)
        if (d->materials[i].type < 0 || d->materials[i].type > RT_LIGHT)
            return prep_fail(err, RT_EINVAL, "material %u has unknown type %d", i, d->materials[i].type);
    for (uint32_t i = 0; i < d->sphere_count; i++)
        if (d->spheres[i].mat_ID >= d->material_count) return prep_fail(err, RT_ERANGE, "sphere %u: material %u does not exist", i, d->spheres[i].mat_ID);
    for (uint32_t i = 0; i < d->plane_count; i++)
        if (d->planes[i].mat_ID >= d->material_count) return prep_fail(err, RT_ERANGE, "plane %u: material %u does not exist", i, d->planes[i].mat_ID);
    for (uint32_t i = 0; i < d->lens_count; i++)
        if (d->lenses[i].mat_ID >= d->material_count) return prep_fail(err, RT_ERANGE, "lens %u: material %u does not exist", i, d->lenses[i].mat_ID);
    uses_tex = false;
    max_tex = 0;
    for (uint32_t i = 0; i < d->model_count; i++) {
        const rt_model &mo = d->models[i];
        if (mo.mat_ID >= d->material_count) return prep_fail(err, RT_ERANGE, "model %u: material %u does not exist", i, mo.mat_ID);
        if ((uint64_t)mo.mesh_anchor + mo.mesh_count > d->mesh_count) return prep_fail(err, RT_ERANGE, "model %u: meshes [%u,+%u) outside the mesh array (%u)", i, mo.mesh_anchor, mo.mesh_count, d->mesh_count);
        bool textured = d->materials[mo.mat_ID].type == RT_TEXTURED;
        for (uint32_t k = 0; k < mo.mesh_count; k++) {
            const rt_mesh &me = d->meshes[mo.mesh_anchor + k];
            if (textured) {
                uses_tex = true;
                if (me.texture_ID > max_tex) max_tex = me.texture_ID;
            }
        }
    }
    for (uint32_t i = 0; i < d->mesh_count; i++) {
        const rt_mesh &me = d->meshes[i];
        if ((uint64_t)me.index_anchor + 3ull * me.face_count > d->index_count)
            return prep_fail(err, RT_ERANGE, "mesh %u: indices [%u,+3*%u) outside the index array (%u)", i, me.index_anchor, me.face_count, d->index_count);
        for (uint64_t k = 0; k < 3ull * me.face_count; k++)
            if ((uint64_t)me.vertex_anchor + d->indices[me.index_anchor + k] >= d->vertex_count)
                return prep_fail(err, RT_ERANGE, "mesh %u: vertex index %u (+anchor %u) outside the vertex array (%u)", i, d->indices[me.index_anchor + k], me.vertex_anchor, d->vertex_count);
    }
    return RT_OK;
}

inline int prepare_scene(const rt_scene_desc &scene, PreparedScene &ps, std::string &err) {
    const rt_scene_desc *d = &scene;
    ps = PreparedScene();
    if (int rc = validate_scene(d, ps.uses_tex, ps.max_tex, err)) return rc;
    if (!build_face_records(d, ps.face_base, ps.faces)) return prep_fail(err, RT_EINVAL, "too many faces");
    {
        const std::vector<uint32_t> &base = ps.face_base;
        const std::vector<float4> &fr = ps.faces;
        // per-mesh BVHs for the "first front-facing hit in face order" rule (pt_mesh_bvh.hpp)
        std::vector<float4> &nodes = ps.mesh_nodes, &lfaces = ps.leaf_faces;
        std::vector<uint32_t> &lidx = ps.leaf_face_idx, &roots = ps.mesh_roots;
        roots.assign(d->mesh_count ? d->mesh_count : 1, MESH_ROOT_NONE);
        for (uint32_t m = 0; m < d->mesh_count; m++) {
            if (d->meshes[m].face_count < MESH_BVH_MIN_FACES || d->meshes[m].face_count >= (1u << 27)) continue;
            MeshBvhBuilder mb;
            mb.rec = &fr[3 * (size_t)base[m]];
            mb.n_faces = d->meshes[m].face_count;
            mb.nodes = &nodes;
            mb.leaf_faces = &lfaces;
            mb.leaf_idx = &lidx;
            roots[m] = mb.build();
            ps.have_mesh_bvh = true;
        }
        // the walks address these arrays with 32-bit byte offsets (at32): everything below 4 GiB, node indices below 2^26
        if (nodes.size() / 4 >= (1u << 26) || lidx.size() >= (1u << 26)) ps.have_mesh_bvh = false;
        if (nodes.empty()) nodes.resize(4, make_float4(0, 0, 0, 0));
        if (lfaces.empty()) lfaces.resize(3, make_float4(0, 0, 0, 0));
        {   // device layout: 48 bytes per node (mesh_node_pack), wide-cone inner nodes spliced out of the links
            ps.mesh_built_links.resize(nodes.size() / 4);
            for (size_t n = 0; n < nodes.size() / 4; n++) {
                memcpy(&ps.mesh_built_links[n].x, &nodes[4 * n].w, 4);
                memcpy(&ps.mesh_built_links[n].y, &nodes[4 * n + 1].w, 4);
            }
            std::vector<uint8_t> is_root(nodes.size() / 4, 0);
            for (uint32_t m = 0; m < d->mesh_count; m++) if (roots[m] != MESH_ROOT_NONE && roots[m] < is_root.size()) is_root[roots[m]] = 1;
            mesh_collapse_links(nodes, is_root);
            ps.mesh_packed.resize(nodes.size() / 4 * 3);
            for (size_t n = 0; n < nodes.size() / 4; n++) mesh_node_pack(&nodes[4 * n], &ps.mesh_packed[3 * n]);
        }
        std::vector<uint2> jobs;
        bool all_bvh = ps.have_mesh_bvh && d->model_count > 0;
        for (uint32_t mo = 0; mo < d->model_count && all_bvh; mo++)
            for (uint32_t k = 0; k < d->models[mo].mesh_count && all_bvh; k++) {
                uint32_t mi = d->models[mo].mesh_anchor + k;
                all_bvh = mi < d->mesh_count && roots[mi] != MESH_ROOT_NONE;
                jobs.push_back(make_uint2(mi, d->models[mo].mat_ID));
            }
        if (all_bvh && !jobs.empty() && jobs.size() < (1u << 16)) ps.walk_jobs.swap(jobs);
        ps.face_base.resize(d->mesh_count);   // (both were built with one element for a scene without meshes)
        ps.mesh_roots.resize(d->mesh_count);
    }
    if (d->sphere_count > 0 && d->sphere_count < (1u << 24)) {   // (32-bit byte offsets into the node / link / leaf arrays: at32; a node's links are 128 bytes)
        bool finite = true;
        for (uint32_t i = 0; i < d->sphere_count && finite; i++)
            finite = std::isfinite(d->spheres[i].pos.x) && std::isfinite(d->spheres[i].pos.y) &&
                     std::isfinite(d->spheres[i].pos.z) && std::isfinite(d->spheres[i].r);
        if (finite) {  // non-finite spheres: no BVH, the brute-force loop handles them as the reference does
            BvhBuild bb;
            bb.sph = d->spheres;
            bb.order.resize(d->sphere_count);
            for (uint32_t i = 0; i < d->sphere_count; i++) bb.order[i] = i;
            bb.build(0, d->sphere_count);
            {   // device layout (hit_spheres_bvh): (centre, B) in 16 bytes; per octant (skip | axis << 28, half extent) in 16 bytes
                std::vector<float4> &boxes = ps.sphere_boxes, &links = ps.sphere_links;
                boxes.resize(bb.nodes.size() / 4);
                links.resize(bb.nodes.size() * 2);
                for (size_t n = 0; n < bb.nodes.size() / 4; n++) {
                    boxes[n] = bb.nodes[4 * n];
                    boxes[n].w = bb.nodes[4 * n + 1].w;
                    uint32_t A, s8[8];
                    memcpy(&A, &bb.nodes[4 * n].w, 4);
                    memcpy(s8, &bb.nodes[4 * n + 2], 32);
                    for (int o = 0; o < 8; o++) {
                        const uint32_t w = s8[o] | (A & 0x30000000u);
                        float4 &l = links[8 * n + o];
                        l = make_float4(0.0f, bb.nodes[4 * n + 1].x, bb.nodes[4 * n + 1].y, bb.nodes[4 * n + 1].z);
                        memcpy(&l.x, &w, 4);
                    }
                }
            }
            // the walk addresses the link array with the 32-bit byte offset node << 7 and leaf slots with slot << 4
            // (at32): a degenerate set whose tree outgrows that takes the brute-force loop
            ps.bvh_node_count = (bb.nodes.size() / 4 < (1u << 25) && bb.leaf_sph.size() < (1u << 28)) ? (uint32_t)(bb.nodes.size() / 4) : 0u;
            ps.bvh_rmax = 0;
            for (int k = 0; k < 3; k++) { ps.bvh_lo[k] = INFINITY; ps.bvh_hi[k] = -INFINITY; }
            for (uint32_t i = 0; i < d->sphere_count; i++) {
                const float c[3] = {d->spheres[i].pos.x, d->spheres[i].pos.y, d->spheres[i].pos.z};
                for (int k = 0; k < 3; k++) { ps.bvh_lo[k] = std::fmin(ps.bvh_lo[k], c[k]); ps.bvh_hi[k] = std::fmax(ps.bvh_hi[k], c[k]); }
                ps.bvh_rmax = std::fmax(ps.bvh_rmax, std::fabs(d->spheres[i].r));
            }
            ps.sphere_nodes.swap(bb.nodes);
            ps.sphere_leaf_idx.swap(bb.leaf_idx);
        }
    }
    return RT_OK;
}

// FNV-1a-64 over the raw bytes of what rt_set_scene hands to upload() or keeps in the context for arithmetic policy 0,
// each array preceded by its element count as a little-endian uint64; the scalars last, as eleven 32-bit words.
struct Fnv64 {
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void *p, size_t n) {
        const uint8_t *b = (const uint8_t *)p;
        for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    }
    template <class T>
    void array(const T *p, size_t count) {
        const uint64_t c = count;
        uint8_t le[8];
        for (int i = 0; i < 8; i++) le[i] = (uint8_t)(c >> (8 * i));
        bytes(le, 8);
        bytes(p, count * sizeof(T));
    }
};
inline uint64_t scene_digest(const PreparedScene &ps) {
    Fnv64 f;
    f.array(ps.face_base.data(), ps.face_base.size());
    f.array(ps.faces.data(), ps.faces.size());
    f.array(ps.mesh_packed.data(), ps.mesh_packed.size());
    f.array(ps.leaf_faces.data(), ps.leaf_faces.size());
    f.array(ps.leaf_face_idx.data(), ps.leaf_face_idx.size());
    f.array(ps.mesh_roots.data(), ps.mesh_roots.size());
    f.array(ps.walk_jobs.data(), ps.walk_jobs.size());
    f.array(ps.sphere_boxes.data(), ps.sphere_boxes.size());
    f.array(ps.sphere_links.data(), ps.sphere_links.size());
    f.array(ps.sphere_leaf_idx.data(), ps.sphere_leaf_idx.size());
    uint32_t w[11] = {ps.bvh_node_count, 0, 0, 0, 0, 0, 0, 0, ps.have_mesh_bvh ? 1u : 0u, ps.uses_tex ? 1u : 0u, ps.max_tex};
    memcpy(&w[1], ps.bvh_lo, 12);
    memcpy(&w[4], ps.bvh_hi, 12);
    memcpy(&w[7], &ps.bvh_rmax, 4);
    f.array(w, 11);
    return f.h;
}

// ---- self-check of the prepared structures ---------------------------------------------------
struct BvhWalkStats { uint64_t nodes = 0, leaves = 0, prims = 0, max_depth = 0; };

// walk the sphere tree the way the kernel does for direction octant `oct` with every box "hit": nearer child
// after an inner node, the octant's skip link after a leaf
inline std::string host_walk_octant(const std::vector<float4> &nodes, uint32_t oct, std::vector<uint32_t> &leaf_visits, BvhWalkStats &st) {
    uint32_t n_nodes = (uint32_t)(nodes.size() / 4), cur = BVH_ROOT;
    for (uint64_t guard = 0; cur != BVH_END; guard++) {
        if (guard > (uint64_t)n_nodes + 8) return "walk does not terminate";
        if (cur >= n_nodes) return "node index out of range";
        uint32_t A, B, sk[8];
        memcpy(&A, &nodes[4 * (size_t)cur].w, 4);
        memcpy(&B, &nodes[4 * (size_t)cur + 1].w, 4);
        memcpy(sk, &nodes[4 * (size_t)cur + 2], 32);
        st.nodes++;
        if (B & 0x80000000u) {
            uint32_t first = B & 0x0FFFFFFFu, cnt = (B >> 28) & 7u;
            st.leaves++;
            for (uint32_t k = 0; k < cnt; k++) {
                if (first + k >= leaf_visits.size()) return "leaf slot out of range";
                leaf_visits[first + k]++;
            }
            cur = sk[oct];
        } else {
            if (((A >> 28) & 3u) > 2) return "bad split axis";
            if (B & 1u) return "left child at an odd index";
            cur = B + ((oct >> ((A >> 28) & 3u)) & 1u);
        }
    }
    return "";
}

// recursive structural check of the sphere tree: the eight skip links, depth
// (boxes: every primitive is checked against the box of EVERY node above it, see check_prepared)
inline std::string host_check_sphere_tree(const std::vector<float4> &nodes, uint32_t me, const uint32_t skip[8], uint32_t depth,
                                          BvhWalkStats &st) {
    const float4 &lo = nodes[4 * (size_t)me], &hi = nodes[4 * (size_t)me + 1];
    uint32_t A, B, sk[8];
    memcpy(&A, &lo.w, 4);
    memcpy(&B, &hi.w, 4);
    memcpy(sk, &nodes[4 * (size_t)me + 2], 32);
    for (int o = 0; o < 8; o++) if (sk[o] != skip[o]) return "wrong skip link";
    st.max_depth = std::max<uint64_t>(st.max_depth, depth);
    if (depth > 60) return "tree deeper than 60 levels";
    if (B & 0x80000000u) return "";
    uint32_t ax = (A >> 28) & 3u, sl[8], sr[8];
    for (uint32_t o = 0; o < 8; o++) {
        bool right_first = ((o >> ax) & 1u) != 0;
        sl[o] = right_first ? skip[o] : B + 1u;
        sr[o] = right_first ? B : skip[o];
    }
    std::string e = host_check_sphere_tree(nodes, B, sl, depth + 1, st);
    if (e.empty()) e = host_check_sphere_tree(nodes, B + 1u, sr, depth + 1, st);
    return e;
}

// the mesh trees are threaded (pt_mesh_bvh.hpp): follow "left child after an inner node, skip link after a leaf".
// nodes: `stride` float4 per node, A in [0].w and B in [1].w — 4 for the builder's form, 3 for the packed one
inline std::string host_walk_threaded(const std::vector<float4> &nodes, size_t stride, uint32_t root, std::vector<uint32_t> &leaf_visits,
                                      BvhWalkStats &st) {
    uint32_t n_nodes = (uint32_t)(nodes.size() / stride), cur = root;
    for (uint64_t guard = 0; cur != 0x0FFFFFFFu; guard++) {
        if (guard > (uint64_t)n_nodes + 8) return "walk does not terminate";
        if (cur >= n_nodes) return "node index out of range";
        uint32_t A, B;
        memcpy(&A, &nodes[stride * cur].w, 4);
        memcpy(&B, &nodes[stride * cur + 1].w, 4);
        st.nodes++;
        if (B & 0x80000000u) {
            uint32_t first = B & 0x0FFFFFFFu, cnt = (B >> 28) & 7u;
            st.leaves++;
            for (uint32_t k = 0; k < cnt; k++) {
                if (first + k >= leaf_visits.size()) return "leaf slot out of range";
                leaf_visits[first + k]++;
            }
            cur = A & 0x0FFFFFFFu;
        } else {
            cur = B;
        }
    }
    return "";
}

// recursive structural check of a threaded tree: skip links, depth
// (boxes: every primitive is checked against the box of EVERY node above it, see check_prepared)
inline std::string host_check_threaded(const std::vector<float4> &nodes, uint32_t me, uint32_t skip, uint32_t depth, BvhWalkStats &st) {
    const float4 &lo = nodes[4 * (size_t)me], &hi = nodes[4 * (size_t)me + 1];
    uint32_t A, B;
    memcpy(&A, &lo.w, 4);
    memcpy(&B, &hi.w, 4);
    if ((A & 0x0FFFFFFFu) != skip) return "wrong skip link";
    st.max_depth = std::max<uint64_t>(st.max_depth, depth);
    if (depth > 60) return "tree deeper than 60 levels";
    if (B & 0x80000000u) return "";
    if (B >= nodes.size() / 4) return "left child out of range";
    uint32_t right;   // = the left child's skip link
    memcpy(&right, &nodes[4 * (size_t)B].w, 4);
    right &= 0x0FFFFFFFu;
    if (right >= nodes.size() / 4) return "left child's skip link out of range";
    std::string e = host_check_threaded(nodes, B, right, depth + 1, st);
    if (e.empty()) e = host_check_threaded(nodes, right, skip, depth + 1, st);
    return e;
}

// The invariants of a prepared scene: every primitive in exactly one leaf and inside the box of every node above it,
// split axes and skip links, the kernels' threaded walks visiting every leaf exactly once (all eight octants of the
// sphere tree; the mesh trees as built and through the collapsed links of the packed nodes), smallest-face indices, normal
// cones, edge bounds, the packed fields rounded to the safe side, the device layout of the sphere tree, the walk jobs.
// stats = {sphere nodes, leaves, depth, mesh nodes, leaves, depth, meshes with a BVH, scene_digest}
inline int check_prepared(const rt_scene_desc &scene, const PreparedScene &ps, uint64_t stats[8], std::string &err) {
    const rt_scene_desc *d = &scene;
    auto bad = [&](const std::string &m) {
        err = m;
        return RT_EINVAL;
    };
    memset(stats, 0, 8 * sizeof(uint64_t));
    stats[7] = scene_digest(ps);
    // ---- sphere BVH
    if (!ps.sphere_nodes.empty()) {
        const std::vector<float4> &nodes = ps.sphere_nodes;
        const std::vector<uint32_t> &leaf_idx = ps.sphere_leaf_idx;
        BvhWalkStats st;
        const uint32_t end[8] = {BVH_END, BVH_END, BVH_END, BVH_END, BVH_END, BVH_END, BVH_END, BVH_END};
        std::string e = host_check_sphere_tree(nodes, BVH_ROOT, end, 0, st);
        if (!e.empty()) return bad("sphere bvh: " + e);
        for (uint32_t oct = 0; oct < 8; oct++) {
            std::vector<uint32_t> visits(leaf_idx.size(), 0);
            BvhWalkStats w;
            e = host_walk_octant(nodes, oct, visits, w);
            if (!e.empty()) return bad("sphere bvh: " + e);
            for (uint32_t v : visits) if (v != 1) return bad("sphere bvh: a leaf slot is not visited exactly once");
            st.nodes = w.nodes; st.leaves = w.leaves;
        }
        std::vector<uint32_t> seen(d->sphere_count, 0);
        if (leaf_idx.size() != d->sphere_count) return bad("sphere bvh: leaf slot count != sphere count");
        for (uint32_t i : leaf_idx) { if (i >= d->sphere_count || seen[i]++) return bad("sphere bvh: sphere missing or duplicated"); }
        // every sphere inside the box (centre ± half extent) of its leaf and of every node above it
        std::function<std::string(uint32_t, std::vector<uint32_t> &)> gather = [&](uint32_t n, std::vector<uint32_t> &sph) -> std::string {
            uint32_t B;
            memcpy(&B, &nodes[4 * (size_t)n + 1].w, 4);
            if (B & 0x80000000u) {
                uint32_t first = B & 0x0FFFFFFFu, cnt = (B >> 28) & 7u;
                for (uint32_t k = 0; k < cnt; k++) sph.push_back(leaf_idx[first + k]);
            } else {
                for (uint32_t k = 0; k < 2; k++) {
                    std::vector<uint32_t> sub;
                    std::string er = gather(B + k, sub);
                    if (!er.empty()) return er;
                    sph.insert(sph.end(), sub.begin(), sub.end());
                }
            }
            const float4 &c = nodes[4 * (size_t)n], &h = nodes[4 * (size_t)n + 1];
            for (uint32_t i : sph) {
                const rt_sphere &sp = d->spheres[i];
                const float r = std::fabs(sp.r), p[3] = {sp.pos.x, sp.pos.y, sp.pos.z};
                for (int k = 0; k < 3; k++) {   // (the sphere's extent in binary32, as BvhBuild::bounds forms it)
                    const double lo = (double)(&c.x)[k] - (double)(&h.x)[k], hi = (double)(&c.x)[k] + (double)(&h.x)[k];
                    const float slo = p[k] - r, shi = p[k] + r;
                    if ((double)slo < lo || (double)shi > hi) return std::string("sphere outside the box of a node above it");
                }
            }
            return "";
        };
        {
            std::vector<uint32_t> all;
            e = gather(BVH_ROOT, all);
            if (!e.empty()) return bad("sphere bvh: " + e);
        }
        // the arrays the kernels walk: (centre, B) per node; per octant the skip link with the axis bits and the half extent
        const size_t n_nodes = nodes.size() / 4;
        if (ps.sphere_boxes.size() != n_nodes || ps.sphere_links.size() != 8 * n_nodes) return bad("sphere bvh: device arrays of the wrong size");
        for (size_t n = 0; n < n_nodes; n++) {
            const float4 &c = nodes[4 * n], &h = nodes[4 * n + 1];
            if (memcmp(&ps.sphere_boxes[n], &c, 12) || memcmp(&ps.sphere_boxes[n].w, &h.w, 4)) return bad("sphere bvh: device box differs from the node's (centre, B)");
            uint32_t A, sk[8];
            memcpy(&A, &c.w, 4);
            memcpy(sk, &nodes[4 * n + 2], 32);
            for (int o = 0; o < 8; o++) {
                const float4 &l = ps.sphere_links[8 * n + o];
                const uint32_t want = sk[o] | (((A >> 28) & 3u) << 28);
                if (memcmp(&l.x, &want, 4)) return bad("sphere bvh: device link is not skip | axis << 28");
                if (memcmp(&l.y, &h.x, 12)) return bad("sphere bvh: device link does not carry the node's half extent");
            }
        }
        stats[0] = st.nodes; stats[1] = st.leaves; stats[2] = st.max_depth;
    }
    // ---- mesh BVHs
    if (ps.have_mesh_bvh) {
        std::vector<float4> nodes = ps.mesh_nodes;   // the trees as built: the collapse rewrote the link words only
        if (ps.mesh_built_links.size() != nodes.size() / 4) return bad("mesh bvh: built links of the wrong size");
        for (size_t n = 0; n < nodes.size() / 4; n++) {
            memcpy(&nodes[4 * n].w, &ps.mesh_built_links[n].x, 4);
            memcpy(&nodes[4 * n + 1].w, &ps.mesh_built_links[n].y, 4);
        }
        const std::vector<uint32_t> &lidx = ps.leaf_face_idx;
        std::vector<uint32_t> visits(lidx.size(), 0), visits_packed(lidx.size(), 0);
        size_t slot0 = 0;   // the trees' leaf slots follow each other in mesh order
        for (uint32_t m = 0; m < d->mesh_count; m++) {
            const uint32_t root = ps.mesh_roots[m], nf = d->meshes[m].face_count;
            if (root == MESH_ROOT_NONE) continue;
            if (root >= nodes.size() / 4) return bad("mesh bvh: root out of range");
            BvhWalkStats st;
            std::string e = host_check_threaded(nodes, root, 0x0FFFFFFFu, 0, st);
            if (!e.empty()) return bad("mesh bvh: " + e);
            if (slot0 + nf > lidx.size()) return bad("mesh bvh: leaf slot count != face count");
            {
                BvhWalkStats w;
                e = host_walk_threaded(nodes, 4, root, visits, w);
                if (!e.empty()) return bad("mesh bvh: " + e);
                for (size_t k = slot0; k < slot0 + nf; k++) if (visits[k] != 1) return bad("mesh bvh: a leaf slot is not visited exactly once");
                st.nodes = w.nodes; st.leaves = w.leaves;
            }
            {   // the links the device walks (wide-cone inner nodes spliced out), in the packed nodes: still every leaf exactly once
                BvhWalkStats w;
                e = host_walk_threaded(ps.mesh_packed, 3, root, visits_packed, w);
                if (!e.empty()) return bad("mesh bvh (collapsed links): " + e);
                for (size_t k = slot0; k < slot0 + nf; k++) if (visits_packed[k] != 1) return bad("mesh bvh (collapsed links): a leaf slot is not visited exactly once");
            }
            std::vector<uint32_t> seen(nf, 0);
            for (size_t k = slot0; k < slot0 + nf; k++) { const uint32_t i = lidx[k]; if (i >= nf || seen[i]++) return bad("mesh bvh: face missing or duplicated"); }
            // per node: min face, normal cone, edge and quality bounds, faces inside leaf boxes — from the leaves up
            const float4 *rec = &ps.faces[3 * (size_t)ps.face_base[m]];
            std::function<std::string(uint32_t, std::vector<uint32_t> &)> collect = [&](uint32_t n, std::vector<uint32_t> &faces) -> std::string {
                uint32_t B;
                memcpy(&B, &nodes[4 * (size_t)n + 1].w, 4);
                if (B & 0x80000000u) {
                    uint32_t first = B & 0x0FFFFFFFu, cnt = (B >> 28) & 7u;
                    for (uint32_t k = 0; k < cnt; k++) faces.push_back(lidx[first + k]);
                } else {
                    uint32_t right;
                    memcpy(&right, &nodes[4 * (size_t)B].w, 4);
                    for (uint32_t k = 0; k < 2; k++) {
                        std::vector<uint32_t> sub;
                        std::string er = collect(k ? (right & 0x0FFFFFFFu) : B, sub);
                        if (!er.empty()) return er;
                        faces.insert(faces.end(), sub.begin(), sub.end());
                    }
                }
                const float4 &lo = nodes[4 * (size_t)n], &hi = nodes[4 * (size_t)n + 1], &cone = nodes[4 * (size_t)n + 2], &ex = nodes[4 * (size_t)n + 3];
                uint32_t min_face;
                memcpy(&min_face, &ex.y, 4);
                uint32_t true_min = 0xFFFFFFFFu;
                for (uint32_t f : faces) {
                    true_min = std::min(true_min, f);
                    const float4 *q = rec + 3 * (size_t)f;
                    double A[3] = {q[0].x, q[0].y, q[0].z}, e1[3] = {q[0].w, q[1].x, q[1].y}, e2[3] = {q[1].z, q[1].w, q[2].x};
                    for (int k = 0; k < 3; k++) {   // (lo, hi here: the node's centre and half extent)
                        const double l = (double)(&lo.x)[k] - (double)(&hi.x)[k], h = (double)(&lo.x)[k] + (double)(&hi.x)[k];
                        double p[3] = {A[k], A[k] + e1[k], A[k] + e2[k]};
                        for (double v : p) if (v < l || v > h) return std::string("face outside its node box");
                    }
                    double nl = std::sqrt((double)q[2].y * q[2].y + (double)q[2].z * q[2].z + (double)q[2].w * q[2].w);
                    if (std::isfinite(nl) && nl > 0.5 && ex.w > 0.0f) {
                        double dt = (cone.x * q[2].y + cone.y * q[2].z + cone.z * q[2].w) / nl;
                        double cos_a = cone.w, sin_a = ex.x;
                        // the face normal must lie inside the cone (cos/sin describe the half angle; 0/1 = hemisphere or wider)
                        if (!(cos_a == 0.0 && sin_a == 1.0) && dt < cos_a - 1e-5) return std::string("face normal outside the node's cone");
                    }
                    double l1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), l2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
                    if (l1 > ex.z * 1.0001 || l2 > ex.z * 1.0001) return std::string("edge longer than the node's bound");
                }
                if (true_min != min_face) return std::string("wrong smallest face index");
                return "";
            };
            std::vector<uint32_t> all;
            e = collect(root, all);
            if (!e.empty()) return bad("mesh bvh: " + e);
            slot0 += nf;
            stats[3] += st.nodes; stats[4] += st.leaves; stats[5] = std::max(stats[5], st.max_depth); stats[6]++;
        }
        if (slot0 != lidx.size()) return bad("mesh bvh: leaf slot count != face count");
        // the device's 48-byte form of every node (mesh_node_pack), as uploaded: binary16 fields rounded to the safe side
        if (ps.mesh_packed.size() != ps.mesh_nodes.size() / 4 * 3) return bad("mesh bvh: packed nodes of the wrong size");
        for (size_t n = 0; n < ps.mesh_nodes.size() / 4; n++) {
            const float4 *nd = &ps.mesh_nodes[4 * n], *pk = &ps.mesh_packed[3 * n];
            uint32_t p[3];
            memcpy(p, &pk[2], 12);
            const float hx = bvh_half_value(p[0] & 0xFFFFu), hy = bvh_half_value(p[0] >> 16), hz = bvh_half_value(p[1] & 0xFFFFu);
            const float sn = bvh_half_value(p[1] >> 16), em = bvh_half_value(p[2] & 0xFFFFu), q = bvh_half_value(p[2] >> 16);
            if (!(hx >= nd[1].x && hy >= nd[1].y && hz >= nd[1].z)) return bad("mesh bvh: packed half extent below the node's");
            if (!(sn >= nd[3].x) || !(em >= nd[3].z) || !(q <= nd[3].w)) return bad("mesh bvh: packed cone / edge / quality on the wrong side");
            if (memcmp(&pk[0], &nd[0], 16) || memcmp(&pk[1], &nd[2], 12) || memcmp(&pk[1].w, &nd[1].w, 4) || memcmp(&pk[2].w, &nd[3].y, 4))
                return bad("mesh bvh: packed node differs in an unpacked field");
        }
    }
    // ---- walk jobs: every mesh of every model, in model order, each with a tree
    if (!ps.walk_jobs.empty()) {
        size_t j = 0;
        for (uint32_t mo = 0; mo < d->model_count; mo++)
            for (uint32_t k = 0; k < d->models[mo].mesh_count; k++, j++) {
                const uint32_t mi = d->models[mo].mesh_anchor + k;
                if (j >= ps.walk_jobs.size() || ps.walk_jobs[j].x != mi || ps.walk_jobs[j].y != d->models[mo].mat_ID)
                    return bad("walk jobs: not the models' meshes in model order");
                if (!ps.have_mesh_bvh || ps.mesh_roots[mi] == MESH_ROOT_NONE) return bad("walk jobs: a job names a mesh without a tree");
            }
        if (j != ps.walk_jobs.size()) return bad("walk jobs: not the models' meshes in model order");
    }
    return RT_OK;
}

}  // namespace scene_prep
