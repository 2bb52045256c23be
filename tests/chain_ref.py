"""Host restatement of rt_render_features_chain exactly as include/rt_amd.h states it, over two probe functions — the
device's (RayTracer.debugHit / debugMaterial) or the CPU oracle's (Oracle.hit / hit_triangle / material) — and the
pair key of RT_DENOISE_SPLIT_CHAINS for the numpy filters of tests/denoise_ref.py, denoise_vg_ref.py and moments_ref.py.
Shared by tests/test_feature_chain_host.py and tests/test_gpu_feature_chain.py."""
import numpy as np

import cases

rt = cases.rt
A = rt._abi
F32 = np.float32
GOLDEN = 0x9E3779B1
HI = np.uint32(0xFFFF0000)
KIND_SHIFT = 30
MAX_PROBES = 1 << 21     # per batched probe call


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def signature(objects):
    """h = 0; h = (h ^ object) * 0x9E3779B1 mod 2^32 over the followed vertices in path order."""
    h = 0
    for o in objects:
        h = ((h ^ int(o)) * GOLDEN) & 0xFFFFFFFF
    return h


def signature_step(h, obj):
    """The same step for arrays of running signatures."""
    return (((h.astype(np.uint64) ^ obj.astype(np.uint64)) * np.uint64(GOLDEN)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def texel(scene, u, v, tex):
    """texture_rgb (pt_device.hpp) on the host in float32: bilinear, edge clamp."""
    f = F32
    T = scene.textures
    layers, H, W = T.shape[:3]
    layer = np.where(tex < layers, tex, 0)
    # the texel coordinate, clamped to [-1, W] before floor, NaN counts as -1
    with np.errstate(invalid="ignore", over="ignore"):
        uu, vv = (u * f(W) - f(0.5)).astype(f), (v * f(H) - f(0.5)).astype(f)
        uu = np.where(uu >= -1, np.where(uu > f(W), f(W), uu), f(-1)).astype(f)
        vv = np.where(vv >= -1, np.where(vv > f(H), f(H), vv), f(-1)).astype(f)
    fu, fv = np.floor(uu), np.floor(vv)
    a, b = (uu - fu).astype(f), (vv - fv).astype(f)
    i0, j0 = fu.astype(np.int64), fv.astype(np.int64)
    i1, j1 = np.clip(i0 + 1, 0, W - 1), np.clip(j0 + 1, 0, H - 1)
    i0, j0 = np.clip(i0, 0, W - 1), np.clip(j0, 0, H - 1)
    t00, t10, t01, t11 = (T[layer, jj, ii, :3] for jj, ii in ((j0, i0), (j0, i1), (j1, i0), (j1, i1)))
    w00, w10, w01, w11 = ((f(1) - a) * (f(1) - b))[:, None], (a * (f(1) - b))[:, None], ((f(1) - a) * b)[:, None], (a * b)[:, None]
    return ((((w00 * t00).astype(f) + (w10 * t10).astype(f)).astype(f) + (w01 * t01).astype(f)).astype(f)
            + (w11 * t11).astype(f)).astype(f)


class DeviceProbes:
    """The probes of a RayTracer under its selected arithmetic policy."""

    def __init__(self, tracer):
        self.t = tracer

    def hit(self, kind, rays, prim=None, face=None):
        return self.t.debugHit(kind, rays, prim, face)

    def material(self, routine, vec):
        return self.t.debugMaterial(routine, vec)


class OracleProbes:
    """The CPU oracle's restatements of the same routines (policy IEEE)."""

    def __init__(self, oracle, scene, table):
        self.o, self.scene, self.table = oracle, scene, table

    def hit(self, kind, rays, prim=None, face=None):
        n = len(rays)
        prim = np.zeros(n, np.uint32) if prim is None else prim
        if kind == 4:
            return self.o.hit_triangle(self.scene, rays, prim, face)
        return self.o.hit(kind, self.scene, rays, prim)

    def material(self, routine, vec):
        return self.o.material(routine, self.scene, self.table, vec)


def _batched(probe, kind, rays, count, face_axis=False, mesh=0):
    """One primitive probe of every ray against primitives (or faces of `mesh`) 0 .. count-1 → (hit, t, u, v), each
    (len(rays), count)."""
    m = len(rays)
    step = max(1, MAX_PROBES // max(count, 1))
    parts = []
    for a in range(0, m, step):
        r = np.repeat(rays[a:a + step], count, axis=0)
        idx = np.tile(np.arange(count, dtype=np.uint32), len(rays[a:a + step]))
        if face_axis:
            o = probe.hit(4, r, np.full(len(r), mesh, np.uint32), idx)
        else:
            o = probe.hit(kind, r, idx)
        parts.append(o.reshape(-1, count, 12))
    o = np.concatenate(parts) if parts else np.zeros((0, count, 12), F32)
    return o[..., 0] > 0, bits(o[..., 1]), bits(o[..., 8]), bits(o[..., 9])


RESIDUAL_BOUND = 1e-3     # |distance from the surface| / (|o| + t + size): tests/test_gpu_denoise.py sees <= 1e-3 on grazing sphere hits


def _surface_residuals(scene, rays, out):
    """How far, relative to the magnitudes the float32 hit point o + t d is formed from, every scene hit lies from every
    sphere, plane and lens surface of the hit's material (inf for the others) → (hits, primitives) float64 and the
    primitives' object ids, in the search's order spheres, planes, lenses."""
    p = out[:, 2:5].astype(np.float64)
    base = np.linalg.norm(rays[:, :3].astype(np.float64), axis=1) + out[:, 1].astype(np.float64)
    mat = bits(out[:, 11])
    res, ids = [], []

    def to_sphere(centre, radius):
        d = np.linalg.norm(p[:, None, :] - centre[None, :, :3].astype(np.float64), axis=2)
        return np.abs(d - radius[None, :]) / (base[:, None] + radius[None, :])

    for kind, arr in ((0, scene.spheres), (1, scene.planes), (2, scene.lenses)):
        if not len(arr):
            continue
        if kind == 0:
            r = to_sphere(arr["pos"], arr["r"].astype(np.float64))
        elif kind == 1:
            nrm = arr["normal"][:, :3].astype(np.float64)
            pos = arr["pos"][:, :3].astype(np.float64)
            d = np.abs(((p[:, None, :] - pos[None]) * nrm[None]).sum(2)) / np.linalg.norm(nrm, axis=1)[None]
            r = d / (base[:, None] + np.linalg.norm(pos, axis=1)[None] + 1.0)
        else:
            r = np.minimum(to_sphere(arr["p1"], arr["r1"].astype(np.float64)), to_sphere(arr["p2"], arr["r2"].astype(np.float64)))
        res.append(np.where(arr["mat_ID"][None, :] == mat[:, None], r, np.inf))
        ids.append((np.uint32(kind) << np.uint32(KIND_SHIFT)) | np.arange(len(arr), dtype=np.uint32))
    if not res:
        return np.full((len(out), 0), np.inf), np.zeros(0, np.uint32)
    return np.concatenate(res, axis=1), np.concatenate(ids)


def _identify_meshes(probe, scene, rays, out, want_face, obj, face):
    """The mesh and face search of `identify`, for the hits whose obj is still NO_ID: fills obj and face in place."""
    t_bits = bits(out[:, 1])
    mat = bits(out[:, 11])
    sel = np.nonzero(obj == A.NO_ID)[0]
    if len(sel):
        tex = bits(out[:, 10])
        models, meshes = scene.models, scene.meshes
        mesh_mat = np.full(len(meshes), A.NO_ID, np.uint32)
        for md in models:
            mesh_mat[md["mesh_anchor"]:md["mesh_anchor"] + md["mesh_count"]] = md["mat_ID"]
        fits = (mesh_mat[None, :] == mat[sel, None]) & (meshes["texture_ID"][None, :] == tex[sel, None])   # (hits, meshes)
        assert fits.any(1).all(), "a scene hit on no primitive and no mesh of its material"
        by_face = want_face[sel] | (fits.sum(1) > 1)
        only = ~by_face
        obj[sel[only]] = (np.uint32(3) << np.uint32(KIND_SHIFT)) | fits[only].argmax(1).astype(np.uint32)
        for m in range(len(meshes)):
            mine = sel[by_face & fits[:, m]]
            mine = mine[obj[mine] == A.NO_ID]
            if not len(mine):
                continue
            h, t, u, v = _batched(probe, 4, rays[mine], int(meshes["face_count"][m]), face_axis=True, mesh=m)
            cand = h & (t == t_bits[mine, None]) & (u == bits(out[mine, 8])[:, None]) & (v == bits(out[mine, 9])[:, None])
            found = cand.any(1)
            obj[mine[found]] = (np.uint32(3) << np.uint32(KIND_SHIFT)) | np.uint32(m)
            face[mine[found]] = cand.argmax(1).astype(np.uint32)[found]
    assert (obj != A.NO_ID).all(), "a mesh hit that no face's own probe returns"
    return obj, face


def identify(probe, scene, rays, out, want_face):
    """The object id (kind << 30 | index) of every scene hit `out` (n x 12 records of the kind-3 probe for `rays`) and,
    where `want_face`, the face of a mesh hit.  The hit records carry no object id, so it is found from the geometry, in
    float64 and independent of the arithmetic policy: the sphere, plane or lens of the hit's material on whose surface the
    hit point lies (residual <= RESIDUAL_BOUND, every other candidate at least ten bounds away); a hit on none of them
    belongs to a mesh — the one of the hit's material and texture id (where several share both, the one with a face that
    returns the hit) — and its face is the first whose triangle probe returns the hit's t, u and v bit for bit."""
    n = len(rays)
    obj = np.full(n, A.NO_ID, np.uint32)
    face = np.full(n, A.NO_ID, np.uint32)
    res, ids = _surface_residuals(scene, rays, out)
    if res.shape[1]:
        order = np.argsort(res, axis=1, kind="stable")
        best = np.take_along_axis(res, order[:, :1], 1)[:, 0]
        on = best <= RESIDUAL_BOUND
        if res.shape[1] > 1:
            second = np.take_along_axis(res, order[:, 1:2], 1)[:, 0]
            assert (second[on] > 10 * RESIDUAL_BOUND).all(), "a hit point on two primitives of one material"
        obj[on] = ids[order[on, 0]]
    return _identify_meshes(probe, scene, rays, out, want_face, obj, face)


def identify_by_probe(probe, scene, rays, out, want_face):
    """`identify` by the search's own rule instead of by geometry, for scenes whose primitives overlap or coincide (tests/
    edge_scenes.py): the scene search keeps the first primitive, in its order spheres, planes, lenses, that reports the
    smallest t, so a hit belongs to the first sphere, plane or lens whose own probe (kind 0, 1, 2) for the ray returns the
    scene hit's t and material bit for bit; a hit that none of them returns belongs to a mesh, found as `identify` finds
    it.  The probes are those of the arithmetic policy under test, so the rule holds under every policy."""
    n = len(rays)
    obj = np.full(n, A.NO_ID, np.uint32)
    face = np.full(n, A.NO_ID, np.uint32)
    t_bits = bits(out[:, 1])
    mat = bits(out[:, 11])
    for kind, count in ((0, len(scene.spheres)), (1, len(scene.planes)), (2, len(scene.lenses))):
        todo = np.nonzero(obj == A.NO_ID)[0]
        if not count or not len(todo):
            continue
        step = max(1, MAX_PROBES // count)
        for a in range(0, len(todo), step):
            sel = todo[a:a + step]
            idx = np.tile(np.arange(count, dtype=np.uint32), len(sel))
            o = probe.hit(kind, np.repeat(rays[sel], count, axis=0), idx).reshape(len(sel), count, 12)
            cand = (o[..., 0] > 0) & (bits(o[..., 1]) == t_bits[sel, None]) & (bits(o[..., 11]) == mat[sel, None])
            found = cand.any(1)
            obj[sel[found]] = (np.uint32(kind) << np.uint32(KIND_SHIFT)) | cand.argmax(1).astype(np.uint32)[found]
    return _identify_meshes(probe, scene, rays, out, want_face, obj, face)


def replay(probe, scene, origin, dirs, follow, max_chain, identify=identify):
    """rt_render_features_chain for the primary rays (origin, dirs[i]) → (records, chain objects): len(dirs) records of
    _abi.FEATURE and, per pixel, the list of followed object ids.  One batched scene probe and one batched call per
    material routine per bounce: routine 0 (rayReflect) for reflective vertices, routine 1 (rayRefract) for refractive
    and followed dielectric ones.  `identify`: the rule that names a hit's object and face — `identify` (the default) or
    `identify_by_probe`."""
    dirs = np.ascontiguousarray(dirs, dtype=F32).reshape(-1, 3)
    n = len(dirs)
    rec = np.zeros(n, A.FEATURE)
    rec["dir"] = dirs
    rec["t"] = np.inf
    rec["object"] = rec["material"] = rec["face"] = A.NO_ID
    rays = np.concatenate([np.repeat(np.asarray(origin, F32)[None, :3], n, 0), dirs], axis=1).astype(F32)
    t_sum = np.zeros(n, F32)
    length = np.zeros(n, np.uint32)
    sig = np.zeros(n, np.uint32)
    chain = [[] for _ in range(n)]
    types = scene.materials["type"]
    alive = np.arange(n)
    for k in range(max_chain + 1):
        if not len(alive):
            break
        out = probe.hit(3, rays[alive])
        h = out[:, 0] > 0
        alive, out = alive[h], out[h]          # (a miss keeps the miss record; its flags are filled in at the end)
        if not len(alive):
            break
        t_sum[alive] = out[:, 1] if k == 0 else (t_sum[alive] + out[:, 1]).astype(F32)
        mat = bits(out[:, 11])
        typ = types[mat]
        followed = (((typ == A.T_REFLECTIVE) & bool(follow & A.FOLLOW_REFLECTIVE)) |
                    ((typ == A.T_REFRACTIVE) & bool(follow & A.FOLLOW_REFRACTIVE)) |
                    ((typ == A.T_DIELECTRIC) & bool(follow & A.FOLLOW_DIELECTRIC)))
        go = followed & (length[alive] < max_chain)
        obj, face = identify(probe, scene, rays[alive], out, ~go)
        # terminals
        ti, to = alive[~go], out[~go]
        r = rec[ti]
        r["pos"], r["t"], r["normal"] = to[:, 2:5], t_sum[ti], to[:, 5:8]
        r["object"], r["material"], r["face"] = obj[~go], mat[~go], face[~go]
        r["u"], r["v"], r["tex"] = to[:, 8], to[:, 9], bits(to[:, 10])
        alb = scene.materials["color"][mat[~go], :3].astype(F32)
        tx = typ[~go] == A.T_TEXTURED
        if tx.any():
            alb[tx] = texel(scene, to[tx, 8], to[tx, 9], bits(to[tx, 10]))
        r["albedo"] = alb
        cut = followed[~go] & (max_chain > 0)
        r["flags"] = np.uint32(A.FEATURE_HIT) | np.where(cut, np.uint32(A.FEATURE_CUT), np.uint32(0))
        rec[ti] = r
        # followed vertices
        gi, go_out = alive[go], out[go]
        if len(gi):
            sig[gi] = signature_step(sig[gi], obj[go])
            length[gi] += 1
            for i, o in zip(gi, obj[go]):
                chain[i].append(int(o))
            vec = np.zeros((len(gi), 16), F32)
            vec[:, 0:3], vec[:, 3:6], vec[:, 6:9], vec[:, 9:12] = rays[gi, 3:6], go_out[:, 2:5], go_out[:, 5:8], 1.0
            vec.view(np.uint32)[:, 12] = mat[go]
            refl = typ[go] == A.T_REFLECTIVE
            nxt = np.zeros((len(gi), 9), F32)
            if refl.any():
                nxt[refl] = probe.material(0, vec[refl])
            if (~refl).any():
                nxt[~refl] = probe.material(1, vec[~refl])
            rays[gi] = nxt[:, :6]
        alive = gi
    assert not len(alive) or k == max_chain
    rec["flags"] |= (length << np.uint32(8)) | (sig & HI)
    return rec, chain


def split(rec):
    return A.split_features(rec)


def pair_labels(feats, split_objects, split_chains):
    """The pair (key, flags >> 8) of the header as ONE dense label per pixel — an enumeration of the pairs present, so
    nothing is folded — for the `obj` argument of the numpy filters (call them with split_objects=True)."""
    key = feats["object"].astype(np.uint64) if split_objects else (~feats["hit"]).astype(np.uint64)
    word = feats["chain_word"].astype(np.uint64) if split_chains else np.zeros_like(key)
    pairs = (key << np.uint64(32)) | word
    _, inv = np.unique(pairs.reshape(-1), return_inverse=True)
    return inv.reshape(pairs.shape).astype(np.uint32)


def with_pair_key(feats, split_objects, split_chains):
    """A features dict whose `object` is the pair label: the existing restatements, given split_objects=True, then
    compare exactly what the kernels compare."""
    f = dict(feats)
    f["object"] = pair_labels(feats, split_objects, split_chains)
    return f
