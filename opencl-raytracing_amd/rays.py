"""Ray batches for RayTracer.renderRays (rt_render_rays) — host-only, numpy float32, no device and no library needed.

A batch is an array of ``_abi.RAY`` records (rt_ray: origin, random-stream x, direction, random-stream y).  The generators
make one ray per pixel of a w x h frame, ray i = pixel (i % w, i // w), row-major, so that a batch can go straight into the
accumulator (``renderRays(rays, first, n)`` with ``out=None``) and through ``resolve`` and the denoisers.

Orientation is the Camera class's: yaw and pitch in degrees give the view direction
``W = (cos p sin y, sin p, cos p cos y)``, ``U = normalize(cross(W, up))`` with the world's up = -y, ``V = cross(U, W)``;
column x grows along U and row y along V, as the pinhole camera's frame coordinates (s, t) do.  Pixels are sampled at their
centres, (x + 0.5) / w — except ``primary_rays``, which restates the pinhole camera and takes x / w as it does.

Directions are unit length to float32 rounding (the tracer uses a direction as given and does not normalise it).  The trig
is done in float64 and rounded once.
"""
import numpy as np

from . import _abi

f32 = np.float32
MAX_DIM = _abi.MAX_DIM


def pack_rays(origins, dirs, ids=None, w=None):
    """(n, 3) origins and (n, 3) directions (origins may be one point, (3,)) → n _abi.RAY records.  ``ids``: (n, 2)
    unsigned (x, y) random-stream ids, the values pixel coordinates take; default (i % w, i // w) with w = MAX_DIM unless
    given, which keeps both below MAX_DIM for every batch rt_render_rays accepts."""
    dirs = np.ascontiguousarray(dirs, dtype=f32).reshape(-1, 3)
    n = len(dirs)
    origins = np.broadcast_to(np.asarray(origins, dtype=f32).reshape(-1, 3), (n, 3))
    out = np.zeros(n, dtype=_abi.RAY)
    out["o"] = origins
    out["d"] = dirs
    if ids is None:
        w = MAX_DIM if w is None else int(w)
        if w < 1:
            raise ValueError("w must be positive")
        i = np.arange(n, dtype=np.uint64)
        out["x"] = (i % np.uint64(w)).astype(np.uint32)
        out["y"] = (i // np.uint64(w)).astype(np.uint32)
    else:
        ids = np.asarray(ids)
        if ids.shape != (n, 2) or (n and (ids.min() < 0 or ids.max() > 0xFFFFFFFF)):
            raise ValueError("ids must be (n, 2) unsigned 32-bit values")
        out["x"] = ids[:, 0].astype(np.uint32)
        out["y"] = ids[:, 1].astype(np.uint32)
    return out


def as_floats(rays):
    """_abi.RAY records → the same bits as (n, 8) float32: what a torch tensor for renderRays holds
    (``torch.from_numpy(as_floats(r)).cuda()``)."""
    return np.ascontiguousarray(rays, dtype=_abi.RAY).reshape(-1).view(f32).reshape(-1, 8)


def basis(yaw=0.0, pitch=0.0):
    """(W, U, V) of the Camera class for yaw / pitch in degrees, float64."""
    ry, rp = np.radians(float(yaw)), np.radians(float(pitch))
    w = np.array([np.cos(rp) * np.sin(ry), np.sin(rp), np.cos(rp) * np.cos(ry)])
    up = np.array([0.0, -1.0, 0.0])
    u = np.cross(w, up)
    u /= np.linalg.norm(u)
    return w, u, np.cross(u, w)


def _offset(offset):
    dx, dy = (float(v) for v in np.asarray(offset, dtype=np.float64).reshape(-1)[:2])
    if not (np.isfinite(dx) and np.isfinite(dy)):
        raise ValueError("offset must be finite")
    return dx, dy


def _grid(w, h, centre=True, offset=(0.0, 0.0)):
    """(s, t) of every pixel, row-major; `offset` = (dx, dy) in pixel units is added to the sampling point (0, 0: the
    centre itself, bit for bit)."""
    w, h = int(w), int(h)
    if not (1 <= w <= MAX_DIM and 1 <= h <= MAX_DIM):
        raise ValueError("frame size outside 1..%d" % MAX_DIM)
    off = 0.5 if centre else 0.0
    dx, dy = _offset(offset)
    s = (np.arange(w, dtype=np.float64) + (off + dx)) / w
    t = (np.arange(h, dtype=np.float64) + (off + dy)) / h
    ss, tt = np.meshgrid(s, t)   # (h, w): row-major, ray i = y * w + x
    return ss.reshape(-1), tt.reshape(-1)


def _unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def primary_rays(camera_block, w, h, offset=(0.0, 0.0)):
    """The pinhole camera's primary rays, normalize(llc + (x / w) hor + (y / h) ver) from the block's position, restated
    in float32 for convenience.  NOT the bit reference: the kernels form the direction with the selected policy's own
    normalize (take those bits from renderFeatures' `dir` where bits matter).  `offset` is added to x and y."""
    cam = np.asarray(camera_block, dtype=f32).reshape(12)
    s, t = _grid(w, h, centre=False, offset=offset)
    s, t = s.astype(f32), t.astype(f32)
    d = cam[3:6][None, :] + s[:, None] * cam[6:9][None, :] + t[:, None] * cam[9:12][None, :]
    d = d / np.sqrt((d * d).sum(axis=1, dtype=f32), dtype=f32)[:, None]
    return pack_rays(cam[0:3], d.astype(f32), w=w)


def equirect_rays(pos, w, h, yaw=0.0, offset=(0.0, 0.0)):
    """Equirectangular panorama from `pos`: column x is the longitude yaw + ((x + 0.5) / w - 0.5) 360 degrees, row y the
    latitude ((y + 0.5) / h - 0.5) 180 degrees along V — d = cos(lat) (sin(lon), 0, cos(lon)) + sin(lat) V with V = (0, -1, 0).  `offset` = (dx, dy) in pixel
    units moves the sampling point off the pixel centre, here and in every generator below (ray_sets)."""
    s, t = _grid(w, h, offset=offset)
    lon = np.radians(float(yaw)) + (s - 0.5) * (2.0 * np.pi)
    lat = (t - 0.5) * np.pi
    d = np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], axis=1)
    return pack_rays(pos, d, w=w)


def fisheye_rays(pos, w, h, fov_deg=180.0, yaw=0.0, pitch=0.0, offset=(0.0, 0.0)):
    """Equidistant fisheye: the image circle of radius min(w, h) / 2 spans fov_deg; a pixel at r radii from the centre
    looks r fov / 2 away from W, towards its own side of the frame (beyond the circle the angle goes on growing)."""
    s, t = _grid(w, h, offset=offset)
    W, U, V = basis(yaw, pitch)
    m = float(min(int(w), int(h)))
    px, py = (2.0 * s - 1.0) * (int(w) / m), (2.0 * t - 1.0) * (int(h) / m)
    r = np.hypot(px, py)
    a = r * np.radians(float(fov_deg)) * 0.5
    k = np.where(r > 0.0, np.sin(a) / np.where(r > 0.0, r, 1.0), 0.0)
    d = np.cos(a)[:, None] * W[None, :] + (k * px)[:, None] * U[None, :] + (k * py)[:, None] * V[None, :]
    return pack_rays(pos, _unit(d), w=w)


def orthographic_rays(pos, w, h, extent, yaw=0.0, pitch=0.0, offset=(0.0, 0.0)):
    """Orthographic view: every ray looks along W; the origins span `extent` world units along U (and extent h / w along V),
    centred on `pos`."""
    s, t = _grid(w, h, offset=offset)
    W, U, V = basis(yaw, pitch)
    e = float(extent)
    o = np.asarray(pos, dtype=np.float64).reshape(1, 3) + ((s - 0.5) * e)[:, None] * U[None, :] + \
        ((t - 0.5) * e * int(h) / int(w))[:, None] * V[None, :]
    d = np.broadcast_to(W.astype(f32), (len(s), 3))
    return pack_rays(o.astype(f32), d, w=w)


# cube-map faces in the usual order +x, -x, +y, -y, +z, -z: (forward, right, down) of each
CUBE_FACES = (((1, 0, 0), (0, 0, -1), (0, -1, 0)), ((-1, 0, 0), (0, 0, 1), (0, -1, 0)),
              ((0, 1, 0), (1, 0, 0), (0, 0, 1)), ((0, -1, 0), (1, 0, 0), (0, 0, -1)),
              ((0, 0, 1), (1, 0, 0), (0, -1, 0)), ((0, 0, -1), (-1, 0, 0), (0, -1, 0)))


def cubemap_rays(pos, face_size, offset=(0.0, 0.0)):
    """A cube-map probe at `pos`: six face_size x face_size faces (+x, -x, +y, -y, +z, -z), face f at rays
    [f n^2, (f + 1) n^2), d = normalize(forward + (2 s - 1) right + (2 t - 1) down) at the pixel centres — a frame of
    face_size x 6 face_size pixels."""
    n = int(face_size)
    s, t = _grid(n, n, offset=offset)
    out = []
    for fwd, right, down in CUBE_FACES:
        F, R, D = (np.asarray(v, dtype=np.float64) for v in (fwd, right, down))
        out.append(_unit(F[None, :] + (2.0 * s - 1.0)[:, None] * R[None, :] + (2.0 * t - 1.0)[:, None] * D[None, :]))
    return pack_rays(pos, np.concatenate(out), w=n)


# ---- ray sets (RayTracer.renderRaySets, rt_render_ray_sets): k records per ray, ray-major ------------------------------------
MAX_SET = _abi.RAY_SET_MAX


def ray_sets(generator, offsets, **kw):
    """An (n_rays, k) array of _abi.RAY records for renderRaySets: record (i, t) is ``generator(offset=offsets[t], **kw)``'s
    ray i — the ray through pixel i's sampling point moved by offsets[t] = (dx, dy) pixels — and all k records of ray i
    carry ray i's random-stream ids.  `offsets`: (k, 2), or Camera.sampleOffsets' (k, 4), of which (dx, dy) are the first
    two columns.  Sample s of a frame rendered through the sets looks through record s mod k."""
    offsets = np.asarray(offsets, dtype=np.float64)
    if offsets.ndim != 2 or offsets.shape[1] not in (2, 4) or not 1 <= len(offsets) <= MAX_SET:
        raise ValueError("offsets must be (k, 2) or (k, 4) with 1 <= k <= %d" % MAX_SET)
    cols = [np.ascontiguousarray(generator(offset=(o[0], o[1]), **kw), dtype=_abi.RAY).reshape(-1) for o in offsets]
    out = np.stack(cols, axis=1)
    out["x"], out["y"] = cols[0]["x"][:, None], cols[0]["y"][:, None]
    return out


def thin_lens(sets, U, V, aperture, focus, lens_points):
    """Depth of field for any projection: record (i, t) = (o, d), d of unit length, becomes
        o' = o + a (lx U + ly V),   d' = normalize(o + F d - o')
    with a = aperture, F = focus and (lx, ly) = lens_points[t], a point of the unit disk ((k, 2), or Camera.sampleOffsets'
    (k, 4), of which (lx, ly) are the last two columns); U, V span the lens.  The point at distance F along the ray stays
    where it is: what lies there is sharp.  float64, rounded once; ids unchanged; aperture 0 returns the input bits."""
    sets = np.ascontiguousarray(sets, dtype=_abi.RAY)
    if sets.ndim != 2:
        raise ValueError("sets must be (n_rays, k)")
    lens = np.asarray(lens_points, dtype=np.float64)
    if lens.ndim != 2 or lens.shape[1] not in (2, 4) or len(lens) != sets.shape[1]:
        raise ValueError("lens_points must be (k, 2) or (k, 4) with k = the set size")
    out = sets.copy()
    a, F = float(aperture), float(focus)
    if a == 0.0:
        return out
    if not F > 0.0:
        raise ValueError("focus must be positive")
    U, V = (np.asarray(v, dtype=np.float64).reshape(3) for v in (U, V))
    shift = a * (lens[:, -2, None] * U[None, :] + lens[:, -1, None] * V[None, :])     # (k, 3)
    o = sets["o"].astype(np.float64)
    o2 = o + shift[None, :, :]
    d2 = o + F * sets["d"].astype(np.float64) - o2
    d2 /= np.linalg.norm(d2, axis=-1, keepdims=True)
    out["o"], out["d"] = o2.astype(f32), d2.astype(f32)
    return out


# ---- hemisphere sets (RayTracer.occludedRays, rt_occluded_rays): k directions about a surface normal, ray-major --------------
def hemisphere_sets(points, normals, k, seed, offset=0.0):
    """An (n, k) array of _abi.RAY records for occludedRays (ambient occlusion, visibility bakes): record (i, t) starts at
    points[i] + offset * n_i and leaves along a cosine-weighted direction about n_i = normals[i] / |normals[i]| — Malley's
    method on the uniforms (u, v) = workloads.uniforms(n * k, 0, seed)[i * k + t, :2]: the disk point sqrt(u) (cos 2 pi v,
    sin 2 pi v) lifted to height sqrt(1 - u) > 0 over the tangent plane.  Deterministic in (points, normals, k, seed);
    float64, rounded once: directions are unit length to 1e-6 and dot(n_i, d) > 0.  The ids are (i, 0)."""
    from . import workloads
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    k = int(k)
    if len(p) != len(nrm) or not 1 <= k <= MAX_SET:
        raise ValueError("hemisphere_sets takes n points, n normals and 1 <= k <= %d" % MAX_SET)
    n = len(p)
    length = np.linalg.norm(nrm, axis=1, keepdims=True)
    if n and not (length > 0).all():
        raise ValueError("a normal of length 0 has no hemisphere")
    nrm = nrm / length
    # a tangent frame: the world axis the normal leans on least, made perpendicular to it
    axis = np.eye(3)[np.argmin(np.abs(nrm), axis=1)]
    tan = np.cross(nrm, axis)
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    bit = np.cross(nrm, tan)
    u = workloads.uniforms(n * k, 0, int(seed))[:, :2].astype(np.float64).reshape(n, k, 2)
    rad, phi = np.sqrt(u[..., 0]), 2.0 * np.pi * u[..., 1]
    d = ((rad * np.cos(phi))[..., None] * tan[:, None, :] + (rad * np.sin(phi))[..., None] * bit[:, None, :] +
         np.sqrt(1.0 - u[..., 0])[..., None] * nrm[:, None, :])
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    out = np.zeros((n, k), dtype=_abi.RAY)
    out["o"] = (p + float(offset) * nrm).astype(f32)[:, None, :]
    out["d"] = d.astype(f32)
    out["x"] = (np.arange(n, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    return out
