"""Host restatements for the wave's fixed cost (csrc/pt_queue.hpp stage_xy, csrc/pt_device.hpp stage_tables): the staged
scene block from a scene's arrays, and queue_stage's division-free tile quotient in float32."""
import numpy as np

import cases

A = cases.rt._abi
f32 = np.float32


def schlick_r0(ratio):
    r0 = (f32(1.0) - ratio) / (f32(1.0) + ratio)
    return r0 * r0


def stage_block(scene):
    """The staged scene block of `scene` (a SceneCreator) in IEEE float32, (rows, 4): what stage_tables writes under the
    `ieee` policy (correctly rounded divisions).  A light's extra_data of 0 gives inf and NaN entries, as on the device."""
    m, s, p = scene.materials, scene.spheres, scene.planes
    m0, w0, p0, rows = A.stage_block_layout(len(m), len(s), len(p))
    out = np.zeros((rows, 4), dtype=f32)
    words = out.view(np.uint32)
    with np.errstate(divide="ignore", invalid="ignore"):
        if w0 > m0:
            extra = m["extra_data"].astype(f32)
            inv = f32(1.0) / extra
            out[m0:w0:2, :3] = m["color"][:, :3]
            out[m0:w0:2, 3] = extra
            words[m0 + 1:w0:2, 0] = m["type"].astype(np.uint32)
            out[m0 + 1:w0:2, 1] = inv
            out[m0 + 1:w0:2, 2] = schlick_r0(extra)
            out[m0 + 1:w0:2, 3] = schlick_r0(inv)
    if p0 > w0:
        out[w0:p0:2, :3] = s["pos"][:, :3]
        out[w0:p0:2, 3] = s["r"]
        words[w0 + 1:p0:2, 0] = s["mat_ID"]
    if rows > p0:
        out[p0:rows, :3] = p["normal"][:, :3]
        words[p0:rows, 3] = p["mat_ID"]
    return out


def same_block(got, ref):
    """Equal as uint32 wherever the reference is a number; a NaN where it is a NaN (payload and sign are not pinned)."""
    nan = np.isnan(ref)
    return got.shape == ref.shape and bool(np.isnan(got[nan]).all()) and \
        np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan])


XY_FAST_MAX_TILES = 1 << 20   # PT_XY_FAST_MAX_TILES


def tile_quotient(t, tiles_x, rcp):
    """stage_xy's quotient: (uint32)(((float)t + 0.5f) * rcp), every step rounded to float32 as the device rounds it."""
    t = np.asarray(t, dtype=np.uint32)
    return ((t.astype(f32) + f32(0.5)) * f32(rcp)).astype(np.uint32)
