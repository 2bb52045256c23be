"""The float64 reference of rt_occluded_hemispheres' rays (tests/test_hemispheres_host.py, tests/test_gpu_hemispheres.py):
which records have a hemisphere, the face-forward rule, then rays.hemisphere_sets — the generator the kernel restates in
binary32 — plus the hand-made feature buffer of the generator test."""
import numpy as np

import cases

rt = cases.rt
A = rt._abi
F32 = np.float32


def valid_mask(features):
    """(n,) bool: the record has RT_FEATURE_HIT and a normal of finite, non-zero length."""
    f = np.asarray(features).reshape(-1)
    nrm = f["normal"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt((nrm * nrm).sum(1))
    return ((f["flags"] & A.FEATURE_HIT) != 0) & np.isfinite(length) & (length > 0)


def facing_normals(features, face_forward):
    """(n, 3) float64: the normal the hemisphere stands on — the record's, negated under face_forward where
    dot(normal, dir) > 0 (evaluated in float64; the test data keeps that dot product away from 0)."""
    f = np.asarray(features).reshape(-1)
    nrm = f["normal"].astype(np.float64)
    if face_forward:
        with np.errstate(invalid="ignore"):
            flip = (nrm * f["dir"].astype(np.float64)).sum(1) > 0
        nrm = np.where(flip[:, None], -nrm, nrm)
    return nrm


def hemisphere_rays(features, k, seed, offset=0.0, face_forward=False):
    """→ (mask, sets): valid_mask and the (n, k) _abi.RAY records rt_occluded_hemispheres is specified against — rays.
    hemisphere_sets on every valid record (counter i * k + t whatever the records before i are), all-zero bytes elsewhere."""
    f = np.asarray(features).reshape(-1)
    mask = valid_mask(f)
    nrm = facing_normals(f, face_forward)
    nrm[~mask] = (0.0, 0.0, 1.0)                       # (a placeholder: hemisphere_sets refuses a zero normal)
    pos = np.where(mask[:, None], f["pos"].astype(np.float64), 0.0)
    sets = rt.rays.hemisphere_sets(pos, nrm, k, seed, offset)
    sets[~mask] = np.zeros((), dtype=A.RAY)
    return mask, sets


def unit_normals(features, face_forward):
    nrm = facing_normals(features, face_forward)
    with np.errstate(invalid="ignore", divide="ignore"):
        return nrm / np.sqrt((nrm * nrm).sum(1, keepdims=True))


def record(pos, normal, direction=(0.0, 0.0, -1.0), hit=True):
    r = np.zeros((), dtype=A.FEATURE)
    r["pos"], r["normal"], r["dir"] = pos, normal, direction
    r["t"] = 1.0 if hit else np.inf
    r["flags"] = A.FEATURE_HIT if hit else 0
    return r


def generator_records(pad_to=0):
    """The hand-made records of the generator test: normals along the six axes, with two equal smallest components,
    scaled by 3 and by 1e-3, zero and NaN; with and without RT_FEATURE_HIT; `dir` on both sides of the normal.  Padded
    with oblique records (Philox normals) up to pad_to records, so that counters beyond 2^16 are met."""
    recs = []
    eye = np.eye(3)
    for s in (1.0, -1.0):
        for a in range(3):
            for side in (1.0, -1.0):
                recs.append(record((a, s, side), s * eye[a], side * s * eye[a] + (0.25, 0.5, -0.125)))
    for normal in ((0.5, 0.5, 0.70710678), (0.6, -0.6, 0.2), (-0.2, 0.7, 0.2), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 1.0, 1.0),
                   (0.3, -0.3, -0.3)):
        for scale in (1.0, 3.0, 1e-3):
            for side in (1.0, -1.0):
                nrm = np.array(normal) * scale
                recs.append(record((1.5, -2.25, 7.0), nrm, side * np.array(normal) + (0.01, -0.02, 0.03)))
    recs.append(record((1, 2, 3), (0, 0, 0)))
    recs.append(record((1, 2, 3), (np.nan, 0, 1)))
    recs.append(record((1, 2, 3), (0, np.inf, 0)))
    recs.append(record((1, 2, 3), (0, 1, 0), hit=False))
    recs.append(record((4, 5, 6), (0, 1, 0)))
    out = np.array(recs, dtype=A.FEATURE)
    if pad_to > len(out):
        m = pad_to - len(out)
        u = rt.workloads.uniforms(m, 9, cases.SEED).astype(np.float64)
        pad = np.zeros(m, dtype=A.FEATURE)
        pad["normal"] = (2 * u[:, :3] - 1).astype(F32)
        pad["pos"] = (8 * rt.workloads.uniforms(m, 10, cases.SEED)[:, :3] - 4).astype(F32)
        pad["dir"] = (2 * rt.workloads.uniforms(m, 11, cases.SEED)[:, :3] - 1).astype(F32)
        pad["t"], pad["flags"] = 1.0, A.FEATURE_HIT
        pad["flags"][::7] = 0                          # misses in between
        out = np.concatenate([out, pad])
    return out
