"""numpy restatement of rt_render_features_cameras' reduction (include/rt_amd.h): n per-sample feature records per pixel →
one record per pixel and the two coverage floats.  Written from the header's statement, not from the kernel: the
dominant (object, flags >> 8) group with its tie rule, the representative's discrete fields, the ten floats as the
xor-butterfly sum over the hit samples divided in float32, RT_FEATURE_MIXED.  Also the launcher's plan."""
import numpy as np

HIT, MIXED = 1, 4
SUMMED = ("pos", "t", "normal", "albedo")      # ten floats
CAMERAS_MAX, MAX_DIM = 64, 16384


def glog2_for(n):
    g = 0
    while (1 << g) < n:
        g += 1
    return g


def plan(width, height, n):
    """rt_debug_plan_feature_cameras: one lane per sample, 2^glog2 lanes per pixel, whole pixels per 256-thread workgroup."""
    g = glog2_for(n)
    per_wg = 256 >> g
    return g, (width * height + per_wg - 1) // per_wg, 256


def butterfly_sum(v):
    """v: float32[g, ...], g a power of two → lane 0's value after the steps v[l] += v[l ^ off], off = g/2 .. 1."""
    v = np.array(v, dtype=np.float32)
    g = v.shape[0]
    idx = np.arange(g)
    off = g >> 1
    while off:
        v = (v + v[idx ^ off]).astype(np.float32)
        off >>= 1
    return v[0]


def votes(records):
    """records[n, P] → (j*[P], m[P], c[P], keys[n, P] as uint64)."""
    n = records.shape[0]
    keys = (records["object"].astype(np.uint64) << np.uint64(32)) | (records["flags"] >> 8).astype(np.uint64)
    count = (keys[:, None, :] == keys[None, :, :]).sum(1)                         # [n, P]: the size of sample j's group
    best = (count.astype(np.int64) << 6) | (63 - np.arange(n, dtype=np.int64))[:, None]
    top = best.max(0)
    hit = (records["flags"] & HIT) != 0
    return 63 - (top & 63), top >> 6, hit.sum(0), keys


def aggregate(records, n):
    """records: FEATURE records [n, P] (sample j, pixel p) → (records[P], coverage[P, 2] float32)."""
    records = np.asarray(records)
    assert records.shape[0] == n and 1 <= n <= CAMERAS_MAX and records.ndim == 2
    P = records.shape[1]
    g = 1 << glog2_for(n)
    jstar, m, c, _ = votes(records)
    out = records[jstar, np.arange(P)].copy()           # every field of the representative, the miss values included
    hit = (records["flags"] & HIT) != 0                 # [n, P]
    rep_hit = (out["flags"] & HIT) != 0
    cf = np.maximum(c, 1).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in SUMMED:
            v = records[f].astype(np.float32)
            v = v.reshape(n, P, -1)
            lanes = np.zeros((g,) + v.shape[1:], np.float32)                       # (+0 in the lanes without a sample)
            lanes[:n] = np.where(hit[:, :, None], v, np.float32(0.0))
            q = (butterfly_sum(lanes) / cf[:, None]).astype(np.float32)
            cur = out[f].reshape(P, -1)
            out[f] = np.where(rep_hit[:, None], q, cur).reshape(out[f].shape)
    out["flags"] = out["flags"] | np.where(m < n, MIXED, 0).astype(np.uint32)
    cov = np.stack([c.astype(np.float32) / np.float32(n), m.astype(np.float32) / np.float32(n)], axis=-1).astype(np.float32)
    return out, cov


def census(records):
    """What a set of per-sample records [n, P] covers: pixels with more than one key, pixels with hit and miss samples,
    pixels whose dominant group is decided by the smallest-j rule (two or more groups of the largest size)."""
    n = records.shape[0]
    jstar, m, c, keys = votes(records)
    count = (keys[:, None, :] == keys[None, :, :]).sum(1)
    largest = count == m[None, :]                        # samples inside a group of the largest size
    tied = largest.sum(0) > m                            # more such samples than one group holds
    return dict(mixed=int((m < n).sum()), hit_and_miss=int(((c > 0) & (c < n)).sum()), ties=int(tied.sum()))
