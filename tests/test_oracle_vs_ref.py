"""CPU: the oracle (C restatement) against the compiled reference kernel (oracle/_ref) on fresh
random inputs.  Where oracle/_ref is built, bit for bit against the reference itself; everywhere,
against the SHA-256 of the reference's output bits on the same inputs, recorded in
tests/golden/oracle_vs_ref.json.  To re-record (needs oracle/_ref):

    RT_RECORD_REF_DIGESTS=1 python -m pytest tests/test_oracle_vs_ref.py
"""
import hashlib
import json
import os

import numpy as np
import pytest

import cases
from oracle import Reference

DIGESTS = os.path.join(cases.ROOT, "tests", "golden", "oracle_vs_ref.json")
RECORD = bool(os.environ.get("RT_RECORD_REF_DIGESTS"))


def _digest(a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return hashlib.sha256(repr(a.shape).encode() + a.view(np.uint32).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def ref():
    if RECORD:
        assert Reference.available(), "RT_RECORD_REF_DIGESTS needs oracle/_ref/libref.so"
    return Reference() if Reference.available() else None


def _same_as_reference(key, ours, reference):
    """`ours` (the oracle's output) bit for bit against the reference's: `reference()` where the compiled reference
    exists, and always against the recorded digest of its output."""
    if reference is not None:
        a = reference()
        assert np.array_equal(a.view(np.uint32), ours.view(np.uint32)), key
        if RECORD:
            recorded = json.load(open(DIGESTS)) if os.path.isfile(DIGESTS) else {}
            recorded[key] = _digest(a)
            with open(DIGESTS, "w") as f:
                json.dump(recorded, f, indent=1, sort_keys=True)
                f.write("\n")
    assert _digest(ours) == json.load(open(DIGESTS))[key], key


@pytest.mark.parametrize("name,kw", [
    ("all_kinds", dict(width=200, height=120)),
    ("c2", dict(width=160, height=90)),
    ("c3", dict(width=160, height=90, tex_size=32)),
    ("c4", dict(width=64, height=36, n_spheres=500)),
    ("c5", dict(width=64, height=36, segments=12, rings=8)),
])
def test_progressive_frames_bit_exact(name, kw, oracle, ref, table):
    wl = cases.rt.workloads.get(name, **kw)
    b, _ = oracle.render(wl.scene, wl.camera, table, wl.width, wl.height, 2, count=6, threads=4)
    _same_as_reference("progressive/" + name, b, ref and (
        lambda: ref.progressive(wl.scene, wl.camera, table, wl.width, wl.height, 6, threads=4)))


def test_random_probes_other_seed_and_camera(oracle, ref):
    table = oracle.make_random_table(12345)
    wl = cases.rt.workloads.get("all_kinds", width=333, height=211)
    cam = cases.rt.Camera(75, 333 / 211, (-5.0, -2.5, -9.0), 30.0, 12.0).transferData()
    rng = np.random.RandomState(7)
    n = 20000
    xs, ys, ss = rng.randint(0, 333, n), rng.randint(0, 211, n), rng.randint(0, 65535, n)
    b, _ = oracle.samples(wl.scene, cam, table, 333, 211, xs, ys, ss)
    _same_as_reference("probes", b, ref and (lambda: ref.samples(wl.scene, cam, table, 333, 211, xs, ys, ss)))
    assert (b.sum(1) > 0).mean() > 0.2  # the probes are not all black


def test_camera_inside_glass_and_grazing(oracle, ref, table):
    """Origins inside the refractive sphere / lens and a camera skimming the floor."""
    wl = cases.rt.workloads.get("all_kinds", width=96, height=64)
    for i, (pos, yaw, pitch) in enumerate((((0.25, 3.1, 0.1), 10.0, 5.0), ((5.2, 0.4, 0.3), 200.0, -20.0),
                                           ((0, 4.99, -9), 0.0, 0.5))):
        cam = cases.rt.Camera(60, 1.5, pos, yaw, pitch).transferData()
        b, _ = oracle.render(wl.scene, cam, table, 96, 64, 2, count=3, threads=4)
        _same_as_reference("camera/%d" % i, b, ref and (lambda: ref.progressive(wl.scene, cam, table, 96, 64, 3, threads=4)))


def test_unit_vectors_ten_thousand_per_routine(oracle, ref, table):
    """10^4 random (ray, primitive) pairs per intersection routine and 10^4 records per material
    routine, oracle against the compiled reference kernel, bit for bit (fresh streams, not the committed ones)."""
    wl = cases.workload("all_kinds")
    n = 10000
    for i, kind in enumerate(("sphere", "plane", "lens")):
        rays, prim, _ = cases.unit_rays(kind, wl.scene, n, 300 + 10 * i)
        _same_as_reference("hit/" + kind, oracle.hit(i, wl.scene, rays, prim),
                           ref and (lambda: ref.hit(i, wl.scene, rays, prim)))
    rays, mesh, face = cases.unit_rays("triangle", wl.scene, n, 340)
    _same_as_reference("hit/triangle", oracle.hit_triangle(wl.scene, rays, mesh, face),
                       ref and (lambda: ref.hit_triangle(wl.scene, rays, mesh, face)))
    for i, routine in enumerate(cases.MATERIAL_ROUTINES):
        vec = cases.material_vectors(wl.scene, n, 400 + 10 * i, routine)
        _same_as_reference("material/" + routine, oracle.material(i, wl.scene, table, vec),
                           ref and (lambda: ref.material(i, wl.scene, table, vec)))
