"""CPU: the degenerate scenes of tests/edge_scenes.py — the oracle against the compiled reference, bit for bit, through
the digest mechanism of tests/test_oracle_vs_ref.py (keys `edge/...`): samples 0-3 of every pixel.  The reference produces
no NaN or Inf on any of them, every scene is lit, and the acceleration structures built for them pass
rt_debug_check_accel (every leaf reached exactly once by the kernels' threaded walks, boxes of no extent included)."""
import numpy as np
import pytest

import cases
import edge_scenes as E
from test_oracle_vs_ref import _same_as_reference, ref  # noqa: F401  (`ref` is the fixture)

rt = cases.rt
SAMPLES = 4


def all_pixels(sample):
    ys, xs = np.mgrid[0:E.H, 0:E.W]
    return xs.ravel(), ys.ravel(), np.full(xs.size, sample, np.uint32)


def oracle_samples(oracle, name, table):
    """(SAMPLES, H * W, 3) linear radiance and the summed counters."""
    s, cam = E.get(name)
    out, bounces = [], 0
    for k in range(SAMPLES):
        a, cn = oracle.samples(s, cam, table, E.W, E.H, *all_pixels(k))
        out.append(a)
        bounces += cn.bounces
    return np.stack(out), bounces


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_oracle_equals_the_compiled_reference(name, oracle, ref, table):  # noqa: F811
    s, cam = E.get(name)
    ours, bounces = oracle_samples(oracle, name, table)

    def reference():
        return np.stack([ref.samples(s, cam, table, E.W, E.H, *all_pixels(k)) for k in range(SAMPLES)])

    _same_as_reference("edge/" + name, ours, ref and reference)
    assert np.isfinite(ours).all(), name
    lit = (ours.sum(axis=2) > 0).mean()
    assert lit > 0.2, (name, lit)
    if name == "facing_mirrors":
        # a path that runs all DEPTH = 30 bounces searches the scene 30 times; the others end at the light after a few
        assert bounces >= 0.5 * rt._abi.DEPTH * ours.shape[0] * ours.shape[1], bounces
    b, _ = oracle.render(s, cam, table, E.W, E.H, 2, count=SAMPLES, threads=2)
    _same_as_reference("edge/" + name + "/progressive", b,
                       ref and (lambda: ref.progressive(s, cam, table, E.W, E.H, SAMPLES, threads=2)))


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_acceleration_structures_hold_their_invariants(built, name):
    s, _ = E.get(name)
    st = rt.check_accel(s)
    if name in E.SPHERE_BVH:
        assert len(s.spheres) >= 64 and st["sphere_leaves"] >= len(s.spheres) // 4
    if name in E.MESH_BVH:
        assert st["meshes"] == 1 and st["mesh_leaves"] >= int(s.meshes["face_count"][0]) // 2
    else:
        assert st["meshes"] == 0
