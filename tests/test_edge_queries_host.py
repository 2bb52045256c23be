"""CPU: the reference side of tests/test_gpu_edge_queries.py — the degenerate scenes of tests/edge_scenes.py under the ray
batch of tests/edge_rays.py and under feature chains.

1. The oracle's hitScene over the batch is the compiled reference's, bit for bit, through the digest mechanism of
   tests/test_oracle_vs_ref.py (keys `edgerays/<scene>`).  The reference never writes u, v and tex of a hit that is not on a
   mesh (oracle/pt_oracle.c, hit_scene), and nothing of a miss but the flag: those words are zeroed on both sides.
2. The batch covers what the GPU test relies on: every hit's t is finite, >= 1 000 hits, with ray_queries_ref.cycled_bounds
   >= 1 000 occluded records and >= 1 000 records that hit and are not occluded, >= 16 of the special rays hit — and
   >= 1 000 misses, except in the three scenes where a miss cannot exist: in `lenses`, `nested_spheres` and
   `nested_spheres_bvh` every origin of the batch lies within 16 units of the centre of the light sphere (0, 0, 0), r = 50,
   and hit_sphere's t = b + sqrt(b^2 + r^2 - |oc|^2) is then between sqrt(2500 - 256) > 47 and 2 |b| + 50 < 1000 whatever
   the direction, (0, 0, 0) and the scaled ones included (|b| <= 16 |d|, |d| <= 2 sqrt 2).  There the test asserts that
   no ray misses (measured: 0 of 12 396, 12 504, 12 612); the records that hit without being occluded carry the negative
   answers.
3. tests/chain_ref.py's two identification rules name the same object and face for every hit wherever the geometric rule
   (`identify`) completes, and with the probe rule (`identify_by_probe`) the chain replay completes on all twelve scenes.
   `identify` ends on its own assertion "a hit point on two primitives of one material" where the 72 ordinary spheres of
   the _bvh scenes overlap at a hit: coincident_spheres_bvh at every (follow, max_chain), nested_spheres_bvh once chains
   are followed far enough."""
import numpy as np
import pytest

import cases
import chain_ref as CH
import edge_rays as ER
import edge_scenes as E
import ray_queries_ref as Q
from test_oracle_vs_ref import _same_as_reference, ref  # noqa: F401  (`ref` is the fixture)

rt = cases.rt
A = rt._abi
F32 = np.float32
FOLLOW_ALL = rt.FOLLOW_ALL
CHAINS = ((0, 0), (FOLLOW_ALL, 3), (FOLLOW_ALL, 30))
# where `identify` does not complete, as measured on the CPU oracle; at (FOLLOW_ALL, 3) it may or may not on these scenes
IDENTIFY_FAILS = {("coincident_spheres_bvh", (0, 0)), ("coincident_spheres_bvh", (FOLLOW_ALL, 30)),
                  ("nested_spheres_bvh", (FOLLOW_ALL, 30))}
IDENTIFY_MAY_FAIL = IDENTIFY_FAILS | {("coincident_spheres_bvh", (FOLLOW_ALL, 3)), ("nested_spheres_bvh", (FOLLOW_ALL, 3))}
TWO_PRIMITIVES = "a hit point on two primitives of one material"
ENCLOSED = ("lenses", "nested_spheres", "nested_spheres_bvh")     # every origin deep inside the light sphere: no miss exists

_batches = {}


def batch(oracle, name):
    """(rays (n, 6), the oracle's hitScene records (n, 12)) of a scene, made once and left unchanged"""
    if name not in _batches:
        s, cam = E.get(name)
        rays6 = ER.edge_rays(oracle, s, cam)
        rays6.setflags(write=False)
        out = ER.scene_hits(oracle, s, rays6)
        out.setflags(write=False)
        _batches[name] = rays6, out
    return _batches[name]


def defined_words(probes, scene, rays6, out):
    """`out` with the words the reference leaves unwritten set to zero: all but the flag of a miss, u, v and tex of a hit
    that is not on a mesh (which hits are, the probe rule says)."""
    out = np.array(out, F32)
    hit = out[:, 0] > 0
    out[~hit, 1:] = 0
    obj, _ = CH.identify_by_probe(probes, scene, rays6[hit], out[hit], np.zeros(int(hit.sum()), bool))
    plain = np.nonzero(hit)[0][(obj >> np.uint32(CH.KIND_SHIFT)) != 3]
    out[plain, 8:11] = 0
    return out


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_hit_scene_over_the_edge_rays_is_the_compiled_reference(name, oracle, ref, table):  # noqa: F811
    s, cam = E.get(name)
    rays6, out = batch(oracle, name)
    probes = CH.OracleProbes(oracle, s, table)
    ours = defined_words(probes, s, rays6, out)

    def reference():
        return defined_words(probes, s, rays6, ref.hit(3, s, rays6, np.zeros(len(rays6), np.uint32)))

    _same_as_reference("edgerays/" + name, ours, ref and reference)


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_the_edge_rays_cover_hits_misses_and_both_answers(name, oracle):
    s, cam = E.get(name)
    rays6, out = batch(oracle, name)
    assert rays6.dtype == F32 and rays6.shape[1] == 6 and np.isfinite(rays6).all()
    assert 9000 <= len(rays6) <= 13000
    hit = out[:, 0] > 0
    assert np.isfinite(out[hit, 1]).all()
    t = Q.first_hit_t(oracle, s, rays6)
    assert np.array_equal(np.isfinite(t), hit)
    bounds = Q.cycled_bounds(t)
    occ = Q.occluded(t, bounds)
    special = ER.special_index(s, cam, len(rays6))
    assert (rays6[special, 3:] == np.tile(ER.DIRECTIONS, (len(special) // len(ER.DIRECTIONS), 1))).all()
    zero = (rays6[:, 3:] == 0).all(1)
    print(name, "rays", len(rays6), "hits", int(hit.sum()), "misses", int((~hit).sum()), "occluded", int(occ.sum()),
          "hit, not occluded", int((hit & ~occ).sum()), "special", len(special), "of which hit", int(hit[special].sum()),
          "zero directions", int(zero.sum()), "of which hit", int(hit[zero].sum()))
    assert hit.sum() >= 1000
    if name in ENCLOSED:
        far = np.linalg.norm(rays6[:, :3].astype(np.float64) - s.spheres["pos"][0, :3].astype(np.float64), axis=1).max()
        assert s.spheres["r"][0] == 50 and far <= 16.0, far
        assert hit.all()
    else:
        assert (~hit).sum() >= 1000
    assert occ.sum() >= 1000 and (hit & ~occ).sum() >= 1000
    assert hit[special].sum() >= 16
    assert zero.sum() == 4 * (len(special) // len(ER.DIRECTIONS))
    # the scaled copies leave the sphere BVH's gate |d.d - 1| < 0.25 on both sides, the first copy stays inside it
    dd = (rays6[:, 3:].astype(np.float64) ** 2).sum(1).reshape(4, -1)
    prim = E.W * E.H
    assert (np.abs(dd[0, :prim] - 1) < 1e-6).all() and (np.abs(dd[1, :prim] - 1.21) < 1e-5).all()
    assert (dd[2, :prim] > 3.9).all() and (dd[3, :prim] < 1e-5).all()


def primary(name):
    s, cam = E.get(name)
    return s, np.asarray(cam, F32).reshape(12)[:3], ER.primary(cam)[:, 3:]


@pytest.mark.parametrize("name", sorted(E.SCENES))
def test_both_identification_rules_agree_and_the_probe_rule_always_completes(name, oracle, table):
    s, eye, dirs = primary(name)
    probes = CH.OracleProbes(oracle, s, table)
    for combo in CHAINS:
        follow, max_chain = combo
        state = {"geometric": True, "compared": 0}

        def both(probe, scene, rays, out, want_face):
            obj, face = CH.identify_by_probe(probe, scene, rays, out, want_face)
            if state["geometric"]:
                try:
                    with np.errstate(invalid="ignore", divide="ignore"):     # (plane_normals: the zero normal's length)
                        o2, f2 = CH.identify(probe, scene, rays, out, want_face)
                except AssertionError as e:
                    assert TWO_PRIMITIVES in str(e), e
                    state["geometric"] = False                              # it does not complete: nothing more to compare
                else:
                    assert np.array_equal(obj, o2) and np.array_equal(face, f2), (name, combo)
                    state["compared"] += len(obj)
            return obj, face

        rec, chain = CH.replay(probes, s, eye, dirs, follow, max_chain, identify=both)
        f = A.split_features(rec)
        n = f["chain_length"]
        print(name, combo, "hits", int(f["hit"].sum()), "longest chain", int(n.max()), "cut", int(f["cut"].sum()),
              "identify completes", state["geometric"], "hits compared", state["compared"])
        if (name, combo) in IDENTIFY_FAILS:
            assert not state["geometric"]
        elif (name, combo) not in IDENTIFY_MAY_FAIL:
            assert state["geometric"] and state["compared"] >= f["hit"].sum() > 0
        assert (n <= max_chain).all()
        for r, c in zip(rec, chain):
            assert ((int(r["flags"]) >> 8) & 31) == len(c) and (int(r["flags"]) & 0xFFFF0000) == (CH.signature(c) & 0xFFFF0000)
        if combo == (0, 0):
            assert (rec["flags"] & ~np.uint32(A.FEATURE_HIT) == 0).all()
        if name == "facing_mirrors" and max_chain:
            assert n.max() == max_chain and f["cut"].sum() >= 1000 and (n[f["cut"]] == max_chain).all()
        if name == "lenses" and max_chain:
            assert n.max() >= 3
