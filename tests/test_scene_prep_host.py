"""CPU: rt_set_scene uploads from, and rt_debug_check_accel checks, ONE prepared scene (csrc/scene_prep.hpp).  Pinned here
against the commit before that header existed (tests/golden/scene_prep.json): for every scene of
tests/scene_prep_scenes.py the self-check passes, its stats[0..6] are the old self-check's and the digest of the prepared
arrays is the digest of what the old rt_set_scene handed to upload().  Where the old self-check built a tree that
rt_set_scene does not (listed in the golden file under `no_tree_in_rt_set_scene`), the new one reports none."""
import json
import os

import numpy as np
import pytest

import cases
import scene_prep_scenes as S

rt = cases.rt
GOLD = json.load(open(os.path.join(cases.GOLDEN_DIR, "scene_prep.json")))
RT_ERANGE = -5   # include/rt_amd.h
KEYS = ("sphere_nodes", "sphere_leaves", "sphere_depth", "mesh_nodes", "mesh_leaves", "mesh_depth", "meshes")


def test_the_golden_file_names_every_scene():
    assert sorted(GOLD["scenes"]) == sorted(S.SCENES)
    assert sorted(GOLD["no_tree_in_rt_set_scene"]) == ["nan_sphere"]


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_prepared_scene_is_the_parents(built, name):
    gold = GOLD["scenes"][name]
    st = rt.check_accel(S.SCENES[name]())
    print(name, st)
    assert "0x%016x" % st["digest"] == gold["digest"]
    want = GOLD["no_tree_in_rt_set_scene"].get(name, gold)["stats"]
    assert [st[k] for k in KEYS] == want


def test_a_non_finite_sphere_means_no_sphere_tree(built):
    st = rt.check_accel(S.nan_sphere())
    assert (st["sphere_nodes"], st["sphere_leaves"], st["sphere_depth"]) == (0, 0, 0)
    assert GOLD["no_tree_in_rt_set_scene"]["nan_sphere"]["parent_stats"][0] > 0   # (the old self-check had built one)


def test_validation_errors_come_back_through_the_self_check(built):
    """The checks and messages of rt_set_scene: the self-check used to dereference such an index."""
    s = S.empty()
    s.addSphere((0, 0, 5), 1, 0)
    s.addSphere((0, 0, 9), 1, 7)
    with pytest.raises(rt.RtError) as e:
        rt.check_accel(s)
    assert e.value.code == RT_ERANGE and "sphere 1: material 7 does not exist" in str(e.value)
    s = S.threshold_31_32()
    s.indices = s.indices.copy()
    s.indices[40] = np.uint32(10 ** 6)
    with pytest.raises(rt.RtError) as e:
        rt.check_accel(s)
    assert e.value.code == RT_ERANGE and "mesh 0: vertex index 1000000 (+anchor 0) outside the vertex array" in str(e.value)
