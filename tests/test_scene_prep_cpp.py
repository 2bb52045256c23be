"""CPU: csrc/scene_prep.hpp as a stand-alone program (tests/host/scene_prep_main.cpp), compiled with g++ under
AddressSanitizer and UBSan and run as a child process on scene files written from scene.desc(): it ends clean and prints
the eight numbers the library gives — so the host compiler of hipcc (-O3) and g++ (-O1) build the same bytes from the
header, and the builders and the self-check touch nothing outside their arrays."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import edge_scenes as E
import scene_prep_scenes as S

rt = cases.rt
ROOT = cases.ROOT
GXX = shutil.which("g++") or "g++"


def rocm_include():
    """<rocm>/include, next to the bin/ of the hipcc the library is built with (the vector types only)."""
    import __graft_entry__ as g
    return os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(g.HIPCC))), "include")


NAMES = ["workload/c4_n_spheres=777", "adversarial_spheres", "degenerate_meshes"] + ["edge/" + e for e in sorted(E.SCENES)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scene_prep") / "scene_prep_main")
    subprocess.run([GXX, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I", rocm_include(), "-I", os.path.join(ROOT, "opencl-raytracing_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "scene_prep_main.cpp"), "-o", exe], check=True)
    return exe


def write_scene(scene, path):
    d = scene.desc()
    arrs = scene._keep   # (the contiguous arrays d points into, in rt_scene_desc's order)
    order = ("materials", "spheres", "planes", "lenses", "vertices", "uvs", "indices", "meshes", "models")
    counts = [d.material_count, d.sphere_count, d.plane_count, d.lens_count, d.vertex_count, d.uv_count, d.index_count,
              d.mesh_count, d.model_count, 0]
    assert counts[:9] == [len(arrs[k]) for k in order]
    with open(path, "wb") as fh:
        fh.write(np.asarray(counts, np.uint32).tobytes())
        for k in order:
            fh.write(arrs[k].tobytes())


@pytest.mark.parametrize("name", NAMES)
def test_standalone_program_under_sanitizers(built, program, name, tmp_path):
    scene = S.SCENES[name]()
    path = str(tmp_path / "scene.bin")
    write_scene(scene, path)
    p = subprocess.run([program, path], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.split()
    st = rt.check_accel(scene)
    keys = ("sphere_nodes", "sphere_leaves", "sphere_depth", "mesh_nodes", "mesh_leaves", "mesh_depth", "meshes")
    assert [int(v) for v in got[:7]] == [st[k] for k in keys]
    assert int(got[7], 16) == st["digest"]
