"""CPU: the surface of rt_render_features_chain that needs no device — the header in plain C, the exports, the chain
signature (rt_feature_chain_signature is the very function the kernel calls) against a numpy restatement, the chain's
restatement over the CPU oracle (tests/chain_ref.py) on C2, and the quality table: the numpy variance-guided filter
guided by first-hit records and by chain records with the pair key of RT_DENOISE_SPLIT_CHAINS."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import chain_ref as CH
import denoise_ref as R
import denoise_vg_ref as V
from test_denoise_vg_host import primary_dirs

rt = cases.rt
A = rt._abi
ROOT = cases.ROOT
NEW = ("rt_render_features_chain", "rt_feature_chain_signature")
EINVAL = -1


def test_header_compiles_in_plain_c(built, tmp_path):
    src = tmp_path / "chain.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_amd.h"\n'
                   'int main(void) {\n'
                   '    rt_feature_chain_params p = {RT_FOLLOW_REFLECTIVE | RT_FOLLOW_REFRACTIVE | RT_FOLLOW_DIELECTRIC, RT_FEATURE_CHAIN_MAX};\n'
                   '    float cam[12] = {0}; uint32_t o[2] = {0x80000001u, 7u}, s = 1u, f = 0xABCD1F00u | RT_FEATURE_CUT | RT_FEATURE_HIT;\n'
                   '    int rc = rt_feature_chain_signature(o, 2u, &s);\n'
                   '    printf("%u %u %d %u %u %u %u %x %d %d %u %d %d\\n", p.follow, p.max_chain, RT_ABI_VERSION, RT_FEATURE_CUT,\n'
                   '           RT_DENOISE_SPLIT_CHAINS, (unsigned)sizeof p, RT_FEATURE_CHAIN_LENGTH(f), RT_FEATURE_CHAIN_SIGNATURE(f),\n'
                   '           rt_render_features_chain(NULL, cam, &p), rc, s, rt_feature_chain_signature(o, 2u, NULL),\n'
                   '           rt_feature_chain_signature(NULL, 2u, &s));\n'
                   '    return 0;\n'
                   '}\n')
    exe = tmp_path / "chain"
    pkg = os.path.dirname(rt.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lrt_amd", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    sig = CH.signature([0x80000001, 7])
    assert out.stdout.split() == ["7", "29", "3", "2", "4", "8", "31", "abcd0000", "-1", "0", str(sig), "-1", "-1"]


def test_library_exports_the_new_symbols(built):
    lib = C.CDLL(rt.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in rt.raytracer.SYMBOLS
    assert rt.load_library().rt_abi_version() == 3
    assert (rt.FOLLOW_REFLECTIVE, rt.FOLLOW_REFRACTIVE, rt.FOLLOW_DIELECTRIC, rt.FOLLOW_ALL) == (1, 2, 4, 7)
    assert A.FEATURE_CUT == 2 and A.DENOISE_SPLIT_CHAINS == 4 and A.FEATURE_CHAIN_MAX == 29
    assert callable(rt.RayTracer.renderFeaturesChain)
    assert A.denoise_flags(True, True) == 5 and A.denoise_flags(False, True) == 4 and A.denoise_flags(True) == 1


@pytest.mark.parametrize("n", [0, 1, 30])
def test_signature_matches_the_restatement(built, n):
    rng = np.random.default_rng(n)
    for _ in range(20):
        obj = rng.integers(0, 1 << 30, size=n, dtype=np.uint32) | (rng.integers(0, 4, size=n, dtype=np.uint32) << np.uint32(30))
        if n:
            obj[rng.integers(0, n)] |= np.uint32(0xC0000000)      # bits 31..30 set: a mesh id
        assert rt.feature_chain_signature(obj) == CH.signature(obj)
        h = np.zeros(1, np.uint32)
        for o in obj:
            h = CH.signature_step(h, np.array([o], np.uint32))
        assert int(h[0]) == CH.signature(obj)
    if n == 0:
        assert rt.feature_chain_signature([]) == 0
    if n == 1:
        assert rt.feature_chain_signature([0xC0000005]) == ((0xC0000005 * 0x9E3779B1) & 0xFFFFFFFF)
        assert rt.feature_chain_signature([0]) == 0


def test_null_pointers_are_errors(built):
    lib = rt.load_library()
    o = (C.c_uint32 * 2)(1, 2)
    out = C.c_uint32(77)
    assert lib.rt_feature_chain_signature(o, 2, None) == EINVAL
    assert lib.rt_feature_chain_signature(None, 2, C.byref(out)) == EINVAL
    assert out.value == 77
    assert lib.rt_feature_chain_signature(None, 0, C.byref(out)) == 0 and out.value == 0    # nothing to read
    p = A.FeatureChainParams(7, 29)
    cam = np.zeros(12, np.float32)
    assert lib.rt_render_features_chain(None, cam.ctypes.data, C.byref(p)) == EINVAL
    assert b"NULL" in lib.rt_last_error(None)


def test_split_features_decodes_the_chain_fields():
    rec = np.zeros((1, 3), A.FEATURE)
    rec["flags"][0] = [A.FEATURE_HIT, A.FEATURE_HIT | A.FEATURE_CUT | (2 << 8) | 0xBEEF0000, (29 << 8) | 0x00010000]
    f = A.split_features(rec)
    assert f["hit"].tolist() == [[True, True, False]] and f["cut"].tolist() == [[False, True, False]]
    assert f["chain_length"].tolist() == [[0, 2, 29]]
    assert f["chain_signature"].tolist() == [[0, 0xBEEF0000, 0x00010000]]
    assert f["chain_word"].tolist() == [[0, 0x00BEEF02, 0x0000011D]]


# ---- the chain over the CPU oracle ---------------------------------------------------------------------------------------

def oracle_chain(oracle, table, wl, follow, max_chain):
    cam = rt.raytracer._cam_block(wl.camera)
    dirs = primary_dirs(cam, wl.width, wl.height).reshape(-1, 3)
    return CH.replay(CH.OracleProbes(oracle, wl.scene, table), wl.scene, cam[:3], dirs, follow, max_chain)


def test_oracle_chains_on_c2_cover_every_case(oracle, table):
    """The figures the GPU test's coverage conditions are set against (C2 64x36, all three glass-like types)."""
    wl = rt.workloads.get("c2", width=64, height=36)
    rec, chain = oracle_chain(oracle, table, wl, 7, 29)
    f = A.split_features(rec)
    n = f["chain_length"]
    types = wl.scene.materials["type"]
    on_light = f["hit"] & (n >= 1) & (types[np.where(f["hit"], f["material"], 0)] == A.T_LIGHT)
    sky = ~f["hit"] & (n >= 1)
    print("C2 64x36 mask 7: chain >= 1: %d, >= 2: %d, longest %d (%d pixels), end in the sky %d, on the light %d, cut %d" %
          ((n >= 1).sum(), (n >= 2).sum(), n.max(), (n == n.max()).sum(), sky.sum(), on_light.sum(), f["cut"].sum()))
    assert (n >= 1).sum() >= 100 and (n >= 2).sum() >= 50 and sky.sum() >= 20 and on_light.sum() >= 1
    assert not f["cut"].any()
    # the flags hold what the chain's objects give, and a terminal is never of a followed type unless cut
    for r, c in zip(rec, chain):
        assert ((int(r["flags"]) >> 8) & 31) == len(c) and (int(r["flags"]) & 0xFFFF0000) == (CH.signature(c) & 0xFFFF0000)
    term_t = types[f["material"][f["hit"]]]
    assert not np.isin(term_t, (A.T_REFLECTIVE, A.T_REFRACTIVE, A.T_DIELECTRIC)).any()
    assert np.isinf(f["depth"][~f["hit"]]).all() and np.isfinite(f["depth"][f["hit"]]).all()
    # max_chain 2 cuts the longer ones; the identity case
    rec2, _ = oracle_chain(oracle, table, wl, 7, 2)
    f2 = A.split_features(rec2)
    print("C2 64x36 mask 7, max_chain 2: cut %d" % f2["cut"].sum())
    assert f2["cut"].sum() >= 30 and (f2["chain_length"][f2["cut"]] == 2).all()
    first, _ = oracle_chain(oracle, table, wl, 0, 29)
    zero, _ = oracle_chain(oracle, table, wl, 7, 0)
    assert first.tobytes() == zero.tobytes() and (first["flags"] & ~np.uint32(1) == 0).all()
    same = f["chain_length"].reshape(-1) == 0
    assert rec[same].tobytes() == first[same].tobytes()


def gamma_rmse(lin, truth, sel):
    return float(np.sqrt(((np.sqrt(lin[sel]) - np.sqrt(truth[sel])) ** 2).mean()))


def test_quality_table_chain_guides_against_first_hit_guides(oracle, table):
    """gamma RMSE against 1024 spp of the noisy frame and of the variance-guided filter (defaults) guided by first-hit
    records and by chain records compared by the pair (key, flags >> 8), C2 128x72, on the whole frame and on the pixels
    with a chain.  Asserted: chain-guided beats noisy on the chain pixels.  Chain-guided against first-hit-guided is
    printed — the number DESIGN.md reports, not one to tune towards."""
    w, h = 128, 72
    wl = rt.workloads.get("c2", width=w, height=h)
    cam = rt.raytracer._cam_block(wl.camera)
    truth = oracle.linear_sum(wl.scene, cam, table, w, h, (0, 0, w, h), 0, 1024) / 1024.0
    first = A.split_features(oracle_chain(oracle, table, wl, 0, 0)[0].reshape(h, w))
    chain = A.split_features(oracle_chain(oracle, table, wl, 7, 29)[0].reshape(h, w))
    sub = chain["chain_length"] >= 1
    everything = np.ones((h, w), bool)
    assert sub.sum() >= 400
    ys, xs = np.mgrid[0:h, 0:w]
    spp = 16
    s, _ = oracle.samples(wl.scene, cam, table, w, h, np.repeat(xs.reshape(-1), spp), np.repeat(ys.reshape(-1), spp),
                          np.tile(np.arange(spp), w * h))
    s = s.reshape(h, w, spp, 3).astype(np.float64)
    kw = dict(A.DENOISE_VARIANCE_DEFAULTS)

    def run(acc, feats, split_chains):
        g = CH.with_pair_key(feats, kw["split_objects"], split_chains)
        return V.filter_linear(acc, g["normal"], g["position"], g["albedo"], g["hit"], g["object"],
                               **dict(kw, split_objects=True))[0]

    print("\n| spp | pixels | noisy | first-hit guides | chain guides |")
    print("|---:|---|---:|---:|---:|")
    for n in (4, 16):
        acc = np.concatenate([s[:, :, :n].sum(2), np.full((h, w, 1), float(n))], axis=-1).astype(np.float32)
        noisy = R.initial_colour(acc)
        by_first, by_chain = run(acc, first, False), run(acc, chain, True)
        rows = {}
        for name, sel in (("whole frame", everything), ("chain >= 1 (%d)" % sub.sum(), sub)):
            rows[name] = [gamma_rmse(x, truth, sel) for x in (noisy, by_first, by_chain)]
            print("| %d | %s | %.4f | %.4f | %.4f |" % ((n, name) + tuple(rows[name])))
        e_noisy, _, e_chain = rows["chain >= 1 (%d)" % sub.sum()]
        assert e_chain < e_noisy, (n, e_chain, e_noisy)


# ---- rt_cli -------------------------------------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "host", "rt_cli")


def _cli(*args):
    return subprocess.run([CLI, "--scene", os.path.join(ROOT, "assets", "scenes", "c1_sphere.scene"), *args],
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [
    ["--denoise", "--follow", "mirror"],
    ["--denoise", "--follow=mirror,glass,dielectric", "--max-chain", "4", "--split-chains"],
    ["--denoise", "--variance-guided", "--measured", "--follow", "dielectric,mirror", "--max-chain=0"],
    ["--follow", "glass", "--aov", "aov"],
    ["--denoise", "--follow", "glass", "--max-chain", "29", "--aov", "aov"],
])
def test_cli_accepts_follow(built, tmp_path, args):
    out = _cli(*args, "--dump-scene", str(tmp_path / "scene.bin"))
    assert out.returncode == 0, out.stderr
    assert (tmp_path / "scene.bin").stat().st_size > 0


@pytest.mark.parametrize("args", [
    ["--follow", "mirror"],                                          # neither --denoise nor --aov
    ["--denoise", "--follow", "mirror,wood"],
    ["--denoise", "--follow", ""],
    ["--denoise", "--follow", "mirror,"],
    ["--denoise", "--max-chain", "3"],                               # without --follow
    ["--denoise", "--split-chains"],
    ["--follow", "mirror", "--aov", "aov", "--split-chains"],        # the flag is the filters'
    ["--denoise", "--follow", "mirror", "--max-chain", "30"],
    ["--denoise", "--follow", "mirror", "--max-chain", "-1"],
])
def test_cli_rejects_bad_follow(built, tmp_path, args):
    out = _cli(*args, "--dump-scene", str(tmp_path / "scene.bin"))
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "--follow" in out.stderr
