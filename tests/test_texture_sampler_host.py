"""CPU: the texel fetch against an independent float64 statement of it (tests/texture_ref.py).

Three float32 copies are pinned here — texture_rgb of oracle/pt_oracle.c through whole samples (in the scenes of
tests/texture_cases.py a sample's radiance is the texel), the read_imagef stand-in of oracle/ref_shim.cpp through the
compiled reference (digests `texture/...`, the mechanism of tests/test_oracle_vs_ref.py), and chain_ref.texel — on
textures that are not square, 1 to 3 layers, uv inside [0, 1], across both edges, far outside, exactly 0 and 1 at the
vertices and at +-1e30.  Before the texel coordinate was clamped ahead of floor(), uv more than half a texel below 0 gave
a sawtooth of texels 0 and 1 instead of the edge texel (0.6 to 0.8 off on 10 to 17 % of a frame): the straddling and far
cases fail on that sampler."""
import numpy as np
import pytest

import cases
import chain_ref
import texture_cases as TC
import texture_ref as R
from test_oracle_vs_ref import _same_as_reference, ref  # noqa: F401  (`ref` is the fixture)

# err / (2^-24 * L) of the CPU oracle over all cases here: largest 1.12 (2x7-straddle; 0.98 on 64x64-straddle, 0.97 on
# 33x17-inside).  C is twice that.
C = 2.3
MIN_HIT, MAX_LEFT_OUT = 0.25, 0.02
F32 = np.float32


def constant_edge(textures, u, v, uv_max):
    """Where both axes are clamped to a constant edge whatever float32 does to uv: the mask and the texel indices (j, i).
    (An axis of one texel is not enough: between the clamps the two taps are the same texel, but (1-a) T + a T rounds.)  A coordinate counts as clamped when its float64 texel coordinate lies outside [-1, W] by
    more than 2^-18 max(1, |uv|max) W texels — 64 times what float32 can move it by."""
    _, Ht, Wt = textures.shape[:3]
    U, V = R.unclamped_coordinates(textures, u, v)

    def axis(X, n):
        m = 2.0 ** -18 * max(1.0, uv_max) * n
        lo, hi = X <= -1 - m, X >= n + m
        return lo | hi, np.where(hi, n - 1, 0)

    cu, i = axis(U, Wt)
    cv, j = axis(V, Ht)
    return cu & cv, j, i


def check_radiance(got, scene, fh, uv_max, what):
    """`got` (h, w, 3) float32 sample radiance against the float64 reference: a miss sees the light, a hit is the texel
    within C 2^-24 L, and exactly the edge texel where uv clamps to one."""
    hit, keep = fh["hit"], fh["edge"] >= R.EDGE_MARGIN
    assert hit.mean() >= MIN_HIT, (what, hit.mean())
    assert (~keep).mean() < MAX_LEFT_OUT, (what, (~keep).mean())
    assert np.isfinite(got).all(), (what, "NaN or Inf radiance")
    assert (got[~hit & keep] == 1.0).all(), what
    k = hit & keep
    u, v, tex = fh["u"][k], fh["v"][k], fh["tex"][k]
    const, j, i = constant_edge(scene.textures, u, v, uv_max)
    edge = scene.textures[tex[const], j[const], i[const], :3]
    assert np.array_equal(got[k][const].view(np.uint32), edge.view(np.uint32)), (what, "not the edge texel")
    err = np.abs(got[k] - R.texel64(scene.textures, u, v, tex)).max(axis=1)
    tol = R.tolerance(scene.textures, uv_max, C)
    print("%s: hit %.3f, left out %.4f, constant edge %.3f, max err %.3g, bound %.3g" %
          (what, hit.mean(), (~keep).mean(), const.mean() if len(const) else 0, err.max(), tol))
    if uv_max < 1e20:
        assert err.max() <= tol, (what, err.max(), tol)
    else:
        # |uv| = 1e30: where uv cancels to (nearly) nothing float64 has no digits left either; everywhere else the texel
        # is an edge texel (checked above), and every colour stays inside the texture's range
        assert const.mean() > 0.9, what
        assert (got[k] >= scene.textures[..., :3].min()).all() and (got[k] <= scene.textures[..., :3].max()).all(), what


_BUILT = {}


def built_case(case):
    """(scene, camera, |uv|max, float64 first hits) of a case, made once and left unchanged."""
    if case not in _BUILT:
        s, cam, uv_max = TC.build(*case)
        _BUILT[case] = (s, cam, uv_max, R.first_hits(s, cam, TC.W, TC.H))
    return _BUILT[case]


def all_pixels(sample):
    ys, xs = np.mgrid[0:TC.H, 0:TC.W]
    return xs.ravel(), ys.ravel(), np.full(xs.size, sample, np.uint32)


@pytest.mark.parametrize("case", TC.CASES, ids=TC.case_id)
def test_oracle_radiance_is_the_float64_texel(case, oracle, table):
    s, cam, uv_max, fh = built_case(case)
    for sample in (0, 1):
        got, _ = oracle.samples(s, cam, table, TC.W, TC.H, *all_pixels(sample))
        check_radiance(got.reshape(TC.H, TC.W, 3), s, fh, uv_max, (TC.case_id(case), sample))


@pytest.mark.parametrize("case", TC.CASES, ids=TC.case_id)
def test_oracle_equals_the_compiled_reference(case, oracle, ref, table):  # noqa: F811
    s, cam, _, _ = built_case(case)
    b, _ = oracle.render(s, cam, table, TC.W, TC.H, 2, count=2, threads=2)
    _same_as_reference("texture/" + TC.case_id(case), b,
                       ref and (lambda: ref.progressive(s, cam, table, TC.W, TC.H, 2, threads=2)))


SPECIAL = np.array([0.0, 1.0, -0.0, -1e-30, -40.0, 40.0, -1e30, 1e30, -3e38, 3e38, -np.inf, np.inf, np.nan], F32)


@pytest.mark.parametrize("name", sorted(TC.TEXTURES))
def test_numpy_texel_is_the_float64_texel(name):
    """chain_ref.texel at float32 uv against the definition at the same uv: only the sampler's own rounding is left."""
    tex = TC.random_texture(name)
    layers, Ht, Wt = tex.shape[:3]

    class Scene:
        textures = tex

    rng = np.random.RandomState(5)
    n = 4000
    u, v = (rng.random_sample(n) * 5 - 2).astype(F32), (rng.random_sample(n) * 5 - 2).astype(F32)
    # texel centres, texel borders and the two ends of the clamp, exactly
    gu = np.concatenate([(np.arange(-3, 2 * Wt + 4) / (2.0 * Wt)), [-0.5 / Wt, (Wt + 0.5) / Wt]]).astype(F32)
    gv = np.concatenate([(np.arange(-3, 2 * Ht + 4) / (2.0 * Ht)), [-0.5 / Ht, (Ht + 0.5) / Ht]]).astype(F32)
    u, v = np.concatenate([u, np.repeat(gu, len(gv))]), np.concatenate([v, np.tile(gv, len(gu))])
    layer = (np.arange(len(u)) % (layers + 1)).astype(np.uint32)      # (one id past the last layer: layer 0)
    got = chain_ref.texel(Scene, u, v, layer)
    exp = R.texel64(tex, u.astype(np.float64), v.astype(np.float64), layer)
    scale = np.maximum(1.0, np.maximum(np.abs(u), np.abs(v)).astype(np.float64))
    tol = C * 2.0 ** -24 * (R.contrast_slope(tex) * scale + 4.0)
    err = np.abs(got - exp).max(axis=1)
    assert (err <= tol).all(), (name, float((err / tol).max()))
    # every pair of special coordinates clamps on both axes: exactly a corner texel, NaN counting as the low edge
    su, sv = np.repeat(SPECIAL, len(SPECIAL)), np.tile(SPECIAL, len(SPECIAL))
    both = ~(np.isin(su, [0.0, 1.0]) & (Wt > 1)) & ~(np.isin(sv, [0.0, 1.0]) & (Ht > 1))
    su, sv = su[both], sv[both]
    lay = (np.arange(len(su)) % layers).astype(np.uint32)
    got = chain_ref.texel(Scene, su, sv, lay)
    i = np.where(su > 0.5, Wt - 1, 0)
    j = np.where(sv > 0.5, Ht - 1, 0)
    assert np.array_equal(got.view(np.uint32), tex[lay, j, i, :3].view(np.uint32)), name
    exp = R.texel64(tex, su.astype(np.float64), sv.astype(np.float64), lay)
    assert np.array_equal(got.astype(np.float64), exp), name
