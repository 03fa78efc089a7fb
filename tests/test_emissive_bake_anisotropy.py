"""The emissive-triangle bake samples the emissive texture at the triangle's centroid with SampleGrad through an anisotropic sampler (LightsBaker.hlsl:591-650,
m_AnisotropicWrapSampler). Restated (scene.h / pt_scene.h sample_grad_anisotropic; unpinned — what a texture unit does with two gradients is implementation defined) in the
formulation of EXT_texture_filter_anisotropic: Px, Py = the gradients' lengths in texels, N = min(ceil(Pmax / Pmin), 16) trilinear taps at LOD log2(Pmax / N), spaced evenly along the
longer gradient and averaged. A reference quirk shapes the result: the bake's two gradients are shortEdge * 2/3 and (longEdge1 + longEdge2) / 3 = -shortEdge / 3 (the UV edges sum to
zero), i.e. collinear with a 2 : 1 length ratio — so the sampler always takes TWO taps, a sixth of the short edge to either side of the centroid, one level finer than a single tap at
the longer gradient's LOD (rounds 1 and 2's restatement). On a stretched-UV emitter over a striped texture the two restatements differ by ~20 %; the light table follows the new one."""
import os, sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rtxpt_amd import scenes
from oracle import ptref
from texture_ref import numpy_anisotropic as _numpy_anisotropic      # the float64 N-tap filter (tests/texture_ref.py)


def _scene():
    b = scenes.SceneBuilder()
    x = np.arange(256, dtype=np.float64)
    tex = np.ones((256, 256, 4), np.float32)
    for c, (period, phase) in enumerate(((48.0, 0.3), (40.0, 1.1), (56.0, 2.0))): tex[:, :, c] = (0.5 + 0.45 * np.sin(2 * np.pi * x / period + phase)).astype(np.float32)[None, :]      # stripes along u
    word = b.add_texture(tex, scenes.TEX_RGBA32F)
    m = b.add_material(scenes.make_material(base=(0.5, 0.5, 0.5), emissive=(4.0, 4.0, 4.0), emissive_tex=word))
    floor = b.add_material(scenes.make_material(base=(0.6, 0.6, 0.6)))
    b.begin_mesh(); b.add_geometry([[0, 1, 0], [1, 1, 0], [0.5, 1, 0.02]], [0, 1, 2], m, uv=UVS); emitter = b.end_mesh()
    p, i, uv, n, t = scenes.quad([-1, 0, -1], [2, 0, -1], [2, 0, 2], [-1, 0, 2])
    b.begin_mesh(); b.add_geometry(p, i, floor, uv=uv, normal=n, tangent=t); ground = b.end_mesh()
    b.add_instance(emitter); b.add_instance(ground)
    return b.finish(), tex


UVS = [[0.1, 0.5], [0.9, 0.5], [0.5, 0.52]]                                  # a long thin triangle in texture space: 205 x 5 texels


def _unpack_radiance(rec):
    """UnpackLightColor (PolymorphicLight.hlsli): R8G8B8_UFLOAT colour x the 16-bit log radiance."""
    c = rec[3]; col = np.array([c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF], np.float64) / 255.0
    lr = int(rec[7]) & 0xFFFF
    return col * (0.0 if lr == 0 else 2.0 ** ((lr - 1) / 65534.0 * 48.0 - 8.0))


def _expected(tex):
    uvs = np.array(UVS, np.float64); e = [uvs[1] - uvs[0], uvs[2] - uvs[1], uvs[0] - uvs[2]]; L = [np.linalg.norm(x) for x in e]
    k = 0 if (L[0] < L[1] and L[0] < L[2]) else (1 if L[1] < L[2] else 2); short, l1, l2 = e[k], e[(k + 1) % 3], e[(k + 2) % 3]
    sg, lg = short * (2 / 3), (l1 + l2) / 3
    new, n, lod = _numpy_anisotropic(tex, uvs.mean(0), sg, lg)
    big = sg if np.hypot(sg[0] * 256, sg[1] * 256) >= np.hypot(lg[0] * 256, lg[1] * 256) else lg
    old, n1, lod1 = _numpy_anisotropic(tex, uvs.mean(0), big, big)                # one tap at the longer gradient's LOD: equal gradients give N = 1
    return new, n, lod, old, lod1


def _check(rec, tex):
    new, n, lod, old, lod1 = _expected(tex)
    assert n == 2 and n * 0 + abs((lod1 - lod) - 1.0) < 1e-9                    # the reference's collinear 2 : 1 gradients: two taps, one level finer
    got = _unpack_radiance(rec)
    assert np.allclose(got, 4.0 * new, rtol=1.5e-2), (got, 4.0 * new)            # (8-bit colour x 16-bit log radiance)
    assert np.abs(new - old).max() / old.max() > 0.05                            # ... and the single-tap restatement would have baked something else
    assert not np.allclose(got, 4.0 * old, rtol=3e-2)
    return got


def test_oracle_emissive_bake_keeps_the_footprint_anisotropic():
    sc, tex = _scene()
    o = ptref.Oracle(); o.set_scene(sc); o.set_settings(scenes.default_settings()); o.resize(8, 8)
    L = o.lights()
    tri = [r for r in L["lights"] if ((r[3] >> 24) & 0xF) == 1]              # PolymorphicLightType kTriangle: the emitter (the floor does not emit)
    assert len(tri) == 1
    _check(tri[0], tex)


@pytest.mark.gpu
def test_device_emissive_bake_equals_the_oracle_and_keeps_the_footprint_anisotropic():
    import rtxpt_amd as pt
    sc, tex = _scene()
    g = pt.PathTracer(); g.set_scene(sc); g.set_settings(scenes.default_settings()); g.set_camera(scenes.bridge_camera(8, 8, pos=(0.5, 2.0, 0.5), direction=(0, -1, 0.01), up=(0, 0, 1), fov_y=1.0)); g.resize(8, 8)
    o = ptref.Oracle(); o.set_scene(sc); o.set_settings(scenes.default_settings()); o.resize(8, 8)
    Lg, Lo = g.lights(), o.lights()
    assert np.array_equal(Lg["lights"], Lo["lights"]) and np.array_equal(Lg["proxyCounters"], Lo["proxyCounters"])
    tri = [r for r in Lg["lights"] if ((r[3] >> 24) & 0xF) == 1]
    _check(tri[0], tex)
