"""Shared by tests/test_inert_terminal.py (CPU) and tests/test_gpu_inert_terminal.py: the scene whose terminal vertices land on every kind of surface the "inert when terminal"
predicate tells apart (rtxpt_amd/csrc/pt_scene.h inert_bits_of / inert_when_terminal), and the predicate restated in numpy from the scene description alone.

The scene is a Cornell room (rtxpt_amd.scenes helpers) under a sky, seen from outside its open front, with four analytic sphere lights (tests/pin_scenes.with_sphere_lights):
  instance 0  the room: white / red / green walls (opaque, cannot emit) and the emissive quad below the ceiling
  instance 1  a glass box: not thin, nested priority 2 — HandleNestedDielectrics may reject a hit on it when nestedDielectricsQuality > 0
  instance 2  a metal box flagged as the stand-in of analytic light 0 (tests/pin_scenes.with_light_proxy: EnableAsAnalyticLightProxy + the instance's link)
  instance 3  a thin alpha-tested card (checkerboard opacity)
  instance 4  a panel whose EmissiveColor is 1e-9 in one component: zero after rounding to binary16, > 0 as the material holds it — "can emit"
"""
import numpy as np

from rtxpt_amd import scenes

MF_PROXY, MF_THIN = 0x800, 0x200      # PTMaterialFlags_EnableAsAnalyticLightProxy, PTMaterialFlags_ThinSurface (MaterialPT.h:24-42)
INERT_NO_LIGHT, INERT_THIN = 1, 2
TINY = 1e-9
assert np.float32(TINY) > 0 and np.float32(TINY).astype(np.float16) == 0


def _room():
    b = scenes.SceneBuilder()
    mm = scenes.make_material
    white = b.add_material(mm(base=(0.725, 0.71, 0.68), roughness=0.6))
    red = b.add_material(mm(base=(0.63, 0.065, 0.05)))
    green = b.add_material(mm(base=(0.14, 0.45, 0.091)))
    light = b.add_material(mm(base=(0.78, 0.78, 0.78), emissive=(17.0, 12.0, 4.0)))
    glass = b.add_material(mm(base=(0.95, 0.95, 0.95), roughness=0.0, ior=1.5, transmission=1.0, thin=False, nested_priority=2, att_color=(0.8, 0.95, 0.85), att_dist=0.25))
    metal = b.add_material(mm(base=(0.95, 0.75, 0.35), roughness=0.3, metalness=1.0))
    a = np.zeros((64, 64, 4), np.uint8); a[..., :3] = (200, 180, 90)
    yy, xx = np.mgrid[0:64, 0:64]; a[..., 3] = np.where(((xx // 8) + (yy // 8)) % 2 == 0, 255, 0)
    card = b.add_material(mm(base=(1, 1, 1), base_tex=b.add_texture(a, scenes.TEX_RGBA8_UNORM), alpha_cutoff=0.5))
    tiny = b.add_material(mm(base=(0.5, 0.5, 0.6), emissive=(0.0, TINY, 0.0)))
    X, Y, Z = 0.5528, 0.5488, 0.5592
    b.begin_mesh()
    for pts, mat in ((((0, 0, 0), (0, 0, Z), (X, 0, Z), (X, 0, 0)), white), (((0, Y, 0), (X, Y, 0), (X, Y, Z), (0, Y, Z)), white), (((0, 0, Z), (0, Y, Z), (X, Y, Z), (X, 0, Z)), white),
                     (((0, 0, 0), (0, Y, 0), (0, Y, Z), (0, 0, Z)), green), (((X, 0, 0), (X, 0, Z), (X, Y, Z), (X, Y, 0)), red)):
        p, i, uv, n, t = scenes.quad(*pts); b.add_geometry(p, i, mat, uv=uv, normal=n, tangent=t)
    ly = Y - 0.0002
    p, i, uv, n, t = scenes.quad((0.213, ly, 0.227), (0.343, ly, 0.227), (0.343, ly, 0.332), (0.213, ly, 0.332)); b.add_geometry(p, i, light, uv=uv, normal=n, tangent=t)
    b.add_instance(b.end_mesh())
    cp, ci, cuv, cn, ct = scenes.unit_cube()
    for mat, xf in ((glass, scenes.trs((0.185, 0.0825 + 1e-4, 0.169), rot_y=-0.29, scale=(0.165, 0.165, 0.165))), (metal, scenes.trs((0.368, 0.165 + 1e-4, 0.351), rot_y=0.30, scale=(0.165, 0.33, 0.165)))):
        b.begin_mesh(); b.add_geometry(cp, ci, mat, uv=cuv, normal=cn, tangent=ct); b.add_instance(b.end_mesh(), xf)
    # the card stands in front of the red wall, facing the camera; the panel lies on the floor in front of the boxes
    p, i, uv, n, t = scenes.quad((0.38, 0.02, 0.12), (0.38, 0.30, 0.12), (0.52, 0.30, 0.12), (0.52, 0.02, 0.12))
    b.begin_mesh(); b.add_geometry(p, i, card, uv=uv, normal=n, tangent=t, geom_flags=scenes.GEOMF_ALPHA_TESTED); b.add_instance(b.end_mesh())
    p, i, uv, n, t = scenes.quad((0.05, 0.001, 0.02), (0.05, 0.001, 0.10), (0.30, 0.001, 0.10), (0.30, 0.001, 0.02))
    b.begin_mesh(); b.add_geometry(p, i, tiny, uv=uv, normal=n, tangent=t); b.add_instance(b.end_mesh())
    b.set_environment(scenes.sky_equirect(256, 128), color_multiplier=(1, 1, 1))
    cam = dict(pos=(0.278, 0.273, -0.8), direction=(0, 0, 1), up=(0, 1, 0), fov_y=0.6859, near_z=0.01, far_z=100.0, focal_distance=1.0)
    return b.finish(), cam


def zoo(proxy_link=True):
    """(scene, camera). proxy_link False: the metal box's material carries the proxy flag, its instance names no light yet (the link a later light bake adds)."""
    import pin_scenes
    sc, cam = pin_scenes.with_light_proxy(pin_scenes.with_sphere_lights(_room), instance=2, light=0, radius=0.06)()
    if not proxy_link:
        sc = dict(sc); inst = sc["instances"].copy(); inst["analyticProxyLight"][2] = 0; sc["instances"] = inst
    return sc, cam


def all_emissive(sc):
    """the scene with every material able to emit: nothing may be dropped"""
    sc = dict(sc); m = sc["materials"].copy()
    dark = ~(m["EmissiveColor"] != 0).any(-1)
    e = m["EmissiveColor"].copy(); e[dark, 2] = np.float32(TINY); m["EmissiveColor"] = e
    sc["materials"] = m
    return sc


def prim_materials(sc):
    """material index of every global primitive, in the order pt_api.hip finalize_geometry numbers them: instance by instance, geometry by geometry of its mesh"""
    out = []
    for inst in sc["instances"]:
        m = sc["meshes"][int(inst["meshIndex"])]
        for g in sc["geometries"][int(m["firstGeometry"]): int(m["firstGeometry"]) + int(m["numGeometries"])]:
            out.append(np.full(int(g["numIndices"]) // 3, int(g["materialIndex"]), np.uint32))
    return np.concatenate(out) if out else np.zeros(0, np.uint32)


def material_bits(materials):
    """inert_bits_of, restated: bit 0 = EmissiveColor exactly zero in all three components (as stored, before any rounding) and no proxy flag; bit 1 = thin surface"""
    e = np.asarray(materials["EmissiveColor"], np.float32); f = np.asarray(materials["Flags"], np.uint32)
    no_light = (e == 0).all(-1) & ((f & MF_PROXY) == 0)
    return (no_light.astype(np.uint32) * INERT_NO_LIGHT) | (((f & MF_THIN) != 0).astype(np.uint32) * INERT_THIN)


def prim_bits(sc): return material_bits(sc["materials"])[prim_materials(sc)]


def inert(bits, quality):
    """inert_when_terminal, restated"""
    bits = np.asarray(bits)
    return ((bits & INERT_NO_LIGHT) != 0) & ((quality == 0) | ((bits & INERT_THIN) != 0))
