"""Skins and morph targets posed on the device (pt_set_skinning / pt_animate_skinned; rtxpt_amd/csrc/pt_skin.h is the one text of the per-vertex pose, k_skin in pt_skin.hip runs
it): held to the host pose (pt_gltf_animation_positions / _normals -> pt_animate_ranges + pt_animate_normals), which is unchanged code. Both sides are built without
contraction and fast math and binary64 + - * / sqrt are correctly rounded on both, so every comparison is np.array_equal — streams bit for bit, frames byte for byte.
Frames are 64 x 48, 1 sample, 2 bounces; the cases are tests/skin_cases.py's."""
import os, sys
import numpy as np
import pytest

import rtxpt_amd as pt
from rtxpt_amd import scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skin_cases

pytestmark = pytest.mark.gpu
W, H = 64, 48
POSES = (0.35, 1.0, 1.6)      # between the keys, on a key (case D: the joint whose scale is 0 on one axis there), between the keys


def tracer(case):
    g = pt.PathTracer(); g.load_scene_gltf(str(case["path"]))
    b, e = pt.convert_light("point", case["light"], (1.0, 0.9, 0.8), 60.0, 0.05, (0.0, 0.0, -1.0), 180.0, 180.0)
    g._chk(g.L.pt_set_lights(g.h, pt._p(b), pt._p(e), 1), "pt_set_lights")
    g.set_settings(scenes.default_settings(bounceCount=2, diffuseBounceCount=2)); g.resize(W, H); g.set_camera(scenes.bridge_camera(W, H, **case["camera"]))
    return g


def ranges_of(desc): return [(int(r["firstVertex"]), int(r["numVertices"])) for r in desc.ranges]


def host_pose(h, anim, desc, t, rebuild=False):
    """the frame the way it was before the device pose: pt_gltf_animation_positions / _normals, pt_animate_ranges, pt_animate_normals"""
    h.animate(anim.instances(t), anim.positions(t), rebuild=rebuild, vertex_ranges=ranges_of(desc)); h.animate_normals(*anim.normals(t))


def frame(g):
    st = g.render(0, 1)
    return g.radiance().view(np.uint32), {k: v for k, v in st.items() if k.endswith("Rays") and np.isscalar(v)}


@pytest.mark.parametrize("name", skin_cases.CASES)
def test_streams_equal_the_hosts_bit_for_bit(name, tmp_path):
    case = skin_cases.make(name, tmp_path); a = pt.GltfAnimation(case["path"]); g = tracer(case)
    bindP, bindN, bindT = skin_cases.bind_streams(case["path"]); s = case["sentinels"]
    p, n, t = g.vertex_streams(); assert np.array_equal(p, bindP) and np.array_equal(n, bindN) and np.array_equal(t, bindT)      # what pt_set_geometry received
    g.set_skinning(a.skinning())
    for time in POSES:
        g.animate_gltf(a, time)
        p, n, t = g.vertex_streams(); wantN, wantT = a.normals(time)
        assert np.array_equal(p.view(np.uint32), a.positions(time).view(np.uint32)), (name, time)
        assert np.array_equal(n, wantN) and np.array_equal(t, wantT), (name, time)
        assert np.array_equal(p[s].view(np.uint32), bindP[s].view(np.uint32)) and np.array_equal(n[s], bindN[s]) and np.array_equal(t[s], bindT[s]), (name, time)
        assert not np.array_equal(p, bindP)
    if name == "E": assert s[0] and s[-1] and s.sum() == 18      # sentinels before the first range, between the two and after the last
    g.close(); a.close()


def test_a_palette_of_300_joints(tmp_path):
    """a palette larger than a byte indexes (JOINTS_0 as unsigned shorts, 37.5 KB of matrices read from global memory), on case C's shape at 331 vertices (a prime)"""
    case = skin_cases.case_c(tmp_path, n=331, joints=300, seed=6); a = pt.GltfAnimation(case["path"]); g = tracer(case); d = a.skinning()
    assert d.num_matrices == 300 and d.joints.max() > 255
    g.set_skinning(d)
    for time in POSES:
        g.animate_gltf(a, time)
        p, n, t = g.vertex_streams(); wantN, wantT = a.normals(time)
        assert np.array_equal(p.view(np.uint32), a.positions(time).view(np.uint32)) and np.array_equal(n, wantN) and np.array_equal(t, wantT), time
    g.close(); a.close()


@pytest.mark.parametrize("rebuild", (False, True))
@pytest.mark.parametrize("name", skin_cases.CASES)
def test_frames_equal_the_host_paths(name, rebuild, tmp_path):
    case = skin_cases.make(name, tmp_path); a = pt.GltfAnimation(case["path"]); d = a.skinning()
    g, h = tracer(case), tracer(case); g.set_skinning(d); seen = []
    for time in POSES:
        g.animate_gltf(a, time, rebuild=rebuild); host_pose(h, a, d, time, rebuild)
        fg, sg = frame(g); fh, sh = frame(h)
        assert np.array_equal(fg, fh), (name, time); assert sg == sh and sum(sg.values()) > 0, (name, time, sg, sh)
        assert fg.view(np.float32)[..., :3].max() > 0; seen.append(fg)
    assert not np.array_equal(seen[0], seen[1])      # (the poses are visible in the frame)
    g.close(); h.close(); a.close()


@pytest.mark.parametrize("name", skin_cases.CASES)
def test_motion_history_keeps_the_previous_pose(name, tmp_path):
    case = skin_cases.make(name, tmp_path); a = pt.GltfAnimation(case["path"]); d = a.skinning()
    g = tracer(case); g.set_skinning(d); g.set_motion_history(True)
    g.animate_gltf(a, POSES[0]); g.animate_gltf(a, POSES[1])
    p, n, t, q = g.vertex_streams(previous=True)
    assert np.array_equal(q.view(np.uint32), a.positions(POSES[0]).view(np.uint32)) and np.array_equal(p.view(np.uint32), a.positions(POSES[1]).view(np.uint32))
    if name == "A":      # the build pass's motion vectors and depth: a context that was handed the same two poses
        h = tracer(case); host_pose(h, a, d, POSES[1]); h.set_previous_pose(a.instances(POSES[0]), a.positions(POSES[0]))
        prm = scenes.stable_planes_params(W, H, scenes.view_projection(W, H, **case["camera"]))
        fg, fh = g.build_stable_planes(0, prm), h.build_stable_planes(0, prm)
        assert np.array_equal(fg["motion_vectors"], fh["motion_vectors"]) and np.array_equal(fg["depth"].view(np.uint32), fh["depth"].view(np.uint32))
        assert fg["motion_vectors"][..., :2].any()      # (something moved on screen)
        h.close()
    g.close(); a.close()


def test_previous_positions_need_the_motion_history(tmp_path):
    case = skin_cases.make("A", tmp_path); g = tracer(case)
    with pytest.raises(pt.PtError) as e: g.vertex_streams(previous=True)
    assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT
    g.close()


def test_a_rejected_call_changes_nothing(tmp_path):
    case = skin_cases.make("B", tmp_path); a = pt.GltfAnimation(case["path"]); d = a.skinning(); m, w = a.palette(POSES[1]); inst = a.instances(POSES[1])
    g = tracer(case); g.set_motion_history(True)
    def rejected(*args):
        with pytest.raises(pt.PtError) as e: g.animate_skinned(*args)
        assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT
    rejected(inst, m, w)                                     # before pt_set_skinning
    g.set_skinning(d); g.animate_gltf(a, POSES[0]); g.animate_gltf(a, POSES[2])
    before = g.vertex_streams(previous=True); fb, sb = frame(g)
    rejected(inst, m[:-1], w)                                # a wrong matrix count
    rejected(inst, m, w[:-1])                                # a wrong weight count
    rejected(inst, np.concatenate([m, m]), w); rejected(inst, m, None)
    after = g.vertex_streams(previous=True)
    for x, y in zip(before, after): assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    fa, sa = frame(g); assert np.array_equal(fa, fb) and sa == sb
    g.close(); a.close()


def test_host_mirrors_follow_a_device_pose(tmp_path):
    """After a device pose the host copies of the streams lag the device. Re-setting the scene's own instances marks the geometry dirty without changing it (the loader's
    materials are not readable back, so this setter stands in for re-setting the same materials): the next frame re-uploads the host copies and rebuilds the BVH from them."""
    case = skin_cases.make("E", tmp_path); a = pt.GltfAnimation(case["path"]); d = a.skinning()
    g = tracer(case); g.set_skinning(d); t = POSES[1]
    g.animate_gltf(a, t); f0, s0 = frame(g)
    inst = a.instances(t); g._chk(g.L.pt_set_instances(g.h, pt._p(inst), len(inst)), "pt_set_instances")
    f1, s1 = frame(g); assert np.array_equal(f0, f1) and s0 == s1
    p, n, tg = g.vertex_streams(); wantN, wantT = a.normals(t)
    assert np.array_equal(p.view(np.uint32), a.positions(t).view(np.uint32)) and np.array_equal(n, wantN) and np.array_equal(tg, wantT)
    g.animate_normals(wantN, wantT); f2, s2 = frame(g); assert np.array_equal(f0, f2) and s0 == s2
    # the skinning description survived the re-upload (only pt_set_geometry invalidates it), and the range path of pt_animate_ranges reads mirrors that are current
    g.animate_gltf(a, POSES[2]); g.animate(None, a.positions(POSES[2]), vertex_ranges=ranges_of(d)[:1]); g._chk(g.L.pt_set_instances(g.h, pt._p(inst), len(inst)), "pt_set_instances")
    p, n, tg = g.vertex_streams(); assert np.array_equal(p.view(np.uint32), a.positions(POSES[2]).view(np.uint32)) and np.array_equal(n, a.normals(POSES[2])[0])
    g.close(); a.close()


def test_bad_descriptions_are_refused(tmp_path):
    case = skin_cases.make("E", tmp_path); a = pt.GltfAnimation(case["path"]); g = tracer(case); bindP = g.vertex_streams()[0]
    def refused(change):
        d = a.skinning(); change(d)
        with pytest.raises(pt.PtError) as e: g.set_skinning(d)
        assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT
    def overlap(d): d.ranges[1]["firstVertex"] = d.ranges[0]["firstVertex"] + d.ranges[0]["numVertices"] - 1
    def beyond(d): d.ranges[1]["numVertices"] = len(d.joints)
    def matrices(d): d.ranges[0]["firstMatrix"] = d.num_matrices - 1
    def weights(d): d.ranges[0]["numTargets"] = 1
    def vertices(d): d.joints = d.joints[:-1]; d.weights = d.weights[:-1]; d.normals = d.normals[:-1]; d.tangents = d.tangents[:-1]
    for change in (overlap, beyond, matrices, weights, vertices): refused(change)
    m, w = a.palette(POSES[0])
    with pytest.raises(pt.PtError): g.animate_skinned(None, m, w)      # nothing was set
    g.set_skinning(a.skinning()); g.animate_gltf(a, POSES[0]); assert not np.array_equal(g.vertex_streams()[0], bindP)
    g.set_skinning(None)
    with pytest.raises(pt.PtError): g.animate_skinned(None, m, w)      # NULL removed it
    g.close(); a.close()


def test_set_geometry_invalidates_the_description(tmp_path):
    case = skin_cases.make("A", tmp_path); a = pt.GltfAnimation(case["path"]); g = tracer(case); g.set_skinning(a.skinning()); g.animate_gltf(a, POSES[0])
    g.load_scene_gltf(str(case["path"]))      # pt_set_geometry
    b, e = pt.convert_light("point", case["light"], (1.0, 0.9, 0.8), 60.0, 0.05, (0.0, 0.0, -1.0), 180.0, 180.0); g._chk(g.L.pt_set_lights(g.h, pt._p(b), pt._p(e), 1), "pt_set_lights")
    m, w = a.palette(POSES[1])
    with pytest.raises(pt.PtError) as err: g.animate_skinned(None, m, w)
    assert err.value.code == pt.PT_ERROR_INVALID_ARGUMENT
    assert np.array_equal(g.vertex_streams()[0], skin_cases.bind_streams(case["path"])[0])      # the new scene's own vertices, not the old pose
    g.close(); a.close()
