"""The denoiser passes of a realtime stable-plane frame on the CPU: the numpy restatement of PostProcess.hlsl (tests/denoiser_inputs_ref.py) on hand-built plane buffers with answers
worked out by hand, over the committed reference-text plane outputs (tests/golden/denoiser_inputs_golden.npz), its camera rays against the oracle's, and the public interface
(include/mi355pt.h declares the entry points, libmi355pt.so exports them). The device runs the same cases in tests/test_gpu_zzz_denoiser_inputs.py."""
import os, re, sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoiser_inputs_ref as ref
from rtxpt_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "denoiser_inputs_golden.npz")
ENTRY_POINTS = ("pt_denoiser_default_params", "pt_denoiser_prepare_dlss_rr", "pt_denoiser_prepare_nrd", "pt_denoiser_merge_nrd", "pt_get_denoiser_inputs", "pt_denoiser_device_buffers")
f32 = np.float32
W, H = 11, 9                  # no multiple of the 8 x 8 addressing tiles


def _params(active=3, suppress=0.6, K=4096.0, w=W, h=H):
    sp = scenes.stable_planes_params(w, h, np.eye(4, dtype=f32), active_planes=active)
    dn = np.zeros((), [("matWorldToView", "<f4", 16), ("preExposedGrayLuminance", "<f4"), ("denoiserRadianceClampK", "<f4"), ("DLSSRRBrightnessClampK", "<f4"),
                       ("stablePlanesSuppressPrimaryIndirectSpecularK", "<f4")])
    dn["matWorldToView"] = np.eye(4, dtype=f32).reshape(16); dn["preExposedGrayLuminance"] = 1.0; dn["denoiserRadianceClampK"] = 8.0
    dn["DLSSRRBrightnessClampK"] = K; dn["stablePlanesSuppressPrimaryIndirectSpecularK"] = suppress
    return sp, dn


def hand_frame(W=W, H=H):
    """plane 0 everywhere (a surface at distance 2 straight ahead) except a sky column at x = 10; plane 1 (vertex 2) at (0, 0) alone and at (3..5, 4); plane 2 (vertex 3) at (4, 4);
    dominant plane 2 at (4, 4); stable radiance 0.25 at (7, 2); specular hit distance 3 at (3, 4) and (10, 0)"""
    fr = ref.make_frame(W, H)
    for y in range(H):
        for x in range(W):
            ref.put(fr, x, y, 0, 1, ref.make_record(scene_length=np.inf if x == 10 else 2.0), W, H)
    ref.put(fr, 0, 0, 1, 0b100, ref.make_record(thp=(0.5, 0.5, 0.5), vertex=2), W, H)
    for x in (3, 4, 5): ref.put(fr, x, 4, 1, 0b100, ref.make_record(thp=(0.1, 0.1, 0.1), vertex=2), W, H)
    ref.put(fr, 4, 4, 2, 0b11001, ref.make_record(thp=(0.5, 0.5, 0.5), vertex=3, noisy=(1.0, 1.0, 1.0, 0.5)), W, H)
    ref.set_dominant(fr, 4, 4, 2)
    fr["stable_radiance"][2, 7] = ref.f32_to_half(np.array([0.25, 0.25, 0.25, 0], f32))
    fr["spec_hit_t"][4, 3] = 3.0; fr["spec_hit_t"][0, 10] = 3.0
    return fr


def hand_cases():
    """the hand-built frames both suites run: (name, frame, params); three-plane, two-plane, one-plane, suppression off, K = 0, and the same frame at 13 x 7 (wider than high,
    neither size a multiple of the 8 x 8 addressing tiles)"""
    fr = hand_frame(); out = []
    for name, kw in (("three_planes", {}), ("two_planes", dict(active=2)), ("one_plane", dict(active=1)), ("suppression_off", dict(suppress=0.0)), ("brightness_clamp_0", dict(K=0.0))):
        sp, dn = _params(**kw); out.append(dict(name=name, frame=fr, sp=sp, dn=dn, w=W, h=H))
    sp, dn = _params(w=13, h=7); out.append(dict(name="frame_13x7", frame=hand_frame(13, 7), sp=sp, dn=dn, w=13, h=7))
    return out


def _rays():
    o = np.zeros((H, W, 3), f32); d = np.zeros((H, W, 3), f32); d[..., 2] = -1
    return o, d


def test_dlss_rr_worked_by_hand():
    sp, dn = _params()
    r = ref.dlss_rr(hand_frame(), sp, dn, W, H)
    # one live plane, nothing stable: weight 1 on plane 0; colour = its noisy radiance; albedos = its BSDF estimates (0.5 / 0.25 -> R11G11B10F words)
    assert np.array_equal(r["output_color"][1, 1], f32([0.5, 0.5, 0.5, 1]))
    assert r["rr_diffuse_albedo"][1, 1] == 0x701C0380 and r["rr_specular_albedo"][1, 1] == 0x681A0340
    assert ref.half_to_f32(r["rr_normal_roughness"][1, 1])[3] == f32(0.5)
    assert np.allclose(ref.half_to_f32(r["rr_normal_roughness"][1, 1])[:3], [0, 0, 1], atol=1e-4)
    # three live planes at (4, 4), dominant 2: thp weights (saturate(0.9 - 0.5), 0.1, 0.5) x 0.2 + 0.01, + 0.05 on plane 2 -> (0.09, 0.03, 0.16) / 0.28
    # `x >= max(y, y)` as written picks layer 0 although z > x (max(y, z) would pick 2)
    assert r["primary_layer"][4, 4] == 0
    w = np.array([0.09, 0.03, 0.16]) / 0.28
    assert abs(float(ref.half_to_f32(r["rr_normal_roughness"][4, 4])[3]) - 0.5) < 1e-3          # every plane has roughness 0.5 and the weights sum to 1
    assert np.array_equal(r["output_color"][4, 4], f32([2.0, 2.0, 2.0, 1]))                      # 0.5 + 0.5 + 1.0
    diff = 0.5 * w.sum()
    assert abs(float(ref.half_to_f32(np.uint16((r["rr_diffuse_albedo"][4, 4] & 0x7FF) << 4))) - diff) < 2e-3
    # a sky pixel (plane 0 with SceneLength = inf): no surface, no weight -> colour = stable radiance (0), albedo floor 0.05, normal (0, 0, 1), roughness 0
    assert np.array_equal(r["output_color"][3, 10], f32([0, 0, 0, 1]))
    assert np.array_equal(ref.half_to_f32(r["rr_normal_roughness"][3, 10]), f32([0, 0, 1, 0]))
    assert r["rr_diffuse_albedo"][3, 10] == ref.pack_r11g11b10(np.array([0.05, 0.05, 0.05], f32))
    # the specular-MV block reads plane 0 anyway: with a hit distance there, the reflection of an infinite hit point is not finite
    assert not np.all(np.isfinite(ref.half_to_f32(r["rr_specular_motion_vectors"][0, 10])))
    # a plane-0 pixel with a hit distance and mixed roughness 0.5 >= 0.25 keeps the frame's motion vectors (0)
    assert np.array_equal(r["rr_specular_motion_vectors"][4, 3], [0, 0])


def test_dlss_rr_brightness_clamp_zero_blacks_out():
    sp, dn = _params(K=0.0)
    r = ref.dlss_rr(hand_frame(), sp, dn, W, H)
    assert np.all(r["output_color"][..., :3] == 0) and np.all(r["output_color"][..., 3] == 1)
    sp, dn = _params(K=0.4)
    r = ref.dlss_rr(hand_frame(), sp, dn, W, H)
    assert np.array_equal(r["output_color"][1, 1], f32([0.4, 0.4, 0.4, 1])) and np.allclose(r["output_color"][2, 7], [0.4, 0.4, 0.4, 1], rtol=1e-6)


def test_nrd_prepare_worked_by_hand():
    sp, dn = _params()
    fr = hand_frame(); o, d = _rays()
    st = ref.nrd_prepare(ref.empty_state(W, H), fr, sp, dn, W, H, 0, True, o, d)
    # init: the output colour is the stable radiance
    assert np.array_equal(st["output_color"][2, 7], f32([0.25, 0.25, 0.25, 1]))
    # a plane-0 surface at distance 2 along -z, identity view: viewZ = -2; radiance split half / half by specAvg 0.25 of 0.5, demodulated by 0.5 and 0.25
    assert st["nrd_view_z"][1, 1] == f32(-2)
    assert np.array_equal(st["nrd_diff_radiance_hit_dist"][1, 1], f32([0.5, 0.5, 0.5, 0])) and np.array_equal(st["nrd_spec_radiance_hit_dist"][1, 1], f32([1, 1, 1, 0]))
    assert st["nrd_normal_roughness"][1, 1, 3] == f32(0.5) and st["nrd_roughness"][1, 1] == f32(0.5)
    assert st["nrd_disocclusion_threshold_mix"][1, 1] == 0                                         # vertex 1: no relaxation
    # sky: the marker, nothing else written
    assert st["nrd_view_z"][0, 10] == ref.FLT_MAX and np.all(st["nrd_spec_radiance_hit_dist"][0, 10] == 0)
    # suppression: plane 0 at (4, 4) has planes 1 and 2 live -> specular x saturate(1 - 0.6); at (3, 4) plane 2 is missing -> none
    assert np.array_equal(st["nrd_spec_radiance_hit_dist"][4, 4, :3], f32([1, 1, 1]) * (f32(1) - f32(0.6)))
    assert np.array_equal(st["nrd_spec_radiance_hit_dist"][4, 3, :3], f32([1, 1, 1]))
    sp0, dn0 = _params(suppress=0.0)
    assert np.array_equal(ref.nrd_prepare(ref.empty_state(W, H), fr, sp0, dn0, W, H, 0, True, o, d)["nrd_spec_radiance_hit_dist"][4, 4, :3], f32([1, 1, 1]))
    # the dominant plane's hit distance: plane 2 at (4, 4) is dominant -> plane 0 carries 0 there, plane 2 the value
    st2 = ref.nrd_prepare(ref.empty_state(W, H), fr, sp, dn, W, H, 2, True, o, d)
    assert st2["nrd_spec_radiance_hit_dist"][4, 4, 3] == fr["spec_hit_t"][4, 4]
    assert st["nrd_spec_radiance_hit_dist"][4, 3, 3] == f32(3)                                     # dominant 0 at (3, 4)


def test_nrd_disocclusion_at_the_frame_edge_and_the_history_clamp():
    sp, dn = _params()
    fr = hand_frame(); o, d = _rays()
    st = ref.nrd_prepare(ref.empty_state(W, H), fr, sp, dn, W, H, 1, True, o, d)
    # plane 1 at the corner (0, 0): left / up clamp to the pixel itself (1 - n.n ~ 0), right / down have no plane 1 (kEdge 0.02 each): (0.04 - 0.00002) x 25 -> 0.9995
    assert st["nrd_disocclusion_threshold_mix"][0, 0] == 255
    assert abs(float(st["nrd_normal_roughness"][0, 0, 3]) - 1.0) < 1e-6                           # saturate(0.5 + 0.9995)
    # (4, 4) has plane-1 neighbours left and right, none up / down: 0.04 as well; thp 0.1 -> history 0.9995 x 0.1
    assert st["nrd_disocclusion_threshold_mix"][4, 4] == 255 and st["nrd_combined_history_clamp_relax"][4, 4] == 25
    # the next plane adds to the stored (quantised) value; an init call clears it first
    st = ref.nrd_prepare(st, fr, sp, dn, W, H, 2, False, o, d)
    assert st["nrd_combined_history_clamp_relax"][4, 4] == 152      # plane 2 alone: 0.08 -> saturate 1, x 0.5, + 25/255 -> x 255 = 152.5: ties to even
    st = ref.nrd_prepare(st, fr, sp, dn, W, H, 0, True, o, d)
    assert st["nrd_combined_history_clamp_relax"][4, 4] == 0


def test_nrd_merge_adds_remodulated_radiance_where_there_is_a_surface():
    sp, dn = _params()
    fr = hand_frame(); o, d = _rays()
    st, _ = ref.nrd_sequence(fr, sp, dn, W, H, {p: (o, d) for p in range(3)})
    # identity denoiser on plane 0 at (1, 1): 0.5 x 0.5 + 1 x 0.25 = 0.5 on top of the stable radiance 0
    assert np.array_equal(st["output_color"][1, 1], f32([0.5, 0.5, 0.5, 1]))
    assert np.array_equal(st["output_color"][2, 10], f32([0, 0, 0, 1]))                           # sky: nothing added
    neg = ref.nrd_merge(st, fr, W, H, 0, -np.ones((H, W, 4), f32), np.zeros((H, W, 4), f32))
    assert np.array_equal(neg[1, 1], st["output_color"][1, 1])                                      # max(0, diff + spec)


def test_camera_rays_equal_the_oracle():
    from oracle import ptref
    sc, cam = scenes.stable_planes_zoo(); w, h = 13, 7
    camd = scenes.bridge_camera(w, h, **cam); S = scenes.config_settings("C2")
    o = ptref.Oracle(); o.set_scene(sc); o.set_camera(camd); o.set_settings(S); o.resize(w, h)
    for s in (0, 5, 6):
        ro, rd = ref.camera_rays(camd, S, w, h, s)
        for y in range(h):
            for x in range(w):
                want = o.camera_ray(x, y, s)
                assert np.array_equal(np.concatenate([ro[y, x], rd[y, x]]).view(np.uint32), want.view(np.uint32)), (x, y, s)


def test_restatement_equals_the_committed_fixture():
    """The fixture is made by the compiled reference text (tests/golden/make_denoiser_inputs_golden.py, which needs the reference checkout). This test needs only the oracle: it
    rebuilds every fixture case's inputs and holds the restatement to every array of the fixture the restatement covers: the DLSS-RR buffers, the state after each plane's
    prepare, the colour after each merge. The thin-lens case runs with the oracle's camera rays (the restatement's own stop at the pinhole camera)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_dn_golden", os.path.join(ROOT, "tests", "golden", "make_denoiser_inputs_golden.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    g = np.load(GOLDEN); seen = set()
    def same(key, want):
        assert want.dtype == g[key].dtype and want.shape == g[key].shape, key
        assert np.array_equal(ref.canonical(want), ref.canonical(g[key])), key
        seen.add(key)
    for case, frame_keys in m.fixture_cases():
        name, fr, sp, dn, w, h = case["name"], case["frame"], case["sp"], case["dn"], case["w"], case["h"]
        for k in frame_keys: same(("frame_" if name == "zoo_fp32" else name + "_frame_") + k, np.asarray(fr[k]))
        rr = ref.dlss_rr(fr, sp, dn, w, h); pre = "" if name == "zoo_fp32" else name + "_"
        for k in m.RR: same(pre + k, rr[k])
        same(pre + "rr_output_color", rr["output_color"])
        rays = case["rays"] if case["rays"] is not None else {p: ref.camera_rays(case["cam"], case["S"], w, h, case["base"] + p) for p in range(3)}
        st, per = ref.nrd_sequence(fr, sp, dn, w, h, rays)
        for p in per:
            for k in ref.NRD_KEYS + ("output_color",): same("%s_p%d_%s" % (name, p, k), per[p][k])
            same("%s_p%d_merged" % (name, p), ref.nrd_merge(per[p], fr, w, h, p, per[p]["nrd_diff_radiance_hit_dist"], per[p]["nrd_spec_radiance_hit_dist"]))
        if name == "zoo_fp32":
            for k in ref.NRD_KEYS: same(k, st[k])
            same("nrd_output_color", st["output_color"])
        assert g[name + "_dims"].tolist() == [w, h, case["base"]]; seen.update(name + "_" + k for k in ("sp", "dn", "cam", "dims"))
    assert seen == set(g.keys()), sorted(set(g.keys()) ^ seen)[:8]


def test_header_declares_and_library_exports_the_entry_points():
    import rtxpt_amd as pt
    text = open(os.path.join(ROOT, "include", "mi355pt.h")).read()
    for n in ENTRY_POINTS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % n, text), n
        assert n in pt.EXPORTS, n
    for t in ("PtDenoiserParams", "PtDenoiserBuffers"): assert "} %s;" % t in text, t
    L = pt.load_library()
    for n in ENTRY_POINTS: assert hasattr(L, n), n
    d = pt.denoiser_default_params()
    assert d["denoiserRadianceClampK"] == 8 and d["DLSSRRBrightnessClampK"] == 4096 and d["stablePlanesSuppressPrimaryIndirectSpecularK"] == f32(0.6)
