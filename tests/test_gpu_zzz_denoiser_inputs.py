"""The denoiser passes of a realtime stable-plane frame on the device (run with -m gpu): pt_denoiser_prepare_dlss_rr, pt_denoiser_prepare_nrd and pt_denoiser_merge_nrd against the
independent numpy restatement of PostProcess.hlsl (tests/denoiser_inputs_ref.py) over the device's own plane buffers, bit for bit, and against the committed fixture, which
the reference's own PostProcess.hlsl text made (compiled by the oracle/refpin recipe): every buffer after every call, a thin-lens camera and a fuzz frame included."""
import os, sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoiser_inputs_ref as ref
import stable_planes_cases as spc
import realtime_cases as rc
import denoiser_text_cases as dtc
from rtxpt_amd import scenes

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denoiser_inputs_golden.npz")
RR_KEYS = ("rr_diffuse_albedo", "rr_specular_albedo", "rr_normal_roughness", "rr_specular_motion_vectors")


def _eq(a, b): return np.array_equal(ref.canonical(np.asarray(a)).view(np.uint8), ref.canonical(np.asarray(b)).view(np.uint8))


def _diff(a, b):
    a, b = ref.canonical(np.asarray(a)), ref.canonical(np.asarray(b))
    return int((a.reshape(a.shape[0], -1) != b.reshape(b.shape[0], -1)).sum())


def _dn(camd, w, h, **kw):
    import rtxpt_amd as pt
    d = ref.case_params(camd, **kw); assert d.dtype == pt.DENOISER_PARAMS_DTYPE
    return d


def _tracer(sc, camd, S, w, h, **kw):
    import rtxpt_amd as pt
    t = pt.PathTracer(**kw); t.set_scene(sc); t.set_camera(camd); t.set_settings(S); t.resize(w, h); return t


def _check_rr(t, frame, prm, dn, w, h, tag):
    t.denoiser_prepare_dlss_rr(prm, dn)
    got = t.get_denoiser_inputs(RR_KEYS); got["output_color"] = t.radiance()
    want = ref.dlss_rr(frame, prm, dn, w, h)
    for k in RR_KEYS + ("output_color",): assert _eq(got[k], want[k]), "%s: %s differs in %d values" % (tag, k, _diff(got[k], want[k]))
    return want


def _upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda")


def _check_nrd(t, frame, prm, dn, camd, S, w, h, base, tag, state=None):
    """the NRD sequence of Sample::Denoise with the identity as the denoiser; returns the restatement's final state"""
    active = int(prm["activeStablePlaneCount"])
    st = ref.empty_state(w, h) if state is None else state
    for n, p in enumerate(range(active - 1, -1, -1)):
        t.denoiser_prepare_nrd(prm, dn, p, n == 0)
        st = ref.nrd_prepare(st, frame, prm, dn, w, h, p, n == 0, *ref.camera_rays(camd, S, w, h, base + p))
        got = t.get_denoiser_inputs(ref.NRD_KEYS)
        for k in ref.NRD_KEYS: assert _eq(got[k], st[k]), "%s plane %d: %s differs in %d values" % (tag, p, k, _diff(got[k], st[k]))
        dd, ss = _upload(got["nrd_diff_radiance_hit_dist"]), _upload(got["nrd_spec_radiance_hit_dist"])
        t.denoiser_merge_nrd(p, dd.data_ptr(), ss.data_ptr())
        st["output_color"] = ref.nrd_merge(st, frame, w, h, p, st["nrd_diff_radiance_hit_dist"], st["nrd_spec_radiance_hit_dist"])
        assert _eq(t.radiance(), st["output_color"]), "%s plane %d: merged colour differs in %d values" % (tag, p, _diff(t.radiance(), st["output_color"]))
    return st


def _zoo_frame(name, motion=False):
    sc, camd, S, prm, lp16 = spc.setup(name)
    t = _tracer(sc, camd, S, spc.W, spc.H)
    if motion:
        t.set_previous_pose(*scenes.previous_pose(sc))
    t.build_stable_planes(spc.SAMPLE, prm); t.fill_stable_planes(spc.SAMPLE, prm, sub_samples=spc.SUBSAMPLES); t.denoise_spec_hit_t()
    return t, t.get_stable_planes(), camd, S, prm


@pytest.mark.parametrize("name", ["zoo_fp32", "zoo_lp16", "zoo_two_planes_no_psr", "zoo_one_plane_depth4", "zoo_object_motion"])
def test_device_equals_the_restatement_on_zoo_frames(name):
    motion = name in spc.motion_cases()
    t, frame, camd, S, prm = _zoo_frame(spc.motion_cases()[name] if motion else name, motion)
    w, h = spc.W, spc.H
    st = None
    for suppress in (0.6, 0.0):      # the second sequence runs over the buffers the first left
        dn = _dn(camd, w, h, stablePlanesSuppressPrimaryIndirectSpecularK=suppress)
        _check_rr(t, frame, prm, dn, w, h, name)
        st = _check_nrd(t, frame, prm, dn, camd, S, w, h, spc.SAMPLE, "%s suppress %g" % (name, suppress), state=st)
    t.close()


def test_device_equals_the_committed_fixture():
    g = np.load(GOLDEN)
    t, frame, camd, S, prm = _zoo_frame("zoo_fp32")
    w, h = spc.W, spc.H
    dn = _dn(camd, w, h)
    for k in ("header", "stable_radiance", "spec_hit_t", "motion_vectors"): assert np.array_equal(frame[k], g["frame_" + k]), k
    t.denoiser_prepare_dlss_rr(prm, dn)
    got = t.get_denoiser_inputs(RR_KEYS)
    for k in RR_KEYS: assert _eq(got[k], g[k]), k
    assert _eq(t.radiance(), g["rr_output_color"])
    st = _check_nrd(t, frame, prm, dn, camd, S, w, h, spc.SAMPLE, "fixture")
    for k in ref.NRD_KEYS: assert _eq(st[k], g[k]), k
    assert _eq(st["output_color"], g["nrd_output_color"])
    t.close()


def _push(t, frame, w, h):
    """hand-built plane buffers into the context through pt_unpack_stable_planes (rank 0 of a world of one: the pixels in pt_shard_layout order)"""
    import rtxpt_amd as pt, torch
    px = pt.shard_layout(w, h, 0, 1)
    xs, ys = px >> 16, px & 0xFFFF
    stride = frame["planes"].shape[0] // 3
    rows = np.zeros((len(px), 71), np.uint32)
    rows[:, 0:4] = frame["header"][:, ys, xs].T
    for p in range(3): rows[:, 4 + 20 * p:24 + 20 * p] = frame["planes"][scenes.stable_planes_address(xs, ys, p, w, h)]
    rows[:, 64:66] = frame["stable_radiance"][ys, xs].view(np.uint32).reshape(-1, 2)
    rows[:, 66] = frame["depth"][ys, xs].view(np.uint32); rows[:, 67] = frame["spec_hit_t"][ys, xs].view(np.uint32)
    rows[:, 68:70] = frame["motion_vectors"][ys, xs].view(np.uint32).reshape(-1, 2); rows[:, 70] = frame["throughput"][ys, xs]
    b = torch.from_numpy(rows.view(np.int32).reshape(-1).copy()).to("cuda")
    t.unpack_stable_planes(b.data_ptr(), b.numel() * 4, 0)
    back = t.get_stable_planes()
    assert np.array_equal(back["header"], frame["header"]) and np.array_equal(back["spec_hit_t"], frame["spec_hit_t"])


FIXTURE_ZOO = {"zoo_fp32": ("zoo_fp32", {}), "zoo_lp16": ("zoo_lp16", {}), "zoo_two_planes_no_psr": ("zoo_two_planes_no_psr", {}), "zoo_thin_lens": ("zoo_fp32", dtc.THIN_LENS)}
FIXTURE_PUSHED = ("hand_frame_13x7", "fuzz0")


def _record(words, dtype): return np.frombuffer(np.ascontiguousarray(words).tobytes(), dtype)[0].copy()


@pytest.mark.parametrize("name", list(FIXTURE_ZOO) + list(FIXTURE_PUSHED))
def test_device_equals_the_reference_text_fixture(name):
    """Every buffer after every call against tests/golden/denoiser_inputs_golden.npz, which the compiled PostProcess.hlsl text made (tests/golden/make_denoiser_inputs_golden.py):
    the DLSS-RR pass, then Sample::Denoise's NRD sequence with the state after each plane's prepare and the colour after each merge. No restatement and no oracle in the loop;
    the thin-lens case has no other reference than the text. Zoo cases render their frame on the device and check its plane inputs against the fixture's first; hand-built and
    fuzz frames go in through pt_unpack_stable_planes."""
    import rtxpt_amd as pt
    g = np.load(GOLDEN)
    w, h, base = (int(v) for v in g[name + "_dims"])
    prm, dn, camd = _record(g[name + "_sp"], scenes.STABLE_PLANES_PARAMS_DTYPE), _record(g[name + "_dn"], pt.DENOISER_PARAMS_DTYPE), _record(g[name + "_cam"], scenes.CAMERA_DTYPE)
    if name in FIXTURE_ZOO:
        zoo, lens = FIXTURE_ZOO[name]
        sc, camd2, S, prm2, _ = dtc.zoo_setup(zoo, w, h, **lens)
        assert camd2.tobytes() == camd.tobytes() and np.asarray(prm2).tobytes() == prm.tobytes() and base == spc.SAMPLE
        if lens: assert float(camd["ApertureRadius"]) > 0
        t = _tracer(sc, camd, S, w, h)
        t.build_stable_planes(base, prm); t.fill_stable_planes(base, prm, sub_samples=spc.SUBSAMPLES); t.denoise_spec_hit_t()
        frame = t.get_stable_planes(); pre = "frame_" if name == "zoo_fp32" else name + "_frame_"
        for k in ("header", "stable_radiance", "spec_hit_t", "motion_vectors"): assert np.array_equal(frame[k].view(np.uint8), g[pre + k].view(np.uint8)), (name, k)
    else:
        sc, cam = scenes.stable_planes_zoo(); S = scenes.config_settings("C2")
        frame = {k: g["%s_frame_%s" % (name, k)] for k in ("header", "planes", "stable_radiance", "depth", "spec_hit_t", "motion_vectors", "throughput")}
        t = _tracer(sc, camd, S, w, h)
        t.build_stable_planes(base, scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam)))
        _push(t, frame, w, h)
    rr = "" if name == "zoo_fp32" else name + "_"      # zoo_fp32's DLSS-RR arrays keep the names they have had
    t.denoiser_prepare_dlss_rr(prm, dn)
    got = t.get_denoiser_inputs(RR_KEYS)
    for k in RR_KEYS: assert _eq(got[k], g[rr + k]), "%s: %s differs in %d values" % (name, k, _diff(got[k], g[rr + k]))
    assert _eq(t.radiance(), g[rr + "rr_output_color"]), "%s: DLSS-RR colour differs in %d values" % (name, _diff(t.radiance(), g[rr + "rr_output_color"]))
    active = int(min(max(int(prm["activeStablePlaneCount"]), 1), 3))
    for n, p in enumerate(range(active - 1, -1, -1)):
        t.denoiser_prepare_nrd(prm, dn, p, n == 0)
        got = t.get_denoiser_inputs(ref.NRD_KEYS); got["output_color"] = t.radiance()
        for k in ref.NRD_KEYS + ("output_color",):
            want = g["%s_p%d_%s" % (name, p, k)]
            assert _eq(got[k], want), "%s plane %d: %s differs in %d values" % (name, p, k, _diff(got[k], want))
        dd, ss = _upload(got["nrd_diff_radiance_hit_dist"]), _upload(got["nrd_spec_radiance_hit_dist"])
        t.denoiser_merge_nrd(p, dd.data_ptr(), ss.data_ptr())
        want = g["%s_p%d_merged" % (name, p)]
        assert _eq(t.radiance(), want), "%s plane %d: merged colour differs in %d values" % (name, p, _diff(t.radiance(), want))
    t.close()


def test_hand_built_corner_cases_on_the_device():
    import test_denoiser_inputs as cpu
    sc, cam = scenes.stable_planes_zoo()
    for case in cpu.hand_cases():
        frame, prm, dn, w, h = case["frame"], case["sp"], case["dn"], case["w"], case["h"]
        camd = scenes.bridge_camera(w, h, **cam); S = scenes.config_settings("C2")
        t = _tracer(sc, camd, S, w, h)
        t.build_stable_planes(0, scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam)))
        _push(t, frame, w, h)
        _check_rr(t, frame, prm, dn, w, h, case["name"])
        _check_nrd(t, frame, prm, dn, camd, S, w, h, 0, case["name"])
        t.close()


def test_second_frame_over_used_buffers_and_a_moving_camera():
    """realtime_cases' zoo: two frames with a moving camera through pt_realtime_frame; the second frame's passes run over the buffers the first left"""
    import rtxpt_amd as pt
    make, S, w, h, frames, subs, step, kw = rc.cases()["zoo_realtime"]
    sc, cam = make()
    t = _tracer(sc, scenes.bridge_camera(w, h, **cam), S, w, h)
    st = None
    for f in range(2):
        cur, prev = rc.camera(cam, step, f), rc.camera(cam, step, max(f - 1, 0))
        prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cur), prev_world_to_clip=scenes.view_projection(w, h, **prev), sub_samples=subs, **kw)
        camd = scenes.bridge_camera(w, h, **cur); t.set_camera(camd)
        frame, _, _ = t.realtime_frame(f * subs, prm); t.denoise_spec_hit_t(); frame = t.get_stable_planes()
        dn = _dn(camd, w, h)
        _check_rr(t, frame, prm, dn, w, h, "frame %d" % f)
        st = _check_nrd(t, frame, prm, dn, camd, S, w, h, f * subs, "frame %d" % f, state=st)
    t.close()


def test_tile_sharded_frame_equals_the_unsharded_one():
    import rtxpt_amd as pt, torch
    sc, camd, S, prm, _ = spc.setup("zoo_fp32"); w, h = spc.W, spc.H
    dn = _dn(camd, w, h)
    ranks = [_tracer(sc, camd, S, w, h, shard_rank=r, shard_count=2) for r in range(2)]
    for t in ranks: t.build_stable_planes(spc.SAMPLE, prm); t.fill_stable_planes(spc.SAMPLE, prm, sub_samples=spc.SUBSAMPLES)
    with pytest.raises(pt.PtError) as e: ranks[0].denoiser_prepare_dlss_rr(prm, dn)
    assert e.value.code == pt.PT_ERROR_NOT_READY
    n = ranks[1].stable_planes_shard_bytes(1); b = torch.empty(n // 4, dtype=torch.int32, device="cuda"); ranks[1].pack_stable_planes(b.data_ptr(), n)
    ranks[0].unpack_stable_planes(b.data_ptr(), n, 1); ranks[0].denoise_spec_hit_t()
    u, frame, _, _, _ = _zoo_frame("zoo_fp32")
    outs = []
    for t in (ranks[0], u):
        t.denoiser_prepare_dlss_rr(prm, dn); rr = t.get_denoiser_inputs(); rr["color"] = t.radiance()
        for p in (2, 1, 0): t.denoiser_prepare_nrd(prm, dn, p, p == 2)
        rr.update({"nrd_" + k: v for k, v in t.get_denoiser_inputs(ref.NRD_KEYS).items()}); rr["nrd_color"] = t.radiance()
        outs.append(rr)
    for k in outs[1]: assert _eq(outs[0][k], outs[1][k]), k
    for t in ranks + [u]: t.close()


def test_refusals():
    import rtxpt_amd as pt
    sc, camd, S, prm, _ = spc.setup("zoo_fp32"); w, h = spc.W, spc.H
    dn = _dn(camd, w, h)
    t = _tracer(sc, camd, S, w, h)
    for call in (lambda: t.denoiser_prepare_dlss_rr(prm, dn), lambda: t.denoiser_prepare_nrd(prm, dn, 0, True), lambda: t.get_denoiser_inputs(), lambda: t.denoiser_device_buffers()):
        with pytest.raises(pt.PtError) as e: call()
        assert e.value.code == pt.PT_ERROR_NOT_READY
    t.build_stable_planes(spc.SAMPLE, prm)
    with pytest.raises(pt.PtError) as e: t.denoiser_merge_nrd(0, 16, 16)      # no NRD prepare yet: refused before any pointer is read
    assert e.value.code == pt.PT_ERROR_NOT_READY
    with pytest.raises(pt.PtError) as e: t.denoiser_prepare_nrd(prm, dn, 3, True)
    assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT
    t.denoiser_prepare_nrd(prm, dn, 0, True)
    with pytest.raises(pt.PtError) as e: t.denoiser_merge_nrd(3, 16, 16)
    assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT
    with pytest.raises(pt.PtError) as e: t.denoiser_merge_nrd(0, 0, 0)
    assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT
    bufs = t.denoiser_device_buffers()
    assert all(p != 0 for p, _ in bufs.values()) and bufs["nrd_normal_roughness"][1] == 16 * w and bufs["nrd_combined_history_clamp_relax"][1] == w
    t.close()
