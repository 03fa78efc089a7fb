"""The numpy restatement of the denoiser passes (tests/denoiser_inputs_ref.py) held against the reference's own PostProcess.hlsl text, compiled by the oracle/refpin recipe
(oracle/refpin/hlsl_tu.py main_pt, hlsl_postprocess_stubs.h; oracle.ptref.denoiser_prepare_dlss_rr / denoiser_prepare_nrd / denoiser_merge_nrd): every pixel and every word of
every output buffer, the output colour after each merge and the state after each plane's prepare included. Nothing is masked; the only normalisation is ref.canonical (NaN
payload and sign). The committed fixture (tests/golden/denoiser_inputs_golden.npz) is made by the same text and must regenerate bit for bit.

The thin-lens case: the restatement's camera_rays covers the pinhole camera only. There the restatement runs with the oracle's camera rays (ptref_camera_ray, the C++
restatement of Bridge::computeCameraRay that the integrator pin holds), so everything but its own ray generation is still compared; the answer itself is the text's, and the
device is held to it through the fixture (tests/test_gpu_zzz_denoiser_inputs.py) without any restatement in the loop."""
import os, sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoiser_inputs_ref as ref
import denoiser_text_cases as dtc
import stable_planes_cases as spc
from oracle import ptref

pytestmark = pytest.mark.skipif(not os.path.isdir("/root/reference/Rtxpt/Shaders"), reason="needs the reference text")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "denoiser_inputs_golden.npz")
RR_KEYS = ("rr_diffuse_albedo", "rr_specular_albedo", "rr_normal_roughness", "rr_specular_motion_vectors", "output_color")
STATE_KEYS = ref.NRD_KEYS + ("output_color",)


def _same(want, got, keys, tag):
    for k in keys:
        a, b = ref.canonical(np.asarray(want[k])), ref.canonical(np.asarray(got[k]))
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, k, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), "%s: %s differs in %d of %d values, first at %s" % (tag, k, int((a != b).sum()), a.size, np.argwhere(a != b)[:3].tolist())


def _rays(case):
    return case["rays"] if case["rays"] is not None else {p: ref.camera_rays(case["cam"], case["S"], case["w"], case["h"], case["base"] + p) for p in range(3)}


def check_case(case, dn=None, state_ref=None, state_text=None):
    """the DLSS-RR pass and the whole NRD sequence of one case, restatement == text after every call; returns both final states and the text's outputs"""
    fr, sp, w, h = case["frame"], case["sp"], case["w"], case["h"]; dn = case["dn"] if dn is None else dn
    rr = ptref.denoiser_prepare_dlss_rr(fr, sp, dn, case["cam"], case["S"], case["base"])
    _same(ref.dlss_rr(fr, sp, dn, w, h), rr, RR_KEYS, case["name"] + " DLSS-RR")
    st, per = ref.nrd_sequence(fr, sp, dn, w, h, _rays(case), state=state_ref)
    tst, tper, tmerged = ptref.denoiser_nrd_sequence(fr, sp, dn, case["cam"], case["S"], case["base"], state=state_text)
    active = len(per); order = list(range(active - 1, -1, -1))
    for n, p in enumerate(order):
        _same(per[p], tper[p], STATE_KEYS, "%s NRD prepare of plane %d" % (case["name"], p))
    # the colour after each merge: replay the restatement's merges over its own per-plane states
    for p in order:
        want = ref.nrd_merge(per[p], fr, w, h, p, per[p]["nrd_diff_radiance_hit_dist"], per[p]["nrd_spec_radiance_hit_dist"])
        _same({"output_color": want}, {"output_color": tmerged[p]}, ("output_color",), "%s colour after the merge of plane %d" % (case["name"], p))
    _same(st, tst, STATE_KEYS, case["name"] + " final state")
    # REBLUR_FrontEnd_GetNormHitDist's recorded arguments: (0, 1) for the diffuse call, (specHitT, the plane's raw roughness) for the specular one
    for p in order:
        calls = tper[p]["norm_hit_dist_calls"]; has = tper[p]["nrd_view_z"] != ref.FLT_MAX
        assert np.all(calls[has][:, 0] == 0) and np.all(calls[has][:, 1] == 1), (case["name"], p)
        assert np.array_equal(calls[has][:, 2].view(np.uint32), tper[p]["nrd_spec_radiance_hit_dist"][has][:, 3].view(np.uint32)), (case["name"], p)
    # USE_RELAX 1 records the same buffers (it has no roughness argument: nrd_roughness stays what the state held, zero from an empty state)
    if state_text is None:
        _, rper, rmerged = ptref.denoiser_nrd_sequence(fr, sp, dn, case["cam"], case["S"], case["base"], use_relax=True)
        for p in order:
            _same(tper[p], rper[p], tuple(k for k in STATE_KEYS if k != "nrd_roughness"), "%s USE_RELAX 1 against 0, plane %d" % (case["name"], p))
            _same({"c": tmerged[p]}, {"c": rmerged[p]}, ("c",), "%s USE_RELAX 1 against 0, merge of plane %d" % (case["name"], p))
            assert not rper[p]["nrd_roughness"].any()
    return st, tst, rr, tper


@pytest.mark.parametrize("name", dtc.ZOO)
def test_restatement_equals_the_text_on_zoo_frames(name):
    case = dtc.oracle_zoo_case(name)
    st = tst = None
    for suppress in (0.6, 0.0):      # the second sequence runs over the buffers the first left
        dn = ref.case_params(case["cam"], stablePlanesSuppressPrimaryIndirectSpecularK=suppress)
        st, tst, _, _ = check_case(case, dn, st, tst)


def test_restatement_equals_the_text_on_the_hand_cases():
    for case in dtc.hand_text_cases(): check_case(case)


def test_restatement_equals_the_text_on_two_realtime_frames():
    st = tst = None
    for case in dtc.oracle_realtime_cases(2): st, tst, _, _ = check_case(case, None, st, tst)


def test_thin_lens_frame():
    case = dtc.oracle_zoo_case("zoo_fp32", tag="zoo_thin_lens", **dtc.THIN_LENS)
    assert float(case["cam"]["ApertureRadius"]) > 0
    with pytest.raises(NotImplementedError): ref.camera_rays(case["cam"], case["S"], case["w"], case["h"], 0)      # the restatement's own rays stop at the pinhole
    _, _, _, tper = check_case(case)
    # the lens matters: the same frame through the pinhole camera of the same pose has another viewZ nearly everywhere there is a surface
    pin = dict(case); pin["cam"] = case["cam"].copy(); pin["cam"]["ApertureRadius"] = 0
    other = ptref.denoiser_prepare_nrd(ptref.denoiser_empty_state(case["w"], case["h"]), case["frame"], case["sp"], case["dn"], pin["cam"], case["S"], 0, True, case["base"])
    has = tper[0]["nrd_view_z"] != ref.FLT_MAX
    assert has.sum() > has.size // 2 and (other["nrd_view_z"][has] != tper[0]["nrd_view_z"][has]).mean() > 0.9


@pytest.mark.parametrize("index", range(len(dtc.FUZZ)))
def test_fuzz_frames_and_their_branch_census(index):
    """Every listed branch of the three entry points is taken both ways by at least 1 % of the frame's pixels, counted from the inputs and the text's outputs
    (denoiser_text_cases.branch_census). One side cannot be reached by any input and is asserted to be empty instead: `weight > 1e-6` (PostProcess.hlsl:301) is true for
    every plane the loop visits, because an available plane's weight is at least 0.01 / 0.68 after the normalisation (kNW = 0.01 is added to every plane before the product
    with spAvailable, and the sum is at most 3 x 0.2 + 3 x 0.01 + 0.05)."""
    case = dtc.fuzz_case(index)
    w, h = case["w"], case["h"]; assert w * h >= 4096
    _, _, rr, tper = check_case(case)
    census = dtc.branch_census(case, rr, tper)
    need = -(-w * h // 100)
    for k, (a, b) in sorted(census.items()): print("%s %-70s %6d %6d" % (case["name"], k, a, b))
    a, b = census.pop("layer weight above / not above 1e-6")
    assert a >= need and b == 0
    for k, (a, b) in census.items(): assert a >= need and b >= need, (case["name"], k, a, b, need)


def test_fuzz_covers_the_plane_counts_and_an_odd_size():
    assert sorted({f[2] for f in dtc.FUZZ}) == [1, 2, 3] and len(dtc.FUZZ) >= 4
    assert any(f[0] % 8 and f[1] % 8 for f in dtc.FUZZ) and any(f[4] == 0 for f in dtc.FUZZ)


def test_the_fixture_regenerates_bit_for_bit():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_dn_golden", os.path.join(ROOT, "tests", "golden", "make_denoiser_inputs_golden.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    got, g = m.generate(), np.load(GOLDEN)
    assert sorted(got) == sorted(g.keys())
    for k in got:
        assert got[k].dtype == g[k].dtype and got[k].shape == g[k].shape, k
        assert np.array_equal(np.asarray(got[k]).view(np.uint8), g[k].view(np.uint8)), k
