"""Generates tests/golden/denoiser_inputs_golden.npz from the COMPILED REFERENCE TEXT: the three denoiser entry points of PostProcess.hlsl as the oracle/refpin recipe compiles
them (oracle.ptref.denoiser_prepare_dlss_rr / denoiser_prepare_nrd / denoiser_merge_nrd, reference=True), not from the numpy restatement. Needs the reference checkout.

  zoo_fp32                 the committed reference-text planes of tests/golden/stable_planes_golden.npz (build pass, fill passes, DenoiseSpecHitT); its arrays keep their
                           unprefixed names (frame_*, rr_*, nrd_* = the state after the last merge), the per-plane arrays below come with the prefix
  zoo_lp16, zoo_two_planes_no_psr, zoo_thin_lens      the oracle's frames at 40 x 24 (the GPU test renders them itself and checks the frame_* inputs first)
  hand_frame_13x7          test_denoiser_inputs.hand_cases' 13 x 7 frame, inputs included
  fuzz0                    the top-left 24 x 16 pixels of denoiser_text_cases.fuzz_case(0), inputs included
Per case: <case>_rr_* and <case>_rr_output_color, then Sample::Denoise's NRD sequence with the identity as the denoiser: <case>_p<plane>_<buffer> after that plane's prepare,
<case>_p<plane>_merged the colour after its merge; <case>_sp / _dn / _cam / _dims the parameter records as words (dims: width, height, sample base index).
Run from the repository root:   python tests/golden/make_denoiser_inputs_golden.py"""
import os, sys
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoiser_inputs_ref as ref
import denoiser_text_cases as dtc
import stable_planes_cases as spc

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "denoiser_inputs_golden.npz")
RR = ("rr_diffuse_albedo", "rr_specular_albedo", "rr_normal_roughness", "rr_specular_motion_vectors")
FRAME_CHECK = ("header", "stable_radiance", "spec_hit_t", "motion_vectors")
FRAME_ALL = ("header", "planes", "stable_radiance", "depth", "spec_hit_t", "motion_vectors", "throughput")
SMALL = (40, 24)


def fixture_cases():
    """name -> the case (denoiser_text_cases layout) and which of the frame's arrays travel with it"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "stable_planes_golden.npz"))
    sc, camd, S, prm, lp16 = spc.setup("zoo_fp32")
    fp32 = dict(name="zoo_fp32", frame=ref.frame_from_stable_planes_golden(g, "zoo_fp32", spc.W, spc.H), sp=prm, dn=ref.case_params(camd), cam=camd, S=S, w=spc.W, h=spc.H, base=spc.SAMPLE, rays=None)
    hand = [c for c in dtc.hand_text_cases() if c["name"] == "hand_frame_13x7"][0]
    return [(fp32, FRAME_CHECK), (dtc.oracle_zoo_case("zoo_lp16", *SMALL), FRAME_CHECK), (dtc.oracle_zoo_case("zoo_two_planes_no_psr", *SMALL), FRAME_CHECK),
            (dtc.oracle_zoo_case("zoo_fp32", *SMALL, tag="zoo_thin_lens", **dtc.THIN_LENS), FRAME_CHECK), (hand, FRAME_ALL), (dtc.crop(dtc.fuzz_case(0), 24, 16), FRAME_ALL)]


def run_text(case):
    """every output of the compiled text for one case: name -> array (unprefixed)"""
    from oracle import ptref
    fr, sp, dn, cam, S, base = case["frame"], case["sp"], case["dn"], case["cam"], case["S"], case["base"]
    out = {}
    rr = ptref.denoiser_prepare_dlss_rr(fr, sp, dn, cam, S, base)
    for k in RR: out[k] = rr[k]
    out["rr_output_color"] = rr["output_color"]
    st, per, merged = ptref.denoiser_nrd_sequence(fr, sp, dn, cam, S, base)
    for p in per:
        for k in ref.NRD_KEYS + ("output_color",): out["p%d_%s" % (p, k)] = per[p][k]
        out["p%d_merged" % p] = merged[p]
    out["sp"] = np.frombuffer(np.ascontiguousarray(sp).tobytes(), np.uint32).copy(); out["dn"] = np.frombuffer(np.ascontiguousarray(dn).tobytes(), np.float32).copy()
    out["cam"] = np.frombuffer(np.ascontiguousarray(cam).tobytes(), np.uint32).copy(); out["dims"] = np.array([case["w"], case["h"], base], np.uint32)
    return out, st


def generate():
    out = {}
    for case, frame_keys in fixture_cases():
        name = case["name"]; res, st = run_text(case)
        if name == "zoo_fp32":      # the names the fixture has had since it was made by the restatement
            for k in FRAME_CHECK: out["frame_" + k] = case["frame"][k]
            for k in RR + ("rr_output_color",): out[k] = res.pop(k)
            for k in ref.NRD_KEYS: out[k] = st[k]
            out["nrd_output_color"] = st["output_color"]
        else:
            for k in frame_keys: out["%s_frame_%s" % (name, k)] = np.asarray(case["frame"][k])
        for k, v in res.items(): out["%s_%s" % (name, k)] = v
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **generate())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
