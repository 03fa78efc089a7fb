"""Generates tests/golden/denoiser_inputs_golden.npz: the denoiser passes of PostProcess.hlsl (tests/denoiser_inputs_ref.py, the numpy restatement of the reference text) over the
reference-text plane outputs of the zoo_fp32 case committed in tests/golden/stable_planes_golden.npz (its build-pass records, the fill passes' noisy radiance and the DenoiseSpecHitT
fill-in): the DLSS-RR inputs and output colour, then Sample::Denoise's NRD sequence (planes 2, 1, 0) with the identity as the denoiser. The GPU tests compare the device with it.
Run from the repository root:   python tests/golden/make_denoiser_inputs_golden.py"""
import os, sys
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoiser_inputs_ref as ref
import stable_planes_cases as spc

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "denoiser_inputs_golden.npz")


def generate():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "stable_planes_golden.npz"))
    sc, camd, S, prm, lp16 = spc.setup("zoo_fp32")
    w, h = spc.W, spc.H
    fr = ref.frame_from_stable_planes_golden(g, "zoo_fp32", w, h)
    dn = ref.case_params(camd)
    out = {"frame_" + k: fr[k] for k in ("header", "stable_radiance", "spec_hit_t", "motion_vectors")}
    rr = ref.dlss_rr(fr, prm, dn, w, h)
    for k in ("rr_diffuse_albedo", "rr_specular_albedo", "rr_normal_roughness", "rr_specular_motion_vectors"): out[k] = rr[k]
    out["rr_output_color"] = rr["output_color"]
    rays = {p: ref.camera_rays(camd, S, w, h, spc.SAMPLE + p) for p in range(3)}
    st, _ = ref.nrd_sequence(fr, prm, dn, w, h, rays)
    for k in ref.NRD_KEYS: out[k] = st[k]
    out["nrd_output_color"] = st["output_color"]
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **generate())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
