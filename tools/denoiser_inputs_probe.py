"""Times the denoiser passes of a realtime stable-plane frame (pt_denoiser_prepare_dlss_rr, pt_denoiser_prepare_nrd per plane, pt_denoiser_merge_nrd per plane) on one frame of the
stable-plane zoo at the given size (default 3840 x 2160). Prints one JSON line: the median wall time of each call over --reps runs (each call ends in a stream synchronise, so this
is kernel time plus the call's fixed overhead). For kernel times alone run it under `rocprofv3 --kernel-trace --stats -- python tools/denoiser_inputs_probe.py` (k_dn_*)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtxpt_amd as pt
from rtxpt_amd import scenes
import denoiser_inputs_ref as ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840); ap.add_argument("--height", type=int, default=2160); ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    w, h = a.width, a.height
    sc, cam = scenes.stable_planes_zoo(); S = scenes.config_settings("C2")
    camd = scenes.bridge_camera(w, h, **cam)
    t = pt.PathTracer(); t.set_scene(sc); t.set_settings(S); t.set_camera(camd); t.resize(w, h)
    prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam))
    t.realtime_frame(0, prm); t.denoise_spec_hit_t()
    dn = ref.case_params(camd)
    diff = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"); spec = torch.zeros_like(diff)

    def timed(fn):
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); fn(); ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms))
    res = {"width": w, "height": h, "reps": a.reps, "dlss_rr_ms": timed(lambda: t.denoiser_prepare_dlss_rr(prm, dn))}
    for p in (2, 1, 0):
        res["nrd_prepare_plane%d_ms" % p] = timed(lambda: t.denoiser_prepare_nrd(prm, dn, p, p == 2))
        res["nrd_merge_plane%d_ms" % p] = timed(lambda: t.denoiser_merge_nrd(p, diff.data_ptr(), spec.data_ptr()))
    live = t.get_stable_planes()["header"][:3] != 0xFFFFFFFF
    res["live_planes_per_pixel"] = float(live.sum()) / (w * h)
    print(json.dumps(res))
    t.close()


if __name__ == "__main__":
    main()
