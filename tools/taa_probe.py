"""Times the temporal anti-aliasing resolve (pt_taa_resolve's gpuMs) on realtime frames of bench.py's scene at 3840 x 2160 and 1920 x 1080, next to the device denoiser's
history-clamp pass (pt_denoise_pass_times) measured in the same process run: the nearest existing kernel, a 3 x 3 LDS stencil of the same tile shape.

Per size: one realtime frame, then `warmup + reps` times pt_denoise_frame's loop (prepare, denoise, merge per plane) followed by pt_taa_resolve with the default parameters
(Catmull-Rom history, clamping with the relax buffer, luminance weighting), all on that frame, so every resolve after the first reprojects into the previous one's result.
Medians of the warm runs; bytes are algorithmic (what the pass must read and write once, from the buffer layouts below). Writes the report to stdout; --out also to a file
(profiles/taa_resolve.txt).

  python tools/taa_probe.py --out profiles/taa_resolve.txt              (on the GPU)
  python tools/taa_probe.py --rehearse                                  (no GPU: argument parsing, scene, byte counts)"""
import argparse, os, sys
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12      # bytes / s (MI355X)
TAA_BYTES = 16 + 8 + 1 + 16 + 16      # per pixel: colour, motion vector, relax byte, the history (every texel once), the resolved picture
CLAMP_BYTES = 161                     # per surface pixel of a plane (tools/denoise_probe.py CLAMP_BYTES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3840x2160,1920x1080"); ap.add_argument("--reps", type=int, default=9); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0); ap.add_argument("--tex", type=int, default=1024); ap.add_argument("--out"); ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    import denoiser_inputs_ref as ref
    lines = []
    def say(s=""): print(s, flush=True); lines.append(s)
    sc, cam = scenes.bistro_like(scale=a.scale, tex_size=a.tex); S = scenes.default_settings(useFp16Types=1)
    say("temporal anti-aliasing resolve on bench.py's scene (bistro-like, scale %g, textures %d^2): warm, event-timed medians of %d runs after %d; bytes are algorithmic" % (a.scale, a.tex, a.reps, a.warmup))
    say("bytes: resolve %d per pixel (colour 16, motion 8, relax 1, history 16, result 16); history clamp %d per surface pixel of a plane; HBM peak %.1f TB/s" % (TAA_BYTES, CLAMP_BYTES, HBM_PEAK * 1e-12))
    if a.rehearse: say("rehearsal: no device, nothing measured"); return
    t = pt.PathTracer(); t.set_scene(sc); t.set_settings(S)
    ds, tp = pt.denoise_default_settings(), pt.taa_default_params()
    for w, h in [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]:
        camd = scenes.bridge_camera(w, h, **cam); t.set_camera(camd); t.resize(w, h)
        prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam), sub_samples=1)
        t.realtime_frame(0, prm); t.denoise_spec_hit_t()
        dn = ref.case_params(camd); active = int(prm["activeStablePlaneCount"])
        t.denoise_pass_times(True)
        surf, clamp, clamp0, taa = {}, [], [], []
        for rep in range(a.warmup + a.reps):
            ms = ms0 = 0.0
            for i, p in enumerate(range(active - 1, -1, -1)):
                t.denoiser_prepare_nrd(prm, dn, p, i == 0)
                if rep == 0: surf[p] = int((t.get_denoiser_inputs(("nrd_view_z",))["nrd_view_z"] != ref.FLT_MAX).sum())
                t.denoise_plane(prm, ds, p, rep == 0); ms0 = float(t.denoise_pass_times(True)[1]); ms += ms0      # (plane 0 comes last)
                dp, sp, _ = t.denoised_device_buffers(p); t.denoiser_merge_nrd(p, dp, sp)
            _, resolve_ms = t.taa_resolve(tp, reset_history=rep == 0, timed=True)
            if rep >= a.warmup: clamp.append(ms); clamp0.append(ms0); taa.append(resolve_ms)
        N = w * h; relax = t.get_denoiser_inputs(("nrd_combined_history_clamp_relax",))["nrd_combined_history_clamp_relax"]
        say(); say("%d x %d, %d planes, surface pixels per plane %s of %d; relax byte not 0 in %d pixels" % (w, h, active, [surf[p] for p in range(active)], N, int((relax != 0).sum())))
        say("  %-36s %9s %9s %9s %10s %9s %8s" % ("pass", "ms", "min", "max", "MB", "GB/s", "% peak"))
        rows = (("taa resolve", taa, float(TAA_BYTES * N)), ("denoiser history clamp (all planes)", clamp, float(sum(CLAMP_BYTES * surf[p] for p in surf))),
                ("denoiser history clamp (plane 0)", clamp0, float(CLAMP_BYTES * surf[0])))
        rates = []
        for name, v, by in rows:
            m = float(np.median(v)); rate = by / (m * 1e-3); rates.append(rate)
            say("  %-36s %9.3f %9.3f %9.3f %10.1f %9.0f %8.1f" % (name, m, min(v), max(v), by * 1e-6, rate * 1e-9, 100 * rate / HBM_PEAK))
        say("  resolve per byte: %.2f x the clamp's rate over all planes, %.2f x plane 0's (the other planes are nearly all sky: blocks that only write zeros)" % (rates[0] / rates[1], rates[0] / rates[2]))
    t.close()
    if a.out:
        with open(a.out, "w") as f: f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
