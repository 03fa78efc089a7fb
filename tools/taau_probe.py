"""Times the temporal upscaling resolve (pt_taa_upscale's gpuMs) on realtime frames of bench.py's scene traced at 1920 x 1080, 2560 x 1440, 1280 x 720 and 3840 x 2160 for a
3840 x 2160 display, next to pt_taa_resolve at 3840 x 2160 measured in the same process run: that kernel is the nearest one (the same tile shape and history taps) and this
pass equals it at ratio 1.

Per render size: one realtime frame behind pt_denoise_frame (so the relax buffer is this frame's), then `warmup + reps` calls of pt_taa_upscale with the default parameters
(Catmull-Rom history, clamping with the relax buffer, luminance and confidence weighting) and the Halton jitters, all on that frame, so every call after the first reprojects
into the previous one's result. Medians of the warm runs with minimum and maximum; bytes are algorithmic (what the pass must read and write once, from the buffer layouts
below). Writes the report to stdout; --out also to a file (profiles/taa_upscale.txt).

  python tools/taau_probe.py --out profiles/taa_upscale.txt             (on the GPU)
  python tools/taau_probe.py --rehearse                                 (no GPU: argument parsing, scene, byte counts)"""
import argparse, os, sys
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12      # bytes / s (MI355X)
DISPLAY_BYTES = 16 + 16               # per display pixel: the history (every texel once), the upscaled picture
RENDER_BYTES = 16 + 8 + 1             # per render pixel: colour, motion vector, relax byte
TAA_BYTES = 16 + 8 + 1 + 16 + 16      # pt_taa_resolve per pixel (tools/taa_probe.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--display", default="3840x2160"); ap.add_argument("--sizes", default="1920x1080,2560x1440,1280x720,3840x2160")
    ap.add_argument("--reps", type=int, default=9); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0); ap.add_argument("--tex", type=int, default=1024); ap.add_argument("--out"); ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    import denoiser_inputs_ref as ref
    lines = []
    def say(s=""): print(s, flush=True); lines.append(s)
    size = lambda s: tuple(int(v) for v in s.split("x"))
    W, H = size(a.display); sizes = [size(s) for s in a.sizes.split(",")]
    sc, cam = scenes.bistro_like(scale=a.scale, tex_size=a.tex)
    say("temporal upscaling resolve on bench.py's scene (bistro-like, scale %g, textures %d^2), display %d x %d: warm, event-timed medians of %d runs after %d; bytes are algorithmic" % (a.scale, a.tex, W, H, a.reps, a.warmup))
    say("bytes: upscale %d per display pixel (history 16, result 16) + %d per render pixel (colour 16, motion 8, relax 1); resolve %d per pixel; HBM peak %.1f TB/s" % (DISPLAY_BYTES, RENDER_BYTES, TAA_BYTES, HBM_PEAK * 1e-12))
    for w, h in sizes:
        say("  render %4d x %4d: %.1f MB, texture LOD bias %+.4f" % (w, h, (DISPLAY_BYTES * W * H + RENDER_BYTES * w * h) * 1e-6, float(pt.upscale_tex_lod_bias(w, h, W, H))))
    if a.rehearse: say("rehearsal: no device, nothing measured"); return
    t = pt.PathTracer(); t.set_scene(sc)
    ds, up, tp = pt.denoise_default_settings(), pt.taa_upscale_default_params(), pt.taa_default_params()
    base = float(scenes.default_settings()["texLODBias"])
    say(); say("  %-44s %9s %9s %9s %10s %9s %8s" % ("pass", "ms", "min", "max", "MB", "GB/s", "% peak"))
    rows = {}
    def row(name, v, by):
        m = float(np.median(v)); rate = by / (m * 1e-3); rows[name] = (m, rate)
        say("  %-44s %9.3f %9.3f %9.3f %10.1f %9.0f %8.1f" % (name, m, min(v), max(v), by * 1e-6, rate * 1e-9, 100 * rate / HBM_PEAK))
    for w, h, resolve in [(w, h, False) for w, h in sizes] + [(W, H, True)]:      # last: pt_taa_resolve at the display size
        t.set_settings(scenes.default_settings(useFp16Types=1, texLODBias=base + (0.0 if resolve else float(pt.upscale_tex_lod_bias(w, h, W, H)))))
        camd = scenes.bridge_camera(w, h, **cam); t.set_camera(camd); t.resize(w, h)
        prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam), sub_samples=1)
        t.realtime_frame(0, prm); t.denoise_spec_hit_t(); t.denoise_frame(prm, ref.case_params(camd), ds, reset_history=True)
        ms = []
        for rep in range(a.warmup + a.reps):
            if resolve: _, v = t.taa_resolve(tp, reset_history=rep == 0, timed=True)
            else: _, v = t.taa_upscale(up, (W, H), pt.taa_jitter(pt.TAA_JITTER_HALTON, rep), reset_history=rep == 0, timed=True)
            if rep >= a.warmup: ms.append(v)
        if resolve: row("pt_taa_resolve %d x %d" % (W, H), ms, float(TAA_BYTES * W * H))
        else: row("pt_taa_upscale %d x %d -> %d x %d" % (w, h, W, H), ms, float(DISPLAY_BYTES * W * H + RENDER_BYTES * w * h))
    say()
    m0, r0 = rows["pt_taa_resolve %d x %d" % (W, H)]
    for name, (m, rate) in rows.items():
        if name.startswith("pt_taa_upscale"): say("  %s: %.2f x the resolve's time, %.2f x its rate per byte" % (name, m / m0, rate / r0))
    t.close()
    if a.out:
        with open(a.out, "w") as f: f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
