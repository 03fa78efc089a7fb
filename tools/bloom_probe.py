"""Times the bloom pass (pt_bloom's gpuMs: its four kernels, first launch to last) on realtime frames of bench.py's scene at 3840 x 2160 and 1920 x 1080, at the default
parameters (radius 8: 6 taps a side) and at radius 64 (48 taps a side), next to the temporal anti-aliasing resolve (pt_taa_resolve's gpuMs) measured in the same process run:
the nearest kernel of the parent tree, one 16-byte record in and out per pixel through an LDS-staged tile.

Per size: one realtime frame behind pt_denoise_frame, then `warmup + reps` times pt_taa_resolve followed by pt_bloom(source 1) at each radius, all on that frame. Medians of the
warm runs; bytes are algorithmic (what the pass must read and write once, from the shapes below), not measured traffic. Writes the report to stdout; --out also to a file
(profiles/bloom.txt).

  python tools/bloom_probe.py --out profiles/bloom.txt                  (on the GPU)
  python tools/bloom_probe.py --rehearse                                (no GPU: argument parsing, scene, byte counts)"""
import argparse, os, sys
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12      # bytes / s (MI355X)
TAA_BYTES = 16 + 8 + 1 + 16 + 16      # per pixel (tools/taa_probe.py TAA_BYTES)
PIXEL_BYTES = 16 + 16 + 16            # per pixel: the reduce's read, the composite's read, the composite's write
QUARTER_BYTES = 16 * (1 + 2 + 2 + 1)  # per quarter-resolution texel: the reduce's write, a read and a write per blur axis, the composite's read
RADII = (8.0, 64.0)


def bloom_bytes(w, h):
    return float(PIXEL_BYTES * w * h + QUARTER_BYTES * ((w + 3) // 4) * ((h + 3) // 4))


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
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    sc, cam = scenes.bistro_like(scale=a.scale, tex_size=a.tex); S = scenes.default_settings(useFp16Types=1)
    say("bloom pass on bench.py's scene (bistro-like, scale %g, textures %d^2): warm, event-timed medians of %d runs after %d; bytes are algorithmic" % (a.scale, a.tex, a.reps, a.warmup))
    say("bytes: bloom %d per pixel (reduce read 16, composite read 16, result 16) + %d per quarter-resolution texel (reduce write 16, blur x 32, blur y 32, composite read 16);"
        " resolve %d per pixel; HBM peak %.1f TB/s" % (PIXEL_BYTES, QUARTER_BYTES, TAA_BYTES, HBM_PEAK * 1e-12))
    for w, h in sizes:
        say("  %d x %d: quarter resolution %d x %d, %.1f MB a call = %.2f bytes per pixel" % (w, h, (w + 3) // 4, (h + 3) // 4, bloom_bytes(w, h) * 1e-6, bloom_bytes(w, h) / (w * h)))
    for r in RADII: say("  radius %g: %d taps a side" % (r, len(pt.bloom_kernel(r)[0]) - 1))
    if a.rehearse: say("rehearsal: no device, nothing measured"); return
    t = pt.PathTracer(); t.set_scene(sc); t.set_settings(S)
    ds, tp = pt.denoise_default_settings(), pt.taa_default_params()
    for w, h in sizes:
        camd = scenes.bridge_camera(w, h, **cam); t.set_camera(camd); t.resize(w, h)
        prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam), sub_samples=1)
        t.realtime_frame(0, prm); t.denoise_spec_hit_t()
        t.denoise_frame(prm, ref.case_params(camd), ds, reset_history=True)
        taa, blm = [], {r: [] for r in RADII}
        for rep in range(a.warmup + a.reps):
            _, resolve_ms = t.taa_resolve(tp, reset_history=rep == 0, timed=True)
            ms = {r: t.bloom(pt.bloom_default_params(radius=r), source=1, timed=True)[1] for r in RADII}
            if rep >= a.warmup:
                taa.append(resolve_ms)
                for r in RADII: blm[r].append(ms[r])
        N = w * h
        say(); say("%d x %d" % (w, h))
        say("  %-36s %9s %9s %9s %10s %9s %8s" % ("pass", "ms", "min", "max", "MB", "GB/s", "% peak"))
        rows = [("taa resolve", taa, float(TAA_BYTES * N))] + [("bloom, radius %g%s" % (r, " (default)" if r == 8.0 else ""), blm[r], bloom_bytes(w, h)) for r in RADII]
        rates = []
        for name, v, by in rows:
            m = float(np.median(v)); rate = by / (m * 1e-3); rates.append(rate)
            say("  %-36s %9.3f %9.3f %9.3f %10.1f %9.0f %8.1f" % (name, m, min(v), max(v), by * 1e-6, rate * 1e-9, 100 * rate / HBM_PEAK))
        say("  bloom per byte: %.2f x the resolve's rate at the default radius, %.2f x at radius 64" % (rates[1] / rates[0], rates[2] / rates[0]))
    t.close()
    if a.out:
        with open(a.out, "w") as f: f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
