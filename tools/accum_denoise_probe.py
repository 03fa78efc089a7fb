"""Times the reference-mode denoiser (pt_accum_denoise's gpuMs: its two launches, first to last) on bench.py's scene at 3840 x 2160 after render_adaptive, at the default
parameters (r 5, f 2) and at the largest window (r 8, f 3), and measures what it does to the picture: the relative L2 distance to a 256-sample frame of the 16- and 64-sample
frames, noisy and denoised, on radiance clamped to maxRadiance so that the brightest pixels do not carry the figure.

Per sample count n: render_adaptive with threshold 0 and minSamples = step = 8, maxSamples = n (the bits of render(0, n)), then `warmup + reps` calls at each parameter set on
that state. Medians of the warm runs with their spread (min, max). Writes the report to stdout; --out also to a file (profiles/accum_denoise.txt).

  python tools/accum_denoise_probe.py --out profiles/accum_denoise.txt        (on the GPU)
  python tools/accum_denoise_probe.py --rehearse                               (no GPU: argument parsing, scene, LDS sizes)"""
import argparse, os, sys
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

SETS = (("r 5, f 2 (default)", dict()), ("r 8, f 3", dict(searchRadius=8, patchRadius=3)), ("r 1, f 0", dict(searchRadius=1, patchRadius=0)))


def lds_bytes(r, f):
    """the filter launch's dynamic LDS (pt_accum_denoise.hip accum_denoise_lds_bytes)"""
    T, E = 16 + 2 * (r + f), 16 + 2 * f
    return 36 * T * T + 8 * E * E + 128 * E + T * T


def rel_l2(a, ref, max_radiance):
    clamp = lambda p: np.clip(np.nan_to_num(p[..., :3].astype(np.float64), nan=0.0, posinf=max_radiance, neginf=0.0), 0.0, max_radiance)
    a, ref = clamp(a), clamp(ref)
    return float(np.sqrt(((a - ref) ** 2).sum() / (ref ** 2).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160"); ap.add_argument("--reps", type=int, default=9); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", default="16,64"); ap.add_argument("--reference-samples", type=int, default=256)
    ap.add_argument("--scale", type=float, default=1.0); ap.add_argument("--tex", type=int, default=1024); ap.add_argument("--out"); ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    lines = []
    def say(s=""): print(s, flush=True); lines.append(s)
    w, h = (int(v) for v in a.size.split("x")); counts = [int(v) for v in a.samples.split(",")]
    say("reference-mode denoiser on bench.py's scene (bistro-like, scale %g, textures %d^2) at %d x %d: warm, event-timed medians of %d runs after %d" % (a.scale, a.tex, w, h, a.reps, a.warmup))
    for name, kw in SETS:
        P = pt.accum_denoise_default_params(**kw); r, f = int(P["searchRadius"]), int(P["patchRadius"])
        say("  %-20s %3d offsets, %2d patch taps, %6d bytes of LDS a workgroup (%d workgroups a CU by LDS)" % (name, (2 * r + 1) ** 2, (2 * f + 1) ** 2, lds_bytes(r, f), 160 * 1024 // lds_bytes(r, f)))
    if a.rehearse: say("rehearsal: no device, nothing measured"); return
    sc, cam = scenes.bistro_like(scale=a.scale, tex_size=a.tex); S = scenes.default_settings(useFp16Types=1)
    t = pt.PathTracer(); t.set_scene(sc); t.set_settings(S); t.set_camera(scenes.bridge_camera(w, h, **cam)); t.resize(w, h)
    for s in range(0, a.reference_samples, 8): t.render(s, min(8, a.reference_samples - s))      # (a call's samples are one wavefront pool: 8 at a time)
    ref = t.radiance(); t.reset_accumulation()
    mr = float(pt.accum_denoise_default_params()["maxRadiance"])
    for n in counts:
        stats, _ = t.render_adaptive(pt.adaptive_default_params(minSamples=8, step=8, maxSamples=n, threshold=0.0))
        noisy = t.radiance()
        say(); say("%d samples a pixel (%d traced); relative L2 to the %d-sample frame, radiance clamped to %g: noisy %.4f" % (n, stats["samplesTraced"], a.reference_samples, mr, rel_l2(noisy, ref, mr)))
        say("  %-20s %9s %9s %9s %12s %12s" % ("parameters", "ms", "min", "max", "ns / pixel", "relative L2"))
        for name, kw in SETS:
            P = pt.accum_denoise_default_params(**kw); v = []
            for rep in range(a.warmup + a.reps):
                out, ms = t.accum_denoise(P, timed=True)
                if rep >= a.warmup: v.append(ms)
            m = float(np.median(v))
            say("  %-20s %9.3f %9.3f %9.3f %12.3f %12.4f" % (name, m, min(v), max(v), m * 1e6 / (w * h), rel_l2(out, ref, mr)))
        assert np.array_equal(t.radiance().view(np.uint32), noisy.view(np.uint32))      # the radiance buffer is only read
    t.close()
    if a.out:
        with open(a.out, "w") as f: f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
