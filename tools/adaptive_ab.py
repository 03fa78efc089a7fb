"""Adaptive sampling A/B on the scene bench.py builds (C3 at 4K), one MI355X. Usage: python tools/adaptive_ab.py [--rounds 5] [--parent-lib FILE]
[--width 3840 --height 2160 --tex 1024 --scale 1.0] [--thresholds 0.05,0.02,0.01] [--skip-overhead] [--skip-gain].
(a) Overhead: pt_render_adaptive with threshold 0 — nothing retires —, minSamples = step = 8, maxSamples 64, against pt_render of the same 64 samples in eight calls of 8.
    The difference is the error and compaction launches plus the half buffer; errorPassMs per evaluation is printed beside it. With --parent-lib the fixed frame is also
    rendered by another build of the library (alternating processes, MI355PT_LIB), with the frames' SHA-256 compared.
(b) Gain: thresholds 0.05, 0.02 and 0.01 with minSamples 16, step 8, maxSamples 256 against the fixed 256-sample frame (32 calls of 8): frame time, samplesTraced and the
    relative L2 distance of each picture to the fixed frame.
Times are the sums of PtFrameStats.gpuMilliseconds over the calls (HIP events around each frame); every figure is the median of --rounds repeats ((b): half as many, a frame
takes seconds) after one warm-up, in (a) the two modes alternating. One JSON line per section at the end."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _tracer(args):
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    sc, cam = scenes.bistro_like(scale=args.scale, tex_size=args.tex)
    sc["env_cube_dim"] = 2048; sc["env_compression"] = 1
    S = scenes.default_settings(useFp16Types=1); W, H = args.width, args.height
    g = pt.PathTracer(device=0); g.set_scene(sc); g.set_camera(scenes.bridge_camera(W, H, **cam)); g.set_settings(S); g.resize(W, H)
    return g


def _fixed(g, total, step):
    g.reset_accumulation()
    st = [g.render(s, step) for s in range(0, total, step)]
    return sum(s["gpuMilliseconds"] for s in st), sum(int(s["extendRays"]) + int(s["shadowRays"]) for s in st)


def _sha(g):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(g.radiance(), np.float32).tobytes()).hexdigest()


def overhead(args):
    import rtxpt_amd as pt
    g = _tracer(args)
    prm = pt.adaptive_default_params(minSamples=8, step=8, maxSamples=64, threshold=0.0)
    def adaptive():
        st, fs = g.render_adaptive(prm); g.reset_accumulation()
        return fs["gpuMilliseconds"], st["errorPassMs"] / st["evaluations"], int(fs["extendRays"]) + int(fs["shadowRays"])
    _fixed(g, 64, 8); adaptive()
    fx, ad = [], []
    for _ in range(args.rounds):
        fx.append(_fixed(g, 64, 8)); ad.append(adaptive())
    _fixed(g, 64, 8); sha_fixed = _sha(g)
    g.render_adaptive(prm); sha_adaptive = _sha(g); g.close()
    out = dict(section="overhead", fixed_ms=[a for a, _ in fx], adaptive_ms=[a for a, _, _ in ad], error_pass_ms_per_evaluation=[b for _, b, _ in ad],
               rays_fixed=fx[-1][1], rays_adaptive=ad[-1][2], frames_equal=sha_fixed == sha_adaptive, sha256=sha_fixed)
    mf, ma = statistics.median(out["fixed_ms"]), statistics.median(out["adaptive_ms"])
    print("(a) 64 samples in rounds of 8: pt_render %.2f ms (min %.2f max %.2f), pt_render_adaptive at threshold 0 %.2f ms (min %.2f max %.2f): %+.2f ms = %+.2f %%; "
          "errorPassMs per evaluation %.4f ms; rays %d / %d; frames equal: %s" % (mf, min(out["fixed_ms"]), max(out["fixed_ms"]), ma, min(out["adaptive_ms"]), max(out["adaptive_ms"]),
                                                                                 ma - mf, 100.0 * (ma - mf) / mf, statistics.median(out["error_pass_ms_per_evaluation"]),
                                                                                 out["rays_fixed"], out["rays_adaptive"], out["frames_equal"]))
    return out


def gain(args):
    import numpy as np
    import rtxpt_amd as pt
    g = _tracer(args)
    _fixed(g, 16, 8)
    fixed = [_fixed(g, 256, 8)[0] for _ in range(max(1, args.rounds // 2))]
    ref = g.radiance()[..., :3].astype(np.float64); nref = np.linalg.norm(ref)
    out = dict(section="gain", fixed_256_ms=fixed, pixels=args.width * args.height, thresholds={})
    print("(b) fixed 256 samples in calls of 8: %.1f ms (min %.1f max %.1f)" % (statistics.median(fixed), min(fixed), max(fixed)))
    for thr in args.thresholds:
        prm = pt.adaptive_default_params(minSamples=16, step=8, maxSamples=256, threshold=thr)
        runs = []
        for _ in range(max(1, args.rounds // 2)):
            st, fs = g.render_adaptive(prm); runs.append((fs["gpuMilliseconds"], st))
        img = g.radiance()[..., :3].astype(np.float64); g.reset_accumulation()
        st = runs[-1][1]; ms = [a for a, _ in runs]
        r = dict(ms=ms, samplesTraced=st["samplesTraced"], rounds=st["rounds"], evaluations=st["evaluations"], unconvergedPixels=st["unconvergedPixels"], minCount=st["minCount"],
                 maxCount=st["maxCount"], errorPassMs=st["errorPassMs"], rel_l2_to_fixed=float(np.linalg.norm(img - ref) / nref))
        out["thresholds"][str(thr)] = r
        print("    threshold %g: %.1f ms = %.3f of the fixed frame; samplesTraced %d = %.3f of %d x 256 (%.1f a pixel); %d rounds, %d pixels unconverged; counts %d .. %d; "
              "error passes %.2f ms in all; relative L2 to the fixed frame %.5f" % (thr, statistics.median(ms), statistics.median(ms) / statistics.median(fixed), r["samplesTraced"],
                                                                                   r["samplesTraced"] / (256.0 * out["pixels"]), out["pixels"], r["samplesTraced"] / out["pixels"], r["rounds"],
                                                                                   r["unconvergedPixels"], r["minCount"], r["maxCount"], r["errorPassMs"], r["rel_l2_to_fixed"]))
    g.close()
    return out


def parent_child(args):
    """one library per process: the fixed 64-sample frame in calls of 8, `rounds` times"""
    g = _tracer(args)
    _fixed(g, 64, 8)
    ms = [_fixed(g, 64, 8)[0] for _ in range(args.rounds)]
    print(json.dumps(dict(ms=ms, sha256=_sha(g)))); g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--width", type=int, default=3840); ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--tex", type=int, default=1024); ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--parent-lib", default=None); ap.add_argument("--child", default=None, help=argparse.SUPPRESS); ap.add_argument("--skip-gain", action="store_true")
    ap.add_argument("--skip-overhead", action="store_true"); ap.add_argument("--thresholds", type=lambda v: [float(x) for x in v.split(",")], default=[0.05, 0.02, 0.01])
    args = ap.parse_args()
    if args.child is not None:
        parent_child(args); return
    res = [] if args.skip_overhead else [overhead(args)]
    if args.parent_lib and not args.skip_overhead:
        # alternating PROCESSES, parent / new / parent / new: each renders the fixed 64-sample frame with its own library (MI355PT_LIB)
        runs = {"parent": [], "new": []}; sha = {}
        base = [sys.executable, os.path.abspath(__file__), "--child", "1"] + [a for k in ("rounds", "width", "height", "tex", "scale") for a in ("--" + k, str(getattr(args, k)))]
        for rep in range(2):
            for who, lib in (("parent", os.path.abspath(args.parent_lib)), ("new", None)):
                env = dict(os.environ); env.pop("MI355PT_LIB", None)
                if lib: env["MI355PT_LIB"] = lib
                p = subprocess.run(base, capture_output=True, text=True, env=env, timeout=600); p.check_returncode()
                r = json.loads(p.stdout.strip().splitlines()[-1]); runs[who].append(statistics.median(r["ms"])); sha[who] = r["sha256"]
        print("    pt_render of the 64 samples, parent library %s ms, this library %s ms (process medians); frames equal: %s; this - parent %.2f ms, parent's spread %.2f ms"
              % (["%.2f" % x for x in runs["parent"]], ["%.2f" % x for x in runs["new"]], sha["parent"] == sha["new"],
                 statistics.median(runs["new"]) - statistics.median(runs["parent"]), max(runs["parent"]) - min(runs["parent"])))
        res.append(dict(section="parent", runs=runs, frames_equal=sha["parent"] == sha["new"]))
    if not args.skip_gain: res.append(gain(args))
    for r in res: print(json.dumps(r))


if __name__ == "__main__":
    main()
