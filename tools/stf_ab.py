"""Stochastic texture filtering A/B on the scene bench.py builds (C3: 4K, 4 spp, 8 bounces): the filter off, LINEAR and POINT, alternating in one process after a warm-up.
Prints per mode the median frame time, the median k_shade stream time (PtFrameStats.shadeKernelMs of serial-kernel frames) and the ray counts of a frame. Usage: python tools/stf_ab.py [--rounds 5]
[--width 3840 --height 2160 --spp 4 --tex 1024 --scale 1.0]. With --parent-lib FILE it also alternates bench frames of another build of the library with this one's
(filter off in both), the two frames' SHA-256 compared: the "feature off is no slower, and computes the same" measurement."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import json

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def frames(args, modes):
    import numpy as np
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    sc, cam = scenes.bistro_like(scale=args.scale, tex_size=args.tex)
    sc["env_cube_dim"] = 2048; sc["env_compression"] = 1
    S = scenes.default_settings(useFp16Types=1); W, H = args.width, args.height
    g = pt.PathTracer(device=0); g.set_scene(sc); g.set_camera(scenes.bridge_camera(W, H, **cam)); g.set_settings(S); g.resize(W, H)
    def frame(mode):
        if hasattr(g, "set_texture_filtering") and mode is not None: g.set_texture_filtering(mode >= 0, max(mode, 0))
        g.reset_accumulation()
        return g.render(0, args.spp)
    for m in modes: frame(m)                                  # warm-up: every mode's kernels loaded, the scene prepared
    res = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes: res[m].append(frame(m))
    # k_shade's stream time: PtFrameStats.shadeKernelMs is filled in serial-kernel frames (one batch, one stream, launches never overlap), so a second set of rounds runs that way
    g.set_serial_kernels(True); serial = {m: [] for m in modes}
    for m in modes: frame(m)
    for _ in range(args.rounds):
        for m in modes: serial[m].append(frame(m))
    g.set_serial_kernels(False)
    out = {}
    for m in modes:
        frame(m); sha = hashlib.sha256(np.ascontiguousarray(g.radiance(), np.float32).tobytes()).hexdigest()
        out[str(m)] = dict(frame_ms=[s["gpuMilliseconds"] for s in res[m]], shade_ms=[s["shadeKernelMs"] for s in serial[m]], serial_frame_ms=[s["gpuMilliseconds"] for s in serial[m]],
                           extendRays=int(res[m][-1]["extendRays"]), shadowRays=int(res[m][-1]["shadowRays"]), hits=int(res[m][-1]["hits"]), sha256=sha)
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--width", type=int, default=3840); ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--spp", type=int, default=4); ap.add_argument("--tex", type=int, default=1024); ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--parent-lib", default=None); ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:                                # one library per process: frames of the filter-off mode only
        print(json.dumps(frames(args, [None]))); return
    names = {"-1": "off", "1": "LINEAR", "0": "POINT"}
    out = frames(args, [-1, 1, 0])
    for m, r in out.items():
        print("%-7s frame %8.3f ms (min %8.3f max %8.3f)  serial-kernel frame %8.3f ms of which k_shade %8.3f ms  extend %d shadow %d hits %d  sha256 %s" % (
            names[m], statistics.median(r["frame_ms"]), min(r["frame_ms"]), max(r["frame_ms"]), statistics.median(r["serial_frame_ms"]), statistics.median(r["shade_ms"]), r["extendRays"], r["shadowRays"], r["hits"], r["sha256"][:16]))
    if args.parent_lib:
        # alternating PROCESSES, parent / new / parent / new: each renders `rounds` filter-off frames with its own library (MI355PT_LIB)
        runs = {"parent": [], "new": []}; sha = {}
        base = [sys.executable, os.path.abspath(__file__), "--child", "1"] + [a for k in ("rounds", "width", "height", "spp", "tex", "scale") for a in ("--" + k, str(getattr(args, k)))]
        for rep in range(3):
            for who, lib in (("parent", os.path.abspath(args.parent_lib)), ("new", None)):
                env = dict(os.environ); env.pop("MI355PT_LIB", None)
                if lib: env["MI355PT_LIB"] = lib
                p = subprocess.run(base, capture_output=True, text=True, env=env, timeout=900); p.check_returncode()
                r = json.loads(p.stdout.strip().splitlines()[-1])["None"]; runs[who].append(statistics.median(r["frame_ms"])); sha[who] = r["sha256"]
        for who in ("parent", "new"):
            print("%-7s filter off: median frame %8.3f ms of process medians %s  sha256 %s" % (who, statistics.median(runs[who]), ["%.3f" % x for x in runs[who]], sha[who][:16]))
        print("frames equal: %s; parent run-to-run spread %.3f ms; new - parent %.3f ms" % (sha["parent"] == sha["new"], max(runs["parent"]) - min(runs["parent"]), statistics.median(runs["new"]) - statistics.median(runs["parent"])))


if __name__ == "__main__":
    main()
