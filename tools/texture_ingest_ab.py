#!/usr/bin/env python3
"""Texture ingest, host path against device path (PT_DEVICE_TEXTURES_ON_DEVICE; docs/WIDENING.md N10). A tool, not a test.

Two texture sets: C3's own 32 x 1024^2 (rtxpt_amd/scenes.py) and a seeded 64 x 2048^2 sRGB + 16 x 2048^2 RGBA32F, on one quad each (the geometry costs nothing: what is
timed is the textures). One process per (set, mode), the modes alternating; in each, three warm contexts and five timed ones. Per context: the host time from
pt_set_materials to the end of the first prepare() (set_scene, then one traced ray), and pt_get_texture_ingest_stats; per process: the peak resident set; per timed context
of the second set: one pt_update_texture of a 2048^2 sRGB texture up to the end of the next prepare(), which on the host path is what a full reload costs as well — the
parent's only way to change a texture was pt_set_materials for all of them, the first number of the same line.

    python tools/texture_ingest_ab.py [--out profiles/r08a_texture_ingest.txt] [--sets c3,2k] [--warm 3] [--timed 5]
"""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_set(name):
    from rtxpt_amd import scenes
    b = scenes.SceneBuilder()
    if name == "c3":
        scenes._make_textures(np.random.default_rng(scenes.SEED_BASE + 3), b, 1024)
    else:
        r = np.random.default_rng(20260817)
        srgb = r.integers(0, 256, (2048, 2048, 4), dtype=np.uint8)
        f32 = np.exp(r.standard_normal((2048, 2048, 4), dtype=np.float32)); f32[..., 3] = r.random((2048, 2048), dtype=np.float32)
        for k in range(64): b.add_texture(np.roll(srgb, 37 * k, axis=1), scenes.TEX_RGBA8_SRGB)          # distinct textures of one seeded image: 2 GB of noise would only time numpy
        for k in range(16): b.add_texture(np.roll(f32, 53 * k, axis=0), scenes.TEX_RGBA32F)
    m = b.add_material(scenes.make_material())
    p, i, uv, n, tg = scenes.quad([0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0])
    b.begin_mesh(); b.add_geometry(p, i, m, uv=uv, normal=n, tangent=tg); b.add_instance(b.end_mesh())
    return b.finish()


def child(name, mode, warm, timed):
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    sc = build_set(name)
    ray = np.float32([[0.5, 0.5, -1, 0, 0, 0, 1, 1e9]])
    update = np.roll(np.ascontiguousarray(sc["textures"][0][3]), 11, axis=0) if name == "2k" else None
    runs = []
    for k in range(warm + timed):
        g = pt.PathTracer(device_textures=(mode == "device"))
        g.set_settings(scenes.default_settings())
        t0 = time.perf_counter(); g.set_scene(sc); g.trace_visibility(ray); t1 = time.perf_counter()
        row = dict(loadMs=1e3 * (t1 - t0), stats=g.texture_ingest_stats())
        if update is not None:
            t0 = time.perf_counter(); g.update_texture(0, update); g.trace_visibility(ray); t1 = time.perf_counter()
            row["updateMs"] = 1e3 * (t1 - t0); row["updateStats"] = g.texture_ingest_stats()
        g.close()
        if k >= warm: runs.append(row)
    print("RESULT " + json.dumps(dict(set=name, mode=mode, runs=runs, peakRssMB=resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("SET", "MODE")); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08a_texture_ingest.txt"))
    ap.add_argument("--sets", default="c3,2k"); ap.add_argument("--warm", type=int, default=3); ap.add_argument("--timed", type=int, default=5)
    a = ap.parse_args()
    if a.child: return child(a.child[0], a.child[1], a.warm, a.timed)
    env = dict(os.environ); env.pop("MI355PT_DEVICE_TEXTURES", None)
    lines = ["texture ingest, host path against device path: %d warm + %d timed contexts per process, one process per (set, mode)" % (a.warm, a.timed),
             "loadMs: pt_set_materials .. end of the first prepare(); updateMs: pt_update_texture of one 2048^2 sRGB texture .. end of the next prepare()", ""]
    for name in a.sets.split(","):
        res = {}
        for mode in ("host", "device"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, mode, "--warm", str(a.warm), "--timed", str(a.timed)], capture_output=True, text=True, env=env)
            out = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not out: raise SystemExit("child %s %s failed:\n%s\n%s" % (name, mode, r.stdout[-2000:], r.stderr[-4000:]))
            res[mode] = json.loads(out[-1][7:])
            print("%s %s: done" % (name, mode), flush=True)
        lines.append("set %s: %s" % (name, "32 x 1024^2 (C3)" if name == "c3" else "64 x 2048^2 sRGB + 16 x 2048^2 RGBA32F"))
        for mode in ("host", "device"):
            d = res[mode]; load = sorted(x["loadMs"] for x in d["runs"]); s = d["runs"][-1]["stats"]
            lines.append("  %-6s loadMs median %.1f (min %.1f max %.1f)  peak RSS %.0f MB  hostBytesHeld %.1f MB  sourceBytes %.1f MB  poolTexels %d" % (
                mode, load[len(load) // 2], load[0], load[-1], d["peakRssMB"], s["hostBytesHeld"] / 2 ** 20, s["sourceBytes"] / 2 ** 20, s["poolTexels"]))
            lines.append("         stats: launches %d stagingChunks %d uploadMs %.2f level0Ms %.2f mipMs %.2f alphaMs %.2f totalMs %.2f" % (
                s["launches"], s["stagingChunks"], s["uploadMs"], s["level0Ms"], s["mipMs"], s["alphaMs"], s["totalMs"]))
            if "updateMs" in d["runs"][-1]:
                up = sorted(x["updateMs"] for x in d["runs"]); u = d["runs"][-1]["updateStats"]
                lines.append("         updateMs median %.2f (min %.2f max %.2f); the update alone: totalMs %.2f launches %d" % (up[len(up) // 2], up[0], up[-1], u["totalMs"], u["launches"]))
        h = sorted(x["loadMs"] for x in res["host"]["runs"]); d = sorted(x["loadMs"] for x in res["device"]["runs"])
        lines.append("  device / host: load %.3f, peak RSS %.3f" % (d[len(d) // 2] / h[len(h) // 2], res["device"]["peakRssMB"] / res["host"]["peakRssMB"]))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f: f.write(text + "\n")


if __name__ == "__main__":
    main()
