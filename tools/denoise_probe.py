"""Times the device denoiser's passes (pt_denoise_plane: temporal, history clamp, a-trous iterations) on realtime frames of bench.py's scene at 3840 x 2160 and 1920 x 1080.

Per pass: the median of warm, event-timed runs (pt_denoise_pass_times) of every plane, summed over the frame's planes; the pass's algorithmic bytes (what it must read and write
once, from the buffer layouts below, for the pixels of the planes that have a surface) and the rate and share of the HBM peak that gives. Beside it the project's own streaming
kernel, k_accumulate, in the same run: its kernel time comes from a child process under `rocprofv3 --kernel-trace` (a serial-kernel pt_render of one sample per size), its bytes from
its text (owned-pixel index 4 + path radiance 16 + accumulation buffer 16 read, 16 written). Writes the report to stdout; --out also to a file (profiles/denoiser_passes.txt).

  python tools/denoise_probe.py --out profiles/denoiser_passes.txt              (on the GPU)
  python tools/denoise_probe.py --rehearse                                      (no GPU: argument parsing, scene, byte counts)"""
import argparse, csv, glob, json, os, shutil, signal, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12      # bytes / s (MI355X)
# algorithmic bytes per surface pixel of a plane
TEMPORAL_BYTES = (4 + 8 + 16 + 16 + 16 + 1) + 5 * 16 + 5 * 16 + 16      # the prepare pass's buffers; the previous history; the new history; the guide record
CLAMP_BYTES = 16 + 2 * 16 + 2 * 16 + 16 + 1 + 2 * 16 + 2 * 16            # guide, fast histories, accumulated radiance, moments, relax; first a-trous input; the clamped history written back
ATROUS_BYTES = 16 + 2 * 16 + 2 * 16                                     # guide, radiance + variance pair in, pair out
ACCUMULATE_BYTES = 4 + 16 + 16 + 16                                      # k_accumulate at one sample per pixel


def sizes_of(text): return [tuple(int(v) for v in s.split("x")) for s in text.split(",")]


def scene(a):
    from rtxpt_amd import scenes
    sc, cam = scenes.bistro_like(scale=a.scale, tex_size=a.tex)
    return sc, cam, scenes.default_settings(useFp16Types=1)


def accumulate_child(a):
    """under rocprofv3: per size, `frames` serial-kernel renders of one sample (one k_accumulate dispatch each, in order)"""
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    sc, cam, S = scene(a)
    t = pt.PathTracer(serial_kernels=True); t.set_scene(sc); t.set_settings(S)
    for w, h in sizes_of(a.sizes):
        t.set_camera(scenes.bridge_camera(w, h, **cam)); t.resize(w, h)
        for f in range(a.accumulate_frames): t.render(f, 1)
    t.close()


class ChildFailed(RuntimeError): pass


def accumulate_times(a, trace_dir):
    """{(w, h): median kernel milliseconds of k_accumulate} from a child under rocprofv3 --kernel-trace. The child runs in a process group of its own; on a time-out the whole
    group is killed (rocprofv3 and the python under it, which holds the GPU). A child that timed out or ended with any non-zero status raises ChildFailed: the caller starts
    nothing more on that GPU."""
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "-o", "accumulate", "--", sys.executable, os.path.abspath(__file__), "--accumulate-child",
           "--sizes", a.sizes, "--scale", str(a.scale), "--tex", str(a.tex), "--accumulate-frames", str(a.accumulate_frames)]
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try: out, _ = p.communicate(timeout=a.child_timeout)
    except subprocess.TimeoutExpired:
        try: os.killpg(p.pid, signal.SIGKILL)
        except ProcessLookupError: pass
        p.communicate()
        raise ChildFailed("the traced child did not finish in %d s and was killed with its process group" % a.child_timeout)
    if p.returncode != 0: raise ChildFailed("the traced child ended with status %d:\n%s" % (p.returncode, out[-2000:]))
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "k_accumulate" in row.get("Kernel_Name", ""): rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    rows.sort(); sizes = sizes_of(a.sizes)
    if len(rows) != len(sizes) * a.accumulate_frames: return "not measured (%d k_accumulate dispatches in the trace, %d expected)" % (len(rows), len(sizes) * a.accumulate_frames)
    out = {}
    for i, s in enumerate(sizes):
        ms = [(e - b) * 1e-6 for b, e in rows[i * a.accumulate_frames:(i + 1) * a.accumulate_frames]]
        out[s] = float(np.median(ms[1:]))      # (the first dispatch of a size is the cold one)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3840x2160,1920x1080"); ap.add_argument("--reps", type=int, default=9); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0); ap.add_argument("--tex", type=int, default=1024); ap.add_argument("--out"); ap.add_argument("--trace-dir", help="where the traced child's rocprofv3 output goes (default: a fresh temporary directory)")
    ap.add_argument("--accumulate-frames", type=int, default=4); ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--accumulate-child", action="store_true"); ap.add_argument("--no-accumulate", action="store_true"); ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.accumulate_child: return accumulate_child(a)
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    import denoiser_inputs_ref as ref
    lines = []
    def say(s=""): print(s, flush=True); lines.append(s)
    sc, cam, S = scene(a)
    say("device denoiser passes on bench.py's scene (bistro-like, scale %g, textures %d^2): warm, event-timed medians of %d runs after %d; bytes are algorithmic" % (a.scale, a.tex, a.reps, a.warmup))
    say("bytes per surface pixel of a plane: temporal %d, history clamp %d, a-trous iteration %d (+4 in the last); k_accumulate %d per pixel; HBM peak %.1f TB/s" %
        (TEMPORAL_BYTES, CLAMP_BYTES, ATROUS_BYTES, ACCUMULATE_BYTES, HBM_PEAK * 1e-12))
    if a.rehearse: say("rehearsal: no device, nothing measured"); return
    acc = "not measured (--no-accumulate)"
    if not a.no_accumulate:
        trace_dir = a.trace_dir or tempfile.mkdtemp(prefix="denoise_probe_trace_")
        try: acc = accumulate_times(a, trace_dir)
        except ChildFailed as e:      # a failed or hung GPU process: nothing more is started on that GPU (--no-accumulate skips the comparison on purpose)
            print("denoise_probe: %s\nstopping before any further GPU work" % e, file=sys.stderr, flush=True); sys.exit(3)
        finally:
            if not a.trace_dir: shutil.rmtree(trace_dir, ignore_errors=True)
    t = pt.PathTracer(); t.set_scene(sc); t.set_settings(S)
    ds = pt.denoise_default_settings(); n_it = int(ds["atrousIterationNum"])
    names = ["temporal", "history clamp"] + ["a-trous step %d (%s)" % (1 << i, "LDS" if i < 2 else "global") for i in range(n_it)]
    for w, h in sizes_of(a.sizes):
        camd = scenes.bridge_camera(w, h, **cam); t.set_camera(camd); t.resize(w, h)
        prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam), sub_samples=1)
        t.realtime_frame(0, prm); t.denoise_spec_hit_t()
        dn = ref.case_params(camd)
        active = int(prm["activeStablePlaneCount"])
        surf = {}; t.denoise_pass_times(True)
        runs = {p: [] for p in range(active)}
        for rep in range(a.warmup + a.reps):
            for i, p in enumerate(range(active - 1, -1, -1)):
                t.denoiser_prepare_nrd(prm, dn, p, i == 0)
                if rep == 0: surf[p] = int((t.get_denoiser_inputs(("nrd_view_z",))["nrd_view_z"] != ref.FLT_MAX).sum())
                t.denoise_plane(prm, ds, p, rep == 0)
                if rep >= a.warmup: runs[p].append(t.denoise_pass_times(True))
        med = {p: np.median(np.stack(runs[p]), axis=0) for p in runs}
        N = w * h
        say(); say("%d x %d, %d planes, surface pixels per plane %s of %d" % (w, h, active, [surf[p] for p in range(active)], N))
        if isinstance(acc, dict):
            acc_rate = ACCUMULATE_BYTES * N / (acc[(w, h)] * 1e-3)
            say("  k_accumulate (1 sample, rocprofv3 kernel trace): %.3f ms, %.0f GB/s = %.1f %% of the HBM peak" % (acc[(w, h)], acc_rate * 1e-9, 100 * acc_rate / HBM_PEAK))
            say("    (warm repeats over the same %.0f MB, which the last-level cache can hold in part: an upper figure for a streaming kernel, not an HBM-only rate)" % (ACCUMULATE_BYTES * N * 1e-6))
        else: say("  k_accumulate: %s" % acc)
        say("  %-28s %9s %10s %9s %8s %s" % ("pass (all planes)", "ms", "MB", "GB/s", "% peak", "x k_accumulate's share" if isinstance(acc, dict) else ""))
        total = 0.0
        for k, name in enumerate(names):
            per = TEMPORAL_BYTES if k == 0 else CLAMP_BYTES if k == 1 else ATROUS_BYTES + (4 if k == len(names) - 1 else 0)
            ms = float(sum(med[p][k] for p in med)); by = float(sum(per * surf[p] for p in med)); rate = by / (ms * 1e-3); total += ms
            say("  %-28s %9.3f %10.1f %9.0f %8.1f %s" % (name, ms, by * 1e-6, rate * 1e-9, 100 * rate / HBM_PEAK, "%.2f" % (rate / acc_rate) if isinstance(acc, dict) else ""))
        say("  %-28s %9.3f   (per plane: %s)" % ("denoiser, whole frame", total, ", ".join("plane %d %.3f" % (p, float(med[p].sum())) for p in sorted(med))))
    t.close()
    if a.out:
        with open(a.out, "w") as f: f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
