"""The value filter (trx_value_filter_dev): what its levels cost next to the AO filter and next to the indirect pass whose term it
filters.

    python tools/gpu_value_filter.py [--rounds 3] [--scenes bistro,hairball] [--out profiles/value_filter.log]

The bistro-class and hairball-class 1080p frames, semantics TRX_SEM_CPU, the 4-sample indirect term of one point light a
quarter of the scene's height above the camera (tools/gpu_indirect.py's), depth tolerance 0.1, cosine 0.9, with normals.  Per
round a fresh child process (the protocol of tools/gpu_ao_visibility.py) builds the scene, runs bench.py's wake frames (140
primary frames), and times in batches of back-to-back calls (one hipEvent pair per batch):
  ao_r2      trx_ao_filter_dev at radius 2 with normals: the same 25 taps out of LDS, and a kernel this change does not touch
             (its instructions are the parent commit's) - timed first and last, the spread of its runs is the margin.
  gi4        trx_trace_indirect_dev, 4 samples, no base: the pass whose term is filtered.
  pass1..5   trx_value_filter_dev with 1..5 levels, the base in d_out.
The prototype names no first level, so level L alone is not a call: its time is pass L minus pass L-1 (level 1 is pass 1).  A
level's distinct bytes are 16 per pixel (the hit record, the value read, the value written) and 24 per surface pixel (the
attribute record): effective GB/s = those bytes over the level's time.
Printed and written to --out: per form the median over rounds of each child's median with the spread over rounds."""
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, COS = 0.1, 0.9


def child(scenes):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import tray_racing_amd as T
    w, h = int(os.environ.get("W", "1920")), int(os.environ.get("H", "1080"))
    sem, n, eps = T.SEM_CPU, 4, 0.01
    out = {}
    for name in scenes:
        verts, counts = T.gen_scene(name, 0, 1)
        flat = T.flat_build(verts, counts)
        eye, look, fov = T.scene_camera(name)
        view = T.view_from_camera(eye, look, fov, w, h)
        pts = flat.tri_verts.reshape(-1, 3)
        lo, hi = pts.min(0), pts.max(0)
        above = np.array(eye, dtype=np.float64) + np.array([0.0, 0.25 * (hi[1] - lo[1]), 0.0])
        point = T.light_array([T.light(T.LIGHT_POINT, above.tolist())])
        sc = T.Scene(flat)
        px = w * h
        prim = torch.zeros(px, dtype=torch.int64, device="cuda")
        attr = torch.zeros(px * 6, dtype=torch.float32, device="cuda")
        cnt = torch.zeros(px, dtype=torch.uint8, device="cuda")
        term = torch.zeros(px, dtype=torch.int32, device="cuda")
        val, work, outp = (torch.zeros(px, dtype=torch.float32, device="cuda") for _ in range(3))
        for _ in range(140):   # the wake frames
            sc.trace_primary_dev(view, w, h, prim.data_ptr(), sem=sem)
        sc.hit_attributes_primary_dev(view, w, h, prim.data_ptr(), attr.data_ptr())
        sc.trace_ao_visibility_dev(view, w, h, prim.data_ptr(), cnt.data_ptr(), n, float("inf"), sem=sem, ao_eps=eps)
        sc.trace_indirect_dev(view, w, h, point, prim.data_ptr(), val.data_ptr(), n_samples=n, sem=sem, bounce_eps=eps, shadow_eps=eps, bounce_albedo=0.5)
        torch.cuda.synchronize()

        def batches(fn, n_batches=6, per=8, warm=8):
            for i in range(warm):
                fn(i)
            ts = []
            for b in range(n_batches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(per):
                    fn(b * per + i)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) / per)
            return statistics.median(ts)

        def ao_r2(i):
            sc.ao_filter_dev(w, h, prim.data_ptr(), cnt.data_ptr(), term.data_ptr(), n, 2, depth_tol=TOL, normal_cos=COS, d_attr=attr.data_ptr())

        def gi4(i):
            sc.trace_indirect_dev(view, w, h, point, prim.data_ptr(), work.data_ptr(), n_samples=n, sem=sem, frame0=n * i, bounce_eps=eps,
                                  shadow_eps=eps, bounce_albedo=0.5)

        def filt(levels):
            def fn(i):
                sc.value_filter_dev(w, h, prim.data_ptr(), val.data_ptr(), outp.data_ptr(), levels, depth_tol=TOL, normal_cos=COS,
                                    d_attr=attr.data_ptr(), d_base=outp.data_ptr(), d_work=work.data_ptr())
            return fn

        res = {"ao_r2": batches(ao_r2)}
        for levels in range(1, 6):
            res["pass%d" % levels] = batches(filt(levels))
        res["gi4"] = batches(gi4, per=4)
        res["ao_r2_again"] = batches(ao_r2)
        res["surface"] = float((prim.view(torch.float32).view(-1, 2)[:, 0] < 3.0e38).float().mean().item())
        sc.check()
        out[name] = res
        sc.close()
    print("VALUE_FILTER_CHILD " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1].split(","))
    rounds, scenes, path = 3, "bistro,hairball", os.path.join(ROOT, "profiles", "value_filter.log")
    while args and args[0].startswith("--"):
        if args[0] == "--rounds":
            rounds = int(args[1])
        elif args[0] == "--scenes":
            scenes = args[1]
        elif args[0] == "--out":
            path = args[1]
        args = args[2:]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with open(os.path.join(ROOT, "tray_racing_amd", "libtrx.so"), "rb") as f:
        say("library %s" % hashlib.sha256(f.read()).hexdigest()[:16])
    res = []
    for r in range(rounds):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scenes], capture_output=True, text=True, timeout=900)
        line = [x for x in p.stdout.splitlines() if x.startswith("VALUE_FILTER_CHILD ")]
        if p.returncode or not line:
            print("child failed (exit %d): %s" % (p.returncode, p.stderr[-600:]), flush=True)
            return 1
        res.append(json.loads(line[0][len("VALUE_FILTER_CHILD "):]))
        say("round %d " % r + json.dumps(res[-1]))
    w, h = int(os.environ.get("W", "1920")), int(os.environ.get("H", "1080"))
    say("\n%dx%d, TRX_SEM_CPU, depth tolerance %g, cosine %g, with normals: median over %d processes [min .. max] of each process's median (ms)"
        % (w, h, TOL, COS, rounds))
    for s in scenes.split(","):
        med = {}
        for key in ["ao_r2", "ao_r2_again", "gi4"] + ["pass%d" % k for k in range(1, 6)]:
            v = [x[s][key] for x in res]
            med[key] = statistics.median(v)
            say("%-9s %-12s %.4f [%.4f .. %.4f]" % (s, key, med[key], min(v), max(v)))
        ref = [x[s][k] for x in res for k in ("ao_r2", "ao_r2_again")]
        base = statistics.median(ref)
        say("%-9s AO filter at radius 2 over all its runs: %.4f [%.4f .. %.4f], spread %.1f %% of the median" %
            (s, base, min(ref), max(ref), 100 * (max(ref) - min(ref)) / base))
        surface = res[0][s]["surface"]
        bytes_level = w * h * (16 + 24 * surface)
        prev = 0.0
        for k in range(1, 6):
            t = med["pass%d" % k] - prev
            prev = med["pass%d" % k]
            say("%-9s level %d (spacing %2d): %.4f ms, x %.2f of the AO filter at radius 2, %.0f GB/s of distinct bytes" %
                (s, k, 1 << (k - 1), t, t / base, bytes_level / (t * 1e-3) / 1e9 if t > 0 else float("nan")))
        say("%-9s surface pixels %.1f %%; 3-level pass %.4f ms, 5-level pass %.4f ms; indirect pass at 4 samples %.4f ms: the 3-level pass is %.1f %% of it" %
            (s, 100 * surface, med["pass3"], med["pass5"], med["gi4"], 100 * med["pass3"] / med["gi4"]))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
