"""Indirect light (trx_trace_indirect_dev): what one diffuse bounce costs next to the AO visibility pass, and the rate of its
closest-hit launch over diffuse bounce rays.

    python tools/gpu_indirect.py [--rounds 3] [--scenes bistro,hairball] [--out profiles/indirect_pass.log]

The bistro-class and hairball-class 1080p frames, semantics TRX_SEM_CPU, 4 bounce samples, one point light a quarter of the
scene's height above the camera (tools/gpu_light.py's).  Per round a fresh child process (the protocol of
tools/gpu_ao_visibility.py: one process's pass time depends on where its scene landed in memory) builds the scene, runs
bench.py's wake frames (140 primary frames), and times in batches of back-to-back launches (one hipEvent pair per batch):
  vis4       trx_trace_ao_visibility_dev, 4 samples, radius +inf: the reference pass, timed first and last.  The change that
             added the indirect pass does not touch its kernels (their instructions are the parent commit's), so its numbers
             are the parent's and their spread over the rounds is the margin everything else is read against.
  gi4        trx_trace_indirect_dev, 4 samples, the point light, no base.
and splits the pass with hipEvents between its launches (trx_debug_indirect_phases; median of 9 passes) into bounce rays /
closest-hit walk / attributes / shadow rays / any-hit walk / weight, gather and finish.  From the building blocks of one
sample it reports the share of the bounce rays that hit, and from the closest-hit walk's time the Mrays/s of that launch over
the bounce rays actually cast (surface pixels x samples; the inert rays of the other pixels are dealt and dropped at once).
Printed and written to --out: per form the median over rounds of each child's median with the spread over rounds."""
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(scenes):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import tray_racing_amd as T
    from tray_racing_amd import _lib as L
    lib = L.load()
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
        prim = torch.zeros(w * h, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(w * h, dtype=torch.uint8, device="cuda")
        val = torch.zeros(w * h, dtype=torch.float32, device="cuda")
        for _ in range(140):   # the wake frames
            sc.trace_primary_dev(view, w, h, prim.data_ptr(), sem=sem)
        torch.cuda.synchronize()

        def batches(fn, n_batches=6, per=4, warm=8):
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

        def vis4(i):
            sc.trace_ao_visibility_dev(view, w, h, prim.data_ptr(), cnt.data_ptr(), n, float("inf"), sem=sem, frame0=n * i, ao_eps=eps)

        def gi4(i):
            sc.trace_indirect_dev(view, w, h, point, prim.data_ptr(), val.data_ptr(), n_samples=n, sem=sem, frame0=n * i, bounce_eps=eps,
                                  shadow_eps=eps, bounce_albedo=0.5)

        def phases():
            rows = []
            for i in range(9):
                ms = (C.c_float * 6)()
                L.check(lib.trx_debug_indirect_phases(sc.handle, C.byref(view), w, h, sem, 0, point, 1, n * i, n, eps, eps, 0.5,
                                                      C.c_void_p(prim.data_ptr()), None, None, C.c_void_p(val.data_ptr()), ms))
                rows.append(list(ms))
            return [statistics.median(x[k] for x in rows) for k in range(6)]

        def bounce_shares():
            """(surface share of the pixels, share of the surface pixels' bounce rays that hit) for seed 0, from the building blocks."""
            rays = torch.zeros(w * h * 8, dtype=torch.float32, device="cuda")
            hits = torch.zeros(w * h * 2, dtype=torch.float32, device="cuda")
            sc.ao_rays_dev(view, w, h, prim.data_ptr(), rays.data_ptr(), float("inf"), frame=0, ao_eps=eps)
            sc.trace_rays_dev(rays.data_ptr(), w * h, hits.data_ptr(), sem=sem)
            torch.cuda.synchronize()
            cast = ~(rays.view(-1, 8)[:, 7] < 0)
            hit = cast & (hits.view(-1, 2)[:, 0] < 3.0e38)
            return float(cast.float().mean().item()), float(hit.float().sum().item() / max(cast.float().sum().item(), 1.0))

        res = {}
        res["vis4"] = batches(vis4)
        res["gi4"] = batches(gi4)
        v = val.cpu().numpy()
        res["lit_share"] = float((v > 0).mean())
        res["phases"] = phases()
        res["surface"], res["bounce_hit"] = bounce_shares()
        res["vis4_again"] = batches(vis4)
        res["bounce_mrays"] = res["surface"] * w * h * n / (res["phases"][1] * 1e-3) / 1e6
        sc.check()
        out[name] = res
        sc.close()
    print("INDIRECT_CHILD " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1].split(","))
    rounds, scenes, path = 3, "bistro,hairball", os.path.join(ROOT, "profiles", "indirect_pass.log")
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
        line = [x for x in p.stdout.splitlines() if x.startswith("INDIRECT_CHILD ")]
        if p.returncode or not line:
            print("child failed (exit %d): %s" % (p.returncode, p.stderr[-600:]), flush=True)
            return 1
        res.append(json.loads(line[0][15:]))
        say("round %d " % r + json.dumps(res[-1]))
    say("\n%sx%s, TRX_SEM_CPU, 4 samples, one point light: median over %d processes [min .. max] of each process's median (ms per pass)"
        % (os.environ.get("W", "1920"), os.environ.get("H", "1080"), rounds))
    names = ("bounce rays", "closest-hit walk", "attributes", "shadow rays", "any-hit walk", "weight + gather")
    for s in scenes.split(","):
        med = {}
        for key in ("vis4", "vis4_again", "gi4", "bounce_mrays"):
            v = [x[s][key] for x in res]
            med[key] = statistics.median(v)
            say("%-9s %-12s %.4f [%.4f .. %.4f]" % (s, key, med[key], min(v), max(v)))
        ref = [x[s][k] for x in res for k in ("vis4", "vis4_again")]
        base = statistics.median(ref)
        say("%-9s AO visibility at 4 samples over all its runs: %.4f [%.4f .. %.4f], spread %.1f %% of the median" %
            (s, base, min(ref), max(ref), 100 * (max(ref) - min(ref)) / base))
        say("%-9s indirect pass / AO visibility: %.3f" % (s, med["gi4"] / base))
        ph = [statistics.median(x[s]["phases"][k] for x in res) for k in range(6)]
        say("%-9s split: %s  (sum %.4f ms)" % (s, "  ".join("%s %.4f" % (names[k], ph[k]) for k in range(6)), sum(ph)))
        say("%-9s surface pixels %.1f %%; bounce rays that hit %.1f %% of those cast; closest-hit launch over the cast bounce rays %.0f Mrays/s; "
            "pixels the bounce lights %.1f %%" % (s, 100 * res[0][s]["surface"], 100 * res[0][s]["bounce_hit"], med["bounce_mrays"], 100 * res[0][s]["lit_share"]))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
