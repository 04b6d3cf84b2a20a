"""AO visibility (trx_trace_ao_visibility_dev): what the any-hit pass costs next to the closest-hit AO batch over the same rays.

    python tools/gpu_ao_visibility.py [--rounds 3] [--scenes bistro,hairball] [--out profiles/ao_visibility.log]

The bistro-class and hairball-class 1080p frames, semantics TRX_SEM_CPU, 4 samples per pixel.  Per round a fresh child
process (as tools/gpu_ab_procs.py does: one process's pass time depends on where its scene landed in memory) builds the
scene, runs bench.py's wake frames (140 primary frames), and times in batches of back-to-back launches (one hipEvent pair
per batch):
  ao4        trx_trace_ao_batch_dev, 4 seeds: the closest-hit AO pass to infinity, 4 x 8 B records per pixel.  This pull
             request does not touch it (the traversal kernels' instructions are the parent commit's), so its numbers are the
             parent's, and their spread over the rounds is the margin the comparison is read against.
  vis4_inf   trx_trace_ao_visibility_dev, 4 samples, radius +inf: the same rays, any-hit, one byte per pixel.
  vis4_r     the same at a finite radius: the tests' radius scaled to the scene (1.4 on the Cornell-class box of diagonal
             3.46: 0.404 x the scene's diagonal).
and splits one visibility pass into ray generation / any-hit walk / reduce with hipEvents between the launches
(trx_debug_ao_visibility_phases; median of 9 passes).  Printed and written to --out: per form the median over rounds of each
child's median batch (ms per pass) with the spread over rounds, the split, and what the counts say (mean unoccluded
share of the surface pixels)."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 1.4 / 3.4641016


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
        radius = SCALE * float(np.linalg.norm(pts.max(0) - pts.min(0)))
        sc = T.Scene(flat)
        prim = torch.zeros(w * h, dtype=torch.int64, device="cuda")
        ao4 = torch.zeros(n * w * h, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(w * h, dtype=torch.uint8, device="cuda")
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

        def share():
            c = cnt.cpu().numpy()
            surf = c[c != L.AO_NO_SURFACE]
            return float(surf.mean() / n) if surf.size else 0.0, float((c != L.AO_NO_SURFACE).mean())

        def phases(r):
            rows = []
            for i in range(9):
                ms = (C.c_float * 3)()
                L.check(lib.trx_debug_ao_visibility_phases(sc.handle, C.byref(view), w, h, sem, n * i, n, eps, r,
                                                           C.c_void_p(prim.data_ptr()), None, C.c_void_p(cnt.data_ptr()), ms))
                rows.append(list(ms))
            return [statistics.median(x[k] for x in rows) for k in range(3)]

        res = {"radius": radius}
        res["ao4"] = batches(lambda i: sc.trace_ao_batch_dev(view, w, h, prim.data_ptr(), ao4.data_ptr(), w * h, n, sem=sem,
                                                             frame0=n * i, ao_eps=eps))
        res["vis4_inf"] = batches(lambda i: sc.trace_ao_visibility_dev(view, w, h, prim.data_ptr(), cnt.data_ptr(), n, float("inf"),
                                                                       sem=sem, frame0=n * i, ao_eps=eps))
        res["open_inf"], res["surface"] = share()
        res["vis4_r"] = batches(lambda i: sc.trace_ao_visibility_dev(view, w, h, prim.data_ptr(), cnt.data_ptr(), n, radius, sem=sem,
                                                                     frame0=n * i, ao_eps=eps))
        res["open_r"], _ = share()
        res["ao4_again"] = batches(lambda i: sc.trace_ao_batch_dev(view, w, h, prim.data_ptr(), ao4.data_ptr(), w * h, n, sem=sem,
                                                                   frame0=n * i, ao_eps=eps))
        res["phases_inf"] = phases(float("inf"))
        res["phases_r"] = phases(radius)
        sc.check()
        res["scratch_mib"] = (sc.device_bytes - flat.n_nodes * 80 - flat.n_tris * 48) / 2.0 ** 20
        out[name] = res
        sc.close()
    print("AOVIS_CHILD " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1].split(","))
    rounds, scenes, path = 3, "bistro,hairball", os.path.join(ROOT, "profiles", "ao_visibility.log")
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

    res = []
    for r in range(rounds):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scenes], capture_output=True, text=True, timeout=900)
        line = [x for x in p.stdout.splitlines() if x.startswith("AOVIS_CHILD ")]
        if p.returncode or not line:
            print("child failed: %s" % p.stderr[-600:], flush=True)
            return 1
        res.append(json.loads(line[0][12:]))
        say("round %d " % r + json.dumps(res[-1]))
    say("\n%sx%s, TRX_SEM_CPU, 4 samples per pixel: median over %d processes [min .. max] of each process's median batch (ms per pass)"
        % (os.environ.get("W", "1920"), os.environ.get("H", "1080"), rounds))
    for s in scenes.split(","):
        med = {}
        for key in ("ao4", "ao4_again", "vis4_inf", "vis4_r"):
            v = [x[s][key] for x in res]
            med[key] = statistics.median(v)
            say("%-9s %-10s %.4f [%.4f .. %.4f]" % (s, key, med[key], min(v), max(v)))
        both = [x[s][k] for x in res for k in ("ao4", "ao4_again")]
        base = statistics.median(both)
        say("%-9s closest-hit batch over all its runs: %.4f [%.4f .. %.4f], spread %.1f %% of the median" %
            (s, base, min(both), max(both), 100 * (max(both) - min(both)) / base))
        say("%-9s visibility at +inf / closest-hit batch: %.3f; at radius %.3g (0.404 x diagonal): %.3f" %
            (s, med["vis4_inf"] / base, res[0][s]["radius"], med["vis4_r"] / base))
        for key, label in (("phases_inf", "+inf"), ("phases_r", "radius")):
            ph = [statistics.median(x[s][key][k] for x in res) for k in range(3)]
            say("%-9s split at %-6s ray generation %.4f  any-hit walk %.4f  reduce %.4f  (sum %.4f ms)" % (s, label, ph[0], ph[1], ph[2], sum(ph)))
        say("%-9s surface pixels %.1f %%; mean unoccluded share at +inf %.3f, at the radius %.3f; device bytes beyond nodes and "
            "triangles %.0f MiB" % (s, 100 * res[0][s]["surface"], res[0][s]["open_inf"], res[0][s]["open_r"], res[0][s]["scratch_mib"]))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
