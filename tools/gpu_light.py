"""Direct light (trx_trace_light_visibility_dev, trx_light_term_dev): what a shadow pass costs next to the AO visibility pass.

    python tools/gpu_light.py [--rounds 3] [--scenes bistro,hairball] [--out profiles/light_pass.log]

The bistro-class and hairball-class 1080p frames, semantics TRX_SEM_CPU.  Per round a fresh child process (the protocol of
tools/gpu_ao_visibility.py: one process's pass time depends on where its scene landed in memory) builds the scene, runs
bench.py's wake frames (140 primary frames), and times in batches of back-to-back launches (one hipEvent pair per batch):
  vis4       trx_trace_ao_visibility_dev, 4 samples, radius +inf: the reference pass.  The change that added the light pass
             does not touch its kernels (their instructions are the parent commit's), so its numbers are the parent's and their
             spread over the rounds is the margin everything else is read against.
  point      trx_trace_light_visibility_dev, one point light a quarter of the scene's height above the camera: one shadow ray
             per pixel.
  rect4      the same with one rect light (a horizontal square around that point, a tenth of the scene's diagonal wide) at 4
             samples.
  term       trx_light_term_dev over both lights' planes.
and splits the point and the rect pass into ray generation / any-hit walk / reduce with hipEvents between the launches
(trx_debug_light_visibility_phases; median of 9 passes).  Printed and written to --out: per form the median over rounds of
each child's median batch (ms per pass) with the spread over rounds, the splits, and what the planes say (lit share of the
surface pixels, share of the pixels whose ray was not cast)."""
import ctypes as C
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
        diag = float(np.linalg.norm(hi - lo))
        above = np.array(eye, dtype=np.float64) + np.array([0.0, 0.25 * (hi[1] - lo[1]), 0.0])
        side = 0.1 * diag
        point = T.light_array([T.light(T.LIGHT_POINT, above.tolist())])
        rect = T.light_array([T.light(T.LIGHT_RECT, (above - np.array([0.5 * side, 0.0, 0.5 * side])).tolist(), (side, 0.0, 0.0), (0.0, 0.0, side))])
        both = T.light_array([point[0], rect[0]])
        sc = T.Scene(flat)
        prim = torch.zeros(w * h, dtype=torch.int64, device="cuda")
        attr = torch.zeros(w * h * 24, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(w * h, dtype=torch.uint8, device="cuda")
        lit = torch.zeros(2 * w * h, dtype=torch.uint8, device="cuda")
        val = torch.zeros(w * h, dtype=torch.float32, device="cuda")
        for _ in range(140):   # the wake frames
            sc.trace_primary_dev(view, w, h, prim.data_ptr(), sem=sem)
        sc.hit_attributes_primary_dev(view, w, h, prim.data_ptr(), attr.data_ptr())
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

        def shares(plane, samples):
            c = plane.cpu().numpy()
            surf = c[c != L.AO_NO_SURFACE]
            return (float(surf.mean() / samples) if surf.size else 0.0), float((c != L.AO_NO_SURFACE).mean())

        def not_cast(light):
            rays = torch.zeros(w * h * 8, dtype=torch.float32, device="cuda")
            sc.light_rays_dev(view, w, h, light, prim.data_ptr(), rays.data_ptr(), shadow_eps=eps)
            torch.cuda.synchronize()
            return float((rays.view(-1, 8)[:, 7] < 0).float().mean().item())

        def phases(lights):
            rows = []
            for i in range(9):
                ms = (C.c_float * 3)()
                L.check(lib.trx_debug_light_visibility_phases(sc.handle, C.byref(view), w, h, sem, 0, lights, len(lights), n * i, n, eps,
                                                              C.c_void_p(prim.data_ptr()), None, C.c_void_p(lit.data_ptr()), ms))
                rows.append(list(ms))
            return [statistics.median(x[k] for x in rows) for k in range(3)]

        def vis4(i):
            sc.trace_ao_visibility_dev(view, w, h, prim.data_ptr(), cnt.data_ptr(), n, float("inf"), sem=sem, frame0=n * i, ao_eps=eps)

        def light_pass(lights):
            return lambda i: sc.trace_light_visibility_dev(view, w, h, lights, prim.data_ptr(), lit.data_ptr(), n_samples=n, sem=sem,
                                                           frame0=n * i, shadow_eps=eps)

        res = {"diag": diag}
        res["vis4"] = batches(vis4)
        res["point"] = batches(light_pass(point))
        res["lit_point"], res["surface"] = shares(lit[:w * h], 1)
        res["rect4"] = batches(light_pass(rect))
        res["lit_rect"], _ = shares(lit[:w * h], n)
        res["vis4_again"] = batches(vis4)
        light_pass(both)(0)
        res["term"] = batches(lambda i: sc.light_term_dev(view, w, h, both, prim.data_ptr(), attr.data_ptr(), lit.data_ptr(), val.data_ptr(),
                                                          n_samples=n, ambient=0.1))
        res["not_cast_point"] = not_cast(point[0])
        res["phases_point"] = phases(point)
        res["phases_rect4"] = phases(rect)
        sc.check()
        out[name] = res
        sc.close()
    print("LIGHT_CHILD " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1].split(","))
    rounds, scenes, path = 3, "bistro,hairball", os.path.join(ROOT, "profiles", "light_pass.log")
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
        line = [x for x in p.stdout.splitlines() if x.startswith("LIGHT_CHILD ")]
        if p.returncode or not line:
            print("child failed (exit %d): %s" % (p.returncode, p.stderr[-600:]), flush=True)
            return 1
        res.append(json.loads(line[0][12:]))
        say("round %d " % r + json.dumps(res[-1]))
    say("\n%sx%s, TRX_SEM_CPU: median over %d processes [min .. max] of each process's median batch (ms per pass)"
        % (os.environ.get("W", "1920"), os.environ.get("H", "1080"), rounds))
    for s in scenes.split(","):
        med = {}
        for key in ("vis4", "vis4_again", "point", "rect4", "term"):
            v = [x[s][key] for x in res]
            med[key] = statistics.median(v)
            say("%-9s %-10s %.4f [%.4f .. %.4f]" % (s, key, med[key], min(v), max(v)))
        ref = [x[s][k] for x in res for k in ("vis4", "vis4_again")]
        base = statistics.median(ref)
        say("%-9s AO visibility at 4 samples over all its runs: %.4f [%.4f .. %.4f], spread %.1f %% of the median" %
            (s, base, min(ref), max(ref), 100 * (max(ref) - min(ref)) / base))
        say("%-9s point light / AO visibility: %.3f; rect light at 4 samples / AO visibility: %.3f" % (s, med["point"] / base, med["rect4"] / base))
        for key, label in (("phases_point", "point"), ("phases_rect4", "rect4")):
            ph = [statistics.median(x[s][key][k] for x in res) for k in range(3)]
            say("%-9s split of %-6s ray generation %.4f  any-hit walk %.4f  reduce %.4f  (sum %.4f ms); term %.4f ms (two lights)"
                % (s, label, ph[0], ph[1], ph[2], sum(ph), med["term"]))
        say("%-9s surface pixels %.1f %%; lit share of them: point %.3f, rect at 4 samples %.3f; pixels whose ray toward the point light "
            "is not cast (no surface or facing away) %.1f %%" % (s, 100 * res[0][s]["surface"], res[0][s]["lit_point"], res[0][s]["lit_rect"],
                                                                 100 * res[0][s]["not_cast_point"]))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
