"""Materials and the colour image: what the colour mode costs next to the grey passes it stands beside.

    python tools/gpu_materials.py [--rounds 3] [--scenes bistro,hairball] [--out profiles/material_pass.log]

The bistro-class and hairball-class 1080p frames, semantics TRX_SEM_CPU, 4 bounce samples, one point light a quarter of the
scene's height above the camera (tools/gpu_indirect.py's), the stand-in palette by object.  Per round a fresh child process
(tools/gpu_indirect.py's protocol) builds the scene, runs the wake frames and times, in batches of back-to-back launches (one
hipEvent pair per batch), in the same process:
  gi4 / gi4_again   trx_trace_indirect_dev, no base: the grey pass, first and last; its spread is the margin.
  rgb4              trx_trace_indirect_rgb_dev: differs from gi4 in the gather and the finish only.
  filter1 / filter3 trx_value_filter_dev, 3 levels: one call, and the three per-plane calls of the colour image.
  up1 / up3         trx_value_upsample_dev from a stride-2 low grid, radius 1: one call, and three.
  value / compose / rgb_shade   trx_shade_value_dev (k_value) against trx_material_compose_dev and trx_shade_rgb_dev.
  gi_sparse / colour   trx_render_image_gi_sparse against trx_render_image_colour, stride 2, 3 levels (host forms: their own ms).
Every step of the parent sits under a time limit of its own; every line carries the library's hash."""
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("gi4", "rgb4", "gi4_again", "filter1", "filter3", "up1", "up3", "value", "compose", "rgb_shade", "gi_sparse", "colour")


def child(scenes):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import tray_racing_amd as T
    w, h = int(os.environ.get("W", "1920")), int(os.environ.get("H", "1080"))
    sem, n, eps = T.SEM_CPU, 4, 0.01
    n_px = w * h
    out = {}
    for name in scenes:
        verts, counts = T.gen_scene(name, 0, 1)
        flat = T.flat_build(verts, counts)
        mats, idx = T.standin_materials(name, verts, counts)
        eye, look, fov = T.scene_camera(name)
        view = T.view_from_camera(eye, look, fov, w, h)
        pts = flat.tri_verts.reshape(-1, 3)
        lo, hi = pts.min(0), pts.max(0)
        above = np.array(eye, dtype=np.float64) + np.array([0.0, 0.25 * (hi[1] - lo[1]), 0.0])
        point = T.light_array([T.light(T.LIGHT_POINT, above.tolist())])
        sc = T.Scene(flat)
        sc.set_materials(mats, idx[flat.tri_source])
        prim = torch.zeros(n_px, dtype=torch.int64, device="cuda")
        attr = torch.zeros(n_px * 6, dtype=torch.float32, device="cuda")
        val = torch.zeros(n_px, dtype=torch.float32, device="cuda")
        rgb = torch.zeros(3 * n_px, dtype=torch.float32, device="cuda")
        rgb2 = torch.zeros(3 * n_px, dtype=torch.float32, device="cuda")
        work = torch.zeros(n_px, dtype=torch.float32, device="cuda")
        rgba = torch.zeros(n_px, dtype=torch.int32, device="cuda")
        for _ in range(140):   # the wake frames
            sc.trace_primary_dev(view, w, h, prim.data_ptr(), sem=sem)
        sc.hit_attributes_primary_dev(view, w, h, prim.data_ptr(), attr.data_ptr())
        torch.cuda.synchronize()

        def batches(fn, n_batches=6, per=4, warm=4):
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

        def gi4(i):
            sc.trace_indirect_dev(view, w, h, point, prim.data_ptr(), val.data_ptr(), n_samples=n, sem=sem, frame0=n * i, bounce_eps=eps,
                                  shadow_eps=eps, bounce_albedo=0.5)

        def rgb4(i):
            sc.trace_indirect_rgb_dev(view, w, h, point, prim.data_ptr(), rgb.data_ptr(), n_samples=n, sem=sem, frame0=n * i, bounce_eps=eps,
                                      shadow_eps=eps)

        def filt(planes):
            def run(i):
                for c in range(planes):
                    sc.value_filter_dev(w, h, prim.data_ptr(), rgb.data_ptr() + c * n_px * 4, rgb2.data_ptr() + c * n_px * 4, 3, d_attr=attr.data_ptr(),
                                        d_work=work.data_ptr())
            return run

        def up(planes):
            n_lo = ((w + 1) // 2) * ((h + 1) // 2)

            def run(i):
                for c in range(planes):
                    sc.value_upsample_dev(w, h, 2, 0, prim.data_ptr(), rgb.data_ptr() + c * n_lo * 4, rgb2.data_ptr() + c * n_px * 4, 1,
                                          d_attr=attr.data_ptr())
            return run

        res = {}
        res["gi4"] = batches(gi4)
        res["rgb4"] = batches(rgb4)
        res["lit_share"] = float((rgb[:n_px] > 0).float().mean().item())
        res["filter1"], res["filter3"] = batches(filt(1)), batches(filt(3))
        res["up1"], res["up3"] = batches(up(1)), batches(up(3))
        res["value"] = batches(lambda i: sc.shade_value_dev(val.data_ptr(), n_px, rgba.data_ptr()), per=16)
        res["compose"] = batches(lambda i: sc.material_compose_dev(prim.data_ptr(), val.data_ptr(), n_px, rgb2.data_ptr(), d_indirect_rgb=rgb.data_ptr()), per=16)
        res["rgb_shade"] = batches(lambda i: sc.shade_rgb_dev(rgb2.data_ptr(), n_px, rgba.data_ptr()), per=16)
        res["gi4_again"] = batches(gi4)
        host = {"gi_sparse": [], "colour": []}
        for i in range(5):
            host["gi_sparse"].append(sc.render_image_gi_sparse(view, w, h, point, n, 2, bounce_filter_levels=3, sem=sem, frame0=n * i)[1])
            host["colour"].append(sc.render_image_colour(view, w, h, point, bounce_samples=n, bounce_stride=2, bounce_filter_levels=3, sem=sem, frame0=n * i)[1])
        res["gi_sparse"], res["colour"] = statistics.median(host["gi_sparse"][1:]), statistics.median(host["colour"][1:])
        sc.check()
        out[name] = res
        sc.close()
    print("MATERIALS_CHILD " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1].split(","))
    rounds, scenes, path = 3, "bistro,hairball", os.path.join(ROOT, "profiles", "material_pass.log")
    while args and args[0].startswith("--"):
        if args[0] == "--rounds":
            rounds = int(args[1])
        elif args[0] == "--scenes":
            scenes = args[1]
        elif args[0] == "--out":
            path = args[1]
        args = args[2:]
    with open(os.path.join(ROOT, "tray_racing_amd", "libtrx.so"), "rb") as f:
        lib = "library %s  " % hashlib.sha256(f.read()).hexdigest()[:16]
    lines = []

    def say(s):
        print(lib + s, flush=True)
        lines.append(lib + s)

    res = []
    for r in range(rounds):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scenes], capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            print("round %d: the child ran into its time limit" % r, flush=True)
            return 1
        line = [x for x in p.stdout.splitlines() if x.startswith("MATERIALS_CHILD ")]
        if p.returncode or not line:
            print("child failed (exit %d): %s" % (p.returncode, p.stderr[-600:]), flush=True)
            return 1
        res.append(json.loads(line[0][16:]))
        say("round %d " % r + json.dumps(res[-1]))
    say("%sx%s, TRX_SEM_CPU, 4 bounce samples, one point light, stand-in palette: median over %d processes [min .. max] of each process's median (ms)"
        % (os.environ.get("W", "1920"), os.environ.get("H", "1080"), rounds))
    for s in scenes.split(","):
        med = {}
        for key in KEYS:
            v = [x[s][key] for x in res]
            med[key] = statistics.median(v)
            say("%-9s %-10s %.4f [%.4f .. %.4f]" % (s, key, med[key], min(v), max(v)))
        ref = [x[s][k] for x in res for k in ("gi4", "gi4_again")]
        base = statistics.median(ref)
        say("%-9s grey indirect pass over all its runs: %.4f [%.4f .. %.4f], spread %.1f %% of the median" %
            (s, base, min(ref), max(ref), 100 * (max(ref) - min(ref)) / base))
        say("%-9s RGB indirect pass / grey indirect pass: %.4f (%+.2f %%)" % (s, med["rgb4"] / base, 100 * (med["rgb4"] / base - 1)))
        say("%-9s three filter calls / one: %.2f; three upsample calls / one: %.2f" % (s, med["filter3"] / med["filter1"], med["up3"] / med["up1"]))
        say("%-9s compose / k_value: %.2f; RGB shade / k_value: %.2f" % (s, med["compose"] / med["value"], med["rgb_shade"] / med["value"]))
        say("%-9s render_image_colour / render_image_gi_sparse (stride 2, 3 levels): %.3f" % (s, med["colour"] / med["gi_sparse"]))
        say("%-9s pixels the bounce lights (R plane) %.1f %%" % (s, 100 * res[0][s]["lit_share"]))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
