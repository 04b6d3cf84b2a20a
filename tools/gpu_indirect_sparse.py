"""The sparse indirect term (trx_trace_indirect_sparse_dev + trx_value_upsample_dev): what tracing one bounce pixel in s x s
and rebuilding the term costs next to the dense indirect pass, and what it does to the image.

    python tools/gpu_indirect_sparse.py [--rounds 3] [--scenes bistro,hairball] [--out profiles/indirect_sparse.log]

The bistro-class and hairball-class 1080p frames, semantics TRX_SEM_CPU, 4 samples per pixel, one point light a quarter of the
scene's height above the camera (tools/gpu_indirect.py's), upsample radius 1, depth tolerance 0.1, cosine 0.9, with normals.
Per round a fresh child process (the protocol of tools/gpu_ao_visibility.py) builds the scene, runs bench.py's wake frames
(140 primary frames), and times in batches of back-to-back calls (one hipEvent pair per batch):
  dense      trx_trace_indirect_dev without a base into a plane, then the 3-level trx_value_filter_dev over it (a base of zeros) -
             timed first and last: THE REFERENCE of every ratio, and the spread of its runs is the margin.
  sparse2/4  trx_trace_indirect_sparse_dev at stride 2 / 4 (phase 0), trx_value_upsample_dev without a base into the plane,
             the same filter.
  up2/4      trx_value_upsample_dev alone.
A ratio is called a gain only when it lies outside the margin.  Then one frame of each form under the same seeds: the filtered
term's plane against the dense one's over the surface pixels (mean and RMS difference), and the whole GI image by the host
forms (trx_render_image_gi_filtered / trx_render_image_gi_sparse, ambient 0.1): the mean and the largest absolute difference of
the RGBA8 codes against the dense filtered image and the share of pixels that differ, and
(round 0 only) the upsample's classes by tests/indirect_sparse_twin.py over the device's records: accepted / fallback / empty
shares of the surface pixels.
Printed and written to --out: per form the median over rounds of each child's median with the spread over rounds."""
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, COS, UP_R, LEVELS = 0.1, 0.9, 1, 3
STRIDES = (2, 4)


def child(scenes, classify):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
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
        lo_c, hi_c = pts.min(0), pts.max(0)
        above = np.array(eye, dtype=np.float64) + np.array([0.0, 0.25 * (hi_c[1] - lo_c[1]), 0.0])
        point = T.light_array([T.light(T.LIGHT_POINT, above.tolist())])
        sc = T.Scene(flat)
        px = w * h
        prim = torch.zeros(px, dtype=torch.int64, device="cuda")
        attr = torch.zeros(px * 24, dtype=torch.uint8, device="cuda")
        low, ind, work, val, zeros = (torch.zeros(px, dtype=torch.float32, device="cuda") for _ in range(5))
        rgba = [torch.zeros(px * 4, dtype=torch.uint8, device="cuda") for _ in range(2)]
        for _ in range(140):   # the wake frames
            sc.trace_primary_dev(view, w, h, prim.data_ptr(), sem=sem)
        sc.hit_attributes_primary_dev(view, w, h, prim.data_ptr(), attr.data_ptr())
        torch.cuda.synchronize()

        def filt():
            # (the light term's place: a base of zeros, so that the image is the indirect term's)
            sc.value_filter_dev(w, h, prim.data_ptr(), ind.data_ptr(), val.data_ptr(), LEVELS, depth_tol=TOL, normal_cos=COS,
                                d_attr=attr.data_ptr(), d_base=zeros.data_ptr(), d_work=work.data_ptr())

        def dense(i):
            sc.trace_indirect_dev(view, w, h, point, prim.data_ptr(), ind.data_ptr(), n_samples=n, sem=sem, frame0=n * i, bounce_eps=eps,
                                  shadow_eps=eps, bounce_albedo=0.5)
            filt()

        def up(stride):
            def run(i):
                sc.value_upsample_dev(w, h, stride, 0, prim.data_ptr(), low.data_ptr(), ind.data_ptr(), UP_R, depth_tol=TOL, normal_cos=COS,
                                      d_attr=attr.data_ptr())
            return run

        def sparse(stride):
            def run(i):
                sc.trace_indirect_sparse_dev(view, w, h, stride, 0, point, prim.data_ptr(), low.data_ptr(), n_samples=n, sem=sem, frame0=n * i,
                                             bounce_eps=eps, shadow_eps=eps, bounce_albedo=0.5)
                up(stride)(i)
                filt()
            return run

        def batches(fn, n_batches=6, per=4, warm=6):
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

        res = {"dense": batches(dense)}
        for s in STRIDES:
            res["sparse%d" % s] = batches(sparse(s))
        for s in STRIDES:
            sparse(s)(0)       # (a low plane of this stride under the upsample)
            res["up%d" % s] = batches(up(s), per=8)
        res["dense_again"] = batches(dense)
        # one frame of each under the same seeds: the term's plane (a base of zeros), and the whole GI image by the host forms
        kw = dict(bounce_depth_tol=TOL, bounce_normal_cos=COS, bounce_eps=eps, bounce_albedo=0.5, sem=sem, shadow_eps=eps, ambient=0.1)
        dense(0)
        torch.cuda.synchronize()
        surf = (prim.view(torch.float32).view(-1, 2)[:, 0] < 3.0e38).cpu().numpy()
        plane_a = val.cpu().numpy().astype(np.float64)
        img_a = sc.render_image_gi_filtered(view, w, h, point, n, LEVELS, **kw)[0].reshape(-1, 4)[:, 0].astype(np.int32)
        res["surface"] = float(surf.mean())
        res["dense_image"] = [float(img_a.mean()), float(plane_a[surf].mean())]
        for s in STRIDES:
            sparse(s)(0)
            torch.cuda.synchronize()
            dp = np.abs(val.cpu().numpy().astype(np.float64) - plane_a)[surf]
            res["plane%d" % s] = [float(dp.mean()), float(np.sqrt((dp ** 2).mean()))]
            img_s = sc.render_image_gi_sparse(view, w, h, point, n, s, bounce_phase=0, bounce_upsample_radius=UP_R, bounce_filter_levels=LEVELS, **kw)[0]
            d = np.abs(img_s.reshape(-1, 4)[:, 0].astype(np.int32) - img_a)
            res["diff%d" % s] = [float(d.mean()), int(d.max()), float((d != 0).mean())]
            if classify:
                from ao_sparse_twin import class_counts, lo_size
                from indirect_sparse_twin import value_upsample
                wlo, hlo = lo_size(w, h, s)
                _, cls = value_upsample(prim.cpu().numpy().view(T.HIT_DTYPE), attr.cpu().numpy().view(T.HIT_ATTR_DTYPE)["normal"],
                                        low.cpu().numpy()[:wlo * hlo], w, h, s, 0, UP_R, TOL, COS, classes=True)
                res["classes%d" % s] = list(class_counts(cls))
        sc.check()
        out[name] = res
        sc.close()
    print("INDIRECT_SPARSE_CHILD " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1].split(","), args[2] == "1")
    rounds, scenes, path = 3, "bistro,hairball", os.path.join(ROOT, "profiles", "indirect_sparse.log")
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
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scenes, "1" if r == 0 else "0"], capture_output=True, text=True,
                           timeout=900)
        line = [x for x in p.stdout.splitlines() if x.startswith("INDIRECT_SPARSE_CHILD ")]
        if p.returncode or not line:
            print("child failed (exit %d): %s" % (p.returncode, p.stderr[-600:]), flush=True)
            return 1
        res.append(json.loads(line[0][len("INDIRECT_SPARSE_CHILD "):]))
        say("round %d " % r + json.dumps(res[-1]))
    w, h = int(os.environ.get("W", "1920")), int(os.environ.get("H", "1080"))
    say("\n%dx%d, TRX_SEM_CPU, 4 samples, one point light, upsample radius %d, %d filter levels at (%g, %g), with normals: median over %d processes "
        "[min .. max] of each process's median (ms)" % (w, h, UP_R, LEVELS, TOL, COS, rounds))
    for s in scenes.split(","):
        med = {}
        for key in ["dense", "dense_again"] + ["sparse%d" % k for k in STRIDES] + ["up%d" % k for k in STRIDES]:
            v = [x[s][key] for x in res]
            med[key] = statistics.median(v)
            say("%-9s %-12s %.4f [%.4f .. %.4f]" % (s, key, med[key], min(v), max(v)))
        ref = [x[s][k] for x in res for k in ("dense", "dense_again")]
        base = statistics.median(ref)
        margin = (max(ref) - min(ref)) / base
        say("%-9s the dense pass and its filter over all their runs: %.4f [%.4f .. %.4f], margin %.1f %% of the median" %
            (s, base, min(ref), max(ref), 100 * margin))
        for st in STRIDES:
            v = [x[s]["sparse%d" % st] for x in res]
            ratio = med["sparse%d" % st] / base
            outside = max(v) < min(ref) or min(v) > max(ref)
            say("%-9s stride %d: x %.3f of the dense form - %s; the upsample alone %.4f ms (%.1f %% of the sparse form)" %
                (s, st, ratio, ("a gain" if ratio < 1 else "a loss") + " outside the margin" if outside else "inside the margin: no difference shown",
                 med["up%d" % st], 100 * med["up%d" % st] / med["sparse%d" % st]))
            mean, largest, share = res[0][s]["diff%d" % st]
            say("%-9s   RGBA8 codes of the GI image (ambient 0.1) against the dense filtered one's (mean code %.1f): mean |difference| %.3f, largest %d, "
                "%.1f %% of the pixels differ" % (s, res[0][s]["dense_image"][0], mean, largest, 100 * share))
            say("%-9s   the filtered term over the surface pixels against the dense one (mean %.5f): mean |difference| %.5f, RMS %.5f" %
                (s, res[0][s]["dense_image"][1], res[0][s]["plane%d" % st][0], res[0][s]["plane%d" % st][1]))
            n, acc, fb, empty = res[0][s]["classes%d" % st]
            say("%-9s   %d surface pixels: %.2f %% accepted, %.2f %% fallback, %.3f %% empty" % (s, n, 100.0 * acc / n, 100.0 * fb / n, 100.0 * empty / n))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
