"""Sparse AO visibility (trx_trace_ao_visibility_sparse_dev + trx_ao_upsample_dev): what tracing one pixel in s x s and
rebuilding the term costs next to the dense pass and its filter, and what it does to the image.

    python tools/gpu_ao_sparse.py [--rounds 3] [--scenes bistro,hairball] [--out profiles/ao_sparse.log]

The bistro-class and hairball-class 1080p frames, semantics TRX_SEM_CPU, 4 samples per pixel, radius +inf.  Per round a
fresh child process (as tools/gpu_ao_visibility.py does) builds the scene, runs bench.py's wake frames, traces the primary
and attribute records once, and times in batches of back-to-back launches (one hipEvent pair per batch):
  dense      (a) trx_trace_ao_visibility_dev, then trx_ao_filter_dev at radius 2 with normals: the parent commit's kernels,
             which this change does not touch.  Timed first and again last; the spread of all its runs is the margin.
  sparse2/4  (b) trx_trace_ao_visibility_sparse_dev at stride 2 / 4, phase 0, then trx_ao_upsample_dev at radius 1 with normals.
and (c) splits (a) and (b) into their two calls with a hipEvent between them (median of 9), (d) shades the terms of (a)
and (b) under the same seeds and reports the mean and largest absolute difference of the RGBA8 codes, (e) classifies the
pixels of (b) with tests/ao_sparse_twin.py over the device's records (round 0 only): accepted / fallback / empty shares of
the surface pixels.  "faster" is written only where (b) beats (a) by more than (a)'s own spread."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER_R, UP_R, TOL, COS = 2, 1, 0.02, 0.9
STRIDES = (2, 4)


def child(scenes, classify):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tray_racing_amd as T
    w, h = int(os.environ.get("W", "1920")), int(os.environ.get("H", "1080"))
    sem, n, eps, inf = T.SEM_CPU, 4, 0.01, float("inf")
    out = {}
    for name in scenes:
        verts, counts = T.gen_scene(name, 0, 1)
        flat = T.flat_build(verts, counts)
        eye, look, fov = T.scene_camera(name)
        view = T.view_from_camera(eye, look, fov, w, h)
        sc = T.Scene(flat)
        px = w * h
        prim = torch.zeros(px, dtype=torch.int64, device="cuda")
        attr = torch.zeros(px * 24, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(px, dtype=torch.uint8, device="cuda")
        lo = torch.zeros(px, dtype=torch.uint8, device="cuda")
        term = torch.zeros(px, dtype=torch.int32, device="cuda")
        term_s = torch.zeros(px, dtype=torch.int32, device="cuda")
        rgba = [torch.zeros(px * 4, dtype=torch.uint8, device="cuda") for _ in range(2)]
        for _ in range(140):   # the wake frames
            sc.trace_primary_dev(view, w, h, prim.data_ptr(), sem=sem)
        sc.hit_attributes_primary_dev(view, w, h, prim.data_ptr(), attr.data_ptr())
        torch.cuda.synchronize()

        def dense(i, mark=None):
            sc.trace_ao_visibility_dev(view, w, h, prim.data_ptr(), cnt.data_ptr(), n, inf, sem=sem, frame0=n * i, ao_eps=eps)
            if mark:
                mark.record()
            sc.ao_filter_dev(w, h, prim.data_ptr(), cnt.data_ptr(), term.data_ptr(), n, FILTER_R, depth_tol=TOL, normal_cos=COS,
                             d_attr=attr.data_ptr())

        def sparse(stride):
            def run(i, mark=None):
                sc.trace_ao_visibility_sparse_dev(view, w, h, stride, 0, prim.data_ptr(), lo.data_ptr(), n, inf, sem=sem, frame0=n * i,
                                                  ao_eps=eps)
                if mark:
                    mark.record()
                sc.ao_upsample_dev(w, h, stride, 0, prim.data_ptr(), lo.data_ptr(), term_s.data_ptr(), n, UP_R, depth_tol=TOL,
                                   normal_cos=COS, d_attr=attr.data_ptr())
            return run

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

        def split(fn):
            rows = []
            for i in range(9):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                fn(i, e[1])
                e[2].record()
                torch.cuda.synchronize()
                rows.append((e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])))
            return [statistics.median(r[k] for r in rows) for k in range(2)]

        res = {"dense": batches(dense)}
        for s in STRIDES:
            res["sparse%d" % s] = batches(sparse(s))
        res["dense_again"] = batches(dense)
        res["split_dense"] = split(dense)
        # (d), (e): one frame of each under the same seeds
        dense(0)
        sc.shade_ao_term_dev(term.data_ptr(), px, rgba[0].data_ptr())
        torch.cuda.synchronize()
        img_a = rgba[0].cpu().numpy().reshape(-1, 4)[:, 0].astype(np.int32)
        for s in STRIDES:
            res["split_sparse%d" % s] = split(sparse(s))
            sparse(s)(0)
            sc.shade_ao_term_dev(term_s.data_ptr(), px, rgba[1].data_ptr())
            torch.cuda.synchronize()
            d = np.abs(rgba[1].cpu().numpy().reshape(-1, 4)[:, 0].astype(np.int32) - img_a)
            res["diff%d" % s] = [float(d.mean()), int(d.max()), float((d != 0).mean())]
            if classify:
                from ao_sparse_twin import ao_upsample, class_counts, lo_size
                wlo, hlo = lo_size(w, h, s)
                _, cls = ao_upsample(prim.cpu().numpy().view(T.HIT_DTYPE), attr.cpu().numpy().view(T.HIT_ATTR_DTYPE)["normal"],
                                     lo.cpu().numpy()[:wlo * hlo], w, h, s, 0, n, UP_R, TOL, COS, classes=True)
                res["classes%d" % s] = list(class_counts(cls))
        sc.check()
        out[name] = res
        sc.close()
    print("AOSPARSE_CHILD " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1].split(","), args[2] == "1")
    rounds, scenes, path = 3, "bistro,hairball", os.path.join(ROOT, "profiles", "ao_sparse.log")
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

    try:
        say("library " + open(os.path.join(ROOT, "tray_racing_amd", ".build_id")).read().strip())
    except OSError:
        say("library unknown")
    res = []
    for r in range(rounds):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scenes, "1" if r == 0 else "0"], capture_output=True,
                           text=True, timeout=900)
        line = [x for x in p.stdout.splitlines() if x.startswith("AOSPARSE_CHILD ")]
        if p.returncode or not line:
            print("child failed: %s" % p.stderr[-600:], flush=True)
            return 1
        res.append(json.loads(line[0][15:]))
        say("round %d " % r + json.dumps(res[-1]))
    say("\n%sx%s, TRX_SEM_CPU, 4 samples per pixel, radius +inf: median over %d processes [min .. max] of each process's median batch "
        "(ms per pass + image pass)" % (os.environ.get("W", "1920"), os.environ.get("H", "1080"), rounds))
    for s in scenes.split(","):
        both = [x[s][k] for x in res for k in ("dense", "dense_again")]
        base = statistics.median(both)
        spread = (max(both) - min(both)) / base
        say("%-9s dense pass + filter r=%d over all its runs: %.4f [%.4f .. %.4f], spread %.1f %% of the median" %
            (s, FILTER_R, base, min(both), max(both), 100 * spread))
        ph = [statistics.median(x[s]["split_dense"][k] for x in res) for k in range(2)]
        say("%-9s   split: visibility pass %.4f  filter %.4f" % (s, ph[0], ph[1]))
        for st in STRIDES:
            v = [x[s]["sparse%d" % st] for x in res]
            med = statistics.median(v)
            verdict = "faster" if max(v) < min(both) and base - med > spread * base else "slower" if min(v) > max(both) else "within the spread"
            say("%-9s stride %d + upsample r=%d: %.4f [%.4f .. %.4f]  x %.3f of dense: %s" % (s, st, UP_R, med, min(v), max(v), med / base, verdict))
            ph = [statistics.median(x[s]["split_sparse%d" % st][k] for x in res) for k in range(2)]
            say("%-9s   split: sparse visibility pass %.4f  upsample %.4f" % (s, ph[0], ph[1]))
            d = res[0][s]["diff%d" % st]
            say("%-9s   image against dense + filter: mean |code difference| %.3f, largest %d, %.1f %% of the pixels differ" %
                (s, d[0], d[1], 100 * d[2]))
            n, acc, fb, empty = res[0][s]["classes%d" % st]
            say("%-9s   %d surface pixels: %.2f %% accepted, %.2f %% fallback, %.3f %% empty" %
                (s, n, 100.0 * acc / max(n, 1), 100.0 * fb / max(n, 1), 100.0 * empty / max(n, 1)))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
