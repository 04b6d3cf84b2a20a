"""Emitters: what sampling the emissive triangles costs next to the passes it stands beside, what it buys in
noise, and the estimator check's figures.

    python tools/gpu_emitters.py [--rounds 2] [--scenes bistro,hairball] [--out profiles/emitter_pass.log]

TIMES.  The bistro-class and hairball-class 1080p frames, semantics TRX_SEM_CPU, the stand-in palette by object with the
smallest objects (up to three, 4 096 triangles together at the most) given an emissive material.  Per round
a fresh child process builds the scene, runs the wake frames and times, in batches of back-to-back launches (one hipEvent pair
per batch), in the same process:
  rect4 / rect4_again   trx_trace_light_visibility_dev, one rect light over the scene, 4 samples: the existing pass the emitter
                        pass is shaped like, first and last; its spread is the margin.
  em1 / em4             trx_trace_emitter_light_dev, 1 and 4 samples, no base.
  rgb4 / rgb4_again     trx_trace_indirect_rgb_dev, one point light, 4 samples: the existing RGB indirect pass.
  rgb4_em               trx_trace_indirect_rgb_emitters_dev, the same light, 4 samples.
NOISE.  The golden Cornell fixture (tests/golden/cornell_64.npz) with the stand-in table and no analytic light: the RMS error
over the surface pixels, relative to the mean, of the 4-sample colour term - emitter pass plus emitter-mode bounce - against
its 64-sample form at another frame0; beside it the existing pass's 4-sample bounce-only term (under a light of intensity 0)
against its own 64-sample form.
ESTIMATOR.  tests/test_gpu_emitters.py's check: the existing pass's mean emission term at frame0 0 and 100000, and the emitter
pass's mean, 64 samples each.
Every step of the parent sits under a time limit of its own; every line carries the library's hash."""
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 4096    # emissive triangles per scene at the most
KEYS = ("rect4", "em1", "em4", "rect4_again", "rgb4", "rgb4_em", "rgb4_again")


def _emissive_table(T, name, verts, counts):
    import numpy as np
    mats, idx = T.standin_materials(name, verts, counts)
    table = np.zeros((mats.shape[0] + 1, 6), dtype=np.float32)
    table[:-1, :3], table[:-1, 3:] = mats["albedo"], mats["emission"]
    table[-1] = (0.8, 0.8, 0.8, 4.0, 4.0, 4.0)
    idx = idx.copy()
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    picked, total = [], 0
    for j in np.argsort(np.asarray(counts), kind="stable").tolist():
        if counts[j] == 0:
            continue
        take = min(int(counts[j]), CAP - total)      # (a scene of few large objects: the first triangles of its smallest one)
        picked.append(j)
        idx[starts[j]:starts[j] + take] = table.shape[0] - 1
        total += take
        if len(picked) == 3 or total >= CAP:
            break
    return table, idx, picked, total


def child(scenes):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import tray_racing_amd as T
    w, h = int(os.environ.get("W", "1920")), int(os.environ.get("H", "1080"))
    sem, eps, eeps = T.SEM_CPU, 0.01, 0.001
    n_px = w * h
    out = {}
    for name in scenes:
        verts, counts = T.gen_scene(name, 0, 1)
        flat = T.flat_build(verts, counts)
        table, idx, picked, total = _emissive_table(T, name, verts, counts)
        eye, look, fov = T.scene_camera(name)
        view = T.view_from_camera(eye, look, fov, w, h)
        pts = flat.tri_verts.reshape(-1, 3)
        lo, hi = pts.min(0), pts.max(0)
        above = np.array(eye, dtype=np.float64) + np.array([0.0, 0.25 * (hi[1] - lo[1]), 0.0])
        point = T.light_array([T.light(T.LIGHT_POINT, above.tolist())])
        size = 0.1 * float((hi - lo).max())
        rect = T.light_array([T.light(T.LIGHT_RECT, (above - [0.5 * size, 0.0, 0.5 * size]).tolist(), (size, 0.0, 0.0), (0.0, 0.0, size))])
        sc = T.Scene(flat)
        sc.set_materials(table, idx[flat.tri_source])
        n_em = sc.build_emitters()
        prim = torch.zeros(n_px, dtype=torch.int64, device="cuda")
        lit = torch.zeros(n_px, dtype=torch.uint8, device="cuda")
        rgb = torch.zeros(3 * n_px, dtype=torch.float32, device="cuda")
        for _ in range(140):   # the wake frames
            sc.trace_primary_dev(view, w, h, prim.data_ptr(), sem=sem)
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

        def rect4(i):
            sc.trace_light_visibility_dev(view, w, h, rect, prim.data_ptr(), lit.data_ptr(), n_samples=4, sem=sem, frame0=4 * i, shadow_eps=eps)

        def em(n):
            def run(i):
                sc.trace_emitter_light_dev(view, w, h, prim.data_ptr(), rgb.data_ptr(), n_samples=n, sem=sem, frame0=n * i, shadow_eps=eps, emitter_eps=eeps)
            return run

        def rgb4(i):
            sc.trace_indirect_rgb_dev(view, w, h, point, prim.data_ptr(), rgb.data_ptr(), n_samples=4, sem=sem, frame0=4 * i, bounce_eps=eps, shadow_eps=eps)

        def rgb4_em(i):
            sc.trace_indirect_rgb_emitters_dev(view, w, h, point, prim.data_ptr(), rgb.data_ptr(), n_samples=4, sem=sem, frame0=4 * i, bounce_eps=eps,
                                               shadow_eps=eps, emitter_eps=eeps)
        res = {"emitters": n_em, "objects": len(picked)}
        res["rect4"] = batches(rect4)
        res["em1"], res["em4"] = batches(em(1)), batches(em(4))
        res["lit_share"] = float((rgb[:n_px] > 0).float().mean().item())
        res["rect4_again"] = batches(rect4)
        res["rgb4"] = batches(rgb4)
        res["rgb4_em"] = batches(rgb4_em)
        res["rgb4_again"] = batches(rgb4)
        sc.check()
        out[name] = res
        sc.close()
    print("EMITTERS_CHILD " + json.dumps(out), flush=True)


def cornell_child():
    """The noise figures and the estimator check's, on the golden Cornell fixture."""
    import ctypes as C
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import tray_racing_amd as T
    from tray_racing_amd import _lib
    g = np.load(os.path.join(ROOT, "tests", "golden", "cornell_64.npz"))
    n_tris = g["tri_verts"].shape[0]
    w, h = int(g["width"]), int(g["height"])
    flat = T.FlatScene(g["nodes"], g["tri_verts"], g["instance_offsets"], int(g["tlas_start"]), np.arange(n_tris), [0, n_tris])
    verts, counts = T.gen_scene("cornell", 0, 1)
    mats, idx = T.standin_materials("cornell", verts, counts)
    where = {v.tobytes(): i for i, v in enumerate(np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9))}
    by_prim = np.array([idx[where[v.tobytes()]] for v in g["tri_verts"].reshape(-1, 9)], dtype=np.uint16)
    view = _lib.View()
    C.memmove(C.byref(view), g["view"].tobytes(), C.sizeof(view))
    sc = T.Scene(flat)
    sc.set_materials(mats, by_prim)
    n_em = sc.build_emitters()
    n = w * h
    prim = torch.zeros(n, dtype=torch.int64, device="cuda")
    sc.trace_primary_dev(view, w, h, prim.data_ptr())
    torch.cuda.synchronize()
    rec = prim.cpu().numpy().view(T.HIT_DTYPE)
    surf = (rec["t"] < 3.0e38) & (rec["prim"] < n_tris)
    dark = T.light_array([T.light(T.LIGHT_POINT, (0.0, 1.0, 0.0), intensity=0.0)])

    def planes(fn):
        out = torch.zeros(3 * n, dtype=torch.float32, device="cuda")
        fn(out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(3, n).astype(np.float64)[:, surf]

    def parent(ns, frame0):
        return planes(lambda p: sc.trace_indirect_rgb_dev(view, w, h, dark, prim.data_ptr(), p, n_samples=ns, frame0=frame0, bounce_eps=0.01, shadow_eps=0.01))

    def direct(ns, frame0):
        return planes(lambda p: sc.trace_emitter_light_dev(view, w, h, prim.data_ptr(), p, n_samples=ns, frame0=frame0, shadow_eps=0.01, emitter_eps=0.001))

    def term(ns, frame0):
        def run(p):
            sc.trace_indirect_rgb_emitters_dev(view, w, h, [], prim.data_ptr(), p, n_samples=ns, frame0=frame0, bounce_eps=0.01, shadow_eps=0.01,
                                               emitter_eps=0.001)
            sc.trace_emitter_light_dev(view, w, h, prim.data_ptr(), p, n_samples=ns, frame0=frame0, shadow_eps=0.01, emitter_eps=0.001, d_base_rgb=p)
        return planes(run)
    res = {"emitters": n_em, "surface_pixels": int(surf.sum())}
    p0, p1, mine = parent(64, 0).mean(1), parent(64, 100000).mean(1), direct(64, 0).mean(1)
    res["estimator"] = {"parent_frame0_0": p0.tolist(), "parent_frame0_100000": p1.tolist(), "parent_run_to_run": (np.abs(p0 - p1) / p0).tolist(),
                        "emitter_pass": mine.tolist(), "emitter_rel_diff": (np.abs(mine - p0) / p0).tolist()}
    ref_new, ref_old = term(64, 1000), parent(64, 1000)
    rms = lambda a, ref: float(np.sqrt(((a - ref) ** 2).mean()) / ref.mean())  # noqa: E731
    res["rms4_emitters"] = statistics.median([rms(term(4, 4 * i), ref_new) for i in range(5)])
    res["rms4_parent"] = statistics.median([rms(parent(4, 4 * i), ref_old) for i in range(5)])
    res["mean_emitters"], res["mean_parent"] = float(ref_new.mean()), float(ref_old.mean())
    sc.check()
    sc.close()
    print("EMITTERS_CORNELL " + json.dumps(res), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1].split(","))
    if args and args[0] == "--cornell-child":
        return cornell_child()
    rounds, scenes, path = 2, "bistro,hairball", os.path.join(ROOT, "profiles", "emitter_pass.log")
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

    def run(mode, tag, limit):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__)] + mode, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print("%s: the child ran into its time limit" % tag, flush=True)
            return None
        line = [x for x in p.stdout.splitlines() if x.startswith(tag + " ")]
        if p.returncode or not line:
            print("child failed (exit %d): %s" % (p.returncode, p.stderr[-600:]), flush=True)
            return None
        return json.loads(line[0][len(tag) + 1:])

    c = run(["--cornell-child"], "EMITTERS_CORNELL", 120)
    if c is None:
        return 1
    e = c["estimator"]
    say("cornell_64, stand-in table, %d emitters, %d surface pixels, 64 samples, mean of each plane over the surface pixels:" % (c["emitters"], c["surface_pixels"]))
    say("  existing pass (trx_trace_indirect_rgb_dev, one light of intensity 0): frame0 0 %s, frame0 100000 %s" % (e["parent_frame0_0"], e["parent_frame0_100000"]))
    say("  existing pass, relative difference between the two: %s" % e["parent_run_to_run"])
    say("  emitter pass (trx_trace_emitter_light_dev): %s, relative difference to the existing pass at frame0 0: %s" % (e["emitter_pass"], e["emitter_rel_diff"]))
    say("cornell_64, no analytic light, RMS error of the 4-sample term against a 64-sample one over the surface pixels, relative to the mean (median of 5 frame0):")
    say("  emitter pass + emitter-mode bounce %.4f (mean %.5f); existing bounce-only term %.4f (mean %.5f); ratio %.2f"
        % (c["rms4_emitters"], c["mean_emitters"], c["rms4_parent"], c["mean_parent"], c["rms4_parent"] / c["rms4_emitters"]))
    res = []
    for r in range(rounds):
        one = run(["--child", scenes], "EMITTERS_CHILD", 280)
        if one is None:
            return 1
        res.append(one)
        say("round %d " % r + json.dumps(one))
    say("%sx%s, TRX_SEM_CPU, stand-in palette with the smallest objects emissive: median over %d processes [min .. max] of each process's median (ms)"
        % (os.environ.get("W", "1920"), os.environ.get("H", "1080"), rounds))
    for s in scenes.split(","):
        med = {}
        say("%-9s %d emitters in %d objects; pixels the 4-sample emitter pass lights (R plane) %.1f %%" % (s, res[0][s]["emitters"], res[0][s]["objects"],
                                                                                                     100 * res[0][s]["lit_share"]))
        for key in KEYS:
            v = [x[s][key] for x in res]
            med[key] = statistics.median(v)
            say("%-9s %-11s %.4f [%.4f .. %.4f]" % (s, key, med[key], min(v), max(v)))
        for a, b in (("rect4", "rect4_again"), ("rgb4", "rgb4_again")):
            ref = [x[s][k] for x in res for k in (a, b)]
            base = statistics.median(ref)
            med[a + "_all"] = base
            say("%-9s %s over all its runs: %.4f [%.4f .. %.4f], spread %.1f %% of the median" % (s, a, base, min(ref), max(ref), 100 * (max(ref) - min(ref)) / base))
        say("%-9s emitter pass / rect-light pass, 4 samples each: %.3f; emitter pass 1 sample / 4 samples: %.3f"
            % (s, med["em4"] / med["rect4_all"], med["em1"] / med["em4"]))
        say("%-9s emitter-mode indirect pass / RGB indirect pass: %.4f (%+.2f %%)" % (s, med["rgb4_em"] / med["rgb4_all"], 100 * (med["rgb4_em"] / med["rgb4_all"] - 1)))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
