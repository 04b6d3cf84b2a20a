"""The frame's image passes (trx_ao_filter_dev, trx_shade_*_dev, trx_render_image): what they cost next to the passes they follow.

    python tools/gpu_image.py [--runs 25] [--scene bistro] [--out profiles/image_passes.log]

The bistro-class 1080p frame, semantics TRX_SEM_CPU, 4 samples per pixel at radius +inf.  One process builds the scene, runs
bench.py's wake frames (140 primary frames), traces the frame's records once (primary, attributes, closest-hit AO, visibility
counts) and then times, one hipEvent pair per run, min and median of --runs runs after 5 warm-up runs:
  filter     trx_ao_filter_dev at radius 0, 2 and 4, with and without normals (depth_tol 0.02, normal_cos 0.9)
  shade      each of trx_shade_reference_dev / _ao_counts_dev / _ao_term_dev over the whole frame
with the bytes each pass moves by its definition (per pixel: 8 B of hit record, 1 B of count, 24 B of attribute record with
normals, 4 B of term out; shades 16 / 1 / 4 B in, 4 B out - every pixel counted, though a pixel without a surface reads its hit
record only) and what fraction of the device's streaming ceiling (trx_debug_copy_rate, bytes read + written per second) that
is.  Then wall-clock time, median of 9 calls each, of the host forms: trx_render_image (4 bytes per pixel back) in its
three forms against trx_trace_primary_ao (16 bytes per pixel back) followed by the host's shading of those records -
numpy's float32 power here, standing in for the command line's loop."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    args = sys.argv[1:]
    runs, scene, path = 25, "bistro", os.path.join(ROOT, "profiles", "image_passes.log")
    while args and args[0].startswith("--"):
        if args[0] == "--runs":
            runs = int(args[1])
        elif args[0] == "--scene":
            scene = args[1]
        elif args[0] == "--out":
            path = args[1]
        args = args[2:]
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import tray_racing_amd as T
    w, h = int(os.environ.get("W", "1920")), int(os.environ.get("H", "1080"))
    sem, n, eps, px = T.SEM_CPU, 4, 0.01, w * h
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    verts, counts = T.gen_scene(scene, 0, 1)
    flat = T.flat_build(verts, counts)
    eye, look, fov = T.scene_camera(scene)
    view = T.view_from_camera(eye, look, fov, w, h)
    sc = T.Scene(flat)
    ceiling = T.copy_rate(0)
    prim = torch.zeros(px, dtype=torch.int64, device="cuda")
    ao = torch.zeros(px, dtype=torch.int64, device="cuda")
    attr = torch.zeros(px * 24, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(px, dtype=torch.uint8, device="cuda")
    term = torch.zeros(px, dtype=torch.int32, device="cuda")
    rgba = torch.zeros(px, dtype=torch.int32, device="cuda")
    for _ in range(140):   # the wake frames
        sc.trace_primary_dev(view, w, h, prim.data_ptr(), sem=sem)
    sc.trace_ao_dev(view, w, h, prim.data_ptr(), ao.data_ptr(), sem=sem, frame=0, ao_eps=eps)
    sc.hit_attributes_primary_dev(view, w, h, prim.data_ptr(), attr.data_ptr())
    torch.cuda.synchronize()
    vis = []
    for i in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sc.trace_ao_visibility_dev(view, w, h, prim.data_ptr(), cnt.data_ptr(), n, float("inf"), sem=sem, frame0=0, ao_eps=eps)
        e1.record()
        torch.cuda.synchronize()
        vis.append(e0.elapsed_time(e1))
    surf = float((cnt != T._lib.AO_NO_SURFACE).float().mean())
    say("%s-class %dx%d, TRX_SEM_CPU, %d samples per pixel at +inf: %.1f %% surface pixels; the visibility pass before these "
        "passes %.3f ms (median of 5 single launches); streaming ceiling %.0f GB/s (trx_debug_copy_rate)"
        % (scene, w, h, n, 100 * surf, statistics.median(vis), ceiling / 1e9))

    def timed(fn):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return min(ts), statistics.median(ts)

    def row(label, fn, bytes_per_pixel):
        mn, med = timed(fn)
        moved = bytes_per_pixel * px
        say("%-34s min %.4f ms  median %.4f ms  %6.1f MB moved  %5.1f %% of the ceiling at the median"
            % (label, mn, med, moved / 1e6, 100 * moved / (med * 1e-3) / ceiling))

    say("\nmin and median of %d runs, one hipEvent pair per run" % runs)
    for r in (0, 2, 4):
        for normals in (True, False):
            row("filter r=%d %s" % (r, "with normals" if normals else "without normals"),
                lambda r=r, normals=normals: sc.ao_filter_dev(w, h, prim.data_ptr(), cnt.data_ptr(), term.data_ptr(), n, r, depth_tol=0.02,
                                                              normal_cos=0.9, d_attr=attr.data_ptr() if normals else 0),
                8 + 1 + (24 if normals else 0) + 4)
    row("shade reference", lambda: sc.shade_reference_dev(prim.data_ptr(), ao.data_ptr(), px, rgba.data_ptr()), 16 + 4)
    row("shade counts", lambda: sc.shade_ao_counts_dev(cnt.data_ptr(), n, px, rgba.data_ptr()), 1 + 4)
    row("shade term", lambda: sc.shade_ao_term_dev(term.data_ptr(), px, rgba.data_ptr()), 4 + 4)
    t = term.cpu().numpy().view(T.AO_TERM_DTYPE)
    say("the last filter's terms (r=4 without normals): mean accepted pixels per surface pixel %.1f of 81"
        % float(t["samples"][t["samples"] > 0].mean() / n))

    def wall(fn, reps=9):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    def host_image():
        p, a, _ = sc.trace_primary_ao(view, w, h, sem=sem, frame=0, ao_eps=eps)
        t0 = time.perf_counter()
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            col = np.where(p["t"] < 3.4028234663852886e38, np.where(a["t"] < 3.4028234663852886e38, a["t"] / (np.float32(1) + a["t"]), np.float32(1)),
                           np.float32(1) / p["t"]).astype(np.float32)
            img = (np.power(col, np.float32(2.2)) * np.float32(255)).astype(np.uint8)
        host_image.shade_ms.append((time.perf_counter() - t0) * 1e3)
        return img
    host_image.shade_ms = []

    say("\nwall-clock time of the host forms, median of 9 calls (ms)")
    say("trx_render_image, reference image (n_samples 0)            %.3f" % wall(lambda: sc.render_image(view, w, h, sem=sem, ao_eps=eps)))
    say("trx_trace_primary_ao + the host's shading of its records   %.3f (of which the numpy shading %.3f)"
        % (wall(host_image), statistics.median(host_image.shade_ms)))
    say("trx_render_image, 4 samples, unfiltered                    %.3f"
        % wall(lambda: sc.render_image(view, w, h, sem=sem, n_samples=n, ao_eps=eps)))
    say("trx_render_image, 4 samples, filter r=2 with normals       %.3f"
        % wall(lambda: sc.render_image(view, w, h, sem=sem, n_samples=n, ao_eps=eps, filter_radius=2)))
    say("trx_trace_ao_visibility (counts back, no image)            %.3f"
        % wall(lambda: sc.trace_ao_visibility(view, w, h, n, float("inf"), sem=sem, ao_eps=eps)))
    sc.check()
    sc.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
