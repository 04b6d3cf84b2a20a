"""Hit attributes (trx_hit_attributes_*): what the post-pass costs next to the trace it follows.

    python tools/gpu_hit_attr.py [reps]

Three workloads, in one fresh process: the bistro-class 1920x1080 primary frame, 2 M random rays over the bistro-class
scene, and the san-miguel-class two-level 3840x2160 frame.  Per workload the trace (trx_trace_*_inst_dev) and then the
attribute pass over its records are enqueued back to back on one stream, `reps` times (default 50); each launch is timed
with its own hipEvent pair (torch.cuda.Event), and min / median per pass are printed, with the bytes the pass requests
per second at its minimum (8 B hit + 4 B instance id + 48 B triangle + 24 B written per record, + 32 B ray for explicit rays).
Semantics TRX_SEM_CPU."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import tray_racing_amd as T  # noqa: E402
from tray_racing_amd import _lib as L  # noqa: E402

SEM = T.SEM_CPU


def timed_pair(trace, attr, reps):
    """Back-to-back trace + attribute launches on the current stream; per-launch event times."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(reps)]
    for _ in range(3):     # warm-up (tile orders learnt, code loaded)
        trace()
        attr()
    torch.cuda.synchronize()
    for a, b, c in ev:
        a.record()
        trace()
        b.record()
        attr()
        c.record()
    torch.cuda.synchronize()
    tt = [a.elapsed_time(b) for a, b, _ in ev]
    ta = [b.elapsed_time(c) for _, b, c in ev]
    return (min(tt), float(np.median(tt))), (min(ta), float(np.median(ta)))


def report(what, n, hit_frac, per_record, times):
    (tmin, tmed), (amin, amed) = times
    print("%-52s trace %.3f / %.3f ms | attributes %.4f / %.4f ms (min / median) = %.1f %% of the trace | %d records, "
          "%.0f %% hits, %.0f GB/s requested at %d B per record (coherent gathers are served from the caches)" % (
              what, tmin, tmed, amin, amed, 100.0 * amin / tmin, n, 100.0 * hit_frac, n * per_record / (amin * 1e-3) / 1e9,
              per_record), flush=True)

def primary(name, tris, w, h, tlas, reps):
    verts, counts = T.gen_scene(name, tris, 1)
    flat = T.flat_build(verts, counts, use_tlas=tlas)
    eye, look, fov = T.scene_camera(name)
    view = T.view_from_camera(eye, look, fov, w, h)
    sc = T.Scene(flat)
    lib, n = T.load(), w * h
    d_hits = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    d_inst = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
    d_attr = torch.empty(n * 24, dtype=torch.uint8, device="cuda")
    S = L.Shard(0, 1, 0, 0)

    def trace():
        st = torch.cuda.current_stream().cuda_stream
        L.check(lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, S, SEM, C.c_void_p(d_hits.data_ptr()),
                                               C.c_void_p(d_inst.data_ptr()), C.c_void_p(st)))

    def attr():
        sc.hit_attributes_primary_dev(view, w, h, d_hits.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr(),
                                      stream=torch.cuda.current_stream().cuda_stream)

    times = timed_pair(trace, attr, reps)
    hits = d_hits.cpu().numpy().view(T.HIT_DTYPE)
    report("%s%s %dx%d primary (%d tris)" % (name, " --tlas" if tlas else "", w, h, flat.n_tris), n,
           float((hits["prim"] != T.MISS_PRIM).mean()), 84, times)
    sc.close()


def rays(name, tris, n, reps):
    verts, counts = T.gen_scene(name, tris, 1)
    flat = T.flat_build(verts, counts)
    sc = T.Scene(flat)
    lib = T.load()
    rng = np.random.default_rng(1)
    pts = flat.tri_verts.reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    r = np.zeros(n, dtype=T.RAY_DTYPE)
    r["origin"] = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    r["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    r["tmax"] = 3.4028234663852886e38
    d_rays = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
    d_hits = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    d_inst = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
    d_attr = torch.empty(n * 24, dtype=torch.uint8, device="cuda")

    def trace():
        st = torch.cuda.current_stream().cuda_stream
        L.check(lib.trx_trace_rays_inst_dev(sc.handle, C.c_void_p(d_rays.data_ptr()), n, SEM, C.c_void_p(d_hits.data_ptr()),
                                            C.c_void_p(d_inst.data_ptr()), C.c_void_p(st)))

    def attr():
        sc.hit_attributes_rays_dev(d_rays.data_ptr(), n, d_hits.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr(),
                                   stream=torch.cuda.current_stream().cuda_stream)

    times = timed_pair(trace, attr, reps)
    hits = d_hits.cpu().numpy().view(T.HIT_DTYPE)
    report("%s %d random rays (%d tris)" % (name, n, flat.n_tris), n, float((hits["prim"] != T.MISS_PRIM).mean()), 116, times)
    sc.close()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    lib_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tray_racing_amd", "libtrx.so")
    with open(lib_path, "rb") as f:
        print("library %s, device %s, %d reps" % (hashlib.sha256(f.read()).hexdigest()[:16], torch.cuda.get_device_name(0), reps),
              flush=True)
    primary("bistro", 0, 1920, 1080, False, reps)
    rays("bistro", 0, 2 * 1024 * 1024, reps)
    primary("san_miguel", 0, 3840, 2160, True, reps)


if __name__ == "__main__":
    main()
