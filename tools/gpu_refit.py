"""BVH refit on the device (trx_scene_refit / trx_scene_refit_dev): what it costs and what it costs the tree.

    python tools/gpu_refit.py [bistro] [san_miguel:tlas] ...

Per scene (BASELINE.json configs[2] bistro-class and configs[4] san-miguel-class --tlas stand-ins by default, built with the
device preset pipeline): the refit's height-level count, the device refit in ms from a torch tensor (trx_scene_refit_dev)
and from host memory (trx_scene_refit), min and median of 25 hipEvent-timed calls, the host twin's seconds
(trx_refit_nodes), and node visits per primary ray (trx_count_primary) for the original build, the same tree refitted
to a deformed copy of the geometry, and a fresh build of the deformed geometry."""
import hashlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import tray_racing_amd as T  # noqa: E402

W, H = 1920, 1080


def deform(v, seed=1):
    """A smooth wave through the scene plus a small per-vertex jitter (skinning / cloth-like motion)."""
    rng = np.random.default_rng(seed)
    p = v.astype(np.float64).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    size = float(np.linalg.norm(hi - lo))
    q = p.copy()
    q[:, 1] += 0.004 * size * np.sin(2 * np.pi * (p[:, 0] - lo[0]) / (0.1 * size))
    q += rng.normal(scale=0.0005 * size, size=q.shape)
    return q.reshape(-1, 9).astype(np.float32)


def timed(fn, reps=25):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return min(ms), float(np.median(ms))


def visits(sc, view):
    st = sc.count_primary(view, W, H, sem=3)
    return st.n_node / max(st.n_rays, 1)


def run(spec):
    name, _, kind = spec.partition(":")
    tlas = kind == "tlas"
    verts, counts = T.gen_scene(name, 0, 1)
    flat = T.flat_build_preset_device(verts, counts, device=0, use_tlas=tlas)
    eye, look, fov = T.scene_camera(name)
    view = T.view_from_camera(eye, look, fov, W, H)
    sc = T.Scene(flat)
    v_orig = visits(sc, view)
    moved = deform(flat.tri_verts)
    d_moved = torch.from_numpy(moved).cuda()
    sc.refit(d_moved)                                               # first call derives the schedule
    dev_min, dev_med = timed(lambda: sc.refit(d_moved))
    host_min, host_med = timed(lambda: sc.refit(moved))
    t = time.perf_counter()
    twin = T.refit_nodes(flat, moved)
    twin_s = time.perf_counter() - t
    same = bool(np.array_equal(twin, sc.read_nodes()))
    v_refit = visits(sc, view)
    n_levels = sc.info()["refit_levels"]                          # the schedule the library derived and cached
    sc.close()
    # a fresh build of the deformed geometry (object order: the permuted records map back through tri_source)
    obj = np.empty_like(verts)
    obj[flat.tri_source] = moved
    fresh = T.flat_build_preset_device(obj, counts, device=0, use_tlas=tlas)
    fs = T.Scene(fresh)
    v_fresh = visits(fs, view)
    fs.close()
    print("%s%s: %d tris, %d nodes, %d height levels | refit_dev %.3f / %.3f ms (min / median of 25), refit from host memory "
          "%.3f / %.3f ms, host twin %.3f s (device bytes equal: %s) | node visits per primary ray (%dx%d, sem 3): "
          "build %.2f, deformed + refit %.2f, fresh build of the deformed geometry %.2f" % (
              name, " --tlas" if tlas else "", flat.n_tris, flat.n_nodes, n_levels, dev_min, dev_med, host_min, host_med,
              twin_s, same, W, H, v_orig, v_refit, v_fresh), flush=True)


def main():
    lib_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tray_racing_amd", "libtrx.so")
    with open(lib_path, "rb") as f:
        print("library %s, device %s" % (hashlib.sha256(f.read()).hexdigest()[:16], torch.cuda.get_device_name(0)), flush=True)
    for spec in sys.argv[1:] or ["bistro", "san_miguel:tlas"]:
        run(spec)


if __name__ == "__main__":
    main()
