"""The textured albedo: what trx_surface_albedo_dev costs beside the attribute pass and the material compose,
and what the textured indirect pass costs beside trx_trace_indirect_rgb_dev.

    python tools/gpu_textures.py [reps] > profiles/texture_pass.log

Two frames, in one fresh process: the bistro-class and the hairball-class stand-ins at 1920x1080, semantics TRX_SEM_CPU, the
stand-in materials, the stand-in texcoords (box mapping) and the stand-in texture (a 64 x 64 bilinear checker on material 0).
Per frame the primary trace runs once; then
  * the attribute pass, the albedo pass and the material compose are enqueued back to back on one stream, `reps` times (default
    50), each launch timed with its own hipEvent pair - and the whole round a second time, so the log carries the attribute
    pass's own run-to-run spread;
  * trx_trace_indirect_rgb_dev and trx_trace_indirect_rgb_textured_dev (4 samples, one point light) alternate, `reps / 5` times,
    dense and sparse at stride 2, again in two rounds: the untextured pass's spread is the yardstick for the difference.
Min / median throughout, and the share of records that sampled a texture."""
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


def timed(passes, reps):
    """Back-to-back launches of `passes` on the current stream, `reps` times; (min, median) ms per pass."""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(passes) + 1)] for _ in range(reps)]
    for _ in range(2):     # warm-up (code loaded, scratch allocated)
        for p in passes:
            p()
    torch.cuda.synchronize()
    for row in ev:
        row[0].record()
        for k, p in enumerate(passes):
            p()
            row[k + 1].record()
    torch.cuda.synchronize()
    out = []
    for k in range(len(passes)):
        t = [row[k].elapsed_time(row[k + 1]) for row in ev]
        out.append((min(t), float(np.median(t))))
    return out


def frame(name, w, h, reps):
    verts, counts = T.gen_scene(name, 0, 1)
    flat = T.flat_build(verts, counts)
    eye, look, fov = T.scene_camera(name)
    view = T.view_from_camera(eye, look, fov, w, h)
    sc = T.Scene(flat)
    mats, idx = T.standin_materials(name, verts, counts)
    sc.set_materials(mats, idx[flat.tri_source])
    sc.set_texcoords(T.standin_texcoords(name, verts)[flat.tri_source])
    descs, texels, mat_tex = T.standin_textures(name, mats.shape[0])
    sc.set_textures(descs, texels, mat_tex)
    lib, n = T.load(), w * h
    stream = torch.cuda.current_stream().cuda_stream
    d_hits, d_inst = torch.empty(n * 8, dtype=torch.uint8, device="cuda"), torch.empty(n * 4, dtype=torch.uint8, device="cuda")
    d_attr, d_alb = torch.empty(n * 24, dtype=torch.uint8, device="cuda"), torch.empty(3 * n * 4, dtype=torch.uint8, device="cuda")
    d_E, d_col = torch.zeros(n * 4, dtype=torch.uint8, device="cuda"), torch.empty(3 * n * 4, dtype=torch.uint8, device="cuda")
    d_ind = torch.empty(3 * n * 4, dtype=torch.uint8, device="cuda")
    L.check(lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, L.Shard(0, 1, 0, 0), SEM, C.c_void_p(d_hits.data_ptr()),
                                           C.c_void_p(d_inst.data_ptr()), None))
    what = "%s %dx%d (%d tris)" % (name, w, h, flat.n_tris)

    def attr():
        sc.hit_attributes_primary_dev(view, w, h, d_hits.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr(), stream=stream)

    def albedo():
        sc.surface_albedo_dev(d_hits.data_ptr(), d_attr.data_ptr(), n, d_alb.data_ptr(), stream=stream)

    def compose():
        sc.material_compose_dev(d_hits.data_ptr(), d_E.data_ptr(), n, d_col.data_ptr(), stream=stream)

    def albedo_compose():
        sc.albedo_compose_dev(d_hits.data_ptr(), d_alb.data_ptr(), d_E.data_ptr(), n, d_col.data_ptr(), stream=stream)

    for round_ in (1, 2):
        (a, s, m, c) = timed([attr, albedo, compose, albedo_compose], reps)
        print("%-36s round %d: attributes %.4f / %.4f | surface albedo %.4f / %.4f | material compose %.4f / %.4f | albedo compose %.4f / %.4f ms "
              "(min / median); albedo = %.2f x the attribute pass" % (what, round_, *a, *s, *m, *c, s[0] / a[0]), flush=True)
    light = [T.light(T.LIGHT_POINT, tuple(float(x) for x in look))]
    kw = dict(n_samples=4, sem=SEM, bounce_eps=0.01, shadow_eps=0.01, d_primary_inst=d_inst.data_ptr(), stream=stream)
    for stride in (1, 2):
        def plain():
            if stride == 1:
                sc.trace_indirect_rgb_dev(view, w, h, light, d_hits.data_ptr(), d_ind.data_ptr(), **kw)
            else:
                sc.trace_indirect_rgb_sparse_dev(view, w, h, stride, 0, light, d_hits.data_ptr(), d_ind.data_ptr(), **kw)

        def textured():
            sc.trace_indirect_rgb_textured_dev(view, w, h, light, d_hits.data_ptr(), d_ind.data_ptr(), stride=stride, phase=0, **kw)

        for round_ in (1, 2):
            (p, t) = timed([plain, textured], max(reps // 5, 3))
            print("%-36s round %d: indirect rgb at stride %d %.3f / %.3f ms | textured %.3f / %.3f ms (min / median) = %.3f x" % (
                what, round_, stride, *p, *t, t[0] / p[0]), flush=True)
    sc.check()
    hits = d_hits.cpu().numpy().view(T.HIT_DTYPE)
    hit = hits["prim"] != T.MISS_PRIM
    textured_share = (mat_tex[idx[flat.tri_source][hits["prim"][hit]]] != T.NO_TEXTURE).mean() if hit.any() else 0.0
    print("%-36s %d records, %.0f %% hits, %.0f %% of the hits on a textured material" % ("", n, 100.0 * hit.mean(), 100.0 * textured_share), flush=True)
    sc.close()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    lib_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tray_racing_amd", "libtrx.so")
    with open(lib_path, "rb") as f:
        print("library %s, device %s, %d reps" % (hashlib.sha256(f.read()).hexdigest()[:16], torch.cuda.get_device_name(0), reps), flush=True)
    frame("bistro", 1920, 1080, reps)
    frame("hairball", 1920, 1080, reps)


if __name__ == "__main__":
    main()
