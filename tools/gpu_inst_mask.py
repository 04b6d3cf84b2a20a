"""Instance masks (trx_trace_*_masked*): what a masked pass costs next to the unmasked one.

    W=3840 H=2160 python tools/gpu_inst_mask.py [rounds]

The san-miguel-class two-level scene (TLAS), its primary frame and 1 M hemisphere rays (tools/prof_config.py), semantics
TRX_SEM_CPU.  Per round a fresh child process times, in batches of back-to-back launches (one hipEvent pair per batch, as
tools/gpu_ab_procs.py does), three forms of each pass: unmasked (trx_trace_primary_dev / trx_trace_rays_dev), masked with
an all-visible table (every mask 0xFF, ray mask 0xFF) and masked with every second TLAS primitive hidden (masks
alternating 0x01 / 0x02, ray mask 0x02).  Printed: per form the median over rounds of each child's median batch
(ms per launch), with the spread over rounds, and the fraction of records that hit."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import tray_racing_amd as T
    from tools.prof_config import hemisphere_rays
    w, h = int(os.environ.get("W", "3840")), int(os.environ.get("H", "2160"))
    sem = T.SEM_CPU
    verts, counts = T.gen_scene("san_miguel", 0, 1)
    flat = T.flat_build(verts, counts, use_tlas=True)
    eye, look, fov = T.scene_camera("san_miguel")
    view = T.view_from_camera(eye, look, fov, w, h)
    sc = T.Scene(flat)
    n_inst = flat.instance_offsets.size
    prim = torch.zeros(w * h, dtype=torch.int64, device="cuda")
    rays = hemisphere_rays(flat, None, eye, 1 << 20, 7)
    d_rays = torch.from_numpy(rays.view("u1").copy()).cuda()
    hits = torch.zeros(len(rays), dtype=torch.int64, device="cuda")

    def batches(fn, n_batches=6, per=10, warm=40):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(n_batches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / per)
        return statistics.median(ts)

    def hit_frac(t):
        return float(((t.cpu().numpy().view(np.uint64) >> np.uint64(32)) != 0xFFFFFFFF).mean())   # (prim: the upper word)

    half = np.where(np.arange(n_inst) % 2 == 0, 0x01, 0x02).astype(np.uint8)
    forms = [("unmasked", None, 0), ("masked, all visible", np.full(n_inst, 0xFF, dtype=np.uint8), 0xFF),
             ("masked, half hidden", half, 0x02)]
    out = {"n_inst": n_inst}
    for name, table, rm in forms:
        sc.set_instance_masks(table)
        if table is None:
            p = batches(lambda: sc.trace_primary_dev(view, w, h, prim.data_ptr(), sem=sem), warm=140)
            fp = hit_frac(prim)
            r = batches(lambda: sc.trace_rays_dev(d_rays.data_ptr(), len(rays), hits.data_ptr(), sem=sem))
        else:
            p = batches(lambda: sc.trace_primary_masked_dev(view, w, h, prim.data_ptr(), rm, sem=sem), warm=140)
            fp = hit_frac(prim)
            r = batches(lambda: sc.trace_rays_masked_dev(d_rays.data_ptr(), len(rays), hits.data_ptr(), rm, sem=sem))
        out[name] = {"primary": p, "rays": r, "primary_hits": fp, "rays_hits": hit_frac(hits)}
    sc.close()
    print("MASK_CHILD " + json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child()
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    res = []
    for r in range(rounds):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=900)
        line = [x for x in p.stdout.splitlines() if x.startswith("MASK_CHILD ")]
        if p.returncode or not line:
            print("child failed: %s" % p.stderr[-600:], flush=True)
            return 1
        res.append(json.loads(line[0][11:]))
        print("round %d " % r + json.dumps(res[-1]), flush=True)
    print("\nsan-miguel-class two-level scene, %d TLAS primitives, %sx%s: median over %d processes [min .. max] of each "
          "process's median batch (ms per launch)" % (res[0]["n_inst"], os.environ.get("W", "3840"), os.environ.get("H", "2160"), rounds))
    for name in ("unmasked", "masked, all visible", "masked, half hidden"):
        row = []
        for key in ("primary", "rays"):
            v = [x[name][key] for x in res]
            row.append("%s %.4f [%.4f .. %.4f] (%.0f %% hits)" % (key, statistics.median(v), min(v), max(v), 100 * res[0][name][key + "_hits"]))
        print("%-22s %s" % (name, "   ".join(row)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
