"""BVH refit on the GPU (trx_scene_refit / trx_scene_refit_dev): the device's node bytes equal the host twin's
(trx_refit_nodes), and every frame traced after a refit is the oracle's over the refitted nodes and the new vertices,
bit for bit."""
import threading
import time

import numpy as np
import pytest

from helpers import ALL_SEMS, aimed_rays, assert_hits_equal, instanced_scene, random_affine, random_rays, w2o_rows

pytestmark = pytest.mark.gpu

W, H = 160, 96


def _deformations(flat, seed):
    rng = np.random.default_rng(seed)
    v = flat.tri_verts.astype(np.float64)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    size = float(np.linalg.norm(hi - lo))
    jitter = v + rng.normal(scale=0.01 * size, size=v.shape)
    M = np.asarray(random_affine(rng, 0.5, 2.0, spread=size), dtype=np.float64).reshape(4, 4).T
    affine = (v.reshape(-1, 3) @ M[:3, :3].T + M[:3, 3]).reshape(-1, 9)
    moved = v.copy()
    sel = flat.tri_source < flat.tri_source.max() // 3          # the first objects' triangles, far outside the old box
    moved[sel] += np.tile(np.array([3.0, -2.0, 1.5]) * size, 3)
    moved = moved.astype(np.float32)
    # (kind, new vertices, what the camera of the frame checks looks at: the moved objects for "moved")
    return [("jitter", jitter.astype(np.float32), None), ("affine", affine.astype(np.float32), None), ("moved", moved, moved[sel])]


def _view(trx, verts):
    """A camera outside the box of `verts`, looking at its centre."""
    p = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    c = 0.5 * (lo + hi)
    d = np.array([0.9, 0.6, 1.4])
    eye = c + 0.4 * float(np.linalg.norm(hi - lo)) * d / np.linalg.norm(d)
    return trx.view_from_camera(eye.astype(np.float32), c.astype(np.float32), 60.0, W, H)


def _world(flat, o2w):
    """World-space triangles of every instance (float64 transform, rounded once)."""
    starts = sorted(set(int(x) for x in flat.instance_offsets))
    bts, out = flat.blas_tri_start, []
    for k in range(flat.instance_offsets.size):
        b = starts.index(int(flat.instance_offsets[k]))
        tv = flat.tri_verts[bts[b]:bts[b + 1]].astype(np.float64).reshape(-1, 3)
        M = np.asarray(o2w[k], dtype=np.float64).reshape(4, 4).T
        out.append((tv @ M[:3, :3].T + M[:3, 3]).reshape(-1, 9).astype(np.float32))
    return np.concatenate(out)


def _oracle(orc, sc, flat, verts):
    """The oracle over what the device now holds: read_nodes() and the new vertices, the kernels' instance rows."""
    w2o = sc.instance_world_to_object() if flat.instance_transforms is not None else None
    return orc.Scene(sc.read_nodes(), verts, flat.instance_offsets, flat.tlas_start, instance_w2o=w2o,
                     instance_entry=flat.instance_entry)


def _frames_match(trx, orc, sc, flat, verts, what, sems=(0, 3), look=None, min_hits=W * H // 20):
    osc = _oracle(orc, sc, flat, verts)
    view = _view(trx, verts if look is None else look)
    ov = orc.view_from_bytes(view)
    for sem in sems:
        prim, pinst, ao, ainst, _ = sc.trace_primary_ao_inst(view, W, H, sem=sem, frame=1, ao_eps=0.01)
        want, winst, st = osc.trace_primary_inst(ov, W, H, sem=sem)
        assert st.n_hits >= min_hits, what
        assert_hits_equal(prim, want, "%s primary sem %d" % (what, sem))
        want_ao, _, _ = osc.trace_ao_inst(ov, W, H, want, winst, sem=sem, frame=1, ao_eps=0.01)
        assert_hits_equal(ao, want_ao, "%s AO sem %d" % (what, sem))
    nflat = type("F", (), {"tri_verts": verts})
    rays = np.concatenate([random_rays(trx, nflat, 2000, 3), aimed_rays(trx, verts, 2000, 4)])
    for sem in ALL_SEMS:
        got, _ = sc.trace_rays(rays, sem=sem)
        want, _ = osc.trace_rays(rays, sem=sem)
        assert_hits_equal(got, want, "%s rays sem %d" % (what, sem))
        assert (want["prim"] != 0xFFFFFFFF).sum() > 500, what
    flags, _ = sc.trace_occluded(rays, sem=3)
    want, _ = osc.trace_rays(rays, sem=3)
    assert np.array_equal(flags.astype(bool), want["prim"] != 0xFFFFFFFF), what


def _scenes(trx):
    v, c = trx.gen_scene("bistro", 20000, 1)
    yield "bistro", trx.flat_build(v, c), None
    v, c = trx.gen_scene("kitchen", 20000, 1)
    yield "kitchen --tlas (re-braided)", trx.flat_build(v, c, use_tlas=True), None
    flat, o2w, *_ = instanced_scene(trx)
    yield "instanced", flat, o2w


def test_device_refit_equals_host_twin_and_frames_follow(trx, orc):
    import torch
    side = torch.cuda.Stream()
    for name, flat, o2w in _scenes(trx):
        sc = trx.Scene(flat)
        view = _view(trx, flat.tri_verts)
        sc.trace_primary_ao_inst(view, W, H, sem=3)                    # a tile order learnt before the refit
        sc.refit(flat.tri_verts)                                      # identity, host memory
        twin = trx.refit_nodes(flat, flat.tri_verts, o2w)
        assert np.array_equal(sc.read_nodes(), twin), name
        if flat.instance_entry is None:
            assert np.array_equal(twin, flat.nodes), name            # the build's own bytes
        for kind, v, look in _deformations(flat, 5):
            twin = trx.refit_nodes(flat, v, o2w)
            with torch.cuda.stream(side):                             # device memory, a non-default stream
                sc.refit(torch.from_numpy(v).cuda())
            assert np.array_equal(sc.read_nodes(), twin), "%s %s (device)" % (name, kind)
            _frames_match(trx, orc, sc, flat, v, "%s %s" % (name, kind), look=look)
            sc.refit(flat.tri_verts)
            sc.refit(v)                                               # host memory
            assert np.array_equal(sc.read_nodes(), twin), "%s %s (host)" % (name, kind)
        sc.close()


def test_moved_instances(trx, orc):
    flat, o2w, *_ = instanced_scene(trx)
    sc = trx.Scene(flat)
    rng = np.random.default_rng(23)
    new = np.stack([random_affine(rng, spread=6.0) for _ in range(o2w.shape[0])])
    sc.trace_primary_ao_inst(_view(trx, flat.tri_verts), W, H, sem=3)
    sc.set_instance_transforms(new)
    sc.refit(flat.tri_verts)
    assert np.array_equal(sc.read_nodes(), trx.refit_nodes(flat, flat.tri_verts, new))
    assert np.array_equal(sc.instance_world_to_object(), np.stack([w2o_rows(m) for m in new]))
    osc = _oracle(orc, sc, flat, flat.tri_verts)
    view = _view(trx, _world(flat, new))
    ov = orc.view_from_bytes(view)
    for sem in (0, 3):
        prim, pinst, ao, ainst, _ = sc.trace_primary_ao_inst(view, W, H, sem=sem, frame=2, ao_eps=0.01)
        want, winst, st = osc.trace_primary_inst(ov, W, H, sem=sem)
        assert st.n_hits > W * H // 20
        assert_hits_equal(prim, want, "moved instances primary sem %d" % sem)
        assert np.array_equal(pinst, winst)
        want_ao, wainst, _ = osc.trace_ao_inst(ov, W, H, want, winst, sem=sem, frame=2, ao_eps=0.01)
        assert_hits_equal(ao, want_ao, "moved instances AO sem %d" % sem)
    sc.close()


def _created_info(trx, flat, nodes, verts):
    """exp_exact / scene_diag of a scene CREATED from `nodes` and `verts`: what trx_scene_create derives from the bytes."""
    f = trx.FlatScene(nodes, verts, flat.instance_offsets, flat.tlas_start, flat.tri_source, flat.blas_tri_start,
                      instance_transforms=flat.instance_transforms, instance_entry=flat.instance_entry)
    sc = trx.Scene(f)
    info = sc.info()
    sc.close()
    return info


def test_launch_words_are_recomputed(trx, orc):
    """trx_scene_create derives exp_exact (which exact shortcuts the node test may take: 2 needs every node origin +0 or
    2^-36 <= |p| <= 2^59) and the scene diagonal (camera-cut detection) from the node bytes; a refit must derive them again,
    as a scene created from its nodes would.  Shifted so that the root's origin lands at x ~ 1e-12, the bistro-class scene
    drops from 2 to 1; scaled, both scenes get another diagonal.  (The encoder's steps are never below 2^-74, exponent byte
    53, so a refit cannot reach exp_exact 0, which needs bytes 1..20.)"""
    v, c = trx.gen_scene("bistro", 20000, 3)
    flat = trx.flat_build(v, c)
    shifted = flat.tri_verts.astype(np.float64)
    shifted[:, 0::3] += 1e-12 - shifted[:, 0::3].min()
    shifted = shifted.astype(np.float32)
    k, kc = trx.gen_scene("kitchen", 20000, 3)
    kflat = trx.flat_build(k, kc, use_tlas=True)
    cases = [(flat, [("shifted", shifted), ("scaled", flat.tri_verts * np.float32(8.0)), ("back", flat.tri_verts)]),
             (kflat, [("scaled", kflat.tri_verts * np.float32(0.25)), ("back", kflat.tri_verts)])]
    for f, steps in cases:
        sc = trx.Scene(f)
        before = sc.info()
        assert before["exp_exact"] == 2 and before["refit_levels"] == 0
        for what, nv in steps:
            sc.refit(nv)
            got, want = sc.info(), _created_info(trx, f, sc.read_nodes(), nv)
            assert got["exp_exact"] == want["exp_exact"] and got["scene_diag"] == want["scene_diag"], (what, got, want)
            assert got["refit_levels"] > 2, what
            if what == "shifted":
                root_px = sc.read_nodes()[f.tlas_start, 0:1].view(np.float32)[0]
                assert 0.0 < root_px < 2.0 ** -36 and got["exp_exact"] == 1
                _frames_match(trx, orc, sc, f, nv, "root origin at 1e-12")
            if what == "scaled":
                assert got["scene_diag"] != before["scene_diag"]
            if what == "back":
                assert got["exp_exact"] == before["exp_exact"] and got["scene_diag"] == before["scene_diag"]
        sc.close()


def test_round_trip_restores_the_scene(trx):
    flat, o2w, *_ = instanced_scene(trx, seed=5)
    ref = trx.Scene(flat)
    sc = trx.Scene(flat)
    view = _view(trx, flat.tri_verts)
    want, _, want_ao, _, _ = ref.trace_primary_ao_inst(view, W, H, sem=3)
    sc.refit(_deformations(flat, 9)[0][1])
    sc.refit(flat.tri_verts)
    got, _, got_ao, _, _ = sc.trace_primary_ao_inst(view, W, H, sem=3)
    assert np.array_equal(sc.read_nodes(), ref.read_nodes())
    assert_hits_equal(got, want, "round trip primary")
    assert_hits_equal(got_ao, want_ao, "round trip AO")
    sc.close()
    ref.close()


def test_refit_beside_the_ray_service(trx, orc):
    """8 threads in trx_traverse1 for ~2 s while another thread refits twice: every call returns, and every answer to a
    call made after the second refit returned is the oracle's on the final geometry."""
    v, c = trx.gen_scene("bistro", 20000, 4)
    flat = trx.flat_build(v, c)
    sc = trx.Scene(flat)
    final = _deformations(flat, 11)[1][1]
    osc = orc.Scene(trx.refit_nodes(flat, final), final)
    rays = np.concatenate([aimed_rays(trx, final, 200, 12), aimed_rays(trx, flat.tri_verts, 200, 13)])
    want, _ = osc.trace_rays(rays, sem=3)
    second_done = threading.Event()
    errors, checked = [], [0] * 8
    stop_at = time.monotonic() + 2.0

    def caller(k):
        try:
            i = k
            while time.monotonic() < stop_at or not second_done.is_set():
                after = second_done.is_set()
                r = rays[i % rays.size]
                hit = sc.traverse(r["origin"], r["direction"], float(r["tmin"]), float(r["tmax"]), sem=3)
                if after:
                    prim = 0xFFFFFFFF if hit.primitive_id == 0xFFFFFFFF else int(flat.blas_tri_start[hit.geometry_id]) + hit.primitive_id
                    w = want[i % rays.size]
                    if np.float32(hit.t).view(np.uint32) != np.float32(w["t"]).view(np.uint32) or prim != int(w["prim"]):
                        errors.append((k, i, hit.t, prim, float(w["t"]), int(w["prim"])))
                    checked[k] += 1
                i += 8
                if time.monotonic() > stop_at + 30.0:
                    errors.append((k, "did not finish"))
                    return
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=caller, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    time.sleep(0.3)
    sc.refit(_deformations(flat, 10)[0][1])
    time.sleep(0.3)
    sc.refit(final)
    second_done.set()
    for t in threads:
        t.join(timeout=60.0)
    assert not any(t.is_alive() for t in threads), "a trx_traverse1 caller did not return"
    assert not errors, errors[:5]
    assert sum(checked) > 100
    sc.close()


def test_refused_refit_leaves_the_scene_unchanged(trx):
    import torch
    v, c = trx.gen_scene("soup", 3000, 5)
    flat = trx.flat_build(v, c)
    sc = trx.Scene(flat)
    view = _view(trx, flat.tri_verts)
    moved = _deformations(flat, 6)[0][1]
    sc.refit(moved)
    nodes = sc.read_nodes()
    want, _ = sc.trace_primary(view, W, H, sem=3)
    bad = moved.copy()
    bad[17, 4] = np.nan
    for arg in (bad, torch.from_numpy(bad).cuda(), moved[:-1], torch.from_numpy(moved[:-1]).cuda()):
        with pytest.raises(trx.TrxError) as e:
            sc.refit(arg)
        assert e.value.code == trx._lib.TRX_ERR_INVALID
    lib = trx.load()
    assert lib.trx_scene_refit(sc.handle, None, flat.n_tris) == trx._lib.TRX_ERR_INVALID
    assert lib.trx_scene_refit_dev(sc.handle, None, flat.n_tris, None) == trx._lib.TRX_ERR_INVALID
    assert np.array_equal(sc.read_nodes(), nodes)
    got, _ = sc.trace_primary(view, W, H, sem=3)
    assert_hits_equal(got, want, "after refused refits")
    # vertices that do not live on the scene's device are refused before anything reads them: a tensor of another
    # device (by the binding), pinned host memory (by the library)
    dev = lib.trx_scene_device(sc.handle)
    other = type("OtherDevice", (), {"is_cuda": True, "dtype": torch.float32, "device": torch.device("cuda", dev + 1),
                                     "numel": lambda self: flat.n_tris * 9, "data_ptr": lambda self: 0})()
    with pytest.raises(trx.TrxError) as e:
        sc.refit(other)
    assert e.value.code == trx._lib.TRX_ERR_INVALID
    pinned = torch.from_numpy(moved).pin_memory()
    assert lib.trx_scene_refit_dev(sc.handle, pinned.data_ptr(), flat.n_tris, None) == trx._lib.TRX_ERR_INVALID
    assert b"device memory" in lib.trx_last_error()
    assert np.array_equal(sc.read_nodes(), nodes)
    f16 = trx.Scene(flat, tri_format=trx.TRI_F16_24, tri_bytes=trx.pack_tris_f16(flat.tri_verts))
    with pytest.raises(trx.TrxError):
        f16.refit(flat.tri_verts)
    f16.close()
    sc.close()


def test_bistro_class_refit_time(trx, orc):
    """BASELINE.json configs[2]'s stand-in (3.9 M triangles): a loose sanity bound on the device refit, not the target
    (tools/gpu_refit.py measures it) - and the only size at which the grid-stride loops of k_refit_tris (8192 x 256 threads)
    and k_refit_stats (1024 x 256) wrap, so the result is checked too: the nodes against the host twin, the launch words
    against a created scene's, and - there is no read-back of the triangle records - rays aimed only at records the second
    pass of k_refit_tris wrote against the oracle."""
    import torch
    v, c = trx.gen_scene("bistro", 0, 1)
    flat = trx.flat_build_preset_device(v, c, device=0)
    sc = trx.Scene(flat)
    moved = _deformations(flat, 1)[0][1]
    d = torch.from_numpy(moved).cuda()
    sc.refit(d)                                                       # schedule derived on the first refit
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(5):
        t0.record()
        sc.refit(d)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    assert min(ms) < 5.0, ms
    assert flat.n_tris > 8192 * 256 and flat.n_nodes > 1024 * 256
    nodes = sc.read_nodes()
    assert np.array_equal(nodes, trx.refit_nodes(flat, moved))
    got, want = sc.info(), _created_info(trx, flat, nodes, moved)
    assert got["exp_exact"] == want["exp_exact"] and got["scene_diag"] == want["scene_diag"], (got, want)
    rng = np.random.default_rng(21)
    tri = moved[rng.integers(8192 * 256, flat.n_tris, size=4000)].astype(np.float64).reshape(-1, 3, 3)
    target = (tri * rng.dirichlet([1, 1, 1], size=4000)[:, :, None]).sum(1)
    lo, hi = moved.reshape(-1, 3).min(0).astype(np.float64), moved.reshape(-1, 3).max(0).astype(np.float64)
    origin = rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), size=(4000, 3))
    rays = np.zeros(4000, dtype=trx.RAY_DTYPE)
    rays["origin"] = origin.astype(np.float32)
    rays["direction"] = ((target - origin) / np.linalg.norm(target - origin, axis=1, keepdims=True)).astype(np.float32)
    rays["tmax"] = 3.4028234663852886e38
    osc = orc.Scene(nodes, moved)
    for sem in (0, 3):
        hits, _ = sc.trace_rays(rays, sem=sem)
        want_hits, _ = osc.trace_rays(rays, sem=sem)
        assert_hits_equal(hits, want_hits, "rays at records of the second pass, sem %d" % sem)
        second = (want_hits["prim"] >= 8192 * 256) & (want_hits["prim"] < flat.n_tris)
        assert second.sum() > 400      # (the other rays stop at nearer geometry)
    sc.close()
