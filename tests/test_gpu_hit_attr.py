"""Hit attributes on the GPU (trx_hit_attributes_rays_dev / _primary_dev, trx_trace_rays_attr): every record is the
numpy twin's (tests/hit_attr_twin.py) bit for bit on u, v and the normal, fed the device's own hits (which
tests/test_gpu_parity.py and test_gpu_instances.py hold bit-equal to the oracle); misses are all-zero records."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import ALL_SEMS, aimed_rays, golden_inputs, instanced_scene, random_rays
from hit_attr_twin import attr_bits, hit_attrs, primary_dirs, primary_origins, primary_pixels, tri_records

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 0xAB


@pytest.fixture(scope="module", autouse=True)
def need_gpu(trx):
    assert trx.load().trx_device_count() > 0, "no HIP device visible to libtrx.so"


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _buf(n, dtype, fill=SENTINEL):
    torch = _torch()
    return torch.full((max(n, 1) * np.dtype(dtype).itemsize,), fill, dtype=torch.uint8, device="cuda")


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _stream(stream):
    return stream.cuda_stream if stream is not None else _torch().cuda.current_stream().cuda_stream


def _rays_case(trx, sc, recs, rays, sem, w2o=None, stream=None, what=""):
    """Trace rays and their attributes on one stream, no host synchronisation in between; compare with the twin."""
    lib, n = trx.load(), rays.shape[0]
    d_rays, d_hits, d_inst, d_attr = _dev(rays), _buf(n, trx.HIT_DTYPE), _buf(n, np.uint32), _buf(n, trx.HIT_ATTR_DTYPE)
    st = _stream(stream)
    trx._lib.check(lib.trx_trace_rays_inst_dev(sc.handle, C.c_void_p(d_rays.data_ptr()), n, sem, C.c_void_p(d_hits.data_ptr()),
                                               C.c_void_p(d_inst.data_ptr()), C.c_void_p(st)))
    sc.hit_attributes_rays_dev(d_rays.data_ptr(), n, d_hits.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr(), stream=st)
    _torch().cuda.synchronize()
    hits, inst, attr = _host(d_hits, trx.HIT_DTYPE), _host(d_inst, np.uint32), _host(d_attr, trx.HIT_ATTR_DTYPE)
    want = hit_attrs(recs, rays["origin"], rays["direction"], hits["prim"], inst, w2o)
    bad = np.flatnonzero((attr_bits(attr) != attr_bits(want)).any(1))
    assert bad.size == 0, "%s sem %d: %d records differ (first %s: %s vs %s)" % (what, sem, bad.size, bad[:3], attr[bad[:1]], want[bad[:1]])
    return hits, inst, attr


def _primary_case(trx, sc, recs, view, w, h, sem, shard=(0, 1), layout=0, w2o=None, stream=None, what=""):
    lib = trx.load()
    S = trx._lib.Shard(shard[0], shard[1], layout, 0)
    n = w * h if layout == 0 else lib.trx_shard_tiles(w, h, S) * 64
    d_hits, d_inst, d_attr = _buf(n, trx.HIT_DTYPE), _buf(n, np.uint32), _buf(n, trx.HIT_ATTR_DTYPE)
    st = _stream(stream)
    trx._lib.check(lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, S, sem, C.c_void_p(d_hits.data_ptr()),
                                                  C.c_void_p(d_inst.data_ptr()), C.c_void_p(st)))
    sc.hit_attributes_primary_dev(view, w, h, d_hits.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr(),
                                  shard=(shard[0], shard[1], layout), stream=st)
    _torch().cuda.synchronize()
    hits, inst, attr = _host(d_hits, trx.HIT_DTYPE), _host(d_inst, np.uint32), _host(d_attr, trx.HIT_ATTR_DTYPE)
    rec, px, py = primary_pixels(w, h, shard, layout)
    want = hit_attrs(recs, primary_origins(view, rec.size), primary_dirs(view, w, h, px, py), hits["prim"][rec], inst[rec], w2o)
    got = attr[rec]
    bad = np.flatnonzero((attr_bits(got) != attr_bits(want)).any(1))
    assert bad.size == 0, "%s sem %d: %d records differ (first pixel %s)" % (what, sem, bad.size, (px[bad[:1]], py[bad[:1]]))
    others = np.ones(n, dtype=bool)
    others[rec] = False   # records of other shards' pixels (image layout) / outside the image (shard layout): untouched
    assert (attr.view(np.uint8).reshape(n, 24)[others] == SENTINEL).all(), what
    assert (hits["prim"][rec] != 0xFFFFFFFF).sum() > rec.size // 20, what
    return hits, attr


def _scene(trx, name, n, tlas=False):
    verts, counts = trx.gen_scene(name, n, 1)
    flat = trx.flat_build(verts, counts, use_tlas=tlas)
    eye, look, fov = trx.scene_camera(name)
    return flat, eye, look, fov


# ---- 1. explicit rays, every semantics word --------------------------------------------------------------------

@pytest.mark.parametrize("name,n", [("soup", 2500), ("cornell", 0), ("bistro", 150000)])
def test_explicit_rays_all_semantics(trx, name, n):
    flat, _, _, _ = _scene(trx, name, n)
    sc = trx.Scene(flat)
    recs = tri_records(flat.tri_verts)
    rays = np.concatenate([random_rays(trx, flat, 3000, 11, zero_dirs=True), aimed_rays(trx, flat.tri_verts, 3000, 12)])
    try:
        for sem in ALL_SEMS:
            hits, _, _ = _rays_case(trx, sc, recs, rays, sem, what=name)
            assert (hits["prim"] != 0xFFFFFFFF).sum() > 2000
        # zero rays: nothing to do, no error
        sc.hit_attributes_rays_dev(0, 0, 0, 0)
    finally:
        sc.close()


# ---- 2. primary frames: image layout, shards in both layouts, the full-size frame -------------------------------

@pytest.mark.parametrize("name,n,w,h", [("cornell", 0, 96, 64), ("soup", 2500, 100, 60)])
def test_primary_frames_and_shards(trx, name, n, w, h):
    flat, eye, look, fov = _scene(trx, name, n)
    view = trx.view_from_camera(eye, look, fov, w, h)
    sc = trx.Scene(flat)
    recs = tri_records(flat.tri_verts)
    try:
        for sem in (0, 3):
            _primary_case(trx, sc, recs, view, w, h, sem, what="%s image" % name)
        for layout in (0, 1):
            _primary_case(trx, sc, recs, view, w, h, 3, shard=(1, 3), layout=layout, what="%s shard 1/3 layout %d" % (name, layout))
    finally:
        sc.close()


def test_full_size_bistro_frame(trx):
    flat, eye, look, fov = _scene(trx, "bistro", 0)
    view = trx.view_from_camera(eye, look, fov, 1920, 1080)
    sc = trx.Scene(flat)
    try:
        _primary_case(trx, sc, tri_records(flat.tri_verts), view, 1920, 1080, 3, what="bistro 1920x1080")
    finally:
        sc.close()


# ---- 3. two-level scenes -----------------------------------------------------------------------------------------

def test_f16_tlas_golden(trx):
    g = np.load(os.path.join(GOLDEN, "kitchen_tlas_f16_56x40.npz"))
    nodes, tri_verts, inst, tlas_start = golden_inputs(trx, g)
    flat = trx.FlatScene(nodes, tri_verts, inst, tlas_start, np.arange(tri_verts.shape[0]), [0, tri_verts.shape[0]])
    view = trx._lib.View()
    C.memmove(C.byref(view), g["view"].tobytes(), C.sizeof(view))
    sc = trx.Scene(flat, tri_format=trx.TRI_F16_24, tri_bytes=g["tri_f16"])
    recs = tri_records(tri_f16=g["tri_f16"])
    w, h = int(g["width"]), int(g["height"])
    try:
        for sem in (0, 3):
            _primary_case(trx, sc, recs, view, w, h, sem, what="f16 tlas")
            _rays_case(trx, sc, recs, g["rays"], sem, what="f16 tlas rays")
    finally:
        sc.close()


def test_transformed_instances(trx):
    flat, o2w, world, _, _ = instanced_scene(trx, n_instances=14, tris_per_object=0, kind="cornell", spread=1.0)
    sc = trx.Scene(flat)
    w2o = sc.instance_world_to_object()
    recs = tri_records(flat.tri_verts)
    lo, hi = world.reshape(-1, 3).min(0), world.reshape(-1, 3).max(0)
    w, h = 200, 120
    view = trx.view_from_camera((hi + 0.1 * (hi - lo)).tolist(), (0.5 * (lo + hi)).tolist(), 80.0, w, h)
    wflat = type("W", (), {"tri_verts": world})
    rays = np.concatenate([random_rays(trx, wflat, 2000, 21), aimed_rays(trx, world, 4000, 22)])
    try:
        for sem in (0, 3):
            _primary_case(trx, sc, recs, view, w, h, sem, w2o=w2o, what="instanced")
            _primary_case(trx, sc, recs, view, w, h, sem, shard=(1, 3), layout=1, w2o=w2o, what="instanced shard")
        for sem in ALL_SEMS:
            _rays_case(trx, sc, recs, rays, sem, w2o=w2o, what="instanced rays")
    finally:
        sc.close()


def test_rebraided_tlas(trx):
    flat, eye, look, fov = _scene(trx, "san_miguel", 120000, tlas=True)
    assert flat.instance_entry is not None, "the build did not re-braid"
    sc = trx.Scene(flat)
    recs = tri_records(flat.tri_verts)
    w, h = 120, 68
    view = trx.view_from_camera(eye, look, fov, w, h)
    try:
        for sem in (0, 3):
            _primary_case(trx, sc, recs, view, w, h, sem, what="rebraided")
            _rays_case(trx, sc, recs, aimed_rays(trx, flat.tri_verts, 4000, 31), sem, what="rebraided rays")
    finally:
        sc.close()


# ---- 4. / 5. refused calls and caller records ------------------------------------------------------------------

def test_transformed_scene_needs_instance_ids(trx):
    flat, _, world, _, _ = instanced_scene(trx)
    sc = trx.Scene(flat)
    lib, n = trx.load(), 256
    rays = aimed_rays(trx, world, n, 41)
    d_rays, d_hits, d_attr = _dev(rays), _buf(n, trx.HIT_DTYPE, 0), _buf(n, trx.HIT_ATTR_DTYPE)
    view = trx.view_from_camera([5.0, 5.0, 5.0], [0.0, 0.0, 0.0], 60.0, 16, 16)
    try:
        rc = lib.trx_hit_attributes_rays_dev(sc.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_hits.data_ptr()), None,
                                             C.c_void_p(d_attr.data_ptr()), None)
        assert rc == trx._lib.TRX_ERR_INVALID and b"instance" in lib.trx_last_error()
        rc = lib.trx_hit_attributes_primary_dev(sc.handle, C.byref(view), 16, 16, trx._lib.Shard(0, 1, 0, 0),
                                                C.c_void_p(d_hits.data_ptr()), None, C.c_void_p(d_attr.data_ptr()), None)
        assert rc == trx._lib.TRX_ERR_INVALID
        _torch().cuda.synchronize()
        assert (d_attr.cpu().numpy() == SENTINEL).all()
    finally:
        sc.close()


def _caller_records(trx, sc, recs, rays, prims, inst, w2o):
    n = rays.shape[0]
    hits = np.zeros(n, dtype=trx.HIT_DTYPE)
    hits["t"], hits["prim"] = 1.0, prims
    d_rays, d_hits, d_inst, d_attr = _dev(rays), _dev(hits), _dev(np.asarray(inst, dtype=np.uint32)), _buf(n, trx.HIT_ATTR_DTYPE)
    sc.hit_attributes_rays_dev(d_rays.data_ptr(), n, d_hits.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr())
    _torch().cuda.synchronize()
    attr = _host(d_attr, trx.HIT_ATTR_DTYPE)
    want = hit_attrs(recs, rays["origin"], rays["direction"], prims, inst, w2o)
    assert (attr_bits(attr) == attr_bits(want)).all()
    return attr


def test_unusable_caller_records_give_zero_records(trx):
    # transformed scene: prim past the triangles, or instance outside the table -> zero; the rest as the twin
    flat, _, world, _, _ = instanced_scene(trx)
    sc = trx.Scene(flat)
    w2o = sc.instance_world_to_object()
    recs, nt, ni = tri_records(flat.tri_verts), flat.n_tris, w2o.shape[0]
    rays = aimed_rays(trx, world, 8, 51)
    prims = np.array([0, nt - 1, nt, 0xFFFFFFFF, 5, 7, 2**31, 3], dtype=np.uint32)
    inst = np.array([0, ni - 1, 0, 0, ni, 0xFFFFFFFF, 1, 2], dtype=np.uint32)
    try:
        attr = _caller_records(trx, sc, recs, rays, prims, inst, w2o)
        assert not attr_bits(attr)[[2, 3, 4, 5, 6]].any()
        assert attr_bits(attr)[[0, 1, 7]].any(1).all()
    finally:
        sc.close()
    # plain scene: instance ids are ignored, prims past the triangles -> zero
    flat, _, _, _ = _scene(trx, "soup", 500)
    sc = trx.Scene(flat)
    recs = tri_records(flat.tri_verts)
    rays = aimed_rays(trx, flat.tri_verts, 8, 52)
    prims = np.array([0, 1, flat.n_tris, 0xFFFFFFFF, 7, 2**31, 9, flat.n_tris - 1], dtype=np.uint32)
    try:
        attr = _caller_records(trx, sc, recs, rays, prims, np.full(8, 0xFFFFFFFF, np.uint32), None)
        assert not attr_bits(attr)[[2, 3, 5]].any()
    finally:
        sc.close()


# ---- 6. refit ordering -----------------------------------------------------------------------------------------

def test_attributes_follow_refit_in_launch_order(trx):
    torch = _torch()
    flat, _, _, _ = _scene(trx, "bistro", 150000)
    sc = trx.Scene(flat)
    rng = np.random.default_rng(61)
    v = flat.tri_verts
    size = float(np.linalg.norm(v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0)))
    moved = (v + rng.normal(scale=2e-3 * size, size=v.shape)).astype(np.float32)
    moved2 = (v + rng.normal(scale=2e-3 * size, size=v.shape)).astype(np.float32)
    rays = aimed_rays(trx, v, 20000, 62)
    try:
        _rays_case(trx, sc, tri_records(v), rays, 3, what="before refit")
        sc.refit(moved)
        hits, inst, _ = _rays_case(trx, sc, tri_records(moved), rays, 3, what="after refit")
        # a busy stream: a long trace, then an attribute launch over hits of the current geometry, then at once a refit
        s = torch.cuda.Stream()
        big = random_rays(trx, flat, 2 * 1024 * 1024, 63, zero_dirs=False)
        d_big, d_bh = _dev(big), _buf(big.shape[0], trx.HIT_DTYPE)
        d_rays, d_hits, d_attr = _dev(rays), _dev(hits), _buf(rays.shape[0], trx.HIT_ATTR_DTYPE)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            sc.trace_rays_dev(d_big.data_ptr(), big.shape[0], d_bh.data_ptr(), sem=3, stream=s.cuda_stream)
            sc.hit_attributes_rays_dev(d_rays.data_ptr(), rays.shape[0], d_hits.data_ptr(), d_attr.data_ptr(), stream=s.cuda_stream)
        sc.refit(moved2)
        s.synchronize()
        attr = _host(d_attr, trx.HIT_ATTR_DTYPE)
        old = hit_attrs(tri_records(moved), rays["origin"], rays["direction"], hits["prim"])
        new = hit_attrs(tri_records(moved2), rays["origin"], rays["direction"], hits["prim"])
        assert (attr_bits(attr) == attr_bits(old)).all(), "the attribute launch saw the refit's geometry"
        assert (attr_bits(old) != attr_bits(new)).any(1).sum() > 1000
        # and a new trace after the refit follows the new vertices
        _rays_case(trx, sc, tri_records(moved2), rays, 3, what="after second refit")
    finally:
        sc.close()


# ---- 7. / 8. one stream without the host; the host-buffer form ---------------------------------------------------

def test_trace_and_attributes_on_one_side_stream(trx):
    torch = _torch()
    flat, eye, look, fov = _scene(trx, "kitchen", 20000)
    sc = trx.Scene(flat)
    recs = tri_records(flat.tri_verts)
    s = torch.cuda.Stream()
    view = trx.view_from_camera(eye, look, fov, 160, 90)
    try:
        with torch.cuda.stream(s):
            _rays_case(trx, sc, recs, aimed_rays(trx, flat.tri_verts, 5000, 71), 0, stream=s, what="side stream")
            _primary_case(trx, sc, recs, view, 160, 90, 0, stream=s, what="side stream primary")
    finally:
        sc.close()


def test_host_form_equals_trace_plus_device_pass(trx):
    cases = []
    flat, _, _, _ = _scene(trx, "soup", 2500)
    cases.append((flat, aimed_rays(trx, flat.tri_verts, 3000, 81), None))
    iflat, _, world, _, _ = instanced_scene(trx)
    cases.append((iflat, aimed_rays(trx, world, 3000, 82), True))
    for fl, rays, xf in cases:
        sc = trx.Scene(fl)
        recs = tri_records(fl.tri_verts)
        w2o = sc.instance_world_to_object() if xf else None
        try:
            for sem in (0, 3):
                hits, inst, attr = sc.trace_rays_attr(rays, sem=sem)
                dh, di, da = _rays_case(trx, sc, recs, rays, sem, w2o=w2o, what="dev form")
                gh, gi, _ = sc.trace_rays_inst(rays, sem=sem)
                assert (hits.view(np.uint32) == gh.view(np.uint32)).all() and (inst == gi).all()
                assert (hits.view(np.uint32) == dh.view(np.uint32)).all()
                assert (attr_bits(attr) == attr_bits(da)).all()
        finally:
            sc.close()
