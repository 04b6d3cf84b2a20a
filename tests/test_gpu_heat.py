"""The PROFILE_RT heat map on the GPU: per-ray counts of the counting kernels (trx_count_*_per_ray) against the oracle's per-ray
counters, and the heat shade (trx_shade_heat_dev, trx_render_heat_image, the command line's --profile-rt) against the numpy
twin of the colour rule (tests/heat_twin.py).

Bar: integer equality for counts, byte equality for colours.  No tolerance anywhere.  tests/test_heat.py asserts, on the
oracle's output alone, that the fixtures' frames hold many different counts.  Run with `-m gpu` on an MI355X.
"""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import heat_twin as H
from ao_visibility_twin import record_map
from helpers import ALL_SEMS, aimed_rays, assert_hits_equal, random_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tray_racing_amd", "tray_racing_hip")
SLACK = 37                 # records past the end of an output buffer: must stay as they were
SENTINEL = 0x5A5A5A5A      # a cost record no pass writes here: n_node = n_tri = 23130, far above any count of these frames
HAIRBALL_TRIS = 700000
ZERO = np.zeros(1, dtype=H.COST_DTYPE)


@pytest.fixture(scope="module", autouse=True)
def need_gpu(trx):
    lib = trx.load()
    assert lib.trx_device_count() > 0, "no HIP device visible to libtrx.so"


def cost_buffer(n):
    import torch
    return torch.full((n + SLACK,), SENTINEL, dtype=torch.int32, device="cuda")


def hit_buffer(n):
    import torch
    return torch.full((n + SLACK,), -1, dtype=torch.int64, device="cuda")


def cost_of(t):
    return t.cpu().numpy().view(H.COST_DTYPE)


def untouched(raw, written):
    """Every record outside `written` (indices) still holds the sentinel."""
    keep = np.ones(raw.size, dtype=bool)
    keep[written] = False
    return bool((raw[keep].view(np.uint32) == SENTINEL).all())


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def six(st):
    return (int(st.n_rays), int(st.n_node), int(st.n_tri), int(st.n_hits), int(st.max_stack), int(st.overflow))


def same_stats(a, b):
    """Two primary passes: whole tiles go to a wave, so the wave-level counters repeat as well.  (Incoherent passes refill
    mid-tile: which rays share a wave differs from run to run, and only the six ray-level counters are compared.)"""
    return six(a) == six(b) and (int(a.n_wave_node), int(a.n_wave_tri)) == (int(b.n_wave_node), int(b.n_wave_tri))


class Golden:
    """A golden fixture on both sides: the device scene over its vertex-format triangles, the oracle's, one view."""

    def __init__(self, trx, orc, name):
        from tray_racing_amd import _lib
        self.g, self.osc, self.ov, self.w, self.h = H.golden(orc, name)
        n = self.g["tri_verts"].shape[0]
        self.sc = trx.Scene(trx.FlatScene(self.g["nodes"], self.g["tri_verts"], self.g["instance_offsets"], int(self.g["tlas_start"]),
                                          np.arange(n), [0, n]))
        self.view = _lib.View.from_buffer_copy(self.g["view"].tobytes())
        self.npx = self.w * self.h


# ---- (a) primary rays ---------------------------------------------------------------------------------------------------

PRIMARY_CASES = [("soup_52x44", ALL_SEMS), ("cornell_64", (0, 3)), ("cornell_tlas_48", ALL_SEMS), ("box14_tlas_48", (0, 3)),
                 ("kitchen_tlas_f16_56x40", (0, 3))]


@pytest.mark.parametrize("name,sems", PRIMARY_CASES)
def test_primary_per_ray_counts_equal_the_oracle(trx, orc, name, sems):
    """trx_count_primary_per_ray in image layout (whole image; shard 1 of 3) and in TRX_LAYOUT_SHARD (shard 1 of 3): every
    owned record is the oracle's count_per_ray record of its pixel, every other record - other shards' pixels, padding of
    tiles that leave the image, 37 records past the end - is untouched; d_hits and trx_stats are trx_count_primary's for the
    same arguments; the records sum to the stats."""
    import torch
    from tray_racing_amd import _lib as L
    c = Golden(trx, orc, name)
    lib = trx.load()
    try:
        for sem in sems:
            want = H.primary_cost(c.osc, c.ov, c.w, c.h, sem)
            for shard in ((0, 1, 0), (1, 3, 0), (1, 3, 1)):
                what = "%s sem %d shard %s" % (name, sem, shard)
                pixels, recs, n_rec = record_map(c.w, c.h, shard)
                assert pixels.size > 0
                d_cost, d_hits, d_ref = cost_buffer(n_rec), hit_buffer(n_rec), hit_buffer(n_rec)
                st = c.sc.count_primary_per_ray(c.view, c.w, c.h, d_cost.data_ptr(), d_hits.data_ptr(), sem=sem, shard=shard)
                ref = L.Stats()
                L.check(lib.trx_count_primary(c.sc.handle, C.byref(c.view), c.w, c.h, L.Shard(*shard), sem, C.c_void_p(d_ref.data_ptr()),
                                              C.byref(ref)))
                got = cost_of(d_cost)
                bad = np.flatnonzero(got[recs] != want[pixels])
                assert bad.size == 0, "%s: %d records differ, first pixel %d: gpu %s oracle %s" % (
                    what, bad.size, pixels[bad[0]], got[recs][bad[0]], want[pixels][bad[0]])
                assert untouched(got, recs), what + ": a record outside the shard's pixels was written"
                assert torch.equal(d_hits, d_ref), what + ": hit records differ from trx_count_primary's"
                assert same_stats(st, ref), what
                assert int(st.n_rays) == pixels.size
                assert (int(got[recs]["n_node"].sum(dtype=np.int64)), int(got[recs]["n_tri"].sum(dtype=np.int64))) == (int(st.n_node), int(st.n_tri)), what
            # the hit records into the scene's scratch (d_hits NULL): the same counts
            d_cost = cost_buffer(c.npx)
            st0 = c.sc.count_primary_per_ray(c.view, c.w, c.h, d_cost.data_ptr(), 0, sem=sem)
            assert (cost_of(d_cost)[:c.npx] == want).all() and untouched(cost_of(d_cost), np.arange(c.npx))
            # and the plain counting call after it writes no per-ray record anywhere: its counters are its own
            st1 = c.sc.count_primary(c.view, c.w, c.h, sem=sem)
            assert six(st1) == six(st0)
        c.sc.check()
    finally:
        c.sc.close()


# ---- (b) explicit rays --------------------------------------------------------------------------------------------------

def check_ray_batch(trx, sc, osc, rays, sem, what, subset=None):
    """trx_count_rays_per_ray over `rays`: records of `subset` (default: all) equal the oracle's walk of each ray alone, all
    records sum to the oracle's batch totals, slack untouched, hits and stats trx_count_rays's."""
    import torch
    from tray_racing_amd import dist as D
    n = rays.shape[0]
    d_rays, d_cost, d_hits, d_ref = to_device(rays), cost_buffer(n), hit_buffer(n), hit_buffer(n)
    st = sc.count_rays_per_ray(d_rays.data_ptr(), n, d_cost.data_ptr(), d_hits.data_ptr(), sem=sem)
    ref = sc.count_rays(d_rays.data_ptr(), n, d_ref.data_ptr(), sem=sem)
    want_hits, ost = osc.trace_rays(rays, sem=sem)
    got = cost_of(d_cost)
    idx = np.arange(n) if subset is None else subset
    want = H.rays_cost(osc, rays, sem, idx)
    bad = np.flatnonzero(got[idx] != want)
    assert bad.size == 0, "%s: %d records differ, first ray %d: gpu %s oracle %s" % (what, bad.size, idx[bad[0]], got[idx][bad[0]], want[bad[0]])
    assert untouched(got, np.arange(n)), what
    assert got[:n]["n_node"].max() < 65535 and got[:n]["n_tri"].max() < 65535
    assert (int(got[:n]["n_node"].sum(dtype=np.int64)), int(got[:n]["n_tri"].sum(dtype=np.int64))) == (int(ost.n_node), int(ost.n_tri)), what
    assert six(st) == six(ost) and six(ref) == six(ost), what
    assert torch.equal(d_hits, d_ref), what
    assert_hits_equal(D.int64_to_hits(d_hits[:n]), want_hits, what)
    return got[:n], ost


@pytest.mark.parametrize("name", ("kitchen_tlas_f16_56x40", "ties_rays"))
def test_ray_per_ray_counts_equal_the_oracle(trx, orc, name):
    """The 700 rays of the kitchen fixture (two-level) and the 579 of ties_rays (exact ties, zero direction components),
    TRX_SEM_HLSL and semantics word 3, every ray against the oracle; and a batch of one ray."""
    g = np.load(os.path.join(H.GOLDEN, name + ".npz"))
    n = g["tri_verts"].shape[0]
    osc = orc.Scene(g["nodes"], g["tri_verts"], g["instance_offsets"], int(g["tlas_start"]))
    sc = trx.Scene(trx.FlatScene(g["nodes"], g["tri_verts"], g["instance_offsets"], int(g["tlas_start"]), np.arange(n), [0, n]))
    rays = np.ascontiguousarray(g["rays"])
    try:
        for sem in (0, 3):
            got, ost = check_ray_batch(trx, sc, osc, rays, sem, "%s sem %d" % (name, sem))
            assert ost.n_tri > 0 and 0 < ost.n_hits and np.unique(got["n_node"]).size >= 3   # (ties_rays: 19 nodes, at most 4 visits)
            busiest = int(np.argmax(got["n_node"]))
            one, ost1 = check_ray_batch(trx, sc, osc, rays[busiest:busiest + 1], sem, "%s sem %d, one ray" % (name, sem))
            assert ost1.n_node > 1 and one[0] == got[busiest]
        sc.check()
    finally:
        sc.close()


def test_ray_per_ray_counts_through_the_pipelined_walk(trx, orc):
    """2 048 mixed rays (a third aimed at triangles, the rest random with ranged, zero-component and axis-parallel ones) over a
    hairball-class scene past the pipelined walk's size threshold: 512 of them against the oracle one by one, all of them by
    their sums."""
    verts, counts = trx.gen_scene("hairball", HAIRBALL_TRIS, 1)
    flat = trx.flat_build(verts, counts)
    osc = orc.Scene.from_flat(flat)
    n = 2048
    n_aimed = (n + 2) // 3
    rays = np.concatenate([aimed_rays(trx, flat.tri_verts, n_aimed, 11), random_rays(trx, flat, n - n_aimed, 12, zero_dirs=True)])
    subset = np.sort(np.random.default_rng(5).choice(n, size=512, replace=False))
    sc = trx.Scene(flat)
    try:
        assert sc.walk_kind(trx.MODE_RAYS) == trx.WALK_PIPELINED, "the hairball-class scene no longer reaches the pipelined walk"
        for sem in (0, 3):
            got, ost = check_ray_batch(trx, sc, osc, rays, sem, "hairball sem %d" % sem, subset)
            assert 0.02 < ost.n_hits / n < 0.99 and ost.n_tri > 0
            assert np.unique(got["n_node"]).size >= 10 and got["n_node"].max() >= 15
        sc.check()
    finally:
        sc.close()


# ---- (c) AO rays ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("soup_52x44", "cornell_tlas_48"))
def test_ao_per_ray_counts_equal_the_twin(trx, orc, name):
    """trx_count_ao_per_ray under seed 3 (and 7 with the small epsilon) over the device's own primary records: every surface
    pixel's record is the oracle's walk of that pixel's AO ray alone (tests/test_heat.py shows these sum to trace_ao's
    totals), every pixel whose primary record is a miss gets {0, 0} exactly; image layout and TRX_LAYOUT_SHARD shard 1 of 3;
    stats and records trx_count_ao's; d_ao NULL gives the same counts."""
    import torch
    from tray_racing_amd import dist as D
    c = Golden(trx, orc, name)
    try:
        for sem in (0, 3):
            prim, _ = c.osc.trace_primary(c.ov, c.w, c.h, sem=sem)
            d_prim = hit_buffer(c.npx)
            c.sc.trace_primary_dev(c.view, c.w, c.h, d_prim.data_ptr(), sem=sem)
            torch.cuda.synchronize()
            assert_hits_equal(D.int64_to_hits(d_prim[:c.npx]), prim, name + " primary")
            for frame, eps in ((3, 0.01), (7, 0.0001)):
                what = "%s sem %d frame %d eps %g" % (name, sem, frame, eps)
                want, surface = H.ao_cost(orc, c.osc, c.ov, c.w, c.h, prim, sem, frame, eps)
                _, ost = c.osc.trace_ao(c.ov, c.w, c.h, prim, sem=sem, frame=frame, ao_eps=eps)
                miss, hit = np.flatnonzero(~surface), np.flatnonzero(surface)
                assert miss.size > 0 and hit.size > 0, what
                d_cost, d_ao, d_ref = cost_buffer(c.npx), hit_buffer(c.npx), hit_buffer(c.npx)
                st = c.sc.count_ao_per_ray(c.view, c.w, c.h, d_prim.data_ptr(), d_cost.data_ptr(), d_ao.data_ptr(), sem=sem, frame=frame, ao_eps=eps)
                ref = c.sc.count_ao(c.view, c.w, c.h, d_prim.data_ptr(), d_ref.data_ptr(), sem=sem, frame=frame, ao_eps=eps)
                got = cost_of(d_cost)
                assert (got[miss] == ZERO).all(), what + ": a pixel without a surface is not {0, 0}"
                bad = np.flatnonzero(got[hit] != want[hit])
                assert bad.size == 0, "%s: %d records differ, first pixel %d: gpu %s twin %s" % (what, bad.size, hit[bad[0]], got[hit][bad[0]], want[hit][bad[0]])
                assert got[hit]["n_node"].min() >= 1 and untouched(got, np.arange(c.npx)), what
                assert six(st) == six(ost) and six(ref) == six(ost) and torch.equal(d_ao, d_ref), what
                assert (int(got[:c.npx]["n_node"].sum(dtype=np.int64)), int(got[:c.npx]["n_tri"].sum(dtype=np.int64))) == (int(st.n_node), int(st.n_tri))
                d_cost0 = cost_buffer(c.npx)
                st0 = c.sc.count_ao_per_ray(c.view, c.w, c.h, d_prim.data_ptr(), d_cost0.data_ptr(), 0, sem=sem, frame=frame, ao_eps=eps)
                assert torch.equal(d_cost0, d_cost) and six(st0) == six(ost), what + ", records into the scratch buffer"
            # TRX_LAYOUT_SHARD, shard 1 of 3: the shard's own primary records, its pixels' AO records
            shard = (1, 3, 1)
            pixels, recs, n_rec = record_map(c.w, c.h, shard)
            want, surface = H.ao_cost(orc, c.osc, c.ov, c.w, c.h, prim, sem, 3, 0.01)
            d_lp, d_cost, d_ao = hit_buffer(n_rec), cost_buffer(n_rec), hit_buffer(n_rec)
            c.sc.trace_primary_dev(c.view, c.w, c.h, d_lp.data_ptr(), sem=sem, shard=shard)
            st = c.sc.count_ao_per_ray(c.view, c.w, c.h, d_lp.data_ptr(), d_cost.data_ptr(), d_ao.data_ptr(), sem=sem, frame=3, ao_eps=0.01, shard=shard)
            got = cost_of(d_cost)
            assert (got[recs] == want[pixels]).all() and untouched(got, recs), "%s sem %d shard layout" % (name, sem)
            assert int(st.n_rays) == int(surface[pixels].sum()) and 0 < int(st.n_rays) < pixels.size
        c.sc.check()
    finally:
        c.sc.close()


# ---- (d) the shade ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_scene(trx):
    sc = trx.Scene(trx.flat_build(trx.gen_scene("soup", 50, 1)[0]))
    yield sc
    sc.close()


def all_counts():
    """65 536 records: n_node runs up, n_tri runs down - a shade that reads the other field shows."""
    rec = np.zeros(65536, dtype=H.COST_DTYPE)
    rec["n_node"] = np.arange(65536)
    rec["n_tri"] = 65535 - np.arange(65536)
    return rec


@pytest.mark.parametrize("which,scale", [(H.HEAT_NODES, H.SCALE_NODES), (H.HEAT_TRIS, H.SCALE_TRIS), (H.HEAT_NODES, 0.00037),
                                         (H.HEAT_TRIS, 0.0031), (H.HEAT_NODES, 0.0), (H.HEAT_TRIS, 3.0e38)])
def test_heat_shade_equals_the_twin_for_every_count(trx, small_scene, which, scale):
    """All 65 536 values of n_node (nodes mode) / n_tri (triangles mode) at the reference scale, at another scale - which
    moves every count to another place of the ramp -, at scale 0 and at a scale whose product overflows: byte for byte the
    twin's image; nothing is written past n_records * 4 bytes."""
    import torch
    rec = all_counts()
    d_cost = to_device(rec)
    d_rgba = torch.full((65536 * 4 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    small_scene.shade_heat_dev(d_cost.data_ptr(), 65536, d_rgba.data_ptr(), which=which, scale=float(np.float32(scale)))
    torch.cuda.synchronize()
    got = d_rgba.cpu().numpy()
    want = H.heat_rgba(rec, which, scale)
    img = got[:65536 * 4].reshape(-1, 4)
    bad = np.flatnonzero((img != want).any(1))
    assert bad.size == 0, "mode %d scale %g: %d records differ, first %s: gpu %s twin %s" % (which, scale, bad.size, rec[bad[0]], img[bad[0]], want[bad[0]])
    assert (got[65536 * 4:] == 0xA5).all()
    # a short, odd number of records starting inside the buffer: the 4-byte output alignment is all the call asks for
    d_rgba.fill_(0xA5)
    small_scene.shade_heat_dev(d_cost.data_ptr() + 4 * 3, 257, d_rgba.data_ptr() + 4, which=which, scale=float(np.float32(scale)))
    torch.cuda.synchronize()
    got = d_rgba.cpu().numpy()
    assert (got[4:4 + 257 * 4].reshape(-1, 4) == want[3:260]).all() and (got[:4] == 0xA5).all() and (got[4 + 257 * 4:] == 0xA5).all()
    small_scene.check()


def test_heat_shade_refusals_leave_the_output_untouched(trx, small_scene):
    import torch
    from tray_racing_amd import _lib as L
    lib = trx.load()
    d_cost = to_device(all_counts()[:64])
    d_rgba = torch.full((64 * 4 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    h, P = small_scene.handle, C.c_void_p
    for args in ((h, P(d_cost.data_ptr()), 64, 2, 0.002, P(d_rgba.data_ptr()), None),
                 (h, P(d_cost.data_ptr()), 64, 0, float("nan"), P(d_rgba.data_ptr()), None),
                 (h, P(d_cost.data_ptr()), 64, 0, -0.002, P(d_rgba.data_ptr()), None),
                 (h, P(d_cost.data_ptr()), 64, 1, float("inf"), P(d_rgba.data_ptr()), None),
                 (h, P(d_cost.data_ptr()), 64, 0, 0.002, P(d_rgba.data_ptr() + 2), None),
                 (h, None, 64, 0, 0.002, P(d_rgba.data_ptr()), None),
                 (h, P(d_cost.data_ptr()), 64, 0, 0.002, None, None),
                 (None, P(d_cost.data_ptr()), 64, 0, 0.002, P(d_rgba.data_ptr()), None)):
        assert lib.trx_shade_heat_dev(*args) == L.TRX_ERR_INVALID, args[2:5]
    assert lib.trx_shade_heat_dev(h, None, 0, 0, 0.002, None, None) == L.TRX_OK   # no records: nothing to do
    st = L.Stats()
    view = trx.view_from_camera((0, 0, 5), (0, 0, 0), 60.0, 8, 8)
    assert lib.trx_count_primary_per_ray(h, C.byref(view), 8, 8, L.Shard(0, 1, 0, 0), 0, None, None, C.byref(st)) == L.TRX_ERR_INVALID
    assert lib.trx_count_rays_per_ray(h, P(d_cost.data_ptr()), 1, 0, None, None, C.byref(st)) == L.TRX_ERR_INVALID
    assert lib.trx_render_heat_image(h, C.byref(view), 8, 8, 0, 2, 0.002, None, None) == L.TRX_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((d_rgba == 0xA5).all())
    small_scene.check()


# ---- (e) the host form and the command line ----------------------------------------------------------------------------

def test_render_heat_image_is_its_composition(trx, orc):
    """trx_render_heat_image = the counted primary pass and the shade: the twin's colours of the oracle's per-ray records,
    the pass's stats; both modes, the reference scale and another; out_rgba / out_stats may be NULL."""
    from tray_racing_amd import _lib as L
    c = Golden(trx, orc, "kitchen_tlas_f16_56x40")
    try:
        for sem in (0, 3):
            want = H.primary_cost(c.osc, c.ov, c.w, c.h, sem)
            _, ost = c.osc.trace_primary(c.ov, c.w, c.h, sem=sem)
            for which, scale in ((H.HEAT_NODES, None), (H.HEAT_TRIS, None), (H.HEAT_NODES, 0.0011)):
                img, st = c.sc.render_heat_image(c.view, c.w, c.h, which=which, scale=scale, sem=sem)
                ref_scale = scale if scale is not None else (H.SCALE_TRIS if which == H.HEAT_TRIS else H.SCALE_NODES)
                assert (img.reshape(-1, 4) == H.heat_rgba(want, which, ref_scale)).all(), (sem, which, scale)
                assert six(st) == six(ost)
                assert np.unique(img.reshape(-1, 4), axis=0).shape[0] >= 10
        L.check(trx.load().trx_render_heat_image(c.sc.handle, C.byref(c.view), c.w, c.h, 0, 0, 0.002, None, None))
        c.sc.check()
    finally:
        c.sc.close()


def read_png(path, w, h):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat = 8, b""
    while pos < len(data):
        size, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if tag == b"IDAT":
            idat += data[pos + 8:pos + 8 + size]
        pos += 12 + size
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 4 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 4)


@pytest.mark.parametrize("mode,extra,which,scale", [("nodes", (), H.HEAT_NODES, H.SCALE_NODES),
                                                    ("tris", ("--profile-rt-scale", "0.02", "--cpu-semantics"), H.HEAT_TRIS, 0.02)])
def test_cli_png_is_the_heat_map(trx, orc, tmp_path, mode, extra, which, scale):
    """--png --profile-rt: `<name>_rend.png` holds the heat map of the frame the command line built and traced - the tree of
    its default build parameters, the stand-in's camera - pixel for pixel the twin's."""
    w, h = 96, 64
    r = subprocess.run([CLI, "-i", "standin:cornell", "--render-time", "0", "--width", str(w), "--height", str(h), "--passes", "1", "--png",
                        "--verbose", "--profile-rt", mode] + list(extra), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert "heat map" in r.stdout
    img = read_png(str(tmp_path / "cornell_rend.png"), w, h)
    verts, counts = trx.gen_scene("cornell", 0, 1)
    bp = trx.build_params(pre_split=0, ploc_search_distance=14, search_depth_threshold=2, reinsertion_batch_ratio=0.15, sort_precision=64,
                          max_prims_per_leaf=3, post_collapse_reinsertion_batch_ratio_multiplier=0.0, collapse_traversal_cost=1.0)
    flat = trx.flat_build_params(verts, counts, bp)
    eye, look, fov = trx.scene_camera("cornell")
    ov = orc.view_from_bytes(trx.view_from_camera(eye, look, fov, w, h))
    sem = 3 if "--cpu-semantics" in extra else 0
    want = H.heat_rgba(H.primary_cost(orc.Scene.from_flat(flat), ov, w, h, sem), which, scale)
    assert (img.reshape(-1, 4) == want).all()
    assert np.unique(want, axis=0).shape[0] >= 10
