"""The shading-normal pass on the GPU, bit for bit (include/trx.h, "vertex normals and the shading normal"):
trx_shading_normals_primary_dev / _rays_dev write the twin's records (tests/shading_normal_twin.py) - fed the device's own hits,
instance ids and attribute records - on single-level, two-level, f16 and transformed scenes, under computed, random and hostile
vertex-normal tables, in both layouts and two shards, in place and out of place; caller records past the tables' ends come back
as they went in; the table's life (read-back, accounting, replacement under a queued pass, refit, refusals); the light term and
the smooth host images against their compositions; power-of-two scene scaling.  Whole buffers are compared, sentinel bytes and
guards included: no record is left out.

Every step that runs on the GPU sits under a time limit of its own (`limit`): a step that hangs ends the process."""
import ctypes as C

import numpy as np
import pytest

import caller_records as CR
import light_twin as LT
import material_twin as MT
import scale_cases as SC
import scale_twin as ST
import shading_normal_cases as CS
import shading_normal_twin as SN
from ao_visibility_twin import instanced_case, record_map
from helpers import random_rays
from hit_attr_twin import ATTR_DTYPE, primary_dirs, tri_records
from test_gpu_light import EPS, _frame, _mixed, _sync, _torch, limit

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = 0xAB
GUARD = 48
HIT = np.dtype([("t", "<f4"), ("prim", "<u4")])
SHARDS = ((0, 1, 0), (0, 1, 1), (1, 3, 0), (1, 3, 1))


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _buf(nbytes, fill=SENTINEL):
    return _torch().full((max(nbytes, 1),), fill, dtype=_torch().uint8, device="cuda")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 6)


def _same_records(got, want, what):
    """Attribute records bit for bit (NaN payloads included: a record that falls back is copied, not computed)."""
    got, want = _bits(got), _bits(want)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, "%s: %d of %d records differ, first %s: %s != %s" % (what, bad.size, got.shape[0], bad[:4], got[bad[:2]], want[bad[:2]])


class World:
    """A scene of shading_normal_cases.SCENES on the device with what the twin needs of it."""

    def __init__(self, trx, orc, name):
        self.trx, self.name = trx, name
        if name == "instanced":
            flat, self.view, _, _, self.w, self.h = instanced_case(trx, orc)
            self.sc = trx.Scene(flat)
            self.recs, self.w2o = tri_records(flat.tri_verts), self.sc.instance_world_to_object()
            self.ray_box = flat                                          # (object-space bounds: the instances lie about the origin too)
        else:
            from tray_racing_amd import _lib
            g, self.recs, f16 = CS.golden(name)
            n = g["tri_verts"].shape[0]
            flat = trx.FlatScene(g["nodes"], g["tri_verts"], g["instance_offsets"], int(g["tlas_start"]), np.arange(n), [0, n])
            self.sc = trx.Scene(flat, tri_format=trx.TRI_F16_24, tri_bytes=f16) if f16 is not None else trx.Scene(flat)
            self.view = _lib.View()
            C.memmove(C.byref(self.view), g["view"].tobytes(), C.sizeof(self.view))
            self.w, self.h, self.w2o = int(g["width"]), int(g["height"]), None
            self.ray_box = flat
        self.flat = flat
        self.n_tris = self.recs.shape[0]
        self.n_inst = int(flat.instance_offsets.size)
        self.tables = {}
        self.current = None

    def table(self, kind):
        if kind not in self.tables:
            self.tables[kind] = CS.table(kind, self.recs)
        return self.tables[kind]

    def use(self, kind):
        if self.current != kind:
            self.sc.set_vertex_normals(self.table(kind))
            self.current = kind
        return self.table(kind)

    def frame(self, shard, sem=0):
        """(d_hits, d_inst, d_attr tensors laid out by `shard`; their host copies as whole buffers)."""
        from tray_racing_amd import _lib as L
        _, _, size = record_map(self.w, self.h, shard)
        d_hits, d_inst, d_attr = _buf(size * 8, 0xEE), _buf(size * 4, 0xFF), _buf(size * 24, 0xCD)
        _sync()
        with limit():
            L.check(self.sc._lib.trx_trace_primary_inst_dev(self.sc.handle, C.byref(self.view), self.w, self.h, L.Shard(*shard, 0), sem,
                                                            C.c_void_p(d_hits.data_ptr()), C.c_void_p(d_inst.data_ptr()), None))
            self.sc.hit_attributes_primary_dev(self.view, self.w, self.h, d_hits.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr(), shard=shard)
            _torch().cuda.synchronize()
        return (d_hits, d_inst, d_attr), (d_hits.cpu().numpy().view(HIT), d_inst.cpu().numpy().view(np.uint32), d_attr.cpu().numpy().view(ATTR_DTYPE))

    def primary_want(self, normals, shard, hits, inst, attr, base):
        """The whole output buffer the primary form must leave: `base` (the buffer before the call) with the twin's records at
        the shard's pixels inside the image."""
        pix, rec, size = record_map(self.w, self.h, shard)
        dirs = primary_dirs(self.view, self.w, self.h, pix % self.w, pix // self.w)
        out, cause = SN.shading_normals(normals, attr[rec], dirs, hits["prim"][rec], inst[rec], self.w2o)
        want = np.array(base, dtype=ATTR_DTYPE, copy=True)
        want[rec] = out
        return want, cause

    def shade_primary(self, shard, d_hits, d_inst, d_attr, d_out, stream=0):
        with limit():
            self.sc.shading_normals_primary(self.view, self.w, self.h, d_hits.data_ptr(), d_attr.data_ptr(), d_out, d_inst=d_inst.data_ptr(), shard=shard,
                                            stream=stream)
            _torch().cuda.synchronize()

    def close(self):
        self.sc.close()


@pytest.fixture(scope="module")
def worlds(trx, orc):
    made = {}

    def get(name):
        if name not in made:
            made[name] = World(trx, orc, name)
        return made[name]
    yield get
    for w in made.values():
        w.close()


# ---- primary mode -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", CS.TABLES)
@pytest.mark.parametrize("name", CS.SCENES)
def test_primary_records_equal_the_twin(trx, worlds, name, kind):
    """Both layouts, shards {0, 1} and {1, 3}; out of place into a sentinel-filled buffer between two guards - the records of
    other shards, a compact tile's pixels outside the image and the guards keep the sentinel - and in place."""
    wd = worlds(name)
    normals = wd.use(kind)
    for shard in SHARDS:
        (d_hits, d_inst, d_attr), (hits, inst, attr) = wd.frame(shard)
        pix, rec, size = record_map(wd.w, wd.h, shard)
        what = "%s %s shard %s" % (name, kind, shard)
        d_out = _buf(size * 24 + 2 * GUARD)
        wd.shade_primary(shard, d_hits, d_inst, d_attr, d_out.data_ptr() + GUARD)
        raw = d_out.cpu().numpy()
        assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all(), what + ": a guard byte was written"
        want, cause = wd.primary_want(normals, shard, hits, inst, attr, np.full(size * 24, SENTINEL, dtype=np.uint8).view(ATTR_DTYPE))
        _same_records(raw[GUARD:-GUARD].view(ATTR_DTYPE), want, what)
        assert (d_attr.cpu().numpy().view(ATTR_DTYPE).tobytes() == attr.tobytes()), what + ": the input was written"
        # in place equals out of place, and the records the pass does not own keep what they held
        wd.shade_primary(shard, d_hits, d_inst, d_attr, d_attr.data_ptr())
        want_in_place, _ = wd.primary_want(normals, shard, hits, inst, attr, attr)
        got = d_attr.cpu().numpy().view(ATTR_DTYPE)
        _same_records(got, want_in_place, what + " in place")
        assert got[rec].tobytes() == raw[GUARD:-GUARD].view(ATTR_DTYPE)[rec].tobytes()
        adopted = cause == SN.ADOPTED
        if shard[1] == 1:
            assert adopted.any() and (~adopted).any(), what
        if rec.size < size:
            assert (_bits(want)[np.setdiff1d(np.arange(size), rec)] == 0xABABABAB).all()        # (some record really is outside)
    wd.sc.check()


# ---- rays mode ------------------------------------------------------------------------------------------------------------------------

def _rays_case(wd, normals, rays, what, doctor=False, stream=0):
    """Trace, attribute pass and shading-normal pass over explicit rays on one stream; the whole output against the twin.
    doctor: some attribute records get a NaN normal and a non-zero pad word first (the rule's c == c, the pad word's fate)."""
    torch, sc, n = _torch(), wd.sc, rays.shape[0]
    d_rays, d_hits, d_inst, d_attr = _dev(rays), _buf(n * 8), _buf(n * 4, 0xFF), _buf(n * 24)
    _sync()
    with limit():
        sc.trace_rays_inst_dev(d_rays.data_ptr(), n, d_hits.data_ptr(), d_inst=d_inst.data_ptr(), stream=stream)
        sc.hit_attributes_rays_dev(d_rays.data_ptr(), n, d_hits.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr(), stream=stream)
        torch.cuda.synchronize()
    hits, inst, attr = d_hits.cpu().numpy().view(HIT), d_inst.cpu().numpy().view(np.uint32), d_attr.cpu().numpy().view(ATTR_DTYPE).copy()
    if doctor:
        hit = np.flatnonzero(hits["prim"] < wd.n_tris)
        attr["normal"][hit[::7], 0] = np.nan
        attr["normal"][hit[3::11]] = np.nan
        attr["_pad"][::3] = 0xDEADBEEF
        d_attr = _dev(attr)
    d_out = _buf(n * 24 + 2 * GUARD)
    with limit():
        sc.shading_normals_rays(d_rays.data_ptr(), n, d_hits.data_ptr(), d_attr.data_ptr(), d_out.data_ptr() + GUARD, d_inst=d_inst.data_ptr(), stream=stream)
        torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all(), what + ": a guard byte was written"
    want, cause = SN.shading_normals(normals, attr, rays["direction"], hits["prim"], inst, wd.w2o)
    _same_records(raw[GUARD:-GUARD].view(ATTR_DTYPE), want, what)
    with limit():
        sc.shading_normals_rays(d_rays.data_ptr(), n, d_hits.data_ptr(), d_attr.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr(), stream=stream)
        torch.cuda.synchronize()
    _same_records(d_attr.cpu().numpy().view(ATTR_DTYPE), want, what + " in place")
    return cause


@pytest.mark.parametrize("name", CS.SCENES)
def test_explicit_rays_equal_the_twin(trx, worlds, name):
    """helpers.random_rays (zero direction components among them: no zero-direction fix is applied) and the AO rays
    trx_ao_rays_dev writes for the scene's primary frame (bounce rays; the inert ray where the primary ray missed)."""
    torch = _torch()
    wd = worlds(name)
    rays = random_rays(trx, wd.ray_box, 4099, 17)
    (d_hits, d_inst, _), _ = wd.frame((0, 1, 0))
    n = wd.w * wd.h
    d_ao = _buf(n * 32)
    with limit():
        wd.sc.ao_rays_dev(wd.view, wd.w, wd.h, d_hits.data_ptr(), d_ao.data_ptr(), float("inf"), frame=5, ao_eps=EPS, d_primary_inst=d_inst.data_ptr())
        torch.cuda.synchronize()
    bounce = d_ao.cpu().numpy().view(trx.RAY_DTYPE).copy()
    seen = set()
    for kind in CS.TABLES:
        normals = wd.use(kind)
        seen |= set(_rays_case(wd, normals, rays, "%s %s random rays" % (name, kind), doctor=kind == "random").tolist())
        cause = _rays_case(wd, normals, bounce, "%s %s bounce rays" % (name, kind), doctor=kind == "random")
        assert (cause == SN.ADOPTED).sum() > 10 and (cause != SN.ADOPTED).any(), (name, kind)
        seen |= set(cause.tolist())
    assert {SN.ADOPTED, SN.OUT_OF_RANGE, SN.Q_NOT_POSITIVE, SN.Q_NOT_FINITE, SN.C_NAN, SN.FLIP_DIFFERS} <= seen, seen
    wd.sc.check()
    if wd.w2o is None:
        wd.sc.shading_normals_rays(0, 0, 0, 0, 0)   # zero rays: nothing to do, no error


# ---- caller records ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell_64", "cornell_tlas_48", "instanced"])
def test_caller_records_outside_the_tables_come_back_as_they_went_in(trx, worlds, name):
    """tests/caller_records.py's table - prim and instance ids at, just past and far past the tables' ends, every t - as explicit
    records: an entry is in range iff its prim is inside the triangle table and, on the transformed scene, its id selects a
    row (the table's hand-written columns; t is not looked at) - and then it is the twin's record; every other entry is its input
    bit for bit.  The same ids doctored into a primary frame; and a frame of nothing but sentinel bytes."""
    torch = _torch()
    wd = worlds(name)
    normals = wd.use("random")
    transformed = wd.w2o is not None
    table = CR.entries(wd.n_tris, wd.n_inst)
    n = len(table)
    rng = np.random.default_rng(23)
    hits, inst = np.zeros(n, dtype=HIT), np.zeros(n, dtype=np.uint32)
    in_range = np.zeros(n, dtype=bool)
    for k, (t, _, p, p_ok, i, i_ok) in enumerate(table):
        hits["t"][k], hits["prim"][k], inst[k] = (f32(0.75) if t is CR.OWN else t), p, i
        in_range[k] = p_ok and (i_ok or not transformed)
    attr = np.zeros(n, dtype=ATTR_DTYPE)
    attr["u"], attr["v"] = rng.random(n, dtype=np.float32) * f32(0.5), rng.random(n, dtype=np.float32) * f32(0.5)
    g = rng.normal(size=(n, 3))
    attr["normal"] = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    attr["_pad"] = rng.integers(1, 2 ** 32, n, dtype=np.uint32)
    rays = random_rays(trx, wd.ray_box, n, 29, zero_dirs=False)
    d_rays, d_hits, d_inst, d_attr, d_out = _dev(rays), _dev(hits), _dev(inst), _dev(attr), _buf(n * 24 + GUARD)
    _sync()
    with limit():
        wd.sc.shading_normals_rays(d_rays.data_ptr(), n, d_hits.data_ptr(), d_attr.data_ptr(), d_out.data_ptr(), d_inst=d_inst.data_ptr())
        torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    got = raw[:n * 24].view(ATTR_DTYPE)
    assert (raw[n * 24:] == SENTINEL).all()
    assert got[~in_range].tobytes() == attr[~in_range].tobytes(), "an entry outside the tables did not come back as it went in"
    want, cause = SN.shading_normals(normals, attr, rays["direction"], hits["prim"], inst, wd.w2o)
    _same_records(got, want, name + " table")
    assert ((cause != SN.OUT_OF_RANGE) == in_range).all() and (cause == SN.ADOPTED).sum() >= 4 and (~in_range).sum() >= 24
    # the same ids at picked pixels of the device's own frame (a whole tile of them among the pixels)
    (d_hits, d_inst, d_attr), (fh, fi, fa) = wd.frame((0, 1, 0))
    pixels, _ = CR.pick_pixels(wd.w, wd.h, len(table), fh["prim"] < wd.n_tris)
    dp, di, _, _, _ = CR.doctor(fh, fi, pixels, table)
    d_dp, d_di = _dev(dp), _dev(di)
    d_out = _buf(wd.w * wd.h * 24)
    wd.shade_primary((0, 1, 0), d_dp, d_di, d_attr, d_out.data_ptr())
    want, cause = wd.primary_want(normals, (0, 1, 0), dp, di, fa, fa)
    got = d_out.cpu().numpy().view(ATTR_DTYPE)
    _same_records(got, want, name + " doctored frame")
    outside = (dp["prim"] >= wd.n_tris) | ((di >= wd.n_inst) if transformed else False)
    assert outside[pixels].sum() >= 32 and got[outside].tobytes() == fa[outside].tobytes()
    # a frame of sentinel bytes: every prim (and id) is far past the tables, every record comes back as it went in
    size = wd.w * wd.h
    d_h, d_i, d_a, d_o = _buf(size * 8), _buf(size * 4), _buf(size * 24), _buf(size * 24, 0x11)
    wd.shade_primary((0, 1, 0), d_h, d_i, d_a, d_o.data_ptr())
    assert (d_o.cpu().numpy() == SENTINEL).all()
    wd.sc.check()


# ---- the table's life -------------------------------------------------------------------------------------------------------------------------

def test_set_get_round_trip_and_accounting(trx, worlds):
    wd = worlds("soup_52x44")
    sc, n = wd.sc, wd.n_tris
    sc.set_vertex_normals(None)
    wd.current = None
    with pytest.raises(trx.TrxError, match="no vertex normals"):
        sc.get_vertex_normals()
    before = sc.device_bytes
    hostile = wd.table("hostile").copy()
    hostile[1, 0], hostile[2, 4] = f32(-0.0), np.float32(1e-45)
    sc.set_vertex_normals(hostile)
    assert sc.device_bytes - before == 48 * n
    assert sc.get_vertex_normals().tobytes() == hostile.tobytes()
    sc.set_vertex_normals(wd.table("random"))                        # replaced: counted once
    assert sc.device_bytes - before == 48 * n and sc.get_vertex_normals().tobytes() == wd.table("random").tobytes()
    # refused calls leave the table in force
    bad = wd.table("random").copy()
    bad[n // 2, 7] = np.inf
    for arg, msg in ((bad, "not finite"), (wd.table("random")[:-1], "n_tris"), (np.concatenate([bad, bad]), "n_tris")):
        with pytest.raises(trx.TrxError, match=msg) as e:
            sc.set_vertex_normals(arg)
        assert e.value.code == -1
    bad[n // 2, 7] = np.nan
    with pytest.raises(trx.TrxError, match="not finite"):
        sc.set_vertex_normals(bad)
    assert sc.get_vertex_normals().tobytes() == wd.table("random").tobytes() and sc.device_bytes - before == 48 * n
    out = np.zeros((n - 1, 9), dtype=np.float32)
    assert sc._lib.trx_scene_get_vertex_normals(sc.handle, out.ctypes.data_as(C.c_void_p), n - 1) == -1
    sc.set_vertex_normals(None)
    assert sc.device_bytes == before
    sc.set_vertex_normals(None)                                      # removing nothing is no error


def test_a_table_replaced_between_two_launches_gives_each_its_own(trx, worlds):
    """On one busy stream: a long trace, the pass under table A, then - the host call waits for the queued pass - table B and the
    pass again.  The first output is A's, the second B's."""
    torch = _torch()
    wd = worlds("cornell_64")
    (d_hits, d_inst, d_attr), (hits, inst, attr) = wd.frame((0, 1, 0))
    size = wd.w * wd.h
    a, b = wd.table("computed"), wd.table("random")
    s = torch.cuda.Stream()
    big = random_rays(trx, wd.flat, 1024 * 1024, 72, zero_dirs=False)
    d_big, d_bh = _dev(big), _buf(big.shape[0] * 8)
    d_one, d_two = _buf(size * 24), _buf(size * 24)
    wd.sc.set_vertex_normals(a)
    wd.current = None
    _sync()
    with limit():
        with torch.cuda.stream(s):
            wd.sc.trace_rays_dev(d_big.data_ptr(), big.shape[0], d_bh.data_ptr(), stream=s.cuda_stream)
            wd.sc.shading_normals_primary(wd.view, wd.w, wd.h, d_hits.data_ptr(), d_attr.data_ptr(), d_one.data_ptr(), d_inst=d_inst.data_ptr(),
                                          stream=s.cuda_stream)
        wd.sc.set_vertex_normals(b)
        with torch.cuda.stream(s):
            wd.sc.shading_normals_primary(wd.view, wd.w, wd.h, d_hits.data_ptr(), d_attr.data_ptr(), d_two.data_ptr(), d_inst=d_inst.data_ptr(),
                                          stream=s.cuda_stream)
        s.synchronize()
    base = np.full(size * 24, SENTINEL, dtype=np.uint8).view(ATTR_DTYPE)
    want_a, _ = wd.primary_want(a, (0, 1, 0), hits, inst, attr, base)
    want_b, _ = wd.primary_want(b, (0, 1, 0), hits, inst, attr, base)
    _same_records(d_one.cpu().numpy().view(ATTR_DTYPE), want_a, "the launch before the swap")
    _same_records(d_two.cpu().numpy().view(ATTR_DTYPE), want_b, "the launch after the swap")
    assert (_bits(want_a) != _bits(want_b)).any(1).sum() > 500
    wd.sc.check()


def test_a_refit_keeps_the_table_and_waits_for_the_pass(trx, worlds):
    torch = _torch()
    wd = worlds("soup_52x44")
    normals = wd.use("random")
    (d_hits, d_inst, d_attr), (hits, inst, attr) = wd.frame((0, 1, 0))
    size = wd.w * wd.h
    bytes_before = wd.sc.device_bytes
    v = wd.flat.tri_verts
    moved = (v + np.random.default_rng(71).normal(scale=1e-3, size=v.shape)).astype(np.float32)
    s = torch.cuda.Stream()
    d_out = _buf(size * 24)
    _sync()
    try:
        with limit():
            with torch.cuda.stream(s):
                wd.sc.shading_normals_primary(wd.view, wd.w, wd.h, d_hits.data_ptr(), d_attr.data_ptr(), d_out.data_ptr(), d_inst=d_inst.data_ptr(),
                                              stream=s.cuda_stream)
            wd.sc.refit(moved)
            s.synchronize()
        want, _ = wd.primary_want(normals, (0, 1, 0), hits, inst, attr, np.full(size * 24, SENTINEL, dtype=np.uint8).view(ATTR_DTYPE))
        _same_records(d_out.cpu().numpy().view(ATTR_DTYPE), want, "the pass before the refit")
        assert wd.sc.get_vertex_normals().tobytes() == normals.tobytes()
        # (the refit's own state is counted from its first call on; the table is neither dropped nor counted twice)
        wd.sc.set_vertex_normals(None)
        without = wd.sc.device_bytes
        wd.sc.set_vertex_normals(normals)
        assert wd.sc.device_bytes - without == 48 * wd.n_tris and wd.sc.device_bytes >= bytes_before
        # the pass over the same caller records still answers from the kept table
        d_again = _buf(size * 24)
        wd.shade_primary((0, 1, 0), d_hits, d_inst, d_attr, d_again.data_ptr())
        _same_records(d_again.cpu().numpy().view(ATTR_DTYPE), want, "the pass after the refit")
    finally:
        with limit():
            wd.sc.refit(v)
            torch.cuda.synchronize()
    wd.sc.check()


def test_refusals_leave_the_output_untouched(trx, worlds):
    torch = _torch()
    wd = worlds("instanced")
    sc, view, w, h = wd.sc, wd.view, wd.w, wd.h
    (d_hits, d_inst, d_attr), _ = wd.frame((0, 1, 0))
    n = w * h
    d_out = _buf(n * 24)
    d_rays = _dev(random_rays(trx, wd.ray_box, n, 3))
    H, I, A, O, R = d_hits.data_ptr(), d_inst.data_ptr(), d_attr.data_ptr(), d_out.data_ptr(), d_rays.data_ptr()
    lights = [l.product(trx) for l in _mixed(1)]

    def refused(msg, call, *args, **kw):
        with pytest.raises(trx.TrxError, match=msg or None) as e:
            call(*args, **kw)
        assert e.value.code == -1, msg

    # no table: both entry points and both host forms
    sc.set_vertex_normals(None)
    wd.current = None
    refused("no vertex normals", sc.shading_normals_primary, view, w, h, H, A, O, d_inst=I)
    refused("no vertex normals", sc.shading_normals_rays, R, n, H, A, O, d_inst=I)
    refused("no vertex normals", sc.shading_normals_rays, R, 0, H, A, O, d_inst=I)
    refused("no vertex normals", sc.render_image_lit_smooth, view, w, h, lights)
    wd.use("random")
    # null buffers, a missing d_inst on the transformed scene, and what the attribute calls refuse of image and shard
    for hits_, attr_, out_ in ((0, A, O), (H, 0, O), (H, A, 0)):
        refused("null", sc.shading_normals_primary, view, w, h, hits_, attr_, out_, d_inst=I)
        refused("null", sc.shading_normals_rays, R, n, hits_, attr_, out_, d_inst=I)
    refused("null", sc.shading_normals_rays, 0, n, H, A, O, d_inst=I)
    refused("instance transforms", sc.shading_normals_primary, view, w, h, H, A, O)
    refused("instance transforms", sc.shading_normals_rays, R, n, H, A, O)
    for kw in ({"shard": (3, 3, 0)}, {"shard": (0, 1, 2)}):
        refused("", sc.shading_normals_primary, view, w, h, H, A, O, d_inst=I, **kw)
        refused("", sc.hit_attributes_primary_dev, view, w, h, H, O, d_inst=I, **kw)              # (the attribute call refuses the same)
    for ww, hh in ((0, h), (w, 0)):
        refused("", sc.shading_normals_primary, view, ww, hh, H, A, O, d_inst=I)
        refused("", sc.hit_attributes_primary_dev, view, ww, hh, H, O, d_inst=I)
    _sync()
    assert (d_out.cpu().numpy() == SENTINEL).all()
    with limit():
        sc.shading_normals_primary(view, w, h, H, A, O, d_inst=I)    # and the scene is still usable
        torch.cuda.synchronize()
    assert (d_out.cpu().numpy() != SENTINEL).any()
    sc.check()


# ---- composition ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cornell(trx):
    """The Cornell stand-in with its stand-in materials, its camera, and normals welded all round, in `prim` order."""
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    sc = trx.Scene(flat)
    mats, idx = trx.standin_materials("cornell", verts, counts)
    sc.set_materials(mats, idx[flat.tri_source])
    normals = trx.compute_vertex_normals(verts, CS.WELD_ALL)[flat.tri_source]
    eye, look, fov = trx.scene_camera("cornell")
    yield sc, flat, normals, eye, look, fov
    sc.close()


@pytest.mark.parametrize("w,h,shard", [(40, 24, (0, 1, 0)), (37, 21, (1, 3, 1))])
def test_light_term_over_the_pass_equals_the_twins(trx, cornell, w, h, shard):
    """trx_light_term_dev fed the pass's output against light_twin fed the twin's normals, for the device's own records."""
    torch = _torch()
    sc, flat, normals, eye, look, fov = cornell
    sc.set_vertex_normals(normals)
    view = trx.view_from_camera(eye, look, fov, w, h)
    lights, n = _mixed(8), 4
    (d_prim, d_inst, d_attr, d_lit), (prim, _, planes) = _frame(trx, sc, view, w, h, shard, lights, n)
    pix, rec, size = record_map(w, h, shard)
    attr = d_attr.cpu().numpy().view(ATTR_DTYPE)
    d_smooth, d_val = _buf(size * 24, 0), _buf(size * 4 + 64)
    with limit():
        sc.shading_normals_primary(view, w, h, d_prim.data_ptr(), d_attr.data_ptr(), d_smooth.data_ptr(), d_inst=d_inst.data_ptr(), shard=shard)
        sc.light_term_dev(view, w, h, [l.product(trx) for l in lights], d_prim.data_ptr(), d_smooth.data_ptr(), d_lit.data_ptr(), d_val.data_ptr(), n_samples=n,
                          ambient=0.25, shard=(*shard, 0))
        torch.cuda.synchronize()
    dirs = primary_dirs(view, w, h, pix % w, pix // w)
    out, cause = SN.shading_normals(normals, attr[rec], dirs, prim["prim"][pix], None, None)
    smooth = np.zeros((w * h, 3), dtype=np.float32)
    smooth[pix] = out["normal"]
    want = np.full(size * 4 + 64, SENTINEL, dtype=np.uint8)
    twin = LT.light_term(view, w, h, prim, smooth, planes, lights, n, 0.25, None)
    want[:size * 4].view(np.uint32)[rec] = twin.view(np.uint32)[pix]
    got = d_val.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%dx%d shard %s: %d bytes differ, first at %s" % (w, h, shard, bad.size, bad[:4])
    flat_normals = np.zeros((w * h, 3), dtype=np.float32)
    flat_normals[pix] = attr["normal"][rec]
    faceted = LT.light_term(view, w, h, prim, flat_normals, planes, lights, n, 0.25, None)
    assert (cause == SN.ADOPTED).sum() > 50 and (twin != faceted).sum() > 20       # (the smooth normals change the term)


def _chain(trx, sc, view, w, h, products, colour, smooth, sem, ao, radius, bn=0, stride=1, levels=0):
    """The host forms' chain from the device-resident calls: the RGBA8 image [h, w, 4]."""
    torch = _torch()
    from tray_racing_amd import _lib as L
    n, ls, phase, up = w * h, 4, stride * stride - 1, 1
    d_prim, d_inst, d_attr, d_lit = _buf(n * 8, 0xEE), _buf(n * 4, 0xFF), _buf(n * 24, 0), _buf(len(products) * n)
    d_cnt, d_term, d_val, d_rgba = _buf(n), _buf(n * 4), _buf(n * 4), _buf(n * 4)
    d_a, d_b, d_work = _buf(3 * n * 4), _buf(3 * n * 4), _buf(n * 4)
    P, I, A = d_prim.data_ptr(), d_inst.data_ptr(), d_attr.data_ptr()
    with limit():
        L.check(sc._lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, L.Shard(0, 1, 0, 0), sem, C.c_void_p(P), C.c_void_p(I), None))
        sc.hit_attributes_primary_dev(view, w, h, P, A, d_inst=I)
        if smooth:
            sc.shading_normals_primary(view, w, h, P, A, A, d_inst=I)
        sc.trace_light_visibility_dev(view, w, h, products, P, d_lit.data_ptr(), n_samples=ls, sem=sem, frame0=2, shadow_eps=EPS, d_primary_inst=I)
        if ao:
            sc.trace_ao_visibility_dev(view, w, h, P, d_cnt.data_ptr(), ao, radius, sem=sem, frame0=2, ao_eps=EPS, d_primary_inst=I)
            sc.ao_filter_dev(w, h, P, d_cnt.data_ptr(), d_term.data_ptr(), ao, 1, d_attr=A)
        sc.light_term_dev(view, w, h, products, P, A, d_lit.data_ptr(), d_val.data_ptr(), n_samples=ls, ambient=0.3, d_term=d_term.data_ptr() if ao else 0)
        if not colour:
            sc.shade_value_dev(d_val.data_ptr(), n, d_rgba.data_ptr())
        else:
            planes = 0
            if bn:
                planes, other = d_a.data_ptr(), d_b.data_ptr()
                if stride > 1:
                    sc.trace_indirect_rgb_sparse_dev(view, w, h, stride, phase, products, P, planes, n_samples=bn, sem=sem, frame0=2, bounce_eps=EPS,
                                                     shadow_eps=EPS, d_primary_inst=I)
                    n_lo = ((w + stride - 1) // stride) * ((h + stride - 1) // stride)
                    for c in range(3):
                        sc.value_upsample_dev(w, h, stride, phase, P, planes + c * n_lo * 4, other + c * n * 4, up, d_attr=A)
                    planes, other = other, planes
                else:
                    sc.trace_indirect_rgb_dev(view, w, h, products, P, planes, n_samples=bn, sem=sem, frame0=2, bounce_eps=EPS, shadow_eps=EPS, d_primary_inst=I)
                if levels:
                    for c in range(3):
                        sc.value_filter_dev(w, h, P, planes + c * n * 4, other + c * n * 4, levels, d_attr=A, d_work=d_work.data_ptr())
                    planes, other = other, planes
            colour_at = planes or d_a.data_ptr()
            sc.material_compose_dev(P, d_val.data_ptr(), n, colour_at, d_indirect_rgb=planes)
            sc.shade_rgb_dev(colour_at, n, d_rgba.data_ptr())
        torch.cuda.synchronize()
    return d_rgba.cpu().numpy().reshape(h, w, 4)


def _images(trx, world):
    """(scene, view, w, h, AO radius, normals in `prim` order) of a composition case: the Cornell stand-in, or the transformed scene."""
    if isinstance(world, tuple):
        sc, flat, normals, eye, look, fov = world
        return sc, trx.view_from_camera(eye, look, fov, 48, 32), 48, 32, 1.4, normals
    if not getattr(world, "has_materials", False):
        mats, idx = MT.seeded_table(world.n_tris, 5, 11)
        world.sc.set_materials(mats, idx)
        world.has_materials = True
    return world.sc, world.view, world.w, world.h, 1.6, world.table("computed")


@pytest.mark.parametrize("which", ["cornell", "instanced"])
def test_smooth_host_forms_are_their_compositions(trx, worlds, cornell, which):
    """render_image_lit_smooth and render_image_colour_smooth (dense, and sparse + upsample + filter: every filter and upsample
    call reads the shading attributes) against the same chain from the _dev calls, byte for byte; they differ from the plain
    forms; with an all-zero table every record falls back and they ARE the plain forms, byte for byte."""
    world = cornell if which == "cornell" else worlds("instanced")
    sc, view, w, h, radius, normals = _images(trx, world)
    products = [l.product(trx) for l in _mixed(3)]
    sem, ao = 3, 4
    lit_kw = dict(sem=sem, frame0=2, light_samples=4, shadow_eps=EPS, ambient=0.3, ao_samples=ao, ao_eps=EPS, ao_radius=radius, filter_radius=1)
    col_kws = [dict(lit_kw, bounce_samples=0), dict(lit_kw, bounce_samples=2, bounce_eps=EPS),
               dict(lit_kw, bounce_samples=2, bounce_eps=EPS, bounce_stride=2, bounce_phase=3, bounce_upsample_radius=1, bounce_filter_levels=2)]
    try:
        sc.set_vertex_normals(normals)
        with limit():
            lit, ms = sc.render_image_lit_smooth(view, w, h, products, **lit_kw)
            plain, _ = sc.render_image_lit(view, w, h, products, **lit_kw)
        assert ms > 0 and (lit == _chain(trx, sc, view, w, h, products, False, True, sem, ao, radius)).all()
        assert (plain == _chain(trx, sc, view, w, h, products, False, False, sem, ao, radius)).all() and (lit != plain).sum() > 20
        cols = []
        for kw in col_kws:
            with limit():
                img, _ = sc.render_image_colour_smooth(view, w, h, products, **kw)
            want = _chain(trx, sc, view, w, h, products, True, True, sem, ao, radius, bn=kw["bounce_samples"], stride=kw.get("bounce_stride", 1),
                          levels=kw.get("bounce_filter_levels", 0))
            assert (img == want).all(), (which, kw, int((img != want).sum()))
            assert (img[..., 3] == 255).all()
            cols.append(img)
        with limit():
            assert (cols[0] != sc.render_image_colour(view, w, h, products, **col_kws[0])[0]).sum() > 20
        # all zero: every record falls back
        sc.set_vertex_normals(np.zeros_like(normals))
        with limit():
            assert (sc.render_image_lit_smooth(view, w, h, products, **lit_kw)[0] == plain).all()
            for kw in col_kws:
                assert (sc.render_image_colour_smooth(view, w, h, products, **kw)[0] == sc.render_image_colour(view, w, h, products, **kw)[0]).all(), kw
        # refused without a table, like the pass itself
        sc.set_vertex_normals(None)
        for call, kw in ((sc.render_image_lit_smooth, lit_kw), (sc.render_image_colour_smooth, col_kws[1])):
            with pytest.raises(trx.TrxError, match="no vertex normals") as e:
                call(view, w, h, products, **kw)
            assert e.value.code == -1
        sc.check()
    finally:
        if which == "instanced":
            world.current = None


# ---- power-of-two scene scaling ---------------------------------------------------------------------------------------------------------------

def _scaled_outputs(trx, s, f, normals_source, w2o_of):
    """{"primary": components, "rays": components} of the pass over caller records `f` of tree `s`, and the twin's."""
    torch = _torch()
    sc = trx.Scene(s.flat)
    try:
        normals = np.ascontiguousarray(normals_source[s.flat.tri_source])
        sc.set_vertex_normals(normals)
        w2o = sc.instance_world_to_object() if s.tlas else None
        n = s.w * s.h
        recs = tri_records(s.flat.tri_verts)
        d_prim, d_inst, d_brays, d_bhits, d_binst = _dev(f.prim), _dev(f.inst), _dev(f.b_rays), _dev(f.b_hits), _dev(f.b_inst)
        d_attr, d_battr, d_out, d_bout = _buf(n * 24), _buf(n * 24), _buf(n * 24 + GUARD), _buf(n * 24 + GUARD)
        _sync()
        with limit():
            sc.hit_attributes_primary_dev(s.view, s.w, s.h, d_prim.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr())
            sc.shading_normals_primary(s.view, s.w, s.h, d_prim.data_ptr(), d_attr.data_ptr(), d_out.data_ptr(), d_inst=d_inst.data_ptr())
            sc.hit_attributes_rays_dev(d_brays.data_ptr(), n, d_bhits.data_ptr(), d_battr.data_ptr(), d_inst=d_binst.data_ptr())
            sc.shading_normals_rays(d_brays.data_ptr(), n, d_bhits.data_ptr(), d_battr.data_ptr(), d_bout.data_ptr(), d_inst=d_binst.data_ptr())
            torch.cuda.synchronize()
            sc.check()
        outs, twins, changed = {}, {}, {}
        px, py = np.arange(n) % s.w, np.arange(n) // s.w
        with np.errstate(all="ignore"):
            pdirs = primary_dirs(s.view, s.w, s.h, px, py)
        for name, d_o, d_a, dirs, prims, inst in (("primary", d_out, d_attr, pdirs, f.prim["prim"], f.inst), ("rays", d_bout, d_battr, f.b_rays["direction"], f.b_hits["prim"], f.b_inst)):
            raw = d_o.cpu().numpy()
            assert (raw[n * 24:] == SENTINEL).all()
            got, attr = raw[:n * 24].view(ATTR_DTYPE), d_a.cpu().numpy().view(ATTR_DTYPE)
            want, cause = SN.shading_normals(normals, attr, dirs, prims, inst, w2o)
            outs[name], twins[name] = ST.attr_of(got), ST.attr_of(want)
            changed[name] = int((_bits(got) != _bits(attr)).any(1).sum())
            assert (got["_pad"][cause == SN.ADOPTED] == 0).all()
        return outs, twins, changed
    finally:
        sc.close()


@pytest.fixture(scope="module")
def scale_bases(trx, orc):
    made = {}

    def get(case):
        if case not in made:
            base = SC.recentred(trx, *case)
            s0, p0 = SC.scaled(trx, base, 0), SC.scaled_params(base, 0)
            f0 = ST.base_frame(orc, s0, p0)
            normals_source = trx.compute_vertex_normals(base.verts, CS.WELD_ALL)
            rng = np.random.default_rng(77)
            normals_source[::3] = rng.normal(size=(normals_source[::3].shape)).astype(np.float32)      # (every third triangle: random, unnormalised)
            dev0, twin0, changed = _scaled_outputs(trx, s0, f0, normals_source, None)
            for name in dev0:
                SC.assert_same(dev0[name], twin0[name], "%s k 0 %s, device against twin" % (case[0], name))
                assert changed[name] > 10, (case, name, changed)
            made[case] = (base, s0, f0, normals_source, dev0)
        return made[case]
    return get


@pytest.mark.parametrize("k", SC.SAFE)
@pytest.mark.parametrize("case", SC.CASES[:2], ids=["%s_%dx%d" % c for c in SC.CASES[:2]])
def test_scaled_scenes_give_the_unit_scale_normals(trx, orc, scale_bases, case, k):
    """The scene, the eye (the origin), the caller's t and the rays' origins times 2^k; the vertex normals as they were: every
    output record - u, v and the normal, adopted or not - holds the k = 0 bits, and is the twin's at k."""
    base, s0, f0, normals_source, dev0 = scale_bases(case)
    s = SC.scaled(trx, base, k)
    f = ST.carried_frame(orc, s0, f0, s)
    dev, twin, _ = _scaled_outputs(trx, s, f, normals_source, None)
    for name in dev:
        SC.assert_same(dev[name], twin[name], "%s k %d %s, device against twin" % (case[0], k, name))
        SC.assert_same(dev[name], dev0[name], "%s k %d %s, device against its own k = 0 output" % (case[0], k, name))
