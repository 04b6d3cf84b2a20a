"""The textured albedo on the GPU, bit for bit (include/trx.h, "texture coordinates and albedo textures"):
trx_surface_albedo_dev writes the twin's planes (tests/texture_twin.py) - fed the device's own hits and attribute records - on
the four golden scenes under stand-in, random and hostile tables, in both layouts and two shards and over explicit rays;
three equalities no twin takes part in (the albedo compose over the plain albedo IS the material compose; all-255 textures ARE
no textures; the textured indirect pass on a scene without textures IS each of the four existing RGB passes); the textured
indirect pass against the twin, dense and sparse, rules 5c and 5e, under a scratch cap that forces several chunks; caller
records; the tables' life; the textured host image against its chain and against the untextured host images; power-of-two
scene scaling.  Whole buffers are compared, sentinel bytes and guards included.

Every step that runs on the GPU sits under a time limit of its own (`limit`): a step that hangs ends the process."""
import ctypes as C

import numpy as np
import pytest

import caller_records as CR
import emitter_twin as ET
import indirect_twin as IT
import material_twin as MT
import scale_cases as SC
import texture_cases as TC
import texture_twin as TT
from ao_visibility_twin import record_map
from helpers import random_rays
from hit_attr_twin import ATTR_DTYPE
from test_gpu_emitters import EEPS, GI_UNIT, Em
from test_gpu_ao_visibility import make_case
from test_gpu_light import EPS, _mixed, _sync, _torch, limit
from test_gpu_shading_normals import World

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = 0xAB
GUARD = 48
HIT = np.dtype([("t", "<f4"), ("prim", "<u4")])
SHARDS = ((0, 1, 0), (0, 1, 1), (1, 3, 0), (1, 3, 1))
BOUNCE_UNIT = 64 * (32 + 1) + 64 * (32 + 8 + 4 + 24 + 4 + 4)     # kernels.h, kBounceUnitBytes


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _buf(nbytes, fill=SENTINEL):
    return _torch().full((max(nbytes, 1),), fill, dtype=_torch().uint8, device="cuda")


def _same(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.size == want.size, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d bytes differ, first at %s: %s != %s" % (what, bad.size, got.size, bad[:4], got[bad[:4]], want[bad[:4]])


class Tex:
    """A World of tests/test_gpu_shading_normals.py with materials and the texture tables of texture_cases on it."""

    def __init__(self, world):
        self.wd, self.sc, self.n_tris = world, world.sc, world.n_tris
        self.mat, self.idx = TC.materials(self.n_tris)
        self.sc.set_materials(self.mat, self.idx)
        self.made, self.current = {}, "none"

    def table(self, kind):
        if kind not in self.made:
            self.made[kind] = TC.tables(kind, self.wd.recs)
        return self.made[kind]

    def use(self, kind):
        """kind: a name of texture_cases.TABLES, or None for no tables at all; returns (uvs, TexSet) or (None, None)."""
        if kind is None:
            if self.current is not None:
                self.sc.set_texcoords(None)
                self.sc.set_textures(None, None, None)
            self.current = None
            return None, None
        uvs, ts = self.table(kind)
        if self.current != kind:
            self.sc.set_texcoords(uvs)
            self.sc.set_textures(ts.descs, ts.texels, ts.material_texture)
            self.current = kind
        return uvs, ts

    def albedo(self, d_hits, d_attr, n, stream=0):
        """The whole output buffer of trx_surface_albedo_dev over n records: guards either side of the three planes."""
        d_out = _buf(3 * n * 4 + 2 * GUARD)
        _sync()
        with limit():
            self.sc.surface_albedo_dev(d_hits.data_ptr(), d_attr.data_ptr(), n, d_out.data_ptr() + GUARD, stream=stream)
            _torch().cuda.synchronize()
        return d_out.cpu().numpy()

    def want(self, hits, attr, uvs, ts):
        planes, cause = TT.surface_albedo(hits, attr, self.mat, self.idx, self.n_tris, uvs, ts)
        guard = np.full(GUARD, SENTINEL, dtype=np.uint8)
        return np.concatenate([guard, planes.reshape(-1).view(np.uint8), guard]), cause


@pytest.fixture(scope="module")
def texs(trx, orc):
    worlds, made = {}, {}

    def get(name):
        if name not in made:
            worlds[name] = World(trx, orc, name)
            made[name] = Tex(worlds[name])
        return made[name]
    yield get
    for w in worlds.values():
        w.close()


# ---- trx_surface_albedo_dev against the twin -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", TC.TABLES)
@pytest.mark.parametrize("name", TC.SCENES)
def test_albedo_planes_equal_the_twin(trx, texs, name, kind):
    """Primary frames in both layouts with shards {0, 1} and {1, 3} - the pass is elementwise over the whole buffer, so the
    records the shard does not own (the frame's fill bytes: a prim outside the scene) are background - and explicit rays."""
    tx = texs(name)
    uvs, ts = tx.use(kind)
    wd = tx.wd
    seen = set()
    for shard in SHARDS:
        (d_hits, d_inst, d_attr), (hits, inst, attr) = wd.frame(shard)
        size = hits.shape[0]
        want, cause = tx.want(hits, attr, uvs, ts)
        _same(tx.albedo(d_hits, d_attr, size), want, "%s %s shard %s" % (name, kind, shard))
        seen |= set(cause.tolist())
        if shard[1] == 1:
            assert (cause == TT.TEXTURED).sum() > 30, (name, kind, np.bincount(cause))
    torch = _torch()
    rays = random_rays(trx, wd.ray_box, 4099, 23)
    n = rays.shape[0]
    d_rays, d_hits, d_inst, d_attr = _dev(rays), _buf(n * 8), _buf(n * 4, 0xFF), _buf(n * 24)
    with limit():
        wd.sc.trace_rays_inst_dev(d_rays.data_ptr(), n, d_hits.data_ptr(), d_inst=d_inst.data_ptr())
        wd.sc.hit_attributes_rays_dev(d_rays.data_ptr(), n, d_hits.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr())
        torch.cuda.synchronize()
    hits, attr = d_hits.cpu().numpy().view(HIT), d_attr.cpu().numpy().view(ATTR_DTYPE)
    want, cause = tx.want(hits, attr, uvs, ts)
    _same(tx.albedo(d_hits, d_attr, n), want, "%s %s explicit rays" % (name, kind))
    seen |= set(cause.tolist())
    assert {TT.BACKGROUND, TT.TEXTURED, TT.NO_TEXTURE_FOR_MATERIAL} <= seen, seen
    if kind == "hostile":
        assert TT.NOT_FINITE in seen
    wd.sc.check()


# ---- three equalities no twin takes part in ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", TC.SCENES)
def test_compose_over_the_plain_albedo_is_the_material_compose(trx, texs, name):
    """No texture set (without and with texcoords), and a texture set without texcoords: trx_albedo_compose_dev over
    trx_surface_albedo_dev's planes equals trx_material_compose_dev bit for bit - with an indirect term, in place on it, and
    without one."""
    tx = texs(name)
    wd, sc = tx.wd, tx.sc
    (d_hits, d_inst, d_attr), (hits, inst, attr) = wd.frame((0, 1, 0))
    n = hits.shape[0]
    rng = np.random.default_rng(8)
    E, I = rng.uniform(0.0, 1.5, n).astype(np.float32), rng.uniform(0.0, 2.0, (3, n)).astype(np.float32)
    d_E = _dev(E)
    uvs, ts = tx.table("random")
    for uv_set, tex_set in ((False, False), (True, False), (False, True)):
        tx.use(None)
        tx.current = "mixed"
        if uv_set:
            sc.set_texcoords(uvs)
        if tex_set:
            sc.set_textures(ts.descs, ts.texels, ts.material_texture)
        what = "%s texcoords %s textures %s" % (name, uv_set, tex_set)
        d_alb = _buf(3 * n * 4)
        d_want, d_got, d_want0, d_got0 = _dev(I), _dev(I), _buf(3 * n * 4), _buf(3 * n * 4)
        with limit():
            sc.surface_albedo_dev(d_hits.data_ptr(), d_attr.data_ptr(), n, d_alb.data_ptr())
            sc.material_compose_dev(d_hits.data_ptr(), d_E.data_ptr(), n, d_want.data_ptr(), d_indirect_rgb=d_want.data_ptr())
            sc.albedo_compose_dev(d_hits.data_ptr(), d_alb.data_ptr(), d_E.data_ptr(), n, d_got.data_ptr(), d_indirect_rgb=d_got.data_ptr())
            sc.material_compose_dev(d_hits.data_ptr(), d_E.data_ptr(), n, d_want0.data_ptr())
            sc.albedo_compose_dev(d_hits.data_ptr(), d_alb.data_ptr(), d_E.data_ptr(), n, d_got0.data_ptr())
            _torch().cuda.synchronize()
        _same(d_got.cpu().numpy(), d_want.cpu().numpy(), what + ": in place on the indirect planes")
        _same(d_got0.cpu().numpy(), d_want0.cpu().numpy(), what + ": no indirect term")
        assert (d_want.cpu().numpy().view(np.float32) != 0).sum() > 100
        # ... and the twin says the same of both
        alb = d_alb.cpu().numpy().view(np.float32).reshape(3, n)
        _same(d_got.cpu().numpy(), TT.albedo_compose(hits, alb, E, I, tx.mat, tx.idx, tx.n_tris), what + ": the twin")
        _same(d_want0.cpu().numpy(), MT.compose(hits, E, None, tx.mat, tx.idx, tx.n_tris), what + ": the material twin")
    tx.use(None)
    sc.check()


@pytest.mark.parametrize("name", ["cornell_64", "kitchen_tlas_f16_56x40"])
def test_all_255_textures_are_no_textures(trx, texs, name):
    """Every texel 255 in every channel: val is exactly 1 under both filters and both formats, so the planes are the planes of
    a scene without textures, bit for bit."""
    tx = texs(name)
    wd, sc = tx.wd, tx.sc
    (d_hits, d_inst, d_attr), (hits, inst, attr) = wd.frame((0, 1, 0))
    n = hits.shape[0]
    tx.use(None)
    plain = tx.albedo(d_hits, d_attr, n)
    assert (plain[GUARD:-GUARD].view(np.float32) != 0).sum() > 100
    uvs, _ = tx.table("random")
    tx.current = "mixed"
    sc.set_texcoords(uvs)
    for filt in (TT.NEAREST, TT.BILINEAR):
        for fmt in (TT.UNORM, TT.SRGB):
            ts = TT.white_textures(TC.N_MATERIALS, filt, fmt)
            sc.set_textures(ts.descs, ts.texels, ts.material_texture)
            _same(tx.albedo(d_hits, d_attr, n), plain, "%s filter %d format %d" % (name, filt, fmt))
    tx.use(None)
    sc.check()


def _indirect(sc, trx, view, w, h, lights, d_prim, d_inst, n, size, textured, stride, emitters, frame0=3, sem=0):
    before = np.full(3 * size * 4 + 64, 0x5A, dtype=np.uint8)
    d_out = _dev(before)
    _sync()
    products = [l.product(trx) for l in lights]
    kw = dict(n_samples=n, sem=sem, frame0=frame0, bounce_eps=EPS, shadow_eps=EPS, d_primary_inst=d_inst.data_ptr() if d_inst is not None else 0)
    with limit():
        if textured:
            sc.trace_indirect_rgb_textured_dev(view, w, h, products, d_prim.data_ptr(), d_out.data_ptr(), stride=stride, phase=stride * stride - 1,
                                               use_emitters=emitters, emitter_eps=EEPS, **kw)
        elif stride > 1 and emitters:
            sc.trace_indirect_rgb_emitters_sparse_dev(view, w, h, stride, stride * stride - 1, products, d_prim.data_ptr(), d_out.data_ptr(),
                                                      emitter_eps=EEPS, **kw)
        elif stride > 1:
            sc.trace_indirect_rgb_sparse_dev(view, w, h, stride, stride * stride - 1, products, d_prim.data_ptr(), d_out.data_ptr(), **kw)
        elif emitters:
            sc.trace_indirect_rgb_emitters_dev(view, w, h, products, d_prim.data_ptr(), d_out.data_ptr(), emitter_eps=EEPS, **kw)
        else:
            sc.trace_indirect_rgb_dev(view, w, h, products, d_prim.data_ptr(), d_out.data_ptr(), **kw)
        _torch().cuda.synchronize()
        sc.check()
    return d_out.cpu().numpy(), before


@pytest.fixture(scope="module")
def ems(trx, orc):
    """test_gpu_emitters' Em (a Case with the Cornell stand-in materials and the emitter tables, twin's and device's)."""
    made, got = {}, {}

    def get(name):
        if name not in got:
            got[name] = Em(trx, make_case(trx, orc, made, name))
        return got[name]
    yield get
    trx.load().trx_debug_ao_scratch_cap(0)
    for c in made.values():
        c.close()


@pytest.mark.parametrize("name", ["cornell_64", "cornell_tlas_48"])
def test_textured_indirect_without_textures_is_each_existing_pass(trx, ems, name):
    """No tables, texcoords alone, textures alone: trx_trace_indirect_rgb_textured_dev equals the four existing entry points bit
    for bit (dense and stride 2, with and without emitters)."""
    em = ems(name)
    case, sc = em.case, em.case.sc
    with limit():
        d_prim, d_inst, prim, inst = case.primary(0)
    lights, w, h = _mixed(2), em.w, em.h
    uvs = TT.random_uvs(case.sc.flat.tri_verts.shape[0], 4)
    ts = TT.random_textures(em.mats.shape[0], 4)
    try:
        for state in ("none", "texcoords", "textures"):
            if state == "texcoords":
                sc.set_texcoords(uvs)
            if state == "textures":
                sc.set_texcoords(None)
                sc.set_textures(ts.descs, ts.texels, ts.material_texture)
            for stride in (1, 2):
                size = ((w + stride - 1) // stride) * ((h + stride - 1) // stride)
                for emitters in (False, True):
                    got, _ = _indirect(sc, trx, case.view, w, h, lights, d_prim, d_inst, 3, size, True, stride, emitters)
                    want, before = _indirect(sc, trx, case.view, w, h, lights, d_prim, d_inst, 3, size, False, stride, emitters)
                    _same(got, want, "%s %s stride %d emitters %s" % (name, state, stride, emitters))
                    assert (want != before).sum() > 1000
    finally:
        sc.set_texcoords(None)
        sc.set_textures(None, None, None)


# ---- the textured indirect pass against the twin ----------------------------------------------------------------------------------------

def _twin_samples(em, prim, inst, lights, frame0, n, sem):
    """Per sample (s_f, surface, bounce prim, bounce attr, X [3, n]): rules 1-4 from indirect_twin, E2-E4 from emitter_twin."""
    orc, osc, w, h = em.case.orc, em.case.osc, em.w, em.h
    occluded = IT.oracle_occluded(osc, sem)
    out = []
    for f in range(n):
        rays, hits, _, attr = IT.bounce(orc, osc, em.case.oview, w, h, prim, inst, em.recs, em.w2o, frame0 + f, EPS, sem)
        s = IT.sample_sum(orc, w, h, rays, hits, attr, lights, frame0, f, EPS, occluded)
        e_rays, cast, wgeo, j = ET.bounce_rays(orc, w, h, rays, hits, attr, em.rec, em.c, frame0, f, EPS, EEPS)
        lit = cast & ~np.asarray(occluded(0, e_rays), dtype=bool)
        Le = ET._emission(em.rec, em.mats, j)
        with np.errstate(invalid="ignore", over="ignore"):
            X = [np.where(lit, (wgeo * Le[:, ch]).astype(np.float32), f32(0.0)).astype(np.float32) for ch in range(3)]
        out.append((s, IT.bounce_surface(rays, hits), np.asarray(hits["prim"], dtype=np.uint32), attr, X))
    return out


@pytest.mark.parametrize("name", ["cornell_64", "cornell_tlas_48"])
def test_textured_indirect_equals_the_twin(trx, ems, name):
    """Rules 5c and 5e with the sampled albedo, dense and sparse at stride 2, under a scratch cap that forces several tile and
    sample chunks.  The twin is material_twin's / emitter_twin's gather with texture_twin's albedo: without tables it IS theirs."""
    em = ems(name)
    case, sc = em.case, em.case.sc
    with limit():
        d_prim, d_inst, prim, inst = case.primary(0)
    lights, w, h, n, frame0 = _mixed(2), em.w, em.h, 3, 3
    samples = _twin_samples(em, prim, inst, lights, frame0, n, 0)
    plain = [x[:3] for x in samples]
    _same(TT.term_rgb([x[:4] for x in samples], prim, em.mats, em.idx, em.n_tris, None, None), MT.term_rgb(plain, prim, em.mats, em.idx, em.n_tris),
          "the twin without tables: rule 5c")
    _same(TT.term_rgb_emitters(samples, prim, em.mats, em.idx, em.n_tris, None, None),
          ET.indirect_rgb_emitters(case.orc, case.osc, case.oview, w, h, prim, inst, em.recs, em.w2o, lights, frame0, n, EPS, EPS, EEPS, 0, em.mats, em.idx,
                                   em.rec, em.c), "the twin without tables: rule 5e")
    uvs = TT.random_uvs(em.n_tris, 4)
    ts = TT.random_textures(em.mats.shape[0], 4)
    ts = ts._replace(material_texture=np.array([5, 10, TT.NO_TEXTURE, 15][:em.mats.shape[0]], dtype=np.uint32))   # (bilinear sRGB / UNORM; one material bare)
    dev_uvs = np.zeros((sc.flat.tri_verts.shape[0], 6), dtype=np.float32)
    dev_uvs[:em.n_tris] = uvs
    lib = trx.load()
    try:
        sc.set_texcoords(dev_uvs)
        sc.set_textures(ts.descs, ts.texels, ts.material_texture)
        for emitters in (False, True):
            unit = GI_UNIT if emitters else BOUNCE_UNIT
            lib.trx_debug_ao_scratch_cap(unit * 5 * 2)          # five tiles, two of the three samples per chunk
            dense = (TT.term_rgb_emitters(samples, prim, em.mats, em.idx, em.n_tris, uvs, ts) if emitters
                     else TT.term_rgb([x[:4] for x in samples], prim, em.mats, em.idx, em.n_tris, uvs, ts))
            untextured = TT.term_rgb_emitters(samples, prim, em.mats, em.idx, em.n_tris, None, None) if emitters else MT.term_rgb(plain, prim, em.mats, em.idx, em.n_tris)
            assert (dense.view(np.uint32) != untextured.view(np.uint32)).sum() > 500
            for stride in (1, 2):
                want_planes = dense if stride == 1 else MT.sparse_rgb(dense, w, h, stride, stride * stride - 1)
                size = want_planes.shape[1]
                got, before = _indirect(sc, trx, case.view, w, h, lights, d_prim, d_inst, n, size, True, stride, emitters, frame0=frame0)
                want = before.copy()
                want[:3 * size * 4] = np.ascontiguousarray(want_planes).reshape(-1).view(np.uint8)
                _same(got, want, "%s emitters %s stride %d" % (name, emitters, stride))
    finally:
        lib.trx_debug_ao_scratch_cap(0)
        sc.set_texcoords(None)
        sc.set_textures(None, None, None)


# ---- caller records -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell_64", "cornell_tlas_48"])
def test_caller_records_through_both_elementwise_passes(trx, texs, name):
    """The id table of tests/caller_records.py as explicit records, doctored into a frame, and a frame of sentinel bytes:
    trx_surface_albedo_dev and trx_albedo_compose_dev against the twins, whole buffers - a record whose prim is no triangle of
    the scene is background whatever else it holds, and u, v are used as they come."""
    tx = texs(name)
    wd, sc = tx.wd, tx.sc
    uvs, ts = tx.use("random")
    (d_hits, d_inst, d_attr), (hits, inst, attr) = wd.frame((0, 1, 0))
    n = hits.shape[0]
    table = CR.entries(tx.n_tris)
    rng = np.random.default_rng(31)
    explicit = np.zeros(len(table), dtype=HIT)
    for k, (t, t_ok, p, p_ok, _, _) in enumerate(table):
        explicit["t"][k], explicit["prim"][k] = (f32(0.5) if t is CR.OWN else t), p
    e_attr = np.zeros(len(table), dtype=ATTR_DTYPE)
    e_attr["u"], e_attr["v"] = rng.uniform(0, 1, len(table)).astype(np.float32), rng.uniform(0, 1, len(table)).astype(np.float32)
    e_attr["u"][::5], e_attr["v"][1::7], e_attr["u"][2::9] = np.nan, np.inf, f32(-3e38)
    surface = (hits["t"] < CR.FLT_MAX) & (hits["prim"] < tx.n_tris)
    pixels, _ = CR.pick_pixels(wd.w, wd.h, len(table), surface)
    doctored, _, _, _, is_surface = CR.doctor(hits, None, pixels, table)
    sentinel_hits, sentinel_attr = np.full(n * 8, SENTINEL, dtype=np.uint8).view(HIT), np.full(n * 24, SENTINEL, dtype=np.uint8).view(ATTR_DTYPE)
    assert is_surface.any()
    for what, h_, a_ in (("explicit", explicit, e_attr), ("doctored", doctored, attr), ("sentinel", sentinel_hits, sentinel_attr)):
        m = h_.shape[0]
        d_h, d_a = _dev(h_), _dev(a_)
        want, cause = tx.want(h_, a_, uvs, ts)
        got = tx.albedo(d_h, d_a, m)
        _same(got, want, "%s %s: the albedo" % (name, what))
        E, I = rng.uniform(0, 1, m).astype(np.float32), rng.uniform(0, 1, (3, m)).astype(np.float32)
        alb = got[GUARD:-GUARD].view(np.float32).reshape(3, m)
        d_alb, d_E, d_I, d_col = _dev(alb), _dev(E), _dev(I), _buf(3 * m * 4 + 2 * GUARD)
        with limit():
            sc.albedo_compose_dev(d_h.data_ptr(), d_alb.data_ptr(), d_E.data_ptr(), m, d_col.data_ptr() + GUARD, d_indirect_rgb=d_I.data_ptr())
            _torch().cuda.synchronize()
        guard = np.full(GUARD, SENTINEL, dtype=np.uint8)
        colour = TT.albedo_compose(h_, alb, E, I, tx.mat, tx.idx, tx.n_tris)
        _same(d_col.cpu().numpy(), np.concatenate([guard, colour.reshape(-1).view(np.uint8), guard]), "%s %s: the compose" % (name, what))
        if what == "sentinel":
            assert (cause == TT.BACKGROUND).all() and not colour.any()
        else:
            assert (cause == TT.BACKGROUND).any() and (cause != TT.BACKGROUND).any()
    sc.check()


# ---- the tables' life -----------------------------------------------------------------------------------------------------------------------

def test_set_get_round_trip_accounting_and_refusals(trx, texs):
    tx = texs("soup_52x44")
    sc, n = tx.sc, tx.n_tris
    tx.use(None)
    lib = trx.load()
    for getter, msg in ((sc.get_texcoords, "no texture coordinates"), (sc.get_textures, "no textures")):
        with pytest.raises(trx.TrxError, match=msg):
            getter()
    before = sc.device_bytes
    uvs, ts = tx.table("hostile")
    sc.set_texcoords(uvs)
    assert sc.device_bytes - before == 24 * n and sc.get_texcoords().tobytes() == uvs.tobytes()
    sc.set_texcoords(tx.table("random")[0])                                   # replaced: counted once
    assert sc.device_bytes - before == 24 * n and sc.get_texcoords().tobytes() == tx.table("random")[0].tobytes()
    sc.set_textures(ts.descs, ts.texels, ts.material_texture)
    tex_bytes = 16 * ts.descs.shape[0] + 4 * ts.texels.size + 4 * TC.N_MATERIALS + 1024
    assert sc.device_bytes - before == 24 * n + tex_bytes
    d, t, m = sc.get_textures()
    assert TT.texset(d, t, m).descs.tobytes() == ts.descs.tobytes() and t.tobytes() == ts.texels.tobytes() and m.tobytes() == ts.material_texture.tobytes()
    other = tx.table("standin")[1]
    sc.set_textures(other.descs, other.texels, other.material_texture)         # replaced: counted once
    assert sc.device_bytes - before == 24 * n + 16 + 4 * 4096 + 4 * TC.N_MATERIALS + 1024
    sc.set_textures(ts.descs, ts.texels, ts.material_texture)
    # every refusal that needs the scene leaves both tables in force (the others: tests/test_textures.py)
    P = lambda a: a.ctypes.data_as(C.c_void_p)    # noqa: E731
    big = ts.material_texture.copy()
    big[2] = ts.descs.shape[0]
    for args in ((P(ts.descs), ts.descs.shape[0], P(ts.texels), ts.texels.size, P(ts.material_texture), TC.N_MATERIALS - 1),
                 (P(ts.descs), ts.descs.shape[0], P(ts.texels), ts.texels.size, P(ts.material_texture), TC.N_MATERIALS + 1),
                 (P(ts.descs), ts.descs.shape[0], P(ts.texels), ts.texels.size, P(big), TC.N_MATERIALS),
                 (P(ts.descs), ts.descs.shape[0], P(ts.texels), ts.texels.size - 1, P(ts.material_texture), TC.N_MATERIALS)):
        assert lib.trx_scene_set_textures(sc.handle, *args) == -1, args[1::2]
    for bad_n in (n - 1, n + 1):
        assert lib.trx_scene_set_texcoords(sc.handle, P(uvs), bad_n) == -1 and b"n_tris" in lib.trx_last_error()
        assert lib.trx_scene_get_texcoords(sc.handle, P(np.zeros((n + 1, 6), dtype=np.float32)), bad_n) == -1
    d, t, m = sc.get_textures()
    assert t.tobytes() == ts.texels.tobytes() and m.tobytes() == ts.material_texture.tobytes()
    assert sc.get_texcoords().tobytes() == tx.table("random")[0].tobytes() and sc.device_bytes - before == 24 * n + tex_bytes
    # materials replaced with the same count keep the set, with another count drop it; texcoords stay
    sc.set_materials(tx.mat, tx.idx)
    assert sc.get_textures()[1].tobytes() == ts.texels.tobytes()
    mat8, idx8 = MT.seeded_table(n, TC.N_MATERIALS + 1, 3)
    sc.set_materials(mat8, idx8)
    with pytest.raises(trx.TrxError, match="no textures"):
        sc.get_textures()
    assert sc.get_texcoords().tobytes() == tx.table("random")[0].tobytes()
    sc.set_materials(tx.mat, tx.idx)
    assert sc.device_bytes - before == 24 * n
    # a scene without materials takes no textures
    bare = trx.Scene(tx.wd.flat)
    try:
        with pytest.raises(trx.TrxError, match="no materials"):
            bare.set_textures(ts.descs, ts.texels, ts.material_texture)
        bare.set_texcoords(uvs)                                               # (texcoords need none)
        d_h, d_a, d_o = _buf(64 * 8), _buf(64 * 24), _buf(3 * 64 * 4)
        for call in (lambda: bare.surface_albedo_dev(d_h.data_ptr(), d_a.data_ptr(), 64, d_o.data_ptr()),
                     lambda: bare.albedo_compose_dev(d_h.data_ptr(), d_o.data_ptr(), d_o.data_ptr(), 64, d_o.data_ptr())):
            with pytest.raises(trx.TrxError, match="no materials"):
                call()
        _sync()
        assert (d_o.cpu().numpy() == SENTINEL).all()
    finally:
        bare.close()
    tx.current = "mixed"
    tx.use(None)
    assert sc.device_bytes == before
    sc.set_textures(None, None, None)                                         # removing nothing is no error
    sc.set_texcoords(None)


def test_tables_replaced_between_two_launches_give_each_its_own(trx, texs):
    """On one busy stream: a long trace, the pass under tables A, then - the host calls wait for the queued pass - tables B and
    the pass again.  The first output is A's, the second B's."""
    torch = _torch()
    tx = texs("cornell_64")
    wd, sc = tx.wd, tx.sc
    (d_hits, d_inst, d_attr), (hits, inst, attr) = wd.frame((0, 1, 0))
    n = hits.shape[0]
    (uv_a, ts_a), (uv_b, ts_b) = tx.table("random"), tx.table("hostile")
    tx.use("random")
    s = torch.cuda.Stream()
    big = random_rays(trx, wd.flat, 1024 * 1024, 72, zero_dirs=False)
    d_big, d_bh = _dev(big), _buf(big.shape[0] * 8)
    d_one, d_two = _buf(3 * n * 4), _buf(3 * n * 4)
    _sync()
    with limit():
        with torch.cuda.stream(s):
            sc.trace_rays_dev(d_big.data_ptr(), big.shape[0], d_bh.data_ptr(), stream=s.cuda_stream)
            sc.surface_albedo_dev(d_hits.data_ptr(), d_attr.data_ptr(), n, d_one.data_ptr(), stream=s.cuda_stream)
        sc.set_textures(ts_b.descs, ts_b.texels, ts_b.material_texture)
        sc.set_texcoords(uv_b)
        tx.current = "hostile"
        with torch.cuda.stream(s):
            sc.surface_albedo_dev(d_hits.data_ptr(), d_attr.data_ptr(), n, d_two.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
    want_a, _ = TT.surface_albedo(hits, attr, tx.mat, tx.idx, tx.n_tris, uv_a, ts_a)
    want_b, _ = TT.surface_albedo(hits, attr, tx.mat, tx.idx, tx.n_tris, uv_b, ts_b)
    _same(d_one.cpu().numpy(), want_a, "the launch before the swap")
    _same(d_two.cpu().numpy(), want_b, "the launch after the swap")
    assert (want_a.view(np.uint32) != want_b.view(np.uint32)).sum() > 500
    sc.check()


def test_a_refit_keeps_both_tables_and_waits_for_the_pass(trx, texs):
    torch = _torch()
    tx = texs("soup_52x44")
    wd, sc = tx.wd, tx.sc
    uvs, ts = tx.use("random")
    (d_hits, d_inst, d_attr), (hits, inst, attr) = wd.frame((0, 1, 0))
    n = hits.shape[0]
    v = wd.flat.tri_verts
    moved = (v + np.random.default_rng(71).normal(scale=1e-3, size=v.shape)).astype(np.float32)
    s = torch.cuda.Stream()
    d_out = _buf(3 * n * 4)
    _sync()
    try:
        with limit():
            with torch.cuda.stream(s):
                sc.surface_albedo_dev(d_hits.data_ptr(), d_attr.data_ptr(), n, d_out.data_ptr(), stream=s.cuda_stream)
            sc.refit(moved)
            s.synchronize()
        want, _ = TT.surface_albedo(hits, attr, tx.mat, tx.idx, tx.n_tris, uvs, ts)
        _same(d_out.cpu().numpy(), want, "the pass before the refit")
        assert sc.get_texcoords().tobytes() == uvs.tobytes() and sc.get_textures()[1].tobytes() == ts.texels.tobytes()
        # the pass over the same caller records still answers from the kept tables (UVs are object space: nothing moved them)
        _same(tx.albedo(d_hits, d_attr, n)[GUARD:-GUARD], want, "the pass after the refit")
    finally:
        with limit():
            sc.refit(v)
            torch.cuda.synchronize()
    sc.check()


# ---- trx_render_image_colour_textured -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cornell(trx):
    """The Cornell stand-in with its stand-in materials, normals welded all round and the stand-in texture tables, in `prim` order."""
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    sc = trx.Scene(flat)
    mats, idx = trx.standin_materials("cornell", verts, counts)
    sc.set_materials(mats, idx[flat.tri_source])
    sc.set_vertex_normals(trx.compute_vertex_normals(verts, -1.0)[flat.tri_source])
    uvs = trx.standin_texcoords("cornell", verts)[flat.tri_source]
    eye, look, fov = trx.scene_camera("cornell")
    yield sc, uvs, trx.standin_textures("cornell", mats.shape[0]), trx.view_from_camera(eye, look, fov, 48, 32)
    sc.close()


def _chain(trx, sc, view, w, h, products, smooth, sem, ao, radius, bn, stride, levels, es):
    """trx_render_image_colour_textured's chain from the device-resident calls: the RGBA8 image [h, w, 4]."""
    torch = _torch()
    from tray_racing_amd import _lib as L
    n, ls, phase, up = w * h, 4, stride * stride - 1, 1
    d_prim, d_inst, d_attr, d_lit = _buf(n * 8, 0xEE), _buf(n * 4, 0xFF), _buf(n * 24, 0), _buf(max(len(products), 1) * n, 0)
    d_cnt, d_term, d_val, d_rgba = _buf(n), _buf(n * 4), _buf(n * 4), _buf(n * 4)
    d_a, d_b, d_work, d_alb = _buf(3 * n * 4), _buf(3 * n * 4), _buf(n * 4), _buf(3 * n * 4)
    P, I, A = d_prim.data_ptr(), d_inst.data_ptr(), d_attr.data_ptr()
    with limit():
        L.check(sc._lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, L.Shard(0, 1, 0, 0), sem, C.c_void_p(P), C.c_void_p(I), None))
        sc.hit_attributes_primary_dev(view, w, h, P, A, d_inst=I)
        if smooth:
            sc.shading_normals_primary(view, w, h, P, A, A, d_inst=I)
        sc.surface_albedo_dev(P, A, n, d_alb.data_ptr())
        sc.trace_light_visibility_dev(view, w, h, products, P, d_lit.data_ptr(), n_samples=ls, sem=sem, frame0=2, shadow_eps=EPS, d_primary_inst=I)
        if ao:
            sc.trace_ao_visibility_dev(view, w, h, P, d_cnt.data_ptr(), ao, radius, sem=sem, frame0=2, ao_eps=EPS, d_primary_inst=I)
            sc.ao_filter_dev(w, h, P, d_cnt.data_ptr(), d_term.data_ptr(), ao, 1, d_attr=A)
        sc.light_term_dev(view, w, h, products, P, A, d_lit.data_ptr(), d_val.data_ptr(), n_samples=ls, ambient=0.3, d_term=d_term.data_ptr() if ao else 0)
        planes = 0
        if bn:
            planes, other = d_a.data_ptr(), d_b.data_ptr()
            sc.trace_indirect_rgb_textured_dev(view, w, h, products, P, planes, n_samples=bn, stride=stride, phase=phase if stride > 1 else 0,
                                               use_emitters=es > 0, emitter_eps=EEPS, sem=sem, frame0=2, bounce_eps=EPS, shadow_eps=EPS, d_primary_inst=I)
            if stride > 1:
                n_lo = ((w + stride - 1) // stride) * ((h + stride - 1) // stride)
                for c in range(3):
                    sc.value_upsample_dev(w, h, stride, phase, P, planes + c * n_lo * 4, other + c * n * 4, up, d_attr=A)
                planes, other = other, planes
            if levels:
                for c in range(3):
                    sc.value_filter_dev(w, h, P, planes + c * n * 4, other + c * n * 4, levels, d_attr=A, d_work=d_work.data_ptr())
                planes, other = other, planes
        colour_at = planes or d_a.data_ptr()
        if es:
            sc.trace_emitter_light_dev(view, w, h, P, colour_at, n_samples=es, sem=sem, frame0=2, shadow_eps=EPS, emitter_eps=EEPS, d_primary_inst=I,
                                       d_base_rgb=planes)
            planes = colour_at
        sc.albedo_compose_dev(P, d_alb.data_ptr(), d_val.data_ptr(), n, colour_at, d_indirect_rgb=planes)
        sc.shade_rgb_dev(colour_at, n, d_rgba.data_ptr())
        torch.cuda.synchronize()
    return d_rgba.cpu().numpy().reshape(h, w, 4)


def test_textured_host_form_is_its_chain_and_untextured_it_is_the_existing_forms(trx, cornell):
    sc, uvs, (descs, texels, mat_tex), view = cornell
    w, h, sem, ao, radius = 48, 32, 3, 4, 1.4
    products = [l.product(trx) for l in _mixed(3)]
    lit_kw = dict(sem=sem, frame0=2, light_samples=4, shadow_eps=EPS, ambient=0.3, ao_samples=ao, ao_eps=EPS, ao_radius=radius, filter_radius=1)
    kws = [dict(lit_kw, bounce_samples=0), dict(lit_kw, bounce_samples=2, bounce_eps=EPS),
           dict(lit_kw, bounce_samples=2, bounce_eps=EPS, bounce_stride=2, bounce_phase=3, bounce_upsample_radius=1, bounce_filter_levels=2)]
    # untextured: byte for byte the three existing host forms
    sc.set_texcoords(None)
    sc.set_textures(None, None, None)
    plain = []
    for kw in kws:
        with limit():
            want, _ = sc.render_image_colour(view, w, h, products, **kw)
            assert (sc.render_image_colour_textured(view, w, h, products, **kw)[0] == want).all(), kw
            assert (sc.render_image_colour_textured(view, w, h, products, smooth=True, **kw)[0] == sc.render_image_colour_smooth(view, w, h, products, **kw)[0]).all(), kw
            assert (sc.render_image_colour_textured(view, w, h, products, emitter_samples=2, emitter_eps=EEPS, **kw)[0] ==
                    sc.render_image_colour_emitters(view, w, h, products, emitter_samples=2, emitter_eps=EEPS, **kw)[0]).all(), kw
        plain.append(want)
    # textured: the chain of _dev calls, byte for byte; the checker shows
    sc.set_texcoords(uvs)
    sc.set_textures(descs, texels, mat_tex)
    for kw, base in zip(kws, plain):
        for smooth, es in ((False, 0), (True, 0), (False, 2)):
            with limit():
                img, ms = sc.render_image_colour_textured(view, w, h, products, smooth=smooth, emitter_samples=es, emitter_eps=EEPS, **kw)
            want = _chain(trx, sc, view, w, h, products, smooth, sem, ao, radius, kw["bounce_samples"], kw.get("bounce_stride", 1),
                          kw.get("bounce_filter_levels", 0), es)
            assert ms > 0 and (img == want).all(), (kw, smooth, es, int((img != want).sum()))
            assert (img[..., 3] == 255).all()
        with limit():
            assert (sc.render_image_colour_textured(view, w, h, products, **kw)[0] != base).sum() > 100
    sc.check()


# ---- power-of-two scene scaling ------------------------------------------------------------------------------------------------------------

def _scaled_albedo(trx, s, uv_source, ts, prim=None):
    """The albedo planes of tree `s` (tests/scale_cases.py) under the texcoords `uv_source` (in the input mesh's numbering) over
    the caller records `prim`, or over the device's own primary frame: (planes bytes, the records)."""
    sc = trx.Scene(s.flat)
    try:
        sc.set_materials(s.mats, s.idx)
        sc.set_texcoords(uv_source[s.flat.tri_source])
        sc.set_textures(ts.descs, ts.texels, ts.material_texture)
        n = s.w * s.h
        d_h, d_a, d_o = (_buf(n * 8) if prim is None else _dev(prim)), _buf(n * 24), _buf(3 * n * 4)
        with limit():
            if prim is None:
                sc.trace_primary_dev(s.view, s.w, s.h, d_h.data_ptr())
            sc.hit_attributes_primary_dev(s.view, s.w, s.h, d_h.data_ptr(), d_a.data_ptr())
            sc.surface_albedo_dev(d_h.data_ptr(), d_a.data_ptr(), n, d_o.data_ptr())
            _torch().cuda.synchronize()
            sc.check()
        return d_o.cpu().numpy(), d_h.cpu().numpy().view(HIT).copy()
    finally:
        sc.close()


@pytest.fixture(scope="module")
def unit_scale(trx):
    """The recentred Cornell stand-in at k = 0: box-mapped texcoords (object space: the caller's, the same at every k), a random
    texture set on its four materials, the device's own primary records and their albedo planes."""
    base = SC.recentred(trx, *SC.CASES[0])
    s0 = SC.scaled(trx, base, 0)
    uv_source = TT.standin_texcoords(base.verts)
    ts = TT.random_textures(base.mats.shape[0], 12)
    ts = ts._replace(material_texture=np.array([7, 13, 2, TT.NO_TEXTURE], dtype=np.uint32))
    planes, prim = _scaled_albedo(trx, s0, uv_source, ts)
    want, cause = TT.surface_albedo(prim, _attr_of(trx, s0, prim), s0.mats, s0.idx, s0.flat.tri_source.size, uv_source[s0.flat.tri_source], ts)
    _same(planes, want, "k 0: the device against the twin")
    assert (cause == TT.TEXTURED).sum() > 500
    return base, s0, uv_source, ts, planes, prim


def _attr_of(trx, s, prim):
    """The device's attribute records of caller records `prim` on tree `s`."""
    sc = trx.Scene(s.flat)
    try:
        n = s.w * s.h
        d_h, d_a = _dev(prim), _buf(n * 24)
        with limit():
            sc.hit_attributes_primary_dev(s.view, s.w, s.h, d_h.data_ptr(), d_a.data_ptr())
            _torch().cuda.synchronize()
        return d_a.cpu().numpy().view(ATTR_DTYPE).copy()
    finally:
        sc.close()


@pytest.mark.parametrize("k", SC.SAFE)
def test_scaled_scenes_give_the_unit_scale_albedo(trx, unit_scale, k):
    """The scene and the caller's t times 2^k about the eye (the origin), the texcoords as they were: UVs and barycentrics do not
    scale, so the albedo planes hold the k = 0 bits."""
    base, s0, uv_source, ts, planes, prim = unit_scale
    s = SC.scaled(trx, base, k)
    carried, _ = SC.carry(prim, None, s0, s)
    got, _ = _scaled_albedo(trx, s, uv_source, ts, prim=carried)
    _same(got, planes, "2^%d against the device's own k = 0 planes" % k)
