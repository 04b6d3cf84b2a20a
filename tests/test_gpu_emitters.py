"""Emitters on the GPU, bit for bit (include/trx.h, "emitters"): the table and c of trx_scene_get_emitters, the device's
selection at every c_i, trx_emitter_rays_dev (all 32 bytes, both layouts, a proper shard, and at pixels and seeds where u0,
u1, u2 are exactly 0 and exactly 1.0f), the three planes of trx_trace_emitter_light_dev (1, 3 and 64 samples, scratch caps
that force several tile and sample chunks, no base, a separate one, the output itself, a ray mask that hides an occluder),
the emitter mode of the indirect pass, dense and sparse, with 0 and 2 lights, and trx_render_image_colour_emitters against
its composition - all against the twin (tests/emitter_twin.py), fed the device's own primary records.  Whole buffers are
compared, guard bytes past the last plane included; no record is left out.  Then the behaviours: unusable records, refusals,
staleness after a refit and after new materials, the accounting; and the estimator check, which is independent of the twin.

The cases are tests/test_gpu_materials.py's: cornell_64 and cornell_64_pipe (the stand-in table: the light quad, 2 emitters),
cornell_tlas_48 (the same table over five instances), instanced (72 x 48, transformed, the 360-triangle object emissive
under every instance of it), soup_52x44 (every fifth triangle emissive: 300 emitters, a deep search), kitchen_56x40.

Every step that runs on the GPU sits under a time limit of its own (`limit`): a step that hangs ends the process."""
import ctypes as C
import types

import numpy as np
import pytest

import emitter_twin as ET
import light_twin as LT
import material_twin as MT
from ao_visibility_twin import record_map
from caller_records import entries
from hit_attr_twin import tri_records
from inst_mask_twin import oracle_twin
from test_gpu_ao_visibility import make_case
from test_gpu_light import EPS, FILL, INERT, _buf, _dev, _mixed, _sync, _torch, limit
from test_gpu_materials import KitchenCase

pytestmark = pytest.mark.gpu
GUARD = 64
EEPS = 0.001
UNIT = 64 * (32 + 1) + 64 * (4 + 4 + 12)                                  # kernels.h, kEmitterUnitBytes
GI_UNIT = 64 * (32 + 1) + 64 * (32 + 8 + 4 + 24 + 4 + 4) + 64 * 8         # kBounceUnitBytes and the emitter mode's 8 bytes per ray
f32 = np.float32
HIT = np.dtype([("t", "<f4"), ("prim", "<u4")])

# The estimator check's bound (test_the_pass_estimates_what_the_parents_bounce_estimates): measured on an MI355X with
#   python tools/gpu_emitters.py      (profiles/emitter_pass.log, its first four lines)
# the existing trx_trace_indirect_rgb_dev, cornell_64, 64 samples, one light of intensity 0, mean of each plane over the 3 478
# surface pixels: 0.0255714 at frame0 = 0 against 0.0241698 at frame0 = 100000 (the stand-in quad emits white: the three
# planes are equal) - the relative difference per plane (R, G, B) below; the bound is three times the larger channel's value,
# 0.1644.  The emitter pass's mean in the same run: 0.0255124, a relative difference of 0.0023 to the existing pass's.
PARENT_RUN_TO_RUN = (0.0548137737174983, 0.0548137737174983, 0.0548137737174983)
ESTIMATOR_BOUND = 3.0 * max(PARENT_RUN_TO_RUN)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.size == want.size, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d bytes differ, first at %s: %s != %s" % (what, bad.size, got.size, bad[:4], got[bad[:4]], want[bad[:4]])


def _cornell_table(trx, tri_verts):
    """The stand-in Cornell table in the order of a golden fixture's triangles (the fixtures hold gen_scene("cornell")'s mesh)."""
    verts, counts = trx.gen_scene("cornell", 0, 1)
    mats, idx = MT.standin("cornell", verts, counts)
    where = {v.tobytes(): i for i, v in enumerate(np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9))}
    return mats, np.array([idx[where[v.tobytes()]] for v in np.ascontiguousarray(tri_verts, dtype=np.float32).reshape(-1, 9)], dtype=np.uint16)


def _table_for(trx, name, osc, inst_prims):
    n_tris = osc.verts.shape[0]
    if name.startswith("cornell"):
        return _cornell_table(trx, osc.verts)
    rng = np.random.default_rng(len(name))
    mats = np.zeros((5, 6), dtype=np.float32)
    mats[:, :3] = rng.uniform(0.1, 1.0, (5, 3)).astype(np.float32)
    mats[3, 3:], mats[4, 3:] = (3.0, 2.0, 1.0), (0.0, 0.5, 6.0)
    idx = rng.integers(0, 3, n_tris).astype(np.uint16)
    if name == "soup_52x44":
        idx[::5] = 3
        idx[::35] = 4
    elif name == "instanced":
        walls = [p for p in inst_prims if p.size == 360]                 # the Cornell-class enclosure: 360 triangles, several instances
        assert walls
        idx[walls[0]] = 3
    else:                                                               # kitchen_56x40: a sprinkle over every object
        idx[::13] = 4
    return mats, idx


class Em:
    """A Case of tests/test_gpu_ao_visibility.py with materials, the twin's emitter table, and the device's built from it."""

    def __init__(self, trx, case):
        self.trx, self.case, self.w, self.h = trx, case, case.w, case.h
        osc = case.osc
        self.recs = tri_records(osc.verts)
        self.n_tris = self.recs.shape[0]
        self.w2o = osc.w2o if case.transformed else None
        self.tlas = osc.inst.size > 0
        self.inst_prims = ET.instance_prims(osc.nodes, osc.inst, int(osc.c.tlas_start)) if self.tlas else None
        self.o2w = case.sc.flat.instance_transforms if case.transformed else None
        self.mats, self.idx = _table_for(trx, case.name, osc, self.inst_prims)
        dev_idx = np.zeros(case.sc.flat.tri_verts.shape[0], dtype=np.uint16)     # (a padded twin: its appended records get material 0)
        dev_idx[:self.n_tris] = self.idx
        self.dev_idx = dev_idx
        case.sc.set_materials(self.mats, dev_idx)
        self.pair = ET.pairs(ET.emissive(self.mats, self.idx), self.inst_prims)
        self.rec, self.c = ET.table(self.recs, self.pair, self.mats, self.idx, self.o2w)
        self.n = case.sc.build_emitters()
        self._geo, self.cache = {}, {}

    def geo(self, prim, inst):
        key = (hash(prim.tobytes()), hash(inst.tobytes()))
        if key not in self._geo:
            self._geo[key] = LT.frame_geometry(self.case.view, self.w, self.h, prim, inst, self.recs, self.w2o)
        return self._geo[key]

    def shadow_scene(self, hidden):
        osc = self.case.osc
        if not hidden:
            return osc
        vis = np.ones(osc.inst.size, dtype=bool)
        vis[list(hidden)] = False
        flat = types.SimpleNamespace(nodes=osc.nodes, tri_verts=osc.verts, instance_offsets=osc.inst, tlas_start=int(osc.c.tlas_start))
        return oracle_twin(self.case.orc, flat, vis, w2o=osc.w2o)

    def twin_light(self, prim, inst, frame0, n, sem, base=None, hidden=None):
        return ET.emitter_light(self.case.orc, self.shadow_scene(hidden), self.case.view, self.w, self.h, self.geo(prim, inst), prim, self.n_tris,
                                self.rec, self.c, self.mats, frame0, n, EPS, EEPS, sem, base=base)

    def twin_indirect(self, prim, inst, lights, frame0, n, sem, hidden=None):
        hs = self.shadow_scene(hidden)
        return ET.indirect_rgb_emitters(self.case.orc, self.case.osc, self.case.oview, self.w, self.h, prim, inst, self.recs, self.w2o, lights, frame0, n,
                                        EPS, EPS, EEPS, sem, self.mats, self.idx, self.rec, self.c, shadow_osc=hs if hidden else None, cache=self.cache)

    def expected(self, values, before, shard):
        pix, rec, size = record_map(self.w, self.h, shard)
        want = before.copy()
        planes = want[:3 * size * 4].view(np.uint32).reshape(3, size)
        for c in range(3):
            planes[c, rec] = np.ascontiguousarray(values[c]).view(np.uint32)[pix]
        return want

    def in_layout(self, values, shard, fill):
        """[3, records] float32 of `shard`'s layout from pixel-order planes; `fill` at the records the shard does not own."""
        pix, rec, size = record_map(self.w, self.h, shard)
        out = np.full((3, size), fill, dtype=np.float32)
        out[:, rec] = values[:, pix]
        return out

    def device_light(self, d_prim, d_inst, n, sem, shard, frame0=0, stream=0, mask=0, base=None, alias=False):
        """(the three planes and GUARD bytes past them, the same buffer before the call).  base: None or a [3, records] array
        in the shard's layout - a separate buffer, or with `alias` what the output itself holds before the call."""
        _, _, size = record_map(self.w, self.h, shard)
        before = np.full(3 * size * 4 + GUARD, FILL, dtype=np.uint8)
        d_base = 0
        if base is not None and alias:
            before[:3 * size * 4] = np.ascontiguousarray(base, dtype=np.float32).reshape(-1).view(np.uint8)
        elif base is not None:
            keep = _dev(base)
            d_base = keep.data_ptr()
        d_out = _dev(before)
        if alias:
            d_base = d_out.data_ptr()
        _sync()
        with limit():
            self.case.sc.trace_emitter_light_dev(self.case.view, self.w, self.h, d_prim.data_ptr(), d_out.data_ptr(), n_samples=n, sem=sem, ray_mask=mask,
                                                 frame0=frame0, shadow_eps=EPS, emitter_eps=EEPS, d_primary_inst=d_inst.data_ptr() if d_inst is not None else 0,
                                                 d_base_rgb=d_base, shard=(*shard, 0), stream=stream)
            _torch().cuda.synchronize()
            self.case.sc.check()
        return d_out.cpu().numpy(), before

    def device_indirect(self, d_prim, d_inst, lights, n, sem, shard, frame0=0, mask=0):
        _, _, size = record_map(self.w, self.h, shard)
        before = np.full(3 * size * 4 + GUARD, FILL, dtype=np.uint8)
        d_out = _dev(before)
        _sync()
        with limit():
            self.case.sc.trace_indirect_rgb_emitters_dev(self.case.view, self.w, self.h, [l.product(self.trx) for l in lights], d_prim.data_ptr(),
                                                         d_out.data_ptr(), n_samples=n, sem=sem, ray_mask=mask, frame0=frame0, bounce_eps=EPS,
                                                         shadow_eps=EPS, emitter_eps=EEPS, d_primary_inst=d_inst.data_ptr() if d_inst is not None else 0,
                                                         shard=(*shard, 0))
            _torch().cuda.synchronize()
            self.case.sc.check()
        return d_out.cpu().numpy(), before


@pytest.fixture(scope="module")
def cases(trx, orc):
    made, ems = {}, {}

    def get(name):
        if name == "kitchen_56x40" and name not in made:
            made[name] = KitchenCase(trx, orc)
        case = make_case(trx, orc, made, name)
        if name not in ems:
            ems[name] = Em(trx, case)
            if case.base is not None:                  # (a padded twin shares its base case's twin answers)
                ems[name].cache, ems[name]._geo = get(case.base.name).cache, get(case.base.name)._geo
        return ems[name]
    yield get
    trx.load().trx_debug_ao_scratch_cap(0)
    for c in made.values():
        c.close()


ALL = ["cornell_64", "cornell_tlas_48", "instanced", "soup_52x44", "kitchen_56x40", "cornell_64_pipe"]


# ---- the table and selection ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_table_and_selection_equal_the_twin(trx, cases, name):
    """trx_scene_get_emitters' records and c bit for bit; the accounting; trx_debug_emitter_select at every c_i, its two float
    neighbours, 0, 1.0 and the hash's values around 1.0."""
    em = cases(name)
    sc = em.case.sc
    assert em.n == em.pair.shape[0] == em.rec.shape[0] and em.n >= 2, (name, em.n)
    if name.startswith("cornell"):
        assert em.n == 2
    if name == "soup_52x44":
        assert em.n == 300
    got_rec, got_c = sc.get_emitters()
    _same(got_rec, em.rec, "%s: the records" % name)
    _same(got_c, em.c, "%s: c" % name)
    if em.tlas:
        inst = em.rec.view(np.uint32)[:, 15]
        assert (np.diff(inst.astype(np.int64)) >= 0).all() and inst.max() < em.case.osc.inst.size
    u0 = np.concatenate([em.c, np.nextafter(em.c, f32(-1)), np.nextafter(em.c, f32(2)), [0.0, 1.0, 0.5],
                         (np.array([0, 1, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF], dtype=np.uint32).astype(np.float32) * f32(2.0 ** -32))]).astype(np.float32)
    d_u0, d_j = _dev(u0), _buf(u0.size * 4 + GUARD)
    _sync()
    with limit():
        sc.debug_emitter_select(d_u0.data_ptr(), u0.size, d_j.data_ptr())
    got = d_j.cpu().numpy()
    want = np.full(u0.size * 4 + GUARD, FILL, dtype=np.uint8)
    want[:u0.size * 4] = ET.select(em.c, u0).view(np.uint8)
    _same(got, want, "%s: the selection" % name)
    # the accounting: a second build replaces the tables, the bytes stay; a bare scene of the same buffers holds none
    bytes_with = sc.device_bytes
    assert sc.build_emitters() == em.n and sc.device_bytes == bytes_with
    bare = trx.Scene(sc.flat)
    try:
        before = bare.device_bytes
        bare.set_materials(em.mats, em.dev_idx)
        with_mats = bare.device_bytes
        assert bare.build_emitters() == em.n
        assert bare.device_bytes == with_mats + em.n * 64 + max(em.n - 1, 1) * 4 and with_mats > before
    finally:
        bare.close()


# ---- trx_emitter_rays_dev ---------------------------------------------------------------------------------------------------------------

def _rays(em, d_prim, d_inst, shard, frame0, sample, stream=0):
    _, _, size = record_map(em.w, em.h, shard)
    d_rays = _buf(size * 32 + GUARD)
    _sync()
    with limit():
        em.case.sc.emitter_rays_dev(em.case.view, em.w, em.h, d_prim.data_ptr(), d_rays.data_ptr(), frame0=frame0, sample=sample, shadow_eps=EPS,
                                    emitter_eps=EEPS, d_primary_inst=d_inst.data_ptr() if d_inst is not None else 0, shard=(*shard, 0), stream=stream)
        _torch().cuda.synchronize()
    return d_rays.cpu().numpy()


def _expected_rays(em, rays, shard):
    pix, rec, size = record_map(em.w, em.h, shard)
    want = np.full(size * 32 + GUARD, FILL, dtype=np.uint8)
    want[:size * 32].view(np.uint32).reshape(size, 8)[rec] = np.ascontiguousarray(rays).view(np.uint32).reshape(-1, 8)[pix]
    return want


@pytest.mark.parametrize("name,shard", [("cornell_64", (0, 1, 0)), ("soup_52x44", (1, 3, 1)), ("soup_52x44", (1, 3, 0)), ("cornell_tlas_48", (0, 1, 1)),
                                        ("instanced", (1, 3, 0)), ("kitchen_56x40", (0, 1, 0))])
def test_rays_equal_the_twin(cases, name, shard):
    """All 32 bytes of every record; the other shards' records and the bytes past the last record untouched."""
    em = cases(name)
    st = _torch().cuda.Stream()
    with limit():
        d_prim, d_inst, prim, inst = em.case.primary(0, shard)
    cast_any = 0
    for frame0, sample, stream in ((0, 0, 0), (7, 63, st.cuda_stream), (0xFFFFF7F0, 33, 0)):     # (the last: the seed wraps past 2^32)
        rays, cast, wgeo, j = ET.primary_rays(em.case.orc, em.case.view, em.w, em.h, em.geo(prim, inst), em.rec, em.c, frame0, sample, EPS, EEPS)
        _same(_rays(em, d_prim, d_inst, shard, frame0, sample, stream), _expected_rays(em, rays, shard), "%s shard %s frame0 %#x sample %d" % (name, shard, frame0, sample))
        assert (np.ascontiguousarray(rays).view(np.uint32).reshape(-1, 8)[~cast] == INERT).all()
        cast_any += int(cast.sum())
        if em.n > 2:
            assert np.unique(j[cast]).size > 1
    assert cast_any > 50, (name, cast_any)


def test_rays_where_the_noise_is_exactly_zero_and_exactly_one(cases):
    """soup_52x44: for each of u0, u1, u2 a frame0 (tests/noise_domain.py, seed_for) that makes it exactly 0 and exactly 1.0f at a
    surface pixel - asserted on the twin's own noise - and the whole buffer against the twin.  u0 == 1.0f selects the last
    emitter without a clamp; u1 == 0 puts the point on V0; u2 == 1.0f on the edge V0 + su * E2."""
    import noise_domain as ND
    em = cases("soup_52x44")
    with limit():
        d_prim, d_inst, prim, inst = em.case.primary(0)
    geo = em.geo(prim, inst)
    surf = geo[0]
    assert surf.size > 200
    sample = 5
    for which, offset in ((0, 0), (1, 1024), (2, 4096)):
        for k, (target, value) in enumerate(((0, 0.0), (0xFFFFFFFF, 1.0), (0xFFFFFF80, 1.0))):
            at = int(surf[(37 * (3 * which + k) + 11) % surf.size])
            px, py = at % em.w, at // em.w
            frame0 = (ND.seed_for(px, py, target) - offset - ET.SEED_PRIMARY - sample) & 0xFFFFFFFF
            se = (frame0 + ET.SEED_PRIMARY + sample) & 0xFFFFFFFF
            u = [ET.hash_noise([px], [py], se + o)[0] for o in (0, 1024, 4096)]
            assert u[which] == f32(value), (which, target, u)
            rays, cast, wgeo, j = ET.primary_rays(em.case.orc, em.case.view, em.w, em.h, geo, em.rec, em.c, frame0, sample, EPS, EEPS)
            if which == 0:
                s = ET.sample(em.rec, em.c, np.array([px]), np.array([py]), se, EEPS, np.zeros((1, 3), dtype=np.float32), np.zeros((1, 3), dtype=np.float32))
                assert s["j"][0] == (em.n - 1 if value == 1.0 else 0)
            _same(_rays(em, d_prim, d_inst, (0, 1, 0), frame0, sample), _expected_rays(em, rays, (0, 1, 0)), "u%d == %g at pixel (%d, %d)" % (which, value, px, py))


# ---- trx_trace_emitter_light_dev ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell_64", "soup_52x44", "instanced", "kitchen_56x40", "cornell_64_pipe"])
def test_planes_equal_the_twin(trx, cases, name):
    """1, 3 and 64 samples; image layout and shard (1, 3) in both layouts; TRX_SEM_HLSL and TRX_SEM_CPU; a non-null stream; no
    base, a separate base, the output as its own base; a frame0 whose seeds wrap past 2^32."""
    em = cases(name)
    if em.case.base is not None:
        assert em.case.sc.walk_kind(trx.MODE_RAYS) == trx.WALK_PIPELINED
    st = _torch().cuda.Stream()
    rng = np.random.default_rng(5)
    for sem, shard, stream, runs in ((0, (0, 1, 0), 0, ((1, 0, None), (3, 3, "sep"), (64, 0, "alias"))), (3, (1, 3, 1), st.cuda_stream, ((3, 0xFFFFF7FF, "alias"),)),
                                     (0, (1, 3, 0), 0, ((3, 3, "sep"),))):
        with limit():
            d_prim, d_inst, prim, inst = em.case.primary(sem, shard, stream)
        for n, frame0, base in runs:
            what = "%s sem %d shard %s n %d frame0 %#x base %s" % (name, sem, shard, n, frame0, base)
            if base is None:
                got, before = em.device_light(d_prim, d_inst, n, sem, shard, frame0=frame0, stream=stream)
                values = em.twin_light(prim, inst, frame0, n, sem)
            else:
                # (a base with -0 in it: a record without a surface keeps its base's bits, a surface record gets base + A / n)
                b = rng.uniform(0.0, 1.0, (3, em.w * em.h)).astype(np.float32)
                b[:, ::7] = f32(-0.0)
                got, before = em.device_light(d_prim, d_inst, n, sem, shard, frame0=frame0, stream=stream, base=em.in_layout(b, shard, f32(9.0)),
                                              alias=base == "alias")
                values = em.twin_light(prim, inst, frame0, n, sem, base=b)
            _same(got, em.expected(values, before, shard), what)
            if base is None:
                surf = LT.surface(prim, em.n_tris)
                assert (values[:, ~surf] == 0).all() and (values[:, surf] > 0).any() and np.unique(values).size > 5, what     # (one sample: few pixels see an emitter)
                assert (values[0] != values[1]).any() or (values[1] != values[2]).any() or name.startswith("cornell"), what


@pytest.mark.parametrize("name", ["cornell_64", "instanced"])
def test_chunk_loops_give_the_same_planes(trx, cases, name):
    """Scratch caps below the pass's need: tiles in several chunks with one sample each, all tiles with two samples at a time,
    one tile and one sample at a time - bit for bit the twin's planes, which know no chunking; with the output as its own base."""
    lib = trx.load()
    em = cases(name)
    tiles = ((em.w + 7) // 8) * ((em.h + 7) // 8)
    n = 5
    try:
        for sem, shard in ((0, (0, 1, 0)), (3, (0, 1, 1))):
            with limit():
                d_prim, d_inst, prim, inst = em.case.primary(sem, shard)
            plain = em.twin_light(prim, inst, 2, n, sem)
            surf = LT.surface(prim, em.n_tris)
            assert (plain[:, ~surf] == 0).all() and (plain[:, surf] > 0).mean() > 0.05 and np.unique(plain).size > 20, (name, sem)
            b = np.random.default_rng(9).uniform(0.0, 1.0, (3, em.w * em.h)).astype(np.float32)
            aliased = em.twin_light(prim, inst, 2, n, sem, base=b)
            for cap in (UNIT * tiles * 2, UNIT * 10, UNIT * (tiles // 3 + 1), 1):
                lib.trx_debug_ao_scratch_cap(cap)
                got, before = em.device_light(d_prim, d_inst, n, sem, shard, frame0=2)
                _same(got, em.expected(plain, before, shard), "%s sem %d cap %d" % (name, sem, cap))
                got, before = em.device_light(d_prim, d_inst, n, sem, shard, frame0=2, base=em.in_layout(b, shard, f32(9.0)), alias=True)
                _same(got, em.expected(aliased, before, shard), "%s sem %d cap %d, aliased" % (name, sem, cap))
            lib.trx_debug_ao_scratch_cap(0)
    finally:
        lib.trx_debug_ao_scratch_cap(0)


def test_a_ray_mask_hides_an_occluder(cases):
    """cornell_tlas_48: the pass with ray_mask 0x0E against the twin scene without TLAS primitive 4 (the big object under the
    light); more light arrives than in the unmasked pass."""
    em = cases("cornell_tlas_48")
    case = em.case
    try:
        for sem, shard in ((0, (0, 1, 0)), (3, (1, 3, 1))):
            with limit():
                d_prim, d_inst, prim, inst = case.primary(sem, shard)
            masks = np.full(case.osc.inst.size, 0xFF, dtype=np.uint8)
            masks[LT.MASK_HIDES] = 0x11
            case.sc.set_instance_masks(masks)
            got, before = em.device_light(d_prim, d_inst, 3, sem, shard)
            plain = em.twin_light(prim, inst, 0, 3, sem)
            _same(got, em.expected(plain, before, shard), "sem %d ray_mask 0" % sem)
            got, before = em.device_light(d_prim, d_inst, 3, sem, shard, mask=0x0E)
            masked = em.twin_light(prim, inst, 0, 3, sem, hidden=(LT.MASK_HIDES,))
            _same(got, em.expected(masked, before, shard), "sem %d ray_mask 0x0E" % sem)
            if shard[1] == 1:
                assert (masked.view(np.uint32) != plain.view(np.uint32)).sum() > 10 and masked.sum() > plain.sum()
            case.sc.set_instance_masks(None)
    finally:
        case.sc.set_instance_masks(None)


# ---- the emitter mode of the indirect pass ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n_lights", [("cornell_64", 0), ("cornell_64", 2), ("soup_52x44", 2), ("instanced", 0), ("cornell_tlas_48", 2)])
def test_indirect_planes_equal_the_twin(trx, cases, name, n_lights):
    """Rule 5e, dense, 3 samples: image layout under the default cap, then a shard in TRX_LAYOUT_SHARD under caps that force
    several tile chunks and several sample chunks; on cornell_tlas_48 also masked."""
    lib = trx.load()
    em = cases(name)
    lights = _mixed(n_lights)
    tiles = ((em.w + 7) // 8) * ((em.h + 7) // 8)
    try:
        with limit():
            d_prim, d_inst, prim, inst = em.case.primary(0)
        values = em.twin_indirect(prim, inst, lights, 1, 3, 0)
        for cap in (0, GI_UNIT * 10, GI_UNIT * tiles * 2):
            lib.trx_debug_ao_scratch_cap(cap)
            got, before = em.device_indirect(d_prim, d_inst, lights, 3, 0, (0, 1, 0), frame0=1)
            _same(got, em.expected(values, before, (0, 1, 0)), "%s %d lights cap %d" % (name, n_lights, cap))
        lib.trx_debug_ao_scratch_cap(0)
        surf = LT.surface(prim, em.n_tris)
        assert (values[:, ~surf] == 0).all() and (values[:, surf] > 0).mean() > 0.05 and np.unique(values).size > 20
        if n_lights == 0:
            # without a light every value is emitter light through one bounce: the parent's pass refuses 0 lights
            with pytest.raises(trx.TrxError, match="n_lights"):
                em.case.sc.trace_indirect_rgb_dev(em.case.view, em.w, em.h, [], d_prim.data_ptr(), d_prim.data_ptr(), n_samples=3)
        if name == "cornell_tlas_48":
            masks = np.full(em.case.osc.inst.size, 0xFF, dtype=np.uint8)
            masks[LT.MASK_HIDES] = 0x11
            em.case.sc.set_instance_masks(masks)
            with limit():
                d_prim, d_inst, prim, inst = em.case.primary(3, (1, 3, 1))
            got, before = em.device_indirect(d_prim, d_inst, lights, 3, 3, (1, 3, 1), mask=0x0E)
            _same(got, em.expected(em.twin_indirect(prim, inst, lights, 0, 3, 3, hidden=(LT.MASK_HIDES,)), before, (1, 3, 1)), "masked, shard layout")
    finally:
        lib.trx_debug_ao_scratch_cap(0)
        if name == "cornell_tlas_48":
            em.case.sc.set_instance_masks(None)


@pytest.mark.parametrize("n_lights", [0, 2])
def test_sparse_cells_are_the_dense_values_of_their_pixels(trx, cases, n_lights):
    """soup 52 x 44, stride 2 phase 3 (and stride 3 phase 7, whose cells leave the image) under a cap that forces chunks; stride 1 is the
    dense pass."""
    lib = trx.load()
    em = cases("soup_52x44")
    lights = _mixed(n_lights)
    with limit():
        d_prim, d_inst, prim, inst = em.case.primary(0)
    dense = em.twin_indirect(prim, inst, lights, 1, 3, 0)

    def sparse(stride, phase):
        wlo, hlo = (em.w + stride - 1) // stride, (em.h + stride - 1) // stride
        before = np.full(3 * wlo * hlo * 4 + GUARD, FILL, dtype=np.uint8)
        d_out = _dev(before)
        _sync()
        with limit():
            em.case.sc.trace_indirect_rgb_emitters_sparse_dev(em.case.view, em.w, em.h, stride, phase, [l.product(trx) for l in lights], d_prim.data_ptr(),
                                                              d_out.data_ptr(), n_samples=3, frame0=1, bounce_eps=EPS, shadow_eps=EPS, emitter_eps=EEPS,
                                                              d_primary_inst=d_inst.data_ptr())
            _torch().cuda.synchronize()
            em.case.sc.check()
        return d_out.cpu().numpy(), before
    try:
        for stride, phase, cap in ((2, 3, 0), (2, 3, GI_UNIT * 7), (3, 7, 0), (1, 0, 0)):
            lib.trx_debug_ao_scratch_cap(cap)
            got, before = sparse(stride, phase)
            want = before.copy()
            lo = MT.sparse_rgb(dense, em.w, em.h, stride, phase)
            want[:lo.size * 4] = lo.reshape(-1).view(np.uint8)
            _same(got, want, "stride %d phase %d cap %d" % (stride, phase, cap))
    finally:
        lib.trx_debug_ao_scratch_cap(0)
    one, _ = sparse(1, 0)
    full, _ = em.device_indirect(d_prim, d_inst, lights, 3, 0, (0, 1, 0), frame0=1)
    _same(one, full, "stride 1 against the dense pass")


# ---- trx_render_image_colour_emitters ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bn,stride,levels,ao,n_lights", [(0, 1, 0, 0, 0), (3, 1, 2, 0, 2), (2, 2, 0, 4, 0), (2, 3, 2, 0, 1)])
def test_host_form_is_its_composition(trx, cases, bn, stride, levels, ao, n_lights):
    """No bounce and no light, dense + filter with lights, sparse + upsample without lights, sparse + upsample + filter:
    trx_render_image_colour_emitters against the device-resident calls it is made of, on the transformed scene."""
    torch = _torch()
    from tray_racing_amd import _lib as L
    em = cases("instanced")
    case = em.case
    sc, view, w, h = case.sc, case.view, case.w, case.h
    n = w * h
    lights, ls, sem, phase, up, es = _mixed(n_lights), 4, 3, stride * stride - 1, 1, 3
    products = [l.product(trx) for l in lights]
    with limit():
        img, ms = sc.render_image_colour_emitters(view, w, h, products, emitter_samples=es, emitter_eps=EEPS, bounce_samples=bn, bounce_stride=stride,
                                                  bounce_phase=phase, bounce_upsample_radius=up, bounce_filter_levels=levels, bounce_eps=EPS, sem=sem, frame0=2,
                                                  light_samples=ls, shadow_eps=EPS, ambient=0.3, ao_samples=ao, ao_eps=EPS, ao_radius=case.radius, filter_radius=1)
    d_prim, d_inst, d_attr, d_lit = _buf(n * 8, 0xEE), _buf(n * 4, 0xFF), _buf(n * 24, 0), _buf(max(len(lights), 1) * n, 0)
    d_cnt, d_term, d_val, d_rgba = _buf(n), _buf(n * 4), _buf(n * 4), _buf(n * 4)
    d_a, d_b, d_work = _buf(3 * n * 4), _buf(3 * n * 4), _buf(n * 4)
    with limit():
        L.check(sc._lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, L.Shard(0, 1, 0, 0), sem, C.c_void_p(d_prim.data_ptr()),
                                                   C.c_void_p(d_inst.data_ptr()), None))
        sc.hit_attributes_primary_dev(view, w, h, d_prim.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr())
        term_lights = products
        if products:
            sc.trace_light_visibility_dev(view, w, h, products, d_prim.data_ptr(), d_lit.data_ptr(), n_samples=ls, sem=sem, frame0=2, shadow_eps=EPS,
                                          d_primary_inst=d_inst.data_ptr())
        else:   # (no light: V is what the light term gives for one light of intensity 0, whatever its plane holds)
            term_lights = [trx.light(trx.LIGHT_DIRECTIONAL, (0.0, 1.0, 0.0), intensity=0.0)]
        if ao:
            sc.trace_ao_visibility_dev(view, w, h, d_prim.data_ptr(), d_cnt.data_ptr(), ao, case.radius, sem=sem, frame0=2, ao_eps=EPS,
                                       d_primary_inst=d_inst.data_ptr())
            sc.ao_filter_dev(w, h, d_prim.data_ptr(), d_cnt.data_ptr(), d_term.data_ptr(), ao, 1, d_attr=d_attr.data_ptr())
        sc.light_term_dev(view, w, h, term_lights, d_prim.data_ptr(), d_attr.data_ptr(), d_lit.data_ptr(), d_val.data_ptr(), n_samples=ls, ambient=0.3,
                          d_term=d_term.data_ptr() if ao else 0)
        planes = 0
        if bn:
            planes, other = d_a.data_ptr(), d_b.data_ptr()
            if stride > 1:
                sc.trace_indirect_rgb_emitters_sparse_dev(view, w, h, stride, phase, products, d_prim.data_ptr(), planes, n_samples=bn, sem=sem, frame0=2,
                                                          bounce_eps=EPS, shadow_eps=EPS, emitter_eps=EEPS, d_primary_inst=d_inst.data_ptr())
                n_lo = ((w + stride - 1) // stride) * ((h + stride - 1) // stride)
                for c in range(3):
                    sc.value_upsample_dev(w, h, stride, phase, d_prim.data_ptr(), planes + c * n_lo * 4, other + c * n * 4, up, d_attr=d_attr.data_ptr())
                planes, other = other, planes
            else:
                sc.trace_indirect_rgb_emitters_dev(view, w, h, products, d_prim.data_ptr(), planes, n_samples=bn, sem=sem, frame0=2, bounce_eps=EPS,
                                                   shadow_eps=EPS, emitter_eps=EEPS, d_primary_inst=d_inst.data_ptr())
            if levels:
                for c in range(3):
                    sc.value_filter_dev(w, h, d_prim.data_ptr(), planes + c * n * 4, other + c * n * 4, levels, d_attr=d_attr.data_ptr(),
                                        d_work=d_work.data_ptr())
                planes, other = other, planes
        colour = planes or d_a.data_ptr()
        sc.trace_emitter_light_dev(view, w, h, d_prim.data_ptr(), colour, n_samples=es, sem=sem, frame0=2, shadow_eps=EPS, emitter_eps=EEPS,
                                   d_primary_inst=d_inst.data_ptr(), d_base_rgb=planes)
        sc.material_compose_dev(d_prim.data_ptr(), d_val.data_ptr(), n, colour, d_indirect_rgb=colour)
        sc.shade_rgb_dev(colour, n, d_rgba.data_ptr())
        torch.cuda.synchronize()
    want = d_rgba.cpu().numpy().reshape(h, w, 4)
    assert ms > 0 and (img == want).all(), (bn, stride, levels, (img != want).sum())
    assert (img[..., 3] == 255).all() and (img[..., :3] > 0).mean() > 0.05
    sc.check()


def test_host_form_builds_a_missing_or_stale_table(trx, cases):
    em = cases("cornell_64")
    sc = trx.Scene(em.case.sc.flat)
    try:
        sc.set_materials(em.mats, em.dev_idx)
        with pytest.raises(trx.TrxError, match="no emitter table"):
            sc.get_emitters()
        with limit():
            first, _ = sc.render_image_colour_emitters(em.case.view, em.w, em.h, emitter_samples=2, ambient=0.0)
        assert sc.get_emitters()[0].shape[0] == em.n
        sc.set_materials(em.mats, em.dev_idx)
        with pytest.raises(trx.TrxError, match="stale"):
            sc.get_emitters()
        with limit():
            again, _ = sc.render_image_colour_emitters(em.case.view, em.w, em.h, emitter_samples=2, ambient=0.0)
        assert (first == again).all() and sc.get_emitters()[0].shape[0] == em.n
    finally:
        sc.close()


# ---- behaviours ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["soup_52x44", "instanced"])
def test_unusable_records_are_all_misses(trx, cases, name):
    """A primary buffer in which every record is one of the caller-record table's misses (tests/caller_records.py: a prim at,
    past and far past the triangle table beside a usable t, a usable prim beside FLT_MAX, +inf, NaN): every ray is the inert
    ray, the pass's planes are the base (+0 without one), the emitter-mode indirect planes +0."""
    em = cases(name)
    n = em.w * em.h
    n_inst = em.case.osc.inst.size
    table = entries(em.n_tris, n_inst)
    misses = [e for e in table if (not e[3] or e[1] is False) and not isinstance(e[0], str)]
    assert len(misses) > 30 and any(e[3] for e in misses) and any(e[1] for e in misses)
    rec, ids = np.zeros(n, dtype=HIT), np.zeros(n, dtype=np.uint32)
    for i in range(n):
        t, _, p, _, ii, _ = misses[i % len(misses)]
        rec["t"][i], rec["prim"][i], ids[i] = t, p, ii
    d_prim, d_inst = _dev(rec), _dev(ids)
    want = np.full(n * 32 + GUARD, FILL, dtype=np.uint8)
    want[:n * 32].view(np.uint32).reshape(n, 8)[:] = INERT
    _same(_rays(em, d_prim, d_inst, (0, 1, 0), 3, 1), want, "%s: the rays" % name)
    got, before = em.device_light(d_prim, d_inst, 3, 0, (0, 1, 0))
    zero = before.copy()
    zero[:3 * n * 4] = 0
    _same(got, zero, "%s: the pass without a base" % name)
    base = np.random.default_rng(2).uniform(-1.0, 1.0, (3, n)).astype(np.float32)
    got, before = em.device_light(d_prim, d_inst, 3, 0, (0, 1, 0), base=base, alias=True)
    _same(got, before, "%s: the pass over its own output" % name)
    got, before = em.device_indirect(d_prim, d_inst, _mixed(1), 2, 0, (0, 1, 0))
    _same(got, zero, "%s: the emitter-mode indirect pass" % name)


def test_every_refusal_leaves_the_output_as_it_was(trx, cases):
    from tray_racing_amd import _lib
    em = cases("instanced")
    sc, lib = em.case.sc, trx.load()
    with limit():
        d_prim, d_inst, prim, inst = em.case.primary(0)
    n = em.w * em.h
    d_out, d_rays = _buf(3 * n * 4 + GUARD), _buf(n * 32 + GUARD)
    view, whole = em.case.view, _lib.Shard(0, 1, 0, 0)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    good = trx.light_array([l.product(trx) for l in _mixed(1)])
    NAN = float("nan")

    def light(n_samples=3, sem=0, mask=0, eps=EPS, eeps=EEPS, inst_=d_inst, w=em.w):
        return lib.trx_trace_emitter_light_dev(sc.handle, C.byref(view), w, em.h, whole, sem, mask, 0, n_samples, eps, eeps, P(d_prim),
                                               P(inst_) if inst_ is not None else None, None, P(d_out), None)

    def rays(sample=0, eps=EPS, eeps=EEPS, inst_=d_inst):
        return lib.trx_emitter_rays_dev(sc.handle, C.byref(view), em.w, em.h, whole, 0, sample, eps, eeps, P(d_prim), P(inst_) if inst_ is not None else None,
                                        P(d_rays), None)

    def indirect(n_lights=1, n_samples=3, eeps=EEPS, beps=EPS, mask=0, inst_=d_inst):
        return lib.trx_trace_indirect_rgb_emitters_dev(sc.handle, C.byref(view), em.w, em.h, whole, 0, mask, good, n_lights, 0, n_samples, beps, EPS, eeps,
                                                       P(d_prim), P(inst_) if inst_ is not None else None, P(d_out), None)
    for call, kws in ((light, ({"n_samples": 0}, {"n_samples": 65}, {"sem": 8}, {"mask": 256}, {"eps": -1.0}, {"eps": NAN}, {"eeps": 1.0}, {"eeps": -0.01},
                               {"eeps": NAN}, {"inst_": None}, {"w": 0})),
                      (rays, ({"sample": 64}, {"eps": NAN}, {"eeps": 1.5}, {"eeps": NAN}, {"inst_": None})),
                      (indirect, ({"n_lights": 9}, {"n_samples": 0}, {"n_samples": 65}, {"eeps": 1.0}, {"eeps": NAN}, {"beps": -1.0}, {"mask": 256}, {"inst_": None}))):
        for kw in kws:
            assert call(**kw) == _lib.TRX_ERR_INVALID, (call.__name__, kw, lib.trx_last_error())
    # a scene with materials and no table; a scene with no emissive material at all
    bare = trx.Scene(sc.flat)
    try:
        with pytest.raises(trx.TrxError, match="no materials"):
            bare.build_emitters()
        dull = em.mats.copy()
        dull[:, 3:] = 0
        bare.set_materials(dull, em.dev_idx)
        with pytest.raises(trx.TrxError, match="no emitters"):
            bare.build_emitters()
        for call in (lambda: bare.trace_emitter_light_dev(view, em.w, em.h, d_prim.data_ptr(), d_out.data_ptr(), d_primary_inst=d_inst.data_ptr()),
                     lambda: bare.emitter_rays_dev(view, em.w, em.h, d_prim.data_ptr(), d_rays.data_ptr(), d_primary_inst=d_inst.data_ptr()),
                     lambda: bare.trace_indirect_rgb_emitters_dev(view, em.w, em.h, [], d_prim.data_ptr(), d_out.data_ptr(), d_primary_inst=d_inst.data_ptr()),
                     lambda: bare.trace_indirect_rgb_emitters_sparse_dev(view, em.w, em.h, 2, 0, [], d_prim.data_ptr(), d_out.data_ptr(), d_primary_inst=d_inst.data_ptr()),
                     lambda: bare.debug_emitter_select(d_out.data_ptr(), 4, d_rays.data_ptr()), bare.get_emitters):
            with pytest.raises(trx.TrxError, match="no emitter table") as e:
                call()
            assert e.value.code == -1
    finally:
        bare.close()
    # too little room
    cap = C.c_uint32(em.n - 1)
    room_r, room_c = np.zeros((em.n, 16), dtype=np.float32), np.zeros(em.n, dtype=np.float32)
    assert lib.trx_scene_get_emitters(sc.handle, room_r.ctypes.data_as(C.c_void_p), C.byref(cap), room_c.ctypes.data_as(C.c_void_p)) == _lib.TRX_ERR_INVALID
    assert not room_r.any() and not room_c.any()
    _sync()
    assert (d_out.cpu().numpy() == FILL).all() and (d_rays.cpu().numpy() == FILL).all()


def test_the_table_goes_stale_and_the_rebuilt_one_matches_the_twin_on_the_moved_geometry(trx, orc, cases):
    """soup_52x44 on a scene of its own: after trx_scene_refit and after trx_scene_set_materials every emitter entry point
    refuses and leaves its output alone; the rebuilt table is the twin's over the moved triangles, and the pass over it the
    twin's on the refitted scene (the oracle walks the host twin's refitted nodes)."""
    em = cases("soup_52x44")
    flat, view, w, h = em.case.sc.flat, em.case.view, em.w, em.h
    n = w * h
    sc = trx.Scene(flat)
    try:
        sc.set_materials(em.mats, em.dev_idx)
        assert sc.build_emitters() == em.n
        moved = (flat.tri_verts.reshape(-1, 3, 3) * f32(1.125) + np.array([0.0625, -0.03125, 0.015625], dtype=np.float32)).astype(np.float32).reshape(-1, 9)
        d_prim, d_out, d_rays = _buf(n * 8, 0xEE), _buf(3 * n * 4 + GUARD), _buf(n * 32 + GUARD)

        def refused():
            for call in (lambda: sc.trace_emitter_light_dev(view, w, h, d_prim.data_ptr(), d_out.data_ptr()),
                         lambda: sc.emitter_rays_dev(view, w, h, d_prim.data_ptr(), d_rays.data_ptr()),
                         lambda: sc.trace_indirect_rgb_emitters_dev(view, w, h, [], d_prim.data_ptr(), d_out.data_ptr()),
                         lambda: sc.trace_indirect_rgb_emitters_sparse_dev(view, w, h, 2, 1, [], d_prim.data_ptr(), d_out.data_ptr()),
                         lambda: sc.debug_emitter_select(d_out.data_ptr(), 4, d_rays.data_ptr()), sc.get_emitters):
                with pytest.raises(trx.TrxError, match="stale") as e:
                    call()
                assert e.value.code == -1
            _sync()
            assert (d_out.cpu().numpy() == FILL).all() and (d_rays.cpu().numpy() == FILL).all()
        with limit():
            sc.refit(moved)
        refused()
        assert sc.build_emitters() == em.n
        rec, c = ET.table(tri_records(moved), em.pair, em.mats, em.idx)
        got_rec, got_c = sc.get_emitters()
        _same(got_rec, rec, "the records over the moved triangles")
        _same(got_c, c, "c over the moved triangles")
        assert (rec[:, :3] != em.rec[:, :3]).any()
        # the pass on the refitted scene
        nodes = trx.refit_nodes(flat, moved)
        osc = orc.Scene(nodes, moved, flat.instance_offsets, flat.tlas_start)
        with limit():
            sc.trace_primary_dev(view, w, h, d_prim.data_ptr())
            _torch().cuda.synchronize()
        prim = d_prim.cpu().numpy().view(orc.HIT_DTYPE)
        inst = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        recs = tri_records(moved)
        geo = LT.frame_geometry(view, w, h, prim, inst, recs, None)
        want_planes = ET.emitter_light(orc, osc, view, w, h, geo, prim, em.n_tris, rec, c, em.mats, 4, 3, EPS, EEPS, 0)
        with limit():
            sc.trace_emitter_light_dev(view, w, h, d_prim.data_ptr(), d_out.data_ptr(), n_samples=3, frame0=4, shadow_eps=EPS, emitter_eps=EEPS)
            _torch().cuda.synchronize()
            sc.check()
        want = np.full(3 * n * 4 + GUARD, FILL, dtype=np.uint8)
        want[:3 * n * 4] = want_planes.reshape(-1).view(np.uint8)
        _same(d_out.cpu().numpy(), want, "the pass on the refitted scene")
        assert (want_planes > 0).mean() > 0.05
        d_out.fill_(FILL)
        # new materials: stale again; other emissive triangles give another table
        idx2 = em.dev_idx.copy()
        idx2[1::5] = 4
        sc.set_materials(em.mats, idx2)
        refused()
        n2 = sc.build_emitters()
        pair2 = ET.pairs(ET.emissive(em.mats, idx2))
        rec2, c2 = ET.table(recs, pair2, em.mats, idx2)
        assert n2 == pair2.shape[0] > em.n
        got_rec, got_c = sc.get_emitters()
        _same(got_rec, rec2, "the records under the new materials")
        _same(got_c, c2, "c under the new materials")
    finally:
        sc.close()


# ---- the estimator check: independent of the twin ------------------------------------------------------------------------------------------------------

def _plane_means(buf, n, surf):
    planes = buf[:3 * n * 4].view(np.float32).reshape(3, n).astype(np.float64)
    return planes[:, surf].mean(1)


def test_the_pass_estimates_what_the_parents_bounce_estimates(trx, cases):
    """cornell_64, the stand-in table: the mean over all surface pixels of each plane of trx_trace_emitter_light_dev at 64 samples
    against the mean of each plane of trx_trace_indirect_rgb_dev (the existing pass, untouched) at 64 samples under one light
    of intensity 0 - there s_f = 0 and the plane is rule 5c's emission term alone.  Bit equality to the twin cannot see a
    wrong constant in kinv or in the area; this can: a factor of pi or of 2 is a relative difference of 2.14 or 1 (0.68 or 0.5
    the other way round), far beyond any such bound.  The bound is three times the existing pass's own relative difference
    between frame0 = 0 and frame0 = 100000 (the larger channel), measured on the GPU and written down above."""
    em = cases("cornell_64")
    sc, view, w, h = em.case.sc, em.case.view, em.w, em.h
    n = w * h
    with limit():
        d_prim, d_inst, prim, inst = em.case.primary(0)
    surf = LT.surface(prim, em.n_tris)
    dark = [trx.light(trx.LIGHT_POINT, (0.0, 1.0, 0.0), intensity=0.0)]
    means = {}
    for frame0 in (0, 100000):
        d_out = _buf(3 * n * 4)
        with limit():
            sc.trace_indirect_rgb_dev(view, w, h, dark, d_prim.data_ptr(), d_out.data_ptr(), n_samples=64, frame0=frame0, bounce_eps=EPS, shadow_eps=EPS)
            _torch().cuda.synchronize()
        means[frame0] = _plane_means(d_out.cpu().numpy(), n, surf)
    got, _ = em.device_light(d_prim, d_inst, 64, 0, (0, 1, 0))
    mine = _plane_means(got, n, surf)
    run_to_run = np.abs(means[0] - means[100000]) / means[0]
    rel = np.abs(mine - means[0]) / means[0]
    print("parent's emission term, 64 samples: means frame0 0 %s, frame0 100000 %s, relative difference %s" % (means[0], means[100000], run_to_run))
    print("emitter pass, 64 samples: means %s, relative difference to the parent's %s; bound %.6f" % (mine, rel, ESTIMATOR_BOUND))
    assert (means[0] > 0).all() and (mine > 0).all()
    assert (rel <= ESTIMATOR_BOUND).all(), (rel, ESTIMATOR_BOUND)
