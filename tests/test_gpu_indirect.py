"""The indirect-light pass on the GPU, bit for bit (include/trx.h, "indirect light"): trx_bounce_light_rays_dev writes the
twin's secondary shadow rays (tests/indirect_twin.py) - fed the device's own bounce rays, hits and attribute records - and
the inert ray; trx_trace_indirect_dev writes the twin's values - fed the device's own primary records - on single-level,
two-level and transformed scenes, in both layouts, for 1, 3 and 8 lights of all kinds, 1, 3, 16 and 64 samples, every
semantics word, masked and unmasked, with and without a base (aliased too), and with a scratch cap small enough that both
chunk loops run; the pass against its building blocks called one by one; the host form against its composition; refusals,
the scratch's accounting and the ordering with a refit.  No record is left out of any comparison.

Every step that runs on the GPU sits under a time limit of its own (`limit`): a step that hangs ends the process."""
import ctypes as C
import os

import numpy as np
import pytest

import indirect_twin as IT
import light_twin as LT
from ao_visibility_twin import record_map
from helpers import ALL_SEMS, random_rays
from hit_attr_twin import ATTR_DTYPE, tri_records
from inst_mask_twin import oracle_twin
from test_gpu_ao_visibility import Case, make_case
from test_gpu_light import EPS, FILL, INERT, _buf, _dev, _mixed, _sync, _torch, limit

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = float("inf")
UNIT = 64 * (32 + 1) + 64 * (32 + 8 + 4 + 24 + 4 + 4)   # scratch bytes the cap counts per tile and sample (kernels.h, kBounceUnitBytes)
ALBEDO = 0.6
f32 = np.float32


def _inert_rays(n):
    """n inert rays (all words 0, tmax = -1) on the device."""
    rays = np.zeros((n, 8), dtype=np.uint32)
    rays[:, 7] = 0xBF800000
    return _dev(rays)


class Gi:
    """A Case of tests/test_gpu_ao_visibility.py with what the indirect twin needs of it."""

    def __init__(self, case):
        self.case, self.w, self.h = case, case.w, case.h
        self.recs = tri_records(case.osc.verts)
        self.w2o = case.osc.w2o if case.transformed else None
        self.cache, self._values = {}, {}

    def twin(self, prim, inst, lights, frame0, n, sem, albedo=ALBEDO, base=None, hidden=None):
        """The twin's values in pixel order; hidden: the TLAS primitives the masked shadow rays do not enter."""
        key = (hash(prim.tobytes()), hash(inst.tobytes()), tuple(l.key() for l in lights), frame0, n, sem, albedo,
               None if base is None else hash(base.tobytes()), hidden)
        if key not in self._values:
            osc, shadow = self.case.osc, None
            if hidden:
                vis = np.ones(osc.inst.size, dtype=bool)
                vis[list(hidden)] = False
                import types
                flat = types.SimpleNamespace(nodes=osc.nodes, tri_verts=osc.verts, instance_offsets=osc.inst, tlas_start=int(osc.c.tlas_start))
                shadow = oracle_twin(self.case.orc, flat, vis, w2o=osc.w2o)
            self._values[key] = IT.indirect(self.case.orc, osc, self.case.oview, self.w, self.h, prim, inst, self.recs, self.w2o, lights, frame0, n,
                                            EPS, EPS, albedo, sem, base=base, shadow_osc=shadow, cache=self.cache)
        return self._values[key]

    def device(self, d_prim, d_inst, lights, n, sem, shard, frame0=0, stream=0, mask=0, albedo=ALBEDO, base=None, alias=False, sc=None, guard=64):
        """(the pass's output buffer - `guard` bytes past the records - as bytes, the same buffer as it was before the call).
        base: float32 per record of the buffer, or None; alias: the base sits in d_value itself."""
        _, _, size = record_map(self.w, self.h, shard)
        before = np.full(size * 4 + guard, FILL, dtype=np.uint8)
        d_base = None
        if base is not None and alias:
            before[:size * 4] = base.view(np.uint8)
        elif base is not None:
            d_base = _dev(base)
        d_out = _dev(before)
        _sync()
        sc = sc or self.case.sc
        with limit():
            sc.trace_indirect_dev(self.case.view, self.w, self.h, [l.product(self.case.trx) for l in lights], d_prim.data_ptr(), d_out.data_ptr(),
                                  n_samples=n, sem=sem, ray_mask=mask, frame0=frame0, bounce_eps=EPS, shadow_eps=EPS, bounce_albedo=albedo,
                                  d_primary_inst=d_inst.data_ptr() if d_inst is not None else 0,
                                  d_base=d_out.data_ptr() if alias and base is not None else d_base.data_ptr() if d_base is not None else 0,
                                  shard=(*shard, 0), stream=stream)
            _torch().cuda.synchronize()
            sc.check()
        return d_out.cpu().numpy(), before

    def expected(self, values, before, shard):
        pix, rec, size = record_map(self.w, self.h, shard)
        want = before.copy()
        want[:size * 4].view(np.uint32)[rec] = values.view(np.uint32)[pix]
        return want

    def base_px(self, base, shard):
        """A record-ordered base as the twin takes it: in pixel order (0 at the pixels of other shards)."""
        pix, rec, _ = record_map(self.w, self.h, shard)
        out = np.zeros(self.w * self.h, dtype=np.float32)
        out[pix] = base[rec]
        return out


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d bytes differ, first at %s: %s != %s" % (what, bad.size, got.size, bad[:4], got[bad[:4]], want[bad[:4]])


def _check(gi, d_prim, d_inst, prim, inst, lights, n, sem, shard, what, frame0=0, stream=0, mask=0, hidden=None, base=None, alias=False, sc=None):
    got, before = gi.device(d_prim, d_inst, lights, n, sem, shard, frame0=frame0, stream=stream, mask=mask, base=base, alias=alias, sc=sc)
    values = gi.twin(prim, inst, lights, frame0, n, sem, base=None if base is None else gi.base_px(base, shard), hidden=hidden)
    _same(got, gi.expected(values, before, shard), what)
    return values


@pytest.fixture(scope="module")
def cases(trx, orc):
    made, gis = {}, {}

    def get(name):
        case = make_case(trx, orc, made, name)
        if name not in gis:
            gis[name] = Gi(case)
            if case.base is not None:           # (a padded twin shares its base case's twin answers)
                gis[name].cache, gis[name]._values = get(case.base.name).cache, get(case.base.name)._values
        return gis[name]
    yield get
    trx.load().trx_debug_ao_scratch_cap(0)
    for c in made.values():
        c.close()


# ---- trx_bounce_light_rays_dev ----------------------------------------------------------------------------------------------

def _device_bounce(case, d_prim, d_inst, shard, frame, sem, stream=0):
    """The building blocks on the device for one seed, record layout of `shard`: (tensors, host copies in pixel order) of the
    bounce rays, their hits, instance ids and attribute records.  Records outside the shard or the image hold the inert ray."""
    w, h = case.w, case.h
    pix, rec, size = record_map(w, h, shard)
    d_rays, d_hits, d_hinst, d_attr = _inert_rays(size), _buf(size * 8, 0xEE), _buf(size * 4, 0xFF), _buf(size * 24, 0)
    _sync()
    with limit():
        case.sc.ao_rays_dev(case.view, w, h, d_prim.data_ptr(), d_rays.data_ptr(), INF, frame=frame, ao_eps=EPS, d_primary_inst=d_inst.data_ptr(),
                            shard=(*shard, 0), stream=stream)
        case.sc.trace_rays_inst_dev(d_rays.data_ptr(), size, d_hits.data_ptr(), d_hinst.data_ptr(), sem=sem, stream=stream)
        case.sc.hit_attributes_rays_dev(d_rays.data_ptr(), size, d_hits.data_ptr(), d_attr.data_ptr(), d_inst=d_hinst.data_ptr(), stream=stream)
        _torch().cuda.synchronize()
    n = w * h
    rays = np.zeros(n, dtype=case.orc.RAY_DTYPE)
    rays["tmax"] = f32(-1.0)
    hits = np.zeros(n, dtype=case.orc.HIT_DTYPE)
    hits["t"], hits["prim"] = np.inf, 0xFFFFFFFF
    attr = np.zeros(n, dtype=ATTR_DTYPE)
    rays[pix] = d_rays.cpu().numpy().view(case.orc.RAY_DTYPE)[rec]
    hits[pix] = d_hits.cpu().numpy().view(case.orc.HIT_DTYPE)[rec]
    attr[pix] = d_attr.cpu().numpy().view(ATTR_DTYPE)[rec]
    return (d_rays, d_hits, d_hinst, d_attr), (rays, hits, attr)


@pytest.mark.parametrize("name,shard,own_stream", [
    ("cornell_64", (0, 1, 0), False), ("cornell_64", (1, 3, 1), True), ("cornell_64", (1, 3, 0), False), ("soup_52x44", (1, 3, 1), False),
    ("soup_52x44", (0, 1, 0), True), ("cornell_tlas_48", (0, 1, 0), True), ("cornell_tlas_48", (1, 3, 1), False), ("instanced", (0, 1, 0), False),
    ("instanced", (1, 3, 1), True)])
def test_secondary_shadow_rays_are_the_twins_rays_and_the_inert_ray(trx, orc, cases, name, shard, own_stream):
    """All 32 bytes of every ray, for the three kinds of light, samples 0 and 7, and a light placed exactly at a secondary
    hit's ray origin; a sentinel record on either side of the buffer and in every record outside the shard or the image."""
    torch = _torch()
    case = cases(name).case
    st = torch.cuda.Stream() if own_stream else None
    stream = st.cuda_stream if st else 0
    with limit():
        d_prim, d_inst, prim, inst = case.primary(0, shard, stream)
    pix, rec, size = record_map(case.w, case.h, shard)
    (d_br, d_bh, _, d_ba), (b_rays, b_hits, b_attr) = _device_bounce(case, d_prim, d_inst, shard, 5, 0, stream)
    has = IT.bounce_surface(b_rays, b_hits)
    assert has.sum() > 10 and (LT.surface(prim) & ~has).sum() > 10, name          # bounces that hit, bounces that miss
    idx, d, _, Q = IT.hit_geometry(b_rays, b_hits, b_attr)
    j = idx.size // 2
    at_origin = LT.Light(LT.POINT, (Q[j] - d[j] * f32(EPS)).tolist())             # dist == 0: NaN, the inert ray
    lights = _mixed(3) + [at_origin]
    for k, light in enumerate(lights):
        for frame0, sample in ((0, 0), (5, 7)) if light.kind == LT.RECT else ((5, 7 * (k & 1)),):
            d_rays = torch.full(((size + 2) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
            _sync()
            with limit():
                case.sc.bounce_light_rays_dev(case.w, case.h, light.product(trx), d_br.data_ptr(), d_bh.data_ptr(), d_ba.data_ptr(),
                                              d_rays.data_ptr() + 32, light_index=k, frame0=frame0, sample=sample, shadow_eps=EPS,
                                              shard=(*shard, 0), stream=stream)
                torch.cuda.synchronize()
            got = d_rays.cpu().numpy().view(np.uint32).reshape(size + 2, 8)
            twin, cast = IT.secondary_rays(orc, case.w, case.h, b_rays, b_hits, b_attr, light, k, frame0, sample, EPS)
            want = np.full((size + 2, 8), 0xA5A5A5A5, dtype=np.uint32)     # the guards, and records outside the shard or the image
            want[1 + rec] = twin.view(np.uint32).reshape(-1, 8)[pix]
            what = "%s shard %s light %d (kind %d) sample %d" % (name, shard, k, light.kind, sample)
            bad = np.flatnonzero((got != want).any(1))
            assert bad.size == 0, "%s: %d of %d records differ, first %s: %s != %s" % (what, bad.size, size, bad[:4], got[bad[:1]], want[bad[:1]])
            assert (got[1 + rec[~cast[pix]]] == INERT).all(), what
            if k < 3:
                assert cast[pix].sum() > 5 and (has & ~cast)[pix].sum() > 5, what      # cast rays, back-facing secondary hits
            else:
                assert has[idx[j]] and not cast[idx[j]], what
    if (shard[1] > 1 and shard[2] == 0) or ((case.w % 8 or case.h % 8) and shard[2] == 1):
        assert (want[1:-1] == 0xA5A5A5A5).all(1).any()                        # (some record really is outside)
    case.sc.check()


# ---- trx_trace_indirect_dev ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell_64", "soup_52x44", "cornell_tlas_48", "instanced"])
def test_values_equal_the_twin(trx, orc, cases, name):
    """1, 3 and 8 lights of mixed kinds; 1, 3 and 16 samples; image and shard layouts, shard (1, 3) among them, with the
    records of the other shards and the bytes past the buffer untouched; a non-null stream; TRX_SEM_HLSL and TRX_SEM_CPU."""
    torch = _torch()
    gi = cases(name)
    case = gi.case
    st = torch.cuda.Stream()
    for sem, shard, stream, runs in ((0, (0, 1, 0), 0, ((1, 1), (3, 3), (8, 16))), (3, (1, 3, 1), st.cuda_stream, ((3, 3), (8, 1))),
                                     (0, (1, 3, 0), 0, ((3, 3),))):
        with limit():
            d_prim, d_inst, prim, inst = case.primary(sem, shard, stream)
        for n_lights, n in runs:
            values = _check(gi, d_prim, d_inst, prim, inst, _mixed(n_lights), n, sem, shard, "%s sem %d shard %s %d lights n %d" % (name, sem, shard, n_lights, n),
                            frame0=3, stream=stream)
            if shard == (0, 1, 0):
                surf = LT.surface(prim)
                assert (values[~surf] == 0).all() and (values[surf] > 0).mean() > 0.05 and np.unique(values).size > 20, (name, n_lights, n)   # (not vacuous: tests/test_indirect.py has the oracle's shares)
        if shard[1] > 1 and shard[2] == 0:
            assert record_map(case.w, case.h, shard)[0].size < case.w * case.h       # (records of other shards: held to FILL above)


def test_64_samples(trx, orc, cases):
    gi = cases("soup_52x44")
    with limit():
        d_prim, d_inst, prim, inst = gi.case.primary(0)
    light = [LT.Light(LT.POINT, LT.POINT_CASES["soup_52x44"], intensity=1.5)]
    values = _check(gi, d_prim, d_inst, prim, inst, light, 64, 0, (0, 1, 0), "soup_52x44 64 samples", frame0=1)
    assert (values[LT.surface(prim)] > 0).mean() > 0.5


def test_every_semantics_word(trx, orc, cases):
    gi = cases("cornell_64")
    for sem in ALL_SEMS:
        with limit():
            d_prim, d_inst, prim, inst = gi.case.primary(sem, (0, 1, 1))
        _check(gi, d_prim, d_inst, prim, inst, _mixed(3), 1, sem, (0, 1, 1), "cornell_64 sem %d" % sem, frame0=2)


@pytest.mark.parametrize("name,patterns", [("cornell_tlas_48", ((LT.MASK_HIDES,), (0, 4))), ("instanced", ((3,), (1, 6, 7, 12)))])
def test_masked_shadow_rays_skip_the_hidden_instances_and_bounce_rays_do_not(trx, orc, cases, name, patterns):
    """ray_mask 0 with a table set reads no table; a masked pass's shadow rays answer what the twin scene with every hidden
    instance pointed at an empty BLAS answers (tests/inst_mask_twin.py), its bounce rays walk the whole scene."""
    gi = cases(name)
    case = gi.case
    lights, n = _mixed(3), 3
    n_inst = case.osc.inst.size
    try:
        for sem, shard in ((0, (0, 1, 0)), (3, (1, 3, 1))):
            with limit():
                d_prim, d_inst, prim, inst = case.primary(sem, shard)
            open_values = gi.twin(prim, inst, lights, 0, n, sem)
            for hidden in patterns:
                masks = np.full(n_inst, 0xFF, dtype=np.uint8)
                masks[list(hidden)] = 0x11
                case.sc.set_instance_masks(masks)
                what = "%s sem %d shard %s hidden %s" % (name, sem, shard, hidden)
                _check(gi, d_prim, d_inst, prim, inst, lights, n, sem, shard, what + " ray_mask 0")
                _check(gi, d_prim, d_inst, prim, inst, lights, n, sem, shard, what + " ray_mask 0x10", mask=0x10)
                masked = _check(gi, d_prim, d_inst, prim, inst, lights, n, sem, shard, what + " ray_mask 0x0E", mask=0x0E, hidden=tuple(hidden))
                if hidden == patterns[0] and shard[1] == 1:
                    assert (masked.view(np.uint32) != open_values.view(np.uint32)).sum() > 10, what + ": the mask changes nothing"
    finally:
        case.sc.set_instance_masks(None)


def test_masked_calls_on_a_single_level_scene_equal_unmasked_ones(trx, orc, cases):
    gi = cases("cornell_64")
    with limit():
        d_prim, d_inst, prim, inst = gi.case.primary(0)
    for mask in (0, 1, 0x80, 0xFF):
        _check(gi, d_prim, d_inst, prim, inst, _mixed(3), 3, 0, (0, 1, 0), "ray_mask %d" % mask, mask=mask)


@pytest.mark.parametrize("name,shard", [("cornell_64", (0, 1, 0)), ("instanced", (1, 3, 1)), ("cornell_tlas_48", (1, 3, 0))])
def test_base_null_separate_and_aliased(trx, orc, cases, name, shard):
    """d_base NULL, a buffer of its own, and d_value itself: the same values; -0.0f and huge bases among them."""
    gi = cases(name)
    with limit():
        d_prim, d_inst, prim, inst = gi.case.primary(0, shard)
    _, _, size = record_map(gi.w, gi.h, shard)
    base = np.random.default_rng(size).uniform(0.0, 1.0, size).astype(np.float32)
    base[::7], base[3::11] = f32(-0.0), f32(1e30)
    lights = _mixed(3)
    plain = _check(gi, d_prim, d_inst, prim, inst, lights, 3, 0, shard, name + " no base")
    apart = _check(gi, d_prim, d_inst, prim, inst, lights, 3, 0, shard, name + " separate base", base=base)
    alias = _check(gi, d_prim, d_inst, prim, inst, lights, 3, 0, shard, name + " aliased base", base=base, alias=True)
    assert (apart.view(np.uint32) == alias.view(np.uint32)).all() and (apart != plain).any()


@pytest.mark.parametrize("name", ["cornell_64", "instanced"])
def test_chunk_loops_give_the_same_values(trx, orc, cases, name):
    """A scratch cap below the pass's need: samples in several chunks (running sums added to), tiles in several chunks, both -
    bit for bit the uncapped pass's values (the order of the float sums does not depend on the chunking), base aliased."""
    lib = trx.load()
    gi = cases(name)
    case = gi.case
    tiles = ((case.w + 7) // 8) * ((case.h + 7) // 8)
    lights, n = _mixed(3), 5
    try:
        for sem, shard in ((0, (0, 1, 0)), (3, (0, 1, 1))):
            with limit():
                d_prim, d_inst, prim, inst = case.primary(sem, shard)
            base = np.random.default_rng(7).uniform(0.0, 1.0, record_map(case.w, case.h, shard)[2]).astype(np.float32)
            whole, _ = gi.device(d_prim, d_inst, lights, n, sem, shard, base=base, alias=True)
            for cap in (UNIT * tiles * 3, UNIT * tiles * 2, UNIT * tiles, UNIT * 10, UNIT * (tiles // 2 + 1) * 2, 1):
                lib.trx_debug_ao_scratch_cap(cap)
                _check(gi, d_prim, d_inst, prim, inst, lights, n, sem, shard, "%s sem %d cap %d" % (name, sem, cap), base=base, alias=True)
                got, _ = gi.device(d_prim, d_inst, lights, n, sem, shard, base=base, alias=True)
                _same(got, whole, "%s sem %d cap %d against the uncapped pass" % (name, sem, cap))
            lib.trx_debug_ao_scratch_cap(0)
    finally:
        lib.trx_debug_ao_scratch_cap(0)


@pytest.fixture(scope="module")
def cornell(trx, orc):
    """The Cornell stand-in on the device and on the oracle, and its camera: views of any size."""
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    sc = trx.Scene(flat)
    eye, look, fov = trx.scene_camera("cornell")
    yield sc, orc.Scene.from_flat(flat), tri_records(flat.tri_verts), eye, look, fov
    sc.close()


@pytest.mark.parametrize("w,h,shard,away", [(1, 1, (0, 1, 0), False), (7, 3, (0, 1, 0), False), (17, 3, (1, 2, 1), False), (37, 21, (2, 3, 0), False),
                                           (16, 9, (0, 1, 0), True)])
def test_small_images_and_an_image_of_misses(trx, orc, cornell, w, h, shard, away):
    """A 1x1 and a 7x3 image, one tile of a 17x3 image's three in shard layout, an odd-sized image in three shards, and the
    camera turned away: every pixel gets its base."""
    torch = _torch()
    from tray_racing_amd import _lib as L
    sc, osc, recs, eye, look, fov = cornell
    eye, look = np.array(eye, dtype=np.float64), np.array(look, dtype=np.float64)
    if away:   # (from far behind the camera, looking further away: every pixel a miss)
        eye, look = eye + 50.0 * (eye - look), eye + 51.0 * (eye - look)
    view = trx.view_from_camera(eye.tolist(), look.tolist(), fov, w, h)
    pix, rec, size = record_map(w, h, shard)
    d_prim, d_inst = _buf(size * 8, 0xEE), _buf(size * 4, 0xFF)
    with limit():
        L.check(sc._lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, L.Shard(*shard, 0), 0, C.c_void_p(d_prim.data_ptr()),
                                                   C.c_void_p(d_inst.data_ptr()), None))
        torch.cuda.synchronize()
    prim = np.zeros(w * h, dtype=orc.HIT_DTYPE)
    prim["t"], prim["prim"] = np.inf, 0xFFFFFFFF
    prim[pix] = d_prim.cpu().numpy().view(orc.HIT_DTYPE)[rec]
    inst = np.full(w * h, 0xFFFFFFFF, dtype=np.uint32)
    lights, n = _mixed(8), 4
    base = np.random.default_rng(w * h).uniform(0.0, 1.0, size).astype(np.float32)
    base_px = np.zeros(w * h, dtype=np.float32)
    base_px[pix] = base[rec]
    for b, b_px in ((None, None), (base, base_px)):
        before = np.full(size * 4 + 64, FILL, dtype=np.uint8)
        d_out, d_base = _dev(before), None if b is None else _dev(b)
        _sync()
        with limit():
            sc.trace_indirect_dev(view, w, h, [l.product(trx) for l in lights], d_prim.data_ptr(), d_out.data_ptr(), n_samples=n, bounce_eps=EPS,
                                  shadow_eps=EPS, bounce_albedo=ALBEDO, d_base=0 if b is None else d_base.data_ptr(), shard=(*shard, 0))
            torch.cuda.synchronize()
        twin = IT.indirect(orc, osc, orc.view_from_bytes(bytes(view)), w, h, prim, inst, recs, None, lights, 0, n, EPS, EPS, ALBEDO, 0, base=b_px)
        want = before.copy()
        want[:size * 4].view(np.uint32)[rec] = twin.view(np.uint32)[pix]
        _same(d_out.cpu().numpy(), want, "%dx%d shard %s base %s" % (w, h, shard, b is not None))
        surf = LT.surface(prim)
        if away:
            assert not surf.any() and (twin.view(np.uint32) == (np.zeros(w * h, dtype=np.float32) if b is None else b_px).view(np.uint32)).all()
        elif w * h > 100:
            assert surf[pix].any() and np.unique(twin[pix]).size > 20
    sc.check()


def test_the_pipelined_walk_gives_the_same_values(trx, orc, cases):
    """cornell_64_pipe: the padded twin of cornell_64, whose rays launches - the closest-hit one over the bounce rays and the
    any-hit one over the shadow rays - take the pipelined walk; bit for bit the twin's values and the unpadded scene's."""
    gi = cases("cornell_64_pipe")
    case = gi.case
    assert case.sc.walk_kind(trx.MODE_RAYS) == trx.WALK_PIPELINED and case.base.sc.walk_kind(trx.MODE_RAYS) == trx.WALK_PLAIN
    lights = _mixed(3)
    for sem, shard in ((0, (0, 1, 0)), (3, (1, 3, 1))):
        with limit():
            d_prim, d_inst, prim, inst = case.primary(sem, shard)
        _check(gi, d_prim, d_inst, prim, inst, lights, 3, sem, shard, "pipelined sem %d" % sem, frame0=2)
        _check(gi, d_prim, d_inst, prim, inst, lights, 3, sem, shard, "plain sem %d" % sem, frame0=2, sc=case.base.sc)


# ---- the pass is its building blocks ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,mask", [("cornell_64", 0), ("cornell_tlas_48", 0x0E), ("instanced", 0)])
def test_the_pass_equals_its_building_blocks(trx, orc, cases, name, mask):
    """2 samples, 2 lights: trx_ao_rays_dev, trx_trace_rays_inst_dev, trx_hit_attributes_rays_dev, trx_bounce_light_rays_dev and
    trx_trace_occluded*_dev called one by one, rules 4 and 5 over the device's records on the host - bit for bit the pass."""
    torch = _torch()
    gi = cases(name)
    case = gi.case
    w, h, n = case.w, case.h, case.w * case.h
    lights = [_mixed(2)[0], _mixed(2)[1]]
    frame0, sem = 4, 3
    with limit():
        d_prim, d_inst, prim, inst = case.primary(sem)
    try:
        if mask:
            masks = np.full(case.osc.inst.size, 0xFF, dtype=np.uint8)
            masks[LT.MASK_HIDES] = 0x11
            case.sc.set_instance_masks(masks)
        sums, n_open, n_occ = [], 0, 0
        for f in range(2):
            (d_br, d_bh, _, d_ba), (b_rays, b_hits, b_attr) = _device_bounce(case, d_prim, d_inst, (0, 1, 0), frame0 + f, sem)
            flags = []
            for k, light in enumerate(lights):
                d_rays, d_flags = _buf(n * 32), _buf(n)
                _sync()
                with limit():
                    case.sc.bounce_light_rays_dev(w, h, light.product(trx), d_br.data_ptr(), d_bh.data_ptr(), d_ba.data_ptr(), d_rays.data_ptr(),
                                                  light_index=k, frame0=frame0, sample=f, shadow_eps=EPS)
                    if mask:
                        case.sc.trace_occluded_masked_dev(d_rays.data_ptr(), n, d_flags.data_ptr(), mask, sem=sem)
                    else:
                        case.sc.trace_occluded_dev(d_rays.data_ptr(), n, d_flags.data_ptr(), sem=sem)
                    torch.cuda.synchronize()
                flags.append(d_flags.cpu().numpy() != 0)
                n_open += int((~flags[-1]).sum())
                n_occ += int(flags[-1].sum())
            sums.append(IT.sample_sum(orc, w, h, b_rays, b_hits, b_attr, lights, frame0, f, EPS, lambda k, r: flags[k]))
        assert n_occ > 20 and n_open > 20
        want = IT.term(sums, prim, ALBEDO)
        got, before = gi.device(d_prim, d_inst, lights, 2, sem, (0, 1, 0), frame0=frame0, mask=mask)
        _same(got, gi.expected(want, before, (0, 1, 0)), "%s: the pass against its building blocks" % name)
        assert (want > 0).sum() > 50
    finally:
        if mask:
            case.sc.set_instance_masks(None)


@pytest.mark.parametrize("ao,mask", [(0, 0), (4, 0x0E)])
def test_host_form_is_its_composition(trx, cases, ao, mask):
    """trx_render_image_gi against the device-resident calls it is made of, on cornell_tlas_48 (with a mask table set) and
    on the transformed scene; and the bounce changes the lit image."""
    torch = _torch()
    from tray_racing_amd import _lib as L
    for name in ("cornell_tlas_48", "instanced"):
        case = cases(name).case
        sc, view, w, h = case.sc, case.view, case.w, case.h
        n_px = w * h
        lights, n, sem, bn = _mixed(3), 4, 3, 3
        products = [l.product(trx) for l in lights]
        masks = np.full(case.osc.inst.size, 0xFF, dtype=np.uint8)
        masks[LT.MASK_HIDES] = 0x11
        sc.set_instance_masks(masks)
        try:
            with limit():
                img, ms = sc.render_image_gi(view, w, h, products, bn, bounce_eps=EPS, bounce_albedo=ALBEDO, sem=sem, ray_mask=mask, frame0=2,
                                             light_samples=n, shadow_eps=EPS, ambient=0.3, ao_samples=ao, ao_eps=EPS, ao_radius=case.radius, filter_radius=1)
                lit, _ = sc.render_image_lit(view, w, h, products, sem=sem, ray_mask=mask, frame0=2, light_samples=n, shadow_eps=EPS, ambient=0.3,
                                             ao_samples=ao, ao_eps=EPS, ao_radius=case.radius, filter_radius=1)
            d_prim, d_inst, d_attr, d_lit = _buf(n_px * 8, 0xEE), _buf(n_px * 4, 0xFF), _buf(n_px * 24, 0), _buf(len(lights) * n_px)
            d_cnt, d_term, d_val, d_rgba = _buf(n_px), _buf(n_px * 4), _buf(n_px * 4), _buf(n_px * 4)
            with limit():
                L.check(sc._lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, L.Shard(0, 1, 0, 0), sem, C.c_void_p(d_prim.data_ptr()),
                                                           C.c_void_p(d_inst.data_ptr()), None))
                sc.hit_attributes_primary_dev(view, w, h, d_prim.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr())
                sc.trace_light_visibility_dev(view, w, h, products, d_prim.data_ptr(), d_lit.data_ptr(), n_samples=n, sem=sem, ray_mask=mask, frame0=2,
                                              shadow_eps=EPS, d_primary_inst=d_inst.data_ptr())
                if ao:
                    sc.trace_ao_visibility_dev(view, w, h, d_prim.data_ptr(), d_cnt.data_ptr(), ao, case.radius, sem=sem, frame0=2, ao_eps=EPS,
                                               d_primary_inst=d_inst.data_ptr())
                    sc.ao_filter_dev(w, h, d_prim.data_ptr(), d_cnt.data_ptr(), d_term.data_ptr(), ao, 1, d_attr=d_attr.data_ptr())
                sc.light_term_dev(view, w, h, products, d_prim.data_ptr(), d_attr.data_ptr(), d_lit.data_ptr(), d_val.data_ptr(), n_samples=n,
                                  ambient=0.3, d_term=d_term.data_ptr() if ao else 0)
                sc.trace_indirect_dev(view, w, h, products, d_prim.data_ptr(), d_val.data_ptr(), n_samples=bn, sem=sem, ray_mask=mask, frame0=2,
                                      bounce_eps=EPS, shadow_eps=EPS, bounce_albedo=ALBEDO, d_primary_inst=d_inst.data_ptr(), d_base=d_val.data_ptr())
                sc.shade_value_dev(d_val.data_ptr(), n_px, d_rgba.data_ptr())
                torch.cuda.synchronize()
            want = d_rgba.cpu().numpy().reshape(h, w, 4)
            assert ms > 0 and (img == want).all(), (name, ao, mask, (img != want).sum())
            assert (img[..., 3] == 255).all() and (img[..., 0] >= lit[..., 0]).all() and (img[..., 0] > lit[..., 0]).mean() > 0.02, name
            sc.check()
        finally:
            sc.set_instance_masks(None)


# ---- refusals, scratch, ordering ---------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(trx, cases):
    torch = _torch()
    gi = cases("instanced")
    case = gi.case
    sc, view, w, h = case.sc, case.view, case.w, case.h
    with limit():
        d_prim, d_inst, _, _ = case.primary(0)
    n = w * h
    good = _mixed(1)[0].product(trx)
    d_val, d_rays, d_in = _buf(n * 4 + 64), _buf(n * 32), _buf(n * 32, 0)

    def pas(lights=(good,), ns=4, mask=0, seps=EPS, beps=EPS, albedo=0.5, sem=0, inst=d_inst.data_ptr(), shard=(0, 1, 0)):
        sc.trace_indirect_dev(view, w, h, lights, d_prim.data_ptr(), d_val.data_ptr(), n_samples=ns, sem=sem, ray_mask=mask, bounce_eps=beps,
                              shadow_eps=seps, bounce_albedo=albedo, d_primary_inst=inst, shard=(*shard, 0))

    bad_kind, bad_pad, bad_nan, bad_dir = (trx.light(7, (0, 1, 0)), trx.light(trx.LIGHT_POINT, (0, 1, 0)), trx.light(trx.LIGHT_POINT, (0, float("nan"), 0)),
                                           trx.light(trx.LIGHT_DIRECTIONAL, (0, 0, 0)))
    bad_pad._pad[2] = 9
    for kw, msg in (({"lights": [good] * 9}, "n_lights"), ({"lights": (good, bad_kind)}, "kind"), ({"lights": (bad_pad,)}, "_pad"),
                    ({"lights": (bad_nan,)}, "finite"), ({"lights": (bad_dir,)}, "zero length"), ({"ns": 0}, "n_samples"), ({"ns": 65}, "n_samples"),
                    ({"mask": 256}, "ray_mask"), ({"seps": -1.0}, "shadow_eps"), ({"seps": float("nan")}, "shadow_eps"), ({"beps": -1.0}, "bounce_eps"),
                    ({"beps": float("nan")}, "bounce_eps"), ({"albedo": float("inf")}, "bounce_albedo"), ({"albedo": float("nan")}, "bounce_albedo"),
                    ({"sem": 8}, "semantics"), ({"inst": 0}, "instance transforms"), ({"shard": (3, 3, 0)}, "shard")):
        with pytest.raises(trx.TrxError, match=msg) as e:
            pas(**kw)
        assert e.value.code == -1, kw
    with pytest.raises(trx.TrxError, match="shadow_eps"):
        sc.bounce_light_rays_dev(w, h, good, d_in.data_ptr(), d_in.data_ptr(), d_in.data_ptr(), d_rays.data_ptr(), shadow_eps=-0.5)
    with pytest.raises(trx.TrxError, match="kind"):
        sc.bounce_light_rays_dev(w, h, bad_kind, d_in.data_ptr(), d_in.data_ptr(), d_in.data_ptr(), d_rays.data_ptr())
    with pytest.raises(trx.TrxError, match="null"):
        sc.bounce_light_rays_dev(w, h, good, d_in.data_ptr(), 0, d_in.data_ptr(), d_rays.data_ptr())
    with pytest.raises(trx.TrxError, match="bounce_samples"):
        sc.render_image_gi(view, w, h, (good,), 0)
    with pytest.raises(trx.TrxError, match="n_lights"):
        sc.render_image_gi(view, w, h, [], 4)
    _sync()
    for t in (d_val, d_rays):
        assert (t.cpu().numpy() == FILL).all()
    with limit():
        pas()   # and the scene is still usable
        torch.cuda.synchronize()
    got = d_val.cpu().numpy()
    assert (got[:n * 4] != FILL).any() and (got[n * 4:] == FILL).all()


def test_device_bytes_count_the_scratch_once(trx, orc):
    """The pass's scratch is counted when it is made, once; a second pass and an AO visibility pass of the same size on the same
    stream add nothing (the shadow rays and flags are the AO pass's buffers)."""
    torch = _torch()
    case = Case(trx, orc, "cornell_64")
    try:
        gi = Gi(case)
        with limit():
            d_prim, d_inst, _, _ = case.primary(0)
        n, tiles = 4, ((case.w + 7) // 8) * ((case.h + 7) // 8)
        # the rays launch of this size first, on the same stream: the launch slot's stack spill area is then sized for it
        d_rays = torch.zeros((tiles * n * 64 * 32,), dtype=torch.uint8, device="cuda")
        d_flags = torch.zeros((tiles * n * 64,), dtype=torch.uint8, device="cuda")
        d_cnt = _buf(case.w * case.h)
        with limit():
            case.sc.trace_occluded_dev(d_rays.data_ptr(), tiles * n * 64, d_flags.data_ptr())
            torch.cuda.synchronize()
        before = case.sc.device_bytes
        gi.device(d_prim, d_inst, _mixed(3), n, 0, (0, 1, 0))
        first = case.sc.device_bytes
        # per ray 32 + 1 (shadow ray, flag) + 32 + 8 + 4 + 24 + 4 (bounce ray, hit, instance id, attributes, sum); per pixel 4
        assert first - before == tiles * n * 64 * 105 + tiles * 64 * 4
        assert first - before <= tiles * n * UNIT
        gi.device(d_prim, d_inst, _mixed(8), n, 0, (0, 1, 0))
        gi.device(d_prim, d_inst, _mixed(3), 2, 3, (1, 3, 1))
        with limit():
            case.sc.trace_ao_visibility_dev(case.view, case.w, case.h, d_prim.data_ptr(), d_cnt.data_ptr(), n, 1.4, d_primary_inst=d_inst.data_ptr())
            torch.cuda.synchronize()
        assert case.sc.device_bytes == first
    finally:
        case.close()


def test_indirect_chain_keeps_its_place_before_a_refit(trx):
    """The pass enqueued on a busy stream, then at once a refit: the refit waits for every launch of the pass, the values are
    the old geometry's."""
    torch = _torch()
    from tray_racing_amd import _lib
    g = np.load(os.path.join(GOLDEN, "soup_52x44.npz"))
    n_tris = g["tri_verts"].shape[0]
    flat = trx.FlatScene(g["nodes"], g["tri_verts"], g["instance_offsets"], int(g["tlas_start"]), np.arange(n_tris), [0, n_tris])
    view = _lib.View()
    C.memmove(C.byref(view), g["view"].tobytes(), C.sizeof(view))
    w, h = int(g["width"]), int(g["height"])
    sc = trx.Scene(flat)
    v = flat.tri_verts
    size = float(np.linalg.norm(v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0)))
    moved = (v + np.random.default_rng(71).normal(scale=2e-2 * size, size=v.shape)).astype(np.float32)
    lights = [LT.Light(LT.POINT, LT.POINT_CASES["soup_52x44"]), LT.Light(LT.RECT, (-0.2, 0.9, -0.2), (0.4, 0.0, 0.0), (0.0, 0.0, 0.4))]
    products = [l.product(trx) for l in lights]
    d_prim = _buf(w * h * 8)

    def chain(stream=0):
        d_val = _buf(w * h * 4)
        sc.trace_indirect_dev(view, w, h, products, d_prim.data_ptr(), d_val.data_ptr(), n_samples=8, bounce_eps=EPS, shadow_eps=EPS, stream=stream)
        return d_val

    try:
        with limit():
            sc.trace_primary_dev(view, w, h, d_prim.data_ptr())
            old = chain()
            torch.cuda.synchronize()
        old = old.cpu().numpy()
        s = torch.cuda.Stream()
        big = random_rays(trx, flat, 2 * 1024 * 1024, 72, zero_dirs=False)
        d_big, d_bh = _dev(big), _buf(big.shape[0] * 8)
        _sync()
        with limit():
            with torch.cuda.stream(s):
                sc.trace_rays_dev(d_big.data_ptr(), big.shape[0], d_bh.data_ptr(), stream=s.cuda_stream)
                got = chain(stream=s.cuda_stream)
            sc.refit(moved)
            s.synchronize()
        assert (got.cpu().numpy() == old).all(), "the pass saw the refit's geometry"
        with limit():
            new = chain()      # (the same primary records: the bounce and shadow rays now meet the moved triangles)
            torch.cuda.synchronize()
        assert (new.cpu().numpy() != old).sum() > 20, "the refit changed nothing"
        sc.check()
    finally:
        sc.close()
