"""The direct-light pass on the GPU, bit for bit and byte for byte (include/trx.h, "direct light"): trx_light_rays_dev writes
the twin's shadow rays (tests/light_twin.py) and the inert ray, trx_trace_light_visibility_dev the twin's planes - fed the
device's own primary records - on single-level, two-level and transformed scenes, in both layouts, for all three kinds of
light, 1, 8 and 64 samples, every semantics word, masked and unmasked, and with a scratch cap small enough that the chunk
loops run; trx_light_term_dev and trx_shade_value_dev against the twin fed the device's records; the host form against its
composition; refusals, the scratch's accounting and the ordering with a refit.  No record is left out of any comparison.

Every step that runs on the GPU sits under a time limit of its own (`limit`): a step that hangs ends the process."""
import contextlib
import ctypes as C
import faulthandler
import os

import numpy as np
import pytest

import light_twin as LT
from ao_visibility_twin import record_map
from helpers import ALL_SEMS, random_rays
from hit_attr_twin import ATTR_DTYPE, tri_records
from image_twin import TERM_DTYPE
from inst_mask_twin import oracle_twin
from test_gpu_ao_visibility import UNIT, Case, make_case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILL = 0x5A
EPS = 0.01
INERT = np.array([0, 0, 0, 0, 0, 0, 0, 0xBF800000], dtype=np.uint32)


def _torch():
    import torch
    return torch


@contextlib.contextmanager
def limit(seconds=120):
    """The time limit of one GPU step: the process ends (with every thread's stack) if the step is still running then."""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _sync():
    with limit():
        _torch().cuda.synchronize()


def _buf(nbytes, fill=FILL):
    torch = _torch()
    return torch.full((max(nbytes, 1),), fill, dtype=torch.uint8, device="cuda")


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _mixed(n):
    """n lights of mixed kinds over the Cornell-class boxes (all within a few units of the origin)."""
    pool = [LT.Light(LT.POINT, (0.0, 1.8, 0.0), intensity=1.5), LT.RECT_CASE, LT.Light(LT.DIRECTIONAL, (0.3, 1.0, 0.4), intensity=0.5),
            LT.Light(LT.POINT, (0.6, 0.4, 0.9)), LT.Light(LT.RECT, (0.5, 0.2, -0.8), (0.0, 0.6, 0.0), (0.4, 0.0, 0.4), intensity=2.0),
            LT.Light(LT.DIRECTIONAL, (-1.0, 0.2, 0.1)), LT.Light(LT.RECT, (-0.9, 1.0, 0.9), (0.3, 0.0, 0.0), (0.0, -0.3, 0.0)),
            LT.Light(LT.POINT, (-0.5, 1.0, -0.5), intensity=0.25)]
    return pool[:n]


class Lit:
    """A Case of tests/test_gpu_ao_visibility.py with what the light twin needs of it."""

    def __init__(self, case):
        self.case, self.w, self.h = case, case.w, case.h
        self.recs = tri_records(case.osc.verts)
        self.w2o = case.osc.w2o if case.transformed else None
        self._geo, self._planes = {}, {}

    def geo(self, prim, inst):
        key = (hash(prim.tobytes()), hash(inst.tobytes()))
        if key not in self._geo:
            self._geo[key] = LT.frame_geometry(self.case.view, self.w, self.h, prim, inst, self.recs, self.w2o)
        return self._geo[key]

    def planes(self, prim, inst, lights, frame0, n, sem, hidden=None):
        """The twin's planes in pixel order; hidden: the TLAS primitives a masked pass does not enter."""
        key = (hash(prim.tobytes()), hash(inst.tobytes()), tuple(l.key() for l in lights), frame0, n, sem, hidden)
        if key not in self._planes:
            osc = self.case.osc
            if hidden:
                vis = np.ones(osc.inst.size, dtype=bool)
                vis[list(hidden)] = False
                import types
                flat = types.SimpleNamespace(nodes=osc.nodes, tri_verts=osc.verts, instance_offsets=osc.inst, tlas_start=int(osc.c.tlas_start))
                osc = oracle_twin(self.case.orc, flat, vis, w2o=osc.w2o)
            self._planes[key] = LT.visibility_planes(self.case.orc, osc, self.case.view, self.w, self.h, self.geo(prim, inst), prim, lights, frame0,
                                                     n, EPS, sem)
        return self._planes[key]

    def device_planes(self, d_prim, d_inst, lights, n, sem, shard, frame0=0, stream=0, mask=0, sc=None, guard=64):
        """The pass's output buffer (n_lights planes and `guard` bytes past them, all FILL before the call)."""
        _, _, size = record_map(self.w, self.h, shard)
        d_out = _buf(len(lights) * size + guard)
        _sync()
        sc = sc or self.case.sc
        with limit():
            sc.trace_light_visibility_dev(self.case.view, self.w, self.h, [l.product(self.case.trx) for l in lights], d_prim.data_ptr(),
                                          d_out.data_ptr(), n_samples=n, sem=sem, ray_mask=mask, frame0=frame0, shadow_eps=EPS,
                                          d_primary_inst=d_inst.data_ptr() if d_inst is not None else 0, shard=(*shard, 0), stream=stream)
            _torch().cuda.synchronize()
            sc.check()
        return d_out.cpu().numpy()

    def expected(self, planes, shard, guard=64):
        pix, rec, size = record_map(self.w, self.h, shard)
        want = np.full(planes.shape[0] * size + guard, FILL, dtype=np.uint8)
        for k in range(planes.shape[0]):
            want[k * size + rec] = planes[k][pix]
        return want


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d bytes differ, first %s: %s != %s" % (what, bad.size, got.size, bad[:4], got[bad[:4]], want[bad[:4]])


@pytest.fixture(scope="module")
def cases(trx, orc):
    made, lit = {}, {}

    def get(name):
        case = make_case(trx, orc, made, name)
        if name not in lit:
            lit[name] = Lit(case)
        return lit[name]
    yield get
    trx.load().trx_debug_ao_scratch_cap(0)
    for c in made.values():
        c.close()


# ---- trx_light_rays_dev ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shard,own_stream", [
    ("cornell_64", (0, 1, 0), False), ("cornell_64", (1, 3, 1), True), ("soup_52x44", (1, 3, 1), False), ("soup_52x44", (0, 1, 0), True),
    ("cornell_tlas_48", (0, 1, 0), True), ("cornell_tlas_48", (1, 3, 1), False), ("instanced", (0, 1, 0), False), ("instanced", (1, 3, 1), True)])
def test_light_rays_are_the_twins_rays_and_the_inert_ray(trx, orc, cases, name, shard, own_stream):
    """All 32 bytes of every ray, for the three kinds of light, samples 0 and 7, and a light placed exactly at a hit point's
    ray origin; a sentinel record on either side of the buffer and in every record outside the shard or the image."""
    torch = _torch()
    lc = cases(name)
    case = lc.case
    st = torch.cuda.Stream() if own_stream else None
    stream = st.cuda_stream if st else 0
    with limit():
        d_prim, d_inst, prim, inst = case.primary(0, shard, stream)
    pix, rec, size = record_map(case.w, case.h, shard)
    geo = lc.geo(prim, inst)
    # a point light exactly at the ray origin of a surface pixel of the shard: dist == 0, NaN, the inert ray
    j = geo[0].size // 2
    eye = np.array(case.view.eye, dtype=np.float32)
    at_origin = LT.Light(LT.POINT, ((eye + geo[3][j] * geo[5][j]) - geo[3][j] * np.float32(EPS)).tolist())
    lights = _mixed(3) + [at_origin]
    for k, light in enumerate(lights):
        for frame0, sample in ((0, 0), (5, 7)) if light.kind == LT.RECT else ((5, 7 * (k & 1)),):
            d_rays = torch.full(((size + 2) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
            _sync()
            with limit():
                case.sc.light_rays_dev(case.view, case.w, case.h, light.product(trx), d_prim.data_ptr(), d_rays.data_ptr() + 32, light_index=k,
                                       frame0=frame0, sample=sample, shadow_eps=EPS, d_primary_inst=d_inst.data_ptr(), shard=(*shard, 0),
                                       stream=stream)
                torch.cuda.synchronize()
            got = d_rays.cpu().numpy().view(np.uint32).reshape(size + 2, 8)
            twin, cast = LT.light_rays(orc, case.view, case.w, case.h, geo, light, k, frame0, sample, EPS)
            want = np.full((size + 2, 8), 0xA5A5A5A5, dtype=np.uint32)     # the guards, and records outside the shard or the image
            want[1 + rec] = twin.view(np.uint32).reshape(-1, 8)[pix]
            what = "%s shard %s light %d (kind %d) sample %d" % (name, shard, k, light.kind, sample)
            bad = np.flatnonzero((got != want).any(1))
            assert bad.size == 0, "%s: %d of %d records differ, first %s: %s != %s" % (what, bad.size, size, bad[:4], got[bad[:1]], want[bad[:1]])
            assert (got[1 + rec[~cast[pix]]] == INERT).all(), what
            if k < 3:
                assert cast[pix].sum() > 30 and (~cast[pix]).sum() > 30, what
            else:
                assert not cast[geo[0][j]] and (got[1 + rec[pix == geo[0][j]]] == INERT).all(), what
    if (shard[1] > 1 and shard[2] == 0) or ((case.w % 8 or case.h % 8) and shard[2] == 1):
        assert (want[1:-1] == 0xA5A5A5A5).all(1).any()                        # (some record really is outside)


# ---- trx_trace_light_visibility_dev -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell_64", "soup_52x44", "cornell_tlas_48", "instanced"])
def test_visibility_planes_equal_the_twin(trx, orc, cases, name):
    """1, 3 and 8 lights of mixed kinds in one call; 1 and 8 samples (64 on the rect light alone); image and shard layouts,
    shard (1, 3) among them, with the planes of the other shards and the bytes past the last plane untouched; a non-null
    stream; TRX_SEM_HLSL and TRX_SEM_CPU everywhere, all eight semantics words on cornell_tlas_48."""
    torch = _torch()
    lc = cases(name)
    case = lc.case
    st = torch.cuda.Stream()
    sets = [_mixed(1), _mixed(3), _mixed(8)]
    for sem in ALL_SEMS if name == "cornell_tlas_48" else (0, 3):
        for shard, stream in (((0, 1, 0), 0), ((1, 3, 1), st.cuda_stream), ((1, 3, 0), 0)) if sem in (0, 3) else (((0, 1, 1), 0),):
            with limit():
                d_prim, d_inst, prim, inst = case.primary(sem, shard, stream)
            for lights in sets if sem in (0, 3) and shard[2] != 0 or shard == (0, 1, 0) and sem == 0 else sets[1:2]:
                for n in (1, 8):
                    got = lc.device_planes(d_prim, d_inst, lights, n, sem, shard, frame0=3, stream=stream)
                    want = lc.expected(lc.planes(prim, inst, lights, 3, n, sem), shard)
                    _same(got, want, "%s sem %d shard %s %d lights n %d" % (name, sem, shard, len(lights), n))
            if sem == 0 and shard == (0, 1, 0):
                got = lc.device_planes(d_prim, d_inst, [LT.RECT_CASE], 64, sem, shard, frame0=1)
                want = lc.expected(lc.planes(prim, inst, [LT.RECT_CASE], 1, 64, sem), shard)
                _same(got, want, "%s 64 samples" % name)
                if name == "cornell_tlas_48":
                    surf = want[:case.w * case.h][want[:case.w * case.h] != LT.NO_SURFACE]
                    assert ((surf > 0) & (surf < 64)).mean() >= 0.05 and (surf == 0).any() and (surf == 64).any()
            if shard[1] > 1 and shard[2] == 0:
                assert (want[:-64] == FILL).any()                               # (records of other shards)


@pytest.mark.parametrize("name,patterns", [("cornell_tlas_48", ((LT.MASK_HIDES,), (0, 4))), ("instanced", ((3,), (1, 6, 7, 12)))])
def test_masked_shadow_rays_skip_the_hidden_instances(trx, orc, cases, name, patterns):
    """ray_mask 0 with a table set reads no table; a masked pass answers what the twin scene with every hidden instance
    pointed at an empty BLAS answers (tests/inst_mask_twin.py)."""
    lc = cases(name)
    case = lc.case
    lights = _mixed(3)
    n_inst = case.osc.inst.size
    try:
        for sem, shard in ((0, (0, 1, 0)), (3, (1, 3, 1))):
            with limit():
                d_prim, d_inst, prim, inst = case.primary(sem, shard)
            open_planes = lc.planes(prim, inst, lights, 0, 8, sem)
            for hidden in patterns:
                masks = np.full(n_inst, 0xFF, dtype=np.uint8)
                masks[list(hidden)] = 0x11
                case.sc.set_instance_masks(masks)
                what = "%s sem %d shard %s hidden %s" % (name, sem, shard, hidden)
                _same(lc.device_planes(d_prim, d_inst, lights, 8, sem, shard), lc.expected(open_planes, shard), what + " ray_mask 0")
                _same(lc.device_planes(d_prim, d_inst, lights, 8, sem, shard, mask=0x10), lc.expected(open_planes, shard), what + " ray_mask 0x10")
                masked = lc.planes(prim, inst, lights, 0, 8, sem, hidden=tuple(hidden))
                _same(lc.device_planes(d_prim, d_inst, lights, 8, sem, shard, mask=0x0E), lc.expected(masked, shard), what + " ray_mask 0x0E")
                if hidden == patterns[0] and shard[1] == 1:
                    assert (masked != open_planes).sum() > 10, what + ": the mask changes nothing"
    finally:
        case.sc.set_instance_masks(None)


def test_masked_calls_on_a_single_level_scene_equal_unmasked_ones(trx, orc, cases):
    lc = cases("cornell_64")
    with limit():
        d_prim, d_inst, prim, inst = lc.case.primary(0)
    want = lc.expected(lc.planes(prim, inst, _mixed(3), 0, 8, 0), (0, 1, 0))
    for mask in (0, 1, 0x80, 0xFF):
        _same(lc.device_planes(d_prim, d_inst, _mixed(3), 8, 0, (0, 1, 0), mask=mask), want, "ray_mask %d" % mask)


@pytest.mark.parametrize("name", ["cornell_64", "instanced"])
def test_chunk_loops_give_the_same_planes(trx, orc, cases, name):
    """A scratch cap below the pass's need: samples in several chunks (counts added to), tiles in several chunks, both."""
    lib = trx.load()
    lc = cases(name)
    case = lc.case
    tiles = ((case.w + 7) // 8) * ((case.h + 7) // 8)
    lights = _mixed(3)
    try:
        for sem, shard in ((0, (0, 1, 0)), (3, (0, 1, 1))):
            with limit():
                d_prim, d_inst, prim, inst = case.primary(sem, shard)
            want = lc.expected(lc.planes(prim, inst, lights, 0, 8, sem), shard)
            for cap in (UNIT * tiles * 3, UNIT * tiles, UNIT * 10, UNIT * (tiles // 2 + 1) * 2, 1):
                lib.trx_debug_ao_scratch_cap(cap)
                _same(lc.device_planes(d_prim, d_inst, lights, 8, sem, shard), want, "%s sem %d cap %d" % (name, sem, cap))
    finally:
        lib.trx_debug_ao_scratch_cap(0)


@pytest.mark.parametrize("name", ["cornell_64", "cornell_tlas_48", "instanced"])
def test_a_point_lights_plane_is_the_occlusion_of_its_rays(trx, cases, name):
    """plane = 1 - trx_trace_occluded_dev over trx_light_rays_dev's rays where the ray is not inert, 0 where it is."""
    torch = _torch()
    lc = cases(name)
    case = lc.case
    n = case.w * case.h
    light = _mixed(1)[0]
    for sem in (0, 3, 6):
        with limit():
            d_prim, d_inst, prim, _ = case.primary(sem)
        d_rays, d_flags = _buf(n * 32), _buf(n)
        with limit():
            case.sc.light_rays_dev(case.view, case.w, case.h, light.product(trx), d_prim.data_ptr(), d_rays.data_ptr(), shadow_eps=EPS,
                                   d_primary_inst=d_inst.data_ptr())
            case.sc.trace_occluded_dev(d_rays.data_ptr(), n, d_flags.data_ptr(), sem=sem)
            torch.cuda.synchronize()
        plane = lc.device_planes(d_prim, d_inst, [light], 4, sem, (0, 1, 0), guard=0)
        rays = d_rays.cpu().numpy().view(np.uint32).reshape(n, 8)
        cast = ~(rays == INERT).all(1)
        flags = d_flags.cpu().numpy()
        surf = LT.surface(prim)
        assert (plane[~surf] == LT.NO_SURFACE).all() and (plane[surf & ~cast] == 0).all() and not cast[~surf].any(), (name, sem)
        assert (plane[cast] == 1 - flags[cast]).all() and 0 < flags[cast].sum() < cast.sum(), (name, sem)


def test_the_pipelined_walk_gives_the_same_planes(trx, orc, cases):
    """cornell_64_pipe: the padded twin of cornell_64, whose any-hit rays launch takes the pipelined walk (asserted by make_case
    as tests/test_gpu_pipelined_walk.py does); byte for byte the twin's planes and the unpadded scene's."""
    lc = cases("cornell_64_pipe")
    case = lc.case
    assert case.sc.walk_kind(trx.MODE_RAYS) == trx.WALK_PIPELINED and case.base.sc.walk_kind(trx.MODE_RAYS) == trx.WALK_PLAIN
    lights = _mixed(3)
    for sem, shard in ((0, (0, 1, 0)), (3, (1, 3, 1))):
        with limit():
            d_prim, d_inst, prim, inst = case.primary(sem, shard)
        want = lc.expected(lc.planes(prim, inst, lights, 2, 8, sem), shard)
        _same(lc.device_planes(d_prim, d_inst, lights, 8, sem, shard, frame0=2), want, "pipelined sem %d" % sem)
        _same(lc.device_planes(d_prim, d_inst, lights, 8, sem, shard, frame0=2, sc=case.base.sc), want, "plain sem %d" % sem)


# ---- trx_light_term_dev, trx_shade_value_dev, trx_render_image_lit ---------------------------------------------------------

@pytest.fixture(scope="module")
def cornell(trx):
    """The Cornell stand-in and its camera: views of any size."""
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    sc = trx.Scene(flat)
    eye, look, fov = trx.scene_camera("cornell")
    yield sc, eye, look, fov
    sc.close()


def _frame(trx, sc, view, w, h, shard, lights, n, sem=0, mask=0):
    """(device buffers, host copies in pixel order) of the primary, attribute and light visibility passes."""
    torch = _torch()
    pix, rec, size = record_map(w, h, shard)
    d_prim, d_inst, d_attr, d_lit = _buf(size * 8, 0xEE), _buf(size * 4, 0xFF), _buf(size * 24, 0), _buf(len(lights) * size)
    from tray_racing_amd import _lib as L
    with limit():
        L.check(sc._lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, L.Shard(*shard, 0), sem, C.c_void_p(d_prim.data_ptr()),
                                                   C.c_void_p(d_inst.data_ptr()), None))
        sc.hit_attributes_primary_dev(view, w, h, d_prim.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr(), shard=(*shard, 0))
        sc.trace_light_visibility_dev(view, w, h, [l.product(trx) for l in lights], d_prim.data_ptr(), d_lit.data_ptr(), n_samples=n, sem=sem,
                                      ray_mask=mask, shadow_eps=EPS, d_primary_inst=d_inst.data_ptr(), shard=(*shard, 0))
        torch.cuda.synchronize()
    prim = np.zeros(w * h, dtype=trx.HIT_DTYPE)
    prim["t"], prim["prim"] = np.inf, 0xFFFFFFFF
    prim[pix] = d_prim.cpu().numpy().view(trx.HIT_DTYPE)[rec]
    normals = np.zeros((w * h, 3), dtype=np.float32)
    normals[pix] = d_attr.cpu().numpy().view(ATTR_DTYPE)["normal"][rec]
    planes = np.full((len(lights), w * h), LT.NO_SURFACE, dtype=np.uint8)
    lit = d_lit.cpu().numpy().reshape(len(lights), size)
    planes[:, pix] = lit[:, rec]
    return (d_prim, d_inst, d_attr, d_lit), (prim, normals, planes)


@pytest.mark.parametrize("w,h,shard,away", [(1, 1, (0, 1, 0), False), (7, 3, (0, 1, 0), False), (40, 24, (0, 1, 0), False), (40, 24, (1, 3, 1), False),
                                           (37, 21, (1, 3, 1), False), (37, 21, (2, 3, 0), False), (16, 9, (0, 1, 0), True)])
def test_light_term_equals_the_twin(trx, cornell, w, h, shard, away):
    """Bit for bit against the twin fed the device's records, with and without d_term; an image of misses among the cases
    (the camera turned away), a 1x1 and a 7x3 image, shard (1, 3) in TRX_LAYOUT_SHARD; the value buffer's other records and
    the bytes past it untouched."""
    torch = _torch()
    sc, eye, look, fov = cornell
    eye, look = np.array(eye, dtype=np.float64), np.array(look, dtype=np.float64)
    if away:   # (from far behind the camera, looking further away: every pixel a miss)
        eye, look = eye + 50.0 * (eye - look), eye + 51.0 * (eye - look)
    view = trx.view_from_camera(eye.tolist(), look.tolist(), fov, w, h)
    lights, n = _mixed(8), 4
    (d_prim, d_inst, d_attr, d_lit), (prim, normals, planes) = _frame(trx, sc, view, w, h, shard, lights, n)
    pix, rec, size = record_map(w, h, shard)
    surf = LT.surface(prim)
    assert not surf.any() if away else surf[pix].any() or w * h < 20     # (the one pixel of the 1x1 image may look past the box)
    rng = np.random.default_rng(w * h)
    term = np.zeros(size, dtype=TERM_DTYPE)
    term["samples"] = rng.choice([0, 4, 36, 100], size)
    term["unoccluded"] = (term["samples"] * rng.random(size)).astype(np.uint16)
    term_px = np.zeros(w * h, dtype=TERM_DTYPE)
    term_px[pix] = term[rec]
    d_term = _dev(term)
    for tm, ambient in ((None, 0.25), (term_px, 0.5), (None, 0.0)):
        d_val = _buf(size * 4 + 64)
        _sync()
        with limit():
            sc.light_term_dev(view, w, h, [l.product(trx) for l in lights], d_prim.data_ptr(), d_attr.data_ptr(), d_lit.data_ptr(), d_val.data_ptr(),
                              n_samples=n, ambient=ambient, d_term=0 if tm is None else d_term.data_ptr(), shard=(*shard, 0))
            torch.cuda.synchronize()
        got = d_val.cpu().numpy()
        want = np.full(size * 4 + 64, FILL, dtype=np.uint8)
        twin = LT.light_term(view, w, h, prim, normals, planes, lights, n, ambient, tm)
        want[:size * 4].view(np.uint32)[rec] = twin.view(np.uint32)[pix]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%dx%d shard %s ambient %g: %d bytes differ, first at %s" % (w, h, shard, ambient, bad.size, bad[:4])
        if not away and w * h > 100:
            assert np.unique(twin[pix]).size > 20
        if away:
            assert (twin == 0).all()
    sc.check()


def test_value_shade_equals_the_code_table_shade(trx, cornell):
    """Negative, NaN, 1.0, infinities, and both neighbours of every eighth threshold; nothing written past n_records * 4."""
    torch = _torch()
    sc = cornell[0]
    thr = trx.image_code_table()
    ks = thr[1::8]
    v = np.concatenate([np.array([-1.0, -0.0, 0.0, np.nan, 1.0, np.nextafter(np.float32(1), np.float32(0)), 2.0, np.inf, -np.inf, 1e-30, 0.5],
                                 dtype=np.float32), ks, np.nextafter(ks, np.float32(0)), np.nextafter(ks, np.float32(2)),
                        np.random.default_rng(9).random(1000, dtype=np.float32)]).astype(np.float32)
    d_v, d_rgba = _dev(v), _buf(v.size * 4 + 64)
    with limit():
        sc.shade_value_dev(d_v.data_ptr(), v.size, d_rgba.data_ptr())
        torch.cuda.synchronize()
    got = d_rgba.cpu().numpy()
    assert (got[v.size * 4:] == FILL).all()
    want = LT.shade_value(v)
    assert (got[:v.size * 4].reshape(-1, 4) == want).all(), np.flatnonzero((got[:v.size * 4].reshape(-1, 4) != want).any(1))[:8]
    assert np.unique(want[:, 0]).size > 60
    with limit():
        sc.shade_value_dev(d_v.data_ptr(), 0, d_rgba.data_ptr())       # n_records == 0 does nothing
        torch.cuda.synchronize()
    assert (d_rgba.cpu().numpy() == got).all()


@pytest.mark.parametrize("ao,mask", [(0, 0), (4, 0), (4, 0x0E)])
def test_host_form_is_its_composition(trx, cases, ao, mask):
    """trx_render_image_lit against the device-resident calls it is made of, on cornell_tlas_48 (with a mask table set) and
    on the transformed scene."""
    torch = _torch()
    for name in ("cornell_tlas_48", "instanced"):
        case = cases(name).case
        sc, view, w, h = case.sc, case.view, case.w, case.h
        n_px = w * h
        lights, n, sem = _mixed(3), 4, 3
        masks = np.full(case.osc.inst.size, 0xFF, dtype=np.uint8)
        masks[LT.MASK_HIDES] = 0x11
        sc.set_instance_masks(masks)
        try:
            with limit():
                img, ms = sc.render_image_lit(view, w, h, [l.product(trx) for l in lights], sem=sem, ray_mask=mask, frame0=2, light_samples=n,
                                              shadow_eps=EPS, ambient=0.3, ao_samples=ao, ao_eps=EPS, ao_radius=case.radius, filter_radius=1)
            (d_prim, d_inst, d_attr, d_lit), _ = _frame(trx, sc, view, w, h, (0, 1, 0), lights, n, sem=sem, mask=mask)
            d_lit = _buf(len(lights) * n_px)
            d_cnt, d_term, d_val, d_rgba = _buf(n_px), _buf(n_px * 4), _buf(n_px * 4), _buf(n_px * 4)
            with limit():
                sc.trace_light_visibility_dev(view, w, h, [l.product(trx) for l in lights], d_prim.data_ptr(), d_lit.data_ptr(), n_samples=n, sem=sem,
                                              ray_mask=mask, frame0=2, shadow_eps=EPS, d_primary_inst=d_inst.data_ptr())
                if ao:
                    sc.trace_ao_visibility_dev(view, w, h, d_prim.data_ptr(), d_cnt.data_ptr(), ao, case.radius, sem=sem, frame0=2, ao_eps=EPS,
                                               d_primary_inst=d_inst.data_ptr())
                    sc.ao_filter_dev(w, h, d_prim.data_ptr(), d_cnt.data_ptr(), d_term.data_ptr(), ao, 1, d_attr=d_attr.data_ptr())
                sc.light_term_dev(view, w, h, [l.product(trx) for l in lights], d_prim.data_ptr(), d_attr.data_ptr(), d_lit.data_ptr(),
                                  d_val.data_ptr(), n_samples=n, ambient=0.3, d_term=d_term.data_ptr() if ao else 0)
                sc.shade_value_dev(d_val.data_ptr(), n_px, d_rgba.data_ptr())
                torch.cuda.synchronize()
            want = d_rgba.cpu().numpy().reshape(h, w, 4)
            assert ms > 0 and (img == want).all(), (name, ao, mask, (img != want).sum())
            assert np.unique(img[..., 0]).size > 8 and (img[..., 3] == 255).all()
            sc.check()
        finally:
            sc.set_instance_masks(None)


# ---- refusals, scratch, ordering ---------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(trx, cases):
    torch = _torch()
    lc = cases("instanced")
    case = lc.case
    sc, view, w, h = case.sc, case.view, case.w, case.h
    with limit():
        d_prim, d_inst, _, _ = case.primary(0)
    n = w * h
    good = _mixed(1)[0].product(trx)
    d_lit, d_rays, d_val, d_attr = _buf(2 * n), _buf(n * 32), _buf(n * 4), _buf(n * 24, 0)

    def vis(lights=(good,), ns=4, mask=0, eps=EPS, sem=0, inst=d_inst.data_ptr()):
        sc.trace_light_visibility_dev(view, w, h, lights, d_prim.data_ptr(), d_lit.data_ptr(), n_samples=ns, sem=sem, ray_mask=mask, shadow_eps=eps,
                                      d_primary_inst=inst)

    bad_kind, bad_pad, bad_nan, bad_dir = (trx.light(7, (0, 1, 0)), trx.light(trx.LIGHT_POINT, (0, 1, 0)), trx.light(trx.LIGHT_POINT, (0, float("nan"), 0)),
                                           trx.light(trx.LIGHT_DIRECTIONAL, (0, 0, 0)))
    bad_pad._pad[2] = 9
    for kw, msg in (({"lights": [good] * 9}, "n_lights"), ({"lights": (good, bad_kind)}, "kind"), ({"lights": (bad_pad,)}, "_pad"),
                    ({"lights": (bad_nan,)}, "finite"), ({"lights": (bad_dir,)}, "zero length"), ({"ns": 0}, "n_samples"), ({"ns": 65}, "n_samples"),
                    ({"mask": 256}, "ray_mask"), ({"eps": -1.0}, "shadow_eps"), ({"eps": float("nan")}, "shadow_eps"), ({"sem": 8}, "semantics"),
                    ({"inst": 0}, "instance transforms")):
        with pytest.raises(trx.TrxError, match=msg) as e:
            vis(**kw)
        assert e.value.code == -1, kw
    with pytest.raises(trx.TrxError, match="instance transforms"):
        sc.light_rays_dev(view, w, h, good, d_prim.data_ptr(), d_rays.data_ptr())
    with pytest.raises(trx.TrxError, match="shadow_eps"):
        sc.light_rays_dev(view, w, h, good, d_prim.data_ptr(), d_rays.data_ptr(), shadow_eps=-0.5, d_primary_inst=d_inst.data_ptr())
    with pytest.raises(trx.TrxError, match="kind"):
        sc.light_rays_dev(view, w, h, bad_kind, d_prim.data_ptr(), d_rays.data_ptr(), d_primary_inst=d_inst.data_ptr())
    with pytest.raises(trx.TrxError, match="ambient"):
        sc.light_term_dev(view, w, h, (good,), d_prim.data_ptr(), d_attr.data_ptr(), d_lit.data_ptr(), d_val.data_ptr(), ambient=float("inf"))
    with pytest.raises(trx.TrxError, match="_pad"):
        sc.light_term_dev(view, w, h, (bad_pad,), d_prim.data_ptr(), d_attr.data_ptr(), d_lit.data_ptr(), d_val.data_ptr())
    with pytest.raises(trx.TrxError, match="n_lights"):
        sc.render_image_lit(view, w, h, [])
    with pytest.raises(trx.TrxError, match="ao_radius"):
        sc.render_image_lit(view, w, h, (good,), ao_samples=4, ao_radius=0.0)
    _sync()
    for t in (d_lit, d_rays, d_val):
        assert (t.cpu().numpy() == FILL).all()
    with limit():
        vis()   # and the scene is still usable
        torch.cuda.synchronize()
    got = d_lit.cpu().numpy()
    assert (got[:n] != FILL).any() and (got[n:] == FILL).all()


def test_device_bytes_count_the_scratch_once(trx, orc):
    """An AO visibility pass and a light pass of the same size on one stream share the launch slot's scratch."""
    torch = _torch()
    case = Case(trx, orc, "cornell_64")
    try:
        lc = Lit(case)
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
        with limit():
            case.sc.trace_ao_visibility_dev(case.view, case.w, case.h, d_prim.data_ptr(), d_cnt.data_ptr(), n, 1.4, d_primary_inst=d_inst.data_ptr())
            torch.cuda.synchronize()
        first = case.sc.device_bytes
        assert first - before == tiles * n * UNIT
        lc.device_planes(d_prim, d_inst, _mixed(8), n, 0, (0, 1, 0))
        lc.device_planes(d_prim, d_inst, _mixed(3), 2, 3, (1, 3, 1))
        assert case.sc.device_bytes == first
    finally:
        case.close()


def test_light_chain_keeps_its_place_before_a_refit(trx):
    """The light visibility pass enqueued on a busy stream, then at once a refit: the refit waits for every launch of the
    pass, the planes are the old geometry's."""
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
        d_lit = _buf(2 * w * h)
        sc.trace_light_visibility_dev(view, w, h, products, d_prim.data_ptr(), d_lit.data_ptr(), n_samples=8, shadow_eps=EPS, stream=stream)
        return d_lit

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
            new = chain()      # (the same primary records: the shadow rays now meet the moved triangles)
            torch.cuda.synchronize()
        assert (new.cpu().numpy() != old).sum() > 20, "the refit changed nothing"
        sc.check()
    finally:
        sc.close()
