"""The sparse indirect term on the GPU, bit for bit (include/trx.h: trx_trace_indirect_sparse_dev, trx_value_upsample_dev,
trx_render_image_gi_sparse).  The sparse values against the twin (tests/indirect_twin.py subsampled by
tests/indirect_sparse_twin.py) - fed the device's own primary records - on single-level, two-level and transformed scenes, for
strides 1..4, 1 and 3 lights (a rect light among them: the noise of the full-resolution pixel), 1, 3 and 16 samples, every
semantics word, masked and unmasked, with sentinels on either side of the low plane, under a scratch cap small enough that
both chunk loops run, and at stride 1 against trx_trace_indirect_dev's own bytes; the upsample against the twin fed the
device's own records and sparse values, and on hand-made images uploaded as records; refusals, the scratch's accounting, the
ordering with a refit; the host form against its composition.  NaN-ness is compared, not a NaN's payload.  No cell and no
pixel is left out of any comparison.

Every step that runs on the GPU sits under a time limit of its own (`limit`): a step that hangs ends the process."""
import ctypes as C
import os

import numpy as np
import pytest

import indirect_sparse_twin as ST
import indirect_twin as IT
import light_twin as LT
import value_filter_twin as VT
from ao_sparse_twin import ACCEPTED, EMPTY, FALLBACK, cell_pixels, class_counts, lo_size
from helpers import ALL_SEMS, random_rays
from hit_attr_twin import ATTR_DTYPE, tri_records
from test_gpu_ao_visibility import Case, make_case
from test_gpu_indirect import ALBEDO, UNIT, Gi
from test_gpu_light import EPS, FILL, _buf, _dev, _mixed, _sync, _torch, limit

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = float("inf")
TOL, COS = 0.10, 0.9
GUARD = 64                # sentinel bytes on either side of the outputs
GRIDS = ((1, 0), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0), (3, 8), (4, 0), (4, 15))   # all phases at 2, the first and the last at 3 and 4
SCENES = ["cornell_64", "soup_52x44", "cornell_tlas_48", "instanced"]
f32 = np.float32


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


def _same(got, want, what):
    bad = VT.same_bits(got, want)
    assert bad.size == 0, "%s: %d of %d values differ, first at %s: %s != %s" % (what, bad.size, np.size(got), bad[:4], np.asarray(got)[bad[:4]],
                                                                                np.asarray(want)[bad[:4]])


def _guarded(n_floats, inner=None):
    """A device buffer of n floats between two sentinels (FILL bytes; `inner`: the floats' initial contents)."""
    raw = np.full(n_floats * 4 + 2 * GUARD, FILL, dtype=np.uint8)
    if inner is not None:
        raw[GUARD:GUARD + n_floats * 4] = np.ascontiguousarray(inner, dtype=np.float32).view(np.uint8)
    return _dev(raw)


def _inner(d_buf, n_floats, what):
    raw = d_buf.cpu().numpy()
    assert (raw[:GUARD] == FILL).all() and (raw[GUARD + n_floats * 4:] == FILL).all(), what + ": a sentinel was written"
    return raw[GUARD:GUARD + n_floats * 4].view(np.float32).copy()


def _sparse(case, d_prim, d_inst, lights, n, sem, stride, phase, frame0=0, mask=0, stream=0, sc=None, what="sparse"):
    """The low plane's floats, after checking the sentinels on either side of it."""
    wlo, hlo = lo_size(case.w, case.h, stride)
    d_lo = _guarded(wlo * hlo)
    _sync()
    sc = sc or case.sc
    with limit():
        sc.trace_indirect_sparse_dev(case.view, case.w, case.h, stride, phase, [l.product(case.trx) for l in lights], d_prim.data_ptr(),
                                     d_lo.data_ptr() + GUARD, n_samples=n, sem=sem, ray_mask=mask, frame0=frame0, bounce_eps=EPS, shadow_eps=EPS,
                                     bounce_albedo=ALBEDO, d_primary_inst=d_inst.data_ptr() if d_inst is not None else 0, stream=stream)
        _torch().cuda.synchronize()
        sc.check()
    return _inner(d_lo, wlo * hlo, what)


# ---- 1. the sparse values ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_sparse_values_equal_the_twin(trx, orc, cases, name):
    """Strides 1..4 (every phase of 2, the first and the last of 3 and 4); 1 light and 1 sample, 3 lights of mixed kinds (a rect
    light among them) and 3 samples, 1 light and 16 samples; a non-null stream; stride 1 is trx_trace_indirect_dev without a
    base, byte for byte."""
    torch = _torch()
    gi = cases(name)
    case, w, h = gi.case, gi.w, gi.h
    st = torch.cuda.Stream()
    with limit():
        d_prim, d_inst, prim, inst = case.primary(0)
    surf = LT.surface(prim)
    for n_lights, n in ((1, 1), (3, 3), (1, 16)):
        lights = _mixed(n_lights)
        assert n_lights == 1 or any(l.kind == LT.RECT for l in lights)
        dense = gi.twin(prim, inst, lights, 3, n, 0)
        for k, (stride, phase) in enumerate(GRIDS):
            what = "%s %d lights n %d stride %d phase %d" % (name, n_lights, n, stride, phase)
            got = _sparse(case, d_prim, d_inst, lights, n, 0, stride, phase, frame0=3, stream=st.cuda_stream if k % 2 else 0, what=what)
            want = ST.sparse_values(dense, prim, w, h, stride, phase)
            _same(got, want, what)
            if stride == 1:
                raw, before = gi.device(d_prim, d_inst, lights, n, 0, (0, 1, 0), frame0=3)
                assert (raw[:w * h * 4].view(np.uint32) == got.view(np.uint32)).all(), what + ": differs from the dense pass"
            if (stride, phase) == (2, 0) and n == 3:
                # not vacuous: a cell without a surface, a surface cell at 0, a surface cell above 0 (tests/test_indirect_sparse.py)
                gx, gy, inside = cell_pixels(w, h, stride, phase)
                c_surf = (inside & surf.reshape(h, w)[np.minimum(gy, h - 1), np.minimum(gx, w - 1)]).reshape(-1)
                assert (~c_surf).any() and (c_surf & (got > 0)).sum() > 10 and np.unique(got).size > 10, what
            if name == "soup_52x44" and (stride, phase) == (3, 8):
                outside = ~cell_pixels(w, h, stride, phase)[2].reshape(-1)           # 52 and 44 are no multiples of 3
                assert outside.sum() > 10 and not got.view(np.uint32)[outside].any(), what


def test_every_semantics_word(trx, orc, cases):
    gi = cases("cornell_64")
    for sem in ALL_SEMS:
        with limit():
            d_prim, d_inst, prim, inst = gi.case.primary(sem)
        lights = _mixed(3)
        stride, phase = (2, sem % 4) if sem % 2 else (3, sem)
        got = _sparse(gi.case, d_prim, d_inst, lights, 1, sem, stride, phase, frame0=2)
        _same(got, ST.sparse_values(gi.twin(prim, inst, lights, 2, 1, sem), prim, gi.w, gi.h, stride, phase), "cornell_64 sem %d" % sem)


def test_masked_shadow_rays_on_a_two_level_scene(trx, orc, cases):
    """ray_mask 0 with a table set reads no table; a masked pass's shadow rays skip the hidden instance, its bounce rays do not."""
    gi = cases("cornell_tlas_48")
    case = gi.case
    lights, n = _mixed(3), 3
    with limit():
        d_prim, d_inst, prim, inst = case.primary(0)
    masks = np.full(case.osc.inst.size, 0xFF, dtype=np.uint8)
    masks[LT.MASK_HIDES] = 0x11
    try:
        case.sc.set_instance_masks(masks)
        open_values = ST.sparse_values(gi.twin(prim, inst, lights, 0, n, 0), prim, gi.w, gi.h, 2, 3)
        _same(_sparse(case, d_prim, d_inst, lights, n, 0, 2, 3), open_values, "ray_mask 0")
        _same(_sparse(case, d_prim, d_inst, lights, n, 0, 2, 3, mask=0x10), open_values, "ray_mask 0x10")
        masked = ST.sparse_values(gi.twin(prim, inst, lights, 0, n, 0, hidden=(LT.MASK_HIDES,)), prim, gi.w, gi.h, 2, 3)
        _same(_sparse(case, d_prim, d_inst, lights, n, 0, 2, 3, mask=0x0E), masked, "ray_mask 0x0E")
        assert (masked.view(np.uint32) != open_values.view(np.uint32)).sum() > 5, "the mask changes nothing"
    finally:
        case.sc.set_instance_masks(None)


@pytest.mark.parametrize("name", ["cornell_64", "instanced"])
def test_chunk_loops_give_the_same_cells(trx, orc, cases, name):
    """A scratch cap below the pass's need: samples in several chunks (running sums added to), tiles of the low grid in several
    chunks, both - bit for bit the uncapped pass's values and the twin's."""
    lib = trx.load()
    gi = cases(name)
    case = gi.case
    lights, n = _mixed(3), 5
    with limit():
        d_prim, d_inst, prim, inst = case.primary(0)
    dense = gi.twin(prim, inst, lights, 0, n, 0)
    try:
        for stride, phase in ((2, 3), (3, 0)):
            wlo, hlo = lo_size(case.w, case.h, stride)
            tiles = ((wlo + 7) // 8) * ((hlo + 7) // 8)
            assert tiles >= 4
            lib.trx_debug_ao_scratch_cap(0)
            whole = _sparse(case, d_prim, d_inst, lights, n, 0, stride, phase)
            _same(whole, ST.sparse_values(dense, prim, case.w, case.h, stride, phase), "%s stride %d uncapped" % (name, stride))
            for cap in (UNIT * tiles * 3, UNIT * tiles, UNIT * 3, UNIT * (tiles // 2 + 1) * 2, 1):
                lib.trx_debug_ao_scratch_cap(cap)
                got = _sparse(case, d_prim, d_inst, lights, n, 0, stride, phase)
                assert (got.view(np.uint32) == whole.view(np.uint32)).all(), "%s stride %d cap %d: %d cells differ" % (
                    name, stride, cap, (got.view(np.uint32) != whole.view(np.uint32)).sum())
    finally:
        lib.trx_debug_ao_scratch_cap(0)


def test_the_pipelined_walk_gives_the_same_values(trx, orc, cases):
    """cornell_64_pipe: the padded twin of cornell_64 (helpers.padded_flat), whose rays launches take the pipelined walk; bit for
    bit the twin's values and the unpadded scene's."""
    gi = cases("cornell_64_pipe")
    case = gi.case
    assert case.sc.walk_kind(trx.MODE_RAYS) == trx.WALK_PIPELINED and case.base.sc.walk_kind(trx.MODE_RAYS) == trx.WALK_PLAIN
    lights = _mixed(3)
    with limit():
        d_prim, d_inst, prim, inst = case.primary(3)
    want = ST.sparse_values(gi.twin(prim, inst, lights, 2, 3, 3), prim, gi.w, gi.h, 2, 1)
    _same(_sparse(case, d_prim, d_inst, lights, 3, 3, 2, 1, frame0=2), want, "pipelined")
    _same(_sparse(case, d_prim, d_inst, lights, 3, 3, 2, 1, frame0=2, sc=case.base.sc), want, "plain")


@pytest.fixture(scope="module")
def cornell(trx, orc):
    """The Cornell stand-in on the device and on the oracle, and its camera: views of any size."""
    verts, counts = trx.gen_scene("cornell", 0, 1)
    flat = trx.flat_build(verts, counts)
    sc = trx.Scene(flat)
    eye, look, fov = trx.scene_camera("cornell")
    yield sc, orc.Scene.from_flat(flat), tri_records(flat.tri_verts), eye, look, fov
    sc.close()


@pytest.mark.parametrize("w,h,away", [(1, 1, False), (7, 3, False), (37, 21, False), (16, 9, True)])
def test_small_images_and_an_image_of_misses(trx, orc, cornell, w, h, away):
    """A 1x1 and a 7x3 image (at stride 4 a low grid of 1x1 and 2x1 cells, at phase 15 every cell's pixel outside the image), an
    odd-sized image, and the camera turned away: every cell +0."""
    torch = _torch()
    from tray_racing_amd import _lib as L
    sc, osc, recs, eye, look, fov = cornell
    eye, look = np.array(eye, dtype=np.float64), np.array(look, dtype=np.float64)
    if away:   # (from far behind the camera, looking further away: every pixel a miss)
        eye, look = eye + 50.0 * (eye - look), eye + 51.0 * (eye - look)
    view = trx.view_from_camera(eye.tolist(), look.tolist(), fov, w, h)
    n = w * h
    d_prim, d_inst = _buf(n * 8, 0xEE), _buf(n * 4, 0xFF)
    with limit():
        L.check(sc._lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, L.Shard(0, 1, 0, 0), 0, C.c_void_p(d_prim.data_ptr()),
                                                   C.c_void_p(d_inst.data_ptr()), None))
        torch.cuda.synchronize()
    prim = d_prim.cpu().numpy().view(orc.HIT_DTYPE).copy()
    inst = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    lights, ns = _mixed(3), 4
    dense = IT.indirect(orc, osc, orc.view_from_bytes(bytes(view)), w, h, prim, inst, recs, None, lights, 0, ns, EPS, EPS, ALBEDO, 0)
    for stride, phase in ((1, 0), (2, 3), (3, 4), (4, 0), (4, 15)):
        wlo, hlo = lo_size(w, h, stride)
        d_lo = _guarded(wlo * hlo)
        _sync()
        with limit():
            sc.trace_indirect_sparse_dev(view, w, h, stride, phase, [l.product(trx) for l in lights], d_prim.data_ptr(), d_lo.data_ptr() + GUARD,
                                         n_samples=ns, bounce_eps=EPS, shadow_eps=EPS, bounce_albedo=ALBEDO)
            torch.cuda.synchronize()
        what = "%dx%d stride %d phase %d" % (w, h, stride, phase)
        got = _inner(d_lo, wlo * hlo, what)
        _same(got, ST.sparse_values(dense, prim, w, h, stride, phase), what)
        if away or ((w, h) in ((1, 1), (7, 3)) and phase == 15):
            assert not got.view(np.uint32).any(), what
    if (w, h) == (7, 3):
        assert lo_size(w, h, 4) == (2, 1)
    if not away and n > 100:
        assert (dense > 0).sum() > 20
    sc.check()


# ---- 2. the upsample ----------------------------------------------------------------------------------------------------------

class Frame:
    """A case's frame on the device and on the host: primary records, attribute records, and per grid the device's own sparse
    4-sample values of a point light - the upsample's inputs as the device made them."""

    def __init__(self, trx, case):
        self.case, self.w, self.h, self.n = case, case.w, case.h, case.w * case.h
        self.light = [LT.Light(LT.POINT, LT.POINT_CASES.get(case.name, (0.0, 1.8, 0.0)), intensity=1.5)]
        with limit():
            self.d_prim, self.d_inst, self.prim, _ = case.primary(0)
        self.d_attr = _buf(self.n * 24, 0)
        with limit():
            case.sc.hit_attributes_primary_dev(case.view, self.w, self.h, self.d_prim.data_ptr(), self.d_attr.data_ptr(), d_inst=self.d_inst.data_ptr())
            _torch().cuda.synchronize()
        self.normals = np.ascontiguousarray(self.d_attr.cpu().numpy().view(ATTR_DTYPE)["normal"])
        self._lo = {}

    def lo(self, stride, phase):
        if (stride, phase) not in self._lo:
            values = _sparse(self.case, self.d_prim, self.d_inst, self.light, 4, 0, stride, phase)
            self._lo[(stride, phase)] = (values, _dev(values))
        return self._lo[(stride, phase)]


@pytest.fixture(scope="module")
def frames(trx, cases):
    fr = {}

    def get(name):
        if name not in fr:
            fr[name] = Frame(trx, cases(name).case)
        return fr[name]
    return get


def run_upsample(sc, w, h, stride, phase, d_prim, d_attr, d_lo, radius, base=None, alias=False, tol=TOL, cos=COS, stream=0, what="upsample"):
    """One call: the n floats of d_out.  d_out sits between sentinels, which must stand afterwards; d_in_lo and a separate base
    must be what they were.  base: float32 per pixel or None; alias: it sits in d_out."""
    n = w * h
    before_lo = d_lo.cpu().numpy().copy()
    d_base = _dev(base) if base is not None and not alias else None
    d_out = _guarded(n, base if alias else None)
    p_out = d_out.data_ptr() + GUARD
    _sync()
    with limit():
        sc.value_upsample_dev(w, h, stride, phase, d_prim.data_ptr(), d_lo.data_ptr(), p_out, radius, depth_tol=tol, normal_cos=cos,
                              d_attr=d_attr.data_ptr() if d_attr is not None else 0,
                              d_base=p_out if alias and base is not None else d_base.data_ptr() if d_base is not None else 0, stream=stream)
        _torch().cuda.synchronize()
    got = _inner(d_out, n, what)
    assert (d_lo.cpu().numpy() == before_lo).all(), what + ": d_in_lo was written"
    if d_base is not None:
        assert (d_base.cpu().numpy().view(np.uint32) == base.view(np.uint32)).all(), what + ": d_base was written"
    return got


def _base(n, seed):
    base = np.random.default_rng(seed).uniform(0.0, 1.0, n).astype(np.float32)
    base[::7], base[3::11] = f32(-0.0), f32(1e30)
    return base


@pytest.mark.parametrize("name", SCENES)
def test_upsample_equals_the_twin(trx, frames, name):
    """Every grid, radii 0..2, with and without d_attr; at radius 1 d_base NULL, separate and aliased to d_out; everything
    accepted and nothing but the own cell accepted; a non-null stream."""
    fr = frames(name)
    sc, w, h, n = fr.case.sc, fr.w, fr.h, fr.n
    surf = VT.surface(fr.prim)
    base = _base(n, n)
    st = _torch().cuda.Stream()
    seen = np.zeros(4, dtype=np.int64)
    for k, (stride, phase) in enumerate(GRIDS):
        lo, d_lo = fr.lo(stride, phase)
        if stride == 2 and phase == 0:
            assert (lo > 0).sum() > 20 and np.unique(lo).size > 10, name            # (a noisy term on the low grid)
        stream = st.cuda_stream if k % 2 else 0
        for r in (0, 1, 2):
            for normals, d_attr in ((fr.normals, fr.d_attr), (None, None)):
                what = "%s stride %d phase %d radius %d attr %s" % (name, stride, phase, r, d_attr is not None)
                want, cls = ST.value_upsample(fr.prim, normals, lo, w, h, stride, phase, r, TOL, COS, classes=True)
                _same(run_upsample(sc, w, h, stride, phase, fr.d_prim, d_attr, d_lo, r, stream=stream, what=what), want, what + " no base")
                seen += np.bincount(cls, minlength=4)[:4]
                if r == 1:
                    based = ST.value_upsample(fr.prim, normals, lo, w, h, stride, phase, r, TOL, COS, base=base)
                    _same(run_upsample(sc, w, h, stride, phase, fr.d_prim, d_attr, d_lo, r, base=base, stream=stream, what=what), based, what + " separate base")
                    _same(run_upsample(sc, w, h, stride, phase, fr.d_prim, d_attr, d_lo, r, base=base, alias=True, stream=stream, what=what), based,
                          what + " aliased base")
                    assert (based != want)[surf].any() and (based.view(np.uint32) == base.view(np.uint32))[~surf].all(), what
        if stride in (2, 4) and phase == 0:
            for tol, cos, label in ((INF, -1.0, "all accepted"), (0.0, 2.0, "own cell only")):
                want, cls = ST.value_upsample(fr.prim, fr.normals, lo, w, h, stride, phase, 2, tol, cos, classes=True)
                _same(run_upsample(sc, w, h, stride, phase, fr.d_prim, fr.d_attr, d_lo, 2, tol=tol, cos=cos), want, "%s stride %d %s" % (name, stride, label))
                _, acc, fb, _ = class_counts(cls)
                assert (fb == 0) if tol == INF else (fb > acc), (name, label, acc, fb)
    assert seen[ACCEPTED] > 0 and seen[FALLBACK] > 0 and (name != "soup_52x44" or seen[EMPTY] > 0), (name, seen)
    sc.check()


def _images():
    for w, h in ((33, 9), (70, 37)):
        yield "%dx%d all-surface" % (w, h), w, h, VT.hand_made(w, h, 31 * w + h, misses=False)
        yield "%dx%d with misses" % (w, h), w, h, VT.hand_made(w, h, 17 * w + h, misses=True)
    yield "7x3 with misses", 7, 3, VT.hand_made(7, 3, 17 * 7 + 3, misses=True)
    yield "1x1", 1, 1, VT.hand_made(1, 1, 18, misses=False)
    yield "70x37 of misses", 70, 37, VT.all_misses(70, 37, 6)


@pytest.mark.parametrize("name,w,h,rec", list(_images()), ids=[i[0].replace(" ", "_") for i in _images()])
def test_hand_made_images(trx, frames, name, w, h, rec):
    """The hand-made images of tests/value_filter_twin.py uploaded as records: tile edges at x = 32 and y = 8, halo cells off the
    low grid on every side, a depth step, a crease, misses of both kinds; -0.0f, +inf and NaN among the low plane's values, and a
    NaN in every cell that must not be looked at."""
    sc = frames("cornell_64").case.sc
    prim, nrm, values, base = rec
    attr = np.zeros(w * h, dtype=ATTR_DTYPE)
    attr["normal"] = nrm
    d_prim, d_attr = _dev(prim), _dev(attr)
    surf = VT.surface(prim)
    rng = np.random.default_rng(w)
    with np.errstate(all="ignore"):
        for stride, phase in GRIDS:
            gx, gy, inside = cell_pixels(w, h, stride, phase)
            c_surf = (inside & surf.reshape(h, w)[np.minimum(gy, h - 1), np.minimum(gx, w - 1)]).reshape(-1)
            lo = np.where(c_surf, values.reshape(h, w)[np.minimum(gy, h - 1), np.minimum(gx, w - 1)].reshape(-1), f32(np.nan)).astype(np.float32)
            at = np.flatnonzero(c_surf)
            if at.size > 6:
                pick = rng.choice(at, 3, replace=False)
                lo[pick[0]], lo[pick[1]], lo[pick[2]] = f32(INF), f32(np.nan), f32(-0.0)
            d_lo = _dev(lo)
            for r in (0, 1, 2):
                for normals, da in ((nrm, d_attr), (None, None)):
                    what = "%s stride %d phase %d radius %d attr %s" % (name, stride, phase, r, da is not None)
                    _same(run_upsample(sc, w, h, stride, phase, d_prim, da, d_lo, r, what=what), ST.value_upsample(prim, normals, lo, w, h, stride, phase, r, TOL, COS), what)
                    want = ST.value_upsample(prim, normals, lo, w, h, stride, phase, r, TOL, COS, base=base)
                    _same(run_upsample(sc, w, h, stride, phase, d_prim, da, d_lo, r, base=base, alias=True, what=what), want, what + " aliased base")
                    if "of misses" in name:
                        assert (want.view(np.uint32) == base.view(np.uint32)).all()
    sc.check()


# ---- refusals, scratch, ordering ---------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(trx, cases, frames):
    torch = _torch()
    gi = cases("instanced")
    case = gi.case
    sc, view, w, h = case.sc, case.view, case.w, case.h
    fr = frames("instanced")
    n = w * h
    good = _mixed(1)[0].product(trx)
    d_lo, d_out = _buf(n * 4 + GUARD), _buf(n * 4 + GUARD)
    d_in = _buf(n * 4, 0)

    def pas(stride=2, phase=0, lights=(good,), ns=4, mask=0, seps=EPS, beps=EPS, albedo=0.5, sem=0, inst=fr.d_inst.data_ptr(), w=w):
        sc.trace_indirect_sparse_dev(view, w, h, stride, phase, lights, fr.d_prim.data_ptr(), d_lo.data_ptr(), n_samples=ns, sem=sem, ray_mask=mask,
                                     bounce_eps=beps, shadow_eps=seps, bounce_albedo=albedo, d_primary_inst=inst)

    bad_kind, bad_dir = trx.light(7, (0, 1, 0)), trx.light(trx.LIGHT_DIRECTIONAL, (0, 0, 0))
    for kw, msg in (({"stride": 0}, "stride"), ({"stride": 5}, "stride"), ({"stride": 2, "phase": 4}, "phase"), ({"stride": 1, "phase": 1}, "phase"),
                    ({"stride": 4, "phase": 16}, "phase"), ({"lights": [good] * 9}, "n_lights"), ({"lights": (good, bad_kind)}, "kind"),
                    ({"lights": (bad_dir,)}, "zero length"), ({"ns": 0}, "n_samples"), ({"ns": 65}, "n_samples"), ({"mask": 256}, "ray_mask"),
                    ({"seps": -1.0}, "shadow_eps"), ({"beps": float("nan")}, "bounce_eps"), ({"albedo": float("inf")}, "bounce_albedo"),
                    ({"sem": 8}, "semantics"), ({"inst": 0}, "instance transforms"), ({"w": 0}, "image")):
        with pytest.raises(trx.TrxError, match=msg) as e:
            pas(**kw)
        assert e.value.code == -1, kw

    def up(stride=2, phase=0, r=1, tol=TOL, cos=COS, prim=fr.d_prim.data_ptr(), lo=d_in.data_ptr(), out=d_out.data_ptr(), base=0, w=w):
        sc.value_upsample_dev(w, h, stride, phase, prim, lo, out, r, depth_tol=tol, normal_cos=cos, d_attr=fr.d_attr.data_ptr(), d_base=base)

    for kw, msg in (({"stride": 0}, "stride"), ({"stride": 5}, "stride"), ({"phase": 4}, "phase"), ({"r": 3}, "radius"), ({"tol": -0.1}, "depth_tol"),
                    ({"tol": float("nan")}, "depth_tol"), ({"cos": float("nan")}, "normal_cos"), ({"w": 0}, "image"), ({"prim": 0}, "null"), ({"lo": 0}, "null"),
                    ({"out": 0}, "null"), ({"lo": d_out.data_ptr()}, "d_in_lo is d_out")):
        with pytest.raises(trx.TrxError, match=msg) as e:
            up(**kw)
        assert e.value.code == -1, kw
    for kw, msg in (({"bounce_stride": 5}, "stride"), ({"bounce_stride": 2, "bounce_phase": 4}, "phase"), ({"bounce_stride": 2, "bounce_upsample_radius": 3}, "radius"),
                    ({"bounce_stride": 2, "bounce_filter_levels": 6}, "bounce_filter_levels"), ({"bounce_stride": 2, "bounce_depth_tol": -1.0}, "depth_tol")):
        with pytest.raises(trx.TrxError, match=msg):
            sc.render_image_gi_sparse(view, w, h, (good,), 4, **kw)
    with pytest.raises(trx.TrxError, match="bounce_samples"):
        sc.render_image_gi_sparse(view, w, h, (good,), 0, 2)
    _sync()
    for t in (d_lo, d_out):
        assert (t.cpu().numpy() == FILL).all()
    with limit():
        pas()   # and the scene is still usable
        up(lo=d_lo.data_ptr())
        torch.cuda.synchronize()
    wlo, hlo = lo_size(w, h, 2)
    got = d_lo.cpu().numpy()
    assert (got[:wlo * hlo * 4] != FILL).any() and (got[wlo * hlo * 4:] == FILL).all()
    assert (d_out.cpu().numpy()[n * 4:] == FILL).all()
    sc.check()


def test_device_bytes_count_the_scratch_once(trx, orc):
    """The pass's scratch is the dense pass's, counted when it is made, once: a second identical call, other phases and a smaller
    grid add nothing, and the upsample owns no device memory."""
    torch = _torch()
    case = Case(trx, orc, "cornell_64")
    try:
        with limit():
            d_prim, d_inst, _, _ = case.primary(0)
        n, stride = 4, 2
        wlo, hlo = lo_size(case.w, case.h, stride)
        tiles = ((wlo + 7) // 8) * ((hlo + 7) // 8)
        # the rays launch of this size first, on the same stream: the launch slot's stack spill area is then sized for it
        d_rays = torch.zeros((tiles * n * 64 * 32,), dtype=torch.uint8, device="cuda")
        d_flags = torch.zeros((tiles * n * 64,), dtype=torch.uint8, device="cuda")
        with limit():
            case.sc.trace_occluded_dev(d_rays.data_ptr(), tiles * n * 64, d_flags.data_ptr())
            torch.cuda.synchronize()
        before = case.sc.device_bytes
        lo = _sparse(case, d_prim, d_inst, _mixed(3), n, 0, stride, 0)
        first = case.sc.device_bytes
        # per ray 32 + 1 (shadow ray, flag) + 32 + 8 + 4 + 24 + 4 (bounce ray, hit, instance id, attributes, sum); per pixel 4
        assert first - before == tiles * n * 64 * 105 + tiles * 64 * 4
        again = _sparse(case, d_prim, d_inst, _mixed(3), n, 0, stride, 0)
        assert case.sc.device_bytes == first and (again.view(np.uint32) == lo.view(np.uint32)).all()
        _sparse(case, d_prim, d_inst, _mixed(1), n, 3, stride, 3)
        _sparse(case, d_prim, d_inst, _mixed(3), n, 0, 4, 15)
        d_lo, d_out = _dev(lo), _buf(case.w * case.h * 4)
        with limit():
            case.sc.value_upsample_dev(case.w, case.h, stride, 0, d_prim.data_ptr(), d_lo.data_ptr(), d_out.data_ptr(), 2)
            torch.cuda.synchronize()
        assert case.sc.device_bytes == first
    finally:
        case.close()


def test_sparse_chain_keeps_its_place_before_a_refit(trx):
    """The sparse pass and the upsample of its values enqueued on a busy stream, then at once a refit: the refit waits for every
    launch of both, the values are the old geometry's."""
    torch = _torch()
    from tray_racing_amd import _lib
    g = np.load(os.path.join(GOLDEN, "soup_52x44.npz"))
    n_tris = g["tri_verts"].shape[0]
    flat = trx.FlatScene(g["nodes"], g["tri_verts"], g["instance_offsets"], int(g["tlas_start"]), np.arange(n_tris), [0, n_tris])
    view = _lib.View()
    C.memmove(C.byref(view), g["view"].tobytes(), C.sizeof(view))
    w, h = int(g["width"]), int(g["height"])
    n = w * h
    sc = trx.Scene(flat)
    v = flat.tri_verts
    size = float(np.linalg.norm(v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0)))
    moved = (v + np.random.default_rng(71).normal(scale=2e-2 * size, size=v.shape)).astype(np.float32)
    lights = [LT.Light(LT.POINT, LT.POINT_CASES["soup_52x44"]), LT.Light(LT.RECT, (-0.2, 0.9, -0.2), (0.4, 0.0, 0.0), (0.0, 0.0, 0.4))]
    products = [l.product(trx) for l in lights]
    d_prim, d_attr = _buf(n * 8), _buf(n * 24, 0)

    def chain(stream=0):
        d_lo, d_out = _buf(n * 4), _buf(n * 4)
        sc.trace_indirect_sparse_dev(view, w, h, 2, 1, products, d_prim.data_ptr(), d_lo.data_ptr(), n_samples=8, bounce_eps=EPS, shadow_eps=EPS, stream=stream)
        sc.value_upsample_dev(w, h, 2, 1, d_prim.data_ptr(), d_lo.data_ptr(), d_out.data_ptr(), 1, depth_tol=TOL, normal_cos=COS, d_attr=d_attr.data_ptr(),
                              stream=stream)
        return d_out, d_lo

    try:
        with limit():
            sc.trace_primary_dev(view, w, h, d_prim.data_ptr())
            sc.hit_attributes_primary_dev(view, w, h, d_prim.data_ptr(), d_attr.data_ptr())
            old, _ = chain()
            torch.cuda.synchronize()
        old = old.cpu().numpy()
        s = torch.cuda.Stream()
        big = random_rays(trx, flat, 2 * 1024 * 1024, 72, zero_dirs=False)
        d_big, d_bh = _dev(big), _buf(big.shape[0] * 8)
        _sync()
        with limit():
            with torch.cuda.stream(s):
                sc.trace_rays_dev(d_big.data_ptr(), big.shape[0], d_bh.data_ptr(), stream=s.cuda_stream)
                got, keep = chain(stream=s.cuda_stream)
            sc.refit(moved)
            s.synchronize()
        assert (got.cpu().numpy() == old).all(), "the chain saw the refit's geometry"
        with limit():
            new, _ = chain()      # (the same primary records: the bounce and shadow rays now meet the moved triangles)
            torch.cuda.synchronize()
        assert (new.cpu().numpy() != old).sum() > 20, "the refit changed nothing"
        sc.check()
    finally:
        sc.close()


# ---- the host form -----------------------------------------------------------------------------------------------------------

def _lit_chain(sc, case, products, n, sem, mask, ao, d):
    """The lit chain up to the light term V (d["val"]), call by call."""
    from tray_racing_amd import _lib as L
    view, w, h = case.view, case.w, case.h
    L.check(sc._lib.trx_trace_primary_inst_dev(sc.handle, C.byref(view), w, h, L.Shard(0, 1, 0, 0), sem, C.c_void_p(d["prim"].data_ptr()),
                                               C.c_void_p(d["inst"].data_ptr()), None))
    sc.hit_attributes_primary_dev(view, w, h, d["prim"].data_ptr(), d["attr"].data_ptr(), d_inst=d["inst"].data_ptr())
    sc.trace_light_visibility_dev(view, w, h, products, d["prim"].data_ptr(), d["lit"].data_ptr(), n_samples=n, sem=sem, ray_mask=mask, frame0=2,
                                  shadow_eps=EPS, d_primary_inst=d["inst"].data_ptr())
    if ao:
        sc.trace_ao_visibility_dev(view, w, h, d["prim"].data_ptr(), d["cnt"].data_ptr(), ao, case.radius, sem=sem, frame0=2, ao_eps=EPS,
                                   d_primary_inst=d["inst"].data_ptr())
        sc.ao_filter_dev(w, h, d["prim"].data_ptr(), d["cnt"].data_ptr(), d["term"].data_ptr(), ao, 1, d_attr=d["attr"].data_ptr())
    sc.light_term_dev(view, w, h, products, d["prim"].data_ptr(), d["attr"].data_ptr(), d["lit"].data_ptr(), d["val"].data_ptr(), n_samples=n,
                      ambient=0.3, d_term=d["term"].data_ptr() if ao else 0)


@pytest.mark.parametrize("ao,mask,levels,stride,phase,radius", [(0, 0, 3, 2, 0, 1), (4, 0x0E, 0, 3, 8, 2), (0, 0, 1, 4, 5, 0), (0, 0, 0, 1, 0, 0)])
def test_host_form_is_its_composition(trx, cases, ao, mask, levels, stride, phase, radius):
    """trx_render_image_gi_sparse against the device-resident calls it is made of, on cornell_tlas_48 (with a mask table set) and
    on the transformed scene, with and without filter levels.  At stride 1, radius 0 and no levels its bytes are
    trx_render_image_gi's, and the composition's float plane equals the dense composition's as values (0.0f + x is not x for
    x = -0.0f)."""
    torch = _torch()
    for name in ("cornell_tlas_48", "instanced"):
        case = cases(name).case
        sc, view, w, h = case.sc, case.view, case.w, case.h
        n_px = w * h
        lights, n, sem, bn = _mixed(3), 4, 3, 3
        products = [l.product(trx) for l in lights]
        kw = dict(bounce_eps=EPS, bounce_albedo=0.6, sem=sem, ray_mask=mask, frame0=2, light_samples=n, shadow_eps=EPS, ambient=0.3, ao_samples=ao,
                  ao_eps=EPS, ao_radius=case.radius, filter_radius=1)
        masks = np.full(case.osc.inst.size, 0xFF, dtype=np.uint8)
        masks[LT.MASK_HIDES] = 0x11
        sc.set_instance_masks(masks)
        try:
            with limit():
                img, ms = sc.render_image_gi_sparse(view, w, h, products, bn, stride, bounce_phase=phase, bounce_upsample_radius=radius,
                                                    bounce_filter_levels=levels, bounce_depth_tol=TOL, bounce_normal_cos=COS, **kw)
                gi, _ = sc.render_image_gi(view, w, h, products, bn, **kw)
            d = dict(prim=_buf(n_px * 8, 0xEE), inst=_buf(n_px * 4, 0xFF), attr=_buf(n_px * 24, 0), lit=_buf(len(lights) * n_px), cnt=_buf(n_px),
                     term=_buf(n_px * 4), val=_buf(n_px * 4))
            wlo, hlo = lo_size(w, h, stride)
            d_lo, d_ind, d_work, d_rgba = _buf(wlo * hlo * 4), _buf(n_px * 4), _buf(n_px * 4), _buf(n_px * 4)
            with limit():
                _lit_chain(sc, case, products, n, sem, mask, ao, d)
                sc.trace_indirect_sparse_dev(view, w, h, stride, phase, products, d["prim"].data_ptr(), d_lo.data_ptr(), n_samples=bn, sem=sem,
                                             ray_mask=mask, frame0=2, bounce_eps=EPS, shadow_eps=EPS, bounce_albedo=0.6, d_primary_inst=d["inst"].data_ptr())
                if levels == 0:
                    sc.value_upsample_dev(w, h, stride, phase, d["prim"].data_ptr(), d_lo.data_ptr(), d["val"].data_ptr(), radius, depth_tol=TOL,
                                          normal_cos=COS, d_attr=d["attr"].data_ptr(), d_base=d["val"].data_ptr())
                else:
                    sc.value_upsample_dev(w, h, stride, phase, d["prim"].data_ptr(), d_lo.data_ptr(), d_ind.data_ptr(), radius, depth_tol=TOL,
                                          normal_cos=COS, d_attr=d["attr"].data_ptr())
                    sc.value_filter_dev(w, h, d["prim"].data_ptr(), d_ind.data_ptr(), d["val"].data_ptr(), levels, depth_tol=TOL, normal_cos=COS,
                                        d_attr=d["attr"].data_ptr(), d_base=d["val"].data_ptr(), d_work=d_work.data_ptr())
                sc.shade_value_dev(d["val"].data_ptr(), n_px, d_rgba.data_ptr())
                torch.cuda.synchronize()
            want = d_rgba.cpu().numpy().reshape(h, w, 4)
            what = (name, ao, mask, levels, stride, phase, radius)
            assert ms > 0 and (img == want).all(), (what, (img != want).sum())
            assert (img[..., 3] == 255).all()
            if stride == 1 and radius == 0 and levels == 0:
                assert (img == gi).all(), (what, (img != gi).sum())
                values = d["val"].cpu().numpy().view(np.float32).copy()
                with limit():
                    _lit_chain(sc, case, products, n, sem, mask, ao, d)
                    sc.trace_indirect_dev(view, w, h, products, d["prim"].data_ptr(), d["val"].data_ptr(), n_samples=bn, sem=sem, ray_mask=mask, frame0=2,
                                          bounce_eps=EPS, shadow_eps=EPS, bounce_albedo=0.6, d_primary_inst=d["inst"].data_ptr(), d_base=d["val"].data_ptr())
                    torch.cuda.synchronize()
                dense = d["val"].cpu().numpy().view(np.float32)
                assert (values == dense).all() and not np.isnan(dense).any(), what
            else:
                assert (img[..., 0] != gi[..., 0]).mean() > 0.02, what                 # (the sparse term is another image)
            sc.check()
        finally:
            sc.set_instance_masks(None)
