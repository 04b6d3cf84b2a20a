"""The value filter on the GPU, bit for bit (include/trx.h, "the value filter"): trx_value_filter_dev writes the twin's values
(tests/value_filter_twin.py) - fed the device's own primary records, attribute records and indirect term - on single-level,
two-level and transformed scenes, for 1..5 levels, with and without normals, with no base, a base of its own and a base in
d_out, sentinels on either side of d_out and d_work; the hand-made images of tests/test_value_filter.py uploaded as records;
one-level calls chained through the API; refusals; the ordering with a refit; the host form against its composition.  NaN-ness
is compared, not a NaN's payload.  No pixel is left out of any comparison.

Every step that runs on the GPU sits under a time limit of its own (`limit`): a step that hangs ends the process."""
import ctypes as C
import os

import numpy as np
import pytest

import light_twin as LT
import value_filter_twin as VT
from helpers import random_rays
from hit_attr_twin import ATTR_DTYPE
from test_gpu_ao_visibility import make_case
from test_gpu_light import EPS, FILL, _buf, _dev, _mixed, _sync, _torch, limit

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL, COS = 0.10, 0.9      # (tests/test_value_filter.py: under this pair the golden cases reject and accept taps at every level)
GUARD = 64                # sentinel bytes on either side of d_out and d_work
f32 = np.float32


class Frame:
    """A case's frame on the device and on the host: primary records, attribute records and the 4-sample indirect term of a
    point light without a base - the filter's inputs as the device made them."""

    def __init__(self, trx, case):
        torch = _torch()
        self.case, self.w, self.h = case, case.w, case.h
        n = self.n = case.w * case.h
        light = LT.Light(LT.POINT, LT.POINT_CASES.get(case.name, (0.0, 1.8, 0.0)), intensity=1.5)
        with limit():
            self.d_prim, self.d_inst, self.prim, _ = case.primary(0)
        self.d_attr, self.d_in = _buf(n * 24, 0), _buf(n * 4)
        with limit():
            case.sc.hit_attributes_primary_dev(case.view, self.w, self.h, self.d_prim.data_ptr(), self.d_attr.data_ptr(), d_inst=self.d_inst.data_ptr())
            case.sc.trace_indirect_dev(case.view, self.w, self.h, [light.product(trx)], self.d_prim.data_ptr(), self.d_in.data_ptr(), n_samples=4,
                                       bounce_eps=EPS, shadow_eps=EPS, bounce_albedo=0.5, d_primary_inst=self.d_inst.data_ptr())
            torch.cuda.synchronize()
            case.sc.check()
        self.normals = np.ascontiguousarray(self.d_attr.cpu().numpy().view(ATTR_DTYPE)["normal"])
        self.values = self.d_in.cpu().numpy().view(np.float32).copy()


def run_filter(sc, w, h, d_prim, d_attr, d_in, levels, base=None, alias=False, tol=TOL, cos=COS, stream=0, work=True):
    """One call: (the n floats of d_out).  d_out and d_work sit between sentinels, which must stand afterwards, and d_in must be
    what it was.  base: float32 per pixel or None; alias: it sits in d_out."""
    n = w * h
    before_in = d_in.cpu().numpy().copy()
    out0 = np.full(n * 4 + 2 * GUARD, FILL, dtype=np.uint8)
    d_base = None
    if base is not None and alias:
        out0[GUARD:GUARD + n * 4] = base.view(np.uint8)
    elif base is not None:
        d_base = _dev(base)
    d_out, d_work = _dev(out0), _buf(n * 4 + 2 * GUARD)
    p_out = d_out.data_ptr() + GUARD
    _sync()
    with limit():
        sc.value_filter_dev(w, h, d_prim.data_ptr(), d_in.data_ptr(), p_out, levels, depth_tol=tol, normal_cos=cos,
                            d_attr=d_attr.data_ptr() if d_attr is not None else 0,
                            d_base=p_out if alias and base is not None else d_base.data_ptr() if d_base is not None else 0,
                            d_work=d_work.data_ptr() + GUARD if work else 0, stream=stream)
        _torch().cuda.synchronize()
    got, wk = d_out.cpu().numpy(), d_work.cpu().numpy()
    for name, b in (("d_out", got), ("d_work", wk)):
        assert (b[:GUARD] == FILL).all() and (b[GUARD + n * 4:] == FILL).all(), "%s: a sentinel was written" % name
    assert (d_in.cpu().numpy() == before_in).all(), "d_in was written"
    if d_base is not None:
        assert (d_base.cpu().numpy().view(np.uint32) == base.view(np.uint32)).all(), "d_base was written"
    return got[GUARD:GUARD + n * 4].view(np.float32).copy()


def _same(got, want, what):
    bad = VT.same_bits(got, want)
    assert bad.size == 0, "%s: %d of %d values differ, first at %s: %s != %s" % (what, bad.size, got.size, bad[:4], got[bad[:4]], want[bad[:4]])


@pytest.fixture(scope="module")
def frames(trx, orc):
    made, fr = {}, {}

    def get(name):
        case = make_case(trx, orc, made, name)
        if name not in fr:
            fr[name] = Frame(trx, case)
        return fr[name]
    yield get
    for c in made.values():
        c.close()


def _base(n, seed):
    base = np.random.default_rng(seed).uniform(0.0, 1.0, n).astype(np.float32)
    base[::7], base[3::11] = f32(-0.0), f32(1e30)
    return base


# ---- the pass against the twin --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell_64", "soup_52x44", "cornell_tlas_48", "instanced"])
def test_values_equal_the_twin(trx, frames, name):
    """Levels 1..5, each with and without d_attr, each with d_base NULL, separate and aliased to d_out."""
    fr = frames(name)
    sc, w, h, n = fr.case.sc, fr.w, fr.h, fr.n
    surf = VT.surface(fr.prim)
    assert surf.sum() > 500 and (fr.values[surf] > 0).mean() > 0.1 and (fr.values[~surf] == 0).all()     # (a frame, and a noisy term on it)
    base = _base(n, n)
    st = _torch().cuda.Stream()
    for with_attr in (True, False):
        normals, d_attr = (fr.normals, fr.d_attr) if with_attr else (None, None)
        for levels in range(1, VT.MAX_LEVELS + 1):
            plain = VT.value_filter(fr.prim, normals, fr.values, w, h, levels, TOL, COS)
            based = VT.value_filter(fr.prim, normals, fr.values, w, h, levels, TOL, COS, base=base)
            what = "%s %d levels attr %s" % (name, levels, with_attr)
            stream = st.cuda_stream if levels & 1 else 0
            _same(run_filter(sc, w, h, fr.d_prim, d_attr, fr.d_in, levels, stream=stream), plain, what + " no base")
            _same(run_filter(sc, w, h, fr.d_prim, d_attr, fr.d_in, levels, base=base, stream=stream), based, what + " separate base")
            _same(run_filter(sc, w, h, fr.d_prim, d_attr, fr.d_in, levels, base=base, alias=True, stream=stream), based, what + " aliased base")
            # (not the input handed through, and the base counts; how many taps are accepted and rejected: tests/test_value_filter.py)
            assert (plain != fr.values)[surf].mean() > 0.1 and (based != plain)[surf].any(), what
        if with_attr:
            without = VT.value_filter(fr.prim, None, fr.values, w, h, 3, TOL, COS)
            assert (VT.value_filter(fr.prim, fr.normals, fr.values, w, h, 3, TOL, COS) != without)[surf].mean() > 0.01, name   # (so do the normals)
    # one level needs no d_work
    _same(run_filter(sc, w, h, fr.d_prim, fr.d_attr, fr.d_in, 1, work=False), VT.value_filter(fr.prim, fr.normals, fr.values, w, h, 1, TOL, COS), name + " no d_work")
    # other tolerances: everything accepted, nothing but the pixel itself accepted
    _same(run_filter(sc, w, h, fr.d_prim, fr.d_attr, fr.d_in, 2, tol=float("inf"), cos=-1.0), VT.value_filter(fr.prim, fr.normals, fr.values, w, h, 2, float("inf"), -1.0),
          name + " all accepted")
    own = run_filter(sc, w, h, fr.d_prim, fr.d_attr, fr.d_in, 2, tol=0.0, cos=2.0)
    _same(own, VT.value_filter(fr.prim, fr.normals, fr.values, w, h, 2, 0.0, 2.0), name + " none accepted")
    sc.check()


def _images():
    for w, h in VT.HAND_SIZES:
        yield "%dx%d all-surface" % (w, h), w, h, VT.hand_made(w, h, 31 * w + h, misses=False)
        yield "%dx%d with misses" % (w, h), w, h, VT.hand_made(w, h, 17 * w + h, misses=True)
    yield "7x3 of misses", 7, 3, VT.all_misses(7, 3, 5)
    yield "70x37 of misses", 70, 37, VT.all_misses(70, 37, 6)


@pytest.mark.parametrize("name,w,h,rec", list(_images()), ids=[i[0].replace(" ", "_") for i in _images()])
def test_hand_made_images(trx, frames, name, w, h, rec):
    """The hand-made images of tests/test_value_filter.py as records: taps leave the image at every level, row classes without
    a row (33x9 at spacing 16), a depth step, a crease, misses of both kinds, -0.0f, +inf and NaN among the values."""
    sc = frames("cornell_64").case.sc
    prim, nrm, values, base = rec
    attr = np.zeros(w * h, dtype=ATTR_DTYPE)
    attr["normal"] = nrm
    d_prim, d_attr, d_in = _dev(prim), _dev(attr), _dev(values)
    with np.errstate(all="ignore"):
        for levels in range(1, VT.MAX_LEVELS + 1):
            for normals, da in ((nrm, d_attr), (None, None)):
                what = "%s %d levels attr %s" % (name, levels, da is not None)
                _same(run_filter(sc, w, h, d_prim, da, d_in, levels), VT.value_filter(prim, normals, values, w, h, levels, TOL, COS), what)
                want = VT.value_filter(prim, normals, values, w, h, levels, TOL, COS, base=base)
                _same(run_filter(sc, w, h, d_prim, da, d_in, levels, base=base, alias=True), want, what + " aliased base")
                if "of misses" in name:
                    assert (want.view(np.uint32) == base.view(np.uint32)).all()
    sc.check()


def test_one_level_calls_chained_through_the_api(trx, frames):
    """The prototype names no first level, so a one-level call is always level 0: three of them chained - each call's d_out the
    next one's d_in, the base added by the last - are the twin's level 0 applied three times, and differ from a 3-level call."""
    fr = frames("soup_52x44")
    sc, w, h, n = fr.case.sc, fr.w, fr.h, fr.n
    base = _base(n, 3)
    u, d_u = fr.values, fr.d_in
    for k in range(3):
        got = run_filter(sc, w, h, fr.d_prim, fr.d_attr, d_u, 1, base=base if k == 2 else None, work=False)
        u = VT.level(fr.prim, fr.normals, u, w, h, 0, TOL, COS)
        want = u if k < 2 else VT.value_filter(fr.prim, fr.normals, u, w, h, 0, TOL, COS, base=base)
        _same(got, want, "chained call %d" % k)
        d_u = _dev(got)
    three = VT.value_filter(fr.prim, fr.normals, fr.values, w, h, 3, TOL, COS, base=base)
    assert VT.same_bits(got, three).size > n // 10


# ---- refusals, ordering ------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_output_untouched(trx, frames):
    fr = frames("cornell_64")
    sc, w, h, n = fr.case.sc, fr.w, fr.h, fr.n
    d_out, d_work = _buf(n * 4 + GUARD), _buf(n * 4 + GUARD)

    def call(levels=3, tol=TOL, cos=COS, d_in=fr.d_in.data_ptr(), prim=fr.d_prim.data_ptr(), work=d_work.data_ptr(), out=d_out.data_ptr(), base=0, w=w, h=h):
        sc.value_filter_dev(w, h, prim, d_in, out, levels, depth_tol=tol, normal_cos=cos, d_attr=fr.d_attr.data_ptr(), d_base=base, d_work=work)

    for kw, msg in (({"levels": 0}, "n_levels"), ({"levels": 6}, "n_levels"), ({"tol": -0.1}, "depth_tol"), ({"tol": float("nan")}, "depth_tol"),
                    ({"cos": float("nan")}, "normal_cos"), ({"w": 0}, "image"), ({"prim": 0}, "null"), ({"d_in": 0}, "null"), ({"out": 0}, "null"),
                    ({"work": 0, "levels": 2}, "d_work"), ({"d_in": d_out.data_ptr()}, "d_in is d_out"), ({"work": d_out.data_ptr()}, "d_work is"),
                    ({"work": fr.d_in.data_ptr()}, "d_work is"), ({"work": d_work.data_ptr(), "base": d_work.data_ptr()}, "d_work is")):
        with pytest.raises(trx.TrxError, match=msg) as e:
            call(**kw)
        assert e.value.code == -1, kw
    good = _mixed(1)[0].product(trx)
    with pytest.raises(trx.TrxError, match="bounce_filter_levels"):
        sc.render_image_gi_filtered(fr.case.view, w, h, (good,), 4, 6)
    with pytest.raises(trx.TrxError, match="depth_tol"):
        sc.render_image_gi_filtered(fr.case.view, w, h, (good,), 4, 3, bounce_depth_tol=-1.0)
    with pytest.raises(trx.TrxError, match="bounce_samples"):
        sc.render_image_gi_filtered(fr.case.view, w, h, (good,), 0, 3)
    _sync()
    for t in (d_out, d_work):
        assert (t.cpu().numpy() == FILL).all()
    with limit():
        call()      # and the scene is still usable
        _torch().cuda.synchronize()
    got = d_out.cpu().numpy()
    _same(got[:n * 4].view(np.float32), VT.value_filter(fr.prim, fr.normals, fr.values, w, h, 3, TOL, COS), "after the refusals")
    assert (got[n * 4:] == FILL).all() and (d_work.cpu().numpy()[n * 4:] == FILL).all()


def test_device_bytes_count_the_slots_plane_once(trx, frames):
    """Only a call with its base in d_out and three levels or more needs a plane of the library's: counted when it is made, once."""
    fr = frames("cornell_tlas_48")
    sc, w, h, n = fr.case.sc, fr.w, fr.h, fr.n
    base = _base(n, 1)
    st = _torch().cuda.Stream()      # (a stream of its own: a launch slot no other test of this module has used)
    run_filter(sc, w, h, fr.d_prim, fr.d_attr, fr.d_in, 5, base=base, stream=st.cuda_stream)
    run_filter(sc, w, h, fr.d_prim, fr.d_attr, fr.d_in, 2, base=base, alias=True, stream=st.cuda_stream)
    before = sc.device_bytes
    run_filter(sc, w, h, fr.d_prim, fr.d_attr, fr.d_in, 3, base=base, alias=True, stream=st.cuda_stream)
    assert sc.device_bytes - before == n * 4
    run_filter(sc, w, h, fr.d_prim, fr.d_attr, fr.d_in, 5, base=base, alias=True, stream=st.cuda_stream)
    assert sc.device_bytes - before == n * 4


def test_filter_chain_keeps_its_place_before_a_refit(trx):
    """The indirect pass and the filter over its term enqueued on a busy stream, then at once a refit: the refit waits for every
    launch of both, the filtered values are the old geometry's."""
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
    products = [LT.Light(LT.POINT, LT.POINT_CASES["soup_52x44"]).product(trx)]
    d_prim, d_attr = _buf(n * 8), _buf(n * 24, 0)

    def chain(stream=0):
        d_val, d_work, d_out = _buf(n * 4), _buf(n * 4), _buf(n * 4)
        sc.trace_indirect_dev(view, w, h, products, d_prim.data_ptr(), d_val.data_ptr(), n_samples=4, bounce_eps=EPS, shadow_eps=EPS, stream=stream)
        sc.value_filter_dev(w, h, d_prim.data_ptr(), d_val.data_ptr(), d_out.data_ptr(), 4, depth_tol=TOL, normal_cos=COS, d_attr=d_attr.data_ptr(),
                            d_work=d_work.data_ptr(), stream=stream)
        return d_out, (d_val, d_work)

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
            new, _ = chain()      # (the same primary records: the bounce rays now meet the moved triangles)
            torch.cuda.synchronize()
        assert (new.cpu().numpy() != old).sum() > 20, "the refit changed nothing"
        sc.check()
    finally:
        sc.close()


# ---- the host form -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ao,mask,levels", [(0, 0, 3), (4, 0x0E, 5), (0, 0, 1)])
def test_host_form_is_its_composition(trx, frames, ao, mask, levels):
    """trx_render_image_gi_filtered against the device-resident calls it is made of, on cornell_tlas_48 and on the transformed
    scene; at level 0 it is trx_render_image_gi byte for byte; and the filter changes the image."""
    torch = _torch()
    from tray_racing_amd import _lib as L
    for name in ("cornell_tlas_48", "instanced"):
        case = frames(name).case
        sc, view, w, h = case.sc, case.view, case.w, case.h
        n_px = w * h
        lights, n, sem, bn = _mixed(3), 4, 3, 3
        products = [l.product(trx) for l in lights]
        kw = dict(bounce_eps=EPS, bounce_albedo=0.6, sem=sem, ray_mask=mask, frame0=2, light_samples=n, shadow_eps=EPS, ambient=0.3, ao_samples=ao,
                  ao_eps=EPS, ao_radius=case.radius, filter_radius=1)
        with limit():
            img, ms = sc.render_image_gi_filtered(view, w, h, products, bn, levels, bounce_depth_tol=TOL, bounce_normal_cos=COS, **kw)
            zero, _ = sc.render_image_gi_filtered(view, w, h, products, bn, 0, bounce_depth_tol=float("nan"), bounce_normal_cos=float("nan"), **kw)
            gi, _ = sc.render_image_gi(view, w, h, products, bn, **kw)
        assert (zero == gi).all(), name
        d_prim, d_inst, d_attr, d_lit = _buf(n_px * 8, 0xEE), _buf(n_px * 4, 0xFF), _buf(n_px * 24, 0), _buf(len(lights) * n_px)
        d_cnt, d_term, d_val, d_ind, d_work, d_rgba = _buf(n_px), _buf(n_px * 4), _buf(n_px * 4), _buf(n_px * 4), _buf(n_px * 4), _buf(n_px * 4)
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
            sc.trace_indirect_dev(view, w, h, products, d_prim.data_ptr(), d_ind.data_ptr(), n_samples=bn, sem=sem, ray_mask=mask, frame0=2,
                                  bounce_eps=EPS, shadow_eps=EPS, bounce_albedo=0.6, d_primary_inst=d_inst.data_ptr())
            sc.value_filter_dev(w, h, d_prim.data_ptr(), d_ind.data_ptr(), d_val.data_ptr(), levels, depth_tol=TOL, normal_cos=COS,
                                d_attr=d_attr.data_ptr(), d_base=d_val.data_ptr(), d_work=d_work.data_ptr())
            sc.shade_value_dev(d_val.data_ptr(), n_px, d_rgba.data_ptr())
            torch.cuda.synchronize()
        want = d_rgba.cpu().numpy().reshape(h, w, 4)
        assert ms > 0 and (img == want).all(), (name, ao, mask, levels, (img != want).sum())
        assert (img[..., 3] == 255).all() and (img[..., 0] != gi[..., 0]).mean() > 0.05, name
        sc.check()
