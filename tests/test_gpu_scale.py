"""Power-of-two scene scaling on the GPU (tests/scale_cases.py is the construction, tests/test_scale.py its CPU check).

For every exponent of SAFE and EDGE, every case and both layouts, each post-walk kernel is fed caller records - the k = 0
records, t times 2^k, prim and instance ids in the rebuilt tree's numbering - and its whole output compared twice:
  * with the twin at that k (the project's usual standard), and
  * for SAFE, with the device's OWN k = 0 output under scale_cases.expect_from_base.  No twin takes part in that one: a
    rule the twin and the kernel misread alike (an absolute epsilon, a clamp) breaks it.
The kernels: trx_hit_attributes_primary_dev and _rays_dev; trx_ao_rays_dev, trx_light_rays_dev (three kinds, samples 0 and 7),
trx_bounce_light_rays_dev, trx_emitter_rays_dev, trx_scene_build_emitters / trx_scene_get_emitters, trx_debug_emitter_select,
trx_light_term_dev; trx_ao_filter_dev, trx_ao_upsample_dev, trx_value_filter_dev (3 levels), trx_value_upsample_dev over the
scaled t and the attribute pass's own normals at that k.  At the EDGE exponents that is where denormal and overflowing
dot(ng, ng), NaN and all-zero normals, +inf distance squares and denormal t meet the kernels' sqrtf and divisions.
WALKED: the whole passes with their walks, fed the device's own primary records, against the twins on the oracle at the same
k; the primary records themselves are the k = 0 records under the table.
The three scalings of tests/adversarial_scenes.py that are no powers of two run as plain device-versus-twin cases.

The comparison is scale_cases.differing: bit for bit, NaN-ness compared and not the payload.  Every byte of every output is
compared, with guard bytes either side; no record is left out, nothing is skipped for being non-finite.

Every step that runs on the GPU sits under a time limit of its own (`limit`): a step that hangs ends the process."""
import ctypes as C
import types

import numpy as np
import pytest

import emitter_twin as ET
import light_twin as LT
import material_twin as MT
import scale_cases as SC
import scale_twin as ST
from ao_visibility_twin import record_map, visibility_counts
from hit_attr_twin import ATTR_DTYPE, tri_records
from image_twin import TERM_DTYPE
from test_gpu_light import FILL, _dev, _sync, _torch, limit

pytestmark = pytest.mark.gpu
GUARD = 64
IDS = ["%s_%dx%d" % c for c in SC.CASES]
LAYOUTS = ((0, 1, 0), (0, 1, 1))


# ---- buffers: FILL everywhere, GUARD bytes either side of the output -----------------------------------------------------------

class Out:
    """An output buffer of `planes` planes of `size` records of `rec_bytes` bytes, between two guards."""

    def __init__(self, rec_bytes, size, planes=1):
        self.rec_bytes, self.size, self.planes = rec_bytes, size, planes
        self.t = _torch().full((2 * GUARD + planes * size * rec_bytes,), FILL, dtype=_torch().uint8, device="cuda")
        self.ptr = self.t.data_ptr() + GUARD

    def taken(self, pix, rec, n, what):
        """[planes, n, rec_bytes] in pixel order; the guards and every record the launch does not own must hold FILL."""
        raw = self.t.cpu().numpy()
        assert (raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all(), what + ": a guard byte was written"
        body = raw[GUARD:-GUARD].reshape(self.planes, self.size, self.rec_bytes)
        other = np.ones(self.size, dtype=bool)
        other[rec] = False
        assert (body[:, other] == FILL).all(), what + ": a record outside the image was written"
        out = np.zeros((self.planes, n, self.rec_bytes), dtype=np.uint8)
        out[:, pix] = body[:, rec]
        return out


def _laid_host(a, rec_bytes, pix, rec, size):
    """Pixel-order records in the layout (pix, rec, size); 0xEE in the records outside the image."""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1, rec_bytes)
    buf = np.full((size, rec_bytes), 0xEE, dtype=np.uint8)
    buf[rec] = a[pix]
    return buf


def _laid(a, rec_bytes, pix, rec, size):
    return _dev(_laid_host(a, rec_bytes, pix, rec, size))


def _attr_of(raw, what):
    a = np.ascontiguousarray(raw).view(ATTR_DTYPE).reshape(-1)
    assert (a["_pad"] == 0).all(), what + ": the pad word"
    return ST.attr_of(a)


class Tree:
    """A tree of tests/scale_cases.py on the device: the scene, its materials and its emitter table."""

    def __init__(self, trx, s):
        self.s, self.sc = s, trx.Scene(s.flat)
        self.sc.set_materials(s.mats, s.idx)
        with limit():
            self.n_emitters = self.sc.build_emitters()
        self.w2o = self.sc.instance_world_to_object() if s.tlas else None

    def close(self):
        self.sc.close()


def device_outputs(trx, tree, p, f, shard, images):
    """Every post-walk output of the device over frame `f`, in the layout of scale_twin.twin_outputs; `images`: the image
    kernels too (whole-image, image-layout records only)."""
    s, sc = tree.s, tree.sc
    w, h, view, n = s.w, s.h, s.view, s.w * s.h
    pix, rec, size = record_map(w, h, shard)
    assert pix.size == n
    sh = (*shard, 0)
    syn = ST.synthetic(s, f.prim)
    d_prim, d_inst = _laid(f.prim, 8, pix, rec, size), _laid(f.inst, 4, pix, rec, size)
    P, I = d_prim.data_ptr(), d_inst.data_ptr()
    what = "%s k %d shard %s" % (s.name, s.k, shard)
    lights = [l.product(trx) for l in p.lights]
    outs, rays, keep = {}, {}, []                            # (keep: inputs stay allocated until the synchronisation)
    _sync()
    with limit():
        o_attr = Out(24, size)
        sc.hit_attributes_primary_dev(view, w, h, P, o_attr.ptr, d_inst=I, shard=sh)
        rays["ao_rays"] = Out(32, size)
        sc.ao_rays_dev(view, w, h, P, rays["ao_rays"].ptr, p.ao_radius, frame=ST.AO_FRAME, ao_eps=p.ao_eps, d_primary_inst=I, shard=sh)
        for name, index, sample in ST.LIGHT_RUNS:
            rays["light_rays_" + name] = Out(32, size)
            sc.light_rays_dev(view, w, h, lights[index], P, rays["light_rays_" + name].ptr, light_index=index, frame0=ST.LIGHT_FRAME0, sample=sample,
                              shadow_eps=p.shadow_eps, d_primary_inst=I, shard=sh)
        rays["emitter_rays"] = Out(32, size)
        sc.emitter_rays_dev(view, w, h, P, rays["emitter_rays"].ptr, frame0=ST.EMITTER_FRAME0, sample=ST.EMITTER_SAMPLE, shadow_eps=p.shadow_eps,
                            emitter_eps=p.emitter_eps, d_primary_inst=I, shard=sh)
        # the light term over the attribute pass's own records
        terms = {}
        for name, sel, ambient in (("light_term_local", slice(0, 2), 0.0), ("light_term_directional", slice(2, 3), 0.25)):
            planes = syn.planes[sel]
            d_lit = _dev(np.stack([_laid_host(pl, 1, pix, rec, size) for pl in planes]))
            keep.append(d_lit)
            terms[name] = Out(4, size)
            sc.light_term_dev(view, w, h, lights[sel], P, o_attr.ptr, d_lit.data_ptr(), terms[name].ptr, n_samples=p.light_samples, ambient=ambient, shard=sh)
        # the bounce: the rays and their hits are the caller's, the attribute records the device's own (pixel order, then laid out)
        d_brays, d_bhits, d_binst = _dev(f.b_rays), _dev(f.b_hits), _dev(f.b_inst)
        o_battr = Out(24, n)
        sc.hit_attributes_rays_dev(d_brays.data_ptr(), n, d_bhits.data_ptr(), o_battr.ptr, d_inst=d_binst.data_ptr())
        _torch().cuda.synchronize()
        everything = np.arange(n)
        b_attr = o_battr.taken(everything, everything, n, what + " bounce_attr")[0]
        l_rays, l_hits, l_attr = _laid(f.b_rays, 32, pix, rec, size), _laid(f.b_hits, 8, pix, rec, size), _laid(b_attr, 24, pix, rec, size)
        for name, index, sample in ST.LIGHT_RUNS[:2] + ST.LIGHT_RUNS[3:]:
            key = "bounce_light_rays_" + name.rstrip("0")
            rays[key] = Out(32, size)
            sc.bounce_light_rays_dev(w, h, lights[index], l_rays.data_ptr(), l_hits.data_ptr(), l_attr.data_ptr(), rays[key].ptr, light_index=index,
                                     frame0=ST.LIGHT_FRAME0, sample=sample, shadow_eps=p.shadow_eps, shard=sh)
        # the emitter table and the selection
        rec_e, c = sc.get_emitters()
        d_u0, o_j = _dev(syn.u0), Out(4, syn.u0.size)
        sc.debug_emitter_select(d_u0.data_ptr(), syn.u0.size, o_j.ptr)
        img = {}
        if images:
            d_cnt, d_cnt_lo, d_val, d_val_lo = _dev(syn.counts), _dev(syn.counts_lo), _dev(syn.values), _dev(syn.values_lo)
            d_work = _torch().zeros((n * 4,), dtype=_torch().uint8, device="cuda")
            img = {"ao_filter": Out(4, n), "ao_upsample": Out(4, n), "value_filter": Out(4, n), "value_upsample": Out(4, n)}
            sc.ao_filter_dev(w, h, P, d_cnt.data_ptr(), img["ao_filter"].ptr, ST.AO_SAMPLES, 1, depth_tol=ST.AO_DEPTH_TOL, normal_cos=p.normal_cos, d_attr=o_attr.ptr)
            sc.ao_upsample_dev(w, h, ST.STRIDE, ST.PHASE, P, d_cnt_lo.data_ptr(), img["ao_upsample"].ptr, ST.AO_SAMPLES, ST.UP_RADIUS, depth_tol=ST.AO_DEPTH_TOL,
                               normal_cos=p.normal_cos, d_attr=o_attr.ptr)
            sc.value_filter_dev(w, h, P, d_val.data_ptr(), img["value_filter"].ptr, ST.LEVELS, depth_tol=p.depth_tol, normal_cos=p.normal_cos, d_attr=o_attr.ptr,
                                d_work=d_work.data_ptr())
            sc.value_upsample_dev(w, h, ST.STRIDE, ST.PHASE, P, d_val_lo.data_ptr(), img["value_upsample"].ptr, ST.UP_RADIUS, depth_tol=p.depth_tol,
                                  normal_cos=p.normal_cos, d_attr=o_attr.ptr)
        _torch().cuda.synchronize()
        sc.check()
    outs["attr"] = _attr_of(o_attr.taken(pix, rec, n, what + " attr")[0], what + " attr")
    outs["bounce_attr"] = _attr_of(b_attr, what + " bounce_attr")
    for name, o in rays.items():
        outs[name] = SC.rays_of(o.taken(pix, rec, n, what + " " + name)[0].view(np.float32))
    for name, o in terms.items():
        outs[name] = {"term": o.taken(pix, rec, n, what + " " + name)[0].view(np.float32).reshape(-1)}
    outs["emitter_records"], outs["emitter_c"] = SC.emitter_records_of(s, rec_e), {"c": c}
    j_all = np.arange(syn.u0.size)
    outs["emitter_select"] = {"j": o_j.taken(j_all, j_all, syn.u0.size, what + " select")[0].view(np.uint32).reshape(-1)}
    for name, o in img.items():
        raw = o.taken(everything, everything, n, what + " " + name)[0]
        outs[name] = {"term": raw.view(TERM_DTYPE).reshape(-1)} if name.startswith("ao_") else {"value": raw.view(np.float32).reshape(-1)}
    return outs


# ---- the k = 0 bases, once -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def worlds(trx, orc):
    made, trees = {}, []

    def get(case):
        if case not in made:
            base = SC.recentred(trx, *case)
            s0, p0 = SC.scaled(trx, base, 0), SC.scaled_params(base, 0)
            f0 = ST.base_frame(orc, s0, p0)
            tree = Tree(trx, s0)
            trees.append(tree)
            dev0 = {shard: device_outputs(trx, tree, p0, f0, shard, images=shard[2] == 0) for shard in LAYOUTS}
            made[case] = types.SimpleNamespace(base=base, s0=s0, p0=p0, f0=f0, tree=tree, dev0=dev0)
        return made[case]
    yield get
    for t in trees:
        t.close()


def _against_twin(orc, tree, p, f, dev, what):
    twin = ST.twin_outputs(orc, tree.s, p, f, w2o=tree.w2o)
    assert set(dev) <= set(twin)
    for name in dev:
        SC.assert_same(dev[name], twin[name], "%s %s, device against twin" % (what, name))
    return twin


@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_the_base_is_an_ordinary_scene(trx, orc, worlds, case):
    """k = 0: the recentred scene is held to the twins like any other, in both layouts."""
    wd = worlds(case)
    assert wd.tree.n_emitters >= 2
    for shard in LAYOUTS:
        _against_twin(orc, wd.tree, wd.p0, wd.f0, wd.dev0[shard], "%s k 0 shard %s" % (case[0], shard))


@pytest.mark.parametrize("k", sorted(SC.SAFE + SC.EDGE))
@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_every_output_at_every_exponent(trx, orc, worlds, case, k):
    """Device against twin at k for every k; for SAFE also device at k against device at 0 under the table, twin-free."""
    wd = worlds(case)
    s, p = SC.scaled(trx, wd.base, k), SC.scaled_params(wd.base, k)
    f = ST.carried_frame(orc, wd.s0, wd.f0, s)
    tree = Tree(trx, s)
    try:
        assert tree.n_emitters == wd.tree.n_emitters
        for shard in LAYOUTS:
            what = "%s k %d shard %s" % (IDS[SC.CASES.index(case)], k, shard)
            dev = device_outputs(trx, tree, p, f, shard, images=shard[2] == 0)
            if k in SC.SAFE:
                for name in dev:
                    SC.assert_same(dev[name], SC.expect_from_base(name, wd.dev0[shard][name], k), "%s %s, device against its own k = 0 output" % (what, name))
            _against_twin(orc, tree, p, f, dev, what)
    finally:
        tree.close()


# ---- the whole passes with their walks ------------------------------------------------------------------------------------------------

def _primary(trx, sc, s, sem=0):
    from tray_racing_amd import _lib as L
    n = s.w * s.h
    o_prim, o_inst = Out(8, n), Out(4, n)
    _sync()
    with limit():
        L.check(sc._lib.trx_trace_primary_inst_dev(sc.handle, C.byref(s.view), s.w, s.h, L.Shard(0, 1, 0, 0), sem, C.c_void_p(o_prim.ptr), C.c_void_p(o_inst.ptr), None))
        _torch().cuda.synchronize()
    every = np.arange(n)
    return (o_prim, o_inst, o_prim.taken(every, every, n, "primary")[0].view(SC.HIT).reshape(-1).copy(),
            o_inst.taken(every, every, n, "primary inst")[0].view(np.uint32).reshape(-1).copy())


def _walked(trx, orc, tree, p):
    """(primary components, {pass: bytes}) of the device, and the twins' bytes for the same passes on the oracle at this k."""
    s, sc = tree.s, tree.sc
    w, h, view, n = s.w, s.h, s.view, s.w * s.h
    o_prim, o_inst, prim, inst = _primary(trx, sc, s)
    prim = prim.view(orc.HIT_DTYPE)
    P, I = o_prim.ptr, o_inst.ptr
    point = [p.point.product(trx)]
    lights = [l.product(trx) for l in p.lights]
    outs = {"ao": Out(1, n), "light": Out(1, n, planes=3), "indirect": Out(4, n, planes=3), "emitter": Out(4, n, planes=3)}
    with limit():
        sc.trace_ao_visibility_dev(view, w, h, P, outs["ao"].ptr, ST.AO_SAMPLES, p.ao_radius, frame0=ST.AO_FRAME, ao_eps=p.ao_eps, d_primary_inst=I)
        sc.trace_light_visibility_dev(view, w, h, lights, P, outs["light"].ptr, n_samples=p.light_samples, frame0=ST.LIGHT_FRAME0, shadow_eps=p.shadow_eps, d_primary_inst=I)
        sc.trace_indirect_rgb_dev(view, w, h, point, P, outs["indirect"].ptr, n_samples=2, frame0=ST.BOUNCE_FRAME, bounce_eps=p.bounce_eps, shadow_eps=p.shadow_eps,
                                  d_primary_inst=I)
        sc.trace_emitter_light_dev(view, w, h, P, outs["emitter"].ptr, n_samples=2, frame0=ST.EMITTER_FRAME0, shadow_eps=p.shadow_eps, emitter_eps=p.emitter_eps,
                                   d_primary_inst=I)
        _torch().cuda.synchronize()
        sc.check()
    every = np.arange(n)
    got = {name: o.taken(every, every, n, name) for name, o in outs.items()}
    got = {"ao": got["ao"].reshape(n), "light": got["light"].reshape(3, n), "indirect": got["indirect"].reshape(3, n * 4).view(np.float32),
           "emitter": got["emitter"].reshape(3, n * 4).view(np.float32)}
    # the twins, on the oracle's walks over this tree
    osc, oview = ST.oracle_scene(orc, s, tree.w2o), orc.view_from_bytes(bytes(view))
    recs = tri_records(s.flat.tri_verts)
    geo = LT.frame_geometry(view, w, h, prim, inst, recs, tree.w2o)
    rec_e, c, _, _ = ST.emitter_table(s, recs)
    want = {"ao": visibility_counts(orc, osc, oview, w, h, prim, inst, 0, ST.AO_FRAME, ST.AO_SAMPLES, p.ao_eps, p.ao_radius),
            "light": LT.visibility_planes(orc, osc, view, w, h, geo, prim, p.lights, ST.LIGHT_FRAME0, p.light_samples, p.shadow_eps, 0),
            "indirect": MT.indirect_rgb(orc, osc, oview, w, h, prim, inst, recs, tree.w2o, [p.point], ST.BOUNCE_FRAME, 2, p.bounce_eps, p.shadow_eps, 0, s.mats, s.idx),
            "emitter": ET.emitter_light(orc, osc, view, w, h, geo, prim, recs.shape[0], rec_e, c, s.mats, ST.EMITTER_FRAME0, 2, p.shadow_eps, p.emitter_eps, 0)}
    return ST.primary_of(s, prim, inst), got, want


@pytest.fixture(scope="module")
def walked_base(trx, orc, worlds):
    made = {}

    def get(case):
        if case not in made:
            wd = worlds(case)
            made[case] = _walked(trx, orc, wd.tree, wd.p0)
        return made[case]
    return get


@pytest.mark.parametrize("k", (0,) + SC.WALKED)
@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_walked_passes_equal_the_twins_on_the_oracle(trx, orc, worlds, walked_base, case, k):
    """trx_trace_ao_visibility_dev, trx_trace_light_visibility_dev, trx_trace_indirect_rgb_dev (2 samples, the point light) and
    trx_trace_emitter_light_dev (2 samples) over the device's own primary records: equal to the twins on the oracle at the
    same k, and the primary records the k = 0 records under the table.  No covariance is asked of the walk-dependent planes
    (a walk clamps at an absolute 0.0001): how many of their bytes differ from k = 0 is printed and left there."""
    wd = worlds(case)
    prim0, got0, _ = walked_base(case)
    tree = wd.tree if k == 0 else Tree(trx, SC.scaled(trx, wd.base, k))
    try:
        prim, got, want = (prim0, got0, walked_base(case)[2]) if k == 0 else _walked(trx, orc, tree, SC.scaled_params(wd.base, k))
        SC.assert_same(prim, SC.expect_from_base("primary", prim0, k), "%s k %d, the device's primary records against its k = 0 records" % (case[0], k))
        assert (prim["prim"] != SC.INVALID).sum() > 100
        for name in got:
            SC.assert_same({name: got[name].reshape(-1)}, {name: np.asarray(want[name], dtype=got[name].dtype).reshape(-1)}, "%s k %d %s" % (case[0], k, name))
            print("%s k %d %s: %d of %d bytes differ from k = 0" % (case[0], k, name, (got[name].view(np.uint8) != got0[name].view(np.uint8)).sum(), got[name].nbytes))
        assert (got["ao"] != 0xFF).sum() > 100 and (got["indirect"] > 0).sum() > 20 and (got["emitter"] > 0).sum() > 10 and np.unique(got["light"]).size >= 3
    finally:
        if k:
            tree.close()


# ---- the scalings that are no powers of two --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SC.ADVERSARIAL)
def test_adversarial_scalings_equal_the_twin(trx, orc, name):
    """tests/adversarial_scenes.py's 1e-30, 1e19 and x-extent-near-FLT_MAX scenes under a sentinel-free frame of caller records
    whose prim cycles through the triangles: every post-walk kernel against the twin, both layouts."""
    s, prim, inst, p = SC.adversarial(trx, name)
    n = s.w * s.h
    b_rays = np.zeros(n, dtype=orc.RAY_DTYPE)
    with np.errstate(all="ignore"):
        d = ST.primary_dirs(s.view, s.w, s.h, np.arange(n) % s.w, np.arange(n) // s.w)
    b_rays["origin"], b_rays["direction"], b_rays["tmax"] = np.array(s.view.eye, dtype=np.float32)[None, :], -d[:, ::-1], SC.F32_MAX
    b_hits = prim.copy()
    b_hits["prim"] = (prim["prim"] + 11) % s.flat.n_tris
    b_hits["prim"][::9] = SC.INVALID
    f = types.SimpleNamespace(prim=prim.view(orc.HIT_DTYPE), inst=inst, b_rays=b_rays, b_hits=b_hits.view(orc.HIT_DTYPE), b_inst=inst)
    tree = Tree(trx, s)
    try:
        for shard in LAYOUTS:
            dev = device_outputs(trx, tree, p, f, shard, images=shard[2] == 0)
            _against_twin(orc, tree, p, f, dev, "%s shard %s" % (name, shard))
    finally:
        tree.close()
