"""Every walk on hostile rays, cameras and instance transforms (tests/hostile_inputs.py), bit for bit against the oracle,
which tests/test_hostile_inputs.py holds to its own brute force on the same inputs.  Run with `-m gpu` on an MI355X.

These are inputs, not attempts to fault the card: no address a kernel forms depends on a ray's or a view's floats.  Rays are
read by item number (trace_refill.inc:151) and records written by it or by a pixel index made of integers
(trace_refill.inc:187-201, trace_stack.inc:63); nodes are addressed by child_base + popcount of a hit mask
(trace_walk_plain.inc:37-45 and :122-133, trace_walk_pipe.inc:29, trace_thin.inc:195), triangles by the node's own
primitive base + a bit index (trace_triangles.inc:56 and :117, trace_thin.inc:108 and :231), and the AO refill and the
attribute pass read the triangle of `prim` from a record a pass wrote, behind prim != TRX_INVALID
(trace_refill.inc:216-220, kernels.hip:861-874); the only float-to-integer conversion in the kernels picks a quadrant
(kernels.hip:470).  A walk of non-finite planes ends: NaN comparisons enter nothing, and the step cap (trace_walk_plain.inc
:238) bounds the rest.  Accordingly every record handed to an AO, attribute or visibility pass below was written by a pass
of the same test.

Two cuts against the issue's "every hostile view, every size, semantics 0, 3 and 4", both for the reference side's cost.
The AO visibility pass runs under semantics 4 on the 8 x 8 and 16 x 16 images only (0 and 3 at every size): its twin builds
the AO rays pixel by pixel in Python, four samples a pixel.  And the views whose rays walk the whole
tree (hostile_inputs.walks_whole_tree: a NaN eye, vw == 0, the all-zero view, eye == look_at, the eye 1e6 diagonals away)
cost the oracle every triangle for every pixel - 3 s a frame on the bistro-class scene at 48 x 24.  They run at every size
on the Cornell-class scene and the instanced soup, and on the 8 x 8 image of the kitchen- and bistro-class scenes, through
every pass below; the kernels take the same path whatever the image size (a tile of NaN rays fails `fits`).

The decode-once diagnostic switch (include/trx_dev.h, tune bits 0x40000 / 0x80000) is compiled into development builds only
(api_launch.cpp, TRX_DEV_TUNE): the shipped library does not honour it, so there is no leg with the step switched off.

The names ending in _pipe are the padded twins of the three single-level scenes (helpers.padded_flat): the same nodes and
triangles followed by unreferenced zero records, which the library walks with the pipelined kernels (trace_walk_pipe.inc) in
every mode but the primary pass and the ray service.  A twin shares its base case's rays, views and oracle answers - the
oracle walks the unpadded scene, once - and differs only in the scene on the device; the calls that never take the pipelined
walk (bare primary passes, the ray service, the attribute pass over a primary frame) are left to the base case."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import hostile_inputs as H
from ao_visibility_twin import visibility_counts
from helpers import ALL_SEMS, assert_walk_kinds, bits, instanced_scene, make_scene, padded_flat, w2o_rows
from hit_attr_twin import attr_bits, hit_attrs, primary_dirs, primary_origins, primary_pixels, tri_records

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
N_RAYS = 4096
# the oracle's workers per call (0 would be one per core of the machine, woken for every one of a few thousand small calls)
THREADS, FEW = 8, 2
SIZES = [(8, 8), (16, 16), (48, 24), (33, 47)]
PIPE_SCENES = ["cornell_pipe", "kitchen_pipe", "bistro_pipe"]
SCENES = ["cornell", "kitchen", "bistro", "bistro_tlas", "instanced"] + PIPE_SCENES
CAMERA_SCENES = ["cornell", "kitchen", "bistro", "bistro_tlas"] + PIPE_SCENES
# the passes that never take the pipelined walk run on the base cases only
PRIMARY_SCENES = ["cornell", "kitchen", "bistro", "bistro_tlas"]


@pytest.fixture(scope="module", autouse=True)
def need_gpu(trx):
    lib = trx.load()
    assert lib.trx_device_count() > 0, "no HIP device visible to libtrx.so"
    buf = C.create_string_buffer(64)
    lib.trx_device_name(0, buf, 64)
    assert buf.value.startswith(b"gfx950"), buf.value


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _records(n, fill=-1):
    torch = _torch()
    return torch.full((max(n, 1),), fill, dtype=torch.int64, device="cuda")


def _hits(t):
    from tray_racing_amd import dist as D
    return D.int64_to_hits(t)


def as_view(raw):
    from tray_racing_amd import _lib
    v = _lib.View()
    C.memmove(C.byref(v), raw, C.sizeof(v))
    return v


class Case:
    """A scene on the device, its oracle twin, one hostile batch and the oracle's answers to it (computed once per
    semantics word, shared by the tests, never modified)."""

    def __init__(self, trx, orc, name):
        self.trx, self.orc, self.name = trx, orc, name
        self.instanced = name == "instanced"
        self.padded = False
        self._memo = {}
        if self.instanced:
            mats, mcls = H.hostile_affines(np.random.default_rng(7), 16)
            self.flat, _o2w, world, self.first, _b = instanced_scene(trx, n_objects=3, tris_per_object=300, matrices=mats)
            self.inst_classes = mcls[self.flat.instance_source]
            self.sc = trx.Scene(self.flat)
            self.w2o = self.sc.instance_world_to_object()   # the oracle walks with the rows the kernels use
            self.osc = orc.Scene(self.flat.nodes, self.flat.tri_verts, self.flat.instance_offsets, self.flat.tlas_start,
                                 instance_w2o=self.w2o)
            # aim at the instances near the origin (the far and the huge ones are met by chance); hostile_views frames them
            self.aim = world[np.abs(world).max(axis=1) < 1e4]
            self.shape = type("W", (), {"tri_verts": self.aim, "nodes": self.flat.nodes})
        else:
            scene, tris, tlas = {"cornell": ("cornell", 0, False), "kitchen": ("kitchen", 20000, False),
                                 "bistro": ("bistro", 60000, False), "bistro_tlas": ("bistro", 60000, True)}[name]
            self.flat, _view, self.osc, _ov = make_scene(trx, orc, scene, tris, 16, 16, tlas=tlas)
            self.sc = trx.Scene(self.flat)
            self.w2o, self.aim, self.shape = None, self.flat.tri_verts, self.flat
        self.rays, self.classes = H.hostile_rays(trx, self.flat, N_RAYS, 5, tri_verts=self.aim)
        self._want, self._views, self._frames, self._tame = {}, {}, {}, {}

    def memo(self, key, arrays, compute):
        """compute() once per (key, contents of `arrays`): a padded twin asks what its base case asked."""
        h = hashlib.sha1()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        key = key + (h.digest(),)
        if key not in self._memo:
            self._memo[key] = compute()
        return self._memo[key]

    def oracle(self, rays, sem):
        """(hits, instance ids or None, stats), computed once per batch and semantics word"""
        threads = THREADS if rays.shape[0] > 256 else FEW

        def compute():
            if self.instanced:
                return self.osc.trace_rays_inst(rays, sem=sem, threads=threads)
            hits, st = self.osc.trace_rays(rays, sem=sem, threads=threads)
            return hits, None, st
        return self.memo(("rays", sem), (rays,), compute)

    def want(self, sem):
        if sem not in self._want:
            self._want[sem] = self.oracle(self.rays, sem)
            assert self._want[sem][2].overflow == 0
        return self._want[sem]

    def views(self, w, h):
        """[(name, product view, oracle view)].  The views whose rays walk the whole tree (H.walks_whole_tree: the oracle
        tests every triangle for every pixel) run at every size on the two small scenes, elsewhere on the 8 x 8 image."""
        if (w, h) not in self._views:
            small = self.name in ("cornell", "instanced") or w * h <= 64
            self._views[(w, h)] = [(n, as_view(raw), self.orc.view_from_bytes(raw)) for n, raw in H.hostile_views(self.trx, self.shape, w, h)
                                   if small or not H.walks_whole_tree(n)]
        return self._views[(w, h)]

    def tame_view(self, w, h):
        """(name, product view, oracle view) of the scene's own camera."""
        if (w, h) not in self._tame:
            eye, look, fov = self.trx.scene_camera("bistro" if self.name.startswith("bistro") else self.name)
            raw = bytes(self.trx.view_from_camera(eye, look, fov, w, h))
            self._tame[(w, h)] = ("tame", as_view(raw), self.orc.view_from_bytes(raw))
        return self._tame[(w, h)]

    def oracle_primary(self, ov, w, h, sem):
        """(hits, instance ids or None, stats) of a frame, computed once per view (the views of `views` live as long as the case)."""
        key = (id(ov), w, h, sem)
        if key not in self._frames:
            if self.instanced:
                self._frames[key] = self.osc.trace_primary_inst(ov, w, h, sem=sem, threads=FEW)
            else:
                hits, st = self.osc.trace_primary(ov, w, h, sem=sem, threads=FEW)
                self._frames[key] = (hits, None, st)
            assert self._frames[key][2].overflow == 0
        return self._frames[key]

    def oracle_ao(self, ov, w, h, prim, sem, frame, eps):
        return self.memo(("ao", id(ov), w, h, sem, frame, eps), (prim,),
                         lambda: self.osc.trace_ao(ov, w, h, prim, sem=sem, frame=frame, ao_eps=eps, threads=FEW)[0])

    def visibility(self, ov, w, h, hits, sem, frame0, n_samples, eps, radius):
        """The AO visibility twin's counts over `hits` (pixel by pixel in Python: once per frame)."""
        return self.memo(("vis", id(ov), w, h, sem, frame0, n_samples, eps, radius), (hits,),
                         lambda: visibility_counts(self.orc, self.osc, ov, w, h, hits, None, sem, frame0, n_samples, eps, radius))

    def close(self):
        self.sc.close()


class PaddedCase:
    """The padded twin of a single-level case: everything is the base case's - rays, classes, views, the unpadded triangles
    and every cached oracle answer - but `sc`, the padded scene on the device, which takes the pipelined walk."""

    def __init__(self, base, name):
        assert not base.instanced and not base.flat.has_tlas
        self.base, self.name, self.padded = base, name, True
        self.sc = base.trx.Scene(padded_flat(base.trx, base.flat))
        self.assert_walks()

    def assert_walks(self):
        """Asked again by every test that takes the twin (the `cases` fixture): pipelined on the twin, plain on the base
        scene, in the three modes these tests launch; the primary pass plain on both."""
        for mode in (self.base.trx.MODE_AO, self.base.trx.MODE_RAYS, self.base.trx.MODE_FUSED):
            assert_walk_kinds(self.base.trx, self.base.sc, self.sc, mode)

    def __getattr__(self, attr):        # (only what the twin does not hold itself)
        return getattr(self.base, attr)

    def close(self):
        self.sc.close()


@pytest.fixture(scope="module")
def cases(trx, orc):
    made = {}

    def get(name):
        if name not in made:
            made[name] = PaddedCase(get(name[:-len("_pipe")]), name) if name.endswith("_pipe") else Case(trx, orc, name)
        if made[name].padded:
            made[name].assert_walks()
        return made[name]
    yield get
    trx.load().trx_set_kernel_variant(0)
    for c in made.values():
        c.close()


def by_class(classes, bad):
    """What a failure message says: how many of which class."""
    names, counts = np.unique(classes[bad], return_counts=True)
    return dict(zip(names.tolist(), counts.tolist()))


def assert_records(got, want, classes, what, got_inst=None, want_inst=None):
    bad = (bits(got["t"]) != bits(want["t"])) | (got["prim"] != want["prim"])
    if want_inst is not None:
        hit = want["prim"] != MISS
        bad |= (got_inst != np.where(hit, want_inst, MISS))
    assert not bad.any(), "%s: %d records differ from the oracle, by class %s (first %s)" % (
        what, bad.sum(), by_class(classes, bad), np.flatnonzero(bad)[:5])


# ---- rays: the full-wave walk ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_trace_rays_all_semantics(cases, name):
    """trx_trace_rays (trx_trace_rays_inst with its instance ids on the instanced soup) over 4096 rays, half of them
    hostile, under all eight semantics words: no overflow error, every record the oracle's."""
    c = cases(name)
    for sem in ALL_SEMS:
        want, winst, _ = c.want(sem)
        if c.instanced:
            got, ginst, _ = c.sc.trace_rays_inst(c.rays, sem=sem)
        else:
            (got, _), ginst = c.sc.trace_rays(c.rays, sem=sem), None
        assert_records(got, want, c.classes, "%s sem %d" % (name, sem), ginst, winst)
    tame = c.classes == H.TAME
    assert (c.want(3)[0]["prim"][tame] != MISS).sum() > tame.sum() // 4          # the tame half is worth having


@pytest.mark.parametrize("name", SCENES)
def test_any_hit_and_the_masked_pair(cases, name):
    """trx_trace_occluded says what the closest-hit oracle says about hit / no hit; the masked calls with mask 0xFF are the
    unmasked ones (semantics 0 and 3)."""
    c = cases(name)
    for sem in (0, 3):
        want, winst, _ = c.want(sem)
        hit = want["prim"] != MISS
        occ, _ = c.sc.trace_occluded(c.rays, sem=sem)
        bad = occ.astype(bool) != hit
        assert set(np.unique(occ)) <= {0, 1} and not bad.any(), (name, sem, by_class(c.classes, bad))
        got, ginst, _ = c.sc.trace_rays_masked(c.rays, 0xFF, sem=sem)
        assert_records(got, want, c.classes, "%s masked sem %d" % (name, sem), ginst if winst is not None else None, winst)
        mocc, _ = c.sc.trace_occluded_masked(c.rays, 0xFF, sem=sem)
        assert (mocc == occ).all(), (name, sem)


@pytest.mark.parametrize("name", SCENES)
def test_counting_pass_counts_what_the_oracle_counts(cases, name):
    """trx_count_rays: node steps, triangle tests, hits and the deepest stack of the hostile batch are the oracle's."""
    c = cases(name)
    d_rays, d_hits = _dev(c.rays), _records(N_RAYS)
    for sem in (0, 3):
        want, _winst, ost = c.want(sem)
        st = c.sc.count_rays(d_rays.data_ptr(), N_RAYS, d_hits.data_ptr(), sem=sem)
        assert (st.n_rays, st.n_node, st.n_tri, st.n_hits, st.max_stack, st.overflow) == (
            ost.n_rays, ost.n_node, ost.n_tri, ost.n_hits, ost.max_stack, 0), (name, sem)
        assert_records(_hits(d_hits), want, c.classes, "%s counting pass sem %d" % (name, sem))


@pytest.mark.parametrize("name", SCENES)
def test_hit_attributes_of_the_calls_own_records(cases, trx, name):
    """trx_trace_rays_attr: hits as above, and attributes that are the numpy twin's on the records the call itself
    produced (a miss: the all-zero record)."""
    c = cases(name)
    recs = tri_records(c.flat.tri_verts)
    for sem in (0, 3):
        want, winst, _ = c.want(sem)
        hits, inst, attr = c.sc.trace_rays_attr(c.rays, sem=sem)
        assert_records(hits, want, c.classes, "%s attr call sem %d" % (name, sem), inst if c.instanced else None, winst)
        twin = hit_attrs(recs, c.rays["origin"], c.rays["direction"], hits["prim"], inst if c.instanced else None, c.w2o)
        bad = (attr_bits(attr) != attr_bits(twin)).any(1)
        assert not bad.any(), (name, sem, by_class(c.classes, bad), np.flatnonzero(bad)[:5])


@pytest.mark.parametrize("name", SCENES)
def test_the_ray_service_and_the_batch_traverse(cases, name):
    """trx_traverse_batch, and trx_traverse1 from 1 and from 8 host threads (the resident ray service, both levels), on
    600 rays: t bit for bit, primitive / geometry / instance ids as the oracle's records translate.  (A padded twin: the
    batch alone - the ray service takes the plain walk whatever the scene's size.)"""
    c = cases(name)
    rays, cls = c.rays[:600], c.classes[:600]
    flat = c.flat
    for sem in (0, 3):
        want, winst, _ = c.want(sem)
        want, winst = want[:600], None if winst is None else winst[:600]
        hit = want["prim"] != MISS
        batch, _ = c.sc.traverse_batch(rays, sem=sem)
        answers = [("batch", batch)] + [("%d threads" % n, c.sc.traverse_threads(rays, threads=n, sem=sem)[0])
                                        for n in (() if c.padded else (1, 8))]
        for how, got in answers:
            bad = bits(got["t"]) != bits(want["t"])
            bad |= (got["primitive_id"] == MISS) != ~hit
            if flat.has_tlas:
                g = np.searchsorted(flat.blas_tri_start, want["prim"][hit], side="right") - 1
                bad[hit] |= (got["geometry_id"][hit] != g) | (got["primitive_id"][hit] != want["prim"][hit] - flat.blas_tri_start[g])
            else:
                bad[hit] |= got["primitive_id"][hit] != want["prim"][hit]
            if winst is not None:
                bad[hit] |= got["instance_id"][hit] != winst[hit]
            assert not bad.any(), "%s sem %d, %s: %s" % (name, sem, how, by_class(cls, bad))


# ---- rays: the thin walk -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_thin_walk_a_handful_of_hostile_rays(cases, trx, name):
    """Batches of 1, 7, 8, 9 and 65 rays run (almost) wholly in the thin walk, eight lanes to a ray: eight rays of a wave
    share its node steps' arithmetic path, so a hostile ray sits beside seven others.  Windows of the hostile batch that
    start on a hostile and on a tame ray, all eight semantics; any hit; thin waves off (variant bit 28) gives the same."""
    c = cases(name)
    lib = trx.load()
    try:
        for n in (1, 7, 8, 9, 65):
            for start in (1 + 70 * n, 70 * n):          # (odd indices are hostile)
                rays, cls = c.rays[start:start + n], c.classes[start:start + n]
                for sem in ALL_SEMS:
                    want, winst, st = c.oracle(rays, sem)
                    assert st.overflow == 0
                    what = "%s rays %d..%d sem %d" % (name, start, start + n, sem)
                    if c.instanced:
                        got, ginst, _ = c.sc.trace_rays_inst(rays, sem=sem)
                    else:
                        (got, _), ginst = c.sc.trace_rays(rays, sem=sem), None
                    assert_records(got, want, cls, what, ginst, winst)
                    if sem in (0, 3):
                        occ, _ = c.sc.trace_occluded(rays, sem=sem)
                        assert (occ.astype(bool) == (want["prim"] != MISS)).all(), what
                        lib.trx_set_kernel_variant(1 << 28)
                        off, _ = c.sc.trace_rays(rays, sem=sem)
                        lib.trx_set_kernel_variant(0)
                        assert_records(off, want, cls, what + ", thin waves off")
    finally:
        lib.trx_set_kernel_variant(0)


# ---- isolation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", [0, 3])
@pytest.mark.parametrize("name", SCENES)
def test_a_hostile_neighbour_never_changes_a_tame_rays_record(cases, trx, name, sem):
    """The same 256 tame rays at the same lanes of two batches: beside hostile rays (56 of every 64 lanes) and beside plain
    misses.  Their records are identical between the two and equal the oracle's - closest hit, any hit and the ray
    service.  Under semantics 0 one out-of-range ray sends every node step of its wave through the divisions."""
    c = cases(name)
    tame = c.rays[c.classes == H.TAME][:256]
    hostile = c.rays[c.classes != H.TAME]
    _isolation(c, trx, name, sem, tame, hostile, service=not c.padded)
    # Beside rays of every class almost every wave holds an out-of-range DIRECTION and divides six times a node step.  The
    # middle path - e * (1/d) kept, (p - o) / d divided: a wave with an out-of-range ORIGIN and no such direction, on a
    # scene that admits both shortcuts (kernels.hip, finish_ray_dir and pow2_exact) - needs neighbours of that kind alone.
    with np.errstate(invalid="ignore"):
        d = np.abs(np.where(hostile["direction"] == 0, np.float32(1.1920929e-7), hostile["direction"]))
        o = np.abs(hostile["origin"])
        dir_in = ((d >= 2.0 ** -30) & (d <= 2.0 ** 20)).all(axis=1)
        org_out = (~((o == 0) | ((o >= 2.0 ** -36) & (o <= 2.0 ** 59)))).any(axis=1)
    assert (dir_in & org_out).sum() >= 100
    _isolation(c, trx, name, sem, tame, hostile[dir_in & org_out], service=False)


def _isolation(c, trx, name, sem, tame, hostile, service):
    a, idx = H.interleaved(trx, tame, hostile)
    b, idx_b = H.with_placeholders(trx, tame)
    assert (idx == idx_b).all() and a.shape == b.shape
    want, winst, _ = c.oracle(tame, sem)
    assert (want["prim"] != MISS).sum() > 64
    tame_cls = np.full(tame.shape[0], H.TAME)

    def closest(rays):
        if c.instanced:
            return c.sc.trace_rays_inst(rays, sem=sem)[:2]
        return c.sc.trace_rays(rays, sem=sem)[0], None
    (ga, ia), (gb, ib) = closest(a), closest(b)
    assert_records(ga[idx], want, tame_cls, "%s sem %d, hostile neighbours" % (name, sem), None if ia is None else ia[idx], winst)
    assert_records(gb[idx], want, tame_cls, "%s sem %d, placeholder neighbours" % (name, sem), None if ib is None else ib[idx], winst)
    assert ga[idx].tobytes() == gb[idx].tobytes()
    oa, ob = c.sc.trace_occluded(a, sem=sem)[0], c.sc.trace_occluded(b, sem=sem)[0]
    assert (oa[idx] == ob[idx]).all() and (oa[idx].astype(bool) == (want["prim"] != MISS)).all()
    if service:
        sa, sb = c.sc.traverse_threads(a, threads=8, sem=sem)[0], c.sc.traverse_threads(b, threads=8, sem=sem)[0]
        assert sa[idx].tobytes() == sb[idx].tobytes() and (bits(sa["t"][idx]) == bits(want["t"])).all()
    # ... and the hostile lanes themselves are the oracle's too
    others = np.setdiff1d(np.arange(a.shape[0]), idx)
    wo, wi, st = c.oracle(a[others], sem)
    assert st.overflow == 0
    assert_records(ga[others], wo, np.full(others.size, "hostile"), "%s sem %d, the hostile lanes" % (name, sem),
                   None if ia is None else ia[others], wi)


# ---- cameras -----------------------------------------------------------------------------------------------------------

def _primary_dev(c, view, w, h, sem, shard=(0, 1), n=None):
    """Records and instance ids of one primary launch (device buffers kept for the passes that read them)."""
    from tray_racing_amd import _lib as L
    n = w * h if n is None else n
    d_hits = _records(n)
    d_inst = _torch().full((n,), -1, dtype=_torch().int32, device="cuda")
    L.check(c.sc._lib.trx_trace_primary_inst_dev(c.sc.handle, C.byref(view), w, h, L.Shard(*shard), sem, C.c_void_p(d_hits.data_ptr()),
                                                 C.c_void_p(d_inst.data_ptr()), C.c_void_p(0)))
    c.sc.check()
    return d_hits, d_inst


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", CAMERA_SCENES)
def test_primary_ao_and_fused_frames_under_every_hostile_view(cases, name, w, h):
    """trx_trace_primary, trx_trace_primary_ao (AO epsilon 0.01 and 1e-4) and trx_trace_frame_dev, every hostile view,
    semantics 0, 3 and 4: the oracle's records, pixel for pixel; a switched-off view hits nothing.  (A padded twin: the AO
    passes and the one-launch frame - the bare primary pass is the base case's.)"""
    c = cases(name)
    n = w * h
    px = np.full(n, "pixel")
    for vname, view, ov in c.views(w, h):
        for sem in (0, 3, 4):
            what = "%s %dx%d %s sem %d" % (name, w, h, vname, sem)
            want, _, _st = c.oracle_primary(ov, w, h, sem)
            if not c.padded:
                got, _ = c.sc.trace_primary(view, w, h, sem=sem)
                assert_records(got, want, px, what + " primary")
                if not H.is_alive(vname):
                    assert (got["prim"] == MISS).all(), what
            for frame, eps in ((1, 0.01), (7, 1e-4)):
                gp, gao, _ = c.sc.trace_primary_ao(view, w, h, sem=sem, frame=frame, ao_eps=eps)
                wao = c.oracle_ao(ov, w, h, gp, sem, frame, eps)
                assert_records(gp, want, px, what + " primary of primary_ao")
                assert_records(gao, wao, px, what + " ao eps %g" % eps)
            d_p, d_a = _records(n), _records(n)
            c.sc.trace_frame_dev(view, w, h, d_p.data_ptr(), d_a.data_ptr(), sem=sem, frame=1, ao_eps=0.01)
            c.sc.check()
            assert_records(_hits(d_p), want, px, what + " fused frame, primary")
            assert_records(_hits(d_a), c.oracle_ao(ov, w, h, want, sem, 1, 0.01), px, what + " fused frame, ao")


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", PRIMARY_SCENES)
def test_batches_mix_hostile_and_tame_views_and_shards_assemble(cases, trx, name, w, h):
    """trx_trace_primary_batch_dev with hostile and tame views in one launch (eight frames a launch, a tame one first and
    fifth): every frame is the oracle's and the tame frames are their single-frame launches'.  trx_trace_primary_dev over
    three compact shards assembles to the same image.  trx_count_primary counts what the oracle counts."""
    from tray_racing_amd import dist as D
    c = cases(name)
    n = w * h
    px = np.full(n, "pixel")
    tame = c.tame_view(w, h)
    hostile = c.views(w, h)
    for sem in (0, 3, 4):
        single = c.sc.trace_primary(tame[1], w, h, sem=sem)[0]
        for k in range(0, len(hostile), 6):
            group = hostile[k:k + 6]
            frames = [tame] + group[:3] + [tame] + group[3:]
            out = _records(len(frames) * n)
            c.sc.trace_primary_batch_dev([v for _, v, _ in frames], w, h, out.data_ptr(), n, sem=sem)
            c.sc.check()
            got = _hits(out)
            for f, (vname, _v, ov) in enumerate(frames):
                want = single if vname == "tame" else c.oracle_primary(ov, w, h, sem)[0]
                assert_records(got[f * n:(f + 1) * n], want, px, "%s %dx%d sem %d batch frame %d (%s)" % (name, w, h, sem, f, vname))
        assert_records(single, c.oracle_primary(tame[2], w, h, sem)[0], px, "tame single frame")
        for vname, view, ov in hostile:
            want, _, ost = c.oracle_primary(ov, w, h, sem)
            fg = D.FrameGather(w, h, 0, 3, "cuda")
            fg.flat.fill_(-1)
            for r in range(3):
                blk = fg.flat[r * fg.records:(r + 1) * fg.records]
                c.sc.trace_primary_dev(view, w, h, blk.data_ptr(), sem=sem, shard=(r, 3, 1))
            c.sc.check()
            assert_records(_hits(fg.assemble()), want, px, "%s %dx%d %s sem %d, three compact shards" % (name, w, h, vname, sem))
            st = c.sc.count_primary(view, w, h, sem=sem)
            assert (st.n_rays, st.n_node, st.n_tri, st.n_hits, st.max_stack, st.overflow) == (
                n, ost.n_node, ost.n_tri, ost.n_hits, ost.max_stack, 0), (name, w, h, vname, sem)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", CAMERA_SCENES)
def test_hit_attributes_and_ao_visibility_over_hostile_primary_frames(cases, name, w, h):
    """trx_hit_attributes_primary_dev against its twin, and trx_trace_ao_visibility_dev with four samples against its
    twin, both fed the records a primary launch of this test wrote under the same view.  (A padded twin: the visibility
    pass, whose any-hit rays launch takes the pipelined walk; the attribute pass walks nothing.)"""
    c = cases(name)
    recs = tri_records(c.flat.tri_verts)
    torch = _torch()
    n = w * h
    rec, ppx, ppy = primary_pixels(w, h)
    for vname, view, ov in c.views(w, h):
        for sem in (0, 3, 4):
            what = "%s %dx%d %s sem %d" % (name, w, h, vname, sem)
            d_hits, d_inst = _primary_dev(c, view, w, h, sem)
            hits = _hits(d_hits)
            if not c.padded:
                d_attr = torch.full((n * 24,), 0xAB, dtype=torch.uint8, device="cuda")
                c.sc.hit_attributes_primary_dev(view, w, h, d_hits.data_ptr(), d_attr.data_ptr(), d_inst=d_inst.data_ptr())
                c.sc.check()
                attr = d_attr.cpu().numpy().view(c.trx.HIT_ATTR_DTYPE)
                twin = hit_attrs(recs, primary_origins(view, rec.size), primary_dirs(view, w, h, ppx, ppy), hits["prim"][rec])
                bad = (attr_bits(attr[rec]) != attr_bits(twin)).any(1)
                assert not bad.any(), (what, int(bad.sum()), (ppx[bad][:3], ppy[bad][:3]))
            if sem == 4 and n > 256:     # (the twin builds its AO rays pixel by pixel in Python: semantics 4 on the two small images)
                continue
            d_out = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
            c.sc.trace_ao_visibility_dev(view, w, h, d_hits.data_ptr(), d_out.data_ptr(), 4, float("inf"), sem=sem, frame0=3,
                                         ao_eps=0.01, d_primary_inst=d_inst.data_ptr())
            c.sc.check()
            want = c.visibility(ov, w, h, hits, sem, 3, 4, 0.01, float("inf"))
            assert (d_out.cpu().numpy() == want).all(), what + ": visibility counts"


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["bistro_tlas", "instanced"])
def test_primary_frames_with_instance_ids_over_two_level_scenes(cases, name, w, h):
    """trx_trace_primary_inst_dev: a two-level scene without transforms (the packet test is on in the TLAS walk) and the
    hostile transforms (it is off: every ray has its own object-space copy) - hits and instance ids, every hostile view."""
    c = cases(name)
    n = w * h
    px = np.full(n, "pixel")
    any_hit = 0
    for vname, view, ov in c.views(w, h):
        for sem in (0, 3, 4):
            want, winst, st = c.osc.trace_primary_inst(ov, w, h, sem=sem, threads=FEW)
            assert st.overflow == 0
            d_hits, d_inst = _primary_dev(c, view, w, h, sem)
            got, ginst = _hits(d_hits), d_inst.cpu().numpy().view(np.uint32)
            assert_records(got, want, px, "%s %dx%d %s sem %d" % (name, w, h, vname, sem), ginst, winst)
            any_hit += int((want["prim"] != MISS).sum())
    assert any_hit > 2 * n          # (some of the views see the scene)


def test_the_rows_the_kernels_use_are_the_rounded_float64_inverse(cases):
    """The instanced cases above hand the oracle the scene's own world-to-object rows, so they cannot see a wrong row.
    Here the rows of every hostile transform - mirror, near-singular shear, scales of 2^-12 and 2^12, a translation of
    1e6 - against numpy's float64 inverse rounded to float32: the library inverts in double and rounds once, and the two
    double inverses differ by (condition number ~ 1e6) x 2^-53, far below half a float32 ulp, so 1 ulp of each row's
    largest entry bounds the difference."""
    c = cases("instanced")
    want = np.stack([w2o_rows(m) for m in c.flat.instance_transforms])
    got = c.w2o
    scale = np.abs(want.reshape(-1, 3, 4)).max(axis=2, keepdims=True)
    err = np.abs(got.reshape(-1, 3, 4).astype(np.float64) - want.reshape(-1, 3, 4))
    bad = (err > scale * 2.0 ** -23).any(axis=(1, 2))
    assert not bad.any(), by_class(c.inst_classes, bad)
    assert set(c.inst_classes) == set(H.AFFINE_CLASSES)
