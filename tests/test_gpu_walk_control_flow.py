"""The plain walk's control flow (trace_walk_plain.inc, trace_stack.inc, node_intersect_kept): the per-lane step behind a scalar
flag of its own, a stack pop whose LDS read is unconditional (its rare path an `if` of its own), the end of a ray behind ONE
wave-level test of a scalar `done` mask with the overflow check folded in (single-level kernels; the two-level ones keep the
per-lane form), a one-comparison loop tail, the uniform step's per-child loop on a 64-bit meta word with `keep == 0` out of
line.  None of that changes an operation, an operand or an order, so every case compares t bit for bit and prim exactly against
the oracle, and every device launch writes into a buffer poisoned just before it (helpers.PoisonedFrames).  Run with
`-m gpu` on an MI355X.  (The triangle phase was rebuilt and measured with this change and left as it was,
profiles/walk_scalar_cost.log; its cases stay: they run the phase between the blocks that did change.)

The shapes are the smallest that reach every block whose layout changed:
  * one 8 x 8 tile of the Cornell-class golden and the 52 x 44 soup golden (partly filled waves);
  * all eight semantics words on the 64 x 48 Cornell frame; the two two-level goldens (lanes with a parked triangle group
    step no node while their neighbours do, and waves in which no lane steps a node while others test triangles);
  * ties under both rules and hits at -0.0 and +0.0: coincident triangles, ray origins in their plane;
  * nested triangles: lanes with 0, 1, 2, 3 and 7 or more pierced triangles in one wave (one-round phases, multi-round
    phases, the cooperative rounds) - the test counts them;
  * chains 13, 40, 64 and 70 deep under primary rays: spill past 12 LDS entries, the HBM pop (lanes past the LDS part beside
    shallow ones in one wave: the pop's clamped LDS read), the last entry, and the overflow error;
  * a tile whose rays all finish in the same trip, and one in which 63 finish together and one goes on and finishes alone:
    the wave-level `done` test with a full and a one-lane mask;
  * explicit rays, any-hit rays and an AO pass on a small scene: the plain walk with refills and thin waves;
  * the counting kernel's totals on the Cornell frame."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import ALL_SEMS, F32_MAX, PoisonedFrames, bits, deep_chain_scene, golden_inputs, image_tile_of, make_scene, random_rays

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MISS = 0xFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def need_gpu(trx):
    lib = trx.load()
    assert lib.trx_device_count() > 0, "no HIP device visible to libtrx.so"
    buf = C.create_string_buffer(64)
    lib.trx_device_name(0, buf, 64)
    assert buf.value.startswith(b"gfx950"), buf.value


def view_of(raw):
    from tray_racing_amd import _lib
    return _lib.View.from_buffer_copy(raw)


class Walk:
    """A scene on the device and in the oracle; the oracle's primary frames computed once per (view, size, sem); every
    device frame goes into a poisoned buffer and is compared there."""

    def __init__(self, trx, orc, nodes, tri_verts, inst=(), tlas_start=0, flat=None):
        self.trx, self.orc = trx, orc
        n = tri_verts.shape[0]
        self.flat = flat if flat is not None else trx.FlatScene(nodes, tri_verts, inst, tlas_start, np.arange(n), [0, n])
        self.osc = orc.Scene.from_flat(self.flat) if flat is not None else orc.Scene(nodes, tri_verts, inst, tlas_start)
        self.sc = trx.Scene(self.flat)
        self._frames, self._bufs = {}, {}

    @classmethod
    def golden(cls, trx, orc, name):
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        self = cls(trx, orc, *golden_inputs(trx, g))
        self.g, self.w, self.h, self.raw = g, int(g["width"]), int(g["height"]), g["view"].tobytes()
        return self

    @classmethod
    def built(cls, trx, orc, verts, counts=None):
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
        flat = trx.flat_build(verts, [verts.shape[0]] if counts is None else counts)
        return cls(trx, orc, None, verts, flat=flat)

    def want(self, raw, w, h, sem):
        key = (raw, w, h, sem)
        if key not in self._frames:
            self._frames[key] = self.osc.trace_primary(self.orc.view_from_bytes(raw), w, h, sem=sem, threads=2)
        return self._frames[key]

    def check(self, raw, w, h, sem, what):
        want, st = self.want(raw, w, h, sem)
        assert st.overflow == 0, what
        if (w, h) not in self._bufs:
            self._bufs[(w, h)] = PoisonedFrames(w * h, tile_of=image_tile_of(w, h), what="%dx%d" % (w, h))
        pf = self._bufs[(w, h)]
        pf.what = what
        expected = pf.expect(want)
        pf.poison()
        self.sc.trace_primary_dev(view_of(raw), w, h, pf.ptr, sem=sem)
        pf.check(expected, what)
        self.sc.check()
        return want, st

    def close(self):
        self.sc.close()


@pytest.fixture(scope="module")
def goldens(trx, orc):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Walk.golden(trx, orc, name)
        return made[name]
    yield get
    for f in made.values():
        f.close()


def camera_view(trx, eye, look, fov, w, h):
    return bytes(trx.view_from_camera(tuple(float(x) for x in eye), tuple(float(x) for x in look), float(fov), w, h))


def cornell_view(trx, w, h, fov=None):
    eye, look, f = trx.scene_camera("cornell")
    return camera_view(trx, eye, look, f if fov is None else fov, w, h)


@pytest.mark.parametrize("fov", [12.0, None])
def test_one_tile(goldens, trx, fov):
    f = goldens("cornell_64")
    for sem in (0, 3):
        want, _ = f.check(cornell_view(trx, 8, 8, fov), 8, 8, sem, "cornell 8x8 fov %s sem %d" % (fov, sem))
        assert (want["prim"] != MISS).sum() > 32


def test_partly_filled_waves(goldens):
    """52 x 44: the last column and row of tiles hold 4 x 8, 8 x 4 and 4 x 4 rays; all eight words."""
    f = goldens("soup_52x44")
    assert (f.w, f.h) == (52, 44)
    for sem in ALL_SEMS:
        want, _ = f.check(f.raw, f.w, f.h, sem, "soup 52x44 sem %d" % sem)
    assert 0 < (want["prim"] != MISS).sum() < f.w * f.h


@pytest.mark.parametrize("sem", ALL_SEMS)
def test_cornell_every_semantics_word(goldens, trx, sem):
    goldens("cornell_64").check(cornell_view(trx, 64, 48), 64, 48, sem, "cornell 64x48 sem %d" % sem)


@pytest.mark.parametrize("name", ["cornell_tlas_48", "kitchen_tlas_f16_56x40"])
def test_two_level_goldens(goldens, name):
    f = goldens(name)
    assert f.flat.has_tlas
    for sem in ALL_SEMS:
        want, _ = f.check(f.raw, f.w, f.h, sem, "%s sem %d" % (name, sem))
    assert (want["prim"] != MISS).sum() > f.w * f.h // 4


def test_two_level_golden_with_f16_records(trx):
    """The fixture's 24-byte triangles through the two-level primary kernel, against the records on file."""
    g = np.load(os.path.join(GOLDEN, "kitchen_tlas_f16_56x40.npz"))
    nodes, tri_verts, inst, tlas_start = golden_inputs(trx, g)
    n = tri_verts.shape[0]
    w, h = int(g["width"]), int(g["height"])
    sc = trx.Scene(trx.FlatScene(nodes, tri_verts, inst, tlas_start, np.arange(n), [0, n]), tri_format=trx.TRI_F16_24, tri_bytes=g["tri_f16"])
    pf = PoisonedFrames(w * h, tile_of=image_tile_of(w, h), what="f16 two-level")
    for sem in (0, 3):
        expected = pf.expect(g["orc_f16_primary_sem%d" % sem])
        pf.poison()
        sc.trace_primary_dev(view_of(g["view"].tobytes()), w, h, pf.ptr, sem=sem)
        pf.check(expected, sem)
    sc.close()


def rays_checked(trx, sc, rays, want, sem, what):
    import torch
    pf = PoisonedFrames(rays.shape[0], what=what)
    expected = pf.expect(want)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
    pf.poison()
    sc.trace_rays_dev(d_rays.data_ptr(), rays.shape[0], pf.ptr, sem=sem)
    pf.check(expected, "sem %d" % sem)
    sc.check()


def test_ties_under_both_rules_golden(trx):
    g = np.load(os.path.join(GOLDEN, "ties_rays.npz"))
    nodes, tri_verts, inst, tlas_start = golden_inputs(trx, g)
    n = tri_verts.shape[0]
    sc = trx.Scene(trx.FlatScene(nodes, tri_verts, inst, tlas_start, np.arange(n), [0, n]))
    for sem in (0, 3):
        rays_checked(trx, sc, g["rays"], g["orc_rays_sem%d" % sem], sem, "ties_rays")
    sc.close()


def coincident_scene():
    """Five copies of one triangle in the plane z = x (a box with a depth: a ray that starts in the plane is inside it past
    the node test's 1e-4) among a few others: every hit of it is a five-way tie."""
    tri = np.array([0, 0, 0, 1, 0, 1, 0, 1, 0], dtype=np.float32)
    others = np.array([[0, 0, -3, 1, 0, -2, 0, 1, -3], [0, 0, 3, 0, 1, 3, 1, 0, 4], [2, 2, 0, 3, 2, 0, 2, 3, 0]], dtype=np.float32)
    return np.concatenate([np.tile(tri, (5, 1)), others])


def coincident_rays(trx):
    """Rays through the coincident triangles from either side, and rays that START in their plane, at (a, b, a) with a and b
    multiples of 1/64: the plane distance -a + a is an exact +0, and t = 0 x (1 / det) is a zero whose sign is the
    determinant's - looking down the z axis gives +0.0, looking up -0.0, both accepted (tmin = 0)."""
    rng = np.random.default_rng(5)
    n = 96
    k = np.arange(n)
    rays = np.zeros(n, dtype=trx.RAY_DTYPE)
    a, b = rng.integers(4, 29, size=n) / 64.0, rng.integers(4, 29, size=n) / 64.0
    up = k % 2 == 1
    in_plane = k % 4 < 2
    rays["origin"][:, 0], rays["origin"][:, 1] = a, b
    rays["origin"][:, 2] = np.where(in_plane, a, np.where(up, a - 0.5, a + 0.5))
    rays["direction"][:, 2] = np.where(up, 1.0, -1.0)
    rays["tmin"], rays["tmax"] = 0.0, F32_MAX
    return rays


def test_ties_at_negative_zero(trx, orc):
    f = Walk.built(trx, orc, coincident_scene())
    rays = coincident_rays(trx)
    first = {}
    for sem in (0, 3):   # (tie: the last accepted wins / the first accepted wins)
        want, _ = f.osc.trace_rays(rays, sem=sem)
        tb = bits(want["t"])
        assert (tb == 0x80000000).sum() >= 8 and (tb == 0).sum() >= 8, "the rays do not produce hits at -0.0 and +0.0"
        first[sem] = want["prim"].copy()
        rays_checked(trx, f.sc, rays, want, sem, "coincident triangles")
    assert (first[0] != first[3]).sum() >= 32, "the two tie rules do not pick different copies"
    f.close()


def nested_scene():
    """adversarial_scenes.nested_triangles at ratio 1.3: sixteen triangles round one centre, 1e-3 to 0.05 across."""
    import adversarial_scenes as A
    return A.nested_triangles(16, ratio=1.3)


def test_lanes_with_0_1_2_3_and_many_triangles(trx, orc):
    """A 16 x 16 frame over sixteen nested triangles: the middle rays pierce all of them - a handful of lanes with 7 to 16
    triangles beside lanes with none, the cooperative rounds' shape - and the rays further out pierce 3, 2, 1 and 0."""
    verts = nested_scene()
    f = Walk.built(trx, orc, verts)
    w = h = 16
    raw = camera_view(trx, (0.004, 0.003, 1.0), (0.0, 0.0, 0.0), 7.5, w, h)
    rays = f.osc.primary_rays(f.orc.view_from_bytes(raw), w, h)
    o, d = rays["origin"].astype(np.float64), rays["direction"].astype(np.float64)
    tz = -o[:, 2] / d[:, 2]
    px, py = o[:, 0] + tz * d[:, 0], o[:, 1] + tz * d[:, 1]
    s = verts[:, 3].astype(np.float64)   # triangle k: (-s, -s), (s, -s), (0, s)
    inside = (py[:, None] >= -s) & (py[:, None] <= s) & (np.abs(px[:, None]) <= (s - py[:, None]) / 2)
    pierced = inside.sum(axis=1)
    assert {0, 1, 2, 3} <= set(pierced.tolist()) and (pierced >= 7).sum() >= 2, sorted(set(pierced.tolist()))
    for sem in (0, 3, 4):
        want, st = f.check(raw, w, h, sem, "nested triangles sem %d" % sem)
        assert st.n_tri >= int(pierced.sum())
    # ... and the same lanes under explicit rays (the plain walk of the ray pass: refills, thin waves)
    want_r, _ = f.osc.trace_rays(rays, sem=3)
    rays_checked(trx, f.sc, rays, want_r, 3, "nested triangles, rays")
    f.close()


@pytest.mark.parametrize("depth", [13, 40, 64])
def test_deep_chains_under_primary_rays(trx, orc, depth):
    """One 8 x 8 tile looking down a chain: every lane's stack passes the 12 LDS entries (13), lives mostly in HBM (40) and
    fills the last entry (64); a second tile looks the other way and stays shallow."""
    nodes, tris = deep_chain_scene(depth)
    f = Walk(trx, orc, nodes, tris)
    for eye, look in (((0.3, 0.3, 1.0), (0.3, 0.3, 0.0)), ((0.3, 0.3, -100.0), (0.3, 0.3, 0.0))):
        raw = camera_view(trx, eye, look, 2.0 if eye[2] > 0 else 0.02, 8, 8)
        want, st = f.check(raw, 8, 8, 0, "chain %d from z = %g" % (depth, eye[2]))
        assert (want["prim"] != MISS).all()
        if eye[2] > 0:
            assert st.max_stack == depth - 1
    f.close()


def test_stack_overflow_under_primary_rays_is_reported(trx, orc):
    nodes, tris = deep_chain_scene(70)
    f = Walk(trx, orc, nodes, tris)
    raw = camera_view(trx, (0.3, 0.3, 1.0), (0.3, 0.3, 0.0), 2.0, 8, 8)
    assert f.want(raw, 8, 8, 0)[1].overflow > 0
    with pytest.raises(trx.TrxError) as e:
        f.sc.trace_primary(view_of(raw), 8, 8, sem=0)
    assert e.value.code == -4 and "overflowed" in str(e.value)
    back = camera_view(trx, (0.3, 0.3, -100.0), (0.3, 0.3, 0.0), 0.02, 8, 8)   # the scene stays usable
    f.check(back, 8, 8, 0, "after the overflow")
    f.close()


def one_pixel_cluster(trx, orc, raw, w, h, pixel, n=48):
    """n small triangles in the plane z = 0 round the point where the ray of `pixel` meets it, the cluster a third of a pixel
    across: a tree two levels deep that one ray of the frame enters."""
    any_scene = orc.Scene.from_flat(trx.flat_build(np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], dtype=np.float32), [1]))
    rays = any_scene.primary_rays(orc.view_from_bytes(raw), w, h)
    o, d = rays["origin"][pixel].astype(np.float64), rays["direction"][pixel].astype(np.float64)
    d1 = rays["direction"][pixel + 1].astype(np.float64)
    p = o - o[2] / d[2] * d
    pitch = float(np.linalg.norm((o - o[2] / d1[2] * d1) - p))
    rng = np.random.default_rng(9)
    centre = p + np.concatenate([rng.uniform(-0.15, 0.15, size=(n, 2)) * pitch, np.zeros((n, 1))], axis=1)
    centre[0] = p
    tri = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0]]) * (0.05 * pitch)
    return (centre[:, None, :] + tri[None, :, :]).reshape(n, 9).astype(np.float32)


def test_rays_of_a_tile_finish_together_and_alone(trx, orc):
    """One 8 x 8 tile over a cluster of small triangles under ONE pixel.  Looking away: 64 rays miss every child of the root -
    every lane finishes in the same trip.  Looking at it: 63 rays finish in the first trip, one goes on through the
    cluster's nodes and finishes in a trip of its own."""
    w = h = 8
    raw = camera_view(trx, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 50.0, w, h)
    f = Walk.built(trx, orc, one_pixel_cluster(trx, orc, raw, w, h, 27))
    assert f.flat.n_nodes >= 3
    want, st = f.check(raw, w, h, 3, "one ray goes on")
    assert (want["prim"] != MISS).sum() == 1 and want["prim"][27] != MISS and st.n_node > w * h + 1
    away = camera_view(trx, (0.0, 0.0, 1.0), (0.0, 0.0, 2.0), 50.0, w, h)
    want, st = f.check(away, w, h, 3, "every ray misses")
    assert (want["prim"] == MISS).all() and st.n_node == w * h
    f.close()


def test_rays_any_hit_and_ao_on_a_small_scene(trx, orc):
    """kitchen-class, 4 000 triangles: small enough for the plain walk in every mode (asserted)."""
    w, h = 40, 24
    flat, view, osc, ov = make_scene(trx, orc, "kitchen", 4000, w, h)
    sc = trx.Scene(flat)
    for mode in (trx.MODE_AO, trx.MODE_RAYS, trx.MODE_PRIMARY):
        assert sc.walk_kind(mode) == trx.WALK_PLAIN
    rays = random_rays(trx, flat, 3000, 21)
    for sem in (0, 3):
        want, _ = osc.trace_rays(rays, sem=sem)
        rays_checked(trx, sc, rays, want, sem, "kitchen rays")
        flags, _ = sc.trace_occluded(rays, sem=sem)
        assert (flags.astype(bool) == (want["prim"] != MISS)).all(), sem
        assert 0.02 < (want["prim"] != MISS).mean() < 0.99
        op, _ = osc.trace_primary(ov, w, h, sem=sem)
        oao, _ = osc.trace_ao(ov, w, h, op, sem=sem, frame=2, ao_eps=0.01)
        pp = PoisonedFrames(w * h, tile_of=image_tile_of(w, h), what="kitchen primary")
        pa = PoisonedFrames(w * h, tile_of=image_tile_of(w, h), what="kitchen ao")
        ep, ea = pp.expect(op), pa.expect(oao)
        pp.poison()
        pa.poison()
        sc.trace_primary_dev(view, w, h, pp.ptr, sem=sem)
        sc.trace_ao_dev(view, w, h, pp.ptr, pa.ptr, sem=sem, frame=2, ao_eps=0.01)
        pp.check(ep, sem)
        pa.check(ea, sem)
    sc.close()


def test_counting_kernel_totals(goldens, trx):
    """The counting primary kernel compiles from the same text: node steps, triangle tests, hits and the deepest stack of the
    64 x 48 Cornell frame are the oracle's."""
    f = goldens("cornell_64")
    w, h = 64, 48
    raw = cornell_view(trx, w, h)
    for sem in (0, 3):
        _, ost = f.want(raw, w, h, sem)
        st = f.sc.count_primary(view_of(raw), w, h, sem=sem)
        assert (int(st.n_rays), int(st.n_node), int(st.n_tri), int(st.n_hits), int(st.max_stack), int(st.overflow)) == (
            w * h, ost.n_node, ost.n_tri, ost.n_hits, ost.max_stack, 0), sem
