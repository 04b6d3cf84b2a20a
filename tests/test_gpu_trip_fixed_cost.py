"""The plain walk's per-trip fixed cost (trace_walk_plain.inc): the node a lane steps to next is worked out once per trip, for
the look, the wave-uniform step and the per-lane step; the uniform step loads the node's first quarter in every lane, ray or
no ray; its exponent words are formed by the scalar unit; node_intersect_kept broadcasts its six frame operands.  None of that
may show in a record: every case compares t bit for bit and prim exactly against the oracle.  Run with `-m gpu` on an MI355X.

The shapes are the smallest at which these paths can go wrong:
  * one 8 x 8 tile of the Cornell-class golden scene - a single wave whose first trips are all uniform, packet test on - and
    64 x 48 (48 tiles);
  * 52 x 44 on the soup golden: neither side a multiple of 8, so uniform steps run with lanes that hold no ray, and those
    lanes load the record too;
  * all eight semantics words on the Cornell frame: both node-test arithmetics, both tie rules, and the literal divisions
    with their shortcut levels (whose exponent words now come from the scalar unit as well - the same floats);
  * a two-level golden: absolute node indices (bvh_off) and lanes that hold a parked triangle group in the shared index
    computation;
  * cameras on a node's origin, one ulp beside it and on a child plane, and axis-aligned views whose rays have a zero
    direction component (tests/hostile_inputs.py): plane bounds of the packet test that are not finite;
  * the counting kernels walk the same text: their totals over the 64 x 48 frame are the oracle's n_node and n_tri."""
import ctypes as C
import os

import numpy as np
import pytest

import hostile_inputs as H
from helpers import ALL_SEMS, assert_hits_equal, golden_inputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def need_gpu(trx):
    lib = trx.load()
    assert lib.trx_device_count() > 0, "no HIP device visible to libtrx.so"
    buf = C.create_string_buffer(64)
    lib.trx_device_name(0, buf, 64)
    assert buf.value.startswith(b"gfx950"), buf.value


class Fixture:
    """A golden fixture's scene on the device and in the oracle; the oracle's frames computed once per (view, size, sem)."""

    def __init__(self, trx, orc, name):
        self.trx, self.orc = trx, orc
        self.g = np.load(os.path.join(GOLDEN, name + ".npz"))
        nodes, tri_verts, inst, tlas_start = golden_inputs(trx, self.g)
        n = tri_verts.shape[0]
        self.flat = trx.FlatScene(nodes, tri_verts, inst, tlas_start, np.arange(n), [0, n])
        self.osc = orc.Scene(nodes, tri_verts, inst, tlas_start)
        self.sc = trx.Scene(self.flat)
        self.w, self.h = int(self.g["width"]), int(self.g["height"])
        self.raw = self.g["view"].tobytes()
        self._frames = {}

    def view(self, raw):
        from tray_racing_amd import _lib
        return _lib.View.from_buffer_copy(raw)

    def want(self, raw, w, h, sem):
        key = (raw, w, h, sem)
        if key not in self._frames:
            self._frames[key] = self.osc.trace_primary(self.orc.view_from_bytes(raw), w, h, sem=sem, threads=2)
            assert self._frames[key][1].overflow == 0
        return self._frames[key]

    def check(self, raw, w, h, sem, what):
        want, st = self.want(raw, w, h, sem)
        got, _ = self.sc.trace_primary(self.view(raw), w, h, sem=sem)
        assert_hits_equal(got, want, what)
        return want, st


@pytest.fixture(scope="module")
def fixtures(trx, orc):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Fixture(trx, orc, name)
        return made[name]
    yield get
    for f in made.values():
        f.sc.close()


def cornell_view(trx, w, h, fov=None):
    eye, look, f = trx.scene_camera("cornell")
    return bytes(trx.view_from_camera(eye, look, f if fov is None else fov, w, h))


@pytest.mark.parametrize("w,h,fov", [(8, 8, 12.0), (8, 8, None), (64, 48, None)])
def test_cornell_one_tile_and_48_tiles(fixtures, trx, w, h, fov):
    """8 x 8 under a narrow field of view: one wave, one octant, every early trip uniform with the packet test on; 8 x 8
    under the scene's own; 64 x 48.  Both presets."""
    f = fixtures("cornell_64")
    raw = cornell_view(trx, w, h, fov)
    for sem in (0, 3):
        want, _ = f.check(raw, w, h, sem, "cornell %dx%d fov %s sem %d" % (w, h, fov, sem))
        assert (want["prim"] != 0xFFFFFFFF).sum() > w * h // 2


def test_soup_partially_filled_waves(fixtures):
    """52 x 44: the last column and row of tiles hold 4 x 8, 8 x 4 and 4 x 4 rays; the fixture's own view, all eight words."""
    f = fixtures("soup_52x44")
    assert (f.w, f.h) == (52, 44)
    for sem in ALL_SEMS:
        want, _ = f.check(f.raw, f.w, f.h, sem, "soup 52x44 sem %d" % sem)
    assert 0 < (want["prim"] != 0xFFFFFFFF).sum() < f.w * f.h


@pytest.mark.parametrize("sem", ALL_SEMS)
def test_cornell_every_semantics_word(fixtures, trx, sem):
    f = fixtures("cornell_64")
    f.check(cornell_view(trx, 64, 48), 64, 48, sem, "cornell 64x48 sem %d" % sem)


def test_two_level_golden(fixtures):
    """cornell_tlas_48: bvh_off in the shared index, lanes with a parked triangle group beside lanes with a node group."""
    f = fixtures("cornell_tlas_48")
    assert f.flat.has_tlas
    for sem in ALL_SEMS:
        want, _ = f.check(f.raw, f.w, f.h, sem, "cornell_tlas_48 sem %d" % sem)
    assert (want["prim"] != 0xFFFFFFFF).sum() > f.w * f.h // 4


@pytest.mark.parametrize("name", ["cornell_64", "cornell_tlas_48"])
def test_cameras_on_node_boundaries_and_zero_direction_components(fixtures, trx, name):
    """hostile_inputs.hostile_views at 16 x 16: the eye on a node's origin, one ulp to either side, on a child plane (zero and
    sign-changing plane distances, the packet test's bounds not finite where 0 meets an infinite 1/d end) and the four
    axis-aligned views (a tile whose rays have a zero direction component, or a rounding residue beside it)."""
    f = fixtures(name)
    w = h = 16
    views = [(n, raw) for n, raw in H.hostile_views(trx, f.flat, w, h) if any(k in n for k in ("eye_node_p", "eye_child_plane", "axis+", "axis-"))]
    assert len(views) == 8, [n for n, _ in views]
    for vname, raw in views:
        assert H.is_alive(vname)
        for sem in (0, 3, 4):
            f.check(raw, w, h, sem, "%s %s sem %d" % (name, vname, sem))


def test_counting_kernels_count_where_they_counted(fixtures, trx):
    """The counting primary kernel compiles from the same walk (without the look): node steps and triangle tests of the
    64 x 48 Cornell frame are the oracle's, ray by ray and in total."""
    import heat_twin as HT
    import torch
    f = fixtures("cornell_64")
    w, h = 64, 48
    raw = cornell_view(trx, w, h)
    for sem in (0, 3):
        want, ost = f.want(raw, w, h, sem)
        st = f.sc.count_primary(f.view(raw), w, h, sem=sem)
        assert (int(st.n_rays), int(st.n_node), int(st.n_tri), int(st.n_hits), int(st.max_stack), int(st.overflow)) == (
            w * h, ost.n_node, ost.n_tri, ost.n_hits, ost.max_stack, 0), sem
        d_cost = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        f.sc.count_primary_per_ray(f.view(raw), w, h, d_cost.data_ptr(), 0, sem=sem)
        per_ray = d_cost.cpu().numpy().view(HT.COST_DTYPE)
        assert (per_ray == HT.primary_cost(f.osc, f.orc.view_from_bytes(raw), w, h, sem)).all(), sem
        assert (int(per_ray["n_node"].sum(dtype=np.int64)), int(per_ray["n_tri"].sum(dtype=np.int64))) == (ost.n_node, ost.n_tri)
