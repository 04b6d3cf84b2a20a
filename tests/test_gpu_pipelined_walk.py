"""The pipelined walk (trace_walk_pipe.inc) at small shapes.  The library takes it for single-level scenes past a size
threshold, in every mode but the primary pass and the ray service (api_launch.cpp, pipelined_walk); helpers.padded_flat
pushes a small scene past that threshold with unreferenced zero triangles, so the oracle's answers for the small scene hold
for its twin - and each test here asks the library itself which walk it launches (Scene.walk_kind) rather than doing the
size arithmetic.  What has a home elsewhere runs there, on cases named *_pipe (test_gpu_parity.py, test_gpu_hostile_inputs.py,
test_gpu_ao_visibility.py, test_gpu_ao_sparse.py); here: the scheduling variants, the counting kernels, a refit, and the
boundary of the decision.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

import heat_twin
import hostile_inputs as H
from helpers import (ALL_SEMS, assert_hits_equal, assert_walk_kinds, deep_chain_scene, make_scene, padded_flat, padded_records,
                     random_rays)

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT = 72, 48
N_RAYS = 4096


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _six(st):
    return (int(st.n_rays), int(st.n_node), int(st.n_tri), int(st.n_hits), int(st.max_stack), int(st.overflow))


def _modes(trx):
    return (trx.MODE_PRIMARY, trx.MODE_AO, trx.MODE_RAYS, trx.MODE_FUSED, trx.MODE_SERVICE)


@pytest.fixture(scope="module")
def kitchen(trx, orc):
    """A kitchen-class scene of 20 000 triangles on the device twice - as it is and padded - and on the oracle once."""
    flat, view, osc, ov = make_scene(trx, orc, "kitchen", 20000, WIDTH, HEIGHT)
    plain, twin = trx.Scene(flat), trx.Scene(padded_flat(trx, flat))
    case = type("Kitchen", (), {"flat": flat, "view": view, "osc": osc, "ov": ov, "plain": plain, "twin": twin})
    yield case
    trx.load().trx_set_kernel_variant(0)
    plain.close()
    twin.close()


# ---- scheduling --------------------------------------------------------------------------------------------------------

VARIANTS = (0, 1 << 16, 2 << 16, 4 << 16, 1 << 28, 1 << 28 | 1 << 16, 7 << 25, 3 << 25, 7 << 29, 1, 64)


def test_scheduling_variants_do_not_change_the_pipelined_walks_results(trx, orc, kitchen):
    """Waves per workgroup 1, 2 and 4 (1 and 4: no drain hand-over), thin waves off, triangle compaction never and at three,
    always-cooperative triangle rounds, refill thresholds 1 and 64: under each, three times over, the AO records of a
    72 x 48 frame and 4096 explicit rays on the padded twin are the oracle's, under TRX_SEM_HLSL and the CPU preset."""
    c = kitchen
    lib = trx.load()
    for mode in (trx.MODE_AO, trx.MODE_RAYS):
        assert_walk_kinds(trx, c.plain, c.twin, mode)
    rays = random_rays(trx, c.flat, N_RAYS, 23)
    want = {}
    for sem in (0, 3):
        op, _ = c.osc.trace_primary(c.ov, WIDTH, HEIGHT, sem=sem)
        want[sem] = (op, c.osc.trace_ao(c.ov, WIDTH, HEIGHT, op, sem=sem, frame=1, ao_eps=0.01)[0], c.osc.trace_rays(rays, sem=sem)[0])
        assert (want[sem][1]["prim"] != trx.MISS_PRIM).sum() > 100 and (want[sem][2]["prim"] != trx.MISS_PRIM).sum() > 100
    try:
        for variant in VARIANTS:
            lib.trx_set_kernel_variant(variant)
            for rep in range(3):
                for sem in (0, 3):
                    what = "variant 0x%x, repetition %d, sem %d" % (variant, rep, sem)
                    gp, gao, _ = c.twin.trace_primary_ao(c.view, WIDTH, HEIGHT, sem=sem, frame=1, ao_eps=0.01)
                    assert_hits_equal(gp, want[sem][0], what + ", primary")
                    assert_hits_equal(gao, want[sem][1], what + ", ao")
                    assert_hits_equal(c.twin.trace_rays(rays, sem=sem)[0], want[sem][2], what + ", rays")
    finally:
        lib.trx_set_kernel_variant(0)


# ---- counting ----------------------------------------------------------------------------------------------------------

def test_counting_kernels_of_both_walks_count_what_the_oracle_counts(trx, orc, kitchen):
    """trx_count_rays and trx_count_rays_per_ray over 4096 rays, half of them hostile (tests/hostile_inputs.py), under
    semantics 0, 3 and 4, on the padded twin (the pipelined walk's counting twins) and on the scene itself (the plain
    walk's): the six counters are the oracle's, every ray's {n_node, n_tri} is the oracle's walk of that ray alone, and the
    hit records are the oracle's and, element for element, those of the launch that does not count."""
    import torch
    from tray_racing_amd import dist as D
    c = kitchen
    assert_walk_kinds(trx, c.plain, c.twin, trx.MODE_RAYS)
    rays, classes = H.hostile_rays(trx, c.flat, N_RAYS, 5)
    assert (classes != H.TAME).sum() >= N_RAYS // 2 - 1
    d_rays = _dev(rays)
    for sem in (0, 3, 4):
        want, ost = c.osc.trace_rays(rays, sem=sem, threads=8)
        assert ost.overflow == 0 and ost.n_hits > N_RAYS // 8
        want_cost = heat_twin.rays_cost(c.osc, rays, sem)
        assert (int(want_cost["n_node"].sum(dtype=np.int64)), int(want_cost["n_tri"].sum(dtype=np.int64))) == (int(ost.n_node), int(ost.n_tri))
        for leg, sc in (("plain walk", c.plain), ("pipelined walk", c.twin)):
            what = "sem %d, %s" % (sem, leg)
            d_hits, d_each, d_ref = (torch.full((N_RAYS,), -1, dtype=torch.int64, device="cuda") for _ in range(3))
            d_cost = torch.full((N_RAYS,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            st = sc.count_rays(d_rays.data_ptr(), N_RAYS, d_hits.data_ptr(), sem=sem)
            assert _six(st) == _six(ost), "%s, trx_count_rays: %s, the oracle %s" % (what, _six(st), _six(ost))
            st = sc.count_rays_per_ray(d_rays.data_ptr(), N_RAYS, d_cost.data_ptr(), d_each.data_ptr(), sem=sem)
            assert _six(st) == _six(ost), "%s, trx_count_rays_per_ray: %s, the oracle %s" % (what, _six(st), _six(ost))
            got = d_cost.cpu().numpy().view(heat_twin.COST_DTYPE)
            bad = np.flatnonzero(got != want_cost)
            assert bad.size == 0, "%s: %d per-ray records differ, first ray %d (%s): gpu %s oracle %s" % (
                what, bad.size, bad[0], classes[bad[0]], got[bad[0]], want_cost[bad[0]])
            sc.trace_rays_dev(d_rays.data_ptr(), N_RAYS, d_ref.data_ptr(), sem=sem)
            sc.check()
            assert torch.equal(d_hits, d_ref) and torch.equal(d_each, d_ref), what + ": a counting launch's records differ from the trace's"
            assert_hits_equal(D.int64_to_hits(d_ref), want, what)


# ---- refit -------------------------------------------------------------------------------------------------------------

def test_a_refitted_padded_scene_still_takes_the_pipelined_walk_and_equals_the_oracle(trx, orc):
    """trx_scene_refit of a padded soup of 2500 triangles: jittered vertices for the real records, zeros for the padding.
    The node bytes are the host twin's over the unpadded scene, the scene still takes the pipelined walk, and an AO frame
    and 4096 rays equal the oracle over those nodes and the new vertices."""
    w, h = 52, 44
    flat, view, _osc, ov = make_scene(trx, orc, "soup", 2500, w, h)
    pf = padded_flat(trx, flat)
    plain, sc = trx.Scene(flat), trx.Scene(pf)
    try:
        for mode in (trx.MODE_AO, trx.MODE_RAYS):
            assert_walk_kinds(trx, plain, sc, mode)
        rng = np.random.default_rng(9)
        v = flat.tri_verts.astype(np.float64)
        size = float(np.linalg.norm(v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0)))
        moved = (v + rng.normal(scale=0.01 * size, size=v.shape)).astype(np.float32)
        sc.refit(padded_records(pf, moved))
        nodes = trx.refit_nodes(flat, moved)
        assert not np.array_equal(nodes, flat.nodes) and np.array_equal(sc.read_nodes(), nodes)
        for mode in (trx.MODE_AO, trx.MODE_RAYS, trx.MODE_FUSED):
            assert sc.walk_kind(mode) == trx.WALK_PIPELINED
        osc = orc.Scene(nodes, moved)
        rays = random_rays(trx, type("F", (), {"tri_verts": moved}), N_RAYS, 31)
        for sem in (0, 3):
            op, st = osc.trace_primary(ov, w, h, sem=sem)
            assert st.n_hits > w * h // 20
            gp, gao, _ = sc.trace_primary_ao(view, w, h, sem=sem, frame=1, ao_eps=0.01)
            assert_hits_equal(gp, op, "refitted twin, primary sem %d" % sem)
            assert_hits_equal(gao, osc.trace_ao(ov, w, h, op, sem=sem, frame=1, ao_eps=0.01)[0], "refitted twin, ao sem %d" % sem)
        for sem in ALL_SEMS:
            want, _ = osc.trace_rays(rays, sem=sem)
            assert_hits_equal(sc.trace_rays(rays, sem=sem)[0], want, "refitted twin, rays sem %d" % sem)
            assert (want["prim"] != trx.MISS_PRIM).sum() > 100
    finally:
        plain.close()
        sc.close()


# ---- the boundary ------------------------------------------------------------------------------------------------------

def test_the_walk_changes_one_triangle_past_32_mib_and_never_on_two_level_scenes(trx, orc):
    """One 80-byte node and 699 049 48-byte triangle records are 32 MiB exactly: the plain walk; one record more: the
    pipelined walk in the AO, rays and one-launch-frame modes, the plain walk for the primary pass and the ray service.
    padded_flat stops at that record.  A two-level scene takes the plain walk in every mode whatever its size, and
    padded_flat refuses it."""
    nodes, tris = deep_chain_scene(1)
    assert nodes.shape[0] == 1
    pipelined = {trx.MODE_PRIMARY: 0, trx.MODE_AO: 1, trx.MODE_RAYS: 1, trx.MODE_FUSED: 1, trx.MODE_SERVICE: 0}
    ray = np.zeros(1, dtype=trx.RAY_DTYPE)
    ray["origin"], ray["direction"], ray["tmax"] = (0.3, 0.3, 1), (0, 0, -1), 3.0e38
    for n, past in ((699049, False), (699050, True)):
        verts = np.zeros((n, 9), dtype=np.float32)
        verts[:1] = tris
        sc = trx.Scene(trx.FlatScene(nodes, verts, [], 0, np.arange(1), [0, 1]))
        try:
            assert {m: sc.walk_kind(m) for m in _modes(trx)} == {m: (k if past else 0) for m, k in pipelined.items()}, n
            got, _ = sc.trace_rays(ray, sem=0)
            assert got["t"][0] == 1.0 and got["prim"][0] == 0
        finally:
            sc.close()
    one = trx.FlatScene(nodes, tris, [], 0, np.arange(1), [0, 1])
    assert padded_flat(trx, one).n_tris == 699050
    with pytest.raises(trx.TrxError):
        sc = trx.Scene(one)
        try:
            sc.walk_kind(5)
        finally:
            sc.close()
    for tris_in in (0, 20000):
        flat, _view, _osc, _ov = make_scene(trx, orc, "cornell" if tris_in == 0 else "kitchen", tris_in, 16, 16, tlas=True)
        with pytest.raises(ValueError):
            padded_flat(trx, flat)
        big = np.zeros((max(flat.n_tris, 800000 if tris_in else 0), 9), dtype=np.float32)   # the larger one: 38 MB of records
        big[:flat.n_tris] = flat.tri_verts
        sc = trx.Scene(trx.FlatScene(flat.nodes, big, flat.instance_offsets, flat.tlas_start, flat.tri_source, flat.blas_tri_start,
                                     instance_source=flat.instance_source, instance_transforms=flat.instance_transforms,
                                     instance_entry=flat.instance_entry))
        try:
            assert [sc.walk_kind(m) for m in _modes(trx)] == [0] * 5, "a two-level scene of %d triangle records" % big.shape[0]
        finally:
            sc.close()
