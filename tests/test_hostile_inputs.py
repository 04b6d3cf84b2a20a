"""The oracle on hostile rays, cameras and instance transforms (tests/hostile_inputs.py), CPU only: before such inputs go to
the device (tests/test_gpu_hostile_inputs.py, bit-exact against the oracle) the oracle has to walk them cleanly and be
right about them - checked against its own BVH-independent brute-force query.

Walk and brute force agree bit for bit except where the shader's max(box entry, 0.0001) clamp (query.hlsl node test) hides
a hit from the walk.  The exclusion rule is stated, not fitted: a ray is excluded when its brute-force hit has t < 2e-4
(twice the clamp: the box of a hit at t is entered no later than t, and its planes carry the quantisation's rounding) or
when its tmin is negative.  The three classes built to trigger the clamp are pinned; every other class may lose at most
1 % of its rays to the rule."""
import numpy as np
import pytest

import hostile_inputs as H
from helpers import ALL_SEMS, aimed_rays, bits, deep_chain_scene, instanced_scene, make_scene, w2o_rows

MISS = 0xFFFFFFFF
N_RAYS = 8192          # 4096 hostile rays, 128 of every class: 1 % of a class is one ray
T_RULE = np.float32(2e-4)


@pytest.fixture(scope="module")
def scenes(trx, orc):
    """name -> (flat, oracle scene, hostile rays, their classes): built once, never modified."""
    out = {}
    for name, tris in (("cornell", 0), ("kitchen", 20000)):
        flat, _view, osc, _ov = make_scene(trx, orc, name, tris, 16, 16)
        out[name] = (flat, osc) + H.hostile_rays(trx, flat, N_RAYS, 5)
    nodes, tris = deep_chain_scene(20)
    flat = trx.FlatScene(nodes, tris, [], 0, np.arange(20), [0, 20])
    out["chain20"] = (flat, orc.Scene(nodes, tris)) + H.hostile_rays(trx, flat, N_RAYS, 5)
    return out


def excluded_by_rule(rays, brute):
    with np.errstate(invalid="ignore"):
        return brute["t"] < T_RULE, rays["tmin"] < 0


@pytest.mark.parametrize("sem", [0, 3])
@pytest.mark.parametrize("name", ["cornell", "kitchen", "chain20"])
def test_the_walk_equals_brute_force_except_where_the_entry_clamp_hides_a_hit(scenes, name, sem):
    _flat, osc, rays, cls = scenes[name]
    walk, st = osc.trace_rays(rays, sem=sem)
    brute = osc.brute_rays(rays, sem=sem)
    assert st.overflow == 0 and not np.isnan(walk["t"]).any()
    miss = walk["prim"] == MISS
    assert np.isposinf(walk["t"][miss]).all() and np.isfinite(walk["t"][~miss]).all()
    near, neg_tmin = excluded_by_rule(rays, brute)
    differs = bits(walk["t"]) != bits(brute["t"])
    print("%s sem %d: %d rays, %d differ, excluded by t < 2e-4 per class:" % (name, sem, rays.shape[0], differs.sum()))
    for c in (H.TAME,) + H.RAY_CLASSES:
        m = cls == c
        print("  %-18s %5d rays  %4d excluded  %4d differ" % (c, m.sum(), (near & m).sum(), (differs & m).sum()))
    # (the overflow class has its own pin below; the rule for every other ray is the one stated above)
    tiny = np.isin(cls, H.OVERFLOW_DIR)
    bad = np.flatnonzero(differs & ~near & ~neg_tmin & ~tiny)
    assert bad.size == 0, "walk != brute force outside the rule: rays %s of classes %s" % (bad[:8], cls[bad[:8]])
    # the clamp's three behaviours, pinned
    for family in (H.CLAMP_TMIN, H.CLAMP_PLANE, H.CLAMP_DIR):
        assert (differs & np.isin(cls, family)).any(), family
    for c in ("tmin_neg", "origin_on_plane", "dscale_2^12", "dscale_2^40"):
        assert (differs & (cls == c)).any(), c
    assert (walk["prim"][cls == "dscale_2^40"] == MISS).all() and (brute["prim"][cls == "dscale_2^40"] != MISS).any()
    # a direction of length 1e-38: where walk and brute force differ, the walk has no hit and brute force has one at a t
    # whose box planes (up to 255 x as far) are beyond the largest float
    with np.errstate(invalid="ignore"):
        assert (walk["prim"][tiny & differs] == MISS).all() and (brute["t"][tiny & differs] > 3.4028234663852886e38 / 256).all()
    if name == "kitchen":      # (the scene large enough for hits that far: the behaviour is there, not only allowed)
        assert (tiny & differs).any() and (brute["prim"][tiny] != MISS).sum() > (walk["prim"][tiny] != MISS).sum()
    # ... and nothing else leans on the rule
    for c in (H.TAME,) + H.RAY_CLASSES:
        if c in H.CLAMP_TMIN + H.CLAMP_PLANE + H.CLAMP_DIR:
            continue
        m = cls == c
        assert (near & m).sum() <= 0.01 * m.sum(), (c, int((near & m).sum()), int(m.sum()))


@pytest.mark.parametrize("name", ["cornell", "kitchen", "chain20"])
def test_simd_and_scalar_node_tests_walk_hostile_rays_alike(orc, scenes, name):
    """The AVX2 node test against the scalar one on whole walks of the hostile set (NaN planes, infinite reciprocals,
    0 x inf): hits and the node and triangle counts, under all eight semantics."""
    if not orc.set_simd(True):
        orc.set_simd(False)
        pytest.skip("this CPU has no AVX2 + FMA")
    _flat, osc, rays, _cls = scenes[name]
    try:
        for sem in ALL_SEMS:
            orc.set_simd(False)
            want, wst = osc.trace_rays(rays, sem=sem)
            orc.set_simd(True)
            got, gst = osc.trace_rays(rays, sem=sem)
            assert (bits(got["t"]) == bits(want["t"])).all() and (got["prim"] == want["prim"]).all(), sem
            assert (gst.n_node, gst.n_tri, gst.n_hits, gst.overflow) == (wst.n_node, wst.n_tri, wst.n_hits, 0), sem
    finally:
        orc.set_simd(False)


@pytest.fixture(scope="module")
def hostile_instances(trx, orc):
    mats, mcls = H.hostile_affines(np.random.default_rng(7), 16)
    flat, o2w, world, first, _blas_of = instanced_scene(trx, n_objects=3, tris_per_object=300, matrices=mats)
    w2o = np.stack([w2o_rows(m) for m in o2w])
    osc = orc.Scene(flat.nodes, flat.tri_verts, flat.instance_offsets, flat.tlas_start, instance_w2o=w2o)
    return flat, osc, world, first, mcls[flat.instance_source]


# Object-space direction lengths: the inverse of the instance's linear part scales the (unit) world direction, and the
# BLAS walk does not renormalise it.  2^12 and about 1e6 (the shear's inverse) are CLAMP_DIR inputs to that walk;
# 2^10 on one axis is at the edge (1 / 2^10 of a unit-size object's distances is about the clamp).
LOSING = ("scale_2^-12", "near_singular_shear")
EXACT = ("identity", "mirror", "rot90", "scale_2^12")


@pytest.mark.parametrize("sem", [0, 3])
def test_instance_walk_against_brute_force_over_world_space_triangles(trx, hostile_instances, sem):
    """trace_rays_inst over hostile_affines against brute force on the world-space copies (t in world units).  The two
    round differently (the ray goes to object space; the triangles went to world space), so the benign classes are held
    to the bounds tests/test_instances.py holds tame transforms to; the classes that hand the BLAS walk a direction of
    2^12 or more lose near hits, as the reference does - pinned.  translate_1e6 has object-size detail below the float
    spacing at its coordinates (0.0625): only a clean walk is asked of it."""
    _flat, osc, world, first, cls_k = hostile_instances
    lost = {c: 0 for c in LOSING}
    for k, c in enumerate(cls_k):
        rays = aimed_rays(trx, world[first[k]:first[k + 1]], 400, 100 + k)
        walk, inst, st = osc.trace_rays_inst(rays, sem=sem)
        assert st.overflow == 0 and not np.isnan(walk["t"]).any()
        brute = osc.brute_rays_over(world, rays, sem=sem)
        near, neg_tmin = excluded_by_rule(rays, brute)
        bhit = (brute["prim"] != MISS) & ~near & ~neg_tmin
        binst = np.searchsorted(first, brute["prim"], side="right") - 1
        mine = bhit & (binst == k)
        if c in EXACT:
            assert mine.sum() > 200
            same = mine & (walk["prim"] != MISS) & (inst == k)
            assert same.sum() >= 0.99 * mine.sum(), (c, int(same.sum()), int(mine.sum()))
            rel = np.abs(walk["t"][same] - brute["t"][same]) / brute["t"][same]
            assert np.median(rel) < 2e-6 and np.quantile(rel, 0.99) < 1e-4, (c, float(np.median(rel)), float(np.quantile(rel, 0.99)))
        elif c in LOSING:
            lost[c] += int((mine & ((walk["prim"] == MISS) | (inst != k))).sum())
    print("sem %d: near hits lost inside instances whose object-space direction is >= 2^12: %s" % (sem, lost))
    assert all(v > 0 for v in lost.values()), lost


def test_simd_and_scalar_agree_through_hostile_instances(trx, orc, hostile_instances):
    if not orc.set_simd(True):
        orc.set_simd(False)
        pytest.skip("this CPU has no AVX2 + FMA")
    flat, osc, world, _first, _cls_k = hostile_instances
    benign = world[np.abs(world).max(axis=1) < 1e4]          # (aim at the instances near the origin; the far ones are hit by chance)
    rays, _cls = H.hostile_rays(trx, flat, 4096, 9, tri_verts=benign)
    try:
        for sem in ALL_SEMS:
            orc.set_simd(False)
            want, winst, wst = osc.trace_rays_inst(rays, sem=sem)
            orc.set_simd(True)
            got, ginst, gst = osc.trace_rays_inst(rays, sem=sem)
            assert (bits(got["t"]) == bits(want["t"])).all() and (got["prim"] == want["prim"]).all() and (ginst == winst).all(), sem
            assert (gst.n_node, gst.n_tri, gst.overflow) == (wst.n_node, wst.n_tri, 0) and (want["prim"] != MISS).sum() > 500, sem
    finally:
        orc.set_simd(False)


# ---- the generators themselves ------------------------------------------------------------------------------------------

def test_every_class_is_present_and_batches_are_reproducible(trx, scenes):
    for name, (flat, _osc, rays, cls) in scenes.items():
        assert set(cls) == set(H.RAY_CLASSES) | {H.TAME}, name
        again, cls2 = H.hostile_rays(trx, flat, N_RAYS, 5)
        assert again.tobytes() == rays.tobytes() and (cls == cls2).all()
        assert (cls[0::2] == H.TAME).all()                    # a tame neighbour beside every hostile ray
        small, scls = H.hostile_rays(trx, flat, 2 * len(H.RAY_CLASSES), 6)
        assert set(scls) == set(H.RAY_CLASSES) | {H.TAME}
        # what the classes say is what the rays hold
        assert np.isnan(rays["tmin"][cls == "tmin_nan"]).all() and (rays["tmin"][cls == "tmin_neg"] < 0).all()
        assert (rays["tmin"][cls == "tmin_gt_tmax"] > rays["tmax"][cls == "tmin_gt_tmax"]).all()
        assert (rays["direction"][cls == "dir_zero"] == 0).all()
        assert np.isnan(rays[cls == "nan"]["origin"]).any(axis=1).__or__(np.isnan(rays[cls == "nan"]["direction"]).any(axis=1)).all()
        node_p = flat.nodes[:, 0:3].copy().view(np.float32)
        assert all((o[:, None, :] == node_p[None, :, :]).any(axis=(1, 2)).all() for o in (rays["origin"][cls == "node_p"],))
    mats, mcls = H.hostile_affines(np.random.default_rng(1), 16)
    assert set(mcls) == set(H.AFFINE_CLASSES) and mats.shape == (16, 16)
    dets = {c: float(np.linalg.det(m.reshape(4, 4).T[:3, :3].astype(np.float64))) for m, c in zip(mats, mcls)}
    assert dets["mirror"] < 0 and 1e-7 < abs(dets["near_singular_shear"]) < 1e-5 and dets["identity"] == 1.0
    assert (mats[list(mcls).index("rot90")] == 0).sum() >= 9


def test_interleaved_and_placeholder_batches_hold_the_same_tame_rays(trx, scenes):
    flat, _osc, rays, cls = scenes["cornell"]
    tame, hostile = rays[cls == H.TAME][:300], rays[cls != H.TAME]
    a, ia = H.interleaved(trx, tame, hostile)
    b, ib = H.with_placeholders(trx, tame)
    assert a.shape == b.shape and a.shape[0] % 64 == 0 and (ia == ib).all()
    assert a[ia].tobytes() == tame.tobytes() == b[ib].tobytes()
    other = np.setdiff1d(np.arange(a.shape[0]), ia)
    assert other.size == a.shape[0] - 300
    assert all(np.isin(np.arange(r * 64, r * 64 + 64), ia).sum() == 8 for r in range(a.shape[0] // 64 - 1))   # 8 tame lanes a run
    assert len(set(int(i) % 64 for i in ia)) == 64                                                            # every lane in turn
    ph = b[other]
    pts = flat.tri_verts.reshape(-1, 3)
    assert (ph["origin"] > pts.max(0) + 1.0).all() and (ph["direction"] > 0).all() and len(set(ph.tobytes()[i:i + 32] for i in range(0, 32 * 8, 32))) == 1
    assert any(a[other].tobytes()[i * 32:(i + 1) * 32] != ph.tobytes()[:32] for i in range(8))


@pytest.mark.parametrize("w,h", [(8, 8), (16, 16), (48, 24), (33, 47)])
def test_alive_views_reach_the_packet_test_and_switched_off_views_do_not(trx, orc, scenes, w, h):
    """tile_qualifies restates the walk's `fits` condition: at least one 8 x 8 tile of every ALIVE view passes it, no tile
    of an OFF view does - and the oracle walks every one of them cleanly, equal to its brute force wherever brute force's
    hit is beyond the clamp rule."""
    for name in ("cornell", "kitchen"):
        flat, osc = scenes[name][:2]
        views = H.hostile_views(trx, flat, w, h)
        if name == "kitchen" and w * h > 256:      # (the whole-tree walkers cost 20000 triangle tests a pixel, twice)
            views = [v for v in views if not H.walks_whole_tree(v[0])]
        assert len(set(n for n, _ in views)) == len(views) and sum(H.is_alive(n) for n, _ in views) >= (16 if min(w, h) >= 16 else 11)
        for vname, raw in views:
            assert len(raw) == 160
            ov = orc.view_from_bytes(raw)
            prays = osc.primary_rays(ov, w, h)
            ok = [H.tile_qualifies(prays[t]) for t in H.tiles(w, h)]
            assert any(ok) if H.is_alive(vname) else not any(ok), (name, vname, sum(ok), len(ok))
            hits, st = osc.trace_primary(ov, w, h, sem=0)
            assert st.overflow == 0 and not np.isnan(hits["t"]).any()
            brute = osc.brute_primary(ov, w, h, sem=0)
            with np.errstate(invalid="ignore"):
                far = ~(brute["t"] < T_RULE)
            assert (bits(hits["t"])[far] == bits(brute["t"])[far]).all(), (name, vname)
            if not H.is_alive(vname):
                assert (hits["prim"] == MISS).all()


def test_a_nan_ray_walks_the_whole_tree_and_hits_nothing(trx, orc, scenes):
    """The exposure behind the hostile classes' cost, pinned: an axis with a NaN in the ray's origin or direction drops
    out of every box test (max / min drop its NaN planes), and a ray with one on all three axes - what a NaN anywhere in
    a view makes of every primary ray, through the normalisation - passes every box test (what is left is 0.0001 <= tmax):
    it visits every node and tests every triangle of the scene, and every triangle test fails.  The views hostile_inputs
    names as whole-tree walkers are exactly those whose frames do this."""
    flat, osc = scenes["cornell"][:2]
    rays = H.placeholder_rays(trx, 3)
    rays["direction"][0] = np.nan
    rays["origin"][1] = np.nan
    rays["origin"][2, 0] = rays["direction"][2, 1] = rays["direction"][2, 2] = np.nan
    for sem in ALL_SEMS:
        hits, st = osc.trace_rays(rays, sem=sem)
        assert (hits["prim"] == MISS).all() and st.overflow == 0
        assert (st.n_node, st.n_tri) == (3 * flat.n_nodes, 3 * flat.n_tris), sem
    w, h = 16, 16
    for vname, raw in H.hostile_views(trx, flat, w, h):
        hits, st = osc.trace_primary(orc.view_from_bytes(raw), w, h, sem=3)
        whole = st.n_tri == w * h * flat.n_tris
        if vname == H.ALIVE + "eye_1e6_diagonals":     # (depends on the scene: bistro-class yes, this one no)
            assert H.walks_whole_tree(vname)
        else:
            assert whole == H.walks_whole_tree(vname), (vname, st.n_tri)
        assert st.n_hits == 0 or not whole


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (5, 1), (3, 2), (199, 1), (7, 119)])
def test_hostile_views_of_images_smaller_than_a_tile(trx, orc, scenes, w, h):
    """tests/fuzz_gpu.py --hostile asks for hostile views at its own image sizes, which go down to one pixel: the generator
    gives the same classes there, every view is 160 bytes the oracle walks cleanly, and a switched-off view hits nothing."""
    flat, osc = scenes["cornell"][:2]
    views = H.hostile_views(trx, flat, w, h)
    assert sum(H.is_alive(n) for n, _ in views) >= 11 and sum(not H.is_alive(n) for n, _ in views) == 7
    for vname, raw in views:
        hits, st = osc.trace_primary(orc.view_from_bytes(raw), w, h, sem=0)
        assert len(raw) == 160 and st.overflow == 0 and not np.isnan(hits["t"]).any()
        assert H.is_alive(vname) or (hits["prim"] == MISS).all()


def test_axis_aligned_views_put_a_zero_or_a_residue_beside_it_into_the_centre_tile(trx, orc, scenes):
    """At w = 16 and 48 the image centre is a tile's first column: under an exactly axis-aligned view that tile's rays
    have, on one axis, a direction component whose magnitude runs from (almost) nothing to a pixel's width - the packet
    test's 1/d interval spans five orders of magnitude or more."""
    flat, osc = scenes["cornell"][:2]
    for w, h in ((16, 16), (48, 24)):
        for vname, raw in H.hostile_views(trx, flat, w, h):
            if not vname.startswith(H.ALIVE + "axis"):
                continue
            prays = osc.primary_rays(orc.view_from_bytes(raw), w, h)
            spans = []
            for t in H.tiles(w, h):
                d = np.abs(prays["direction"][t].astype(np.float64))
                d[d == 0] = 1.1920929e-7
                spans.append((d.max(axis=0) / d.min(axis=0)).max())
            assert max(spans) > 1e5, (vname, w, max(spans))


def test_view_from_camera_refuses_a_camera_that_looks_at_itself(trx, orc):
    """trx_view_from_camera answers eye == look_at with TRX_ERR_INVALID and writes no usable view; the oracle's unchecked
    orc_view_from_camera (the reference's from_camera) normalises the zero vector and returns a view_inv without a finite
    entry - the view hostile_views hands to the trace calls under that name."""
    with pytest.raises(trx.TrxError) as e:
        trx.view_from_camera([1.0, 2.0, 3.0], [1.0, 2.0, 3.0], 60.0, 16, 16)
    assert e.value.code == -1 and "eye == look_at" in str(e.value)
    ov = orc.view_from_camera([1.0, 2.0, 3.0], [1.0, 2.0, 3.0], 60.0, 16, 16)
    assert not np.isfinite(np.array(ov.view_inv[:])).any()
    assert np.isfinite(np.array(ov.proj_inv[:])).all() and list(ov.eye) == [1.0, 2.0, 3.0]
