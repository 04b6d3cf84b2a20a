"""BVH refit (trx_refit_nodes, the host twin of trx_scene_refit): new vertices under a kept topology.  CPU only: the
oracle walks the refitted nodes over the new vertices and must find what brute force over those vertices finds."""
import ctypes as C

import numpy as np
import pytest

from helpers import aimed_rays, bits, instanced_scene, random_affine, random_rays, w2o_rows
from refit_twin import _topology_kept


@pytest.fixture()
def build_knobs(trx):
    lib = trx.load()
    yield lib
    lib.trx_set_build_rebraid(C.c_float(1.0 / 4096.0))   # the defaults
    lib.trx_set_build_split(C.c_float(0.0))


def _flat(trx, name, n, tlas=False, seed=1):
    verts, counts = trx.gen_scene(name, n, seed)
    return trx.flat_build(verts, counts, use_tlas=tlas), counts


def _hits_match_brute_force(orc, osc, rays, what):
    """The walk over the refitted tree finds brute force's hits (the slab test's razor-edge rounding aside, as for
    every built tree: tests/test_rebraid.py)."""
    assert osc.validate() == (0, ""), what
    for sem in (0, 3):
        hits, st = osc.trace_rays(rays, sem=sem)
        assert st.overflow == 0
        bf = osc.brute_rays(rays, sem=sem)
        same = bits(hits["t"]) == bits(bf["t"])   # (coplanar duplicates tie: which one is reported depends on the order)
        assert same.mean() > 0.9995, "%s sem %d: %d of %d rays differ" % (what, sem, (~same).sum(), same.size)
        assert (bf["prim"] != 0xFFFFFFFF).sum() > rays.size // 4


# ---- identity: a refit with the build's own inputs returns the build's bytes ------------------------------------

@pytest.mark.parametrize("name,n", [("soup", 3000), ("cornell", 0), ("bistro", 12000)])
def test_identity_single_level(trx, name, n):
    flat, _ = _flat(trx, name, n)
    assert np.array_equal(trx.refit_nodes(flat, flat.tri_verts), flat.nodes)


def test_identity_where_the_root_extent_overflows(trx):
    """Finite vertices whose x range (6e38) is +inf in binary32: the refit and the builder take the same quantisation
    step there, a finite one (exponent byte 255 would be +inf)."""
    import adversarial_scenes as A
    verts = A.extent_overflow_x(3000)
    with np.errstate(over="ignore"):
        assert np.isfinite(verts).all() and np.isinf(verts[:, 0::3].max() - verts[:, 0::3].min())
    flat = trx.flat_build(verts, np.array([verts.shape[0]], dtype=np.uint64))
    assert np.array_equal(trx.refit_nodes(flat, flat.tri_verts), flat.nodes)
    root_e = np.ascontiguousarray(flat.nodes).view(np.uint8).reshape(-1, 80)[0, 12:15]
    assert root_e[0] < 255, root_e


def test_identity_device_pipeline_builder(trx):
    """The preset pipeline's encoder (k8_encode's host twin) agrees with the refit too."""
    verts, counts = trx.gen_scene("bistro", 40000, 2)
    flat = trx.flat_build_preset_device(verts, counts, device=-1)
    assert np.array_equal(trx.refit_nodes(flat, flat.tri_verts), flat.nodes)


@pytest.mark.parametrize("name,n", [("kitchen", 20000), ("san_miguel", 30000)])
def test_identity_tlas_without_rebraiding(trx, build_knobs, name, n):
    assert build_knobs.trx_set_build_rebraid(C.c_float(0.0)) == 0
    flat, _ = _flat(trx, name, n, tlas=True)
    assert flat.instance_entry is None
    assert np.array_equal(trx.refit_nodes(flat, flat.tri_verts), flat.nodes)


def test_identity_instanced_with_transforms(trx):
    flat, o2w, *_ = instanced_scene(trx)
    assert np.array_equal(trx.refit_nodes(flat, flat.tri_verts, o2w), flat.nodes)


def test_rebraided_and_presplit_refits_are_valid(trx, orc, build_knobs):
    """Not the build's bytes (whole-triangle boxes for split references, exact boxes for entry subtrees), but valid
    trees that find what brute force finds."""
    flat, _ = _flat(trx, "san_miguel", 30000, tlas=True)
    assert flat.instance_entry is not None
    out = trx.refit_nodes(flat, flat.tri_verts)
    _topology_kept(flat.nodes, out)
    osc = orc.Scene(out, flat.tri_verts, flat.instance_offsets, flat.tlas_start, instance_entry=flat.instance_entry)
    _hits_match_brute_force(orc, osc, random_rays(trx, flat, 4000, 5), "re-braided")

    assert build_knobs.trx_set_build_split(C.c_float(0.5)) == 0
    verts, counts = trx.gen_scene("cornell", 0, 1)
    split = trx.flat_build(verts, counts)
    assert split.n_tris > verts.shape[0]                              # some triangles were split
    out = trx.refit_nodes(split, split.tri_verts)
    _topology_kept(split.nodes, out)
    osc = orc.Scene(out, split.tri_verts)
    _hits_match_brute_force(orc, osc, aimed_rays(trx, split.tri_verts, 4000, 6), "pre-split")


# ---- deformation --------------------------------------------------------------------------------------------------

def _deformations(flat, counts, seed):
    rng = np.random.default_rng(seed)
    v = flat.tri_verts.astype(np.float64)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    size = float(np.linalg.norm(hi - lo))
    # per-vertex jitter
    jitter = v + rng.normal(scale=0.01 * size, size=v.shape)
    # a global affine map
    M = np.asarray(random_affine(rng, 0.5, 2.0, spread=size), dtype=np.float64).reshape(4, 4).T
    affine = (v.reshape(-1, 3) @ M[:3, :3].T + M[:3, 3]).reshape(-1, 9)
    # one object translated far outside its old box
    first = np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))])
    obj = int(np.argmax(np.diff(first)))
    moved = v.copy()
    sel = (flat.tri_source >= first[obj]) & (flat.tri_source < first[obj + 1])
    moved[sel] += np.tile(np.array([3.0, -2.0, 1.5]) * size, 3)
    return {"jitter": jitter, "affine": affine, "moved_object": moved}


@pytest.mark.parametrize("name,n,tlas", [("bistro", 12000, False), ("kitchen", 20000, True)])
def test_deformed_geometry_is_found_like_brute_force(trx, orc, name, n, tlas):
    flat, counts = _flat(trx, name, n, tlas=tlas)
    for kind, v in _deformations(flat, counts, 7).items():
        v = v.astype(np.float32)
        out = trx.refit_nodes(flat, v)
        _topology_kept(flat.nodes, out)
        assert not np.array_equal(out, flat.nodes)
        osc = orc.Scene(out, v, flat.instance_offsets, flat.tlas_start, instance_entry=flat.instance_entry)
        nflat = type("F", (), {"tri_verts": v})
        rays = np.concatenate([random_rays(trx, nflat, 2000, 8), aimed_rays(trx, v, 3000, 9)])
        _hits_match_brute_force(orc, osc, rays, "%s %s" % (name, kind))
        if kind == "moved_object":   # the old tree over the moved geometry loses the object: what the refit fixes
            stale = orc.Scene(flat.nodes, v, flat.instance_offsets, flat.tlas_start, instance_entry=flat.instance_entry)
            hits, _ = stale.trace_rays(rays, sem=0)
            assert (bits(hits["t"]) != bits(osc.brute_rays(rays, sem=0)["t"])).mean() > 0.01


def test_refit_in_place_and_round_trip(trx):
    flat, counts = _flat(trx, "soup", 3000)
    v = _deformations(flat, counts, 3)["jitter"].astype(np.float32)
    there = trx.refit_nodes(flat, v)
    back = trx.refit_nodes(flat, flat.tri_verts, nodes=there)
    assert np.array_equal(back, flat.nodes)


# ---- moved instances ----------------------------------------------------------------------------------------------

def _world(flat, o2w, blas_of):
    bts, out = flat.blas_tri_start, []
    for k in range(flat.instance_offsets.size):
        b = blas_of[int(flat.instance_offsets[k])]
        tv = flat.tri_verts[bts[b]:bts[b + 1]].astype(np.float64).reshape(-1, 3)
        M = np.asarray(o2w[k], dtype=np.float64).reshape(4, 4).T
        out.append((tv @ M[:3, :3].T + M[:3, 3]).reshape(-1, 9).astype(np.float32))
    return np.concatenate(out)


def test_moved_instances(trx, orc):
    flat, o2w, world, first, blas_of = instanced_scene(trx)
    rng = np.random.default_rng(17)
    new = np.stack([random_affine(rng, spread=12.0) for _ in range(o2w.shape[0])])
    w2o = np.stack([w2o_rows(m) for m in new])
    nworld = _world(flat, new, blas_of)
    rays = np.concatenate([random_rays(trx, type("W", (), {"tri_verts": nworld}), 2000, 3), aimed_rays(trx, nworld, 6000, 4)])
    out = trx.refit_nodes(flat, flat.tri_verts, new)
    _topology_kept(flat.nodes, out)
    bf = orc.Scene(flat.nodes, flat.tri_verts, flat.instance_offsets, flat.tlas_start).brute_rays_over(nworld, rays, sem=3)
    bf_hit = bf["prim"] != 0xFFFFFFFF
    assert bf_hit.sum() > 3000

    def agreement(nodes):
        osc = orc.Scene(nodes, flat.tri_verts, flat.instance_offsets, flat.tlas_start, instance_w2o=w2o)
        hits, inst, st = osc.trace_rays_inst(rays, sem=3)
        assert st.overflow == 0
        hit = hits["prim"] != 0xFFFFFFFF
        both = hit & bf_hit
        b = np.array([blas_of[int(o)] for o in flat.instance_offsets[inst[both]]])
        widx = first[inst[both]] + (hits["prim"][both] - flat.blas_tri_start[b])
        # hit / miss as brute force over the world-space copies, the same triangle (the two transform directions round
        # differently: razor-edge rays and near-ties aside, as tests/test_instances.py allows)
        return (hit == bf_hit).mean(), (widx == bf["prim"][both]).mean()

    hit_ok, tri_ok = agreement(out)
    assert hit_ok > 0.999 and tri_ok > 0.995
    stale_hit_ok, _ = agreement(flat.nodes)                           # the build's boxes do not bound the moved instances
    assert stale_hit_ok < 0.95


# ---- refused input ------------------------------------------------------------------------------------------------

def test_refused_input(trx):
    lib = trx.load()
    flat, _ = _flat(trx, "soup", 500)
    out = np.zeros_like(flat.nodes)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def refit(nodes, verts, n):
        return lib.trx_refit_nodes(nodes, flat.n_nodes, verts, n, None, 0, 0, None, None, ptr(out))

    assert refit(ptr(flat.nodes), ptr(flat.tri_verts), flat.n_tris) == 0
    assert refit(ptr(flat.nodes), ptr(flat.tri_verts), flat.n_tris - 1) == trx._lib.TRX_ERR_INVALID   # fewer than referenced
    assert refit(None, ptr(flat.tri_verts), flat.n_tris) == trx._lib.TRX_ERR_INVALID
    assert refit(ptr(flat.nodes), None, flat.n_tris) == trx._lib.TRX_ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        v = flat.tri_verts.copy()
        v[flat.n_tris // 2, 4] = bad
        assert refit(ptr(flat.nodes), ptr(v), flat.n_tris) == trx._lib.TRX_ERR_INVALID
        assert b"finite" in lib.trx_last_error()
    with pytest.raises(trx.TrxError):
        trx.refit_nodes(flat, flat.tri_verts[:-1])
