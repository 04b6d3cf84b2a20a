"""The device refit (trx_scene_refit / trx_scene_refit_dev) against the numpy restatement of its rule (tests/refit_twin.py),
not only against the host twin that shares its code: the targets and two-level cases of tests/test_refit_twin.py from host
and from device memory, frames and aimed rays against the oracle after each, and the device path's own edges - level lists
longer than a block, the finiteness check's second grid-stride pass, the allocation range check, the launch words."""
import ctypes as C

import numpy as np
import pytest

import adversarial_scenes as A
import refit_twin as R
from helpers import F32_MAX, assert_hits_equal, instanced_scene
from test_gpu_refit import _created_info, _oracle, _world

pytestmark = pytest.mark.gpu

W, H = 64, 48
# nothing there for a ray to hit, or triangle tests whose products underflow or overflow: the oracle itself finds nothing
NO_HITS = ("denormal", "one_point", "all_negative_zero", "underflow_1e-30", "overflow_1e19", "near_flt_max")


def aimed(trx, verts, n, seed):
    """n rays from around the geometry towards random points of random triangles, drawn in
    binary64 so that scenes as wide as binary32 itself still get finite origins; a scene of one point gets rays without a
    direction, which every trace call accepts."""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3, 3)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    o = np.clip(rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), size=(n, 3)), -3e38, 3e38)
    pick = rng.integers(0, v.shape[0], size=n)
    target = (v[pick] * rng.dirichlet([1, 1, 1], size=n)[:, :, None]).sum(1)
    d = target - o
    length = np.linalg.norm(d, axis=1, keepdims=True)
    d = np.divide(d, length, out=np.zeros_like(d), where=length > 0)
    rays = np.zeros(n, dtype=trx.RAY_DTYPE)
    rays["origin"], rays["direction"] = o.astype(np.float32), d.astype(np.float32)
    rays["tmax"] = F32_MAX
    return rays


def oracle_answers(trx, orc, osc, look):
    """What the oracle finds over `osc`: the 64x48 primary + AO frame of A.camera_for(look) at semantics 0 and 3, and 2000
    rays aimed at `look`.  Returns (view, {sem: (primary, primary inst, ao)}, rays, {sem: hits}, hit count)."""
    eye, at, fov = A.camera_for(look)
    if eye == at:   # a scene of one point away from the origin: the camera's 1e-12 is below the point's rounding
        eye = tuple(float(np.float32(x + d)) for x, d in zip(at, (0.48, 0.37, 0.80)))
    if eye == at:   # a centre at 1e37, where the camera's largest distance (1e15) is lost too: look at the origin instead
        eye, at = (0.48e15, 0.37e15, 0.80e15), (0.0, 0.0, 0.0)
    view = trx.view_from_camera(eye, at, fov, W, H)
    ov = orc.view_from_bytes(view)
    frames, ray_hits, n_hits = {}, {}, 0
    rays = aimed(trx, look, 2000, 31)
    for sem in (0, 3):
        want, winst, st = osc.trace_primary_inst(ov, W, H, sem=sem)
        assert st.overflow == 0
        want_ao, _, _ = osc.trace_ao_inst(ov, W, H, want, winst, sem=sem, frame=1, ao_eps=0.01)
        frames[sem] = (want, winst, want_ao)
        ray_hits[sem], _ = osc.trace_rays(rays, sem=sem)
        n_hits += int(st.n_hits) + int((ray_hits[sem]["prim"] != 0xFFFFFFFF).sum())
    return view, frames, rays, ray_hits, n_hits


def frames_match(trx, orc, sc, flat, verts, what, look=None, expect_hits=True):
    osc = _oracle(orc, sc, flat, verts)
    view, frames, rays, ray_hits, n_hits = oracle_answers(trx, orc, osc, verts if look is None else look)
    if expect_hits:
        assert n_hits > 0, "%s: the oracle finds nothing" % what
    else:
        assert n_hits == 0, "%s: the oracle finds %d hits where there is nothing to hit" % (what, n_hits)
    for sem in (0, 3):
        prim, pinst, ao, _, _ = sc.trace_primary_ao_inst(view, W, H, sem=sem, frame=1, ao_eps=0.01)
        assert_hits_equal(prim, frames[sem][0], "%s primary sem %d" % (what, sem))
        assert_hits_equal(ao, frames[sem][2], "%s AO sem %d" % (what, sem))
        got, _ = sc.trace_rays(rays, sem=sem)
        assert_hits_equal(got, ray_hits[sem], "%s rays sem %d" % (what, sem))


def refit_both_ways(trx, orc, sc, flat, verts, o2w, what, look=None, expect_hits=True):
    """Scene.refit from host memory, then (after a refit back to the build's vertices) from device memory on a side
    stream: the twin's bytes and its level count both times, the oracle's frames and rays over what the device holds."""
    import torch
    want, _, levels = R.twin_of(flat, verts, o2w)
    sc.refit(verts)
    assert np.array_equal(sc.read_nodes(), want), what + " (host memory)"
    sc.refit(flat.tri_verts)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sc.refit(torch.from_numpy(np.ascontiguousarray(verts)).cuda())
    assert np.array_equal(sc.read_nodes(), want), what + " (device memory, side stream)"
    assert sc.info()["refit_levels"] == len(levels), what
    frames_match(trx, orc, sc, flat, verts, what, look, expect_hits)
    return want, levels


@pytest.fixture(scope="module")
def soup_scenes(trx):
    scenes = {}

    def get(n):
        if n not in scenes:
            scenes[n] = trx.Scene(R.soup_tree(trx, n))
        return scenes[n]
    yield get
    for sc in scenes.values():
        sc.close()


def expected_exp_exact(nodes):
    """trx_scene_create's rule (include/trx.h), from the bytes: 0 unless every exponent byte is 0 or >= 21, then 2 when
    every origin is +0 or 2^-36 <= |p| <= 2^59, else 1."""
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 20)
    e = nodes.view(np.uint8).reshape(-1, 80)[:, 12:15]
    if not ((e == 0) | (e >= 21)).all():
        return 0
    a = np.abs(nodes[:, 0:3].view(np.float32).astype(np.float64))
    return 2 if ((nodes[:, 0:3] == 0) | ((a >= 2.0 ** -36) & (a <= 2.0 ** 59))).all() else 1


# ---- device bytes against the numpy twin ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.target_names())
def test_refit_targets(trx, orc, soup_scenes, name):
    n = R.target_size(name)
    flat, sc = R.soup_tree(trx, n), soup_scenes(n)
    verts = trx.record_order_verts(flat, R.target_verts(name, n))
    want, levels = refit_both_ways(trx, orc, sc, flat, verts, None, name, expect_hits=name not in NO_HITS)
    assert np.array_equal(want, trx.refit_nodes(flat, verts))
    info = sc.info()
    assert info["exp_exact"] == expected_exp_exact(want), name
    assert info == _created_info(trx, flat, want, verts) | {"refit_levels": len(levels)}, name
    # a level list longer than one 256-thread block with a last block that is not full, and a level of one node
    assert any(k > 256 and k % 256 for k in levels) and levels[-1] == 1, levels


@pytest.mark.parametrize("transforms", ["own", "random", "mirrored_far", "tiny_scale"])
def test_instanced_scene(trx, orc, transforms):
    flat, *_ = instanced_scene(trx)
    o2w = R.instance_transform_sets(trx, flat)[transforms]
    verts = R.jitter(flat.tri_verts, 8)
    sc = trx.Scene(flat)
    try:
        sc.set_instance_transforms(o2w)
        refit_both_ways(trx, orc, sc, flat, verts, o2w, transforms, look=_world(type("F", (), {
            "instance_offsets": flat.instance_offsets, "blas_tri_start": flat.blas_tri_start, "tri_verts": verts}), o2w))
        assert sc.info()["exp_exact"] == expected_exp_exact(sc.read_nodes())
    finally:
        sc.close()


@pytest.mark.parametrize("rebraid", [True, False])
def test_two_level_kitchen(trx, orc, rebraid):
    flat = R.kitchen_tlas(trx, rebraid)
    assert (flat.instance_entry is not None and np.count_nonzero(flat.instance_entry) > 20) if rebraid else flat.instance_entry is None
    sc = trx.Scene(flat)
    try:
        refit_both_ways(trx, orc, sc, flat, R.jitter(flat.tri_verts, 4), None, "kitchen --tlas, re-braided: %s" % rebraid)
        sc.refit(flat.tri_verts)
        want, _, _ = R.twin_of(flat, flat.tri_verts)
        assert np.array_equal(sc.read_nodes(), want)
        if not rebraid:
            assert np.array_equal(want, flat.nodes)
    finally:
        sc.close()


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 24, 25])
def test_tiny_trees(trx, n):
    import torch
    flat = trx.flat_build(A.soup(n, 5), np.array([n], dtype=np.uint64))
    sc = trx.Scene(flat)
    try:
        for what, verts in (("jitter", R.jitter(flat.tri_verts, 6, 0.2)), ("one point", R.target_verts("one_point", n))):
            want, _, levels = R.twin_of(flat, verts)
            sc.refit(verts)
            assert np.array_equal(sc.read_nodes(), want), (n, what)
            if n:   # (a tensor of no elements has no address to hand over)
                sc.refit(flat.tri_verts)
                sc.refit(torch.from_numpy(verts).cuda())
                assert np.array_equal(sc.read_nodes(), want), (n, what)
            assert sc.info()["refit_levels"] == len(levels)
    finally:
        sc.close()


# ---- the launch words ------------------------------------------------------------------------------------------------

def test_launch_words_with_signed_zeros(trx, soup_scenes):
    """A -0 origin fails trx_scene_create's and the refit reduction's test for exp_exact == 2 alike; the encoders and the
    refit write a zero origin as +0, so neither a refit to the signed-zero vertices nor an identity refit of a tree built
    over them moves exp_exact or the diagonal away from what a scene created from the same bytes has."""
    n = R.target_size("signed_zero")
    zeros = A.signed_zero(n)
    flat, sc = R.soup_tree(trx, n), soup_scenes(n)
    verts = trx.record_order_verts(flat, zeros)
    sc.refit(verts)
    nodes = sc.read_nodes()
    assert not (nodes[:, 0:3] == 0x80000000).any() and (nodes[:, 0] == 0).any()
    got, want = sc.info(), _created_info(trx, flat, nodes, verts)
    assert (got["exp_exact"], got["scene_diag"]) == (want["exp_exact"], want["scene_diag"]) and got["exp_exact"] == expected_exp_exact(nodes) == 2

    built = trx.flat_build(zeros, np.array([n], dtype=np.uint64))
    own = trx.Scene(built)
    try:
        before = own.info()
        assert before["exp_exact"] == expected_exp_exact(built.nodes) == 2
        own.refit(built.tri_verts)
        assert np.array_equal(own.read_nodes(), built.nodes)
        after = own.info()
        assert (after["exp_exact"], after["scene_diag"]) == (before["exp_exact"], before["scene_diag"])
    finally:
        own.close()
    # what a -0 origin costs: the same tree with one zero origin written as -0 is created with exp_exact 1, and the
    # refit, which writes +0, gives the scene its 2 back
    patched = built.nodes.copy()
    node = int(np.flatnonzero(patched[:, 0] == 0)[0])
    patched[node, 0] = 0x80000000
    assert expected_exp_exact(patched) == 1
    neg = trx.Scene(trx.FlatScene(patched, built.tri_verts, built.instance_offsets, built.tlas_start, built.tri_source, built.blas_tri_start))
    try:
        assert neg.info()["exp_exact"] == 1
        neg.refit(built.tri_verts)
        assert np.array_equal(neg.read_nodes(), built.nodes) and neg.info()["exp_exact"] == 2
    finally:
        neg.close()


# ---- the finiteness check's second grid-stride pass ------------------------------------------------------------------------

def test_one_nan_anywhere_in_a_device_buffer_is_refused(trx):
    """k_refit_check runs 4096 x 256 = 1 048 576 threads: the 1 080 000 floats of 120 000 triangles take a second pass of
    the grid-stride loop.  One NaN in the first thread's first float, the last thread's first float, the first thread's
    second float and the last float of all."""
    import torch
    n = 120000
    flat = trx.flat_build(A.soup(n, 3), np.array([n], dtype=np.uint64))
    assert flat.n_tris * 9 > 4096 * 256
    sc = trx.Scene(flat)
    try:
        good = R.jitter(flat.tri_verts, 5)
        d = torch.from_numpy(good).cuda()
        sc.refit(d)
        nodes = sc.read_nodes()
        assert np.array_equal(nodes, trx.refit_nodes(flat, good))
        for at in (0, 4096 * 256 - 1, 4096 * 256, n * 9 - 1):
            bad = d.clone()
            bad.view(-1)[at] = float("nan")
            with pytest.raises(trx.TrxError) as e:
                sc.refit(bad)
            assert e.value.code == trx._lib.TRX_ERR_INVALID and "finite" in str(e.value), at
            assert np.array_equal(sc.read_nodes(), nodes), at
        sc.refit(d)
        assert np.array_equal(sc.read_nodes(), nodes)
    finally:
        sc.close()


# ---- the range check -------------------------------------------------------------------------------------------------

def test_views_into_a_larger_allocation(trx, soup_scenes):
    """trx_scene_refit_dev asks whether the ALLOCATION holds n x 9 floats from the pointer on: a view that ends exactly
    where the allocation ends and a view into its middle are accepted and refit correctly, a view that starts one record
    later than the former - one trailing record short - is refused."""
    import torch
    n = R.target_size("soup")
    flat, sc = R.soup_tree(trx, n), soup_scenes(n)
    lib = trx.load()
    verts = R.jitter(flat.tri_verts, 14)
    want, _, _ = R.twin_of(flat, verts)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    big = torch.zeros(24 << 18, dtype=torch.float32, device="cuda")    # 24 MiB: a device allocation of its own
    end = big.data_ptr() + big.numel() * 4
    seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= big.data_ptr() < s["address"] + s["total_size"]]
    assert len(seg) == 1 and seg[0]["address"] + seg[0]["total_size"] == end, "the tensor does not end where its allocation ends"
    v = torch.from_numpy(verts).cuda().view(-1)
    last, middle = big.numel() - n * 9, 1000 * 9
    for start in (last, middle):
        big.zero_()
        big[start:start + n * 9] = v
        sc.refit(flat.tri_verts)
        sc.refit(big[start:start + n * 9])
        assert np.array_equal(sc.read_nodes(), want), start
    torch.cuda.synchronize()
    for start in (last + 9, last + 1):
        rc = lib.trx_scene_refit_dev(sc.handle, C.c_void_p(big.data_ptr() + 4 * start), n, None)
        assert rc == trx._lib.TRX_ERR_INVALID and b"does not hold" in lib.trx_last_error(), start
        assert np.array_equal(sc.read_nodes(), want), start
