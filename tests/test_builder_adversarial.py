"""The host ploc_cwbvh pipeline (trx_flat_build_params, and trx_flat_build_preset_device with device = -1) on degenerate
geometry at the sizes that reach the device stage: exact ties of the merge areas, zero extents, duplicates, half-areas
that underflow to 0 or overflow to +inf, signed zeros (tests/adversarial_scenes.py).  Every build must return a valid tree
no deeper than the validator's 512 levels, hold every triangle once, answer like brute force, not depend on the thread
count and stay within a build-time cap; non-finite vertices are refused by every flat builder."""
import time

import numpy as np
import pytest

import adversarial_scenes as A

W, H = 64, 48

PARAM_SETS = {
    "default": dict(),
    "sort128": dict(sort_precision=128),
    "dist2": dict(ploc_search_distance=2, search_depth_threshold=0),
    "no_reinsertion": dict(reinsertion_batch_ratio=0.0),
    "medium_preset": None,   # trx_flat_build_preset_device(preset="medium_build", device=-1)
    # the binned-SAH preset path (trx_flat_build), its reinsertion in whole-iteration batches: the host twin of what
    # test_gpu_builder_adversarial.py runs on the device (its exact sweep read order[-1] on the 1e19 soup)
    "sah_whole_iterations": "sah",
}

# Build-time cap: an adversarial build may take at most 10x the wall time the parent commit (187b7bb) needs for the plain
# random soup (adversarial_scenes.soup) of the same n and parameters.  Parent times in seconds, median of 5 builds on the
# 8-core machine this file was written on, default thread count; the cap in seconds is ten times the entry:
#   default         0.592  0.483  0.513      sort128         0.611  0.480  0.601      dist2          0.462  0.352  0.434
#   no_reinsertion  0.373  0.242  0.292      medium_preset   0.546  0.558  0.831      sah_whole_it.  0.243  0.220  0.183
# What the cap is there to catch is 200-600x (one merge per PLOC round: 7 s at 8192 identical triangles, 63-75 s at
# 32768) or 80-150x (reinsertion searches that cannot prune: 4.6-8.6 s on the 1e19 soup); the degenerate builds
# themselves take 0.3-2x the soup's time.
PARENT_SOUP_SECONDS = {
    # params:          n = 32768, 32769, 40001
    "default":        (0.0592, 0.0483, 0.0513),
    "sort128":        (0.0611, 0.0480, 0.0601),
    "dist2":          (0.0462, 0.0352, 0.0434),
    "no_reinsertion": (0.0373, 0.0242, 0.0292),
    "medium_preset":  (0.0546, 0.0558, 0.0831),
    "sah_whole_iterations": (0.0243, 0.0220, 0.0183),
}
CAP_FACTOR = 10.0
SIZES = (A.N_THRESHOLD, A.N_PAST, A.N_ODD)


def cap_seconds(params, n):
    return CAP_FACTOR * PARENT_SOUP_SECONDS[params][SIZES.index(n)]


def build(trx, verts, params, threads=0):
    counts = np.array([verts.shape[0]], dtype=np.uint64)
    if PARAM_SETS[params] is None:
        return trx.flat_build_preset_device(verts, counts, preset="medium_build", device=-1, threads=threads)
    if PARAM_SETS[params] == "sah":
        lib = trx.load()
        try:
            assert lib.trx_set_build_reinsertion_batches(1) == 0
            return trx.flat_build(verts, counts, preset="medium_build", reinsertion=(0.05, 6), threads=threads)
        finally:
            lib.trx_set_build_reinsertion_batches(0)
            lib.trx_set_build_preset(b"medium_build")
    return trx.flat_build_params(verts, counts, trx.build_params(**PARAM_SETS[params]), threads=threads)


_scenes = {}


def scene(trx, orc, case):
    """(verts, oracle view, brute-force t bits of the frame): computed once per case, never changed."""
    if case not in _scenes:
        verts = A.FINITE[case]()
        verts.setflags(write=False)
        eye, look, fov = A.camera_for(verts)
        ov = orc.view_from_bytes(trx.view_from_camera(eye, look, fov, W, H))
        brute = orc.Scene(np.zeros((1, 20), np.uint32), verts).brute_primary(ov, W, H, sem=3)
        want = brute["t"].view(np.uint32).copy()
        want.setflags(write=False)
        _scenes[case] = (verts, ov, want)
    return _scenes[case]


@pytest.mark.parametrize("params", list(PARAM_SETS))
@pytest.mark.parametrize("case", list(A.FINITE))
def test_adversarial_host_build(trx, orc, case, params):
    verts, ov, want_t = scene(trx, orc, case)
    n = verts.shape[0]
    assert verts.dtype == np.float32 and verts.shape == (n, 9) and n in SIZES and np.isfinite(verts).all()
    t0 = time.perf_counter()
    flat = build(trx, verts, params)
    seconds = time.perf_counter() - t0
    cap = cap_seconds(params, n)
    if seconds > cap:   # one more measurement before judging: a stall of the machine is not the builder's
        t0 = time.perf_counter()
        flat = build(trx, verts, params)
        seconds = min(seconds, time.perf_counter() - t0)
    print("%s / %s: n = %d, build %.3f s, cap %.3f s" % (case, params, n, seconds, cap))
    osc = orc.Scene.from_flat(flat)
    assert osc.validate() == (0, "")
    assert flat.n_tris == n and (np.sort(flat.tri_source) == np.arange(n, dtype=np.uint32)).all()
    assert (flat.tri_verts.view(np.uint32) == verts[flat.tri_source].view(np.uint32)).all()
    got, st = osc.trace_primary(ov, W, H, sem=3)
    assert st.overflow == 0
    assert (got["t"].view(np.uint32) == want_t).all()
    one, five = build(trx, verts, params, threads=1), build(trx, verts, params, threads=5)
    assert one.nodes.tobytes() == five.nodes.tobytes() == flat.nodes.tobytes()
    assert one.tri_source.tobytes() == five.tri_source.tobytes() == flat.tri_source.tobytes()
    assert seconds <= cap, "build took %.3f s, cap %.3f s" % (seconds, cap)


@pytest.mark.parametrize("case", list(A.NON_FINITE))
def test_non_finite_vertices_are_refused(trx, case):
    """The rule trx_scene_refit states (TRX_ERR_INVALID for a non-finite vertex) holds for the flat builders as well."""
    L = trx._lib
    verts = A.NON_FINITE[case]()
    n = verts.shape[0]
    assert not np.isfinite(verts).all() and np.isfinite(verts).sum() == verts.size - 1
    counts = np.array([n], dtype=np.uint64)
    halves = np.array([n // 2, n - n // 2], dtype=np.uint64)
    builds = {
        "trx_flat_build": lambda: trx.flat_build(verts, counts),
        "trx_flat_build (tlas)": lambda: trx.flat_build(verts, halves, use_tlas=True),
        "trx_flat_build_params": lambda: trx.flat_build_params(verts, counts, trx.build_params()),
        "trx_flat_build_preset_device": lambda: trx.flat_build_preset_device(verts, counts, preset="medium_build", device=-1),
        "trx_flat_build_instanced": lambda: trx.flat_build_instanced(verts, halves, [0, 1, 1], None),
    }
    for name, call in builds.items():
        with pytest.raises(trx.TrxError, match="finite") as e:
            call()
        assert e.value.code == L.TRX_ERR_INVALID, name
    # nothing is returned: the out pointer stays as it was
    import ctypes as C
    fp = C.POINTER(L.Flat)()
    lib = trx.load()
    assert lib.trx_flat_build(verts.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), 1, 0, 3, 0,
                              C.byref(fp)) == L.TRX_ERR_INVALID
    assert not fp


def test_a_tree_past_the_depth_limit_is_refused_not_returned(trx, orc):
    """Nested boxes make PLOC's BVH2 a chain whatever the tie rule; the collapse packs about seven of its levels into a
    node.  3000 triangles stay within the 512 levels the validator and the traversal stacks allow and build; 4500 do not,
    and the build is refused with TRX_ERR_INVALID - the recursive emission used to follow a chain to any depth, and ran
    off the stack on the 32767 levels of the 1e-30 soup."""
    for kw in (dict(), dict(reinsertion_batch_ratio=0.0)):
        verts = A.nested_triangles(3000)
        flat = trx.flat_build_params(verts, np.array([3000], dtype=np.uint64), trx.build_params(**kw))
        assert orc.Scene.from_flat(flat).validate() == (0, "")
        assert (np.sort(flat.tri_source) == np.arange(3000, dtype=np.uint32)).all()
        verts = A.nested_triangles(4500)
        for threads in (0, 1):
            with pytest.raises(trx.TrxError, match="deeper than 512 levels") as e:
                trx.flat_build_params(verts, np.array([4500], dtype=np.uint64), trx.build_params(**kw), threads=threads)
            assert e.value.code == trx._lib.TRX_ERR_INVALID
