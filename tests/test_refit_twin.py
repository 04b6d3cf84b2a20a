"""The host refit (trx_refit_nodes) against the numpy restatement of its rule and against invariants checked in exact
arithmetic (tests/refit_twin.py): deformed and degenerate geometry, every builder's identity, trees of one to four nodes,
two-level scenes with hostile transforms.  CPU only.  Every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import adversarial_scenes as A
import refit_twin as R
from helpers import instanced_scene

BUILDERS = ("flat_build", "flat_build_params", "flat_build_preset_device")


@pytest.fixture()
def build_knobs(trx):
    lib = trx.load()
    yield lib
    lib.trx_set_build_rebraid(C.c_float(1.0 / 4096.0))   # the defaults
    lib.trx_set_build_split(C.c_float(0.0))


def _build(trx, builder, verts):
    counts = np.array([verts.shape[0]], dtype=np.uint64)
    if builder == "flat_build":
        return trx.flat_build(verts, counts)
    if builder == "flat_build_params":
        return trx.flat_build_params(verts, counts, trx.build_params())
    return trx.flat_build_preset_device(verts, counts, preset="medium_build", device=-1)


def _differing(a, b):
    a, b = np.asarray(a).reshape(-1, 20), np.asarray(b).reshape(-1, 20)
    rows = np.flatnonzero((a != b).any(axis=1))
    return "%d of %d nodes differ, first %s: words %s" % (rows.size, a.shape[0], rows[:4].tolist(),
                                                            np.flatnonzero(a[rows[0]] != b[rows[0]]).tolist() if rows.size else [])


def _host_equals_twin(trx, flat, verts, what, o2w=None):
    """trx_refit_nodes of flat's tree over `verts` equals the twin and satisfies the invariants; returns the bytes."""
    got = trx.refit_nodes(flat, verts, o2w)
    want, _, _ = R.twin_of(flat, verts, o2w)
    assert np.array_equal(got, want), "%s: %s" % (what, _differing(got, want))
    R.check_flat(flat, got, verts, o2w)
    return got


# ---- refit targets: a soup's tree over other geometry ---------------------------------------------------------------------

@pytest.mark.parametrize("name", R.target_names())
def test_refit_targets(trx, name):
    n = R.target_size(name)
    flat = R.soup_tree(trx, n)
    verts = trx.record_order_verts(flat, R.target_verts(name, n))
    got = _host_equals_twin(trx, flat, verts, name)
    if name in ("one_point", "all_negative_zero"):
        # every frame collapses onto the point: the origin there (+0 for the zeros), floor steps, every plane byte 0
        b = got.view(np.uint8).reshape(-1, 80)
        assert (b[:, 12:15] == 53).all()
        assert (got[:, 0:3].view(np.float32) == verts[0, 0:3]).all() and (got[:, 0:3] != 0x80000000).all()
        used = np.tile(b[:, 24:32] != 0, (1, 6))
        assert (b[:, 32:80][used] == 0).all()


# ---- identity: a refit with the build's own inputs returns the build's bytes -----------------------------------------------

@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", list(A.FINITE))
def test_identity_on_degenerate_geometry(trx, builder, name):
    """On signed_zero the builders' boxes (folded in merge order) and the refit's (slot order) keep different zeros as a
    minimum: 79 to 86 of 643 to 731 nodes differed in bit 31 of origin word 0 before frame_origin wrote every zero origin
    as +0."""
    flat = _build(trx, builder, A.FINITE[name](R.target_size(name)))
    got = trx.refit_nodes(flat, flat.tri_verts)
    assert np.array_equal(got, flat.nodes), "%s %s: %s" % (builder, name, _differing(got, flat.nodes))
    assert not (flat.nodes[:, 0:3] == 0x80000000).any(), "a -0 origin"


def test_identity_keeps_the_twin_too(trx):
    """... and the twin states the same rule: it returns the build's bytes where the library does."""
    for name in ("signed_zero", "lattice_plane", "extent_overflow_x"):
        flat = _build(trx, "flat_build", A.FINITE[name](2000))
        want, _, _ = R.twin_of(flat, flat.tri_verts)
        assert np.array_equal(want, flat.nodes), "%s: %s" % (name, _differing(want, flat.nodes))
        R.check_flat(flat, flat.nodes, flat.tri_verts)


def test_presplit_and_rebraided_trees(trx, build_knobs):
    """Not the build's bytes (include/trx.h): the twin's, and tight."""
    assert build_knobs.trx_set_build_split(C.c_float(0.5)) == 0
    verts, counts = trx.gen_scene("cornell", 0, 1)
    split = trx.flat_build(verts, counts)
    assert split.n_tris > verts.shape[0]                              # some triangles were split
    assert build_knobs.trx_set_build_split(C.c_float(0.0)) == 0
    _host_equals_twin(trx, split, split.tri_verts, "pre-split")
    _host_equals_twin(trx, split, R.jitter(split.tri_verts, 3), "pre-split, jitter")

    flat = R.kitchen_tlas(trx, True)
    assert flat.instance_entry is not None and np.count_nonzero(flat.instance_entry) > 20
    _host_equals_twin(trx, flat, flat.tri_verts, "re-braided")
    _host_equals_twin(trx, flat, R.jitter(flat.tri_verts, 4), "re-braided, jitter")


# ---- tiny trees ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 24, 25])
def test_tiny_trees(trx, n):
    flat = trx.flat_build(A.soup(n, 5), np.array([n], dtype=np.uint64))
    assert 1 <= flat.n_nodes <= 4 and flat.n_tris == n
    same = _host_equals_twin(trx, flat, flat.tri_verts, "n = %d, identity" % n)
    assert np.array_equal(same, flat.nodes)
    _host_equals_twin(trx, flat, R.jitter(flat.tri_verts, 6, 0.2), "n = %d, jitter" % n)
    _host_equals_twin(trx, flat, R.target_verts("one_point", n), "n = %d, one point" % n)


# ---- two-level scenes --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("transforms", ["own", "random", "mirrored_far", "tiny_scale"])
def test_instanced_scene(trx, transforms):
    flat, *_ = instanced_scene(trx)
    o2w = R.instance_transform_sets(trx, flat)[transforms]
    got = _host_equals_twin(trx, flat, flat.tri_verts, transforms, o2w)
    if transforms == "own":
        assert np.array_equal(got, flat.nodes)
    _host_equals_twin(trx, flat, R.jitter(flat.tri_verts, 8), transforms + ", jitter", o2w)


def test_tlas_without_rebraiding(trx):
    flat = R.kitchen_tlas(trx, False)
    assert flat.has_tlas and flat.instance_entry is None
    got = _host_equals_twin(trx, flat, flat.tri_verts, "kitchen --tlas")
    assert np.array_equal(got, flat.nodes)
    _host_equals_twin(trx, flat, R.jitter(flat.tri_verts, 9), "kitchen --tlas, jitter")


# ---- the checker itself can fail -----------------------------------------------------------------------------------------

def test_the_invariants_notice_loose_and_cutting_planes(trx):
    """Loose planes on a slot, a plane that cuts its content, a doubled step and a -0 origin each fail the checker (it is
    what would notice a refit that is conservative but not tight, which no walk can)."""
    flat = R.soup_tree(trx, R.target_size("soup"))
    verts = R.jitter(flat.tri_verts, 12)
    good = trx.refit_nodes(flat, verts)
    R.check_flat(flat, good, verts)
    b = good.view(np.uint8).reshape(-1, 80)
    node = int(np.flatnonzero((b[:, 24] != 0) & (b[:, 32] >= 3) & (b[:, 40] <= 252))[0])   # slot 0 used, x planes off the clamps

    def broken(change):
        bad = good.copy()
        change(bad.view(np.uint8).reshape(-1, 80)[node], bad[node])
        with pytest.raises(AssertionError):
            R.check_flat(flat, bad, verts)

    def lower(k):
        def f(bytes_, words):
            bytes_[32] = int(bytes_[32]) - k
        return f

    def upper(k):
        def f(bytes_, words):
            bytes_[40] = int(bytes_[40]) + k
        return f

    def step(bytes_, words):
        bytes_[12] = int(bytes_[12]) + 2

    def origin(bytes_, words):
        words[0] = 0x80000000

    for change in (lower(3), upper(3), lower(-3), upper(-3), step, origin):
        broken(change)
