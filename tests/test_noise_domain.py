"""The helper of the noise-domain tests (tests/noise_domain.py) and the oracle's side of them, without a GPU: seed_for inverts
the hash, every target reaches the branch its name claims, the oracle's ray at every target has the properties the
DEFINITION gives it (not the code), orc_ao_rays is the per-call function in a loop, and the dense leg's committed seeds show
what makes that leg worth running.  tests/test_gpu_noise_domain.py then holds the device to the oracle at these inputs."""
import ctypes as C
import math

import numpy as np
import pytest

import noise_domain as ND
from ao_visibility_twin import ao_rays
from helpers import w2o_rows

F32_MAX = 3.4028234663852886e38
INERT = np.array([0, 0, 0, 0, 0, 0, 0, 0xBF800000], dtype=np.uint32)


@pytest.fixture(scope="module")
def scenes(trx, orc):
    """name -> (oracle scene, oracle view, records, instance ids or None, world-space unit normals in binary64 per record)."""
    eye, look, fov = ND.CAMERA
    oview = orc.view_from_bytes(bytes(trx.view_from_camera(eye, look, fov, ND.W, ND.H)))
    flat = ND.single_level(trx)
    flat2, pairs = ND.two_level(trx)
    w2o = np.stack([w2o_rows(m) for m in flat2.instance_transforms])
    out = {}
    for name, fl, osc, pr in (("single", flat, orc.Scene.from_flat(flat), None),
                              ("two-level", flat2, orc.Scene(flat2.nodes, flat2.tri_verts, flat2.instance_offsets, flat2.tlas_start,
                                                             instance_w2o=w2o), pairs)):
        rec, inst = ND.records(orc.HIT_DTYPE, ND.W, ND.H, n_tris=fl.n_tris, pairs=pr)
        n = ND.geometric_normals(fl.tri_verts).astype(np.float64)[rec["prim"]]
        if inst is not None:      # object-space normal -> world: the transpose of the world-to-object rows' 3 x 3 part
            m = w2o.astype(np.float64).reshape(-1, 3, 4)[inst][:, :, :3]
            n = np.einsum("irc,ir->ic", m, n)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        out[name] = (osc, oview, rec, inst, n)
    return out, flat, flat2


def _primary_dirs(orc, oview, w, h):
    lib = orc.load()
    o, d = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    out = np.zeros((w * h, 3))
    for i in range(w * h):
        lib.orc_primary_ray(C.byref(oview), w, h, i % w, i // w, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p))
        out[i] = d
    return out


def test_seed_for_inverts_both_noises_at_every_target(orc):
    lib = orc.load()
    assert len(ND.TARGETS) == 5 + 27 and len(set(ND.TARGETS.values())) == len(ND.TARGETS)
    # pixels in different lanes of a tile, of partial tiles, of the dense image, and rows where py << 11 reaches the top bits
    pixels = ND.PIXELS + ((130, 255), (1919, 1079), (5, 1 << 20), (3, (1 << 21) + 77))
    for name, target in ND.TARGETS.items():
        for px, py in pixels:
            for second in (False, True):
                seed = ND.seed_for(px, py, target, second)
                assert 0 <= seed <= 0xFFFFFFFF
                noise_seed = (seed + 1024) & 0xFFFFFFFF if second else seed
                assert lib.orc_uhash(px, ((py << 11) + noise_seed) & 0xFFFFFFFF) == target, (name, px, py, second)
                u = np.float32(lib.orc_hash_noise(px, py, noise_seed))
                assert u.tobytes() == ND.u_of(target).tobytes(), (name, px, py, second)
    # the vectorised hash the dense leg counts with is the oracle's
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32)
    assert (ND.uhash_np(a, b) == np.array([lib.orc_uhash(int(x), int(y)) for x, y in zip(a, b)], dtype=np.uint32)).all()
    for frame in (0, 0xFFFFFFFF, 0xFFFFFC00):
        for second in (False, True):
            got = ND.image_hashes(ND.W, ND.H, frame, second)
            want = [lib.orc_uhash(i % ND.W, (((i // ND.W) << 11) + frame + (1024 if second else 0)) & 0xFFFFFFFF) for i in range(ND.W * ND.H)]
            assert (got == np.array(want, dtype=np.uint32)).all()


def test_every_target_reaches_what_its_name_claims(orc, capsys):
    lib = orc.load()
    T = {k: ND.classify(v) for k, v in ND.TARGETS.items()}
    with capsys.disabled():
        print("\nwhat each target reaches on the oracle (as u2; as u1 the same u):")
        for name, target in ND.TARGETS.items():
            print("  " + ND.table_row(name, target))
    # u == 0, the smallest u, the last value below 1.0 and both ends of the 128 values that round up to exactly 1.0
    assert T["0"]["u"] == 0 and T["0"]["theta"] == 0 and T["0"]["branch"] == "small"
    assert T["1"]["u"] == np.float32(2.0 ** -32) and T["1"]["branch"] == "small"
    assert T["below-1.0"]["u"] == np.float32(1.0) - np.float32(2.0 ** -24) and not T["below-1.0"]["lz_zero"]
    for name in ("first-1.0", "last-1.0"):
        assert T[name]["u"] == 1.0 and T[name]["lz_zero"] and T[name]["n"] == 4 and T[name]["branch"] == "reduced"
        assert T[name]["theta"] == np.float32(ND.TWO_PI)
    assert ND.u_of(ND.TARGETS["first-1.0"] - 1) < 1.0
    # the small-angle switch and the reduction switch: -256 before, +256 behind; +0 is the last value before 2^-12 (the
    # product u * fl(2 pi) rounds below it) and the first value at 0.75
    assert [T["2^-12%+d" % o]["branch"] for o in (-256, 0, 256)] == ["small", "small", "direct"]
    assert T["2^-12+0"]["theta"] < np.float32(2.0 ** -12) <= T["2^-12+256"]["theta"]
    assert [T["0.75%+d" % o]["branch"] for o in (-256, 0, 256)] == ["direct", "reduced", "reduced"]
    assert T["0.75+0"]["theta"] == np.float32(0.75) and T["0.75+0"]["n"] == 0
    # the quadrant switches: n changes between -256 and +0 at the odd multiples of pi / 4 and not at the even ones
    for k, name in ((1, "pi/4"), (3, "3pi/4"), (5, "5pi/4"), (7, "7pi/4")):
        assert [T["%s%+d" % (name, o)]["n"] for o in (-256, 0, 256)] == [k // 2, k // 2 + 1, k // 2 + 1], name
    for k, name in ((1, "pi/2"), (2, "pi"), (3, "3pi/2")):
        assert [T["%s%+d" % (name, o)]["n"] for o in (-256, 0, 256)] == [k, k, k], name
    for name in ND.CORE_TARGETS:
        assert name in ND.TARGETS
    # the vectorised classifier the dense leg counts with is this one: at every target, its two neighbours and random words
    words = np.array([(v + d) & 0xFFFFFFFF for v in ND.TARGETS.values() for d in (-1, 0, 1)] +
                     list(np.random.default_rng(9).integers(0, 1 << 32, 4000, dtype=np.uint64)), dtype=np.uint32)
    u, small, n = ND.classify_image(words)
    one = [ND.classify(int(v)) for v in words]
    assert u.tobytes() == np.array([c["u"] for c in one], dtype=np.float32).tobytes()
    assert (small == [c["branch"] == "small" for c in one]).all() and (n == [c["n"] for c in one]).all()
    # the classifier's branch is the oracle's: where it says 'small' the oracle returns (theta, 1) in quadrant 0, and the
    # oracle's sine / cosine at every target is glibc's algorithm's value = the correctly rounded one to within one ulp
    s, c = np.zeros(1, dtype=np.float32), np.zeros(1, dtype=np.float32)
    for name, t in T.items():
        lib.orc_sincos(float(t["theta"]), s.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p))
        if t["branch"] == "small":
            assert s[0].tobytes() == t["theta"].tobytes() and c[0] == 1.0, name
        for got, exact in ((s[0], math.sin(float(t["theta"]))), (c[0], math.cos(float(t["theta"])))):
            assert abs(float(got) - exact) <= float(np.spacing(np.float32(abs(exact)))) + 1e-45, name


def test_the_scene_holds_the_normals_the_basis_switches_on(trx, scenes):
    _, flat, flat2 = scenes
    n = ND.geometric_normals(flat.tri_verts)
    assert flat.n_tris == 18 and not flat.has_tlas and flat2.has_tlas
    unit = n / np.sqrt((n.astype(np.float64) ** 2).sum(1))[:, None]
    for axis in range(3):
        for sign in (1.0, -1.0):
            want = np.zeros(3)
            want[axis] = sign
            assert ((unit == want).all(1)).sum() >= 2, (axis, sign)         # both windings of two faces give each axis normal
    z = n[:, 2]
    assert ((z == 0) & ~np.signbit(z)).any() and ((z == 0) & np.signbit(z)).any()          # nz = +0 and nz = -0
    tiny = (z != 0) & (np.abs(unit[:, 2]) < 1e-5)
    assert (z[tiny] > 0).any() and (z[tiny] < 0).any() and (np.abs(z[tiny]) < 1e-29).any()
    near = (np.abs(unit[:, 2]) < 1) & (np.abs(unit[:, 2]) > 0.999)
    assert (z[near] > 0).any() and (z[near] < 0).any()
    det = [np.linalg.det(m.astype(np.float64).reshape(4, 4).T[:3, :3]) for m in flat2.instance_transforms]
    assert min(det) < 0 < max(det)                                           # a mirrored instance among them
    sv = [np.linalg.svd(m.astype(np.float64).reshape(4, 4).T[:3, :3], compute_uv=False) for m in flat2.instance_transforms]
    assert max(s[0] / s[2] for s in sv) > 2                                   # and a non-uniform scale


@pytest.mark.parametrize("name", ["single", "two-level"])
def test_oracle_rays_at_every_target_have_the_definitions_properties(orc, scenes, name):
    """Properties of the definition, not of the code under test (they would show an oracle wrong in the kernel's way): the
    direction is finite, of unit length, in the hemisphere of the normal flipped toward the viewer; at u1 == 1 it lies in the
    tangent plane, at u1 == 0 it is the normal.  Unit length to 2 ulp of 1.0 (2^-23 each): the normalisation rounds the
    squared length (three products, two sums: below 2 ulp of 2^-24 relative, halved by the root), the root, the reciprocal and
    the final product, half an ulp of 2^-24 each - 2.5 * 2^-24 in all."""
    osc, oview, rec, inst, normal = scenes[0][name]
    w, h = ND.W, ND.H
    rd = _primary_dirs(orc, oview, w, h)
    nd = -(normal * rd).sum(1)
    assert np.abs(nd).min() > 1e-4                   # (the flip's sign is the same in binary32 and binary64)
    flipped = normal * np.sign(nd)[:, None]
    n_tangent = n_normal = 0
    for k, (tname, target) in enumerate(ND.TARGETS.items()):
        for second in (False, True):
            px, py = ND.target_pixel(k + second)
            seed = ND.seed_for(px, py, target, second)
            rays = osc.ao_rays(oview, w, h, rec, inst, frame=seed, ao_eps=0.01, tmax=F32_MAX, threads=2)
            d = rays["direction"].astype(np.float64)
            assert np.isfinite(rays["origin"]).all() and np.isfinite(d).all() and (rays["tmax"] == np.float32(F32_MAX)).all()
            assert np.abs(np.sqrt((d * d).sum(1)) - 1.0).max() <= 2 * 2.0 ** -23, (tname, second)
            dn = (d * flipped).sum(1)
            assert dn.min() >= -1e-6, (tname, second, dn.min())
            i = py * w + px
            lib = orc.load()
            u1 = np.float32(lib.orc_hash_noise(px, py, seed))
            u2 = np.float32(lib.orc_hash_noise(px, py, (seed + 1024) & 0xFFFFFFFF))
            assert (u2 if second else u1).tobytes() == ND.u_of(target).tobytes()
            if u1 == 1.0:
                assert abs(dn[i]) <= 1e-6, (tname, second, dn[i])
                n_tangent += 1
            if u1 == 0.0:
                assert dn[i] >= 1 - 1e-6 and np.abs(d[i] - flipped[i]).max() <= 1e-6, (tname, second)
                n_normal += 1
    assert n_tangent >= 2 and n_normal >= 1


def test_orc_ao_rays_is_orc_ao_ray_inst_in_a_loop(orc, scenes):
    for name in ("single", "two-level"):
        osc, oview, rec, inst, _ = scenes[0][name]
        rec = rec.copy()
        rec["t"][5], rec["prim"][11] = np.inf, 0xFFFFFFFF              # two misses: the inert ray
        rec["t"][17] = np.float32(F32_MAX)
        for frame, eps, radius in ((0, 0.01, np.inf), (0xFFFFFC7F, 0.0001, 1.5)):
            want, surface = ao_rays(orc, osc, oview, ND.W, ND.H, rec, inst, frame, eps, radius)
            got = osc.ao_rays(oview, ND.W, ND.H, rec, inst, frame=frame, ao_eps=eps, tmax=float(want["tmax"][0]), threads=3)
            assert got.tobytes() == want.tobytes(), name
            assert (~surface).sum() == 3 and (got.view(np.uint32).reshape(-1, 8)[~surface] == INERT).all()


def test_dense_leg_seeds_show_what_the_leg_is_for(orc):
    """On the oracle alone: over the eight committed seeds the 2^19 rays hold at least 8 in the small-angle branch (about 20
    expected), at least 1000 in each quadrant word n = 0 .. 4 - n == 4 from theta >= 7 pi / 4 up to its top theta == fl(2 pi),
    which only u2 == 1.0 produces and which must be there - and a ray with u1 == 1.0."""
    lib = orc.load()
    assert len(ND.DENSE_SEEDS) == 8 and len(set(ND.DENSE_SEEDS)) == 8
    (p1, h1), (p2, h2) = ND.DENSE_U1_ONE, ND.DENSE_U2_ONE
    assert ND.DENSE_SEEDS[6] == ND.seed_for(*p1, h1) and ND.DENSE_SEEDS[7] == ND.seed_for(*p2, h2, second=True)
    assert np.float32(lib.orc_hash_noise(*p1, ND.DENSE_SEEDS[6])) == 1.0
    assert np.float32(lib.orc_hash_noise(*p2, (ND.DENSE_SEEDS[7] + 1024) & 0xFFFFFFFF)) == 1.0
    n_small, n_quadrant, n_u1_one, n_u2_one = 0, np.zeros(5, dtype=np.int64), 0, 0
    for seed in ND.DENSE_SEEDS:
        u1, _, _ = ND.classify_image(ND.image_hashes(ND.DENSE, ND.DENSE, seed))
        u2, small, n = ND.classify_image(ND.image_hashes(ND.DENSE, ND.DENSE, seed, second=True))
        assert n.min() >= 0 and n.max() <= 4
        n_small += int(small.sum())
        n_quadrant += np.bincount(n, minlength=5)
        n_u1_one += int((u1 == 1.0).sum())
        n_u2_one += int((u2 == 1.0).sum())
    assert n_small >= 8 and (n_quadrant >= 1000).all() and n_u2_one >= 1 and n_u1_one >= 1, (n_small, n_quadrant, n_u1_one, n_u2_one)
