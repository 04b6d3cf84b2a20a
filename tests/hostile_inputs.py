"""Seeded generators of hostile traversal inputs (numpy only; no oracle, no device): rays, cameras and instance
transforms whose floats are non-finite, out of range, un-normalised or placed exactly on the structures the walks decide
by - a node's quantisation origin, a triangle's plane, the edges of the literal-division shortcuts.  Every generator names
the class of each ray / view / matrix, so tests can report and count by class.

The reference shader clamps a box's entry distance to max(..., 0.0001) (query.hlsl node test).  Three classes are built
to trigger what follows from that clamp, and the tests pin them instead of expecting walk == brute force:
  CLAMP_TMIN   a negative tmin lets brute force accept hits the walk never reaches;
  CLAMP_PLANE  an origin on (or within a rounding of) a triangle's plane has a hit nearer than the clamp;
  CLAMP_DIR    a direction component of magnitude >= 2^12 shrinks every t below the clamp."""
import numpy as np

from helpers import F32_MAX, aimed_rays, random_rays

F = np.float32
FLT_MIN = F(1.17549435e-38)
DENORM_MIN = F(1e-45)

# ---- rays -------------------------------------------------------------------------------------------------------------

# value classes: the value overwrites one to three of a ray's origin / direction components.  The huge and infinite values
# go into origins only: in a direction they belong to CLAMP_DIR and have classes of their own there (dir_3e38, dir_inf).
VALUES = (("nan", F(np.nan), "od"), ("+inf", F(np.inf), "o"), ("-inf", F(-np.inf), "o"), ("+0", F(0.0), "od"),
          ("-0", F(-0.0), "od"), ("denorm_min", DENORM_MIN, "od"), ("1e-39", F(1e-39), "od"), ("flt_min", FLT_MIN, "od"),
          ("+3e38", F(3e38), "o"), ("-3e38", F(-3e38), "o"))
DSCALES = (("dscale_2^-40", -40), ("dscale_2^-12", -12), ("dscale_2^12", 12), ("dscale_2^40", 40))
RANGE_CLASSES = ("tmin_neg", "tmin_nan", "tmin_inf", "tmin_eq_tmax", "tmin_gt_tmax", "tmax_zero", "tmax_neg", "tmax_nan",
                 "tmax_inf")
PLACED = ("origin_on_plane", "node_p", "node_p+ulp", "node_p-ulp", "vertex_along_edge")
RAY_CLASSES = (tuple(v[0] for v in VALUES) + tuple(s[0] for s in DSCALES) + ("dir_zero", "dir_tiny_all", "dir_3e38", "dir_inf") +
               RANGE_CLASSES + PLACED)

CLAMP_TMIN = ("tmin_neg",)
CLAMP_PLANE = ("origin_on_plane", "vertex_along_edge")    # both origins lie on a triangle's plane (a vertex lies on its triangle's)
CLAMP_DIR = ("dscale_2^12", "dscale_2^40", "dir_3e38", "dir_inf")
# A fourth behaviour, found by these generators and not the clamp's: a direction of length about 1e-38 has its hits at t
# near 1e38, where a box's planes q * (e / d) + (p - o) / d (q up to 255) overflow before the triangle test's t does - the
# walk misses what brute force still finds.  One class of its own; the value classes replace at most two direction
# components with a tiny value.
OVERFLOW_DIR = ("dir_tiny_all",)
TAME = "tame"


def _hit_points(o, d, tri_verts, chunk=64):
    """Nearest intersection of every ray (o, d: [R, 3] float64) with the triangles, in float64 (Moeller-Trumbore, both
    faces): (point [R, 3], found [R])."""
    v = np.asarray(tri_verts, dtype=np.float64).reshape(-1, 3, 3)
    v0, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    best = np.full(o.shape[0], np.inf)
    for s in range(0, o.shape[0], chunk):
        oo, dd = o[s:s + chunk, None, :], d[s:s + chunk, None, :]
        with np.errstate(all="ignore"):
            pv = np.cross(dd, e2[None])
            det = (e1[None] * pv).sum(-1)
            inv = 1.0 / det
            tv = oo - v0[None]
            u = (tv * pv).sum(-1) * inv
            qv = np.cross(tv, e1[None])
            w = (dd * qv).sum(-1) * inv
            t = (e2[None] * qv).sum(-1) * inv
            ok = (np.abs(det) > 1e-12) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 1e-3)
        best[s:s + chunk] = np.where(ok, t, np.inf).min(axis=1)
    found = np.isfinite(best)
    return o + d * np.where(found, best, 0.0)[:, None], found


# A unit-length ray that starts a distance s from a plane meets it at t >= s, so an origin kept 1e-3 away from every
# axis-aligned triangle's plane cannot, by that plane, have a hit nearer than the tests' t < 2e-4 exclusion rule.
_PLANE_CLEARANCE = 1e-3


def _flat_coords(v3):
    """Per axis, the sorted coordinates of the triangles that lie in an axis-aligned plane (all three vertices agree)."""
    out = []
    for ax in range(3):
        c = v3[:, :, ax]
        out.append(np.unique(c[(c[:, 0] == c[:, 1]) & (c[:, 1] == c[:, 2]), 0].astype(np.float64)))
    return out


def _clear_of_planes(flat_coords, axis, value):
    c = flat_coords[axis]
    return c.size == 0 or float(np.abs(c - float(value)).min()) > _PLANE_CLEARANCE


def node_origin_values(flat, rng, flat_coords=None):
    """(axis, (p, p + 1 ulp, p - 1 ulp)) of a random node's quantisation origin on a random axis: p - o is +0, or the
    smallest difference either way.  With flat_coords, (node, axis) pairs whose p lies on an axis-aligned triangle's plane
    are drawn again (a box's minimum is a vertex coordinate: in a scene of walls it would be an origin on a plane).
    test_literal_division_shortcut_is_exact_at_its_edges (tests/test_gpu_parity.py) keeps its own inline construction: it
    draws node, axis and its other edge values from ONE generator in one loop, so no shared function called from there
    can reproduce its rays byte for byte, and its rays are what its history was measured on."""
    node_p = flat.nodes[:, 0:3].copy().view(F)
    for _ in range(64):
        ax = int(rng.integers(3))
        pv = node_p[rng.integers(0, node_p.shape[0]), ax]
        if flat_coords is None or _clear_of_planes(flat_coords, ax, pv):
            break
    return ax, (pv, np.nextafter(pv, F(np.inf)), np.nextafter(pv, F(-np.inf)))


def hostile_rays(T, flat, n, seed, tri_verts=None):
    """(rays [n], classes [n] of str): `random_rays` and `aimed_rays` in halves (most of the tame ones hit), every second
    ray hostile, the hostile classes dealt in turn from a seeded start - so every class is present once
    n >= 2 * len(RAY_CLASSES).  tri_verts: the (world-space) triangles to aim at, default flat.tri_verts."""
    rng = np.random.default_rng(seed)
    tv = flat.tri_verts if tri_verts is None else tri_verts
    box = type("B", (), {"tri_verts": np.asarray(tv, dtype=F).reshape(-1, 9)})
    half = n // 2
    rays = np.concatenate([random_rays(T, box, half, seed, zero_dirs=False), aimed_rays(T, tv, n - half, seed + 1)])
    rays = rays[rng.permutation(n)]
    classes = np.full(n, TAME, dtype=object)
    v3 = np.asarray(tv, dtype=F).reshape(-1, 3, 3)
    hostile = np.arange(1, n, 2) if n > 1 else np.arange(n)
    start = int(rng.integers(len(RAY_CLASSES)))
    # hit points of the tame neighbours, for origin_on_plane
    on_plane = [int(i) for k, i in enumerate(hostile) if RAY_CLASSES[(start + k) % len(RAY_CLASSES)] == "origin_on_plane"]
    if on_plane:
        src = np.array([(i - 1) % n for i in on_plane])
        pts, found = _hit_points(rays["origin"][src].astype(np.float64), rays["direction"][src].astype(np.float64), v3)
        # (a tame ray that missed: the centroid of a random triangle, on its plane up to rounding all the same)
        cent = v3[rng.integers(0, v3.shape[0], size=len(on_plane))].astype(np.float64).mean(axis=1)
        plane_origin = dict(zip(on_plane, np.where(found[:, None], pts, cent).astype(F)))
    values = {name: (val, where) for name, val, where in VALUES}
    flat_coords = _flat_coords(v3)
    for k, i in enumerate(hostile):
        c = RAY_CLASSES[(start + k) % len(RAY_CLASSES)]
        classes[i] = c
        o, d = rays["origin"][i], rays["direction"][i]
        if c in values:
            val, where = values[c]
            # (a zero or tiny origin component only on an axis whose plane through 0 holds no triangle: the floor of most
            # scenes lies there, and the ray would belong to CLAMP_PLANE)
            want = int(rng.integers(1, 4))
            allowed = [f for f in range(6 if "d" in where else 3)
                       if f >= 3 or not np.isfinite(val) or abs(float(val)) > 1.0 or _clear_of_planes(flat_coords, f, val)]
            # (never the origin and the direction component of ONE axis: such a ray runs inside the plane x = value, along
            # every box face and triangle edge that lies there - in most scenes many do at 0 - where a box rightly culls
            # what the triangle test's rounding accepts, and walk and brute force differ for a reason that is not the clamp)
            taken = []
            for f in rng.permutation(allowed):
                if len(taken) < want and (f + 3) % 6 not in taken and not (f >= 3 and sum(g >= 3 for g in taken) == 2):
                    taken.append(int(f))
                    (o if f < 3 else d)[f % 3] = val
        elif c.startswith("dscale_"):
            d *= F(2.0) ** F(dict(DSCALES)[c])
        elif c == "dir_zero":
            d[:] = (F(0.0), F(-0.0), F(0.0))[int(rng.integers(3))]
        elif c == "dir_tiny_all":
            d[:] = (FLT_MIN, F(1e-39), DENORM_MIN)[int(rng.integers(3))] * np.where(rng.integers(2, size=3) == 1, F(1), F(-1))
        elif c == "dir_3e38":
            d[rng.integers(3)] = F(3e38) * (1 if rng.integers(2) else -1)
        elif c == "dir_inf":
            d[rng.integers(3)] = F(np.inf) * (1 if rng.integers(2) else -1)
        elif c == "tmin_neg":
            rays["tmin"][i] = (F(-np.inf), F(-3e38), F(-1e6), F(-1.0))[int(rng.integers(4))]
        elif c == "tmin_nan":
            rays["tmin"][i] = F(np.nan)
        elif c == "tmin_inf":
            rays["tmin"][i] = F(np.inf)
        elif c in ("tmin_eq_tmax", "tmin_gt_tmax"):
            tm = F(rng.uniform(0.5, 3.0))
            rays["tmax"][i] = tm
            rays["tmin"][i] = tm if c == "tmin_eq_tmax" else np.nextafter(tm, F(np.inf))
        elif c == "tmax_zero":
            rays["tmax"][i] = (F(0.0), F(-0.0))[int(rng.integers(2))]
        elif c == "tmax_neg":
            rays["tmax"][i] = (F(-1.0), F(-np.inf), F(-1e-45))[int(rng.integers(3))]
        elif c == "tmax_nan":
            rays["tmax"][i] = F(np.nan)
        elif c == "tmax_inf":
            rays["tmax"][i] = F(np.inf)
        elif c == "origin_on_plane":
            o[:] = plane_origin[int(i)]
        elif c.startswith("node_p"):
            ax, vals = node_origin_values(flat, rng, flat_coords)
            o[ax] = vals[PLACED.index(c) - 1]
        elif c == "vertex_along_edge":
            tri = v3[rng.integers(0, v3.shape[0])]
            a, b = int(rng.integers(3)), int(rng.integers(1, 3))
            e = (tri[(a + b) % 3] - tri[a]).astype(np.float64)
            ln = np.linalg.norm(e)
            o[:] = tri[a]
            d[:] = (e / ln).astype(F) if ln > 0 else (F(1), F(0), F(0))
        rays["origin"][i], rays["direction"][i] = o, d
    return rays, classes.astype(str)


def tame_lanes(n_tame):
    """Indices of the tame rays in the batches of `interleaved` / `with_placeholders`: eight to a run of 64, at lanes that
    move with the run (run r: lanes l with l % 8 == r % 8), so over eight runs every lane has held a tame ray."""
    runs = (n_tame + 7) // 8
    idx = np.array([r * 64 + 8 * j + r % 8 for r in range(runs) for j in range(8)])
    return idx[:n_tame], runs * 64


def placeholder_rays(T, n, far=1e6):
    """n copies of a plain miss: an origin far outside any scene of this suite, pointing away from it (finite, unit
    length, inside the range of every shortcut: it reroutes nothing)."""
    rays = np.zeros(n, dtype=T.RAY_DTYPE)
    rays["origin"] = F(far)
    rays["direction"] = F(1.0 / np.sqrt(3.0))
    rays["tmax"] = F(F32_MAX)
    return rays


def interleaved(T, tame, hostile):
    """The tame rays at `tame_lanes`, hostile rays (cycled) in every other lane of each run of 64."""
    idx, total = tame_lanes(tame.shape[0])
    out = np.resize(hostile, total).astype(T.RAY_DTYPE)
    out[idx] = tame
    return out, idx


def with_placeholders(T, tame):
    """The same tame rays at the same indices, a plain miss in every other lane."""
    idx, total = tame_lanes(tame.shape[0])
    out = placeholder_rays(T, total)
    out[idx] = tame
    return out, idx


# ---- cameras ----------------------------------------------------------------------------------------------------------

ALIVE, OFF = "alive:", "off:"
_EYE_OFFSET = 32 * 4        # trx_view: view_inv[16], proj_inv[16], eye[3], ...
_PROJ_OFFSET = 16 * 4


def _poke(view, offset, floats):
    raw = bytearray(bytes(view))
    raw[offset:offset + 4 * len(floats)] = np.asarray(floats, dtype=F).tobytes()
    return bytes(raw)


def decoded_plane(flat, node, child, axis):
    """p + q_lo * e of one child of one node on one axis, in float32 as the walks compute it."""
    b = flat.nodes[node].view(np.uint8)
    p = flat.nodes[node, axis:axis + 1].view(F)[0]
    e = np.array([int(b[12 + axis]) << 23], dtype=np.uint32).view(F)[0]
    return F(p + F(b[32 + 16 * axis + child]) * e)


def hostile_views(T, flat, w, h):
    """[(name, 160 view bytes)]: names start with ALIVE (one eye for all pixels, finite 1/d: the packet test of the primary
    walk stays on) or OFF (every tile must fail its `fits` condition)."""
    pts = flat.tri_verts.reshape(-1, 3)
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    centre, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    dist = 1.2 * diag
    out = []

    # one 8 x 8 tile is the whole of a small image: a narrower field of view keeps its rays in one octant
    wide = 60.0 if min(w, h) >= 16 else 20.0
    oblique = np.array([0.5, 0.4, 0.77])

    def cam(name, eye, look=None, fov=wide):
        eye = [float(F(x)) for x in eye]
        if look is None:     # obliquely (no direction component near zero) towards the side of the scene's centre
            look = np.array(eye, dtype=np.float64) + np.where(centre >= np.array(eye), 1.0, -1.0) * oblique * max(diag, 1.0)
        out.append((ALIVE + name, bytes(T.view_from_camera(eye, [float(x) for x in look], fov, w, h))))

    # exactly axis-aligned view directions: at w = 16, 48 a tile's first column is the image centre, and that tile's rays
    # have a direction component that is zero or a rounding residue beside it (1/d runs from about 1 to 1/eps)
    # (images of one tile cannot hold these two kinds: their rays span octants)
    for name, axis in (("axis+x", (1, 0, 0)), ("axis-x", (-1, 0, 0)), ("axis+z", (0, 0, 1)), ("axis-z", (0, 0, -1))) if min(w, h) >= 16 else ():
        a = np.array(axis, dtype=np.float64)
        eye = np.round(centre - dist * a)            # integers: eye - look_at is exactly along the axis in float32
        cam(name, eye, look=eye + np.round(dist) * a, fov=60.0)
    cam("fov0.01", centre + np.array([0.3, 0.2, 1.0]) * dist, look=centre, fov=0.01)
    if min(w, h) >= 16:
        cam("fov179", centre + np.array([0.3, 0.2, 1.0]) * 0.3 * diag, look=centre, fov=179.0)
    rng = np.random.default_rng(w * 1000 + h)
    node = int(rng.integers(flat.nodes.shape[0]))
    p = flat.nodes[node, 0:3].copy().view(F)
    cam("eye_node_p", p)
    cam("eye_node_p+ulp", np.nextafter(p, F(np.inf)))
    cam("eye_node_p-ulp", np.nextafter(p, F(-np.inf)))
    cam("eye_child_plane", [decoded_plane(flat, node, 0, k) for k in range(3)])
    tri = flat.tri_verts[int(rng.integers(flat.tri_verts.shape[0]))].reshape(3, 3)
    cam("eye_vertex", tri[0])
    cam("eye_in_leaf_box", 0.5 * (tri.min(0).astype(np.float64) + tri.max(0)))
    cam("eye_on_tri_plane", tri.astype(np.float64).mean(0))
    cam("eye_1e6_diagonals", centre + np.array([0.6, 0.48, 0.64]) * 1e6 * diag)
    lo36, hi59 = F(2.0 ** -36), F(2.0 ** 59)
    cam("eye_2^-36", [lo36, np.nextafter(lo36, F(0)), -np.nextafter(lo36, F(1))])
    cam("eye_2^59", [np.nextafter(hi59, F(np.inf)), 0.8 * hi59, 0.6 * hi59], look=centre)
    cam("eye_2^59_below", [hi59, 0.7 * hi59, np.nextafter(hi59, F(0))], look=centre)

    base = T.view_from_camera([float(x) for x in centre + np.array([0.3, 0.2, 1.0]) * dist], [float(x) for x in centre], 60.0, w, h)
    raw = bytes(base)
    eye = np.frombuffer(raw, dtype=F, count=3, offset=_EYE_OFFSET)
    for name, k, val in (("eye_nan_x", 0, np.nan), ("eye_nan_z", 2, np.nan), ("eye_+inf_y", 1, np.inf), ("eye_-inf_x", 0, -np.inf)):
        e = eye.copy()
        e[k] = val
        out.append((OFF + name, _poke(base, _EYE_OFFSET, e)))
    proj = np.frombuffer(raw, dtype=F, count=16, offset=_PROJ_OFFSET).copy()
    proj[[3, 7, 11, 15]] = 0.0                      # vw = row 3 of proj_inv . (cx, cy, 1, 1) = 0 for every pixel
    out.append((OFF + "proj_vw_zero", _poke(base, _PROJ_OFFSET, proj)))
    out.append((OFF + "all_zero", bytes(160)))
    # eye == look_at: trx_view_from_camera refuses it (TRX_ERR_INVALID); an unchecked from_camera (the reference's, the
    # oracle's) normalises a zero vector, so the view it hands over has a view_inv without a finite entry
    nan_view = np.frombuffer(raw, dtype=F).copy()
    nan_view[0:16] = np.nan
    nan_view[32:35] = centre.astype(F)
    out.append((OFF + "eye_is_look_at", nan_view.tobytes()))
    return out


def is_alive(name):
    return name.startswith(ALIVE)


# Views whose every ray walks the WHOLE tree and tests every triangle (tests/test_hostile_inputs.py pins it): a NaN in the
# view reaches all three direction components through the normalisation, every plane distance is a NaN, the shader's
# max / min drop NaN operands, and what is left - max(0.0001) <= tmax - lets every box through; from 1e6 diagonals away the planes' q * a can be absorbed by b, and on some scenes (the
# bistro-class one) every box then passes the same way.  Nothing is hit, but such a frame costs (nodes + triangles) per pixel: tests keep them to small images.
_WHOLE_TREE = (ALIVE + "eye_1e6_diagonals", OFF + "eye_nan_x", OFF + "eye_nan_z", OFF + "proj_vw_zero", OFF + "all_zero",
               OFF + "eye_is_look_at")


def walks_whole_tree(name):
    return name in _WHOLE_TREE


def tile_qualifies(rays_of_tile):
    """The `fits` condition of trace_refill.inc restated: the rays have one origin (bit for bit - a NaN equals itself
    here), one octant after the zero-direction fix, and finite reciprocals of the fixed direction."""
    o = np.ascontiguousarray(rays_of_tile["origin"]).view(np.uint32)
    d = np.ascontiguousarray(rays_of_tile["direction"]).astype(F).copy()
    d[d == 0.0] = F(1.1920929e-7)
    with np.errstate(all="ignore"):
        inv = F(1.0) / d
    octant = d < 0
    return bool((o == o[0]).all() and (octant == octant[0]).all() and np.isfinite(inv).all())


def tiles(w, h, size=8):
    """Pixel indices of every size x size tile of a w x h image (edge tiles smaller)."""
    return [np.array([y * w + x for y in range(ty, min(ty + size, h)) for x in range(tx, min(tx + size, w))])
            for ty in range(0, h, size) for tx in range(0, w, size)]


# ---- instance transforms ----------------------------------------------------------------------------------------------

AFFINE_CLASSES = ("scale_2^-12", "scale_2^12", "scale_1:2^-10:2^10", "mirror", "rot90", "near_singular_shear",
                  "translate_1e6", "identity")


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def hostile_affines(rng, n, spread=4.0):
    """([n, 16] column-major object-to-world matrices, classes [n]): AFFINE_CLASSES dealt in turn."""
    mats, classes = [], []
    for k in range(n):
        c = AFFINE_CLASSES[k % len(AFFINE_CLASSES)]
        A, t = np.eye(3), rng.uniform(-spread, spread, size=3)
        if c == "scale_2^-12":
            A = _rotation(rng) * 2.0 ** -12
        elif c == "scale_2^12":
            A = _rotation(rng) * 2.0 ** 12
        elif c == "scale_1:2^-10:2^10":
            A = _rotation(rng) @ np.diag([1.0, 2.0 ** -10, 2.0 ** 10])
        elif c == "mirror":
            A = _rotation(rng) @ np.diag([-1.0, 1.0, 1.0])
        elif c == "rot90":
            A = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        elif c == "near_singular_shear":
            A = _rotation(rng) @ np.array([[1.0, 1.0, 0.0], [1.0, 1.0 + 1e-6, 0.0], [0.0, 0.0, 1.0]])   # det = 1e-6
        elif c == "translate_1e6":
            A, t = _rotation(rng), np.array([1e6, -1e6, 1e6]) + t
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = A, t
        mats.append(M.T.reshape(16).astype(F))
        classes.append(c)
    return np.stack(mats), np.array(classes)
