"""The noise-driven ray generators at chosen hash values: shared by tests/test_noise_domain.py (the oracle alone) and
tests/test_gpu_noise_domain.py (the device against the oracle).  No pytest in here.

Every stochastic pass draws u1 = hash_noise(px, py, seed) and u2 = hash_noise(px, py, seed + 1024), u = (float)uhash * 2^-32.
uhash is a bijection of its mixed word (odd multipliers, xorshifts), so for any pixel and any wanted 32-bit hash value there
is exactly one seed that produces it: `seed_for` computes it.  `TARGETS` names the hash values at which the generators can go
wrong (u == 0, u == 1.0f, the small-angle branch of the sine / cosine, its reduction switch, the quadrant switches), and
`classify` restates in Python integers and binary64 which branch a value reaches, so that a test asserts it instead of
trusting the name.  The scenes and the primary records are hand-made: every *_rays_dev entry point takes the caller's
records, so they need not be real hits."""
import math

import numpy as np

M32 = 0xFFFFFFFF
MUL_A, MUL_B = 1597334673, 3812015801            # uhash(a, b) mixes a * MUL_A ^ b * MUL_B
MUL_1, MUL_2 = 0x7feb352d, 0x846ca68b
INV_B, INV_1, INV_2 = pow(MUL_B, -1, 1 << 32), pow(MUL_1, -1, 1 << 32), pow(MUL_2, -1, 1 << 32)
SECOND = 1024                                    # the second noise's seed offset
INVALID = 0xFFFFFFFF


# ---- the hash, forwards (numpy, for counting over whole images) and backwards ------------------------------------------------

def uhash_np(a, b):
    """uhash over uint32 arrays (tests/test_noise_domain.py holds it to orc_uhash)."""
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    x = (a * np.uint32(MUL_A)) ^ (b * np.uint32(MUL_B))
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(MUL_1)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(MUL_2)
    return x ^ (x >> np.uint32(16))


def image_hashes(w, h, frame, second=False):
    """[w * h] uint32 in pixel order: the uhash behind hash_noise(px, py, frame [+ 1024])."""
    py, px = np.divmod(np.arange(w * h, dtype=np.uint32), np.uint32(w))
    seed = np.uint32((int(frame) + (SECOND if second else 0)) & M32)
    return uhash_np(px, (py << np.uint32(11)) + seed)


def seed_for(px, py, target, second=False):
    """The 32-bit `frame` for which hash_noise(px, py, frame) - with `second`, hash_noise(px, py, frame + 1024) - has
    uhash == target."""
    x = int(target) & M32
    x ^= x >> 16                                  # undo x ^= x >> 16
    x = (x * INV_2) & M32
    x ^= (x >> 15) ^ (x >> 30)                    # undo x ^= x >> 15
    x = (x * INV_1) & M32
    x ^= x >> 16
    b = ((x ^ (int(px) * MUL_A)) * INV_B) & M32
    return (b - (int(py) << 11) - (SECOND if second else 0)) & M32


# ---- the targets -------------------------------------------------------------------------------------------------------------

TWO_PI = 6.28318530717958647692
THETAS = (("2^-12", 2.0 ** -12), ("0.75", 0.75), ("pi/4", math.pi / 4), ("pi/2", math.pi / 2), ("3pi/4", 3 * math.pi / 4),
          ("pi", math.pi), ("5pi/4", 5 * math.pi / 4), ("3pi/2", 3 * math.pi / 2), ("7pi/4", 7 * math.pi / 4))


def _targets():
    t = {"0": 0, "1": 1, "below-1.0": 0xFFFFFF7F, "first-1.0": 0xFFFFFF80, "last-1.0": 0xFFFFFFFF}
    for name, theta in THETAS:
        at = math.floor(theta / TWO_PI * 2.0 ** 32)
        for off in (-256, 0, 256):
            t["%s%+d" % (name, off)] = at + off
    return t


TARGETS = _targets()
# the closest-hit passes, the bounce and the sparse passes take these (test_gpu_noise_domain.py, 4c / 4f)
CORE_TARGETS = ("0", "1", "first-1.0", "last-1.0", "2^-12+0", "0.75+0", "pi/4+0", "3pi/4+0", "5pi/4+0", "7pi/4+0")


# ---- the classifier: orc_sincos's branches in Python integers and binary64 ------------------------------------------------------

def _f32_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def u_of(target):
    """(float)uhash * 2^-32 as binary32: one rounding of the integer, then an exact scaling."""
    return np.float32(np.float32(np.uint32(target)) * np.float32(1.0 / 4294967296.0))


def classify(target):
    """What a hash value reaches as u2: {u, theta (binary32), branch: 'small' (top < 0x398: sp = theta, cp = 1) | 'direct'
    (no reduction) | 'reduced' (top >= 0x3f4), n (the quadrant word, before & 3), lz_zero (as u1: 1 - u == 0)}."""
    u = u_of(target)
    theta = np.float32(u * np.float32(TWO_PI))
    top = (_f32_bits(theta) >> 20) & 0x7ff
    n = 0
    if top >= 0x3f4:
        q = float(theta) * float.fromhex("0x1.45F306DC9C883p+23")      # binary64, as the C text
        n = (int(q) + 0x800000) >> 24
    branch = "small" if top < 0x398 else "reduced" if top >= 0x3f4 else "direct"
    return {"u": u, "theta": theta, "branch": branch, "n": n, "lz_zero": bool(np.float32(1.0) - u == 0)}


def classify_image(hashes):
    """classify over a uint32 array: (u [n] f32, small [n] bool, n [n] int) - the same statements, vectorised."""
    u = hashes.astype(np.float32) * np.float32(1.0 / 4294967296.0)
    theta = (u * np.float32(TWO_PI)).astype(np.float32)
    top = (theta.view(np.uint32) >> np.uint32(20)) & np.uint32(0x7ff)
    q = theta.astype(np.float64) * float.fromhex("0x1.45F306DC9C883p+23")
    n = np.where(top >= 0x3f4, (q.astype(np.int64) + 0x800000) >> 24, 0)
    return u, top < 0x398, n


def table_row(name, target):
    c = classify(target)
    return "%-12s 0x%08X  u %-13.9g theta %-13.9g %-8s n %d" % (name, target, float(c["u"]), float(c["theta"]), c["branch"], c["n"])


# ---- the hand-made scene -----------------------------------------------------------------------------------------------------

def scene_verts():
    """([18, 9] float32 vertices, object counts).  Twelve axis-aligned triangles: the faces x = 0, y = 0, z = 0 and their
    copies at 1, each in both windings, so the geometric normals cross(e1, e2) are +-x, +-y, +-z with exact zeros of both
    signs in the other components (nz is exactly +-1 after the normalisation for the z faces, +0 or -0 for the others).  Six
    tilted triangles: |nz| tiny of either sign (1e-6: a normal float; 1e-30: squared it underflows), and nz a hair from -1 and
    +1, where the orthonormal basis takes its other branch."""
    tris = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for k, at in enumerate((0.0, 1.0)):
            p0, p1, p2 = np.zeros(3), np.zeros(3), np.zeros(3)
            p0[axis] = p1[axis] = p2[axis] = at
            p0[u], p0[v] = -0.5 + 0.25 * k, -0.25            # (edges of length 1 and 2: the normal's length is exactly 2)
            p1[u], p1[v] = p0[u] + (1.0 if k == 0 else -1.0), p0[v]
            p2[u], p2[v] = p0[u], p0[v] + (2.0 if axis != 1 else -2.0)
            tris.append(np.concatenate([p0, p1, p2]))
            tris.append(np.concatenate([p0, p2, p1]))        # the other winding
    for eps in (1e-6, -1e-6, 1e-30, -1e-30):                 # normal (-1, 0, eps)
        tris.append(np.array([0, 0, 0, 0, 1, 0, eps, 0, 1]))        # (from the origin: e2.x is eps itself)
    for sgn in (1.0, -1.0):                                  # normal (1e-4, 0, -+1) after the cross product
        tris.append(np.array([0, 0, 0.2 * sgn, 0, sgn, 0.2 * sgn, 1, 0, 0.2 * sgn + 1e-4]))
    verts = np.array(tris, dtype=np.float32)
    return verts, [12, 6]


def geometric_normals(tri_verts):
    """cross(e1, e2), e1 = v0 - v1, e2 = v2 - v0, in binary32 with the oracle's operation order: [n, 3], not normalised."""
    v = np.asarray(tri_verts, dtype=np.float32).reshape(-1, 3, 3)
    e1, e2 = v[:, 0] - v[:, 1], v[:, 2] - v[:, 0]
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(np.float32)


CAMERA = ((0.37, 0.81, 2.3), (0.05, 0.1, 0.0), 60.0)      # eye, look-at, fov: no primary direction lies in a face's plane
W, H = 20, 12                                             # six 8 x 8 tiles, the right and the bottom ones partial
DENSE = 256                                               # the dense leg's image is DENSE x DENSE
T_VALUES = (0.5, 1.0, 3.75, 0.001, 100.0)                 # the records' t: finite, positive
# the target pixel, rotated over lane positions: corners of a tile, its inside, the partial tiles at the right and the bottom
PIXELS = ((0, 0), (7, 7), (3, 5), (8, 0), (19, 11), (17, 9), (12, 8), (5, 10), (15, 3), (19, 0))


def target_pixel(k):
    return PIXELS[k % len(PIXELS)]


def single_level(T):
    """The flat scene of scene_verts()."""
    verts, counts = scene_verts()
    return T.flat_build(verts, counts)


def instance_matrices():
    """[5, 16] column-major object-to-world matrices: the identity, a mirror (negative determinant), a non-uniform scale, a
    rotation about a skew axis with a scale, and a mirrored non-uniform scale."""
    def mat(A, t):
        M = np.eye(4)
        M[:3, :3] = A
        M[:3, 3] = t
        return M.T.reshape(16)
    c, s = math.cos(0.7), math.sin(0.7)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    return np.array([mat(np.eye(3), (0, 0, 0)), mat(np.diag([-1.0, 1.0, 1.0]), (1.5, 0.0, -0.5)), mat(np.diag([2.0, 0.5, 1.25]), (-1.0, 0.5, 0.0)),
                     mat(rot * 0.8, (0.2, -0.7, 0.4)), mat(rot @ np.diag([1.0, -3.0, 0.25]), (0.0, 1.0, 1.0))], dtype=np.float32)


def two_level(T):
    """(flat, [n_pairs, 2] (TLAS primitive, triangle of its BLAS) in the flat scene's numbering): the two objects of
    scene_verts() under instance_matrices(), objects alternating."""
    verts, counts = scene_verts()
    o2w = instance_matrices()
    inst_obj = np.array([k % len(counts) for k in range(o2w.shape[0])], dtype=np.uint32)
    flat = T.flat_build_instanced(verts, counts, inst_obj, o2w)
    bts = flat.blas_tri_start
    blas_of_offset = {int(off): b for b, off in enumerate(sorted(set(int(x) for x in flat.instance_offsets)))}
    pairs = []
    for k in range(flat.instance_offsets.size):
        b = blas_of_offset[int(flat.instance_offsets[k])]
        pairs += [(k, p) for p in range(int(bts[b]), int(bts[b + 1]))]
    return flat, np.array(pairs, dtype=np.uint32)


def records(hit_dtype, w, h, n_tris=None, pairs=None, shift=0):
    """Hand-made primary records in pixel order: every pixel a surface, prim cycling over the triangles (or, with `pairs`,
    (instance, prim) over the pairs), t cycling over T_VALUES with another period.  Returns (records, instance ids or None)."""
    i = np.arange(w * h) + shift
    rec = np.zeros(w * h, dtype=hit_dtype)
    rec["t"] = np.array(T_VALUES, dtype=np.float32)[(i * 3 + i // 7) % len(T_VALUES)]
    if pairs is None:
        rec["prim"] = i % n_tris
        return rec, None
    pick = pairs[i % pairs.shape[0]]
    rec["prim"] = pick[:, 1]
    return rec, np.ascontiguousarray(pick[:, 0], dtype=np.uint32)


# ---- the dense leg's seeds ---------------------------------------------------------------------------------------------------
# Chosen on the CPU (tests/test_noise_domain.py asserts what they must show, on the oracle alone): six plain seeds, one near
# the top of the 32-bit range among them, and two made by seed_for: DENSE_SEEDS[6] gives pixel (201, 77) u1 == 1.0f (hash
# 0xFFFFFFC3), DENSE_SEEDS[7] gives pixel (130, 255) u2 == 1.0f (hash 0xFFFFFFFF: theta == fl(2 pi), the top of n == 4).
DENSE_U1_ONE = ((201, 77), 0xFFFFFFC3)
DENSE_U2_ONE = ((130, 255), 0xFFFFFFFF)
DENSE_SEEDS = (0, 1, 7, 1000, 0x9E3779B9, 0xFFFFFE00, 0x8B798F02, 0xD2E43296)
