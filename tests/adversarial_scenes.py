"""Seeded generators of degenerate geometry for the builder tests (host: test_builder_adversarial.py, device:
test_gpu_builder_adversarial.py): exact ties of the PLOC merge areas, zero extents, duplicates, areas that underflow
to 0 or overflow to +inf, a box extent that overflows, signed zeros and non-finite coordinates.  Every function returns
float32 vertices [n, 9].

The sizes are the smallest that reach the device build stage (kDevicePlocMinPrims = 32768) and its block edges:
32768 is the threshold itself, 32769 one past it, 40001 no multiple of the 256-thread block."""
import numpy as np

N_THRESHOLD, N_PAST, N_ODD = 32768, 32769, 40001


def soup(n, seed=1):
    """Small random triangles in the cube [-1, 1]^3: the well-behaved scene every case below starts from."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1.0, 1.0, size=(n, 1, 3))
    v = centre + rng.uniform(-0.03, 0.03, size=(n, 3, 3))
    return np.ascontiguousarray(v.reshape(n, 9).astype(np.float32))


def lattice_plane(n=N_THRESHOLD, seed=1):
    """Unit right triangles tiling an integer grid in z = 0 (two per cell, shuffled): every box is a unit square, so the
    union areas tie everywhere, and one axis has no extent at all."""
    side = int(np.ceil(np.sqrt((n + 1) // 2)))
    k = np.arange(n) // 2
    x, y = (k % side).astype(np.float32), (k // side).astype(np.float32)
    upper = (np.arange(n) % 2).astype(bool)
    v = np.zeros((n, 3, 3), dtype=np.float32)
    v[:, 0, 0], v[:, 0, 1] = x, y
    v[:, 1, 0], v[:, 1, 1] = x + 1, y
    v[:, 2, 0], v[:, 2, 1] = x, y + 1
    v[upper, 0, 0], v[upper, 0, 1] = x[upper] + 1, y[upper] + 1
    np.random.default_rng(seed).shuffle(v, axis=0)
    return np.ascontiguousarray(v.reshape(n, 9))


def flat_x_random(n=N_ODD, seed=2):
    """A random soup in the plane x = 0.25: the Morton scale of that axis is 0.  One random triangle in every cell of a
    grid over [-1, 1]^2, in random order, so that no two of them overlap: where coplanar triangles overlap, their hit
    distances differ by an ulp of rounding and the closest one is not well defined between a walk and brute force."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    cell = rng.permutation(side * side)[:n]
    centre = (np.stack([cell % side, cell // side], axis=1) + 0.5) * (2.0 / side) - 1.0
    v = np.empty((n, 3, 3))
    v[:, :, 0] = 0.25
    v[:, :, 1:] = centre[:, None, :] + rng.uniform(-0.45, 0.45, size=(n, 3, 2)) * (2.0 / side)
    return np.ascontiguousarray(v.reshape(n, 9).astype(np.float32))


def dup8(n=N_THRESHOLD, seed=3):
    """Every triangle of a soup of n / 8 eight times over, the copies next to each other."""
    return np.ascontiguousarray(np.repeat(soup(n // 8, seed), 8, axis=0))


def _identical_block(n, block, seed):
    v = soup(n, seed)
    first = n // 3
    v[first:first + block] = v[first]
    return v


def identical_block_512(n=N_PAST, seed=4):
    """A soup in which 512 consecutive triangles are one and the same."""
    return _identical_block(n, 512, seed)


def identical_block_4096(n=N_THRESHOLD, seed=5):
    """A soup in which 4096 consecutive triangles are one and the same."""
    return _identical_block(n, 4096, seed)


def axis_segments_4096(n=N_THRESHOLD, seed=6):
    """A soup with 4096 zero-width segments along x, each the degenerate triangle {(x_i,0,0), (x_i+1,0,0), (x_i+1,0,0)}:
    the union of any two of them has half-area 0."""
    v = soup(n, seed)
    first = n // 3
    x = np.linspace(-1.0, 1.0, 4097, dtype=np.float32)
    seg = np.zeros((4096, 9), dtype=np.float32)
    seg[:, 0], seg[:, 3], seg[:, 6] = x[:-1], x[1:], x[1:]
    v[first:first + 4096] = seg
    return v


def all_identical(n=N_THRESHOLD, seed=7):
    """One triangle n times."""
    return np.ascontiguousarray(np.repeat(soup(1, seed), n, axis=0))


def underflow_1e30(n=N_THRESHOLD, seed=8):
    """The soup scaled by 1e-30: every box half-area underflows to 0."""
    return soup(n, seed) * np.float32(1e-30)


def overflow_1e19(n=N_THRESHOLD, seed=9):
    """The soup scaled by 1e19: the half-areas of the larger unions overflow to +inf."""
    return soup(n, seed) * np.float32(1e19)


def extent_overflow_x(n=N_THRESHOLD, seed=14):
    """The soup with its x coordinates rescaled to [-3e38, 3e38]: every vertex is finite, but the x extent of the root's
    box (6e38) is +inf in binary32, where the encoder's quantisation step must still come out finite."""
    v = soup(n, seed).reshape(n, 3, 3).astype(np.float64)
    x = v[:, :, 0]
    v[:, :, 0] = (2.0 * (x - x.min()) / (x.max() - x.min()) - 1.0) * 3e38
    return np.ascontiguousarray(v.reshape(n, 9).astype(np.float32))


def points_every_50th(n=N_ODD, seed=10):
    """Every 50th triangle of a soup collapsed to its first vertex."""
    v = soup(n, seed)
    v[::50, 3:6] = v[::50, 0:3]
    v[::50, 6:9] = v[::50, 0:3]
    return v


def signed_zero(n=N_THRESHOLD, seed=11):
    """A soup in which about 30 % of the x coordinates are exactly +0.0 in the first half of the triangles and exactly
    -0.0 in the second half: a box minimum over both is +0 or -0 depending on how the minimum is taken."""
    v = soup(n, seed).reshape(n, 3, 3)
    zero = np.random.default_rng(seed + 1000).random((n, 3)) < 0.3
    x = v[:, :, 0]
    x[zero] = np.float32(0.0)
    second = np.zeros((n, 3), dtype=bool)
    second[n // 2:] = True
    x[zero & second] = np.float32(-0.0)
    return np.ascontiguousarray(v.reshape(n, 9))


def one_nan(n=N_THRESHOLD, seed=12):
    """A soup with one coordinate of one triangle NaN."""
    v = soup(n, seed)
    v[n // 2, 4] = np.float32(np.nan)
    return v


def one_inf(n=N_THRESHOLD, seed=13):
    """A soup with one coordinate of one triangle +inf."""
    v = soup(n, seed)
    v[n // 2, 4] = np.float32(np.inf)
    return v


def nested_triangles(n, ratio=1.004):
    """Triangles around the origin, each `ratio` times the size of the one before: every box contains all the smaller
    ones and all the centres coincide.  No merge areas tie where it matters - a cluster's union with ANY smaller one is
    its own box, with a larger one that one's - so PLOC can merge one pair a round whatever it does among equals, and
    the BVH2 is a chain n levels deep: the input for the builder's depth limit (not one of the device cases)."""
    s = (1e-3 * ratio ** np.arange(n)).astype(np.float32)
    v = np.zeros((n, 9), dtype=np.float32)
    v[:, 0], v[:, 1] = -s, -s
    v[:, 3], v[:, 4] = s, -s
    v[:, 7] = s
    return v


FINITE = {
    "lattice_plane": lattice_plane,
    "flat_x_random": flat_x_random,
    "dup8": dup8,
    "identical_block_512": identical_block_512,
    "identical_block_4096": identical_block_4096,
    "axis_segments_4096": axis_segments_4096,
    "all_identical": all_identical,
    "underflow_1e-30": underflow_1e30,
    "overflow_1e19": overflow_1e19,
    "extent_overflow_x": extent_overflow_x,
    "points_every_50th": points_every_50th,
    "signed_zero": signed_zero,
}
NON_FINITE = {"one_nan": one_nan, "one_inf": one_inf}


def camera_for(verts):
    """(eye, look_at, fov in degrees) of a camera that looks at the centre of the vertex bounds, off every axis, from
    outside them; the distance stays where its square is a normal binary32 number (trx_view_from_camera normalises the
    view direction in binary32), so the eye is far outside the 1e-30 scene and inside the 1e19 one.  The point looked at
    is a little off the centre: the centre of the lattice is a lattice vertex, and with it the middle pixel column runs
    along a lattice line, where a ray sits on the shared edge of neighbouring boxes and the quantised node test of any
    CWBVH may drop it (three rays of the frame did) - a property of the walk, not of the tree under test."""
    p = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    centre = 0.5 * (lo + hi) + (hi - lo) * np.array([0.0137, 0.0071, 0.0053])
    distance = min(max(1.1 * float(np.linalg.norm(hi - lo)), 1e-12), 1e15)
    eye = centre + distance * np.array([0.48, 0.37, 0.80]) / np.linalg.norm([0.48, 0.37, 0.80])
    return tuple(float(np.float32(x)) for x in eye), tuple(float(np.float32(x)) for x in centre), 55.0
