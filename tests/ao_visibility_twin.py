"""The twin of the AO visibility pass (include/trx.h, trx_ao_rays_dev / trx_trace_ao_visibility_dev), on the oracle alone.

THE DEFINITION.  For a surface pixel and a seed: the AO ray's (o, d) is what the oracle's `orc_ao_ray_inst` builds from the
pixel's primary record; the ray is orc_ray{o, tmin 0, d, tmax} with tmax = the AO radius (+inf stored as FLT_MAX);
`OracleScene.trace_rays` walks it; it is occluded when the answer's prim is not 0xFFFFFFFF.  A pixel's count is the number
of its samples (seeds frame0 .. frame0 + n_samples - 1) that are NOT occluded; a pixel whose primary record is a miss
carries the inert ray (all words 0, tmax = -1) and the count NO_SURFACE.

CALLER RECORDS (include/trx.h): the pass takes its records from the caller.  A record is a surface record of the scene iff
t < FLT_MAX and prim < n_tris; every other record - whatever its words hold - is a miss.  On a transformed scene an
instance id >= n_instances selects no row: the object-space normal is used as it is.  `surface_records` is that rule here;
`orc_ao_ray_inst` states it a second time, and `ao_rays` asserts that the two agree on every record.

Thresholding the closest-hit AO record's t against the radius is NOT the definition: at t == radius the tie rule of the
semantics word decides, and a walk with a shorter tmax culls node boxes the long walk enters.

`orc_ao_ray_inst` is not among oracle/binding.py's wrappers; it is an exported symbol whose prototype the binding sets, and
is called here through ctypes."""
import ctypes as C

import numpy as np

INVALID = 0xFFFFFFFF
NO_SURFACE = 0xFF
F32_MAX = np.float32(3.4028234663852886e38)
THREADS = 4   # the oracle's workers per call: a few thousand rays a call, many calls (0 = one per core of the machine)


def stored_tmax(ao_radius):
    """The tmax the rays carry: the radius, +inf stored as FLT_MAX."""
    r = np.float32(ao_radius)
    assert r > 0
    return F32_MAX if np.isinf(r) else r


def surface_records(primary, n_tris):
    """The caller-record rule: [n] bool, t < FLT_MAX and prim < n_tris (unsigned: 0xFFFFFFFF is never below it)."""
    return (primary["t"] < F32_MAX) & (primary["prim"].astype(np.uint64) < np.uint64(n_tris))


def record_map(w, h, shard=(0, 1, 0)):
    """(pixel ids y * w + x, record indices) of the pixels of `shard` = (index, count[, layout]) inside the image, and the
    number of records the buffer holds (image layout: w * h; TRX_LAYOUT_SHARD: the shard's tiles * 64)."""
    index, count = shard[0], max(shard[1], 1)
    compact = len(shard) > 2 and shard[2] == 1
    tx, ty = (w + 7) // 8, (h + 7) // 8
    py, px = np.divmod(np.arange(w * h, dtype=np.int64), w)
    tile = (py // 8) * tx + px // 8
    mine = tile % count == index
    local = tile // count
    rec = np.where(compact, local * 64 + (py & 7) * 8 + (px & 7), py * w + px)
    n_local = (tx * ty - index + count - 1) // count if tx * ty > index else 0
    return np.flatnonzero(mine), rec[mine], (n_local * 64 if compact else w * h)


def ao_rays(orc, osc, oview, w, h, primary, primary_inst, frame, ao_eps, ao_radius):
    """([w * h] rays in pixel order, surface mask): the twin's ray of every pixel for seed `frame`; the inert ray where the
    primary record is a miss.  Seeds are 32-bit words: `frame` is taken mod 2^32, as the device's frame0 + f wraps."""
    lib = orc.load()
    frame = int(frame) & 0xFFFFFFFF
    rays = np.zeros(w * h, dtype=orc.RAY_DTYPE)
    rays["tmax"] = np.float32(-1.0)
    surface = np.zeros(w * h, dtype=bool)
    o, d = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    po, pd = o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)
    tmax = stored_tmax(ao_radius)
    sc, vw = C.byref(osc.c), C.byref(oview)
    rule = surface_records(primary, int(osc.c.n_tris))
    for i in np.flatnonzero(primary["t"] < F32_MAX):                   # (the oracle decides on prim for itself)
        inst = int(primary_inst[i]) if primary_inst is not None else INVALID
        ok = lib.orc_ao_ray_inst(sc, vw, w, h, int(i % w), int(i // w), orc.HitC(float(primary["t"][i]), int(primary["prim"][i])),
                                 inst, int(frame), float(ao_eps), po, pd)
        assert ok == int(rule[i]), "the oracle and the twin disagree on record %d" % i
        if not ok:
            continue
        rays["origin"][i] = o
        rays["direction"][i] = d
        rays["tmax"][i] = tmax
        surface[i] = True
    return rays, surface


def visibility_counts(orc, osc, oview, w, h, primary, primary_inst, sem, frame0, n_samples, ao_eps, ao_radius):
    """[w * h] uint8 in pixel order: unoccluded samples per surface pixel, NO_SURFACE elsewhere."""
    counts = np.full(w * h, NO_SURFACE, dtype=np.uint8)
    for f in range(n_samples):
        rays, surface = ao_rays(orc, osc, oview, w, h, primary, primary_inst, frame0 + f, ao_eps, ao_radius)
        if f == 0:
            counts[surface] = 0
        hits, _ = osc.trace_rays(rays, sem=sem, threads=THREADS)
        assert (hits["prim"][~surface] == INVALID).all(), "an inert ray committed a hit"
        counts[surface] += (hits["prim"][surface] == INVALID).astype(np.uint8)
    return counts


def shares(counts, n_samples):
    """(partly occluded, fully occluded, fully open) as shares of the surface pixels, and NO_SURFACE as a share of all."""
    surf = counts[counts != NO_SURFACE]
    n = max(surf.size, 1)
    return (np.count_nonzero((surf > 0) & (surf < n_samples)) / n, np.count_nonzero(surf == 0) / n,
            np.count_nonzero(surf == n_samples) / n, np.count_nonzero(counts == NO_SURFACE) / max(counts.size, 1))


# ---- the cases both test files use --------------------------------------------------------------------------------
# Finite radii were picked with the oracle (tests/test_ao_visibility.py asserts what makes them non-vacuous at 8 samples:
# partly occluded, fully occluded and fully open pixels all present): a radius is an input, not a tolerance.
GOLDEN_RADIUS = {"cornell_64": 1.4, "cornell_tlas_48": 1.4}
INSTANCED_RADIUS = 1.6
INSTANCED_SIZE = (72, 48)


def golden_case(T, orc, name):
    """(oracle scene, oracle view, w, h, fixture) of a golden fixture."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    osc = orc.Scene(g["nodes"], g["tri_verts"], g["instance_offsets"], int(g["tlas_start"]))
    return osc, orc.view_from_bytes(g["view"].tobytes()), int(g["width"]), int(g["height"]), g


def instanced_case(T, orc, w2o=None):
    """(flat, product view, oracle scene, oracle view, w, h): fourteen transformed instances of the Cornell-class objects
    seen from a corner of their box.  w2o: the world-to-object rows to give the oracle (the device's own on the GPU;
    default: helpers.w2o_rows of every instance)."""
    from helpers import instanced_scene, w2o_rows
    flat, _, world, _, _ = instanced_scene(T, seed=3, n_instances=14, tris_per_object=0, kind="cornell", spread=1.0)
    if w2o is None:
        w2o = np.stack([w2o_rows(m) for m in flat.instance_transforms])
    osc = orc.Scene(flat.nodes, flat.tri_verts, flat.instance_offsets, flat.tlas_start, instance_w2o=w2o)
    lo, hi = world.reshape(-1, 3).min(0), world.reshape(-1, 3).max(0)
    w, h = INSTANCED_SIZE
    view = T.view_from_camera((hi + 0.1 * (hi - lo)).tolist(), (0.5 * (lo + hi)).tolist(), 80.0, w, h)
    return flat, view, osc, orc.view_from_bytes(bytes(view)), w, h
