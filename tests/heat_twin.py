"""The twin of the PROFILE_RT heat map (include/trx.h, trx_count_*_per_ray / trx_shade_heat_dev), on numpy and the oracle alone.

THE COLOUR.  `heat_rgba` is the rule of include/trx.h evaluated on numpy float32 arrays: every intermediate is a float32
array, so every operation is one binary32 operation rounded once (numpy's float32 division is the IEEE division), in the
order the rule states them.  Nothing here is fitted to what the device gives.

THE COUNTS.  A ray's n_node / n_tri are the counters the oracle's walk of that ray alone reports, saturated at 65535:
  * primary rays      `Scene.count_per_ray` (orc_count_primary_per_ray);
  * explicit rays     `Scene.trace_rays` on one ray at a time, n_node / n_tri of its stats;
  * AO rays           the rays of tests/ao_visibility_twin.py at tmax = FLT_MAX (what the closest-hit AO pass walks), one at
                      a time; {0, 0} where the primary record is a miss (no ray).  tests/test_heat.py checks that these sum to
                      `trace_ao`'s pass totals before anything relies on them.
"""
import os

import numpy as np

from ao_visibility_twin import ao_rays

HEAT_NODES, HEAT_TRIS = 0, 1
SCALE_NODES, SCALE_TRIS = np.float32(0.002), np.float32(0.01)
COST_DTYPE = np.dtype([("n_node", "<u2"), ("n_tri", "<u2")])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

PALETTE_K = np.array([(0, 2, 91), (0, 108, 251), (0, 221, 221), (51, 221, 0), (255, 252, 0), (255, 180, 0), (255, 104, 0),
                      (226, 22, 0), (191, 0, 83), (145, 0, 65)], dtype=np.float32)
PALETTE = PALETTE_K / np.float32(255.0)   # binary32 k / 255.0f
assert PALETTE.dtype == np.float32

f32 = np.float32


def _step(a, b, v):
    """S(a, b, v): q = clamp((v - a) / (b - a), 0, 1), (q * q) * (3 - 2 * q)."""
    q = (v - a) / (b - a)
    q = np.minimum(np.maximum(q, f32(0.0)), f32(1.0))
    return (q * q) * (f32(3.0) - f32(2.0) * q)


def heat_rgba(cost, which, scale):
    """[n, 4] uint8 of n COST_DTYPE records (or of an integer array of counts: n_node in nodes mode, n_tri in triangles mode)."""
    if getattr(cost, "dtype", None) == COST_DTYPE:
        cost = cost["n_node"] if which == HEAT_NODES else cost["n_tri"]
    count = np.asarray(cost).astype(np.uint32)
    scale = f32(scale)
    assert np.isfinite(scale) and scale >= 0
    with np.errstate(over="ignore", invalid="ignore"):
        x = ((count * np.uint32(8)) if which == HEAT_NODES else count).astype(np.float32) * scale
        s = x * f32(10.0)
        cur = np.minimum(s, f32(9.0)).astype(np.int32)   # min((int)s, 9): truncation; s >= 9 (+inf included) gives 9
        prv, nxt = np.maximum(cur - 1, 0), np.minimum(cur + 1, 9)
        c = cur.astype(np.float32)
        lo = _step(c - f32(0.8), c + f32(0.8), s)
        hi = _step((c + f32(1.0)) - f32(0.8), (c + f32(1.0)) + f32(0.8), s)
        wc, wp, wn = lo * (f32(1.0) - hi), f32(1.0) - lo, hi
        out = np.full((count.size, 4), 255, dtype=np.uint8)
        for ch in range(3):
            r = (wc * PALETTE[cur, ch] + wp * PALETTE[prv, ch]) + wn * PALETTE[nxt, ch]
            r = np.minimum(np.maximum(r, f32(0.0)), f32(1.0))
            assert r.dtype == np.float32
            out[:, ch] = np.floor(r * f32(255.0) + f32(0.5)).astype(np.uint8)
    return out


def pack(n_node, n_tri):
    out = np.zeros(len(n_node), dtype=COST_DTYPE)
    out["n_node"], out["n_tri"] = np.minimum(n_node, 65535), np.minimum(n_tri, 65535)
    return out


def primary_cost(osc, oview, w, h, sem):
    """[w * h] COST_DTYPE in pixel order."""
    nn, nt = osc.count_per_ray(oview, w, h, sem=sem)
    return pack(nn, nt)


def rays_cost(osc, rays, sem, which=None):
    """COST_DTYPE of the rays `which` (indices; default all), each walked alone."""
    idx = np.arange(rays.shape[0]) if which is None else np.asarray(which)
    nn, nt = np.zeros(idx.size, dtype=np.int64), np.zeros(idx.size, dtype=np.int64)
    for k, i in enumerate(idx):
        _, st = osc.trace_rays(rays[i:i + 1], sem=sem, threads=1)
        nn[k], nt[k] = st.n_node, st.n_tri
    return pack(nn, nt)


def ao_cost(orc, osc, oview, w, h, primary, sem, frame, ao_eps):
    """([w * h] COST_DTYPE in pixel order, surface mask): the AO rays of seed `frame`, each walked alone; {0, 0} off the
    surface.  (Scenes without instance transforms: the primary records carry no instance ids.)"""
    rays, surface = ao_rays(orc, osc, oview, w, h, primary, None, frame, ao_eps, float("inf"))
    out = np.zeros(w * h, dtype=COST_DTYPE)
    idx = np.flatnonzero(surface)
    out[idx] = rays_cost(osc, rays, sem, idx)
    return out, surface


def golden(orc, name):
    """(fixture, oracle scene over its vertex-format triangles, oracle view, w, h)."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    osc = orc.Scene(g["nodes"], g["tri_verts"], g["instance_offsets"], int(g["tlas_start"]))
    return g, osc, orc.view_from_bytes(g["view"].tobytes()), int(g["width"]), int(g["height"])
