"""numpy twin of the value filter (include/trx.h, "the value filter"): the edge-aware a-trous filter over a per-pixel float
plane, restated from the header's rules in binary32 - the taps in the stated order, one operation at a time, a skipped tap
leaving the sums as they are - so the device must give the same bits (tests/test_gpu_value_filter.py).  Also what the CPU
tests measure with it: the taps' shares (`tap_shares`) and the hand-made images both test files use (`hand_made`)."""
import numpy as np

from image_twin import surface

KERNEL = (1, 4, 6, 4, 1)
MAX_LEVELS = 5
HIT = np.dtype([("t", "<f4"), ("prim", "<u4")])
INF = float("inf")
F32_MAX = 3.4028234663852886e38
f32 = np.float32


def _pad(a, r, fill):
    out = np.full((a.shape[0] + 2 * r, a.shape[1] + 2 * r) + a.shape[2:], fill, dtype=a.dtype)
    out[r:r + a.shape[0], r:r + a.shape[1]] = a
    return out


def _accepted(t, surf, n, s, depth_tol, normal_cos):
    """Per tap (dy, dx) in the stated order: (inside the image, accepted), both [h, w] - for surface pixels p."""
    h, w = t.shape
    r = 2 * s
    pt, ps = _pad(t, r, f32(0)), _pad(surf, r, False)
    pin = _pad(np.ones((h, w), dtype=bool), r, False)
    pn = None if n is None else _pad(n, r, f32(0))
    with np.errstate(invalid="ignore", over="ignore"):
        bound = f32(depth_tol) * t                                   # depth_tol * t_p, rounded once
        for dy in range(5):
            for dx in range(5):
                y0, x0 = dy * s, dx * s
                tq, sq, inside = pt[y0:y0 + h, x0:x0 + w], ps[y0:y0 + h, x0:x0 + w], pin[y0:y0 + h, x0:x0 + w]
                ok = sq & (np.abs(tq - t) <= bound)
                if pn is not None:
                    nq = pn[y0:y0 + h, x0:x0 + w]
                    dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    ok &= dot >= f32(normal_cos)
                if dy == 2 and dx == 2:
                    ok = np.ones((h, w), dtype=bool)                 # p itself, unconditionally
                yield dy, dx, inside, ok & inside


def level(primary, normals, u, w, h, j, depth_tol, normal_cos):
    """LEVEL j: the plane u [w*h] f32 -> u' [w*h] f32."""
    s = 1 << j
    t = np.asarray(primary["t"], dtype=np.float32).reshape(h, w)
    surf = surface(primary).reshape(h, w)
    n = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(h, w, 3)
    u2 = np.asarray(u, dtype=np.float32).reshape(h, w)
    pu = _pad(u2, 2 * s, f32(0))
    num = np.zeros((h, w), dtype=np.float32)
    den = np.zeros((h, w), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for dy, dx, _, ok in _accepted(t, surf, n, s, depth_tol, normal_cos):
            wgt = f32(KERNEL[dy] * KERNEL[dx])
            uq = pu[dy * s:dy * s + h, dx * s:dx * s + w]
            term = wgt * uq                                          # w * u[q], rounded once
            num = np.where(ok, num + term, num)
            den = np.where(ok, den + wgt, den)
        out = num / den
    res = u2.copy().view(np.uint32)                                  # a pixel without a surface: its bits copied
    res[surf] = out.view(np.uint32)[surf]
    return res.view(np.float32).reshape(-1)


def value_filter(primary, normals, values, w, h, n_levels, depth_tol, normal_cos, base=None):
    """trx_value_filter_dev: primary [w*h] hit records, normals [w*h, 3] f32 or None, values [w*h] f32, base [w*h] f32 or None
    -> [w*h] f32."""
    u = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    for j in range(int(n_levels)):
        u = level(primary, normals, u, w, h, j, depth_tol, normal_cos)
    if base is None:
        return u
    base = np.ascontiguousarray(base, dtype=np.float32).reshape(-1)
    surf = surface(primary)
    with np.errstate(invalid="ignore", over="ignore"):
        total = base + u
    out = base.copy().view(np.uint32)
    out[surf] = total.view(np.uint32)[surf]
    return out.view(np.float32)


def tap_shares(primary, normals, w, h, j, depth_tol, normal_cos):
    """Of the surface pixels at level j: (the share with both a rejected in-image tap and an accepted non-centre tap, the share
    with a tap outside the image)."""
    t = np.asarray(primary["t"], dtype=np.float32).reshape(h, w)
    surf = surface(primary).reshape(h, w)
    n = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(h, w, 3)
    rejected = np.zeros((h, w), dtype=bool)
    accepted = np.zeros((h, w), dtype=bool)
    outside = np.zeros((h, w), dtype=bool)
    for dy, dx, inside, ok in _accepted(t, surf, n, 1 << j, depth_tol, normal_cos):
        rejected |= inside & ~ok
        outside |= ~inside
        if not (dy == 2 and dx == 2):
            accepted |= ok
    k = max(int(surf.sum()), 1)
    return (rejected & accepted & surf).sum() / k, (outside & surf).sum() / k


def hand_made(w, h, seed, misses=True):
    """(primary, normals [w*h, 3], values, base) of a hand-made w x h image.  Without `misses` every pixel is a surface pixel, so
    taps leave the image at every level; with them misses of both kinds are strewn in.  The records carry a depth step (right
    of the middle column the depth doubles), a normal crease (below the middle row the normal turns), depth and normal jitter
    around the tolerances, and the values -0.0f, one +inf and one NaN."""
    rng = np.random.default_rng(seed)
    n = w * h
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    prim = np.zeros(n, dtype=HIT)
    t = np.where(x > w // 2, 4.0, 2.0) * (1.0 + 0.08 * rng.random((h, w)))
    prim["t"] = t.reshape(-1).astype(np.float32)
    prim["prim"] = rng.integers(0, 40, n).astype(np.uint32)
    nrm = np.where((y > h // 2)[..., None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])) + 0.25 * rng.normal(size=(h, w, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=2)[..., None]).reshape(n, 3).astype(np.float32)
    values = rng.uniform(0.0, 2.0, n).astype(np.float32)
    values[::5] = f32(-0.0)
    base = rng.uniform(0.0, 1.0, n).astype(np.float32)
    base[::7] = f32(-0.0)
    if n > 20:
        values[n // 3], values[(2 * n) // 3] = f32(INF), f32(np.nan)
    if misses:
        kind = rng.random(n)
        prim["t"][kind < 0.10] = f32(INF)
        prim["prim"][kind < 0.10] = 0xFFFFFFFF
        prim["t"][(kind >= 0.10) & (kind < 0.14)] = f32(F32_MAX)          # t = FLT_MAX: not a surface
        prim["prim"][(kind >= 0.14) & (kind < 0.18)] = 0xFFFFFFFF         # a finite t without a triangle: not a surface
    return prim, nrm, values, base


def all_misses(w, h, seed):
    prim, nrm, values, base = hand_made(w, h, seed, misses=False)
    prim["t"], prim["prim"] = f32(INF), 0xFFFFFFFF
    return prim, nrm, values, base


HAND_SIZES = ((1, 1), (7, 3), (33, 9), (70, 37))


def same_bits(got, want):
    """Bit for bit, NaN-ness compared and not the payload: the indices that differ."""
    got, want = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.flatnonzero((gn != wn) | (~gn & (got.view(np.uint32) != want.view(np.uint32))))
