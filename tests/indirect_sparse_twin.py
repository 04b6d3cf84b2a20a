"""numpy twin of the sparse indirect term (include/trx.h: trx_trace_indirect_sparse_dev, trx_value_upsample_dev): THE
DEFINITION, restated from the header's rules in binary32, one operation at a time.

THE SPARSE VALUES.  The grid is the sparse visibility pass's (tests/ao_sparse_twin.py: phase_xy, lo_size, cell_pixels).  Cell
(X, Y) holds the value the dense pass (tests/indirect_twin.py, `indirect` without a base) gives its pixel; +0 where the pixel
lies outside the image or is not a surface pixel.

THE UPSAMPLE.  The window, the surface cells and the accepted cells are trx_ao_upsample_dev's (ao_sparse_twin.ao_upsample);
the cells are visited dy ascending, dx ascending inside, with the weight (radius + 1 - |dy|) * (radius + 1 - |dx|);
num = num + w * u[q], den = den + w for the accepted cells, a cell that is not accepted leaving both as they are; without an
accepted cell the same sums over every surface cell (FALLBACK); without one of those +0 (EMPTY).  A surface pixel gets
base + F, any other pixel its base's bits (+0 without a base)."""
import numpy as np

from ao_sparse_twin import ACCEPTED, EMPTY, FALLBACK, NOT_SURFACE, cell_pixels, lo_size, phase_xy
from ao_visibility_twin import surface_records
from image_twin import surface

MAX_RADIUS = 2
f32 = np.float32


def sparse_values(dense_values_without_base, primary, w, h, stride, phase, n_tris=None):
    """[Wlo * Hlo] float32: the dense pass's values [w * h] (no base) at the cells' pixels, +0 where the pixel is outside the
    image or no surface pixel.  n_tris: the scene's triangle count - the pass reads the scene's tables, so a caller's record
    with prim >= n_tris is no surface pixel (light_twin.surface); None: records the library wrote itself."""
    gx, gy, inside = cell_pixels(w, h, stride, phase)
    dense = np.asarray(dense_values_without_base, dtype=np.float32).reshape(h, w)
    surf = (surface(primary) if n_tris is None else surface_records(primary, n_tris)).reshape(h, w)
    out = np.zeros(gx.shape, dtype=np.float32)
    take = inside.copy()
    take[inside] = surf[gy[inside], gx[inside]]
    out[take] = dense[gy[take], gx[take]]
    return out.reshape(-1)


def value_upsample(primary, normals, lo, w, h, stride, phase, radius, depth_tol, normal_cos, base=None, classes=False):
    """trx_value_upsample_dev: primary [w * h] hit records, normals [w * h, 3] f32 or None, lo [Wlo * Hlo] f32, base [w * h] f32 or
    None -> [w * h] f32 (and, with classes, [w * h] of NOT_SURFACE / ACCEPTED / FALLBACK / EMPTY)."""
    s, r = int(stride), int(radius)
    assert 0 <= r <= MAX_RADIUS
    px0, py0 = phase_xy(s, phase)
    wlo, hlo = lo_size(w, h, s)
    t = np.asarray(primary["t"], dtype=np.float32).reshape(h, w)
    surf = surface(primary).reshape(h, w)
    n = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(h, w, 3)
    tol, cos = f32(depth_tol), f32(normal_cos)
    # the cells: a surface cell carries the full-resolution records of its pixel and the low grid's value
    gx, gy, inside = cell_pixels(w, h, s, phase)
    cx, cy = np.minimum(gx, w - 1), np.minimum(gy, h - 1)            # (clamped for the gather; `inside` masks them out)
    c_surf = inside & surf[cy, cx]
    c_t = t[cy, cx]
    c_u = np.asarray(lo, dtype=np.float32).reshape(hlo, wlo)
    c_n = None if n is None else n[cy, cx]

    def pad(a, fill):
        out = np.full((hlo + 2 * r, wlo + 2 * r) + a.shape[2:], fill, dtype=a.dtype)
        out[r:r + hlo, r:r + wlo] = a
        return out

    p_surf, p_t, p_u = pad(c_surf, False), pad(c_t, f32(0)), pad(c_u, f32(0))
    p_n = None if c_n is None else pad(c_n, f32(0))
    y, x = np.mgrid[0:h, 0:w]
    qx, qy = x // s, y // s
    own_cell = (x - qx * s == px0) & (y - qy * s == py0)             # the pixel is the pixel of its own cell
    num, den = np.zeros((h, w), dtype=np.float32), np.zeros((h, w), dtype=np.float32)
    num_all, den_all = np.zeros((h, w), dtype=np.float32), np.zeros((h, w), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        bound = tol * t                                               # depth_tol * t_p, rounded once
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                wgt = f32((r + 1 - abs(dy - r)) * (r + 1 - abs(dx - r)))
                iy, ix = qy + dy, qx + dx                             # (padded coordinates of cell (qx + dx - r, qy + dy - r))
                sq, tq, uq = p_surf[iy, ix], p_t[iy, ix], p_u[iy, ix]
                ok = sq & (np.abs(tq - t) <= bound)
                if p_n is not None:
                    nq = p_n[iy, ix]
                    dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    ok &= dot >= cos
                if dy == r and dx == r:
                    ok |= own_cell                                    # p itself, unconditionally
                term = wgt * uq                                       # w * u[q], rounded once
                num = np.where(ok, num + term, num)
                den = np.where(ok, den + wgt, den)
                num_all = np.where(sq, num_all + term, num_all)
                den_all = np.where(sq, den_all + wgt, den_all)
        fallback = ~(den > 0)                                         # (the weights are positive: den > 0 iff a cell was accepted)
        num, den = np.where(fallback, num_all, num), np.where(fallback, den_all, den)
        empty = ~(den > 0)
        F = np.where(empty, f32(0), num / np.where(empty, f32(1), den)).astype(np.float32)
        if base is None:
            total, b = F, np.zeros((h, w), dtype=np.float32)
        else:
            b = np.ascontiguousarray(base, dtype=np.float32).reshape(h, w)
            total = (b + F).astype(np.float32)
    out = b.copy().view(np.uint32)                                    # a pixel without a surface: its base's bits copied
    out[surf] = total.view(np.uint32)[surf]
    out = out.view(np.float32).reshape(-1)
    if not classes:
        return out
    cls = np.where(~fallback, ACCEPTED, np.where(empty, EMPTY, FALLBACK))
    return out, np.where(surf, cls, NOT_SURFACE).reshape(-1).astype(np.uint8)
