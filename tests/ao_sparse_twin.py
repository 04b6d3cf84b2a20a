"""numpy twin of sparse AO visibility (include/trx.h: trx_trace_ao_visibility_sparse_dev, trx_ao_upsample_dev), restated
from the header's rules.

THE SPARSE COUNTS.  Stride s, phase -> (px0, py0) = (phase % s, phase // s); the low grid is ceil(w / s) x ceil(h / s) cells;
cell (X, Y) stands for pixel (X * s + px0, Y * s + py0) and holds that pixel's byte of the dense visibility pass
(tests/ao_visibility_twin.py), NO_SURFACE where the pixel lies outside the image.

THE UPSAMPLE.  The window of a surface pixel (x, y) is the low cells (x // s + dx, y // s + dy), |dx|, |dy| <= radius,
clipped to the low grid.  A cell is a surface cell iff its pixel is inside the image and a surface pixel; it is accepted iff
it is a surface cell that passes the filter's depth and normal tests against the pixel (tests/image_twin.py: binary32,
every operation rounded once, evaluated on the full-resolution records of the cell's pixel), or its pixel is the pixel
itself.  With accepted cells the term is their sums; without, the sums over every surface cell of the window (FALLBACK);
without any of those, {0, 0} (EMPTY).  Comparisons in float, sums in integers - the device must give the same bits."""
import numpy as np

from image_twin import TERM_DTYPE, surface

NO_SURFACE = 0xFF
MAX_STRIDE = 4
MAX_RADIUS = 2
NOT_SURFACE, ACCEPTED, FALLBACK, EMPTY = 0, 1, 2, 3   # a pixel's class (upsample_classes)


def phase_xy(stride, phase):
    assert 1 <= stride <= MAX_STRIDE and 0 <= phase < stride * stride
    return phase % stride, phase // stride


def lo_size(w, h, stride):
    return (w + stride - 1) // stride, (h + stride - 1) // stride


def cell_pixels(w, h, stride, phase):
    """(gx, gy, inside), each [Hlo, Wlo]: the pixel every low cell stands for, and whether it lies inside the image."""
    px0, py0 = phase_xy(stride, phase)
    wlo, hlo = lo_size(w, h, stride)
    gy, gx = np.mgrid[0:hlo, 0:wlo]
    gx, gy = gx * stride + px0, gy * stride + py0
    return gx, gy, (gx < w) & (gy < h)


def sparse_counts(dense_counts, w, h, stride, phase):
    """[Wlo * Hlo] uint8: the dense pass's counts [w * h] subsampled at the cells' pixels, NO_SURFACE outside the image."""
    gx, gy, inside = cell_pixels(w, h, stride, phase)
    dense = np.asarray(dense_counts, dtype=np.uint8).reshape(h, w)
    out = np.full(gx.shape, NO_SURFACE, dtype=np.uint8)
    out[inside] = dense[gy[inside], gx[inside]]
    return out.reshape(-1)


def ao_upsample(primary, normals, counts_lo, w, h, stride, phase, n_samples, radius, depth_tol, normal_cos, classes=False):
    """trx_ao_upsample_dev: primary [w * h] hit records, normals [w * h, 3] f32 or None, counts_lo [Wlo * Hlo] u8 ->
    [w * h] TERM_DTYPE (and, with classes, [w * h] of NOT_SURFACE / ACCEPTED / FALLBACK / EMPTY)."""
    s, r = int(stride), int(radius)
    assert 0 <= r <= MAX_RADIUS
    px0, py0 = phase_xy(s, phase)
    wlo, hlo = lo_size(w, h, s)
    t = np.asarray(primary["t"], dtype=np.float32).reshape(h, w)
    surf = surface(primary).reshape(h, w)
    n = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(h, w, 3)
    tol, cos = np.float32(depth_tol), np.float32(normal_cos)
    # the cells: a surface cell carries the full-resolution records of its pixel and the low grid's count
    gx, gy, inside = cell_pixels(w, h, s, phase)
    cx, cy = np.minimum(gx, w - 1), np.minimum(gy, h - 1)            # (clamped for the gather; `inside` masks them out)
    c_surf = inside & surf[cy, cx]
    c_t = t[cy, cx]
    c_cnt = np.asarray(counts_lo, dtype=np.uint8).reshape(hlo, wlo).astype(np.int64)
    c_n = None if n is None else n[cy, cx]

    def pad(a, fill):
        out = np.full((hlo + 2 * r, wlo + 2 * r) + a.shape[2:], fill, dtype=a.dtype)
        out[r:r + hlo, r:r + wlo] = a
        return out

    p_surf, p_t, p_cnt = pad(c_surf, False), pad(c_t, np.float32(0)), pad(c_cnt, 0)
    p_n = None if c_n is None else pad(c_n, np.float32(0))
    y, x = np.mgrid[0:h, 0:w]
    qx, qy = x // s, y // s
    own_cell = (x - qx * s == px0) & (y - qy * s == py0)             # the pixel is the pixel of its own cell
    total, accepted = np.zeros((h, w), dtype=np.int64), np.zeros((h, w), dtype=np.int64)
    total_all, cells = np.zeros((h, w), dtype=np.int64), np.zeros((h, w), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        bound = tol * t                                               # depth_tol * t_p, rounded once
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                iy, ix = qy + dy, qx + dx                             # (padded coordinates of cell (qx + dx - r, qy + dy - r))
                sq, tq, cq = p_surf[iy, ix], p_t[iy, ix], p_cnt[iy, ix]
                ok = sq & (np.abs(tq - t) <= bound)
                if p_n is not None:
                    nq = p_n[iy, ix]
                    dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    ok &= dot >= cos
                if dy == r and dx == r:
                    ok |= own_cell                                    # p itself, unconditionally
                total += np.where(ok, cq, 0)
                accepted += ok
                total_all += np.where(sq, cq, 0)
                cells += sq
    fallback = accepted == 0
    total = np.where(fallback, total_all, total)
    accepted = np.where(fallback, cells, accepted)
    out = np.zeros(w * h, dtype=TERM_DTYPE)
    out["unoccluded"] = np.where(surf, total, 0).reshape(-1)
    out["samples"] = np.where(surf, accepted * int(n_samples), 0).reshape(-1)
    if not classes:
        return out
    cls = np.where(~fallback, ACCEPTED, np.where(cells > 0, FALLBACK, EMPTY))
    return out, np.where(surf, cls, NOT_SURFACE).reshape(-1).astype(np.uint8)


def class_counts(cls):
    """(surface pixels, accepted, fallback, empty)."""
    cls = np.asarray(cls)
    return (int((cls != NOT_SURFACE).sum()), int((cls == ACCEPTED).sum()), int((cls == FALLBACK).sum()), int((cls == EMPTY).sum()))
