"""numpy twin of the frame's image passes (include/trx.h, "the frame's image"): the edge-aware AO filter and the three
shades, restated from the header's definitions.  The filter compares in binary32 and sums in integers, the shades divide
once in binary32 and then take the host's colour code - glibc's powf, called through ctypes (np.power may take a SIMD
variant with other roundings) - so the device must give the same bits (tests/test_gpu_image.py)."""
import ctypes as C
import itertools

import numpy as np

F32_MAX = np.float32(3.4028234663852886e38)
MISS_PRIM = 0xFFFFFFFF
AO_NO_SURFACE = 0xFF
TERM_DTYPE = np.dtype([("unoccluded", "<u2"), ("samples", "<u2")])

_libm = C.CDLL("libm.so.6")
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]


def codes(col):
    """The 8-bit colour code of binary32 colours: (uint8)(uint32)(powf(col, 2.2f) * 255.0f) as the reference's host
    computes it, 0 for col < 0 or NaN, 255 for col >= 1."""
    col = np.ascontiguousarray(col, dtype=np.float32)
    flat = col.reshape(-1)
    out = np.zeros(flat.shape, dtype=np.uint8)
    out[flat >= np.float32(1.0)] = 255
    mid = np.flatnonzero((flat >= np.float32(0.0)) & (flat < np.float32(1.0)))
    uniq, inverse = np.unique(flat[mid], return_inverse=True)
    p = np.array(list(map(_libm.powf, uniq.tolist(), itertools.repeat(2.2))), dtype=np.float32)
    out[mid] = (p * np.float32(255.0)).astype(np.uint32).astype(np.uint8)[inverse]
    return out.reshape(col.shape)


def codes_from_table(thr, col):
    """What the device does: the number of k >= 1 with col >= thr[k]."""
    col = np.ascontiguousarray(col, dtype=np.float32).reshape(-1)
    thr = np.asarray(thr, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (col[:, None] >= thr[None, 1:]).sum(1).astype(np.uint8)


def surface(primary):
    return (primary["t"] < F32_MAX) & (primary["prim"] != MISS_PRIM)


def ao_filter(primary, normals, counts, w, h, n_samples, radius, depth_tol, normal_cos):
    """trx_ao_filter_dev: primary [w*h] hit records, normals [w*h, 3] f32 or None, counts [w*h] u8 -> [w*h] TERM_DTYPE."""
    t = np.asarray(primary["t"], dtype=np.float32).reshape(h, w)
    surf = surface(primary).reshape(h, w)
    cnt = np.asarray(counts, dtype=np.uint8).reshape(h, w).astype(np.int64)
    n = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(h, w, 3)
    r = int(radius)
    tol = np.float32(depth_tol)
    cos = np.float32(normal_cos)

    def pad(a, fill):
        out = np.full((h + 2 * r, w + 2 * r) + a.shape[2:], fill, dtype=a.dtype)
        out[r:r + h, r:r + w] = a
        return out

    pt, ps, pc = pad(t, np.float32(0)), pad(surf, False), pad(cnt, 0)
    pn = None if n is None else pad(n, np.float32(0))
    total = np.zeros((h, w), dtype=np.int64)
    accepted = np.zeros((h, w), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        bound = tol * t                                       # depth_tol * t_p, rounded once
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                tq, sq, cq = pt[dy:dy + h, dx:dx + w], ps[dy:dy + h, dx:dx + w], pc[dy:dy + h, dx:dx + w]
                ok = sq & (np.abs(tq - t) <= bound)
                if pn is not None:
                    nq = pn[dy:dy + h, dx:dx + w]
                    dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    ok &= dot >= cos
                if dy == r and dx == r:
                    ok = np.ones((h, w), dtype=bool)          # p itself, unconditionally
                total += np.where(ok, cq, 0)
                accepted += ok
    out = np.zeros(w * h, dtype=TERM_DTYPE)
    out["unoccluded"] = np.where(surf, total, 0).reshape(-1)
    out["samples"] = np.where(surf, accepted * int(n_samples), 0).reshape(-1)
    return out


def _rgba(col):
    c = codes(col).reshape(-1)
    out = np.empty((c.size, 4), dtype=np.uint8)
    out[:, 0] = out[:, 1] = out[:, 2] = c
    out[:, 3] = 255
    return out


def shade_reference(primary, ao):
    """The reference's shading, the arithmetic of the command line's save_png: 1 / t where the primary ray missed, else
    ao.t / (1 + ao.t), 1 where the AO ray reached nothing."""
    t = np.asarray(primary["t"], dtype=np.float32)
    at = np.asarray(ao["t"], dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        miss = np.float32(1.0) / t
        term = np.where(at < F32_MAX, at / (np.float32(1.0) + at), np.float32(1.0)).astype(np.float32)
        col = np.where(t < F32_MAX, term, miss).astype(np.float32)
    return _rgba(col)


def shade_counts(counts, n_samples):
    c = np.asarray(counts, dtype=np.uint8)
    col = np.where(c == AO_NO_SURFACE, np.float32(0.0), c.astype(np.float32) / np.float32(n_samples)).astype(np.float32)
    return _rgba(col)


def shade_term(term):
    u, s = term["unoccluded"].astype(np.float32), term["samples"].astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        col = np.where(term["samples"] == 0, np.float32(0.0), u / s).astype(np.float32)
    return _rgba(col)
