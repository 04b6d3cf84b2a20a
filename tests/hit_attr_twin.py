"""numpy float32 twin of the hit-attribute definition (include/trx.h, trx_hit_attr): the same operations in the same
order as k_hit_attr (and as the committing triangle test, kernels.hip intersect_tri), so its bits are the device's."""
import numpy as np

F32_EPS = np.float32(1.1920929e-7)
ATTR_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("normal", "<f4", 3), ("_pad", "<u4")])
INVALID = 0xFFFFFFFF


def _dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def tri_records(tri_verts=None, tri_f16=None):
    """[n, 12] f32: the scene's 48-byte device records {v0, e1 = v0 - v1, e2 = v2 - v0, ng = cross(e1, e2)} as
    trx_scene_create builds them from TRX_TRI_VERTS_36 vertices or TRX_TRI_F16_24 words."""
    if tri_f16 is not None:
        raw = np.ascontiguousarray(tri_f16, dtype=np.uint32).reshape(-1, 6)
        v0 = np.ascontiguousarray(raw[:, 0:3]).view(np.float32)
        e = raw[:, 3:6]
        e1 = -((e >> 16).astype(np.uint16).view(np.float16).astype(np.float32))
        e2 = (e & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)
    else:
        v = np.ascontiguousarray(tri_verts, dtype=np.float32).reshape(-1, 9)
        v0 = v[:, 0:3]
        e1 = v[:, 0:3] - v[:, 3:6]
        e2 = v[:, 6:9] - v[:, 0:3]
    ng = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                   e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    return np.concatenate([v0, e1, e2, ng], axis=1).astype(np.float32)


def primary_dirs(view, w, h, px, py):
    """kernels.hip primary_dir for pixels (px, py), vectorised; view is a trx_view (ctypes)."""
    pinv = np.array(view.proj_inv, dtype=np.float32)
    vinv = np.array(view.view_inv, dtype=np.float32)
    eye = np.array(view.eye, dtype=np.float32)
    u = np.asarray(px).astype(np.float32) / np.float32(w)
    v = np.float32(1.0) - np.asarray(py).astype(np.float32) / np.float32(h)
    cx, cy = u * np.float32(2.0) - np.float32(1.0), v * np.float32(2.0) - np.float32(1.0)
    one = np.float32(1.0)

    def mul(m, a, b, c, d):
        return [((m[r] * a + m[4 + r] * b) + m[8 + r] * c) + m[12 + r] * d for r in range(4)]

    vx, vy, vz, vw = mul(pinv, cx, cy, one, one)
    s = vw
    vx, vy, vz, vw = vx / s, vy / s, vz / s, vw / s
    wx, wy, wz, _ = mul(vinv, vx, vy, vz, vw)
    dx, dy, dz = wx - eye[0], wy - eye[1], wz - eye[2]
    inv = np.float32(1.0) / np.sqrt(_dot3(dx, dy, dz, dx, dy, dz))
    return np.stack([dx * inv, dy * inv, dz * inv], axis=1).astype(np.float32)


def primary_pixels(w, h, shard=(0, 1), layout=0):
    """(record index, px, py) of every record trx_trace_primary*_dev writes for `shard` (trx.h, trx_shard)."""
    index, count = shard
    tx, ty = (w + 7) // 8, (h + 7) // 8
    tiles = np.arange(index, tx * ty, count, dtype=np.int64)
    k = np.arange(64, dtype=np.int64)
    tile = np.repeat(tiles, 64)
    kk = np.tile(k, tiles.size)
    px = (tile % tx) * 8 + (kk & 7)
    py = (tile // tx) * 8 + (kk >> 3)
    local = np.arange(tile.size, dtype=np.int64)
    inside = (px < w) & (py < h)
    rec = local if layout == 1 else py * w + px
    return rec[inside], px[inside], py[inside]


def primary_origins(view, n):
    return np.tile(np.array(view.eye, dtype=np.float32), (n, 1))


def hit_attrs(recs, origins, dirs, prims, inst=None, w2o=None):
    """trx_hit_attr records for hit records `prims` (u32) over rays (origins, dirs: [n, 3] f32, the world rays as
    given).  w2o: [n_instances, 12] world-to-object rows of a scene with instance transforms (None: no transforms);
    inst: the hits' instance ids."""
    prims = np.asarray(prims, dtype=np.uint32)
    n = prims.size
    out = np.zeros(n, dtype=ATTR_DTYPE)
    ok = prims < recs.shape[0]
    if w2o is not None:
        inst = np.asarray(inst, dtype=np.uint32)
        ok &= inst < w2o.shape[0]
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return out
    t = recs[prims[idx]]
    o = np.asarray(origins, dtype=np.float32)[idx]
    d = np.asarray(dirs, dtype=np.float32)[idx]
    ox, oy, oz = o[:, 0], o[:, 1], o[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    nx, ny, nz = t[:, 9], t[:, 10], t[:, 11]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if w2o is not None:
            m = w2o[inst[idx]]
            r = [m[:, 4 * i:4 * i + 4] for i in range(3)]
            ox, oy, oz = [((r[i][:, 0] * o[:, 0] + r[i][:, 1] * o[:, 1]) + r[i][:, 2] * o[:, 2]) + r[i][:, 3] for i in range(3)]
            dx, dy, dz = [(r[i][:, 0] * d[:, 0] + r[i][:, 1] * d[:, 1]) + r[i][:, 2] * d[:, 2] for i in range(3)]
        dx, dy, dz = [np.where(c == 0, F32_EPS, c).astype(np.float32) for c in (dx, dy, dz)]
        cx, cy, cz = t[:, 0] - ox, t[:, 1] - oy, t[:, 2] - oz
        rx = dy * cz - dz * cy
        ry = dz * cx - dx * cz
        rz = dx * cy - dy * cx
        det = _dot3(nx, ny, nz, dx, dy, dz)
        inv_det = np.float32(1.0) / det
        u = _dot3(rx, ry, rz, t[:, 6], t[:, 7], t[:, 8]) * inv_det
        v = _dot3(rx, ry, rz, t[:, 3], t[:, 4], t[:, 5]) * inv_det
        if w2o is not None:
            nx, ny, nz = [(r[0][:, i] * t[:, 9] + r[1][:, i] * t[:, 10]) + r[2][:, i] * t[:, 11] for i in range(3)]
        ninv = np.float32(1.0) / np.sqrt(_dot3(nx, ny, nz, nx, ny, nz))
        out["u"][idx] = u
        out["v"][idx] = v
        out["normal"][idx] = np.stack([nx * ninv, ny * ninv, nz * ninv], axis=1)
    return out


def object_rays(origins, dirs, inst=None, w2o=None):
    """The ray the committing test saw, in float64 for geometric checks: the zero-fixed world ray, or the world ray
    through the instance's rows and then fixed."""
    o = np.asarray(origins, dtype=np.float32)
    d = np.asarray(dirs, dtype=np.float32)
    if w2o is not None:
        m = w2o[np.asarray(inst, dtype=np.uint32)]
        r = [m[:, 4 * i:4 * i + 4] for i in range(3)]
        o = np.stack([((r[i][:, 0] * o[:, 0] + r[i][:, 1] * o[:, 1]) + r[i][:, 2] * o[:, 2]) + r[i][:, 3] for i in range(3)], 1)
        d = np.stack([(r[i][:, 0] * d[:, 0] + r[i][:, 1] * d[:, 1]) + r[i][:, 2] * d[:, 2] for i in range(3)], 1)
    d = np.where(d == 0, F32_EPS, d)
    return o.astype(np.float64), d.astype(np.float64)


def attr_bits(a):
    """[n, 6] u32 view of attribute records, for bit-exact comparisons."""
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 6)
