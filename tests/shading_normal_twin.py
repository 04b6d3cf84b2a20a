"""Twins of the vertex-normal feature (include/trx.h, "vertex normals and the shading normal"); none of them calls the library.

`shading_normals`        THE SHADING NORMAL in numpy float32: the header's rule N1..N5 operation for operation, so its bits are
                         k_shading_normal's.  Beside the records it returns why every record fell back.
`vertex_normals`         trx_compute_vertex_normals in float64 (Python floats for the sums: the same IEEE additions in the same
                         order).
`read_obj_normals`       a small OBJ reader for `v`, `vn` and `f` with v, v/vt, v//vn and v/vt/vn corners.
`hostile_normals`        the hostile table of the tests: its kinds cycled over the triangles.
`light_flip`             the light term's sg for a normal and a direction (tests/light_twin.py, flip)."""
import math

import numpy as np

from hit_attr_twin import ATTR_DTYPE

f32 = np.float32
F32_MAX = f32(3.4028234663852886e38)

# why a record came out as it did
ADOPTED, OUT_OF_RANGE, Q_NOT_POSITIVE, Q_NOT_FINITE, C_NAN, FLIP_DIFFERS = 0, 1, 2, 3, 4, 5
FALLBACKS = {OUT_OF_RANGE: "out of range", Q_NOT_POSITIVE: "q > 0 fails", Q_NOT_FINITE: "q < +inf fails", C_NAN: "c is NaN",
             FLIP_DIFFERS: "the light term's flip differs"}


def _dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def light_flip(n, d):
    """copysignf(1, (n.x*-d.x + n.y*-d.y) + n.z*-d.z): the sg of trx_light_term_dev."""
    n, d = np.asarray(n, dtype=np.float32), np.asarray(d, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.copysign(f32(1.0), (n[:, 0] * -d[:, 0] + n[:, 1] * -d[:, 1]) + n[:, 2] * -d[:, 2])


def shading_normals(normals, attr, dirs, prims, inst=None, w2o=None):
    """(out records, cause per record): the rule for attribute records `attr` (ATTR_DTYPE), world ray directions `dirs`
    ([n, 3] f32, as given), hit records' `prims` (u32) and - on a scene with instance transforms, w2o = its [n_instances, 12]
    world-to-object rows - the instance ids `inst`.  normals: [n_tris, 9] f32, the table as set."""
    normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 9)
    attr = np.ascontiguousarray(attr, dtype=ATTR_DTYPE)
    prims = np.asarray(prims, dtype=np.uint32)
    d = np.asarray(dirs, dtype=np.float32).reshape(-1, 3)
    n = prims.size
    out = attr.copy()
    cause = np.full(n, OUT_OF_RANGE, dtype=np.uint8)
    ok = prims.astype(np.uint64) < np.uint64(normals.shape[0])
    if w2o is not None:
        inst = np.asarray(inst, dtype=np.uint32)
        ok &= inst.astype(np.uint64) < np.uint64(w2o.shape[0])
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return out, cause
    t = normals[prims[idx]]
    A = attr[idx]
    u, v = A["u"], A["v"]
    g = A["normal"]
    dx, dy, dz = d[idx, 0], d[idx, 1], d[idx, 2]
    one = f32(1.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        w = (one - u) - v
        m = [(w * t[:, c] + u * t[:, 3 + c]) + v * t[:, 6 + c] for c in range(3)]
        if w2o is not None:
            rows = w2o[inst[idx]]
            r = [rows[:, 4 * i:4 * i + 4] for i in range(3)]
            m = [(r[0][:, i] * m[0] + r[1][:, i] * m[1]) + r[2][:, i] * m[2] for i in range(3)]
        q = _dot3(m[0], m[1], m[2], m[0], m[1], m[2])
        inv = one / np.sqrt(q)
        s = [m[0] * inv, m[1] * inv, m[2] * inv]
        c = _dot3(s[0], s[1], s[2], g[:, 0], g[:, 1], g[:, 2])
        sg = np.copysign(one, c)
        s = [s[0] * sg, s[1] * sg, s[2] * sg]
        a = (g[:, 0] * -dx + g[:, 1] * -dy) + g[:, 2] * -dz
        b = (s[0] * -dx + s[1] * -dy) + s[2] * -dz
        same_flip = ((a > 0) & (b > 0)) | ((a < 0) & (b < 0))
        why = np.where(~(q > 0), Q_NOT_POSITIVE, np.where(~(q < np.inf), Q_NOT_FINITE, np.where(~(c == c), C_NAN,
                       np.where(~same_flip, FLIP_DIFFERS, ADOPTED)))).astype(np.uint8)
    cause[idx] = why
    got = idx[why == ADOPTED]
    out["normal"][got] = np.stack(s, axis=1).astype(np.float32)[why == ADOPTED]
    out["_pad"][got] = 0
    return out, cause


def face_vectors(verts):
    """([n, 3] f64 face vectors cross(v1 - v0, v2 - v0), [n, 3] unit face vectors, [n] bool: the face contributes)."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        f = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        ln = np.sqrt(_dot3(f[:, 0], f[:, 1], f[:, 2], f[:, 0], f[:, 1], f[:, 2]))
        valid = np.isfinite(ln) & (ln > 0)
        unit = np.where(valid[:, None], f / ln[:, None], 0.0)
    return f, unit, valid


def vertex_normals(verts, crease_cos):
    """[n, 9] f32: trx_compute_vertex_normals' rule.  Welding by the position's bits with -0.0 taken as +0.0."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
    n = verts.shape[0]
    f, unit, valid = face_vectors(verts)
    bits = verts.view(np.uint32).reshape(n, 3, 3).copy()
    bits[bits == 0x80000000] = 0
    at = {}
    for t in range(n):
        if valid[t]:
            for k in range(3):
                at.setdefault(bits[t, k].tobytes(), []).append(t)      # (ascending: t runs upward)
    out = np.zeros((n, 9), dtype=np.float32)
    fl, ul = f.tolist(), unit.tolist()
    cc = float(crease_cos)
    for t in range(n):
        if not valid[t]:
            continue
        a = ul[t]
        for k in range(3):
            sx = sy = sz = 0.0
            for t2 in at[bits[t, k].tobytes()]:
                b = ul[t2]
                if t2 != t and not ((b[0] * a[0] + b[1] * a[1]) + b[2] * a[2] >= cc):
                    continue
                sx += fl[t2][0]
                sy += fl[t2][1]
                sz += fl[t2][2]
            q = (sx * sx + sy * sy) + sz * sz
            ln = math.sqrt(q) if q == q and q != math.inf else math.inf
            if not (math.isfinite(ln) and ln > 0.0):
                continue
            out[t, 3 * k:3 * k + 3] = (np.float32(sx / ln), np.float32(sy / ln), np.float32(sz / ln))
    return out


def read_obj_normals(path):
    """(verts [n, 9] f32, normals [n, 9] f32, any): the triangles of an OBJ's faces (corners 0,1,2 and, for a quad, 0,2,3) and
    each corner's `vn` - the third index of v/vt/vn or v//vn, relative to the records read so far when negative; +0 where the
    corner names none or one out of range at that point of the file."""
    pos, nrm, verts, normals = [], [], [], []
    any_vn = False
    for line in open(path):
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "v":
            pos.append([np.float32(x) for x in tok[1:4]])
        elif tok[0] == "vn":
            nrm.append([np.float32(x) for x in tok[1:4]])
        elif tok[0] == "f":
            corners = []
            for c in tok[1:]:
                parts = c.split("/")
                vi = int(parts[0])
                vi = len(pos) + vi if vi < 0 else vi - 1
                ni = -1
                if len(parts) >= 3 and parts[2]:
                    ni = int(parts[2])
                    ni = len(nrm) + ni if ni < 0 else ni - 1
                corners.append((vi, ni))
            tris = [(0, 1, 2)] if len(corners) >= 3 else []
            if len(corners) == 4:
                tris.append((0, 2, 3))
            for tri in tris:
                if any(not 0 <= corners[k][0] < len(pos) for k in tri):
                    continue
                for k in tri:
                    vi, ni = corners[k]
                    verts.extend(pos[vi])
                    have = 0 <= ni < len(nrm)
                    any_vn = any_vn or have
                    normals.extend(nrm[ni] if have else [np.float32(0.0)] * 3)
    return (np.array(verts, dtype=np.float32).reshape(-1, 9), np.array(normals, dtype=np.float32).reshape(-1, 9), any_vn)


HOSTILE_KINDS = ("all zero", "minus the face normal", "denormal", "near FLT_MAX", "one zero and two opposite")


def hostile_normals(tri_verts):
    """[n, 9] f32: the hostile table for triangles `tri_verts` ([n, 9] f32 vertices, or hit_attr_twin.tri_records' [n, 12]
    {v0, e1, e2, ng}) - triangle i gets kind i % 5 of HOSTILE_KINDS:
      0  all zero: q == 0;
      1  exactly minus the unit face normal at all three vertices: c < 0, the copysign flip brings s back to g's side;
      2  denormal components (the unit face normal times 1e-39, or 1e-42 for every other one): q underflows to 0;
      3  components of magnitude 3e38: q overflows to +inf;
      4  vertex 0 zero, vertices 1 and 2 plus and minus the unit direction of the triangle's first edge: m = (u - v) * e lies
         in the triangle's plane, so c is a rounding residue of either sign (or m == 0 where u == v) and the light term's flip
         for s disagrees with the one for g on about half the records."""
    tv = np.ascontiguousarray(tri_verts, dtype=np.float32)
    if tv.shape[1] == 12:
        ng, edge = tv[:, 9:12].astype(np.float64), tv[:, 3:6].astype(np.float64)
    else:
        ng, edge = face_vectors(tv)[0], tv[:, 3:6].astype(np.float64) - tv[:, 0:3].astype(np.float64)
    n = tv.shape[0]

    def unit(a):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ln = np.sqrt((a * a).sum(1))
            good = np.isfinite(ln) & (ln > 0)
            return np.where(good[:, None], a / np.where(good, ln, 1.0)[:, None], np.array([0.0, 0.0, 1.0])[None, :]).astype(np.float32)

    un, ue = unit(ng), unit(edge)
    out = np.zeros((n, 9), dtype=np.float32)
    i = np.arange(n)
    kind = i % 5
    k = kind == 1
    out[k] = np.tile(-un[k], (1, 3))
    k = kind == 2
    out[k] = np.tile(un[k], (1, 3)) * np.where(i[k] % 10 == 2, f32(1e-39), f32(1e-42))[:, None]
    k = kind == 3
    out[k] = np.tile(np.where(un[k] < 0, f32(-3.0e38), f32(3.0e38)), (1, 3))
    k = kind == 4
    out[k, 3:6] = ue[k]
    out[k, 6:9] = -ue[k]
    return out
