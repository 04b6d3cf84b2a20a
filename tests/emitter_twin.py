"""The twin of the emitter passes (include/trx.h, "emitters"): THE DEFINITION of the emitter table (pairs, records, P, kinv,
c), of selection, of rules E1-E5 and of rule 5e, in numpy - float32 one operation at a time for the device's arithmetic,
float64 for the host's table - and on the oracle alone.  It calls nothing of the library under test: surface pixels, normals
and origins come from tests/light_twin.py, bounce rays and s_f from tests/indirect_twin.py, occlusion from the oracle's
trace_rays; the noise is tests/noise_domain.py's uhash_np (tests/test_noise_domain.py holds it to orc_uhash, tests/test_emitters.py
holds `hash_noise` here to orc_hash_noise).

Every function takes whole-image records in pixel order (y * w + x); planes are rows of a [3, n] array."""
import numpy as np

import indirect_twin as IT
import light_twin as LT
from noise_domain import uhash_np

f32 = np.float32
INVALID = 0xFFFFFFFF
MAX_EMITTERS = 1 << 20
SEED_PRIMARY, SEED_BOUNCE = 2048, 8192


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ---- the table ------------------------------------------------------------------------------------------------------------------

def emissive(materials, tri_material):
    """[n_tris] bool: the triangle's material has an emission component > 0.  materials: [n, 6] (albedo rgb, emission rgb)."""
    mat = np.asarray(materials, dtype=np.float32).reshape(-1, 6)
    return (mat[:, 3:] > 0).any(1)[np.asarray(tri_material, dtype=np.uint16)]


def instance_prims(nodes, instance_offsets, tlas_start, entry=None):
    """Per TLAS primitive the triangles reachable from its entry node, ascending: the 80-byte nodes ([n, 20] uint32) walked -
    word 4 child_base_idx (relative to the BLAS's first node), word 5 primitive_base_idx, words 6-7 the eight child_meta bytes
    (0: empty; bits 3-4 both set: an inner child, the r-th of them at child_base_idx + r; else a leaf of 1, 2 or 3 triangles
    (top three bits 001, 011, 111) from primitive_base_idx + (meta & 31))."""
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 20)
    meta = nodes[:, 6:8].copy().view(np.uint8).reshape(-1, 8)
    out, seen = [], {}
    for k, seg in enumerate(np.asarray(instance_offsets, dtype=np.uint32).tolist()):
        start = seg + (0 if entry is None else int(entry[k]))
        if start not in seen:
            prims, stack = [], [start]
            while stack:
                i = stack.pop()
                assert i < tlas_start
                rank = 0
                for m in meta[i].tolist():
                    if m == 0:
                        continue
                    if m & 0x18 == 0x18:
                        stack.append(seg + int(nodes[i, 4]) + rank)
                        rank += 1
                    else:
                        first = int(nodes[i, 5]) + (m & 0x1F)
                        prims += range(first, first + {1: 1, 3: 2, 7: 3}[m >> 5])
            seen[start] = np.unique(np.array(prims, dtype=np.uint32))
        out.append(seen[start])
    return out


def pairs(emit, inst_prims=None):
    """[n, 2] uint32 (instance, prim): single level (inst_prims None) the emissive triangles in prim order under instance
    0xFFFFFFFF; two levels every instance, ascending, crossed with the emissive triangles of its list, ascending."""
    emit = np.asarray(emit, dtype=bool)
    if inst_prims is None:
        prim = np.flatnonzero(emit).astype(np.uint32)
        return np.stack([np.full(prim.size, INVALID, dtype=np.uint32), prim], axis=1)
    rows = [np.stack([np.full(int(emit[p].sum()), k, dtype=np.uint32), np.sort(p[emit[p]]).astype(np.uint32)], axis=1) for k, p in enumerate(inst_prims)]
    return np.concatenate(rows).astype(np.uint32) if rows else np.zeros((0, 2), dtype=np.uint32)


def records(recs, pair, tri_material, o2w=None):
    """[n, 16] float32 with kinv = +0: V0 | E1 = -e1 | E2 = e2 | NG = cross(E1, E2), the indices in the w lanes as bit patterns.
    recs: hit_attr_twin.tri_records ([n_tris, 12]: v0, e1 = v0 - v1, e2 = v2 - v0, ng); o2w: [n_instances, 16] column-major
    object-to-world matrices of a scene with instance transforms (None: none).  A point goes through
    ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r], an edge through the same without the last addition."""
    pair = np.asarray(pair, dtype=np.uint32).reshape(-1, 2)
    r = np.asarray(recs, dtype=np.float32)[pair[:, 1]]
    V0, E1, E2 = r[:, 0:3].copy(), -r[:, 3:6], r[:, 6:9].copy()
    if o2w is not None:
        m = np.asarray(o2w, dtype=np.float32).reshape(-1, 16)[pair[:, 0]]

        def lin(v):
            return np.stack([((m[:, k] * v[:, 0]).astype(np.float32) + (m[:, 4 + k] * v[:, 1]).astype(np.float32)).astype(np.float32)
                             + (m[:, 8 + k] * v[:, 2]).astype(np.float32) for k in range(3)], axis=1).astype(np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            V0 = (lin(V0) + m[:, 12:15]).astype(np.float32)
            E1, E2 = lin(E1), lin(E2)
    with np.errstate(over="ignore", invalid="ignore"):
        NG = np.stack([(E1[:, 1] * E2[:, 2]).astype(np.float32) - (E1[:, 2] * E2[:, 1]).astype(np.float32),
                       (E1[:, 2] * E2[:, 0]).astype(np.float32) - (E1[:, 0] * E2[:, 2]).astype(np.float32),
                       (E1[:, 0] * E2[:, 1]).astype(np.float32) - (E1[:, 1] * E2[:, 0]).astype(np.float32)], axis=1).astype(np.float32)
    out = np.zeros((pair.shape[0], 16), dtype=np.float32)
    bits = out.view(np.uint32)
    out[:, 0:3], out[:, 4:7], out[:, 8:11], out[:, 12:15] = V0, E1, E2, NG
    bits[:, 7] = np.asarray(tri_material, dtype=np.uint16)[pair[:, 1]].astype(np.uint32)
    bits[:, 11], bits[:, 15] = pair[:, 1], pair[:, 0]
    return out


def selection(rec, materials):
    """(P [n] float32, kinv [n] float32, c [n - 1] float32) from the records, in float64 and in index order."""
    mat = np.asarray(materials, dtype=np.float32).reshape(-1, 6)
    rec = np.asarray(rec, dtype=np.float32).reshape(-1, 16)
    n = rec.shape[0]
    Le = mat[rec.view(np.uint32)[:, 7], 3:].astype(np.float64)
    NG = rec[:, 12:15].astype(np.float64)
    w = [float(np.sqrt(NG[j, 0] * NG[j, 0] + NG[j, 1] * NG[j, 1] + NG[j, 2] * NG[j, 2]) * (Le[j, 0] + Le[j, 1] + Le[j, 2])) for j in range(n)]
    W = 0.0
    for x in w:
        W += x
    p = [1.0 / n if W == 0.0 else 0.5 * x / W + 0.5 / n for x in w]
    P = np.array(p, dtype=np.float64).astype(np.float32)
    kinv = (1.0 / (3.14159265358979323846 * P.astype(np.float64))).astype(np.float32)
    run, c = 0.0, []
    for x in p[:-1]:
        run += x
        c.append(run)
    return P, kinv, np.array(c, dtype=np.float64).astype(np.float32)


def table(recs, pair, materials, tri_material, o2w=None):
    """(records [n, 16] with kinv filled in, c [n - 1]) - what trx_scene_get_emitters hands out."""
    rec = records(recs, pair, tri_material, o2w)
    _, kinv, c = selection(rec, materials)
    rec[:, 3] = kinv
    return rec, c


def select(c, u0):
    """j = the number of i with c[i] <= u0 - counted, not searched."""
    c, u0 = np.asarray(c, dtype=np.float32), np.asarray(u0, dtype=np.float32).reshape(-1)
    out = np.zeros(u0.size, dtype=np.uint32)
    with np.errstate(invalid="ignore"):
        for at in range(0, u0.size, 4096):
            out[at:at + 4096] = (c[None, :] <= u0[at:at + 4096, None]).sum(1)
    return out


# ---- rules E2 - E4 ----------------------------------------------------------------------------------------------------------------

def hash_noise(px, py, seed):
    """hash_noise(px, py, seed) over pixel arrays: (float)uhash(px, (py << 11) + seed) * 2^-32."""
    px, py = np.asarray(px).astype(np.uint32), np.asarray(py).astype(np.uint32)
    h = uhash_np(px, (py << np.uint32(11)) + np.uint32(int(seed) & 0xFFFFFFFF))
    return (h.astype(np.float32) * f32(1.0 / 4294967296.0)).astype(np.float32)


def sample(rec, c, px, py, se, emitter_eps, o, n, u=None):
    """Rules E2-E4 at the points o [k, 3] with flipped normals n [k, 3] for pixels (px, py) and seed se: a dictionary of
    j [k], y, l [k, 3], tmax, wgeo [k] float32 and cast [k] bool.  u: (u0, u1, u2) in the hash's place."""
    u0, u1, u2 = u if u is not None else (hash_noise(px, py, se), hash_noise(px, py, se + 1024), hash_noise(px, py, se + 4096))
    j = select(c, u0)
    r = np.asarray(rec, dtype=np.float32).reshape(-1, 16)[j]
    V0, E1, E2, NG, kinv = r[:, 0:3], r[:, 4:7], r[:, 8:11], r[:, 12:15], r[:, 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        su = np.sqrt(u1).astype(np.float32)
        b1 = (su * (f32(1.0) - u2).astype(np.float32)).astype(np.float32)
        b2 = (su * u2).astype(np.float32)
        y = ((V0 + (b1[:, None] * E1).astype(np.float32)).astype(np.float32) + (b2[:, None] * E2).astype(np.float32)).astype(np.float32)
        v = (y - o).astype(np.float32)
        q = _dot3(v, v).astype(np.float32)
        dist = np.sqrt(q).astype(np.float32)
        inv = (f32(1.0) / dist).astype(np.float32)
        l = (v * inv[:, None]).astype(np.float32)
        tmax = (dist - (dist * f32(emitter_eps)).astype(np.float32)).astype(np.float32)
        cs = _dot3(n, l).astype(np.float32)
        a = (f32(0.5) * np.abs(_dot3(NG, l).astype(np.float32))).astype(np.float32)
        wgeo = ((((cs * a).astype(np.float32)) / q).astype(np.float32) * kinv).astype(np.float32)
        cast = (cs > f32(0.0)) & (wgeo > f32(0.0)) & (wgeo < f32(np.inf))
    return {"j": j, "y": y, "l": l, "tmax": tmax, "wgeo": wgeo, "cast": cast, "u": (u0, u1, u2)}


def _inert(orc, n_rec):
    rays = np.zeros(n_rec, dtype=orc.RAY_DTYPE)
    rays["tmax"] = f32(-1.0)
    return rays, np.zeros(n_rec, dtype=bool), np.zeros(n_rec, dtype=np.float32), np.zeros(n_rec, dtype=np.uint32)


def _rays_of(orc, n_rec, at, o, s):
    """([n_rec] rays, cast, wgeo, j): the sample's rays at the records `at`, the inert ray everywhere else."""
    rays, cast, wgeo, j = _inert(orc, n_rec)
    c = s["cast"]
    rays["origin"][at[c]] = o[c]
    rays["direction"][at[c]] = s["l"][c]
    rays["tmax"][at[c]] = s["tmax"][c]
    cast[at[c]], wgeo[at[c]], j[at[c]] = True, s["wgeo"][c], s["j"][c]
    return rays, cast, wgeo, j


def primary_rays(orc, view, w, h, geometry, rec, c, frame0, f, shadow_eps, emitter_eps):
    """E1-E4 for sample f: ([w * h] rays in pixel order, cast, wgeo, j).  geometry: light_twin.frame_geometry's tuple."""
    idx, px, py, d, n, t = geometry
    if idx.size == 0:
        return _inert(orc, w * h)
    eye = np.array(view.eye, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        o = ((eye[None, :] + d * t[:, None]).astype(np.float32) - d * f32(shadow_eps)).astype(np.float32)
    se = (int(frame0) + SEED_PRIMARY + int(f)) & 0xFFFFFFFF
    return _rays_of(orc, w * h, idx, o, sample(rec, c, px, py, se, emitter_eps, o, n))


def _emission(rec, materials, j):
    mat = np.asarray(materials, dtype=np.float32).reshape(-1, 6)
    return mat[np.asarray(rec, dtype=np.float32).reshape(-1, 16).view(np.uint32)[j, 7], 3:]


def emitter_light(orc, osc, view, w, h, geometry, primary, n_tris, rec, c, materials, frame0, n_samples, shadow_eps, emitter_eps, sem, base=None):
    """E5: [3, w * h] float32.  osc: the oracle scene the shadow rays walk (a masked pass: the twin scene of the visible
    instances); base: [3, w * h] or None."""
    occluded = IT.oracle_occluded(osc, sem)
    A = np.zeros((3, w * h), dtype=np.float32)
    for f in range(n_samples):
        rays, cast, wgeo, j = primary_rays(orc, view, w, h, geometry, rec, c, frame0, f, shadow_eps, emitter_eps)
        add = cast & ~np.asarray(occluded(0, rays), dtype=bool)
        Le = _emission(rec, materials, j)
        for ch in range(3):
            A[ch] = np.where(add, A[ch] + (wgeo * Le[:, ch]).astype(np.float32), A[ch]).astype(np.float32)
    b = np.zeros((3, w * h), dtype=np.float32) if base is None else np.asarray(base, dtype=np.float32).reshape(3, w * h)
    out = (b + (A / f32(n_samples)).astype(np.float32)).astype(np.float32)
    bits = np.where(LT.surface(primary, n_tris)[None, :], out.view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    return bits.astype(np.uint32).view(np.float32)


# ---- rule 5e ----------------------------------------------------------------------------------------------------------------------

def bounce_rays(orc, w, h, b_rays, b_hits, b_attr, rec, c, frame0, f, shadow_eps, emitter_eps):
    """E2-E4 at the bounce hits of sample f: ([w * h] rays, cast, wgeo, j); seed frame0 + 8192 + f at the record's own pixel."""
    idx, d, n, Q = IT.hit_geometry(b_rays, b_hits, b_attr)
    if idx.size == 0:
        return _inert(orc, w * h)
    with np.errstate(invalid="ignore", over="ignore"):
        o = (Q - d * f32(shadow_eps)).astype(np.float32)
    se = (int(frame0) + SEED_BOUNCE + int(f)) & 0xFFFFFFFF
    return _rays_of(orc, w * h, idx, o, sample(rec, c, idx % w, idx // w, se, emitter_eps, o, n))


def indirect_rgb_emitters(orc, osc, oview, w, h, primary, primary_inst, recs, w2o, lights, frame0, n_samples, bounce_eps, shadow_eps, emitter_eps,
                          sem, materials, tri_material, rec, c, shadow_osc=None, cache=None):
    """The emitter-mode indirect pass, dense: [3, w * h] float32.  Rules 1-4 are indirect_twin's (s_f = +0 without lights)."""
    mat = np.asarray(materials, dtype=np.float32).reshape(-1, 6)
    tri_material = np.asarray(tri_material, dtype=np.uint16)
    occluded = IT.oracle_occluded(shadow_osc or osc, sem)
    A = np.zeros((3, w * h), dtype=np.float32)
    for f in range(n_samples):
        key = (frame0 + f, float(bounce_eps), sem, hash(primary.tobytes()), hash(np.asarray(primary_inst).tobytes()))
        if cache is not None and key in cache:
            b = cache[key]
        else:
            b = IT.bounce(orc, osc, oview, w, h, primary, primary_inst, recs, w2o, frame0 + f, bounce_eps, sem)
            if cache is not None:
                cache[key] = b
        rays, hits, _, attr = b
        s = IT.sample_sum(orc, w, h, rays, hits, attr, lights, frame0, f, shadow_eps, occluded)
        e_rays, cast, wgeo, j = bounce_rays(orc, w, h, rays, hits, attr, rec, c, frame0, f, shadow_eps, emitter_eps)
        lit = cast & ~np.asarray(occluded(0, e_rays), dtype=bool)
        Le = _emission(rec, materials, j)
        idx = np.flatnonzero(IT.bounce_surface(rays, hits))
        m = mat[tri_material[hits["prim"][idx]]]
        with np.errstate(invalid="ignore", over="ignore"):
            for ch in range(3):
                X = np.where(lit, (wgeo * Le[:, ch]).astype(np.float32), f32(0.0)).astype(np.float32)
                inner = (s[idx] + X[idx]).astype(np.float32)
                A[ch, idx] = (A[ch, idx] + (m[:, ch] * inner).astype(np.float32)).astype(np.float32)
    out = (A / f32(n_samples)).astype(np.float32)
    out[:, ~LT.surface(primary, recs.shape[0])] = f32(0.0)
    return out
