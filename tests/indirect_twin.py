"""The twin of the indirect-light pass (include/trx.h, "indirect light"): THE DEFINITION of the bounce rays, the secondary
shadow rays, the weights and the term, in numpy float32 and on the oracle alone.

Rule 1: the bounce rays are `ao_visibility_twin.ao_rays` under seed frame0 + f with the bounce offset and no radius.
Rule 2: they go through the oracle's closest-hit walk (`OracleScene.trace_rays_inst`: trace_rays with the instance of every
hit, which a transformed scene's normals need); `hit_attr_twin.hit_attrs` gives every hit its attribute record.
Rule 3: `light_twin`'s statements (light point, direction, reach, facing test, `orc_hash_noise` for a rect light) with the
bounce hit in the primary hit's place, one binary32 operation at a time.
Rule 4: the shadow rays go through `OracleScene.trace_rays` (a masked pass: through `inst_mask_twin.oracle_twin` of the
visible instances); occluded = the answer's prim is not 0xFFFFFFFF.  g is the light term's, at the bounce hit.
Rule 5: the sums in float32, samples ascending, lights ascending inside a sample.

Every function takes whole-image records in pixel order (y * w + x)."""
import numpy as np

import light_twin as LT
from ao_visibility_twin import THREADS, ao_rays
from hit_attr_twin import hit_attrs

INVALID = 0xFFFFFFFF
F32_MAX = LT.F32_MAX
f32 = np.float32
INF = float("inf")


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def bounce_surface(b_rays, b_hits):
    """Rule 2: the bounce has a surface iff its ray is not inert, t < FLT_MAX and prim != 0xFFFFFFFF."""
    return ~(b_rays["tmax"] < f32(0.0)) & (b_hits["t"] < F32_MAX) & (b_hits["prim"] != INVALID)


def bounce(orc, osc, oview, w, h, primary, primary_inst, recs, w2o, frame, bounce_eps, sem):
    """Rules 1 and 2 for one seed: (rays, hits, instance ids, attribute records) of every pixel."""
    rays, _ = ao_rays(orc, osc, oview, w, h, primary, primary_inst, frame, bounce_eps, INF)
    hits, inst, _ = osc.trace_rays_inst(rays, sem=sem, threads=THREADS)
    assert (hits["prim"][rays["tmax"] < 0] == INVALID).all(), "an inert ray committed a hit"
    attr = hit_attrs(recs, rays["origin"], rays["direction"], hits["prim"], inst=None if w2o is None else inst, w2o=w2o)
    return rays, hits, inst, attr


def hit_geometry(b_rays, b_hits, b_attr):
    """(indices of the bounces with a surface, d, flipped n, Q) - rule 3's d, n and Q."""
    idx = np.flatnonzero(bounce_surface(b_rays, b_hits))
    d = np.asarray(b_rays["direction"], dtype=np.float32)[idx]
    n = LT.flip(np.asarray(b_attr["normal"], dtype=np.float32)[idx], d)
    t = np.asarray(b_hits["t"], dtype=np.float32)[idx]
    with np.errstate(over="ignore", invalid="ignore"):
        Q = (np.asarray(b_rays["origin"], dtype=np.float32)[idx] + d * t[:, None]).astype(np.float32)
    return idx, d, n, Q


def secondary_rays(orc, w, h, b_rays, b_hits, b_attr, light, light_index, frame0, sample, shadow_eps):
    """Rule 3: ([w * h] rays, cast mask) - the shadow ray from every bounce hit toward `light`; the inert ray where the bounce
    has no surface or the hit does not face the light."""
    n_rec = w * h
    rays = np.zeros(n_rec, dtype=orc.RAY_DTYPE)
    rays["tmax"] = f32(-1.0)
    cast = np.zeros(n_rec, dtype=bool)
    idx, d, n, Q = hit_geometry(b_rays, b_hits, b_attr)
    if idx.size == 0:
        return rays, cast
    eps = f32(shadow_eps)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        o = (Q - d * eps).astype(np.float32)
        if light.kind == LT.DIRECTIONAL:
            l = np.tile(LT.directional(light), (idx.size, 1)).astype(np.float32)
            tmax = np.full(idx.size, F32_MAX, dtype=np.float32)
        else:
            L = np.tile(light.position, (idx.size, 1)).astype(np.float32)
            if light.kind == LT.RECT:
                seed = (int(frame0) + int(light_index) * 64 + int(sample)) & 0xFFFFFFFF
                u1 = LT.hash_noise(orc, idx % w, idx // w, seed)
                u2 = LT.hash_noise(orc, idx % w, idx // w, seed + 1024)
                L = ((L + u1[:, None] * light.edge1[None, :]) + u2[:, None] * light.edge2[None, :]).astype(np.float32)
            v = (L - o).astype(np.float32)
            dist = np.sqrt(_dot3(v, v))
            inv = f32(1.0) / dist
            l = (v * inv[:, None]).astype(np.float32)
            tmax = np.fmin(dist, F32_MAX).astype(np.float32)
        facing = _dot3(n, l) > f32(0.0)
    at = idx[facing]
    rays["origin"][at] = o[facing]
    rays["direction"][at] = l[facing]
    rays["tmax"][at] = tmax[facing]
    rays["tmin"][at] = f32(0.0)
    cast[at] = True
    return rays, cast


def light_weight(b_rays, b_hits, b_attr, light):
    """Rule 4's g of every record ([n] float32; 0 where the bounce has no surface)."""
    g = np.zeros(b_rays.shape[0], dtype=np.float32)
    idx, d, n, Q = hit_geometry(b_rays, b_hits, b_attr)
    if idx.size == 0:
        return g
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if light.kind == LT.DIRECTIONAL:
            g[idx] = _dot3(n, LT.directional(light)[None, :])
        else:
            C = light.position
            if light.kind == LT.RECT:
                C = (C + f32(0.5) * light.edge1) + f32(0.5) * light.edge2
            v = (C[None, :] - Q).astype(np.float32)
            q = _dot3(v, v)
            inv = f32(1.0) / np.sqrt(q)
            g[idx] = _dot3(n, (v * inv[:, None]).astype(np.float32)) / q
    return g


def sample_sum(orc, w, h, b_rays, b_hits, b_attr, lights, frame0, sample, shadow_eps, occluded):
    """Rule 4: s_f of every record.  occluded(k, rays) -> [n] bool: the any-hit answer for light k's shadow rays."""
    s = np.zeros(w * h, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, light in enumerate(lights):
            rays, cast = secondary_rays(orc, w, h, b_rays, b_hits, b_attr, light, k, frame0, sample, shadow_eps)
            occ = np.asarray(occluded(k, rays), dtype=bool)
            g = light_weight(b_rays, b_hits, b_attr, light)
            s = np.where(cast & ~occ & (g > f32(0.0)), s + light.intensity * g, s).astype(np.float32)
    return s


def term(sums, primary, bounce_albedo, base=None, n_tris=None):
    """Rule 5: [w * h] float32 from the samples' sums [n_samples, w * h] (ascending).  n_tris: the scene's triangle count -
    a caller's record with prim >= n_tris is no surface pixel (LT.surface); None: every prim but 0xFFFFFFFF is one."""
    n_samples = len(sums)
    A = np.zeros(primary.shape[0], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in sums:
            A = (A + s).astype(np.float32)
        b = np.zeros(primary.shape[0], dtype=np.float32) if base is None else np.asarray(base, dtype=np.float32)
        out = (b + (f32(bounce_albedo) * A) / f32(n_samples)).astype(np.float32)
    bits = np.where(LT.surface(primary, n_tris), out.view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    return bits.astype(np.uint32).view(np.float32)                 # (a pixel without a surface: its base's bits copied)


def oracle_occluded(osc, sem):
    """The `occluded` of sample_sum on an oracle scene (a masked pass: the twin scene of the visible instances)."""
    def occluded(k, rays):
        hits, _ = osc.trace_rays(rays, sem=sem, threads=THREADS)
        assert (hits["prim"][rays["tmax"] < 0] == INVALID).all(), "an inert ray committed a hit"
        return hits["prim"] != INVALID
    return occluded


def indirect(orc, osc, oview, w, h, primary, primary_inst, recs, w2o, lights, frame0, n_samples, bounce_eps, shadow_eps, bounce_albedo,
             sem, base=None, shadow_osc=None, cache=None, stats=None):
    """The pass: [w * h] float32.  shadow_osc: the scene the shadow rays walk (default osc; the bounce rays always walk osc: they
    are unmasked).  cache: a dictionary that keeps the bounces (rules 1, 2) per seed across calls over the same records.
    stats: a list that receives (bounce surface mask, per light (cast, occluded)) per sample."""
    sums = []
    for f in range(n_samples):
        key = (frame0 + f, float(bounce_eps), sem, hash(primary.tobytes()), hash(np.asarray(primary_inst).tobytes()))
        if cache is not None and key in cache:
            b = cache[key]
        else:
            b = bounce(orc, osc, oview, w, h, primary, primary_inst, recs, w2o, frame0 + f, bounce_eps, sem)
            if cache is not None:
                cache[key] = b
        rays, hits, _, attr = b
        occluded = oracle_occluded(shadow_osc or osc, sem)
        if stats is not None:
            seen = []

            def occluded(k, r, inner=occluded, seen=seen):
                occ = inner(k, r)
                seen.append((~(r["tmax"] < 0), occ))
                return occ
            stats.append((bounce_surface(rays, hits), seen))
        sums.append(sample_sum(orc, w, h, rays, hits, attr, lights, frame0, f, shadow_eps, occluded))
    return term(sums, primary, bounce_albedo, base, n_tris=recs.shape[0])
