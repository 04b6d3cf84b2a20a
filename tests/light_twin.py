"""The twin of the direct-light pass (include/trx.h, "direct light"): THE DEFINITION of the shadow rays, the visibility
planes, the light term and the value shade, in numpy float32 and on the oracle alone.

Rays.  `hit_attr_twin.primary_dirs` gives d and `hit_attr_twin.hit_attrs` the unit geometric normal (through the instance's
world-to-object rows on a transformed scene - the routine the attribute pass is held to); the flip, the origin, the light
point (the oracle's `orc_hash_noise` for a rect light), the direction, the reach and the facing test are the header's
statements restated one binary32 operation at a time.
Visibility.  The rays go through `OracleScene.trace_rays`; a ray is occluded when the answer's prim is not 0xFFFFFFFF.  A
masked pass walks `inst_mask_twin.oracle_twin` of the visibility vector (masks & ray_mask) != 0.
Term and shade.  The header's order of operations in float32; `image_twin` supplies the code table shade.
Caller records (include/trx.h).  The rays and the planes take the scene's rule: a surface record has t < FLT_MAX and
prim < n_tris (`surface(primary, n_tris)`), an instance id >= n_instances selects no row.  The light term reads no scene
table and keeps prim != 0xFFFFFFFF (`surface(primary)`)."""
import numpy as np

from ao_visibility_twin import THREADS, surface_records
from hit_attr_twin import hit_attrs, primary_dirs, primary_origins
from image_twin import _rgba

INVALID = 0xFFFFFFFF
NO_SURFACE = 0xFF
F32_MAX = np.float32(3.4028234663852886e38)
DIRECTIONAL, POINT, RECT = 0, 1, 2
MAX_LIGHTS = 8
f32 = np.float32


class Light:
    """A trx_light: kind, position, edge1, edge2 (float32 triples) and a float32 intensity."""

    def __init__(self, kind, position, edge1=(0, 0, 0), edge2=(0, 0, 0), intensity=1.0):
        self.kind = int(kind)
        self.position = np.array(position, dtype=np.float32)
        self.edge1 = np.array(edge1, dtype=np.float32)
        self.edge2 = np.array(edge2, dtype=np.float32)
        self.intensity = np.float32(intensity)

    def key(self):
        return (self.kind, self.position.tobytes(), self.edge1.tobytes(), self.edge2.tobytes(), self.intensity.tobytes())

    def samples(self, n_samples):
        return n_samples if self.kind == RECT else 1

    def product(self, T):
        """The same light as the product's ctypes record."""
        return T.light(self.kind, self.position.tolist(), self.edge1.tolist(), self.edge2.tolist(), float(self.intensity))


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def surface(primary, n_tris=None):
    """n_tris None: the rule of the passes that read no scene table; else the caller-record rule of those that do."""
    if n_tris is None:
        return (primary["t"] < F32_MAX) & (primary["prim"] != INVALID)
    return surface_records(primary, n_tris)


def hash_noise(orc, px, py, seed):
    """orc_hash_noise for arrays of pixels and one seed."""
    fn = orc.load().orc_hash_noise
    seed = int(seed) & 0xFFFFFFFF
    return np.array([fn(int(x), int(y), seed) for x, y in zip(px, py)], dtype=np.float32)


def directional(light):
    """l of a directional light."""
    p = light.position
    return p * (f32(1.0) / np.sqrt(_dot3(p, p)))


def frame_geometry(view, w, h, primary, primary_inst, recs, w2o=None):
    """(indices of the surface pixels, their px, py, d [n, 3], flipped unit normal n [n, 3], t [n]) for whole-image records in
    pixel order.  recs: hit_attr_twin.tri_records; w2o: [n_instances, 12] rows of a transformed scene (else None)."""
    idx = np.flatnonzero(surface(primary, recs.shape[0]))
    px, py = idx % w, idx // w
    d = primary_dirs(view, w, h, px, py)
    inst = None if w2o is None else np.asarray(primary_inst, dtype=np.uint32)[idx]
    n = hit_attrs(recs, primary_origins(view, idx.size), d, primary["prim"][idx], inst=inst, w2o=w2o)["normal"]
    if w2o is not None:
        # an id outside the table selects no row: the unit object-space normal (the attribute pass's own rule zeroes it)
        no_row = np.flatnonzero(inst >= w2o.shape[0])
        n[no_row] = hit_attrs(recs, primary_origins(view, no_row.size), d[no_row], primary["prim"][idx][no_row])["normal"]
    return idx, px, py, d, flip(n, d), np.asarray(primary["t"], dtype=np.float32)[idx]


def flip(n, d):
    """n * sg, sg = copysignf(1, (n.x*-d.x + n.y*-d.y) + n.z*-d.z)."""
    nd = (n[:, 0] * -d[:, 0] + n[:, 1] * -d[:, 1]) + n[:, 2] * -d[:, 2]
    return (n * np.copysign(f32(1.0), nd)[:, None]).astype(np.float32)


def light_rays(orc, view, w, h, geometry, light, light_index, frame0, sample, shadow_eps):
    """([w * h] rays in pixel order, cast mask): the shadow ray of every pixel toward `light` for one sample; the inert ray
    where there is no surface or the sample does not face the light.  geometry: frame_geometry's tuple."""
    idx, px, py, d, n, t = geometry
    rays = np.zeros(w * h, dtype=orc.RAY_DTYPE)
    rays["tmax"] = f32(-1.0)
    cast = np.zeros(w * h, dtype=bool)
    if idx.size == 0:
        return rays, cast
    eye = np.array(view.eye, dtype=np.float32)
    eps = f32(shadow_eps)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        o = ((eye[None, :] + d * t[:, None]) - d * eps).astype(np.float32)
        if light.kind == DIRECTIONAL:
            l = np.tile(directional(light), (idx.size, 1)).astype(np.float32)
            tmax = np.full(idx.size, F32_MAX, dtype=np.float32)
        else:
            L = np.tile(light.position, (idx.size, 1)).astype(np.float32)
            if light.kind == RECT:
                seed = (int(frame0) + int(light_index) * 64 + int(sample)) & 0xFFFFFFFF
                u1 = hash_noise(orc, px, py, seed)
                u2 = hash_noise(orc, px, py, seed + 1024)
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


def visibility_planes(orc, osc, view, w, h, geometry, primary, lights, frame0, n_samples, shadow_eps, sem):
    """[n_lights, w * h] uint8 in pixel order: per light the samples cast and not occluded, NO_SURFACE without a surface.
    osc: the oracle scene the shadow rays walk (a masked pass: inst_mask_twin.oracle_twin of the visible instances)."""
    surf = np.zeros(w * h, dtype=bool)
    surf[geometry[0]] = True                                        # (frame_geometry's surface pixels: the scene's rule)
    planes = np.full((len(lights), w * h), NO_SURFACE, dtype=np.uint8)
    for k, light in enumerate(lights):
        planes[k][surf] = 0
        for f in range(light.samples(n_samples)):
            rays, cast = light_rays(orc, view, w, h, geometry, light, k, frame0, f, shadow_eps)
            hits, _ = osc.trace_rays(rays, sem=sem, threads=THREADS)
            assert (hits["prim"][~cast] == INVALID).all(), "an inert ray committed a hit"
            planes[k] += (cast & (hits["prim"] == INVALID)).astype(np.uint8)
    return planes


def light_term(view, w, h, primary, normals, planes, lights, n_samples, ambient, term=None):
    """[w * h] float32: trx_light_term_dev for whole-image records in pixel order.  normals: [w * h, 3] trx_hit_attr.normal;
    planes: [n_lights, w * h] uint8; term: image_twin.TERM_DTYPE records or None."""
    out = np.zeros(w * h, dtype=np.float32)
    idx = np.flatnonzero(surface(primary))
    if idx.size == 0:
        return out
    px, py = idx % w, idx // w
    d = primary_dirs(view, w, h, px, py)
    n = flip(np.asarray(normals, dtype=np.float32)[idx], d)
    t = np.asarray(primary["t"], dtype=np.float32)[idx]
    eye = np.array(view.eye, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        P = (eye[None, :] + d * t[:, None]).astype(np.float32)
        if term is None:
            a = np.ones(idx.size, dtype=np.float32)
        else:
            u, s = term["unoccluded"][idx].astype(np.float32), term["samples"][idx].astype(np.float32)
            a = np.where(term["samples"][idx] == 0, f32(0.0), u / s).astype(np.float32)
        E = (f32(ambient) * a).astype(np.float32)
        for k, light in enumerate(lights):
            if light.kind == DIRECTIONAL:
                g = _dot3(n, directional(light)[None, :])
            else:
                C = light.position
                if light.kind == RECT:
                    C = (C + f32(0.5) * light.edge1) + f32(0.5) * light.edge2
                v = (C[None, :] - P).astype(np.float32)
                q = _dot3(v, v)
                inv = f32(1.0) / np.sqrt(q)
                g = _dot3(n, (v * inv[:, None]).astype(np.float32)) / q
            cnt = planes[k][idx]
            cnt = np.where(cnt == NO_SURFACE, 0, cnt).astype(np.float32)
            vis = cnt / f32(light.samples(n_samples))
            E = np.where(g > f32(0.0), E + (light.intensity * g) * vis, E).astype(np.float32)
    out[idx] = E
    return out


def shade_value(values):
    """trx_shade_value_dev: [n, 4] uint8."""
    return _rgba(np.asarray(values, dtype=np.float32))


def shares(plane, cast0):
    """(back-facing, lit, shadowed) as shares of the surface pixels of a one-sample plane whose cast mask is cast0."""
    surf = plane != NO_SURFACE
    n = max(int(surf.sum()), 1)
    return ((surf & ~cast0).sum() / n, (surf & cast0 & (plane == 1)).sum() / n, (surf & cast0 & (plane == 0)).sum() / n)


# ---- the cases the test files share -------------------------------------------------------------------------------------
POINT_CASES = {"cornell_64": (0.0, 1.8, 0.0), "soup_52x44": (0.03, 0.97, 0.01), "cornell_tlas_48": (0.0, 1.8, 0.0)}
RECT_CASE = Light(RECT, (-0.4, 1.9, -0.4), (0.8, 0.0, 0.0), (0.0, 0.0, 0.8))     # on cornell_tlas_48, 8 samples
MASK_HIDES = 4                                                                   # the TLAS primitive the mask case hides


def golden_flat(g):
    """What inst_mask_twin.twin_buffers reads of a flat scene, from a golden fixture."""
    import types
    return types.SimpleNamespace(nodes=g["nodes"], tri_verts=g["tri_verts"], instance_offsets=g["instance_offsets"],
                                 tlas_start=int(g["tlas_start"]))
