"""Power-of-two scene scaling (tests/test_scale.py, tests/test_gpu_scale.py): the construction, in numpy alone - the only
library calls are scene generation, the camera and the host builder.

Multiply a scene by 2^k about the camera's eye, with the eye at the origin, and every length the caller passes by 2^k as
well (light positions and rect edges, shadow_eps, ao_eps, ao_radius, bounce_eps, the caller's t).  That is the same
computation with every exponent shifted: as long as nothing under- or overflows, every binary32 operation rounds the same
way, and every output after the walk follows from the k = 0 output without any twin - `expect_from_base` is that table.

`recentred` makes the k = 0 base (an ordinary scene, held to the twins like any other), `scaled` its image under 2^k on a
rebuilt tree, `carry` takes hit records from one tree's numbering to another's through tri_source / instance_source, and
`scaled_params` scales what the caller passes.  SAFE, WALKED and EDGE are the exponent sets; ADVERSARIAL names the three
scalings of tests/adversarial_scenes.py that are no powers of two."""
import types

import numpy as np

import material_twin as MT
from light_twin import DIRECTIONAL, POINT, RECT, Light

f32 = np.float32
INVALID = 0xFFFFFFFF
F32_MAX = f32(3.4028234663852886e38)
HIT = np.dtype([("t", "<f4"), ("prim", "<u4")])

SAFE = (-20, -10, 10, 20, 30)                               # covariance must be exact
WALKED = (-10, 10, 20, 30)                                  # a primary walk still finds the k = 0 surface
# only "device equals twin" is required.  (+68 is there for the overflowing distance squares: at +62 the light twin's q = dot(v, v)
# stays finite on these scenes - at most 1.1e38 on the Cornell case - and is +inf at every surface pixel from +67 on.)
EDGE = (-50, -38, -35, -32, -29, -26, 33, 36, 48, 62, 68)
ADVERSARIAL = ("underflow_1e-30", "overflow_1e19", "extent_overflow_x")

# (scene, width, height): the Cornell stand-in with its materials; fourteen transformed instances of its objects; and a
# frame whose last tile column and row are partial
CASES = (("cornell", 48, 32), ("instanced", 40, 24), ("cornell", 33, 23))
N_INSTANCES = 14


def pow2(a, k):
    """a * 2^k for float32 a, computed in float64 and rounded once: exact unless the result is denormal or overflows."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.ldexp(np.asarray(a, dtype=np.float32).astype(np.float64), int(k)).astype(np.float32)


# ---- the scenes -------------------------------------------------------------------------------------------------------------

def _finish(trx, base, k, flat):
    """The scene `base` at exponent k over its rebuilt `flat`: the view (the same bits for every k: the eye is the origin),
    the materials in the tree's triangle order, the maps from source numbering to the tree's."""
    s = types.SimpleNamespace(name=base.name, k=k, w=base.w, h=base.h, flat=flat, view=base.view, mats=base.mats, tlas=base.tlas)
    s.idx = np.ascontiguousarray(base.idx_source[flat.tri_source], dtype=np.uint16)
    s.prim_of_source = np.full(base.idx_source.size, INVALID, dtype=np.uint32)
    s.prim_of_source[flat.tri_source] = np.arange(flat.tri_source.size, dtype=np.uint32)
    assert flat.tri_source.size == base.idx_source.size and (s.prim_of_source != INVALID).all(), "a pre-split build: records are not carried one to one"
    s.o2w = flat.instance_transforms if base.tlas else None
    if base.tlas:
        s.inst_of_source = np.full(N_INSTANCES, INVALID, dtype=np.uint32)
        s.inst_of_source[flat.instance_source] = np.arange(N_INSTANCES, dtype=np.uint32)
    return s


def recentred(trx, name, w, h):
    """The k = 0 base: a stand-in scene translated by minus its camera's eye, in binary32, once.  `name`: "cornell" (one
    level, the stand-in materials: the light quad's two emitters) or "instanced" (helpers.instanced_scene's fourteen
    transformed instances of the Cornell-class objects, the 360-triangle object emissive)."""
    base = types.SimpleNamespace(name=name, w=w, h=h, tlas=name == "instanced")
    if name == "cornell":
        verts, counts = trx.gen_scene("cornell", 0, 1)
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
        base.mats, base.idx_source = MT.standin("cornell", verts, counts)
        eye, look, fov = trx.scene_camera("cornell")
        eye32 = np.array(eye, dtype=np.float32)
        base.verts = (verts.reshape(-1, 3, 3) - eye32[None, None, :]).astype(np.float32).reshape(-1, 9)
        base.counts = [int(c) for c in counts]
    else:
        from helpers import instanced_scene
        flat0, _, world, _, _ = instanced_scene(trx, seed=3, n_instances=N_INSTANCES, tris_per_object=0, kind="cornell", spread=1.0)
        verts, counts = trx.gen_scene("cornell", 0, 3)
        base.verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
        base.counts = [int(c) for c in counts if c]
        n_obj = len(base.counts)
        base.inst_obj = np.array([i % n_obj for i in range(N_INSTANCES)], dtype=np.uint32)
        o2w = np.zeros((N_INSTANCES, 16), dtype=np.float32)
        o2w[flat0.instance_source] = flat0.instance_transforms           # (the caller's order)
        lo, hi = world.reshape(-1, 3).min(0), world.reshape(-1, 3).max(0)
        centre = 0.5 * (lo + hi)                                         # (the eye inside the bounds: about half the pixels a surface)
        eye, look, fov = (centre + 0.7 * (hi - centre)).tolist(), centre.tolist(), 80.0
        eye32 = np.array(eye, dtype=np.float32)
        o2w[:, 12:15] = (o2w[:, 12:15] - eye32[None, :]).astype(np.float32)
        base.o2w_source = o2w
        base.mats = np.zeros((3, 6), dtype=np.float32)
        base.mats[:, :3] = ((0.8, 0.8, 0.8), (0.8, 0.1, 0.1), (0.2, 0.2, 0.2))
        base.mats[2, 3:] = (3.0, 2.0, 1.0)
        base.idx_source = (np.arange(base.verts.shape[0]) % 2).astype(np.uint16)
        first = np.concatenate([[0], np.cumsum(base.counts)])
        walls = [i for i, c in enumerate(base.counts) if c == 360]
        assert walls, "the Cornell-class enclosure has 360 triangles"
        base.idx_source[first[walls[0]]:first[walls[0] + 1]] = 2
    base.look = (np.array(look, dtype=np.float64) - eye32.astype(np.float64)).astype(np.float32)
    base.view = trx.view_from_camera((0.0, 0.0, 0.0), base.look.tolist(), fov, w, h)
    assert not any(base.view.eye) and not any(base.view.view_inv[12:15]), "the view of a camera at the origin has no translation"
    return base


def scaled(trx, base, k):
    """`base` times 2^k (vertices - and, with instances, the translation columns; the linear parts unchanged), rebuilt."""
    verts = pow2(base.verts, k)
    if base.tlas:
        o2w = base.o2w_source.copy()
        o2w[:, 12:15] = pow2(o2w[:, 12:15], k)
        flat = trx.flat_build_instanced(verts, base.counts, base.inst_obj, o2w)
    else:
        flat = trx.flat_build(verts, base.counts)
    return _finish(trx, base, k, flat)


def carry(prim, inst, frm, to):
    """Hit records and instance ids of tree `frm` in the numbering of tree `to`, t times 2^(to.k - frm.k); a miss stays one."""
    out = np.zeros(prim.shape[0], dtype=HIT)
    out["t"] = pow2(prim["t"], to.k - frm.k)
    hit = prim["prim"] != INVALID
    out["prim"] = INVALID
    out["prim"][hit] = to.prim_of_source[frm.flat.tri_source[prim["prim"][hit]]]
    ids = np.full(prim.shape[0], INVALID, dtype=np.uint32)
    if frm.tlas:
        had = np.asarray(inst, dtype=np.uint32) != INVALID
        ids[had] = to.inst_of_source[frm.flat.instance_source[np.asarray(inst, dtype=np.uint32)[had]]]
    return out, ids


def source_ids(s, prim, inst=None):
    """prim (and instance) words of tree `s` in the numbering of the input mesh, which no rebuild changes; 0xFFFFFFFF stays."""
    prim = np.asarray(prim, dtype=np.uint32)
    out = np.where(prim < s.flat.tri_source.size, s.flat.tri_source[np.minimum(prim, s.flat.tri_source.size - 1)], prim).astype(np.uint32)
    if inst is None or not s.tlas:
        return out
    inst = np.asarray(inst, dtype=np.uint32)
    return out, np.where(inst < N_INSTANCES, s.flat.instance_source[np.minimum(inst, N_INSTANCES - 1)], inst).astype(np.uint32)


# ---- what the caller passes ---------------------------------------------------------------------------------------------------

def scaled_params(base, k):
    """Every length parameter and light times 2^k, intensities unchanged: one point light, one rect light (8 samples, edges
    scaled), one directional light (unchanged), placed around the point the camera looks at."""
    c = base.look.astype(np.float32)
    p = types.SimpleNamespace(k=k, light_samples=8, emitter_eps=0.001, depth_tol=0.1, normal_cos=0.9)
    for name, value in (("shadow_eps", 0.01), ("ao_eps", 0.01), ("ao_radius", 1.4), ("bounce_eps", 0.01)):
        setattr(p, name, float(pow2(f32(value), k)))
    point = (c + np.array([0.0, 0.8, 0.0], dtype=np.float32)).astype(np.float32)
    corner = (c + np.array([-0.4, 0.9, -0.4], dtype=np.float32)).astype(np.float32)
    p.point = Light(POINT, pow2(point, k), intensity=1.5)
    p.rect = Light(RECT, pow2(corner, k), pow2(np.array([0.8, 0.0, 0.0], dtype=np.float32), k), pow2(np.array([0.0, 0.0, 0.8], dtype=np.float32), k), intensity=2.0)
    p.directional = Light(DIRECTIONAL, (0.3, 1.0, 0.4), intensity=0.5)
    p.lights = [p.point, p.rect, p.directional]
    return p


# ---- the covariance table -----------------------------------------------------------------------------------------------------

def _tmax(a, k):
    """A ray's reach: times 2^k, except the two values that are no lengths - FLT_MAX (no reach) and the inert ray's -1."""
    a = np.asarray(a, dtype=np.float32)
    return np.where((a == F32_MAX) | (a < 0), a, pow2(a, k)).astype(np.float32)


SAME, LEN, AREA, INV_AREA, REACH = "same", "len", "area", "inv_area", "reach"
_RAYS = {"origin": LEN, "tmin": SAME, "direction": SAME, "tmax": REACH}
# output -> component -> how it follows from the k = 0 value.  Barycentrics, normals, directions, cast masks, wgeo, selection
# indices and 8-bit counts are the same bits; origins, tmax and t are multiplied by 2^k; the geometric normal of an emitter
# record (an area) by 2^2k; the light term of point and rect lights (an inverse square) by 2^-2k.
RULES = {
    "primary": {"t": LEN, "prim": SAME, "inst": SAME},
    "attr": {"u": SAME, "v": SAME, "normal": SAME}, "bounce_attr": {"u": SAME, "v": SAME, "normal": SAME},
    "ao_rays": _RAYS, "light_rays_point": _RAYS, "light_rays_rect0": _RAYS, "light_rays_rect7": _RAYS, "light_rays_directional": _RAYS,
    "bounce_light_rays_point": _RAYS, "bounce_light_rays_rect": _RAYS, "bounce_light_rays_directional": _RAYS, "emitter_rays": _RAYS,
    "emitter_wgeo": {"wgeo": SAME},
    "light_term_local": {"term": INV_AREA},               # point + rect lights, no ambient
    "light_term_directional": {"term": SAME},             # a directional light and the ambient term
    "bounce_weight_point": {"g": INV_AREA}, "bounce_weight_directional": {"g": SAME},
    "emitter_records": {"V0": LEN, "kinv": SAME, "E1": LEN, "E2": LEN, "NG": AREA, "material": SAME, "prim": SAME, "inst": SAME},
    "selection": {"P": SAME, "kinv": SAME, "c": SAME},
    "emitter_c": {"c": SAME},                             # (what trx_scene_get_emitters hands out beside the records)
    "emitter_select": {"j": SAME},
    "emitter_sample": {"j": SAME, "l": SAME, "wgeo": SAME, "cast": SAME, "y": LEN, "tmax": LEN},
    "ao_filter": {"term": SAME}, "ao_upsample": {"term": SAME}, "value_filter": {"value": SAME}, "value_upsample": {"value": SAME},
}


def expect_from_base(name_of_output, base_value, k):
    """What output `name_of_output` must be at exponent k, from its k = 0 value (a dictionary component -> array)."""
    rules = RULES[name_of_output]
    assert set(rules) == set(base_value), (name_of_output, sorted(base_value))
    out = {}
    for comp, a in base_value.items():
        rule = rules[comp]
        out[comp] = (a if rule == SAME else pow2(a, k) if rule == LEN else pow2(a, 2 * k) if rule == AREA else pow2(a, -2 * k) if rule == INV_AREA
                     else _tmax(a, k))
    return out


def differing(got, want):
    """The comparison rule, for one component: bit for bit, NaN-ness compared and not the payload (an x86 twin and the device
    produce different default NaNs).  Returns the indices of the records that differ; nothing is left out for being non-finite."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        gn, wn = np.isnan(got), np.isnan(want)
        bad = (gn != wn) | (~gn & (got.view(np.uint32) != want.view(np.uint32)))
    elif got.dtype.names:                                     # (a structured array of integers: field by field)
        bad = np.zeros(got.shape, dtype=bool)
        for f in got.dtype.names:
            bad |= got[f] != want[f]
    else:
        bad = got != want
    return np.flatnonzero(bad.reshape(bad.shape[0], -1).any(1)) if bad.ndim > 1 else np.flatnonzero(bad)


def assert_same(got, want, what):
    """Every component of an output against its expectation, under `differing`."""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for comp in got:
        bad = differing(got[comp], want[comp])
        assert bad.size == 0, "%s, %s: %d of %d records differ, first %s: %s != %s" % (what, comp, bad.size, np.asarray(got[comp]).shape[0], bad[:4],
                                                                                      np.asarray(got[comp])[bad[:2]], np.asarray(want[comp])[bad[:2]])


def share_same(got, want):
    """The share of records (over every component) that equal their expectation - the tables of DESIGN.md."""
    n = np.asarray(next(iter(got.values()))).shape[0]
    bad = np.zeros(n, dtype=bool)
    for comp in got:
        bad[differing(got[comp], want[comp])] = True
    return 1.0 - bad.sum() / max(n, 1)


def rays_of(rays):
    """A [n] ray array (or [n, 8] words) as the components of _RAYS."""
    r = np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)
    return {"origin": r[:, 0:3].copy(), "tmin": r[:, 3].copy(), "direction": r[:, 4:7].copy(), "tmax": r[:, 7].copy()}


def emitter_records_of(s, rec):
    """[n, 16] emitter records as components; the prim and instance words in the input mesh's numbering."""
    rec = np.ascontiguousarray(rec, dtype=np.float32).reshape(-1, 16)
    bits = rec.view(np.uint32)
    ids = source_ids(s, bits[:, 11], bits[:, 15])
    prim, inst = ids if s.tlas else (ids, bits[:, 15].copy())
    return {"V0": rec[:, 0:3].copy(), "kinv": rec[:, 3].copy(), "E1": rec[:, 4:7].copy(), "E2": rec[:, 8:11].copy(), "NG": rec[:, 12:15].copy(),
            "material": bits[:, 7].copy(), "prim": prim, "inst": inst}


# ---- the adversarial scalings: no powers of two, caller records alone -------------------------------------------------------------

def adversarial(trx, name, w=40, h=24, n=4096):
    """One of tests/adversarial_scenes.py's three scalings (`n` triangles are enough for kernels that walk nothing) with its
    camera, and a sentinel-free frame of caller records whose prim cycles through the triangles: every record a surface
    record, t the distance from the eye to the triangle's first vertex (rounded; finite, or the record is a miss by rule)."""
    import adversarial_scenes as AS
    verts = np.ascontiguousarray(AS.FINITE[name](n), dtype=np.float32)
    flat = trx.flat_build(verts)
    eye, look, fov = AS.camera_for(verts)
    s = types.SimpleNamespace(name=name, k=0, w=w, h=h, flat=flat, view=trx.view_from_camera(eye, look, fov, w, h), tlas=False, o2w=None)
    s.mats = np.zeros((2, 6), dtype=np.float32)
    s.mats[:, :3], s.mats[1, 3:] = 0.5, (1.0, 2.0, 3.0)
    s.idx = np.zeros(n, dtype=np.uint16)
    s.idx[::97] = 1
    prim = np.zeros(w * h, dtype=HIT)
    prim["prim"] = (np.arange(w * h, dtype=np.uint64) * 7 % n).astype(np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = flat.tri_verts[prim["prim"], 0:3].astype(np.float64) - np.array(eye, dtype=np.float64)[None, :]
        prim["t"] = np.sqrt((d * d).sum(1)).astype(np.float32)
    return s, prim, np.full(w * h, INVALID, dtype=np.uint32), adversarial_params(verts)


def adversarial_params(verts):
    """scaled_params' lights and lengths for a scene of any size: placed by the vertex bounds (in binary64, kept finite in
    binary32), the lengths a hundredth of the smallest extent."""
    pts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    c, e = 0.5 * (lo + hi), hi - lo
    fin = lambda v: np.clip(v, -3e38, 3e38).astype(np.float32)  # noqa: E731
    p = types.SimpleNamespace(k=None, light_samples=8, emitter_eps=0.001, depth_tol=0.1, normal_cos=0.9)
    p.shadow_eps = p.ao_eps = p.bounce_eps = float(np.float32(0.01 * e.min()))
    p.ao_radius = float(np.float32(0.7 * e.min()))
    p.point = Light(POINT, fin(c + np.array([0.0, 0.4, 0.0]) * e), intensity=1.5)
    p.rect = Light(RECT, fin(c + np.array([-0.2, 0.45, -0.2]) * e), fin(np.array([0.4, 0.0, 0.0]) * e), fin(np.array([0.0, 0.0, 0.4]) * e), intensity=2.0)
    p.directional = Light(DIRECTIONAL, (0.3, 1.0, 0.4), intensity=0.5)
    p.lights = [p.point, p.rect, p.directional]
    return p
