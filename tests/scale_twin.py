"""What the scale tests compute on the CPU (tests/test_scale.py, tests/test_gpu_scale.py): the frame of caller records of a
scene at exponent k, carried from the k = 0 walk (tests/scale_cases.py), and every post-walk output of the twins over it -
one dictionary output -> components, in the layout of scale_cases.RULES.  The twins are the existing ones, unchanged; the
oracle is called for its AO ray and its noise, never for a walk (the walks of the k = 0 base and of WALKED are the tests')."""
import types

import numpy as np

import ao_sparse_twin as AS
import emitter_twin as ET
import image_twin as IM
import indirect_sparse_twin as IS
import indirect_twin as IT
import light_twin as LT
import scale_cases as SC
import value_filter_twin as VF
from ao_visibility_twin import NO_SURFACE, ao_rays
from hit_attr_twin import hit_attrs, primary_dirs, primary_origins, tri_records
from helpers import w2o_rows

f32 = np.float32
AO_SAMPLES, AO_FRAME, LIGHT_FRAME0, BOUNCE_FRAME, EMITTER_FRAME0, EMITTER_SAMPLE = 4, 3, 5, 11, 7, 2
STRIDE, PHASE, UP_RADIUS, LEVELS, AO_DEPTH_TOL = 2, 3, 1, 3, 0.02
LIGHT_RUNS = (("point", 0, 0), ("rect0", 1, 0), ("rect7", 1, 7), ("directional", 2, 0))     # (name, light index, sample)


def oracle_scene(orc, s, w2o=None):
    """The oracle's scene over tree `s`; w2o: the world-to-object rows to give it (default helpers.w2o_rows of every instance)."""
    flat = s.flat
    if s.tlas and w2o is None:
        w2o = np.stack([w2o_rows(m) for m in flat.instance_transforms])
    return orc.Scene(flat.nodes, flat.tri_verts, flat.instance_offsets, flat.tlas_start, instance_w2o=w2o if s.tlas else None,
                     instance_entry=getattr(flat, "instance_entry", None))


def base_frame(orc, s0, p0):
    """The k = 0 frame: the oracle's primary records over the base tree and, for the bounce outputs, one sample's bounce rays
    with the oracle's closest hits."""
    osc = oracle_scene(orc, s0)
    oview = orc.view_from_bytes(bytes(s0.view))
    prim, inst, _ = osc.trace_primary_inst(oview, s0.w, s0.h)
    if not s0.tlas:
        inst = np.full(prim.shape[0], SC.INVALID, dtype=np.uint32)
    b_rays, _ = ao_rays(orc, osc, oview, s0.w, s0.h, prim, inst, BOUNCE_FRAME, p0.bounce_eps, float("inf"))
    b_hits, b_inst, _ = osc.trace_rays_inst(b_rays)
    if not s0.tlas:
        b_inst = np.full(prim.shape[0], SC.INVALID, dtype=np.uint32)
    return types.SimpleNamespace(prim=prim, inst=inst, b_rays=b_rays, b_hits=b_hits, b_inst=b_inst)


def carried_frame(orc, s0, f0, s):
    """`f0` (the base frame) as caller records of tree `s`: t times 2^k, prim and instance ids in the tree's numbering, the
    bounce rays' origins times 2^k."""
    prim, inst = SC.carry(f0.prim, f0.inst, s0, s)
    b_hits, b_inst = SC.carry(f0.b_hits, f0.b_inst, s0, s)
    b_rays = f0.b_rays.copy()
    b_rays["origin"] = SC.pow2(f0.b_rays["origin"], s.k - s0.k)
    return types.SimpleNamespace(prim=prim.view(orc.HIT_DTYPE), inst=inst, b_rays=b_rays, b_hits=b_hits.view(orc.HIT_DTYPE), b_inst=b_inst)


def synthetic(s, prim):
    """The image kernels' inputs that no scale changes: AO counts, visibility planes, a value plane and the low grids, drawn
    once per frame size over the surface mask (the same bits at every k: t stays below FLT_MAX)."""
    n = s.w * s.h
    rng = np.random.default_rng(1000 * s.w + s.h)
    surf = IM.surface(prim)
    counts = np.where(surf, rng.integers(0, AO_SAMPLES + 1, n), NO_SURFACE).astype(np.uint8)
    planes = np.where(surf[None, :], rng.integers(0, 9, (3, n)), LT.NO_SURFACE).astype(np.uint8)
    planes[0] = np.minimum(planes[0], np.where(surf, 1, LT.NO_SURFACE))                       # (a point light: one sample)
    planes[2] = np.minimum(planes[2], np.where(surf, 1, LT.NO_SURFACE))                       # (a directional light: one sample)
    values = rng.uniform(0.0, 2.0, n).astype(np.float32)
    values[::5] = f32(-0.0)
    return types.SimpleNamespace(counts=counts, planes=planes, values=values, counts_lo=AS.sparse_counts(counts, s.w, s.h, STRIDE, PHASE),
                                 values_lo=IS.sparse_values(values, prim, s.w, s.h, STRIDE, PHASE),
                                 u0=np.concatenate([np.linspace(0.0, 1.0, 61), [0.5, 1.0]]).astype(np.float32))


def emitter_table(s, recs):
    """(records [n, 16], c, P, kinv) of the twin's emitter table over tree `s`."""
    inst_prims = ET.instance_prims(s.flat.nodes, s.flat.instance_offsets, s.flat.tlas_start, entry=getattr(s.flat, "instance_entry", None)) if s.tlas else None
    pair = ET.pairs(ET.emissive(s.mats, s.idx), inst_prims)
    with np.errstate(all="ignore"):
        rec = ET.records(recs, pair, s.idx, s.o2w)
        P, kinv, c = ET.selection(rec, s.mats)
    rec[:, 3] = kinv
    return rec, c, P, kinv


def attr_of(a):
    return {"u": a["u"].copy(), "v": a["v"].copy(), "normal": a["normal"].copy()}


def twin_outputs(orc, s, p, f, w2o=None, only=None):
    """Every post-walk output of the twins over frame `f` of tree `s` under parameters `p`.  w2o: the world-to-object rows (the
    device's own on the GPU; default helpers.w2o_rows).  only: a set of output names to restrict the work to."""
    w, h, view = s.w, s.h, s.view
    n = w * h
    if s.tlas and w2o is None:
        w2o = np.stack([w2o_rows(m) for m in s.flat.instance_transforms])
    if not s.tlas:
        w2o = None
    with np.errstate(all="ignore"):
        recs = tri_records(s.flat.tri_verts)
    osc = oracle_scene(orc, s, w2o)
    oview = orc.view_from_bytes(bytes(view))
    syn = synthetic(s, f.prim)
    out = {}
    py, px = np.divmod(np.arange(n), w)
    with np.errstate(all="ignore"):
        attr = hit_attrs(recs, primary_origins(view, n), primary_dirs(view, w, h, px, py), f.prim["prim"], inst=f.inst if s.tlas else None, w2o=w2o)
        out["attr"] = attr_of(attr)
        normals = attr["normal"]
        out["ao_rays"] = SC.rays_of(ao_rays(orc, osc, oview, w, h, f.prim, f.inst, AO_FRAME, p.ao_eps, p.ao_radius)[0])
        geo = LT.frame_geometry(view, w, h, f.prim, f.inst, recs, w2o)
        for name, index, sample in LIGHT_RUNS:
            out["light_rays_" + name] = SC.rays_of(LT.light_rays(orc, view, w, h, geo, p.lights[index], index, LIGHT_FRAME0, sample, p.shadow_eps)[0])
        out["light_term_local"] = {"term": LT.light_term(view, w, h, f.prim, normals, syn.planes[:2], p.lights[:2], p.light_samples, 0.0)}
        out["light_term_directional"] = {"term": LT.light_term(view, w, h, f.prim, normals, syn.planes[2:], p.lights[2:], p.light_samples, 0.25)}
        # the bounce: caller records too - the rays, their hits and the attribute records of those hits
        b_attr = hit_attrs(recs, f.b_rays["origin"], f.b_rays["direction"], f.b_hits["prim"], inst=f.b_inst if s.tlas else None, w2o=w2o)
        out["bounce_attr"] = attr_of(b_attr)
        for name, index, sample in LIGHT_RUNS[:2] + LIGHT_RUNS[3:]:
            out["bounce_light_rays_" + name.rstrip("0")] = SC.rays_of(
                IT.secondary_rays(orc, w, h, f.b_rays, f.b_hits, b_attr, p.lights[index], index, LIGHT_FRAME0, sample, p.shadow_eps)[0])
        out["bounce_weight_point"] = {"g": IT.light_weight(f.b_rays, f.b_hits, b_attr, p.point)}
        out["bounce_weight_directional"] = {"g": IT.light_weight(f.b_rays, f.b_hits, b_attr, p.directional)}
        # the emitters
        rec, c, P, kinv = emitter_table(s, recs)
        out["emitter_records"] = SC.emitter_records_of(s, rec)
        out["selection"] = {"P": P, "kinv": kinv, "c": c}
        out["emitter_c"] = {"c": c}
        out["emitter_select"] = {"j": ET.select(c, syn.u0)}
        e_rays, _, wgeo, _ = ET.primary_rays(orc, view, w, h, geo, rec, c, EMITTER_FRAME0, EMITTER_SAMPLE, p.shadow_eps, p.emitter_eps)
        out["emitter_rays"], out["emitter_wgeo"] = SC.rays_of(e_rays), {"wgeo": wgeo}
        idx, gx, gy, d, gn, t = geo
        o = ((np.array(view.eye, dtype=np.float32)[None, :] + d * t[:, None]).astype(np.float32) - d * f32(p.shadow_eps)).astype(np.float32)
        sm = ET.sample(rec, c, gx, gy, (EMITTER_FRAME0 + ET.SEED_PRIMARY + EMITTER_SAMPLE) & 0xFFFFFFFF, p.emitter_eps, o, gn)
        out["emitter_sample"] = {key: np.asarray(sm[key]) for key in ("j", "l", "wgeo", "cast", "y", "tmax")}
        # the image kernels over the scaled t and this k's normals
        out.update(image_outputs(s, p, f.prim, normals, syn))
    return out if only is None else {name: v for name, v in out.items() if name in only}


def image_outputs(s, p, prim, normals, syn):
    """The AO filter and upsample, the value filter (3 levels) and upsample over records `prim` and `normals` [w * h, 3]."""
    w, h = s.w, s.h
    with np.errstate(all="ignore"):
        return {"ao_filter": {"term": IM.ao_filter(prim, normals, syn.counts, w, h, AO_SAMPLES, 1, AO_DEPTH_TOL, p.normal_cos)},
                "ao_upsample": {"term": AS.ao_upsample(prim, normals, syn.counts_lo, w, h, STRIDE, PHASE, AO_SAMPLES, UP_RADIUS, AO_DEPTH_TOL, p.normal_cos)},
                "value_filter": {"value": VF.value_filter(prim, normals, syn.values, w, h, LEVELS, p.depth_tol, p.normal_cos)},
                "value_upsample": {"value": IS.value_upsample(prim, normals, syn.values_lo, w, h, STRIDE, PHASE, UP_RADIUS, p.depth_tol, p.normal_cos)}}


# ---- the regimes of the normal ------------------------------------------------------------------------------------------------

def normal_regime(s, f, w2o=None):
    """Per surface pixel of frame `f`: (dot(ng, ng) as the attribute pass forms it, the twin's normal [n, 3])."""
    if s.tlas and w2o is None:
        w2o = np.stack([w2o_rows(m) for m in s.flat.instance_transforms])
    with np.errstate(all="ignore"):
        recs = tri_records(s.flat.tri_verts)
    surf = np.flatnonzero(LT.surface(f.prim, recs.shape[0]))
    t = recs[f.prim["prim"][surf]]
    nx, ny, nz = t[:, 9], t[:, 10], t[:, 11]
    with np.errstate(all="ignore"):
        if s.tlas:
            m = w2o[f.inst[surf]]
            r = [m[:, 4 * i:4 * i + 4] for i in range(3)]
            nx, ny, nz = [(r[0][:, i] * t[:, 9] + r[1][:, i] * t[:, 10]) + r[2][:, i] * t[:, 11] for i in range(3)]
        q = ((nx * nx + ny * ny) + nz * nz).astype(np.float32)
    return surf, q


def primary_of(s, prim, inst):
    """Primary records as components, prim and instance ids in the input mesh's numbering."""
    ids = SC.source_ids(s, prim["prim"], inst)
    p, i = ids if s.tlas else (ids, np.full(prim.shape[0], SC.INVALID, dtype=np.uint32))
    return {"t": np.asarray(prim["t"], dtype=np.float32).copy(), "prim": p, "inst": i}


# ---- the table of DESIGN.md ("scene scale") -----------------------------------------------------------------------------------

def _share(x):
    """A share as the table prints it: 100 only when no record differs, 0 only when every record does."""
    return "100" if x == 1.0 else "0" if x == 0.0 else "%.1f" % min(max(100.0 * x, 0.1), 99.9)


def table_rows(trx, orc, base, s0, f0, out0):
    """The markdown rows of DESIGN.md's table for one case: per exponent of SAFE and EDGE the regime of the normal over the
    surface pixels (how many differ from the k = 0 normal, have a denormal dot(ng, ng), are non-finite, are all-zero), then per
    output the share of the frame's records (in per cent) that are the k = 0 records under scale_cases.expect_from_base."""
    ks = sorted(SC.SAFE + SC.EDGE)
    tiny = np.float32(np.finfo(np.float32).tiny)
    regime, shares = [], {name: [] for name in out0}
    for k in ks:
        s, p = SC.scaled(trx, base, k), SC.scaled_params(base, k)
        f = carried_frame(orc, s0, f0, s)
        out = twin_outputs(orc, s, p, f)
        surf, q = normal_regime(s, f)
        n = out["attr"]["normal"][surf]
        regime.append("| %+d | %d | %d | %d | %d | %d |" % (k, surf.size, SC.differing(n, out0["attr"]["normal"][surf]).size, int(((q > 0) & (q < tiny)).sum()),
                                                          int((~np.isfinite(n)).any(1).sum()), int((n == 0).all(1).sum())))
        for name in out0:
            shares[name].append(_share(SC.share_same(out[name], SC.expect_from_base(name, out0[name], k))))
    rows = ["| k | surface pixels | normal differs | dot(ng, ng) denormal | normal non-finite | normal all-zero |", "|---|---|---|---|---|---|"] + regime
    rows += ["| output | " + " | ".join("%+d" % k for k in ks) + " |", "|---|" + "---|" * len(ks)]
    return rows + ["| %s | %s |" % (name, " | ".join(shares[name])) for name in out0]
