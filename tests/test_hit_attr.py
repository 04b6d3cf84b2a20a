"""Hit attributes (include/trx.h, trx_hit_attr) without a GPU: the record and its entry points at the boundary, and the
numpy twin of the definition (tests/hit_attr_twin.py) checked on the oracle's hits - clear sign bits, the barycentric
point on the ray, a unit normal perpendicular to the triangle - which pins the convention (u weights v1, v weights v2)
independently of the device.  tests/test_gpu_hit_attr.py holds the device to the twin bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import aimed_rays, golden_inputs, instanced_scene, random_rays, w2o_rows
from hit_attr_twin import ATTR_DTYPE, hit_attrs, object_rays, primary_dirs, primary_origins, tri_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("trx_hit_attributes_rays_dev", "trx_hit_attributes_primary_dev", "trx_trace_rays_attr")


# ---- the boundary ------------------------------------------------------------------------------------------------

def test_record_layout_matches_the_header(trx):
    from tray_racing_amd import _lib
    assert C.sizeof(_lib.HitAttr) == 24 and trx.HitAttr is _lib.HitAttr
    assert [f[0] for f in _lib.HitAttr._fields_] == ["u", "v", "normal", "_pad"]
    assert trx.HIT_ATTR_DTYPE.itemsize == 24 and trx.HIT_ATTR_DTYPE == ATTR_DTYPE
    assert _lib.HitAttr.normal.offset == 8 and _lib.HitAttr._pad.offset == 20
    # ... and the header is still plain C11 with the same layout
    src = (b'#include <stddef.h>\n#include "trx.h"\n'
           b'_Static_assert(sizeof(trx_hit_attr) == 24, "size");\n'
           b'_Static_assert(offsetof(trx_hit_attr, v) == 4 && offsetof(trx_hit_attr, normal) == 8, "fields");\n'
           b'_Static_assert(offsetof(trx_hit_attr, _pad) == 20, "pad");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", "-I",
                    os.path.join(ROOT, "include"), "-"], input=src, check=True)


def test_entry_points_are_declared_exported_and_bound(trx):
    from tray_racing_amd import _lib
    header = open(os.path.join(ROOT, "include", "trx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    lib = trx.load()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and (" T %s\n" % name) in out and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for name in ("trace_rays_attr", "hit_attributes_rays_dev", "hit_attributes_primary_dev"):
        assert callable(getattr(trx.Scene, name))


def test_bad_input_is_a_status_not_a_crash(trx):
    from tray_racing_amd import _lib
    lib = trx.load()
    view = _lib.View()
    attr = np.zeros(4, dtype=trx.HIT_ATTR_DTYPE)
    rays = np.zeros(4, dtype=trx.RAY_DTYPE)
    hits = np.zeros(4, dtype=trx.HIT_DTYPE)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.trx_hit_attributes_rays_dev(None, None, 4, None, None, None, None) == _lib.TRX_ERR_INVALID
    assert lib.trx_hit_attributes_rays_dev(None, None, 0, None, None, None, None) == _lib.TRX_ERR_INVALID
    assert lib.trx_hit_attributes_primary_dev(None, C.byref(view), 8, 8, _lib.Shard(0, 1, 0, 0), None, None, None,
                                              None) == _lib.TRX_ERR_INVALID
    assert lib.trx_trace_rays_attr(None, P(rays), 4, 0, P(hits), None, P(attr), None) == _lib.TRX_ERR_INVALID
    assert lib.trx_trace_rays_attr(None, None, 0, 0, None, None, None, None) == _lib.TRX_ERR_INVALID
    assert b"null" in lib.trx_last_error()
    assert not attr.view(np.uint32).any()
    if lib.trx_device_count() == 0:
        # no device: there is no scene to call them on - scene creation is where the absence is reported
        with pytest.raises(trx.TrxError) as e:
            trx.Scene(trx.flat_build(trx.gen_scene("soup", 50, 1)[0]))
        assert e.value.code == _lib.TRX_ERR_NO_DEVICE


# ---- the twin on the oracle's hits ---------------------------------------------------------------------------------

def _golden(trx, orc, name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    nodes, tri_verts, inst, tlas_start = golden_inputs(trx, g)
    view = orc.view_from_bytes(g["view"].tobytes())
    return g, orc.Scene(nodes, tri_verts, inst, tlas_start), tri_verts, view, int(g["width"]), int(g["height"])


def _check_geometry(attr, hits, origins, dirs, tri_verts, prims, inst=None, w2o=None, what=""):
    """The properties that pin the definition: every committed test has u, v, 1 - u - v >= 0 (sign bits clear), the
    barycentric point is the ray's point at t, the normal is unit length and perpendicular to both world-space edges."""
    sel = np.flatnonzero(hits["prim"] != 0xFFFFFFFF)
    assert sel.size > 50, what
    a = attr[sel]
    u, v = a["u"], a["v"]
    w = (np.float32(1.0) - u) - v
    for name, x in (("u", u), ("v", v), ("1-u-v", w)):
        assert not (x.view(np.uint32) >> 31).any(), "%s: %s has a set sign bit" % (what, name)
    tv = np.asarray(tri_verts, dtype=np.float64).reshape(-1, 9)[prims[sel]]
    v0, v1, v2 = tv[:, 0:3], tv[:, 3:6], tv[:, 6:9]
    o, d = object_rays(origins[sel], dirs[sel], None if inst is None else inst[sel], w2o)
    p_bary = (1.0 - u - v).astype(np.float64)[:, None] * v0 + u.astype(np.float64)[:, None] * v1 + v.astype(np.float64)[:, None] * v2
    p_ray = o + hits["t"][sel].astype(np.float64)[:, None] * d
    pts = np.asarray(tri_verts, dtype=np.float64).reshape(-1, 3)
    diag = float(np.linalg.norm(pts.max(0) - pts.min(0)))
    err = np.linalg.norm(p_bary - p_ray, axis=1)
    assert err.max() <= 1e-4 * diag, "%s: barycentric point %.3g off the ray (diag %.3g)" % (what, err.max(), diag)
    # (the other weighting - u on v2, v on v1 - must NOT fit: the convention is pinned, not just consistent)
    p_swapped = (1.0 - u - v).astype(np.float64)[:, None] * v0 + u.astype(np.float64)[:, None] * v2 + v.astype(np.float64)[:, None] * v1
    assert np.median(np.linalg.norm(p_swapped - p_ray, axis=1)) > 1e-3 * diag, what
    n = a["normal"].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-5, what
    e1, e2 = v1 - v0, v2 - v0
    if w2o is not None:
        rows = w2o[inst[sel]].astype(np.float64).reshape(-1, 3, 4)[:, :, :3]
        A = np.linalg.inv(rows)                                   # object-to-world linear part
        e1, e2 = np.einsum("nij,nj->ni", A, e1), np.einsum("nij,nj->ni", A, e2)
    for e in (e1, e2):
        cos = np.abs((n * e).sum(1)) / np.linalg.norm(e, axis=1)
        assert np.quantile(cos, 0.999) < 1e-5 and cos.max() < 1e-3, "%s: normal not perpendicular (%.3g)" % (what, cos.max())
    # misses (and only they) are all zero
    miss = np.flatnonzero(hits["prim"] == 0xFFFFFFFF)
    assert not attr[miss].view(np.uint32).reshape(-1, 6).any(), what


@pytest.mark.parametrize("name", ["cornell_64", "soup_52x44", "box14_tlas_48"])
def test_twin_on_oracle_primary_frames(trx, orc, name):
    g, osc, tri_verts, view, w, h = _golden(trx, orc, name)
    recs = tri_records(tri_verts)
    rays = osc.primary_rays(view, w, h)
    px, py = np.arange(w * h) % w, np.arange(w * h) // w
    dirs = primary_dirs(view, w, h, px, py)
    # the twin's primary_dir is the oracle's (and the kernel's) bit for bit
    assert (dirs.view(np.uint32) == rays["direction"].view(np.uint32)).all()
    for sem in (0, 3):
        hits, _ = osc.trace_primary(view, w, h, sem=sem)
        attr = hit_attrs(recs, primary_origins(view, w * h), dirs, hits["prim"])
        _check_geometry(attr, hits, rays["origin"], dirs, tri_verts, hits["prim"], what="%s primary sem %d" % (name, sem))


@pytest.mark.parametrize("name", ["cornell_64", "soup_52x44", "box14_tlas_48"])
def test_twin_on_oracle_explicit_rays(trx, orc, name):
    g, osc, tri_verts, view, w, h = _golden(trx, orc, name)
    recs = tri_records(tri_verts)
    flat = type("F", (), {"tri_verts": tri_verts})
    rays = np.concatenate([random_rays(trx, flat, 3000, 5), aimed_rays(trx, tri_verts, 3000, 6)])
    for sem in (0, 2, 3, 7):
        hits, inst, _ = osc.trace_rays_inst(rays, sem=sem)
        attr = hit_attrs(recs, rays["origin"], rays["direction"], hits["prim"])
        _check_geometry(attr, hits, rays["origin"], rays["direction"], tri_verts, hits["prim"],
                        what="%s rays sem %d" % (name, sem))


def test_twin_on_oracle_f16_records(trx, orc):
    """TRX_TRI_F16_24 records: the twin decodes the f16 edges as the upload does (the oracle's own decode agrees)."""
    g = np.load(os.path.join(GOLDEN, "kitchen_tlas_f16_56x40.npz"))
    nodes, tri_verts, inst_off, tlas_start = golden_inputs(trx, g)
    osc = orc.Scene(nodes, None, inst_off, tlas_start, tri_f16=g["tri_f16"])
    recs = tri_records(tri_f16=g["tri_f16"])
    assert (recs[:, 0:9].view(np.uint32) == osc.tris.view(np.uint32)).all()
    # the f16 triangles' own vertices (v1 = v0 - e1, v2 = v0 + e2 exactly as the records hold them)
    v16 = np.concatenate([recs[:, 0:3], recs[:, 0:3].astype(np.float64) - recs[:, 3:6], recs[:, 0:3].astype(np.float64) + recs[:, 6:9]], 1)
    rays = g["rays"]
    hits, inst, _ = osc.trace_rays_inst(rays, sem=0)
    attr = hit_attrs(recs, rays["origin"], rays["direction"], hits["prim"])
    _check_geometry(attr, hits, rays["origin"], rays["direction"], v16, hits["prim"], what="f16 rays")


def test_twin_on_oracle_transformed_instances(trx, orc):
    flat, o2w, world, first, _ = instanced_scene(trx)
    w2o = np.stack([w2o_rows(m) for m in flat.instance_transforms])
    osc = orc.Scene(flat.nodes, flat.tri_verts, flat.instance_offsets, flat.tlas_start, instance_w2o=w2o)
    recs = tri_records(flat.tri_verts)
    wflat = type("W", (), {"tri_verts": world})
    rays = np.concatenate([random_rays(trx, wflat, 2000, 7), aimed_rays(trx, world, 4000, 8)])
    for sem in (0, 3):
        hits, inst, _ = osc.trace_rays_inst(rays, sem=sem)
        attr = hit_attrs(recs, rays["origin"], rays["direction"], hits["prim"], inst, w2o)
        _check_geometry(attr, hits, rays["origin"], rays["direction"], flat.tri_verts, hits["prim"], inst, w2o,
                        what="instanced rays sem %d" % sem)
        # an instance outside the table, or a record past the triangles, is all zero
        bad = hit_attrs(recs, rays["origin"][:4], rays["direction"][:4], [0, 1, len(recs), 0xFFFFFFFF],
                        [len(w2o), 0xFFFFFFFF, 0, 0], w2o)
        assert not bad.view(np.uint32).any()
