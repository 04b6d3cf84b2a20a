"""Emitters without a GPU (include/trx.h, "emitters"): the boundary (symbols, plain C, ABI version), the refusals decided
before a device is touched, the table rules of the twin (tests/emitter_twin.py) on hand-made inputs - one emitter, a
zero-area emitter among real ones, all areas zero, 1 000 emitters of very unequal area, two-level pairs in the stated order -
selection at u0 = 0, 1.0, every c_i and its two float neighbours against the device's bisection restated, every sampled
point inside its triangle, the twin's noise against the oracle's, the twin's node walk against the builder's own triangle
ranges, the estimator's constant on the oracle, the new kernels' resources, and the command line's new refusals."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import emitter_twin as ET
import light_twin as LT
import material_twin as MT
import noise_domain as ND
from ao_visibility_twin import golden_case
from hit_attr_twin import tri_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW_SYMBOLS = ("trx_scene_build_emitters", "trx_scene_get_emitters", "trx_emitter_rays_dev", "trx_trace_emitter_light_dev",
               "trx_trace_indirect_rgb_emitters_dev", "trx_trace_indirect_rgb_emitters_sparse_dev", "trx_render_image_colour_emitters")
NEW_KERNELS = ("k_emitter_build", "k_emitter_select", "k_emitter_rays", "k_emitter_gather_rgb", "k_bounce_emitter_rays", "k_bounce_emitter_gather")


# ---- the boundary ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_bound(trx):
    from tray_racing_amd import _lib
    header = open(os.path.join(ROOT, "include", "trx.h")).read()
    dev = open(os.path.join(ROOT, "include", "trx_dev.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    lib = trx.load()
    for name in NEW_SYMBOLS + ("trx_debug_emitter_select",):
        assert (" T %s\n" % name) in out and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert name + "(" in (dev if name.startswith("trx_debug_") else header)
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [2, 4, 13, 16, 18, 19, 30]
    for name in ("build_emitters", "get_emitters", "emitter_rays_dev", "trace_emitter_light_dev", "trace_indirect_rgb_emitters_dev",
                 "trace_indirect_rgb_emitters_sparse_dev", "render_image_colour_emitters", "debug_emitter_select"):
        assert callable(getattr(trx.Scene, name)), name
    assert trx.MAX_EMITTERS == 1 << 20 == ET.MAX_EMITTERS
    src = (b'#include "trx.h"\n'
           b'_Static_assert(TRX_MAX_EMITTERS == 1048576u, "2^20");\n'
           b'int f(trx_scene *s, const trx_view *v, const trx_hit *p, float *out, trx_ray *rays, unsigned char *img) {\n'
           b'    trx_shard whole = {0, 1, TRX_LAYOUT_IMAGE, 0};\n'
           b'    uint32_t n = 0;\n'
           b'    int rc = trx_scene_build_emitters(s, &n) | trx_scene_get_emitters(s, out, &n, out);\n'
           b'    rc |= trx_emitter_rays_dev(s, v, 8, 8, whole, 0, TRX_MAX_AO_SAMPLES - 1, 0.01f, 0.001f, p, 0, rays, 0);\n'
           b'    rc |= trx_trace_emitter_light_dev(s, v, 8, 8, whole, 0, 0, 0, 4, 0.01f, 0.001f, p, 0, out, out, 0);\n'
           b'    rc |= trx_trace_indirect_rgb_emitters_dev(s, v, 8, 8, whole, 0, 0, 0, 0, 0, 4, 0.01f, 0.01f, 0.001f, p, 0, out, 0);\n'
           b'    rc |= trx_trace_indirect_rgb_emitters_sparse_dev(s, v, 8, 8, 2, 3, 0, 0, 0, 0, 0, 4, 0.01f, 0.01f, 0.001f, p, 0, out, 0);\n'
           b'    return rc | trx_render_image_colour_emitters(s, v, 8, 8, 0, 0, 0, 0, 0, 1, 0.01f, 0.1f, 0, 0.01f, 1.0f, 0, 0.02f, 0.9f, 4, 0.01f, 3,\n'
           b'                                                 0.1f, 0.9f, 2, 0, 1, 4, 0.001f, img, 0);\n}\n'
           b'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", "-I",
                    os.path.join(ROOT, "include"), "-"], input=src, check=True)
    assert lib.trx_abi_version() == 1   # additions only


def test_bad_arguments_are_refused_before_any_device_work(trx):
    from tray_racing_amd import _lib
    lib = trx.load()
    buf = np.zeros(64, dtype=np.uint32)
    P = buf.ctypes.data_as(C.c_void_p)
    inv, view, whole, n = _lib.TRX_ERR_INVALID, _lib.View(), _lib.Shard(0, 1, 0, 0), C.c_uint32(4)
    NAN = float("nan")
    assert lib.trx_scene_build_emitters(None, C.byref(n)) == inv
    assert lib.trx_scene_get_emitters(None, P, C.byref(n), P) == inv and lib.trx_scene_get_emitters(P, None, C.byref(n), P) == inv
    assert lib.trx_scene_get_emitters(P, P, None, P) == inv and lib.trx_scene_get_emitters(P, P, C.byref(n), None) == inv
    assert lib.trx_debug_emitter_select(None, P, 4, P) == inv and lib.trx_debug_emitter_select(P, None, 4, P) == inv
    assert lib.trx_debug_emitter_select(P, P, 4, None) == inv
    # (a scene pointer that is never dereferenced: every call below is refused on the arguments that come first)

    def rays(scene=P, sample=0, eps=0.01, eeps=0.001, prim=P, out=P):
        return lib.trx_emitter_rays_dev(scene, C.byref(view), 4, 4, whole, 0, sample, eps, eeps, prim, None, out, None)

    def light(scene=P, sem=0, mask=0, n_samples=4, eps=0.01, eeps=0.001, prim=P, out=P):
        return lib.trx_trace_emitter_light_dev(scene, C.byref(view), 4, 4, whole, sem, mask, 0, n_samples, eps, eeps, prim, None, None, out, None)
    for kw in ({"scene": None}, {"prim": None}, {"out": None}, {"sample": 64}, {"eps": -1.0}, {"eps": NAN}, {"eeps": -0.5}, {"eeps": 1.0}, {"eeps": NAN},
               {"eeps": float("inf")}):
        assert rays(**kw) == inv, kw
    assert b"emitter_eps" in lib.trx_last_error()
    for kw in ({"scene": None}, {"prim": None}, {"out": None}, {"n_samples": 0}, {"n_samples": 65}, {"sem": 8}, {"mask": 256}, {"eps": NAN}, {"eeps": 1.0},
               {"eeps": -1e-9}, {"eeps": NAN}):
        assert light(**kw) == inv, kw
    assert lib.trx_trace_indirect_rgb_emitters_dev(None, C.byref(view), 4, 4, whole, 0, 0, None, 0, 0, 4, 0.01, 0.01, 0.001, P, None, P, None) == inv
    assert lib.trx_trace_indirect_rgb_emitters_dev(P, C.byref(view), 4, 4, whole, 0, 0, None, 0, 0, 4, 0.01, 0.01, 0.001, P, None, None, None) == inv
    assert lib.trx_trace_indirect_rgb_emitters_sparse_dev(None, C.byref(view), 4, 4, 2, 0, 0, 0, None, 0, 0, 4, 0.01, 0.01, 0.001, P, None, P, None) == inv

    def render(scene=P, n_lights=0, ls=1, bn=2, samples=4, eeps=0.001, stride=1):
        return lib.trx_render_image_colour_emitters(scene, C.byref(view), 4, 4, 0, 0, None, n_lights, 0, ls, 0.01, 0.1, 0, 0.01, 1.0, 0, 0.02, 0.9, bn, 0.01,
                                                    0, 0.1, 0.9, stride, 0, 1, samples, eeps, P, None)
    for kw in ({"scene": None}, {"n_lights": 1}, {"ls": 0}, {"bn": 65}, {"samples": 0}, {"samples": 65}, {"eeps": 1.0}, {"eeps": NAN}, {"stride": 5}):
        assert render(**kw) == inv, kw
    assert not buf.any()


# ---- the table --------------------------------------------------------------------------------------------------------------

def _tri(v0, v1, v2):
    return np.array([*v0, *v1, *v2], dtype=np.float32)


def _checked_table(verts, materials, idx, pair=None, o2w=None):
    recs = tri_records(np.asarray(verts, dtype=np.float32).reshape(-1, 9))
    materials = np.asarray(materials, dtype=np.float32).reshape(-1, 6)
    if pair is None:
        pair = ET.pairs(ET.emissive(materials, idx))
    rec = ET.records(recs, pair, idx, o2w)
    P, kinv, c = ET.selection(rec, materials)
    n = rec.shape[0]
    assert P.shape == kinv.shape == (n,) and c.shape == (n - 1,)
    assert (P >= f32(0.5 / n) * f32(1 - 2 ** -23)).all() and abs(float(P.astype(np.float64).sum()) - 1.0) < n * 2.0 ** -24
    assert (kinv == (1.0 / (np.pi * P.astype(np.float64))).astype(np.float32)).all() and np.isfinite(kinv).all() and (kinv > 0).all()
    assert (np.diff(c) >= 0).all() and (c.size == 0 or (c[0] >= P[0] * f32(1 - 2 ** -23) and c[-1] < f32(1.0)))
    return rec, P, kinv, c, pair


def test_one_emitter():
    verts = [_tri((0, 0, 0), (1, 0, 0), (0, 2, 0)), _tri((0, 0, 1), (1, 0, 1), (0, 1, 1))]
    mats = [[0.8, 0.8, 0.8, 0, 0, 0], [0, 0, 0, 0, 2.5, 0]]
    rec, P, kinv, c, pair = _checked_table(verts, mats, [0, 1])
    assert pair.tolist() == [[0xFFFFFFFF, 1]] and P[0] == 1.0 and c.size == 0 and kinv[0] == f32(1.0 / np.pi)
    assert rec[0, 0:3].tolist() == [0, 0, 1] and rec[0, 4:7].tolist() == [1, 0, 0] and rec[0, 8:11].tolist() == [0, 1, 0] and rec[0, 12:15].tolist() == [0, 0, 1]
    assert rec.view(np.uint32)[0, [7, 11, 15]].tolist() == [1, 1, 0xFFFFFFFF]
    for u0 in (0.0, 0.5, 1.0, np.nan):
        assert ET.select(c, [u0]).tolist() == [0]


def test_a_zero_area_emitter_among_real_ones_and_all_areas_zero():
    flat = _tri((1, 1, 1), (1, 1, 1), (1, 1, 1))                         # a point
    line = _tri((0, 0, 0), (1, 0, 0), (2, 0, 0))                         # collinear
    verts = [_tri((0, 0, 0), (1, 0, 0), (0, 1, 0)), flat, _tri((0, 0, 0), (2, 0, 0), (0, 2, 0)), line]
    mats = [[0, 0, 0, 1, 1, 1]]
    rec, P, kinv, c, _ = _checked_table(verts, mats, [0, 0, 0, 0])
    # areas 0.5, 0, 2, 0: w = |NG| * 3 = 3, 0, 12, 0; the defensive half gives the degenerate ones 0.5 / 4
    want = np.array([0.5 * 3 / 15 + 0.125, 0.125, 0.5 * 12 / 15 + 0.125, 0.125])
    assert (P == want.astype(np.float32)).all() and (c == np.cumsum(want)[:3].astype(np.float32)).all()
    rec[:, 3] = kinv
    # a sample on a zero-area emitter is never cast: NG is zero, so a = 0 and wgeo = 0
    o, n = np.array([[0.3, 0.3, -1.0]] * 2, dtype=np.float32), np.array([[0, 0, 1.0]] * 2, dtype=np.float32)
    s = ET.sample(rec, c, None, None, 0, 0.001, o, n, u=(np.array([c[0], c[2]], dtype=np.float32), np.array([0.3, 0.6], dtype=np.float32), np.array([0.2, 0.9], dtype=np.float32)))
    assert s["j"].tolist() == [1, 3] and not s["cast"].any() and (s["wgeo"] == 0).all()
    rec, P, kinv, c, _ = _checked_table([flat, line, flat], mats, [0, 0, 0])
    assert (P == f32(1.0 / 3.0)).all() and (c == np.array([1.0 / 3.0, 1.0 / 3.0 + 1.0 / 3.0]).astype(np.float32)).all()


def test_a_thousand_emitters_of_very_unequal_area_and_selection_at_every_c():
    rng = np.random.default_rng(24)
    n = 1000
    scale = (10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
    v0 = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    verts = np.concatenate([v0, v0 + scale[:, None] * rng.uniform(-1, 1, (n, 3)).astype(np.float32), v0 + scale[:, None] * rng.uniform(-1, 1, (n, 3)).astype(np.float32)], axis=1)
    mats = np.zeros((3, 6), dtype=np.float32)
    mats[0, 3:], mats[1, 3:], mats[2, 3:] = (4, 4, 4), (0, 1e-3, 0), (50, 0, 7)
    rec, P, kinv, c, pair = _checked_table(verts, mats, rng.integers(0, 3, n).astype(np.uint16))
    assert pair.shape == (n, 2) and (pair[:, 1] == np.arange(n)).all() and P.max() / P.min() > 100 and (np.diff(c) > 0).all()
    u0 = np.concatenate([c, np.nextafter(c, f32(-1)), np.nextafter(c, f32(2)), [f32(0.0), f32(1.0), f32(0.5)], ND.u_of(np.array([0, 1, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF]))]).astype(np.float32)
    j = ET.select(c, u0)
    assert (j[:n - 1] == np.arange(1, n)).all() and (j[n - 1:2 * (n - 1)] == np.arange(n - 1)).all() and (j[2 * (n - 1):3 * (n - 1)] == np.arange(1, n)).all()
    assert j[3 * (n - 1):3 * (n - 1) + 2].tolist() == [0, n - 1] and j[-1] == n - 1 and j[-5] == 0 and j.max() == n - 1
    assert (j == _bisect(c, u0)).all()


def _bisect(c, u0):
    """The device's search (kernels.hip, emitter_select) restated: lo = 0, hi = n - 1; c[mid] <= u0 moves lo past mid."""
    out = []
    for u in np.asarray(u0, dtype=np.float32).tolist():
        lo, hi, steps = 0, len(c), 0
        while lo < hi:
            mid = (lo + hi) >> 1
            if c[mid] <= f32(u):
                lo = mid + 1
            else:
                hi = mid
            steps += 1
        assert steps <= 20
        out.append(lo)
    return np.array(out, dtype=np.uint32)


def test_selection_counts_and_bisection_agree_on_tied_and_tiny_tables():
    for c in ([], [0.5], [0.0, 0.0, 1.0 - 2.0 ** -24], [0.25, 0.25, 0.25, 0.75], [2.0 ** -30, 2.0 ** -29]):
        c = np.array(c, dtype=np.float32)
        u0 = np.concatenate([c, np.nextafter(c, f32(-1)), np.nextafter(c, f32(2)), [0.0, 1.0]]).astype(np.float32)
        assert (ET.select(c, u0) == _bisect(c, u0)).all() and ET.select(c, [1.0])[0] == c.size


def test_two_level_pairs_come_by_instance_then_by_prim(trx):
    """noise_domain's two-level scene: the twin's node walk finds, per TLAS primitive, exactly the triangle range the builder
    reports for its BLAS; the pairs are every instance crossed with its emissive triangles in the stated order; the records go
    through the instance's matrix in the header's association."""
    flat, by_range = ND.two_level(trx)
    prims = ET.instance_prims(flat.nodes, flat.instance_offsets, flat.tlas_start)
    for k, p in enumerate(prims):
        assert p.tolist() == sorted(by_range[by_range[:, 0] == k, 1].tolist()), k
    n_tris = flat.tri_verts.shape[0]
    mats = np.array([[0.5, 0.5, 0.5, 0, 0, 0], [0, 0, 0, 1, 2, 3]], dtype=np.float32)
    idx = (np.arange(n_tris) % 3 == 1).astype(np.uint16)
    pair = ET.pairs(ET.emissive(mats, idx), prims)
    want = [(k, p) for k, plist in enumerate(prims) for p in plist.tolist() if p % 3 == 1]
    assert pair.tolist() == [list(x) for x in want] and len(want) > 10
    assert (np.lexsort((pair[:, 1], pair[:, 0])) == np.arange(len(want))).all()
    rec, P, kinv, c, _ = _checked_table(flat.tri_verts, mats, idx, pair=pair, o2w=flat.instance_transforms)
    v = flat.tri_verts.reshape(-1, 3, 3).astype(np.float64)
    M = flat.instance_transforms.reshape(-1, 4, 4).transpose(0, 2, 1).astype(np.float64)      # M[k] @ (x, y, z, 1)
    for row, (k, p) in zip(rec, want):
        w = (M[k][:3, :3] @ v[p].T).T + M[k][:3, 3]
        for got, ref in ((row[0:3], w[0]), (row[4:7], w[1] - w[0]), (row[8:11], w[2] - w[0]), (row[12:15], np.cross(w[1] - w[0], w[2] - w[0]))):
            assert np.allclose(got, ref, rtol=1e-5, atol=1e-5), (k, p)
    assert rec.view(np.uint32)[:, 15].tolist() == [k for k, _ in want] and rec.view(np.uint32)[:, 11].tolist() == [p for _, p in want]


def test_every_sampled_point_lies_in_its_triangle():
    """u1, u2 at 0, 1.0 and everything between: y within the triangle's plane and bounds, to the rounding of its own arithmetic."""
    rng = np.random.default_rng(3)
    n = 64
    verts = rng.uniform(-2, 2, (n, 9)).astype(np.float32)
    mats = np.array([[0, 0, 0, 1, 1, 1]], dtype=np.float32)
    rec, P, kinv, c, _ = _checked_table(verts, mats, np.zeros(n, dtype=np.uint16))
    rec[:, 3] = kinv
    edge = ND.u_of(np.array([0, 1, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF])).astype(np.float32)
    u1 = np.concatenate([np.repeat(edge, edge.size), rng.random(4000).astype(np.float32)])
    u2 = np.concatenate([np.tile(edge, edge.size), rng.random(4000).astype(np.float32)])
    u0 = rng.random(u1.size).astype(np.float32)
    o = np.tile(np.array([[0.1, 0.2, 9.0]], dtype=np.float32), (u1.size, 1))
    s = ET.sample(rec, c, None, None, 0, 0.001, o, np.tile(np.array([[0, 0, -1.0]], dtype=np.float32), (u1.size, 1)), u=(u0, u1, u2))
    v = verts.reshape(-1, 3, 3).astype(np.float64)[s["j"]]
    y = s["y"].astype(np.float64)
    # barycentrics of y in float64: y = v0 + b1 (v1 - v0) + b2 (v2 - v0)
    e1, e2, r = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], y - v[:, 0]
    ng = np.cross(e1, e2)
    d11, d12, d22, r1, r2 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1), (r * e1).sum(1), (r * e2).sum(1)
    det = d11 * d22 - d12 * d12
    b1, b2 = (r1 * d22 - r2 * d12) / det, (r2 * d11 - r1 * d12) / det
    tol = 1e-5
    assert (b1 > -tol).all() and (b2 > -tol).all() and (b1 + b2 < 1 + tol).all()
    assert (np.abs((r * ng).sum(1)) / np.linalg.norm(ng, axis=1) < 1e-5).all()
    assert (y >= v.min(1) - 1e-5).all() and (y <= v.max(1) + 1e-5).all()
    at = np.flatnonzero(u1 == 0)
    assert at.size >= edge.size and (s["y"][at] == rec[s["j"][at], 0:3]).all()                  # (u1 == 0: the vertex V0 itself)
    assert s["cast"].any() and (s["tmax"][s["cast"]] >= 0).all()


def test_the_twins_noise_is_the_oracles(orc):
    px, py = np.array([0, 7, 19, 511, 1919]), np.array([0, 3, 11, 300, 1079])
    for seed in (0, 2048, 8192 + 63, 0xFFFFFFF0, ND.seed_for(19, 11, 0xFFFFFFFF), ND.seed_for(7, 3, 0)):
        for off in (0, 1024, 4096):
            assert (ET.hash_noise(px, py, seed + off) == LT.hash_noise(orc, px, py, seed + off)).all(), (seed, off)
    assert ET.hash_noise([19], [11], ND.seed_for(19, 11, 0xFFFFFFFF))[0] == f32(1.0) and ET.hash_noise([7], [3], ND.seed_for(7, 3, 0))[0] == f32(0.0)


# ---- the estimator's constant, on the oracle --------------------------------------------------------------------------------------

def test_the_pass_estimates_rule_5cs_emission_term(orc):
    """cornell_64 with its stand-in table on the oracle: the mean over the surface pixels of the emitter pass (twin, 16 samples)
    against the mean of rule 5c's emission term over 16 cosine-distributed bounce rays under a light of intensity 0.  Two
    estimators of one integral; a factor of pi or of 2 in kinv or in the area would show as a ratio of 3.14 or 2.  The bound is
    loose (25 %): the sharp one is the GPU test's, from the parent pass's own run-to-run difference."""
    osc, oview, w, h, g = golden_case(None, orc, "cornell_64")
    prim, inst, _ = osc.trace_primary_inst(oview, w, h, sem=0)
    recs = tri_records(g["tri_verts"])
    n_tris = recs.shape[0]
    v = g["tri_verts"].reshape(-1, 3, 3)
    mats = np.array([[0.8, 0.8, 0.8, 0, 0, 0], [0, 0, 0, 4, 3, 2]], dtype=np.float32)
    # the ceiling's central triangles emit (y at the top of the box, |x|, |z| small)
    top = v[:, :, 1].max()
    idx = ((v[:, :, 1] == top).all(1) & (np.abs(v[:, :, 0]).max(1) <= 0.5) & (np.abs(v[:, :, 2]).max(1) <= 0.5)).astype(np.uint16)
    assert 2 <= idx.sum() < n_tris // 4
    rec, c = ET.table(recs, ET.pairs(ET.emissive(mats, idx)), mats, idx)
    geometry = LT.frame_geometry(oview, w, h, prim, inst, recs)
    n = 16
    direct = ET.emitter_light(orc, osc, oview, w, h, geometry, prim, n_tris, rec, c, mats, 0, n, 0.01, 0.001, 0)
    dark = [LT.Light(LT.POINT, (0.0, 1.0, 0.0), intensity=0.0)]
    bounce = MT.indirect_rgb(orc, osc, oview, w, h, prim, inst, recs, None, dark, 0, n, 0.01, 0.01, 0, mats, idx)
    surf = LT.surface(prim, n_tris) & (idx[np.where(LT.surface(prim, n_tris), prim["prim"], 0)] == 0)    # (not the emitter's own pixels)
    for ch in range(3):
        a, b = float(direct[ch][surf].mean()), float(bounce[ch][surf].mean())
        print("plane %d: emitter pass %.5f, rule 5c's emission term %.5f, ratio %.4f" % (ch, a, b, a / b))
        assert b > 0 and abs(a / b - 1.0) < 0.25, (ch, a, b)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------

def test_emitter_kernel_resources():
    """The seven new kernels of build/kernels.s are streaming kernels: no scratch, no LDS, at most 128 VGPRs (the counts are
    printed)."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "tray_racing_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "build/kernels.s"], check=True, capture_output=True, timeout=900)
    text = open(os.path.join(csrc, "build", "kernels.s")).read()
    found = []
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n.*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        name, body = m.group(2), m.group(3)
        key = [k for k in NEW_KERNELS if re.search(r"\d%sE" % k, name) or re.search(r"\d%sI" % k, name)]
        if not key:
            continue
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        print("%s: %d VGPRs, %d B scratch, %d B LDS" % (name, vgprs, scratch, int(m.group(1))))
        assert scratch == 0 and vgprs <= 128 and int(m.group(1)) == 0, name
        found.append(key[0])
    assert sorted(found) == sorted(NEW_KERNELS + ("k_bounce_emitter_rays",))      # (dense and sparse)


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def test_cli_lists_and_checks_the_emitter_flags():
    cli = os.path.join(ROOT, "tray_racing_amd", "tray_racing_hip")

    def run(*args):
        return subprocess.run([cli] + list(args), capture_output=True, text=True, timeout=120)
    usage = run("--help")
    assert usage.returncode == 0 and "--emitters" in usage.stdout and "--emitter-eps" in usage.stdout
    base = ("-i", "standin:cornell", "--dry-run", "--passes", "1")
    pt = ("--light", "point:0,1.8,0")
    for extra, msg in ((("--png", "--emitters", "4"), "--colour"), (("--png", *pt, "--emitters", "4"), "--colour"), (("--colour", "--emitters", "4"), "--png"),
                       (("--png", "--colour", "--emitters", "0"), "--emitters"), (("--png", "--colour", "--emitters", "65"), "--emitters"),
                       (("--png", "--colour", "--emitters", "4", "--emitter-eps", "1"), "--emitter-eps"),
                       (("--png", "--colour", "--emitters", "4", "--emitter-eps", "-0.1"), "--emitter-eps"),
                       (("--png", "--colour", "--emitters", "4", "--emitter-eps", "nan"), "--emitter-eps"),
                       (("--png", *pt, "--colour", "--emitter-eps", "0.01"), "--emitters"),
                       (("--png", "--colour"), "--light"), (("--png", "--colour", "--bounce-samples", "4"), "--light")):
        r = run(*base, *extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert run(*base, "--png", "--colour", "--emitters", "4").returncode == 0
    assert run(*base, "--png", "--colour", "--emitters", "4", "--emitter-eps", "0.01", "--bounce-samples", "4", "--bounce-stride", "2", "--bounce-filter", "2",
               "--shadow-eps", "0.02", "--ambient", "0").returncode == 0
    assert run(*base, "--png", *pt, "--colour", "--emitters", "64", "--bounce-samples", "2", "--light-samples", "4").returncode == 0
