"""Texture coordinates and albedo textures without a GPU (include/trx.h, "texture coordinates and albedo textures"): the
boundary (symbols, plain C, ABI version), every refusal decided before a device is touched, the sRGB table against the twin
(tests/texture_twin.py), the stand-in tables against the twin, the twin's own properties under the oracle's hits on every
(scene, table) pair the GPU file uses, the addressing rule against exact arithmetic (Python fractions) on explicit records, and
the new kernels' resources, the OBJ / MTL loaders against the twin's readers and trx_load_model's bytes, and the command line's
--textures: its refusals, and its two image decoders on a --dry-run."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import texture_cases as TC
import texture_twin as TT
from hit_attr_twin import hit_attrs, primary_dirs, primary_origins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW_SYMBOLS = ("trx_scene_set_texcoords", "trx_scene_get_texcoords", "trx_scene_set_textures", "trx_scene_get_textures",
               "trx_scene_remove_textures", "trx_texture_srgb_table", "trx_surface_albedo_dev", "trx_albedo_compose_dev",
               "trx_trace_indirect_rgb_textured_dev", "trx_render_image_colour_textured", "trx_standin_texcoords", "trx_standin_textures",
               "trx_load_model_texcoords", "trx_load_model_material_maps")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "tray_racing_amd", "tray_racing_hip")


# ---- the boundary ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_bound(trx):
    from tray_racing_amd import _lib
    header = open(os.path.join(ROOT, "include", "trx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    lib = trx.load()
    for name in NEW_SYMBOLS:
        assert (" T %s\n" % name) in out and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert name + "(" in header
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [3, 3, 7, 7, 1, 1, 6, 8, 21, 31, 4, 7, 7, 3]
    for name in ("set_texcoords", "get_texcoords", "set_textures", "get_textures", "surface_albedo_dev", "albedo_compose_dev",
                 "trace_indirect_rgb_textured_dev", "render_image_colour_textured"):
        assert callable(getattr(trx.Scene, name)), name
    assert callable(trx.load_model_texcoords) and callable(trx.load_model_material_maps)
    assert callable(trx.standin_texcoords) and callable(trx.standin_textures) and trx.TEXTURE_DESC_DTYPE.itemsize == 16
    assert "THE TEXTURED ALBEDO" in header and trx.NO_TEXTURE == 0xFFFFFFFF
    # the header stays plain C11, and a caller can pass the new arguments
    src = (b'#include "trx.h"\n'
           b'_Static_assert(sizeof(trx_texture_desc) == 16, "16 B");\n'
           b'int f(trx_scene *s, const trx_view *v, const trx_light *l, const trx_hit *p, const trx_hit_attr *a, float *out, unsigned char *img) {\n'
           b'    trx_shard whole = {0, 1, TRX_LAYOUT_IMAGE, 0};\n'
           b'    trx_texture_desc d = {TRX_MAX_TEXTURE_SIZE, 1, TRX_TEX_RGBA8_SRGB, TRX_TEX_BILINEAR};\n'
           b'    uint32_t texel[1] = {0}, mt[1] = {TRX_NO_TEXTURE}, n = TRX_MAX_TEXTURES, nm = 1;\n'
           b'    uint64_t nt = 1;\n'
           b'    float table[256];\n'
           b'    trx_texture_srgb_table(table);\n'
           b'    int rc = trx_scene_set_texcoords(s, out, 1) | trx_scene_get_texcoords(s, out, 1) | trx_scene_remove_textures(s);\n'
           b'    rc |= trx_scene_set_textures(s, &d, 1, texel, 1, mt, 1) | trx_scene_get_textures(s, &d, &n, texel, &nt, mt, &nm);\n'
           b'    rc |= trx_surface_albedo_dev(s, p, a, 64, out, 0) | trx_albedo_compose_dev(s, p, out, out, out, 64, out, 0);\n'
           b'    rc |= trx_trace_indirect_rgb_textured_dev(s, v, 8, 8, whole, 2, 3, 0, 0, l, 1, 0, 4, 0.01f, 0.01f, 1, 0.001f, p, 0, out, 0);\n'
           b'    return rc | trx_render_image_colour_textured(s, v, 8, 8, 0, 0, l, 1, 0, 1, 0.01f, 0.1f, 0, 0.01f, 1.0f, 0, 0.02f, 0.9f, 4, 0.01f, 3,\n'
           b'                                                 0.1f, 0.9f, 2, 0, 1, 2, 0.001f, 1, img, 0);\n}\n'
           b'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", "-I",
                    os.path.join(ROOT, "include"), "-"], input=src, check=True)
    assert lib.trx_abi_version() == 1   # additions only


def test_bad_arguments_are_refused_before_any_device_work(trx):
    """(a scene pointer that is never dereferenced: every call below is refused on the arguments that come first; the refusals
    that need the scene - no materials, another n_materials, another n_tris - are in tests/test_gpu_textures.py)"""
    from tray_racing_amd import _lib
    lib = trx.load()
    buf = np.zeros(64, dtype=np.uint32)
    P = buf.ctypes.data_as(C.c_void_p)
    inv = _lib.TRX_ERR_INVALID
    n32, n64, m32 = C.c_uint32(4), C.c_uint64(4), C.c_uint32(4)
    assert lib.trx_scene_set_texcoords(None, P, 1) == inv and lib.trx_scene_get_texcoords(None, P, 1) == inv
    assert lib.trx_scene_get_texcoords(P, None, 1) == inv and lib.trx_scene_remove_textures(None) == inv
    lib.trx_texture_srgb_table(None)                                    # (nothing to fill: no fault)

    def descs(*rows):
        return np.array(rows, dtype=np.uint32).reshape(-1, 4)

    def set_textures(scene=P, d=descs((2, 2, 0, 0)), n_tex=None, texels=P, n_texels=4, mt=np.array([0], dtype=np.uint32), n_mat=None):
        return lib.trx_scene_set_textures(scene, None if d is None else d.ctypes.data_as(C.c_void_p), d.shape[0] if n_tex is None and d is not None else n_tex or 0,
                                          texels, n_texels, None if mt is None else mt.ctypes.data_as(C.c_void_p), (mt.size if mt is not None else 1) if n_mat is None else n_mat)

    one = descs((2, 2, 0, 0))
    for kw, msg in (({"scene": None}, b"null"), ({"d": None, "n_tex": 1}, b"null"), ({"texels": None}, b"null"), ({"mt": None}, b"null"),
                    ({"n_tex": 0}, b"n_textures"), ({"n_tex": 65536}, b"n_textures"),
                    ({"d": descs((0, 2, 0, 0)), "n_texels": 0}, b"outside 1.."), ({"d": descs((2, 0, 0, 0)), "n_texels": 0}, b"outside 1.."),
                    ({"d": descs((8193, 1, 0, 0)), "n_texels": 8193}, b"outside 1.."), ({"d": descs((1, 8193, 0, 0)), "n_texels": 8193}, b"outside 1.."),
                    ({"d": descs((2, 2, 2, 0))}, b"format"), ({"d": descs((2, 2, 0, 2))}, b"filter"), ({"d": descs((2, 2, 0xFFFFFFFF, 0))}, b"format"),
                    ({"n_texels": 3}, b"n_texels"), ({"n_texels": 5}, b"n_texels"), ({"d": descs((2, 2, 0, 0), (3, 1, 1, 1)), "n_texels": 4}, b"n_texels"),
                    ({"d": np.tile(descs((8192, 8192, 0, 0)), (32, 1)), "n_texels": 2 ** 31}, b"2^31"),
                    ({"mt": np.array([1], dtype=np.uint32)}, b"texture index"), ({"mt": np.array([0, 0xFFFFFFFE], dtype=np.uint32)}, b"texture index")):
        assert set_textures(**kw) == inv and msg in lib.trx_last_error(), (kw, lib.trx_last_error())
    assert one.shape == (1, 4)
    for args in ((None, P, C.byref(n32), P, C.byref(n64), P, C.byref(m32)), (P, None, C.byref(n32), P, C.byref(n64), P, C.byref(m32)),
                 (P, P, None, P, C.byref(n64), P, C.byref(m32)), (P, P, C.byref(n32), None, C.byref(n64), P, C.byref(m32)),
                 (P, P, C.byref(n32), P, None, P, C.byref(m32)), (P, P, C.byref(n32), P, C.byref(n64), None, C.byref(m32)),
                 (P, P, C.byref(n32), P, C.byref(n64), P, None)):
        assert lib.trx_scene_get_textures(*args) == inv
    for args in ((None, P, P, 16, P), (P, None, P, 16, P), (P, P, None, 16, P), (P, P, P, 16, None), (P, P, P, 0, P), (P, P, P, 2 ** 31, P)):
        assert lib.trx_surface_albedo_dev(*args, None) == inv, args
    for args in ((None, P, P, P, P, 16, P), (P, None, P, P, P, 16, P), (P, P, None, P, P, 16, P), (P, P, P, None, P, 16, P), (P, P, P, P, P, 16, None),
                 (P, P, P, P, P, 0, P), (P, P, P, P, P, 2 ** 31, P)):
        assert lib.trx_albedo_compose_dev(*args, None) == inv, args
    view = _lib.View()
    good = trx.light_array([trx.light(trx.LIGHT_POINT, (0, 1, 0))])
    whole = _lib.Shard(0, 1, 0, 0)

    def indirect(scene=None, shard=whole, stride=1, phase=0, use=0, out=P):
        return lib.trx_trace_indirect_rgb_textured_dev(scene, C.byref(view), 4, 4, shard, stride, phase, 0, 0, good, 1, 0, 4, 0.01, 0.01, use, 0.001, P, None,
                                                       out, None)

    for kw, msg in (({}, b"null"), ({"scene": P, "out": None}, b"null"), ({"scene": P, "use": 2}, b"use_emitters"), ({"scene": P, "stride": 0}, b"stride"),
                    ({"scene": P, "stride": 5}, b"stride"), ({"scene": P, "stride": 2, "phase": 4}, b"phase"), ({"scene": P, "phase": 1}, b"phase"),
                    ({"scene": P, "stride": 2, "shard": _lib.Shard(1, 3, 0, 0)}, b"whole image"), ({"scene": P, "stride": 2, "shard": _lib.Shard(0, 1, 1, 0)}, b"whole image")):
        assert indirect(**kw) == inv and msg in lib.trx_last_error(), (kw, lib.trx_last_error())

    def render(scene=None, smooth=0, es=0, n_lights=1, bn=0):
        return lib.trx_render_image_colour_textured(scene, C.byref(view), 4, 4, 0, 0, good, n_lights, 0, 1, 0.01, 0.1, 0, 0.01, 1.0, 0, 0.02, 0.9, bn, 0.01, 0, 0.1,
                                                    0.9, 1, 0, 1, es, 0.001, smooth, P, None)

    for kw, msg in (({}, b"null"), ({"scene": P, "smooth": 2}, b"smooth"), ({"scene": P, "n_lights": 0}, b"n_lights"), ({"scene": P, "es": 65}, b"emitter_samples"),
                    ({"scene": P, "bn": 65}, b"bounce_samples")):
        assert render(**kw) == inv and msg in lib.trx_last_error(), (kw, lib.trx_last_error())


# ---- the sRGB table and the stand-ins ------------------------------------------------------------------------------------------

def test_srgb_table_equals_the_twin_entry_by_entry(trx):
    got, want = trx.texture_srgb_table(), TT.srgb_table()
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert got[0] == 0.0 and got[255] == 1.0 and (np.diff(got) > 0).all()
    # the two branches meet between codes 10 and 11 (10 / 255 = 0.0392 <= 0.04045 < 11 / 255)
    assert got[10] == f32(10 / 255.0 / 12.92) and got[11] == f32(math.pow((11 / 255.0 + 0.055) / 1.055, 2.4))


@pytest.mark.parametrize("name,n_tris", [("cornell", 0), ("soup", 333), ("kitchen", 5000)])
def test_standin_tables_equal_the_twin(trx, name, n_tris):
    verts, counts = trx.gen_scene(name, n_tris, 1)
    got, want = trx.standin_texcoords(name, verts), TT.standin_texcoords(verts)
    assert got.shape == (verts.shape[0], 6) and (got.view(np.uint32) == want.view(np.uint32)).all()
    v = verts.reshape(-1, 3, 3)
    for c in range(3):                                         # every (s, t) is two of the corner's own coordinates, in axis order
        pairs = [(got[:, 2 * c] == v[:, c, a]) & (got[:, 2 * c + 1] == v[:, c, b]) for a, b in ((1, 2), (0, 2), (0, 1))]
        assert (pairs[0] | pairs[1] | pairs[2]).all()
    descs, texels, mt = trx.standin_textures(name, 6)
    ts = TT.standin_textures(6)
    assert TT.texset(descs, texels, mt).descs.tobytes() == ts.descs.tobytes() and (texels == ts.texels).all() and (mt == ts.material_texture).all()
    assert mt[0] == 0 and (mt[1:] == trx.NO_TEXTURE).all() and set(np.unique(texels).tolist()) == {0xFF808080, 0xFFFFFFFF}
    assert texels[0] == 0xFF808080 and texels[8] == 0xFFFFFFFF and texels[8 * 64] == 0xFFFFFFFF and texels[8 * 64 + 8] == 0xFF808080


def test_standin_texcoords_ties_and_degenerates(trx):
    """Ties go to the lower axis; a NaN component loses to any number; a degenerate triangle (all components zero) takes axis x."""
    tris = np.array([[0, 0, 0, 1, 1, 0, 0, 1, 1],        # n = (1, -1, 1): a three-way tie -> axis x: (y, z)
                     [0, 0, 0, 0, 1, 0, 1, 1, 1],        # n = (1, 0, -1): x and z tie -> axis x
                     [0, 0, 0, 1, 0, 0, 1, 0, 1],        # n = (0, -1, 0): axis y: (x, z)
                     [0, 0, 0, 1, 0, 0, 0, 1, 0],        # n = (0, 0, 1): axis z: (x, y)
                     [1, 2, 3, 1, 2, 3, 1, 2, 3],        # degenerate: axis x
                     [0, 0, 0, np.inf, 0, 0, 0, 1, 0]],  # n = (0, NaN, inf): axis z
                    dtype=np.float32)
    got = trx.standin_texcoords("any", tris)
    assert (got.view(np.uint32) == TT.standin_texcoords(tris).view(np.uint32)).all()
    assert got[0].tolist() == [0, 0, 1, 0, 1, 1] and got[1].tolist() == [0, 0, 1, 0, 1, 1] and got[2].tolist() == [0, 0, 1, 0, 1, 1]
    assert got[3].tolist() == [0, 0, 1, 0, 0, 1] and got[4].tolist() == [2, 3, 2, 3, 2, 3] and got[5].tolist() == [0, 0, np.inf, 0, 0, 1]


def test_standin_refusals(trx):
    from tray_racing_amd import _lib
    lib = trx.load()
    v = np.zeros((2, 9), dtype=np.float32)
    out = np.zeros((2, 6), dtype=np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)    # noqa: E731
    assert lib.trx_standin_texcoords(None, P(v), 2, P(out)) == _lib.TRX_ERR_INVALID
    assert lib.trx_standin_texcoords(b"x", None, 2, P(out)) == _lib.TRX_ERR_INVALID and lib.trx_standin_texcoords(b"x", P(v), 2, None) == _lib.TRX_ERR_INVALID
    assert lib.trx_standin_texcoords(b"x", None, 0, None) == 0
    dp, tp, mp, n, nt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint64()
    ok = (b"x", 3, C.byref(dp), C.byref(n), C.byref(tp), C.byref(nt), C.byref(mp))
    for k in (0, 2, 3, 4, 5, 6):
        args = list(ok)
        args[k] = None
        assert lib.trx_standin_textures(*args) == _lib.TRX_ERR_INVALID, k
    assert lib.trx_standin_textures(b"x", 0, *ok[2:]) == _lib.TRX_ERR_INVALID
    assert dp.value is None and tp.value is None and mp.value is None


# ---- the twin's own properties on the scenes and tables the GPU file uses ---------------------------------------------------------

def _oracle_frame(trx, orc, name):
    """(records [n, 12], the oracle's primary hits, their attribute records) of a golden scene."""
    from tray_racing_amd import _lib
    g, recs, f16 = TC.golden(name)
    w, h = int(g["width"]), int(g["height"])
    prim = g["orc_f16_primary_sem0" if f16 is not None else "orc_primary_sem0"]
    view = _lib.View()
    C.memmove(C.byref(view), g["view"].tobytes(), C.sizeof(view))
    px, py = np.arange(w * h) % w, np.arange(w * h) // w
    attr = hit_attrs(recs, primary_origins(view, w * h), primary_dirs(view, w, h, px, py), prim["prim"], None, None)
    return recs, prim, attr


@pytest.mark.parametrize("name", TC.SCENES)
def test_twin_properties_on_the_scenes_the_gpu_tests_use(trx, orc, name):
    """Under every table: textured and fallback records both exist, every fallback cause occurs over the tables, a fallback
    record holds the material's albedo bit for bit, a background record +0, a textured one albedo * val with val in [0, 1]."""
    recs, prim, attr = _oracle_frame(trx, orc, name)
    n_tris = recs.shape[0]
    mat, idx = TC.materials(n_tris)
    plain, why = TT.surface_albedo(prim, attr, mat, idx, n_tris)
    assert set(why.tolist()) <= {TT.BACKGROUND, TT.NO_TABLES}
    seen = set()
    for kind in TC.TABLES:
        uvs, ts = TC.tables(kind, recs)
        got, cause = TT.surface_albedo(prim, attr, mat, idx, n_tris, uvs, ts)
        seen |= set(cause.tolist())
        textured = cause == TT.TEXTURED
        assert textured.sum() > 30 and (~textured & (cause != TT.BACKGROUND)).sum() > 30, (name, kind, np.bincount(cause))
        assert (got[:, ~textured].view(np.uint32) == plain[:, ~textured].view(np.uint32)).all()
        assert not got[:, cause == TT.BACKGROUND].any()
        assert (got[:, textured] >= 0).all() and (got[:, textured] <= plain[:, textured]).all()
        assert (got[:, textured] != plain[:, textured]).any()
        for only in ((uvs, None), (None, ts)):                     # either table alone changes nothing
            alone, c2 = TT.surface_albedo(prim, attr, mat, idx, n_tris, *only)
            assert (alone.view(np.uint32) == plain.view(np.uint32)).all() and set(c2.tolist()) <= {TT.BACKGROUND, TT.NO_TABLES}
    assert {TT.TEXTURED, TT.NO_TEXTURE_FOR_MATERIAL, TT.NOT_FINITE} <= seen, (name, seen)
    if (why == TT.BACKGROUND).any():
        assert TT.BACKGROUND in seen
    for filt in (TT.NEAREST, TT.BILINEAR):                         # all-255 textures: the plain albedo, bit for bit
        for fmt in (TT.UNORM, TT.SRGB):
            white, _ = TT.surface_albedo(prim, attr, mat, idx, n_tris, TC.tables("random", recs)[0], TT.white_textures(TC.N_MATERIALS, filt, fmt))
            assert (white.view(np.uint32) == plain.view(np.uint32)).all()


# ---- the addressing rule against exact arithmetic ------------------------------------------------------------------------------

def _exact_address(s, W):
    """(nearest index, ix0, ix1, fx) of a finite float32 s by the header's rule, every float operation done as: exact value in
    fractions, then rounded to float32."""
    def rnd(q):
        return Fraction(float(f32(float(q)))) if abs(q) >= Fraction(1, 2 ** 200) or q == 0 else Fraction(0)   # (float(q): correctly rounded to binary64, then to binary32; no double rounding at these magnitudes)
    sf = Fraction(float(s))
    fs = rnd(sf - math.floor(sf))
    if fs >= 1:
        fs = Fraction(0)
    p = rnd(fs * W)
    near = min(int(p), W - 1)
    x = rnd(p - Fraction(1, 2))
    x0 = math.floor(x)
    fx = rnd(x - x0)
    ix0, ix1 = (W - 1 if x0 == -1 else x0), (0 if x0 + 1 == W else x0 + 1)
    return near, ix0, ix1, fx


@pytest.mark.parametrize("W,H", [(1, 1), (2, 1), (3, 5), (64, 64)])
def test_tap_addresses_lie_inside_and_equal_exact_arithmetic(W, H):
    """Explicit coordinates: exactly 0, 1, -0.0, -1e-9 (fs rounds to 1: the fs >= 1 case), 0.5 / W, 1 - 0.5 / W, 1e30, -1e30, a
    denormal, and their neighbours; NaN and the infinities are not addressed at all (the rule's fallback, below)."""
    values = [0.0, 1.0, -0.0, -1e-9, 0.5 / W, 1 - 0.5 / W, 0.5 / H, 1 - 0.5 / H, 1e30, -1e30, 1e-42, -1e-42, 0.25, 0.75, 2.5, -2.5, 0.999999, 1 - 2 ** -24,
              -(2 ** -25), 1 / 3.0, 2 / 3.0, 7.0 + 1 / 64.0]
    s = np.array(values, dtype=np.float32)
    s = np.unique(np.concatenate([s, np.nextafter(s, f32(np.inf)), np.nextafter(s, f32(-np.inf))]))
    assert (TT.wrap(np.array([-1e-9], dtype=np.float32)) == 0).all() and f32(-1e-9) - np.floor(f32(-1e-9)) == f32(1.0)
    for size in (W, H):
        dim = np.full(s.size, size, dtype=np.uint32)
        fs = TT.wrap(s)
        assert (fs >= 0).all() and (fs < 1).all()
        near = TT.nearest_index(fs, dim)
        ix0, ix1, fx = TT.bilinear_index(fs, dim)
        for arr in (near, ix0, ix1):
            assert (arr >= 0).all() and (arr < size).all()
        assert (fx >= 0).all() and (fx <= 1).all()          # (exactly 1 where x is a tiny negative number: x - (-1) rounds up)
        for k in range(s.size):
            want = _exact_address(s[k], size)
            assert (int(near[k]), int(ix0[k]), int(ix1[k])) == want[:3] and Fraction(float(fx[k])) == want[3], (size, float(s[k]), want)
    # the sampler reads inside its texture for every pair of these coordinates (its own assertion), in all formats and filters
    ss, tt = np.meshgrid(s, s)
    for fmt in (TT.UNORM, TT.SRGB):
        for filt in (TT.NEAREST, TT.BILINEAR):
            ts = TT.texset([[7, 3, 0, 0], [W, H, fmt, filt]], np.arange(21 + W * H, dtype=np.uint32) * np.uint32(2654435761), [1])
            val = TT.sample(ss.reshape(-1), tt.reshape(-1), np.ones(ss.size, dtype=np.int64), ts)
            assert np.isfinite(val).all() and (val >= 0).all() and (val <= 1).all()


def test_records_that_are_not_finite_fall_back(trx):
    """NaN and both infinities, in the table or in u, v: the material's albedo, nothing sampled."""
    mat = np.array([[0.25, 0.5, 0.75, 0, 0, 0]], dtype=np.float32)
    idx = np.zeros(4, dtype=np.uint16)
    ts = TT.texset([[3, 5, TT.SRGB, TT.BILINEAR]], np.arange(15, dtype=np.uint32) * np.uint32(0x01010101), [0])
    uvs = np.array([[0.1, 0.2, 0.3, 0.4, 0.5, 0.6], [np.nan, 0, 0, 0, 0, 0], [0, 0, 0, np.inf, 0, 0], [0, 0, 0, 0, 0, -np.inf]], dtype=np.float32)
    hits = np.zeros(8, dtype=np.dtype([("t", "<f4"), ("prim", "<u4")]))
    hits["t"], hits["prim"] = 1.0, [0, 1, 2, 3, 0, 0, 0, 0]
    attr = np.zeros(8, dtype=[("u", "<f4"), ("v", "<f4"), ("normal", "<f4", 3), ("_pad", "<u4")])
    attr["u"], attr["v"] = 0.25, 0.5
    attr["u"][4], attr["v"][5], attr["u"][6] = np.nan, np.inf, -np.inf
    got, cause = TT.surface_albedo(hits, attr, mat, idx, 4, uvs, ts)
    assert cause.tolist() == [TT.TEXTURED, TT.NOT_FINITE, TT.NOT_FINITE, TT.NOT_FINITE, TT.NOT_FINITE, TT.NOT_FINITE, TT.NOT_FINITE, TT.TEXTURED]
    assert (got[:, 1:7] == mat[0, :3, None]).all() and (got[:, 0] < mat[0, :3]).all()
    # the interpolation is the header's association, by hand for record 0: w = (1 - u) - v = 0.25
    w = f32(f32(1.0) - f32(0.25)) - f32(0.5)
    s = f32(f32(f32(w * f32(0.1)) + f32(f32(0.25) * f32(0.3))) + f32(f32(0.5) * f32(0.5)))
    assert TT.interpolate(attr["u"][:1], attr["v"][:1], uvs[:1])[0][0] == s


# ---- where UVs and textures come from: the loaders and the command line -------------------------------------------------------------

def test_texcoord_loader_gives_load_models_mesh_and_the_twins_table(trx, tmp_path):
    path = os.path.join(GOLDEN, "quad_tex.obj")
    verts, counts, uvs, has = trx.load_model_texcoords(path)
    plain_v, plain_c = trx.load_meshs(path)
    assert verts.tobytes() == plain_v.tobytes() and (counts == plain_c).all() and has is True
    want, any_vt = TT.load_obj_texcoords(path)
    assert any_vt and uvs.shape == (4, 6) and (uvs.view(np.uint32) == want.view(np.uint32)).all()
    # by hand: the quad split 0,1,2 / 0,2,3; negative, positive and absent indices; indices outside the five `vt` read
    assert uvs.tolist() == [[0, 0, 2, 0, 2, 2], [0, 0, 2, 2, 0, 2], [0.25, 0.75, 2, 0, 0, 0], [0, 0, 0, 0, 0, 0]]
    assert not np.signbit(uvs).any()
    # an OBJ without any `vt`, a `vt` with one number, and a JSON model
    bare = tmp_path / "bare.obj"
    bare.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0.5\nf 1 2 3\nf 1/1 2//1 3/\n")
    v, c, uv, has = trx.load_model_texcoords(str(bare))
    want, any_vt = TT.load_obj_texcoords(str(bare))
    assert (uv.view(np.uint32) == want.view(np.uint32)).all() and has == any_vt
    assert uv.tolist() == [[0] * 6, [0.5, 0, 0, 0, 0, 0]] and has is True and v.tobytes() == trx.load_meshs(str(bare))[0].tobytes()
    none = tmp_path / "none.obj"
    none.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    assert trx.load_model_texcoords(str(none))[3] is False and not trx.load_model_texcoords(str(none))[2].any()
    js = tmp_path / "m.json"
    js.write_text('[{"v0":[0,0,0], "v1":[1,0,0], "v2":[0,1,0]}]')
    v, c, uv, has = trx.load_model_texcoords(str(js))
    assert uv.shape == (1, 6) and not uv.any() and has is False and v.tobytes() == trx.load_meshs(str(js))[0].tobytes()
    assert trx.load_model_material_maps(str(js)) == [""]


def test_material_maps_on_the_fixture_and_loader_refusals(trx, tmp_path):
    from tray_racing_amd import _lib
    path = os.path.join(GOLDEN, "quad_tex.obj")
    maps = trx.load_model_material_maps(path)
    assert maps == ["", "checker_4x3.ppm", ""] == TT.load_obj_material_maps(path)         # (options before the name are skipped)
    assert len(maps) == trx.load_model_materials(path)[2].shape[0]
    obj = tmp_path / "two.obj"
    obj.write_text("mtllib a.mtl\nmtllib missing.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl b\nf 1 2 3\n")
    (tmp_path / "a.mtl").write_text("map_Kd before_any_newmtl.png\nnewmtl a\n\tmap_Kd first.png\nmap_Kd -bm 0.5 dir/second.PNG\nnewmtl b\nnewmtl c\nmap_Kd\tc.ppm\n")
    assert trx.load_model_material_maps(str(obj)) == ["", "dir/second.PNG", "", "c.ppm"] == TT.load_obj_material_maps(str(obj))
    lib = trx.load()
    p, n = C.c_void_p(), C.c_uint32()
    vp, cp, up = C.POINTER(C.c_float)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_float)()
    nt, no, has = C.c_uint64(), C.c_uint32(), C.c_uint32()
    assert lib.trx_load_model_material_maps(None, C.byref(p), C.byref(n)) == _lib.TRX_ERR_INVALID
    assert lib.trx_load_model_material_maps(path.encode(), None, C.byref(n)) == _lib.TRX_ERR_INVALID
    assert lib.trx_load_model_material_maps(path.encode(), C.byref(p), None) == _lib.TRX_ERR_INVALID
    assert lib.trx_load_model_material_maps(str(tmp_path / "nothing.obj").encode(), C.byref(p), C.byref(n)) == _lib.TRX_ERR_IO
    assert lib.trx_load_model_texcoords(None, C.byref(vp), C.byref(nt), C.byref(cp), C.byref(no), C.byref(up), C.byref(has)) == _lib.TRX_ERR_INVALID
    assert lib.trx_load_model_texcoords(path.encode(), C.byref(vp), C.byref(nt), C.byref(cp), C.byref(no), None, C.byref(has)) == _lib.TRX_ERR_INVALID
    assert lib.trx_load_model_texcoords(path.encode(), C.byref(vp), C.byref(nt), C.byref(cp), C.byref(no), C.byref(up), None) == _lib.TRX_ERR_INVALID
    assert lib.trx_load_model_texcoords(str(tmp_path / "nothing.obj").encode(), C.byref(vp), C.byref(nt), C.byref(cp), C.byref(no), C.byref(up),
                                        C.byref(has)) == _lib.TRX_ERR_IO
    assert p.value is None and not up


def test_cli_lists_and_checks_the_textures_flag(tmp_path):
    def run(*args, inp="standin:cornell"):
        return subprocess.run([CLI, "-i", inp, "--dry-run", "--passes", "1"] + list(args), capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert "--textures" in subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    light = ["--light", "point:0,1.8,0"]
    for extra, msg in ((["--png", "--textures"] + light, "--colour"), (["--textures"], "--colour"),
                       (["--png", "--colour", "--textures", "--benchmark"] + light, "--benchmark"),
                       (["--png", "--colour", "--textures", "--profile-rt", "tris"] + light, "--profile-rt")):
        r = run(*extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    for extra in ([], ["--emitters", "2"], ["--smooth"]):
        r = run("--png", "--colour", "--textures", *light, *extra)
        assert r.returncode == 0, (extra, r.stderr)
    # the decoders on a dry run: the fixture's PPM and both PNGs are read without a word; anything else gives a message and the
    # material stays untextured
    import shutil as sh
    for name in ("quad_tex.obj", "checker_4x3.ppm", "checker_4x3.png", "checker_4x3_rgba.png"):
        sh.copy(os.path.join(GOLDEN, name), str(tmp_path / name))
    (tmp_path / "truncated.png").write_bytes(open(os.path.join(GOLDEN, "checker_4x3.png"), "rb").read()[:60])
    (tmp_path / "ascii.ppm").write_text("P3\n1 1\n255\n1 2 3\n")
    (tmp_path / "deep.ppm").write_bytes(b"P6\n1 1\n65535\n" + bytes(6))
    for image, bad in (("checker_4x3.ppm", False), ("checker_4x3.png", False), ("checker_4x3_rgba.png", False), ("truncated.png", True), ("ascii.ppm", True),
                       ("deep.ppm", True), ("absent.png", True)):
        (tmp_path / "quad_tex.mtl").write_text("newmtl tex\nmap_Kd %s\nnewmtl plain\nKd 0.2 0.4 0.8\n" % image)
        r = run("--png", "--colour", "--textures", *light, inp=str(tmp_path / "quad_tex.obj"))
        assert r.returncode == 0, r.stderr
        assert (("stays untextured" in r.stderr) and (image in r.stderr)) == bad, (image, r.stderr)


# ---- the new kernels' resources ---------------------------------------------------------------------------------------------------

def test_texture_kernel_resources():
    """k_surface_albedo and k_albedo_compose (make build/image.s), k_bounce_gather_tex<false | true> (build/kernels.s): no
    scratch, no LDS, at most 128 VGPRs - the bound of the other post-walk kernels (the counts are printed)."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "tray_racing_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "build/kernels.s", "build/image.s"], check=True, capture_output=True, timeout=900)

    def resources(path, wanted):
        text = open(os.path.join(csrc, "build", path)).read()
        found = []
        for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n.*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
            name, body = m.group(2), m.group(3)
            key = [k for k in wanted if k in name]
            if not key:
                continue
            vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
            print("%s: %d VGPRs, %d B scratch, %d B LDS" % (name, vgprs, scratch, int(m.group(1))))
            assert scratch == 0 and vgprs <= 128 and int(m.group(1)) == 0, name
            found.append(key[0])
        return sorted(found)

    assert resources("kernels.s", ("k_bounce_gather_tex",)) == ["k_bounce_gather_tex"] * 2
    assert resources("image.s", ("k_surface_albedo", "k_albedo_compose")) == ["k_albedo_compose", "k_surface_albedo"]
