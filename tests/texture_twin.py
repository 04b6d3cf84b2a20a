"""The twin of the textured albedo (include/trx.h, "texture coordinates and albedo textures"): THE TEXTURED ALBEDO restated in
numpy float32 - interpolation, repeat wrap, nearest and bilinear addressing, texel decode, the albedo - with the sRGB table
entry by entry through math.pow, the albedo compose, the textured gathers of rules 5c and 5e, the stand-in tables, and small
readers of an OBJ's `vt`, a mtl's `map_Kd` and a binary PPM.  It calls nothing of the library.

Records are numpy arrays in any order; planes are rows of a [3, n] array (0 = R, 1 = G, 2 = B).  A material table is a [n, 6]
float32 array (albedo r, g, b, emission r, g, b).  A texture set is a TexSet: descs [n, 4] uint32 (width, height, format,
filter), texels uint32 (R in the low byte), material_texture [n_materials] uint32."""
import math
from collections import namedtuple

import numpy as np

f32 = np.float32
INVALID = 0xFFFFFFFF
NO_TEXTURE = 0xFFFFFFFF
F32_MAX = f32(3.402823466e+38)
UNORM, SRGB = 0, 1
NEAREST, BILINEAR = 0, 1
# why a record got the value it got (surface_albedo's second result)
BACKGROUND, TEXTURED, NO_TABLES, NO_TEXTURE_FOR_MATERIAL, NOT_FINITE = 0, 1, 2, 3, 4

TexSet = namedtuple("TexSet", "descs texels material_texture")


def texset(descs, texels, material_texture):
    d = np.asarray(descs)
    if d.dtype.names:
        d = np.stack([d["width"], d["height"], d["format"], d["filter"]], axis=1)
    return TexSet(np.ascontiguousarray(d, dtype=np.uint32).reshape(-1, 4), np.ascontiguousarray(texels, dtype=np.uint32).reshape(-1),
                  np.ascontiguousarray(material_texture, dtype=np.uint32).reshape(-1))


def srgb_table():
    """[256] float32: c / 255 / 12.92 up to 0.04045, pow((c / 255 + 0.055) / 1.055, 2.4) above, in binary64, rounded once."""
    out = np.zeros(256, dtype=np.float32)
    for c in range(256):
        x = c / 255.0
        out[c] = f32(x / 12.92 if x <= 0.04045 else math.pow((x + 0.055) / 1.055, 2.4))
    return out


def surface(hits, n_tris):
    prim = np.asarray(hits["prim"], dtype=np.uint64)
    return (np.asarray(hits["t"], dtype=np.float32) < F32_MAX) & (prim != INVALID) & (prim < n_tris)


def interpolate(u, v, uv6):
    """(s, t) float32: w = (1 - u) - v, s = (w * s0 + u * s1) + v * s2, t likewise; uv6 is [n, 6] (s0, t0, s1, t1, s2, t2)."""
    u, v, uv6 = np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32), np.asarray(uv6, dtype=np.float32).reshape(-1, 6)
    with np.errstate(invalid="ignore", over="ignore"):
        w = ((f32(1.0) - u).astype(np.float32) - v).astype(np.float32)
        out = []
        for k in (0, 1):
            a = ((w * uv6[:, k]).astype(np.float32) + (u * uv6[:, 2 + k]).astype(np.float32)).astype(np.float32)
            out.append((a + (v * uv6[:, 4 + k]).astype(np.float32)).astype(np.float32))
    return out[0], out[1]


def wrap(s):
    """fs = s - floorf(s), 0 where that is >= 1 (finite s only)."""
    s = np.asarray(s, dtype=np.float32)
    fs = (s - np.floor(s)).astype(np.float32)
    return np.where(fs >= f32(1.0), f32(0.0), fs).astype(np.float32)


def nearest_index(fs, W):
    """min((uint32)(fs * (float)W), W - 1)"""
    W = np.asarray(W, dtype=np.uint32)
    p = (np.asarray(fs, dtype=np.float32) * W.astype(np.float32)).astype(np.float32)
    return np.minimum(p.astype(np.int64), W.astype(np.int64) - 1)


def bilinear_index(fs, W):
    """(ix0, ix1, fx): x = fs * (float)W - 0.5f, x0 = floorf(x), fx = x - x0, ix0 = (int)x0 (-1 -> W - 1), ix1 = ix0 + 1 (W -> 0)."""
    W = np.asarray(W, dtype=np.uint32)
    Wi = W.astype(np.int64)
    x = ((np.asarray(fs, dtype=np.float32) * W.astype(np.float32)).astype(np.float32) - f32(0.5)).astype(np.float32)
    x0 = np.floor(x).astype(np.float32)
    fx = (x - x0).astype(np.float32)
    j = x0.astype(np.int64)
    return np.where(j == -1, Wi - 1, j), np.where(j + 1 == Wi, 0, j + 1), fx


def decode(words, fmt, table):
    """[3, n] float32: the R, G, B channels of the texel words - (float)c8 / 255.0f, or the sRGB table's entry."""
    words = np.asarray(words, dtype=np.uint32)
    out = np.zeros((3, words.shape[0]), dtype=np.float32)
    for c in range(3):
        c8 = (words >> np.uint32(8 * c)) & np.uint32(0xFF)
        out[c] = np.where(np.asarray(fmt) == SRGB, table[c8], (c8.astype(np.float32) / f32(255.0)).astype(np.float32))
    return out


def sample(s, t, tex, ts, table=None):
    """[3, n] float32 val for finite (s, t) and texture indices tex into the set ts."""
    table = srgb_table() if table is None else table
    d = ts.descs[tex]
    W, H, fmt, filt = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    off = np.concatenate([[0], np.cumsum(ts.descs[:, 0].astype(np.int64) * ts.descs[:, 1].astype(np.int64))])[tex]
    fs, ft = wrap(s), wrap(t)
    Wi = W.astype(np.int64)

    def tap(ix, iy):
        at = off + iy * Wi + ix
        assert ((ix >= 0) & (ix < Wi) & (iy >= 0) & (iy < H.astype(np.int64))).all(), "a tap outside its texture"
        return decode(ts.texels[at], fmt, table)
    near = tap(nearest_index(fs, W), nearest_index(ft, H))
    ix0, ix1, fx = bilinear_index(fs, W)
    iy0, iy1, fy = bilinear_index(ft, H)
    c00, c10, c01, c11 = tap(ix0, iy0), tap(ix1, iy0), tap(ix0, iy1), tap(ix1, iy1)
    top = (c00 + (fx * (c10 - c00).astype(np.float32)).astype(np.float32)).astype(np.float32)
    bot = (c01 + (fx * (c11 - c01).astype(np.float32)).astype(np.float32)).astype(np.float32)
    lin = (top + (fy * (bot - top).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return np.where(filt == BILINEAR, lin, near).astype(np.float32)


def albedo_at(prim, u, v, materials, tri_material, uvs=None, ts=None, table=None):
    """([3, n] float32 A, [n] cause) for surface records given by their prim and barycentrics - THE TEXTURED ALBEDO after
    "which records"."""
    mat = np.asarray(materials, dtype=np.float32).reshape(-1, 6)
    prim = np.asarray(prim, dtype=np.int64)
    m = np.asarray(tri_material, dtype=np.uint16)[prim].astype(np.int64)
    A = np.ascontiguousarray(mat[m, :3].T).astype(np.float32)
    cause = np.full(prim.shape[0], NO_TABLES, dtype=np.uint8)
    if uvs is None or ts is None:
        return A, cause
    T = ts.material_texture[m]
    cause[:] = NO_TEXTURE_FOR_MATERIAL
    has = np.flatnonzero(T != NO_TEXTURE)
    s, t = interpolate(np.asarray(u)[has], np.asarray(v)[has], np.asarray(uvs, dtype=np.float32).reshape(-1, 6)[prim[has]])
    fin = np.isfinite(s) & np.isfinite(t)
    cause[has[~fin]] = NOT_FINITE
    go = has[fin]
    cause[go] = TEXTURED
    if go.size:
        val = sample(s[fin], t[fin], T[go].astype(np.int64), ts, table)
        A[:, go] = (A[:, go] * val).astype(np.float32)
    return A, cause


def surface_albedo(hits, attr, materials, tri_material, n_tris, uvs=None, ts=None, table=None):
    """([3, n] float32, [n] cause): what trx_surface_albedo_dev writes for the records (hits, attr)."""
    n = hits.shape[0]
    out, cause = np.zeros((3, n), dtype=np.float32), np.full(n, BACKGROUND, dtype=np.uint8)
    idx = np.flatnonzero(surface(hits, n_tris))
    if idx.size:
        A, why = albedo_at(hits["prim"][idx], np.asarray(attr["u"])[idx], np.asarray(attr["v"])[idx], materials, tri_material, uvs, ts, table)
        out[:, idx], cause[idx] = A, why
    return out, cause


def albedo_compose(primary, albedo, direct, indirect, materials, tri_material, n_tris):
    """colour_c = emission_c + A_c * (E + I_c) at a surface record (the inner addition left out without `indirect`); +0 elsewhere."""
    mat = np.asarray(materials, dtype=np.float32).reshape(-1, 6)
    n = primary.shape[0]
    idx = np.flatnonzero(surface(primary, n_tris))
    m = mat[np.asarray(tri_material, dtype=np.uint16)[primary["prim"][idx].astype(np.int64)]]
    E = np.asarray(direct, dtype=np.float32)[idx]
    albedo = np.asarray(albedo, dtype=np.float32).reshape(3, n)
    out = np.zeros((3, n), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            inner = E if indirect is None else (E + np.asarray(indirect, dtype=np.float32).reshape(3, n)[c, idx]).astype(np.float32)
            out[c, idx] = (m[:, 3 + c] + (albedo[c, idx] * inner).astype(np.float32)).astype(np.float32)
    return out


# ---- the textured gathers: material_twin.term_rgb (rule 5c) and emitter_twin's loop (rule 5e) with the sampled albedo ------------

def term_rgb(samples, primary, materials, tri_material, n_tris, uvs, ts, table=None):
    """Rule 5c, textured: samples ascending, each (s_f [n], has a surface [n] bool, bounce prim [n], bounce attr [n])."""
    mat = np.asarray(materials, dtype=np.float32).reshape(-1, 6)
    tri_material = np.asarray(tri_material, dtype=np.uint16)
    A = np.zeros((3, primary.shape[0]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, has, prim, attr in samples:
            s = np.asarray(s, dtype=np.float32)
            idx = np.flatnonzero(has & (np.asarray(prim, dtype=np.uint64) < n_tris))
            alb, _ = albedo_at(prim[idx], attr["u"][idx], attr["v"][idx], mat, tri_material, uvs, ts, table)
            m = mat[tri_material[prim[idx]]]
            for c in range(3):
                inner = ((alb[c] * s[idx]).astype(np.float32) + m[:, 3 + c]).astype(np.float32)
                A[c, idx] = (A[c, idx] + inner).astype(np.float32)
        out = (A / f32(len(samples))).astype(np.float32)
    out[:, ~surface(primary, n_tris)] = f32(0.0)
    return out


def term_rgb_emitters(samples, primary, materials, tri_material, n_tris, uvs, ts, table=None):
    """Rule 5e, textured: samples ascending, each (s_f, has a surface, bounce prim, bounce attr, X [3, n]) with X_c the
    emitter's contribution wgeo * emission_c where its ray was cast and is not occluded, else +0."""
    mat = np.asarray(materials, dtype=np.float32).reshape(-1, 6)
    tri_material = np.asarray(tri_material, dtype=np.uint16)
    A = np.zeros((3, primary.shape[0]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, has, prim, attr, X in samples:
            s = np.asarray(s, dtype=np.float32)
            idx = np.flatnonzero(has & (np.asarray(prim, dtype=np.uint64) < n_tris))
            alb, _ = albedo_at(prim[idx], attr["u"][idx], attr["v"][idx], mat, tri_material, uvs, ts, table)
            for c in range(3):
                inner = (s[idx] + X[c][idx]).astype(np.float32)
                A[c, idx] = (A[c, idx] + (alb[c] * inner).astype(np.float32)).astype(np.float32)
        out = (A / f32(len(samples))).astype(np.float32)
    out[:, ~surface(primary, n_tris)] = f32(0.0)
    return out


# ---- the stand-in tables ------------------------------------------------------------------------------------------------------------

def standin_texcoords(verts):
    """[n, 6] float32: box mapping - the two coordinates other than the dominant axis of cross(v1 - v0, v2 - v0) (binary32; ties
    to the lower axis; a NaN component loses to any number), in ascending axis order."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = (v[:, 1] - v[:, 0]).astype(np.float32), (v[:, 2] - v[:, 0]).astype(np.float32)
        n = np.zeros_like(e1)
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            n[:, k] = ((e1[:, a] * e2[:, b]).astype(np.float32) - (e1[:, b] * e2[:, a]).astype(np.float32)).astype(np.float32)
    mag = np.where(np.isnan(n), f32(-1.0), np.abs(n))
    axis = np.argmax(mag, axis=1)                      # (the first of equal maxima: the lower axis)
    a, b = np.where(axis == 0, 1, 0), np.where(axis == 2, 1, 2)
    rows = np.arange(v.shape[0])
    out = np.zeros((v.shape[0], 6), dtype=np.float32)
    for c in range(3):
        out[:, 2 * c], out[:, 2 * c + 1] = v[rows, c, a], v[rows, c, b]
    return out


def checker():
    """[64 * 64] uint32: texel (x, y) has R = G = B = 255 where ((x >> 3) + (y >> 3)) & 1, else 128; alpha 255."""
    y, x = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    g = np.where(((x >> 3) + (y >> 3)) & 1, 255, 128).astype(np.uint32)
    return (g | g << np.uint32(8) | g << np.uint32(16) | np.uint32(0xFF000000)).reshape(-1).astype(np.uint32)


def standin_textures(n_materials):
    mt = np.full(n_materials, NO_TEXTURE, dtype=np.uint32)
    mt[0] = 0
    return texset([[64, 64, UNORM, BILINEAR]], checker(), mt)


# ---- tables for the tests --------------------------------------------------------------------------------------------------------------

HOSTILE_ST = [0.0, 1.0, -0.0, -1e-9, 1e30, -1e30, 1e-42, float("nan"), float("inf"), float("-inf"), 0.5, 0.25]


def random_uvs(n_tris, seed):
    """Seeded coordinates in about [-2, 3]: every wrap case of ordinary values."""
    return np.random.default_rng(seed).uniform(-2.0, 3.0, (n_tris, 6)).astype(np.float32)


def hostile_uvs(n_tris, seed):
    """Every corner's s and t drawn from HOSTILE_ST; about half the triangles keep ordinary values in some corners."""
    rng = np.random.default_rng(seed)
    out = np.array(HOSTILE_ST, dtype=np.float32)[rng.integers(0, len(HOSTILE_ST), (n_tris, 6))]
    plain = rng.random((n_tris, 6)) < 0.5
    out[plain] = rng.uniform(-1.0, 2.0, int(plain.sum())).astype(np.float32)
    whole = rng.random(n_tris) < 0.3                      # (whole triangles of the constants that are finite)
    out[whole] = np.array([0.0, 1.0, -0.0, -1e-9, 1e-42, 0.5], dtype=np.float32)[rng.integers(0, 6, (int(whole.sum()), 6))]
    return out


def random_textures(n_materials, seed, sizes=((1, 1), (2, 1), (3, 5), (17, 9))):
    """Every size in both formats and both filters, random texels; about one material in five stays untextured - material 1 always
    (with three or more) - material 0 and the last one are textured."""
    rng = np.random.default_rng(seed)
    descs = [[w, h, fmt, filt] for (w, h) in sizes for fmt in (UNORM, SRGB) for filt in (NEAREST, BILINEAR)]
    n_texels = sum(d[0] * d[1] for d in descs)
    texels = rng.integers(0, 2 ** 32, n_texels, dtype=np.uint64).astype(np.uint32)
    mt = rng.integers(0, len(descs), n_materials).astype(np.uint32)
    mt[rng.random(n_materials) < 0.2] = NO_TEXTURE
    mt[0], mt[-1] = 3, len(descs) - 1
    if n_materials >= 3:
        mt[1] = NO_TEXTURE
    return texset(descs, texels, mt)


def white_textures(n_materials, filt, fmt=UNORM, sizes=((1, 1), (2, 1), (3, 5), (17, 9))):
    """Every texel 255 in every channel, every material textured: val is exactly 1 and the albedo the material's."""
    descs = [[w, h, fmt, filt] for (w, h) in sizes]
    texels = np.full(sum(d[0] * d[1] for d in descs), 0xFFFFFFFF, dtype=np.uint32)
    return texset(descs, texels, (np.arange(n_materials) % len(descs)).astype(np.uint32))


# ---- the loaders restated ---------------------------------------------------------------------------------------------------------------

def load_obj_texcoords(path):
    """(uvs [n_tris, 6] float32, any): the OBJ's `vt` of every corner in the triangle order of trx_load_model.  `vt` records hold
    two numbers (a missing second one is 0); the second index of v/vt or v/vt/vn names one, counted back from the last `vt` read
    when negative; a corner without an index, or with one outside the `vt` read so far, gets +0, +0.  A face gives vertices 0, 1,
    2 and - with exactly four - 0, 2, 3; a triangle with a position index outside the vertices read so far is dropped."""
    n_pos, vts, rows, any_vt = 0, [], [], False
    for line in open(path, "rb").read().decode("latin-1").split("\n"):
        if line[:2] in ("v ", "v\t"):
            n_pos += 1
        elif line[:3] in ("vt ", "vt\t"):
            nums = line[3:].split()
            vts.append((f32(float(nums[0])) if nums else f32(0.0), f32(float(nums[1])) if len(nums) > 1 else f32(0.0)))
        elif line[:2] in ("f ", "f\t"):
            corners = []
            for tok in line[2:].split():
                parts = tok.split("/")
                try:
                    v = int(parts[0])
                except ValueError:
                    break
                t = None
                if len(parts) > 1 and parts[1] not in ("", "-", "+"):
                    try:
                        t = int(parts[1])
                        t = len(vts) + t if t < 0 else t - 1
                    except ValueError:
                        t = None
                corners.append((n_pos + v if v < 0 else v - 1, t))
            tris = ([corners[:3]] if len(corners) >= 3 else []) + ([[corners[0], corners[2], corners[3]]] if len(corners) == 4 else [])
            for tri in tris:
                if all(0 <= i < n_pos for i, _ in tri):
                    row = []
                    for _, t in tri:
                        have = t is not None and 0 <= t < len(vts)
                        any_vt = any_vt or have
                        row += list(vts[t]) if have else [f32(0.0), f32(0.0)]
                    rows.append(row)
    return np.array(rows, dtype=np.float32).reshape(-1, 6), any_vt


def load_obj_material_maps(path):
    """[n_materials] list of str: "" for material 0, then per `newmtl` of every `mtllib` file (read from the OBJ's directory, a
    missing one adds nothing) the last blank-separated word of its last `map_Kd` line, "" without one."""
    import os
    maps = [""]
    for line in open(path, "rb").read().decode("latin-1").split("\n"):
        if line[:7] in ("mtllib ", "mtllib\t"):
            mtl = os.path.join(os.path.dirname(path), line[6:].strip(" \t\r\n"))
            if not os.path.exists(mtl):
                continue
            open_ = False
            for ml in open(mtl, "rb").read().decode("latin-1").split("\n"):
                ml = ml.lstrip(" \t")
                if ml[:7] in ("newmtl ", "newmtl\t"):
                    maps.append("")
                    open_ = True
                elif open_ and ml[:7] in ("map_Kd ", "map_Kd\t"):
                    words = ml[6:].split()
                    maps[-1] = words[-1] if words else ""
    return maps


def read_ppm(path):
    """([h, w] uint32 RGBA8 words with alpha 255, row 0 the file's top row) of a binary PPM with maxval 255."""
    d = open(path, "rb").read()
    assert d[:2] == b"P6"
    nums, p = [], 2
    while len(nums) < 3:
        while d[p:p + 1].isspace():
            p += 1
        if d[p:p + 1] == b"#":
            p = d.index(b"\n", p)
            continue
        q = p
        while d[q:q + 1].isdigit():
            q += 1
        nums.append(int(d[p:q]))
        p = q
    w, h, maxval = nums
    assert maxval == 255
    rgb = np.frombuffer(d[p + 1:p + 1 + w * h * 3], dtype=np.uint8).reshape(h, w, 3).astype(np.uint32)
    return rgb[..., 0] | rgb[..., 1] << np.uint32(8) | rgb[..., 2] << np.uint32(16) | np.uint32(0xFF000000)
