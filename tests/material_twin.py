"""The twin of the colour passes (include/trx.h, "materials"): THE DEFINITION of rule 5c's sums, the sparse form, the compose,
the RGB shade and the stand-in tables, in numpy float32.  It calls nothing of the library's colour code: s_f, the bounce rays
and the bounce hits come from tests/indirect_twin.py (`bounce`, `sample_sum`), which stands on the oracle alone.

Every function takes whole-image records in pixel order (y * w + x); planes are rows of a [3, n] array (0 = R, 1 = G, 2 = B).
A material table is a [n, 6] float32 array: albedo r, g, b, emission r, g, b."""
import numpy as np

import indirect_twin as IT
import light_twin as LT

f32 = np.float32
INVALID = 0xFFFFFFFF
PALETTE = np.array([(.8, .8, .8), (.8, .4, .3), (.3, .6, .8), (.5, .7, .3), (.8, .7, .4), (.6, .5, .7)], dtype=np.float32)


def table(materials):
    """[n, 6] float32 from a [n, 6] array or a structured (albedo, emission) array."""
    m = np.asarray(materials)
    if m.dtype.names:
        m = np.concatenate([m["albedo"], m["emission"]], axis=1)
    return np.ascontiguousarray(m, dtype=np.float32).reshape(-1, 6)


def term_rgb(samples, primary, materials, tri_material, n_tris):
    """Rule 5c: [3, n] float32 from the samples, ascending - each (s_f [n], has a surface [n] bool, bounce prim [n])."""
    mat = table(materials)
    tri_material = np.asarray(tri_material, dtype=np.uint16)
    n = primary.shape[0]
    A = np.zeros((3, n), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, has, prim in samples:
            s = np.asarray(s, dtype=np.float32)
            idx = np.flatnonzero(has)
            m = mat[tri_material[prim[idx]]]
            for c in range(3):
                inner = (m[:, c] * s[idx]).astype(np.float32)              # albedo_c * s_f
                inner = (inner + m[:, 3 + c]).astype(np.float32)           # + emission_c
                A[c, idx] = (A[c, idx] + inner).astype(np.float32)         # A_c + (...)
        out = (A / f32(len(samples))).astype(np.float32)
    out[:, ~LT.surface(primary, n_tris)] = f32(0.0)
    return out


def indirect_rgb(orc, osc, oview, w, h, primary, primary_inst, recs, w2o, lights, frame0, n_samples, bounce_eps, shadow_eps, sem, materials,
                 tri_material, shadow_osc=None, cache=None, keep=None):
    """The dense pass: [3, w * h] float32.  cache: keeps the bounces (rules 1, 2) per seed; keep: a list that receives the
    samples (s_f, surface mask, bounce prim) - the material-free part, which other tables can reuse through term_rgb."""
    samples = []
    for f in range(n_samples):
        key = (frame0 + f, float(bounce_eps), sem, hash(primary.tobytes()), hash(np.asarray(primary_inst).tobytes()))
        if cache is not None and key in cache:
            b = cache[key]
        else:
            b = IT.bounce(orc, osc, oview, w, h, primary, primary_inst, recs, w2o, frame0 + f, bounce_eps, sem)
            if cache is not None:
                cache[key] = b
        rays, hits, _, attr = b
        s = IT.sample_sum(orc, w, h, rays, hits, attr, lights, frame0, f, shadow_eps, IT.oracle_occluded(shadow_osc or osc, sem))
        samples.append((s, IT.bounce_surface(rays, hits), np.asarray(hits["prim"], dtype=np.uint32)))
    if keep is not None:
        keep.extend(samples)
    return term_rgb(samples, primary, materials, tri_material, recs.shape[0])


def sparse_rgb(dense, w, h, stride, phase):
    """The sparse pass from the dense planes [3, w * h]: [3, Wlo * Hlo], every cell the value of its pixel, +0 where the pixel
    leaves the image (a pixel without a surface holds +0 already)."""
    wlo, hlo = (w + stride - 1) // stride, (h + stride - 1) // stride
    px0, py0 = phase % stride, phase // stride
    X, Y = np.meshgrid(np.arange(wlo), np.arange(hlo))
    px, py = (X * stride + px0).reshape(-1), (Y * stride + py0).reshape(-1)
    inside = (px < w) & (py < h)
    out = np.zeros((3, wlo * hlo), dtype=np.float32)
    out[:, inside] = dense[:, py[inside] * w + px[inside]]
    return out


def compose(primary, direct, indirect, materials, tri_material, n_tris):
    """colour_c = emission_c + albedo_c * (E + I_c) at a record with t < FLT_MAX, prim != 0xFFFFFFFF and prim < n_tris (the
    inner addition is left out without `indirect`); +0 elsewhere.  [3, n] float32."""
    mat = table(materials)
    tri_material = np.asarray(tri_material, dtype=np.uint16)
    n = primary.shape[0]
    prim = np.asarray(primary["prim"], dtype=np.uint64)
    surf = (primary["t"] < LT.F32_MAX) & (prim != INVALID) & (prim < n_tris)
    idx = np.flatnonzero(surf)
    m = mat[tri_material[prim[idx]]]
    E = np.asarray(direct, dtype=np.float32)[idx]
    out = np.zeros((3, n), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            inner = E if indirect is None else (E + np.asarray(indirect, dtype=np.float32)[c, idx]).astype(np.float32)
            out[c, idx] = (m[:, 3 + c] + (m[:, c] * inner).astype(np.float32)).astype(np.float32)
    return out


def shade_rgb(colour, thr):
    """[n, 4] uint8 {code(R), code(G), code(B), 255}: a value's code is the number of thresholds thr[1..255] it reaches (NaN and
    negative values reach none, everything from 1 upward all) - the value shade's statement."""
    colour = np.asarray(colour, dtype=np.float32)
    out = np.full((colour.shape[1], 4), 255, dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        for c in range(3):
            out[:, c] = (colour[c][:, None] >= np.asarray(thr, dtype=np.float32)[None, 1:]).sum(1).astype(np.uint8)
    return out


def standin(name, verts, counts):
    """(materials [n, 6], tri_material [n_tris] uint16) of a generated scene, in the order of verts ([n_tris, 9])."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 9)
    counts = [int(c) for c in counts]
    n_tris = verts.shape[0]
    assert sum(counts) == n_tris
    idx = np.zeros(n_tris, dtype=np.uint16)
    if name == "cornell":
        mat = np.zeros((4, 6), dtype=np.float32)
        mat[0, :3] = f32(0.8)
        mat[1, 0] = f32(0.8)
        mat[2, 1] = f32(0.8)
        mat[3, 3:] = f32(4.0)
        x = verts[:, 0::3]
        idx[(x == f32(-1.0)).all(1)] = 1
        idx[(x == f32(1.0)).all(1)] = 2
        idx[n_tris - counts[-1]:] = 3
        return mat, idx
    mat = np.zeros((6, 6), dtype=np.float32)
    mat[:, :3] = PALETTE
    idx[:] = np.repeat(np.arange(len(counts)) % 6, counts).astype(np.uint16)
    return mat, idx


def seeded_table(n_tris, n_materials, seed):
    """A table for a scene that has no stand-in: materials 0 and n_materials - 1 are used, triangle 0 and triangle n_tris - 1 get
    distinct materials (with two or more), about one material in eight emits, some albedos are 0 and some 1."""
    rng = np.random.default_rng(seed)
    mat = np.zeros((n_materials, 6), dtype=np.float32)
    mat[:, :3] = rng.uniform(0.0, 1.0, (n_materials, 3)).astype(np.float32)
    mat[rng.random(n_materials) < 0.1, 0] = f32(0.0)
    mat[rng.random(n_materials) < 0.1, 1] = f32(1.0)
    emit = rng.random(n_materials) < 0.125
    mat[emit, 3:] = rng.uniform(0.0, 3.0, (int(emit.sum()), 3)).astype(np.float32)
    idx = rng.integers(0, n_materials, n_tris).astype(np.uint16)
    idx[0], idx[-1] = 0, n_materials - 1
    return mat, idx


def load_obj_materials(path):
    """The loader's table restated: (materials [n, 6], tri_material [n_tris] uint16) of an OBJ, in the triangle order of
    trx_load_model.  Material 0 is the default (0.8, 0.8, 0.8; 0); the `newmtl` entries of every `mtllib` file (read from the
    OBJ's directory, a missing one adds nothing) follow in file order with Kd (missing: 0.8) and Ke (missing: 0); a `usemtl` name
    is looked up once the whole file is read, the first material of a name wins, an unknown name and faces before any usemtl get
    0.  A face gives vertices 0, 1, 2 and - with exactly four - 0, 2, 3; a triangle with an index outside the vertices read so
    far is dropped; negative indices count back from the last vertex."""
    import os
    names, rows = [], [[0.8, 0.8, 0.8, 0.0, 0.0, 0.0]]
    tri_names, n_pos, use = [], 0, None
    for line in open(path, "rb").read().decode("latin-1").split("\n"):
        if line[:2] in ("v ", "v\t"):
            n_pos += 1
        elif line[:7] in ("mtllib ", "mtllib\t"):
            mtl = os.path.join(os.path.dirname(path), line[6:].strip(" \t\r\n"))
            if not os.path.exists(mtl):
                continue
            open_ = False
            for ml in open(mtl, "rb").read().decode("latin-1").split("\n"):
                ml = ml.lstrip(" \t")
                if ml[:7] in ("newmtl ", "newmtl\t"):
                    names.append(ml[6:].strip(" \t\r\n"))
                    rows.append([0.8, 0.8, 0.8, 0.0, 0.0, 0.0])
                    open_ = True
                elif open_ and ml[:3] in ("Kd ", "Kd\t", "Ke ", "Ke\t"):
                    at = 0 if ml[1] == "d" else 3
                    rows[-1][at:at + 3] = [float(x) for x in ml[2:].split()[:3]]
        elif line[:7] in ("usemtl ", "usemtl\t"):
            use = line[6:].strip(" \t\r\n")
        elif line[:2] in ("f ", "f\t"):
            idx = []
            for tok in line[2:].split():
                try:
                    v = int(tok.split("/")[0])
                except ValueError:
                    break
                idx.append(n_pos + v if v < 0 else v - 1)
            tris = ([idx[:3]] if len(idx) >= 3 else []) + ([[idx[0], idx[2], idx[3]]] if len(idx) == 4 else [])
            for t in tris:
                if all(0 <= i < n_pos for i in t):
                    tri_names.append(use)
    where = {}
    for k, nm in enumerate(names):
        where.setdefault(nm, k + 1)
    return np.array(rows, dtype=np.float32), np.array([where.get(nm, 0) for nm in tri_names], dtype=np.uint16)
