"""Host-side mirror of the reference's CWBVH GPU path over the C-ABI.

Names follow the reference: `cwbvh_gpu_runner` (src/rt_gpu/mod.rs:16-112)
assembles the flat node / triangle / instance buffers, `Scene` owns what
rt_gpu_software::start uploaded (src/rt_gpu/rt_gpu_software.rs:24-32,83-160),
and `Scene.start` returns the frame time in ms like the reference does (:376).
"""
import ctypes as C

import numpy as np

from . import _lib as L

HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<u4")])
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("direction", "<f4", 3), ("tmax", "<f4")])
RAYHIT_DTYPE = np.dtype([("primitive_id", "<u4"), ("geometry_id", "<u4"), ("instance_id", "<u4"), ("t", "<f4")])  # obvhs RayHit
# trx_hit_attr: barycentrics of the committed triangle test (u weights v1, v weights v2) and the world-space unit
# geometric normal; all zero for a miss
HIT_ATTR_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("normal", "<f4", 3), ("_pad", "<u4")])
# trx_ao_term: the edge-aware AO filter's output per pixel
AO_TERM_DTYPE = np.dtype([("unoccluded", "<u2"), ("samples", "<u2")])
RAY_COST_DTYPE = np.dtype([("n_node", "<u2"), ("n_tri", "<u2")])
# trx_material: diffuse albedo and emission, linear RGB
MATERIAL_DTYPE = np.dtype([("albedo", "<f4", 3), ("emission", "<f4", 3)])
# trx_texture_desc: one texture of a scene's texture set
TEXTURE_DESC_DTYPE = np.dtype([("width", "<u4"), ("height", "<u4"), ("format", "<u4"), ("filter", "<u4")])
TEX_RGBA8_UNORM, TEX_RGBA8_SRGB = 0, 1
TEX_NEAREST, TEX_BILINEAR = 0, 1
NO_TEXTURE = 0xFFFFFFFF
MISS_PRIM = 0xFFFFFFFF


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- scenes / models ----------------------------------------------------------

def _take_mesh(verts_p, n, counts_p, nobj):
    lib = L.load()
    verts = np.ctypeslib.as_array(verts_p, shape=(max(n.value, 1), 9))[: n.value].copy()
    counts = np.ctypeslib.as_array(counts_p, shape=(max(nobj.value, 1),))[: nobj.value].copy()
    lib.trx_free(C.cast(verts_p, C.c_void_p))
    lib.trx_free(C.cast(counts_p, C.c_void_p))
    return verts, counts.astype(np.uint64)


def gen_scene(name, n_tris=0, seed=1):
    """Seeded procedural stand-in for one of the reference's absent assets."""
    lib = L.load()
    vp, cp = C.POINTER(C.c_float)(), C.POINTER(C.c_uint64)()
    n, nobj = C.c_uint64(), C.c_uint32()
    L.check(lib.trx_gen_scene(name.encode(), n_tris, seed, C.byref(vp), C.byref(n), C.byref(cp), C.byref(nobj)))
    return _take_mesh(vp, n, cp, nobj)


def standin_materials(name, verts, counts):
    """(materials [n] MATERIAL_DTYPE, tri_material [n_tris] uint16): trx_standin_materials - the materials of a generated
    scene for the mesh gen_scene returned (cornell: grey, red left wall, green right wall, emissive light quad; any other
    name: a palette of six albedos by object).  tri_material is in the order of verts."""
    lib = L.load()
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
    c = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    mp, ip, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
    L.check(lib.trx_standin_materials(name.encode(), _ptr(v), v.shape[0], _ptr(c), c.size, C.byref(mp), C.byref(n), C.byref(ip)))
    mats = np.frombuffer(C.string_at(mp.value, n.value * MATERIAL_DTYPE.itemsize), dtype=MATERIAL_DTYPE).copy()
    idx = np.frombuffer(C.string_at(ip.value, v.shape[0] * 2), dtype=np.uint16).copy()
    lib.trx_free(mp)
    lib.trx_free(ip)
    return mats, idx


def standin_texcoords(name, verts):
    """[n_tris, 6] f32 (s0, t0, s1, t1, s2, t2): trx_standin_texcoords - box mapping of the mesh as given (per triangle the two
    coordinates other than the dominant axis of its face vector), in the order of verts."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
    out = np.zeros((v.shape[0], 6), dtype=np.float32)
    L.check(L.load().trx_standin_texcoords(name.encode(), _ptr(v), v.shape[0], _ptr(out)))
    return out


def standin_textures(name, n_materials):
    """(descs [n] TEXTURE_DESC_DTYPE, texels [n_texels] uint32, material_texture [n_materials] uint32): trx_standin_textures -
    one 64 x 64 UNORM bilinear checker on material 0, NO_TEXTURE everywhere else."""
    lib = L.load()
    dp, tp, mp = C.c_void_p(), C.c_void_p(), C.c_void_p()
    n, nt = C.c_uint32(), C.c_uint64()
    L.check(lib.trx_standin_textures(name.encode(), n_materials, C.byref(dp), C.byref(n), C.byref(tp), C.byref(nt), C.byref(mp)))
    descs = np.frombuffer(C.string_at(dp.value, n.value * TEXTURE_DESC_DTYPE.itemsize), dtype=TEXTURE_DESC_DTYPE).copy()
    texels = np.frombuffer(C.string_at(tp.value, nt.value * 4), dtype=np.uint32).copy()
    mat_tex = np.frombuffer(C.string_at(mp.value, n_materials * 4), dtype=np.uint32).copy()
    for p in (dp, tp, mp):
        lib.trx_free(p)
    return descs, texels, mat_tex


def texture_srgb_table():
    """[256] f32: trx_texture_srgb_table - the sRGB decode of every byte, computed in binary64 and rounded once."""
    out = np.zeros(256, dtype=np.float32)
    L.load().trx_texture_srgb_table(_ptr(out))
    return out


def load_meshs(path):
    """load_meshs (src/main.rs:494-561): OBJ or JSON -> (verts [n,9], triangles per object)."""
    lib = L.load()
    vp, cp = C.POINTER(C.c_float)(), C.POINTER(C.c_uint64)()
    n, nobj = C.c_uint64(), C.c_uint32()
    L.check(lib.trx_load_model(str(path).encode(), C.byref(vp), C.byref(n), C.byref(cp), C.byref(nobj)))
    return _take_mesh(vp, n, cp, nobj)


def load_model_materials(path):
    """(verts [n,9], triangles per object, materials [m] MATERIAL_DTYPE, tri_material [n] uint16): trx_load_model_materials -
    load_meshs' mesh with the materials of the OBJ's mtl files (Kd: albedo, Ke: emission; material 0 is the default 0.8 / 0 and
    goes to faces without a known usemtl, and to every triangle of a JSON model)."""
    lib = L.load()
    vp, cp = C.POINTER(C.c_float)(), C.POINTER(C.c_uint64)()
    n, nobj, nmat = C.c_uint64(), C.c_uint32(), C.c_uint32()
    mp, ip = C.c_void_p(), C.c_void_p()
    L.check(lib.trx_load_model_materials(str(path).encode(), C.byref(vp), C.byref(n), C.byref(cp), C.byref(nobj), C.byref(mp), C.byref(nmat),
                                         C.byref(ip)))
    mats = np.frombuffer(C.string_at(mp.value, nmat.value * MATERIAL_DTYPE.itemsize), dtype=MATERIAL_DTYPE).copy()
    idx = np.frombuffer(C.string_at(ip.value, n.value * 2), dtype=np.uint16).copy()
    lib.trx_free(mp)
    lib.trx_free(ip)
    verts, counts = _take_mesh(vp, n, cp, nobj)
    return verts, counts, mats, idx


def load_model_normals(path):
    """(verts [n,9], triangles per object, normals [n,9] f32, has_normals): trx_load_model_normals - load_meshs' mesh with
    the OBJ's `vn` record of every corner (v/vt/vn, v//vn; +0 for a corner that names none or one out of range, and for every
    corner of a JSON model); has_normals says whether any corner got one."""
    lib = L.load()
    vp, cp, np_ = C.POINTER(C.c_float)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_float)()
    n, nobj, has = C.c_uint64(), C.c_uint32(), C.c_uint32()
    L.check(lib.trx_load_model_normals(str(path).encode(), C.byref(vp), C.byref(n), C.byref(cp), C.byref(nobj), C.byref(np_), C.byref(has)))
    normals = np.ctypeslib.as_array(np_, shape=(max(n.value, 1), 9))[: n.value].copy()
    lib.trx_free(C.cast(np_, C.c_void_p))
    verts, counts = _take_mesh(vp, n, cp, nobj)
    return verts, counts, normals, bool(has.value)


def load_model_texcoords(path):
    """(verts [n,9], triangles per object, uvs [n,6] f32, has_texcoords): trx_load_model_texcoords - load_meshs' mesh with the
    OBJ's `vt` record of every corner (v/vt, v/vt/vn; +0, +0 for a corner that names none or one out of range, and for every
    corner of a JSON model); has_texcoords says whether any corner got one."""
    lib = L.load()
    vp, cp, up = C.POINTER(C.c_float)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_float)()
    n, nobj, has = C.c_uint64(), C.c_uint32(), C.c_uint32()
    L.check(lib.trx_load_model_texcoords(str(path).encode(), C.byref(vp), C.byref(n), C.byref(cp), C.byref(nobj), C.byref(up), C.byref(has)))
    uvs = np.ctypeslib.as_array(up, shape=(max(n.value, 1), 6))[: n.value].copy()
    lib.trx_free(C.cast(up, C.c_void_p))
    verts, counts = _take_mesh(vp, n, cp, nobj)
    return verts, counts, uvs, bool(has.value)


def load_model_material_maps(path):
    """[n_materials] list of str: trx_load_model_material_maps - the map_Kd file name of every material in
    load_model_materials' order, "" where a material names none (material 0 never does)."""
    lib = L.load()
    p, n = C.c_void_p(), C.c_uint32()
    L.check(lib.trx_load_model_material_maps(str(path).encode(), C.byref(p), C.byref(n)))
    out, at = [], p.value
    for _ in range(n.value):
        s = C.string_at(at)
        out.append(s.decode("latin-1"))
        at += len(s) + 1
    lib.trx_free(p)
    return out


def compute_vertex_normals(verts, crease_cos=0.70710678):
    """[n,9] f32: trx_compute_vertex_normals - per corner the area-weighted sum, normalised, of the face vectors of the
    triangles that share the corner's position (bitwise, -0.0 as +0.0) and lie within the crease angle of the corner's own
    triangle (unit face vectors' dot product >= crease_cos); +0 for the corners of a degenerate triangle."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
    out = np.zeros_like(v)
    L.check(L.load().trx_compute_vertex_normals(_ptr(v), v.shape[0], crease_cos, _ptr(out)))
    return out


def load_scene(path):
    """A scene file of the reference (assets/scenes/*.ron) as src/main.rs:259-298 reads it: (verts [n,9], triangles per
    object, eye, look_at, fov) - trx_load_scene."""
    lib = L.load()
    vp, cp = C.POINTER(C.c_float)(), C.POINTER(C.c_uint64)()
    n, nobj = C.c_uint64(), C.c_uint32()
    eye, look, fov = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()
    L.check(lib.trx_load_scene(str(path).encode(), C.byref(vp), C.byref(n), C.byref(cp), C.byref(nobj), eye, look, C.byref(fov)))
    verts, counts = _take_mesh(vp, n, cp, nobj)
    return verts, counts, list(eye), list(look), fov.value


def image_code_table():
    """[256] f32 (trx_image_code_table, no device needed): thr[k] is the smallest colour in [0, 1] whose 8-bit code on this
    host, uint8(powf(col, 2.2f) * 255), is >= k; the device's code of a colour is the number of k >= 1 with col >= thr[k]."""
    out = np.empty(256, dtype=np.float32)
    L.check(L.load().trx_image_code_table(_ptr(out)))
    return out


def copy_rate(device=0, nbytes=1 << 30, reps=5):
    """Streaming ceiling of the device's memory, bytes read + written per second by a float4 copy kernel (trx_debug_copy_rate)."""
    out = C.c_double()
    L.check(L.load().trx_debug_copy_rate(device, nbytes, reps, C.byref(out)))
    return out.value


def scene_camera(name):
    lib = L.load()
    eye, look, fov = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()
    L.check(lib.trx_scene_camera(name.encode(), eye, look, C.byref(fov)))
    return list(eye), list(look), fov.value


def view_from_camera(eye, look_at, fov_deg, width, height):
    """ViewUniform::from_camera (src/main.rs:602-616)."""
    lib = L.load()
    v = L.View()
    L.check(lib.trx_view_from_camera((C.c_float * 3)(*eye), (C.c_float * 3)(*look_at), fov_deg, float(width),
                                     float(height), C.byref(v)))
    return v


# ---- flat buffers (cwbvh_gpu_runner's assembly half) -----------------------------

def light(kind, position, edge1=(0.0, 0.0, 0.0), edge2=(0.0, 0.0, 0.0), intensity=1.0):
    """An L.Light (trx_light): kind L.LIGHT_DIRECTIONAL (position = the direction toward the light), L.LIGHT_POINT or
    L.LIGHT_RECT (position = a corner, the light spans edge1 and edge2 from it)."""
    out = L.Light()
    out.kind = kind
    out.position[:] = [float(x) for x in position]
    out.edge1[:] = [float(x) for x in edge1]
    out.edge2[:] = [float(x) for x in edge2]
    out.intensity = float(intensity)
    return out


def light_array(lights):
    """A contiguous ctypes array of L.Light from a sequence of them (or the array itself)."""
    if isinstance(lights, C.Array):
        return lights
    lights = list(lights)
    return (L.Light * len(lights))(*lights)


class FlatScene:
    """The buffers rt_gpu_software::start receives: bvh_bytes, tri_bytes, instance_bytes, tlas_start."""

    def __init__(self, nodes, tri_verts, instance_offsets, tlas_start, tri_source, blas_tri_start,
                 blas_build_s=0.0, tlas_build_s=0.0, tri_boxes=None, instance_source=None, instance_transforms=None,
                 instance_entry=None):
        self.nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 20)
        self.tri_verts = np.ascontiguousarray(tri_verts, dtype=np.float32).reshape(-1, 9)
        self.instance_offsets = np.ascontiguousarray(instance_offsets, dtype=np.uint32)
        self.tlas_start = int(tlas_start)
        self.tri_source = np.ascontiguousarray(tri_source, dtype=np.uint32)
        self.blas_tri_start = np.ascontiguousarray(blas_tri_start, dtype=np.uint32)
        self.blas_build_s = blas_build_s
        self.tlas_build_s = tlas_build_s
        # box every triangle entry was built with (pre-split references cover only part of their triangle)
        self.tri_boxes = None if tri_boxes is None else np.ascontiguousarray(tri_boxes, dtype=np.float32).reshape(-1, 6)
        # TLAS primitive k = the caller's object / instance instance_source[k]; object-to-world 4x4 (column-major)
        # per TLAS primitive, or None = identity (the reference, src/cwbvh.rs:163-165)
        self.instance_source = None if instance_source is None else np.ascontiguousarray(instance_source, dtype=np.uint32)
        self.instance_transforms = None if instance_transforms is None else np.ascontiguousarray(
            instance_transforms, dtype=np.float32).reshape(-1, 16)
        # node of its BLAS at which TLAS primitive k starts (re-braided TLAS), or None = node 0 (the reference)
        self.instance_entry = None if instance_entry is None else np.ascontiguousarray(instance_entry, dtype=np.uint32)

    @property
    def n_nodes(self):
        return self.nodes.shape[0]

    @property
    def n_tris(self):
        return self.tri_verts.shape[0]

    @property
    def has_tlas(self):
        return self.instance_offsets.size > 0


def flat_build(verts, object_counts=None, use_tlas=False, max_prims_per_leaf=3, threads=0, traversal_cost=None,
               prim_cost=None, reinsertion=None, preset=None, split=None):
    """`reinsertion`: None keeps the process-wide setting; a float is the batch ratio (2 iterations),
    a (ratio, iterations) pair sets both (trx_set_build_reinsertion)."""
    lib = L.load()
    if preset is not None:   # the reference's --preset names (trx_set_build_preset); "" = defaults
        L.check(lib.trx_set_build_preset(preset.encode()))
    if split is not None:    # pre-splitting: extra triangle references as a fraction of n (trx_set_build_split)
        L.check(lib.trx_set_build_split(float(split)))
    if traversal_cost is not None or prim_cost is not None:
        L.check(lib.trx_set_build_costs(traversal_cost or 1.0, prim_cost or 0.3))
    if reinsertion is not None:
        ratio, iters = reinsertion if isinstance(reinsertion, (tuple, list)) else (reinsertion, 2)
        L.check(lib.trx_set_build_reinsertion(float(ratio), int(iters)))
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
    if object_counts is None:
        object_counts = [verts.shape[0]]
    counts = np.ascontiguousarray(object_counts, dtype=np.uint64)
    if int(counts.sum()) != verts.shape[0]:
        raise L.TrxError(L.TRX_ERR_INVALID, "object counts do not add up to the triangle count")
    fp = C.POINTER(L.Flat)()
    L.check(lib.trx_flat_build(_ptr(verts), _ptr(counts), counts.size, 1 if use_tlas else 0, max_prims_per_leaf,
                               threads, C.byref(fp)))
    return _take_flat(lib, fp)


class _FlatOwner:
    """Keeps a trx_flat alive while numpy views of its buffers exist (trx_flat_destroy when the last one goes)."""

    def __init__(self, lib, fp):
        self.lib, self.fp = lib, fp

    def __del__(self):
        try:
            self.lib.trx_flat_destroy(self.fp)
        except Exception:   # interpreter shutdown
            pass


def _view(owner, address, dtype, count, shape):
    """A numpy array over `count` items of the library's memory at `address` (no copy: a 3.9 M triangle scene has
    280 MB of them); the array holds `owner`."""
    dtype = np.dtype(dtype)
    if count == 0 or not address:
        return np.zeros(shape, dtype=dtype)
    raw = (C.c_uint8 * (count * dtype.itemsize)).from_address(address)
    raw._trx_owner = owner
    return np.frombuffer(raw, dtype=dtype).reshape(shape)


def _take_flat(lib, fp):
    f = fp.contents
    owner = _FlatOwner(lib, fp)
    addr = lambda p: C.cast(p, C.c_void_p).value
    nodes = _view(owner, f.bvh_bytes, np.uint32, f.n_nodes * 20, (f.n_nodes, 20))
    tris = _view(owner, addr(f.tri_verts), np.float32, f.n_tris * 9, (f.n_tris, 9))
    inst = _view(owner, addr(f.instance_offsets), np.uint32, f.n_instances, (f.n_instances,))
    src = _view(owner, addr(f.tri_source), np.uint32, f.n_tris, (f.n_tris,))
    bts = _view(owner, addr(f.blas_tri_start), np.uint32, f.n_blas + 1, (f.n_blas + 1,))
    boxes = _view(owner, addr(f.tri_boxes), np.float32, f.n_tris * 6, (f.n_tris, 6))
    isrc = _view(owner, addr(f.instance_source), np.uint32, f.n_instances, (f.n_instances,))
    ixf = _view(owner, addr(f.instance_transforms), np.float32, f.n_instances * 16, (f.n_instances, 16)) if f.instance_transforms else None
    ient = _view(owner, addr(f.instance_entry_nodes), np.uint32, f.n_instances, (f.n_instances,)) if f.instance_entry_nodes else None
    return FlatScene(nodes, tris, inst, f.tlas_start, src, bts, f.blas_build_s, f.tlas_build_s, boxes, isrc, ixf, ient)


def flat_build_instanced(verts, object_counts, instance_object, object_to_world=None, max_prims_per_leaf=3, threads=0):
    """One BLAS per object, a TLAS over instances of them (trx_flat_build_instanced).  object_to_world: [n, 16]
    column-major affine matrices (glam Mat4), or None for identity."""
    lib = L.load()
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
    counts = np.ascontiguousarray(object_counts, dtype=np.uint64)
    io = np.ascontiguousarray(instance_object, dtype=np.uint32)
    xf = None if object_to_world is None else np.ascontiguousarray(object_to_world, dtype=np.float32).reshape(-1, 16)
    if xf is not None and xf.shape[0] != io.size:
        raise L.TrxError(L.TRX_ERR_INVALID, "one transform per instance")
    fp = C.POINTER(L.Flat)()
    L.check(lib.trx_flat_build_instanced(_ptr(verts), _ptr(counts), counts.size, _ptr(io), _ptr(xf) if xf is not None else None,
                                         io.size, max_prims_per_leaf, threads, C.byref(fp)))
    return _take_flat(lib, fp)


def build_params(**fields):
    """trx_build_params with the reference's command-line defaults (src/main.rs:85-124), fields overridden by name."""
    lib = L.load()
    bp = L.BuildParams()
    lib.trx_build_params_default(C.byref(bp))
    for k, v in fields.items():
        if not hasattr(bp, k):
            raise AttributeError("BvhBuildParams has no field %r" % k)
        setattr(bp, k, v)
    return bp


def flat_build_params(verts, object_counts, params, use_tlas=False, threads=0):
    """cwbvh_gpu_runner's build half driven by a BvhBuildParams (src/main.rs:571-585) instead of process-wide knobs."""
    lib = L.load()
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
    counts = np.ascontiguousarray(object_counts if object_counts is not None else [verts.shape[0]], dtype=np.uint64)
    fp = C.POINTER(L.Flat)()
    L.check(lib.trx_flat_build_params(_ptr(verts), _ptr(counts), counts.size, 1 if use_tlas else 0, C.byref(params), threads,
                                      C.byref(fp)))
    return _take_flat(lib, fp)


def flat_build_preset_device(verts, object_counts, preset="medium_build", device=0, use_tlas=False, max_prims_per_leaf=3, threads=0):
    """A preset's build with every stage on the device (trx_flat_build_preset_device); device < 0: its host twin."""
    lib = L.load()
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
    counts = np.ascontiguousarray(object_counts if object_counts is not None else [verts.shape[0]], dtype=np.uint64)
    fp = C.POINTER(L.Flat)()
    L.check(lib.trx_flat_build_preset_device(_ptr(verts), _ptr(counts), counts.size, 1 if use_tlas else 0, preset.encode(),
                                             max_prims_per_leaf, threads, device, C.byref(fp)))
    return _take_flat(lib, fp)


def pack_tris_f16(tri_verts):
    """obvhs RtCompressedTriangle (24 B): v0 f32x3 + f16 edges, e2 in the low half (query.hlsl:75-85)."""
    v = np.ascontiguousarray(tri_verts, dtype=np.float32).reshape(-1, 9)
    e1 = (v[:, 3:6] - v[:, 0:3]).astype(np.float16).view(np.uint16).astype(np.uint32)
    e2 = (v[:, 6:9] - v[:, 0:3]).astype(np.float16).view(np.uint16).astype(np.uint32)
    out = np.empty((v.shape[0], 6), dtype=np.uint32)
    out[:, 0:3] = v[:, 0:3].view(np.uint32)
    out[:, 3:6] = e2 | (e1 << 16)
    return out


# ---- refit (host twin) ----------------------------------------------------------------

def record_order_verts(flat, object_verts):
    """Object-order vertices (what the build was given, [n, 9]) in the scene's triangle-record order: flat.tri_source
    names the input triangle of every record (pre-split references repeat theirs)."""
    return np.ascontiguousarray(np.asarray(object_verts, dtype=np.float32).reshape(-1, 9)[flat.tri_source])


def refit_nodes(flat, tri_verts, object_to_world=None, nodes=None):
    """trx_refit_nodes, the host twin of Scene.refit (no GPU): `nodes` (default flat.nodes) refitted over tri_verts
    (record order) with flat's instance table and entry nodes; object_to_world [n_instances, 16] or None.  Returns the
    new [n_nodes, 20] u32 buffer."""
    lib = L.load()
    src = np.ascontiguousarray(flat.nodes if nodes is None else nodes, dtype=np.uint32).reshape(-1, 20)
    v = np.ascontiguousarray(tri_verts, dtype=np.float32).reshape(-1, 9)
    inst = flat.instance_offsets
    entry = getattr(flat, "instance_entry", None)
    xf = None if object_to_world is None else np.ascontiguousarray(object_to_world, dtype=np.float32).reshape(-1, 16)
    out = np.empty_like(src)
    L.check(lib.trx_refit_nodes(_ptr(src), src.shape[0], _ptr(v), v.shape[0], _ptr(inst) if inst.size else None, inst.size,
                                flat.tlas_start, _ptr(entry) if entry is not None else None,
                                _ptr(xf) if xf is not None else None, _ptr(out)))
    return out


# ---- device scene ---------------------------------------------------------------------

class Scene:
    """Device-resident CWBVH scene (what rt_gpu_software::start uploads)."""

    def __init__(self, flat, device=0, tri_format=L.TRI_VERTS_36, tri_bytes=None):
        lib = L.load()
        self._lib = lib
        self._h = C.c_void_p()
        self.flat = flat
        nodes = flat.nodes
        if tri_bytes is None:
            tri_bytes = flat.tri_verts
        tri_bytes = np.ascontiguousarray(tri_bytes)
        inst = flat.instance_offsets
        L.check(lib.trx_scene_create(_ptr(nodes), flat.n_nodes, _ptr(tri_bytes), flat.n_tris, tri_format,
                                     _ptr(inst) if inst.size else None, inst.size, flat.tlas_start, device,
                                     C.byref(self._h)))
        if flat.blas_tri_start.size > 1:
            L.check(lib.trx_scene_set_geometry_ranges(self._h, _ptr(flat.blas_tri_start),
                                                      flat.blas_tri_start.size - 1))
        if getattr(flat, "instance_transforms", None) is not None:
            self.set_instance_transforms(flat.instance_transforms)
        if getattr(flat, "instance_entry", None) is not None:
            L.check(lib.trx_scene_set_instance_entry_nodes(self._h, _ptr(flat.instance_entry), flat.instance_entry.size))

    def set_instance_transforms(self, object_to_world):
        """Object-to-world 4x4 (column-major) per TLAS primitive; None restores identity."""
        if object_to_world is None:
            L.check(self._lib.trx_scene_set_instance_transforms(self._h, None, 0))
            return
        xf = np.ascontiguousarray(object_to_world, dtype=np.float32).reshape(-1, 16)
        L.check(self._lib.trx_scene_set_instance_transforms(self._h, _ptr(xf), xf.shape[0]))

    def instance_transform(self, instance_id):
        """Traversable::get_instance_transform (traversable/src/lib.rs:25-27): object-to-world, column-major."""
        m = np.zeros(16, dtype=np.float32)
        L.check(self._lib.trx_scene_get_instance_transform(self._h, instance_id, _ptr(m)))
        return m

    def instance_world_to_object(self):
        """[n_instances, 12] world-to-object rows exactly as the kernels use them."""
        n = self.flat.instance_offsets.size
        out = np.zeros((n, 12), dtype=np.float32)
        for k in range(n):
            L.check(self._lib.trx_scene_get_instance_world_to_object(self._h, k, _ptr(out[k])))
        return out

    def set_instance_masks(self, masks):
        """8-bit mask per TLAS primitive (uint8, n_instances), read by the *_masked calls only; None removes the table
        (every instance 0xFF).  Refused on single-level scenes."""
        if masks is None:
            L.check(self._lib.trx_scene_set_instance_masks(self._h, None, 0))
            return
        m = np.ascontiguousarray(masks, dtype=np.uint8).reshape(-1)
        L.check(self._lib.trx_scene_set_instance_masks(self._h, _ptr(m), m.size))

    def instance_masks(self):
        """The mask table as set, 0xFF everywhere when none is (single-level scenes: one instance)."""
        out = np.empty(max(self.flat.instance_offsets.size, 1), dtype=np.uint8)
        L.check(self._lib.trx_scene_get_instance_masks(self._h, _ptr(out), out.size))
        return out

    def set_materials(self, materials, tri_material):
        """trx_scene_set_materials: the material table ([n] MATERIAL_DTYPE, or [n, 6] floats: albedo rgb, emission rgb) and
        one uint16 index per triangle in `prim` order (the order of flat.tri_verts; a table in mesh order goes through
        flat.tri_source).  Validated on the host; replaces an earlier table after the scene's launches in flight."""
        m = np.ascontiguousarray(materials)
        if m.dtype != MATERIAL_DTYPE:
            m = np.ascontiguousarray(m, dtype=np.float32).reshape(-1, 6)
        idx = np.ascontiguousarray(tri_material, dtype=np.uint16).reshape(-1)
        L.check(self._lib.trx_scene_set_materials(self._h, _ptr(m), m.shape[0], _ptr(idx), idx.size))

    def get_materials(self):
        """(materials [n] MATERIAL_DTYPE, tri_material [n_tris] uint16) as set; refused on a scene without materials."""
        mats = np.zeros(L.MAX_MATERIALS, dtype=MATERIAL_DTYPE)
        idx = np.zeros(self.flat.tri_verts.shape[0], dtype=np.uint16)
        n = C.c_uint32(mats.size)
        L.check(self._lib.trx_scene_get_materials(self._h, _ptr(mats), C.byref(n), _ptr(idx), idx.size))
        return mats[:n.value].copy(), idx

    def set_vertex_normals(self, normals):
        """trx_scene_set_vertex_normals: nine floats per triangle ([n_tris, 9] f32: the object-space normals of vertices 0, 1,
        2) in `prim` order (the order of flat.tri_verts; normals in mesh order go through flat.tri_source); None removes the
        table.  Validated on the host; replaces an earlier table after the scene's launches in flight.  A refit keeps it."""
        if normals is None:
            L.check(self._lib.trx_scene_set_vertex_normals(self._h, None, 0))
            return
        nr = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 9)
        L.check(self._lib.trx_scene_set_vertex_normals(self._h, _ptr(nr), nr.shape[0]))

    def get_vertex_normals(self):
        """[n_tris, 9] f32 as set, bit for bit; refused on a scene without a table."""
        out = np.zeros((self.flat.tri_verts.shape[0], 9), dtype=np.float32)
        L.check(self._lib.trx_scene_get_vertex_normals(self._h, _ptr(out), out.shape[0]))
        return out

    def set_texcoords(self, uvs):
        """trx_scene_set_texcoords: six floats per triangle ([n_tris, 6] f32: s, t of vertices 0, 1, 2) in `prim` order (the
        order of flat.tri_verts; coordinates in mesh order go through flat.tri_source); None removes the table.  Any float is
        legal.  Replaces an earlier table after the scene's launches in flight.  A refit keeps it."""
        if uvs is None:
            L.check(self._lib.trx_scene_set_texcoords(self._h, None, 0))
            return
        uv = np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 6)
        L.check(self._lib.trx_scene_set_texcoords(self._h, _ptr(uv), uv.shape[0]))

    def get_texcoords(self):
        """[n_tris, 6] f32 as set, bit for bit; refused on a scene without a table."""
        out = np.zeros((self.flat.tri_verts.shape[0], 6), dtype=np.float32)
        L.check(self._lib.trx_scene_get_texcoords(self._h, _ptr(out), out.shape[0]))
        return out

    def set_textures(self, descs, texels, material_texture):
        """trx_scene_set_textures: descs ([n] TEXTURE_DESC_DTYPE, or [n, 4] integers: width, height, format, filter), the RGBA8
        words of all textures back to back (row 0 at t = 0), and one texture index or NO_TEXTURE per material; None for descs
        removes the set (trx_scene_remove_textures).  Validated on the host; needs materials."""
        if descs is None:
            L.check(self._lib.trx_scene_remove_textures(self._h))
            return
        d = np.ascontiguousarray(descs)
        if d.dtype != TEXTURE_DESC_DTYPE:
            d = np.ascontiguousarray(d, dtype=np.uint32).reshape(-1, 4)
        tx = np.ascontiguousarray(texels, dtype=np.uint32).reshape(-1)
        mt = np.ascontiguousarray(material_texture, dtype=np.uint32).reshape(-1)
        L.check(self._lib.trx_scene_set_textures(self._h, _ptr(d), d.shape[0], _ptr(tx), tx.size, _ptr(mt), mt.size))

    def get_textures(self):
        """(descs [n] TEXTURE_DESC_DTYPE, texels uint32, material_texture uint32) as set; refused on a scene without a set."""
        nt, nx, nm = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        one = np.zeros(4, dtype=np.uint32)
        rc = self._lib.trx_scene_get_textures(self._h, _ptr(one), C.byref(nt), _ptr(one), C.byref(nx), _ptr(one), C.byref(nm))
        if nt.value == 0:   # (no set: the refusal; otherwise the call above reported the counts and refused for room)
            L.check(rc)
        d = np.zeros(nt.value, dtype=TEXTURE_DESC_DTYPE)
        tx, mt = np.zeros(nx.value, dtype=np.uint32), np.zeros(nm.value, dtype=np.uint32)
        L.check(self._lib.trx_scene_get_textures(self._h, _ptr(d), C.byref(nt), _ptr(tx), C.byref(nx), _ptr(mt), C.byref(nm)))
        return d, tx, mt

    def refit(self, tri_verts):
        """New vertices for every triangle record, in record order ([n_tris, 9] f32; record_order_verts maps object-order
        vertices): trx_scene_refit for a numpy array, trx_scene_refit_dev on torch.cuda.current_stream() for a tensor on
        the GPU.  Nodes and records are rewritten in place, the topology kept (include/trx.h, "refit")."""
        n = self.flat.n_tris
        if hasattr(tri_verts, "data_ptr") and getattr(tri_verts, "is_cuda", False):
            import torch
            if tri_verts.dtype != torch.float32 or tri_verts.numel() != n * 9:
                raise L.TrxError(L.TRX_ERR_INVALID, "refit needs %d x 9 float32 vertices" % n)
            dev = self._lib.trx_scene_device(self._h)
            if tri_verts.device.index != dev:   # (the library refuses it too: the kernels read the tensor on the scene's device)
                raise L.TrxError(L.TRX_ERR_INVALID, "vertices on %s for a scene on device %d" % (tri_verts.device, dev))
            t = tri_verts.contiguous()
            L.check(self._lib.trx_scene_refit_dev(self._h, C.c_void_p(t.data_ptr()), n,
                                                  C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)))
            return
        v = np.ascontiguousarray(tri_verts, dtype=np.float32).reshape(-1, 9)
        L.check(self._lib.trx_scene_refit(self._h, _ptr(v), v.shape[0]))

    def info(self):
        """The scene's derived launch words (trx_debug_scene_info): exp_exact, scene_diag and the refit schedule's level count."""
        e, d, lv = C.c_uint32(), C.c_float(), C.c_uint32()
        L.check(self._lib.trx_debug_scene_info(self._h, C.byref(e), C.byref(d), C.byref(lv)))
        return {"exp_exact": e.value, "scene_diag": d.value, "refit_levels": lv.value}

    def walk_kind(self, mode):
        """L.WALK_PLAIN or L.WALK_PIPELINED: the walk the library launches for trace mode `mode` (L.MODE_PRIMARY, MODE_AO,
        MODE_RAYS, MODE_FUSED, MODE_SERVICE) on this scene (trx_debug_walk_kind)."""
        kind = self._lib.trx_debug_walk_kind(self._h, mode)
        if kind < 0:
            L.check(kind)
        return kind

    def schedule_state(self, kind, stream=0, order=True):
        """trx_debug_schedule_state: the scheduling state of the launch slot `stream` last used, for pass kind 0 (primary) or
        1 (AO), as a dict of the struct's fields - after waiting for the stream, changing nothing.  With `order`, the key
        "order" holds the tile ids of the set on file in the order a frame reads them (u32 array, empty without lists)."""
        st = L.ScheduleState()
        L.check(self._lib.trx_debug_schedule_state(self._h, C.c_void_p(stream), kind, C.byref(st), None, 0))
        out = {name: int(getattr(st, name)) for name, _ in L.ScheduleState._fields_}
        if order:
            # room for every entry the counts name (a stale or overflowed set is returned as it stands, cut at lpt_cap per list)
            ids = np.full(min(out["count_sum"], 128 * out["lpt_cap"]), 0xFFFFFFFF, dtype=np.uint32)
            if ids.size:
                L.check(self._lib.trx_debug_schedule_state(self._h, C.c_void_p(stream), kind, C.byref(st), _ptr(ids), ids.size))
            out["order"] = ids
        return out

    def read_nodes(self):
        """[n_nodes, 20] u32: the node buffer as the kernels now see it (trx_scene_read_nodes)."""
        out = np.empty((self.flat.n_nodes, 20), dtype=np.uint32)
        L.check(self._lib.trx_scene_read_nodes(self._h, _ptr(out), out.shape[0]))
        return out

    def close(self):
        if self._h:
            self._lib.trx_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def device_bytes(self):
        return self._lib.trx_scene_device_bytes(self._h)

    # host-buffer entry points -------------------------------------------------------
    def trace_primary(self, view, width, height, sem=L.SEM_HLSL):
        hits = np.empty(width * height, dtype=HIT_DTYPE)
        ms = C.c_float()
        L.check(self._lib.trx_trace_primary(self._h, C.byref(view), width, height, sem, _ptr(hits), C.byref(ms)))
        return hits, ms.value

    def trace_primary_ao(self, view, width, height, sem=L.SEM_HLSL, frame=0, ao_eps=0.01):
        prim = np.empty(width * height, dtype=HIT_DTYPE)
        ao = np.empty(width * height, dtype=HIT_DTYPE)
        ms = C.c_float()
        L.check(self._lib.trx_trace_primary_ao(self._h, C.byref(view), width, height, sem, frame, ao_eps, _ptr(prim),
                                               _ptr(ao), C.byref(ms)))
        return prim, ao, ms.value

    def frame_loop(self, view, width, height, sem=L.SEM_HLSL, frames=16, frame0=0, animate=True, ao_eps=0.01, overlap=False,
                   fetch=True):
        """The reference's frame loop, device-resident (trx_frame_loop): (total ms, last primary records, last AO records)."""
        prim = np.empty(width * height, dtype=HIT_DTYPE) if fetch else None
        ao = np.empty(width * height, dtype=HIT_DTYPE) if fetch else None
        ms = C.c_float()
        L.check(self._lib.trx_frame_loop(self._h, C.byref(view), width, height, sem, frame0, 1 if animate else 0, ao_eps, frames,
                                         int(overlap), _ptr(prim) if fetch else None, _ptr(ao) if fetch else None, C.byref(ms)))
        return ms.value, prim, ao

    def trace_primary_ao_inst(self, view, width, height, sem=L.SEM_HLSL, frame=0, ao_eps=0.01):
        """(primary, primary instance ids, ao, ao instance ids, ms): RayHit.instance_id beside every hit."""
        n = width * height
        prim, ao = np.empty(n, dtype=HIT_DTYPE), np.empty(n, dtype=HIT_DTYPE)
        pi, ai = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        ms = C.c_float()
        L.check(self._lib.trx_trace_primary_ao_inst(self._h, C.byref(view), width, height, sem, frame, ao_eps, _ptr(prim),
                                                    _ptr(pi), _ptr(ao), _ptr(ai), C.byref(ms)))
        return prim, pi, ao, ai, ms.value

    def trace_rays_inst(self, rays, sem=L.SEM_HLSL):
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.empty(rays.shape[0], dtype=HIT_DTYPE)
        inst = np.empty(rays.shape[0], dtype=np.uint32)
        ms = C.c_float()
        L.check(self._lib.trx_trace_rays_inst(self._h, _ptr(rays), rays.shape[0], sem, _ptr(hits), _ptr(inst), C.byref(ms)))
        return hits, inst, ms.value

    def trace_rays_attr(self, rays, sem=L.SEM_HLSL):
        """(hits, instance ids, hit attributes): trx_trace_rays_attr, the trace and the attribute pass over its hits."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        n = rays.shape[0]
        hits, inst, attr = np.empty(n, dtype=HIT_DTYPE), np.empty(n, dtype=np.uint32), np.empty(n, dtype=HIT_ATTR_DTYPE)
        ms = C.c_float()
        L.check(self._lib.trx_trace_rays_attr(self._h, _ptr(rays), n, sem, _ptr(hits), _ptr(inst), _ptr(attr), C.byref(ms)))
        return hits, inst, attr

    def trace_rays_masked(self, rays, ray_mask, sem=L.SEM_HLSL):
        """(hits, instance ids, ms) of a masked trace: instance k is entered only if its mask & ray_mask != 0."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.empty(rays.shape[0], dtype=HIT_DTYPE)
        inst = np.empty(rays.shape[0], dtype=np.uint32)
        ms = C.c_float()
        L.check(self._lib.trx_trace_rays_masked(self._h, _ptr(rays), rays.shape[0], sem, ray_mask, _ptr(hits), _ptr(inst),
                                                C.byref(ms)))
        return hits, inst, ms.value

    def trace_occluded_masked(self, rays, ray_mask, sem=L.SEM_HLSL):
        """(uint8 flags, ms): trace_occluded over the instances ray_mask sees."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        flags = np.empty(rays.shape[0], dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_trace_occluded_masked(self._h, _ptr(rays), rays.shape[0], sem, ray_mask, _ptr(flags),
                                                    C.byref(ms)))
        return flags, ms.value

    def trace_rays(self, rays, sem=L.SEM_HLSL):
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.empty(rays.shape[0], dtype=HIT_DTYPE)
        ms = C.c_float()
        L.check(self._lib.trx_trace_rays(self._h, _ptr(rays), rays.shape[0], sem, _ptr(hits), C.byref(ms)))
        return hits, ms.value

    def trace_occluded(self, rays, sem=L.SEM_HLSL):
        """intersects_bl_bvh (query.hlsl:440-445) for a batch: uint8 flags, 1 = something is hit."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        flags = np.empty(rays.shape[0], dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_trace_occluded(self._h, _ptr(rays), rays.shape[0], sem, _ptr(flags), C.byref(ms)))
        return flags, ms.value

    def trace_ao_visibility(self, view, width, height, n_samples, ao_radius, sem=L.SEM_HLSL, frame0=0, ao_eps=0.01):
        """(uint8 counts [width * height], ms): the primary pass and the AO visibility pass over it (trx_trace_ao_visibility) -
        per surface pixel how many of n_samples AO rays of length ao_radius (float('inf') allowed) reach nothing,
        L.AO_NO_SURFACE where the primary ray missed."""
        counts = np.empty(width * height, dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_trace_ao_visibility(self._h, C.byref(view), width, height, sem, frame0, n_samples, ao_eps,
                                                  ao_radius, _ptr(counts), C.byref(ms)))
        return counts, ms.value

    def render_image(self, view, width, height, sem=L.SEM_HLSL, frame0=0, n_samples=0, ao_eps=0.01, ao_radius=float("inf"),
                     filter_radius=0, depth_tol=0.02, normal_cos=0.9):
        """(uint8 image [height, width, 4], ms): trx_render_image - the frame traced, its AO term optionally filtered, and
        shaded to RGBA8 on the device; only the image crosses the bus.  n_samples == 0: the reference's image (closest-hit AO
        pass under seed frame0); n_samples >= 1: the AO visibility pass's counts / n_samples, through the edge-aware
        filter (with normals) when filter_radius >= 1."""
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_render_image(self._h, C.byref(view), width, height, sem, frame0, n_samples, ao_eps, ao_radius,
                                           filter_radius, depth_tol, normal_cos, _ptr(rgba), C.byref(ms)))
        return rgba, ms.value

    def render_image_sparse(self, view, width, height, n_samples, ao_stride, ao_phase=0, upsample_radius=1, sem=L.SEM_HLSL, frame0=0,
                            ao_eps=0.01, ao_radius=float("inf"), depth_tol=0.02, normal_cos=0.9):
        """(uint8 image [height, width, 4], ms): trx_render_image_sparse - the AO visibility pass at one pixel in every
        ao_stride x ao_stride block (the pixel ao_phase names), the full-resolution term rebuilt by the edge-aware upsample of
        upsample_radius low cells (with normals), shaded to RGBA8 on the device; only the image crosses the bus."""
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_render_image_sparse(self._h, C.byref(view), width, height, sem, frame0, n_samples, ao_eps, ao_radius,
                                                  ao_stride, ao_phase, upsample_radius, depth_tol, normal_cos, _ptr(rgba), C.byref(ms)))
        return rgba, ms.value

    def render_image_lit(self, view, width, height, lights, sem=L.SEM_HLSL, ray_mask=0, frame0=0, light_samples=1, shadow_eps=0.01,
                         ambient=0.0, ao_samples=0, ao_eps=0.01, ao_radius=float("inf"), filter_radius=0, depth_tol=0.02, normal_cos=0.9):
        """(uint8 image [height, width, 4], ms): trx_render_image_lit - the frame traced, shadow rays toward every light
        (masked by ray_mask when it is not 0), the light term (ambient, scaled by the filtered AO term when ao_samples >= 1,
        plus every light's analytic term times its visibility) shaded to RGBA8 on the device; only the image crosses the bus."""
        arr = light_array(lights)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_render_image_lit(self._h, C.byref(view), width, height, sem, ray_mask, arr, len(arr), frame0, light_samples,
                                               shadow_eps, ambient, ao_samples, ao_eps, ao_radius, filter_radius, depth_tol, normal_cos,
                                               _ptr(rgba), C.byref(ms)))
        return rgba, ms.value

    def render_image_gi(self, view, width, height, lights, bounce_samples, bounce_eps=0.01, bounce_albedo=0.5, sem=L.SEM_HLSL, ray_mask=0,
                        frame0=0, light_samples=1, shadow_eps=0.01, ambient=0.0, ao_samples=0, ao_eps=0.01, ao_radius=float("inf"),
                        filter_radius=0, depth_tol=0.02, normal_cos=0.9):
        """(uint8 image [height, width, 4], ms): trx_render_image_gi - render_image_lit's passes up to the light term, one
        diffuse bounce of bounce_samples rays per pixel added to it (trace_indirect_dev), the value shade; only the image
        crosses the bus."""
        arr = light_array(lights)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_render_image_gi(self._h, C.byref(view), width, height, sem, ray_mask, arr, len(arr), frame0, light_samples,
                                              shadow_eps, ambient, ao_samples, ao_eps, ao_radius, filter_radius, depth_tol, normal_cos,
                                              bounce_samples, bounce_eps, bounce_albedo, _ptr(rgba), C.byref(ms)))
        return rgba, ms.value

    def render_image_gi_filtered(self, view, width, height, lights, bounce_samples, bounce_filter_levels, bounce_depth_tol=0.1,
                                 bounce_normal_cos=0.9, bounce_eps=0.01, bounce_albedo=0.5, sem=L.SEM_HLSL, ray_mask=0, frame0=0,
                                 light_samples=1, shadow_eps=0.01, ambient=0.0, ao_samples=0, ao_eps=0.01, ao_radius=float("inf"),
                                 filter_radius=0, depth_tol=0.02, normal_cos=0.9):
        """(uint8 image [height, width, 4], ms): trx_render_image_gi_filtered - render_image_gi with the indirect term put
        through bounce_filter_levels (0..5; 0: render_image_gi itself) levels of the value filter (value_filter_dev, with the
        attribute pass's normals) before it is added to the light term; only the image crosses the bus."""
        arr = light_array(lights)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_render_image_gi_filtered(self._h, C.byref(view), width, height, sem, ray_mask, arr, len(arr), frame0,
                                                       light_samples, shadow_eps, ambient, ao_samples, ao_eps, ao_radius, filter_radius,
                                                       depth_tol, normal_cos, bounce_samples, bounce_eps, bounce_albedo,
                                                       bounce_filter_levels, bounce_depth_tol, bounce_normal_cos, _ptr(rgba), C.byref(ms)))
        return rgba, ms.value

    def render_image_gi_sparse(self, view, width, height, lights, bounce_samples, bounce_stride, bounce_phase=0, bounce_upsample_radius=1,
                               bounce_filter_levels=0, bounce_depth_tol=0.1, bounce_normal_cos=0.9, bounce_eps=0.01, bounce_albedo=0.5,
                               sem=L.SEM_HLSL, ray_mask=0, frame0=0, light_samples=1, shadow_eps=0.01, ambient=0.0, ao_samples=0, ao_eps=0.01,
                               ao_radius=float("inf"), filter_radius=0, depth_tol=0.02, normal_cos=0.9):
        """(uint8 image [height, width, 4], ms): trx_render_image_gi_sparse - render_image_gi_filtered with the indirect term
        traced at one pixel of every bounce_stride x bounce_stride block (the pixel bounce_phase names;
        trace_indirect_sparse_dev) and rebuilt at full resolution by the edge-aware upsample of bounce_upsample_radius low
        cells (value_upsample_dev, with the attribute pass's normals) before the filter; only the image crosses the bus."""
        arr = light_array(lights)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_render_image_gi_sparse(self._h, C.byref(view), width, height, sem, ray_mask, arr, len(arr), frame0,
                                                     light_samples, shadow_eps, ambient, ao_samples, ao_eps, ao_radius, filter_radius,
                                                     depth_tol, normal_cos, bounce_samples, bounce_eps, bounce_albedo,
                                                     bounce_filter_levels, bounce_depth_tol, bounce_normal_cos, bounce_stride,
                                                     bounce_phase, bounce_upsample_radius, _ptr(rgba), C.byref(ms)))
        return rgba, ms.value

    def render_image_colour(self, view, width, height, lights, bounce_samples=0, bounce_stride=1, bounce_phase=0, bounce_upsample_radius=1,
                            bounce_filter_levels=0, bounce_depth_tol=0.1, bounce_normal_cos=0.9, bounce_eps=0.01, sem=L.SEM_HLSL, ray_mask=0,
                            frame0=0, light_samples=1, shadow_eps=0.01, ambient=0.0, ao_samples=0, ao_eps=0.01, ao_radius=float("inf"),
                            filter_radius=0, depth_tol=0.02, normal_cos=0.9):
        """(uint8 image [height, width, 4], ms): trx_render_image_colour - render_image_gi_sparse in colour on a scene with
        materials: the lit chain up to the light term, the RGB indirect pass (trace_indirect_rgb_dev at bounce_stride 1,
        trace_indirect_rgb_sparse_dev above it; none with bounce_samples 0), per plane the upsample (bounce_stride > 1) and
        the value filter (bounce_filter_levels >= 1), material_compose_dev and shade_rgb_dev; only the image crosses the bus."""
        arr = light_array(lights)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_render_image_colour(self._h, C.byref(view), width, height, sem, ray_mask, arr, len(arr), frame0, light_samples,
                                                  shadow_eps, ambient, ao_samples, ao_eps, ao_radius, filter_radius, depth_tol, normal_cos,
                                                  bounce_samples, bounce_eps, bounce_filter_levels, bounce_depth_tol, bounce_normal_cos,
                                                  bounce_stride, bounce_phase, bounce_upsample_radius, _ptr(rgba), C.byref(ms)))
        return rgba, ms.value

    def render_image_lit_smooth(self, view, width, height, lights, sem=L.SEM_HLSL, ray_mask=0, frame0=0, light_samples=1, shadow_eps=0.01,
                                ambient=0.0, ao_samples=0, ao_eps=0.01, ao_radius=float("inf"), filter_radius=0, depth_tol=0.02,
                                normal_cos=0.9):
        """(uint8 image [height, width, 4], ms): trx_render_image_lit_smooth - render_image_lit with the shading-normal pass
        after the attribute pass: the light term and the AO filter read the interpolated vertex normals (set_vertex_normals),
        every ray is still built from the geometric normal."""
        arr = light_array(lights)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_render_image_lit_smooth(self._h, C.byref(view), width, height, sem, ray_mask, arr, len(arr), frame0,
                                                      light_samples, shadow_eps, ambient, ao_samples, ao_eps, ao_radius, filter_radius,
                                                      depth_tol, normal_cos, _ptr(rgba), C.byref(ms)))
        return rgba, ms.value

    def render_image_colour_smooth(self, view, width, height, lights, bounce_samples=0, bounce_stride=1, bounce_phase=0,
                                   bounce_upsample_radius=1, bounce_filter_levels=0, bounce_depth_tol=0.1, bounce_normal_cos=0.9,
                                   bounce_eps=0.01, sem=L.SEM_HLSL, ray_mask=0, frame0=0, light_samples=1, shadow_eps=0.01, ambient=0.0,
                                   ao_samples=0, ao_eps=0.01, ao_radius=float("inf"), filter_radius=0, depth_tol=0.02, normal_cos=0.9):
        """(uint8 image [height, width, 4], ms): trx_render_image_colour_smooth - render_image_colour with the shading-normal
        pass after the attribute pass (the light term, the filters and the upsample read the interpolated vertex normals)."""
        arr = light_array(lights)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_render_image_colour_smooth(self._h, C.byref(view), width, height, sem, ray_mask, arr, len(arr), frame0,
                                                         light_samples, shadow_eps, ambient, ao_samples, ao_eps, ao_radius, filter_radius,
                                                         depth_tol, normal_cos, bounce_samples, bounce_eps, bounce_filter_levels,
                                                         bounce_depth_tol, bounce_normal_cos, bounce_stride, bounce_phase,
                                                         bounce_upsample_radius, _ptr(rgba), C.byref(ms)))
        return rgba, ms.value

    def render_image_colour_emitters(self, view, width, height, lights=(), emitter_samples=4, emitter_eps=0.001, bounce_samples=0,
                                     bounce_stride=1, bounce_phase=0, bounce_upsample_radius=1, bounce_filter_levels=0, bounce_depth_tol=0.1,
                                     bounce_normal_cos=0.9, bounce_eps=0.01, sem=L.SEM_HLSL, ray_mask=0, frame0=0, light_samples=1,
                                     shadow_eps=0.01, ambient=0.0, ao_samples=0, ao_eps=0.01, ao_radius=float("inf"), filter_radius=0,
                                     depth_tol=0.02, normal_cos=0.9):
        """(uint8 image [height, width, 4], ms): trx_render_image_colour_emitters - render_image_colour with the scene's
        emissive triangles sampled as lights: the indirect pass in its emitter mode, then trace_emitter_light_dev at full
        resolution over the (filtered) planes, then compose and shade.  `lights` may be empty; the emitter table is built if
        the scene has none or a stale one."""
        arr = light_array(lights)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_render_image_colour_emitters(self._h, C.byref(view), width, height, sem, ray_mask, arr if len(arr) else None,
                                                           len(arr), frame0, light_samples, shadow_eps, ambient, ao_samples, ao_eps, ao_radius,
                                                           filter_radius, depth_tol, normal_cos, bounce_samples, bounce_eps,
                                                           bounce_filter_levels, bounce_depth_tol, bounce_normal_cos, bounce_stride,
                                                           bounce_phase, bounce_upsample_radius, emitter_samples, emitter_eps, _ptr(rgba),
                                                           C.byref(ms)))
        return rgba, ms.value

    def render_image_colour_textured(self, view, width, height, lights=(), emitter_samples=0, emitter_eps=0.001, smooth=False,
                                     bounce_samples=0, bounce_stride=1, bounce_phase=0, bounce_upsample_radius=1, bounce_filter_levels=0,
                                     bounce_depth_tol=0.1, bounce_normal_cos=0.9, bounce_eps=0.01, sem=L.SEM_HLSL, ray_mask=0, frame0=0,
                                     light_samples=1, shadow_eps=0.01, ambient=0.0, ao_samples=0, ao_eps=0.01, ao_radius=float("inf"),
                                     filter_radius=0, depth_tol=0.02, normal_cos=0.9):
        """(uint8 image [height, width, 4], ms): trx_render_image_colour_textured - render_image_colour (emitter_samples 0),
        render_image_colour_emitters (emitter_samples >= 1) and, with smooth, the shading-normal pass, with the textured
        albedo: surface_albedo_dev after the attribute pass, trace_indirect_rgb_textured_dev, albedo_compose_dev."""
        arr = light_array(lights)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        ms = C.c_float()
        L.check(self._lib.trx_render_image_colour_textured(self._h, C.byref(view), width, height, sem, ray_mask, arr if len(arr) else None,
                                                           len(arr), frame0, light_samples, shadow_eps, ambient, ao_samples, ao_eps, ao_radius,
                                                           filter_radius, depth_tol, normal_cos, bounce_samples, bounce_eps,
                                                           bounce_filter_levels, bounce_depth_tol, bounce_normal_cos, bounce_stride,
                                                           bounce_phase, bounce_upsample_radius, emitter_samples, emitter_eps,
                                                           1 if smooth else 0, _ptr(rgba), C.byref(ms)))
        return rgba, ms.value

    def render_heat_image(self, view, width, height, which=L.HEAT_NODES, scale=None, sem=L.SEM_HLSL):
        """(uint8 image [height, width, 4], Stats): trx_render_heat_image - the counted primary pass and the PROFILE_RT heat map
        of its per-ray counts (which: L.HEAT_NODES or L.HEAT_TRIS; scale None: the reference's, 0.002 / 0.01); only the image
        crosses the bus."""
        if scale is None:
            scale = L.HEAT_SCALE_TRIS if which == L.HEAT_TRIS else L.HEAT_SCALE_NODES
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        st = L.Stats()
        L.check(self._lib.trx_render_heat_image(self._h, C.byref(view), width, height, sem, which, scale, _ptr(rgba), C.byref(st)))
        return rgba, st

    def traverse(self, origin, direction, tmin=0.0, tmax=3.4028234663852886e38, sem=L.SEM_HLSL):
        """Traversable::traverse (traversable/src/lib.rs:17-21) for one ray."""
        ray = L.Ray((C.c_float * 3)(*origin), tmin, (C.c_float * 3)(*direction), tmax)
        out = L.RayHit()
        L.check(self._lib.trx_traverse1(self._h, C.byref(ray), sem, C.byref(out)))
        return out

    def traverse_threads(self, rays, threads=16, sem=L.SEM_HLSL):
        """The reference's CPU pixel loop over the literal traverse (src/rt_cpu/rt_cpu.rs:35-57): `threads` host threads
        (native ones, inside the library: trx_debug_traverse1_threads), thread k calls trx_traverse1 for rays k,
        k + threads, ...  Returns (RAYHIT_DTYPE array, seconds, launches the calls shared)."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        out = np.zeros(rays.shape[0], dtype=RAYHIT_DTYPE)
        secs, launches = C.c_double(), C.c_uint64()
        L.check(self._lib.trx_debug_traverse1_threads(self._h, _ptr(rays), rays.shape[0], threads, sem, _ptr(out),
                                                      C.byref(secs), C.byref(launches)))
        return out, secs.value, int(launches.value)

    def service_stats(self):
        """The scene's ray services so far (trx_debug_service_stats): dict of rays, starts, us_per_call, gpu_us_per_call, trips_per_call."""
        v = [C.c_uint64() for _ in range(5)]
        L.check(self._lib.trx_debug_service_stats(self._h, *[C.byref(x) for x in v]))
        n = max(v[0].value, 1)
        return {"rays": v[0].value, "starts": v[1].value, "us_per_call": v[2].value / n * 1e-3, "gpu_us_per_call": v[3].value / n * 1e-2,
                "trips_per_call": v[4].value / n}

    def traverse_batch(self, rays, sem=L.SEM_HLSL):
        """Traversable::traverse for a whole batch in one launch: (RAYHIT_DTYPE array, ms)."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        out = np.empty(rays.shape[0], dtype=RAYHIT_DTYPE)
        ms = C.c_float()
        L.check(self._lib.trx_traverse_batch(self._h, _ptr(rays), rays.shape[0], sem, _ptr(out), C.byref(ms)))
        return out, ms.value

    def count_ao(self, view, width, height, d_primary, d_ao, sem=L.SEM_HLSL, frame=0, ao_eps=0.01, shard=(0, 1)):
        """Node steps / triangle tests of one AO pass over device-resident primary hits (counting kernel)."""
        st = L.Stats()
        L.check(self._lib.trx_count_ao(self._h, C.byref(view), width, height, L.Shard(*shard), sem, frame, ao_eps,
                                       C.c_void_p(d_primary), C.c_void_p(d_ao), C.byref(st)))
        return st

    def count_rays(self, d_rays, n, d_hits, sem=L.SEM_HLSL):
        """Node steps / triangle tests of one explicit-ray batch (counting kernel)."""
        st = L.Stats()
        L.check(self._lib.trx_count_rays(self._h, C.c_void_p(d_rays), n, sem, C.c_void_p(d_hits), C.byref(st)))
        return st

    def count_primary_per_ray(self, view, width, height, d_cost, d_hits=0, sem=L.SEM_HLSL, shard=(0, 1)):
        """trx_count_primary_per_ray: count_primary, and one RAY_COST_DTYPE record per pixel at d_cost, laid out by the shard like
        the hit buffer (d_hits 0: the hit records go to the scene's scratch)."""
        st = L.Stats()
        L.check(self._lib.trx_count_primary_per_ray(self._h, C.byref(view), width, height, L.Shard(*shard), sem, C.c_void_p(d_hits),
                                                    C.c_void_p(d_cost), C.byref(st)))
        return st

    def count_ao_per_ray(self, view, width, height, d_primary, d_cost, d_ao=0, sem=L.SEM_HLSL, frame=0, ao_eps=0.01, shard=(0, 1)):
        """trx_count_ao_per_ray: count_ao, and one RAY_COST_DTYPE record per AO ray at d_cost ({0, 0} where the primary record
        is a miss)."""
        st = L.Stats()
        L.check(self._lib.trx_count_ao_per_ray(self._h, C.byref(view), width, height, L.Shard(*shard), sem, frame, ao_eps,
                                               C.c_void_p(d_primary), C.c_void_p(d_ao), C.c_void_p(d_cost), C.byref(st)))
        return st

    def count_rays_per_ray(self, d_rays, n, d_cost, d_hits=0, sem=L.SEM_HLSL):
        """trx_count_rays_per_ray: count_rays, and one RAY_COST_DTYPE record per ray at d_cost."""
        st = L.Stats()
        L.check(self._lib.trx_count_rays_per_ray(self._h, C.c_void_p(d_rays), n, sem, C.c_void_p(d_hits), C.c_void_p(d_cost),
                                                 C.byref(st)))
        return st

    def fetch_rate(self, tris_per_node=0.0, steps=400):
        """Measured ceiling of the node-fetch loop on this scene's buffers (trx_debug_fetch_rate): random 80-byte nodes
        and, tris_per_node per node on average, random 48-byte triangle records per second, nothing else running."""
        nps, tps = C.c_double(), C.c_double()
        L.check(self._lib.trx_debug_fetch_rate(self._h, steps, int(round(tris_per_node * 256)), C.byref(nps), C.byref(tps)))
        return nps.value, tps.value

    def count_primary(self, view, width, height, sem=L.SEM_HLSL, shard=(0, 1)):
        st = L.Stats()
        L.check(self._lib.trx_count_primary(self._h, C.byref(view), width, height, L.Shard(*shard), sem, None,
                                            C.byref(st)))
        return st

    def footprint(self, view, width, height, sem=L.SEM_HLSL):
        """(distinct nodes fetched, distinct triangles tested) by one primary frame."""
        n, t = C.c_uint64(), C.c_uint64()
        L.check(self._lib.trx_debug_footprint(self._h, C.byref(view), width, height, sem, C.byref(n), C.byref(t)))
        return n.value, t.value

    def bench_primary(self, view, width, height, sem=L.SEM_HLSL, warmup=1, frames=20):
        mn, mean = C.c_float(), C.c_float()
        L.check(self._lib.trx_bench_primary(self._h, C.byref(view), width, height, sem, warmup, frames, C.byref(mn),
                                            C.byref(mean)))
        return mn.value, mean.value

    # device-resident entry points (pointers are ints: tensor.data_ptr(), stream.cuda_stream) ----
    def trace_primary_dev(self, view, width, height, d_hits, sem=L.SEM_HLSL, shard=(0, 1), stream=0):
        L.check(self._lib.trx_trace_primary_dev(self._h, C.byref(view), width, height, L.Shard(*shard), sem,
                                                C.c_void_p(d_hits), C.c_void_p(stream)))

    def trace_primary_batch_dev(self, views, width, height, d_hits, frame_stride, sem=L.SEM_HLSL, shard=(0, 1),
                                stream=0):
        """len(views) frames (1..8) in one launch; frame f lands at d_hits + f*frame_stride records."""
        arr = (L.View * len(views))(*views)
        L.check(self._lib.trx_trace_primary_batch_dev(self._h, arr, len(views), width, height, L.Shard(*shard), sem,
                                                      C.c_void_p(d_hits), frame_stride, C.c_void_p(stream)))

    def trace_ao_dev(self, view, width, height, d_primary, d_ao, sem=L.SEM_HLSL, frame=0, ao_eps=0.01,
                     shard=(0, 1), stream=0):
        L.check(self._lib.trx_trace_ao_dev(self._h, C.byref(view), width, height, L.Shard(*shard), sem, frame, ao_eps,
                                           C.c_void_p(d_primary), C.c_void_p(d_ao), C.c_void_p(stream)))

    def trace_frame_dev(self, view, width, height, d_primary, d_ao, sem=L.SEM_HLSL, frame=0, ao_eps=0.01, shard=(0, 1),
                        stream=0, d_primary_inst=0, d_ao_inst=0):
        """Primary + AO of one frame in ONE launch (the reference's single dispatch)."""
        L.check(self._lib.trx_trace_frame_dev(self._h, C.byref(view), width, height, L.Shard(*shard), sem, frame, ao_eps,
                                              C.c_void_p(d_primary), C.c_void_p(d_primary_inst), C.c_void_p(d_ao),
                                              C.c_void_p(d_ao_inst), C.c_void_p(stream)))

    def trace_ao_batch_dev(self, view, width, height, d_primary, d_ao, frame_stride, n_frames, sem=L.SEM_HLSL, frame0=0,
                           ao_eps=0.01, shard=(0, 1), stream=0, d_primary_inst=0, d_ao_inst=0):
        """n_frames AO passes (seeds frame0 ..) over one view and one primary hit buffer in ONE launch."""
        L.check(self._lib.trx_trace_ao_batch_dev(self._h, C.byref(view), width, height, L.Shard(*shard), sem, frame0, n_frames,
                                                 ao_eps, C.c_void_p(d_primary), C.c_void_p(d_primary_inst), C.c_void_p(d_ao),
                                                 C.c_void_p(d_ao_inst), frame_stride, C.c_void_p(stream)))

    def trace_rays_dev(self, d_rays, n, d_hits, sem=L.SEM_HLSL, stream=0):
        L.check(self._lib.trx_trace_rays_dev(self._h, C.c_void_p(d_rays), n, sem, C.c_void_p(d_hits),
                                             C.c_void_p(stream)))

    def trace_rays_inst_dev(self, d_rays, n, d_hits, d_inst=0, sem=L.SEM_HLSL, stream=0):
        """trx_trace_rays_inst_dev: trace_rays_dev with the instance id of every hit at d_inst (n u32; 0: not wanted)."""
        L.check(self._lib.trx_trace_rays_inst_dev(self._h, C.c_void_p(d_rays), n, sem, C.c_void_p(d_hits), C.c_void_p(d_inst),
                                                  C.c_void_p(stream)))

    def trace_occluded_dev(self, d_rays, n, d_flags, sem=L.SEM_HLSL, stream=0):
        L.check(self._lib.trx_trace_occluded_dev(self._h, C.c_void_p(d_rays), n, sem, C.c_void_p(d_flags),
                                                 C.c_void_p(stream)))

    def trace_rays_masked_dev(self, d_rays, n, d_hits, ray_mask, sem=L.SEM_HLSL, d_inst=0, stream=0):
        L.check(self._lib.trx_trace_rays_masked_dev(self._h, C.c_void_p(d_rays), n, sem, ray_mask, C.c_void_p(d_hits),
                                                    C.c_void_p(d_inst), C.c_void_p(stream)))

    def trace_occluded_masked_dev(self, d_rays, n, d_flags, ray_mask, sem=L.SEM_HLSL, stream=0):
        L.check(self._lib.trx_trace_occluded_masked_dev(self._h, C.c_void_p(d_rays), n, sem, ray_mask, C.c_void_p(d_flags),
                                                        C.c_void_p(stream)))

    def trace_primary_masked_dev(self, view, width, height, d_hits, ray_mask, sem=L.SEM_HLSL, d_inst=0, shard=(0, 1),
                                 stream=0):
        L.check(self._lib.trx_trace_primary_masked_dev(self._h, C.byref(view), width, height, L.Shard(*shard), sem, ray_mask,
                                                       C.c_void_p(d_hits), C.c_void_p(d_inst), C.c_void_p(stream)))

    def trace_ao_masked_dev(self, view, width, height, d_primary, d_ao, ray_mask, sem=L.SEM_HLSL, frame=0, ao_eps=0.01,
                            d_primary_inst=0, d_ao_inst=0, shard=(0, 1), stream=0):
        L.check(self._lib.trx_trace_ao_masked_dev(self._h, C.byref(view), width, height, L.Shard(*shard), sem, frame, ao_eps,
                                                  ray_mask, C.c_void_p(d_primary), C.c_void_p(d_primary_inst),
                                                  C.c_void_p(d_ao), C.c_void_p(d_ao_inst), C.c_void_p(stream)))

    def ao_rays_dev(self, view, width, height, d_primary, d_rays, ao_radius, frame=0, ao_eps=0.01, d_primary_inst=0,
                    shard=(0, 1), stream=0):
        """trx_ao_rays_dev: the AO pass's rays for seed `frame` as explicit rays at d_rays, one per record laid out like the
        hit buffers of `shard`; the inert ray (tmax = -1) where the primary record is a miss."""
        L.check(self._lib.trx_ao_rays_dev(self._h, C.byref(view), width, height, L.Shard(*shard), frame, ao_eps, ao_radius,
                                          C.c_void_p(d_primary), C.c_void_p(d_primary_inst), C.c_void_p(d_rays),
                                          C.c_void_p(stream)))

    def trace_ao_visibility_dev(self, view, width, height, d_primary, d_unoccluded, n_samples, ao_radius, sem=L.SEM_HLSL,
                                frame0=0, ao_eps=0.01, d_primary_inst=0, shard=(0, 1), stream=0):
        """trx_trace_ao_visibility_dev: one byte per record at d_unoccluded - the number of the n_samples AO rays (seeds
        frame0 ..) that are not occluded within ao_radius, L.AO_NO_SURFACE where the primary record is a miss."""
        L.check(self._lib.trx_trace_ao_visibility_dev(self._h, C.byref(view), width, height, L.Shard(*shard), sem, frame0,
                                                      n_samples, ao_eps, ao_radius, C.c_void_p(d_primary),
                                                      C.c_void_p(d_primary_inst), C.c_void_p(d_unoccluded),
                                                      C.c_void_p(stream)))

    def trace_ao_visibility_sparse_dev(self, view, width, height, stride, phase, d_primary, d_unoccluded_lo, n_samples, ao_radius,
                                       sem=L.SEM_HLSL, frame0=0, ao_eps=0.01, d_primary_inst=0, stream=0):
        """trx_trace_ao_visibility_sparse_dev: the visibility pass at pixel (X * stride + phase % stride, Y * stride + phase //
        stride) of every cell (X, Y) of the ceil(width / stride) x ceil(height / stride) low grid, one byte per cell at
        d_unoccluded_lo - that pixel's byte of trx_trace_ao_visibility_dev, L.AO_NO_SURFACE where the pixel leaves the image.
        d_primary / d_primary_inst are whole-image, image-layout, full-resolution records."""
        L.check(self._lib.trx_trace_ao_visibility_sparse_dev(self._h, C.byref(view), width, height, stride, phase, sem, frame0,
                                                             n_samples, ao_eps, ao_radius, C.c_void_p(d_primary),
                                                             C.c_void_p(d_primary_inst), C.c_void_p(d_unoccluded_lo),
                                                             C.c_void_p(stream)))

    def light_rays_dev(self, view, width, height, light, d_primary, d_rays, light_index=0, frame0=0, sample=0, shadow_eps=0.01,
                       d_primary_inst=0, shard=(0, 1), stream=0):
        """trx_light_rays_dev: the shadow rays toward `light` (an L.Light; its index among the pass's lights and the sample
        pick a rect light's seed) as explicit rays at d_rays, one per record laid out like the hit buffers of `shard`; the
        inert ray (tmax = -1) where there is no surface or the surface faces away."""
        L.check(self._lib.trx_light_rays_dev(self._h, C.byref(view), width, height, L.Shard(*shard), C.byref(light), light_index,
                                             frame0, sample, shadow_eps, C.c_void_p(d_primary), C.c_void_p(d_primary_inst),
                                             C.c_void_p(d_rays), C.c_void_p(stream)))

    def trace_light_visibility_dev(self, view, width, height, lights, d_primary, d_lit, n_samples=1, sem=L.SEM_HLSL, ray_mask=0,
                                   frame0=0, shadow_eps=0.01, d_primary_inst=0, shard=(0, 1), stream=0):
        """trx_trace_light_visibility_dev: one plane of one byte per record per light at d_lit - the samples (n_samples for a
        rect light, one otherwise) whose shadow ray was cast and not occluded, L.AO_NO_SURFACE where there is no surface.
        ray_mask 1..255: instances whose mask shares no bit with it cast no shadow."""
        arr = light_array(lights)
        L.check(self._lib.trx_trace_light_visibility_dev(self._h, C.byref(view), width, height, L.Shard(*shard), sem, ray_mask, arr,
                                                         len(arr), frame0, n_samples, shadow_eps, C.c_void_p(d_primary),
                                                         C.c_void_p(d_primary_inst), C.c_void_p(d_lit), C.c_void_p(stream)))

    def light_term_dev(self, view, width, height, lights, d_primary, d_attr, d_lit, d_value, n_samples=1, ambient=0.0, d_term=0,
                       shard=(0, 1), stream=0):
        """trx_light_term_dev: one float per record at d_value - ambient (times the AO term at d_term, if given) plus every
        light's unshadowed term times its visibility count / samples; 0 where there is no surface."""
        arr = light_array(lights)
        L.check(self._lib.trx_light_term_dev(self._h, C.byref(view), width, height, L.Shard(*shard), arr, len(arr), n_samples,
                                             C.c_void_p(d_primary), C.c_void_p(d_attr), C.c_void_p(d_lit), C.c_void_p(d_term), ambient,
                                             C.c_void_p(d_value), C.c_void_p(stream)))

    def bounce_light_rays_dev(self, width, height, light, d_bounce_rays, d_bounce_hits, d_bounce_attr, d_rays, light_index=0, frame0=0,
                              sample=0, shadow_eps=0.01, shard=(0, 1), stream=0):
        """trx_bounce_light_rays_dev: the shadow rays from the bounce hits (the rays at d_bounce_rays, their hits and attribute
        records, one per record laid out like the hit buffers of `shard`) toward `light` as explicit rays at d_rays; the inert
        ray where the bounce found no surface or the surface faces away."""
        L.check(self._lib.trx_bounce_light_rays_dev(self._h, width, height, L.Shard(*shard), C.byref(light), light_index, frame0, sample,
                                                    shadow_eps, C.c_void_p(d_bounce_rays), C.c_void_p(d_bounce_hits),
                                                    C.c_void_p(d_bounce_attr), C.c_void_p(d_rays), C.c_void_p(stream)))

    def trace_indirect_dev(self, view, width, height, lights, d_primary, d_value, n_samples=1, sem=L.SEM_HLSL, ray_mask=0, frame0=0,
                           bounce_eps=0.01, shadow_eps=0.01, bounce_albedo=0.5, d_primary_inst=0, d_base=0, shard=(0, 1), stream=0):
        """trx_trace_indirect_dev: one float per record at d_value - d_base's value (0 without one; d_base may be d_value) plus
        bounce_albedo / n_samples times the direct light found at the hits of n_samples cosine-hemisphere bounce rays (seeds
        frame0 ..); ray_mask masks the shadow rays from the bounce hits, not the bounce rays."""
        arr = light_array(lights)
        L.check(self._lib.trx_trace_indirect_dev(self._h, C.byref(view), width, height, L.Shard(*shard), sem, ray_mask, arr, len(arr),
                                                 frame0, n_samples, bounce_eps, shadow_eps, bounce_albedo, C.c_void_p(d_primary),
                                                 C.c_void_p(d_primary_inst), C.c_void_p(d_base), C.c_void_p(d_value), C.c_void_p(stream)))

    def trace_indirect_sparse_dev(self, view, width, height, stride, phase, lights, d_primary, d_value_lo, n_samples=1, sem=L.SEM_HLSL,
                                  ray_mask=0, frame0=0, bounce_eps=0.01, shadow_eps=0.01, bounce_albedo=0.5, d_primary_inst=0, stream=0):
        """trx_trace_indirect_sparse_dev: the indirect pass at pixel (X * stride + phase % stride, Y * stride + phase // stride)
        of every cell (X, Y) of the ceil(width / stride) x ceil(height / stride) low grid, one float per cell at d_value_lo -
        that pixel's value of trx_trace_indirect_dev without a base, +0 where the pixel leaves the image or has no surface.
        d_primary / d_primary_inst are whole-image, image-layout, full-resolution records."""
        arr = light_array(lights)
        L.check(self._lib.trx_trace_indirect_sparse_dev(self._h, C.byref(view), width, height, stride, phase, sem, ray_mask, arr, len(arr),
                                                        frame0, n_samples, bounce_eps, shadow_eps, bounce_albedo, C.c_void_p(d_primary),
                                                        C.c_void_p(d_primary_inst), C.c_void_p(d_value_lo), C.c_void_p(stream)))

    def trace_indirect_rgb_dev(self, view, width, height, lights, d_primary, d_value_rgb, n_samples=1, sem=L.SEM_HLSL, ray_mask=0, frame0=0,
                               bounce_eps=0.01, shadow_eps=0.01, d_primary_inst=0, shard=(0, 1), stream=0):
        """trx_trace_indirect_rgb_dev: trace_indirect_dev with the material of the triangle every bounce ray hits in
        bounce_albedo's place - three planes of floats at d_value_rgb (plane c at c * records, records as for
        trace_light_visibility_dev's planes): per sample albedo * s + emission summed, over n_samples; +0 without a surface."""
        arr = light_array(lights)
        L.check(self._lib.trx_trace_indirect_rgb_dev(self._h, C.byref(view), width, height, L.Shard(*shard), sem, ray_mask, arr, len(arr),
                                                     frame0, n_samples, bounce_eps, shadow_eps, C.c_void_p(d_primary),
                                                     C.c_void_p(d_primary_inst), C.c_void_p(d_value_rgb), C.c_void_p(stream)))

    def trace_indirect_rgb_sparse_dev(self, view, width, height, stride, phase, lights, d_primary, d_value_rgb_lo, n_samples=1,
                                      sem=L.SEM_HLSL, ray_mask=0, frame0=0, bounce_eps=0.01, shadow_eps=0.01, d_primary_inst=0, stream=0):
        """trx_trace_indirect_rgb_sparse_dev: trace_indirect_sparse_dev's grid in colour - three low planes at d_value_rgb_lo
        (plane c at c * Wlo * Hlo), every cell its full-resolution pixel's value of trace_indirect_rgb_dev."""
        arr = light_array(lights)
        L.check(self._lib.trx_trace_indirect_rgb_sparse_dev(self._h, C.byref(view), width, height, stride, phase, sem, ray_mask, arr,
                                                            len(arr), frame0, n_samples, bounce_eps, shadow_eps, C.c_void_p(d_primary),
                                                            C.c_void_p(d_primary_inst), C.c_void_p(d_value_rgb_lo), C.c_void_p(stream)))

    # emitters (include/trx.h, "emitters") ---------------------------------------------
    def build_emitters(self):
        """trx_scene_build_emitters: the table of the scene's emissive (instance, triangle) pairs, built on the device from
        the scene's own triangle records; returns the number of emitters.  Needs materials; stale after set_materials, a
        refit or an instance change, until it is built again."""
        n = C.c_uint32()
        L.check(self._lib.trx_scene_build_emitters(self._h, C.byref(n)))
        return n.value

    def get_emitters(self):
        """(records [n, 16] float32 - V0 kinv | E1 material | E2 prim | NG instance, the three indices as bit patterns -,
        c [n - 1] float32: the cumulative selection probabilities)."""
        rec = np.zeros((L.MAX_EMITTERS, 16), dtype=np.float32)
        c = np.zeros(L.MAX_EMITTERS, dtype=np.float32)
        n = C.c_uint32(L.MAX_EMITTERS)
        L.check(self._lib.trx_scene_get_emitters(self._h, _ptr(rec), C.byref(n), _ptr(c)))
        return rec[:n.value].copy(), c[:n.value - 1].copy()

    def debug_emitter_select(self, d_u0, n, d_j):
        """trx_debug_emitter_select: the device's selection function over n float32 u0 values at d_u0, one uint32 j each at
        d_j (synchronous)."""
        L.check(self._lib.trx_debug_emitter_select(self._h, C.c_void_p(d_u0), n, C.c_void_p(d_j)))

    def emitter_rays_dev(self, view, width, height, d_primary, d_rays, frame0=0, sample=0, shadow_eps=0.01, emitter_eps=0.001,
                         d_primary_inst=0, shard=(0, 1), stream=0):
        """trx_emitter_rays_dev: one sample's shadow rays toward the emitters its noise selects (seed frame0 + 2048 + sample),
        one per record laid out like the hit buffers of `shard`; the inert ray where nothing is cast."""
        L.check(self._lib.trx_emitter_rays_dev(self._h, C.byref(view), width, height, L.Shard(*shard), frame0, sample, shadow_eps,
                                               emitter_eps, C.c_void_p(d_primary), C.c_void_p(d_primary_inst), C.c_void_p(d_rays),
                                               C.c_void_p(stream)))

    def trace_emitter_light_dev(self, view, width, height, d_primary, d_out_rgb, n_samples=1, sem=L.SEM_HLSL, ray_mask=0, frame0=0,
                                shadow_eps=0.01, emitter_eps=0.001, d_primary_inst=0, d_base_rgb=0, shard=(0, 1), stream=0):
        """trx_trace_emitter_light_dev: three planes of floats at d_out_rgb (plane c at c * records) - d_base_rgb's value (0
        without one; it may be d_out_rgb) plus the mean over n_samples of wgeo * emission of the emitters whose shadow ray
        was cast and not occluded."""
        L.check(self._lib.trx_trace_emitter_light_dev(self._h, C.byref(view), width, height, L.Shard(*shard), sem, ray_mask, frame0,
                                                      n_samples, shadow_eps, emitter_eps, C.c_void_p(d_primary),
                                                      C.c_void_p(d_primary_inst), C.c_void_p(d_base_rgb), C.c_void_p(d_out_rgb),
                                                      C.c_void_p(stream)))

    def trace_indirect_rgb_emitters_dev(self, view, width, height, lights, d_primary, d_value_rgb, n_samples=1, sem=L.SEM_HLSL, ray_mask=0,
                                        frame0=0, bounce_eps=0.01, shadow_eps=0.01, emitter_eps=0.001, d_primary_inst=0, shard=(0, 1),
                                        stream=0):
        """trx_trace_indirect_rgb_emitters_dev: trace_indirect_rgb_dev with the emitters sampled from every bounce hit (rule
        5e) in place of the bounce triangle's own emission; `lights` may be empty."""
        arr = light_array(lights)
        L.check(self._lib.trx_trace_indirect_rgb_emitters_dev(self._h, C.byref(view), width, height, L.Shard(*shard), sem, ray_mask,
                                                              arr if len(arr) else None, len(arr), frame0, n_samples, bounce_eps, shadow_eps,
                                                              emitter_eps, C.c_void_p(d_primary), C.c_void_p(d_primary_inst),
                                                              C.c_void_p(d_value_rgb), C.c_void_p(stream)))

    def trace_indirect_rgb_emitters_sparse_dev(self, view, width, height, stride, phase, lights, d_primary, d_value_rgb_lo, n_samples=1,
                                               sem=L.SEM_HLSL, ray_mask=0, frame0=0, bounce_eps=0.01, shadow_eps=0.01, emitter_eps=0.001,
                                               d_primary_inst=0, stream=0):
        """trx_trace_indirect_rgb_emitters_sparse_dev: trace_indirect_rgb_sparse_dev's grid, every cell its full-resolution
        pixel's value of trace_indirect_rgb_emitters_dev."""
        arr = light_array(lights)
        L.check(self._lib.trx_trace_indirect_rgb_emitters_sparse_dev(self._h, C.byref(view), width, height, stride, phase, sem, ray_mask,
                                                                     arr if len(arr) else None, len(arr), frame0, n_samples, bounce_eps,
                                                                     shadow_eps, emitter_eps, C.c_void_p(d_primary),
                                                                     C.c_void_p(d_primary_inst), C.c_void_p(d_value_rgb_lo),
                                                                     C.c_void_p(stream)))

    def material_compose_dev(self, d_primary, d_direct, n, d_colour_rgb, d_indirect_rgb=0, stream=0):
        """trx_material_compose_dev: three planes of n floats at d_colour_rgb - emission + albedo * (direct + indirect_c) of the
        primary record's material (indirect 0 without d_indirect_rgb, which may be d_colour_rgb); +0 where the record is no
        surface record of the scene."""
        L.check(self._lib.trx_material_compose_dev(self._h, C.c_void_p(d_primary), C.c_void_p(d_direct), C.c_void_p(d_indirect_rgb), n,
                                                   C.c_void_p(d_colour_rgb), C.c_void_p(stream)))

    def surface_albedo_dev(self, d_hits, d_attr, n, d_albedo_rgb, stream=0):
        """trx_surface_albedo_dev: three planes of n floats at d_albedo_rgb - the albedo of every hit record's material, times
        the material's texture sampled at the record's interpolated texcoords where the scene has both tables (THE TEXTURED
        ALBEDO, include/trx.h); +0 where the record is no surface record of the scene."""
        L.check(self._lib.trx_surface_albedo_dev(self._h, C.c_void_p(d_hits), C.c_void_p(d_attr), n, C.c_void_p(d_albedo_rgb),
                                                 C.c_void_p(stream)))

    def albedo_compose_dev(self, d_primary, d_albedo_rgb, d_direct, n, d_colour_rgb, d_indirect_rgb=0, stream=0):
        """trx_albedo_compose_dev: material_compose_dev with the albedo read from the planes surface_albedo_dev wrote."""
        L.check(self._lib.trx_albedo_compose_dev(self._h, C.c_void_p(d_primary), C.c_void_p(d_albedo_rgb), C.c_void_p(d_direct),
                                                 C.c_void_p(d_indirect_rgb), n, C.c_void_p(d_colour_rgb), C.c_void_p(stream)))

    def trace_indirect_rgb_textured_dev(self, view, width, height, lights, d_primary, d_value_rgb, n_samples=1, stride=1, phase=0,
                                        use_emitters=False, sem=L.SEM_HLSL, ray_mask=0, frame0=0, bounce_eps=0.01, shadow_eps=0.01,
                                        emitter_eps=0.001, d_primary_inst=0, shard=(0, 1), stream=0):
        """trx_trace_indirect_rgb_textured_dev: the four RGB modes of the indirect pass (stride 1: dense over `shard`; stride
        2..: sparse at (stride, phase); use_emitters: rule 5e) with the albedo of every bounce hit sampled from its texture."""
        arr = light_array(lights)
        L.check(self._lib.trx_trace_indirect_rgb_textured_dev(self._h, C.byref(view), width, height, L.Shard(*shard), stride, phase, sem,
                                                              ray_mask, arr if len(arr) else None, len(arr), frame0, n_samples, bounce_eps,
                                                              shadow_eps, 1 if use_emitters else 0, emitter_eps, C.c_void_p(d_primary),
                                                              C.c_void_p(d_primary_inst), C.c_void_p(d_value_rgb), C.c_void_p(stream)))

    def shade_rgb_dev(self, d_colour_rgb, n, d_rgba, stream=0):
        """trx_shade_rgb_dev: three planes of n floats as RGBA8, every channel through shade_value_dev's code table."""
        L.check(self._lib.trx_shade_rgb_dev(self._h, C.c_void_p(d_colour_rgb), n, C.c_void_p(d_rgba), C.c_void_p(stream)))

    def value_upsample_dev(self, width, height, stride, phase, d_primary, d_in_lo, d_out, radius, depth_tol=0.1, normal_cos=0.9, d_attr=0,
                           d_base=0, stream=0):
        """trx_value_upsample_dev: one float per full-resolution pixel at d_out from a low-grid float plane - the weighted mean
        (weights (radius + 1 - |dy|) * (radius + 1 - |dx|)) of the accepted low cells of the (2 * radius + 1)^2 window around
        cell (x // stride, y // stride), accepted as in trx_ao_upsample_dev; of every surface cell of the window where none is
        accepted; d_base's value (none without one; d_base may be d_out) is added at surface pixels and copied elsewhere."""
        L.check(self._lib.trx_value_upsample_dev(self._h, width, height, stride, phase, C.c_void_p(d_primary), C.c_void_p(d_attr),
                                                 C.c_void_p(d_in_lo), C.c_void_p(d_base), radius, depth_tol, normal_cos,
                                                 C.c_void_p(d_out), C.c_void_p(stream)))

    def shade_value_dev(self, d_value, n, d_rgba, stream=0):
        """trx_shade_value_dev: n float values as RGBA8 through the code table (0 for negative or NaN, 255 from 1 upward)."""
        L.check(self._lib.trx_shade_value_dev(self._h, C.c_void_p(d_value), n, C.c_void_p(d_rgba), C.c_void_p(stream)))

    def hit_attributes_rays_dev(self, d_rays, n, d_hits, d_attr, d_inst=0, stream=0):
        """trx_hit_attributes_rays_dev: n trx_hit_attr records at d_attr for the hits d_hits of the rays d_rays (d_inst: the
        hits' instance ids, required on scenes with instance transforms)."""
        L.check(self._lib.trx_hit_attributes_rays_dev(self._h, C.c_void_p(d_rays), n, C.c_void_p(d_hits),
                                                      C.c_void_p(d_inst), C.c_void_p(d_attr), C.c_void_p(stream)))

    def hit_attributes_primary_dev(self, view, width, height, d_hits, d_attr, d_inst=0, shard=(0, 1), stream=0):
        """trx_hit_attributes_primary_dev: attributes of a primary frame's records, laid out as the trace wrote them
        (shard = (index, count) or (index, count, layout))."""
        L.check(self._lib.trx_hit_attributes_primary_dev(self._h, C.byref(view), width, height, L.Shard(*shard),
                                                         C.c_void_p(d_hits), C.c_void_p(d_inst), C.c_void_p(d_attr),
                                                         C.c_void_p(stream)))

    def shading_normals_rays(self, d_rays, n, d_hits, d_attr, d_out, d_inst=0, stream=0):
        """trx_shading_normals_rays_dev: the n attribute records d_attr (device pointers throughout) with their normal replaced
        by the interpolated vertex normal where the header's rule adopts it, at d_out (may be d_attr); d_inst as for the
        attribute pass.  Refused on a scene without vertex normals."""
        L.check(self._lib.trx_shading_normals_rays_dev(self._h, C.c_void_p(d_rays), n, C.c_void_p(d_hits), C.c_void_p(d_inst),
                                                       C.c_void_p(d_attr), C.c_void_p(d_out), C.c_void_p(stream)))

    def shading_normals_primary(self, view, width, height, d_hits, d_attr, d_out, d_inst=0, shard=(0, 1), stream=0):
        """trx_shading_normals_primary_dev: the same for a primary frame's records, laid out as the trace wrote them
        (shard = (index, count) or (index, count, layout))."""
        L.check(self._lib.trx_shading_normals_primary_dev(self._h, C.byref(view), width, height, L.Shard(*shard), C.c_void_p(d_hits),
                                                          C.c_void_p(d_inst), C.c_void_p(d_attr), C.c_void_p(d_out), C.c_void_p(stream)))

    def ao_filter_dev(self, width, height, d_primary, d_unoccluded, d_term, n_samples, radius, depth_tol=0.02, normal_cos=0.9,
                      d_attr=0, stream=0):
        """trx_ao_filter_dev: one trx_ao_term per pixel at d_term from whole-image, image-layout records - the counts of
        the accepted pixels of the (2 * radius + 1)^2 window summed (accepted: a surface, depth within depth_tol * t_p and,
        with d_attr, normals within normal_cos; the pixel itself always)."""
        L.check(self._lib.trx_ao_filter_dev(self._h, width, height, C.c_void_p(d_primary), C.c_void_p(d_attr),
                                            C.c_void_p(d_unoccluded), n_samples, radius, depth_tol, normal_cos,
                                            C.c_void_p(d_term), C.c_void_p(stream)))

    def value_filter_dev(self, width, height, d_primary, d_in, d_out, n_levels, depth_tol=0.1, normal_cos=0.9, d_attr=0, d_base=0,
                         d_work=0, stream=0):
        """trx_value_filter_dev: n_levels (1..5) levels of the edge-aware a-trous filter over the float plane d_in into d_out,
        taps 1, 2, 4, .. pixels apart, each accepted as in the AO filter; d_base's value (none without one; d_base may be d_out)
        is added at surface pixels and copied elsewhere.  d_work: a plane of the caller's, needed from two levels on."""
        L.check(self._lib.trx_value_filter_dev(self._h, width, height, C.c_void_p(d_primary), C.c_void_p(d_attr), C.c_void_p(d_in),
                                               C.c_void_p(d_base), n_levels, depth_tol, normal_cos, C.c_void_p(d_work),
                                               C.c_void_p(d_out), C.c_void_p(stream)))

    def ao_upsample_dev(self, width, height, stride, phase, d_primary, d_unoccluded_lo, d_term, n_samples, radius, depth_tol=0.02,
                        normal_cos=0.9, d_attr=0, stream=0):
        """trx_ao_upsample_dev: one trx_ao_term per full-resolution pixel at d_term from the sparse pass's low-grid counts -
        the counts of the accepted low cells of the (2 * radius + 1)^2 window around cell (x // stride, y // stride) summed
        (accepted as in the filter, on the full-resolution records of the cell's pixel); every surface cell of the window
        where none is accepted."""
        L.check(self._lib.trx_ao_upsample_dev(self._h, width, height, stride, phase, C.c_void_p(d_primary), C.c_void_p(d_attr),
                                              C.c_void_p(d_unoccluded_lo), n_samples, radius, depth_tol, normal_cos,
                                              C.c_void_p(d_term), C.c_void_p(stream)))

    def shade_reference_dev(self, d_primary, d_ao, n, d_rgba, stream=0):
        """trx_shade_reference_dev: the reference's grey image of n primary / AO record pairs, 4 bytes per record."""
        L.check(self._lib.trx_shade_reference_dev(self._h, C.c_void_p(d_primary), C.c_void_p(d_ao), n, C.c_void_p(d_rgba),
                                                  C.c_void_p(stream)))

    def shade_ao_counts_dev(self, d_unoccluded, n_samples, n, d_rgba, stream=0):
        """trx_shade_ao_counts_dev: count / n_samples of n visibility counts (0 where there is no surface) as RGBA8."""
        L.check(self._lib.trx_shade_ao_counts_dev(self._h, C.c_void_p(d_unoccluded), n_samples, n, C.c_void_p(d_rgba),
                                                  C.c_void_p(stream)))

    def shade_ao_term_dev(self, d_term, n, d_rgba, stream=0):
        """trx_shade_ao_term_dev: unoccluded / samples of n filtered terms (0 where samples == 0) as RGBA8."""
        L.check(self._lib.trx_shade_ao_term_dev(self._h, C.c_void_p(d_term), n, C.c_void_p(d_rgba), C.c_void_p(stream)))

    def shade_heat_dev(self, d_cost, n, d_rgba, which=L.HEAT_NODES, scale=None, stream=0):
        """trx_shade_heat_dev: the PROFILE_RT heat map of n per-ray count records as RGBA8 (scale None: the reference's)."""
        if scale is None:
            scale = L.HEAT_SCALE_TRIS if which == L.HEAT_TRIS else L.HEAT_SCALE_NODES
        L.check(self._lib.trx_shade_heat_dev(self._h, C.c_void_p(d_cost), n, which, scale, C.c_void_p(d_rgba), C.c_void_p(stream)))

    def check(self, stream=0):
        L.check(self._lib.trx_scene_check(self._h, C.c_void_p(stream)))


def cwbvh_gpu_runner(verts, object_counts, width, height, camera, tlas=False, max_prims_per_leaf=3, benchmark=True,
                     frames=20, sem=L.SEM_HLSL, device=0, threads=0):
    """cwbvh_gpu_runner (src/rt_gpu/mod.rs:16-112) on the HIP backend: build the BLAS/TLAS,
    assemble the flat buffers, upload, trace, return (frame_ms, blas_build_s, tlas_build_ms)."""
    flat = flat_build(verts, object_counts, use_tlas=tlas, max_prims_per_leaf=max_prims_per_leaf, threads=threads)
    scene = Scene(flat, device=device)
    try:
        eye, look_at, fov = camera
        view = view_from_camera(eye, look_at, fov, width, height)
        mn, _mean = scene.bench_primary(view, width, height, sem=sem, warmup=1 if benchmark else 0, frames=frames)
        return mn, flat.blas_build_s, flat.tlas_build_s * 1000.0
    finally:
        scene.close()
