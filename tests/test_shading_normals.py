"""Vertex normals and the shading normal without a GPU (include/trx.h, "vertex normals and the shading normal"): the boundary,
trx_compute_vertex_normals against its float64 twin bit for bit, the OBJ `vn` loader against the twin's reader and
trx_load_model, the refusals decided before a device is touched, the twin's own properties on the golden scenes under the
oracle's hits (tests/shading_normal_twin.py, tests/hit_attr_twin.py), the kernel's resources and the command line's flags."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import shading_normal_cases as CS
import shading_normal_twin as SN
from ao_visibility_twin import instanced_case
from hit_attr_twin import hit_attrs, primary_dirs, primary_origins, tri_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tray_racing_amd", "tray_racing_hip")
f32 = np.float32
NEW_SYMBOLS = ("trx_scene_set_vertex_normals", "trx_scene_get_vertex_normals", "trx_shading_normals_primary_dev", "trx_shading_normals_rays_dev",
               "trx_render_image_lit_smooth", "trx_render_image_colour_smooth", "trx_compute_vertex_normals", "trx_load_model_normals")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the boundary ------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_bound(trx):
    from tray_racing_amd import _lib
    header = open(os.path.join(ROOT, "include", "trx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    lib = trx.load()
    for name in NEW_SYMBOLS:
        assert (" T %s\n" % name) in out and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert name + "(" in header
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [3, 3, 10, 8, 20, 28, 4, 7]
    for name in ("set_vertex_normals", "get_vertex_normals", "shading_normals_primary", "shading_normals_rays", "render_image_lit_smooth",
                 "render_image_colour_smooth"):
        assert callable(getattr(trx.Scene, name)), name
    assert callable(trx.compute_vertex_normals) and callable(trx.load_model_normals)
    # the smooth forms take the plain forms' arguments
    assert _lib.SIGNATURES["trx_render_image_lit_smooth"] == _lib.SIGNATURES["trx_render_image_lit"]
    assert _lib.SIGNATURES["trx_render_image_colour_smooth"] == _lib.SIGNATURES["trx_render_image_colour"]
    src = (b'#include "trx.h"\n'
           b'int f(trx_scene *s, const trx_view *v, const trx_ray *r, const trx_hit *p, trx_hit_attr *a, const float *n, float *o) {\n'
           b'    trx_shard whole = {0, 1, TRX_LAYOUT_IMAGE, 0};\n'
           b'    int rc = trx_scene_set_vertex_normals(s, n, 1) | trx_scene_get_vertex_normals(s, o, 1);\n'
           b'    rc |= trx_shading_normals_primary_dev(s, v, 8, 8, whole, p, 0, a, a, 0) | trx_shading_normals_rays_dev(s, r, 64, p, 0, a, a, 0);\n'
           b'    return rc | trx_compute_vertex_normals(n, 1, 0.5f, o);\n}\n'
           b'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", "-I",
                    os.path.join(ROOT, "include"), "-"], input=src, check=True)
    assert lib.trx_abi_version() == 1   # additions only


def test_shading_normal_kernel_resources():
    """Both k_shading_normal instantiations exist (make build/kernels.s): streaming gathers - no scratch, no LDS, within the
    128 VGPRs tests/test_materials.py holds the other post-walk kernels to (the counts are printed)."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "tray_racing_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "build/kernels.s"], check=True, capture_output=True, timeout=900)
    text = open(os.path.join(csrc, "build", "kernels.s")).read()
    found = []
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n.*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        name, body = m.group(2), m.group(3)
        if "k_shading_normal" not in name:
            continue
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        print("%s: %d VGPRs, %d B scratch, %d B LDS" % (name, vgprs, scratch, int(m.group(1))))
        assert scratch == 0 and vgprs <= 128 and int(m.group(1)) == 0, name
        found.append(name)
    assert len(found) == 2 and any("ILi0E" in n for n in found) and any("ILi1E" in n for n in found), found


# ---- the generator against its twin ----------------------------------------------------------------------------------------------

def _generated(trx, verts, crease_cos):
    got = trx.compute_vertex_normals(verts, crease_cos)
    want = SN.vertex_normals(verts, f32(crease_cos))
    bad = np.flatnonzero((_bits(got) != _bits(want)).any(1))
    assert bad.size == 0, "crease_cos %g: %d triangles differ from the twin, first %s: %s != %s" % (crease_cos, bad.size, bad[:3], got[bad[:1]], want[bad[:1]])
    return got


def test_cube_with_a_crease_keeps_the_axis_normals(trx):
    cube = CS.cube()
    got = _generated(trx, cube, 0.5).reshape(12, 3, 3)
    face = SN.face_vectors(cube)[1]                                    # (unit face vectors: exactly the axes)
    assert (np.abs(face).sum(1) == 1.0).all() and (np.abs(face).max(1) == 1.0).all()
    assert (got == face[:, None, :].astype(np.float32)).all()          # (== : a -0.0 component is the axis normal too)


def test_cube_welded_all_round_gets_the_corner_diagonals(trx):
    cube = CS.cube()
    got = _generated(trx, cube, -1.0).reshape(12, 3, 3)
    pos = cube.reshape(12, 3, 3)
    k = f32(1.0 / np.sqrt(3.0))
    want = np.where(pos == 1.0, k, -k).astype(np.float32)              # outward: + where the corner's coordinate is 1
    assert (_bits(got) == _bits(want)).all(), (got[0], want[0])


def test_signed_zeros_weld(trx):
    """Two triangles folded along the edge (0,0,0)-(0,1,0), written with -0.0 in one and +0.0 in the other."""
    a = np.array([[0.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.5]], dtype=np.float32)
    b = np.array([[-0.0, 1.0, -0.0, -0.0, -0.0, 0.0, 1.0, 0.0, 0.5]], dtype=np.float32)
    verts = np.concatenate([a, b])
    assert (_bits(verts[0, 0:3]) != _bits(verts[1, 3:6])).any()        # (the shared corner's bits really differ)
    got = _generated(trx, verts, -1.0).reshape(2, 3, 3)
    flat = _generated(trx, verts, 1.0).reshape(2, 3, 3)
    assert (_bits(got[0, 0]) == _bits(got[1, 1])).all() and (_bits(got[0, 1]) == _bits(got[1, 0])).all()
    assert (got[0, 0] != flat[0, 0]).any() and (got[0, 2] == flat[0, 2]).all() and (got[1, 2] == flat[1, 2]).all()
    assert abs(float(got[0, 0, 2])) == 1.0 and got[0, 0, 0] == 0.0    # (the fold is symmetric: the welded normal is the z axis)


def test_a_zero_area_triangle_gets_zero_and_changes_no_neighbour(trx):
    rng = np.random.default_rng(3)
    pts = rng.integers(-2, 3, size=(12, 3)).astype(np.float32)
    tri = rng.integers(0, 12, size=(40, 3))
    verts = pts[tri].reshape(-1, 9).astype(np.float32)
    keep = SN.face_vectors(verts)[2]
    verts = verts[keep]
    degenerate = np.concatenate([verts[3, 0:3], verts[5, 3:6], verts[3, 0:3]])[None, :]       # two corners at one position, both shared
    line = np.concatenate([verts[7, 0:3], verts[7, 0:3] * 2 + 1, verts[7, 0:3] * 3 + 2])[None, :]   # three corners on a line
    both = np.concatenate([verts[:10], degenerate, verts[10:], line]).astype(np.float32)
    for cc in (-1.0, 0.3):
        with_it, without = _generated(trx, both, cc), _generated(trx, verts, cc)
        assert (_bits(with_it[10]) == 0).all() and (_bits(with_it[-1]) == 0).all()           # +0, not -0
        assert (_bits(np.delete(with_it, [10, both.shape[0] - 1], axis=0)) == _bits(without)).all()


def test_a_seeded_soup_equals_the_twin(trx):
    rng = np.random.default_rng(5)
    pts = rng.integers(-3, 4, size=(60, 3)).astype(np.float32) * f32(0.37)
    verts = pts[rng.integers(0, 60, size=(300, 3))].reshape(-1, 9).astype(np.float32)
    verts[verts == 0] = np.where(rng.random((verts == 0).sum()) < 0.5, f32(-0.0), f32(0.0))   # signed zeros scattered over the shared corners
    shared = 0
    for cc in (-1.0, 0.0, 0.5, 0.70710678, 1.0):
        got = _generated(trx, verts, cc)
        shared = max(shared, int((got != _generated(trx, verts, 1.0)).any(1).sum()))
    assert shared > 100 and (SN.face_vectors(verts)[2] == 0).sum() > 3                        # (welds happen; degenerate faces are there)


def test_generator_refusals(trx):
    v = CS.cube()
    for bad in (1.5, -1.0001, float("nan"), float("inf")):
        with pytest.raises(trx.TrxError, match="crease_cos") as e:
            trx.compute_vertex_normals(v, bad)
        assert e.value.code == -1
    assert trx.compute_vertex_normals(np.zeros((0, 9), dtype=np.float32)).shape == (0, 9)


# ---- the loader -----------------------------------------------------------------------------------------------------------------

OBJ = """# corners of every form
o first
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0.5 0.5
vn 0 0 1
vn 0.6 0 0.8
vn -0.25 0.5 2
f 1//1 2//2 3//3
f 1/1/2 2/1/3 3/1/1 4/1/-1
o second
v 0 0 1
v 2 0 1
v 0 2 1
vn 1e-3 -7 0.125
f -3//-1 -2//-4 -1//2
f 5 6 7
f 5/1 6/1 7/1
f 5//9 6//0 7//-9
f 5//4 6//4 7//4 4//1 1//1
"""


def test_obj_normals_equal_the_twin_reader_and_the_mesh_is_load_models(trx, tmp_path):
    path = tmp_path / "corners.obj"
    path.write_text(OBJ)
    verts, counts, normals, has = trx.load_model_normals(path)
    v0, c0 = trx.load_meshs(path)
    assert verts.tobytes() == v0.tobytes() and counts.tobytes() == c0.tobytes()
    tv, tn, tany = SN.read_obj_normals(str(path))
    assert has and tany and verts.tobytes() == tv.tobytes() and normals.tobytes() == tn.tobytes()
    assert verts.shape == (8, 9) and counts.tolist() == [3, 5]
    n = normals.reshape(-1, 3, 3)
    assert n[0].tolist() == [[0, 0, 1], [f32(0.6), 0, f32(0.8)], [-0.25, 0.5, 2]]                  # v//vn
    assert n[1].tolist() == [n[0, 1].tolist(), n[0, 2].tolist(), n[0, 0].tolist()]                 # v/vt/vn, the quad's 0,1,2
    assert n[2].tolist() == [n[0, 1].tolist(), n[0, 0].tolist(), n[0, 2].tolist()]                 # ... and 0,2,3 with the relative -1
    assert n[3].tolist() == [[f32(1e-3), -7, 0.125], n[0, 0].tolist(), n[0, 1].tolist()]           # relative -1, -4 and absolute 2
    assert (_bits(n[4:7]) == 0).all()                                                              # no index, v/vt, out of range: +0
    assert n[7].tolist() == [n[3, 0].tolist()] * 3 and normals.shape == (8, 9)                     # a five-gon keeps its first triangle


def test_obj_without_usable_normals_and_json_models(trx, tmp_path):
    plain = tmp_path / "plain.obj"
    plain.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1 2 3\nf 1//7 2//7 3//7\n")
    verts, _, normals, has = trx.load_model_normals(plain)
    assert not has and verts.shape == (2, 9) and (_bits(normals) == 0).all() and not SN.read_obj_normals(str(plain))[2]
    js = tmp_path / "tri.json"
    js.write_text('[{"v0":[0,0,0], "v1":[1,0,0], "v2":[0,1,0]}, {"v0":[0,0,1], "v1":[1,0,1], "v2":[0,1,1]}]')
    verts, counts, normals, has = trx.load_model_normals(js)
    assert not has and verts.tobytes() == trx.load_meshs(js)[0].tobytes() and normals.shape == (2, 9) and (_bits(normals) == 0).all()
    for text in ("vn 0 nan 1\n", "vn inf 0 0\n", "vn 0 0 -inf\n"):
        bad = tmp_path / "bad.obj"
        bad.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\n" + text + "f 1//1 2//1 3//1\n")
        with pytest.raises(trx.TrxError, match="not finite") as e:
            trx.load_model_normals(bad)
        assert e.value.code == -1
        assert trx.load_meshs(bad)[0].shape == (1, 9)                                              # (the plain loader reads no vn)
    with pytest.raises(trx.TrxError) as e:
        trx.load_model_normals(tmp_path / "missing.obj")
    assert e.value.code == -6


# ---- the twin's own properties, under the oracle's hits -----------------------------------------------------------------------------

def _scene_frames(trx, orc, name):
    """(records, w2o, [(prims, inst, dirs, attr)] - a primary frame and a batch of explicit rays) of a scene of CS.SCENES."""
    if name == "instanced":
        flat, view, osc, oview, w, h = instanced_case(trx, orc)
        recs, w2o = tri_records(flat.tri_verts), osc.w2o
        prim, inst, _ = osc.trace_primary_inst(oview, w, h)
    else:
        g, recs, f16 = CS.golden(name)
        w2o, w, h = None, int(g["width"]), int(g["height"])
        prim, inst = g["orc_f16_primary_sem0" if f16 is not None else "orc_primary_sem0"], None
        from tray_racing_amd import _lib
        view = _lib.View()
        C.memmove(C.byref(view), g["view"].tobytes(), C.sizeof(view))
    px, py = np.arange(w * h) % w, np.arange(w * h) // w
    dirs = primary_dirs(view, w, h, px, py)
    attr = hit_attrs(recs, primary_origins(view, w * h), dirs, prim["prim"], inst, w2o)
    return recs, w2o, prim, inst, dirs, attr


@pytest.mark.parametrize("name", CS.SCENES)
def test_twin_properties_on_the_scenes_the_gpu_tests_use(trx, orc, name):
    """For every table: adopted and fallen-back records both exist; an adopted normal is a unit vector on the geometric normal's
    side for which the light term flips exactly as for the geometric normal; a record that falls back is its input bit for bit."""
    recs, w2o, prim, inst, dirs, attr = _scene_frames(trx, orc, name)
    in_range = prim["prim"] < recs.shape[0]
    assert in_range.sum() > 200 and (~in_range).any()
    seen = set()
    for kind in CS.TABLES:
        out, cause = SN.shading_normals(CS.table(kind, recs), attr, dirs, prim["prim"], inst, w2o)
        adopted = cause == SN.ADOPTED
        fell = in_range & ~adopted
        print("%s %s: %d adopted, %s" % (name, kind, adopted.sum(), {SN.FALLBACKS[c]: int((cause == c).sum()) for c in SN.FALLBACKS}))
        assert adopted.any() and (~adopted).any(), (name, kind)
        if kind != "computed":
            assert fell.any(), (name, kind)
        assert (cause[~in_range] == SN.OUT_OF_RANGE).all() and not (cause[in_range] == SN.OUT_OF_RANGE).any()
        same = out.view(np.uint32).reshape(-1, 6) == attr.view(np.uint32).reshape(-1, 6)
        assert same[~adopted].all() and same[:, :2].all() and (out["_pad"] == 0).all()
        s, g = out["normal"][adopted], attr["normal"][adopted]
        assert (SN.light_flip(s, dirs[adopted]) == SN.light_flip(g, dirs[adopted])).all(), (name, kind)
        assert np.abs(np.sqrt((s.astype(np.float64) ** 2).sum(1)) - 1.0).max() < 1e-6
        assert ((s.astype(np.float64) * g.astype(np.float64)).sum(1) > -1e-6).all()
        if kind == "hostile":
            hk = prim["prim"][in_range] % 5
            by_kind = {k: set(cause[in_range][hk == k].tolist()) for k in range(5)}
            assert by_kind[0] == {SN.Q_NOT_POSITIVE} and by_kind[2] == {SN.Q_NOT_POSITIVE} and SN.Q_NOT_FINITE in by_kind[3], by_kind
            assert SN.ADOPTED in by_kind[1] and {SN.ADOPTED, SN.FLIP_DIFFERS} <= by_kind[4], by_kind
            # kind 1: the flipped normal is the geometric one again, to rounding
            k1 = adopted & in_range & (prim["prim"] % 5 == 1)
            if w2o is None:
                assert np.abs(out["normal"][k1] - attr["normal"][k1]).max() < 1e-6
        seen |= set(cause.tolist())
    assert {SN.OUT_OF_RANGE, SN.Q_NOT_POSITIVE, SN.Q_NOT_FINITE, SN.FLIP_DIFFERS} <= seen


def test_a_nan_geometric_normal_falls_back():
    """c == c: the one condition no table can fail on its own - it guards a record whose geometric normal carries a NaN (the
    attribute pass writes one for a zero-area triangle)."""
    normals = np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), (1, 3))
    attr = np.zeros(3, dtype=SN.ATTR_DTYPE)
    attr["u"], attr["v"], attr["_pad"] = 0.25, 0.25, 7
    attr["normal"] = [[0, 0, 1], [np.nan, 0, 1], [0, 0, np.nan]]
    dirs = np.tile(np.array([0.0, 0.0, -1.0], dtype=np.float32), (3, 1))
    out, cause = SN.shading_normals(normals, attr, dirs, np.zeros(3, dtype=np.uint32))
    assert cause.tolist() == [SN.ADOPTED, SN.C_NAN, SN.C_NAN]
    assert out[0]["_pad"] == 0 and out[0]["normal"].tolist() == [0, 0, 1]
    assert out[1:].tobytes() == attr[1:].tobytes()                     # the pad word and the NaN's payload included


# ---- refusals decided before a device is touched, and the command line --------------------------------------------------------------------

def test_refusals_that_need_no_device(trx):
    lib = trx.load()
    one = np.zeros(9, dtype=np.float32)
    assert lib.trx_scene_set_vertex_normals(None, one.ctypes.data_as(C.c_void_p), 1) == -1
    assert lib.trx_scene_get_vertex_normals(None, one.ctypes.data_as(C.c_void_p), 1) == -1
    assert lib.trx_shading_normals_rays_dev(None, None, 0, None, None, None, None, None) == -1
    assert lib.trx_compute_vertex_normals(None, 1, 0.5, one.ctypes.data_as(C.c_void_p)) == -1
    assert lib.trx_load_model_normals(None, None, None, None, None, None, None) == -1


def test_the_command_lines_flags():
    def run(*args):
        return subprocess.run([CLI, "-i", "standin:cornell", "--dry-run", "--passes", "1"] + list(args), capture_output=True, text=True, timeout=120)
    light = ("--light", "point:0,1.8,0")
    for extra, msg in ((("--smooth",), "--smooth"), (("--png", "--smooth"), "--smooth"), (("--png", "--smooth-crease", "30") + light, "--smooth-crease goes with --smooth"),
                       (("--png", "--smooth", "--smooth-crease", "181") + light, "0..180"), (("--png", "--smooth", "--smooth-crease", "-1") + light, "0..180"),
                       (("--png", "--smooth", "--bounce-samples", "2") + light, "grey --bounce-samples"),
                       (("--png", "--smooth", "--benchmark") + light, "--benchmark"), (("--png", "--smooth", "--profile-rt", "nodes"), "--profile-rt"),
                       (("--png", "--smooth", "--colour", "--emitters", "4"), "--emitters")):
        r = run(*extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    for ok in (("--png", "--smooth") + light, ("--png", "--smooth", "--smooth-crease", "60") + light, ("--png", "--colour", "--smooth") + light,
               ("--png", "--colour", "--smooth", "--bounce-samples", "2") + light):
        r = run(*ok)
        assert r.returncode == 0, (ok, r.stderr)
