"""The direct-light pass without a GPU: the boundary (symbols, the 64-byte trx_light, plain C), the new kernels' resources,
the twin (tests/light_twin.py) held against the header's rules restated pixel by pixel in binary32 scalars, the refusals -
decided before a device is touched - the command line's options, and the oracle's word that the cases of
tests/test_gpu_light.py are not vacuous."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import light_twin as LT
from ao_visibility_twin import golden_case
from hit_attr_twin import tri_records
from image_twin import TERM_DTYPE, codes
from inst_mask_twin import oracle_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tray_racing_amd", "tray_racing_hip")
HIT = np.dtype([("t", "<f4"), ("prim", "<u4")])
INF = float("inf")
f32 = np.float32
NEW_SYMBOLS = ("trx_light_rays_dev", "trx_trace_light_visibility_dev", "trx_light_term_dev", "trx_shade_value_dev",
               "trx_render_image_lit")


# ---- the boundary ------------------------------------------------------------------------------------------------------

def test_symbols_defines_and_the_64_byte_light(trx):
    from tray_racing_amd import _lib
    assert C.sizeof(_lib.Light) == 64 and _lib.MAX_LIGHTS == 8
    assert (_lib.LIGHT_DIRECTIONAL, _lib.LIGHT_POINT, _lib.LIGHT_RECT) == (0, 1, 2)
    src = (b'#include <stddef.h>\n#include "trx.h"\n_Static_assert(sizeof(trx_light) == 64, "size");\n'
           b'_Static_assert(offsetof(trx_light, position) == 4 && offsetof(trx_light, edge1) == 16, "layout");\n'
           b'_Static_assert(offsetof(trx_light, edge2) == 28 && offsetof(trx_light, intensity) == 40, "layout");\n'
           b'_Static_assert(offsetof(trx_light, _pad) == 44, "layout");\n'
           b'_Static_assert(TRX_LIGHT_DIRECTIONAL == 0u && TRX_LIGHT_POINT == 1u && TRX_LIGHT_RECT == 2u, "kinds");\n'
           b'_Static_assert(TRX_MAX_LIGHTS == 8 && TRX_MAX_LIGHTS * 64 <= 256 * 64, "lights");\n'
           b'int main(void) { trx_light l = {TRX_LIGHT_POINT, {0, 1, 0}, {0, 0, 0}, {0, 0, 0}, 1.0f, {0, 0, 0, 0, 0}}; return (int)l._pad[4]; }\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", "-I",
                    os.path.join(ROOT, "include"), "-"], input=src, check=True)
    for field, (name, _) in zip(("kind", "position", "edge1", "edge2", "intensity", "_pad"), _lib.Light._fields_):
        assert field == name
    assert [getattr(_lib.Light, n).offset for n in ("kind", "position", "edge1", "edge2", "intensity", "_pad")] == [0, 4, 16, 28, 40, 44]
    header = open(os.path.join(ROOT, "include", "trx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    lib = trx.load()
    for name in NEW_SYMBOLS + ("trx_debug_light_visibility_phases",):
        assert (" T %s\n" % name) in out and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for name in NEW_SYMBOLS:
        assert name + "(" in header
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [14, 16, 15, 5, 20]
    for name in ("light_rays_dev", "trace_light_visibility_dev", "light_term_dev", "shade_value_dev", "render_image_lit"):
        assert callable(getattr(trx.Scene, name))
    lt = trx.light(trx.LIGHT_RECT, (1, 2, 3), (4, 5, 6), (7, 8, 9), 0.5)
    assert bytes(lt) == np.array([2], dtype="<u4").tobytes() + np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 0.5], dtype="<f4").tobytes() + bytes(20)
    assert lib.trx_abi_version() == 1   # additions only


def test_light_kernel_resources():
    """k_light_rays, k_light_reduce, k_light_term (make build/kernels.s): streaming kernels - no scratch, no LDS, at most 128
    VGPRs (the counts are printed); and the value shade (k_value, build/image.s) keeps the shade's 1 KiB table and no scratch."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "tray_racing_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "build/kernels.s", "build/image.s"], check=True, capture_output=True, timeout=900)

    def resources(path, wanted):
        text = open(os.path.join(csrc, "build", path)).read()
        found = {}
        for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n.*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
            name, body = m.group(2), m.group(3)
            key = [k for k in wanted if k in name]
            if not key:
                continue
            vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
            print("%s: %d VGPRs, %d B scratch, %d B LDS" % (name, vgprs, scratch, int(m.group(1))))
            assert scratch == 0 and vgprs <= 128, name
            found[key[0]] = int(m.group(1))
        return found

    assert resources("kernels.s", ("k_light_rays", "k_light_reduce", "k_light_term")) == {"k_light_rays": 0, "k_light_reduce": 0, "k_light_term": 0}
    assert resources("image.s", ("k_value",)) == {"k_value": 1024}


def test_cli_lists_and_checks_the_light_flags():
    def run(*args):
        return subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=120)
    usage = run("--help")
    assert usage.returncode == 0
    for flag in ("--light point:x,y,z[:i]", "dir:x,y,z[:i]", "rect:cx,cy,cz:ax,ay,az:bx,by,bz[:i]", "--light-samples 1..64", "--light-mask 0..255",
                 "--shadow-eps", "--ambient"):
        assert flag in usage.stdout, flag
    base = ("-i", "standin:cornell", "--dry-run", "--passes", "1")
    pt = ("--light", "point:0,1.8,0")
    for extra, msg in (((*pt,), "--png"), (("--png", "--light", "point:0,1"), "--light takes"), (("--png", "--light", "spot:0,1,2"), "--light takes"),
                       (("--png", "--light", "point:0,1,x"), "--light takes"), (("--png", "--light", "rect:0,1,2:1,0,0"), "--light takes"),
                       (("--png", "--light", "point:0,1,2:1:2"), "--light takes"), (("--png", "--light", "dir:0,0,0"), "non-zero"),
                       (("--png", "--light", "point:0,inf,0"), "--light takes"),
                       (("--png", "--light-samples", "4"), "go with --light"), (("--png", "--ambient", "0.5"), "go with --light"),
                       (("--png", "--light-mask", "1"), "go with --light"), (("--png", "--shadow-eps", "0.1"), "go with --light"),
                       (("--png", *pt, "--light-samples", "0"), "1..64"), (("--png", *pt, "--light-samples", "65"), "1..64"),
                       (("--png", *pt, "--light-mask", "256"), "0..255"), (("--png", *pt, "--shadow-eps", "-1"), ">= 0"),
                       (("--png", *pt, "--ambient", "-1"), ">= 0"), (("--png", *pt * 9), "at most 8"),
                       (("--png", *pt, "--profile-rt", "nodes"), "not together"),
                       (("--png", *pt, "--ao-samples", "4", "--ao-stride", "2"), "not together")):
        r = run(*base, *extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert run(*base, "--png", *pt * 8).returncode == 0
    assert run(*base, "--png", *pt, "--light", "dir:0,1,0:0.5", "--light", "rect:-0.4,1.9,-0.4:0.8,0,0:0,0,0.8:2", "--light-samples", "8", "--light-mask",
               "3", "--shadow-eps", "0.001", "--ambient", "0.2", "--ao-samples", "4", "--ao-filter", "2").returncode == 0


# ---- the twin against the header's rules, pixel by pixel in binary32 scalars ----------------------------------------------

def _mul(m, a, b, c, d):
    return [((m[r] * a + m[4 + r] * b) + m[8 + r] * c) + m[12 + r] * d for r in range(4)]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _primary_dir(view, w, h, px, py):
    pinv, vinv, eye = [f32(x) for x in view.proj_inv], [f32(x) for x in view.view_inv], [f32(x) for x in view.eye]
    u = f32(px) / f32(w)
    v = f32(1.0) - f32(py) / f32(h)
    cx, cy = u * f32(2.0) - f32(1.0), v * f32(2.0) - f32(1.0)
    vx, vy, vz, vw = _mul(pinv, cx, cy, f32(1.0), f32(1.0))
    s = vw
    wx, wy, wz, _ = _mul(vinv, vx / s, vy / s, vz / s, vw / s)
    d = [wx - eye[0], wy - eye[1], wz - eye[2]]
    inv = f32(1.0) / np.sqrt(_dot(d, d))
    return [d[0] * inv, d[1] * inv, d[2] * inv]


def _unit_normal(recs, prim, rows):
    """trx_hit_attr.normal: the record's ng, through the instance's rows, times 1 / sqrtf(dot3(ng, ng))."""
    ng = [f32(x) for x in recs[prim, 9:12]]
    if rows is not None:
        r = [[f32(x) for x in rows[4 * i:4 * i + 4]] for i in range(3)]
        ng = [(r[0][i] * ng[0] + r[1][i] * ng[1]) + r[2][i] * ng[2] for i in range(3)]
    inv = f32(1.0) / np.sqrt(_dot(ng, ng))
    return [ng[0] * inv, ng[1] * inv, ng[2] * inv]


def _flip(n, d):
    sg = np.copysign(f32(1.0), (n[0] * -d[0] + n[1] * -d[1]) + n[2] * -d[2])
    return [n[0] * sg, n[1] * sg, n[2] * sg]


def _is_surface(prim, i):
    return bool(prim["t"][i] < LT.F32_MAX) and int(prim["prim"][i]) != 0xFFFFFFFF


def _ray_by_the_letter(orc, view, w, h, prim, inst, recs, w2o, light, k, frame0, f, eps, i):
    """The eight words of the shadow ray of pixel i."""
    inert = np.array([0, 0, 0, 0, 0, 0, 0, -1.0], dtype=np.float32)
    if not _is_surface(prim, i):
        return inert
    px, py, t = i % w, i // w, f32(prim["t"][i])
    d = _primary_dir(view, w, h, px, py)
    n = _flip(_unit_normal(recs, int(prim["prim"][i]), None if w2o is None else w2o[int(inst[i])]), d)
    eye, eps = [f32(x) for x in view.eye], f32(eps)
    o = [(eye[c] + d[c] * t) - d[c] * eps for c in range(3)]
    if light.kind == LT.DIRECTIONAL:
        p = [f32(x) for x in light.position]
        inv = f32(1.0) / np.sqrt(_dot(p, p))
        l, tmax = [p[0] * inv, p[1] * inv, p[2] * inv], LT.F32_MAX
    else:
        L = [f32(x) for x in light.position]
        if light.kind == LT.RECT:
            seed = (frame0 + k * 64 + f) & 0xFFFFFFFF
            u1 = f32(orc.load().orc_hash_noise(px, py, seed))
            u2 = f32(orc.load().orc_hash_noise(px, py, (seed + 1024) & 0xFFFFFFFF))
            L = [(L[c] + u1 * f32(light.edge1[c])) + u2 * f32(light.edge2[c]) for c in range(3)]
        v = [L[c] - o[c] for c in range(3)]
        dist = np.sqrt(_dot(v, v))
        inv = f32(1.0) / dist
        l, tmax = [v[0] * inv, v[1] * inv, v[2] * inv], min(dist, LT.F32_MAX) if dist == dist else LT.F32_MAX
    if not (_dot(n, l) > f32(0.0)):
        return inert
    return np.array(o + [f32(0.0)] + l + [tmax], dtype=np.float32)


def _term_by_the_letter(view, w, h, prim, normals, planes, lights, n_samples, ambient, term, i):
    if not _is_surface(prim, i):
        return f32(0.0)
    px, py, t = i % w, i // w, f32(prim["t"][i])
    d = _primary_dir(view, w, h, px, py)
    n = _flip([f32(x) for x in normals[i]], d)
    eye = [f32(x) for x in view.eye]
    P = [eye[c] + d[c] * t for c in range(3)]
    a = f32(1.0)
    if term is not None:
        a = f32(0.0) if term["samples"][i] == 0 else f32(term["unoccluded"][i]) / f32(term["samples"][i])
    E = f32(ambient) * a
    for k, light in enumerate(lights):
        if light.kind == LT.DIRECTIONAL:
            p = [f32(x) for x in light.position]
            inv = f32(1.0) / np.sqrt(_dot(p, p))
            g = _dot(n, [p[0] * inv, p[1] * inv, p[2] * inv])
        else:
            Cc = [f32(x) for x in light.position]
            if light.kind == LT.RECT:
                Cc = [(Cc[c] + f32(0.5) * f32(light.edge1[c])) + f32(0.5) * f32(light.edge2[c]) for c in range(3)]
            v = [Cc[c] - P[c] for c in range(3)]
            q = _dot(v, v)
            inv = f32(1.0) / np.sqrt(q)
            g = _dot(n, [v[0] * inv, v[1] * inv, v[2] * inv]) / q
        cnt = int(planes[k][i])
        cnt = 0 if cnt == LT.NO_SURFACE else cnt
        if g > f32(0.0):
            E = E + (f32(light.intensity) * g) * (f32(cnt) / f32(n_samples if light.kind == LT.RECT else 1))
    return E


def _hand_made(trx, w, h, seed, transformed):
    """Random triangles, a camera, and records that point into them: hits at several depths, misses of both kinds."""
    rng = np.random.default_rng(seed)
    n = w * h
    verts = rng.uniform(-1.0, 1.0, (40, 9)).astype(np.float32)
    recs = tri_records(verts)
    view = trx.view_from_camera((0.3, 0.4, 2.5), (0.0, 0.1, 0.0), 55.0, w, h)
    prim = np.zeros(n, dtype=HIT)
    prim["t"] = rng.choice(np.array([1.0, 2.25, 3.5, INF, 3.4028234663852886e38], dtype=np.float32), n, p=[.35, .3, .2, .1, .05])
    prim["prim"] = np.where(rng.random(n) < 0.1, 0xFFFFFFFF, rng.integers(0, 40, n)).astype(np.uint32)
    inst, w2o = None, None
    if transformed:
        w2o = rng.uniform(-1.5, 1.5, (5, 12)).astype(np.float32)
        inst = rng.integers(0, 5, n).astype(np.uint32)
    return view, recs, prim, inst, w2o


def _lights_for(orc, view, w, h, prim, inst, recs, w2o, eps):
    """All three kinds, among them a point light exactly at a surface pixel's ray origin (the inert ray: dist == 0)."""
    i = int(np.flatnonzero(LT.surface(prim))[3])
    geo = LT.frame_geometry(view, w, h, prim, inst, recs, w2o)
    at = int(np.flatnonzero(geo[0] == i)[0])
    eye = np.array(view.eye, dtype=np.float32)
    o = (eye + geo[3][at] * geo[5][at]) - geo[3][at] * f32(eps)
    return i, [LT.Light(LT.POINT, (0.4, 1.5, 0.8), intensity=2.0), LT.Light(LT.DIRECTIONAL, (0.3, 1.0, 0.2), intensity=0.75),
               LT.Light(LT.RECT, (-0.5, 1.6, -0.5), (1.0, 0.0, 0.1), (0.0, 0.2, 1.0), intensity=1.5), LT.Light(LT.POINT, o.tolist()),
               LT.Light(LT.DIRECTIONAL, (0.0, -2.0, 0.0)), LT.Light(LT.RECT, (0.2, -0.3, 3.0), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0), intensity=0.3)]


@pytest.mark.parametrize("w,h,transformed", [(7, 3, False), (7, 3, True), (33, 9, False), (33, 9, True)])
def test_twin_equals_the_rules_by_the_letter(trx, orc, w, h, transformed):
    eps = 0.01
    view, recs, prim, inst, w2o = _hand_made(trx, w, h, 11 * w + h + int(transformed), transformed)
    at_hit, lights = _lights_for(orc, view, w, h, prim, inst, recs, w2o, eps)
    geo = LT.frame_geometry(view, w, h, prim, inst, recs, w2o)
    assert 0 < geo[0].size < w * h
    n_cast = 0
    with np.errstate(all="ignore"):
        for k, light in enumerate(lights):
            for frame0, f in ((0, 0), (5, 7)) if light.kind == LT.RECT else ((0, 0),):
                rays, cast = LT.light_rays(orc, view, w, h, geo, light, k, frame0, f, eps)
                got = rays.view(np.uint32).reshape(-1, 8)
                for i in range(w * h):
                    want = _ray_by_the_letter(orc, view, w, h, prim, inst, recs, w2o, light, k, frame0, f, eps, i).view(np.uint32)
                    assert (got[i] == want).all(), (k, i, got[i], want)
                    assert bool(cast[i]) == (want[7] != 0xBF800000)
                n_cast += int(cast.sum())
                if k == 3:
                    assert not cast[at_hit] and LT.surface(prim)[at_hit]      # the light at the hit point's origin: inert
        assert n_cast > w * h // 2
        # the term, over planes of every count a pass can write, with and without the AO term
        rng = np.random.default_rng(w)
        n_samples = 8
        planes = np.stack([np.where(LT.surface(prim), rng.integers(0, l.samples(n_samples) + 1, w * h), LT.NO_SURFACE).astype(np.uint8)
                           for l in lights])
        planes[0][np.flatnonzero(LT.surface(prim))[:2]] = LT.NO_SURFACE         # (taken as 0)
        normals = np.zeros((w * h, 3), dtype=np.float32)
        normals[geo[0]] = geo[4]
        normals[geo[0][::3]] *= f32(-1.0)                                     # (an attribute normal may face away: the term flips it)
        term = np.zeros(w * h, dtype=TERM_DTYPE)
        term["samples"] = rng.choice([0, 4, 36], w * h)
        term["unoccluded"] = (term["samples"] * rng.random(w * h)).astype(np.uint16)
        for tm, ambient in ((None, 0.25), (term, 0.6), (None, 0.0)):
            got = LT.light_term(view, w, h, prim, normals, planes, lights, n_samples, ambient, tm)
            want = np.array([_term_by_the_letter(view, w, h, prim, normals, planes, lights, n_samples, ambient, tm, i) for i in range(w * h)],
                            dtype=np.float32)
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:4]
            assert (got[~LT.surface(prim)] == 0).all() and (got > 0).any()


def test_the_ray_normal_is_the_attribute_normal_times_the_flip(trx, orc):
    """n of the rays is bit-equal to trx_hit_attr.normal times sg; the twin's flip is exact (a multiplication by +-1)."""
    view, recs, prim, inst, w2o = _hand_made(trx, 33, 9, 5, True)
    idx, px, py, d, n, t = LT.frame_geometry(view, 33, 9, prim, inst, recs, w2o)
    with np.errstate(all="ignore"):
        for j in range(0, idx.size, 7):
            want = _flip(_unit_normal(recs, int(prim["prim"][idx[j]]), w2o[int(inst[idx[j]])]), _primary_dir(view, 33, 9, int(px[j]), int(py[j])))
            assert (np.array(want, dtype=np.float32).view(np.uint32) == n[j].view(np.uint32)).all()
    assert (np.abs(n) == np.abs(LT.flip(n, -d))).all()


def test_value_shade_is_the_code_table_shade():
    v = np.array([-1.0, np.nan, 0.0, 0.5, 1.0, 1.5, INF, -0.0, 1e-30], dtype=np.float32)
    got = LT.shade_value(v)
    assert (got[:, 3] == 255).all() and (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all()
    assert got[:, 0].tolist() == [0, 0, 0, int(codes(np.array([0.5], dtype=np.float32))[0]), 255, 255, 255, 0, 0]


# ---- refusals decided before a device is touched -------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_device_work(trx):
    from tray_racing_amd import _lib
    lib = trx.load()
    buf = np.zeros(64, dtype=np.uint32)
    P = buf.ctypes.data_as(C.c_void_p)
    fake = P   # never dereferenced: every call below is refused on its arguments
    inv = _lib.TRX_ERR_INVALID
    view = _lib.View()
    NAN = float("nan")
    good = trx.light(trx.LIGHT_POINT, (0, 1, 0))

    def arr(*lights):
        return trx.light_array(lights)

    def bad_lights():
        """(lights, what the message names) of every refused light."""
        out = []
        l = trx.light(3, (0, 1, 0))
        out.append((arr(good, l), b"kind"))
        for pad in range(5):
            l = trx.light(trx.LIGHT_RECT, (0, 1, 0), (1, 0, 0), (0, 0, 1))
            l._pad[pad] = 1
            out.append((arr(l), b"_pad"))
        for field in ("position", "edge1", "edge2"):
            for c in range(3):
                for x in (NAN, INF, -INF):
                    l = trx.light(trx.LIGHT_RECT, (0, 1, 0), (1, 0, 0), (0, 0, 1))
                    getattr(l, field)[c] = x
                    out.append((arr(good, good, l), b"finite"))
        for x in (NAN, INF):
            out.append((arr(trx.light(trx.LIGHT_POINT, (0, 1, 0), intensity=x)), b"finite"))
        out.append((arr(trx.light(trx.LIGHT_DIRECTIONAL, (0, 0, 0))), b"zero length"))
        out.append((arr(good, trx.light(trx.LIGHT_DIRECTIONAL, (0.0, -0.0, 0.0))), b"zero length"))
        return out

    def vis(scene=fake, v=C.byref(view), w=4, h=4, sem=0, mask=0, lights=arr(good), n_lights=None, n=4, eps=0.01, prim=P, out=P):
        return lib.trx_trace_light_visibility_dev(scene, v, w, h, _lib.Shard(0, 1, 0, 0), sem, mask, lights, len(lights) if n_lights is None else n_lights,
                                                  0, n, eps, prim, None, out, None)

    assert vis(n_lights=0) == inv and b"n_lights" in lib.trx_last_error()
    assert vis(lights=arr(*[good] * 9)) == inv and b"n_lights" in lib.trx_last_error()
    assert vis(lights=None, n_lights=1) == inv and b"null" in lib.trx_last_error()
    for lights, msg in bad_lights():
        assert vis(lights=lights) == inv and msg in lib.trx_last_error(), msg
    assert vis(n=0) == inv and b"n_samples" in lib.trx_last_error()
    assert vis(n=65) == inv and b"n_samples" in lib.trx_last_error()
    assert vis(mask=256) == inv and b"ray_mask" in lib.trx_last_error()
    for eps in (NAN, -0.01, -INF):
        assert vis(eps=eps) == inv and b"shadow_eps" in lib.trx_last_error()
    assert vis(sem=8) == inv and b"semantics" in lib.trx_last_error()
    assert vis(w=0) == inv and vis(h=0) == inv and vis(v=None) == inv
    for kw in ({"scene": None}, {"prim": None}, {"out": None}):
        assert vis(**kw) == inv and b"null" in lib.trx_last_error()

    def rays(scene=fake, v=C.byref(view), w=4, h=4, light=good, k=0, f=0, eps=0.01, prim=P, out=P):
        return lib.trx_light_rays_dev(scene, v, w, h, _lib.Shard(0, 1, 0, 0), C.byref(light) if light is not None else None, k, 0, f, eps, prim, None,
                                      out, None)

    for lights, msg in bad_lights():
        assert rays(light=lights[len(lights) - 1]) == inv and msg in lib.trx_last_error(), msg
    assert rays(light=None) == inv and rays(k=8) == inv and b"light_index" in lib.trx_last_error()
    assert rays(f=64) == inv and b"sample" in lib.trx_last_error()
    assert rays(eps=NAN) == inv and rays(eps=-1.0) == inv and b"shadow_eps" in lib.trx_last_error()
    assert rays(w=0) == inv and rays(v=None) == inv
    for kw in ({"scene": None}, {"prim": None}, {"out": None}):
        assert rays(**kw) == inv and b"null" in lib.trx_last_error()

    def term(scene=fake, v=C.byref(view), w=4, h=4, lights=arr(good), n_lights=None, n=4, prim=P, attr=P, lit=P, ambient=0.1, out=P):
        return lib.trx_light_term_dev(scene, v, w, h, _lib.Shard(0, 1, 0, 0), lights, len(lights) if n_lights is None else n_lights, n, prim, attr, lit,
                                      None, ambient, out, None)

    for lights, msg in bad_lights():
        assert term(lights=lights) == inv and msg in lib.trx_last_error(), msg
    assert term(n_lights=0) == inv and term(n_lights=9) == inv and term(n=0) == inv and term(n=65) == inv
    for ambient in (NAN, INF):
        assert term(ambient=ambient) == inv and b"ambient" in lib.trx_last_error()
    assert term(w=0) == inv and term(v=None) == inv
    for kw in ({"scene": None}, {"prim": None}, {"attr": None}, {"lit": None}, {"out": None}):
        assert term(**kw) == inv and b"null" in lib.trx_last_error()

    assert lib.trx_shade_value_dev(None, P, 4, P, None) == inv
    assert lib.trx_shade_value_dev(fake, None, 4, P, None) == inv and lib.trx_shade_value_dev(fake, P, 4, None, None) == inv
    assert lib.trx_shade_value_dev(fake, P, 4, C.c_void_p(P.value + 2), None) == inv and b"aligned" in lib.trx_last_error()

    def render(scene=fake, v=C.byref(view), w=4, h=4, sem=0, mask=0, lights=arr(good), n_lights=None, n=4, eps=0.01, ambient=0.1, ao=0, radius=INF,
               r=0, tol=0.02, cos=0.9):
        return lib.trx_render_image_lit(scene, v, w, h, sem, mask, lights, len(lights) if n_lights is None else n_lights, 0, n, eps, ambient, ao, 0.01,
                                        radius, r, tol, cos, P, None)

    for lights, msg in bad_lights():
        assert render(lights=lights) == inv and msg in lib.trx_last_error(), msg
    assert render(n_lights=0) == inv and render(n_lights=9) == inv and render(n=0) == inv and render(n=65) == inv
    assert render(mask=256) == inv and render(eps=NAN) == inv and render(eps=-1.0) == inv and render(ambient=NAN) == inv
    assert render(ao=65) == inv and render(ao=4, radius=0.0) == inv and render(ao=4, radius=NAN) == inv
    assert render(ao=4, r=5) == inv and render(ao=4, tol=-1.0) == inv and render(ao=4, cos=NAN) == inv and render(sem=8) == inv
    assert render(w=0) == inv and render(scene=None) == inv and render(v=None) == inv
    assert not buf.any()


# ---- the GPU cases are not vacuous: the oracle's word ----------------------------------------------------------------------

def _golden_frame(orc, name):
    osc, oview, w, h, g = golden_case(None, orc, name)
    prim, inst, _ = osc.trace_primary_inst(oview, w, h, sem=0)
    geo = LT.frame_geometry(oview, w, h, prim, inst, tri_records(g["tri_verts"]))
    return osc, oview, w, h, g, prim, geo


@pytest.mark.parametrize("name", sorted(LT.POINT_CASES))
def test_point_light_cases_have_back_facing_lit_and_shadowed_pixels(orc, name):
    """A point light at shadow_eps 0.01 over the oracle's TRX_SEM_HLSL primary records: back-facing (inert), lit and shadowed
    pixels are each at least 5 % of the surface pixels."""
    osc, oview, w, h, g, prim, geo = _golden_frame(orc, name)
    light = LT.Light(LT.POINT, LT.POINT_CASES[name])
    plane = LT.visibility_planes(orc, osc, oview, w, h, geo, prim, [light], 0, 1, 0.01, 0)[0]
    _, cast = LT.light_rays(orc, oview, w, h, geo, light, 0, 0, 0, 0.01)
    back, lit, shadowed = LT.shares(plane, cast)
    print("%s: %d surface pixels, %.1f %% back-facing, %.1f %% lit, %.1f %% shadowed" % (name, geo[0].size, 100 * back, 100 * lit, 100 * shadowed))
    assert abs(back + lit + shadowed - 1.0) < 1e-9 and min(back, lit, shadowed) >= 0.05, (name, back, lit, shadowed)


def test_rect_light_case_has_partly_lit_pixels_and_both_ends(orc):
    """The rect light of the GPU tests on cornell_tlas_48 at 8 samples: partly lit pixels (count strictly between 0 and 8), count 0
    and count 8 are each at least 5 % of the surface pixels."""
    osc, oview, w, h, g, prim, geo = _golden_frame(orc, "cornell_tlas_48")
    plane = LT.visibility_planes(orc, osc, oview, w, h, geo, prim, [LT.RECT_CASE], 0, 8, 0.01, 0)[0]
    surf = plane[plane != LT.NO_SURFACE]
    part, none, full = ((surf > 0) & (surf < 8)).mean(), (surf == 0).mean(), (surf == 8).mean()
    print("cornell_tlas_48 rect light: %d surface pixels, %.1f %% partly lit, %.1f %% count 0, %.1f %% count 8" % (surf.size, 100 * part, 100 * none, 100 * full))
    assert surf.size == geo[0].size and min(part, none, full) >= 0.05, (part, none, full)


def test_mask_case_changes_occlusion_flags(orc):
    """Hiding TLAS primitive 4 of cornell_tlas_48 from the shadow rays of the point light: the occlusion flag of at least 2 %
    of the surface pixels changes, all of them from shadowed to lit."""
    osc, oview, w, h, g, prim, geo = _golden_frame(orc, "cornell_tlas_48")
    light = LT.Light(LT.POINT, LT.POINT_CASES["cornell_tlas_48"])
    plane = LT.visibility_planes(orc, osc, oview, w, h, geo, prim, [light], 0, 1, 0.01, 0)[0]
    vis = np.ones(len(g["instance_offsets"]), dtype=bool)
    vis[LT.MASK_HIDES] = False
    masked = LT.visibility_planes(orc, oracle_twin(orc, LT.golden_flat(g), vis), oview, w, h, geo, prim, [light], 0, 1, 0.01, 0)[0]
    changed = (plane != masked).sum() / geo[0].size
    print("cornell_tlas_48 mask hiding primitive %d: %.1f %% of the surface pixels change" % (LT.MASK_HIDES, 100 * changed))
    assert changed >= 0.02 and (masked >= plane).all()
