"""The indirect-light pass without a GPU: the boundary (symbols, plain C, ABI version), the new kernels' resources, the twin
(tests/indirect_twin.py) held against the header's rules restated record by record in binary32 scalars, the refusals -
decided before a device is touched - the command line's options, and the oracle's word that the cases of
tests/test_gpu_indirect.py are not vacuous."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import indirect_twin as IT
import light_twin as LT
from ao_visibility_twin import golden_case
from hit_attr_twin import ATTR_DTYPE, tri_records
from inst_mask_twin import oracle_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tray_racing_amd", "tray_racing_hip")
HIT = np.dtype([("t", "<f4"), ("prim", "<u4")])
INF = float("inf")
F32_MAX = 3.4028234663852886e38
f32 = np.float32
NEW_SYMBOLS = ("trx_bounce_light_rays_dev", "trx_trace_indirect_dev", "trx_render_image_gi")


# ---- the boundary ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_bound(trx):
    from tray_racing_amd import _lib
    header = open(os.path.join(ROOT, "include", "trx.h")).read()
    dev = open(os.path.join(ROOT, "include", "trx_dev.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    lib = trx.load()
    for name in NEW_SYMBOLS + ("trx_debug_indirect_phases",):
        assert (" T %s\n" % name) in out and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for name in NEW_SYMBOLS:
        assert name + "(" in header
    assert "trx_debug_indirect_phases(" in dev and "trx_debug_indirect_phases" not in header
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [14, 19, 23]
    for name in ("bounce_light_rays_dev", "trace_indirect_dev", "render_image_gi"):
        assert callable(getattr(trx.Scene, name))
    # the header stays plain C11, and a caller can pass the new arguments
    src = (b'#include "trx.h"\n'
           b'int f(trx_scene *s, const trx_view *v, const trx_light *l, const trx_hit *p, float *out) {\n'
           b'    trx_shard whole = {0, 1, TRX_LAYOUT_IMAGE, 0};\n'
           b'    return trx_trace_indirect_dev(s, v, 8, 8, whole, 0, 0, l, 1, 0, TRX_MAX_AO_SAMPLES, 0.01f, 0.01f, 0.5f, p, 0, out, out, 0);\n}\n'
           b'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", "-I",
                    os.path.join(ROOT, "include"), "-"], input=src, check=True)
    assert lib.trx_abi_version() == 1   # additions only


def test_bounce_kernel_resources():
    """k_bounce_light_rays, k_bounce_weight, k_bounce_gather, k_bounce_finish (make build/kernels.s): streaming kernels - no
    scratch, no LDS, at most 128 VGPRs (the counts are printed)."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "tray_racing_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "build/kernels.s"], check=True, capture_output=True, timeout=900)
    text = open(os.path.join(csrc, "build", "kernels.s")).read()
    wanted = ("k_bounce_light_rays", "k_bounce_weight", "k_bounce_gather", "k_bounce_finish")
    found = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n.*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        name, body = m.group(2), m.group(3)
        key = [k for k in wanted if k in name]
        if not key:
            continue
        assert not any(k in name for k in ("k_trace", "k_shade", "k_ao_filter")), name   # (other tests count those names)
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        print("%s: %d VGPRs, %d B scratch, %d B LDS" % (name, vgprs, scratch, int(m.group(1))))
        assert scratch == 0 and vgprs <= 128, name
        found[key[0]] = int(m.group(1))
    assert found == {k: 0 for k in wanted}


def test_cli_lists_and_checks_the_bounce_flags():
    def run(*args):
        return subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=120)
    usage = run("--help")
    assert usage.returncode == 0
    for flag in ("--bounce-samples 1..64", "--bounce-albedo a", "--bounce-eps e"):
        assert flag in usage.stdout, flag
    base = ("-i", "standin:cornell", "--dry-run", "--passes", "1")
    pt = ("--light", "point:0,1.8,0")
    for extra, msg in ((("--png", "--bounce-samples", "4"), "--light"), ((*pt, "--bounce-samples", "4"), "--png"),
                       (("--png", *pt, "--bounce-samples", "0"), "1..64"), (("--png", *pt, "--bounce-samples", "65"), "1..64"),
                       (("--png", *pt, "--bounce-albedo", "0.5"), "go with --bounce-samples"), (("--png", *pt, "--bounce-eps", "0.1"), "go with --bounce-samples"),
                       (("--png", *pt, "--bounce-samples", "4", "--bounce-albedo", "-1"), ">= 0"),
                       (("--png", *pt, "--bounce-samples", "4", "--bounce-albedo", "inf"), "finite"),
                       (("--png", *pt, "--bounce-samples", "4", "--bounce-eps", "-0.1"), ">= 0"),
                       (("--png", *pt, "--bounce-samples", "4", "--bounce-eps", "nan"), ">= 0"),
                       (("--png", *pt, "--bounce-samples", "4", "--profile-rt", "nodes"), "not together"),
                       (("--png", *pt, "--bounce-samples", "4", "--ao-samples", "4", "--ao-stride", "2"), "not together")):
        r = run(*base, *extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert run(*base, "--png", *pt, "--bounce-samples", "1").returncode == 0
    assert run(*base, "--png", *pt, "--light", "rect:-0.4,1.9,-0.4:0.8,0,0:0,0,0.8:2", "--light-samples", "8", "--light-mask", "3", "--bounce-samples", "64",
               "--bounce-albedo", "0.8", "--bounce-eps", "0.001", "--ambient", "0.2", "--ao-samples", "4", "--ao-filter", "2").returncode == 0
    assert run(*base, "--png", *pt).returncode == 0          # (without the option: the direct-light image as before)


# ---- the twin against the header's rules, record by record in binary32 scalars ---------------------------------------------

def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _bounce_by_the_letter(ray, hit, attr):
    """(d, n, Q) of a bounce with a surface, or None."""
    if ray["tmax"] < 0 or not (hit["t"] < f32(F32_MAX)) or int(hit["prim"]) == 0xFFFFFFFF:
        return None
    d = [f32(x) for x in ray["direction"]]
    n = [f32(x) for x in attr["normal"]]
    sg = np.copysign(f32(1.0), _dot(n, [-d[0], -d[1], -d[2]]))
    n = [n[0] * sg, n[1] * sg, n[2] * sg]
    t = f32(hit["t"])
    Q = [f32(ray["origin"][c]) + d[c] * t for c in range(3)]
    return d, n, Q


def _ray_by_the_letter(orc, w, ray, hit, attr, light, k, frame0, f, eps, i):
    """The eight words of the secondary shadow ray of record i."""
    inert = np.array([0, 0, 0, 0, 0, 0, 0, -1.0], dtype=np.float32)
    b = _bounce_by_the_letter(ray, hit, attr)
    if b is None:
        return inert
    d, n, Q = b
    eps = f32(eps)
    o = [Q[c] - d[c] * eps for c in range(3)]
    if light.kind == LT.DIRECTIONAL:
        p = [f32(x) for x in light.position]
        inv = f32(1.0) / np.sqrt(_dot(p, p))
        l, tmax = [p[0] * inv, p[1] * inv, p[2] * inv], LT.F32_MAX
    else:
        L = [f32(x) for x in light.position]
        if light.kind == LT.RECT:
            seed = (frame0 + k * 64 + f) & 0xFFFFFFFF
            u1 = f32(orc.load().orc_hash_noise(i % w, i // w, seed))
            u2 = f32(orc.load().orc_hash_noise(i % w, i // w, (seed + 1024) & 0xFFFFFFFF))
            L = [(L[c] + u1 * f32(light.edge1[c])) + u2 * f32(light.edge2[c]) for c in range(3)]
        v = [L[c] - o[c] for c in range(3)]
        dist = np.sqrt(_dot(v, v))
        inv = f32(1.0) / dist
        l, tmax = [v[0] * inv, v[1] * inv, v[2] * inv], min(dist, LT.F32_MAX) if dist == dist else LT.F32_MAX
    if not (_dot(n, l) > f32(0.0)):
        return inert
    return np.array(o + [f32(0.0)] + l + [tmax], dtype=np.float32)


def _g_by_the_letter(ray, hit, attr, light):
    d, n, Q = _bounce_by_the_letter(ray, hit, attr)
    if light.kind == LT.DIRECTIONAL:
        p = [f32(x) for x in light.position]
        inv = f32(1.0) / np.sqrt(_dot(p, p))
        return _dot(n, [p[0] * inv, p[1] * inv, p[2] * inv])
    Cc = [f32(x) for x in light.position]
    if light.kind == LT.RECT:
        Cc = [(Cc[c] + f32(0.5) * f32(light.edge1[c])) + f32(0.5) * f32(light.edge2[c]) for c in range(3)]
    v = [Cc[c] - Q[c] for c in range(3)]
    q = _dot(v, v)
    inv = f32(1.0) / np.sqrt(q)
    return _dot(n, [v[0] * inv, v[1] * inv, v[2] * inv]) / q


def _hand_made(orc, w, h, seed):
    """Primary records (hits, misses of both kinds) and, per sample, hand-made bounce rays, hits and attribute records: bounces
    with a surface at several depths, bounce misses of both kinds, inert bounce rays where the primary record is a miss."""
    rng = np.random.default_rng(seed)
    n = w * h
    prim = np.zeros(n, dtype=HIT)
    prim["t"] = rng.choice(np.array([1.0, 2.25, INF, F32_MAX], dtype=np.float32), n, p=[.45, .4, .1, .05])
    prim["prim"] = np.where(rng.random(n) < 0.1, 0xFFFFFFFF, rng.integers(0, 40, n)).astype(np.uint32)
    surf = LT.surface(prim)
    samples = []
    for f in range(3):
        rays = np.zeros(n, dtype=orc.RAY_DTYPE)
        rays["tmax"] = f32(-1.0)
        d = rng.normal(size=(n, 3)).astype(np.float32)
        d /= np.linalg.norm(d, axis=1)[:, None].astype(np.float32)
        rays["origin"][surf] = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)[surf]
        rays["direction"][surf] = d[surf]
        rays["tmax"][surf] = f32(F32_MAX)
        hits = np.zeros(n, dtype=HIT)
        hits["t"] = rng.choice(np.array([0.5, 1.75, 3.0, INF, F32_MAX], dtype=np.float32), n, p=[.3, .25, .2, .15, .1])
        hits["prim"] = np.where(rng.random(n) < 0.1, 0xFFFFFFFF, rng.integers(0, 40, n)).astype(np.uint32)
        hits["t"][~surf], hits["prim"][~surf] = INF, 0xFFFFFFFF
        attr = np.zeros(n, dtype=ATTR_DTYPE)
        nn = rng.normal(size=(n, 3)).astype(np.float32)
        attr["normal"] = nn / np.linalg.norm(nn, axis=1)[:, None].astype(np.float32)
        samples.append((rays, hits, attr))
    return prim, samples


@pytest.mark.parametrize("w,h", [(7, 3), (33, 9)])
def test_twin_equals_the_rules_by_the_letter(orc, w, h):
    eps, albedo, frame0 = 0.01, 0.6, 5
    prim, samples = _hand_made(orc, w, h, 17 * w + h)
    n = w * h
    rays0, hits0, attr0 = samples[0]
    has0 = np.flatnonzero(IT.bounce_surface(rays0, hits0))
    assert 3 < has0.size < LT.surface(prim).sum()                           # (bounce misses among the surface pixels)
    # a point light exactly at the secondary shadow ray's origin of one bounce of sample 0: dist == 0, NaN, the inert ray
    j = int(has0[2])
    d, _, Q = _bounce_by_the_letter(rays0[j], hits0[j], attr0[j])
    at_hit = LT.Light(LT.POINT, [Q[c] - d[c] * f32(eps) for c in range(3)])
    lights = [LT.Light(LT.POINT, (0.4, 1.5, 0.8), intensity=2.0), LT.Light(LT.DIRECTIONAL, (0.3, 1.0, 0.2), intensity=0.75),
              LT.Light(LT.RECT, (-0.5, 1.6, -0.5), (1.0, 0.0, 0.1), (0.0, 0.2, 1.0), intensity=1.5), at_hit,
              LT.Light(LT.POINT, (-3.0, -2.0, 0.5), intensity=40.0)]
    rng = np.random.default_rng(w)
    occ = rng.random((len(samples), len(lights), n)) < 0.3                 # the any-hit answers, hand-made
    n_cast = n_back = 0
    sums = []
    with np.errstate(all="ignore"):
        for f, (rays, hits, attr) in enumerate(samples):
            casts = []
            for k, light in enumerate(lights):
                got, cast = IT.secondary_rays(orc, w, h, rays, hits, attr, light, k, frame0, f, eps)
                got = got.view(np.uint32).reshape(-1, 8)
                for i in range(n):
                    want = _ray_by_the_letter(orc, w, rays[i], hits[i], attr[i], light, k, frame0, f, eps, i).view(np.uint32)
                    assert (got[i] == want).all(), (f, k, i, got[i], want)
                    assert bool(cast[i]) == (want[7] != 0xBF800000)
                has = IT.bounce_surface(rays, hits)
                n_cast += int(cast.sum())
                n_back += int((has & ~cast).sum())                          # (back-facing secondary hits: inert)
                assert not cast[~has].any()
                if k == 3 and f == 0:
                    assert has[j] and not cast[j]                           # the light at the secondary hit: NaN, inert
                casts.append(cast)
            s = IT.sample_sum(orc, w, h, rays, hits, attr, lights, frame0, f, eps, lambda k, r: occ[f, k])
            want_s = np.zeros(n, dtype=np.float32)
            for i in range(n):
                sf = f32(0.0)
                for k, light in enumerate(lights):
                    if casts[k][i] and not occ[f, k, i]:
                        g = _g_by_the_letter(rays[i], hits[i], attr[i], light)
                        if g > f32(0.0):
                            sf = sf + f32(light.intensity) * g
                want_s[i] = sf
            assert (s.view(np.uint32) == want_s.view(np.uint32)).all(), (f, np.flatnonzero(s.view(np.uint32) != want_s.view(np.uint32))[:4])
            sums.append(s)
        assert n_cast > n // 2 and n_back > n // 4
        base = rng.uniform(0.0, 1.0, n).astype(np.float32)
        base[::5] = f32(-0.0)
        for b in (None, base):
            got = IT.term(sums, prim, albedo, b)
            want = np.zeros(n, dtype=np.float32)
            for i in range(n):
                bi = f32(0.0) if b is None else b[i]
                if not (prim["t"][i] < f32(F32_MAX) and int(prim["prim"][i]) != 0xFFFFFFFF):
                    want[i] = bi
                    continue
                A = f32(0.0)
                for s in sums:
                    A = A + s[i]
                want[i] = bi + (f32(albedo) * A) / f32(len(sums))
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:4]
            assert (got[LT.surface(prim)] != (0 if b is None else b[LT.surface(prim)])).any()
        # one sample, no base: the term is albedo * s
        assert (IT.term(sums[:1], prim, 1.0).view(np.uint32)[LT.surface(prim)] == (f32(0.0) + sums[0]).view(np.uint32)[LT.surface(prim)]).all()


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
    whole = _lib.Shard(0, 1, 0, 0)

    def arr(*lights):
        return trx.light_array(lights)

    def bad_lights():
        out = [(arr(good, trx.light(3, (0, 1, 0))), b"kind")]
        l = trx.light(trx.LIGHT_RECT, (0, 1, 0), (1, 0, 0), (0, 0, 1))
        l._pad[3] = 1
        out.append((arr(l), b"_pad"))
        for field, x in (("position", NAN), ("edge1", INF), ("edge2", -INF)):
            l = trx.light(trx.LIGHT_RECT, (0, 1, 0), (1, 0, 0), (0, 0, 1))
            getattr(l, field)[1] = x
            out.append((arr(good, l), b"finite"))
        out.append((arr(trx.light(trx.LIGHT_POINT, (0, 1, 0), intensity=INF)), b"finite"))
        out.append((arr(trx.light(trx.LIGHT_DIRECTIONAL, (0, 0, 0))), b"zero length"))
        return out

    def pas(scene=fake, v=C.byref(view), w=4, h=4, shard=whole, sem=0, mask=0, lights=arr(good), n_lights=None, n=4, beps=0.01, seps=0.01,
            albedo=0.5, prim=P, base=None, out=P):
        return lib.trx_trace_indirect_dev(scene, v, w, h, shard, sem, mask, lights, len(lights) if n_lights is None else n_lights, 0, n, beps, seps,
                                          albedo, prim, None, base, out, None)

    assert pas(n_lights=0) == inv and b"n_lights" in lib.trx_last_error()
    assert pas(lights=arr(*[good] * 9)) == inv and b"n_lights" in lib.trx_last_error()
    assert pas(lights=None, n_lights=1) == inv and b"null" in lib.trx_last_error()
    for lights, msg in bad_lights():
        assert pas(lights=lights) == inv and msg in lib.trx_last_error(), msg
    assert pas(n=0) == inv and b"n_samples" in lib.trx_last_error()
    assert pas(n=65) == inv and b"n_samples" in lib.trx_last_error()
    assert pas(mask=256) == inv and b"ray_mask" in lib.trx_last_error()
    for eps in (NAN, -0.01, -INF):
        assert pas(seps=eps) == inv and b"shadow_eps" in lib.trx_last_error()
        assert pas(beps=eps) == inv and b"bounce_eps" in lib.trx_last_error()
    for albedo in (NAN, INF, -INF):
        assert pas(albedo=albedo) == inv and b"bounce_albedo" in lib.trx_last_error()
    assert pas(sem=8) == inv and b"semantics" in lib.trx_last_error()
    assert pas(w=0) == inv and pas(h=0) == inv and pas(v=None) == inv
    assert pas(shard=_lib.Shard(3, 3, 0, 0)) == inv and pas(shard=_lib.Shard(0, 1, 2, 0)) == inv
    for kw in ({"scene": None}, {"prim": None}, {"out": None}):
        assert pas(**kw) == inv and b"null" in lib.trx_last_error()

    def rays(scene=fake, w=4, h=4, shard=whole, light=good, k=0, f=0, eps=0.01, br=P, bh=P, ba=P, out=P):
        return lib.trx_bounce_light_rays_dev(scene, w, h, shard, C.byref(light) if light is not None else None, k, 0, f, eps, br, bh, ba, out, None)

    for lights, msg in bad_lights():
        assert rays(light=lights[len(lights) - 1]) == inv and msg in lib.trx_last_error(), msg
    assert rays(light=None) == inv and rays(k=8) == inv and b"light_index" in lib.trx_last_error()
    assert rays(f=64) == inv and b"sample" in lib.trx_last_error()
    assert rays(eps=NAN) == inv and rays(eps=-1.0) == inv and b"shadow_eps" in lib.trx_last_error()
    assert rays(w=0) == inv and rays(h=0) == inv and rays(shard=_lib.Shard(2, 2, 0, 0)) == inv
    for kw in ({"scene": None}, {"br": None}, {"bh": None}, {"ba": None}, {"out": None}):
        assert rays(**kw) == inv and b"null" in lib.trx_last_error()

    def render(scene=fake, v=C.byref(view), w=4, h=4, sem=0, mask=0, lights=arr(good), n_lights=None, n=4, eps=0.01, ambient=0.1, ao=0, radius=INF,
               r=0, tol=0.02, cos=0.9, bn=4, beps=0.01, albedo=0.5):
        return lib.trx_render_image_gi(scene, v, w, h, sem, mask, lights, len(lights) if n_lights is None else n_lights, 0, n, eps, ambient, ao, 0.01,
                                       radius, r, tol, cos, bn, beps, albedo, P, None)

    for lights, msg in bad_lights():
        assert render(lights=lights) == inv and msg in lib.trx_last_error(), msg
    assert render(n_lights=0) == inv and render(n_lights=9) == inv and render(n=0) == inv and render(n=65) == inv
    assert render(mask=256) == inv and render(eps=NAN) == inv and render(eps=-1.0) == inv and render(ambient=NAN) == inv
    assert render(ao=65) == inv and render(ao=4, radius=0.0) == inv and render(ao=4, r=5) == inv and render(sem=8) == inv
    assert render(bn=0) == inv and b"bounce_samples" in lib.trx_last_error()
    assert render(bn=65) == inv and b"bounce_samples" in lib.trx_last_error()
    assert render(beps=NAN) == inv and render(beps=-1.0) == inv and b"bounce_eps" in lib.trx_last_error()
    assert render(albedo=NAN) == inv and render(albedo=INF) == inv and b"bounce_albedo" in lib.trx_last_error()
    assert render(w=0) == inv and render(scene=None) == inv and render(v=None) == inv
    assert lib.trx_debug_indirect_phases(None, C.byref(view), 4, 4, 0, 0, arr(good), 1, 0, 4, 0.01, 0.01, 0.5, P, None, None, P, None) == inv
    assert not buf.any()


# ---- the GPU cases are not vacuous: the oracle's word ----------------------------------------------------------------------

def _measure(orc, name, shadow_hidden=None):
    osc, oview, w, h, g = golden_case(None, orc, name)
    prim, inst, _ = osc.trace_primary_inst(oview, w, h, sem=0)
    recs = tri_records(g["tri_verts"])
    light = LT.Light(LT.POINT, LT.POINT_CASES[name])
    stats, cache = [], {}
    out = IT.indirect(orc, osc, oview, w, h, prim, inst, recs, None, [light], 0, 4, 0.01, 0.01, 0.5, 0, stats=stats, cache=cache)
    masked = None
    if shadow_hidden is not None:
        vis = np.ones(len(g["instance_offsets"]), dtype=bool)
        vis[shadow_hidden] = False
        masked = IT.indirect(orc, osc, oview, w, h, prim, inst, recs, None, [light], 0, 4, 0.01, 0.01, 0.5, 0,
                             shadow_osc=oracle_twin(orc, LT.golden_flat(g), vis), cache=cache)
    surf = LT.surface(prim)
    hit = np.stack([s[0] for s in stats])[:, surf]
    cast = np.stack([s[1][0][0] for s in stats])[:, surf]
    occ = np.stack([s[1][0][1] for s in stats])[:, surf]
    assert not (cast & ~hit).any()
    n_hit = max(int(hit.sum()), 1)
    lit, back, shadowed = (cast & ~occ).sum() / n_hit, (hit & ~cast).sum() / n_hit, (cast & occ).sum() / n_hit
    per = (cast & ~occ).sum(0)
    print("%s: %d surface pixels, %.1f %% of the bounce samples hit; of those %.1f %% lit, %.1f %% back-facing, %.1f %% shadowed; "
          "pixels with 0 / some / all 4 samples lit %.1f / %.1f / %.1f %%" % (name, surf.sum(), 100 * hit.mean(), 100 * lit, 100 * back, 100 * shadowed,
                                                                              100 * (per == 0).mean(), 100 * ((per > 0) & (per < 4)).mean(), 100 * (per == 4).mean()))
    assert (out[~surf] == 0).all() and ((out[surf] > 0) == (per > 0)).all()
    return hit.mean(), lit, back, shadowed, out, masked, surf


@pytest.mark.parametrize("name", sorted(LT.POINT_CASES))
def test_point_light_cases_have_hits_and_lit_back_facing_and_shadowed_bounces(orc, name):
    """sem 0, seeds 0..3, both offsets 0.01, 4 samples, the point light of light_twin.POINT_CASES: at least 5 % of the bounce
    samples hit, and lit, back-facing and shadowed bounces are each at least 5 % of those."""
    hit, lit, back, shadowed, _, _, _ = _measure(orc, name)
    assert abs(lit + back + shadowed - 1.0) < 1e-9 and min(hit, lit, back, shadowed) >= 0.05, (name, hit, lit, back, shadowed)


def test_mask_case_changes_values(orc):
    """Hiding TLAS primitive 4 of cornell_tlas_48 from the secondary shadow rays: the value of at least 8 % of the surface
    pixels changes (the oracle gives 16.6 %), every one of them upward - a hidden instance casts no shadow; the bounce rays
    still see it."""
    _, _, _, _, out, masked, surf = _measure(orc, "cornell_tlas_48", shadow_hidden=LT.MASK_HIDES)
    changed = (out.view(np.uint32) != masked.view(np.uint32))[surf].mean()
    print("cornell_tlas_48 mask hiding primitive %d: %.1f %% of the surface pixels change" % (LT.MASK_HIDES, 100 * changed))
    assert changed >= 0.08 and (masked >= out).all()
