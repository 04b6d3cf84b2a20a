"""The sparse indirect term without a GPU (include/trx.h: trx_trace_indirect_sparse_dev, trx_value_upsample_dev,
trx_render_image_gi_sparse): the boundary (symbols, plain C, ABI version), the twin (tests/indirect_sparse_twin.py) held
against the header's rules restated pixel by pixel in binary32 scalars and on hand-made images that reach every branch by
construction, identities of the twin, the refusals - decided before a device is touched - the new kernels' resources, the
command line's options, the oracle's word that the cases of tests/test_gpu_indirect_sparse.py are not vacuous, and what the
pass is for: the error of the sparse, upsampled and filtered 4-sample term against a 64-sample dense one."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import indirect_sparse_twin as ST
import light_twin as LT
import value_filter_twin as VT
from ao_sparse_twin import ACCEPTED, EMPTY, FALLBACK, NOT_SURFACE, ao_upsample, cell_pixels, class_counts, lo_size, phase_xy
from test_ao_sparse import _golden_records
from test_value_filter import _golden_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tray_racing_amd", "tray_racing_hip")
INF = float("inf")
NAN = float("nan")
f32 = np.float32
NEW_SYMBOLS = ("trx_trace_indirect_sparse_dev", "trx_value_upsample_dev", "trx_render_image_gi_sparse")
TOL, COS = 0.10, 0.9          # the value filter's tolerance pair (tests/test_value_filter.py)
GRIDS = ((1, 0), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0), (3, 8), (4, 0), (4, 15))   # (stride, phase): all phases at 2, first and last at 3, 4


# ---- the boundary ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_bound(trx):
    from tray_racing_amd import _lib
    header = open(os.path.join(ROOT, "include", "trx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    lib = trx.load()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and (" T %s\n" % name) in out and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [19, 14, 29]
    assert _lib.SIGNATURES["trx_render_image_gi_sparse"][1][:24] == _lib.SIGNATURES["trx_render_image_gi_filtered"][1][:24]
    for name in ("trace_indirect_sparse_dev", "value_upsample_dev", "render_image_gi_sparse"):
        assert callable(getattr(trx.Scene, name))
    assert _lib.MAX_VALUE_UPSAMPLE_RADIUS == ST.MAX_RADIUS == 2
    # the header stays plain C11, and a caller can pass the new arguments
    src = (b'#include "trx.h"\n'
           b'_Static_assert(TRX_MAX_VALUE_UPSAMPLE_RADIUS == 2, "radius");\n'
           b'int f(trx_scene *s, const trx_view *v, const trx_light *l, const trx_hit *p, const trx_hit_attr *a, float *lo, float *out,\n'
           b'      unsigned char *rgba) {\n'
           b'    int rc = trx_trace_indirect_sparse_dev(s, v, 8, 8, TRX_MAX_AO_STRIDE, 15, 0, 0, l, 1, 0, TRX_MAX_AO_SAMPLES, 0.01f, 0.01f, 0.5f, p, 0, lo, 0);\n'
           b'    if (rc) return rc;\n'
           b'    rc = trx_value_upsample_dev(s, 8, 8, TRX_MAX_AO_STRIDE, 15, p, a, lo, out, TRX_MAX_VALUE_UPSAMPLE_RADIUS, 0.1f, 0.9f, out, 0);\n'
           b'    if (rc) return rc;\n'
           b'    return trx_render_image_gi_sparse(s, v, 8, 8, 0, 0, l, 1, 0, 1, 0.01f, 0.1f, 0, 0.01f, 1.0f, 0, 0.02f, 0.9f, 4, 0.01f, 0.5f, 3, 0.1f, 0.9f,\n'
           b'                                      2, 3, 1, rgba, 0);\n}\n'
           b'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", "-I",
                    os.path.join(ROOT, "include"), "-"], input=src, check=True)
    assert lib.trx_abi_version() == 1   # additions only


def test_new_kernel_resources():
    """k_plane_upsample<NORMALS> (make build/image.s): no scratch, at most 128 VGPRs, LDS at most 64 KiB and exactly the 432
    cells of image.h - 20 bytes each with normals, 8 without; its name holds none of the substrings other tests select the
    image kernels by.  The sparse instantiations of k_bounce_light_rays and k_bounce_finish (make build/kernels.s): streaming
    kernels - no scratch, no LDS, at most 128 VGPRs.  The numbers are printed."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "tray_racing_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "build/image.s", "build/kernels.s"], check=True, capture_output=True, timeout=900)

    def kernels(file, select):
        text = open(os.path.join(csrc, "build", file)).read()
        for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n.*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
            name, body = m.group(2), m.group(3)
            if not select(name):
                continue
            vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
            sgprs = int(re.search(r"\.sgpr_count:\s+(\d+)", body).group(1))
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
            print("%s: %d VGPRs, %d SGPRs, %d B scratch, %d B LDS" % (name, vgprs, sgprs, scratch, int(m.group(1))))
            assert scratch == 0 and vgprs <= 128 and int(m.group(1)) <= 65536, name
            yield name, int(m.group(1))

    lds = []
    for name, size in kernels("image.s", lambda n: "k_plane_upsample" in n):
        assert not any(k in name for k in ("k_ao_filter", "k_ao_upsample", "k_shade", "k_value", "k_atrous", "k_heat", "k_trace")), name
        lds.append(size)
    assert sorted(lds) == [432 * 8, 432 * 20], lds
    sparse = dict(kernels("kernels.s", lambda n: ("k_bounce_light_rays" in n or "k_bounce_finish" in n) and "ILb1E" in n))
    assert len(sparse) == 2 and set(sparse.values()) == {0}, sparse


def test_cli_lists_and_checks_the_stride_flags():
    def run(*args):
        return subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=120)
    usage = run("--help")
    assert usage.returncode == 0
    for flag in ("--bounce-stride 1..4", "--bounce-phase P", "--bounce-upsample 0..2"):
        assert flag in usage.stdout, flag
    base = ("-i", "standin:cornell", "--dry-run", "--passes", "1", "--png", "--light", "point:0,1.8,0")
    bn = ("--bounce-samples", "4")
    for extra, msg in ((("--bounce-stride", "2"), "--bounce-samples"), ((*bn, "--bounce-stride", "0"), "1..4"), ((*bn, "--bounce-stride", "5"), "1..4"),
                       ((*bn, "--bounce-stride", "2", "--bounce-phase", "4"), "S*S-1"), ((*bn, "--bounce-stride", "1", "--bounce-phase", "1"), "S*S-1"),
                       ((*bn, "--bounce-stride", "2", "--bounce-phase", "-1"), "S*S-1"),
                       ((*bn, "--bounce-stride", "2", "--bounce-upsample", "3"), "0..2"), ((*bn, "--bounce-stride", "2", "--bounce-upsample", "-1"), "0..2"),
                       ((*bn, "--bounce-phase", "1"), "--bounce-stride"), ((*bn, "--bounce-upsample", "1"), "--bounce-stride"),
                       ((*bn, "--bounce-filter-tol", "0.1"), "go with --bounce-filter"),
                       ((*bn, "--bounce-stride", "2", "--ao-samples", "4", "--ao-stride", "2"), "not together")):
        r = run(*base, *extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert run(*base, *bn, "--bounce-stride", "2").returncode == 0
    assert run(*base, *bn, "--bounce-stride", "4", "--bounce-phase", "15", "--bounce-upsample", "2", "--bounce-filter", "3").returncode == 0
    assert run(*base, *bn, "--bounce-stride", "3", "--bounce-upsample", "0", "--bounce-filter-tol", "inf", "--bounce-filter-cos", "-1", "--ao-samples", "4",
               "--ao-filter", "2").returncode == 0
    assert run(*base, *bn).returncode == 0 and run(*base, *bn, "--bounce-filter", "3").returncode == 0   # (without the option: as before)


# ---- the twin against the header's rules, pixel by pixel in binary32 scalars ---------------------------------------------

def _by_the_letter(prim, normals, lo, w, h, s, phase, r, depth_tol, normal_cos, base):
    """(values, classes): the header's rules, pixel by pixel and cell by cell."""
    px0, py0 = phase % s, phase // s
    wlo, hlo = (w + s - 1) // s, (h + s - 1) // s
    t, pr = prim["t"], prim["prim"]
    tol, cos = f32(depth_tol), f32(normal_cos)
    surf = [bool(t[i] < f32(VT.F32_MAX)) and int(pr[i]) != 0xFFFFFFFF for i in range(w * h)]
    out = np.zeros(w * h, dtype=np.float32)
    cls = np.zeros(w * h, dtype=np.uint8)
    for y in range(h):
        for x in range(w):
            p = y * w + x
            if not surf[p]:
                if base is not None:
                    out.view(np.uint32)[p] = base.view(np.uint32)[p]
                continue
            tp = f32(t[p])
            num, den, num_all, den_all = f32(0.0), f32(0.0), f32(0.0), f32(0.0)
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    X, Y = x // s + dx, y // s + dy
                    if not (0 <= X < wlo and 0 <= Y < hlo):
                        continue                                   # clipped to the low grid
                    gx, gy = X * s + px0, Y * s + py0
                    if gx >= w or gy >= h or not surf[gy * w + gx]:
                        continue                                   # no surface cell: never looked at
                    q = gy * w + gx
                    wgt = f32((r + 1 - abs(dy)) * (r + 1 - abs(dx)))
                    u = f32(lo[Y * wlo + X])
                    ok = bool(np.abs(f32(t[q]) - tp) <= tol * tp)
                    if ok and normals is not None:
                        a, b = normals[p], normals[q]
                        ok = bool((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2] >= cos)
                    if ok or q == p:
                        num = num + wgt * u
                        den = den + wgt
                    num_all = num_all + wgt * u
                    den_all = den_all + wgt
            if den > 0:
                F, cls[p] = num / den, ACCEPTED
            elif den_all > 0:
                F, cls[p] = num_all / den_all, FALLBACK
            else:
                F, cls[p] = f32(0.0), EMPTY
            assert float(den_all) == int(den_all) and den_all <= (r + 1) ** 4
            out[p] = F if base is None else base[p] + F
    return out, cls


def _low_plane(prim, values, w, h, s, phase, seed):
    """A low plane for the upsample: the image's values at the cells' pixels - -0.0f, +inf and a NaN among them - and a NaN in
    every cell without a surface or outside the image: such a cell must never be looked at."""
    gx, gy, inside = cell_pixels(w, h, s, phase)
    surf = VT.surface(prim).reshape(h, w)
    lo = np.full(gx.shape, NAN, dtype=np.float32)
    take = inside.copy()
    take[inside] = surf[gy[inside], gx[inside]]
    lo[take] = values.reshape(h, w)[gy[take], gx[take]]
    flat = lo.reshape(-1)
    at = np.flatnonzero(take.reshape(-1))
    if at.size > 6:
        rng = np.random.default_rng(seed)
        pick = rng.choice(at, 3, replace=False)
        flat[pick[0]], flat[pick[1]], flat[pick[2]] = f32(INF), f32(NAN), f32(-0.0)
    return flat


def _images():
    for w, h in VT.HAND_SIZES:
        yield "%dx%d with misses" % (w, h), w, h, VT.hand_made(w, h, 17 * w + h, misses=True)
    for w, h in VT.HAND_SIZES[1:3]:
        yield "%dx%d all-surface" % (w, h), w, h, VT.hand_made(w, h, 31 * w + h, misses=False)
    yield "7x3 of misses", 7, 3, VT.all_misses(7, 3, 5)


@pytest.mark.parametrize("name,w,h,rec", list(_images()), ids=[i[0].replace(" ", "_") for i in _images()])
def test_twin_upsample_equals_the_rules_by_the_letter(name, w, h, rec):
    """Hand-made records with a depth step, a normal crease and misses of both kinds; strides 1..4 (all phases at 2, the first
    and the last at 3 and 4), radii 0..2, with and without normals; values -0.0f, +inf and NaN among the cells; no base, a base
    with -0.0f in it.  NaN-ness is compared, not the payload."""
    prim, nrm, values, base = rec
    assert (base.view(np.uint32) == 0x80000000).any()
    big = w * h > 1000
    grids = ((2, 0), (2, 3), (3, 8), (4, 15), (1, 0)) if big else GRIDS
    seen, n_special = set(), 0
    with np.errstate(all="ignore"):
        for s, phase in grids:
            lo = _low_plane(prim, values, w, h, s, phase, 7 * s + phase)
            for r in (0, 1, 2):
                for normals, tol, cos in ((nrm, TOL, COS),) if big else ((nrm, TOL, COS), (None, TOL, COS), (nrm, INF, -1.0), (nrm, 0.0, 1.0)):
                    for b in (None, base):
                        got, cls = ST.value_upsample(prim, normals, lo, w, h, s, phase, r, tol, cos, base=b, classes=True)
                        want, wcls = _by_the_letter(prim, normals, lo, w, h, s, phase, r, tol, cos, b)
                        bad = VT.same_bits(got, want)
                        assert bad.size == 0 and (cls == wcls).all(), (name, s, phase, r, normals is None, tol, cos, b is None, bad[:4], got[bad[:4]], want[bad[:4]])
                        assert (got.view(np.uint32)[cls == NOT_SURFACE] == (0 if b is None else b.view(np.uint32)[cls == NOT_SURFACE])).all()
                        if b is None:
                            assert not got.view(np.uint32)[cls == EMPTY].any()
                        seen |= set(np.unique(cls).tolist())
                        n_special += int(np.isnan(got).sum() + np.isinf(got).sum())
    if "of misses" in name:
        assert seen == {NOT_SURFACE}
    elif w * h > 100:
        assert {ACCEPTED, FALLBACK} <= seen and n_special > 0, (name, seen)
        if "with misses" in name:
            assert {NOT_SURFACE, EMPTY} <= seen, (name, seen)


def test_rejected_cells_keep_nan_and_inf_out():
    """Everything but the own cell rejected (tolerance 0, cosine 1 on jittered records): no NaN and no infinity leaves its own
    cell's pixels; everything accepted: they spread."""
    w, h = 33, 9
    prim, nrm, values, _ = VT.hand_made(w, h, 3, misses=False)
    lo = np.ones(lo_size(w, h, 2)[0] * lo_size(w, h, 2)[1], dtype=np.float32)
    lo[20], lo[40] = f32(NAN), f32(INF)
    with np.errstate(all="ignore"):
        tight, cls = ST.value_upsample(prim, nrm, lo, w, h, 2, 0, 2, 0.0, 1.0, classes=True)
        loose = ST.value_upsample(prim, nrm, lo, w, h, 2, 0, 2, INF, -1.0)
    gx, gy, _ = cell_pixels(w, h, 2, 0)
    own = np.zeros(w * h, dtype=bool)
    own[(gy * w + gx).reshape(-1)] = True
    acc = cls == ACCEPTED
    assert acc[own].all() and (tight[own] == lo).sum() == lo.size - 1          # the pixel of a cell takes its cell, alone (NaN != NaN)
    assert np.isnan(tight[acc]).sum() == 1 and np.isinf(tight[acc]).sum() == 1
    assert np.isnan(loose).sum() > 8 and np.isinf(loose).sum() > 8


# ---- accepted, FALLBACK and EMPTY by hand ----------------------------------------------------------------------------------

def _image(w, h, t=2.0):
    prim = np.zeros(w * h, dtype=VT.HIT)
    prim["t"], prim["prim"] = t, 7
    return prim, np.tile(np.array([0, 0, 1], dtype=np.float32), (w * h, 1))


def test_accepted_fallback_and_empty_by_hand():
    w, h = 4, 4
    prim, normals = _image(w, h)
    lo = np.array([1, 2, 3, 4], dtype=np.float32)                 # stride 2, phase 0: the cells of pixels (0,0) (2,0) (0,2) (2,2)
    out, cls = ST.value_upsample(prim, normals, lo, w, h, 2, 0, 0, 0.02, 0.9, classes=True)
    assert (out.reshape(h, w) == [[1, 1, 2, 2], [1, 1, 2, 2], [3, 3, 4, 4], [3, 3, 4, 4]]).all() and (cls == ACCEPTED).all()
    out, cls = ST.value_upsample(prim, normals, lo, w, h, 2, 0, 1, 0.02, 0.9, classes=True)
    v = out.reshape(h, w)
    # radius 1: the centre cell weighs 4, an edge neighbour 2, the diagonal one 1; the window is clipped to the 2 x 2 grid
    assert v[0, 0] == (((f32(4) * f32(1) + f32(2) * f32(2)) + f32(2) * f32(3)) + f32(1) * f32(4)) / f32(9)
    assert v[3, 3] == (((f32(1) * f32(1) + f32(2) * f32(2)) + f32(2) * f32(3)) + f32(4) * f32(4)) / f32(9) and (cls == ACCEPTED).all()
    # FALLBACK: pixel (1, 1) lies behind a depth step no cell shares
    prim["t"].reshape(h, w)[1, 1] = 10.0
    for r, want in ((0, f32(1)), (1, v[0, 0])):
        out, cls = ST.value_upsample(prim, normals, lo, w, h, 2, 0, r, 0.02, 0.9, classes=True)
        assert out.reshape(h, w)[1, 1] == want and cls.reshape(h, w)[1, 1] == FALLBACK and (np.delete(cls, 5) == ACCEPTED).all()
    # ... and a tolerance that reaches across the step accepts them again
    out, cls = ST.value_upsample(prim, normals, lo, w, h, 2, 0, 0, 1.0, 0.9, classes=True)
    assert cls.reshape(h, w)[1, 1] == ACCEPTED and out.reshape(h, w)[1, 1] == 1
    # EMPTY: the only cell of the window has no surface (a miss at its pixel; its value is never looked at)
    prim["t"].reshape(h, w)[0, 0], prim["prim"].reshape(h, w)[0, 0], lo[0] = INF, 0xFFFFFFFF, NAN
    base = np.full(w * h, 0.25, dtype=np.float32)
    for b in (None, base):
        out, cls = ST.value_upsample(prim, normals, lo, w, h, 2, 0, 0, 0.02, 0.9, base=b, classes=True)
        c, v0 = cls.reshape(h, w), out.reshape(h, w)
        assert c[0, 0] == NOT_SURFACE and c[0, 1] == EMPTY and c[1, 0] == EMPTY and c[1, 1] == EMPTY and c[0, 2] == ACCEPTED
        assert (v0[:2, :2] == (0.0 if b is None else 0.25)).all() and v0[0, 2] == (2.0 if b is None else 2.25)
    out, cls = ST.value_upsample(prim, normals, lo, w, h, 2, 0, 1, 0.02, 0.9, classes=True)
    c, v1 = cls.reshape(h, w), out.reshape(h, w)
    assert c[0, 1] == ACCEPTED and v1[0, 1] == ((f32(2) * f32(2) + f32(2) * f32(3)) + f32(1) * f32(4)) / f32(5) and c[1, 1] == FALLBACK
    assert not np.isnan(out).any()
    # the classes are the count upsample's
    _, acls = ao_upsample(prim, normals, np.array([0xFF, 2, 3, 4], dtype=np.uint8), w, h, 2, 0, 4, 1, 0.02, 0.9, classes=True)
    assert (acls == cls).all()


# ---- identities on the twin ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (33, 9)])
def test_stride_one_radius_zero_returns_the_input_on_surface_pixels(w, h):
    prim, nrm, values, base = VT.hand_made(w, h, 9 + w, misses=True)
    surf = VT.surface(prim)
    with np.errstate(all="ignore"):
        out, cls = ST.value_upsample(prim, nrm, values, w, h, 1, 0, 0, 0.0, 1.0, classes=True)
    # as values: 0.0f + 1.0f * -0.0f is +0.0f
    assert (np.isnan(out[surf]) == np.isnan(values[surf])).all() and (out[surf] == values[surf])[~np.isnan(values[surf])].all()
    assert not out.view(np.uint32)[~surf].any()
    assert (cls[surf] == ACCEPTED).all()
    assert (ST.sparse_values(values, prim, w, h, 1, 0).view(np.uint32) == np.where(surf, values, f32(0)).view(np.uint32)).all()


def test_the_phases_of_a_stride_visit_every_pixel_once():
    w, h = 7, 5
    prim, _, values, _ = VT.hand_made(w, h, 2, misses=True)
    surf = VT.surface(prim)
    for s in (1, 2, 3, 4):
        visited = np.zeros((h, w), dtype=int)
        for phase in range(s * s):
            gx, gy, inside = cell_pixels(w, h, s, phase)
            visited[gy[inside], gx[inside]] += 1
            lo = ST.sparse_values(values, prim, w, h, s, phase).reshape(inside.shape)
            assert lo.shape == lo_size(w, h, s)[::-1] and not lo.view(np.uint32)[~inside].any()
            want = np.where(surf, values, f32(0)).reshape(h, w)[gy[inside], gx[inside]]
            assert VT.same_bits(lo[inside], want).size == 0, (s, phase)
            assert phase_xy(s, phase) == (int(gx[0, 0]), int(gy[0, 0]))
        assert (visited == 1).all(), s


# ---- refusals decided before a device is touched -------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_device_work(trx):
    from tray_racing_amd import _lib
    lib = trx.load()
    buf = np.zeros(64, dtype=np.uint32)

    def at(k):
        return C.c_void_p(buf.ctypes.data + 16 * k)
    P, LO, OUT, BASE = at(0), at(1), at(2), at(3)
    fake = P   # never dereferenced: every call below is refused on its arguments
    inv = _lib.TRX_ERR_INVALID
    view = _lib.View()
    good = trx.light(trx.LIGHT_POINT, (0, 1, 0))

    def arr(*lights):
        return trx.light_array(lights)

    def pas(scene=fake, v=C.byref(view), w=4, h=4, s=2, phase=0, sem=0, mask=0, lights=arr(good), n_lights=None, n=4, beps=0.01, seps=0.01, albedo=0.5,
            prim=P, out=LO):
        return lib.trx_trace_indirect_sparse_dev(scene, v, w, h, s, phase, sem, mask, lights, len(lights) if n_lights is None else n_lights, 0, n, beps,
                                                 seps, albedo, prim, None, out, None)

    assert pas(s=0) == inv and b"stride" in lib.trx_last_error()
    assert pas(s=5) == inv and b"stride" in lib.trx_last_error()
    assert pas(s=2, phase=4) == inv and b"phase" in lib.trx_last_error()
    assert pas(s=1, phase=1) == inv and pas(s=3, phase=9) == inv and pas(s=4, phase=16) == inv
    assert pas(n_lights=0) == inv and b"n_lights" in lib.trx_last_error()
    assert pas(lights=arr(*[good] * 9)) == inv and pas(lights=None, n_lights=1) == inv and b"null" in lib.trx_last_error()
    assert pas(lights=arr(good, trx.light(3, (0, 1, 0)))) == inv and b"kind" in lib.trx_last_error()
    assert pas(lights=arr(trx.light(trx.LIGHT_POINT, (0, NAN, 0)))) == inv and b"finite" in lib.trx_last_error()
    assert pas(lights=arr(trx.light(trx.LIGHT_DIRECTIONAL, (0, 0, 0)))) == inv and b"zero length" in lib.trx_last_error()
    assert pas(n=0) == inv and pas(n=65) == inv and b"n_samples" in lib.trx_last_error()
    assert pas(mask=256) == inv and b"ray_mask" in lib.trx_last_error()
    for eps in (NAN, -0.01, -INF):
        assert pas(seps=eps) == inv and b"shadow_eps" in lib.trx_last_error()
        assert pas(beps=eps) == inv and b"bounce_eps" in lib.trx_last_error()
    for albedo in (NAN, INF, -INF):
        assert pas(albedo=albedo) == inv and b"bounce_albedo" in lib.trx_last_error()
    assert pas(sem=8) == inv and b"semantics" in lib.trx_last_error()
    assert pas(w=0) == inv and pas(h=0) == inv and pas(v=None) == inv
    for kw in ({"scene": None}, {"prim": None}, {"out": None}):
        assert pas(**kw) == inv and b"null" in lib.trx_last_error(), kw

    def up(scene=fake, w=4, h=4, s=2, phase=0, prim=P, attr=None, lo=LO, base=None, r=1, tol=0.1, cos=0.9, out=OUT):
        return lib.trx_value_upsample_dev(scene, w, h, s, phase, prim, attr, lo, base, r, tol, cos, out, None)

    assert up(s=0) == inv and up(s=5) == inv and b"stride" in lib.trx_last_error()
    assert up(phase=4) == inv and up(s=1, phase=1) == inv and b"phase" in lib.trx_last_error()
    assert up(r=3) == inv and b"radius" in lib.trx_last_error()
    for tol in (-0.5, NAN, -INF):
        assert up(tol=tol) == inv and b"depth_tol" in lib.trx_last_error()
    assert up(cos=NAN) == inv and b"normal_cos" in lib.trx_last_error()
    assert up(w=0) == inv and up(h=0) == inv and b"image" in lib.trx_last_error()
    assert up(w=65536, h=32768) == inv and b"image" in lib.trx_last_error()
    for kw in ({"scene": None}, {"prim": None}, {"lo": None}, {"out": None}):
        assert up(**kw) == inv and b"null" in lib.trx_last_error(), kw
    assert up(lo=OUT) == inv and b"d_in_lo is d_out" in lib.trx_last_error()
    assert up(lo=OUT, base=OUT) == inv

    def render(scene=fake, v=C.byref(view), w=4, h=4, lights=arr(good), n_lights=1, bn=4, beps=0.01, albedo=0.5, levels=3, tol=0.1, cos=0.9, s=2, phase=0,
               up_r=1, r=0, ao=0, sem=0, mask=0):
        return lib.trx_render_image_gi_sparse(scene, v, w, h, sem, mask, lights, n_lights, 0, 1, 0.01, 0.1, ao, 0.01, INF, r, 0.02, 0.9, bn, beps, albedo,
                                              levels, tol, cos, s, phase, up_r, P, None)

    assert render(s=0) == inv and render(s=5) == inv and b"stride" in lib.trx_last_error()
    assert render(phase=4) == inv and b"phase" in lib.trx_last_error()
    assert render(up_r=3) == inv and b"radius" in lib.trx_last_error()
    assert render(levels=6) == inv and b"bounce_filter_levels" in lib.trx_last_error()
    for levels in (0, 3):                                   # (the upsample looks at the tolerances whatever the levels)
        assert render(levels=levels, tol=-1.0) == inv and render(levels=levels, tol=NAN) == inv and b"depth_tol" in lib.trx_last_error()
        assert render(levels=levels, cos=NAN) == inv and b"normal_cos" in lib.trx_last_error()
    assert render(bn=0) == inv and b"bounce_samples" in lib.trx_last_error()
    assert render(bn=65) == inv and render(beps=-1.0) == inv and render(albedo=INF) == inv and render(n_lights=0) == inv
    assert render(ao=4, r=5) == inv and render(sem=8) == inv and render(mask=256) == inv
    assert render(w=0) == inv and render(scene=None) == inv and render(v=None) == inv
    assert not buf.any()


# ---- the golden cases: not vacuous, and what the pass is for -----------------------------------------------------------

@pytest.mark.parametrize("name", ["soup_52x44", "cornell_tlas_48"])
def test_the_three_branches_occur_on_the_goldens(trx, orc, name):
    """The conditions tests/test_ao_sparse.py holds for the count upsample, for this twin's classes: stride 2, radius 1, phase 0,
    tolerance 0.02, cosine 0.9 over the oracle's TRX_SEM_CPU records - accepted and fallback pixels are each at least 10 % of the
    surface pixels of both frames, and soup_52x44 has empty pixels.  The classes are the count upsample's, pixel for pixel."""
    _, _, w, h, prim, normals = _golden_records(trx, orc, name)
    surf = VT.surface(prim)
    wlo, hlo = lo_size(w, h, 2)
    lo = np.where(surf.reshape(h, w)[::2, ::2], 0.5, NAN).astype(np.float32).reshape(-1)
    assert lo.size == wlo * hlo
    out, cls = ST.value_upsample(prim, normals, lo, w, h, 2, 0, 1, 0.02, 0.9, classes=True)
    n, acc, fb, empty = class_counts(cls)
    print("%s: %d surface pixels, %.1f %% accepted, %.1f %% fallback, %d empty" % (name, n, 100.0 * acc / n, 100.0 * fb / n, empty))
    assert n == int(surf.sum()) and acc + fb + empty == n
    assert acc >= 0.1 * n and fb >= 0.1 * n, (name, n, acc, fb, empty)
    if name == "soup_52x44":
        assert empty >= 1
    counts = np.where(surf.reshape(h, w)[::2, ::2], 2, 0xFF).astype(np.uint8).reshape(-1)
    _, acls = ao_upsample(prim, normals, counts, w, h, 2, 0, 4, 1, 0.02, 0.9, classes=True)
    assert (acls == cls).all()
    assert (out[(cls == ACCEPTED) | (cls == FALLBACK)] == 0.5).all() and not out[(cls == EMPTY) | (cls == NOT_SURFACE)].any()


@pytest.mark.parametrize("name", sorted(LT.POINT_CASES))
def test_sparse_values_hold_all_three_kinds_of_cell(orc, name):
    """Stride 2, phase 0, sem 0, seeds 0..3, 4 samples, the fixture's point light: the sparse values contain a cell off the image
    or without a surface, a surface cell with the value 0 and a surface cell with a value above 0."""
    w, h, prim, _, noisy, _ = _golden_frame(orc, name)
    lo = ST.sparse_values(noisy, prim, w, h, 2, 0)
    gx, gy, inside = cell_pixels(w, h, 2, 0)
    surf = VT.surface(prim).reshape(h, w)
    c_surf = inside.copy()
    c_surf[inside] = surf[gy[inside], gx[inside]]
    c_surf = c_surf.reshape(-1)
    print("%s: %d cells, %d without a surface, %d surface cells at 0, %d above 0" % (name, lo.size, (~c_surf).sum(), (c_surf & (lo == 0)).sum(),
                                                                                     (c_surf & (lo > 0)).sum()))
    assert (~c_surf).any() and (c_surf & (lo == 0)).any() and (c_surf & (lo > 0)).any(), name
    assert not lo.view(np.uint32)[~c_surf].any()


_refs = {}


def _reference(orc, name):
    if name not in _refs:
        _refs[name] = _golden_frame(orc, name)[5]()
    return _refs[name]


def test_sparse_upsampled_filtered_term_against_the_64_sample_term(orc):
    """The RMSE over the surface pixels of [sparse 4-sample term at stride 2, phase 0 -> upsample radius 1 -> 3 filter levels at
    (0.10, 0.9)] against the twin's 64-sample dense term (seeds 1000..1063), beside the unfiltered and the dense-filtered
    4-sample terms.  Asserted: on the two Cornell fixtures it is below the unfiltered dense 4-sample RMSE.  The figures are
    reported in DESIGN section 21."""
    for name in sorted(LT.POINT_CASES):
        w, h, prim, normals, noisy, _ = _golden_frame(orc, name)
        ref = _reference(orc, name)
        surf = LT.surface(prim)

        def rmse(a):
            return float(np.sqrt(np.mean((a[surf].astype(np.float64) - ref[surf].astype(np.float64)) ** 2)))
        dense = VT.value_filter(prim, normals, noisy, w, h, 3, TOL, COS)
        lo = ST.sparse_values(noisy, prim, w, h, 2, 0)
        up = ST.value_upsample(prim, normals, lo, w, h, 2, 0, 1, TOL, COS)
        sparse = VT.value_filter(prim, normals, up, w, h, 3, TOL, COS)
        before, mid, dfl, after = rmse(noisy), rmse(up), rmse(dense), rmse(sparse)
        print("%s: RMSE against 64 samples %.4f dense unfiltered, %.4f dense filtered, %.4f sparse upsampled, %.4f sparse upsampled and filtered" % (
            name, before, dfl, mid, after))
        if name.startswith("cornell"):
            assert after < before, (name, after, before)
