"""Sparse AO visibility (include/trx.h: trx_trace_ao_visibility_sparse_dev, trx_ao_upsample_dev, trx_render_image_sparse)
without a GPU: the numpy twin (tests/ao_sparse_twin.py) against the filter's twin at stride 1, against a literal scalar
restatement of the header's rules, and on hand-made record images that reach every branch by construction; the branches
on the golden fixtures; the refusals that are decided before a device is touched; the boundary and the kernel's resources.
tests/test_gpu_ao_sparse.py holds the device to the twin bit for bit."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ao_sparse_twin import (ACCEPTED, EMPTY, FALLBACK, NO_SURFACE, NOT_SURFACE, ao_upsample, cell_pixels, class_counts, lo_size,
                            phase_xy, sparse_counts)
from ao_visibility_twin import golden_case, visibility_counts
from hit_attr_twin import tri_records
from image_twin import F32_MAX, TERM_DTYPE, ao_filter, surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tray_racing_amd", "tray_racing_hip")
INF = float("inf")
HIT = np.dtype([("t", "<f4"), ("prim", "<u4")])
NEW_SYMBOLS = ("trx_trace_ao_visibility_sparse_dev", "trx_ao_upsample_dev", "trx_render_image_sparse")


# ---- the boundary ------------------------------------------------------------------------------------------------

def test_symbols_defines_and_bindings(trx):
    from tray_racing_amd import _lib
    assert _lib.MAX_AO_STRIDE == 4 and _lib.MAX_AO_UPSAMPLE_RADIUS == 2
    src = (b'#include "trx.h"\n_Static_assert(TRX_MAX_AO_STRIDE == 4, "stride");\n'
           b'_Static_assert(TRX_MAX_AO_UPSAMPLE_RADIUS == 2, "radius");\n'
           b'_Static_assert(25 * 255 <= 65535, "the largest sum fits uint16_t");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", "-I",
                    os.path.join(ROOT, "include"), "-"], input=src, check=True)
    header = open(os.path.join(ROOT, "include", "trx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    lib = trx.load()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and (" T %s\n" % name) in out and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [15, 14, 16]
    for name in ("trace_ao_visibility_sparse_dev", "ao_upsample_dev", "render_image_sparse"):
        assert callable(getattr(trx.Scene, name))
    assert lib.trx_abi_version() == 1   # additions only: every existing prototype and record is what it was


def test_upsample_kernel_resources():
    """k_ao_upsample (make build/image.s): no scratch, within the product kernels' 128 VGPRs (the counts are reported), and
    its LDS is the largest tile and halo of image.h - 432 cells of 20 bytes with normals, 8 without."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "tray_racing_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "build/image.s"], check=True, capture_output=True, timeout=600)
    text = open(os.path.join(csrc, "build", "image.s")).read()
    found = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n.*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        name, body = m.group(2), m.group(3)
        if "k_ao_upsample" not in name:
            continue
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        print("%s: %d VGPRs, %d B scratch, %d B LDS" % (name, vgprs, scratch, int(m.group(1))))
        assert scratch == 0 and vgprs <= 128, name
        found[name] = int(m.group(1))
    assert sorted(found.values()) == [432 * 8, 432 * 20], found


def test_cli_lists_and_checks_the_sparse_flags():
    def run(*args):
        return subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=120)
    usage = run("--help")
    assert usage.returncode == 0 and "--ao-stride 1..4" in usage.stdout and "--ao-phase" in usage.stdout and "--ao-upsample 0..2" in usage.stdout
    base = ("-i", "standin:cornell", "--dry-run", "--passes", "1")
    for extra, msg in ((("--ao-stride", "2"), "--ao-samples"), (("--ao-samples", "4", "--ao-stride", "0"), "1..4"),
                       (("--ao-samples", "4", "--ao-stride", "5"), "1..4"), (("--ao-samples", "4", "--ao-stride", "2", "--ao-phase", "4"), "S*S-1"),
                       (("--ao-samples", "4", "--ao-stride", "2", "--ao-upsample", "3"), "0..2"),
                       (("--ao-samples", "4", "--ao-phase", "1"), "--ao-stride"), (("--ao-samples", "4", "--ao-upsample", "1"), "--ao-stride"),
                       (("--ao-samples", "4", "--ao-stride", "2", "--ao-filter", "1"), "not together")):
        r = run(*base, *extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert run(*base, "--png", "--ao-samples", "4", "--ao-stride", "2", "--ao-phase", "3", "--ao-upsample", "2").returncode == 0


# ---- hand-made records ------------------------------------------------------------------------------------------------

def _image(w, h, t=2.0):
    prim = np.zeros(w * h, dtype=HIT)
    prim["t"], prim["prim"] = t, 7
    return prim, np.tile(np.array([0, 0, 1], dtype=np.float32), (w * h, 1))


def _random_image(w, h, seed):
    """Depth steps, misses of both kinds, three normals: denser in edges than a traced frame."""
    rng = np.random.default_rng(seed)
    n = w * h
    prim = np.zeros(n, dtype=HIT)
    prim["t"] = rng.choice(np.array([1.0, 1.01, 1.5, INF, 3.4028234663852886e38], dtype=np.float32), n, p=[.4, .3, .15, .1, .05])
    prim["prim"] = np.where(rng.random(n) < 0.08, 0xFFFFFFFF, rng.integers(0, 1000, n)).astype(np.uint32)
    normals = np.array([[0, 0, 1], [0, 0.6, 0.8], [1, 0, 0]], dtype=np.float32)[rng.integers(0, 3, n)]
    dense = np.where(surface(prim), rng.integers(0, 5, n), NO_SURFACE).astype(np.uint8)
    return prim, normals, dense


def _terms(out, w, h):
    return out["unoccluded"].reshape(h, w).astype(int), out["samples"].reshape(h, w).astype(int)


def _by_the_letter(prim, normals, lo, w, h, s, phase, n, r, tol, cos):
    """The header's rules, pixel by pixel and cell by cell, in binary32 scalars."""
    px0, py0 = phase % s, phase // s
    wlo, hlo = (w + s - 1) // s, (h + s - 1) // s
    f = np.float32
    out, cls = np.zeros(w * h, dtype=TERM_DTYPE), np.zeros(w * h, dtype=np.uint8)

    def is_surface(i):
        return bool(prim["t"][i] < F32_MAX) and int(prim["prim"][i]) != 0xFFFFFFFF

    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(h):
            for x in range(w):
                p = y * w + x
                if not is_surface(p):
                    continue
                tp = f(prim["t"][p])
                acc, cells = [], []
                for Y in range(y // s - r, y // s + r + 1):
                    for X in range(x // s - r, x // s + r + 1):
                        if not (0 <= X < wlo and 0 <= Y < hlo):
                            continue
                        gx, gy = X * s + px0, Y * s + py0
                        if gx >= w or gy >= h or not is_surface(gy * w + gx):
                            continue
                        q = gy * w + gx
                        cells.append(int(lo[Y * wlo + X]))
                        ok = bool(np.abs(f(prim["t"][q]) - tp) <= f(tol) * tp)
                        if normals is not None:
                            a, b = normals[p].astype(f), normals[q].astype(f)
                            ok = ok and bool(f(f(f(a[0] * b[0]) + f(a[1] * b[1])) + f(a[2] * b[2])) >= f(cos))
                        if ok or q == p:
                            acc.append(int(lo[Y * wlo + X]))
                use, cls[p] = (acc, ACCEPTED) if acc else (cells, FALLBACK if cells else EMPTY)
                out[p] = (sum(use), n * len(use))
    return out, cls


@pytest.mark.parametrize("w,h,s,phases", [(7, 3, 3, (0, 4, 8)), (7, 3, 2, (0, 3)), (33, 9, 2, (1,)), (33, 9, 4, (15,)), (70, 19, 3, (0, 8)),
                                          (1, 1, 4, (0, 15))])
def test_twin_equals_the_rules_by_the_letter(w, h, s, phases):
    """Widths and heights that are no multiples of the stride (stride 3 on 7x3 and 70x19 among them): cells whose pixel lies
    outside the image, windows clipped at every border, all three branches."""
    prim, normals, dense = _random_image(w, h, 11 * w + s)
    seen = set()
    for phase in phases:
        lo = sparse_counts(dense, w, h, s, phase)
        gx, gy, inside = cell_pixels(w, h, s, phase)
        assert lo.size == lo_size(w, h, s)[0] * lo_size(w, h, s)[1] and (lo.reshape(inside.shape)[~inside] == NO_SURFACE).all()
        if s == 3 and phase == 8:
            assert (~inside).any(), "no cell outside the image"
        lo[~inside.reshape(-1)] = 200   # (such a cell's count must never be looked at)
        for r, nrm, tol, cos in ((0, True, 0.02, 0.9), (1, True, 0.02, 0.9), (2, False, 0.02, 0.9), (2, True, INF, -1.0), (1, True, 0.0, 1.0)):
            got, cls = ao_upsample(prim, normals if nrm else None, lo, w, h, s, phase, 4, r, tol, cos, classes=True)
            want, wcls = _by_the_letter(prim, normals if nrm else None, lo, w, h, s, phase, 4, r, tol, cos)
            assert (got.view(np.uint32) == want.view(np.uint32)).all() and (cls == wcls).all(), (w, h, s, phase, r, nrm, tol, cos)
            assert not got.view(np.uint32)[cls == NOT_SURFACE].any() and not got.view(np.uint32)[cls == EMPTY].any()
            seen |= set(np.unique(cls).tolist())
    if w * h > 1:
        assert {ACCEPTED, FALLBACK, EMPTY} <= seen and (NOT_SURFACE in seen or w * h < 100), seen


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (33, 9), (40, 17)])
def test_twin_at_stride_one_is_the_filters_twin(w, h):
    prim, normals, dense = _random_image(w, h, 3 + w)
    assert (sparse_counts(dense, w, h, 1, 0) == dense).all()
    for r in (0, 1, 2):
        for nrm in (normals, None):
            for tol in (0.0, 0.02, INF):
                for cos in (-1.0, 0.9, 1.0):
                    got, cls = ao_upsample(prim, nrm, dense, w, h, 1, 0, 4, r, tol, cos, classes=True)
                    want = ao_filter(prim, nrm, dense, w, h, 4, r, tol, cos)
                    assert (got.view(np.uint32) == want.view(np.uint32)).all(), (w, h, r, nrm is None, tol, cos)
                    assert not ((cls == FALLBACK) | (cls == EMPTY)).any()   # every pixel is its own cell


def test_accepted_fallback_and_empty_by_hand():
    w, h, n = 4, 4, 4
    prim, normals = _image(w, h)
    lo = np.array([1, 2, 3, 4], dtype=np.uint8)                   # stride 2, phase 0: the cells of pixels (0,0) (2,0) (0,2) (2,2)
    out, cls = ao_upsample(prim, normals, lo, w, h, 2, 0, n, 0, 0.02, 0.9, classes=True)
    u, s = _terms(out, w, h)
    assert (u == [[1, 1, 2, 2], [1, 1, 2, 2], [3, 3, 4, 4], [3, 3, 4, 4]]).all() and (s == n).all() and (cls == ACCEPTED).all()
    out, cls = ao_upsample(prim, normals, lo, w, h, 2, 0, n, 1, 0.02, 0.9, classes=True)
    u, s = _terms(out, w, h)
    assert (u == 10).all() and (s == 4 * n).all()                  # every window is the whole low grid
    # FALLBACK: pixel (1, 1) lies behind a depth step no cell shares
    prim["t"].reshape(h, w)[1, 1] = 10.0
    for r, want in ((0, (1, n)), (1, (10, 4 * n))):
        out, cls = ao_upsample(prim, normals, lo, w, h, 2, 0, n, r, 0.02, 0.9, classes=True)
        u, s = _terms(out, w, h)
        assert (u[1, 1], s[1, 1]) == want and cls.reshape(h, w)[1, 1] == FALLBACK and (np.delete(cls, 5) == ACCEPTED).all()
    # ... and a tolerance that reaches across the step accepts them again
    out, cls = ao_upsample(prim, normals, lo, w, h, 2, 0, n, 0, 1.0, 0.9, classes=True)
    assert cls.reshape(h, w)[1, 1] == ACCEPTED and _terms(out, w, h)[0][1, 1] == 1
    # EMPTY: the only cell of the window has no surface (a miss at its pixel; its count is never looked at)
    prim["t"].reshape(h, w)[0, 0], prim["prim"].reshape(h, w)[0, 0], lo[0] = INF, 0xFFFFFFFF, 200
    out, cls = ao_upsample(prim, normals, lo, w, h, 2, 0, n, 0, 0.02, 0.9, classes=True)
    u, s = _terms(out, w, h)
    c = cls.reshape(h, w)
    assert c[0, 0] == NOT_SURFACE and c[0, 1] == EMPTY and c[1, 0] == EMPTY and c[1, 1] == EMPTY and c[0, 2] == ACCEPTED
    assert (u[:2, :2] == 0).all() and (s[:2, :2] == 0).all()
    out, cls = ao_upsample(prim, normals, lo, w, h, 2, 0, n, 1, 0.02, 0.9, classes=True)
    u, s = _terms(out, w, h)
    assert (u[0, 1], s[0, 1]) == (9, 3 * n) and cls.reshape(h, w)[0, 1] == ACCEPTED and cls.reshape(h, w)[1, 1] == FALLBACK


def test_a_cell_outside_the_image_is_no_surface_cell():
    w, h, n = 7, 3, 2
    prim, normals = _image(w, h)
    dense = np.arange(w * h, dtype=np.uint8) % 3
    assert lo_size(w, h, 3) == (3, 1) and lo_size(70, 19, 3) == (24, 7)
    for phase, outside in ((0, []), (4, [2]), (8, [2]), (2, [2])):
        px0, py0 = phase_xy(3, phase)
        lo = sparse_counts(dense, w, h, 3, phase)
        assert [int(c) for c in np.flatnonzero(lo == NO_SURFACE)] == outside, phase
        out, cls = ao_upsample(prim, normals, lo, w, h, 3, phase, n, 0, 0.02, 0.9, classes=True)
        u, s = _terms(out, w, h)
        for x in range(w):
            cell_in = (x // 3) * 3 + px0 < w
            assert (cls.reshape(h, w)[:, x] == (ACCEPTED if cell_in else EMPTY)).all(), (phase, x)
            assert (u[:, x] == (dense[py0 * w + (x // 3) * 3 + px0] if cell_in else 0)).all() and (s[:, x] == (n if cell_in else 0)).all()
        # one cell further out the window reaches a cell inside
        out, cls = ao_upsample(prim, normals, lo, w, h, 3, phase, n, 1, 0.02, 0.9, classes=True)
        assert (cls == ACCEPTED).all() and (_terms(out, w, h)[1][:, 6] == n * (1 if outside else 2)).all()
    gx, gy, inside = cell_pixels(70, 19, 3, 8)
    assert not inside[:, 23].any() and not inside[6, :].any() and inside[:6, :23].all()


def test_own_cell_is_accepted_although_its_normal_test_fails():
    """normal_cos = 1 with a unit normal whose dot product with itself rounds below 1: the pixel of a cell still takes its
    cell, its neighbour with the same normal does not."""
    rng = np.random.default_rng(5)
    for _ in range(1000):
        v = rng.normal(size=3).astype(np.float32)
        v = (v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])).astype(np.float32)
        if (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] < np.float32(1.0):
            break
    else:
        raise AssertionError("no such normal found")
    w, h, n = 4, 2, 4
    prim, normals = _image(w, h)
    normals[:] = v
    lo = np.array([3, 1], dtype=np.uint8)
    out, cls = ao_upsample(prim, normals, lo, w, h, 2, 0, n, 1, INF, 1.0, classes=True)
    u, s = _terms(out, w, h)
    c = cls.reshape(h, w)
    assert c[0, 0] == ACCEPTED and (u[0, 0], s[0, 0]) == (3, n) and c[0, 2] == ACCEPTED and (u[0, 2], s[0, 2]) == (1, n)
    for y, x in ((0, 1), (1, 0), (1, 1), (0, 3), (1, 2), (1, 3)):   # not the pixel of a cell: nothing accepted, both cells
        assert c[y, x] == FALLBACK and (u[y, x], s[y, x]) == (4, 2 * n)
    # the same image under a cosine the normal reaches: everything accepted
    out, cls = ao_upsample(prim, normals, lo, w, h, 2, 0, n, 1, INF, 0.999, classes=True)
    assert (cls == ACCEPTED).all() and (out["samples"] == 2 * n).all()


def test_window_clipped_at_all_four_borders():
    w, h, n, s = 10, 6, 4, 2
    prim, normals = _image(w, h)
    wlo, hlo = lo_size(w, h, s)
    lo = np.full(wlo * hlo, 3, dtype=np.uint8)
    for phase in range(4):
        for r in (1, 2):
            u, smp = _terms(ao_upsample(prim, normals, lo, w, h, s, phase, n, r, 0.0, 1.0), w, h)
            for y in range(h):
                for x in range(w):
                    qx, qy = x // s, y // s
                    cells = (min(qx + r, wlo - 1) - max(qx - r, 0) + 1) * (min(qy + r, hlo - 1) - max(qy - r, 0) + 1)
                    assert u[y, x] == 3 * cells and smp[y, x] == n * cells, (phase, r, x, y)
            assert u[0, 0] == 3 * (r + 1) ** 2 and u[h - 1, w - 1] == 3 * (r + 1) ** 2 and u[2, 4] == 3 * 3 * min(2 * r + 1, wlo)


def test_every_phase_of_stride_two():
    w, h, n = 5, 5, 1
    prim, normals = _image(w, h)
    dense = (np.arange(w * h) % 5).astype(np.uint8)
    visited = np.zeros((h, w), dtype=int)
    for phase in range(4):
        px0, py0 = phase_xy(2, phase)
        lo = sparse_counts(dense, w, h, 2, phase)
        gx, gy, inside = cell_pixels(w, h, 2, phase)
        visited[gy[inside], gx[inside]] += 1
        out, cls = ao_upsample(prim, normals, lo, w, h, 2, phase, n, 0, 0.02, 0.9, classes=True)
        u, s = _terms(out, w, h)
        for y in range(h):
            for x in range(w):
                cx, cy = (x // 2) * 2 + px0, (y // 2) * 2 + py0
                if cx < w and cy < h:
                    assert (u[y, x], s[y, x], cls[y * w + x]) == (dense[cy * w + cx], n, ACCEPTED), (phase, x, y)
                else:
                    assert (u[y, x], s[y, x], cls[y * w + x]) == (0, 0, EMPTY), (phase, x, y)
    assert (visited == 1).all(), "the phases of a stride do not visit every pixel once"


# ---- the golden fixtures ------------------------------------------------------------------------------------------------

def _golden_records(trx, orc, name):
    osc, oview, w, h, g = golden_case(trx, orc, name)
    prim, _ = osc.trace_primary(oview, w, h, sem=orc.SEM_CPU)
    ng = tri_records(tri_verts=g["tri_verts"])[:, 9:12]
    normals = np.zeros((w * h, 3), dtype=np.float32)
    s = surface(prim)
    nn = ng[prim["prim"][s]]
    normals[s] = nn / np.linalg.norm(nn, axis=1, keepdims=True)
    return osc, oview, w, h, prim, normals


@pytest.mark.parametrize("name", ["soup_52x44", "cornell_tlas_48"])
def test_the_three_branches_occur_on_the_goldens(trx, orc, name):
    """Stride 2, radius 1, phase 0, tolerance 0.02, cosine 0.9 over the oracle's TRX_SEM_CPU primary records and
    numpy-normalised geometric normals: accepted and fallback pixels are each at least 10 % of the surface pixels of both
    frames, and soup_52x44 has empty pixels.  (The images are tiny, so 0.02 of t is a tight tolerance on them: an input.)"""
    osc, oview, w, h, prim, normals = _golden_records(trx, orc, name)
    wlo, hlo = lo_size(w, h, 2)
    lo = np.where(surface(prim).reshape(h, w)[::2, ::2], 2, NO_SURFACE).astype(np.uint8).reshape(-1)   # (the classes ignore the counts)
    assert lo.size == wlo * hlo
    _, cls = ao_upsample(prim, normals, lo, w, h, 2, 0, 4, 1, 0.02, 0.9, classes=True)
    n, acc, fb, empty = class_counts(cls)
    print("%s: %d surface pixels, %.1f %% accepted, %.1f %% fallback, %d empty" % (name, n, 100.0 * acc / n, 100.0 * fb / n, empty))
    assert n == int(surface(prim).sum()) and acc + fb + empty == n
    assert acc >= 0.1 * n and fb >= 0.1 * n, (name, n, acc, fb, empty)
    if name == "soup_52x44":
        assert empty >= 1


def test_twin_sparse_counts_are_the_dense_twins_subsampled(trx, orc):
    osc, oview, w, h, prim, _ = _golden_records(trx, orc, "soup_52x44")
    dense = visibility_counts(orc, osc, oview, w, h, prim, None, orc.SEM_CPU, 0, 2, 0.01, 0.8)
    assert ((dense > 0) & (dense < 2)).any() and (dense == NO_SURFACE).any()
    for s, phase in ((1, 0), (2, 0), (2, 3), (3, 0), (3, 8), (4, 0), (4, 15)):
        px0, py0 = phase_xy(s, phase)
        wlo, hlo = lo_size(w, h, s)
        lo = sparse_counts(dense, w, h, s, phase).reshape(hlo, wlo)
        for Y in range(hlo):
            for X in range(wlo):
                x, y = X * s + px0, Y * s + py0
                assert lo[Y, X] == (dense[y * w + x] if x < w and y < h else NO_SURFACE), (s, phase, X, Y)


# ---- refusals decided before a device is touched -------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_device_work(trx):
    from tray_racing_amd import _lib
    lib = trx.load()
    buf = np.zeros(64, dtype=np.uint32)
    P = buf.ctypes.data_as(C.c_void_p)
    fake = P   # never dereferenced: every call below is refused on its arguments
    inv = _lib.TRX_ERR_INVALID
    view = _lib.View()

    def sparse(scene=fake, v=C.byref(view), w=4, h=4, s=2, phase=0, sem=0, n=4, radius=INF, prim=P, out=P):
        return lib.trx_trace_ao_visibility_sparse_dev(scene, v, w, h, s, phase, sem, 0, n, 0.01, radius, prim, None, out, None)

    assert sparse(s=0) == inv and b"stride" in lib.trx_last_error()
    assert sparse(s=5) == inv and b"stride" in lib.trx_last_error()
    assert sparse(s=2, phase=4) == inv and b"phase" in lib.trx_last_error()
    assert sparse(s=1, phase=1) == inv and sparse(s=4, phase=16) == inv and sparse(s=3, phase=9) == inv
    assert sparse(n=0) == inv and b"n_samples" in lib.trx_last_error()
    assert sparse(n=65) == inv
    for radius in (0.0, -1.0, float("nan")):
        assert sparse(radius=radius) == inv and b"ao_radius" in lib.trx_last_error()
    assert sparse(sem=8) == inv and b"semantics" in lib.trx_last_error()
    assert sparse(w=0) == inv and sparse(h=0) == inv and sparse(w=65536, h=65536) == inv and sparse(v=None) == inv
    for kw in ({"scene": None}, {"prim": None}, {"out": None}):
        assert sparse(**kw) == inv and b"null" in lib.trx_last_error()

    def up(scene=fake, w=4, h=4, s=2, phase=0, prim=P, lo=P, n=4, r=1, tol=0.02, cos=0.9, term=P):
        return lib.trx_ao_upsample_dev(scene, w, h, s, phase, prim, None, lo, n, r, tol, cos, term, None)

    assert up(s=0) == inv and up(s=5) == inv and b"stride" in lib.trx_last_error()
    assert up(phase=4) == inv and b"phase" in lib.trx_last_error()
    assert up(r=3) == inv and b"radius" in lib.trx_last_error()
    assert up(n=0) == inv and up(n=65) == inv and b"n_samples" in lib.trx_last_error()
    assert up(tol=-0.5) == inv and b"depth_tol" in lib.trx_last_error()
    assert up(tol=float("nan")) == inv
    assert up(cos=float("nan")) == inv and b"normal_cos" in lib.trx_last_error()
    assert up(w=0) == inv and up(h=0) == inv and b"image" in lib.trx_last_error()
    assert up(w=65536, h=65536) == inv
    for kw in ({"scene": None}, {"prim": None}, {"lo": None}, {"term": None}):
        assert up(**kw) == inv and b"null" in lib.trx_last_error()

    def render(scene=fake, v=C.byref(view), w=4, h=4, sem=0, n=4, radius=INF, s=2, phase=0, r=1, tol=0.02, cos=0.9):
        return lib.trx_render_image_sparse(scene, v, w, h, sem, 0, n, 0.01, radius, s, phase, r, tol, cos, P, None)

    assert render(n=0) == inv and render(n=65) == inv and render(radius=0.0) == inv and render(radius=float("nan")) == inv
    assert render(s=0) == inv and render(s=5) == inv and render(phase=4) == inv and render(r=3) == inv
    assert render(tol=-1.0) == inv and render(cos=float("nan")) == inv and render(sem=8) == inv
    assert render(w=0) == inv and render(scene=None) == inv and render(v=None) == inv
    assert not buf.any()
